#!/usr/bin/env python3
"""tests/golden/realism_clip.npz: transformers' CLIPVisionModelWithProjection at OpenAI's ViT-B/32 configuration
(width 768, 12 layers, 12 heads, patch 32, 224 x 224, projection 512, quick_gelu), every parameter filled by
oracle.weights.fill_module_(seed 31), run in float64 on seeded images in [0, 1] (CLIP's Normalize applied first) ->
`image_embeds` of the reference and the predicted images and the pairwise 100 cos.  The weights are not stored: the test
refills them from the seed (tests/realism_ref.py clip_b32_state).

    python tests/golden/make_golden_realism.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import weights as W                 # noqa: E402
import realism_ref as R                         # noqa: E402

SEED, N = 31, 6


def images():
    ref = R.clip_images("realism.clip.ref", N)
    other = R.clip_images("realism.clip.other", N)
    w = torch.linspace(0.0, 1.0, N).view(N, 1, 1, 1)       # pair 0: identical images ... pair N-1: unrelated ones
    return ref, ((1 - w) * ref + w * other).float()


def main():
    import transformers
    cfg = transformers.CLIPVisionConfig(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                                        image_size=224, patch_size=32, projection_dim=512, hidden_act="quick_gelu",
                                        layer_norm_eps=1e-5)
    model = transformers.CLIPVisionModelWithProjection(cfg).eval()
    W.fill_module_(model, seed=SEED)
    model = model.double()
    ref, pred = images()
    mean = torch.tensor(R.CLIP_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(R.CLIP_STD, dtype=torch.float64).view(1, 3, 1, 1)
    with torch.no_grad():
        er = model(pixel_values=(ref.double() - mean) / std).image_embeds
        ep = model(pixel_values=(pred.double() - mean) / std).image_embeds
    score = 100.0 * torch.nn.functional.cosine_similarity(er, ep, dim=-1)
    np.savez_compressed(os.path.join(HERE, "realism_clip.npz"), embeds_ref=er.numpy(), embeds_pred=ep.numpy(),
                        score=score.numpy(), seed=np.int64(SEED), transformers_version=np.array(transformers.__version__))
    print("realism_clip.npz:", score.numpy())


if __name__ == "__main__":
    main()
