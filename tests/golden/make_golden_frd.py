"""Regenerate tests/golden/frd.npz from the reference's own FRD code (eval_tool/lidar/frd_score.py, rangenet/model.py), on CPU:

    python tests/golden/make_golden_frd.py /path/to/reference

Stored: the codes of six synthetic 512 x 512 range views (tests/frd_ref.view_codes: depth and intensity on the rows the
64-row nearest resize reads; tests/frd_ref.views_from_codes rebuilds the views, angles and boundary depths included), the
reference RangePathDataset's validity mask (bit-packed) and a strided sample of its channel values, the
reference Model's fp64 features (loaded strict=True from tests/frd_ref.seeded_state_dicts, calibrated on these views, so
our key names are pinned to the reference's), and calculate_frechet_distance on the four cases of tests/frd_ref.frechet_cases (regenerated
from their seed, not stored).  Weights are not stored.
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import frd_ref as R  # noqa: E402

SEED_WEIGHTS, SEED_A, SEED_B = 20261016, 11, 12
SAMPLE = 256          # every 256th pixel of the prepared 64 x 1024 channels is stored


def codes():
    a, b = R.view_codes(3, SEED_A), R.view_codes(3, SEED_B, far=True)
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "eval_tool", "lidar"))
    import frd_score as ref                                   # noqa: E402  (the reference tool)
    from rangenet.model import Model                          # noqa: E402
    import yaml

    dcode, icode = codes()
    v = R.views_from_codes(dcode, icode)
    with tempfile.TemporaryDirectory() as d:
        for i, a in enumerate(v):
            np.save(os.path.join(d, f"{i:02d}.npy"), a)
        ds = ref.RangePathDataset(d)
        order = [int(os.path.basename(str(f))[:2]) for f in ds.files]
        prep = torch.stack([ds[order.index(i)] for i in range(len(v))])          # f32 [6, 5, 64, 1024]
    mask = ~(prep == -1).all(1)
    x = prep.double()
    bb, dec = R.seeded_state_dicts(SEED_WEIGHTS, x)
    cfg = yaml.safe_load(open(os.path.join(ref_root, "eval_tool", "lidar", "rangenet", "config.yaml")))
    model = Model(cfg).double().eval()
    model.backbone.load_state_dict(bb, strict=True)
    model.decoder.load_state_dict(dec, strict=True)
    with torch.no_grad():
        feats = model(x, return_final_logits=True, agg_type="depth")

    stat = lambda f: (f.mean(0), np.cov(f, rowvar=False))
    out = {f"fd_{k}": np.float64(ref.calculate_frechet_distance(*stat(p), *stat(q))) for k, (p, q) in R.frechet_cases().items()}
    np.savez_compressed(os.path.join(HERE, "frd.npz"), depth_codes=dcode, int_codes=icode,
                        mask=np.packbits(mask.numpy(), axis=-1), prep_sample=prep.reshape(6, 5, -1)[:, :, ::SAMPLE].numpy(),
                        features=feats.astype(np.float64), seeds=np.array([SEED_WEIGHTS, SEED_A, SEED_B]), **out)
    print("features", feats.shape, float(np.abs(feats).max()), "distances", out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MOBI_REFERENCE_ROOT", "../reference"))
