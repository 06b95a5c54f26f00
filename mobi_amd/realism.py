"""Realism metrics on the engine: LPIPS (AlexNet) and CLIP score (ViT-B/32) -- the per-pair columns of MObI's realism table
(LPIPS, CLIP, and LPIPS of the lidar depth / intensity range images: D-LPIPS, I-LPIPS), as the reference's
`eval_tool/camera/{lpips,clip}_score.py` compute them, without the `lpips`, `clip` or `torchvision` packages.

  LPIPS      lpips 0.1.4 `LPIPS(net='alex', version='0.1')`, normalize=False, spatial=False: ScalingLayer
             (mobi_image_normalize, into conv1's 32-channel padded operand) -> AlexNet features[0:12] (five mobi_igemm
             convolutions; the ReLUs are taken by mobi_maxpool3s2 and mobi_lpips_distance) -> per layer
             mean_hw sum_c lin_c (unit-normalised a - unit-normalised b)^2 (mobi_lpips_distance, fp32), summed over layers.
  CLIP       OpenAI ViT-B/32 `encode_image` on CLIPVisionTower (the conditioning producer's tower at another config) ->
             768 -> 512 projection (mobi_linear_f32) -> 100 cos (mobi_row_cosine).

Storage type: fp16 unless asked otherwise (bf16 accepted), whatever `set_engine_dtype` says; norms, sums and the
projection are fp32.

    python -m mobi_amd.realism lpips --path_target A --path_pred B --alexnet alexnet-owt-7be5be79.pth --lin alex.pth
    python -m mobi_amd.realism clip --path_ref A --path_pred B --weights ViT-B-32.pt
print `LPIPS:  <mean>` / `CLIP:  <mean>`, the reference tools' lines.
"""
import argparse
import contextlib
import ctypes as C
import math
import pathlib
import sys

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, ops
import mobi_amd

IMAGE_EXTENSIONS = {"bmp", "jpg", "jpeg", "pgm", "png", "ppm", "tif", "tiff", "webp"}

# lpips.pretrained_networks.alexnet: torchvision alexnet().features indices of the five convolutions
# (index, cin, cout, kernel, stride, pad); a ReLU follows each, a 3 x 3 / 2 max-pool follows the first two ReLUs
ALEX_CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1),
              (10, 256, 256, 3, 1, 1))
LPIPS_SHIFT = (-0.030, -0.088, -0.188)              # lpips ScalingLayer
LPIPS_SCALE = (0.458, 0.448, 0.450)
LPIPS_EPS = 1e-10                                    # lpips.normalize_tensor
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
CIN_PAD = 32                                         # conv1's input channels, zero-padded for mobi_igemm


@contextlib.contextmanager
def storage_type(dtype):
    """Run the engine's modules with storage type `dtype`, restoring the caller's afterwards."""
    prev = mobi_amd.engine_dtype()
    mobi_amd.set_engine_dtype(dtype)
    try:
        yield
    finally:
        mobi_amd.set_engine_dtype(prev)


def _check_dtype(dtype):
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("realism metrics store in torch.float16 or torch.bfloat16")
    return dtype


def alexnet_shapes(h, w):
    """[(hin, win, hout, wout)] of the five convolutions for an h x w input."""
    out = []
    for i, (_, _, _, k, s, p) in enumerate(ALEX_CONVS):
        if i in (1, 2):                                   # the max-pools after relu1, relu2
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        out.append((h, w, ho, wo))
        h, w = ho, wo
    return out


# ---------------------------------------------------------------------------------------------------------------------
# LPIPS
# ---------------------------------------------------------------------------------------------------------------------
def lpips_state_from_dicts(alex_sd, lin_sd):
    """torchvision AlexNet state dict (`features.{0,3,6,8,10}.{weight,bias}`; classifier keys ignored) and lpips 0.1.4's
    `weights/v0.1/alex.pth` (`lin{0..4}.model.1.weight` [1, C, 1, 1]) -> ([(weight OIHW, bias)] x 5, [lin [C]] x 5), fp32."""
    convs, lins = [], []
    for j, (idx, cin, cout, k, _, _) in enumerate(ALEX_CONVS):
        wt, b = alex_sd[f"features.{idx}.weight"], alex_sd[f"features.{idx}.bias"]
        if tuple(wt.shape) != (cout, cin, k, k) or tuple(b.shape) != (cout,):
            raise ValueError(f"features.{idx}: shape {tuple(wt.shape)} / {tuple(b.shape)}, expected {(cout, cin, k, k)}")
        lin = lin_sd[f"lin{j}.model.1.weight"]
        if tuple(lin.shape) != (1, cout, 1, 1):
            raise ValueError(f"lin{j}.model.1.weight: shape {tuple(lin.shape)}, expected {(1, cout, 1, 1)}")
        convs.append((wt.detach().float().cpu(), b.detach().float().cpu()))
        lins.append(lin.detach().float().reshape(cout).cpu())
    return convs, lins


class LPIPS:
    """lpips 0.1.4 `LPIPS(net='alex')` forward (version 0.1, normalize=False, spatial=False) on the engine."""

    def __init__(self, convs, lins, dtype=torch.float16, device="cuda"):
        self.dtype, self.device = _check_dtype(dtype), torch.device(device)
        self.convs = [(w.float(), b.float()) for w, b in convs]        # fp32 host copies (plans, tests)
        self.packed = []
        for j, (w, b) in enumerate(self.convs):
            if j == 0:
                self.packed.append(ops.pack_conv_padded_cin(w, b, dtype, self.device, CIN_PAD))
            else:
                self.packed.append(ops.pack_conv(w, b, dtype, self.device))
        self.lins = [l.float().to(self.device).contiguous() for l in lins]

    @classmethod
    def from_state_dicts(cls, alex_sd, lin_sd, dtype=torch.float16, device="cuda"):
        return cls(*lpips_state_from_dicts(alex_sd, lin_sd), dtype=dtype, device=device)

    @classmethod
    def from_files(cls, alexnet_pth, lin_pth, dtype=torch.float16, device="cuda"):
        """torchvision's `alexnet-owt-7be5be79.pth` and lpips 0.1.4's `weights/v0.1/alex.pth`."""
        alex = torch.load(alexnet_pth, map_location="cpu")
        lin = torch.load(lin_pth, map_location="cpu")
        return cls.from_state_dicts(alex, lin, dtype=dtype, device=device)

    def __call__(self, a, b):
        """a, b: f32 [N, 3, H, W] in [-1, 1] -> f32 [N]."""
        if a.shape != b.shape or a.dim() != 4 or a.shape[1] != 3:
            raise ValueError(f"LPIPS takes two [N, 3, H, W] batches of the same shape, got {tuple(a.shape)}, {tuple(b.shape)}")
        n = a.shape[0]
        x = torch.cat([a, b], 0).to(device=self.device, dtype=torch.float32).contiguous()
        h = ops.image_normalize(x, LPIPS_SHIFT, LPIPS_SCALE, dtype=self.dtype, nhwc_channels=CIN_PAD)
        out = torch.zeros((n,), device=self.device, dtype=torch.float32)
        for j, (_, _, _, _, s, p) in enumerate(ALEX_CONVS):
            if j in (1, 2):
                h = ops.maxpool3s2(h, relu=True)                       # relu1 / relu2 then the pool
            h = ops.igemm(h, self.packed[j], stride=s, pad=(p, p))
            ops.lpips_distance(h, self.lins[j], out, LPIPS_EPS, relu_in_place=j in (2, 3))
        return out


def igemm_plan(h=256, w=256, pairs=64, dtype=torch.float16):
    """(mobi_igemm_kernel_variant, mobi_igemm_plan_splits) of the five AlexNet launches of a batch of `pairs` pairs at h x w,
    computed by the library's host logic without a launch (no device needed)."""
    lib = _lib.load()
    plans = []
    for j, ((idx, cin, cout, k, s, p), (hi, wi, ho, wo)) in enumerate(zip(ALEX_CONVS, alexnet_shapes(h, w))):
        q = _lib.IgemmParams()
        q.src0 = q.weight = q.out = q.bias = q.weight_tiled = 4096                  # placeholders: nothing is launched
        q.c0 = CIN_PAD if j == 0 else cin
        q.batch, q.hin, q.win, q.hout, q.wout = 2 * pairs, hi, wi, ho, wo
        q.kh = q.kw = k
        q.stride, q.pad_h, q.pad_w, q.groups = s, p, p, 1
        q.n_packed = q.cout = cout
        q.scale, q.dtype = 1.0, ops._dt(dtype)
        plans.append((lib.mobi_igemm_kernel_variant(C.byref(q)), lib.mobi_igemm_plan_splits(C.byref(q))))
    return plans


# ---------------------------------------------------------------------------------------------------------------------
# CLIP score
# ---------------------------------------------------------------------------------------------------------------------
def openai_to_hf(sd):
    """OpenAI CLIP state dict (`visual.*`; text-tower keys ignored) -> the tower's Hugging Face names plus
    `visual_projection.weight` [512, 768] (the transpose of `visual.proj`)."""
    out = {}
    pre = "visual."
    simple = {"conv1.weight": "embeddings.patch_embedding.weight", "class_embedding": "embeddings.class_embedding",
              "positional_embedding": "embeddings.position_embedding.weight", "ln_pre.weight": "pre_layrnorm.weight",
              "ln_pre.bias": "pre_layrnorm.bias", "ln_post.weight": "post_layernorm.weight", "ln_post.bias": "post_layernorm.bias"}
    block = {"attn.out_proj": "self_attn.out_proj", "ln_1": "layer_norm1", "ln_2": "layer_norm2", "mlp.c_fc": "mlp.fc1",
             "mlp.c_proj": "mlp.fc2"}
    for k, v in sd.items():
        if not k.startswith(pre):
            continue
        k = k[len(pre):]
        if k in simple:
            out[simple[k]] = v
        elif k == "proj":
            out["visual_projection.weight"] = v.t().contiguous()
        elif k.startswith("transformer.resblocks."):
            n, rest = k[len("transformer.resblocks."):].split(".", 1)
            dst = f"encoder.layers.{n}."
            if rest in ("attn.in_proj_weight", "attn.in_proj_bias"):
                leaf = rest.rsplit("_", 1)[1]
                for name, part in zip(("q_proj", "k_proj", "v_proj"), v.chunk(3, 0)):
                    out[f"{dst}self_attn.{name}.{leaf}"] = part.contiguous()
                continue
            mod, leaf = rest.rsplit(".", 1)
            if mod not in block:
                raise KeyError(f"unexpected OpenAI CLIP key visual.{k}")
            out[f"{dst}{block[mod]}.{leaf}"] = v
        else:
            raise KeyError(f"unexpected OpenAI CLIP key visual.{k}")
    return out


def _hf_config(sd):
    w = sd["embeddings.patch_embedding.weight"]
    width, patch = w.shape[0], w.shape[-1]
    layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layers."))
    tokens = sd["embeddings.position_embedding.weight"].shape[0]
    grid = int(round(math.sqrt(tokens - 1)))
    return dict(hidden_size=width, intermediate_size=sd["encoder.layers.0.mlp.fc1.weight"].shape[0],
                num_hidden_layers=layers, num_attention_heads=width // 64, image_size=grid * patch, patch_size=patch)


def _read_checkpoint(path):
    """A TorchScript archive (what `clip.load` caches) or a plain `torch.save` state dict / module -> state dict."""
    try:
        return torch.jit.load(path, map_location="cpu").state_dict()
    except RuntimeError:
        obj = torch.load(path, map_location="cpu", weights_only=False)
        return obj.state_dict() if hasattr(obj, "state_dict") else obj


class CLIPScore:
    """100 cos(encode_image(ref), encode_image(pred)) with OpenAI's ViT-B/32 image tower on the engine."""

    def __init__(self, tower, projection, dtype=torch.float16, device="cuda"):
        self.dtype, self.device = _check_dtype(dtype), torch.device(device)
        self.tower = tower.to(self.device).eval()
        self.proj = projection.detach().float().to(self.device).contiguous()    # [embed, width]

    @classmethod
    def from_state_dict(cls, sd, dtype=torch.float16, device="cuda"):
        """Hugging Face names (`vision_model.` prefix optional) plus `visual_projection.weight`."""
        from .ldm.modules.encoders.modules import CLIPVisionTower
        sd = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items()}
        sd = {k: v for k, v in sd.items() if not k.endswith("position_ids")}
        proj = sd.pop("visual_projection.weight")
        tower = CLIPVisionTower(**_hf_config(sd))
        tower.load_state_dict({k: v.float() for k, v in sd.items()})
        return cls(tower, proj.float(), dtype=dtype, device=device)

    @classmethod
    def from_openai(cls, path, dtype=torch.float16, device="cuda"):
        """OpenAI's `ViT-B-32.pt` (the file `clip.load('ViT-B/32')` caches)."""
        return cls.from_state_dict(openai_to_hf(_read_checkpoint(path)), dtype=dtype, device=device)

    def embed(self, images):
        """f32 [N, 3, S, S] in [0, 1] -> f32 [N, embed] (encode_image)."""
        x = images.to(device=self.device, dtype=torch.float32).contiguous()
        x = ops.image_normalize(x, CLIP_MEAN, CLIP_STD)
        with torch.no_grad(), storage_type(self.dtype):
            pooled = self.tower.pooled(x)
        return ops.linear_f32(pooled, self.proj)

    def __call__(self, ref, pred):
        if ref.shape != pred.shape:
            raise ValueError(f"CLIP score takes two batches of the same shape, got {tuple(ref.shape)}, {tuple(pred.shape)}")
        n = ref.shape[0]
        e = self.embed(torch.cat([ref, pred], 0))
        return ops.row_cosine(e[:n].contiguous(), e[n:].contiguous(), eps=1e-8, scale=100.0)


# ---------------------------------------------------------------------------------------------------------------------
# files (the reference tools' data path)
# ---------------------------------------------------------------------------------------------------------------------
def image_files(path):
    """Sorted over the reference's IMAGE_EXTENSIONS, as its ImagePathsDataset.get_files."""
    path = pathlib.Path(path)
    return sorted([f for ext in IMAGE_EXTENSIONS for f in path.glob(f"*.{ext}")])


def paired_files(path_a, path_b):
    fa, fb = image_files(path_a), image_files(path_b)
    if len(fa) != len(fb):
        raise ValueError(f"Number of reference and predicted images should be same ({len(fa)} in {path_a}, {len(fb)} in {path_b})")
    return list(zip(fa, fb))


def _to_tensor(img):
    """PIL -> f32 [C, H, W] / 255 (torchvision ToTensor)."""
    a = np.asarray(img, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(a.copy()).permute(2, 0, 1).float().div(255)


def lpips_image(path, size=256):
    """The LPIPS tool's transform: .convert('RGB') -> /255 -> bilinear resize to size x size (align_corners=False, no
    antialias: torchvision 0.11's tensor Resize) -> (x - 0.5) / 0.5.  f32 [3, size, size]."""
    from PIL import Image
    with Image.open(path) as im:
        x = _to_tensor(im.convert("RGB"))
    x = F.interpolate(x[None], size=(size, size), mode="bilinear", align_corners=False)[0]
    return (x - 0.5) / 0.5


def clip_resize_crop(img, size=224):
    """torchvision 0.11 Resize(size, BICUBIC) + CenterCrop(size) on a PIL image."""
    from PIL import Image
    w, h = img.size
    short, long = (w, h) if w <= h else (h, w)
    if short != size:
        ns, nl = size, int(size * long / short)
        img = img.resize((ns, nl) if w <= h else (nl, ns), Image.BICUBIC)
    w, h = img.size
    top, left = int(round((h - size) / 2.0)), int(round((w - size) / 2.0))
    return img.crop((left, top, left + size, top + size))


def clip_image(path, size=224):
    """clip's preprocess without the Normalize (CLIPScore applies it on the device): f32 [3, size, size] in [0, 1]."""
    from PIL import Image
    with Image.open(path) as im:
        return _to_tensor(clip_resize_crop(im, size).convert("RGB"))


def _score_pairs(pairs, load, metric, batch_size):
    vals = []
    for i in range(0, len(pairs), batch_size):
        chunk = pairs[i:i + batch_size]
        a = torch.stack([load(p) for p, _ in chunk])
        b = torch.stack([load(q) for _, q in chunk])
        vals.append(metric(a, b))
    return torch.cat(vals) if vals else torch.zeros((0,))


def lpips_score_paths(path_target, path_pred, model, batch_size=64):
    """(mean, per-pair f32 tensor) over the sorted, index-paired images of two directories."""
    per = _score_pairs(paired_files(path_target, path_pred), lpips_image, model, batch_size)
    return per.mean().item(), per


def clip_score_paths(path_ref, path_pred, model, batch_size=64):
    per = _score_pairs(paired_files(path_ref, path_pred), clip_image, model, batch_size)
    return per.mean().item(), per


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m mobi_amd.realism", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    sub = ap.add_subparsers(dest="metric", required=True)
    lp = sub.add_parser("lpips", help="LPIPS (AlexNet) between index-paired images")
    lp.add_argument("--path_target", required=True)
    lp.add_argument("--path_pred", required=True)
    lp.add_argument("--alexnet", required=True, help="torchvision alexnet-owt-7be5be79.pth")
    lp.add_argument("--lin", required=True, help="lpips 0.1.4 weights/v0.1/alex.pth")
    cp = sub.add_parser("clip", help="CLIP score (ViT-B/32) between index-paired images")
    cp.add_argument("--path_ref", required=True)
    cp.add_argument("--path_pred", required=True)
    cp.add_argument("--weights", required=True, help="OpenAI ViT-B-32.pt")
    for p in (lp, cp):
        p.add_argument("--batch-size", type=int, default=64)
        p.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
    args = ap.parse_args(argv)
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    if args.metric == "lpips":
        model = LPIPS.from_files(args.alexnet, args.lin, dtype=dtype)
        v, _ = lpips_score_paths(args.path_target, args.path_pred, model, args.batch_size)
        print("LPIPS: ", v)
    else:
        model = CLIPScore.from_openai(args.weights, dtype=dtype)
        v, _ = clip_score_paths(args.path_ref, args.path_pred, model, args.batch_size)
        print("CLIP: ", v)
    return v


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
