"""Realism metrics on the engine: LPIPS (AlexNet) and CLIP score (ViT-B/32) -- the per-pair columns of MObI's realism table
(LPIPS, CLIP, and LPIPS of the lidar depth / intensity range images: D-LPIPS, I-LPIPS), as the reference's
`eval_tool/camera/{lpips,clip}_score.py` compute them, without the `lpips`, `clip` or `torchvision` packages.

  LPIPS      lpips 0.1.4 `LPIPS(net='alex', version='0.1')`, normalize=False, spatial=False: ScalingLayer
             (mobi_image_normalize, into conv1's 32-channel padded operand) -> AlexNet features[0:12] (five mobi_igemm
             convolutions; the ReLUs are taken by mobi_maxpool3s2 and mobi_lpips_distance) -> per layer
             mean_hw sum_c lin_c (unit-normalised a - unit-normalised b)^2 (mobi_lpips_distance, fp32), summed over layers.
  CLIP       OpenAI ViT-B/32 `encode_image` on CLIPVisionTower (the conditioning producer's tower at another config) ->
             768 -> 512 projection (mobi_linear_f32) -> 100 cos (mobi_row_cosine).
  FID        `eval_tool/camera/fid_score.py`: the Fréchet distance of raw CLIP `encode_image` embeddings of two un-paired
             image sets (CLIPScore.embed), moments in fp64 on the device (mobi_feature_moments), distance on the host.
  FRD        `eval_tool/lidar/frd_score.py`: the same distance on RangeNet++ 'depth' features of 64 x 1024 range views:
             mobi_frd_input -> 67 mobi_igemm launches (BN folded, MOBI_EPI_LEAKY_RELU; stride-(1, 2) and transposed
             convolutions rewritten on the paired-width view) -> mobi_band_mean (with the last decoder skip).

Storage type: fp16 unless asked otherwise (bf16 accepted), whatever `set_engine_dtype` says; norms, sums and the
projection are fp32.

    python -m mobi_amd.realism lpips --path_target A --path_pred B --alexnet alexnet-owt-7be5be79.pth --lin alex.pth
    python -m mobi_amd.realism clip --path_ref A --path_pred B --weights ViT-B-32.pt
    python -m mobi_amd.realism fid --path_target A --path_pred B --weights ViT-B-32.pt
    python -m mobi_amd.realism frd --path-target A --path-pred B --weights-dir DIR
print `LPIPS:  <mean>` / `CLIP:  <mean>` / `FID:  <v>` / `FRD:  <v>`, the reference tools' lines.
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
# Fréchet distance (FID, FRD): fp64 moments on the device, the distance on the host
# ---------------------------------------------------------------------------------------------------------------------
def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2), fp64 numpy, without scipy: tr sqrtm(S1 S2) is the sum of
    sqrt(max(lambda, 0)) over the eigenvalues of the symmetric S1^1/2 S2 S1^1/2 (S1^1/2 from eigh(S1), eigenvalues clamped
    at 0), which has the eigenvalues of S1 S2.  Intended differences to the reference's scipy.linalg.sqrtm form: no complex
    branch (the eigenvalues of a product of two PSD matrices are real and >= 0; rounding below 0 is clamped), hence no
    'Imaginary component' error, and no eps-offset retry."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    s1, s2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    if mu1.shape != mu2.shape or s1.shape != s2.shape:
        raise ValueError(f"Fréchet distance of mismatched statistics: {mu1.shape} / {mu2.shape}, {s1.shape} / {s2.shape}")
    w, v = np.linalg.eigh((s1 + s1.T) / 2)
    r = (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T
    m = r @ s2 @ r
    lam = np.linalg.eigvalsh((m + m.T) / 2)
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.clip(lam, 0.0, None)).sum())


class FrechetStats:
    """Streaming mean / covariance (ddof 1) of f32 [rows, dim] feature batches: sum and cross products of rows minus a shift
    (the first batch's mean) accumulated in fp64 on the device by mobi_feature_moments, in a fixed order (bit-reproducible);
    nothing goes to the host before `mu_sigma`."""

    def __init__(self, dim, device="cuda"):
        self.dim, self.device, self.n = dim, torch.device(device), 0
        self.shift = None
        self.sum = torch.zeros((dim,), device=self.device, dtype=torch.float64)
        self.cross = torch.zeros((dim, dim), device=self.device, dtype=torch.float64)

    def update(self, feat):
        feat = feat.to(device=self.device, dtype=torch.float32).contiguous()
        if feat.dim() != 2 or feat.shape[1] != self.dim:
            raise ValueError(f"feature batch {tuple(feat.shape)}, expected [rows, {self.dim}]")
        if feat.shape[0] == 0:
            return self
        if self.shift is None:
            s = torch.zeros((self.dim,), device=self.device, dtype=torch.float64)
            ops.feature_moments(feat, None, s)
            self.shift = s / feat.shape[0]
        ops.feature_moments(feat, self.shift, self.sum, self.cross)
        self.n += feat.shape[0]
        return self

    def mu_sigma(self):
        if self.n < 2:
            raise ValueError(f"a Fréchet distance needs at least 2 feature rows per set, got {self.n}")
        s, c, shift = (t.cpu().numpy() for t in (self.sum, self.cross, self.shift))
        mu = shift + s / self.n
        sigma = (c - np.outer(s, s) / self.n) / (self.n - 1)
        return mu, (sigma + sigma.T) / 2


def _stats_of_batches(batches, embed, dim, device):
    st = FrechetStats(dim, device)
    for b in batches:
        st.update(embed(b))
    return st.mu_sigma()


def _batches(x, batch_size):
    return [x[i:i + batch_size] for i in range(0, x.shape[0], batch_size)]


class FID:
    """FID as eval_tool/camera/fid_score.py computes it: the Fréchet distance of raw CLIP ViT-B/32 `encode_image` embeddings
    (512-d, not L2-normalised; its InceptionV3 wrapper returns the CLIP embedding), over two un-paired image sets."""

    def __init__(self, clip, batch_size=64):
        self.clip, self.batch_size = clip, batch_size

    @classmethod
    def from_openai(cls, path, dtype=torch.float16, device="cuda", batch_size=64):
        return cls(CLIPScore.from_openai(path, dtype=dtype, device=device), batch_size)

    def stats(self, images):
        """f32 [N, 3, 224, 224] in [0, 1] (or an iterable of such batches) -> (mu, sigma), fp64 numpy."""
        batches = _batches(images, self.batch_size) if torch.is_tensor(images) else images
        return _stats_of_batches(batches, self.clip.embed, self.clip.proj.shape[0], self.clip.device)

    def __call__(self, set_a, set_b):
        return frechet_distance(*self.stats(set_a), *self.stats(set_b))


# ---------------------------------------------------------------------------------------------------------------------
# RangeNet++ (Darknet-53 backbone + decoder, OS 32, eval_tool/lidar/rangenet/model.py) on mobi_igemm
# ---------------------------------------------------------------------------------------------------------------------
RANGENET_BLOCKS = (1, 2, 8, 8, 4)                 # Darknet-53 BasicBlocks per encoder stage
RANGENET_ENC = ((32, 64), (64, 128), (128, 256), (256, 512), (512, 1024))
RANGENET_DEC = ((1024, 512), (512, 256), (256, 128), (128, 64), (64, 32))
RANGENET_H, RANGENET_W, RANGENET_BANDS = 64, 1024, 16
FRD_DEPTH = (1.4, 54.0)
BN_EPS = 1e-5
BN_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
RANGENET_MAX_BATCH = 128        # every operand of the heaviest launches below 2 GB (the ring kernels' buffer offsets)


def rangenet_keys():
    """(backbone keys, decoder keys) of the reference's two state dicts (312 and 95)."""
    bn = lambda pre: [f"{pre}.{k}" for k in BN_KEYS]
    block = lambda pre: [f"{pre}.conv1.weight", *bn(f"{pre}.bn1"), f"{pre}.conv2.weight", *bn(f"{pre}.bn2")]
    bb = ["conv1.weight", *bn("bn1")]
    for i, nb in enumerate(RANGENET_BLOCKS, 1):
        bb += [f"enc{i}.conv.weight", *bn(f"enc{i}.bn")]
        for r in range(nb):
            bb += block(f"enc{i}.residual_{r}")
    dec = []
    for i in range(5, 0, -1):
        dec += [f"dec{i}.upconv.weight", f"dec{i}.upconv.bias", *bn(f"dec{i}.bn"), *block(f"dec{i}.residual")]
    return bb, dec


def _check_keys(sd, want, what):
    have, want = set(sd.keys()), set(want)
    missing, extra = sorted(want - have), sorted(have - want)
    if missing or extra:
        raise KeyError(f"RangeNet {what} state dict: missing keys {missing[:8]}{' ...' if len(missing) > 8 else ''}, "
                       f"unexpected keys {extra[:8]}{' ...' if len(extra) > 8 else ''}")


def fold_bn(weight, sd, pre, bias=None, eps=BN_EPS):
    """Conv weight [O, ...] (+ bias) followed by eval-mode BatchNorm `pre` -> (weight, bias) with the BN folded, fp64."""
    w = weight.double()
    s = sd[f"{pre}.weight"].double() / torch.sqrt(sd[f"{pre}.running_var"].double() + eps)
    b = sd[f"{pre}.bias"].double() - sd[f"{pre}.running_mean"].double() * s
    if bias is not None:
        b = b + bias.double() * s
    return w * s.reshape(-1, *([1] * (w.dim() - 1))), b


def stride2_weight(w):
    """3 x 3 conv, stride (1, 2), pad 1 on [H][W][C] == 3 x 2 conv, stride 1, pad (1, 1 left) on the paired view [H][W/2][2C]:
    tap 0 (pair x - 1) = [0 | W[..., 0]], tap 1 (pair x) = [W[..., 1] | W[..., 2]].  [O, C, 3, 3] -> [O, 2C, 3, 2]."""
    o, c, kh, kw = w.shape
    assert (kh, kw) == (3, 3)
    out = w.new_zeros((o, 2 * c, 3, 2))
    out[:, c:, :, 0] = w[:, :, :, 0]
    out[:, :c, :, 1] = w[:, :, :, 1]
    out[:, c:, :, 1] = w[:, :, :, 2]
    return out


def upconv_weight(w, bias):
    """ConvTranspose2d(k [1, 4], stride [1, 2], pad [0, 1]) weight [Cin, Cout, 1, 4] (+ bias [Cout]) == 1 x 3 conv, pad (0, 1),
    with 2 Cout outputs whose [H][W][2 Cout] result IS the [H][2W][Cout] one: even half taps (W3^T, W1^T, 0), odd half
    (0, W2^T, W0^T), bias duplicated.  -> ([2 Cout, Cin, 1, 3], [2 Cout])."""
    cin, cout, kh, kw = w.shape
    assert (kh, kw) == (1, 4)
    t = w[:, :, 0, :].permute(1, 0, 2)                     # [Cout, Cin, 4]
    out = w.new_zeros((2 * cout, cin, 1, 3))
    out[:cout, :, 0, 0], out[:cout, :, 0, 1] = t[:, :, 3], t[:, :, 1]
    out[cout:, :, 0, 1], out[cout:, :, 0, 2] = t[:, :, 2], t[:, :, 0]
    return out, torch.cat([bias, bias])


def rangenet_layers(bb, dec):
    """The 67 convolutions in launch order: (name, weight OIHW fp64, bias fp64, kind) with BN folded and the stride / transpose
    rewrites applied.  kind: 'stem' (5 -> 32, input padded to 32), 'down' (3 x 2 on the paired view), '1x1', '3x3', 'up'."""
    out = [("conv1", *fold_bn(bb["conv1.weight"], bb, "bn1"), "stem")]
    for i, nb in enumerate(RANGENET_BLOCKS, 1):
        w, b = fold_bn(bb[f"enc{i}.conv.weight"], bb, f"enc{i}.bn")
        out.append((f"enc{i}.conv", stride2_weight(w), b, "down"))
        for r in range(nb):
            pre = f"enc{i}.residual_{r}"
            out.append((f"{pre}.conv1", *fold_bn(bb[f"{pre}.conv1.weight"], bb, f"{pre}.bn1"), "1x1"))
            out.append((f"{pre}.conv2", *fold_bn(bb[f"{pre}.conv2.weight"], bb, f"{pre}.bn2"), "3x3"))
    for i in range(5, 0, -1):
        w, b = fold_bn(dec[f"dec{i}.upconv.weight"].transpose(0, 1), dec, f"dec{i}.bn", bias=dec[f"dec{i}.upconv.bias"])
        w, b = upconv_weight(w.transpose(0, 1), b)            # (the BN scales the transpose's output channels: axis 1)
        out.append((f"dec{i}.upconv", w, b, "up"))
        pre = f"dec{i}.residual"
        out.append((f"{pre}.conv1", *fold_bn(dec[f"{pre}.conv1.weight"], dec, f"{pre}.bn1"), "1x1"))
        out.append((f"{pre}.conv2", *fold_bn(dec[f"{pre}.conv2.weight"], dec, f"{pre}.bn2"), "3x3"))
    return out


def rangenet_shapes(batch, h=RANGENET_H, w=RANGENET_W):
    """[(batch, hin, win, cin, hout, wout, cout, kh, kw, pad_h, pad_w)] of the 67 launches (cin / cout as mobi_igemm sees them)."""
    out = [(batch, h, w, CIN_PAD, h, w, 32, 3, 3, 1, 1)]
    for (ci, co), nb in zip(RANGENET_ENC, RANGENET_BLOCKS):
        out.append((batch, h, w // 2, 2 * ci, h, w // 2, co, 3, 2, 1, 1))
        w //= 2
        out += [(batch, h, w, co, h, w, ci, 1, 1, 0, 0), (batch, h, w, ci, h, w, co, 3, 3, 1, 1)] * nb
    for ci, co in RANGENET_DEC:
        out.append((batch, h, w, ci, h, w, 2 * co, 1, 3, 0, 1))
        w *= 2
        out += [(batch, h, w, co, h, w, ci, 1, 1, 0, 0), (batch, h, w, ci, h, w, co, 3, 3, 1, 1)]
    return out


def rangenet_igemm_plan(batch=64, dtype=torch.float16):
    """(mobi_igemm_kernel_variant, mobi_igemm_plan_splits) of the 67 MOBI_EPI_LEAKY_RELU launches of a batch, computed by the
    library's host logic without a launch (no device needed)."""
    lib = _lib.load()
    plans = []
    for j, (n, hi, wi, ci, ho, wo, co, kh, kw, ph, pw) in enumerate(rangenet_shapes(batch)):
        q = _lib.IgemmParams()
        q.src0 = q.weight = q.out = q.bias = q.weight_tiled = 4096                  # placeholders: nothing is launched
        q.c0, q.batch, q.hin, q.win, q.hout, q.wout = ci, n, hi, wi, ho, wo
        q.kh, q.kw, q.stride, q.pad_h, q.pad_w, q.groups = kh, kw, 1, ph, pw, 1
        q.n_packed = q.cout = co
        q.scale, q.dtype, q.epilogue = 1.0, ops._dt(dtype), _lib.EPI_LEAKY_RELU
        if kh == 3 and kw == 3 and j > 0:
            q.residual = 4096
        plans.append((lib.mobi_igemm_kernel_variant(C.byref(q)), lib.mobi_igemm_plan_splits(C.byref(q))))
    return plans


class RangeNet:
    """RangeNet++ (Darknet-53, OS 32) features for FRD: Model(x, return_final_logits=True, agg_type='depth') in eval mode.
    Every convolution is one mobi_igemm launch with BatchNorm folded into weights and bias and MOBI_EPI_LEAKY_RELU (the
    BasicBlock's residual in the same epilogue, after the activation); decoder skips by mobi_add, the last one inside
    mobi_band_mean."""

    def __init__(self, layers, dtype=torch.float16, device="cuda"):
        self.dtype, self.device = _check_dtype(dtype), torch.device(device)
        self.packed = {}
        for name, w, b, kind in layers:
            w = w.float()
            if kind == "stem":
                self.packed[name] = ops.pack_conv_padded_cin(w, b.float(), dtype, self.device, CIN_PAD)
            else:
                self.packed[name] = ops.pack_conv(w, b.float(), dtype, self.device)

    @classmethod
    def from_state_dicts(cls, backbone_sd, decoder_sd, dtype=torch.float16, device="cuda"):
        bb_keys, dec_keys = rangenet_keys()
        _check_keys(backbone_sd, bb_keys, "backbone")
        _check_keys(decoder_sd, dec_keys, "segmentation_decoder")
        bb = {k: v.detach().cpu() for k, v in backbone_sd.items()}
        dec = {k: v.detach().cpu() for k, v in decoder_sd.items()}
        return cls(rangenet_layers(bb, dec), dtype=dtype, device=device)

    def _conv(self, x, name, residual=None, **kw):
        return ops.igemm(x, self.packed[name], residual=residual, leaky=True, **kw)

    def _block(self, x, pre):
        t = self._conv(x, f"{pre}.conv1")
        return self._conv(t, f"{pre}.conv2", residual=x)

    def forward_prepared(self, x):
        """T [B, 64, 1024, 32] (mobi_frd_input) -> f32 [B, 512]."""
        n, h, w, _ = x.shape
        x = self._conv(x, "conv1")
        skips = [x]
        for i, nb in enumerate(RANGENET_BLOCKS, 1):
            n, h, w, c = x.shape
            x = self._conv(x.view(n, h, w // 2, 2 * c), f"enc{i}.conv", hout=h, wout=w // 2)
            for r in range(nb):
                x = self._block(x, f"enc{i}.residual_{r}")
            skips.append(x)
        skips.pop()                                          # the last encoder output is the decoder's input, not a skip
        for i in range(5, 0, -1):
            u = self._conv(x, f"dec{i}.upconv")
            n, h, w, c2 = u.shape
            u = u.view(n, h, 2 * w, c2 // 2)                 # [H][W][2C] is [H][2W][C]
            x = self._block(u, f"dec{i}.residual")
            skip = skips.pop()
            if i > 1:
                x = ops.add(x, skip)
        return ops.band_mean(x, skip, RANGENET_BANDS)

    def prepare(self, raw):
        """f32 [B, 4, h, w] range views -> T [B, 64, 1024, 32] (mobi_frd_input)."""
        raw = raw.to(device=self.device, dtype=torch.float32).contiguous()
        return ops.frd_input(raw, self.dtype, RANGENET_H, RANGENET_W, CIN_PAD, *FRD_DEPTH)

    def features(self, raw, batch_size=64):
        """f32 [B, 4, h, w] range views (normalised depth, intensity, pitch, yaw) -> f32 [B, 512]."""
        if raw.dim() != 4 or raw.shape[1] != 4:
            raise ValueError(f"RangeNet takes [B, 4, h, w] range views, got {tuple(raw.shape)}")
        bs = max(1, min(batch_size, RANGENET_MAX_BATCH))
        outs = []
        with torch.no_grad():
            for i in range(0, raw.shape[0], bs):
                outs.append(self.forward_prepared(self.prepare(raw[i:i + bs])))
        return torch.cat(outs) if outs else torch.zeros((0, 512), device=self.device)


class FRD:
    """FRD as eval_tool/lidar/frd_score.py computes it: the Fréchet distance of RangeNet++ 'depth' features (512-d)."""

    def __init__(self, net, batch_size=64):
        self.net, self.batch_size = net, batch_size

    @classmethod
    def from_state_dicts(cls, backbone_sd, decoder_sd, dtype=torch.float16, device="cuda", batch_size=64):
        return cls(RangeNet.from_state_dicts(backbone_sd, decoder_sd, dtype=dtype, device=device), batch_size)

    @classmethod
    def from_folder(cls, path, dtype=torch.float16, device="cuda", batch_size=64):
        """The reference's model folder: `<path>/backbone` and `<path>/segmentation_decoder` state dicts."""
        path = pathlib.Path(path)
        bb = torch.load(path / "backbone", map_location="cpu", weights_only=True)
        dec = torch.load(path / "segmentation_decoder", map_location="cpu", weights_only=True)
        return cls.from_state_dicts(bb, dec, dtype=dtype, device=device, batch_size=batch_size)

    def features(self, raw):
        return self.net.features(raw, self.batch_size)

    def stats(self, views):
        """f32 [N, 4, h, w] (or an iterable of such batches) -> (mu, sigma), fp64 numpy."""
        batches = _batches(views, self.batch_size) if torch.is_tensor(views) else views
        return _stats_of_batches(batches, self.features, RANGENET_BANDS * 32, self.net.device)

    def __call__(self, set_a, set_b):
        return frechet_distance(*self.stats(set_a), *self.stats(set_b))


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


def range_files(path):
    """Sorted `*.npy` range views of a directory (the reference globs them unsorted: the statistics do not depend on order)."""
    return sorted(pathlib.Path(path).glob("*.npy"))


def load_range_view(path):
    """[4, h, w] (normalised depth, intensity, pitch, yaw) -> f32 [4, h, w]."""
    a = np.load(path)
    if a.ndim != 3 or a.shape[0] != 4:
        raise ValueError(f"{path}: range view of shape {a.shape}, expected [4, h, w]")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _need_two(files, path):
    if len(files) < 2:
        raise ValueError(f"a Fréchet distance needs at least 2 files per set, found {len(files)} in {path}")
    return files


def _load_batches(files, load, batch_size):
    for i in range(0, len(files), batch_size):
        yield torch.stack([load(f) for f in files[i:i + batch_size]])


def fid_paths(path_target, path_pred, model, batch_size=64):
    """FID between the (un-paired, any count >= 2) images of two directories."""
    files = [_need_two(image_files(p), p) for p in (path_target, path_pred)]
    stats = [model.stats(_load_batches(f, clip_image, batch_size)) for f in files]
    return frechet_distance(*stats[0], *stats[1])


def frd_paths(path_target, path_pred, model, batch_size=64):
    """FRD between the (un-paired, any count >= 2) `*.npy` range views of two directories."""
    files = [_need_two(range_files(p), p) for p in (path_target, path_pred)]
    stats = [model.stats(_load_batches(f, load_range_view, batch_size)) for f in files]
    return frechet_distance(*stats[0], *stats[1])


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
    fp = sub.add_parser("fid", help="FID on CLIP ViT-B/32 embeddings between two image sets")
    fp.add_argument("--path_target", required=True)
    fp.add_argument("--path_pred", required=True)
    fp.add_argument("--weights", required=True, help="OpenAI ViT-B-32.pt")
    rp = sub.add_parser("frd", help="FRD on RangeNet++ features between two sets of *.npy range views")
    rp.add_argument("--path-target", required=True)
    rp.add_argument("--path-pred", required=True)
    rp.add_argument("--weights-dir", required=True, help="folder with the RangeNet++ `backbone` and `segmentation_decoder`")
    for p in (lp, cp, fp, rp):
        p.add_argument("--batch-size", type=int, default=64)
        p.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
    args = ap.parse_args(argv)
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    if args.metric == "lpips":
        model = LPIPS.from_files(args.alexnet, args.lin, dtype=dtype)
        v, _ = lpips_score_paths(args.path_target, args.path_pred, model, args.batch_size)
        print("LPIPS: ", v)
    elif args.metric == "clip":
        model = CLIPScore.from_openai(args.weights, dtype=dtype)
        v, _ = clip_score_paths(args.path_ref, args.path_pred, model, args.batch_size)
        print("CLIP: ", v)
    elif args.metric == "fid":
        model = FID.from_openai(args.weights, dtype=dtype, batch_size=args.batch_size)
        v = fid_paths(args.path_target, args.path_pred, model, args.batch_size)
        print("FID: ", v)
    else:
        model = FRD.from_folder(args.weights_dir, dtype=dtype, batch_size=args.batch_size)
        v = frd_paths(args.path_target, args.path_pred, model, args.batch_size)
        print("FRD: ", v)
    return v


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
