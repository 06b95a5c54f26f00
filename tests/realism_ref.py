"""float64 torch restatements of the two realism metrics (test-only), written from their definitions:

  LPIPS-alex (Zhang et al. 2018; lpips 0.1.4 `LPIPS(net='alex', version='0.1')`, normalize=False, spatial=False):
      x -> (x - shift) / scale -> AlexNet features[0:12], taps relu1..relu5 ->
      per tap: f / (sqrt(sum_c f^2) + 1e-10) for both images, squared difference, 1 x 1 lin (no bias), mean over h, w ->
      summed over the five taps.
  CLIP image embedding (OpenAI `VisionTransformer.forward`, i.e. `CLIP.encode_image`):
      conv1 (patch, no bias) -> [class_embedding ; patches] + positional_embedding -> ln_pre -> resblocks
      { x + attn(ln_1(x)), x + mlp(ln_2(x)) with QuickGELU } -> ln_post(x[:, 0]) @ proj.

No `lpips` or `clip` package is available offline, so LPIPS is pinned to this restatement, not to the package.  Parameters
come as HF-named tower tensors (mobi_amd.realism.openai_to_hf's target names) and the AlexNet / lin tensors of
mobi_amd.realism.lpips_state_from_dicts.
"""
import torch
import torch.nn.functional as F

LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_ALEX = ((4, 2), (1, 2), (1, 1), (1, 1), (1, 1))          # (stride, pad) of conv1..conv5


def alexnet_taps(x, convs, dtype=torch.float64):
    """x: [N, 3, H, W] already scaled; convs [(w, b)] x 5 -> [relu1, ..., relu5] (in `dtype`, float64 by default)."""
    taps = []
    h = x.to(dtype)
    for j, ((w, b), (s, p)) in enumerate(zip(convs, _ALEX)):
        if j in (1, 2):
            h = F.max_pool2d(h, 3, 2)
        h = torch.relu(F.conv2d(h, w.to(h), b.to(h), stride=s, padding=p))
        taps.append(h)
    return taps


def unit_normalise(f, eps=1e-10):
    return f / (torch.sqrt(torch.sum(f * f, dim=1, keepdim=True)) + eps)


def layer_distance(fa, fb, lin, eps=1e-10):
    """One tap's term: fa, fb [N, C, H, W] (post-ReLU), lin [C] -> [N]."""
    d = (unit_normalise(fa, eps) - unit_normalise(fb, eps)) ** 2
    return (d * lin.to(d).view(1, -1, 1, 1)).sum(1).mean(dim=(1, 2))


def lpips(a, b, convs, lins, dtype=torch.float64):
    """a, b: [N, 3, H, W] in [-1, 1] -> [N] (float64 by default; tools/realism_timing.py times it in fp32)."""
    shift = torch.tensor(LPIPS_SHIFT, dtype=dtype, device=a.device).view(1, 3, 1, 1)
    scale = torch.tensor(LPIPS_SCALE, dtype=dtype, device=a.device).view(1, 3, 1, 1)
    ta = alexnet_taps((a.to(dtype) - shift) / scale, convs, dtype)
    tb = alexnet_taps((b.to(dtype) - shift) / scale, convs, dtype)
    return sum(layer_distance(fa, fb, l) for fa, fb, l in zip(ta, tb, lins))


def _ln(x, sd, name, eps=1e-5):
    return F.layer_norm(x, x.shape[-1:], sd[name + ".weight"].to(x), sd[name + ".bias"].to(x), eps)


def clip_layer(x, sd, pre, heads):
    """One encoder layer (OpenAI's ResidualAttentionBlock with QuickGELU) on tokens x [N, T, width]; sd: HF-named tower
    tensors, `pre` = "encoder.layers.<i>." -> [N, T, width] in x's type."""
    n, t, width = x.shape
    dh = width // heads

    def lin(v, name):
        return F.linear(v, sd[pre + name + ".weight"].to(v), sd[pre + name + ".bias"].to(v))

    h = _ln(x, sd, pre + "layer_norm1")
    q, k, v = (lin(h, f"self_attn.{m}_proj").view(n, t, heads, dh).transpose(1, 2) for m in "qkv")
    att = torch.softmax((q * dh ** -0.5) @ k.transpose(-1, -2), dim=-1)
    x = x + lin((att @ v).transpose(1, 2).reshape(n, t, width), "self_attn.out_proj")
    h = lin(_ln(x, sd, pre + "layer_norm2"), "mlp.fc1")
    return x + lin(h * torch.sigmoid(1.702 * h), "mlp.fc2")


def clip_embed(images, sd, heads=None, dtype=torch.float64):
    """images [N, 3, S, S] in [0, 1]; sd: HF-named tower + `visual_projection.weight` -> [N, embed] (float64 by default)."""
    sd = {k[len("vision_model."):] if k.startswith("vision_model.") else k: v for k, v in sd.items()}
    mean = torch.tensor(CLIP_MEAN, dtype=dtype, device=images.device).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD, dtype=dtype, device=images.device).view(1, 3, 1, 1)
    x = (images.to(dtype) - mean) / std
    wp = sd["embeddings.patch_embedding.weight"].to(x)
    width, patch = wp.shape[0], wp.shape[-1]
    heads = heads or width // 64
    x = F.conv2d(x, wp, stride=patch).flatten(2).transpose(1, 2)                    # [N, grid^2, width]
    cls = sd["embeddings.class_embedding"].to(x).expand(x.shape[0], 1, width)
    x = torch.cat([cls, x], 1) + sd["embeddings.position_embedding.weight"].to(x)
    x = _ln(x, sd, "pre_layrnorm")
    layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("encoder.layers."))
    for i in range(layers):
        x = clip_layer(x, sd, f"encoder.layers.{i}.", heads)
    pooled = _ln(x[:, 0], sd, "post_layernorm")
    return pooled @ sd["visual_projection.weight"].to(pooled).t()


def clip_score(ref, pred, sd, dtype=torch.float64):
    """100 cos of the two embeddings, [N]."""
    return 100.0 * F.cosine_similarity(clip_embed(ref, sd, dtype=dtype), clip_embed(pred, sd, dtype=dtype), dim=-1)


# ---------------------------------------------------------------------------------------------------------------------
# seeded parameters (oracle.weights: a parameter's values depend on its name, shape and seed only)
# ---------------------------------------------------------------------------------------------------------------------
CLIP_B32 = dict(hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12, image_size=224,
                patch_size=32, projection_dim=512)


def clip_b32_shapes(cfg=CLIP_B32):
    """transformers' CLIPVisionModelWithProjection parameter names and shapes at `cfg` (no transformers needed)."""
    w, inner, p = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"]
    grid = cfg["image_size"] // p
    v = "vision_model."
    s = {v + "embeddings.class_embedding": (w,), v + "embeddings.patch_embedding.weight": (w, 3, p, p),
         v + "embeddings.position_embedding.weight": (grid * grid + 1, w),
         v + "pre_layrnorm.weight": (w,), v + "pre_layrnorm.bias": (w,)}
    for i in range(cfg["num_hidden_layers"]):
        pre = f"{v}encoder.layers.{i}."
        for m in ("k_proj", "v_proj", "q_proj", "out_proj"):
            s[pre + f"self_attn.{m}.weight"], s[pre + f"self_attn.{m}.bias"] = (w, w), (w,)
        for n in ("layer_norm1", "layer_norm2"):
            s[pre + n + ".weight"], s[pre + n + ".bias"] = (w,), (w,)
        s[pre + "mlp.fc1.weight"], s[pre + "mlp.fc1.bias"] = (inner, w), (inner,)
        s[pre + "mlp.fc2.weight"], s[pre + "mlp.fc2.bias"] = (w, inner), (w,)
    s[v + "post_layernorm.weight"], s[v + "post_layernorm.bias"] = (w,), (w,)
    s["visual_projection.weight"] = (cfg["projection_dim"], w)
    return s


def clip_b32_state(seed, cfg=CLIP_B32):
    from oracle import weights as W
    return W.synth_state_dict(clip_b32_shapes(cfg), seed)


def clip_images(name, n, size=224):
    """Seeded images in [0, 1], f32 [n, 3, size, size]."""
    from oracle import weights as W
    return ((W.synth_input(name, (n, 3, size, size), kind="uniform") + 1.0) * 0.5).clamp(0.0, 1.0)


def alex_state(seed):
    """Seeded torchvision-AlexNet `features.*` and lpips `lin{k}.model.1.weight` dicts (lins 0.1 |noise|: trained lins are
    non-negative, of about that size)."""
    from oracle import weights as W
    shapes = {}
    for idx, cin, cout, k in ((0, 3, 64, 11), (3, 64, 192, 5), (6, 192, 384, 3), (8, 384, 256, 3), (10, 256, 256, 3)):
        shapes[f"features.{idx}.weight"], shapes[f"features.{idx}.bias"] = (cout, cin, k, k), (cout,)
    alex = W.synth_state_dict(shapes, seed)
    lin = {f"lin{j}.model.1.weight": torch.from_numpy(W.unit_noise(f"lin{j}", (1, c, 1, 1), seed)).float().abs() * 0.1
           for j, c in enumerate((64, 192, 384, 256, 256))}
    return alex, lin


def lpips_images(name, n, h, w):
    """Seeded images in [-1, 1], f32 [n, 3, h, w]."""
    from oracle import weights as W
    return W.synth_input(name, (n, 3, h, w), kind="uniform")
