"""fp64 restatement of FRD's feature path (eval_tool/lidar/frd_score.py + rangenet/model.py), written from the model's
definition in plain torch functional ops, plus the seeded RangeNet++ state dicts and synthetic range views the tests and
tests/golden/make_golden_frd.py share.

    prepare(view)                 RangePathDataset.__getitem__: [4, h, w] fp64 numpy -> f32 [5, 64, 1024]
    forward(bb, dec, x)           Model(x, return_final_logits=True, agg_type='depth'), eval mode, fp64 -> [B, 512]
    seeded_state_dicts(seed, x)   backbone / decoder state dicts with the reference's key names; BatchNorm running
                                  statistics calibrated on x so every layer's activations stay O(1) (fp16-safe)
    synthetic_views(...)          512 x 512 range views, including depths on and around the 1.4 m / 54 m mask boundaries,
                                  stored compactly as view_codes and rebuilt by views_from_codes
"""
import numpy as np
import torch
import torch.nn.functional as F

from mobi_amd.realism import BN_EPS, FRD_DEPTH, RANGENET_BLOCKS, RANGENET_DEC, RANGENET_ENC, rangenet_keys

SLOPE = 0.1


def prepare(view, h=64, w=1024):
    """[depth, intensity, pitch, yaw] numpy [4, H, W] -> f32 [5, h, w]: [depth, intensity, x, y, z], -1 where invalid."""
    d, inten, pitch, yaw = (np.asarray(view[i]) for i in range(4))
    depth = (d + 1) / 2 * FRD_DEPTH[1]
    valid = np.logical_and(depth > FRD_DEPTH[0], depth < FRD_DEPTH[1])
    x = np.cos(yaw) * np.cos(pitch) * depth
    y = -np.sin(yaw) * np.cos(pitch) * depth
    z = np.sin(pitch) * depth
    out = np.stack([depth, inten, x, y, z]).astype(np.float64)
    out[:, ~valid] = -1
    t = torch.from_numpy(out).float()
    return F.interpolate(t[:, None], size=(h, w), mode="nearest")[:, 0]


def _bn(x, sd, pre):
    return F.batch_norm(x, sd[f"{pre}.running_mean"], sd[f"{pre}.running_var"], sd[f"{pre}.weight"], sd[f"{pre}.bias"],
                        False, 0.0, BN_EPS)


def _cbl(x, sd, pre_conv, pre_bn, calib, **conv):
    """conv -> BN -> leaky; with `calib`, the BN's running statistics are first set to this batch's (calibration)."""
    y = conv.pop("fn", F.conv2d)(x, sd[f"{pre_conv}.weight"], sd.get(f"{pre_conv}.bias"), **conv)
    if calib:
        sd[f"{pre_bn}.running_mean"] = y.mean((0, 2, 3))
        sd[f"{pre_bn}.running_var"] = y.var((0, 2, 3), unbiased=False)
    return F.leaky_relu(_bn(y, sd, pre_bn), SLOPE)


def _block(x, sd, pre, calib):
    t = _cbl(x, sd, f"{pre}.conv1", f"{pre}.bn1", calib)
    return _cbl(t, sd, f"{pre}.conv2", f"{pre}.bn2", calib, padding=1) + x


def forward(bb, dec, x, calib=False):
    """x f64 [B, 5, 64, 1024] -> f64 [B, 512] (feature index c * 16 + band)."""
    x = _cbl(x, bb, "conv1", "bn1", calib, padding=1)
    skips = []
    for i, nb in enumerate(RANGENET_BLOCKS, 1):
        skips.append(x)
        x = _cbl(x, bb, f"enc{i}.conv", f"enc{i}.bn", calib, stride=(1, 2), padding=1)
        for r in range(nb):
            x = _block(x, bb, f"enc{i}.residual_{r}", calib)
    for i in range(5, 0, -1):
        x = _cbl(x, dec, f"dec{i}.upconv", f"dec{i}.bn", calib, fn=F.conv_transpose2d, stride=(1, 2), padding=(0, 1))
        x = _block(x, dec, f"dec{i}.residual", calib) + skips.pop()
    b, c, h, w = x.shape
    return x.reshape(b, c, 16, h // 16, w).mean((3, 4)).reshape(b, -1)


def seeded_state_dicts(seed, calib_x=None):
    """(backbone, decoder) state dicts, fp64, the reference's keys.  Kaiming-normal convolutions, BN affine near (1, 0);
    with calib_x (f64 [B, 5, 64, 1024]) every BN's running mean / variance is that layer's batch statistics on calib_x."""
    g = torch.Generator().manual_seed(seed)
    bb_keys, dec_keys = rangenet_keys()
    shapes, bn_c = {"conv1.weight": (32, 5, 3, 3)}, {"bn1": 32}
    for i, ((ci, co), nb) in enumerate(zip(RANGENET_ENC, RANGENET_BLOCKS), 1):
        shapes[f"enc{i}.conv.weight"], bn_c[f"enc{i}.bn"] = (co, ci, 3, 3), co
        for r in range(nb):
            shapes[f"enc{i}.residual_{r}.conv1.weight"], bn_c[f"enc{i}.residual_{r}.bn1"] = (ci, co, 1, 1), ci
            shapes[f"enc{i}.residual_{r}.conv2.weight"], bn_c[f"enc{i}.residual_{r}.bn2"] = (co, ci, 3, 3), co
    for i, (ci, co) in zip(range(5, 0, -1), RANGENET_DEC):
        shapes[f"dec{i}.upconv.weight"], shapes[f"dec{i}.upconv.bias"], bn_c[f"dec{i}.bn"] = (ci, co, 1, 4), (co,), co
        shapes[f"dec{i}.residual.conv1.weight"], bn_c[f"dec{i}.residual.bn1"] = (ci, co, 1, 1), ci
        shapes[f"dec{i}.residual.conv2.weight"], bn_c[f"dec{i}.residual.bn2"] = (co, ci, 3, 3), co

    def make(keys):
        sd = {}
        for k in keys:
            if k in shapes:
                s = shapes[k]
                if k.endswith(".bias"):
                    sd[k] = 0.1 * torch.randn(s, generator=g, dtype=torch.float64)
                else:
                    fan_in = s[0] * s[3] if "upconv" in k else s[1] * s[2] * s[3]
                    sd[k] = torch.randn(s, generator=g, dtype=torch.float64) * (2.0 / fan_in) ** 0.5
                continue
            pre, leaf = k.rsplit(".", 1)
            c = bn_c[pre]
            if leaf == "weight":
                sd[k] = 0.75 + 0.5 * torch.rand((c,), generator=g, dtype=torch.float64)
            elif leaf == "bias":
                sd[k] = 0.2 * torch.randn((c,), generator=g, dtype=torch.float64)
            elif leaf == "running_mean":
                sd[k] = torch.zeros((c,), dtype=torch.float64)
            elif leaf == "running_var":
                sd[k] = torch.ones((c,), dtype=torch.float64)
            else:
                sd[k] = torch.tensor(0, dtype=torch.long)
        return sd

    bb, dec = make(bb_keys), make(dec_keys)
    if calib_x is not None:
        with torch.no_grad():
            forward(bb, dec, calib_x, calib=True)
    return bb, dec


def _boundary_depths():
    """Normalised f32 depths on / beside the mask boundaries: 1.4 m has no exact f32 preimage, so its two f32 neighbours
    (one each side in fp64); 54 m is d = 1 exactly, with its neighbours; and the far ends."""
    lo = np.float32(1.4 * 2 / FRD_DEPTH[1] - 1)
    near = [np.nextafter(lo, np.float32(-2)), lo, np.nextafter(lo, np.float32(2))]
    one = np.float32(1.0)
    return np.array(near + [np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2)), -1.0, 1.5, -1.5],
                    np.float32)


RESIZE_ROWS, COL_RUN = 64, 8          # the nearest resize to 64 rows reads every 8th row; codes are constant over 8 columns
DEPTH_SCALE, INT_SCALE = 1024, 128     # normalised depth = code / 1024, intensity = code / 128 (exact in f32)


def view_angles(h=512, w=512):
    """pitch (by row) and yaw (by column) of a synthetic range view, f32-representable, fp64 [h, w] each."""
    rows = np.arange(h, dtype=np.float64)[:, None]
    cols = np.arange(w, dtype=np.float64)[None, :]
    pitch = np.broadcast_to(0.17 - rows * (0.44 / h), (h, w)).astype(np.float32).astype(np.float64)
    yaw = np.broadcast_to(np.pi - cols * (2 * np.pi / w), (h, w)).astype(np.float32).astype(np.float64)
    return pitch, yaw


def view_codes(n, seed, w=512, far=False):
    """Compact random content of n views: int16 depth codes and int8 intensity codes on the rows the resize reads, one code
    per run of COL_RUN columns ([n, 64, w / COL_RUN] each).  `far` shifts the depth distribution (a set that differs clearly)."""
    rng = np.random.default_rng(seed)
    shape = (n, RESIZE_ROWS, w // COL_RUN)
    base = rng.uniform(-0.95, 0.9 if far else 0.2, size=shape) * 0.3
    walk = np.cumsum(rng.normal(0, 0.05, size=shape), axis=2)
    d = np.clip(base + walk + (0.3 if far else -0.3), -1.2, 1.2)
    dcode = np.rint(d * DEPTH_SCALE).astype(np.int16)
    icode = rng.integers(-127, 128, size=shape).astype(np.int8)
    return dcode, icode


def views_from_codes(dcode, icode, h=512, w=512):
    """f64 [n, 4, h, w] of f32-representable values (normalised depth, intensity, pitch, yaw) from view_codes: each code row
    fills the 8 rows from a sampled one, each code a run of columns.  The sampled rows also carry the boundary depths."""
    n, r, b = dcode.shape
    grow = lambda c, scale: np.repeat(np.repeat(c.astype(np.float64) / scale, h // r, axis=1), w // b, axis=2)
    d, inten = grow(dcode, DEPTH_SCALE), grow(icode, INT_SCALE)
    for j, v in enumerate(_boundary_depths()):                 # boundary values on the sampled rows, spread over columns
        d[:, 8 * (j + 1), 2 * j::64] = v
    pitch, yaw = view_angles(h, w)
    out = np.stack([d, inten, np.broadcast_to(pitch, d.shape), np.broadcast_to(yaw, d.shape)], axis=1)
    return out.astype(np.float32).astype(np.float64)


def synthetic_views(n, seed, h=512, w=512, far=False):
    """f64 [n, 4, h, w] synthetic range views (view_codes -> views_from_codes)."""
    return views_from_codes(*view_codes(n, seed, w, far), h=h, w=w)


def frechet_cases():
    """Feature-set pairs for the distance: well-conditioned (d 512, N 2000), rank-deficient (N 100 < d), identical sets,
    and 1-d.  Regenerated from a seed (numpy's PCG64 stream)."""
    rng = np.random.default_rng(5)
    mix_a, mix_b = rng.normal(size=(512, 512)) * 0.05, rng.normal(size=(512, 512)) * 0.05
    well = (rng.normal(size=(2000, 512)) @ mix_a, rng.normal(size=(2000, 512)) @ mix_b + 0.1)
    a_rd, b_rd = rng.normal(size=(100, 512)), rng.normal(size=(100, 512)) * 1.3 + 0.2
    one = (rng.normal(size=(50, 1)), rng.normal(size=(70, 1)) * 2 + 1)
    return {"well": well, "rankdef": (a_rd, b_rd), "same": (a_rd, a_rd.copy()), "one": one}
