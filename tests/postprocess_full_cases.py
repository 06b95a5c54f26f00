"""Inputs of the post-processing checks at the product's geometry (configs/mobi_nusc_512.yaml: 512 x 512 range views,
a 32 x 1096 sweep, width_crop in {64, 128, 256, 512}), shared by tests/golden/make_golden_postprocess_full.py (which
ran the reference on them) and by the tests (which run the oracle / the engine).  Nothing large is stored: every array
comes from `oracle.weights.synth_input` (counter-based, version independent)."""
import numpy as np
import torch

from oracle import weights as W

B, HC, WC, H0, W0, POOL_H = 4, 512, 512, 32, 1096, 32
WIDTH_CROP = [64, 128, 256, 512]
# the tiled 3 x 1096 coordinate the dataset hands over; 1 and 3 wrap around the sweep (996 + 128, 700 + 512 > 1096)
CROP_LEFT = [1096 + 37, 2 * 1096 - 100, 3 * 1096 - 512 - 1, 700]


def _u(name, shape):
    return torch.clamp(W.synth_input(name, shape) * 0.6, -1, 1)


def window_columns(i):
    """columns of the sweep that sample i's crop window covers, in window order"""
    return (CROP_LEFT[i] % W0 + np.arange(WIDTH_CROP[i])) % W0


def angles():
    yaw = np.tile(np.linspace(np.pi, -np.pi, W0, dtype=np.float32)[None], (H0, 1))
    pitch = np.tile(np.linspace(0.18, -0.5, H0, dtype=np.float32)[:, None], (1, W0))
    return np.stack([pitch] * B), np.stack([yaw] * B)


def paste_inputs():
    pitch, yaw = angles()
    return dict(depth=_u("ppf.depth", (B, 1, HC, WC)), inten=_u("ppf.int", (B, 1, HC, WC)),
                d_orig=_u("ppf.d0", (B, H0, W0)), i_orig=_u("ppf.i0", (B, H0, W0)),
                gt_mask=(W.synth_input("ppf.gt", (B, H0, W0)) > 1.2).numpy(), pitch=pitch, yaw=yaw,
                crop_left=torch.tensor(CROP_LEFT), width_crop=torch.tensor(WIDTH_CROP))


def _cells_to_pixels(cells, filled):
    """[POOL_H, wc] bool cells -> [HC, WC] 0/1 floats: the whole pooling window set, or ONE pixel of it at a position
    that changes from cell to cell (the max over the window must find it)."""
    wc = cells.shape[1]
    kh, kw = HC // POOL_H, WC // wc
    if filled:
        return np.kron(cells, np.ones((kh, kw))).astype(np.float32)
    out = np.zeros((HC, WC), dtype=np.float32)
    ys, xs = np.nonzero(cells)
    out[ys * kh + (ys * 7 + xs * 3) % kh, xs * kw + (ys + xs * 5) % kw] = 1.0
    return out


def metric_inputs():
    """B = 4 views with the four widths.  Instance masks: 0 -> an ODD number of selected cells, 1 -> an EVEN number
    (the lower median), 2 -> none (NaN, dropped), 3 -> all ones at width_crop = 512 (32 x 512 = 16384 cells, the whole
    sort space of the kernel).  Edit region (1 - range_mask): a filled block of cells plus scattered single pixels."""
    inst, rmask = [], []
    for i, wc in enumerate(WIDTH_CROP):
        cells = W.synth_input(f"ppf.m.inst{i}", (POOL_H, wc)).numpy() > 0.8
        if i < 2 and int(cells.sum()) % 2 != (1 - i):
            cells[0, 0] = ~cells[0, 0]
        m = _cells_to_pixels(cells, filled=False)
        if i == 2:
            m[:] = 0
        if i == 3:
            m[:] = 1
        inst.append(m)
        block = np.zeros((POOL_H, wc), dtype=bool)
        block[6:26, wc // 4:3 * wc // 4] = True
        sparse = (W.synth_input(f"ppf.m.box{i}", (POOL_H, wc)).numpy() > 1.5) & ~block
        box = np.maximum(_cells_to_pixels(block, filled=True), _cells_to_pixels(sparse, filled=False))
        rmask.append(1.0 - box)
    t = lambda a: torch.from_numpy(np.stack(a))[:, None]
    return dict(sample=_u("ppf.m.sample", (B, 2, HC, WC)), rec=_u("ppf.m.rec", (B, 2, HC, WC)),
                data_in=_u("ppf.m.in", (B, 2, HC, WC)), inst=t(inst), rmask=t(rmask),
                min_d=torch.tensor([-0.6, -0.9, 0.1, -0.3]), max_d=torch.tensor([0.3, -0.2, 0.95, 0.5]),
                width_crop=torch.tensor(WIDTH_CROP))


# ---- camera side: a 512 x 512 patch pasted into a 900 x 1600 frame ----------------------------------------------------
FRAME_H, FRAME_W = 900, 1600
# (left, top, crop_W, crop_H): odd sizes inside the frame; hanging over the right and the bottom edge; negative top and
# left; wholly off-frame (nothing may be written)
PASTE_CROPS = [(301, 77, 701, 433), (1250, 600, 613, 517), (-97, -55, 555, 333), (1700, 100, 301, 201)]


def camera_patch():
    return torch.clamp(W.synth_input("ppf.patch", (3, 512, 512)) * 0.4, -1, 1)


def frame_pattern():
    y, x, c = np.meshgrid(np.arange(FRAME_H), np.arange(FRAME_W), np.arange(3), indexing="ij")
    return ((y * 7 + x * 13 + c * 101) % 251).astype(np.uint8)


def _bilinear_axis(n_src, n_dst):
    """source taps of F.interpolate(bilinear, align_corners=False) along one axis: the fp32 source coordinate
    scale * (dst + 0.5) - 0.5 clamped at 0 (the tensor's own type, as torch computes it), -> (i0, i1, weight of i1)."""
    s = np.float32(n_src) / np.float32(n_dst)
    f = np.maximum(s * (np.arange(n_dst, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = f.astype(np.int64)
    return i0, i0 + (i0 < n_src - 1), (f - i0.astype(np.float32)).astype(np.float64)


def paste_patch_f64(patch, crop_h, crop_w, eps=1e-3):
    """The harness's resized uint8 patch with the four-tap expression and (v + 1) / 2 * 255 evaluated in FLOAT64:
    (bytes uint8 [crop_h, crop_w, 3] BGR, undecidable bool [crop_h, crop_w, 3]).  A byte is undecidable when the float64
    value lies within `eps` of an integer: an fp32 evaluation (error < 1e-4 on the 0..255 scale) may then truncate to the
    neighbouring byte; every other byte is determined."""
    p = np.asarray(patch, dtype=np.float64)
    y0, y1, ly = _bilinear_axis(p.shape[1], crop_h)
    x0, x1, lx = _bilinear_axis(p.shape[2], crop_w)
    ly, lx = ly[None, :, None], lx[None, None, :]
    g = lambda ys, xs: p[:, ys][:, :, xs]
    v = (1 - ly) * ((1 - lx) * g(y0, x0) + lx * g(y0, x1)) + ly * ((1 - lx) * g(y1, x0) + lx * g(y1, x1))
    u = np.clip((v + 1.0) / 2.0 * 255.0, 0.0, 255.0).transpose(1, 2, 0)[..., ::-1]
    return np.floor(u).astype(np.uint8), np.abs(u - np.round(u)) < eps
