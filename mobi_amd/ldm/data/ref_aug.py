"""Reference-image augmentation of the training splits (`ref_aug: true`; reference: ldm/data/nuscenes.py:239-250, the
albumentations 0.4.3 chain HorizontalFlip(p=.5) -> Rotate(limit=30, border_mode=0) -> Blur(p=.5) ->
RandomBrightnessContrast(+-0.3, +-0.3, p=.5) after Resize(224)).

Neither albumentations nor OpenCV is a dependency here: every stage is restated in integer arithmetic from their
documentation / sources (parity with the two libraries is unpinned, like the other cv2 pieces of the data side), so that
the host form (`ref_augment_u8`, numpy) and the device form (`ops.ref_augment`, one launch per batch) agree bit for bit:

  draw    one `RefAugDraw` per item from Python's `random` (albumentations 0.4.3 draws from it; torch seeds it per worker)
  flip    F[y, x] = P0[y, S - 1 - x]
  rotate  OpenCV's 8-bit warpAffine in fixed point: centre (S / 2, S / 2), positive angle counter-clockwise, bilinear on
          a 1/32-pixel grid, constant border 0.  The host inverts the fp64 matrix and rounds it into four int32 tables
          (`warp_tables`); the per-pixel part is integer only
  blur    k x k box filter, BORDER_REFLECT_101, (2 * sum + k^2) // (2 * k^2)   (k odd: no ties)
  b / c   albumentations' uint8 look-up table in float32 (`brightness_contrast_lut`)
  output  `get_tensor_clip()`; for the device folded with the look-up table into one fp32 [3][256] table per sample,
          built by running `get_tensor_clip()` over the table's 256 values (`output_table`)"""
import math
import random
from collections import namedtuple

import numpy as np

# flip / rotate / blur / bc: the stage is on; angle in degrees; k the box side; alpha, beta as albumentations names them
RefAugDraw = namedtuple("RefAugDraw", "flip rotate angle blur k bc alpha beta")
IDENTITY = RefAugDraw(False, False, 0.0, False, 3, False, 1.0, 0.0)

FLAG_FLIP, FLAG_ROTATE = 1, 2            # device form: flags[0] bits; flags[1] = box side (0: no blur)


def draw_ref_aug():
    """The chain's draws in albumentations' order; a stage's parameters are drawn only when that stage is on."""
    flip = random.random() < 0.5
    rotate = random.random() < 0.5
    angle = random.uniform(-30, 30) if rotate else 0.0
    blur = random.random() < 0.5
    k = random.choice([3, 5, 7]) if blur else 3
    bc = random.random() < 0.5
    alpha = 1 + random.uniform(-0.3, 0.3) if bc else 1.0
    beta = random.uniform(-0.3, 0.3) if bc else 0.0
    return RefAugDraw(flip, rotate, angle, blur, k, bc, alpha, beta)


def warp_tables(angle, size=224):
    """int32 [4, size] = (ax, bx, X0, Y0): source position of output pixel (x, y) at 1/1024 pixel,
    X = X0[y] + ax[x], Y = Y0[y] + bx[x] (X0 / Y0 carry the + 16 that rounds to the 1/32-pixel grid)."""
    t = math.radians(angle)
    a, b = math.cos(t), math.sin(t)
    cx = cy = size / 2
    m = [[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]]
    det = m[0][0] * m[1][1] - m[0][1] * m[1][0]                         # cv2.invertAffineTransform
    det = 1.0 / det if det != 0 else 0.0
    d00, d11, d01, d10 = m[1][1] * det, m[0][0] * det, -m[0][1] * det, -m[1][0] * det
    d02, d12 = -d00 * m[0][2] - d01 * m[1][2], -d10 * m[0][2] - d11 * m[1][2]
    n = np.arange(size, dtype=np.float64)
    return np.stack([np.rint(d00 * n * 1024), np.rint(d10 * n * 1024),
                     np.rint((d01 * n + d02) * 1024) + 16, np.rint((d11 * n + d12) * 1024) + 16]).astype(np.int32)


def rotate_u8(img, angle):
    src = np.asarray(img)
    size = src.shape[0]
    ax, bx, x0, y0 = warp_tables(angle, size).astype(np.int64)
    X, Y = (x0[:, None] + ax[None, :]) >> 5, (y0[:, None] + bx[None, :]) >> 5
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    padded = np.zeros((size + 2, size + 2, src.shape[2]), dtype=np.int64)    # S = 0 outside the image
    padded[1:-1, 1:-1] = src

    def tap(yy, xx):
        inside = (yy >= -1) & (yy <= size) & (xx >= -1) & (xx <= size)
        v = padded[np.clip(yy, -1, size) + 1, np.clip(xx, -1, size) + 1]
        return v * inside[..., None]
    w = lambda wy, wx: (wy * wx)[..., None]
    out = (w(32 - fy, 32 - fx) * tap(sy, sx) + w(32 - fy, fx) * tap(sy, sx + 1) +
           w(fy, 32 - fx) * tap(sy + 1, sx) + w(fy, fx) * tap(sy + 1, sx + 1) + 512) >> 10
    return out.astype(np.uint8)


def blur_u8(img, k):
    src = np.asarray(img).astype(np.int64)
    h, w = src.shape[:2]
    r = k // 2
    p = np.pad(src, ((r, r), (r, r), (0, 0)), mode="reflect")
    total = sum(p[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k))
    return ((2 * total + k * k) // (2 * k * k)).astype(np.uint8)


def brightness_contrast_lut(alpha, beta):
    lut = np.arange(256, dtype=np.float32)
    if alpha != 1:
        lut *= np.float32(alpha)
    if beta != 0:
        lut += np.float32(beta * 255)                                    # brightness_by_max
    return np.clip(lut, 0, 255).astype(np.uint8)


def ref_augment_u8(p0, draw):
    """uint8 [S, S, 3] -> uint8 [S, S, 3]: the chain on the resized patch, with the given draws."""
    out = np.asarray(p0)
    if draw.flip:
        out = out[:, ::-1]
    if draw.rotate:
        out = rotate_u8(out, draw.angle)
    if draw.blur:
        out = blur_u8(out, draw.k)
    if draw.bc:
        out = brightness_contrast_lut(draw.alpha, draw.beta)[out]
    return np.ascontiguousarray(out)


def output_table(draw):
    """fp32 [3, 256]: `get_tensor_clip()` of every value the look-up table can give, per channel."""
    from .nuscenes import get_tensor_clip
    lut = brightness_contrast_lut(draw.alpha, draw.beta) if draw.bc else np.arange(256, dtype=np.uint8)
    return get_tensor_clip()(np.repeat(lut[:, None, None], 3, axis=2))[:, :, 0].contiguous()


def device_form(draw, size=224):
    """What `ops.ref_augment` takes for one sample: flags int32 [2], warp int32 [4, size], table fp32 [3, 256]."""
    import torch
    flags = torch.tensor([FLAG_FLIP * bool(draw.flip) + FLAG_ROTATE * bool(draw.rotate), draw.k if draw.blur else 0],
                         dtype=torch.int32)
    warp = torch.from_numpy(warp_tables(draw.angle, size)) if draw.rotate else torch.zeros((4, size), dtype=torch.int32)
    return {"flags": flags, "warp": warp, "table": output_table(draw)}
