"""A helper, not a test: the copy-paste baseline's camera pictures of ONE object (include/mobi_engine.h, mobi_camera_copy_paste)
written independently of the product, and the cases its tests share.

The dilation is scipy's (`grey_dilation`, 5 x 5, constant border -inf: the border never wins); the two resizes go through
`resize_linear_u8`, the integer definition of cv2's 8-bit INTER_LINEAR the project keeps in numpy and the export test already
uses as its yardstick; I, object_ref and recon are numpy fp32 expressions, every operation rounded on its own.  Everything is
integer arithmetic or a single fp32 operation in a fixed order, so given P(patch_pred) every byte is defined: no tolerance."""
import numpy as np
from scipy import ndimage

# name: (frame H, W, patch side, crop (left, top, crop_W, crop_H), steps); a step is (rows, columns, value) written in order
_A = ((20, 70), (40, 130), 0.0)
CASES = {
    "A": (90, 160, 64, (30, 10, 101, 77), (_A,)),                                   # the plain case
    "B": (90, 160, 64, (0, 0, 67, 53), (((0, 40), (0, 50), 0.0),)),                 # dilation at the frame's corner: the border never wins
    "D": (90, 160, 64, (60, 20, 40, 30), (((30, 36), (70, 78), 0.0),)),             # 5 x 7 box: 224 -> 5 x 7 and back; 8 edit pixels survive
    "E": (90, 160, 64, (96, 37, 64, 53), (((60, 90), (120, 160), 0.0),)),           # box and window end with the frame
    "G": (90, 160, 64, (40, 20, 60, 50), (((30, 60), (70, 74), 0.0),)),             # a 4-wide strip: the dilation removes every edit pixel
    "T": (90, 160, 64, (30, 10, 120, 70), (((30, 66), (62, 130), 0.0),)),           # dilated edges on the 64 x 32 tile boundaries
    "O": (90, 160, 64, (60, 20, 40, 30), (((10, 60), (50, 120), 0.0),)),            # the box is larger than the crop window on every side
    "L": (90, 160, 64, (30, 10, 125, 77), (_A, ((5, 6), (150, 151), 0.0), ((45, 46), (85, 86), 1.0))),   # a stray edit pixel, a keep island
    "Q": (90, 160, 64, (30, 10, 101, 77), (_A, ((20, 70), (40, 46), 0.25), ((40, 44), (80, 100), 0.5))),  # fractional m
    "C": (61, 47, 32, (5, 3, 40, 55), (((10, 50), (8, 40), 0.0),)),                 # a frame narrower than a tile
    "F": (40, 300, 32, (8, 2, 288, 36), (((5, 35), (10, 290), 0.0),)),              # a 279-column box: up in x, down in y
}
LAUNCHES = (("A", "B", "D", "E", "G", "T", "O", "L", "Q"), ("C",), ("F",))
EDIT_PIXELS = {"A": 3956, "B": 1824, "D": 8, "E": 1064, "G": 0, "T": 2048, "O": 3036, "L": 3931, "Q": 3956, "C": 1008, "F": 7176}
CLIP_MEAN = np.array([0.48145466, 0.4578275, 0.40821073], dtype=np.float32)
CLIP_STD = np.array([0.26862954, 0.26130258, 0.27577711], dtype=np.float32)


def mask_of(case):
    H, W, _, _, steps = CASES[case]
    mask = np.ones((H, W), dtype=np.float32)
    for (r0, r1), (c0, c1), value in steps:
        mask[r0:r1, c0:c1] = value
    return mask


def dilate(mask):
    return ndimage.grey_dilation(np.asarray(mask, dtype=np.float32), size=(5, 5), mode="constant", cval=-np.inf)


def box_of(mask):
    """(y1, y2, x1, x2) of the pixels with 1 - mask != 0, max EXCLUSIVE as the reference slices; None when that slice is empty."""
    ys, xs = np.nonzero(1 - np.asarray(mask, dtype=np.float32))
    if len(ys) == 0 or ys.max() - ys.min() <= 0 or xs.max() - xs.min() <= 0:
        return None
    return int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())


def object_ref_u8(ref):
    """fp32 [3, 224, 224] CLIP-normalised -> uint8 [224, 224, 3]: a multiply, an add, a multiply in fp32, clamped, truncated."""
    x = np.asarray(ref, dtype=np.float32)
    u = (x * CLIP_STD[:, None, None] + CLIP_MEAN[:, None, None]) * np.float32(255)
    return u.clip(0, 255).astype(np.uint8).transpose(1, 2, 0)


def reference(window_u8, crop, image, mask, ref):
    """window_u8: uint8 [crop_H, crop_W, 3], the launch's own P(patch_pred); image fp32 [3, H, W]; mask fp32 [H, W]; ref fp32
    [3, 224, 224] -> dict(frame, patch_pred, object_pred (None with an empty box), object_ref, pred, m, box)."""
    from ldm.data.nuscenes import resize_linear_u8
    left, top, cw, ch = crop
    mask = np.asarray(mask, dtype=np.float32)
    object_ref = object_ref_u8(ref)
    pred = np.zeros(mask.shape + (3,), dtype=np.uint8)
    pred[top:top + ch, left:left + cw] = window_u8
    box = box_of(mask)
    object_pred = None
    if box is not None:
        y1, y2, x1, x2 = box
        pred[y1:y2, x1:x2] = resize_linear_u8(object_ref, y2 - y1, x2 - x1)
        object_pred = resize_linear_u8(pred[y1:y2, x1:x2], 224, 224)
    m = dilate(mask)[..., None]
    x = np.asarray(image, dtype=np.float32).transpose(1, 2, 0)
    I = ((x + np.float32(1)) / np.float32(2) * np.float32(255)).clip(0, 255).astype(np.uint8).astype(np.float32)
    recon = m * I + (np.float32(1) - m) * pred.astype(np.float32)
    assert recon.dtype == np.float32
    frame = np.clip(np.rint(recon), 0, 255).astype(np.uint8)
    return dict(frame=frame, patch_pred=frame[top:top + ch, left:left + cw], object_pred=object_pred, object_ref=object_ref, pred=pred,
                m=m[..., 0], box=box, I=I.astype(np.uint8))
