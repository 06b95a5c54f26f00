"""GPU: `mobi_camera_export` / `du.export_camera_batch` -- the test bench's camera pictures of a batch in one launch -- against the
oracle's paste-back (cv2 is absent: parity with OpenCV is unpinned), against the per-sample engine path it replaces, and against the
integer definition of cv2.resize the project keeps in numpy.

recon is a uint8 rounding of a fp32 blend.  Two fp32 evaluations of that blend agree to 2e-3 on the 0..255 scale (the existing blend
tolerance), so a byte may differ from np.rint(reference) only where the reference lies within 2e-3 of a half-integer, or where the
uint8 prediction under it differs (F.interpolate on the CPU may fuse its multiply-adds: within 1 LSB on at most 0.5 % of bytes, the
existing bound).  Such excused bytes are within 2 and are under 1 % of a picture.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import postprocess as op
from oracle import weights as W

pytestmark = pytest.mark.gpu

# name: (frame H, W, patch side, crop (left, top, crop_W, crop_H), zero region of the mask rows, columns)
CASES = {
    "A": (90, 160, 64, (30, 10, 101, 77), (20, 70), (40, 130)),            # the existing paste-back test's case
    "B": (90, 160, 64, (0, 0, 67, 53), (0, 40), (0, 50)),                  # frame corner: the reflected border inside the window
    "D": (90, 160, 64, (60, 20, 40, 30), (30, 36), (70, 78)),              # 6 x 8 edit pixels: object_pred upscales 5 x 7
    "E": (90, 160, 64, (96, 37, 64, 53), (60, 90), (120, 160)),            # the far corner: window and box end with the frame
    "C": (61, 47, 32, (5, 3, 40, 55), (10, 50), (8, 40)),                  # a frame narrower than a tile
    "F": (40, 300, 32, (8, 2, 288, 36), (5, 35), (10, 290)),               # a 279-column box: object_pred DOWNscales in x
}
LAUNCHES = (("A", "B", "D", "E"), ("C",), ("F",))


def _inputs(names):
    H, Wd, ps = CASES[names[0]][:3]
    n = len(names)
    tag = "".join(names)
    g = lambda what, shape: torch.clamp(W.synth_input(f"ce.{what}.{tag}", shape) * 0.5, -1, 1)
    d = dict(patch_pred=g("pred", (n, 3, ps, ps)), patch_gt=g("gt", (n, 3, ps, ps)), image=g("image", (n, 3, H, Wd)),
             ref_image=W.synth_input(f"ce.ref.{tag}", (n, 3, 224, 224)), mask=torch.ones(n, H, Wd), crop=[CASES[k][3] for k in names])
    for i, k in enumerate(names):
        (r0, r1), (c0, c1) = CASES[k][4:]
        d["mask"][i, r0:r1, c0:c1] = 0
    return d


@pytest.fixture(scope="module")
def runs():
    """Every launch once: the export with and without frames, the export with patch_pred in patch_gt's place (its patch_gt
    picture is then the kernel's own `pred` on the crop window), the per-sample engine path and the oracle."""
    from mobi_amd.ldm.data import utils as du
    out = {}
    for names in LAUNCHES:
        d = _inputs(names)
        dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
        full = du.export_camera_batch(**dev, frames=True)
        crops_only = du.export_camera_batch(**dev, frames=False)
        pred_probe = du.export_camera_batch(**{**dev, "patch_gt": dev["patch_pred"]}, frames=False)
        for i, k in enumerate(names):
            ref_recon, ref_pred = op.paste_camera_patch(d["patch_pred"][[i]], d["image"][i], d["mask"][i], d["crop"][i])
            recon, pred = du.paste_camera_patch(patch_pred=dev["patch_pred"][[i]], image=dev["image"][i], mask=dev["mask"][i],
                                                crop=d["crop"][i])
            out[k] = dict(inputs={key: (v[i] if not isinstance(v, list) else v[i]) for key, v in d.items()}, full=full[i],
                          crops=crops_only[i], probe=pred_probe[i]["patch_gt"],
                          oracle=(ref_recon[..., ::-1], ref_pred[..., ::-1]),                       # BGR -> RGB
                          engine=(recon.cpu().numpy()[..., ::-1], pred.cpu().numpy()[..., ::-1]))
    return out


def _window(arr, crop):
    left, top, cw, ch = crop
    return arr[top:top + ch, left:left + cw]


def _one_lsb(got, want, what):
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"{what}: max {diff.max()}, differing {(diff != 0).mean():.5f}")
    assert diff.max() <= 1 and (diff != 0).mean() < 5e-3, what


def _recon_rule(got, ref_recon, pred_differs, what):
    want = np.clip(np.rint(ref_recon), 0, 255).astype(np.int32)
    near_half = np.abs(ref_recon - np.floor(ref_recon) - 0.5) <= 2e-3
    excused = near_half | pred_differs
    diff = np.abs(got.astype(np.int32) - want)
    print(f"{what}: differing {(diff != 0).mean():.5f}, excused {excused.mean():.5f}, max {diff.max()}")
    assert not (diff != 0)[~excused].any(), what
    assert diff.max() <= 2 and excused.mean() < 1e-2, what


@pytest.mark.parametrize("case", list(CASES))
def test_against_the_oracle(runs, case):
    r = runs[case]
    crop = r["inputs"]["crop"]
    ref_recon, ref_pred = r["oracle"]
    _one_lsb(r["probe"], _window(ref_pred, crop), "pred")
    pred_mine = np.zeros_like(ref_pred)
    _window(pred_mine, crop)[...] = r["probe"]
    _recon_rule(r["full"]["frame"], ref_recon, pred_mine != ref_pred, "recon")
    gt = F.interpolate(r["inputs"]["patch_gt"][None], (crop[3], crop[2]), mode="bilinear")[0].numpy().transpose(1, 2, 0)
    _one_lsb(r["full"]["patch_gt"], (((gt + 1.0) / 2.0) * 255).astype(np.uint8), "patch_gt")


@pytest.mark.parametrize("case", list(CASES))
def test_against_the_per_sample_engine_path(runs, case):
    r = runs[case]
    crop = r["inputs"]["crop"]
    recon, pred = r["engine"]
    _one_lsb(r["probe"], _window(pred, crop), "pred")
    pred_mine = np.zeros_like(pred)
    _window(pred_mine, crop)[...] = r["probe"]
    _recon_rule(r["full"]["frame"], recon, pred_mine != pred, "recon")


@pytest.mark.parametrize("case", list(CASES))
def test_crops_are_the_frame_window_with_and_without_frames(runs, case):
    r = runs[case]
    assert np.array_equal(r["full"]["patch_pred"], _window(r["full"]["frame"], r["inputs"]["crop"]))
    assert "frame" not in r["crops"] and set(r["full"]) == set(r["crops"]) | {"frame"}
    for name, pic in r["crops"].items():
        assert np.array_equal(pic, r["full"][name]), name


@pytest.mark.parametrize("case", list(CASES))
def test_object_pictures_bit_for_bit(runs, case):
    """object_pred: integer arithmetic on the kernel's own pred (read back through the probe), the box from numpy on the mask,
    its last row and column excluded as the reference slices; asserted on the upscaling case (D: 5 x 7), a downscaling one (F: 279
    columns) and the edge-touching boxes (B, E) among the rest.  object_ref: the torch-CPU fp32 expression."""
    from ldm.data.nuscenes import resize_linear_u8
    from mobi_amd.ldm.data.utils import un_norm_clip
    r = runs[case]
    mask, crop = r["inputs"]["mask"].numpy(), r["inputs"]["crop"]
    ys, xs = np.nonzero(1 - mask)
    y1, y2, x1, x2 = ys.min(), ys.max(), xs.min(), xs.max()
    if case == "D":
        assert (y2 - y1, x2 - x1) == (5, 7)
    if case == "F":
        assert x2 - x1 > 224
    pred = np.zeros(mask.shape + (3,), dtype=np.uint8)
    _window(pred, crop)[...] = r["probe"]
    assert np.array_equal(r["full"]["object_pred"], resize_linear_u8(pred[y1:y2, x1:x2], 224, 224))
    ref = un_norm_clip(r["inputs"]["ref_image"][None], size=(224, 224))[0]
    want = (ref * 255).clamp(0, 255).numpy().transpose(1, 2, 0).astype(np.uint8)
    assert np.array_equal(r["full"]["object_ref"], want)


def test_empty_box_is_reported_and_spares_the_others(runs):
    """A one-row edit region: the reference's exclusive slice is empty.  ValueError names the object; the rest of the batch is whole."""
    from mobi_amd.ldm.data import utils as du
    names = ("A", "B", "D", "E")
    d = _inputs(names)
    d["mask"][2] = 1
    d["mask"][2, 33, 70:78] = 0
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    with pytest.raises(ValueError, match=r"object\(s\) \[2\]") as e:
        du.export_camera_batch(**dev, frames=True)
    for i, k in enumerate(names):
        for name, pic in runs[k]["full"].items():
            if i != 2:
                assert np.array_equal(e.value.pictures[i][name], pic), (k, name)


def test_launches_do_not_depend_on_the_batch():
    from mobi_amd import ops
    from mobi_amd.ldm.data import utils as du
    counts = []
    for n in (1, 5):
        d = _inputs(("A",) * n)
        dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
        sink = []
        ops.set_profiler(sink)
        try:
            du.export_camera_batch(**dev, frames=True)
        finally:
            ops.set_profiler(None)
        kinds = [s[0] for s in sink]
        counts.append(kinds.count("camera_export"))
        assert kinds.count("camera_export_d2h") == 1 and len(kinds) == counts[-1] + 1
    assert counts[0] == counts[1] <= 2


def test_bad_arguments_are_refused_before_the_launch():
    from mobi_amd import _lib, ops
    d = _inputs(("A",))
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    taps = torch.ones(15, device="cuda") / 15
    with pytest.raises(ValueError):
        ops.camera_export(dev["patch_pred"], dev["patch_gt"], dev["ref_image"], dev["image"], dev["mask"], [(100, 10, 101, 77)], taps)
    with pytest.raises(_lib.EngineError, match="unsupported"):
        ops.camera_export(dev["patch_pred"], dev["patch_gt"], dev["ref_image"][:, :, :200, :200].contiguous(), dev["image"],
                          dev["mask"], d["crop"], taps)
