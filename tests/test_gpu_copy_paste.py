"""GPU: `mobi_camera_copy_paste` / `du.export_camera_batch(copy_paste=True)` -- the export launch in copy-paste mode -- against the
independent definition of tests/copy_paste_ref.py, byte for byte.

The only floating-point sum whose order is free in the export is the blur, and this mode has none: the paste and the two resizes
are integer arithmetic, the dilation is a maximum, and I, object_ref and recon are single fp32 operations in a fixed order.  So
given the launch's own P(patch_pred) -- read back through the patch_gt picture of a launch that is handed patch_pred in patch_gt's
place -- every byte of every picture is defined, Q's fractional m included, and no byte is excused."""
import numpy as np
import pytest
import torch

from oracle import weights as W
from tests import copy_paste_ref as cr

pytestmark = pytest.mark.gpu


def _inputs(names):
    """As tests/test_gpu_camera_export.py builds them, seeded per case: a case's inputs are the same in any batch."""
    H, Wd, ps = cr.CASES[names[0]][:3]
    g = lambda what, shape: torch.clamp(W.synth_input(f"cp.{what}", shape) * 0.5, -1, 1)
    per = lambda what, shape, fn=g: torch.stack([fn(f"{what}.{k}", shape) for k in names])
    return dict(patch_pred=per("pred", (3, ps, ps)), patch_gt=per("gt", (3, ps, ps)), image=per("image", (3, H, Wd)),
                ref_image=per("ref", (3, 224, 224), lambda what, shape: W.synth_input(f"cp.{what}", shape)),
                mask=torch.from_numpy(np.stack([cr.mask_of(k) for k in names])), crop=[cr.CASES[k][3] for k in names])


def _cuda(d):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


@pytest.fixture(scope="module")
def runs():
    """Every launch once: the export of case A first (before any copy-paste launch), then per frame size the copy-paste launch with
    and without frames and the two probes, and the helper's pictures from the probe."""
    from mobi_amd.ldm.data import utils as du
    out = {"export_A_before": du.export_camera_batch(**_cuda(_inputs(("A",))), frames=True)[0]}
    for names in cr.LAUNCHES:
        d = _inputs(names)
        dev = _cuda(d)
        probe_args = {**dev, "patch_gt": dev["patch_pred"]}
        full = du.export_camera_batch(**dev, frames=True, copy_paste=True)
        crops_only = du.export_camera_batch(**dev, frames=False, copy_paste=True)
        probe = du.export_camera_batch(**probe_args, frames=False, copy_paste=True)
        probe_export = du.export_camera_batch(**probe_args, frames=False)
        for i, k in enumerate(names):
            window = probe[i]["patch_gt"]
            out[k] = dict(full=full[i], crops=crops_only[i], probe=window, probe_export=probe_export[i]["patch_gt"], crop=d["crop"][i],
                          want=cr.reference(window, d["crop"][i], d["image"][i].numpy(), d["mask"][i].numpy(), d["ref_image"][i].numpy()))
    out["export_A_after"] = du.export_camera_batch(**_cuda(_inputs(("A",))), frames=True)[0]
    return out


@pytest.mark.parametrize("case", list(cr.CASES))
def test_probe_is_the_export_launch_s_own_patch(runs, case):
    r = runs[case]
    assert r["probe"].shape == (r["crop"][3], r["crop"][2], 3) and r["probe"].any()
    assert np.array_equal(r["probe"], r["probe_export"])


@pytest.mark.parametrize("case", list(cr.CASES))
def test_pictures_equal_the_definition_byte_for_byte(runs, case):
    r = runs[case]
    want, got = r["want"], r["full"]
    assert want["box"] is not None and int((want["m"] != 1).sum()) == cr.EDIT_PIXELS[case]
    for name in ("object_ref", "object_pred", "frame", "patch_pred"):
        diff = got[name] != want[name]
        print(f"{case} {name}: {int(diff.sum())} of {diff.size} bytes differ")
        assert not diff.any(), (case, name, int(diff.sum()))
    left, top, cw, ch = r["crop"]
    gt = torch.nn.functional.interpolate(_inputs((case,))["patch_gt"], (ch, cw), mode="bilinear")[0].numpy().transpose(1, 2, 0)
    off = np.abs(got["patch_gt"].astype(np.int32) - (((gt + 1.0) / 2.0) * 255).astype(np.uint8))     # as in the export: its bound
    assert off.max() <= 1 and (off != 0).mean() < 5e-3
    if case == "G":                                                                 # no edit pixel survives: the frame is I,
        assert np.array_equal(got["frame"], want["I"])                              # object_pred still the reference, twice resized
    if case == "O":                                                                 # pasted outside the crop window too
        y1, y2, x1, x2 = want["box"]
        outside = np.ones(want["m"].shape, dtype=bool)
        outside[top:top + ch, left:left + cw] = False
        assert (want["frame"] != want["I"])[outside].any() and y1 < top and x1 < left
    if case == "Q":
        assert int(((want["m"] != 0) & (want["m"] != 1)).sum()) == 468


@pytest.mark.parametrize("case", list(cr.CASES))
def test_crops_are_the_frame_window_with_and_without_frames(runs, case):
    r = runs[case]
    left, top, cw, ch = r["crop"]
    assert np.array_equal(r["full"]["patch_pred"], r["full"]["frame"][top:top + ch, left:left + cw])
    assert "frame" not in r["crops"] and set(r["full"]) == set(r["crops"]) | {"frame"}
    for name, pic in r["crops"].items():
        assert np.array_equal(pic, r["full"][name]), name


def test_empty_box_is_reported_and_spares_the_others(runs):
    """A one-row edit region in a batch of four: status 1, nothing pasted, object_pred not written; the rest is whole."""
    from mobi_amd.ldm.data import utils as du
    names = ("A", "B", "D", "E")
    d = _inputs(names)
    d["mask"][2] = 1
    d["mask"][2, 33, 70:78] = 0
    with pytest.raises(ValueError, match=r"object\(s\) \[2\]") as e:
        du.export_camera_batch(**_cuda(d), frames=True, copy_paste=True)
    for i, k in enumerate(names):
        if i != 2:
            for name, pic in runs[k]["full"].items():
                assert np.array_equal(e.value.pictures[i][name], pic), (k, name)
    want = cr.reference(runs["D"]["probe"], d["crop"][2], d["image"][2].numpy(), d["mask"][2].numpy(), d["ref_image"][2].numpy())
    assert want["box"] is None and want["object_pred"] is None
    for name in ("frame", "patch_pred", "object_ref"):
        assert np.array_equal(e.value.pictures[2][name], want[name]), name
    assert np.array_equal(e.value.pictures[2]["patch_gt"], runs["D"]["full"]["patch_gt"])


def test_launches_do_not_depend_on_the_batch():
    from mobi_amd import ops
    from mobi_amd.ldm.data import utils as du
    counts = []
    for n in (1, 5):
        dev = _cuda(_inputs(("A",) * n))
        sink = []
        ops.set_profiler(sink)
        try:
            du.export_camera_batch(**dev, frames=True, copy_paste=True)
        finally:
            ops.set_profiler(None)
        kinds = [s[0] for s in sink]
        counts.append(kinds.count("camera_export"))
        assert kinds.count("camera_export_d2h") == 1 and len(kinds) == counts[-1] + 1
        assert all(s[5].endswith(".cp") for s in sink if s[0] == "camera_export")
    assert counts[0] == counts[1] <= 2


def test_export_is_unchanged_beside_the_new_mode(runs):
    """`mobi_camera_export` on case A: the same bytes before and after the copy-paste launches, its own definition of object_pred
    (the patch on the box, not the reference), and a frame that is not the baseline's."""
    from ldm.data.nuscenes import resize_linear_u8
    before, after, r = runs["export_A_before"], runs["export_A_after"], runs["A"]
    for name, pic in before.items():
        assert np.array_equal(pic, after[name]), name
    left, top, cw, ch = r["crop"]
    y1, y2, x1, x2 = r["want"]["box"]
    pred = np.zeros(before["frame"].shape, dtype=np.uint8)
    pred[top:top + ch, left:left + cw] = r["probe"]
    assert np.array_equal(before["object_pred"], resize_linear_u8(pred[y1:y2, x1:x2], 224, 224))
    assert np.array_equal(before["object_ref"], r["full"]["object_ref"]) and np.array_equal(before["patch_gt"], r["full"]["patch_gt"])
    assert not np.array_equal(before["frame"], r["full"]["frame"]) and not np.array_equal(before["object_pred"], r["full"]["object_pred"])


def test_taps_may_be_absent_and_bad_arguments_are_refused():
    from mobi_amd import _lib, ops
    d = _inputs(("A",))
    dev = _cuda(d)
    args = (dev["patch_pred"], dev["patch_gt"], dev["ref_image"], dev["image"], dev["mask"])
    out, layout = ops.camera_export(*args, d["crop"], None, copy_paste=True)
    again, _ = ops.camera_export(*args, d["crop"], torch.full((15,), float("nan"), device="cuda"), copy_paste=True)
    for name, (o, (h, w, _)) in layout["objects"][0].items():                       # taps are ignored
        assert torch.equal(out[o:o + h * w * 3], again[o:o + h * w * 3]), name
    with pytest.raises(ValueError):
        ops.camera_export(*args, [(100, 10, 101, 77)], None, copy_paste=True)
    with pytest.raises(_lib.EngineError, match="unsupported"):
        ops.camera_export(args[0], args[1], dev["ref_image"][:, :, :200, :200].contiguous(), args[3], args[4], d["crop"], None,
                          copy_paste=True)
