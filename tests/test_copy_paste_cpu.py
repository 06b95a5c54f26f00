"""CPU: the copy-paste baseline's host side -- `du.copy_paste_camera_patch` (the numpy definition) against the independent helper
byte for byte on every case of the shared table, `mobi_camera_copy_paste`'s refusals (host checks: no launch), the command
`python -m mobi_amd.copy_paste`, the scripts/inference_test_bench.py shim and the overlay file jobs."""
import ctypes as C
import os
import runpy
import sys

import numpy as np
import pytest

from tests import copy_paste_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from mobi_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _dilate_by_hand(mask):
    H, W = mask.shape
    out = np.empty_like(mask)
    for y in range(H):
        for x in range(W):
            out[y, x] = mask[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3].max()
    return out


def test_the_table_is_what_it_says():
    """Every box is non-empty, the edit pixels left by the dilation are the listed counts, only Q has fractional m, and scipy's
    dilation is the maximum over the in-frame 5 x 5 neighbourhood."""
    assert set(cr.CASES) == set(cr.EDIT_PIXELS) == {k for names in cr.LAUNCHES for k in names} and len(cr.CASES) == 11
    for case in cr.CASES:
        mask = cr.mask_of(case)
        m = cr.dilate(mask)
        assert cr.box_of(mask) is not None, case
        assert int((m != 1).sum()) == cr.EDIT_PIXELS[case], case
        fractional = int(((m != 0) & (m != 1)).sum())
        assert fractional == (468 if case == "Q" else 0), (case, fractional)
        assert np.array_equal(m, _dilate_by_hand(mask)), case
    y1, y2, x1, x2 = cr.box_of(cr.mask_of("D"))
    assert (y2 - y1, x2 - x1) == (5, 7)
    y1, y2, x1, x2 = cr.box_of(cr.mask_of("F"))
    assert x2 - x1 == 279 and y2 - y1 < 224
    left, top, cw, ch = cr.CASES["O"][3]
    y1, y2, x1, x2 = cr.box_of(cr.mask_of("O"))
    assert y1 < top and y2 > top + ch and x1 < left and x2 > left + cw


@pytest.mark.parametrize("case", list(cr.CASES))
def test_numpy_definition_equals_the_helper(case):
    from mobi_amd.ldm.data import utils as du
    H, W, _, crop, _ = cr.CASES[case]
    left, top, cw, ch = crop
    rng = np.random.default_rng(sorted(cr.CASES).index(case))
    window = rng.integers(0, 256, (ch, cw, 3), dtype=np.uint8)                      # synthetic P(patch_pred)
    image = rng.uniform(-1.1, 1.1, (3, H, W)).astype(np.float32)
    ref = rng.normal(0, 1.2, (3, 224, 224)).astype(np.float32)
    mask = cr.mask_of(case)
    want = cr.reference(window, crop, image, mask, ref)
    pred_u8 = np.zeros((H, W, 3), dtype=np.uint8)
    pred_u8[top:top + ch, left:left + cw] = window
    recon, pred, box = du.copy_paste_camera_patch(pred_u8, image, mask, want["object_ref"])
    assert box == want["box"]
    assert recon.dtype == np.uint8 and np.array_equal(recon, want["frame"])
    assert np.array_equal(pred, want["pred"])
    if case == "G":                                                                 # every edit pixel is dilated away
        assert np.array_equal(recon, want["I"])
    else:
        assert not np.array_equal(recon, want["I"])
    assert np.array_equal(pred_u8[top:top + ch, left:left + cw], window)            # the argument is not written


def test_numpy_definition_with_an_empty_box():
    from mobi_amd.ldm.data import utils as du
    rng = np.random.default_rng(3)
    mask = np.ones((30, 40), dtype=np.float32)
    mask[12, 5:30] = 0                                                              # one row: the exclusive slice is empty
    pred_u8 = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)
    image = rng.uniform(-1, 1, (3, 30, 40)).astype(np.float32)
    recon, pred, box = du.copy_paste_camera_patch(pred_u8, image, mask, np.zeros((224, 224, 3), np.uint8))
    assert box is None and np.array_equal(pred, pred_u8)
    assert np.array_equal(recon, du.frame_u8(image))                                # and one row does not survive the dilation
    assert du.copy_paste_camera_patch(pred_u8, image, np.ones((30, 40), np.float32), np.zeros((224, 224, 3), np.uint8))[2] is None


def test_copy_paste_validates_before_any_launch(lib):
    """No GPU here: every call must return on the host, with `mobi_camera_export`'s answer -- except that `taps` may be NULL."""
    from mobi_amd import _lib, ops
    assert lib.mobi_struct_size(31) == C.sizeof(_lib.CameraExportParams)
    crops = [(30, 10, 101, 77), (0, 0, 67, 53)]
    lay = ops.camera_export_layout(crops, 90, 160, True)

    def call(fn, crops=crops, out_bytes=lay["bytes"], shift=0, ref=224, frames=1, null=None, batch=None, status=lay["status"]):
        n = len(crops)
        crop = (C.c_int32 * (4 * n))(*[v for c in crops for v in c])
        offs = (C.c_int64 * (5 * n))(*[o[name][0] + shift for o in lay["objects"][:n] for name in ops.CAMERA_EXPORT_PICTURES])
        p = _lib.CameraExportParams()
        for name in ("patch_pred", "patch_gt", "ref", "image", "mask", "taps", "box_ws", "out"):
            setattr(p, name, 4096)
        p.crop, p.offsets = C.cast(crop, C.c_void_p), C.cast(offs, C.c_void_p)
        p.out_bytes, p.status_offset = out_bytes, status
        p.batch, p.hs, p.ws, p.ref_h, p.ref_w, p.H, p.W, p.frames = (n if batch is None else batch), 64, 64, ref, ref, 90, 160, frames
        if null:
            setattr(p, null, None)
        return fn(C.byref(p), None)

    refusals = [dict(null=name) for name in ("patch_pred", "patch_gt", "ref", "image", "mask", "crop", "offsets", "box_ws", "out")]
    refusals += [dict(crops=[c]) for c in [(100, 10, 101, 77), (0, 40, 10, 51), (-1, 0, 5, 5), (0, 0, 0, 5)]]
    refusals += [dict(shift=2), dict(status=lay["status"] + 2, out_bytes=lay["bytes"] + 4), dict(out_bytes=lay["bytes"] - 8),
                 dict(out_bytes=lay["objects"][1]["object_ref"][0] + 100), dict(shift=-4), dict(ref=200), dict(batch=33), dict(batch=0)]
    assert lib.mobi_camera_copy_paste(None, None) == -1
    for kw in refusals:
        got = call(lib.mobi_camera_copy_paste, **kw)
        assert got < 0 and got == call(lib.mobi_camera_export, **kw), kw
    assert call(lib.mobi_camera_export, null="taps") == -1
    for kw in refusals[9:]:                                                         # `taps` is ignored: NULL changes no answer
        assert call(lib.mobi_camera_copy_paste, null="taps", **kw) == call(lib.mobi_camera_export, **kw), kw


def test_command_forces_one_step_and_refuses_dpm(monkeypatch):
    from mobi_amd import bench_tree as bt
    from mobi_amd import copy_paste as cp
    from mobi_amd import test_bench as tb
    flags = lambda ap: {s for a in ap._actions for s in a.option_strings}
    assert "--copy-paste" not in flags(tb.build_parser()) | flags(bt.build_parser())
    assert flags(bt.build_parser()) - flags(tb.build_parser()) == {"--no_overlays"}
    opt = cp.parse(["--config", "c.yaml", "--ddim_steps", "7", "--plms", "--scale", "5", "--save_samples", "a.b=3"])
    assert opt.copy_paste is True and opt.ddim_steps == 1 and opt.plms and opt.scale == 5.0 and opt.overrides == ["a.b=3"]
    assert cp.parse([]).ddim_steps == 1
    with pytest.raises(SystemExit, match="--dpm"):
        cp.parse(["--dpm"])
    with pytest.raises(SystemExit, match="--dpm"):
        cp.main(["--config", "c.yaml", "--dpm"])
    # the options reach `run` with copy_paste set; the plain command's do not carry it
    from mobi_amd.ldm import util
    seen = []
    monkeypatch.setattr(util, "load_config", lambda path, overrides=None: {"path": path, "overrides": overrides})
    monkeypatch.setattr(bt, "run", lambda opt, config, model=None: seen.append((opt, config)) or {})
    cp.main(["--config", "c.yaml", "--ddim_steps", "7", "--outdir", "o", "--", "a.b=3"])
    bt.main(["--config", "c.yaml", "--ddim_steps", "7", "--outdir", "o", "--no_overlays"])
    (opt, config), (plain, _) = seen
    assert opt.copy_paste is True and opt.ddim_steps == 1 and config == {"path": "c.yaml", "overrides": ["a.b=3"]}
    assert not opt.no_overlays and not hasattr(plain, "copy_paste") and plain.ddim_steps == 7 and plain.no_overlays
    # and the loop stops where the existing parser test stops it
    def stop(path, overrides=None):
        raise KeyboardInterrupt
    monkeypatch.setattr(util, "load_config", stop)
    with pytest.raises(KeyboardInterrupt):
        cp.main(["--config", "c.yaml"])


def test_shim_routes_copy_paste_and_leaves_other_command_lines_alone(monkeypatch):
    """A command line with `--copy-paste` goes to the baseline command without that word; any other reaches the test bench as it
    is (the command with the overlays, `mobi_amd.bench_tree`)."""
    from mobi_amd import bench_tree as bt
    from mobi_amd import copy_paste as cp
    calls = []
    monkeypatch.setattr(cp, "main", lambda argv=None: calls.append(("copy_paste", argv)))
    monkeypatch.setattr(bt, "main", lambda argv=None: calls.append(("test_bench", argv, list(sys.argv[1:]))))
    shim = os.path.join(ROOT, "scripts", "inference_test_bench.py")
    path = list(sys.path)
    try:
        monkeypatch.setattr(sys, "argv", [shim, "--config", "c.yaml", "--copy-paste", "--plms", "--save_samples", "a.b=3"])
        runpy.run_path(shim, run_name="__main__")
        monkeypatch.setattr(sys, "argv", [shim, "--config", "c.yaml", "--plms", "--save_samples", "a.b=3"])
        runpy.run_path(shim, run_name="__main__")
    finally:
        sys.path[:] = path
    assert calls == [("copy_paste", ["--config", "c.yaml", "--plms", "--save_samples", "a.b=3"]),
                     ("test_bench", None, ["--config", "c.yaml", "--plms", "--save_samples", "a.b=3"])]


def test_overlay_jobs_write_the_reference_paths(tmp_path):
    from PIL import Image
    from mobi_amd import bench_tree as bt
    from mobi_amd import test_bench as tb
    rng = np.random.default_rng(11)
    out, ids = str(tmp_path / "out"), ["car_a_1", "ped_b_2"]
    orig = [rng.integers(0, 256, (20, 30, 3), dtype=np.uint8) for _ in ids]
    pred = [rng.integers(0, 256, (20, 30, 3), dtype=np.uint8) for _ in ids]
    jobs = bt.overlay_jobs(out, ids, orig, pred)
    assert [os.path.relpath(p, out) for p, _ in jobs] == ["lidar/overlay_orig/car_a_1.png", "lidar/overlay_pred/car_a_1.png",
                                                          "lidar/overlay_orig/ped_b_2.png", "lidar/overlay_pred/ped_b_2.png"]
    w = tb.TreeWriter(threads=2)
    w.put(jobs)
    w.wait()
    for i, id_ in enumerate(ids):                                                   # PNG at PIL's defaults: lossless, no seed in the name
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "lidar", "overlay_orig", f"{id_}.png"))), orig[i])
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "lidar", "overlay_pred", f"{id_}.png"))), pred[i])
    assert sorted(os.listdir(os.path.join(out, "lidar"))) == ["overlay_orig", "overlay_pred"]
    assert bt.build_parser().parse_args(["--no_overlays"]).no_overlays and not bt.build_parser().parse_args([]).no_overlays
