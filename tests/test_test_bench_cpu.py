"""CPU: the test-bench command's host side -- its parser against the reference's command line (tests/golden/test_bench_cli.json),
`ops.camera_export_layout`, `mobi_camera_export`'s refusals (host checks: no launch) and the result-tree writer on synthetic arrays."""
import ctypes as C
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_OFFERED = {"--copy-paste"}


@pytest.fixture(scope="module")
def lib():
    from mobi_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_parser_takes_the_reference_command_line(tmp_path, monkeypatch):
    from mobi_amd import test_bench as tb
    with open(os.path.join(ROOT, "tests", "golden", "test_bench_cli.json")) as f:
        ref = json.load(f)["arguments"]
    assert len(ref) == 24
    ap = tb.build_parser()
    mine = {s: a for a in ap._actions for s in a.option_strings}
    types = {"int": int, "float": float, "str": str}
    for arg in ref:
        flag = arg["flags"][0]
        if flag in NOT_OFFERED:
            assert flag not in mine
            continue
        if flag == "overrides":
            continue
        a = mine[flag]
        assert a.default == (False if arg.get("action") == "store_true" else arg.get("default")), flag
        assert (a.nargs == 0) == (arg.get("action") == "store_true") and a.choices == arg.get("choices"), flag
        if "type" in arg:
            assert a.type is types[arg["type"]], flag
    opt = ap.parse_args(["--config", "c.yaml", "--plms", "--scale", "5", "--save_samples", "ref_mode=track-ref", "a.b=3"])
    assert opt.overrides == ["ref_mode=track-ref", "a.b=3"] and opt.plms and opt.scale == 5.0 and opt.dtype == "fp16" and not opt.dpm
    # the overrides reach load_config
    from mobi_amd.ldm import util
    seen = {}

    def stop(path, overrides=None):
        seen.update(path=path, overrides=overrides)
        raise KeyboardInterrupt

    monkeypatch.setattr(util, "load_config", stop)
    with pytest.raises(KeyboardInterrupt):
        tb.main(["--config", "c.yaml", "--dtype", "bf16", "--", "ref_mode=track-ref", "a.b=3"])
    assert seen == {"path": "c.yaml", "overrides": ["ref_mode=track-ref", "a.b=3"]}
    import mobi_amd
    import torch
    assert mobi_amd.engine_dtype() == torch.bfloat16
    mobi_amd.set_engine_dtype(torch.float16)


@pytest.mark.parametrize("frames", [True, False])
def test_camera_export_layout(frames):
    from mobi_amd import ops
    crops = [(30, 10, 101, 77), (0, 0, 67, 53), (5, 3, 1, 1), (59, 37, 101, 53)]
    lay = ops.camera_export_layout(crops, 90, 160, frames)
    spans = []
    for crop, entry in zip(crops, lay["objects"]):
        want = {"patch_pred": (crop[3], crop[2], 3), "patch_gt": (crop[3], crop[2], 3), "object_pred": (224, 224, 3),
                "object_ref": (224, 224, 3)}
        if frames:
            want["frame"] = (90, 160, 3)
        assert {k: v[1] for k, v in entry.items()} == want
        spans += [(o, o + int(np.prod(s))) for o, s in entry.values()]
    spans.append((lay["status"], lay["status"] + 4 * len(crops)))
    assert all(lo % 4 == 0 for lo, _ in spans) and max(hi for _, hi in spans) == lay["bytes"]
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))                      # no two pictures overlap
    for bad in [(100, 10, 101, 77), (-1, 0, 5, 5), (0, 0, 0, 5), (0, 40, 10, 51)]:
        with pytest.raises(ValueError):
            ops.camera_export_layout([bad], 90, 160, frames)


def test_camera_export_validates_before_any_launch(lib):
    """No GPU here: every call must return on the host."""
    from mobi_amd import _lib, ops
    assert lib.mobi_struct_size(31) == C.sizeof(_lib.CameraExportParams) and _lib.STRUCT_IDS[31] is _lib.CameraExportParams
    assert lib.mobi_abi_version() == 6
    crops = [(30, 10, 101, 77), (0, 0, 67, 53)]
    lay = ops.camera_export_layout(crops, 90, 160, True)

    def call(crops=crops, out_bytes=lay["bytes"], shift=0, ref=224, frames=1, null=None, batch=None, status=lay["status"]):
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
        return lib.mobi_camera_export(C.byref(p), None)

    assert lib.mobi_camera_export(None, None) == -1
    for name in ("patch_pred", "patch_gt", "ref", "image", "mask", "taps", "crop", "offsets", "box_ws", "out"):
        assert call(null=name) == -1, name                                          # null pointers
    assert call(crops=[(100, 10, 101, 77)]) == -1 and call(crops=[(0, 40, 10, 51)]) == -1      # a crop outside the frame
    assert call(crops=[(-1, 0, 5, 5)]) == -1 and call(crops=[(0, 0, 0, 5)]) == -1
    assert call(shift=2) == -4                                                      # a misaligned offset
    assert call(status=lay["status"] + 2, out_bytes=lay["bytes"] + 4) == -4
    assert call(out_bytes=lay["bytes"] - 8) == -1                                   # a picture (here the status words) past out_bytes
    assert call(out_bytes=lay["objects"][1]["object_ref"][0] + 100) == -1
    assert call(shift=-4) == -1                                                     # a negative offset
    assert call(ref=200) == -2                                                      # ref is resized to 224 x 224 by the Python layer
    assert call(batch=33) == -2 and call(batch=0) == -1


def _pictures(rng, crops, H=20, W=30):
    return [{"frame": rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "patch_pred": rng.integers(0, 256, (ch, cw, 3), dtype=np.uint8),
             "patch_gt": rng.integers(0, 256, (ch, cw, 3), dtype=np.uint8), "object_pred": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8),
             "object_ref": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)} for cw, ch in crops]


def test_tree_writer_writes_the_reference_tree(tmp_path):
    from PIL import Image
    from mobi_amd import test_bench as tb
    rng = np.random.default_rng(7)
    out, seed, ids = str(tmp_path / "out"), 42, ["car_a_1", "ped_b_2"]
    pics = _pictures(rng, [(7, 5), (11, 3)])
    H0, W0, base = 32, 1096, 16
    range_pred = rng.uniform(-1, 1, (2, 4, H0, W0)).astype(np.float32)
    range_orig = rng.uniform(-1, 1, (2, 4, H0, W0)).astype(np.float32)
    grids = rng.integers(0, 256, (2, 2, 3, 4 * base, base), dtype=np.uint8)
    pcs = rng.integers(0, 256, (2, 3, 24, 40), dtype=np.uint8)
    depth = tb.collage_u8(rng.uniform(-1, 1, (2, 1, 5 * base, base)).astype(np.float32))
    inten = tb.collage_u8(rng.uniform(-1, 1, (2, 1, 5 * base, base)).astype(np.float32))
    w = tb.TreeWriter(threads=3)
    w.put(tb.camera_sample_jobs(out, seed, ids, ["cam_a.jpg", "cam_b.jpg"], pics))
    w.put(tb.lidar_sample_jobs(out, seed, ids, ["sweep_a.pcd.bin", "sweep_b.pcd.bin"], range_pred, range_orig))
    w.put(tb.camera_vis_jobs(out, seed, ids, grids[0], grids[1]) + tb.lidar_vis_jobs(out, seed, ids, pcs, depth, inten))
    w.wait()
    tb.write_metrics_csv(out, {"test/mse/object_pred_depth": [1.0, 2.0], "test/mse/mask_pred_depth": [0.5],
                               "test/median_error/object_pred_depth": [0.25, 0.25], "test/median_error/mask_pred_depth": []})
    listing = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    want = ["metrics.csv"]
    for i, id_ in enumerate(ids):
        want += [f"samples_seed42/cam_{'ab'[i]}.jpg", f"samples_seed42/sweep_{'ab'[i]}.pcd.bin.npy",
                 f"camera/object_pred/{id_}_object_pred_seed42.png", f"camera/object_ref/{id_}_object_ref_seed42.png",
                 f"camera/patch_gt/{id_}_gt_seed42.png", f"camera/patch_pred/{id_}_pred_seed42.png",
                 f"lidar/range_pred/{id_}_range_pred_seed42.npy", f"lidar/range_orig/{id_}_range_orig_seed42.npy",
                 f"camera/grid/{id_}_grid_seed42.jpg", f"lidar/point_clouds/{id_}_grid_pc_seed42.jpg"]
        for kind in ("depth", "intensity"):
            want += [f"lidar/range_{kind}_collage/{id_}_grid_{kind}_seed42.jpg", f"lidar/range_{kind}_pred/{id_}_seed42.png",
                     f"lidar/range_{kind}_target/{id_}_seed42.png"]
    assert listing == sorted(want)
    for i, id_ in enumerate(ids):
        for name, tag in tb.CAMERA_SAMPLE_FOLDERS.items():                          # PNG is lossless: RGB in, RGB back
            got = np.asarray(Image.open(os.path.join(out, "camera", name, f"{id_}_{tag}_seed42.png")))
            assert np.array_equal(got, pics[i][name]), name
        assert np.asarray(Image.open(os.path.join(out, "samples_seed42", f"cam_{'ab'[i]}.jpg"))).shape == (20, 30, 3)
        assert np.array_equal(np.load(os.path.join(out, "lidar", "range_pred", f"{id_}_range_pred_seed42.npy")), range_pred[i])
        assert np.array_equal(np.load(os.path.join(out, "lidar", "range_orig", f"{id_}_range_orig_seed42.npy")), range_orig[i])
        cloud = np.load(os.path.join(out, "samples_seed42", f"sweep_{'ab'[i]}.pcd.bin.npy"))
        d = (range_pred[i, 0] + 1) / 2 * 54
        assert cloud.shape == (int(((d > 1.4) & (d < 54)).sum()), 5)
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "lidar", "range_depth_pred", f"{id_}_seed42.png"))),
                              depth[i][3 * base:4 * base])
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "lidar", "range_intensity_target", f"{id_}_seed42.png"))),
                              inten[i][:base])
        assert np.asarray(Image.open(os.path.join(out, "camera", "grid", f"{id_}_grid_seed42.jpg"))).shape == (4 * base, 2 * base, 3)
        assert np.asarray(Image.open(os.path.join(out, "lidar", "range_depth_collage", f"{id_}_grid_depth_seed42.jpg"))).shape == (5 * base, base, 3)
    assert open(os.path.join(out, "metrics.csv")).read() == ",mse,median_error\nobject_pred_depth,1.5,0.25\nmask_pred_depth,0.5,\n"


def test_a_side_that_is_off_writes_nothing_and_errors_surface(tmp_path):
    from mobi_amd import test_bench as tb
    out = str(tmp_path / "out")
    w = tb.TreeWriter()
    w.put([])                                                                       # use_camera = use_lidar = False: no jobs
    w.wait()
    assert not os.path.exists(out)
    w = tb.TreeWriter(threads=8)                                                    # two objects of one scene: the later file stays
    same = os.path.join(out, "same.npy")
    for k in range(12):
        w.put([(same, (lambda k=k: np.full(200000, k))), (os.path.join(out, f"other{k}.npy"), np.zeros(1))])
    w.wait()
    assert np.load(same)[0] == 11 and np.load(same).shape == (200000,)
    blocker = tmp_path / "file"
    blocker.write_text("x")
    w = tb.TreeWriter(threads=2)
    good = os.path.join(out, "a.npy")
    w.put([(os.path.join(str(blocker), "sub", "b.png"), np.zeros((2, 2, 3), np.uint8)), (good, np.zeros(3))])
    for k in range(5):                                                              # more batches than the queue is deep: no deadlock
        w.put([(os.path.join(out, f"c{k}.npy"), np.zeros(1))])
    with pytest.raises(OSError):
        w.wait()
    assert tb.TreeWriter(threads=64)._pool._max_workers == 8
