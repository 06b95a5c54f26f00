"""GPU: the copy-paste baseline (`python -m mobi_amd.copy_paste`) and the lidar-on-camera overlays of the test bench
(`python -m mobi_amd.bench_tree`: `mobi_amd/test_bench.py` is kept as it is, and its own command writes no overlays), end to end
on the miniature database with the reduced model of tests/test_gpu_test_bench.py: 4 objects on two 450 x 800 frames, each frame
shared by two objects."""
import os

import numpy as np
import pytest
import torch

from tests import copy_paste_ref as cr
from tests import overlay_ref as ovr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    """Run 1: the plain command, 2 steps.  Runs 2 and 3: the baseline asked for 7 steps and for 1.  Run 4: the baseline with
    --no_overlays, on run 3's model.  Run 5: `mobi_amd.test_bench`'s own command, with run 1's arguments."""
    import mobi_amd
    from mobi_amd import bench_tree as bt
    from mobi_amd import copy_paste as cp
    from mobi_amd import test_bench as tb
    from mobi_amd.ldm.util import instantiate_from_config, load_config
    from oracle import weights as W
    from tests import mini_db
    root = tmp_path_factory.mktemp("baseline")
    csv, pkl = mini_db.build(str(root / "db"))
    data = "data.params.test.params."
    overrides = ["latent_size=16", "image_height=128", "image_width=128", "range_height=128", "range_width=128", "use_lidar=True",
                 "ref_mode=id-ref",
                 "model.params.lidar_stage_config.params.ckpt_path=null",
                 "model.params.unet_config.params.model_channels=64",
                 "model.params.first_stage_config.params.ddconfig.ch=32",
                 "model.params.lidar_stage_config.params.ddconfig.ch=32",
                 "model.params.cond_stage_config.params.clip_config.hidden_size=1024",
                 "model.params.cond_stage_config.params.clip_config.intermediate_size=256",
                 "model.params.cond_stage_config.params.clip_config.num_hidden_layers=1",
                 "model.params.cond_stage_config.params.clip_config.num_attention_heads=16",
                 f"{data}object_database_path={csv}", f"{data}scene_database_path={pkl}", f"{data}num_samples_per_class=2",
                 f"{data}min_lidar_points=8", f"{data}range_int_norm=True"]
    config = os.path.join(ROOT, "configs", "mobi_nusc_256.yaml")
    mobi_amd.set_engine_dtype(torch.float16)
    cfg = load_config(config, overrides)
    model = instantiate_from_config(cfg["model"])
    W.fill_module_(model, seed=29)
    ckpt = str(root / "model.ckpt")
    torch.save({"state_dict": model.state_dict()}, ckpt)
    del model
    cfg["data"]["params"]["test"]["params"]["return_original_image"] = True
    tb.seed_everything(42)                                   # as the command does before it builds the split
    dataset = instantiate_from_config(cfg["data"]["params"]["test"])
    items = [dataset[i] for i in range(len(dataset))]
    common = ["--config", config, "--ckpt", ckpt, "--scale", "5", "--n_samples", "2", "--n_workers", "0", "--save_samples"]
    dirs = [str(root / f"run{k}") for k in (1, 2, 3, 4, 5)]
    bt.main(common + ["--outdir", dirs[0], "--ddim_steps", "2", *overrides])
    cp.main(common + ["--outdir", dirs[1], "--ddim_steps", "7", *overrides])
    loaded, load_model = [], tb.load_model
    tb.load_model = lambda *a: loaded.append(load_model(*a)) or loaded[-1]
    try:
        cp.main(common + ["--outdir", dirs[2], "--ddim_steps", "1", *overrides])
    finally:
        tb.load_model = load_model
    opt = cp.parse(common + ["--outdir", dirs[3], "--no_overlays", *overrides])
    tb.seed_everything(opt.seed)
    bt.run(opt, load_config(config, overrides), loaded[0])
    tb.main(common + ["--outdir", dirs[4], "--ddim_steps", "2", *overrides])
    return dirs, items


def _files(d):
    return sorted(os.path.relpath(os.path.join(p, f), d) for p, _, fs in os.walk(d) for f in fs)


def _png(*path):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(*path)))


def test_the_step_count_is_forced(bench):
    dirs, _ = bench
    a, b = _files(dirs[1]), _files(dirs[2])
    assert a == b and len(a) > 10
    for f in a:
        with open(os.path.join(dirs[1], f), "rb") as fa, open(os.path.join(dirs[2], f), "rb") as fb:
            assert fa.read() == fb.read(), f
    plain = _files(dirs[0])
    assert plain == a                                        # the same tree as the plain command's, with other pictures
    differs = [f for f in a if f.startswith("camera/object_pred/")
               and open(os.path.join(dirs[0], f), "rb").read() != open(os.path.join(dirs[1], f), "rb").read()]
    assert len(differs) == len([f for f in a if f.startswith("camera/object_pred/")])


def test_the_loop_is_test_bench_s_plus_the_overlays(bench):
    """`bench_tree.run` repeats `test_bench.run`, which is kept as it is: apart from the overlays the two commands write the same
    bytes."""
    dirs, _ = bench
    mine, kept = _files(dirs[0]), _files(dirs[4])
    assert [f for f in mine if not f.startswith("lidar/overlay_")] == kept and len(kept) > 10 and len(mine) == len(kept) + 8
    for f in kept:
        with open(os.path.join(dirs[0], f), "rb") as fa, open(os.path.join(dirs[4], f), "rb") as fb:
            assert fa.read() == fb.read(), f


def test_overlay_folders(bench):
    from PIL import Image
    dirs, items = bench
    ids = [it["id_name"] for it in items]
    assert len(ids) == 4 == len(set(ids))
    for d in dirs[:3]:
        for folder in ("overlay_orig", "overlay_pred"):
            assert sorted(os.listdir(os.path.join(d, "lidar", folder))) == sorted(f"{i}.png" for i in ids), (d, folder)
            for i in ids:
                assert Image.open(os.path.join(d, "lidar", folder, f"{i}.png")).size == (800, 450)
    for i in ids:                                            # the original sweep on the original frame: the same in every run
        with open(os.path.join(dirs[0], "lidar", "overlay_orig", f"{i}.png"), "rb") as fa:
            with open(os.path.join(dirs[1], "lidar", "overlay_orig", f"{i}.png"), "rb") as fb:
                assert fa.read() == fb.read(), i
    lidar = sorted(os.listdir(os.path.join(dirs[3], "lidar")))                      # --no_overlays leaves both folders out
    assert lidar == ["range_orig", "range_pred"]
    assert sorted(os.listdir(os.path.join(dirs[3], "camera"))) == sorted(os.listdir(os.path.join(dirs[1], "camera")))


def test_baseline_pictures_of_every_object(bench):
    from ldm.data.nuscenes import resize_linear_u8
    dirs, items = bench
    d = dirs[1]
    for it in items:
        id_ = it["id_name"]
        orig = it["image"]["orig"]
        mask = np.asarray(orig["mask"], dtype=np.float32)
        left, top, cw, ch = (int(v) for v in orig["crop"])
        box = cr.box_of(mask)
        assert box is not None
        y1, y2, x1, x2 = box
        object_ref = _png(d, "camera", "object_ref", f"{id_}_object_ref_seed42.png")
        object_pred = _png(d, "camera", "object_pred", f"{id_}_object_pred_seed42.png")
        assert np.array_equal(object_pred, resize_linear_u8(resize_linear_u8(object_ref, y2 - y1, x2 - x1), 224, 224)), id_
        patch_pred = _png(d, "camera", "patch_pred", f"{id_}_pred_seed42.png")
        assert patch_pred.shape == (ch, cw, 3)
        x = np.asarray(orig["image"], dtype=np.float32).transpose(1, 2, 0)
        I = ((x + np.float32(1)) / np.float32(2) * np.float32(255)).clip(0, 255).astype(np.uint8)
        keep = (cr.dilate(mask) == 1)[top:top + ch, left:left + cw]
        assert keep.any() and not keep.all(), id_
        assert np.array_equal(patch_pred[keep], I[top:top + ch, left:left + cw][keep]), id_
        # inside the dilated edit region the crop window shows the pasted reference
        pasted = np.zeros(mask.shape + (3,), dtype=np.uint8)
        pasted[y1:y2, x1:x2] = resize_linear_u8(object_ref, y2 - y1, x2 - x1)
        edit = np.zeros(mask.shape, dtype=bool)
        edit[y1:y2, x1:x2] = True
        edit &= cr.dilate(mask) == 0
        edit = edit[top:top + ch, left:left + cw]
        assert edit.any() and np.array_equal(patch_pred[edit], pasted[top:top + ch, left:left + cw][edit]), id_


def test_overlays_against_the_overlay_reference(bench):
    from mobi_amd.ldm.data import utils as du
    dirs, items = bench
    d = dirs[1]
    lut = du.turbo_lut()
    for it in items:
        id_ = it["id_name"]
        orig, lid = it["image"]["orig"], it["lidar"]
        matrix = np.asarray(orig["lidar2image"])
        ref = ovr.reference(np.asarray(lid["range_depth_orig"]), np.asarray(lid["range_pitch"]), np.asarray(lid["range_yaw"]), matrix,
                            np.asarray(orig["image"], dtype=np.float32), 3, lut)
        ovr.condition(ref)
        print(f"{id_}: kept {ref['count']}, fragile {int(ref['fragile'].sum())}")
        assert ovr.check_picture(_png(d, "lidar", "overlay_orig", f"{id_}.png"), ref, lut, f"overlay_orig {id_}") > 0
        # the edited sweep on the recomposed frame, inside the crop window (the written files hold both)
        left, top, cw, ch = (int(v) for v in orig["crop"])
        sweep = np.load(os.path.join(d, "lidar", "range_pred", f"{id_}_range_pred_seed42.npy"))
        canvas = np.zeros((450, 800, 3), dtype=np.uint8)
        canvas[top:top + ch, left:left + cw] = _png(d, "camera", "patch_pred", f"{id_}_pred_seed42.png")
        ref = ovr.reference(sweep[0], sweep[2], sweep[3], matrix, canvas, 3, lut)
        window = np.zeros((450, 800), dtype=bool)
        window[top:top + ch, left:left + cw] = True
        left_out, covered = int((ref["left_out"] & window).sum()), int((ref["covered"] & window).sum())
        print(f"{id_}: overlay_pred window covered {covered}, left out {left_out}")
        assert not ref["near_plane"].any() and left_out <= 0.25 * max(covered, 1), (id_, left_out, covered)
        ref["left_out"] = ref["left_out"] | ~window
        ovr.check_picture(_png(d, "lidar", "overlay_pred", f"{id_}.png"), ref, lut, f"overlay_pred {id_}")
