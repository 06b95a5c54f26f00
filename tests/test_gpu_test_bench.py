"""GPU: `python -m mobi_amd.test_bench` end to end on the miniature database with a reduced model: the result tree of the reference's
scripts/inference_test_bench.py, written twice byte for byte, and what the save flags switch off."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE_FOLDERS = {"camera/object_pred": "{id}_object_pred_seed42.png", "camera/object_ref": "{id}_object_ref_seed42.png",
                  "camera/patch_gt": "{id}_gt_seed42.png", "camera/patch_pred": "{id}_pred_seed42.png",
                  "lidar/range_pred": "{id}_range_pred_seed42.npy", "lidar/range_orig": "{id}_range_orig_seed42.npy"}
VIS_FOLDERS = {"camera/grid": "{id}_grid_seed42.jpg", "lidar/point_clouds": "{id}_grid_pc_seed42.jpg",
               "lidar/range_depth_collage": "{id}_grid_depth_seed42.jpg", "lidar/range_depth_pred": "{id}_seed42.png",
               "lidar/range_depth_target": "{id}_seed42.png", "lidar/range_intensity_collage": "{id}_grid_intensity_seed42.jpg",
               "lidar/range_intensity_pred": "{id}_seed42.png", "lidar/range_intensity_target": "{id}_seed42.png"}


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    """The mini database, a reduced model's checkpoint, and runs 1 - 3 of the command."""
    import mobi_amd
    from mobi_amd import test_bench as tb
    from mobi_amd.ldm.util import instantiate_from_config, load_config
    from oracle import weights as W
    from tests import mini_db
    root = tmp_path_factory.mktemp("test_bench")
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
    common = ["--config", config, "--ckpt", ckpt, "--scale", "5", "--n_samples", "2", "--n_workers", "0"]
    dirs = [str(root / f"run{k}") for k in (1, 2, 3)]
    for d in dirs[:2]:
        tb.main(common + ["--outdir", d, "--ddim_steps", "2", "--save_samples", "--save_visualisations", *overrides])
    # (4 steps, not 3: the uniform schedule takes every 1000 // S-th step plus one, and S = 3 ends on index 1000 of a 1000-entry
    # table, in the reference as here)
    tb.main(common + ["--outdir", dirs[2], "--plms", "--ddim_steps", "4", *overrides])
    return dirs, dataset


def _files(d):
    return sorted(os.path.relpath(os.path.join(p, f), d) for p, _, fs in os.walk(d) for f in fs)


def test_run_writes_the_whole_tree(bench):
    from PIL import Image
    dirs, dataset = bench
    d = dirs[0]
    items = [dataset[i] for i in range(len(dataset))]
    ids = [it["id_name"] for it in items]
    assert len(set(ids)) == len(ids) >= 3
    for folder, pattern in {**SAMPLE_FOLDERS, **VIS_FOLDERS}.items():
        assert sorted(os.listdir(os.path.join(d, folder))) == sorted(pattern.format(id=i) for i in ids), folder
    samples = set(os.listdir(os.path.join(d, "samples_seed42")))
    assert samples == {it["image"]["orig"]["file_name"] for it in items} | {it["lidar"]["file_name"] + ".npy" for it in items}
    for it in items:
        id_ = it["id_name"]
        left, top, cw, ch = (int(v) for v in it["image"]["orig"]["crop"])
        for name in ("patch_gt", "patch_pred"):
            tag = name.split("_")[1]
            assert Image.open(os.path.join(d, "camera", name, f"{id_}_{tag}_seed42.png")).size == (cw, ch)
        for name in ("object_pred", "object_ref"):
            assert Image.open(os.path.join(d, "camera", name, f"{id_}_{name}_seed42.png")).size == (224, 224)
        frame = np.asarray(Image.open(os.path.join(d, "samples_seed42", it["image"]["orig"]["file_name"])))
        assert frame.shape == (450, 800, 3)
        pred = np.load(os.path.join(d, "lidar", "range_pred", f"{id_}_range_pred_seed42.npy"))
        orig = np.load(os.path.join(d, "lidar", "range_orig", f"{id_}_range_orig_seed42.npy"))
        assert pred.shape == orig.shape == (4, 32, 1096) and np.array_equal(pred[2:], orig[2:])
        cloud = np.load(os.path.join(d, "samples_seed42", it["lidar"]["file_name"] + ".npy"))
        assert cloud.ndim == 2 and cloud.shape[1] == 5 and len(cloud) > 0
        # the sweep changes only where an object is (the ground-truth instance) or was put (inside the box)
        from mobi_amd.ldm.data.box_np_ops import box_planes
        from oracle import postprocess as op
        xyz, valid = op.range2pcd_dense(pred[0], pred[2], pred[3])
        planes = box_planes(np.asarray(it["bbox_3d"])[None])[0]
        inside = valid & ((xyz @ planes[:, :3].T + planes[:, 3]) < 1e-3).all(-1)      # (1e-3: the kernel's fp32 sum order)
        changed = (pred[:2] != orig[:2]).any(0)
        assert not (changed & ~(inside | (np.asarray(it["lidar"]["range_instance_mask_orig"]) != 0))).any()
    from mobi_amd import realism                              # the realism commands pair these folders by sorted name
    pairs = realism.paired_files(os.path.join(d, "camera", "patch_gt"), os.path.join(d, "camera", "patch_pred"))
    assert len(pairs) == len(ids) and all(a.name.replace("_gt_", "_pred_") == b.name for a, b in pairs)
    assert len(realism.range_files(os.path.join(d, "lidar", "range_pred"))) == len(ids)
    text = open(os.path.join(d, "metrics.csv")).read().splitlines()
    assert text[0] == ",mse,median_error" and len(text) == 9 and all(len(line.split(",")) == 3 for line in text)


def test_second_run_is_byte_identical(bench):
    dirs, _ = bench
    a, b = _files(dirs[0]), _files(dirs[1])
    assert a == b and len(a) > 10
    for f in a:
        with open(os.path.join(dirs[0], f), "rb") as fa, open(os.path.join(dirs[1], f), "rb") as fb:
            assert fa.read() == fb.read(), f


def test_without_the_save_flags_only_the_metrics_are_written(bench):
    dirs, _ = bench
    assert _files(dirs[2]) == ["metrics.csv"]
    assert open(os.path.join(dirs[2], "metrics.csv")).read().startswith(",mse,median_error\n")
