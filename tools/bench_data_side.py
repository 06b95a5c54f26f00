#!/usr/bin/env python3
"""Dataset side timed at production geometry: a miniature database with 1600 x 900 frames and 512 x 512
views; host `__getitem__` per object (the reference's design, CPU), `raw_item` + `collate_device` (host IO / geometry,
device per-pixel work) and the two kernels alone against the HBM roofline; then the training splits' additions: the
reference-image augmentation on the host (`ref_augment_u8`) and on the device (`mobi_ref_augment`), `mobi_drop_context`, and
`raw_item` + `collate_device` per object with and without `ref_aug`.   python tools/bench_data_side.py"""
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from mobi_amd import build, ops
    build.build(verbose=False)
    from tests import mini_db
    from mobi_amd.ldm.data.nuscenes import NuScenesDataset
    from tools.sweep_split import timeit
    root = tempfile.mkdtemp(prefix="mobi_mini_db_")
    csv, pkl = mini_db.build(root, n_scenes=4, image_hw=(900, 1600))
    R = 512
    ds = NuScenesDataset(state="test", use_lidar=True, use_camera=True, object_database_path=csv, scene_database_path=pkl,
                         expand_mask_ratio=0.1, object_area_crop=0.2, num_samples_per_class=4, fixed_sampling=True,
                         object_random_crop=False, ref_aug=False, image_height=R, image_width=R, range_height=R, range_width=R,
                         object_classes=["car", "pedestrian"], range_object_norm=True, range_int_norm=True, min_lidar_points=8)
    B = len(ds)
    ds[0]; ds.raw_item(0)
    t0 = time.perf_counter()
    host = [ds[i] for i in range(B)]
    t_host = (time.perf_counter() - t0) / B
    t0 = time.perf_counter()
    raw = [ds.raw_item(i) for i in range(B)]
    t_raw = (time.perf_counter() - t0) / B
    ds.collate_device(raw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    batch = ds.collate_device(raw)
    torch.cuda.synchronize()
    t_col = (time.perf_counter() - t0) / B
    print(f"{B} objects, {R} x {R} views, 1600 x 900 frames: host __getitem__ {t_host * 1e3:.1f} ms per object (1 core); "
          f"raw_item {t_raw * 1e3:.1f} ms + collate_device {t_col * 1e3:.2f} ms per object")
    lid = batch["lidar"]
    d0, i0, m0 = (lid[k].float().contiguous() for k in ("range_depth_orig", "range_int_orig", "range_instance_mask_orig"))
    args = (d0, i0, m0, lid["range_shift_left"], lid["width_crop"], lid["min_depth_obj"].float(), lid["max_depth_obj"].float(), lid["range_mask"])
    us = timeit(lambda: ops.range_prepare(*args, height=R, width=R, alpha=0.75, object_norm=True, int_norm=True), 20, warm=2)
    nbytes = B * R * R * 4 * (2 + 2 + 1 + 1)                     # written views + the edit mask read (sweeps: L2-resident)
    print(f"mobi_range_prepare [{B}, {R}, {R}]: {us:.1f} us, {nbytes / us / 1e3:.0f} GB/s of {8000} (algorithmic {nbytes / 1e6:.1f} MB)")
    corners = (torch.rand(B, 8, 2, device="cuda") * R).to(torch.int32)
    us = timeit(lambda: ops.box_mask(corners, R, R), 20, warm=2)
    print(f"mobi_box_mask [{B}, {R}, {R}]: {us:.1f} us, {B * R * R * 4 / us / 1e3:.0f} GB/s written (24 edge tests per pixel in fp64: ALU-bound)")
    frames = torch.randint(0, 256, (B, 900, 1600, 3), dtype=torch.uint8, device="cuda")
    cw = (torch.rand(B, 8, 2, device="cuda") * 300 + 500).to(torch.int32)
    crop = torch.tensor([[400, 300, 420, 420]] * B, dtype=torch.int32).cuda()
    inv = torch.zeros(B, dtype=torch.int32, device="cuda")
    us = timeit(lambda: ops.image_prepare(frames, cw, inv, crop, height=R, width=R), 20, warm=2)
    nb = B * R * R * 4 * 7 + B * 420 * 420 * 3
    print(f"mobi_image_prepare [{B}, 900 x 1600 -> {R} x {R}]: {us:.1f} us, {nb / us / 1e3:.0f} GB/s (algorithmic {nb / 1e6:.1f} MB)")
    us = timeit(lambda: ops.box_mask(cw, 900, 1600, want_mask=False, want_stats=True), 20, warm=2)
    print(f"mobi_box_mask stats only [{B}, 900, 1600]: {us:.1f} us")
    bench_training_side(csv, pkl, R, timeit)


def bench_training_side(csv, pkl, R, timeit):
    """The train / val splits' per-pixel additions; kernel times are device events around a replayed graph of 20 launches,
    the median of 10 such measurements, inputs warmed."""
    from mobi_amd import ops
    from mobi_amd.ldm.data import ref_aug as RA
    from mobi_amd.ldm.data.nuscenes import NuScenesDataset, get_tensor_clip
    median = lambda fn: float(np.median([timeit(fn, 20, warm=2) for _ in range(10)]))
    rng = np.random.default_rng(1)
    B, S = 8, 224
    patches = rng.integers(0, 256, (B, S, S, 3)).astype(np.uint8)
    random.seed(1)
    draws = [RA.RefAugDraw(True, True, 30.0, True, 7, True, 1.3, 0.3)] + [RA.draw_ref_aug() for _ in range(B - 1)]
    RA.ref_augment_u8(patches[0], draws[0])
    t0 = time.perf_counter()
    for p, d in zip(patches, draws):
        get_tensor_clip()(RA.ref_augment_u8(p, d))
    t_mixed = (time.perf_counter() - t0) / B
    t0 = time.perf_counter()
    get_tensor_clip()(RA.ref_augment_u8(patches[0], draws[0]))
    t_all = time.perf_counter() - t0
    print(f"host ref_augment_u8 + get_tensor_clip [224, 224, 3]: {t_mixed * 1e3:.1f} ms per object over {B} drawn records, "
          f"{t_all * 1e3:.1f} ms with every stage on (7 x 7 box) (1 core)")
    forms = [RA.device_form(d, S) for d in draws]
    dev = lambda k: torch.stack([f[k] for f in forms]).cuda()
    src, flags, warp, table = torch.from_numpy(patches).cuda(), dev("flags"), dev("warp"), dev("table")
    us = median(lambda: ops.ref_augment(src, flags, warp, table))
    nb = B * S * S * (3 + 12)
    print(f"mobi_ref_augment [{B}, {S}, {S}] ({sum(d.rotate for d in draws)} rotated, {sum(d.blur for d in draws)} blurred): "
          f"{us:.1f} us, {nb / us / 1e3:.0f} GB/s (algorithmic {nb / 1e6:.1f} MB)")
    all_on = [forms[0]] * B
    dev = lambda k: torch.stack([f[k] for f in all_on]).cuda()
    flags1, warp1, table1 = dev("flags"), dev("warp"), dev("table")
    us = median(lambda: ops.ref_augment(src, flags1, warp1, table1))
    print(f"mobi_ref_augment [{B}, {S}, {S}] every stage on in every sample (7 x 7 box): {us:.1f} us")
    gt, inp = torch.randn(B, 3, R, R, device="cuda"), torch.randn(B, 3, R, R, device="cuda")
    mask = (torch.rand(B, 1, R, R, device="cuda") > 0.3).float()
    for name, fl in (("every sample dropped", torch.ones(B, dtype=torch.int32, device="cuda")),
                     ("half the samples dropped", (torch.arange(B, device="cuda") % 2).to(torch.int32))):
        us = median(lambda: ops.drop_context(gt, inp, mask, fl))
        nb = int(fl.sum()) * R * R * 4 * (1 + 3 * 3)
        print(f"mobi_drop_context [{B}, 3, {R}, {R}] {name}: {us:.1f} us, {nb / us / 1e3:.0f} GB/s (algorithmic {nb / 1e6:.1f} MB)")
    for aug in (False, True):
        np.random.seed(0)
        random.seed(0)
        ds = NuScenesDataset(state="train", use_lidar=True, use_camera=True, object_database_path=csv, scene_database_path=pkl,
                             expand_mask_ratio=0.1, object_area_crop=0.2, num_samples_per_class=4, fixed_sampling=True,
                             object_random_crop=False, ref_aug=aug, prob_drop_context=0.2 if aug else 0, image_height=R,
                             image_width=R, range_height=R, range_width=R, object_classes=["car", "pedestrian"],
                             range_object_norm=True, range_int_norm=True, min_lidar_points=8)
        n = len(ds)
        ds.raw_item(0)
        t0 = time.perf_counter()
        raw = [ds.raw_item(i) for i in range(n)]
        t_raw = (time.perf_counter() - t0) / n
        ds.collate_device(raw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ds.collate_device(raw)
        torch.cuda.synchronize()
        t_col = (time.perf_counter() - t0) / n
        print(f"state=train, ref_aug={aug}, prob_drop_context={0.2 if aug else 0}: raw_item {t_raw * 1e3:.1f} ms + collate_device "
              f"{t_col * 1e3:.2f} ms per object ({n} objects)")


if __name__ == "__main__":
    main()
