#!/usr/bin/env python3
"""tests/golden/postprocess_full.npz: the harness post-processing of make_golden_postprocess2.py again, produced by the
REFERENCE's own functions on CPU (build container only), at the PRODUCT's geometry -- 512 x 512 samples, a 32 x 1096
sweep, width_crop = [64, 128, 256, 512] mixed in one batch (pooling windows 16 x 8 / 4 / 2 / 1), crop_left in the tiled
3 x 1096 coordinate with two windows that wrap around the sweep:
  * ldm.data.utils.postprocess_range_depth_int (-> LidarConverter.undo_default_transforms, pool_resize);
  * the range-view paste of scripts/inference_test_bench.py:583-610 restated AROUND the reference's functions
    (LidarConverter.range2pcd, ldm.data.box_np_ops.points_in_bbox_corners);
  * LatentDiffusion.log_data's lidar error scores (ddpm.py:1545-1597) on the batch and on each sample alone, with an
    empty object, an all-ones object at width_crop = 512 (32 x 512 = 16384 cells) and an odd / even cell count.
The inputs are tests/postprocess_full_cases.py (synthesised, NOT stored).  Stored: the reference's outputs on the
columns of each crop window (everywhere else the un-cropped and the pasted sweep equal the original, which the
generator asserts), the predicted masks, the boxes, the metric dicts and cell counts.
    python tests/golden/make_golden_postprocess_full.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                   # noqa: E402
from tests import postprocess_full_cases as cases         # noqa: E402


def main():
    numba = types.ModuleType("numba")
    deco = lambda *a, **k: (a[0] if a and callable(a[0]) and not k else (lambda f: f))
    numba.jit = numba.njit = deco
    sys.modules["numba"] = numba
    R = mg.import_reference()
    import ldm.data.utils as du
    import ldm.data.box_np_ops as bo
    from ldm.data.lidar_converter import LidarConverter, pool_resize
    out = {}
    B, h0, w0 = cases.B, cases.H0, cases.W0

    # ---- 1. un-crop (postprocess_range_depth_int) ------------------------------------------------------------------
    p = cases.paste_inputs()
    d_unc, i_unc = du.postprocess_range_depth_int(range_depth=p["depth"], range_depth_orig=p["d_orig"], range_int=p["inten"],
                                                  range_int_orig=p["i_orig"], crop_left=p["crop_left"],
                                                  width_crop=p["width_crop"])
    d_orig, i_orig = p["d_orig"].numpy(), p["i_orig"].numpy()

    # ---- 2. paste (inference_test_bench.py:583-610 around the reference's range2pcd / points_in_bbox_corners) --------
    conv = LidarConverter(H=h0, W=w0)
    boxes, pred_masks = [], []
    for i in range(B):
        cols = cases.window_columns(i)
        outside = np.setdiff1d(np.arange(w0), cols)
        assert np.array_equal(d_unc[i][:, outside], d_orig[i][:, outside]) and np.array_equal(i_unc[i][:, outside], i_orig[i][:, outside])
        assert (d_unc[i][:, cols] != d_orig[i][:, cols]).mean() > 0.99
        label = np.arange(0, h0 * w0).reshape(h0, w0)
        points, points_label, _ = conv.range2pcd(d_unc[i], p["pitch"][i], p["yaw"][i], label)
        # a box that catches a patch of the sweep INSIDE the crop window: built around a point of the un-cropped prediction
        in_window = np.nonzero(np.isin(points_label % w0, cols))[0]
        c = points[in_window[len(in_window) // 3]]
        half = np.array([4.0, 3.0, 2.5], dtype=np.float32) * (1 + 0.3 * i)
        sx = np.array([[-1, -1, -1], [-1, 1, -1], [1, 1, -1], [1, -1, -1], [-1, -1, 1], [-1, 1, 1], [1, 1, 1], [1, -1, 1]],
                      dtype=np.float32)
        th = 0.4 * i
        rot = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], dtype=np.float32)
        box = ((sx * half) @ rot.T + c).astype(np.float32)[None]       # [1, 8, 3], corner order of the nuScenes boxes
        object_points = bo.points_in_bbox_corners(points, box)
        pred = np.zeros(h0 * w0)
        pred[points_label[object_points[:, 0]]] = 1
        pred = pred.reshape(h0, w0)
        inst = np.logical_or(pred, p["gt_mask"][i])
        fd, fi = np.where(inst, d_unc[i], d_orig[i]), np.where(inst, i_unc[i], i_orig[i])
        assert np.array_equal(fd[:, outside], d_orig[i][:, outside]) and np.array_equal(fi[:, outside], i_orig[i][:, outside])
        n_in = int(pred[:, cols].sum())
        assert 0 < n_in < h0 * len(cols), f"sample {i}: the box caught {n_in} window pixels: the golden would be vacuous"
        print(f"sample {i}: predicted mask {int(pred.sum())} pixels, {n_in} of them inside the {len(cols)}-column window")
        out.update({f"unc_depth_win{i}": d_unc[i][:, cols], f"unc_int_win{i}": i_unc[i][:, cols],
                    f"paste_depth_win{i}": fd[:, cols], f"paste_int_win{i}": fi[:, cols]})
        pred_masks.append(pred.astype(np.uint8))
        boxes.append(box[0])
    out.update(paste_boxes=np.stack(boxes), paste_pred_mask=np.stack(pred_masks))

    # ---- 3. lidar error scores (LatentDiffusion.log_data, ddpm.py:1499-1597) ------------------------------------------
    LD = R.ddpm.LatentDiffusion
    m = cases.metric_inputs()
    counts = np.zeros((B, 2), dtype=np.int64)
    for i in range(B):
        size = (cases.POOL_H, cases.WIDTH_CROP[i])
        counts[i, 0] = int((pool_resize(m["inst"][[i]], size, mode="max_pool") == 1).sum())
        counts[i, 1] = int((pool_resize(1 - m["rmask"][[i]], size, mode="max_pool") == 1).sum())
    print("selected cells (object, mask) per sample:", counts.tolist())
    assert counts[0, 0] % 2 == 1 and counts[1, 0] % 2 == 0 and counts[1, 0] > 0 and counts[2, 0] == 0
    assert counts[3, 0] == 16384 and (counts[:, 1] > 0).all()

    def scores(sel):
        n = len(sel)

        class Fake:
            use_camera, use_lidar = False, True
            range_object_norm, range_object_norm_scale, range_int_norm = True, 0.75, True
            decode_first_stage = lambda self, h, module_name=None: m["sample"][sel].clone()
            log_dict = lambda self, *a, **k: None

        R.ddpm.get_lidar_vis = lambda **k: (torch.zeros(n, 3, 4, 4),) * 3
        batch = {"lidar": {"range_data": m["data_in"][sel].clone(), "range_data_inpaint": m["data_in"][sel] * m["rmask"][sel],
                           "range_mask": m["rmask"][sel], "range_instance_mask": m["inst"][sel], "min_depth_obj": m["min_d"][sel],
                           "max_depth_obj": m["max_d"][sel], "width_crop": m["width_crop"][sel],
                           "range_depth_orig": None, "range_shift_left": None, "range_pitch": None, "range_yaw": None},
                 "bbox_3d": None}
        return LD.log_data(Fake(), batch, {"lidar_rec": m["rec"][sel].clone()}, None, None, log_metrics=False,
                           return_sample=True, split="test")

    log, metrics = scores(list(range(B)))
    keys = sorted(metrics)
    per_sample = np.array([[scores([i])[1][k] for k in keys] for i in range(B)])
    assert np.isnan(per_sample[2]).sum() == 8 and np.isfinite(np.delete(per_sample, 2, 0)).all()
    out.update(met_keys=np.array(keys), met_values=np.array([metrics[k] for k in keys]), met_per_sample=per_sample,
               met_counts=counts,
               # the de-normalised depth (log_data overwrites the logged tensor in place): a 64 x 8 sub-grid and the sum
               met_range_sample_depth_sub=log["range_sample_depth"][:, 0, ::8, ::64],
               met_range_sample_depth_sum=log["range_sample_depth"].double().sum())
    mg.save("postprocess_full", **out)


if __name__ == "__main__":
    main()
