"""Harness post-processing at the PRODUCT's geometry, CPU part: the oracle (oracle/postprocess.py) against
tests/golden/postprocess_full.npz, which the REFERENCE's functions produced on 512 x 512 samples, a 32 x 1096 sweep and
width_crop = [64, 128, 256, 512] in one batch (tests/golden/make_golden_postprocess_full.py; inputs synthesised by
tests/postprocess_full_cases.py, not stored).  Arrays bit-exact, scores to rtol 1e-12, as tests/test_postprocess2.py
holds them at the reduced geometry.  Plus the condition the GPU paste-back test rests on: the share of bytes of the
resized patch that a float64 evaluation cannot decide."""
import numpy as np
import pytest
import torch

from oracle import postprocess as op
from tests import postprocess_full_cases as cases
from tests.golden_cases import load


@pytest.fixture(scope="module")
def g():
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in load("postprocess_full").items()}


def test_oracle_uncrop_and_paste_match_the_reference_full_geometry(g):
    p = cases.paste_inputs()
    d0, i0 = p["d_orig"].numpy(), p["i_orig"].numpy()
    wraps = 0
    for i in range(cases.B):
        cl, wc, cols = cases.CROP_LEFT[i], cases.WIDTH_CROP[i], cases.window_columns(i)
        wraps += int(cols[-1] < cols[0])
        outside = np.setdiff1d(np.arange(cases.W0), cols)
        d = op.undo_default_transforms(cl, wc, p["depth"][i, 0].numpy(), d0[i])
        it = op.undo_default_transforms(cl, wc, p["inten"][i, 0].numpy(), i0[i])
        assert np.array_equal(d[:, cols], g[f"unc_depth_win{i}"]) and np.array_equal(it[:, cols], g[f"unc_int_win{i}"])
        assert np.array_equal(d[:, outside], d0[i][:, outside]) and np.array_equal(it[:, outside], i0[i][:, outside])
        pm, df, itf = op.paste_object(d, it, d0[i], i0[i], p["pitch"][i], p["yaw"][i], g["paste_boxes"][i], p["gt_mask"][i])
        assert 0 < pm[:, cols].sum() < pm[:, cols].size and np.array_equal(pm, g["paste_pred_mask"][i] != 0)
        assert np.array_equal(df[:, cols], g[f"paste_depth_win{i}"]) and np.array_equal(itf[:, cols], g[f"paste_int_win{i}"])
        assert np.array_equal(df[:, outside], d0[i][:, outside]) and np.array_equal(itf[:, outside], i0[i][:, outside])
    assert wraps == 2


def oracle_metric_pairs(m, sel=slice(None)):
    den = lambda t: op.range_denorm(t[sel], m["min_d"][sel], m["max_d"][sel], alpha=0.75, object_norm=True, int_norm=True)
    (sd, si), (rd, ri), (idp, ii) = den(m["sample"]), den(m["rec"]), den(m["data_in"])
    return {"pred_depth": (sd, idp), "rec_depth": (rd, idp), "pred_int": (si, ii), "rec_int": (ri, ii)}


def test_oracle_lidar_scores_match_the_reference_full_geometry(g):
    m = cases.metric_inputs()
    keys = [str(k) for k in g["met_keys"]]
    ref, per = dict(zip(keys, g["met_values"])), g["met_per_sample"]
    box = 1 - m["rmask"]
    pairs = oracle_metric_pairs(m)
    assert np.array_equal(pairs["pred_depth"][0][:, 0, ::8, ::64].numpy(), g["met_range_sample_depth_sub"])
    assert np.isclose(float(pairs["pred_depth"][0].double().sum()), float(g["met_range_sample_depth_sum"]), rtol=1e-12)
    assert g["met_counts"][:, 0].tolist() == [463, 878, 0, 16384] and g["met_counts"][0, 0] % 2 == 1
    for name, (p, q) in pairs.items():
        sc = op.lidar_scores(p, q, m["inst"], box, m["width_crop"])
        scale = (54 - 1.4) / 2 if "depth" in name else 128
        for si, score in ((0, "mse"), (1, "median_error")):
            obj = sc[:, 0, si]
            assert np.isnan(obj).tolist() == [False, False, True, False]   # sample 2 has no object pixels: dropped
            assert np.isclose(obj[~np.isnan(obj)].mean() * scale, ref[f"test/{score}/object_{name}"], rtol=1e-12)
            assert np.isclose(sc[:, 1, si].mean() * scale, ref[f"test/{score}/mask_{name}"], rtol=1e-12)
            # each sample alone (the reference's log_data on a batch of one)
            ko, km = keys.index(f"test/{score}/object_{name}"), keys.index(f"test/{score}/mask_{name}")
            assert np.allclose(sc[:, 0, si] * scale, per[:, ko], rtol=1e-12, atol=0, equal_nan=True)
            assert np.allclose(sc[:, 1, si] * scale, per[:, km], rtol=1e-12, atol=0)


def test_paste_patch_undecidable_share():
    """A byte of the resized patch is decided by the float64 evaluation unless (v + 1) / 2 * 255 lies within 1e-3 of an
    integer.  The GPU test holds every decided byte EXACT; that is only a sharp test while few bytes are undecidable:
    at most 1 % for every committed crop (uniformly spread values give 0.2 %; saturated pixels of the patch, which land
    exactly on 0 / 255, add to it)."""
    patch = cases.camera_patch().numpy()
    assert 0 < (np.abs(patch) == 1).mean() < 0.02
    for left, top, cw, ch in cases.PASTE_CROPS:
        want, und = cases.paste_patch_f64(patch, ch, cw)
        assert want.shape == (ch, cw, 3) and und.mean() <= 0.01, (cw, ch, und.mean())
        assert want.min() < 16 and want.max() > 239              # the patch spans the byte range
    # the restatement itself: torch-CPU's fp32 F.interpolate agrees on every decided byte of the first crop
    left, top, cw, ch = cases.PASTE_CROPS[0]
    want, und = cases.paste_patch_f64(patch, ch, cw)
    t = torch.nn.functional.interpolate(torch.from_numpy(patch)[None], (ch, cw), mode="bilinear")[0].numpy()
    t8 = (((t.transpose(1, 2, 0)[..., ::-1] + 1.0) / 2.0) * 255).astype(np.uint8)
    diff = np.abs(t8.astype(np.int32) - want.astype(np.int32))
    assert diff[~und].max() == 0 and diff.max() <= 1
