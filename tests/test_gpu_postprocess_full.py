"""The harness post-processing and the dataset side (row 3) -- mobi_amd/csrc/postprocess.hip and
mobi_range_denorm -- at the geometry the PRODUCT runs (configs/mobi_nusc_512.yaml): 512 x 512 range views, a 32 x 1096
sweep, 900 x 1600 camera frames, 16 objects per batch, width_crop in {64, 128, 256, 512} mixed inside one batch.  The
small-geometry tests (tests/test_postprocess2.py, tests/test_gpu_data_side.py) never reach the LDS sort at its capacity
(32 x 512 = 16384 cells), a grid-stride loop's second trip (launches are capped at 8192 blocks, `mobi_box_mask` at 256
per box) or the 16 x 8 pooling window.  Every comparison keeps the criterion of the small-geometry test of the same
kernel; references are tests/golden/postprocess_full.npz (the reference's own functions), oracle/postprocess.py and
restatements in numpy / torch-CPU.  Every batched call is also compared, bit for bit, with B = 1 calls on its slices:
that catches a wrong second trip independently of any reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import postprocess as op
from tests import postprocess_full_cases as cases
from tests.golden_cases import load

pytestmark = pytest.mark.gpu

WIDTHS16 = [64, 128, 256, 512] * 4


@pytest.fixture(scope="module")
def g():
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in load("postprocess_full").items()}


def _cuda(d):
    return {k: (torch.as_tensor(v).cuda() if isinstance(v, (np.ndarray, torch.Tensor)) else v) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------------
# range view: un-crop + paste
# ---------------------------------------------------------------------------------------------------------------------
def _expected_sweeps(g, p, kind):
    """the reference's full sweeps rebuilt from the stored window columns: the original everywhere else"""
    out = []
    for i in range(cases.B):
        d, it = p["d_orig"][i].numpy().copy(), p["i_orig"][i].numpy().copy()
        cols = cases.window_columns(i)
        d[:, cols], it[:, cols] = g[f"{kind}_depth_win{i}"], g[f"{kind}_int_win{i}"]
        out.append((d, it))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _paste_kwargs(g, p, sel=slice(None)):
    c = lambda t: torch.as_tensor(t)[sel].cuda()
    return dict(range_depth=c(p["depth"]), range_int=c(p["inten"]), range_depth_orig=c(p["d_orig"]),
                range_int_orig=c(p["i_orig"]), crop_left=p["crop_left"][sel], width_crop=p["width_crop"][sel],
                range_pitch=p["pitch"][sel], range_yaw=p["yaw"][sel], bbox_3d=g["paste_boxes"][sel],
                gt_instance_mask=p["gt_mask"][sel])


def test_gpu_uncrop_and_paste_bit_exact_full_geometry(g):
    """Pooling windows 16 x 8 / 4 / 2 / 1 in ONE launch, two windows that wrap around the 1096-column sweep, crop_left in
    the tiled 3 x 1096 coordinate.  The 128-addend fp32 window sum in (row, column) order is the order of the reference's
    F.avg_pool2d on torch-CPU: a numpy restatement of that order reproduces the fixture's four windows with 0 differing
    values, so the criterion stays bit-exact equality."""
    from mobi_amd.ldm.data import utils as du
    p = cases.paste_inputs()
    want_d, want_i = _expected_sweeps(g, p, "unc")
    fin_d, fin_i = _expected_sweeps(g, p, "paste")
    c = lambda t: t.cuda()
    d, it = du.postprocess_range_depth_int(range_depth=c(p["depth"]), range_depth_orig=c(p["d_orig"]), range_int=c(p["inten"]),
                                           range_int_orig=c(p["i_orig"]), crop_left=p["crop_left"], width_crop=p["width_crop"])
    print("un-crop: differing values", int((d != want_d).sum()), int((it != want_i).sum()))
    assert isinstance(d, np.ndarray) and np.array_equal(d, want_d) and np.array_equal(it, want_i)
    out = du.paste_range_objects(**_paste_kwargs(g, p))
    assert torch.equal(out["depth_unc"].cpu(), torch.from_numpy(want_d)) and torch.equal(out["int_unc"].cpu(), torch.from_numpy(want_i))
    assert np.array_equal(out["pred_mask"].cpu().numpy() != 0, g["paste_pred_mask"] != 0)
    assert torch.equal(out["depth_final"].cpu(), torch.from_numpy(fin_d)) and torch.equal(out["int_final"].cpu(), torch.from_numpy(fin_i))
    # B = 1 on every slice == the slice of the batched launch
    for i in range(cases.B):
        one = du.paste_range_objects(**_paste_kwargs(g, p, slice(i, i + 1)))
        assert set(one) == set(out)
        for k in out:
            assert torch.equal(one[k][0], out[k][i]), (k, i)


def test_gpu_range_paste_second_trip_and_optional_outputs(g):
    """64 samples: 64 x 32 x 1096 pixels are 8768 blocks, past the 8192-block cap, so the grid-stride loop takes a second
    trip; the result must be the 4-sample result 16 times.  Then the optional arguments: exactly the keys the docstring
    names, and the same depth_unc."""
    from mobi_amd import ops
    from mobi_amd.ldm.data.utils import box_planes
    p = cases.paste_inputs()
    c = lambda t: torch.as_tensor(t).cuda()
    planes = torch.from_numpy(box_planes(g["paste_boxes"])).cuda()
    args = (c(p["depth"])[:, 0], c(p["d_orig"]), p["crop_left"], p["width_crop"])
    full = dict(sample_int=c(p["inten"])[:, 0], int_orig=c(p["i_orig"]), pitch=c(p["pitch"]), yaw=c(p["yaw"]), planes=planes,
                gt_mask=c(p["gt_mask"]))
    base = ops.range_paste(*args, **full)
    assert set(base) == {"depth_unc", "int_unc", "depth_final", "int_final", "pred_mask"}
    rep = lambda t: t.repeat(16, *([1] * (t.dim() - 1))).contiguous()
    big = ops.range_paste(rep(args[0]), rep(args[1]), rep(args[2]), rep(args[3]), **{k: rep(v) for k, v in full.items()})
    for k, v in base.items():
        assert torch.equal(big[k], rep(v)), k
    no_int = ops.range_paste(*args, **{k: v for k, v in full.items() if k not in ("sample_int", "int_orig")})
    assert set(no_int) == {"depth_unc", "depth_final", "pred_mask"}
    no_planes = ops.range_paste(*args, sample_int=full["sample_int"], int_orig=full["int_orig"])
    assert set(no_planes) == {"depth_unc", "int_unc"}
    bare = ops.range_paste(*args)
    assert set(bare) == {"depth_unc"}
    for o in (no_int, no_planes, bare):
        assert torch.equal(o["depth_unc"], base["depth_unc"])
    assert torch.equal(no_int["depth_final"], base["depth_final"]) and torch.equal(no_int["pred_mask"], base["pred_mask"])
    assert torch.equal(no_planes["int_unc"], base["int_unc"])


def test_gpu_window_arguments_are_checked_before_any_launch():
    """Host-resident windows: 0 < wc <= width and width % wc == 0, or ValueError BEFORE a launch (the reference's
    F.avg_pool2d(kernel = w // wc) yields wc columns only then; a wc > w would index past the kernel's sort space).
    Device-resident windows are not read back: the kernel clamps them, seen through the count column."""
    from mobi_amd import _lib, ops
    z = torch.zeros(2, 512, 512, device="cuda")
    one = torch.ones(2, 512, 512, device="cuda")
    for bad in ([512, 1024], [0, 64], [-64, 64], [96, 64], [512, 300]):
        with pytest.raises(ValueError):
            ops.lidar_metrics(z, z, one, one, bad)
        with pytest.raises(ValueError):
            ops.lidar_metrics(z, z, one, one, torch.tensor(bad))
        with pytest.raises(ValueError):
            ops.range_paste(z, torch.zeros(2, 32, 1096, device="cuda"), [0, 0], bad)
    with pytest.raises(ValueError):                                   # a window wider than the sweep it is pasted into
        ops.range_paste(z, torch.zeros(2, 32, 256, device="cuda"), [0, 0], [512, 64])
    p = _lib.LidarMetricsParams()                                     # the library's own check: max_width > w
    out = torch.empty(2, 2, 3, device="cuda")
    wc = torch.tensor([64, 64], dtype=torch.int32, device="cuda")
    ptr = lambda t: t.data_ptr()
    p.pred, p.gt, p.inst_mask, p.box_mask, p.width_crop, p.out = ptr(z), ptr(z), ptr(one), ptr(one), ptr(wc), ptr(out)
    p.batch, p.h, p.w, p.pool_h, p.max_width = 2, 512, 512, 32, 1024
    import ctypes
    with pytest.raises(_lib.EngineError, match="argument"):
        _lib.check(_lib.load().mobi_lidar_metrics(ctypes.byref(p), None), "mobi_lidar_metrics")
    # device-resident, out of range: clamped to the view's width / skipped, never past the sort space
    e = torch.rand(2, 512, 512, device="cuda")
    got = ops.lidar_metrics(e, z, one, one, torch.tensor([1024, 0], device="cuda")).cpu()
    ref = ops.lidar_metrics(e, z, one, one, [512, 512]).cpu()
    assert got[0, :, 2].tolist() == [16384.0, 16384.0] and torch.equal(got[0], ref[0])
    assert got[1, :, 2].tolist() == [0.0, 0.0] and bool(torch.isnan(got[1, :, :2]).all())
    sweep = torch.rand(2, 32, 1096, device="cuda")
    un = ops.range_paste(e, sweep, torch.tensor([40, 40], device="cuda"), torch.tensor([4096, 0], device="cuda"))["depth_unc"]
    assert torch.equal(un[0], ops.range_paste(e[:1], sweep[:1], [40], [512])["depth_unc"][0]) and torch.equal(un[1], sweep[1])


# ---------------------------------------------------------------------------------------------------------------------
# lidar error scores
# ---------------------------------------------------------------------------------------------------------------------
def test_gpu_log_data_scores_full_geometry(g):
    """LatentDiffusion.log_data on the engine against the reference's metric dict at 512 x 512 with the four widths in
    one batch: medians exact, depth RMSE 1e-6 relative, intensity scores 1e-5 relative (device logf), as at the reduced
    geometry."""
    import mobi_amd
    from mobi_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    mobi_amd.set_engine_dtype(torch.float16)
    m = cases.metric_inputs()
    ref = dict(zip([str(k) for k in g["met_keys"]], g["met_values"]))

    class Stub(LatentDiffusion):
        def __init__(self):                                       # no networks: decode_first_stage is given
            torch.nn.Module.__init__(self)
            self.use_camera, self.use_lidar = False, True
            self.range_object_norm, self.range_object_norm_scale, self.range_int_norm = True, 0.75, True

        def decode_first_stage(self, z, **kw):
            return m["sample"].cuda()

    c = lambda t: t.cuda()
    batch = {"lidar": {"range_data": c(m["data_in"]), "range_data_inpaint": c(m["data_in"] * m["rmask"]),
                       "range_mask": c(m["rmask"]), "range_instance_mask": c(m["inst"]), "min_depth_obj": c(m["min_d"]),
                       "max_depth_obj": c(m["max_d"]), "width_crop": m["width_crop"]}}
    log, metrics = Stub().log_data(batch, {"lidar_rec": c(m["rec"])}, None, None, log_metrics=False, return_sample=True,
                                   split="test")
    assert sorted(metrics) == sorted(ref) and len(ref) == 16
    for k, v in ref.items():
        tol = 1e-5 if "int" in k else (0 if "median" in k else 1e-6)
        print(f"{k}: engine {metrics[k]!r} reference {v!r} rel {abs(metrics[k] - v) / abs(v):.2e}")
        assert abs(metrics[k] - v) <= tol * abs(v), (k, metrics[k], v)
    assert np.array_equal(log["range_sample_depth"][:, 0, ::8, ::64].cpu().numpy(), g["met_range_sample_depth_sub"])
    assert abs(float(log["range_sample_depth"].double().sum()) - float(g["met_range_sample_depth_sum"])) < 1e-6


def _scores_and_counts(pred, gt, inst, box, widths):
    sc = op.lidar_scores(pred[:, None], gt[:, None], inst[:, None], box[:, None], widths)
    cnt = np.zeros((len(widths), 2))
    for i, wc in enumerate(widths):
        k = (512 // 32, 512 // int(wc))
        cnt[i] = [float((F.max_pool2d(m[[i]][None], k) == 1).sum()) for m in (inst, box)]
    return sc, cnt


def test_gpu_lidar_metrics_table_at_capacity_and_batch_16(g):
    """The table itself, B = 16, against oracle.postprocess.lidar_scores (pinned to the reference by the fixture) and the
    max-pooled cell counts: count and median exact, RMSE 1e-6 relative.  Sample 3 (and 7, 11, 15) is the all-ones mask at
    width_crop = 512: n = cap = 16384, the whole bitonic network, nothing to pad; sample 2 has no object: NaN, NaN, 0."""
    from mobi_amd import ops
    m = cases.metric_inputs()
    den = op.range_denorm(torch.cat([m["sample"], m["rec"], m["data_in"], m["sample"].flip(0)]),
                          m["min_d"].repeat(4), m["max_d"].repeat(4))[0][:, 0]              # 16 de-normalised depth views
    gt = op.range_denorm(torch.cat([m["data_in"]] * 2 + [m["rec"]] * 2), m["min_d"].repeat(4), m["max_d"].repeat(4))[0][:, 0]
    inst, box = m["inst"][:, 0].repeat(4, 1, 1), (1 - m["rmask"])[:, 0].repeat(4, 1, 1)
    gt[8:12] = den[8:12]                                              # pred == gt: every score exactly 0
    want, cnt = _scores_and_counts(den, gt, inst, box, WIDTHS16)
    assert cnt[3].tolist() == [16384.0, float(g["met_counts"][3, 1])] and cnt[2, 0] == 0
    c = lambda t: t.cuda().contiguous()
    got = ops.lidar_metrics(c(den), c(gt), c(inst), c(box), WIDTHS16)
    again = ops.lidar_metrics(c(den), c(gt), c(inst), c(box), torch.tensor(WIDTHS16).cuda())
    assert torch.equal(got.cpu().view(torch.int32), again.cpu().view(torch.int32))          # the atomicAdd fill order does not leak
    got32 = got.cpu().numpy()
    got = got32.astype(np.float64)
    for i in range(16):
        one = ops.lidar_metrics(c(den[[i]]), c(gt[[i]]), c(inst[[i]]), c(box[[i]]), WIDTHS16[i:i + 1]).cpu()
        assert np.array_equal(one.numpy()[0].view(np.int32), got32[i].view(np.int32)), i
        for r in range(2):
            assert got[i, r, 2] == cnt[i, r], (i, r, got[i, r, 2], cnt[i, r])
            if cnt[i, r] == 0:
                assert np.isnan(got[i, r, 0]) and np.isnan(got[i, r, 1])
                continue
            rel = abs(got[i, r, 0] - want[i, r, 0]) / max(want[i, r, 0], 1e-30)
            print(f"sample {i} region {r}: n {int(cnt[i, r])} rmse rel {rel:.2e} median {got[i, r, 1]!r} / {want[i, r, 1]!r}")
            assert got[i, r, 1] == want[i, r, 1], (i, r)
            assert abs(got[i, r, 0] - want[i, r, 0]) <= 1e-6 * want[i, r, 0], (i, r)
    assert (got[8:12, :, :2][~np.isnan(got[8:12, :, :2])] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# dataset side
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("int_norm", [False, True])
def test_gpu_range_prepare_batch_16_full_geometry(int_norm):
    """B = 16 views of 512 x 512 are 16384 blocks: the second trip of the grid-stride loop (from B = 9).  Widths
    {64, 128, 256, 512} mixed, windows that wrap, against np.tile / slice / np.repeat and the dataset's torch expressions."""
    from mobi_amd import ops
    from mobi_amd.ldm.data.utils import depth_normalization
    rng = np.random.default_rng(11)
    B, H0, W0, R = 16, 32, 1096, 512
    depth = rng.uniform(-1, 1, (B, H0, W0)).astype(np.float32)
    depth[:, :, ::7] = -1.0                                            # empty pixels
    inten = rng.integers(0, 256, (B, H0, W0)).astype(np.float32)
    inst = (rng.uniform(0, 1, (B, H0, W0)) > 0.9).astype(np.float32)
    width_crop = np.array(WIDTHS16)
    # in the tiled 3 x 1096 coordinate: windows that wrap (one by a single column, one starting at the last column), that
    # end flush with the sweep's and with the tiled array's last column, that start at column 0
    crop_left = np.array([1096 + 37, 2 * 1096 - 100, 3 * 1096 - 256, 1096 + 700, 1096 + 1060, 2192, 1096 + 900, 2192 + 300,
                          1096 + 1095, 2192 + 968, 1096 + 841, 1096 + 584, 1096, 2192 + 500, 2192 + 100, 1096 + 1000])
    assert (crop_left + width_crop <= 3 * W0).all()                    # the window lies inside the three tiled sweeps
    assert ((crop_left % W0 + width_crop) > W0).sum() == 7 and (crop_left >= 2 * W0).sum() == 6
    lo = rng.uniform(-0.9, 0.0, B).astype(np.float32)
    hi = (lo + rng.uniform(0.05, 0.9, B)).astype(np.float32)
    mask = (rng.uniform(0, 1, (B, 1, R, R)) > 0.3).astype(np.float32)
    t = lambda a: torch.tensor(a).cuda()
    call = lambda s: ops.range_prepare(t(depth[s]), t(inten[s]), t(inst[s]), t(crop_left[s]), t(width_crop[s]), t(lo[s]),
                                       t(hi[s]), t(mask[s]), height=R, width=R, alpha=0.75, object_norm=True, int_norm=int_norm)
    rd, rdi, io = (x.cpu() for x in call(slice(None)))
    for b in range(B):
        views = []
        for a in (depth[b], inten[b], inst[b]):
            win = np.tile(a, 3)[:, crop_left[b]:crop_left[b] + width_crop[b]]
            assert win.shape == (H0, width_crop[b])
            views.append(np.repeat(np.repeat(win, R // H0, 0), R // width_crop[b], 1))
        d = depth_normalization(torch.from_numpy(views[0])[None], torch.tensor(lo[b]), torch.tensor(hi[b]), alpha=0.75)
        v = torch.from_numpy(((views[1] / 255) - 0.5) * 2)[None]
        if int_norm:
            v = torch.clamp(2 * (1 - torch.exp(-2 * (v + 1))) - 1, -1, 1)
        assert torch.equal(rd[b, :1], d), b                                # piecewise-linear map: bit for bit
        if int_norm:
            assert float((rd[b, 1:] - v).abs().max()) <= 2e-7, b           # expf on the device vs torch's exp
        else:
            assert torch.equal(rd[b, 1:], v), b
        assert torch.equal(rdi[b], rd[b] * torch.from_numpy(mask[b])), b
        assert torch.equal(io[b, 0], torch.from_numpy(views[2])), b
        one = call(slice(b, b + 1))
        assert torch.equal(one[0][0].cpu(), rd[b]) and torch.equal(one[1][0].cpu(), rdi[b]) and torch.equal(one[2][0].cpu(), io[b]), b


def _boxes_900x1600():
    rng = np.random.default_rng(13)
    H, W = cases.FRAME_H, cases.FRAME_W
    corners = []
    for k in range(8):
        c = np.array([rng.uniform(100, W - 100), rng.uniform(100, H - 100)])
        corners.append(c + rng.normal(0, 20 + 15 * k, (8, 2)))
    corners.append(np.array([[100, 50], [1500, 60], [1480, 850], [120, 840], [140, 90], [1450, 100], [1440, 800], [160, 790]], dtype=np.float64))
    corners.append(np.full((8, 2), 5000.0))                                                  # off-frame
    corners.append(np.array([[1400, 700], [1599, 700], [1599, 899], [1400, 899]] * 2, dtype=np.float64))   # touches x = 1599, y = 899
    corners.append(np.array([[-80, -40], [300.7, -60], [350.2, 260.9], [-120, 200]] * 2))   # partly outside, fractional
    return np.stack(corners)


def test_gpu_box_mask_900x1600_twelve_boxes():
    """A 900 x 1600 frame is 5625 blocks of pixels for a launch of 256 per box: every block walks 22 trips and the stats
    are reduced over all of them.  12 boxes incl. one covering more than half the frame, one off-frame, one touching the
    last column and row; against the host's fill_box_faces, exact."""
    from mobi_amd import ops
    from mobi_amd.ldm.data.utils import fill_box_faces
    H, W = cases.FRAME_H, cases.FRAME_W
    corners = _boxes_900x1600()
    assert len(corners) == 12
    dev = torch.tensor(corners).cuda()
    got, stats = ops.box_mask(dev, H, W, want_stats=True)
    only = ops.box_mask(dev, H, W, want_mask=False, want_stats=True)
    assert torch.equal(only, stats)
    got, stats = got.cpu().numpy(), stats.cpu().numpy()
    for k in range(len(corners)):
        filled = fill_box_faces(corners[k], H, W) > 0.5
        assert np.array_equal(got[k], (1.0 - filled).astype(np.float32)), k
        ys, xs = np.nonzero(filled)
        want = [filled.sum(), xs.min(), xs.max(), ys.min(), ys.max()] if filled.any() else [0, W, -1, H, -1]
        assert list(stats[k]) == want, k
        m1, s1 = ops.box_mask(dev[[k]], H, W, want_stats=True)
        assert np.array_equal(m1[0].cpu().numpy(), got[k]) and list(s1[0].cpu().numpy()) == want, k
    assert stats[8, 0] > H * W // 2 and stats[9, 0] == 0 and got[9].min() == 1
    assert list(stats[10]) == [200 * 200, 1400, 1599, 700, 899] and stats[11, 1] == 0 and stats[11, 3] == 0


def test_gpu_image_prepare_batch_16_900x1600():
    """B = 16 frames of 900 x 1600 into 512 x 512 views (16384 blocks: second trip), against torch-CPU F.interpolate
    (bilinear, align_corners=False, no antialias) of the normalised crop and of the fill_box_faces mask, <= 1e-6 absolute
    (tests/test_gpu_data_side.py::test_collate_device_equals_host_items).  Crops: flush with the right / bottom edge, larger
    than the output (1500 x 850, down-scaling), smaller (up-scaling), the whole frame."""
    from mobi_amd import ops
    from mobi_amd.ldm.data.utils import fill_box_faces
    rng = np.random.default_rng(17)
    B, H, W, R = 16, cases.FRAME_H, cases.FRAME_W, 512
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    fixed = [(900, 400, 700, 500), (50, 25, 1500, 850), (600, 300, 301, 257), (0, 0, 1600, 900)]    # left, top, crop_W, crop_H
    crops = []
    for b in range(B):
        if b < len(fixed):
            crops.append(fixed[b])
            continue
        cw, ch = int(rng.integers(97, 1200)), int(rng.integers(97, 880))
        crops.append((int(rng.integers(0, W - cw + 1)), int(rng.integers(0, H - ch + 1)), cw, ch))
    crops = np.array(crops)
    assert crops[0, 0] + crops[0, 2] == W and crops[0, 1] + crops[0, 3] == H
    corners = np.stack([np.array([l + cw / 2, t + ch / 2]) + rng.normal(0, 0.2 * min(cw, ch), (8, 2)) for l, t, cw, ch in crops])
    corners[5] = 5000.0                                               # no edit pixel: the dataset sets invert
    invert = np.array([1 if b in (5, 6, 11) else 0 for b in range(B)])
    dev = lambda a: torch.as_tensor(a).cuda()
    gt, inp, mk = (x.cpu() for x in ops.image_prepare(dev(frames), dev(corners), invert, torch.tensor(crops, dtype=torch.int32),
                                                      height=R, width=R))
    worst = 0.0
    for b in range(B):
        l, t, cw, ch = (int(v) for v in crops[b])
        image = (torch.from_numpy(frames[b]).permute(2, 0, 1).float().div(255) - 0.5) / 0.5
        mask = 1. - torch.tensor(fill_box_faces(corners[b], H, W) > 0.5).float()
        if invert[b]:
            mask = 1 - mask
        image, mask = image[:, t:t + ch, l:l + cw], mask[t:t + ch, l:l + cw]
        image = F.interpolate(image[None], size=(R, R), mode="bilinear", align_corners=False)[0]
        mask = F.interpolate(mask[None, None], size=(R, R), mode="bilinear", align_corners=False)[0]
        errs = [float((gt[b] - image).abs().max()), float((mk[b] - mask).abs().max()), float((inp[b] - image * mask).abs().max())]
        worst = max(worst, *errs)
        assert max(errs) <= 1e-6, (b, errs)
        assert 0 < float(mk[b].mean()) < 1 or b == 5, b              # the edit region shows in the view
        one = ops.image_prepare(dev(frames[[b]]), dev(corners[[b]]), invert[[b]], torch.tensor(crops[[b]], dtype=torch.int32),
                                height=R, width=R)
        assert torch.equal(one[0][0].cpu(), gt[b]) and torch.equal(one[1][0].cpu(), inp[b]) and torch.equal(one[2][0].cpu(), mk[b]), b
    print(f"image_prepare: worst absolute deviation {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# camera paste-back
# ---------------------------------------------------------------------------------------------------------------------
def test_gpu_gaussian_blur_900x1600_and_smaller_than_the_kernel():
    """15 taps, sigma 7 on a 900 x 1600 mask (5625 blocks, two passes) and on a 7 x 9 mask, where BORDER_REFLECT_101
    reaches past the FAR edge (n < ksize: the reflected index is reflected again); <= 2e-6 absolute on 0..1."""
    from mobi_amd import ops
    k = torch.from_numpy(op.gaussian_kernel1d(15, 7.0)).cuda()
    H, W = cases.FRAME_H, cases.FRAME_W
    rng = np.random.default_rng(19)
    big = np.ones((H, W), dtype=np.float32)
    big[200:700, 400:1300] = 0
    big[850:, 1500:] = 0                                              # an edit region in the last rows / columns
    big[:9, :30] = rng.uniform(0, 1, (9, 30)).astype(np.float32)
    small = rng.uniform(0, 1, (7, 9)).astype(np.float32)
    for name, m in (("900x1600", big), ("7x9", small), ("1x40", small.reshape(1, 63)[:, :40].copy())):
        got = ops.gaussian_blur(torch.from_numpy(m).cuda(), k).cpu().numpy()
        # (one row: the vertical pass reads that row for every tap, as two equal rows do)
        want = op.gaussian_blur_reflect101(m, 15, 7.0) if m.shape[0] > 1 else op.gaussian_blur_reflect101(np.concatenate([m, m]), 15, 7.0)[:1]
        err = float(np.abs(got - want).max())
        print(f"blur {name}: max abs deviation {err:.2e}")
        assert err <= 2e-6, (name, err)


def test_gpu_paste_patch_exact_where_float64_decides():
    """The 512 x 512 patch resized into a 900 x 1600 frame at odd crop sizes, over the right / bottom edge, with negative
    top / left, and wholly off-frame.  Sharper than the 1-LSB-on-0.5-% criterion of the small test: the four-tap
    expression in float64 DECIDES every byte whose value is not within 1e-3 of an integer (at most 1 % are not:
    tests/test_postprocess_full_cpu.py); decided bytes are exact, the others within 1 LSB; everything outside the crop
    keeps the frame's pattern."""
    from mobi_amd import ops
    H, W = cases.FRAME_H, cases.FRAME_W
    patch = cases.camera_patch()
    pattern = cases.frame_pattern()
    for left, top, cw, ch in cases.PASTE_CROPS:
        frame = torch.from_numpy(pattern.copy()).cuda()
        got = ops.paste_patch(patch.cuda(), frame, top, left, ch, cw).cpu().numpy()
        want, und = cases.paste_patch_f64(patch.numpy(), ch, cw)
        y0, y1, x0, x1 = max(top, 0), min(top + ch, H), max(left, 0), min(left + cw, W)
        outside = np.ones((H, W), dtype=bool)
        if y1 > y0 and x1 > x0:
            outside[y0:y1, x0:x1] = False
            w, u = want[y0 - top:y1 - top, x0 - left:x1 - left], und[y0 - top:y1 - top, x0 - left:x1 - left]
            diff = np.abs(got[y0:y1, x0:x1].astype(np.int32) - w.astype(np.int32))
            print(f"paste {(left, top, cw, ch)}: undecidable {u.mean():.4%}, off by one {int((diff != 0).sum())} bytes")
            assert u.mean() <= 0.01 and diff[~u].max() == 0 and diff.max() <= 1
        else:
            assert (left, top, cw, ch) == cases.PASTE_CROPS[-1]
        assert np.array_equal(got[outside], pattern[outside])


def test_gpu_blend_frame_900x1600():
    """The full camera paste-back on a 900 x 1600 frame against the oracle: <= 2e-3 absolute on 0..255 where the uint8
    patch agrees (as at 90 x 160).  Then the blend alone: where its mask is EXACTLY 1 the frame's own uint8 conversion
    comes back exactly (1 * u8 + 0 * pred), where it is exactly 0 the pasted bytes do.  The fp32 taps of the 15-tap
    sigma-7 kernel sum to 0.99999994, so a BLURRED mask never is exactly 1 (its maximum on this frame: 0.9999999); the
    exact ones are therefore written into the blurred mask far from the edit region before the second blend."""
    from mobi_amd import ops
    from mobi_amd.ldm.data import utils as du
    from oracle import weights as Wt
    H, W = cases.FRAME_H, cases.FRAME_W
    patch = cases.camera_patch()[None]
    image = torch.clamp(Wt.synth_input("ppf.image", (3, H, W)) * 0.5, -1, 1)
    crop = cases.PASTE_CROPS[0]
    left, top, cw, ch = crop
    mask = torch.ones(H, W)
    mask[top + 40:top + ch - 40, left + 60:left + cw - 60] = 0
    ref_recon, ref_pred = op.paste_camera_patch(patch, image, mask, crop)
    recon, pred = du.paste_camera_patch(patch_pred=patch.cuda(), image=image.cuda(), mask=mask.cuda(), crop=crop)
    diff = np.abs(pred.cpu().numpy().astype(np.int32) - ref_pred.astype(np.int32))
    assert diff.max() <= 1 and (diff != 0).mean() < 5e-3
    same = diff.max(-1) == 0
    assert np.abs(recon.cpu().numpy() - ref_recon)[same].max() < 2e-3
    blur = ops.gaussian_blur(mask.cuda(), torch.from_numpy(op.gaussian_kernel1d(15, 7.0)).cuda())
    far = torch.ones(H, W, dtype=torch.bool)
    far[top + 20:top + ch - 20, left + 40:left + cw - 40] = False     # more than 7 pixels from the edit region
    assert float(blur.max()) < 1.0 and float(blur.cpu()[far].min()) > 0.999999
    blur[far.cuda()] = 1.0
    out = ops.blend_frame(blur, image.cuda().contiguous(), pred).cpu().numpy()
    blur = blur.cpu().numpy()
    u8 = (((image.numpy().transpose(1, 2, 0)[..., ::-1] + 1.0) / 2.0) * 255).astype(np.uint8)
    keep, gone = blur == 1.0, blur == 0.0
    assert keep.mean() > 0.8 and gone.sum() > 10000 and ((blur > 0) & (blur < 1)).sum() > 10000
    assert np.array_equal(out[keep], u8[keep].astype(np.float32))
    assert np.array_equal(out[gone], pred.cpu().numpy()[gone].astype(np.float32))
    mid = ~keep & ~gone
    want = blur[..., None] * u8.astype(np.float32) + (1 - blur[..., None]) * pred.cpu().numpy().astype(np.float32)
    assert np.abs(out - want)[mid].max() < 2e-3
