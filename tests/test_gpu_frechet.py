"""FID / FRD on the MI355X (mobi_amd/realism.py): mobi_igemm's MOBI_EPI_LEAKY_RELU on every variant RangeNet routes to, the
RangeNet input, band-mean and moments kernels, RangeNet features against the reference model's golden
(tests/golden/frd.npz, made by tests/golden/make_golden_frd.py), FRD and FID end to end against fp64, and the file tools
against the tensor API.  Each test prints its measured error; bounds are recorded next to them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import frd_ref                                                          # noqa: E402
import realism_ref as RR                                                # noqa: E402
from mobi_amd import _lib, ops, realism as M                            # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.float16, torch.bfloat16)
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}            # unit roundoff of T

# Bounds = the value measured on the MI355X + 20 % (fp16 ceilings: feature rel-L2 5e-3, relative distance error 1e-2).
# leaky igemm, max |err| / (|ref| + 1e-2 max |ref|): measured 4.79e-4 (fp16), 3.82e-3 (bf16)
LEAKY_BOUND = {torch.float16: 5.8e-4, torch.bfloat16: 4.6e-3}
# RangeNet feature rel-L2 against the reference model's fp64 features (tests/golden/frd.npz): measured 2.78e-4 (fp16),
# 1.70e-3 (bf16)
FEAT_BOUND = {torch.float16: 3.4e-4, torch.bfloat16: 2.1e-3}
# relative distance error against fp64: FRD measured 1.69e-4 (fp16), 1.49e-3 (bf16); FID 2.15e-4 (fp16), 1.18e-4 (bf16)
FRD_BOUND = {torch.float16: 2.1e-4, torch.bfloat16: 1.8e-3}
FID_BOUND = {torch.float16: 2.6e-4, torch.bfloat16: 1.5e-4}


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "frd.npz"))


def golden_views():
    """The golden's six 512 x 512 range views, rebuilt from their stored codes."""
    gd = golden()
    return frd_ref.views_from_codes(gd["depth_codes"], gd["int_codes"])


def _variant(x, pw, hout, wout, pad, residual):
    q = _lib.IgemmParams()
    n, hi, wi, ci = x.shape
    q.src0 = q.weight = q.out = q.bias = q.weight_tiled = 4096
    q.c0, q.batch, q.hin, q.win, q.hout, q.wout = ci, n, hi, wi, hout, wout
    q.kh, q.kw, q.stride, q.pad_h, q.pad_w, q.groups = pw.kh, pw.kw, 1, pad[0], pad[1], 1
    q.n_packed = q.cout = pw.cout
    q.residual = 4096 if residual else None
    q.scale, q.dtype, q.epilogue = 1.0, ops._dt(x.dtype), _lib.EPI_LEAKY_RELU
    lib = _lib.load()
    return lib.mobi_igemm_kernel_variant(C.byref(q)), lib.mobi_igemm_plan_splits(C.byref(q))


# (batch, h, w, cin, cout, kh, kw, pad, wout, expected variant): RING_128 = 4, RING_256 = 5
LEAKY_CASES = [(4, 64, 64, 64, 64, 3, 3, (1, 1), 64, 4),        # a 3 x 3 block conv, 128-pixel tiles
               (16, 64, 128, 128, 256, 3, 3, (1, 1), 128, 5),   # 256-pixel tiles, 256 channels
               (2, 64, 128, 32, 64, 1, 1, (0, 0), 128, 4),      # 1 x 1, 32-channel source
               (2, 64, 64, 64, 64, 3, 2, (1, 1), 64, 4),        # the stride-(1, 2) rewrite on a paired view
               (8, 64, 64, 512, 512, 1, 3, (0, 1), 64, 5),      # the transposed-conv rewrite
               (3, 64, 32, 32, 32, 3, 3, (1, 1), 32, 4)]        # the stem's 32-channel shape


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", LEAKY_CASES)
@pytest.mark.parametrize("bias,resid", [(False, False), (True, False), (True, True)])
def test_igemm_leaky_relu_against_fp64(dtype, case, bias, resid):
    n, h, w, ci, co, kh, kw, pad, wout, want_variant = case
    g = torch.Generator().manual_seed(ci + co + kh)
    x = torch.randn((n, h, w, ci), generator=g).to(dtype)
    wt = (torch.randn((co, ci, kh, kw), generator=g) / (ci * kh * kw) ** 0.5).to(dtype).float()
    b = torch.randn((co,), generator=g) if bias else None
    res = torch.randn((n, h, wout, co), generator=g).to(dtype) if resid else None
    pw = ops.pack_conv(wt, b, dtype, DEV)
    assert _variant(x, pw, h, wout, pad, resid) == (want_variant, 1)
    got = ops.igemm(x.to(DEV), pw, pad=pad, hout=h, wout=wout, residual=None if res is None else res.to(DEV), leaky=True)
    xp = F.pad(x.double().permute(0, 3, 1, 2), (pad[1], pad[1] + kw, pad[0], pad[0] + kh))
    y = F.conv2d(xp, wt.double(), None if b is None else b.double())[:, :, :h, :wout]
    y = F.leaky_relu(y, 0.1).permute(0, 2, 3, 1)
    if res is not None:
        y = y + res.double()
    err = (got.cpu().double() - y).abs()
    scale = y.abs() + 1e-2 * y.abs().max()
    rel = (err / scale).max().item()
    print(f"leaky {dtype} {case} bias={bias} resid={resid}: variant {want_variant}, max rel err {rel:.2e}")
    assert rel < LEAKY_BOUND[dtype], rel                          # one rounding of T (unit roundoff EPS) + fp32 accumulation


def test_igemm_leaky_relu_refuses_split_and_transposed():
    x = torch.zeros((2, 16, 16, 64), device=DEV, dtype=torch.float16)
    pw = ops.pack_conv(torch.zeros((64, 64, 3, 3)), None, torch.float16, DEV)
    with pytest.raises(_lib.EngineError):
        ops.igemm(x, pw, leaky=True, out_mode=_lib.OUT_TRANSPOSED)
    with pytest.raises(_lib.EngineError):
        ops.igemm(x, pw, leaky=True, split_k=2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_frd_input_against_golden(dtype):
    gd = golden()
    views = golden_views()
    want = torch.stack([frd_ref.prepare(v) for v in views])                       # f32 [6, 5, 64, 1024]
    mask_want = ~(want == -1).all(1)
    assert np.array_equal(np.packbits(mask_want.numpy(), axis=-1), gd["mask"])
    got = ops.frd_input(torch.from_numpy(views).float().to(DEV), dtype).cpu()     # T [6, 64, 1024, 32]
    assert got.shape == (6, 64, 1024, 32)
    assert torch.equal(got[..., 5:], torch.zeros_like(got[..., 5:]))
    g5 = got[..., :5].permute(0, 3, 1, 2)
    mask_got = ~(g5 == -1).all(1)
    assert torch.equal(mask_got, mask_want), int((mask_got != mask_want).sum())  # bit-exact mask
    wt = want.to(dtype)
    ulp = (torch.nextafter(wt.float().abs().to(dtype), torch.tensor(float("inf")).to(dtype)).float() - wt.float().abs())
    d = (g5.float() - wt.float()).abs()
    print(f"frd_input {dtype}: {int((d > 0).sum())} of {d.numel()} values differ from the rounded reference, max {float((d / ulp).max()):.2f} ulp")
    assert bool((d <= ulp).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("skip", [False, True])
def test_band_mean_against_fp64(dtype, skip):
    torch.manual_seed(0)
    x = (torch.randn((5, 64, 1024, 32), device=DEV) * 2).to(dtype)
    s = (torch.randn_like(x.float()) + 1).to(dtype) if skip else None
    got = ops.band_mean(x, s)
    t = x.double() + (s.double() if skip else 0)
    want = t.permute(0, 3, 1, 2).reshape(5, 32, 16, 4, 1024).mean((3, 4)).reshape(5, -1)
    err = ((got.double() - want).abs().max() / want.abs().max()).item()
    print(f"band_mean {dtype} skip={skip}: max err / max {err:.2e}")
    assert err < 4.5e-7                                           # measured at most 3.74e-7 (fp32 sums of 4096 pixels)
    assert torch.equal(got, ops.band_mean(x, s))


def test_moments_against_fp64_and_reproducible():
    g = torch.Generator().manual_seed(9)
    feat = (torch.randn((100, 512), generator=g) * 0.3 + 40.0).float()               # mean large against the spread
    st = M.FrechetStats(512, DEV).update(feat.to(DEV))
    mu, sigma = st.mu_sigma()
    f = feat.double().numpy()
    mu_w, sig_w = f.mean(0), np.cov(f, rowvar=False)
    e_mu = np.abs(mu - mu_w).max() / np.abs(mu_w).max()
    e_sig = np.abs(sigma - sig_w).max() / np.abs(sig_w).max()
    print(f"moments: mu rel err {e_mu:.2e}, sigma rel err {e_sig:.2e}")
    assert e_mu < 1e-15 and e_sig < 1e-15                          # measured 0 and 7.65e-16
    again = M.FrechetStats(512, DEV).update(feat.to(DEV))
    assert torch.equal(again.sum, st.sum) and torch.equal(again.cross, st.cross)    # bit for bit
    split = M.FrechetStats(512, DEV).update(feat[:64].to(DEV)).update(feat[64:].to(DEV))
    mu2, sig2 = split.mu_sigma()
    e = max(np.abs(mu2 - mu).max() / np.abs(mu).max(), np.abs(sig2 - sigma).max() / np.abs(sigma).max())
    print(f"moments: 64 + 36 against 100 rows rel diff {e:.2e}")
    assert e < 8e-16                                               # measured 6.56e-16


@pytest.fixture(scope="module")
def frd_weights():
    gd = golden()
    x = torch.stack([frd_ref.prepare(v) for v in golden_views()]).double()
    return frd_ref.seeded_state_dicts(int(gd["seeds"][0]), x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rangenet_features_against_golden(frd_weights, dtype):
    gd = golden()
    net = M.RangeNet.from_state_dicts(*frd_weights, dtype=dtype, device=DEV)
    got = net.features(torch.from_numpy(golden_views()).float()).cpu().double().numpy()          # batch 6
    want = gd["features"]
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"RangeNet features {dtype}: rel-L2 {err:.2e} against the reference model (fp64)")
    assert err < FEAT_BOUND[dtype]
    again = net.features(torch.from_numpy(golden_views()).float(), batch_size=4).cpu().double().numpy()   # 4 + 2
    assert np.array_equal(again, got)


@pytest.mark.parametrize("dtype", DTYPES)
def test_frd_end_to_end_and_files(frd_weights, dtype, tmp_path):
    gd = golden()
    views = torch.from_numpy(golden_views()).float()
    model = M.FRD.from_state_dicts(*frd_weights, dtype=dtype, device=DEV)
    got = model(views[:3], views[3:])
    f = gd["features"]
    stat = lambda a: (a.mean(0), np.cov(a, rowvar=False))
    want = M.frechet_distance(*stat(f[:3]), *stat(f[3:]))
    rel = abs(got - want) / abs(want)
    print(f"FRD {dtype}: engine {got:.6f} fp64 {want:.6f} rel err {rel:.2e}")
    assert rel < FRD_BOUND[dtype]
    for name, part in (("t", views[:3]), ("p", views[3:])):
        (tmp_path / name).mkdir()
        for i, v in enumerate(part):
            np.save(tmp_path / name / f"{i:03d}.npy", v.numpy())
    files = M.frd_paths(tmp_path / "t", tmp_path / "p", model)
    assert abs(files - got) <= 1e-12 * abs(got), (files, got)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fid_end_to_end_and_files(dtype, tmp_path):
    from PIL import Image
    sd = RR.clip_b32_state(31)
    a = (RR.clip_images("fid.a", 6) * 255).round() / 255
    b = ((RR.clip_images("fid.b", 8) * 0.6 + 0.35).clamp(0, 1) * 255).round() / 255
    model = M.FID(M.CLIPScore.from_state_dict(sd, dtype=dtype, device=DEV))
    got = model(a, b)
    ea, eb = RR.clip_embed(a, sd).numpy(), RR.clip_embed(b, sd).numpy()
    stat = lambda e: (e.mean(0), np.cov(e, rowvar=False))
    want = M.frechet_distance(*stat(ea), *stat(eb))
    rel = abs(got - want) / abs(want)
    print(f"FID {dtype}: engine {got:.6f} fp64 {want:.6f} rel err {rel:.2e}")
    assert rel < FID_BOUND[dtype]
    for name, part in (("t", a), ("p", b)):
        (tmp_path / name).mkdir()
        for i, im in enumerate(part):
            Image.fromarray((im.permute(1, 2, 0).numpy() * 255).round().astype(np.uint8)).save(tmp_path / name / f"{i:03d}.png")
    files = M.fid_paths(tmp_path / "t", tmp_path / "p", model)
    assert abs(files - got) <= 1e-9 * abs(got), (files, got)
