"""GPU parity of every normalisation path on the data where statistics go wrong: a common offset far larger than the spread
(|mean| / std = 16, 128), a variance close to eps, and constant images / groups / rows (the range images' -1 fill of pixels
without a return, ldm/data/lidar_converter.py; a non-dyadic constant whose fp32 sums round).

Every path is compared with a float64 torch reference on the same storage-rounded inputs, at the tolerance its own test in
test_gpu_ops.py / test_gpu_backward.py already holds it to.  Constant data must in addition stay finite and reproduce the
constant's output (beta, silu(beta), ...) to 2 ulps of the storage type, and the small-variance case is run a second time with
4 eps to show the comparison would notice eps being mishandled.

Measured on the MI355X (about 30 s): before the statistics were made shift-safe, 41 cases failed -- fp32-source
GroupNorm at offset 128 3.9e-4 against 2e-6, the two-launch GroupNorm of two sources at offset 128 1.5e-3 against 5e-4 (fp16),
GroupNorm backward of a constant group 5.2e-2 against 8e-4, layernorm_rows_f32 at offset 128 6.2e-6 against 2e-6, constant groups
50 - 2800 ulps off beta.

Worst rel-L2 measured on the MI355X after the fix, over every regime a test holds (fp16 / bf16; the 4 eps runs excluded):
  GroupNorm forward, every form                2.1e-4 / 1.7e-3     (fp32 outputs <= 2.5e-6: the bf16 hi + lo pair, limit 2e-5)
  GroupNorm -> scale / shift                   5.4e-6 / 5.1e-6     (x scale + shift in fp64)
  LayerNorm, LayerNorm fold (to offset 16)     2.1e-4 / 1.7e-3
  layernorm_rows_f32                           8.7e-8 (fp32)
  two-key adapter, chain adapter               2.2e-4 / 1.8e-3
  chain rowstats + folded product              6.2e-4 / 2.3e-3     (limit 1.5 TOL)
  GroupNorm / LayerNorm backward               2.1e-4 / 1.7e-3
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import weights as W
from tests.test_gpu_ops import DT, TOL, rel, rnd  # noqa: F401  (rnd: the storage rounding every other parity test uses)
from tests.test_gpu_backward import TOL1

pytestmark = pytest.mark.gpu

EPS_UNET, EPS_VAE = 1e-5, 1e-6
TOL_F32 = 2e-6                      # fp32 outputs (test_groupnorm_fp32_source_and_precise_outputs)
OFFSETS = (16.0, 128.0)
REGIMES = ["centred", "off16", "off128", "small", "small_off", "const"]
CONST = 10.3                        # rounded to the storage type: a value whose fp32 sums round


@pytest.fixture(scope="module")
def ops():
    from mobi_amd import ops as o
    return o


def _z(name, shape):
    return W.synth_input(name, shape).double()


def regime_data(regime, name, shape, eps, group_dims=None):
    """fp64 data of one regime, NOT yet rounded; the mask marks the constant elements (or None).
    shape (N, ..., C); group_dims: channels per group for GroupNorm (None: LayerNorm rows)."""
    z = _z(name, shape)
    mask = None
    if regime == "centred":
        x = z
    elif regime.startswith("off"):
        x = float(regime[3:]) + z
    elif regime == "small":
        x = 2.0 * math.sqrt(eps) * z
    elif regime == "small_off":
        s = 2.0 * math.sqrt(eps)
        x = s * (8.0 + z)
    elif regime == "const":
        x = z.clone()
        mask = torch.zeros(shape, dtype=torch.bool)
        mask[0] = True                                              # a whole image / the first rows: the range images' fill
        if group_dims is None:
            mask[1, :3] = True
        else:
            mask[1, ..., 3 * group_dims:4 * group_dims] = True      # one group inside an ordinary image
        x[0] = -1.0
        x[mask & (torch.arange(shape[0]).view(-1, *[1] * (len(shape) - 1)) > 0)] = CONST
    else:
        raise ValueError(regime)
    return x, mask


def stored(x, dtype):
    """(fp64 cpu copy of the rounded values, device tensor of the storage type)."""
    xt = x.to(dtype)
    return xt.double(), xt.cuda()


def ulp(v, dtype):
    bits, tiny = {torch.float16: (10, 2.0 ** -14), torch.bfloat16: (7, 2.0 ** -126)}[dtype]
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(tiny))) - bits)


def judge(y, ref, dtype, tol, mask=None, what="", slack=None, const_rel=False):
    """y (any device / type) against the fp64 reference; constant elements, where marked, to 2 ulps (16-bit) or to the fp32
    criteria; the rest to the path's tolerance.  Returns the rel-L2 of the ordinary elements."""
    y = y.detach().double().cpu()
    ref = ref.double()
    assert y.shape == ref.shape, what
    assert bool(torch.isfinite(y).all()), f"{what}: NaN / Inf"
    if mask is None:
        err = rel(y, ref)
        assert err < tol, (what, err)
        return err
    mask = mask.expand_as(y) if mask.shape != y.shape else mask
    yc, rc = y[mask], ref[mask]
    from tests.golden_cases import record
    if dtype == torch.float32:
        ec = rel(yc, rc)
        assert ec < TOL_F32, (what, "constant", ec)
        assert float((yc - rc).abs().max()) <= 1e-5 * float(rc.abs().max()), (what, "constant max")
    elif const_rel:
        ec = rel(yc, rc)
        assert ec < tol, (what, "constant", ec)
    else:
        allow = ulp(rc, dtype) if slack is None else ulp(rc, dtype) + slack.expand_as(y)[mask] / 2
        in_ulps = (yc - rc).abs() / allow
        record("const_ulps", float(in_ulps.max()))
        bad = in_ulps > 2
        assert not bool(bad.any()), (what, "constant", float((yc - rc).abs().max()), int(bad.sum()))
    err = rel(y[~mask], ref[~mask])
    assert err < tol, (what, err)
    return err


def sensitive(y4, ref, tol, what=""):
    """the same call with 4 eps: the comparison must see it (error above 10x the tolerance)"""
    err = rel(y4.detach().double().cpu(), ref.double())
    assert err > 10 * tol, (what, "eps insensitive", err)


# ---------------------------------------------------------------------------------------------
# GroupNorm forward, 16-bit sources.  (path, c0, c1, hw, knobs); N = 2 images, silu on.
GN_PATHS = [
    ("regs", 320, 0, 1024, {}),
    ("regs_2src", 1280, 640, 64, {}),
    ("lds", 320, 0, 256, {"MOBI_GN_FUSED": "1"}),
    ("two_launch", 640, 0, 1024, {"MOBI_GN_FUSED": "0"}),
    ("two_launch_2src", 1280, 640, 256, {"MOBI_GN_FUSED": "0"}),
    ("regs_64x64_640", 640, 0, 4096, {}),          # the 64 x 64 level's 640-channel input: the router takes registers
    ("coop", 320, 0, 1024, {"MOBI_GN_COOP": "1"}),
    ("coop_1280", 1280, 0, 256, {"MOBI_GN_COOP": "1"}),
]


def _gn_ref(x64, g, b, eps, silu=True):
    ref = F.group_norm(x64.permute(0, 3, 1, 2), 32, g.double(), b.double(), eps).permute(0, 2, 3, 1)
    return F.silu(ref) if silu else ref


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("path", GN_PATHS, ids=[p[0] for p in GN_PATHS])
def test_groupnorm_paths(ops, dtype, regime, path, tune):
    name, c0, c1, hw, knobs = path
    for k, v in knobs.items():
        tune.setenv(k, v)
    h = int(math.isqrt(hw))
    C = c0 + c1
    eps = EPS_UNET
    x, mask = regime_data(regime, f"ns.gn.{name}", (2, h, hw // h, C), eps, C // 32)
    x64, xd = stored(x, dtype)
    x0, x1 = (xd[..., :c0].contiguous(), xd[..., c0:].contiguous()) if c1 else (xd, None)
    g = torch.from_numpy(W.synth_param(f"ns.gn{C}.weight", (C,)))
    b = torch.from_numpy(W.synth_param(f"ns.gn{C}.bias", (C,)))
    ref = _gn_ref(x64, g, b, eps)
    y = ops.groupnorm(x0, g.cuda(), b.cuda(), eps, True, x2=x1)
    slack = None
    if name.startswith("regs") and mask is not None:
        # gn_regs_kernel applies y = x sc + (beta - mean sc) (norm.hip): on a constant group (rstd = 1 / sqrt(eps)) the fp32
        # rounding of x sc and of the shift, 2^-24 |x sc| each, is part of its contract; the other forms give beta exactly
        xg = x64.view(2, -1, 32, C // 32)
        sc = (g.double().view(32, -1) / torch.sqrt(xg.var((1, 3), unbiased=False) + eps)[..., None]).reshape(2, 1, 1, C)
        slack = 2.0 ** -23 * (x64 * sc).abs()
    judge(y, ref, dtype, TOL[dtype], mask, f"{name}/{regime}", slack)
    if regime == "small":
        sensitive(ops.groupnorm(x0, g.cuda(), b.cuda(), 4 * eps, True, x2=x1), ref, TOL[dtype], name)
    if name.startswith("coop"):
        torch.cuda.synchronize()
        assert all(int(buf.abs().sum()) == 0 for buf in ops._SYNC.values())


# ---------------------------------------------------------------------------------------------
# The two-launch form of the fp32 source / precise outputs (VAE decoder streams, lidar tail): eps 1e-6.
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("regime", REGIMES)
def test_groupnorm_fp32_source_paths(ops, dtype, regime):
    n, side, c = 2, 32, 128
    eps = EPS_VAE
    x, mask = regime_data(regime, "ns.gn32", (n, side, side, c), eps, c // 32)
    x = x.float()
    xd = x.cuda()
    g = torch.from_numpy(W.synth_param("ns.gn32.weight", (c,)))
    b = torch.from_numpy(W.synth_param("ns.gn32.bias", (c,)))
    ref = _gn_ref(x.double(), g, b, eps)
    y32 = ops.groupnorm(xd, g.cuda(), b.cuda(), eps, True, out_mode=ops.GN_OUT_F32, dtype=dtype)
    judge(y32, ref, torch.float32, TOL_F32, mask, f"f32 out/{regime}")
    y = ops.groupnorm(xd, g.cuda(), b.cuda(), eps, True, dtype=dtype)
    judge(y, ref, dtype, TOL[dtype], mask, f"T out/{regime}")
    pair = ops.groupnorm(xd, g.cuda(), b.cuda(), eps, True, out_mode=ops.GN_OUT_SPLIT, dtype=dtype)
    assert torch.equal(pair[..., :c], y32.to(dtype))
    both = pair[..., :c].double() + pair[..., c:].double()
    judge(both, y32.cpu(), torch.float32, 2e-6 if dtype == torch.float16 else 2e-5, None, f"hi+lo/{regime}")
    tri = ops.groupnorm(xd, g.cuda(), b.cuda(), eps, True, out_mode=ops.GN_OUT_SPLIT3, dtype=dtype)
    assert torch.equal(tri[..., :2 * c], pair)
    # a 16-bit source through the same kernels, fp32 out
    xs64, xs = stored(x.double(), dtype)
    judge(ops.groupnorm(xs, g.cuda(), b.cuda(), eps, True, out_mode=ops.GN_OUT_F32), _gn_ref(xs64, g, b, eps), torch.float32,
          TOL_F32, mask, f"T src f32 out/{regime}")
    if regime == "small":
        sensitive(ops.groupnorm(xd, g.cuda(), b.cuda(), 4 * eps, True, out_mode=ops.GN_OUT_F32, dtype=dtype), ref, TOL_F32)


# ---------------------------------------------------------------------------------------------
# GroupNorm -> per-image (scale, shift) of the chain's GroupNorm fold; the consumer computes x * scale + shift
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("regime", REGIMES)
def test_groupnorm_scale_shift(ops, dtype, regime):
    n, side, c = 2, 16, 320
    eps = EPS_UNET
    x, mask = regime_data(regime, "ns.gnss", (n, side, side, c), eps, c // 32)
    x64, xd = stored(x, dtype)
    g = torch.from_numpy(W.synth_param("ns.gnss.weight", (c,)))
    b = torch.from_numpy(W.synth_param("ns.gnss.bias", (c,)))
    sc, sh = ops.groupnorm_scale_shift(xd, g.cuda(), b.cuda(), eps)
    xg = x64.view(n, -1, 32, c // 32)
    var = xg.var((1, 3), unbiased=False)
    sc_ref = (g.double().view(32, -1) / torch.sqrt(var + eps)[..., None]).reshape(n, c)
    assert bool(torch.isfinite(sc).all() and torch.isfinite(sh).all())
    # the scale carries rstd: to fp32 statistics' accuracy whatever the offset (1e-5 elementwise)
    assert float(((sc.double().cpu() - sc_ref).abs() / sc_ref.abs()).max()) < 1e-5, regime
    got = x64 * sc.double().cpu()[:, None, None, :] + sh.double().cpu()[:, None, None, :]
    ref = _gn_ref(x64, g, b, eps, silu=False)
    # x * scale + shift cancels in the format itself: shift = beta - mean * scale is one fp32 number, so y carries ~|mean scale|
    # 2^-24 of absolute error whatever the statistics (at rstd = 1 / sqrt(eps) on a constant group, or a large offset).  The
    # ordinary elements are held to test_gpu_chain's 1e-5 plus the offset's share; the constant ones to that limit of the format
    off = float(x64.abs().mean() / x64.std().clamp_min(1e-30)) if regime.startswith("off") else 0.0
    keep = torch.ones_like(ref, dtype=torch.bool) if mask is None else ~mask
    assert rel(got[keep], ref[keep]) < 1e-5 + 2 * off * 2.0 ** -24, regime
    if mask is not None:
        lim = 2.0 ** -23 * (x64 * sc.double().cpu()[:, None, None, :]).abs() + 2.0 ** -24 * ref.abs()
        assert bool(((got - ref).abs() <= lim + 1e-12)[mask].all()), regime
    if regime == "small":
        sc4, _ = ops.groupnorm_scale_shift(xd, g.cuda(), b.cuda(), 4 * eps)
        assert float(((sc4.double().cpu() - sc_ref).abs() / sc_ref.abs()).max()) > 0.1


# ---------------------------------------------------------------------------------------------
# LayerNorm: 16-bit rows (layernorm_kernel, incl. a batch-strided view) and fp32 rows (the text encoder's)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("n,t,c,strided", [(4, 100, 640, True), (2, 77, 1280, False), (2, 64, 320, False)])
def test_layernorm_paths(ops, dtype, regime, n, t, c, strided):
    eps = EPS_UNET
    x, mask = regime_data(regime, f"ns.ln{c}", (n, t, c), eps)
    x64, xd = stored(x, dtype)
    g = torch.from_numpy(W.synth_param(f"ns.ln{c}.weight", (c,)))
    b = torch.from_numpy(W.synth_param(f"ns.ln{c}.bias", (c,)))
    view = xd
    if strided:                                                     # every other image of a batch: rows 2 * t * c apart
        full = torch.zeros((2 * n, t, c), dtype=dtype, device="cuda")
        full[1::2] = xd
        view = full[1::2]
    ref = F.layer_norm(x64, (c,), g.double(), b.double(), eps)
    judge(ops.layernorm(view, g.cuda(), b.cuda(), eps), ref, dtype, TOL[dtype], mask, f"ln/{regime}")
    if regime == "small":
        sensitive(ops.layernorm(view, g.cuda(), b.cuda(), 4 * eps), ref, TOL[dtype])


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("rows,cols", [(154, 768), (64, 1024)])
def test_layernorm_rows_f32(ops, regime, rows, cols):
    eps = EPS_UNET
    x, mask = regime_data(regime, f"ns.lnf32.{cols}", (2, rows // 2, cols), eps)
    x, mask = x.float().reshape(rows, cols), None if mask is None else mask.reshape(rows, cols)
    g = torch.from_numpy(W.synth_param(f"ns.lnf32.{cols}.weight", (cols,)))
    b = torch.from_numpy(W.synth_param(f"ns.lnf32.{cols}.bias", (cols,)))
    ref = F.layer_norm(x.double(), (cols,), g.double(), b.double(), eps)
    judge(ops.layernorm_rows_f32(x.cuda(), g.cuda(), b.cuda(), eps), ref, torch.float32, TOL_F32, mask, f"ln f32/{regime}")
    if regime == "small":
        sensitive(ops.layernorm_rows_f32(x.cuda(), g.cuda(), b.cuda(), 4 * eps), ref, TOL_F32)


# ---------------------------------------------------------------------------------------------
# LayerNorm folded into the GEMM (mobi_igemm_params.ln_svec): the LN_FOLD_CASES geometries of test_gpu_ops.py
LNF = [
    (2, 100, 320, 960, False),        # ragged tiles, LDS-staged epilogue
    (4, 1024, 640, 1280, True),       # 256 x 320 ring tiles, GEGLU register epilogue
    (4, 256, 1280, 3840, False),      # 128 x 160 ring tiles
]


# The fold's row statistics are one fp32 pass of sum x and sum x^2 over the A fragments (igemm.hip rowstat_acc / ln_fold_acc),
# and rstd (acc - mean s) cancels in fp32: it meets the LayerNorm tolerance up to |mean| / std = 16 only.  The two regimes it
# does not meet stay in the suite as expected failures, with what they measured: at 128, 7.2e-4 / 8.5e-4 against 5e-4 (fp16,
# lnf1 / lnf2); constant rows up to 250 ulps (fp16) and ~30 absolute (bf16, lnf1) off W beta + b -- the spurious variance
# times rstd = 1 / sqrt(eps).  Open: a shift-safe fold.
_LNF_OPEN = pytest.mark.xfail(reason="one-pass fp32 row statistics of the GEMM LayerNorm fold (igemm.hip rowstat_acc)",
                              strict=False)
LNF_REGIMES = ["centred", "off16", pytest.param("off128", marks=_LNF_OPEN), "small", "small_off",
               pytest.param("const", marks=_LNF_OPEN)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("regime", LNF_REGIMES)
@pytest.mark.parametrize("case", LNF, ids=[f"lnf{i}" for i in range(len(LNF))])
def test_layernorm_fold(ops, dtype, regime, case):
    n, t, c, n_out, geglu = case
    eps = EPS_UNET
    x, mask = regime_data(regime, f"ns.lnf{c}", (n, t, c), eps)
    x64, xd = stored(x, dtype)
    rows = n_out * (2 if geglu else 1)
    w = torch.from_numpy(W.synth_param("lnf.w", (rows, c)))
    b = torch.from_numpy(W.synth_param("lnf.b", (rows,)))
    gamma = 1.0 + 0.3 * torch.from_numpy(W.synth_param("lnf.g", (c,))) * c ** 0.5 * 0.1
    beta = torch.from_numpy(W.synth_param("lnf.be", (c,))) * 2.0
    wf, bf = ops.fold_layernorm(w, b, gamma, beta)
    pack = ops.pack_geglu if geglu else ops.pack_linear
    wr = wf.to(dtype).double()

    def ref_of(e):
        mean, var = x64.mean(-1, keepdim=True), x64.var(-1, unbiased=False, keepdim=True)
        pre = (x64 - mean) / torch.sqrt(var + e) @ wr.t() + bf.double()
        return pre[..., :n_out] * F.gelu(pre[..., n_out:]) if geglu else pre

    ref = ref_of(eps)
    y = ops.linear(xd, ops.with_row_sums(pack(wf, bf, dtype, "cuda"), eps))
    rmask = None if mask is None else mask[..., :1]
    judge(y, ref, dtype, TOL[dtype], rmask, f"lnf/{regime}")
    if regime == "small":
        sensitive(ops.linear(xd, ops.with_row_sums(pack(wf, bf, dtype, "cuda"), 4 * eps)), ref, TOL[dtype])


# ---------------------------------------------------------------------------------------------
# The two-key (bbox) adapter: LayerNorm statistics of each token row, per-head gates, gated per-image vectors; and its
# second result, LayerNorm of the updated rows (ln_pair).
TKA_FORMS = [("default", None), ("vector", "0"), ("lds_tile", "1")]


def _tka_ref(x64, a, u, b, cc, eps):
    mean = x64.mean(-1, keepdim=True)
    xc = x64 - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    z = rstd * torch.einsum("ntc,nhc->nth", xc, a.double()) + cc.double()[:, None, :]
    return x64 + b.double()[:, None, :] + torch.einsum("nth,nhc->ntc", torch.sigmoid(z), u.double())


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("n,t,c", [(4, 100, 320), (2, 64, 640), (2, 37, 1280)])
def test_two_key_adapter_paths(ops, dtype, regime, n, t, c, tune):
    eps = EPS_UNET
    name = f"ns.tka.{n}.{t}.{c}"
    x, mask = regime_data(regime, name + ".x", (n, t, c), eps)
    x64, xd = stored(x, dtype)
    a = W.synth_input(name + ".a", (n, 8, c)) * 0.05
    u = W.synth_input(name + ".u", (n, 8, c))
    b = W.synth_input(name + ".b", (n, c))
    cc = W.synth_input(name + ".c", (n, 8))
    gb = [(torch.from_numpy(W.synth_param(f"{name}.g{i}", (c,))), torch.from_numpy(W.synth_param(f"{name}.b{i}", (c,))))
          for i in range(2)]
    ref = _tka_ref(x64, a, u, b, cc, eps)
    args = (a.cuda(), a.sum(-1).contiguous().cuda(), cc.cuda(), u.cuda(), b.cuda())
    for form, knob in TKA_FORMS:
        if knob is not None:
            tune.setenv("MOBI_TKA_MFMA", knob)
        y = ops.two_key_adapter(xd, *args, eps)
        # the gate's argument is computed folded, rstd (x . a - mean sum(a)) + c: on a constant row (rstd = 1 / sqrt(eps)) the
        # fp32 cancellation of the two products is amplified ~316x whatever the statistics (measured up to 4.4e-3 / 5.1e-2
        # absolute, fp16 / bf16, on outputs near zero).  Constant rows are held to the path's rel-L2 tolerance, not to 2 ulps.
        judge(y, ref, dtype, TOL[dtype], mask, f"tka {form}/{regime}", const_rel=True)
        if regime == "small":
            # x dominates the output; the gates are what eps changes: judge them through y - x
            d4 = ops.two_key_adapter(xd, *args, 4 * eps).double().cpu() - x64
            err = rel(d4, ref - x64)
            assert err > 10 * TOL[dtype], (form, err)
        if ops.two_key_adapter_fuses_ln(c, n * t):
            y2, (l0, l1) = ops.two_key_adapter(xd, *args, eps, ln_pair=((gb[0][0].cuda(), gb[0][1].cuda()),
                                                                        (gb[1][0].cuda(), gb[1][1].cuda()), eps))
            assert torch.equal(y2, y)
            for got, half, (g_, b_) in ((l0, y[0::2], gb[0]), (l1, y[1::2], gb[1])):
                want = F.layer_norm(half.double().cpu(), (c,), g_.double(), b_.double(), eps)
                judge(got, want, dtype, TOL[dtype], None, f"tka ln_pair {form}/{regime}")


# ---------------------------------------------------------------------------------------------
# Backward: GroupNorm (three coalesced passes; one block per (image, group)) and LayerNorm, dx against fp64 autograd
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("c,hw", [(320, 256), (128, 100)])
def test_groupnorm_backward_paths(ops, dtype, regime, c, hw):
    n, side = 2, int(math.isqrt(hw))
    eps = EPS_UNET
    x, mask = regime_data(regime, f"ns.gnb{c}", (n, side, side, c), eps, c // 32)
    x64, xd = stored(x, dtype)
    dy64, dyd = stored(_z(f"ns.gnb.dy{c}", (n, side, side, c)), dtype)
    g = torch.from_numpy(W.synth_param(f"ns.gnb{c}.weight", (c,)))
    b = torch.from_numpy(W.synth_param(f"ns.gnb{c}.bias", (c,)))

    def ref_of(e):
        xr = x64.clone().requires_grad_(True)
        F.silu(F.group_norm(xr.permute(0, 3, 1, 2), 32, g.double(), b.double(), e)).backward(dy64.permute(0, 3, 1, 2))
        return xr.grad

    ref = ref_of(eps)
    for obg in (False, True):
        dx = ops.groupnorm_bwd(xd, dyd, g.cuda(), b.cuda(), eps, True, one_block_per_group=obg)
        judge(dx, ref, dtype, TOL1[dtype], None, f"gn bwd obg={obg}/{regime}")
        if regime == "small":
            sensitive(ops.groupnorm_bwd(xd, dyd, g.cuda(), b.cuda(), 4 * eps, True, one_block_per_group=obg), ref, TOL1[dtype])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("n,t,c", [(2, 64, 320), (2, 77, 1280)])
def test_layernorm_backward_paths(ops, dtype, regime, n, t, c):
    eps = EPS_UNET
    x, mask = regime_data(regime, f"ns.lnb{c}", (n, t, c), eps)
    x64, xd = stored(x, dtype)
    dy64, dyd = stored(_z(f"ns.lnb.dy{c}", (n, t, c)), dtype)
    g = torch.from_numpy(W.synth_param(f"ns.lnb{c}.weight", (c,)))
    xr = x64.clone().requires_grad_(True)
    F.layer_norm(xr, (c,), g.double(), None, eps).backward(dy64)
    dx, _, _ = ops.layernorm_bwd(xd, dyd, g.cuda(), eps)
    judge(dx, xr.grad, dtype, TOL1[dtype], None, f"ln bwd/{regime}")
    if regime == "small":
        sensitive(ops.layernorm_bwd(xd, dyd, g.cuda(), 4 * eps)[0], xr.grad, TOL1[dtype])


# ---------------------------------------------------------------------------------------------
# The row chain (csrc/chain.hip, 320-channel token rows): the adapter operation (the bbox adapter's route at large row counts,
# ldm/modules/attention.py) and rowstats + a LayerNorm-folded product (norm -> projection of a transformer block)
CH = 320


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("regime", REGIMES)
def test_chain_adapter_paths(ops, dtype, regime):
    n, t, eps = 2, 256, EPS_UNET
    name = "ns.chain.a"
    x, mask = regime_data(regime, name + ".x", (n, t, CH), eps)
    x64, xd = stored(x, dtype)
    a = W.synth_input(name + ".a", (n, 8, CH)) * 0.05
    u = W.synth_input(name + ".u", (n, 8, CH))
    b = W.synth_input(name + ".b", (n, CH))
    cc = W.synth_input(name + ".c", (n, 8))
    ref = _tka_ref(x64, a, u, b, cc, eps)
    image = ops.chain_adapter_image(a.cuda(), cc.cuda(), u.cuda(), b.cuda(), dtype)

    def run(e):
        out = torch.empty_like(xd)
        ops.row_chain([ops.ChainProgram().load(xd, "s").adapter(dst=out)], n, t, dtype, adapter=(image, e))
        return out

    # constant rows: the folded gate, as in test_two_key_adapter_paths
    judge(run(eps), ref, dtype, TOL[dtype], mask, f"chain adapter/{regime}", const_rel=True)
    if regime == "small":
        err = rel(run(4 * eps).double().cpu() - x64, ref - x64)
        assert err > 10 * TOL[dtype], err


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("regime", REGIMES)
def test_chain_rowstats_fold_paths(ops, dtype, regime):
    n, t, eps = 2, 256, EPS_UNET
    name = "ns.chain.f"
    x, mask = regime_data(regime, name + ".x", (n, t, CH), eps)
    x64, xd = stored(x, dtype)
    w = torch.from_numpy(W.synth_param(name + ".w.weight", (CH, CH)))
    b = torch.from_numpy(W.synth_param(name + ".w.bias", (CH,)))
    g = torch.from_numpy(W.synth_param(name + ".ln.weight", (CH,)))
    bt = torch.from_numpy(W.synth_param(name + ".ln.bias", (CH,)))
    cw = ops.pack_chain_weight(w, b, dtype, "cuda", ln=(g, bt), scale=0.25)

    def run(e):
        q = torch.empty_like(xd)
        ops.row_chain([ops.ChainProgram().load(xd, "s").rowstats(e).product(cw, fold=True, dst=q)], n, t, dtype)
        return q

    ref = F.linear(F.layer_norm(x64, (CH,), g.double(), bt.double(), eps), w.double() * 0.25, b.double() * 0.25)
    # test_chain_layernorm_fold's tolerance (the packed W diag(gamma) is rounded to the storage type; the reference is not);
    # constant rows give W beta + b through the fold's rs * acc + cs * s, held to the same rel-L2
    judge(run(eps), ref, dtype, TOL[dtype] * 1.5, None if mask is None else mask[..., :1], f"chain fold/{regime}",
          const_rel=True)
    if regime == "small":
        sensitive(run(4 * eps), ref, TOL[dtype] * 1.5)
