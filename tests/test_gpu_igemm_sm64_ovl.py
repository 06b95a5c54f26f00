"""The 64-deep-step small-m loop with its requests dealt out between the MFMAs (igemm_ring64_kernel, MOBI_IGEMM_SM64_OVL,
the default) at the smallest shapes at which that loop can go wrong.  Every case runs through ops.igemm / ops.linear with
the routing forced onto the kernel, and asserts (a) rel-L2 against an fp32 / fp64 torch reference within the family's TOL
of tests/test_gpu_ops.py and (b) bit equality with the same launch through the sequential step (MOBI_IGEMM_SM64_OVL=0):
the same MFMAs in the same k order, so the same sums and the same rounding."""
import pytest
import torch
import torch.nn.functional as F

from oracle import weights as W
from tests.test_gpu_ops import DT, SM_CASES, TOL, _conv_ref, rel, rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from mobi_amd import ops as o
    return o


def _both(tune, run):
    """run() on the overlapped loop and on the sequential one, both forced onto the 128 x 160 (128) tiles with 64-deep steps."""
    tune.setenv("MOBI_IGEMM_WM", "2")
    tune.setenv("MOBI_IGEMM_WIDE", "0")
    tune.setenv("MOBI_IGEMM_SMALL", "0")
    tune.setenv("MOBI_IGEMM_SM64", "1")
    tune.delenv("MOBI_IGEMM_SM64_OVL")
    y_ovl = run()
    tune.setenv("MOBI_IGEMM_SM64_OVL", "0")
    y_seq = run()
    return y_ovl, y_seq


def _check(y_ovl, y_seq, ref, dtype, what):
    assert torch.isfinite(y_ovl.float()).all(), what
    assert rel(y_ovl.float(), ref) < TOL[dtype], what
    assert torch.equal(y_ovl, y_seq), what


def _weights(name, cout, cin, k, dtype):
    wf = torch.from_numpy(W.synth_param(name + ".weight", (cout, cin, k, k))).to(dtype).float()
    return wf, torch.from_numpy(W.synth_param(name + ".bias", (cout,)))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("k", [64, 128, 192, 256])
def test_prologue_deeper_than_the_loop(ops, dtype, k, tune):
    """1 x 1 with 1 .. 4 steps under a three-step prologue: the requests past the k range are all-zero and land in slots
    nobody reads; m = 256 (two pixel tiles), n = 320 (two 160-wide tiles)."""
    name = f"ovl.pro{k}"
    xf, xd = rnd(name + ".x", (1, 16, 16, k), dtype)
    wf, bias = _weights(name, 320, k, 1, dtype)
    pw = ops.pack_conv(wf, bias, dtype, "cuda")
    y_ovl, y_seq = _both(tune, lambda: ops.igemm(xd, pw, split_k=1))
    _check(y_ovl, y_seq, _conv_ref(xf, wf, bias, 1, (0, 0)), dtype, k)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cout", [192, 128])
def test_ragged_column_tile(ops, dtype, cout, tune):
    """n = 192 on 160-wide tiles (weight rows at and beyond n_packed come back as zeros from beyond the descriptor) and n = 128
    (four 16-column MFMA tiles per wave)."""
    name = f"ovl.col{cout}"
    xf, xd = rnd(name + ".x", (2, 8, 16, 128), dtype)
    wf, bias = _weights(name, cout, 128, 1, dtype)
    pw = ops.pack_conv(wf, bias, dtype, "cuda")
    y_ovl, y_seq = _both(tune, lambda: ops.igemm(xd, pw, split_k=1))
    _check(y_ovl, y_seq, _conv_ref(xf, wf, bias, 1, (0, 0)), dtype, cout)


@pytest.mark.parametrize("dtype", DT)
def test_ragged_pixel_tile(ops, dtype, tune):
    """3 images of 8 x 8: 192 rows on 128-pixel tiles, 3 x 3 taps with padding on every side."""
    name = "ovl.pix"
    xf, xd = rnd(name + ".x", (3, 8, 8, 128), dtype)
    rf, rd = rnd(name + ".res", (3, 8, 8, 320), dtype)
    wf, bias = _weights(name, 320, 128, 3, dtype)
    pw = ops.pack_conv(wf, bias, dtype, "cuda")
    y_ovl, y_seq = _both(tune, lambda: ops.igemm(xd, pw, residual=rd, split_k=1))
    _check(y_ovl, y_seq, _conv_ref(xf, wf, bias, 1, (1, 1)) + rf, dtype, "ragged pixels")


@pytest.mark.parametrize("dtype", DT)
def test_uneven_last_split_range(ops, dtype, tune):
    """3 x 3, C = 320: 45 steps in 4 splits of 12, 12, 12 and 9; the fp32 slabs are compared too."""
    name = "ovl.split"
    xf, xd = rnd(name + ".x", (2, 8, 8, 320), dtype)
    wf, bias = _weights(name, 320, 320, 3, dtype)
    pw = ops.pack_conv(wf, bias, dtype, "cuda")
    y_ovl, y_seq = _both(tune, lambda: ops.igemm(xd, pw, split_k=4))
    _check(y_ovl, y_seq, _conv_ref(xf, wf, bias, 1, (1, 1)), dtype, "split")

    def slabs():
        d = ops.igemm(xd, pw, split_k=4, defer="keep")
        assert isinstance(d, ops.Deferred) and d.count == 4
        s = d.ws[: d.count * 128 * 320 * 4].clone()
        assert torch.equal(ops.finished(d), y_ovl)
        return s
    s_ovl, s_seq = _both(tune, slabs)
    assert torch.equal(s_ovl, s_seq)


@pytest.mark.parametrize("dtype", DT)
def test_two_sources_tap_changes_mid_ring(ops, dtype, tune):
    """3 x 3 over the un-materialised concat of 256 + 64 channels: five steps per tap, the source changes inside every tap."""
    name = "ovl.two"
    xf, xd = rnd(name + ".x", (2, 16, 16, 256), dtype)
    x2f, x2d = rnd(name + ".x2", (2, 16, 16, 64), dtype)
    wf, bias = _weights(name, 320, 320, 3, dtype)
    pw = ops.pack_conv(wf, bias, dtype, "cuda")
    y_ovl, y_seq = _both(tune, lambda: ops.igemm(xd, pw, x2=x2d, split_k=1))
    _check(y_ovl, y_seq, _conv_ref(torch.cat([xf, x2f], 3), wf, bias, 1, (1, 1)), dtype, "two sources")


@pytest.mark.parametrize("dtype", DT)
def test_per_group_weights(ops, dtype, tune):
    """groups = 2: 4 images x 64 tokens, C = 640; each half of the images times its own stacked matrix (w_group_stride)."""
    xf, xd = rnd("ovl.grp.x", (4, 64, 640), dtype)
    w0 = torch.from_numpy(W.synth_param("ovl.grp.w0", (640, 640))).to(dtype).float()
    w1 = torch.from_numpy(W.synth_param("ovl.grp.w1", (640, 640))).to(dtype).float()
    pw = ops.pack_linear(torch.cat([w0, w1], 0), None, dtype, "cuda")
    y_ovl, y_seq = _both(tune, lambda: ops.linear(xd, pw, groups=2, split_k=1))
    ref = torch.cat([xf[:2] @ w0.t(), xf[2:] @ w1.t()], 0)
    _check(y_ovl, y_seq, ref, dtype, "groups")


@pytest.mark.parametrize("dtype", DT)
def test_transposed_output(ops, dtype, tune):
    """MOBI_OUT_TRANSPOSED: the operands swap places in the MFMA."""
    from mobi_amd._lib import OUT_TRANSPOSED
    name = "ovl.tr"
    xf, xd = rnd(name + ".x", (2, 192, 192), dtype)                # 192 tokens per image: ragged pixel tiles
    wf, bias = _weights(name, 320, 192, 1, dtype)
    pw = ops.pack_linear(wf[:, :, 0, 0], bias, dtype, "cuda")
    y_ovl, y_seq = _both(tune, lambda: ops.linear(xd, pw, out_mode=OUT_TRANSPOSED, split_k=1))
    assert y_ovl.shape == (2, 320, 192)
    ref = (xf @ wf[:, :, 0, 0].t() + bias).transpose(1, 2)
    _check(y_ovl, y_seq, ref, dtype, "transposed")


@pytest.mark.parametrize("dtype", DT)
def test_layernorm_fold(ops, dtype, tune):
    """Linear(LayerNorm(x)) as one launch, 512 rows, C = 320 -> 960, rows whose |mean| is far above their spread: the row
    statistics come from the activation fragments (their v_dot2c ride in the first MFMA group of each k half)."""
    n, t, c, n_out, eps = 2, 256, 320, 960, 1e-5
    xf, _ = rnd("ovl.lnf.x", (n, t, c), dtype, scale=0.25)
    xd = (xf + 6.0).to(dtype).cuda()
    x64 = xd.double().cpu()
    w = torch.from_numpy(W.synth_param("ovl.lnf.w", (n_out, c)))
    b = torch.from_numpy(W.synth_param("ovl.lnf.b", (n_out,)))
    gamma = 1.0 + 0.3 * torch.from_numpy(W.synth_param("ovl.lnf.g", (c,))) * c ** 0.5 * 0.1
    beta = torch.from_numpy(W.synth_param("ovl.lnf.be", (c,))) * 2.0
    wf, bf = ops.fold_layernorm(w, b, gamma, beta)
    pw = ops.with_row_sums(ops.pack_linear(wf, bf, dtype, "cuda"), eps)
    y_ovl, y_seq = _both(tune, lambda: ops.linear(xd, pw))
    wr = wf.to(dtype).double()
    mean, var = x64.mean(-1, keepdim=True), x64.var(-1, unbiased=False, keepdim=True)
    ref = (x64 @ wr.t() - mean * wr.sum(1)) / torch.sqrt(var + eps) + bf.double()
    _check(y_ovl, y_seq, ref.float(), dtype, "LayerNorm fold")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("direct", ["1", "0"])
@pytest.mark.parametrize("case", SM_CASES, ids=[f"sm{i}" for i in range(len(SM_CASES))])
def test_epilogue_forms(ops, dtype, case, direct, tune):
    """The forms of test_igemm_ring128_epilogues at their sizes (residual + per-image vector, bias + residual, two sources,
    GEGLU, split-K slabs, 128-wide tiles), with the register epilogue / register slab stores and with the LDS-staged epilogue
    (which takes over the ring once it has drained)."""
    n, h, w, cin, cin2, cout, k, res, rowvec, geglu, split = case
    name = "sm." + ".".join(str(v) for v in case)
    xf, xd = rnd(name + ".x", (n, h, w, cin), dtype)
    x2f, x2d = rnd(name + ".x2", (n, h, w, cin2), dtype) if cin2 else (None, None)
    wf = torch.from_numpy(W.synth_param(name + ".weight", ((2 if geglu else 1) * cout, cin + cin2, k, k))).to(dtype).float()
    bias = torch.from_numpy(W.synth_param(name + ".bias", ((2 if geglu else 1) * cout,)))
    rf, rd = rnd(name + ".res", (n, h, w, cout), dtype) if res else (None, None)
    rv = W.synth_input(name + ".rv", (n, cout)) if rowvec else None
    ref = _conv_ref(xf if x2f is None else torch.cat([xf, x2f], 3), wf, None if rowvec else bias, 1, (k // 2, k // 2))
    if geglu:
        a_, g_ = ref.chunk(2, dim=-1)
        ref = a_ * F.gelu(g_)
    if rv is not None:
        ref = ref + rv[:, None, None, :]
    if rf is not None:
        ref = ref + rf
    tune.setenv("MOBI_IGEMM_SM_DIRECT", direct)

    def run():
        if geglu:
            return ops.linear(xd.view(n, h * w, cin), ops.pack_geglu(wf[:, :, 0, 0], bias, dtype, "cuda")).view(n, h, w, cout)
        pw = ops.pack_conv(wf, None if rowvec else bias, dtype, "cuda")
        return ops.igemm(xd, pw, x2=x2d, residual=rd, rowvec=None if rv is None else rv.cuda(), rowvec_has_bias=rowvec,
                         split_k=split)
    y_ovl, y_seq = _both(tune, run)
    _check(y_ovl, y_seq, ref, dtype, (case, direct))
