"""The launch shadow's own references and metric (tests/launch_shadow.py), on the CPU: every igemm reference form against
F.conv2d / F.linear in fp64, the other references against torch's fp64 ops, the ff_geglu chunk-image decode against the
packer, and the metric passing a merely storage-rounded result while failing a dropped k-chunk tile, a NaN row and a write
outside a strided view."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import launch_shadow as ls
from tests.test_gpu_ops import TOL

DT = [torch.float16, torch.bfloat16]


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64) * scale


def _op(x, w, bias=None, x2=None, stride=1, pad=None, upsample=False, hout=None, wout=None, rowvec=None, rowvec_has_bias=False,
        residual=None, scale=1.0, groups=1, geglu=False, ln_eps=None, cout=None):
    """x NHWC, w OIHW (fp64) -> the shadow's igemm operand record, weights packed k = tap * C + c as ops.pack_conv does."""
    o, i, kh, kw = w.shape
    src_w = (x.shape[2] * 2 if upsample else x.shape[2], x.shape[1] * 2 if upsample else x.shape[1])
    ph, pw = (kh // 2, kw // 2) if pad is None else pad
    ho = (src_w[1] + 2 * ph - kh) // stride + 1 if hout is None else hout
    wo = (src_w[0] + 2 * pw - kw) // stride + 1 if wout is None else wout
    npk = o // groups
    return dict(x=x, x2=x2, w=w.permute(0, 2, 3, 1).reshape(o, kh * kw * i), bias=bias, kh=kh, kw=kw, stride=stride, pad_h=ph,
                pad_w=pw, upsample=upsample, hout=ho, wout=wo, cout=cout or npk, n_packed=npk, groups=groups, geglu=geglu,
                ln=ln_eps is not None, ln_eps=ln_eps or 0.0, scale=scale, rowvec=rowvec, rowvec_has_bias=rowvec_has_bias,
                residual=residual)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _flat(t):
    return t.reshape(t.shape[0], -1, t.shape[-1])


CONV_CASES = [
    # name, cin, cout, k, h, w, stride, upsample
    ("c3", 32, 48, 3, 9, 7, 1, False),
    ("c1", 64, 40, 1, 6, 5, 1, False),
    ("c3_s2", 32, 32, 3, 8, 8, 2, False),
    ("c3_up", 32, 16, 3, 5, 4, 1, True),
    ("c15", 32, 24, (1, 5), 4, 9, 1, False),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_igemm_reference_conv_forms(case):
    name, cin, cout, k, h, w, stride, up = case
    kh, kw = (k, k) if isinstance(k, int) else k
    x = _rand((3, cin, h, w), 1)
    wt = _rand((cout, cin, kh, kw), 2, 0.1)
    b = _rand((cout,), 3)
    op = _op(_nhwc(x), wt, bias=b, stride=stride, upsample=up)
    xi = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    want = F.conv2d(xi, wt, b, stride=stride, padding=(kh // 2, kw // 2))
    got = ls.igemm_reference(op)
    assert torch.allclose(got, _flat(_nhwc(want)), rtol=1e-12, atol=1e-12)
    rows = torch.tensor([0, 5, got.shape[0] * got.shape[1] - 1])
    assert torch.allclose(ls.igemm_reference(op, rows=rows), got.reshape(-1, cout)[rows], rtol=1e-13, atol=1e-13)


def test_igemm_reference_stride2_explicit_size_concat_and_epilogue():
    """stride 2 with an explicit hout / wout (the asymmetric-pad Downsample: reads past the bottom / right edge are zero), a
    second source concatenated on channels, rowvec with and without the layer's bias in it, residual, scale."""
    x0, x1 = _rand((2, 32, 8, 8), 4), _rand((2, 32, 8, 8), 5)
    wt = _rand((24, 64, 3, 3), 6, 0.1)
    b = _rand((24,), 7)
    op = _op(_nhwc(x0), wt, x2=_nhwc(x1), bias=b, stride=2, pad=(0, 0), hout=4, wout=4)
    want = F.conv2d(F.pad(torch.cat([x0, x1], 1), (0, 1, 0, 1)), wt, b, stride=2)
    assert torch.allclose(ls.igemm_reference(op), _flat(_nhwc(want)), rtol=1e-12, atol=1e-12)
    rv, res = _rand((2, 24), 8), _rand((2, 4, 4, 24), 9)
    base = F.conv2d(F.pad(torch.cat([x0, x1], 1), (0, 1, 0, 1)), wt, None, stride=2)
    for has_bias in (False, True):
        op = _op(_nhwc(x0), wt, x2=_nhwc(x1), bias=b, stride=2, pad=(0, 0), hout=4, wout=4, rowvec=rv, rowvec_has_bias=has_bias,
                 residual=res.reshape(2, 16, 24), scale=0.5)
        want = _nhwc(base) * 0.5 + (0 if has_bias else b) + rv[:, None, None, :] + res
        assert torch.allclose(ls.igemm_reference(op), _flat(want), rtol=1e-12, atol=1e-12), has_bias


def test_igemm_reference_linear_groups_ln_fold_geglu():
    """Token rows as [N, T, 1, C]: groups (image i takes matrix i // (N / g)), the LayerNorm fold, the packed GEGLU rows."""
    n, t, c = 4, 6, 64
    x = _rand((n, t, 1, c), 10, 2.0) + 0.5
    w = _rand((2 * 32, c), 11, 0.1)
    op = _op(x, w[:, :, None, None], groups=2)
    want = torch.cat([F.linear(x[:2, :, 0], w[:32]), F.linear(x[2:, :, 0], w[32:])])
    assert torch.allclose(ls.igemm_reference(op), want, rtol=1e-12, atol=1e-12)
    # LayerNorm folded: W' = W diag(gamma), bias' = W beta + b  ==  Linear(LayerNorm(x))
    wl, bl = _rand((40, c), 12, 0.1), _rand((40,), 13)
    gamma, beta = _rand((c,), 14) * 0.2 + 1.0, _rand((c,), 15) * 0.1
    op = _op(x, (wl * gamma)[:, :, None, None], bias=wl @ beta + bl, ln_eps=1e-5)
    want = F.linear(F.layer_norm(x[:, :, 0], (c,), gamma, beta, 1e-5), wl, bl)
    assert torch.allclose(ls.igemm_reference(op), want, rtol=1e-10, atol=1e-10)
    # GEGLU: rows of every 16-row tile = 8 value rows, then the 8 gate rows of the same outputs (ops.pack_geglu / geglu_layout)
    from mobi_amd import ops
    inner = 32
    wg, bg = _rand((2 * inner, c), 16, 0.1), _rand((2 * inner,), 17)
    pk = ops.pack_geglu(wg.float(), bg.float(), torch.float32, "cpu")
    op = _op(x, pk.w.double()[:, :, None, None], bias=pk.bias.double(), geglu=True, cout=inner)
    op["n_packed"] = 2 * inner
    pre = F.linear(x[:, :, 0], wg.float().double(), bg.float().double())
    want = pre[..., :inner] * F.gelu(pre[..., inner:])
    assert torch.allclose(ls.igemm_reference(op), want, rtol=1e-6, atol=1e-6)


def test_norm_and_attention_references():
    x = _rand((3, 4, 5, 64), 20, 1.5) + 2.0
    x2 = _rand((3, 4, 5, 32), 21)
    g, b = _rand((96,), 22), _rand((96,), 23)
    op = dict(x=x, x2=x2, gamma=g, beta=b, eps=1e-5, silu=True)
    want = F.silu(F.group_norm(torch.cat([x, x2], 3).permute(0, 3, 1, 2), 32, g, b, 1e-5)).permute(0, 2, 3, 1)
    got = ls.groupnorm_reference(op)
    assert torch.allclose(got, _flat(want), rtol=1e-11, atol=1e-11)
    rows = torch.tensor([0, 19, 20, 59])
    assert torch.allclose(ls.groupnorm_reference(op, rows=rows), got.reshape(-1, 96)[rows], rtol=1e-13, atol=1e-13)
    t = _rand((4, 7, 64), 24)
    gl, bl = _rand((64,), 25), _rand((64,), 26)
    assert torch.allclose(ls.layernorm_reference(dict(x=t[1::2], gamma=gl, beta=bl, eps=1e-5)),
                          F.layer_norm(t[1::2], (64,), gl, bl, 1e-5), rtol=1e-12, atol=1e-12)
    # attention: strided q / k / v views (stacked projections), V^T and V rows, q pre-scaled by scale * log2 e
    n, tq, tk, h, dh = 2, 9, 11, 4, 8
    c = h * dh
    qkv = _rand((n, tq, 3 * c), 27)
    kv = _rand((n, tk, 2 * c), 28)
    scale = dh ** -0.5
    split = lambda z, tt: z.reshape(n, tt, h, dh).transpose(1, 2)
    want = F.scaled_dot_product_attention(split(qkv[..., :c], tq), split(kv[..., :c], tk), split(kv[..., c:], tk), scale=scale)
    want = want.transpose(1, 2).reshape(n, tq, c)
    for v_rows in (True, False):
        v = kv[..., c:] if v_rows else kv[..., c:].transpose(1, 2)
        got = ls.attention_reference(dict(q=qkv[..., :c], k=kv[..., :c], v=v, heads=h, scale=scale, v_rows=v_rows,
                                          q_log2_scaled=False))
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), v_rows
    got = ls.attention_reference(dict(q=qkv[..., :c] * (scale * math.log2(math.e)), k=kv[..., :c], v=kv[..., c:], heads=h,
                                      scale=123.0, v_rows=True, q_log2_scaled=True))
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    rows = torch.tensor([0, 3, tq, 2 * tq - 1])
    assert torch.allclose(ls.attention_reference(dict(q=qkv[..., :c], k=kv[..., :c], v=kv[..., c:], heads=h, scale=scale,
                                                      v_rows=True, q_log2_scaled=False), rows=rows),
                          want.reshape(-1, c)[rows], rtol=1e-12, atol=1e-12)


def test_two_key_adapter_reference_is_two_key_attention():
    """The shared restatement x + b + sum_h sigmoid(...) u_h against what it folds (BasicTransformerBlock._two_key_terms):
    x + W (softmax over two keys of q_h = LN(x) Wq_h^T) v, W the folded output projection, for per-head tables built from
    k / v of the two tokens."""
    n, t, c, h = 2, 5, 32, 4
    dh = c // h
    x = _rand((n, t, c), 30, 2.0) + 0.3
    wq, w = _rand((c, c), 31, 0.2), _rand((c, c), 32, 0.2)
    k, v = _rand((n, 2, c), 33), _rand((n, 2, c), 34)
    b0 = _rand((c,), 35)
    ln = F.layer_norm(x, (c,), None, None, 1e-5)
    q = (ln @ wq.T).reshape(n, t, h, dh)
    sc = torch.einsum("nthd,nkhd->nthk", q, k.reshape(n, 2, h, dh)) * dh ** -0.5
    att = torch.einsum("nthk,nkhd->nthd", sc.softmax(-1), v.reshape(n, 2, h, dh)).reshape(n, t, c)
    want = x + att @ w.T + b0
    mask = torch.zeros(h, c, dtype=torch.float64)
    for i in range(h):
        mask[i, i * dh:(i + 1) * dh] = 1
    dk, dv = (k[:, 0] - k[:, 1])[:, None] * mask, (v[:, 0] - v[:, 1])[:, None] * mask
    a = dk @ wq * dh ** -0.5                                         # Wq_h^T dk_h, scaled
    u = dv @ w.T
    got = ls.two_key_adapter_reference(x, a, a.sum(-1), torch.zeros(n, h, dtype=torch.float64), u, v[:, 1] @ w.T + b0, 1e-5)
    assert torch.allclose(got, want, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("dtype", DT)
def test_ff_geglu_decode_round_trips_the_packer(dtype):
    """decode_ff_geglu restates the chunk-image layout of include/mobi_engine.h; the packer's images must decode to the
    storage-rounded masters, and the reference must be the plain GEGLU feed-forward of them."""
    from mobi_amd import ops
    c, hidden = 320, 64
    w1, b1 = _rand((2 * hidden, c), 40, 0.05).float(), _rand((2 * hidden,), 41).float()
    w2, b2 = _rand((c, hidden), 42, 0.05).float(), _rand((c,), 43).float()
    pf = ops.pack_ff_geglu(w1, b1, w2, b2, dtype, "cpu")
    d1, db1, d2 = ls.decode_ff_geglu(pf.buf, c, hidden, dtype)
    assert torch.equal(d1, w1.to(dtype)) and torch.equal(d2, w2.to(dtype)) and torch.equal(db1, b1)
    x = _rand((2, 3, c), 44).to(dtype)
    res = _rand((2, 3, c), 45).to(dtype)
    g, bt = _rand((c,), 46).float(), _rand((c,), 47).float()
    got = ls.ff_geglu_reference(dict(x=x, residual=res, b2=pf.b2, ln=(g, bt, 1e-5), dec=(d1, db1, d2)))
    xl = F.layer_norm(x.double(), (c,), g.double(), bt.double(), 1e-5)
    pre = F.linear(xl, w1.to(dtype).double(), b1.double())
    want = F.linear(pre[..., :hidden] * F.gelu(pre[..., hidden:]), w2.to(dtype).double(), b2.double()) + res.double()
    assert torch.allclose(got, want, rtol=1e-11, atol=1e-11)


# ---- the metric -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_metric_passes_storage_rounding(dtype):
    ref = _rand((4, 300, 320), 50) * torch.linspace(0.1, 10, 320, dtype=torch.float64)
    res = ls.compare(ref.to(dtype), ref)
    assert ls.passes(res, TOL[dtype]), res


@pytest.fixture(scope="module")
def dropped_chunk():
    """A 65,536 x 320 product with K = 2,880 whose 128 x 64 tile at rows 4,096.. / channels 128.. lost one 64-deep k-chunk:
    the tensor is drawn with the product's statistics, the tile is the real product of its operands."""
    k, r0, c0 = 2880, 4096, 128
    ref = _rand((1, 65536, 320), 51) * math.sqrt(k)
    a, w = _rand((128, k), 52), _rand((64, k), 53)
    ref[0, r0:r0 + 128, c0:c0 + 64] = a @ w.T
    bad = ref.clone()
    bad[0, r0:r0 + 128, c0:c0 + 64] = a[:, 64:] @ w[:, 64:].T
    return ref, bad, (0, r0, c0)


@pytest.mark.parametrize("dtype", DT)
def test_metric_fails_dropped_k_chunk(dtype, dropped_chunk):
    ref, bad, where = dropped_chunk
    res = ls.compare(bad.to(dtype), ref)
    assert res["tile"] > 0.1 and res["where"] == where, res                       # ~ sqrt(1 / 45)
    assert not ls.passes(res, TOL[dtype]), res
    if dtype == torch.bfloat16:
        assert res["rel"] < TOL[dtype], res                                      # whole-tensor rel-L2 alone would pass


@pytest.mark.parametrize("dtype", DT)
def test_metric_fails_nan_row(dtype):
    ref = _rand((2, 256, 64), 54)
    got = ref.to(dtype)
    got[1, 77] = float("nan")
    res = ls.compare(got, ref)
    assert not res["finite"] and not ls.passes(res, TOL[dtype]), res


@pytest.mark.parametrize("dtype", DT)
def test_outside_view_write_is_caught(dtype):
    """The camera / lidar halves are updated in place through batch-strided views: a write one row past a view's rows, or
    into the partner image, must show; writes inside the view must not."""
    base = _rand((4, 20, 64), 55).to(dtype)
    view = base[::2, 2:18]
    ov = ls.OutsideView(view)
    view.add_(1.0)
    assert ov.unchanged()
    base[0, 18] += 1.0                                          # one row past the view's last row of image 0
    assert not ov.unchanged()
    base2 = _rand((4, 16, 64), 56).to(dtype)
    ov2 = ls.OutsideView(base2[::2])
    base2[1, 0] = float("nan")                                  # the partner image's first row
    assert not ov2.unchanged()


# ---- the VAEs' entry points -------------------------------------------------------------------------------------------
def _per_image_op(x, w, n, npk, k, stride, scale=1.0):
    return dict(x=x, x2=None, w=ls.per_image_weights(w, n, npk, k, stride), bias=None, kh=1, kw=1, stride=1, pad_h=0, pad_w=0,
                upsample=False, hout=x.shape[1], wout=1, cout=npk, n_packed=npk, groups=n, geglu=False, ln=False, ln_eps=0.0,
                scale=scale, rowvec=None, rowvec_has_bias=False, residual=None)


def test_per_image_weight_reference_is_einsum():
    """S = q k^T * scale with the keys as per-image weights, and O = P v from the transposed v, against fp64 einsum; image i
    multiplies slab i of the tensor's own shape."""
    n, t, c = 3, 40, 16
    q, k, vt = _rand((n, t, 1, c), 60), _rand((n, t, c), 61), _rand((n, c, t), 62)
    s = ls.igemm_reference(_per_image_op(q, k, n, t, c, t * c, scale=c ** -0.5))
    want_s = torch.einsum("ntc,nsc->nts", q[:, :, 0], k) * c ** -0.5
    assert torch.allclose(s, want_s, rtol=1e-12, atol=1e-12)
    p = torch.softmax(want_s, dim=-1)
    o = ls.igemm_reference(_per_image_op(p.unsqueeze(2), vt, n, c, t, c * t))
    assert torch.allclose(o, torch.einsum("nts,ncs->ntc", p, vt), rtol=1e-12, atol=1e-12)
    rows = torch.tensor([0, t - 1, t, 2 * t + 5, 3 * t - 1])
    sub = ls.igemm_reference(_per_image_op(q, k, n, t, c, t * c, scale=c ** -0.5), rows=rows)
    assert torch.allclose(sub, want_s.reshape(n * t, t)[rows], rtol=1e-12, atol=1e-12)


def test_per_image_weights_reject_a_disagreeing_stride():
    n, t, c = 3, 8, 16
    k = _rand((n, t, c), 63)
    assert ls.per_image_weights(k, n, t, c, t * c).shape == (n, t, c)
    for bad in (0, c, 2 * t * c):                               # every image reading image 0's keys; a row stride; past the end
        with pytest.raises(ValueError, match="w_group_stride"):
            ls.per_image_weights(k, n, t, c, bad)
    with pytest.raises(ValueError):
        ls.per_image_weights(k[:, :, :8], n, t, c, t * c)       # not the tensor's own slabs


@pytest.mark.parametrize("dtype", DT)
def test_metric_fails_image_read_with_image_0_weights(dtype):
    """The fp32 scores of a batch where image 1 multiplied image 0's keys (w_group_stride 0): whole rel-L2 and tiles fail."""
    n, t, c = 3, 256, 64
    q, k = _rand((n, t, c), 64).to(dtype).double(), _rand((n, t, c), 65).to(dtype).double()
    ref = torch.einsum("ntc,nsc->nts", q, k) * c ** -0.5
    got = ref.float().clone()
    got[1] = (q[1] @ k[0].T * c ** -0.5).float()
    assert ls.passes(ls.compare(ref.float(), ref), ls.bound_f32_rows(dtype))
    res = ls.compare(got, ref)
    assert not ls.passes(res, ls.bound_f32_rows(dtype)) and res["where"][0] == 1, res


@pytest.mark.parametrize("dtype", DT)
def test_split_check(dtype):
    x = _rand((2, 5, 7, 64), 66).float() * 3.0
    hi = x.to(dtype)
    lo = (x - hi.float()).to(dtype)
    assert ls.check_split(x, torch.cat([hi, lo], -1), 2, dtype) == []
    assert ls.check_split(x, torch.cat([hi, lo, hi], -1), 3, dtype) == []
    assert any("third part" in m for m in ls.check_split(x, torch.cat([hi, lo, lo], -1), 3, dtype))
    assert any("hi + lo" in m for m in ls.check_split(x, torch.cat([hi, torch.zeros_like(lo)], -1), 2, dtype))
    bumped = hi.clone()
    bumped[1, 2, 3, 4] = bumped[1, 2, 3, 4] * 2
    assert any("hi is not" in m for m in ls.check_split(x, torch.cat([bumped, lo], -1), 2, dtype))


@pytest.mark.parametrize("dtype", DT)
def test_trunk_add_check(dtype):
    trunk, inc = _rand((2, 4, 4, 64), 67).float(), _rand((2, 4, 4, 64), 68).to(dtype)
    after = trunk + inc.float()
    assert ls.check_trunk_add(trunk, inc, after, after.to(dtype), dtype) == []
    assert ls.check_trunk_add(trunk, None, trunk.clone(), trunk.to(dtype), dtype) == []
    assert ls.check_trunk_add(trunk, inc, trunk.clone(), trunk.to(dtype), dtype)                   # the update was lost
    assert ls.check_trunk_add(trunk, inc, after, trunk.to(dtype), dtype)                           # copy of the old trunk
    assert ls.check_trunk_add(trunk, None, after, after.to(dtype), dtype)                          # trunk written with no inc


def test_softmax_reference_and_row_sums():
    s = _rand((70, 1000), 69) * 5.0
    s[3] = 0.0
    ref = ls.softmax_reference(dict(s=s))
    assert torch.allclose(ref, torch.softmax(s, dim=-1), rtol=1e-13, atol=1e-16)
    rows = torch.tensor([0, 3, 69])
    assert torch.equal(ls.softmax_reference(dict(s=s), rows=rows), ref[rows])
    assert ls.softmax_row_sums(ref) < 1e-12
    for dtype in DT:
        got = ref.to(dtype)
        assert ls.softmax_row_sums(got) < TOL[dtype] and ls.passes(ls.compare(got[None], ref[None]), TOL[dtype])
        bad = got.clone()
        bad[17] = (bad[17].double() * 1.01).to(dtype)                  # one row that sums to 1.01
        assert ls.softmax_row_sums(bad) > TOL[dtype]


@pytest.mark.parametrize("k,clamp", [((3, 3), (-0.5, 0.5)), ((1, 5), None)])
def test_conv_small_cout_reference_is_conv2d(k, clamp):
    kh, kw = k
    x, w, b = _rand((2, 64, 6, 20), 70), _rand((3, 64, kh, kw), 71, 0.1), _rand((3,), 72)
    op = _op(_nhwc(x), w, bias=b)
    op["clamp"] = clamp
    want = F.conv2d(x, w, b, padding=(kh // 2, kw // 2))
    if clamp:
        want = want.clamp(*clamp)
    got = ls.conv_small_cout_reference(op)
    assert torch.allclose(got, _flat(_nhwc(want)), rtol=1e-12, atol=1e-12)


def test_conv_small_cin_op_is_conv2d():
    """The OIHW-flattened fp32 weight and the NCHW sources of conv_small_cin, through the igemm reference."""
    a, z = _rand((2, 3, 5, 9), 73), _rand((2, 1, 5, 9), 74)
    w, b = _rand((6, 4, 1, 5), 75, 0.2), _rand((6,), 76)
    op = ls.conv_small_cin_op([a, z], w.reshape(6, -1), b, 1, 5, (0, 2))
    got = ls.igemm_reference(op)
    assert torch.allclose(got, _flat(_nhwc(F.conv2d(torch.cat([a, z], 1), w, b, padding=(0, 2)))), rtol=1e-12, atol=1e-12)
    op = ls.conv_small_cin_op([z], _rand((8, 1, 1, 1), 77).reshape(8, -1), None, 1, 1, (0, 0))
    assert torch.allclose(ls.igemm_reference(op), _flat(z.permute(0, 2, 3, 1)) * op["w"].reshape(1, 1, 8), rtol=1e-12)


def test_census_reports_an_unshadowed_launch():
    """A launch the shadow did not judge, or an entry point that is neither shadowed nor query-only, is a census failure."""
    class Lib:
        def __getattr__(self, name):
            return lambda *a: 0

    class Shadow(ls.LaunchShadow):
        def __init__(self):
            self.calls, self.counts = {}, {}

    sh = Shadow()
    lib = ls.LibCensus(Lib(), sh.calls)
    lib.mobi_igemm_plan_splits(None)
    lib.mobi_igemm_workspace_bytes(None, 2)
    lib.mobi_tile_weights(None)
    lib.mobi_igemm(None)
    sh.counts["igemm"] = 1
    assert sh.census_failures() == []
    lib.mobi_igemm(None)
    lib.mobi_nearest_resize(None)
    bad = sh.census_failures()
    assert any(m.startswith("mobi_igemm:") for m in bad) and any(m.startswith("mobi_nearest_resize:") for m in bad), bad


def test_igemm_reference_leaky_is_before_the_residual():
    """MOBI_EPI_LEAKY_RELU: leaky_relu(conv + bias + rowvec, 0.1) + residual; on the paired-width view a 3 x 2 launch with an
    explicit output size is the stride-(1, 2) convolution realism.stride2_weight rewrites."""
    from mobi_amd.realism import stride2_weight
    x, wt, b = _rand((2, 32, 6, 8), 81), _rand((24, 32, 3, 3), 82, 0.1), _rand((24,), 83)
    rv, res = _rand((2, 24), 84), _rand((2, 6, 8, 24), 85)
    op = dict(_op(_nhwc(x), wt, bias=b, rowvec=rv, residual=res.reshape(2, 48, 24)), leaky=True)
    want = F.leaky_relu(_nhwc(F.conv2d(x, wt, b, padding=1)) + rv[:, None, None, :], 0.1) + res
    assert torch.allclose(ls.igemm_reference(op), _flat(want), rtol=1e-12, atol=1e-12)
    plain = dict(op, leaky=False)
    assert not torch.allclose(ls.igemm_reference(plain), _flat(want), rtol=1e-3, atol=1e-3)
    paired = _nhwc(x).reshape(2, 6, 4, 64)
    op = dict(_op(paired, stride2_weight(wt), bias=b, hout=6, wout=4), leaky=True)
    want = F.leaky_relu(F.conv2d(x, wt, b, stride=(1, 2), padding=1), 0.1)
    assert torch.allclose(ls.igemm_reference(op), _flat(_nhwc(want)), rtol=1e-12, atol=1e-12)


def test_extra_kinds_are_opt_in_and_counted_per_library_call():
    """Without `extra` the wrapped set is the UNet's and the VAEs'; an unknown kind is refused; every extra kind has its entry
    point in LAUNCH_KINDS; a skinny_linear judged once for 17 rows accounts for two library calls."""
    class MP:
        pass
    assert ls.LaunchShadow(MP()).wrapped == ls.LaunchShadow.WRAPPED
    both = ls.LaunchShadow(MP(), extra=ls.EXTRA_KINDS).wrapped
    assert both == ls.LaunchShadow.WRAPPED + ls.EXTRA_KINDS and len(set(both)) == len(both)
    assert ls.LaunchShadow(MP(), extra=("quick_gelu",)).wrapped == ls.LaunchShadow.WRAPPED + ("quick_gelu",)
    with pytest.raises(ValueError):
        ls.LaunchShadow(MP(), extra=("quick_gelu", "nearest_resize"))
    assert set(ls.EXTRA_KINDS) <= set(ls.LAUNCH_KINDS.values())
    assert all(hasattr(ls.LaunchShadow, "_" + k) for k in both)
    assert ls.is_query_only("mobi_lpips_distance_ws_floats") and not ls.is_query_only("mobi_lpips_distance")

    class Lib:
        def __getattr__(self, name):
            return lambda *a: 0
    sh = ls.LaunchShadow(MP(), extra=("skinny_linear",))
    lib = ls.LibCensus(Lib(), sh.calls)
    lib.mobi_skinny_linear(None)
    lib.mobi_skinny_linear(None)
    sh._count("skinny_linear", (17 + 15) // 16)
    assert sh.census_failures() == []
    lib.mobi_quick_gelu(None)
    assert [m for m in sh.census_failures() if m.startswith("mobi_quick_gelu: 1 calls, 0 judged")]


# ---- row chains -----------------------------------------------------------------------------------------------------------
def test_chain_kinds_are_wrapped_and_counted():
    """row_chain, chain_adapter_image and groupnorm_scale_shift are launch kinds of the default set; the image-size query is
    query-only, the image launch is not; an unjudged chain launch is a census failure."""
    class MP:
        pass
    for kind, name in (("row_chain", "mobi_row_chain"), ("chain_adapter_image", "mobi_row_chain_adapter_image"),
                       ("groupnorm_scale_shift", "mobi_groupnorm_scale_shift")):
        assert ls.LAUNCH_KINDS[name] == kind and kind in ls.LaunchShadow.WRAPPED and hasattr(ls.LaunchShadow, "_" + kind)
    assert ls.is_query_only("mobi_row_chain_adapter_image_bytes") and ls.is_query_only("mobi_row_chain_weight_bytes")
    assert ls.is_query_only("mobi_row_chain_supported") and not ls.is_query_only("mobi_row_chain_adapter_image")

    class Lib:
        def __getattr__(self, name):
            return lambda *a: 0
    sh = ls.LaunchShadow(MP())
    lib = ls.LibCensus(Lib(), sh.calls)
    lib.mobi_row_chain(None)
    lib.mobi_row_chain_adapter_image_bytes(320)
    assert [m for m in sh.census_failures() if m.startswith("mobi_row_chain: 1 calls, 0 judged")]
    sh._count("row_chain")
    assert sh.census_failures() == []


@pytest.mark.parametrize("dtype", DT)
def test_row_chain_wrapper_judges_an_emulated_launch(dtype, monkeypatch):
    """The shadow's row_chain wrapper around an fp32 emulation of the kernel (tests/chain_cases.py): the clean launch passes
    with one record per stored tensor under the launch's note; a launch with products 0 and 1 swapped fails; the adapter's
    tables are found by the CONTENT of the image (a copy in another buffer matches), and an image no chain_adapter_image call
    produced is a failure."""
    from tests import chain_cases as cc, chain_ref
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)

    class MP:
        pass

    def run(defect, image_of, note="post_attn1 rows=1024"):
        case = cc.build_case("post_attn1-4x256", dtype, "cpu", chain_ref.ProgramDescription)
        sh = ls.LaunchShadow(MP(), label="cpu")
        tb = case.tables
        made = torch.arange(4 * 64, dtype=torch.int64).view(4, 64).to(torch.uint8)       # stands in for the image's bytes
        sh.adapter_images.append(dict(a=tb["a"], c=tb["c"], u=tb["u"], b=tb["b"], image=made.clone(), dtype=dtype))
        sh.adapter_images.append(dict(a=tb["a"] * 2, c=tb["c"], u=tb["u"], b=tb["b"], image=made.clone() + 1, dtype=dtype))
        orig = lambda programs, images, rows, dt, adapter=None, flops=0.0, nbytes=0.0, note="": cc.emulate(case, defect)
        sh._row_chain(orig, case.programs, case.images, case.rows, dtype, adapter=(image_of(made), tb["eps"]), note=note)
        return sh

    sh = run(None, lambda made: made.clone())
    assert sh.failures == [] and sh.counts == {"row_chain": 1}
    assert len(sh.records) == 6 and all(r["kind"] == "row_chain" and r["form"]["note"] == "post_attn1" for r in sh.records)
    assert sorted(r["bound"] for r in sh.records) == sorted([TOL[dtype]] * 4 + [1.5 * TOL[dtype]] * 2)
    sh = run("swap_weights", lambda made: made.clone())
    assert sh.failures and sh.counts == {"row_chain": 1}
    sh = run(None, lambda made: made.clone() + 7)
    assert len(sh.failures) == 1 and "matches no chain_adapter_image call" in sh.failures[0] and sh.counts == {"row_chain": 1}
    # a program that did not come from the recording class cannot be judged: a failure, not a silent pass
    sh = ls.LaunchShadow(MP(), label="cpu")
    sh._row_chain(lambda *a, **kw: None, [object()], 2, 128, dtype)
    assert len(sh.failures) == 1 and "not built through ops.ChainProgram" in sh.failures[0]


# ---- the training step's kinds (TRAIN_KINDS) --------------------------------------------------------------------------------
# Every judge is fed the float64 reference rounded once to the type the launch stores (it passes, at a quarter of its bound or
# less) and one planted fault (it fails, and the failure names the launch).
from tests import backward_ref as R, loss_grad_ref           # noqa: E402
from tests.golden_cases import record                        # noqa: E402


class _MP:
    pass


# Rounding to a 16-bit type with unit roundoff u (2^-11 fp16, 2^-8 bf16) leaves an error uniform within half a unit in the last
# place: rms ulp / sqrt(12) = u 2^e / sqrt(3) for a value in [2^e, 2^(e+1)), so the rel-L2 of a once-rounded tensor is at most
# u / sqrt(3) = 2.82e-4 (fp16) / 2.26e-3 (bf16) whatever its mantissas, and 2.07e-4 / 1.66e-3 for Gaussian values (measured; TOL1 /
# 3.86 and / 3.98).  A factor 4 below TOL1 is out of reach of ANY once-rounded 16-bit result; those checks are held to
# TOL1 / (u / sqrt(3)) = 2.8, which every correct rounding meets.  Round-to-nearest is within half a storage ulp: a factor 2 below
# the one ulp the l2 dy is allowed.  Everything else (fp32 results, the loss terms, the 1.5 TOL1 of the matrix-core attention
# route, the fp32 weight gradient) keeps the factor 4.
ROOM, ROOM_ROUNDED_ONCE, ROOM_ULP = 4.0, 2.8, 2.0


def _room(ck):
    if ck.what.endswith("(storage ulp)"):
        return ROOM_ULP
    return ROOM_ROUNDED_ONCE if ck.mode == "tiles" and ck.bound in ls.TOL1.values() else ROOM


def _clean(kind, checks):
    """The rounded reference passes every check, with room: rel-L2 (and the worst tile) a factor `_room` inside the bound."""
    assert ls.check_failures(kind, "clean", checks) == []
    for ck in checks:
        res = ls.evaluate(ck)
        if ck.mode in ("tiles", "value", "figure"):
            record(f"shadow cpu {kind} {ck.what} clean", res["rel"], ck.bound)
            assert _room(ck) * res["rel"] <= ck.bound, (kind, ck.what, res["rel"], ck.bound)
        if ck.mode == "tiles":
            assert _room(ck) * res["tile"] <= ls.TILE_FACTOR * ck.bound, (kind, ck.what, res["tile"], ck.bound)


def _faulty(kind, checks, *outputs):
    """The planted fault is reported on exactly the named outputs, each failure naming the launch."""
    bad = ls.check_failures(kind, "planted", checks)
    assert bad and all(m.startswith(f"{kind} planted") for m in bad), bad
    for what in outputs:
        assert any(f"{kind} planted {what}" in m for m in bad), (what, bad)
    return bad


def test_train_kinds_are_opt_in():
    assert ls.LaunchShadow(_MP()).wrapped == ls.LaunchShadow.WRAPPED
    both = ls.LaunchShadow(_MP(), extra=ls.TRAIN_KINDS + ("linear_f32", "add")).wrapped
    assert both == ls.LaunchShadow.WRAPPED + ("linear_f32", "add") + ls.TRAIN_KINDS and len(set(both)) == len(both)
    assert set(ls.TRAIN_KINDS) <= set(ls.LAUNCH_KINDS.values()) and not set(ls.TRAIN_KINDS) & set(ls.EXTRA_KINDS)
    assert all(hasattr(ls.LaunchShadow, "_" + k) and ls.LAUNCH_KINDS["mobi_" + k] == k for k in ls.TRAIN_KINDS)
    for q in ("mobi_backward_partial_blocks", "mobi_groupnorm_bwd_workspace_floats", "mobi_loss_grad_blocks_per_sample"):
        assert ls.is_query_only(q), q
    assert not any(ls.is_query_only("mobi_" + k) for k in ls.TRAIN_KINDS)


def test_census_reports_an_unwrapped_layernorm_bwd():
    """A mobi_layernorm_bwd call no wrapper judged (a shadow without TRAIN_KINDS around a training step) is a census failure;
    its partial-block query is not."""
    class Lib:
        def __getattr__(self, name):
            return lambda *a: 0
    sh = ls.LaunchShadow(_MP())
    lib = ls.LibCensus(Lib(), sh.calls)
    lib.mobi_backward_partial_blocks(1024)
    assert sh.census_failures() == []
    lib.mobi_layernorm_bwd(None, None)
    assert sh.census_failures() == ["mobi_layernorm_bwd: 1 calls, 0 judged by the shadow"]
    sh._count("layernorm_bwd")
    assert sh.census_failures() == []


@pytest.mark.parametrize("dtype", DT)
def test_colsum_and_layernorm_bwd_judges(dtype):
    """1,000 rows = 63 partial blocks, the last of 8 rows: column sums and d gamma that lost them; dx that lost dx_add in one
    of four images."""
    n, t, c = 4, 250, 64
    x, dy, add = (_rand((n, t, c), s, sc).to(dtype) for s, sc in ((100, 2.0), (101, 1.0), (102, 1.0)))
    gamma = _rand((c,), 103).float() * 0.2 + 1.0
    assert R.partial_blocks(n * t) == 63 and n * t - 62 * 16 == 8
    cs = R.colsum_ref(dy.reshape(-1, c))
    _clean("colsum", ls.colsum_checks(dy.reshape(-1, c), cs.float()))
    _faulty("colsum", ls.colsum_checks(dy.reshape(-1, c), R.colsum_ref(dy.reshape(-1, c)[:62 * 16]).float()), "out")
    rdx, rdg, rdb = R.layernorm_bwd_ref(x.reshape(-1, c), dy.reshape(-1, c), gamma, 1e-5, dx_add=add.reshape(-1, c))
    good = (rdx.reshape(n, t, c).to(dtype), rdg.float(), rdb.float())
    _clean("layernorm_bwd", ls.layernorm_bwd_checks(x, dy, gamma, 1e-5, add, *good))
    _, sdg, _ = R.layernorm_bwd_ref(x.reshape(-1, c)[:62 * 16], dy.reshape(-1, c)[:62 * 16], gamma, 1e-5)
    bad = _faulty("layernorm_bwd", ls.layernorm_bwd_checks(x, dy, gamma, 1e-5, add, good[0], sdg.float(), good[2]), "dgamma")
    assert len(bad) == 1
    no_add = R.layernorm_bwd_ref(x.reshape(-1, c), dy.reshape(-1, c), gamma, 1e-5)[0].reshape(n, t, c)
    dx = good[0].clone()
    dx[2] = no_add[2].to(dtype)
    bad = _faulty("layernorm_bwd", ls.layernorm_bwd_checks(x, dy, gamma, 1e-5, add, dx, good[1], good[2]), "dx")
    assert len(bad) == 1 and "at (2, " in bad[0]                                  # the worst tile is in image 2


@pytest.mark.parametrize("dtype", DT)
def test_groupnorm_bwd_judge(dtype):
    """One group of one image computed without its mean term: dx + rstd mean(dxh) there.  dy carries a common offset (a
    gradient whose group means are not 0, as a bias' is): with zero-mean noise the dropped term is 1 / 16 of an element on 4 of a
    tile's 64 channels, 1.5e-2 of the tile -- under the bf16 tile bound, so it is the offset that makes this fault visible."""
    n, side, c = 2, 8, 128
    x, dy, add = (_rand((n, side, side, c), s, sc).to(dtype) for s, sc in ((110, 1.5), (111, 1.0), (112, 1.0)))
    dy = (dy.double() + 1.5).to(dtype)
    g, b = _rand((c,), 113).float() * 0.2 + 1.0, _rand((c,), 114).float() * 0.1
    ref = R.groupnorm_bwd_ref(x.reshape(n, -1, c), dy.reshape(n, -1, c), g, b, 1e-5, True, dx_add=add.reshape(n, -1, c))
    _clean("groupnorm_bwd", ls.groupnorm_bwd_checks(x, dy, g, b, 1e-5, True, add, ref.reshape(x.shape).to(dtype)))
    img, grp, cg = 1, 5, c // 32
    sl = slice(grp * cg, (grp + 1) * cg)
    xg, dyg = x[img, ..., sl].double(), dy[img, ..., sl].double()
    rstd = (xg.var(unbiased=False) + 1e-5).rsqrt()
    z = (xg - xg.mean()) * rstd * g[sl].double() + b[sl].double()
    sg = torch.sigmoid(z)
    dxh = dyg * sg * (1.0 + z * (1.0 - sg)) * g[sl].double()
    bad_dx = ref.reshape(x.shape).clone()
    bad_dx[img, ..., sl] += rstd * dxh.mean()
    assert float((bad_dx - ref.reshape(x.shape)).abs().max()) > 0
    bad = _faulty("groupnorm_bwd", ls.groupnorm_bwd_checks(x, dy, g, b, 1e-5, True, add, bad_dx.to(dtype)), "dx")
    assert "at (1, " in bad[0]


@pytest.mark.parametrize("dtype", DT)
def test_geglu_sumpool2_silu_and_transpose_judges(dtype):
    pre, dh = _rand((2, 100, 2 * 96), 120, 1.5).to(dtype), _rand((2, 100, 96), 121).to(dtype)
    h, dpre = R.geglu_fwd_ref(pre), R.geglu_bwd_ref(pre, dh)
    _clean("geglu_fwd", ls.geglu_fwd_checks(pre, h.to(dtype)))
    _clean("geglu_bwd", ls.geglu_bwd_checks(pre, dh, dpre.to(dtype)))
    swapped = torch.cat([dpre[..., 96:], dpre[..., :96]], -1)                    # d gate where d value belongs
    _faulty("geglu_bwd", ls.geglu_bwd_checks(pre, dh, swapped.to(dtype)), "dpre")
    _faulty("geglu_fwd", ls.geglu_fwd_checks(pre, (pre[..., :96].double() * F.silu(pre[..., 96:].double())).to(dtype)), "h")
    # sumpool2: the corner (1, 1) of one 2 x 2 block left out
    src = _rand((2, 8, 12, 64), 122).to(dtype)
    pooled = R.sumpool2_ref(src)
    _clean("sumpool2", ls.sumpool2_checks(src, pooled.to(dtype)))
    short = pooled.clone()
    short[1, 2, 3] -= src[1, 5, 7].double()
    _faulty("sumpool2", ls.sumpool2_checks(src, short.to(dtype)), "out")
    # silu_bwd_f32: the derivative without its z (1 - sigmoid) term
    z, dz = _rand((6, 512), 123, 2.0).float(), _rand((6, 512), 124).float()
    _clean("silu_bwd_f32", ls.silu_bwd_f32_checks(z, dz, R.silu_bwd_ref(z, dz).float()))
    _faulty("silu_bwd_f32", ls.silu_bwd_f32_checks(z, dz, (dz * torch.sigmoid(z)).float()), "dx")
    # transpose: one 8 x 8 block left untransposed
    xt = _rand((64, 40), 125).to(dtype)
    assert ls.check_failures("transpose", "clean", ls.transpose_checks(xt, xt.t().contiguous())) == []
    out = xt.t().contiguous()
    out[8:16, 16:24] = xt[8:16, 16:24]
    assert not torch.equal(out, xt.t())
    bad = _faulty("transpose", ls.transpose_checks(xt, out), "out")
    assert "bit for bit" in bad[0]


@pytest.mark.parametrize("dtype", DT)
def test_attention_bwd_judge(dtype):
    """Keys and values with a common offset three times the tokens' own spread (test_attention_backward_with_common_offsets):
    the matrix-core restatement with the row term D from the pass's own P and dP passes; with D = do . o on the STORED output
    (the 26 % finding of tests/test_gpu_backward.py) dq fails; one head's dk swapped with its dv fails on both."""
    n, heads, dh, t = 2, 4, 16, 128
    c, scale = heads * dh, dh ** -0.5
    off = lambda s: 3.0 * _rand((1, 1, c), s)
    q, do = _rand((n, t, c), 130).to(dtype), _rand((n, t, c), 131).to(dtype)
    k, v = (_rand((n, t, c), 132) + off(133)).to(dtype), (_rand((n, t, c), 134) + off(135)).to(dtype)
    ref = R.attention_bwd_ref(q, k, v, do, heads, scale)
    for route in ("mfma", "vector"):
        _clean("attention_bwd", ls.attention_bwd_checks(q, k, v, do, heads, scale, route, *(r.to(dtype) for r in ref)))
    assert ls.check_failures("attention_bwd", "restated", ls.attention_bwd_checks(
        q, k, v, do, heads, scale, "mfma", *R.attention_bwd_restated(q, k, v, do, heads, scale, dtype, "mfma"))) == []
    o = R.attention_fwd_ref(q, k, v, heads, scale).to(dtype)
    stored = R.attention_bwd_restated(q, k, v, do, heads, scale, dtype, "mfma", o_stored=o)
    bad = _faulty("attention_bwd", ls.attention_bwd_checks(q, k, v, do, heads, scale, "mfma", *stored), "dq")
    assert not any(" dv:" in m for m in bad)                                   # dv does not read the row term
    dq, dk, dv = (r.to(dtype) for r in ref)
    dk2, dv2 = dk.clone(), dv.clone()
    dk2[..., dh:2 * dh], dv2[..., dh:2 * dh] = dv[..., dh:2 * dh], dk[..., dh:2 * dh]
    bad = _faulty("attention_bwd", ls.attention_bwd_checks(q, k, v, do, heads, scale, "mfma", dq, dk2, dv2), "dk", "dv")
    assert len(bad) == 2


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("loss_type", ["l2", "l1"])
def test_loss_grad_and_timestep_embedding_judges(dtype, loss_type):
    n, c, h, w = 3, 4, 5, 7
    eps, target = _rand((n, c, h, w), 140).float(), _rand((n, c, h, w), 141).float()
    t = torch.tensor([0, 1, 999])
    logvar, lvlb = _rand((1000,), 142).float().clamp(-1, 1), _rand((1000,), 143).float().abs()
    kw = dict(loss_type=loss_type, l_simple_weight=1.0, elbo_weight=0.25, loss_scale=4.0)
    rdy, rper, rterms = loss_grad_ref.loss_grad_ref(eps, target, t, logvar, lvlb, **kw)
    dy = loss_grad_ref.to_storage(rdy, dtype)
    args = (eps, target, t, logvar, lvlb, kw, dtype, 32)
    _clean("loss_grad", ls.loss_grad_checks(*args, dy, rper.float(), rterms.float()))
    z = torch.zeros(1)                                                          # the default objective: loss_vlb is exactly 0
    zdy, zper, zterms = loss_grad_ref.loss_grad_ref(eps, target, t, z, z, **dict(kw, elbo_weight=0.0))
    zargs = (eps, target, t, z, z, dict(kw, elbo_weight=0.0), dtype, 32)
    assert float(zterms[1]) == 0.0
    assert ls.check_failures("loss_grad", "zero", ls.loss_grad_checks(*zargs, loss_grad_ref.to_storage(zdy, dtype), zper.float(), zterms.float())) == []
    zbad = zterms.float().clone()
    zbad[1] = 1e-9
    _faulty("loss_grad", ls.loss_grad_checks(*zargs, loss_grad_ref.to_storage(zdy, dtype), zper.float(), zbad), "terms")
    spill = dy.clone()
    spill[1, 2, 3, c] = dy[1, 2, 3, c - 1]                                      # the last channel written once more, beyond out_channels
    bad = _faulty("loss_grad", ls.loss_grad_checks(*args, spill, rper.float(), rterms.float()))
    assert "beyond the 4 out_channels" in bad[0] and len(bad) == (2 if loss_type == "l1" else 1)      # (l1 is also bit-compared)
    minus = dy.clone()
    minus[..., c:] = -0.0
    assert "beyond the 4 out_channels" in _faulty("loss_grad", ls.loss_grad_checks(*args, minus, rper.float(), rterms.float()))[0]
    other = loss_grad_ref.to_storage(rdy * 1.01, dtype)                          # a wrong coefficient
    _faulty("loss_grad", ls.loss_grad_checks(*args, other, rper.float(), rterms.float()), "dy")
    _faulty("loss_grad", ls.loss_grad_checks(*args, dy, rper.float() * (1 + 1e-5), rterms.float()), "per_sample")
    if loss_type == "l2":
        from mobi_amd.ldm.modules.diffusionmodules.util import timestep_freqs
        from oracle.unet import timestep_embedding as ref_temb
        tt = torch.tensor([1, 21, 500, 981, 999])
        freqs = timestep_freqs(64, 10000).float()
        _clean("timestep_embedding", ls.timestep_embedding_checks(tt, freqs, ref_temb(tt, 64)))
        _faulty("timestep_embedding", ls.timestep_embedding_checks(tt, freqs, ref_temb(tt, 64).roll(32, 1)), "out")     # [sin | cos]


def _emulated_igemm(fault=None):
    """Stands in for ops.igemm on the CPU: the shadow's own fp64 reference of the operands, rounded once to what the launch
    stores, written through `out`; `fault(x, pw, y, out)` then plants one."""
    from mobi_amd import ops

    def run(x, pw, *, residual=None, out=None, out_mode=0, **kw):
        n, h, w, _ = x.shape
        op = dict(x=x, x2=None, w=pw.w, bias=None, kh=1, kw=1, stride=1, pad_h=0, pad_w=0, upsample=False, hout=h, wout=w,
                  cout=pw.cout, n_packed=pw.n_packed, groups=1, geglu=False, ln=False, ln_eps=0.0, scale=1.0, rowvec=None,
                  rowvec_has_bias=False, residual=None if residual is None else residual.reshape(n, h * w, pw.cout))
        y = ls.igemm_reference(op).reshape(n, h, w, pw.cout).to(torch.float32 if out_mode == ops.OUT_ROWS_F32 else x.dtype)
        if out is not None:
            out.copy_(y)
            y = out
        return y if fault is None else fault(x, pw, y, out)
    return run


def _cpu_shadow(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    sh = ls.LaunchShadow(_MP(), label="cpu")
    sh.sink = []
    return sh


@pytest.mark.parametrize("dtype", DT)
def test_igemm_wrapper_judges_a_weight_gradient(dtype, monkeypatch):
    """ops.linear_wgrad's launch as the wrapper sees it: dy^T [1, 1, n, rows] times x^T [k, rows] with the token rows as k and
    fp32 output.  The clean launch passes a factor 4 inside its bound; with the last 32 token rows of k dropped it fails."""
    from mobi_amd import ops
    rows, n, k = 1024, 96, 64
    dyt, xt = _rand((n, rows), 150).to(dtype), _rand((k, rows), 151).to(dtype)
    pw = ops.Packed(xt, None, 1, 1, rows, k, k)
    sh = _cpu_shadow(monkeypatch)
    sh._igemm(_emulated_igemm(), dyt.view(1, 1, n, rows), pw, out_mode=ops.OUT_ROWS_F32)
    assert sh.failures == [] and sh.counts == {"igemm": 1}
    rec, = sh.records
    assert rec["form"]["out_mode"] == ops.OUT_ROWS_F32 and rec["form"]["k"] == rows and rec["bound"] == ls.bound_f32_rows(dtype)
    assert not (rec["form"]["src_strided"] or rec["form"]["out_strided"] or rec["form"]["res_strided"] or rec["form"]["zero_spread"])
    assert 4.0 * rec["rel"] <= rec["bound"] and 4.0 * rec["tile"] <= ls.TILE_FACTOR * rec["bound"]

    def drop_tail(x, pw, y, out):
        return (x[0, 0, :, :-32].double() @ pw.w[:, :-32].double().t()).float().view(1, 1, n, k)
    sh = _cpu_shadow(monkeypatch)
    sh._igemm(_emulated_igemm(drop_tail), dyt.view(1, 1, n, rows), pw, out_mode=ops.OUT_ROWS_F32)
    assert len(sh.failures) == 1 and sh.failures[0].startswith("cpu igemm") and f"x=(1, 1, {n}, {rows})" in sh.failures[0], sh.failures
    assert sh.records[0]["rel"] > 0.1                                          # ~ sqrt(32 / 1024)


@pytest.mark.parametrize("dtype", DT)
def test_igemm_wrapper_judges_strided_views(dtype, monkeypatch):
    """block_forward's `ops.linear(y, connector, residual=x3[::2], out=x4[::2])` on two camera / lidar pairs: source, residual
    and output with two images each behind a doubled image stride.  Clean: passes, and the form says which operands were
    strided.  A launch that also writes the partner image's first row fails by name."""
    from mobi_amd import ops
    t, c = 40, 64
    src, x3, x4 = _rand((4, t, 1, c), 160).to(dtype), _rand((4, t, 1, c), 161).to(dtype), torch.zeros((4, t, 1, c), dtype=dtype)
    pw = ops.Packed((_rand((c, c), 162) * c ** -0.5).to(dtype), None, 1, 1, c, c, c)
    sh = _cpu_shadow(monkeypatch)
    sh._igemm(_emulated_igemm(), src[::2], pw, residual=x3[::2], out=x4[::2])
    assert sh.failures == []
    form = sh.records[0]["form"]
    assert form["src_strided"] and form["out_strided"] and form["res_strided"] and form["images"] == 2 and form["residual"]
    assert not bool(x4[1::2].any()) and bool(x4[::2].any())

    def spill(x, pw, y, out):
        out._base[1, 0] = 1.0                                                  # the lidar image between the two camera images
        return y
    sh = _cpu_shadow(monkeypatch)
    sh._igemm(_emulated_igemm(spill), src[::2], pw, residual=x3[::2], out=torch.zeros((4, t, 1, c), dtype=dtype)[::2])
    assert len(sh.failures) == 1 and "wrote outside its out view" in sh.failures[0], sh.failures
    # an image stride the launch ignored: image 1 of the view computed from the partner image (rows 1 instead of 2)
    def wrong_image(x, pw, y, out):
        y[1] = (src[1, :, 0].double() @ pw.w.double().t() + x3[2, :, 0].double()).to(dtype).view(t, 1, c)
        return y
    sh = _cpu_shadow(monkeypatch)
    sh._igemm(_emulated_igemm(wrong_image), src[::2], pw, residual=x3[::2], out=torch.zeros((4, t, 1, c), dtype=dtype)[::2])
    assert len(sh.failures) == 1 and sh.failures[0].startswith("cpu igemm") and "at (1, " in sh.failures[0], sh.failures


def test_zero_spread_form(monkeypatch):
    """The stride-2 data gradient's input (dy on the even pixels of a zero tensor) is recognised; a dense input is not."""
    from mobi_amd import ops
    c = 32
    w = (_rand((c, 9 * c), 170) * (9 * c) ** -0.5).to(torch.float16)
    pw = ops.Packed(w, None, 3, 3, c, c, c)

    def conv(x, pw, **kw):
        op = dict(x=x, x2=None, w=pw.w, bias=None, kh=3, kw=3, stride=1, pad_h=1, pad_w=1, upsample=False, hout=x.shape[1],
                  wout=x.shape[2], cout=c, n_packed=c, groups=1, geglu=False, ln=False, ln_eps=0.0, scale=1.0, rowvec=None,
                  rowvec_has_bias=False, residual=None)
        return ls.igemm_reference(op).reshape(x.shape[0], x.shape[1], x.shape[2], c).to(x.dtype)
    dz = torch.zeros((2, 8, 8, c), dtype=torch.float16)
    dz[:, ::2, ::2] = _rand((2, 4, 4, c), 171).to(torch.float16)
    for x, want in ((dz, True), (_rand((2, 8, 8, c), 172).to(torch.float16), False)):
        sh = _cpu_shadow(monkeypatch)
        sh._igemm(conv, x, pw)
        assert sh.failures == [] and sh.records[0]["form"]["zero_spread"] is want


@pytest.mark.parametrize("dtype", DT)
def test_train_wrappers_run_on_emulated_launches(dtype, monkeypatch):
    """Every TRAIN_KINDS wrapper around the storage restatement of its kernel (tests/backward_ref.py `*_restated`): counted,
    recorded per output, no failure; a layernorm_bwd over `x3[1::2]` of two pairs whose launch read `x3[::2]` fails by name
    with the operands' shapes and strides in the message."""
    sh = _cpu_shadow(monkeypatch)
    n, t, c, heads = 4, 48, 64, 4
    x3, dy, add = _rand((n, t, c), 180, 2.0).to(dtype), _rand((2, t, c), 181).to(dtype), _rand((2, t, c), 182).to(dtype)
    gamma = _rand((c,), 183).float() * 0.2 + 1.0
    rows = lambda v: v.reshape(-1, c)

    def ln_bwd(x, dy_, g, eps, dx_add=None):
        dx, dg, db = R.layernorm_bwd_restated(rows(x), rows(dy_), g, eps, dtype, dx_add=None if dx_add is None else rows(dx_add))
        return dx.reshape(x.shape).to(dtype), dg, db
    sh._layernorm_bwd(ln_bwd, x3[1::2], dy, gamma, 1e-5, dx_add=add)
    assert [r["extra"] for r in sh.records] == ["dx", "dgamma", "dbeta"] and sh.records[0]["form"]["x_strided"]
    sh._colsum(lambda d: R.colsum_restated(d), rows(dy))
    sh._transpose(lambda v: v.t().contiguous(), rows(dy)[:, :40])
    g4 = lambda v: v.reshape(2, 6, 8, c)
    gn = _rand((c,), 184).float() * 0.1
    sh._groupnorm_bwd(lambda x, d, g, b, eps, silu, dx_add=None, one_block_per_group=False:
                      R.groupnorm_bwd_restated(x.reshape(2, -1, c), d.reshape(2, -1, c), g, b, eps, silu, dtype,
                                               dx_add=dx_add.reshape(2, -1, c)).reshape(x.shape).to(dtype),
                      g4(x3[::2].contiguous()), g4(dy), gamma, gn, 1e-5, True, dx_add=g4(add))
    pre = _rand((2, t, 2 * c), 185, 1.5).to(dtype)
    sh._geglu_fwd(lambda p: R.geglu_fwd_restated(p, dtype).to(dtype), pre)
    sh._geglu_bwd(lambda p, d: R.geglu_bwd_restated(p, d, dtype).to(dtype), pre, dy)
    q, k, v = x3[::2], _rand((2, 2, c), 186).to(dtype), _rand((2, 2, c), 187).to(dtype)
    sh._attention_bwd(lambda q_, k_, v_, o_, do_, h_, s_, force_vector=False:
                      tuple(r.to(dtype) for r in R.attention_bwd_restated(q_, k_, v_, do_, h_, s_, dtype, "mfma")),
                      q, k, v, torch.zeros_like(dy), dy, heads, (c // heads) ** -0.5)
    assert [r["extra"] for r in sh.records[-3:]] == ["dq", "dk", "dv"] and sh.records[-1]["form"]["route"] == "mfma"
    assert sh.records[-1]["bound"] == 1.5 * ls.TOL1[dtype] and sh.records[-1]["form"]["tk"] == 2
    sh._sumpool2(lambda s: R.sumpool2_restated(s, dtype).to(dtype), g4(dy))
    z = _rand((4, 512), 188, 2.0).float()
    sh._silu_bwd_f32(lambda z_, d_: R.silu_bwd_restated(z_, d_), z, _rand((4, 512), 189).float())
    from mobi_amd.ldm.modules.diffusionmodules.util import timestep_freqs
    from oracle.unet import timestep_embedding as ref_temb
    sh._timestep_embedding(lambda t_, f_: ref_temb(t_, 2 * f_.shape[0]), torch.tensor([741, 741, 21, 21]), timestep_freqs(64, 10000).float())
    eps, target = _rand((4, 4, 8, 8), 190).float(), _rand((4, 4, 8, 8), 191).float()
    zt = torch.zeros(1)

    def loss(e, g, t_, lv, lw, dtype=None, c_pad=32, **kw):
        rdy, per, terms = loss_grad_ref.loss_grad_ref(e, g, t_, lv, lw, **kw)
        return loss_grad_ref.to_storage(rdy, dtype, c_pad), per.float(), terms.float()
    out = sh._loss_grad(loss, eps, target, torch.tensor([741, 741, 21, 21]), zt, zt, loss_scale=256.0, dtype=dtype)
    assert sh.thin[out[0].data_ptr()] == 1
    assert sh.failures == [], sh.failures
    assert sh.counts == {k: 1 for k in ls.TRAIN_KINDS}
    # the wrong half of the pairs
    sh = _cpu_shadow(monkeypatch)
    sh._layernorm_bwd(lambda x, d, g, eps, dx_add=None: ln_bwd(x3[::2], d, g, eps, dx_add), x3[1::2], dy, gamma, 1e-5, dx_add=add)
    assert sh.failures and all(m.startswith("cpu layernorm_bwd x=(2, 48, 64)/(6144, 64, 1)") for m in sh.failures), sh.failures


def test_a_pinned_launch_is_judged_at_its_written_bound():
    """`pinned={"<kind> #<ordinal> <output>": bound}`: that output of that launch alone is judged at the written bound, with the
    storage restatement's own figure on the same operands recorded beside it; the unpinned launch keeps its unit test's bound and
    its failure carries the operands' diagnosis; a pin whose launch never ran is a failure."""
    dtype = torch.float16
    q, k, v, do = (_rand((1, 64, 32), s).to(dtype) for s in (200, 201, 202, 203))

    def off(q_, k_, v_, o_, do_, h_, s_, force_vector=False):
        dq, dk, dv = (t.to(dtype) for t in R.attention_bwd_ref(q_, k_, v_, do_, h_, s_))
        return (dq.double() * 1.002).to(dtype), dk, dv

    def run(pinned):
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(torch.cuda, "synchronize", lambda *a: None)
            sh = ls.LaunchShadow(mp, label="cpu", pinned=pinned)
            sh.sink = []
            sh._attention_bwd(off, q, k, v, torch.zeros_like(q), do, 4, 8 ** -0.5)
            sh.__exit__(None, None, None)
        return sh
    sh = run(None)
    assert len(sh.failures) == 1 and sh.failures[0].startswith("cpu attention_bwd #1 ") and " dq: " in sh.failures[0]
    assert "restated mfma: dq" in sh.failures[0] and "below 2^-14" in sh.failures[0]
    sh = run({"attention_bwd #1 dq": 5e-3})
    assert sh.failures == [] and [r["bound"] for r in sh.records] == [5e-3, 1.5 * ls.TOL1[dtype], 1.5 * ls.TOL1[dtype]]
    assert sh.records[0]["pinned"] == "attention_bwd #1 dq" and 0 < sh.records[0]["form"]["restated"]["dq"] < ls.TOL1[dtype]
    sh = run({"attention_bwd #2 dq": 5e-3})
    assert len(sh.failures) == 2 and "pinned launch 'attention_bwd #2 dq' did not run" in sh.failures[1]
