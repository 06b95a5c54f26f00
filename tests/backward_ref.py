"""Plain references of the backward kernels (csrc/backward.hip) and of the convolution data gradients of mobi_amd/train.py, for
tests/test_gpu_backward_geometry.py and tests/test_backward_ref_cpu.py.  CPU torch only, no engine code.

Two forms of every operation, both on inputs ALREADY rounded to the storage type:
  * `*_ref`       float64: closed forms (checked against float64 torch.autograd in tests/test_backward_ref_cpu.py) or autograd itself
                  -- what the kernel is measured against;
  * `*_restated`  the same mathematics in fp32 torch with the kernel's documented rounding points: 16-bit outputs are rounded to the
                  storage type; on the matrix-core attention route P and dS are rounded to the storage type before their products;
                  GroupNorm / LayerNorm statistics stay in fp32; the fp32 reductions (column sums, d gamma / d beta) are added in
                  the order the header documents (sixteen-row blocks of four interleaved chains, then the one- or two-stage fold of
                  the per-block partials).  Its own error against the float64 form is what a correct kernel may show: the tests
                  allow a kernel 2x the restatement's row measure.
Two error measures: the whole-tensor rel-L2 the suite has always used, and the ROW measure -- the worst row's error against the
typical row's norm -- which one wrong tail row or one wrong chunk cannot hide in.
"""
import math

import torch
import torch.nn.functional as F


# ----------------------------------------------------------------------------------------------------------------------
# error measures
def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def as_rows(t, block=None):
    """[.., C] -> [rows, C] (a row: one token / pixel of one image with all its channels); block = 64 for fp32 [C] / [n, k]
    results: consecutive 64-element pieces of the flattened tensor (zero-padded at the end)."""
    t = t.detach().double().cpu()
    if block is None:
        return t.reshape(-1, t.shape[-1])
    flat = t.reshape(-1)
    pad = (-flat.numel()) % block
    if pad:
        flat = torch.cat([flat, flat.new_zeros(pad)])
    return flat.view(-1, block)


def row_measure(got, ref, block=None):
    """max over rows of |got_row - ref_row|_2 / rms over the tensor's rows of |ref_row|_2."""
    g, r = as_rows(got, block), as_rows(ref, block)
    scale = float(r.pow(2).sum(1).mean().sqrt().clamp_min(1e-30))
    return float((g - r).pow(2).sum(1).max().sqrt()) / scale


def to_storage(x, dtype):
    """round to the 16-bit storage type and return as fp32."""
    return x.to(dtype).float()


# ----------------------------------------------------------------------------------------------------------------------
# fixed-order fp32 sums (the documented order of mobi_colsum / mobi_layernorm_bwd)
def partial_blocks(rows):
    """include/mobi_engine.h, mobi_backward_partial_blocks: 16 rows per block up to 4,096 blocks."""
    return max(1, min(4096, (rows + 15) // 16))


def _chain(t):
    """fp32 sum over axis 0 in ascending order (one rounding per addition)."""
    s = torch.zeros_like(t[0])
    for i in range(t.shape[0]):
        s = s + t[i]
    return s


def _pad_rows(t, rows):
    if t.shape[0] == rows:
        return t
    return torch.cat([t, t.new_zeros((rows - t.shape[0],) + tuple(t.shape[1:]))])


def fold_partials_restated(partial):
    """fp32 [nblk, L] -> [L]: ascending order; above 64 blocks 64 contiguous ranges first, then the 64 range sums."""
    nblk = partial.shape[0]
    if nblk <= 64:
        return _chain(partial)
    per = (nblk + 63) // 64
    p = _pad_rows(partial, 64 * per).view(64, per, -1)
    return _chain(_chain(p.transpose(0, 1).contiguous()))


def blocked_sum_restated(terms, waves):
    """fp32 [rows, L] -> [L] in the kernels' order: blocks of rows_per_block consecutive rows; inside a block one chain
    (waves = 1: column sums) or four interleaved chains (row r0 + w, + 4, ..) combined as (0 + 1) + (2 + 3); then the fold."""
    rows, length = terms.shape
    nblk = partial_blocks(rows)
    rpb = (rows + nblk - 1) // nblk
    steps = (rpb + waves - 1) // waves
    t = _pad_rows(terms, nblk * rpb).view(nblk, rpb, length)
    if steps * waves != rpb:
        t = torch.cat([t, t.new_zeros((nblk, steps * waves - rpb, length))], 1)
    t = t.view(nblk, steps, waves, length)
    s = _chain(t.transpose(0, 1).contiguous())                 # [nblk, waves, L]
    s = s[:, 0] if waves == 1 else (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])
    return fold_partials_restated(s)


# ----------------------------------------------------------------------------------------------------------------------
# column sums, weight gradient
def colsum_ref(dy):
    return dy.double().sum(0)


def colsum_restated(dy):
    return blocked_sum_restated(dy.float(), 1)


def linear_wgrad_ref(dy, x):
    return dy.double().t() @ x.double()


def linear_wgrad_restated(dy, x):
    """rows % 32 == 0: the matrix cores (fp32 sums of exact products; torch's fp32 product).  Any other row count runs on
    mobi_linear_f32, which the header documents as ONE fp32 FMA chain per output with k (here: the rows) ascending -- the products
    of two 16-bit values are exact in fp32, so the chain is one rounded addition per row, in order."""
    dy, x = dy.float(), x.float()
    if dy.shape[0] % 32 == 0:
        return dy.t() @ x
    acc = torch.zeros((dy.shape[1], x.shape[1]), dtype=torch.float32)
    for r in range(dy.shape[0]):
        acc += torch.outer(dy[r], x[r])
    return acc


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
def layernorm_bwd_ref(x, dy, gamma, eps, dx_add=None, dt=torch.float64):
    """x, dy [rows, C], gamma [C] -> dx [rows, C], d gamma [C], d beta [C] (closed form, in `dt`)."""
    x, dy, gamma = x.to(dt), dy.to(dt), gamma.to(dt)
    mean = x.mean(1, keepdim=True)
    d = x - mean
    rstd = (d.pow(2).mean(1, keepdim=True) + eps).rsqrt()
    xh = d * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if dx_add is not None:
        dx = dx + dx_add.to(dt)
    return dx, (dy * xh).sum(0), dy.sum(0)


def layernorm_bwd_restated(x, dy, gamma, eps, dtype, dx_add=None):
    x, dy, gamma = x.float(), dy.float(), gamma.float()
    mean = x.mean(1, keepdim=True)
    d = x - mean
    rstd = (d.pow(2).mean(1, keepdim=True) + eps).rsqrt()
    xh = d * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if dx_add is not None:
        dx = dx + dx_add.float()
    dgb = blocked_sum_restated(torch.cat([dy * xh, dy], 1), 4)
    c = x.shape[1]
    return to_storage(dx, dtype), dgb[:c], dgb[c:]


# ----------------------------------------------------------------------------------------------------------------------
# GEGLU on the un-fused projection: pre [rows, 2 inner] = [value | gate]
def _geglu(pre, dh, dt):
    inner = pre.shape[-1] // 2
    v, g = pre[..., :inner].to(dt), pre[..., inner:].to(dt)
    cdf = 0.5 * (1.0 + torch.erf(g * 0.7071067811865476))
    pdf = 0.3989422804014327 * torch.exp(-0.5 * g * g)
    h = v * g * cdf
    if dh is None:
        return h, None
    d = dh.to(dt)
    return h, torch.cat([d * g * cdf, d * v * (cdf + g * pdf)], -1)


def geglu_fwd_ref(pre):
    return _geglu(pre, None, torch.float64)[0]


def geglu_bwd_ref(pre, dh):
    return _geglu(pre, dh, torch.float64)[1]


def geglu_fwd_restated(pre, dtype):
    return to_storage(_geglu(pre, None, torch.float32)[0], dtype)


def geglu_bwd_restated(pre, dh, dtype):
    return to_storage(_geglu(pre, dh, torch.float32)[1], dtype)


# ----------------------------------------------------------------------------------------------------------------------
# element-wise and pooling
def add_ref(a, b):
    return a.double() + b.double()


def add_restated(a, b, dtype):
    return to_storage(a.float() + b.float(), dtype)


def _pool(src):
    n, h2, w2, c = src.shape
    v = src.view(n, h2 // 2, 2, w2 // 2, 2, c)
    return (v[:, :, 0, :, 0] + v[:, :, 0, :, 1]) + (v[:, :, 1, :, 0] + v[:, :, 1, :, 1])


def sumpool2_ref(src):
    return _pool(src.double())


def sumpool2_restated(src, dtype):
    return to_storage(_pool(src.float()), dtype)


def _silu_bwd(z, dy):
    sg = torch.sigmoid(z)
    return dy * sg * (1.0 + z * (1.0 - sg))


def silu_bwd_ref(z, dy):
    return _silu_bwd(z.double(), dy.double())


def silu_bwd_restated(z, dy):
    return _silu_bwd(z.float(), dy.float())


def adamw_ref(p, grads, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, dt=torch.float64):
    """torch.optim.AdamW's update over len(grads) steps (closed form, in `dt`); returns (p, exp_avg, exp_avg_sq)."""
    p = p.to(dt).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    b1, b2 = betas
    for step, g in enumerate(grads, 1):
        g = g.to(dt)
        p = p * (1.0 - lr * weight_decay)
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def adamw_restated(p, grads, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
    """fp32 throughout, the scalars included (mobi_adamw_step takes them as floats: 1 - beta, 1 - beta^step and their
    quotients are fp32 values)."""
    import numpy as np
    f = np.float32
    p = p.float().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    b1, b2, lr, eps, wd, one = f(betas[0]), f(betas[1]), f(lr), f(eps), f(weight_decay), f(1.0)
    for step, g in enumerate(grads, 1):
        g = g.float()
        bc1, bc2s = one - f(b1 ** f(step)), np.sqrt(one - f(b2 ** f(step)))
        p = p * float(one - lr * wd)
        m = float(b1) * m + float(one - b1) * g
        v = float(b2) * v + float(one - b2) * g * g
        p = p - float(lr / bc1) * m / (v.sqrt() / float(bc2s) + float(eps))
    return p, m, v


# ----------------------------------------------------------------------------------------------------------------------
# attention backward, head by head (the 4096 x 4096 case holds a handful of [tq, tk] matrices of one head at a time)
def _attention_bwd(q, k, v, dout, heads, scale, dt, round_to=None, o_stored=None):
    n, tq, c = dout.shape
    tk, dh = k.shape[1], c // heads
    dq = torch.empty((n, tq, c), dtype=dt)
    dk = torch.empty((n, tk, c), dtype=dt)
    dv = torch.empty((n, tk, c), dtype=dt)
    rnd = (lambda t: t) if round_to is None else (lambda t: t.to(round_to).to(dt))
    for i in range(n):
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            qh, kh, vh, doh = q[i, :, sl].to(dt), k[i, :, sl].to(dt), v[i, :, sl].to(dt), dout[i, :, sl].to(dt)
            p = torch.softmax((qh @ kh.t()) * scale, -1)
            dp = doh @ vh.t()
            if o_stored is None:
                dvec = (p * dp).sum(1, keepdim=True)
            else:
                dvec = (doh * o_stored[i, :, sl].to(dt)).sum(1, keepdim=True)
            ds = dp.sub_(dvec).mul_(p).mul_(scale)
            del dp
            p, ds = rnd(p), rnd(ds)
            dv[i, :, sl] = p.t() @ doh
            dq[i, :, sl] = ds @ kh
            dk[i, :, sl] = ds.t() @ qh
    return dq, dk, dv


def attention_bwd_ref(q, k, v, dout, heads, scale):
    """q [n, tq, c], k, v [n, tk, c], dout [n, tq, c] -> dq, dk, dv float64 of softmax(q k^T scale) v per head."""
    return _attention_bwd(q, k, v, dout, heads, scale, torch.float64)


def attention_fwd_ref(q, k, v, heads, scale):
    n, tq, c = q.shape
    dh = c // heads
    o = torch.empty((n, tq, c), dtype=torch.float64)
    for i in range(n):
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            o[i, :, sl] = torch.softmax((q[i, :, sl].double() @ k[i, :, sl].double().t()) * scale, -1) @ v[i, :, sl].double()
    return o


def attention_bwd_restated(q, k, v, dout, heads, scale, dtype, route, o_stored=None):
    """route "mfma": P and dS rounded to the storage type before their products (the matrix-core passes); "vector": fp32
    throughout.  o_stored: the A/B form of the row term, D = do . o with the output as it was stored."""
    out = _attention_bwd(q, k, v, dout, heads, scale, torch.float32, round_to=dtype if route == "mfma" else None, o_stored=o_stored)
    return tuple(to_storage(t, dtype) for t in out)


def attention_bwd_route(dh, strides, pointers, force_vector):
    """The host's rule (include/mobi_engine.h, mobi_attention_bwd_params.force_vector): the matrix-core passes when the head
    dim is a multiple of 8 whose 16-padded width is 16 / 32 / 48 / 64 / 80 / 160, every stride a multiple of 8 elements and
    every pointer 16-byte aligned; else the vector passes."""
    ok = dh % 8 == 0 and (dh + 15) // 16 in (1, 2, 3, 4, 5, 10) and all(s % 8 == 0 for s in strides) and all(p % 16 == 0 for p in pointers)
    return "mfma" if ok and not force_vector else "vector"


# ----------------------------------------------------------------------------------------------------------------------
# GroupNorm (32 groups) (+ SiLU) backward, data gradient: x, dy [n, hw, C]
def _groupnorm_bwd(x, dy, gamma, beta, eps, silu, dt):
    n, hw, c = x.shape
    x, dy, gamma, beta = x.to(dt), dy.to(dt), gamma.to(dt), beta.to(dt)
    xg = x.view(n, hw, 32, c // 32)
    mean = xg.mean((1, 3), keepdim=True)
    d = xg - mean
    rstd = (d.pow(2).mean((1, 3), keepdim=True) + eps).rsqrt()
    xh = d * rstd
    ga, be = gamma.view(1, 1, 32, c // 32), beta.view(1, 1, 32, c // 32)
    dxh = dy.view(n, hw, 32, c // 32)
    if silu:
        z = xh * ga + be
        sg = torch.sigmoid(z)
        dxh = dxh * (sg * (1.0 + z * (1.0 - sg)))
    dxh = dxh * ga
    dx = rstd * (dxh - dxh.mean((1, 3), keepdim=True) - xh * (dxh * xh).mean((1, 3), keepdim=True))
    return dx.reshape(n, hw, c)


def groupnorm_bwd_ref(x, dy, gamma, beta, eps, silu, dx_add=None):
    dx = _groupnorm_bwd(x, dy, gamma, beta, eps, silu, torch.float64)
    return dx if dx_add is None else dx + dx_add.double()


def groupnorm_bwd_restated(x, dy, gamma, beta, eps, silu, dtype, dx_add=None):
    dx = _groupnorm_bwd(x, dy, gamma, beta, eps, silu, torch.float32)
    return to_storage(dx if dx_add is None else dx + dx_add.float(), dtype)


# ----------------------------------------------------------------------------------------------------------------------
# convolution data gradients: dy [n, ho, wo, cout] NHWC, weight [cout, cin, kh, kw] -> dx [n, h, w, cin]
def _conv_dgrad(dy, weight, in_hw, stride, upsample, dt):
    n, cout = dy.shape[0], dy.shape[3]
    cin, kh = weight.shape[1], weight.shape[2]
    x = torch.zeros((n, cin) + tuple(in_hw), dtype=dt, requires_grad=True)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if upsample else x
    y = F.conv2d(xin, weight.to(dt), None, stride=stride, padding=kh // 2)
    y.backward(dy.to(dt).permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1).contiguous()


def conv_dgrad_ref(dy, weight, in_hw, stride=1, upsample=False):
    """float64 autograd through F.conv2d (padding kh // 2), after F.interpolate(nearest, x2) when `upsample`."""
    return _conv_dgrad(dy, weight, in_hw, stride, upsample, torch.float64)


def conv_dgrad_restated(dy, weight, in_hw, dtype, stride=1, upsample=False):
    """fp32 on the weight as the engine stores it (rounded to the storage type); the result rounded to the storage type; for
    nearest x2 the data gradient at the doubled size is rounded, then its 2 x 2 sums are (two launches, two stored tensors)."""
    w = to_storage(weight, dtype)
    if not upsample:
        return to_storage(_conv_dgrad(dy, w, in_hw, stride, False, torch.float32), dtype)
    big = to_storage(_conv_dgrad(dy, w, (2 * in_hw[0], 2 * in_hw[1]), 1, False, torch.float32), dtype)
    return sumpool2_restated(big, dtype)
