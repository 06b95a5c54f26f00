"""Forward attention (mobi_attention, csrc/attention.hip) in plain torch on the CPU: the float64 reference, the storage
restatement of each kernel, the per-(image, query, head) row measure and the operand builder of
tests/test_gpu_attention_forward.py.  Nothing here needs a GPU (tests/test_attention_ref_cpu.py runs it alone).

Operands are always handed over as [n, tq, C] / [n, tk, C] / [n, tk, C] tensors (V as rows); the V^T forms exist only in the
device views the builder makes."""
import math

import torch

from oracle import weights as W
from tests.launch_shadow import attention_reference

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
BODIES = (1, 2, 3, 4, 5, 6, 8, 10)          # the KS instantiations of attention_kernel (launch_attention_v)


def route(dh, v_rows, v3=True):
    """Which kernel of csrc/attention.hip a launch runs, as read from launch_attention_v, and the two facts the restatement
    needs: whether the kernel rounds Q' = Q * scale * log2(e) itself (attention_rows_kernel, 'Q fragments, scaled once'),
    whether the denominator is a column of ones riding in P.V, i.e. the sum of the ROUNDED probabilities
    (attention_rows_kernel: ONES = QSH || (KS & 1); attention_kernel: ONES = dh < DT * 32, i.e. dh % 32 != 0), and whether
    the probabilities are rounded under a shift other than the row maximum (attention_rows_kernel: rows_kernel_shifts)."""
    ks = (dh + 15) // 16
    if v_rows and ks <= 5 and v3:
        qsh = dh % 16 != 0
        return dict(kernel="attention_rows_kernel", ks=ks, qsh=qsh, scales_q=True, ones=qsh or ks % 2 == 1, shifted=True,
                    body=f"rows<{ks},{'QSH' if qsh else 'C'}>")
    body = min(b for b in BODIES if b >= ks)
    return dict(kernel="attention_kernel", ks=body, qsh=False, scales_q=False, ones=dh % 32 != 0, shifted=False,
                body=f"exact<{body}>")


def restated_args(r, nw=4):
    """(kernel_scales_q, ones, rows_shift) of `restated` for a route; nw: waves per block of the launch (MOBI_ATTN_NW)."""
    return r["scales_q"], r["ones"], ((r["qsh"], nw) if r["shifted"] else None)


def _heads(x, heads):
    """[n, t, C] -> [n, heads, t, dh]"""
    n, t, c = x.shape
    return x.reshape(n, t, heads, c // heads).permute(0, 2, 1, 3)


def _tokens(x):
    """[n, heads, t, dh] -> [n, t, C]"""
    n, h, t, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(n, t, h * d)


def reference(q, k, v, heads, scale, v_rows=True, q_log2_scaled=False):
    """float64, softmax spelled out as max / exp / sum (tests/launch_shadow.attention_reference).  v: [n, tk, C] when v_rows,
    else V^T [n, C, tk]."""
    return attention_reference(dict(q=q, k=k, v=v, heads=heads, scale=scale, v_rows=v_rows, q_log2_scaled=q_log2_scaled),
                               dev=torch.device("cpu"))


def probabilities(q, k, heads, scale, q_log2_scaled=False):
    """float64 softmax rows [n, heads, tq, tk]."""
    s = _heads(q.double(), heads) @ _heads(k.double(), heads).transpose(-1, -2) * (LN2 if q_log2_scaled else scale)
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    return e / e.sum(dim=-1, keepdim=True)


def effective_keys(q, k, heads, scale, q_log2_scaled=False):
    """1 / sum p^2 per (image, head, query) row of the float64 softmax: how many keys a row really mixes."""
    return 1.0 / probabilities(q, k, heads, scale, q_log2_scaled).pow(2).sum(-1)


def rows_kernel_shifts(t, dtype, qsh, nw=4):
    """The shift attention_rows_kernel subtracts from each exponent before it rounds the probability, per (row, key), and the
    row's final shift.  t: [n, heads, tq, tk] fp32 exponents of two.

    The kernel does NOT round P relative to the row maximum (csrc/attention.hip, the comment above AttnBias and raise_shift):
      * the first shift is the maximum of the first 32 keys + BIAS (8 for bf16, 4 for fp16): 'float d = mx + BIAS';
      * per 32-key half of a full tile the shift stays unless a ROUNDED probability of one of the wave's 32 queries reaches
        2.0 ('orr & 0x40004000u', wave-uniform); every query of the wave then moves by max(its half's maximum + BIAS, 0);
      * the halves of the ragged last tile always take that step ('tile(std::true_type{}, ...)');
      * where the shift rides in Q' (QSH) it is a value of T ('const T new_q = (T)(old_q - d)') and the full tiles of the
        first attempt are not tested; a block (32 NW queries) with a denominator outside (0, 1e30) repeats with the test.
    So the largest probability of a row is 2^-BIAS times a fraction, not 1.0: it carries a rounding error of its own, which
    a ones-column denominator cancels and the unrounded sum of dh = 32 / 64 does not (measured on the MI355X before this was
    restated: kernel rows at 1.6 - 2.04 x the true-maximum restatement on exactly those two head dims, <= 1.5 x elsewhere)."""
    bias = 8.0 if dtype == torch.bfloat16 else 4.0
    rt = lambda x: x.to(dtype).float()
    n, h, tq, tk = t.shape
    blk = 32 * nw
    pad = (-tq) % blk
    if pad:                                  # rows past tq are q = 0: every exponent 0, they never trip the test
        t = torch.cat([t, t.new_zeros(n, h, pad, tk)], dim=2)
    rows = t.shape[2]
    tw = t.view(n, h, rows // 32, 32, tk)
    nfull = tk // 64

    def one_pass(tested):
        s = tw[..., :min(32, tk)].amax(-1) + bias
        s = rt(s) if qsh else s
        skey = torch.empty_like(tw)
        for j in range((tk + 31) // 32):
            cols = slice(32 * j, min(tk, 32 * j + 32))
            e = tw[..., cols] - s.unsqueeze(-1)
            if j // 2 >= nfull:
                fire = torch.ones_like(s, dtype=torch.bool)
            elif tested:
                p = rt(torch.exp2(e))
                fire = (~(p < 2.0)).flatten(-2).any(-1)[..., None].expand_as(s)
            else:
                fire = torch.zeros_like(s, dtype=torch.bool)
            raised = s + (e.amax(-1) + bias).clamp_min(0.0)
            s = torch.where(fire, rt(raised) if qsh else raised, s)
            skey[..., cols] = s.unsqueeze(-1)
        return skey, s

    skey, s = one_pass(not qsh)
    if qsh:
        den = (rt(torch.exp2(tw - skey)) * torch.exp2(skey - s.unsqueeze(-1))).sum(-1)
        bad = ~((den > 0) & (den < 1.0e30))
        bad = bad.reshape(n, h, rows // blk, blk).any(-1)[..., None].expand(n, h, rows // blk, blk).reshape(s.shape)
        if bool(bad.any()):
            skey2, s2 = one_pass(True)
            skey, s = torch.where(bad.unsqueeze(-1), skey2, skey), torch.where(bad, s2, s)
    return skey.reshape(n, h, rows, tk)[:, :, :tq], s.reshape(n, h, rows)[:, :, :tq]


def restated_parts(q, k, v, heads, scale, q_log2_scaled, dtype, kernel_scales_q, ones, rows_shift=None):
    """The pieces of `restated` before the division: (numerator [n, heads, tq, dh], denominator [n, heads, tq], the shift of
    the exponents -- the row maximum, or attention_rows_kernel's final shift -- [n, heads, tq]), all fp32."""
    qh, kh, vh = (_heads(t.float(), heads) for t in (q, k, v))
    cexp = torch.tensor(1.0 if q_log2_scaled else scale, dtype=torch.float32)
    if not q_log2_scaled:
        cexp = cexp * torch.tensor(LOG2E, dtype=torch.float32)         # mobi_attention: p->scale * 1.4426950408889634f
    if kernel_scales_q:
        # attention_rows_kernel: f[j] = (T)((float)f[j] * cexp) -- with q_log2_scaled cexp is 1 and q stays bit for bit
        qh = (qh * cexp).to(dtype).float()
        t = qh @ kh.transpose(-1, -2)
    else:
        # attention_kernel: exp2(fma(s, cexp, -m * cexp)) on the fp32 product of the stored q and k
        t = (qh @ kh.transpose(-1, -2)) * cexp
    if rows_shift is None:
        m = t.amax(dim=-1)
        p = torch.exp2(t - m.unsqueeze(-1))
        back = 1.0
    else:
        # attention_rows_kernel: each probability is rounded under the shift in force at its 32-key half; O and the running
        # sum are carried to the final shift in fp32 ('alpha = exp2(-d)')
        qsh, nw = rows_shift
        skey, m = rows_kernel_shifts(t, dtype, qsh, nw)
        p = torch.exp2(t - skey)
        back = torch.exp2(skey - m.unsqueeze(-1))
    pr = p.to(dtype).float() * back             # P is rounded to T before P.V (pack2 / the (T) casts in front of the MFMA)
    den = (pr if ones else p * back).sum(-1)    # a ones column accumulates what the matrix core was fed; else 'psum += e0 + e1'
    return pr @ vh, den, m


def restated(q, k, v, heads, scale, q_log2_scaled, dtype, kernel_scales_q, ones, rows_shift=None):
    """The same operation in fp32 torch with the kernel's documented rounding points and nothing else: single pass; Q' rounded
    where the kernel scales q itself; P rounded to T -- relative to the true row maximum for attention_kernel, under
    attention_rows_kernel's shift where rows_shift = (QSH, NW) says so (route(...)['qsh'], waves per block); the
    denominator from the rounded P where a ones column carries it; the output rounded to T.  Returns [n, tq, C] fp32."""
    num, den, _ = restated_parts(q, k, v, heads, scale, q_log2_scaled, dtype, kernel_scales_q, ones, rows_shift)
    return _tokens((num / den.unsqueeze(-1)).to(dtype).float())


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def head_rows(x, heads):
    x = x.detach().double().cpu()
    return x.reshape(-1, x.shape[-1] // heads)


def head_row_measure(got, ref, heads):
    """backward_ref.row_measure with the head as part of the row: a row is one (image, query, head) slice of dh values; the
    worst row's |got - ref|_2 over the rms of |ref row|_2 over the tensor."""
    g, r = head_rows(got, heads), head_rows(ref, heads)
    scale = float(r.pow(2).sum(1).mean().sqrt().clamp_min(1e-30))
    return float((g - r).pow(2).sum(1).max().sqrt()) / scale


def standard_inputs(n, heads, dh, tq, tk, dtype):
    """synth_input x 1.5 for q and k (scores of a few nats: a median of ~12 effective keys at tk ~ 200), x 1 for v, rounded
    to the storage type.  The names carry dh and the token count only: cases that share them share the data."""
    c = heads * dh
    q = (W.synth_input(f"af.q{dh}.{tq}", (n, tq, c)) * 1.5).to(dtype)
    k = (W.synth_input(f"af.k{dh}.{tk}", (n, tk, c)) * 1.5).to(dtype)
    v = W.synth_input(f"af.v{dh}.{tk}", (n, tk, c)).to(dtype)
    return q, k, v


def log2_scaled(q, dh, dtype):
    """Q' = round_T(Q * dh^-0.5 * log2 e): what a caller with the factor folded into to_q hands over (q_log2_scaled)."""
    return (q.float() * (dh ** -0.5 * LOG2E)).to(dtype)


def extremes(kind, q, k):
    """The score extremes of test_attention_shift_path (tests/test_gpu_ops.py) on fp32 copies of q and k."""
    q, k = q.float().clone(), k.float().clone()
    tk = k.shape[1]
    if kind == "ramp":                       # scores that keep rising along the keys
        k = k * torch.linspace(0.2, 6.0, tk).view(1, tk, 1)
    elif kind == "huge":                     # scores of magnitude ~1e3
        k, q = k * 60.0, q * 8.0
    elif kind == "negative":                 # every score far below zero
        q, k = q.abs() + 1.0, -(k.abs() + 1.0) * 4.0
    elif kind == "spike":                    # one late dominant key
        k[:, tk - 3] = q[:, 0:1].mean(1) * 9.0
    else:
        raise ValueError(kind)
    return q, k


# ----------------------------------------------------------------------------------------------------------------------
FORMS = ("dense", "stacked", "partner")
V_FORMS = ("rows", "vt", "vt_aligned", "vt_ragged")


class Operands:
    """fp32 CPU copies (q, k, v as rows) and the device views (qd, kd, vd: vd is [n, tk, C] rows or V^T [n, C, tk]) of one
    case; `buffers` are the allocations the views live in, `unchanged()` compares them bit for bit with what was uploaded."""

    def __init__(self, q, k, v, qd, kd, vd, v_rows, buffers):
        self.q, self.k, self.v, self.qd, self.kd, self.vd, self.v_rows = q.float(), k.float(), v.float(), qd, kd, vd, v_rows
        self.buffers = buffers
        self._bits = [b.view(torch.int16).clone() for b in buffers]

    def unchanged(self):
        return all(torch.equal(b.view(torch.int16), s) for b, s in zip(self.buffers, self._bits))


def build_operands(q, k, v, form="dense", v_form="rows", device="cuda"):
    """q [n, tq, C], k, v [n, tk, C]: CPU tensors of the storage type.  Every element of the device buffers that is not an
    operand is NaN: rows beyond tq / tk, gap columns, unused images, the tail of a padded V^T row.
      dense      one allocation per operand, no gaps (V^T forms: [n, C, tk] unless padded below)
      stacked    q | k | v as thirds of one [n, T + 2, 3 C + 8] buffer, T = max(tq, tk) (a V^T operand is its own buffer and
                 the v third stays NaN)
      partner    buffers of 2 n images: q is every even image, k and v every odd one (the cross-modal call), one spare
                 row per image
      v_form     rows | vt (row stride tk) | vt_aligned (tk rounded up to 8, plus 8) | vt_ragged (tk + 3)"""
    assert form in FORMS and v_form in V_FORMS
    dtype = q.dtype
    n, tq, c = q.shape
    tk = k.shape[1]
    v_rows = v_form == "rows"
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=dtype)
    bufs = []

    def up(t):
        d = t.to(device)
        bufs.append(d)
        return d

    step, first = (2, 1) if form == "partner" else (1, 0)
    if form == "stacked":
        t = max(tq, tk) + 2
        s = nan(n, t, 3 * c + 8)
        s[:, :tq, :c], s[:, :tk, c:2 * c] = q, k
        if v_rows:
            s[:, :tk, 2 * c:3 * c] = v
        sd = up(s)
        qd, kd, vd = sd[:, :tq, :c], sd[:, :tk, c:2 * c], sd[:, :tk, 2 * c:3 * c]
    elif form == "partner":
        qb, kb, vb = nan(2 * n, tq + 1, c), nan(2 * n, tk + 1, c), nan(2 * n, tk + 1, c)
        qb[0::2, :tq], kb[1::2, :tk], vb[1::2, :tk] = q, k, v
        qd, kd = up(qb)[0::2, :tq], up(kb)[1::2, :tk]
        vd = up(vb)[1::2, :tk] if v_rows else None
    else:
        qd, kd = up(q.clone()), up(k.clone())
        vd = up(v.clone()) if v_rows else None
    if not v_rows:
        stride = {"vt": tk, "vt_aligned": (tk + 7) // 8 * 8 + 8, "vt_ragged": tk + 3}[v_form]
        vt = nan(step * n, c, stride)
        vt[first::step, :, :tk] = v.permute(0, 2, 1)
        vd = up(vt)[first::step, :, :tk]
    return Operands(q, k, v, qd, kd, vd, v_rows, bufs)
