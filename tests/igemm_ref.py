"""The implicit GEMM (mobi_igemm, csrc/igemm.hip + csrc/igemm_plan.hip + csrc/igemm_small.hip) in plain torch on the CPU: the float64 reference of
the contract in include/mobi_engine.h, the fp32 restatement with the kernels' rounding points, the row / channel measures, the
a-priori fp32 bound, the operand builder and the launch plan of tests/test_gpu_igemm_rows.py.  Nothing here calls the engine or
needs a GPU (tests/test_igemm_ref_cpu.py runs it alone); the builder only needs one when asked for device views.

A case is a `Case`; its host operands (`host_operands`) are tensors ALREADY rounded to the storage type:
  x  [n, hin, win, c0]   x2 [n, hin, win, c1] | None   w [groups, n_packed, taps * C] (k = tap * C + c)
  bias f32 [n_packed] | None   rowvec f32 [n, cout] | None   res [n, hw, cout] | None   svec f32 [n_packed] | None
Outputs are [n, hw, cout] ("rows": MOBI_OUT_ROWS / MOBI_OUT_ROWS_F32) or [n, cout, hw] (MOBI_OUT_TRANSPOSED)."""
import dataclasses
import math
from typing import Optional

import torch
import torch.nn.functional as F

from oracle import weights as W

U32 = 2.0 ** -24                        # unit roundoff of fp32
STAGED_128, STAGED_256, DIRECT_LDS, PINGPONG, RING_128, RING_256, RING_128W, SMALL = range(8)   # MOBI_IGEMM_* (mobi_engine.h)
BODY_NAMES = ("staged128", "staged256", "direct_lds", "pingpong", "ring128", "ring256", "ring128w", "small")
COMPUTE_UNITS = 256                     # MI355X (compute_units() of csrc/igemm_plan.hip; also its answer without a device)
LN_EPS = 1e-5


@dataclasses.dataclass(frozen=True)
class Case:
    n: int
    hin: int
    win: int
    c0: int
    cout: int
    c1: int = 0
    kh: int = 1
    kw: int = 1
    stride: int = 1
    pad_h: int = 0
    pad_w: int = 0
    upsample: bool = False
    hout: Optional[int] = None          # None: (logical size + 2 pad - k) // stride + 1
    wout: Optional[int] = None
    groups: int = 1
    bias: bool = True
    rowvec: bool = False
    residual: str = ""                  # "" | "dense" | "strided" | "inplace" (out IS the residual's view)
    scale: float = 1.0
    epilogue: str = ""                  # "" | "leaky" | "geglu"
    out_mode: str = "rows"              # "rows" | "tr" | "f32"
    ln: bool = False                    # LayerNorm folded into the launch (ln_svec)
    split_k: int = 0
    finish: str = ""                    # split_k > 1: "" reduce launch | "sync" in-launch finish | "defer" + mobi_igemm_finish
    w_tiled: bool = False               # weight_tiled handed over
    src_strided: bool = False           # src_img_stride beyond dense (one source only: the ABI's rule)
    out_strided: bool = False
    rowvec_strided: bool = False
    w_gap: int = 0                      # elements between the per-group matrices beyond dense (groups > 1)
    seed: str = ""                      # cases with equal geometry and seed share their data

    # ---- derived geometry -------------------------------------------------------------------------------------------
    @property
    def C(self):
        return self.c0 + self.c1

    @property
    def taps(self):
        return self.kh * self.kw

    @property
    def ktot(self):
        return self.taps * self.C

    @property
    def logical(self):
        return (2 * self.hin, 2 * self.win) if self.upsample else (self.hin, self.win)

    @property
    def ho(self):
        return self.hout if self.hout is not None else (self.logical[0] + 2 * self.pad_h - self.kh) // self.stride + 1

    @property
    def wo(self):
        return self.wout if self.wout is not None else (self.logical[1] + 2 * self.pad_w - self.kw) // self.stride + 1

    @property
    def hw(self):
        return self.ho * self.wo

    @property
    def m(self):
        return self.n * self.hw

    @property
    def geglu(self):
        return self.epilogue == "geglu"

    @property
    def n_packed(self):
        return 2 * self.cout if self.geglu else self.cout

    @property
    def data_key(self):
        return (self.n, self.hin, self.win, self.c0, self.c1, self.cout, self.kh, self.kw, self.groups, self.geglu, self.ho,
                self.wo, self.ln, self.seed)


def storage_name(dtype):
    return "fp16" if dtype == torch.float16 else "bf16"


# ----------------------------------------------------------------------------------------------------------------------
# data
def host_operands(case, dtype):
    """Every operand a case can use (a case reads the ones it names), deterministic in the case's geometry: activations and
    residual N(0, 1) (N(1, 1) under a LayerNorm fold: the mean term must not vanish; the second source scaled by
    sqrt(c0 / c1) so that both carry the same share of the sum), weights N(0, 1 / k), bias and the per-image vector
    N(0, 0.5^2) -- large enough for a wrong index to move a channel far beyond the bound."""
    name = "ig." + ".".join(str(v) for v in case.data_key)
    syn = lambda leaf, shape: W.synth_input(name + "." + leaf, shape)
    x = syn("x", (case.n, case.hin, case.win, case.c0)) + (1.0 if case.ln else 0.0)
    x2 = syn("x2", (case.n, case.hin, case.win, case.c1)) * math.sqrt(case.c0 / case.c1) if case.c1 else None
    w = syn("w", (case.groups, case.n_packed, case.ktot)) / math.sqrt(case.ktot)
    if case.ln:                                                 # W diag(gamma): the fold of ops.fold_layernorm
        w = w * (1.0 + 0.3 * syn("gamma", (case.ktot,)))
    w = w.to(dtype)
    return dict(x=x.to(dtype), x2=None if x2 is None else x2.to(dtype), w=w,
                bias=0.5 * syn("bias", (case.n_packed,)), rowvec=0.5 * syn("rowvec", (case.n, case.cout)),
                res=syn("res", (case.n, case.hw, case.cout)).to(dtype),
                svec=w.double().sum(dim=2)[0].float())          # ops.with_row_sums: row sums of the ROUNDED matrix


def used(case, h):
    """The operands of `h` this case hands to the launch (None for the others)."""
    return dict(x=h["x"], x2=h["x2"], w=h["w"], bias=h["bias"] if case.bias else None,
                rowvec=h["rowvec"] if case.rowvec else None, res=h["res"] if case.residual else None,
                svec=h["svec"] if case.ln else None)


# ----------------------------------------------------------------------------------------------------------------------
# gather
def tap_index(case, tap, clamp=False):
    """Source pixel (sy, sx) and validity of every output pixel for one tap: top / left padding pad_h / pad_w, reads past
    the bottom / right edge zero, nearest x2 upsampling.  clamp: every read is valid and lands on the nearest pixel (the
    input conditions' contrast, never the contract)."""
    hl, wl = case.logical
    p = torch.arange(case.hw)
    oy, ox = p // case.wo, p % case.wo
    ly = oy * case.stride - case.pad_h + tap // case.kw
    lx = ox * case.stride - case.pad_w + tap % case.kw
    ok = (ly >= 0) & (ly < hl) & (lx >= 0) & (lx < wl)
    sy, sx = ly.clamp(0, hl - 1), lx.clamp(0, wl - 1)
    if case.upsample:
        sy, sx = sy // 2, sx // 2
    return sy, sx, (torch.ones_like(ok) if clamp else ok)


def gathered(case, x, x2, tap, dtype, clamp=False):
    """[n, hw, C] in `dtype`: the rows of A for one tap, the two sources concatenated on channels."""
    src = x if x2 is None else torch.cat([x, x2], dim=3)
    sy, sx, ok = tap_index(case, tap, clamp)
    return src[:, sy, sx].to(dtype) * ok.to(dtype)[None, :, None]


def im2col(case, x, x2, dtype, clamp=False):
    """[n, hw, taps * C], k = tap * C + c."""
    return torch.cat([gathered(case, x, x2, t, dtype, clamp) for t in range(case.taps)], dim=2)


def per_image(case, t):
    """[groups, ...] -> [n, ...]: image i uses matrix i // (n / groups)."""
    return t.repeat_interleave(case.n // case.groups, dim=0)


def product(case, o, dtype=torch.float64, clamp=False, absolute=False):
    """sum_k A[m][k] W[n][k] as ONE matmul per tap, [n, hw, n_packed] in `dtype` (absolute: sum |a| |w|)."""
    f = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    w = per_image(case, f(o["w"]).reshape(case.groups, case.n_packed, case.taps, case.C))
    acc = torch.zeros((case.n, case.hw, case.n_packed), dtype=dtype)
    for tap in range(case.taps):
        a = gathered(case, o["x"], o["x2"], tap, dtype, clamp)
        acc += (a.abs() if absolute else a) @ w[:, :, tap].transpose(1, 2)
    return acc


def ln_rows(case, o, dtype=torch.float64):
    """The 1 x 1 launch's own input rows [n, hw, C] (a LayerNorm-folded launch has one source, stride 1, no padding)."""
    return o["x"].reshape(case.n, case.hw, case.C).to(dtype)


def geglu_pairs(v):
    """packed columns (ops.pack_geglu: per 16, 8 value columns then the 8 gate columns of the same outputs) -> (value, gate)."""
    t = v.reshape(*v.shape[:-1], v.shape[-1] // 16, 2, 8)
    return t[..., 0, :].reshape(*v.shape[:-1], -1), t[..., 1, :].reshape(*v.shape[:-1], -1)


def _finish_layout(case, v):
    return v.transpose(1, 2).contiguous() if case.out_mode == "tr" else v


def rows_of(case, out):
    """[n, hw, cout] whatever the output mode."""
    return out.transpose(1, 2) if case.out_mode == "tr" else out


# ----------------------------------------------------------------------------------------------------------------------
# the contract
def reference(case, o, clamp=False, leaky_after_residual=False, pre_activation=False):
    """float64 restatement of mobi_igemm_params: out = residual + leaky( scale * sum + bias + rowvec ), GEGLU as
    value * gelu_erf(gate) of the packed pairs (before rowvec: the ABI refuses GEGLU with rowvec or residual), the LayerNorm
    fold as rstd (x W'^T - mean svec) + bias with the statistics of the raw rows.  `o`: used(case, host_operands(...)).
    The keyword arguments are for the CPU tests' contrasts only."""
    acc = product(case, o, torch.float64, clamp)
    if case.ln:
        r = ln_rows(case, o)
        mean = r.mean(dim=2, keepdim=True)
        var = (r - mean).square().mean(dim=2, keepdim=True)
        acc = (acc - mean * o["svec"].double()) / torch.sqrt(var + LN_EPS)
    v = acc * case.scale
    if o["bias"] is not None:
        v = v + o["bias"].double()
    if case.geglu:
        val, gate = geglu_pairs(v)
        v = val * F.gelu(gate)
    if o["rowvec"] is not None:
        v = v + o["rowvec"].double()[:, None, :]
    if pre_activation:
        return v
    res = None if o["res"] is None else o["res"].double()
    if leaky_after_residual and res is not None:
        v, res = v + res, None
    if case.epilogue == "leaky":
        v = F.leaky_relu(v, 0.1)
    if res is not None:
        v = v + res
    return _finish_layout(case, v)


def magnitude(case, o):
    """A = |scale| sum |x| |w| + |bias| + |rowvec| + |residual| per output element (rows layout, fp64): the scale of the
    a-priori bound below, for the epilogues an fp32 output can have (plain, leaky, LayerNorm fold; GEGLU writes T only).
    Leaky: |leaky(v)| <= |v| and leaky is 1-Lipschitz, so A stands and the 0.1 v product is one more rounding.
    LayerNorm fold, out = rstd (acc - mean svec) + bias with one-pass fp32 statistics (ln_fold_acc): to first order in u,
      |d mean| <= k u m1                    (m1 = sum |x| / k: a k-term fp32 sum)
      |d var|  <= (k + 2) u (m2 + 2 |mean| m1)   (var = m2 - mean^2, m2 = sum x^2 / k: the cancellation term)
      |d rstd| / rstd <= |d var| / (2 (var + eps)) + 2 u      (rsqrtf to ~1 ulp)
      |d out|  <= rstd (|d acc| + |d mean| |svec| + 2 u |mean svec|) + |d rstd| |acc - mean svec| + u |out|
    which (k + 8) u A covers with
      A = rstd (sum |x| |w| + (|mean| + m1) |svec|) + |rstd (acc - mean svec)| ((m2 + 2 |mean| m1) / (2 (var + eps)) + 2) + |bias|."""
    a = product(case, o, torch.float64, absolute=True) * abs(case.scale)
    if case.ln:
        r = ln_rows(case, o)
        mean, m1, m2 = r.mean(2, keepdim=True), r.abs().mean(2, keepdim=True), r.square().mean(2, keepdim=True)
        var = (r - mean).square().mean(2, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + LN_EPS)
        sv = o["svec"].double()
        folded = rstd * (product(case, o, torch.float64) - mean * sv)
        a = rstd * (a + (mean.abs() + m1) * sv.abs()) + folded.abs() * ((m2 + 2 * mean.abs() * m1) / (2 * (var + LN_EPS)) + 2)
    if o["bias"] is not None:
        a = a + o["bias"].double().abs()
    if o["rowvec"] is not None:
        a = a + o["rowvec"].double().abs()[:, None, :]
    if o["res"] is not None:
        a = a + o["res"].double().abs()
    return a


def f32_bound(case, o):
    """Element-wise bound of |fp32 result - exact| for ANY summation order: (k + 8) 2^-24 A.  The products of two 16-bit
    values are exact in fp32; a term passes through at most k - 1 additions of the k-sum, the scale, bias, rowvec, leaky
    and residual: k + 4 roundings, (k + 4) u A to first order; the remaining 4 u cover the second-order terms.  A split does
    not add to that for the cases here: a term sees the k_s - 1 additions of its own range and at most S slab additions, and
    k_s + S <= k for S <= 8 slabs of at least one 64-deep tile each.  `magnitude` gives A, per epilogue."""
    return (case.ktot + 8) * U32 * magnitude(case, o)


def split_ranges(case, split_k):
    """k ranges of a split launch, split_ranges of csrc/igemm_plan.hip: nk = ceil(k / 64) tiles, nk_per = ceil(nk / split_k) per range, ranges
    never empty ('a.splits = (a.nk + a.nk_per - 1) / a.nk_per')."""
    nk = (case.ktot + 63) // 64
    per = (nk + split_k - 1) // split_k
    count = (nk + per - 1) // per
    return [(s * per * 64, min(case.ktot, (s + 1) * per * 64)) for s in range(count)]


def slab_products(case, o, split_k, dtype, absolute=False):
    """[slabs, n, hw, n_packed]: scale * the partial sum of each k range (what a defer_finish launch leaves in `ws`)."""
    f = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    a = im2col(case, o["x"], o["x2"], dtype)
    a = a.abs() if absolute else a
    w = per_image(case, f(o["w"]))
    sc = abs(case.scale) if absolute else case.scale
    return torch.stack([(a[:, :, k0:k1] @ w[:, :, k0:k1].transpose(1, 2)) * sc for k0, k1 in split_ranges(case, split_k)])


# ----------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic
def restated(case, o, dtype, acc_hook=None, leaky_after_residual=False):
    """The same operation in fp32 torch with the rounding points the kernels document and nothing else (csrc/igemm.hip, cited
    as function + a phrase of the line; the register epilogues are direct_epilogue, ring_register_epilogue and pp_epilogue):
      * operands are T, their products exact, every sum fp32 (the MFMAs accumulate in fp32: `f32x4 acc[NT][..]`);
      * LayerNorm fold: sum and sum of squares of the RAW rows in fp32 (both rowstat_acc overloads), `mean = sm * inv_k`,
        var = max(sumsq / k - mean^2, 0), `rsqrtf(var + a.ln_eps)` and `rstd * (acc[ni][mi] - mean * sv) + bv` (ln_fold_acc);
      * v = acc * scale + bias in fp32 (igemm_epilogue `v = v * scale + bias4[ni]`, twice; direct_epilogue
        `acc[ni][2 * p] * scale`; the ping-pong / 256 x 320 ring register forms start the sums from bias or rowvec
        instead -- another order, no other rounding);
      * GEGLU value * gelu_erf(gate) in fp32 (igemm_epilogue `av[j] * gelu_erf_f(gv[j])`; `xs[r] * gelu_erf_f(ys[r])` in each
        register epilogue);
      * + rowvec (`o[j] += rv[j]`), leaky 0.1 (`0.1f * o[j]`), + residual read as T (`o[j] += rf[j]`, igemm_epilogue and each
        register epilogue), all fp32;
      * split-K: each slab is acc * scale in fp32 (igemm_epilogue `v = v * scale + bias4[ni]` with use_bias false, stored by its
        `*reinterpret_cast<f32x4*>(d) =` copy); the finish sums them in ascending order from `o[j] = 0.f`, then + bias +
        rowvec + residual (igemm_splitk_reduce_kernel);
      * ONE rounding to T (`pack8<T>(o)` in igemm_epilogue's three `st16(outT + ...` stores, in each register epilogue's
        `vm_store16(rowp + ...` and in igemm_splitk_reduce_kernel; `from_f32<T>(o[j])` in igemm_epilogue's ragged transposed
        store); fp32 outputs are stored as they are (`*reinterpret_cast<f32x4*>(outF + off)` in igemm_epilogue and
        igemm_splitk_reduce_kernel).
    acc_hook(acc) -> acc and leaky_after_residual plant faults (tests/test_igemm_ref_cpu.py); a launch has neither.
    Returns fp32 in the case's output layout."""
    f32 = torch.float32
    bias = o["bias"]
    if case.split_k > 1:
        v = torch.zeros((case.n, case.hw, case.n_packed), dtype=f32)
        for s in slab_products(case, o, case.split_k, f32):
            v = v + s
        if acc_hook is not None:
            v = acc_hook(v)
    else:
        acc = product(case, o, f32)
        if acc_hook is not None:
            acc = acc_hook(acc)
        if case.ln:
            r = ln_rows(case, o, f32)
            inv_k = torch.tensor(1.0 / case.ktot, dtype=f32)
            mean = r.sum(dim=2, keepdim=True) * inv_k
            var = (r.square().sum(dim=2, keepdim=True) * inv_k - mean * mean).clamp_min(0.0)
            acc = torch.rsqrt(var + torch.tensor(LN_EPS, dtype=f32)) * (acc - mean * o["svec"])
        v = acc * torch.tensor(case.scale, dtype=f32)
    if bias is not None:
        v = v + bias
    if case.geglu:
        val, gate = geglu_pairs(v)
        v = val * F.gelu(gate)
    if o["rowvec"] is not None:
        v = v + o["rowvec"][:, None, :]
    res = None if o["res"] is None else o["res"].float()
    if leaky_after_residual and res is not None:
        v, res = v + res, None
    if case.epilogue == "leaky":
        v = torch.where(v > 0, v, torch.tensor(0.1, dtype=f32) * v)
    if res is not None:
        v = v + res
    if case.out_mode != "f32":
        v = v.to(dtype).float()
    return _finish_layout(case, v)


# ----------------------------------------------------------------------------------------------------------------------
# measures (all on [n, hw, cout] fp64)
def _rows(case, t):
    return rows_of(case, t.detach().double().cpu())


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def row_measure(case, got, ref):
    """backward_ref.row_measure: the worst (image, pixel) row's |got - ref|_2 over the rms of |ref row|_2."""
    g, r = _rows(case, got).reshape(-1, case.cout), _rows(case, ref).reshape(-1, case.cout)
    scale = float(r.pow(2).sum(1).mean().sqrt().clamp_min(1e-30))
    return float((g - r).pow(2).sum(1).max().sqrt()) / scale


def channel_measure(case, got, ref):
    """The same with a column: one output channel of one image over its pixels (the row of the transposed output)."""
    g = _rows(case, got).transpose(1, 2).reshape(-1, case.hw)
    r = _rows(case, ref).transpose(1, 2).reshape(-1, case.hw)
    scale = float(r.pow(2).sum(1).mean().sqrt().clamp_min(1e-30))
    return float((g - r).pow(2).sum(1).max().sqrt()) / scale


def bound_ratio(got, ref, bound):
    """max |got - ref| / bound (0 / 0 counts as 0)."""
    d = (got.detach().double().cpu() - ref.double()).abs()
    return float(torch.where(d > 0, d / bound.clamp_min(1e-300), torch.zeros_like(d)).max())


def tolerance(case, dtype):
    """Whole-tensor rel-L2 bound the form already has in this project: TOL of tests/test_gpu_ops.py, x 1.5 for a
    LayerNorm-folded product (launch_shadow._igemm, tests/test_gpu_chain.py)."""
    from tests.test_gpu_ops import TOL
    return TOL[dtype] * (1.5 if case.ln else 1.0)


MARGIN = 2.0                            # kernel / restated: the backward and attention suites' margin for another summation order


def judge(case, dtype, got, ref, rest, o):
    """Criteria 1 - 4 of tests/test_gpu_igemm_rows.py on one output -> (figures, failures), both dicts; the keys of
    `failures` name the criterion: finite, rel, row, channel, f32."""
    got = got.detach().cpu()
    fig, bad = {}, {}
    nonfinite = int((~torch.isfinite(got)).sum())
    if nonfinite:
        bad["finite"] = f"{nonfinite} non-finite outputs"
        got = torch.nan_to_num(got.float(), nan=0.0, posinf=0.0, neginf=0.0)
    tol = tolerance(case, dtype)
    fig["rel"], fig["rel.restated"] = rel_l2(got, ref), rel_l2(rest, ref)
    if not fig["rel"] < tol:
        bad["rel"] = f"rel-L2 {fig['rel']:.3e} >= {tol:.1e}"
    if case.out_mode == "f32":
        bound = f32_bound(case, o)
        fig["f32"], fig["f32.restated"] = bound_ratio(got, ref, bound), bound_ratio(rest, ref, bound)
        if not fig["f32"] <= 1.0:
            bad["f32"] = f"|got - ref| reaches {fig['f32']:.3f} x (k + 8) 2^-24 A"
    else:
        for key, measure in (("row", row_measure), ("channel", channel_measure)):
            k, r = measure(case, got, ref), measure(case, rest, ref)
            fig[key], fig[key + ".restated"] = k, r
            if not k <= MARGIN * r:
                bad[key] = f"{key} measure {k:.3e} > {MARGIN:g} x restated {r:.3e}"
    return fig, bad


def input_conditions(case, dtype, o, ref, rest):
    """Conditions on a case's DATA, from the reference alone, without which it could pass by being insensitive -> the list of
    those that do not hold."""
    bad = []
    tol = tolerance(case, dtype)
    row_bound = MARGIN * row_measure(case, rest, ref) if case.out_mode != "f32" else tol
    if case.epilogue == "leaky":
        pre = reference(case, o, pre_activation=True)
        pos = float((pre > 0).double().mean())
        if not 0.25 <= pos <= 0.75:
            bad.append(f"leaky: {pos:.2f} of the pre-activation values are positive")
    hl, wl = case.logical
    reads_outside = (case.pad_h > 0 or case.pad_w > 0 or (case.ho - 1) * case.stride - case.pad_h + case.kh > hl or
                     (case.wo - 1) * case.stride - case.pad_w + case.kw > wl)
    if reads_outside:
        d = row_measure(case, reference(case, o, clamp=True), ref)
        if not d > 10 * row_bound:
            bad.append(f"padding: clamp and zero padding differ by {d:.3e} in the worst row, bound in use {row_bound:.3e}")
    if case.c1:
        z = lambda t: torch.zeros_like(t)
        e0 = float(product(case, dict(o, x2=z(o["x2"]))).square().sum())
        e1 = float(product(case, dict(o, x=z(o["x"]))).square().sum())
        if not min(e0, e1) >= 0.25 * (e0 + e1):
            bad.append(f"two sources: energies {e0:.3e} / {e1:.3e}")
    for key in ("res", "rowvec"):
        if o[key] is not None:
            d = rel_l2(reference(case, dict(o, **{key: None})), ref)
            if not d > 10 * tol:
                bad.append(f"{key} moves the output by {d:.3e} only")
    if case.ln:
        r = ln_rows(case, o)
        q = float((r.mean(2).abs() / r.std(2, unbiased=False)).min())
        if not q >= 0.25:
            bad.append(f"LayerNorm fold: |mean| / std is {q:.3f} in some row")
    return bad


# ----------------------------------------------------------------------------------------------------------------------
# launch plan
def _exact_log2(v):
    s = 0
    while (1 << s) < v:
        s += 1
    return s if (1 << s) == v else -1


def _small_tile(case, t, split_k):
    """small_tile of csrc/igemm_plan.hip."""
    if t("SMALL") == 0:
        return 0
    if t("SMALL") < 0 and (t("WM") in (2, 4) or t("WIDE") >= 0 or t("SM") == 0):
        return 0
    conv3 = case.kh == 3 and case.kw == 3 and case.pad_h == 1 and case.pad_w == 1
    if not (case.kh == 1 and case.kw == 1) and not conv3:
        return 0
    if case.stride != 1 or case.upsample or case.groups != 1 or case.epilogue or split_k > 1:
        return 0
    if case.out_mode == "tr" or case.ho != case.hin or case.wo != case.win:
        return 0
    if case.C % 320 or (case.c1 > 0 and case.c0 % 80) or case.n_packed % 32:
        return 0
    if t("SMALL") > 0:
        return 32
    k = case.ktot
    if conv3:
        return 32 if case.m <= max(t("SMALL_CONV_M"), 0) else 0
    cap = t("SMALL_MFLOP") if t("SMALL_MFLOP") >= 0 else (1000 if k == 320 else 1800)
    return 0 if 2.0 * case.m * case.n_packed * k > 1e6 * cap else 32


def plan(case, knobs=None, cu=COMPUTE_UNITS):
    """The body (MOBI_IGEMM_*) and the sub-forms a launch of `case` takes under the MOBI_IGEMM_* environment `knobs`
    ({'WM': 2, ...}, unset = -1): a restatement of the predicates of igemm_plan (csrc/igemm_plan.hip: pixel_waves,
    wide_tiles, route; the comments below quote the line each one restates) and the instantiation launch_igemm (csrc/igemm.hip) picks, for operands far below 2 GB and
    tap-major k (the only order there is).  The GPU test asserts `body` against mobi_igemm_kernel_variant; nothing in the library reports the other fields
    (sm64, sm_direct, ring_direct, epi_direct / pp, in-launch finish, w_tiled, the kernel symbol): they are a restated claim,
    only as good as this reading of the code."""
    knobs = knobs or {}
    t = lambda k: int(knobs.get(k, -1))
    rows, tr = case.out_mode == "rows", case.out_mode == "tr"
    leaky, geglu, lnf = case.epilogue == "leaky", case.geglu, case.ln
    npk, C, hw = case.n_packed, case.C, case.hw
    bias, rowvec, resid = case.bias, case.rowvec, bool(case.residual)
    split_k = case.split_k if case.split_k > 1 else 0
    M = (case.n // case.groups) * hw                                    # rows of ONE group (`a.M = a.imgs_per_group * a.hw_out`)
    nk = (case.ktot + 63) // 64
    bn = 160 if npk % 160 == 0 else 128
    up = lambda a, b: (a + b - 1) // b
    tiles256 = up(M, 256) * up(npk, bn)                                 # pixel_waves: `const long long tiles256 =` .. `wm = tuning().wm`
    wm = 4 if tiles256 >= 256 else 2
    if split_k and M % 256 == 0 and tiles256 * split_k >= 256 and nk // split_k >= 16:
        wm = 4
    if t("PP_SPLIT") == 0 and split_k and tiles256 < 256:
        wm = 2
    if t("WM") in (2, 4):
        wm = t("WM")
    tiles_m, tiles_n = up(M, 64 * wm), up(npk, bn)
    fast = C % 64 == 0 and (case.c1 == 0 or case.c0 % 64 == 0) and t("FAST") != 0        # `const bool fast =` (extents < 2 GB here)
    glds = t("GLDS") != 0
    sm = wm == 2 and t("SM") != 0                                       # `g.ring_ok && t.sm != 0 ? Body::Ring128` (small operands)
    splits, nk_per = 1, nk
    if split_k:                                                         # `if (p->split_k > 1) {`
        nk_per = up(nk, split_k)
        splits = up(nk, nk_per)
    split_ws = bool(split_k)
    vec_ok = lambda mult: not rowvec or (not bias and hw % mult == 0)
    epi_direct = (wm == 4 and fast and glds and rows and not split_ws and vec_ok(64) and M % 256 == 0 and npk % bn == 0 and
                  nk_per >= 3 and t("EPI_DIRECT") != 0)                 # `const bool epi_direct =`
    shifts = _exact_log2(hw) >= 6 and _exact_log2(case.wo) >= 0
    pp = epi_direct and splits == 1 and case.scale == 1.0 and shifts    # `const bool pp =`, the form without a split
    if split_ws and wm == 4 and fast and glds and not tr and M % 256 == 0 and npk % bn == 0 and nk_per >= 3 and \
            case.scale == 1.0 and shifts:                               # `const bool pp =`, `split ? pp_tiles && !tr`
        pp = True
    if t("PP") == 0:
        pp = False
    wide = 0
    if (wm == 4 or t("WIDE") > 0) and t("WIDE") != 0:                   # wide_tiles: `if (!((wm == 4 || knob > 0) && g.ring_ok`
        bnw = 320 if npk % 160 == 0 else 256
        tn = up(npk, bnw)

        def fills(blocks):
            rounds = up(blocks, 256)
            return blocks >= 190 and blocks * 5 >= rounds * 256 * 4 - 64 * (rounds == 1)
        t256, t128 = up(M, 256) * tn * splits, up(M, 128) * tn * splits
        pick = t("WIDE") if t("WIDE") > 0 else (2 if fills(t256) else (1 if fills(t128) and t("WIDE128") == 1 else 0))
        if t("WIDE") <= 0 and pick == 2 and npk * 2 <= bnw and pp:
            pick = 0
        if not pick and wm == 4 and not pp and (C >= 64 or not rows or npk < 256):
            pick = 2
        if lnf:
            pick = 2 if wm == 4 else 0
        if pick:
            wide, wm, sm = pick, (4 if pick == 2 else 2), False
            tiles_m, tiles_n = up(M, 64 * wm), tn
    k64 = C % 64 == 0 and (case.c1 == 0 or case.c0 % 64 == 0)
    sm64 = sm and k64 and nk_per >= 1 and tiles_m * tiles_n * splits * case.groups <= cu and t("SM64") != 0     # `body = Body::Ring64`
    if t("SM64") == 1 and sm and k64:
        sm64 = True
    dense_groups = case.groups == 1 or case.w_gap == 0
    tileable = case.w_tiled and dense_groups and npk % 16 == 0 and case.ktot % 32 == 0 and t("WTILED") != 0
    w_tiled = tileable and not sm64 and (sm or wide > 0)                # `a.w_tiled =`
    sm_direct = ((sm or wide == 1) and (rows or split_ws) and not tr and M % 128 == 0 and
                 npk % (2 * bn if wide == 1 else bn) == 0 and (split_ws or vec_ok(64)) and t("SM_DIRECT") != 0)    # `a.sm_direct =`
    bnw = 320 if npk % 160 == 0 else 256
    rd = (wide == 2 and rows and not split_ws and case.groups == 1 and vec_ok(128) and M % 256 == 0 and npk % bnw == 0 and
          case.scale == 1.0)
    ring_direct = (rd and not resid and t("RING_DIRECT") != 0) or (rd and resid and t("RING_DIRECT") == 1)        # `a.ring_direct =`
    if leaky:                                                           # `if (leaky) {`
        pp = epi_direct = sm_direct = ring_direct = sm64 = False
        if wm == 4 and npk >= 256:
            wide, sm, tiles_m, tiles_n = 2, False, up(M, 256), up(npk, bnw)
        else:
            wide, wm, sm, tiles_m, tiles_n = 0, 2, True, up(M, 128), up(npk, bn)
        w_tiled = tileable
    small = 0 if lnf or leaky else _small_tile(case, t, split_k)        # `const int small =`
    pp_launch = not wide and wm == 4 and fast and glds and pp
    sync_mode = 0
    if split_ws and case.finish == "sync" and not small and t("FUSED_SPLIT") != 0 and splits <= 4:                # `if (split && p->sync && !small`, in_launch_finish
        mode = 1 if t("FUSED_SPLIT") == 1 else 2
        tiles = tiles_m * tiles_n
        if ((wide or sm) or (pp_launch and tiles <= cu)) and (mode == 1 or tiles % 8 == 0):
            sync_mode = mode
    # mobi_igemm_kernel_variant and launch_igemm
    nt = 5 if npk % 160 == 0 else 4
    flag = lambda b: "1" if b else "0"
    if small:
        body, kernel, epi = SMALL, "small_gemm", "small"
    elif leaky:
        body = RING_256 if wide == 2 else RING_128
        kernel, epi = f"ring<{nt},0,{'8,8' if wide == 2 else '4,4'},lnf0,leaky1>", "staged"
    elif wide == 2:
        body, kernel = RING_256, f"ring<{nt},{flag(tr)},8,8,lnf{flag(lnf)},leaky0>"
        epi = "register" if ring_direct else "staged"
    elif wide == 1:
        body, kernel, epi = RING_128W, f"ring<{nt},0,8,4,lnf0,leaky0>", "register" if sm_direct else "staged"
    elif wm == 4 and fast and glds and pp:
        body, kernel = PINGPONG, f"pp<{nt},geglu{flag(geglu and not split_ws)},slab{flag(split_ws)}>"
        epi = "slab" if split_ws else "register"
    elif wm == 4:
        body = DIRECT_LDS if fast and glds else STAGED_256              # the library has no direct-to-LDS kernel: the
        kernel, epi = f"staged<{nt},{flag(tr)},4>", "staged"            # register-staged one runs (MOBI_IGEMM_BY_TR)
    elif sm and sm64:
        body, kernel = RING_128, f"ring64<{nt},{flag(tr)},lnf{flag(lnf)},ovl{flag(t('SM64_OVL') != 0)}>"
        epi = "register" if sm_direct else "staged"
    elif sm:
        body, kernel = RING_128, f"ring<{nt},{flag(tr)},4,4,lnf{flag(lnf)},leaky0>"
        epi = "register" if sm_direct else "staged"
    else:
        body, kernel, epi = STAGED_128, f"staged<{nt},{flag(tr)},2>", "staged"
    if split_ws and not small:
        epi += ".finish%d" % sync_mode if sync_mode else (".defer" if case.finish == "defer" else ".reduce")
    pixel_tile = 32 if small else 64 * wm
    channel_tile = 32 if small else (bnw if wide == 2 else (2 * bn if wide == 1 else bn))
    return dict(body=body, body_name=BODY_NAMES[body], kernel=kernel, epilogue=epi, nt=nt, wm=wm, wide=wide, sm=bool(sm),
                sm64=bool(sm64), sm_direct=bool(sm_direct), ring_direct=bool(ring_direct), epi_direct=bool(epi_direct),
                pp=bool(pp), w_tiled=bool(w_tiled), sync_mode=sync_mode, splits=splits, small=small, pixel_tile=pixel_tile,
                channel_tile=channel_tile, lds_dma=bool(small == 0 and (wide or sm or leaky or (wm == 4 and fast and glds and pp))),
                ragged_m=M % pixel_tile != 0, ragged_n=npk % channel_tile != 0)


def fill_params(p, case, dtype, ptr, strides=None):
    """Set the fields of a mobi_igemm_params-shaped object `p` (mobi_amd._lib.IgemmParams) for `case`.  ptr: addresses by
    name (src0, src1, weight, weight_tiled, bias, rowvec, residual, out, ws, sync, ln_svec; absent = NULL); strides: the
    image strides of Operands (absent = dense)."""
    s = strides or {}
    for name in ("src0", "src1", "weight", "weight_tiled", "bias", "rowvec", "residual", "out", "ws", "sync", "ln_svec"):
        setattr(p, name, ptr.get(name))
    p.c0, p.c1, p.batch, p.hin, p.win = case.c0, case.c1, case.n, case.hin, case.win
    p.upsample, p.hout, p.wout = int(case.upsample), case.ho, case.wo
    p.kh, p.kw, p.stride, p.pad_h, p.pad_w = case.kh, case.kw, case.stride, case.pad_h, case.pad_w
    p.src_img_stride = s.get("src", 0)
    p.groups = case.groups
    p.w_group_stride = s.get("w", case.n_packed * case.ktot) if case.groups > 1 else 0
    p.n_packed, p.cout = case.n_packed, case.cout
    p.rowvec_stride, p.res_img_stride, p.out_img_stride = s.get("rowvec", 0), s.get("res", 0), s.get("out", 0)
    p.out_mode = {"rows": 0, "tr": 1, "f32": 2}[case.out_mode]
    p.epilogue = {"": 0, "geglu": 1, "leaky": 2}[case.epilogue]
    p.scale = case.scale
    p.dtype = 0 if dtype == torch.float16 else 1            # MOBI_F16 / MOBI_BF16
    p.split_k = case.split_k
    p.k_order = 0
    p.ln_eps = LN_EPS if case.ln else 0.0
    p.defer_finish = 0
    return p


def fake_pointers(case):
    """16-byte-aligned non-NULL addresses for the queries that launch nothing (mobi_igemm_kernel_variant, ..._slab_count)."""
    a = 1 << 20
    ptr = dict(src0=a, weight=a, out=a)
    for name, on in (("src1", case.c1 > 0), ("bias", case.bias), ("rowvec", case.rowvec), ("residual", bool(case.residual)),
                     ("ln_svec", case.ln), ("weight_tiled", case.w_tiled), ("ws", case.split_k > 1),
                     ("sync", case.finish == "sync")):
        if on:
            ptr[name] = a
    return ptr


# ----------------------------------------------------------------------------------------------------------------------
# operands on the device
def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


class Placed:
    """One operand: `view` inside `buffer`, a larger allocation whose every other element is NaN."""

    def __init__(self, buffer, view):
        self.buffer, self.view = buffer, view


def place(values, img_stride, device, guard):
    """values [images, ...] -> a view of the same shape, dense within an image and `img_stride` elements between images,
    `guard` NaN elements in front of and behind it (multiples of 8: 16-byte alignment survives)."""
    n = values.shape[0]
    inner = values[0].numel()
    assert img_stride >= inner and guard % 8 == 0
    buf = torch.full((2 * guard + n * img_stride,), float("nan"), dtype=values.dtype)
    dense = [1] * values.dim()
    for d in range(values.dim() - 2, -1, -1):
        dense[d] = dense[d + 1] * values.shape[d + 1]
    dense[0] = img_stride
    buf.as_strided(values.shape, dense, guard).copy_(values)
    dbuf = buf.to(device)
    assert dbuf.data_ptr() % 16 == 0
    return Placed(dbuf, dbuf.as_strided(values.shape, dense, guard))


class Operands:
    """The device side of one (case, dtype): every operand a view inside a NaN-filled allocation (`place`), image strides
    beyond dense where the case says so, the output view NaN before the launch.  `unchanged()`: the input allocations are
    bit for bit what was uploaded; `outside_unchanged()`: nothing outside the output view was written
    (launch_shadow.OutsideView)."""

    def __init__(self, case, dtype, o, device="cuda"):
        from tests.launch_shadow import OutsideView
        self.case, self.dtype = case, dtype
        c = case
        pix = lambda ch: 8 * ((c.win + 2) * ch // 8 + 1)             # guard: more than one row of pixels
        ips = c.hin * c.win + (3 if c.src_strided else 0)
        assert not (c.src_strided and c.c1)
        self.x = place(o["x"], ips * c.c0, device, pix(c.c0))
        self.x2 = None if o["x2"] is None else place(o["x2"], ips * c.c1, device, pix(c.c1))
        self.src_img_stride = ips * c.c0 if c.src_strided else 0
        wdense = c.n_packed * c.ktot
        self.w = place(o["w"], wdense + c.w_gap, device, 8 * (c.ktot // 8 + 1))
        self.w_group_stride = wdense + c.w_gap
        f32p = lambda t: None if t is None else place(t.reshape(1, -1), t.numel(), device, 8)
        self.bias, self.svec = f32p(o["bias"]), f32p(o["svec"])
        self.rowvec = None
        self.rowvec_stride = 0
        if o["rowvec"] is not None:
            rs = c.cout + (12 if c.rowvec_strided else 0)
            self.rowvec = place(o["rowvec"], rs, device, 8)
            self.rowvec_stride = rs if c.rowvec_strided else 0
        dense_out = c.hw * c.cout
        self.res, self.res_img_stride = None, 0
        if o["res"] is not None:
            gap = 8 * c.cout + 8 if c.residual == "strided" or (c.residual == "inplace" and c.out_strided) else 0
            self.res = place(o["res"], dense_out + gap, device, 8 * (c.cout // 8 + 2))
            self.res_img_stride = dense_out + gap if gap else 0
        out_t = torch.float32 if c.out_mode == "f32" else dtype
        shape = (c.n, c.cout, c.hw) if c.out_mode == "tr" else (c.n, c.hw, c.cout)
        if c.residual == "inplace":
            self.out, self.out_img_stride = self.res, self.res_img_stride
        else:
            gap = 8 * c.cout + 8 if c.out_strided else 0
            self.out = place(torch.full(shape, float("nan"), dtype=out_t), dense_out + gap, device, 8 * (c.cout // 8 + 2))
            self.out_img_stride = dense_out + gap if gap else 0
        self.inputs = [p for p in (self.x, self.x2, self.w, self.bias, self.svec, self.rowvec,
                                   None if c.residual == "inplace" else self.res) if p is not None]
        self._bits = [_bits(p.buffer).clone() for p in self.inputs]
        self.outside = OutsideView(self.out.view)
        self._out0 = _bits(self.out.buffer).clone()

    def reset_output(self):
        """The output allocation as it was before the first launch (NaN, or the residual of an in-place case)."""
        _bits(self.out.buffer).copy_(self._out0)

    def output_untouched(self):
        return torch.equal(_bits(self.out.buffer), self._out0)

    def unchanged(self):
        return all(torch.equal(_bits(p.buffer), b) for p, b in zip(self.inputs, self._bits))

    def outside_unchanged(self):
        return self.outside.unchanged()
