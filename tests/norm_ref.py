"""A helper, not a test: GroupNorm(32) (+ SiLU) and LayerNorm as mobi_groupnorm / mobi_layernorm state them
(include/mobi_engine.h), for tests/test_gpu_norm_groups.py and tests/test_norm_ref_cpu.py.

  reference / ln_reference   the float64 contract on the STORED inputs (channels-last [n, hw, c0 (+ c1)], all four out_modes,
                             the fp32 source, the split source: slabs ascending from zero, + bias, + rowvec, + residual, one
                             rounding -- `finish_slabs`, in fp32, is bit for bit what the launch must reconstruct);
  restated / ln_restated     the same operation in fp32 torch, rounded ONCE to the storage type where the output is 16-bit and
                             not at all where it is fp32; `perm` sums the pixels (LayerNorm: the channels) in another order,
                             `hook` lets tests/test_norm_ref_cpu.py seed a fault;
  measures, all against float64: (a) rel-L2 per (image, group) / per row, (b) rel-L2 per (image, channel) / per channel over
                             all rows, (c) the statistics recovered from the rounded output of a launch WITHOUT SiLU -- the
                             least-squares line of (y - beta) / gamma over x on a group's elements has slope rstd and root mean --
                             as |rstd_fit / rstd - 1| and |mean_fit - mean| rstd, (d) the whole-tensor rel-L2;
  judge / ln_judge           the criteria of tests/test_gpu_norm_groups.py on one output;
  Operands / LnOperands      every operand a view inside a NaN-filled allocation with guard elements on both sides.
The launch plan is never restated here: `decode_plan` only unpacks what mobi_groupnorm_kernel_variant answers."""
import ctypes as C
import dataclasses

import torch

from oracle import weights as W
from tests.igemm_ref import _bits, place

FORM_NAMES = ("two", "precise", "lds", "regs", "slabs", "chunks")      # MOBI_GN_FORM_* of include/mobi_engine.h
TWO, PRECISE, LDS, REGS, SLABS, CHUNKS = range(6)
MARGIN = 2.0                                    # kernel / restated (criterion 3 of tests/test_gpu_igemm_rows.py)
TOL_F32 = 2e-6                                  # test_groupnorm_fp32_source_and_precise_outputs
KNOBS = ("MOBI_GN_FUSED", "MOBI_GN_COOP", "MOBI_GN_SPLIT_PW4")


def storage_name(dtype):
    return {torch.float16: "f16", torch.bfloat16: "bf16"}[dtype]


def tolerance(dtype, f32_out=False):
    from tests.test_gpu_ops import TOL
    return TOL_F32 if f32_out else TOL[dtype]


def decode_plan(v):
    """The packing include/mobi_engine.h documents for mobi_groupnorm_kernel_variant (MOBI_GN_PLAN_*)."""
    assert v >= 0, v
    return dict(form=v & 15, gb=v >> 4 & 63, pw=v >> 10 & 15, items=v >> 14 & 63, threads=v >> 20 & 2047)


def body_of(plan):
    """(threads, items, pw) of a register-form plan."""
    return plan["threads"], plan["items"], plan["pw"]


def decode_ln(v):
    assert v >= 0, v
    return v & 255, v >> 8                                            # MAXV, LPR


# ----------------------------------------------------------------------------------------------------------------------
# GroupNorm
@dataclasses.dataclass(frozen=True)
class Case:
    n: int
    hw: int
    c0: int
    c1: int = 0
    knobs: tuple = ()                 # ((environment variable, value), ...) the case runs under
    src_f32: bool = False
    out_mode: int = 0                 # 0: T;  1: T hi | lo;  2: f32;  3: T hi | lo | hi
    eps: float = 1e-5
    splits: int = 0                   # > 0: src0 arrives as this many fp32 slabs (mobi_split_source)
    bias: bool = False
    rowvec: str = ""                  # "", "dense", "strided"
    residual: str = ""                # "", "dense", "strided"
    finished: bool = False
    row_extra: int = 0                # slab row_stride - c0

    @property
    def C(self):
        return self.c0 + self.c1

    @property
    def cpg(self):
        return self.C // 32

    @property
    def f32_out(self):
        return self.out_mode == 2


def finish_slabs(slabs, bias, rowvec, res, dtype):
    """mobi_split_source's contract in fp32, one operation after the other: slabs [s][n][hw][row] ascending from zero,
    + bias[c], + rowvec[image][c], + residual, one rounding to T."""
    acc = torch.zeros_like(slabs[0])
    for s in range(slabs.shape[0]):
        acc = acc + slabs[s]
    if bias is not None:
        acc = acc + bias
    if rowvec is not None:
        acc = acc + rowvec[:, None, :]
    if res is not None:
        acc = acc + res.float()
    return acc.to(dtype)


def host_operands(case, dtype):
    """The operands of a case on the CPU, already in their stored types: data 2 z + 0.7 (the second source plain z) as
    test_groupnorm has it, gamma / beta from W.synth_param.  A split source's `x0` is the finished tensor by the contract."""
    c = case
    tag = f"{c.n}.{c.hw}.{c.c0}.{c.c1}"
    o = dict(x1=None, slabs=None, bias=None, rowvec=None, res=None)
    o["gamma"] = torch.from_numpy(W.synth_param("g.weight", (c.C,)))
    o["beta"] = torch.from_numpy(W.synth_param("g.bias", (c.C,)))
    if c.c1:
        o["x1"] = W.synth_input("gn2." + tag, (c.n, c.hw, c.c1)).to(dtype)
    if not c.splits:
        x = W.synth_input("gn." + tag, (c.n, c.hw, c.c0)) * 2.0 + 0.7
        o["x0"] = x if c.src_f32 else x.to(dtype)
        return o
    row = c.c0 + c.row_extra
    target = W.synth_input("gn." + tag, (c.n, c.hw, c.c0)) * 2.0 + 0.7
    slabs = W.synth_input("gns." + tag, (c.splits, c.n, c.hw, row)) * 0.5
    slabs[..., :c.c0] += target / c.splits
    slabs[..., c.c0:] = float("nan")                                  # columns of the producer's padding: never read
    o["slabs"] = slabs
    if c.bias:
        o["bias"] = torch.from_numpy(W.synth_param("gns.bias", (c.c0,))) * 4.0
    if c.rowvec:
        o["rowvec"] = W.synth_input("gnv." + tag, (c.n, c.c0)) * 0.3
    if c.residual:
        o["res"] = (W.synth_input("gnr." + tag, (c.n, c.hw, c.c0)) * 0.8).to(dtype)
    o["x0"] = finish_slabs(slabs[..., :c.c0], o["bias"], o["rowvec"], o["res"], dtype)
    return o


def source(case, o, dtype=torch.float64):
    x = o["x0"].to(dtype)
    return x if o["x1"] is None else torch.cat([x, o["x1"].to(dtype)], dim=2)


def by_group(t):
    """[n, hw, C] -> [n * 32, hw * C / 32]: one row per (image, group)."""
    n, hw, ch = t.shape
    return t.reshape(n, hw, 32, ch // 32).permute(0, 2, 1, 3).reshape(n * 32, hw * (ch // 32))


def silu(y):
    return y * torch.sigmoid(y)


def reference(case, o, with_silu):
    """float64 -> (y [n, hw, C], mean [n * 32], rstd [n * 32])."""
    x = source(case, o)
    g = by_group(x)
    mean = g.mean(1)
    var = (g - mean[:, None]).pow(2).mean(1)
    rstd = 1.0 / torch.sqrt(var + case.eps)
    per = lambda v: v.reshape(case.n, 1, 32, 1).expand(case.n, 1, 32, case.cpg).reshape(case.n, 1, case.C)
    y = (x - per(mean)) * per(rstd) * o["gamma"].double() + o["beta"].double()
    return (silu(y) if with_silu else y), mean, rstd


def shaped(case, y32, dtype):
    """An fp32 result in the launch's output form: one rounding to T (mode 0), hi | lo (| hi) (1, 3), fp32 as it is (2)."""
    if case.out_mode == 2:
        return y32
    hi = y32.to(dtype)
    if case.out_mode == 0:
        return hi
    lo = (y32 - hi.float()).to(dtype)
    return torch.cat([hi, lo] + ([hi] if case.out_mode == 3 else []), dim=2)


def restated(case, o, dtype, with_silu, perm=None, hook=None):
    """fp32 torch.  perm: a permutation of the pixels the sums run over (the output comes back in the true order).  hook: a dict
    of callables for seeded faults -- "x"(x [n, hw, C]) -> x as the kernel reads it; "stats"(mean_c, var_c [n, C]) and
    "affine"(gamma_c, beta_c [n, C]) edit the per-channel tables in place; "y"(y, out) edits the stored output."""
    hook = hook or {}
    x = source(case, o, torch.float32)
    if "x" in hook:
        x = hook["x"](x)
    xs = x if perm is None else x[:, perm].contiguous()
    g = by_group(xs)
    mean = g.sum(1) / g.shape[1]
    var = (g - mean[:, None]).pow(2).sum(1) / g.shape[1]
    per = lambda v: v.reshape(case.n, 32, 1).expand(case.n, 32, case.cpg).reshape(case.n, case.C).clone()
    mean_c, var_c = per(mean), per(var)
    gamma_c, beta_c = o["gamma"].expand(case.n, case.C).clone(), o["beta"].expand(case.n, case.C).clone()
    if "stats" in hook:
        hook["stats"](mean_c, var_c)
    if "affine" in hook:
        hook["affine"](gamma_c, beta_c)
    rstd_c = 1.0 / torch.sqrt(var_c + case.eps)
    y = (xs - mean_c[:, None]) * rstd_c[:, None] * gamma_c[:, None] + beta_c[:, None]
    if with_silu:
        y = silu(y)
    if perm is not None:
        y = y[:, torch.argsort(perm)].contiguous()
    out = shaped(case, y, dtype)
    if "y" in hook:
        out = hook["y"](out)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# measures, on [groups, elements] float64
def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def rows_rel(got, ref):
    """rel-L2 of every row of [rows, elements] -> [rows]."""
    return (got - ref).pow(2).sum(1).sqrt() / ref.pow(2).sum(1).sqrt().clamp_min(1e-30)


def fitted(y, x, gamma, beta):
    """y, x, gamma, beta as [groups, elements] float64, y without SiLU -> (rstd_fit, mean_fit, usable): the least-squares line
    of t = (y - beta) / gamma over x.  A group whose elements are all equal has no line (usable False)."""
    t = (y - beta) / gamma
    mx, mt = x.mean(1, keepdim=True), t.mean(1, keepdim=True)
    sxx = (x - mx).pow(2).sum(1)
    sxt = ((x - mx) * (t - mt)).sum(1)
    usable = sxx > 0
    slope = sxt / torch.where(usable, sxx, torch.ones_like(sxx))
    icpt = mt[:, 0] - slope * mx[:, 0]
    ok = usable & (slope != 0)
    mean_fit = -icpt / torch.where(ok, slope, torch.ones_like(slope))
    return slope, mean_fit, ok


def stat_figures(y, x, gamma, beta, mean, rstd):
    """measure (c): (worst |rstd_fit / rstd - 1|, worst |mean_fit - mean| rstd) over the groups that have a line; a group whose
    fitted slope is zero (an output that does not follow its input at all) counts as deviation 1."""
    slope, mean_fit, ok = fitted(y, x, gamma, beta)
    has_line = (x - x.mean(1, keepdim=True)).pow(2).sum(1) > 0
    if not bool(has_line.any()):
        return 0.0, 0.0
    d_r = torch.where(ok, (slope / rstd - 1.0).abs(), torch.ones_like(rstd))[has_line]
    d_m = torch.where(ok, (mean_fit - mean).abs() * rstd, torch.ones_like(rstd))[has_line]
    return float(d_r.max()), float(d_m.max())


def figures(case, o, out, ref, with_silu):
    """Measures (a) - (d) of one output in the launch's form (modes 1 / 3: of its hi part) against reference()."""
    y64, mean, rstd = ref
    y = out.detach().cpu()[..., :case.C].double()
    fig = {"rel": rel_l2(y, y64),
           "group": float(rows_rel(by_group(y), by_group(y64)).max()),
           "channel": float(rows_rel(y.transpose(1, 2).reshape(-1, case.hw), y64.transpose(1, 2).reshape(-1, case.hw)).max())}
    if not with_silu:
        per = lambda v: by_group(v.double().expand(case.n, case.hw, case.C))
        fig["rstd"], fig["mean"] = stat_figures(by_group(y), by_group(source(case, o)), per(o["gamma"]), per(o["beta"]), mean, rstd)
    return fig


def judge(case, dtype, out, ref, rest_fig, o, with_silu, margin=MARGIN):
    """Criteria 1 - 4 of tests/test_gpu_norm_groups.py on one output -> (figures, failures); `rest_fig` = figures() of the
    restatement: every limit comes from the reference side."""
    out = out.detach().cpu()
    fig, bad = {}, {}
    nonfinite = int((~torch.isfinite(out)).sum())
    if nonfinite:
        bad["finite"] = f"{nonfinite} non-finite outputs"
        out = torch.nan_to_num(out.float(), nan=0.0, posinf=0.0, neginf=0.0)
    got = figures(case, o, out, ref, with_silu)
    tol = tolerance(dtype, case.f32_out)
    for k, v in got.items():
        fig[k], fig[k + ".restated"] = v, rest_fig[k]
        if k == "rel":
            if not v < tol:
                bad[k] = f"rel-L2 {v:.3e} >= {tol:.1e}"
        elif not v <= margin * rest_fig[k]:
            bad[k] = f"{k} measure {v:.3e} > {margin:g} x restated {rest_fig[k]:.3e}"
    return fig, bad


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm
@dataclasses.dataclass(frozen=True)
class LnCase:
    images: int
    rows: int
    C: int
    src_gap: int = 0                  # elements between images beyond dense (multiples of 8)
    out_gap: int = 0
    eps: float = 1e-5


def ln_operands(case, dtype):
    tag = f"{case.images}.{case.rows}.{case.C}"
    return dict(x=(W.synth_input("ln." + tag, (case.images, case.rows, case.C)) * 2.0 + 0.7).to(dtype),
                gamma=torch.from_numpy(W.synth_param("ln.weight", (case.C,))),
                beta=torch.from_numpy(W.synth_param("ln.bias", (case.C,))))


def ln_reference(case, o):
    x = o["x"].double().reshape(-1, case.C)
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt((x - mean[:, None]).pow(2).mean(1) + case.eps)
    return (x - mean[:, None]) * rstd[:, None] * o["gamma"].double() + o["beta"].double(), mean, rstd


def ln_restated(case, o, dtype, perm=None, hook=None):
    """fp32 torch on [rows, C]; perm: a permutation of the channels the sums run over; hook "stats"(mean, var [rows])."""
    x = o["x"].float().reshape(-1, case.C)
    xs = x if perm is None else x[:, perm].contiguous()
    mean = xs.sum(1) / case.C
    var = (xs - mean[:, None]).pow(2).sum(1) / case.C
    if hook and "stats" in hook:
        hook["stats"](mean, var)
    y = (x - mean[:, None]) / torch.sqrt(var + case.eps)[:, None] * o["gamma"] + o["beta"]
    return y.to(dtype)


def ln_figures(case, o, out, ref):
    y64, mean, rstd = ref
    y = out.detach().cpu().double().reshape(-1, case.C)
    x = o["x"].double().reshape(-1, case.C)
    fig = {"rel": rel_l2(y, y64), "group": float(rows_rel(y, y64).max()), "channel": float(rows_rel(y.t(), y64.t()).max())}
    fig["rstd"], fig["mean"] = stat_figures(y, x, o["gamma"].double().expand_as(x), o["beta"].double().expand_as(x), mean, rstd)
    return fig


def ln_judge(case, dtype, out, ref, rest_fig, o, margin=MARGIN):
    out = out.detach().cpu()
    fig, bad = {}, {}
    nonfinite = int((~torch.isfinite(out)).sum())
    if nonfinite:
        bad["finite"] = f"{nonfinite} non-finite outputs"
        out = torch.nan_to_num(out.float(), nan=0.0, posinf=0.0, neginf=0.0)
    got = ln_figures(case, o, out, ref)
    tol = tolerance(dtype)
    for k, v in got.items():
        fig[k], fig[k + ".restated"] = v, rest_fig[k]
        if k == "rel":
            if not v < tol:
                bad[k] = f"rel-L2 {v:.3e} >= {tol:.1e}"
        elif not v <= margin * rest_fig[k]:
            bad[k] = f"{k} measure {v:.3e} > {margin:g} x restated {rest_fig[k]:.3e}"
    return fig, bad


# ----------------------------------------------------------------------------------------------------------------------
# parameters
def fill_params(case, dtype, ptr, with_silu):
    """-> (GroupNormParams, SplitSource or None); `ptr`: name -> address.  The caller keeps both alive over the call."""
    from mobi_amd import _lib
    p = _lib.GroupNormParams()
    p.src0, p.src1 = ptr.get("x0"), ptr.get("x1")
    p.c0, p.c1, p.batch, p.hw = case.c0, case.c1, case.n, case.hw
    p.gamma, p.beta, p.eps, p.silu = ptr["gamma"], ptr["beta"], case.eps, int(with_silu)
    p.out, p.ws, p.dtype = ptr["out"], ptr["ws"], {torch.float16: 0, torch.bfloat16: 1}[dtype]
    p.src_f32, p.out_mode, p.sync = int(case.src_f32), case.out_mode, None
    ss = None
    if case.splits:
        ss = _lib.SplitSource()
        ss.slabs, ss.count, ss.row_stride = ptr["slabs"], case.splits, case.c0 + case.row_extra
        ss.bias, ss.rowvec, ss.rowvec_stride = ptr.get("bias"), ptr.get("rowvec"), ptr.get("rowvec_stride", 0)
        ss.residual, ss.res_img_stride, ss.finished = ptr.get("res"), ptr.get("res_img_stride", 0), ptr.get("finished")
        p.src0_split = C.pointer(ss)
    return p, ss


def fake_pointers(case):
    """16-byte-aligned non-NULL addresses for the query, which launches nothing."""
    a = 1 << 20
    ptr = dict(gamma=a, beta=a, out=a, ws=a)
    for name, on in (("x0", not case.splits), ("x1", case.c1 > 0), ("slabs", case.splits > 0), ("bias", case.bias),
                     ("rowvec", bool(case.rowvec)), ("res", bool(case.residual)), ("finished", case.finished)):
        if on:
            ptr[name] = a
    return ptr


def query(lib, case, dtype=torch.float16):
    """mobi_groupnorm_kernel_variant for the case under the environment as it stands: the packed plan or the error."""
    p, ss = fill_params(case, dtype, fake_pointers(case), True)
    return lib.mobi_groupnorm_kernel_variant(C.byref(p))


def ln_params(case, dtype, ptr, strides=(0, 0)):
    from mobi_amd import _lib
    p = _lib.LayerNormParams()
    p.src, p.out, p.images, p.rows_per_image, p.channels = ptr["x"], ptr["out"], case.images, case.rows, case.C
    p.src_img_stride, p.out_img_stride = strides
    p.gamma, p.beta, p.eps, p.dtype = ptr["gamma"], ptr["beta"], case.eps, {torch.float16: 0, torch.bfloat16: 1}[dtype]
    return p


def ln_query(lib, C_):
    a = 1 << 20
    p = ln_params(LnCase(1, 1, C_), torch.float16, dict(x=a, out=a, gamma=a, beta=a))
    return lib.mobi_layernorm_kernel_variant(C.byref(p))


# ----------------------------------------------------------------------------------------------------------------------
# operands on the device
class _Placed:
    """Shared bookkeeping: the inputs' bits as uploaded, the bytes outside every output view."""

    def _watch(self, inputs, outputs):
        from tests.launch_shadow import OutsideView
        self.inputs = [p for p in inputs if p is not None]
        self._in_bits = [_bits(p.buffer).clone() for p in self.inputs]
        self.outputs = [p for p in outputs if p is not None]
        self._outside = [OutsideView(p.view) for p in self.outputs]
        self._out0 = [_bits(p.buffer).clone() for p in self.outputs]

    def reset_outputs(self):
        for p, b in zip(self.outputs, self._out0):
            _bits(p.buffer).copy_(b)

    def unchanged(self):
        return all(torch.equal(_bits(p.buffer), b) for p, b in zip(self.inputs, self._in_bits))

    def outside_unchanged(self):
        return all(v.unchanged() for v in self._outside)


class Operands(_Placed):
    """The device side of one (case, dtype): sources, second source, gamma, beta, output, slabs, bias, rowvec, residual and
    `finished`, each a view inside a NaN-filled allocation (igemm_ref.place); the workspace starts as NaN too (the statistics
    launch writes every partial sum the apply launch reads)."""

    def __init__(self, lib, case, dtype, o, device="cuda"):
        c = case
        pix = lambda ch: 8 * (ch // 8 + 1)                            # guard: more than one pixel's channels
        dense = lambda t, guard: None if t is None else place(t.reshape(1, -1), t.numel(), device, guard)
        self.x0 = None if c.splits else place(o["x0"], c.hw * c.c0, device, pix(c.c0))
        self.x1 = None if o["x1"] is None else place(o["x1"], c.hw * c.c1, device, pix(c.c1))
        self.gamma, self.beta = dense(o["gamma"], 8), dense(o["beta"], 8)
        self.slabs, self.bias = dense(o["slabs"], pix(c.c0 + c.row_extra)), dense(o["bias"], 8)
        self.ptr = ptr = {}
        self.rowvec = self.res = self.finished = None
        if o["rowvec"] is not None:
            rs = c.c0 + (12 if c.rowvec == "strided" else 0)
            self.rowvec = place(o["rowvec"], rs, device, 8)
            ptr["rowvec_stride"] = rs if c.rowvec == "strided" else 0
        if o["res"] is not None:
            gap = 8 * c.c0 + 8 if c.residual == "strided" else 0
            self.res = place(o["res"], c.hw * c.c0 + gap, device, pix(c.c0))
            ptr["res_img_stride"] = c.hw * c.c0 + gap if gap else 0
        if c.finished:
            self.finished = place(torch.full((c.n, c.hw, c.c0), float("nan"), dtype=dtype), c.hw * c.c0, device, pix(c.c0))
        width = c.C * {0: 1, 1: 2, 2: 1, 3: 3}[c.out_mode]
        out_t = torch.float32 if c.out_mode == 2 else dtype
        self.out = place(torch.full((c.n, c.hw, width), float("nan"), dtype=out_t), c.hw * width, device, pix(width))
        nbytes = lib.mobi_groupnorm_workspace_bytes(c.n, c.hw)
        self.ws = torch.full((nbytes // 4 + 8,), float("nan"), dtype=torch.float32, device=device)
        for name in ("x0", "x1", "gamma", "beta", "slabs", "bias", "rowvec", "res", "finished", "out"):
            if getattr(self, name) is not None:
                ptr[name] = getattr(self, name).view.data_ptr()
        ptr["ws"] = self.ws.data_ptr()
        self._watch([self.x0, self.x1, self.gamma, self.beta, self.slabs, self.bias, self.rowvec, self.res],
                    [self.out, self.finished])


class LnOperands(_Placed):
    def __init__(self, case, dtype, o, device="cuda"):
        c = case
        dense = c.rows * c.C
        guard = 8 * (c.C // 8 + 1)
        self.x = place(o["x"], dense + c.src_gap, device, guard)
        self.out = place(torch.full((c.images, c.rows, c.C), float("nan"), dtype=dtype), dense + c.out_gap, device, guard)
        self.gamma = place(o["gamma"].reshape(1, -1), c.C, device, 8)
        self.beta = place(o["beta"].reshape(1, -1), c.C, device, 8)
        self.strides = (dense + c.src_gap if c.src_gap else 0, dense + c.out_gap if c.out_gap else 0)
        self.ptr = dict(x=self.x.view.data_ptr(), out=self.out.view.data_ptr(), gamma=self.gamma.view.data_ptr(),
                        beta=self.beta.view.data_ptr())
        self._watch([self.x, self.gamma, self.beta], [self.out])
