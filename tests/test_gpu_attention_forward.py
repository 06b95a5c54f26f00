"""Forward attention (mobi_attention) per (image, query, head) row: every accepted head dim in the three V forms, the tile
edges of every kernel body, strided operands and outputs through the C ABI, the score extremes on the kernels
test_attention_shift_path does not reach, and the refusals.

Criteria, for every launch (tests/attention_ref.py; tests/test_attention_ref_cpu.py shows what they reject):
  1. the output is finite;
  2. whole-tensor rel-L2 against float64 below TOL of tests/test_gpu_ops.py, x 1.5 where the kernel rounds Q' = Q scale log2(e)
     itself (attention_rows_kernel without q_log2_scaled) -- the rule of launch_shadow._attention;
  3. the head-row measure (worst row's error / rms row norm, a row being the dh values of one image, query and head) at most
     2 x that of the storage restatement -- fp32 torch with the kernel's documented rounding points -- against the same float64
     reference, computed on the CPU beside the case; 2 is the backward suite's margin for a different summation order.
     The restatement rounds Q' where the kernel scales q itself, rounds P to T -- relative to the row maximum for
     attention_kernel, under attention_rows_kernel's own shift schedule (attention_ref.rows_kernel_shifts: its largest
     probability is 2^-BIAS times a fraction, not 1.0) --, sums the rounded P where a ones column carries the denominator,
     and rounds the output.  Measured on the MI355X (profiles/attention_forward_rows.txt): kernel / restated <= 1.05 over
     every launch of this file; with P rounded relative to the true maximum for both kernels it was 1.6 - 2.04 at
     dh = 32 / 64 on V rows, the two instantiations whose denominator does not see that rounding;
  4. a second call returns the same bits;
  5. the standard inputs really mix keys: the median of 1 / sum p^2 is at least 8 (from the reference).
Every kernel and restated figure goes through MOBI_RECORD_ERRORS (tests/golden_cases.record) under a name that starts with
<kernel body>.<layout>.<dtype>; profiles/attention_forward_rows.txt is the worst of them per such triple.
A test collects all its cases' figures before it fails, so one run lists every miss.

Head dim -> instantiation, as read from launch_attention_v (T = f16_t / bf16_t; NW = 4 here unless MOBI_ATTN_NW=8):
  dh        V rows (v_layout 1), default route            V rows with MOBI_ATTN_V3=0        V^T 16-byte rows / ragged rows
  8         attention_rows_kernel<T, 1, NW, true>         attention_kernel<T, 1, 2, 2[, 8]>  attention_kernel<T, 1, 1 / 0, 2>
  16        attention_rows_kernel<T, 1, NW, false>        <T, 1, 2, 2[, 8]>                  <T, 1, 1 / 0, 2>
  24        attention_rows_kernel<T, 2, NW, true>         <T, 2, 2, 2[, 8]>                  <T, 2, 1 / 0, 2>
  32        attention_rows_kernel<T, 2, NW, false>        <T, 2, 2, 2[, 8]>                  <T, 2, 1 / 0, 2>
  40        attention_rows_kernel<T, 3, NW, true>         <T, 3, 2, 2[, 8]>                  <T, 3, 1 / 0, 2>
            (MOBI_ATTN_H16=1: <T, 3, NW, true, true>)
  48        attention_rows_kernel<T, 3, NW, false>        <T, 3, 2, 2[, 8]>                  <T, 3, 1 / 0, 2>
  56        attention_rows_kernel<T, 4, NW, true>         <T, 4, 2, 2[, 8]>                  <T, 4, 1 / 0, 2>
  64        attention_rows_kernel<T, 4, NW, false>        <T, 4, 2, 2[, 8]>                  <T, 4, 1 / 0, 2>
  72        attention_rows_kernel<T, 5, NW, true>         <T, 5, 2, 2[, 8]>                  <T, 5, 1 / 0, 2>
  80        attention_rows_kernel<T, 5, NW, false>        <T, 5, 2, 2[, 8]>                  <T, 5, 1 / 0, 2>
  88, 96    attention_kernel<T, 6, 2, 2>                  the same                           <T, 6, 1 / 0, 2>
  104 - 128 attention_kernel<T, 8, 2, 1>  (104, 112: seven k-steps in the KS = 8 body)       <T, 8, 1 / 0, 1>
  136 - 160 attention_kernel<T, 10, 2, 1> (136, 144: nine k-steps in the KS = 10 body)       <T, 10, 1 / 0, 1>
The denominator is a ones column of P.V (the sum of the ROUNDED probabilities) unless dh is 32 / 64 in attention_rows_kernel
or a multiple of 32 in attention_kernel (attention_ref.route)."""
import ctypes as C
import functools

import pytest
import torch

from tests import attention_ref as A
from tests.golden_cases import record
from tests.test_gpu_ops import DT, TOL

pytestmark = pytest.mark.gpu
N, HEADS = 2, 3
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -4                # include/mobi_engine.h
ALL_DH = list(range(8, 168, 8))
LAYOUTS = {"v_rows": ("rows", 197), "vt_aligned": ("vt", 200), "vt_ragged": ("vt", 197)}


@pytest.fixture(scope="module")
def ops():
    from mobi_amd import ops as o
    return o


def tag(dtype):
    return "fp16" if dtype == torch.float16 else "bf16"


# ----------------------------------------------------------------------------------------------------------------------
# the CPU side of a case, computed once and shared (never written to)
@functools.lru_cache(maxsize=64)
def cpu_inputs(dh, tq, tk, dtype, qlog, kind):
    """(q, k, v of the storage type, float64 reference).  qlog: q is Q' = round_T(Q dh^-0.5 log2 e), the reference is built
    from that same Q' (the transformer blocks' call, as in test_attention_shift_path)."""
    q, k, v = A.standard_inputs(N, HEADS, dh, tq, tk, dtype)
    if kind != "standard":
        q, k = (t.to(dtype) for t in A.extremes(kind, q, k))
    if qlog:
        q = A.log2_scaled(q, dh, dtype)
    return q, k, v, A.reference(q, k, v, HEADS, dh ** -0.5, q_log2_scaled=bool(qlog))


@functools.lru_cache(maxsize=64)
def cpu_restated(dh, tq, tk, dtype, qlog, kind, scales_q, ones, rows_shift):
    q, k, v, _ = cpu_inputs(dh, tq, tk, dtype, qlog, kind)
    return A.restated(q, k, v, HEADS, dh ** -0.5, bool(qlog), dtype, scales_q, ones, rows_shift)


class Checker:
    """Collects the figures of every case and fails at the end with every miss."""

    def __init__(self):
        self.bad = []

    def check(self, name, got, ref, restated, tol):
        got = got.detach().float().cpu()
        if not bool(torch.isfinite(got).all()):
            self.bad.append(f"{name}: {int((~torch.isfinite(got)).sum())} non-finite outputs")
            got = torch.nan_to_num(got, nan=0.0, posinf=0.0, neginf=0.0)
        e = A.rel_l2(got, ref)
        rk, rr = A.head_row_measure(got, ref, HEADS), A.head_row_measure(restated, ref, HEADS)
        record(name + ".rel", e, tol)
        record(name + ".rel.restated", A.rel_l2(restated, ref))
        record(name + ".row.restated", rr)
        record(name + ".row.kernel", rk, 2 * rr)
        ratio = rk / rr if rr > 0 else (0.0 if rk == 0 else float("inf"))
        print(f"{name}: rel {e:.3e} (< {tol:.1e})  row kernel {rk:.3e} restated {rr:.3e} ratio {ratio:.2f}", flush=True)
        if not e < tol:
            self.bad.append(f"{name}: rel-L2 {e:.3e} >= {tol:.1e}")
        if not rk <= 2 * rr:
            self.bad.append(f"{name}: head-row measure {rk:.3e} > 2 x restated {rr:.3e}")

    def equal(self, name, a, b):
        if not torch.equal(a.view(torch.int16), b.view(torch.int16)):
            self.bad.append(f"{name}: not bit-identical")

    def true(self, name, cond):
        if not cond:
            self.bad.append(name)

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def run(ck, ops, name, od, dh, dtype, qlog, kind, route, launch=None, nw=4):
    """Two launches of one case on the operands `od`, criteria 1 - 4 and the inputs unchanged.  nw: waves per block of the
    launch (4 at these sizes unless MOBI_ATTN_NW says 8)."""
    q, k, v, ref = cpu_inputs(dh, od.q.shape[1], od.k.shape[1], dtype, qlog, kind)
    rest = cpu_restated(dh, od.q.shape[1], od.k.shape[1], dtype, qlog, kind, *A.restated_args(route, nw))
    launch = launch or (lambda: ops.attention(od.qd, od.kd, od.vd, HEADS, dh ** -0.5, v_rows=od.v_rows, q_log2_scaled=bool(qlog)))
    y1, y2 = launch(), launch()
    torch.cuda.synchronize()
    tol = TOL[dtype] * (1.5 if route["scales_q"] and not qlog else 1.0)
    ck.check(name, y1, ref, rest, tol)
    ck.equal(name + ": second call", y1, y2)
    ck.true(name + ": an input changed", od.unchanged())
    return y1


def operands(dh, tq, tk, dtype, qlog, kind, form, v_form):
    q, k, v, _ = cpu_inputs(dh, tq, tk, dtype, qlog, kind)
    return A.build_operands(q, k, v, form, v_form)


def env_variants(dh, v_rows, h16=True):
    """(label, environment, route) of the launches a V-rows case at dh <= 80 additionally runs."""
    out = []
    if v_rows and dh <= 80:
        for nw in ("4", "8"):
            out.append((f"nw{nw}", {"MOBI_ATTN_NW": nw}, A.route(dh, True)))
            out.append((f"v3off.nw{nw}", {"MOBI_ATTN_NW": nw, "MOBI_ATTN_V3": "0"}, A.route(dh, True, v3=False)))
        if dh == 40 and h16:
            for nw in (None, "4", "8"):
                env = {"MOBI_ATTN_H16": "1", **({"MOBI_ATTN_NW": nw} if nw else {})}
                out.append((f"h16.nw{nw or 'default'}", env, dict(A.route(dh, True), body="rows<3,QSH,H16>")))
    return out


class Env:
    def __init__(self, tune, env):
        self.tune, self.env = tune, env

    def __enter__(self):
        for key, value in self.env.items():
            self.tune.setenv(key, value)

    def __exit__(self, *exc):
        for key in self.env:
            self.tune.delenv(key)


# ----------------------------------------------------------------------------------------------------------------------
# a. every accepted head dim
@pytest.mark.parametrize("dtype", DT, ids=tag)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dh", ALL_DH)
def test_every_head_dim(ops, tune, dh, layout, dtype):
    """n = 2, heads = 3, tq = 161 (two 128-query blocks with a one-row last wave, or one ragged 256-query block), tk = 197 / 200
    (four key tiles: the two-image LDS ring wraps; a last tile of 5 / 8 keys); q as it is and as Q' (q_log2_scaled) on the
    standard inputs, and q as it is on the 'negative' ones, where a key past the end would weigh (test_tile_edges)."""
    ck = Checker()
    v_form, tk = LAYOUTS[layout]
    tq, v_rows = 161, v_form == "rows"
    q, k, _, _ = cpu_inputs(dh, tq, tk, dtype, 0, "standard")
    eff = float(A.effective_keys(q, k, HEADS, dh ** -0.5).median())
    record(f"dh{dh}.{layout}.{tag(dtype)}.effective_keys", eff)
    ck.true(f"dh {dh}: median effective keys {eff:.1f} < 8", eff >= 8.0)
    for kind, qlog in (("standard", 0), ("standard", 1), ("negative", 0)):
        od = operands(dh, tq, tk, dtype, qlog, kind, "dense", v_form)
        r = A.route(dh, v_rows)
        case = f"{layout}.{tag(dtype)}.dh{dh}.log2q{qlog}" + ("" if kind == "standard" else "." + kind)
        run(ck, ops, f"{r['body']}.{case}", od, dh, dtype, qlog, kind, r)
        for label, env, r in env_variants(dh, v_rows):
            with Env(tune, env):
                run(ck, ops, f"{r['body']}.{case}.{label}", od, dh, dtype, qlog, kind, r, nw=int(env.get("MOBI_ATTN_NW", 4)))
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
# b. tile edges
TQ_SWEEP = [(tq, 65) for tq in (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)]
TK_SWEEP = [(33, tk) for tk in (1, 2, 8, 63, 64, 65, 127, 128, 129, 136, 192)]


@pytest.mark.parametrize("dtype", DT, ids=tag)
@pytest.mark.parametrize("layout", ["v_rows", "vt"])
@pytest.mark.parametrize("dh", [40, 72, 96, 112, 160])
def test_tile_edges(ops, tune, dh, layout, dtype):
    """One head dim per body -- 40 (rows, QSH, odd KS), 72 (rows, QSH, KS = 5), 96 (KS = 6), 112 (seven k-steps in the KS = 8
    body), 160 (KS = 10) -- over the query counts around a wave, a 128- and a 256-query block and the key counts around a
    32-key half, a 64-key tile and the LDS ring's wrap.  V^T rows are 16-byte aligned where tk % 8 == 0 and ragged elsewhere.
    Each shape runs on the standard inputs and on the 'negative' ones (every score far below zero): only there does a key
    past the end, whose score is 0, weigh anything in a denominator (tests/test_attention_ref_cpu.py)."""
    ck = Checker()
    v_rows = layout == "v_rows"
    for tq, tk in TQ_SWEEP + TK_SWEEP:
        form = layout if v_rows else ("vt_aligned" if tk % 8 == 0 else "vt_ragged")
        for kind in ("standard", "negative"):
            od = operands(dh, tq, tk, dtype, 0, kind, "dense", "rows" if v_rows else "vt")
            r = A.route(dh, v_rows)
            name = f"{r['body']}.{form}.{tag(dtype)}.dh{dh}.tq{tq}.tk{tk}.{kind}"
            run(ck, ops, name, od, dh, dtype, 0, kind, r)
            for label, env, r in env_variants(dh, v_rows, h16=False):
                if label.startswith("nw"):
                    with Env(tune, env):
                        run(ck, ops, f"{name}.{label}", od, dh, dtype, 0, kind, r, nw=int(env["MOBI_ATTN_NW"]))
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
# c. strides and guards, through the C ABI
PATTERN = 0x3C5A                        # a finite value in both storage types (fp16 1.088, bf16 0.0133)


def abi_params(od, out, dh, dtype, qlog, ops):
    """mobi_attention_params as ops.attention fills it, the output being any [n, tq, C] view."""
    from mobi_amd import _lib
    p = _lib.AttentionParams()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    p.q, p.q_img_stride, p.q_row_stride = ptr(od.qd), od.qd.stride(0), od.qd.stride(1)
    p.k, p.k_img_stride, p.k_row_stride = ptr(od.kd), od.kd.stride(0), od.kd.stride(1)
    p.vt, p.vt_img_stride, p.vt_row_stride = ptr(od.vd), od.vd.stride(0), od.vd.stride(1)
    p.out, p.out_img_stride, p.out_row_stride = ptr(out), out.stride(0), out.stride(1)
    p.v_layout, p.q_log2_scaled = (1 if od.v_rows else 0), qlog
    p.images, p.heads, p.dh, p.tq, p.tk = od.qd.shape[0], HEADS, dh, od.qd.shape[1], od.kd.shape[1]
    p.scale, p.dtype = dh ** -0.5, ops._dt(dtype)
    return p


def call(ops, p):
    from mobi_amd import _lib
    return _lib.load().mobi_attention(C.byref(p), ops._stream())


def strided_output(n, tq, c, row_stride, dtype):
    """(buffer, [n, tq, C] view at element 64 with the given row stride and two spare rows per image, mask of the view)."""
    img = (tq + 2) * row_stride
    buf = torch.full((64 + n * img + 64,), PATTERN, dtype=torch.int16, device="cuda").view(dtype)
    view = buf.as_strided((n, tq, c), (img, row_stride, 1), 64)
    mask = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
    mask.as_strided((n, tq, c), (img, row_stride, 1), 64).fill_(True)
    return buf, view, mask


@pytest.mark.parametrize("dtype", DT, ids=tag)
@pytest.mark.parametrize("dh", [40, 96, 160])
def test_strides_and_guards(ops, dh, dtype):
    """q | k | v as thirds of one [n, T, 3 C + 8] buffer and the partner form (image stride of two images), V as rows, as V^T
    with padded 16-byte rows and as V^T with rows of tk + 3; the output a view into a larger pre-filled buffer with row
    strides C + 4 and C + 8 and an image stride above tq rows.  Every element around the operands is NaN and lies in memory
    this test owns: a NaN in the output is a read outside the operands.  Outside the view the output buffer keeps its
    pattern; the inputs keep their bits."""
    ck = Checker()
    tq, c = 129, HEADS * dh
    for form in ("stacked", "partner"):
        for v_form in ("rows", "vt_aligned", "vt_ragged"):
            for tk in (130, 136):
                od = operands(dh, tq, tk, dtype, 0, "standard", form, v_form)
                r = A.route(dh, od.v_rows)
                path = "v_rows" if od.v_rows else v_form if tk % 8 == 0 else "vt_ragged"      # tk = 130: element loads
                for row_stride in (c + 4, c + 8):
                    buf, view, mask = strided_output(N, tq, c, row_stride, dtype)
                    p = abi_params(od, view, dh, dtype, 0, ops)
                    name = f"{r['body']}.{path}.{tag(dtype)}.dh{dh}.{form}.{v_form}.tk{tk}.out{row_stride - c}"

                    def launch():
                        rc = call(ops, p)
                        ck.true(f"{name}: mobi_attention returned {rc}", rc == OK)
                        return view.clone()

                    run(ck, ops, name, od, dh, dtype, 0, "standard", r, launch)
                    outside = buf.view(torch.int16)[~mask]
                    ck.true(f"{name}: {int((outside != PATTERN).sum())} elements outside the output view were written",
                            bool((outside == PATTERN).all()))
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
# d. score extremes on the exact online-softmax path
EXTREME_CASES = [("v_rows", 96, {}), ("v_rows", 160, {}), ("vt_aligned", 40, {}), ("vt_aligned", 80, {}),
                 ("v_rows", 40, {"MOBI_ATTN_V3": "0"}), ("v_rows", 40, {"MOBI_ATTN_V3": "0", "MOBI_ATTN_NW": "8"})]


@pytest.mark.parametrize("dtype", DT, ids=tag)
@pytest.mark.parametrize("layout,dh,env", EXTREME_CASES,
                         ids=[f"{c[0]}-{c[1]}" + "".join(f"-{k[10:].lower()}{v}" for k, v in c[2].items()) for c in EXTREME_CASES])
def test_score_extremes_on_the_exact_path(ops, tune, layout, dh, env, dtype):
    """The ramp / huge / negative / spike inputs of test_attention_shift_path through attention_kernel: V rows at dh 96 and
    160, V^T at dh 40 and 80, V rows at dh 40 with MOBI_ATTN_V3=0 (four- and eight-wave blocks); tq = 64, tk = 200."""
    ck = Checker()
    v_rows = layout == "v_rows"
    r = A.route(dh, v_rows, v3="MOBI_ATTN_V3" not in env)
    assert r["kernel"] == "attention_kernel"
    with Env(tune, env):
        for kind in ("ramp", "huge", "negative", "spike"):
            od = operands(dh, 64, 200, dtype, 0, kind, "dense", "rows" if v_rows else "vt")
            label = ".".join(f"{k[10:].lower()}{v}" for k, v in env.items())
            run(ck, ops, f"{r['body']}.{layout}.{tag(dtype)}.dh{dh}.{kind}{'.' + label if label else ''}", od, dh, dtype, 0, kind, r)
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
def test_cpu_self_test_judges_with_the_same_bound():
    from tests.test_attention_ref_cpu import TOL as cpu_tol
    assert cpu_tol == TOL


# e. refusals: nothing is launched
def test_refusals(ops):
    dtype, tq, tk = torch.float16, 16, 16
    buf = torch.zeros(1 << 16, dtype=dtype, device="cuda")

    def params(dh=40, v_rows=True, **over):
        c = HEADS * dh
        q = buf.as_strided((N, tq, c), (tq * c, c, 1), 0)
        out = buf.as_strided((N, tq, c), (tq * c, c, 1), 1 << 15)
        vd = q if v_rows else buf.as_strided((N, c, tk), (c * tk, tk, 1), 0)
        od = A.Operands(q, q, q, q, q, vd, v_rows, [])
        p = abi_params(od, out, dh, dtype, 0, ops)
        for key, value in over.items():
            setattr(p, key, value)
        return p

    before = buf.clone()
    for dh in (4, 12, 164, 168):
        assert call(ops, params(dh=dh)) == ERR_UNSUPPORTED, dh
    c = HEADS * 40
    for field in ("q_row_stride", "k_row_stride", "q_img_stride", "k_img_stride"):
        for off in (1, 4, 7):
            assert call(ops, params(**{field: (c if "row" in field else tq * c) + off})) == ERR_ALIGN, (field, off)
    for field in ("out_row_stride", "out_img_stride"):
        for off in (1, 2, 3):
            assert call(ops, params(**{field: (c if "row" in field else tq * c) + off})) == ERR_ALIGN, (field, off)
    assert call(ops, params(q=C.c_void_p(buf.data_ptr() + 8))) == ERR_ALIGN
    assert call(ops, params(v_layout=2)) == ERR_ARG
    # a V row stride off 8 elements is refused for V rows ...
    assert call(ops, params(vt_row_stride=c + 3)) == ERR_ALIGN
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    # ... and is the ragged-row form of V^T (launched and checked in test_strides_and_guards): accepted
    vt = torch.zeros((N, c, tk + 3), dtype=dtype, device="cuda")
    p = params(v_rows=False)
    p.vt, p.vt_img_stride, p.vt_row_stride = C.c_void_p(vt.data_ptr()), c * (tk + 3), tk + 3
    assert call(ops, p) == OK
    torch.cuda.synchronize()
