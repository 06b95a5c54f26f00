"""GPU: the attention probe -- `mobi_attention_health` against the fp64 definition (`health.attention_health_ref`), planted late
rises and bad operands, determinism and company, that it writes nothing but its records, and `health.probe(attention=True)` on
the reduced UNet: the rows it must not change, the two kernels' agreement on inf + nan, and the production kernel's error on
Gaussian and heavy-tailed weights.  `out` is always what `ops.attention` returned for the same operands."""
import numpy as np
import pytest
import torch

from tests import attention_health_cases as AC, attention_ref as AR
from tests.test_gpu_health import _forward, _setup

pytestmark = pytest.mark.gpu

EXACT = ("q_absmax_bits", "k_absmax_bits", "v_absmax_bits", "in_nonfinite", "out_nonfinite")
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def _run(od, heads, scale, log2, rise_limit=None, out=None, records=None):
    from mobi_amd import ops
    if out is None:
        out = ops.attention(od.qd, od.kd, od.vd, heads, scale, v_rows=od.v_rows, q_log2_scaled=bool(log2))
    rec = ops.attention_health(od.qd, od.kd, od.vd, out, heads, scale, v_rows=od.v_rows, q_log2_scaled=bool(log2),
                               rise_limit=rise_limit, records=records)
    return out, rec


def _ref(q, k, v, out, heads, scale, log2, rise_limit=None, rises=False):
    from mobi_amd import health
    return health.attention_health_ref(q, k, v, out.cpu(), heads, scale, True, bool(log2), rise_limit, rises=rises)


def _gap(rises, width):
    """The midpoint of the widest gap of the sorted rises, which must be wider than `width` and have rows on both sides."""
    s = np.sort(rises.reshape(-1))
    d = np.diff(s)
    i = int(np.argmax(d))
    assert d[i] > width, (d[i], width)
    return 0.5 * (s[i] + s[i + 1])


@pytest.mark.parametrize("case", AC.CASES, ids=AC.case_id)
def test_kernel_against_the_fp64_definition(case):
    """Bit patterns and counts exactly; e_max, e_min within the fp32 dot-product bound dh * 2^-24 * cexp * max_ij sum_c
    |q_ic k_jc| of the case, rise_max within twice that; rows_rise_over exactly, with rise_limit at the midpoint of a gap of
    the fp64 rises wider than twice the rise's bound (every row counts; where tk <= 32 every rise is 0 by definition and no
    gap can exist: there rise_max must be exactly 0, no row lies over a limit of 0 and every row over a limit of -1);
    ref_absmax and err_max within the measured tolerance of attention_health_cases.measured_tolerance (4 x the worst error of
    the kernel's algorithm restated in fp32 numpy: profiles/attention_health.txt holds both numbers)."""
    from mobi_amd import ops
    dtype, dh, tq, tk, form, v_form, log2 = case
    q, k, v, scale = AC.inputs(dtype, dh, tq, tk, log2)
    od = AR.build_operands(q, k, v, form, v_form)
    out, _ = _run(od, AC.HEADS, scale, log2)
    base, rises = _ref(q, k, v, out, AC.HEADS, scale, log2, rises=True)
    bound = dh * 2.0 ** -24 * base["dot_abs_max"]                     # per head
    if tk > 32:
        limit = _gap(rises, 2.0 * 2.0 * float(bound.max()))
        assert rises.min() < limit < rises.max()
    else:
        assert not rises.any()
        limit = 0.0
    _, rec = _run(od, AC.HEADS, scale, log2, rise_limit=limit, out=out)
    got = ops.read_attention_health(rec)
    want = _ref(q, k, v, out, AC.HEADS, scale, log2, rise_limit=limit)
    _, tol = AC.measured_tolerance()
    bits_f32 = lambda b: b.astype(np.uint32).view(np.float32).astype(np.float64)
    figures = dict(e_max=np.abs(got["e_max"] - want["e_max"]).max(), e_min=np.abs(got["e_min"] - want["e_min"]).max(),
                   rise=np.abs(got["rise_max"] - want["rise_max"]).max(), bound=float(bound.min()),
                   ref=np.abs(bits_f32(got["ref_absmax_bits"]) - want["ref_absmax"]).max(),
                   err=np.abs(got["err_max"] - want["err_max"]).max(), tol=tol, err_max=float(want["err_max"].max()))
    print(AC.case_id(case), " ".join(f"{n}={x:.3g}" for n, x in figures.items()))
    assert len(got) == AC.IMAGES * AC.HEADS
    for name in EXACT:
        assert np.array_equal(got[name], want[name]), name
    assert not got["in_nonfinite"].any() and not got["out_nonfinite"].any()
    assert (np.abs(got["e_max"] - want["e_max"]) <= bound).all() and (np.abs(got["e_min"] - want["e_min"]) <= bound).all()
    assert (np.abs(got["rise_max"] - want["rise_max"]) <= 2.0 * bound).all()
    assert (got["rise_max"] >= 0).all()
    assert np.array_equal(got["rows_rise_over"], want["rows_rise_over"])
    if tk > 32:
        assert 0 < want["rows_rise_over"].sum() < rises.size
    else:
        assert not got["rise_max"].any() and not got["rows_rise_over"].any()
        _, rec = _run(od, AC.HEADS, scale, log2, rise_limit=-1.0, out=out)
        assert (ops.read_attention_health(rec)["rows_rise_over"] == tq).all()
    assert (np.abs(bits_f32(got["ref_absmax_bits"]) - want["ref_absmax"]) <= tol).all()
    assert (np.abs(got["err_max"] - want["err_max"]) <= tol).all()
    # err_row: the row the kernel names attains the fp64 maximum within the tolerance
    o64 = AC.exact64(q, k, v, AC.HEADS, scale, log2)
    oh = AR._heads(out.cpu().double(), AC.HEADS).numpy()
    for i in range(AC.IMAGES):
        for h in range(AC.HEADS):
            g = got[i * AC.HEADS + h]
            assert 0 <= g["err_row"] < tq
            assert np.abs(oh[i, h, g["err_row"]] - o64[i, h, g["err_row"]]).max() >= want["err_max"][i * AC.HEADS + h] - tol
    assert od.unchanged()


def _planted(dtype, dh=40, tq=70, tk=96, late=50, amount=12.0):
    """2 images x 2 heads whose keys are all equal inside a head (every score of a row is the same number: rise 0, uniform p),
    with one key at index `late` >= 32 of (image 1, head 0) replaced by 1.5 x the common key: that head's scores at the late
    key exceed the rest by 0.5 x the common score, which the fixed q and k make exactly `amount` octaves."""
    c = 2 * dh
    q = torch.zeros(2, tq, c)
    k = torch.zeros(2, tk, c)
    q[..., 0::dh] = 2.0                        # q . k = 2 * kc on the first channel of each head, exact in both types
    k[..., 0::dh] = amount                     # common score 2 * amount as an exponent of two (q_log2_scaled)
    k[1, late, 0] = 1.5 * amount
    v = AR.standard_inputs(2, 2, dh, tq, tk, dtype)[2].float()
    return q.to(dtype), k.to(dtype), v.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_late_rise_and_bad_operands_on_the_device(dtype):
    """The planted cases of tests/test_attention_health_cpu.py through the kernel.  Heads that a plant does not touch keep
    their records bit for bit."""
    from mobi_amd import ops
    heads, dh, tq, tk, late, amount = 2, 40, 70, 96, 50, 12.0
    q, k, v = _planted(dtype, dh, tq, tk, late, amount)
    read = ops.read_attention_health

    def records(q, k, v, limit, out=None, v_form="rows"):
        od = AR.build_operands(q, k, v, "dense", v_form)
        out, rec = _run(od, heads, 1.0, 1, rise_limit=limit, out=out)
        return out, read(rec)

    out, got = records(q, k, v, amount - 0.5)
    assert got["rise_max"].tolist() == [0.0, 0.0, amount, 0.0]                  # exact: every product and sum is a small integer
    assert got["rows_rise_over"].tolist() == [0, 0, tq, 0]
    assert got["e_max"].tolist() == [2 * amount, 2 * amount, 3 * amount, 2 * amount] and (got["e_min"] == 2 * amount).all()
    _, over = records(q, k, v, amount + 0.5, out=out)
    assert over["rows_rise_over"].tolist() == [0, 0, 0, 0]
    # uniform p: o is the mean of v, to fp32 rounding of a sum of tk terms below 8 in magnitude
    mean = AR._heads(v.double(), heads).mean(2).abs().amax(-1).reshape(-1).numpy()
    ref = got["ref_absmax_bits"].view(np.float32)
    for i in (0, 1, 3):
        assert abs(ref[i] - mean[i]) <= tk * 2.0 ** -24 * 8.0
    # the same plant below 32 keys: no rise by definition
    ke = k[:, :32].clone()
    ke[:, 20] = k[:, late]
    _, early = records(q, ke, v[:, :32].clone(), 0.0)
    assert not early["rise_max"].any() and not early["rows_rise_over"].any() and early["e_max"][2] == 3 * amount
    # attention_ref.extremes: one late dominant key ("spike") and scores that keep rising ("ramp"), against the definition
    for kind in ("spike", "ramp"):
        qs, ks, vs = AR.standard_inputs(2, heads, dh, tq, tk, dtype)
        qe, ke = AR.extremes(kind, qs, ks)
        qe, ke = qe.to(dtype), ke.to(dtype)
        oe, ge = records(qe, ke, vs, None, v_form="vt")
        we = _ref(qe, ke, vs, oe, heads, 1.0, 1)
        bound = dh * 2.0 ** -24 * we["dot_abs_max"]
        for name in EXACT + ("rows_rise_over",):
            assert np.array_equal(ge[name], we[name]), (kind, name)
        assert (np.abs(ge["rise_max"] - we["rise_max"]) <= 2 * bound).all() and (ge["rise_max"] > 1.0).all(), kind
    # an inf in one head's k: that head's count moves, the other three records do not
    kb = k.clone()
    kb[0, 7, dh + 3] = float("inf")
    _, bad = records(q, kb, v, amount - 0.5, out=out)
    assert bad["in_nonfinite"].tolist() == [0, 1, 0, 0]
    for name in ("q_absmax_bits", "k_absmax_bits", "v_absmax_bits", "out_nonfinite"):
        assert np.array_equal(bad[name], got[name]), name
    for i in (0, 2, 3):
        assert bad[i].tobytes() == got[i].tobytes()
    # a nan in out: counted, and err_max is over the finite elements only
    ob = out.clone()
    ob[1, 5, dh + 2] = float("nan")
    _, withnan = records(q, k, v, amount - 0.5, out=ob)
    assert withnan["out_nonfinite"].tolist() == [0, 0, 0, 1]
    want = _ref(q, k, v, ob, heads, 1.0, 1, amount - 0.5)
    assert want["out_nonfinite"].tolist() == [0, 0, 0, 1]
    assert np.isfinite(withnan["err_max"]).all() and abs(withnan["err_max"][3] - want["err_max"][3]) <= AC.measured_tolerance()[1]
    for i in (0, 1, 2):
        assert withnan[i].tobytes() == got[i].tobytes()
    # no finite element in a head's slice of out: err_row -1
    ob = out.clone()
    ob[0, :, :dh] = float("inf")
    _, allbad = records(q, k, v, amount - 0.5, out=ob)
    assert allbad["err_row"][0] == -1 and allbad["err_max"][0] == 0 and allbad["out_nonfinite"][0] == tq * dh
    assert allbad[1].tobytes() == got[1].tobytes()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_determinism_and_company(dtype):
    """Two launches give bit-equal records; a head probed alone (heads = 1 on the head's columns) gives the record it gets
    inside a batch of 2 x 8."""
    from mobi_amd import ops
    heads, dh, tq, tk = 8, 40, 130, 150
    q, k, v = AR.standard_inputs(2, heads, dh, tq, tk, dtype)
    q = AR.log2_scaled(q, dh, dtype)
    od = AR.build_operands(q, k, v, "dense", "rows")
    out, a = _run(od, heads, 1.0, 1)
    a = a.cpu()
    _, b = _run(od, heads, 1.0, 1, out=out)
    assert torch.equal(a, b.cpu())
    for img, h in ((0, 0), (1, 3), (1, 7)):
        cols = slice(h * dh, (h + 1) * dh)
        alone = ops.attention_health(od.qd[img:img + 1, :, cols], od.kd[img:img + 1, :, cols], od.vd[img:img + 1, :, cols],
                                     out[img:img + 1, :, cols], 1, 1.0, v_rows=True, q_log2_scaled=True)
        assert torch.equal(alone.cpu()[0], a[img * heads + h]), (img, h)


@pytest.mark.parametrize("v_form", ["rows", "vt_ragged"])
def test_writes_nothing_but_the_records(v_form):
    from mobi_amd import ops
    heads, dh, tq, tk = 2, 64, 65, 100
    q, k, v = AR.standard_inputs(2, heads, dh, tq, tk, torch.bfloat16)
    od = AR.build_operands(q, k, v, "stacked", v_form)
    out = ops.attention(od.qd, od.kd, od.vd, heads, dh ** -0.5, v_rows=od.v_rows)
    before = out.clone()
    count = 2 * heads
    buf = torch.full((count + 2, 12), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    _, rec = _run(od, heads, dh ** -0.5, 0, out=out, records=buf[1:])
    torch.cuda.synchronize()
    assert rec.data_ptr() == buf[1].data_ptr() and rec.shape == (count, 12)
    assert (buf[0] == 0x5a5a5a5a).all() and (buf[-1] == 0x5a5a5a5a).all()
    assert od.unchanged() and torch.equal(out.view(torch.int16), before.view(torch.int16))
    fresh = ops.attention_health(od.qd, od.kd, od.vd, out, heads, dh ** -0.5, v_rows=od.v_rows)
    assert torch.equal(fresh, rec)


# --------------------------------------------------------------------------------------
# the probe
# --------------------------------------------------------------------------------------
_RUNS = {}


def _probed(dtype):
    """The reduced UNet of tests/test_gpu_health.py, Gaussian weights, forward alone, under probe() and under
    probe(attention=True): computed once per storage type."""
    from mobi_amd import health
    if dtype not in _RUNS:
        model, net, i = _setup(dtype)
        plain_out = _forward(net, i)
        with health.probe() as hp:
            probe_out = _forward(net, i)
        with health.probe(attention=True) as ha:
            att_out = _forward(net, i)
        torch.cuda.synchronize()
        _RUNS[dtype] = dict(plain=plain_out, probe=probe_out, att=att_out, rep=hp.report(), rep_att=ha.report())
    return _RUNS[dtype]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_probe_integration(dtype):
    from mobi_amd import health, ops
    r = _probed(dtype)
    rep, ra = r["rep"], r["rep_att"]
    assert ops._HEALTH is None
    assert torch.equal(r["plain"], r["probe"]) and torch.equal(r["plain"], r["att"])
    assert rep.attention == [] and ra.rows == rep.rows and len(rep.rows) > 40      # Row compares field for field
    launches = [x for x in ra.rows if x.kind == "attention"]
    assert len(ra.attention) == len(launches) > 4
    assert [a.seq for a in ra.attention] == [x.seq for x in launches]
    for a, x in zip(ra.attention, launches):
        assert ra.attention_for(x.seq) is a and a.module == x.module and a.dtype == health.DTYPE_NAMES[dtype]
        assert a.out_nonfinite == x.inf + x.nan                       # two independent kernels agree
        assert a.in_nonfinite == 0
        assert x.shape == (a.images, a.tq, a.heads * a.dh) and len(a.per_head) == a.images * a.heads
        assert a.rise_limit == health.RISE_LIMIT[a.dtype]
    assert ra.attention_for(launches[0].seq + 1) is None or ra.rows[launches[0].seq + 1].kind == "attention"
    back = health.Report.from_json(ra.to_json())
    assert back.rows == ra.rows and back.attention == ra.attention
    assert all(np.array_equal(p.per_head, q.per_head) for p, q in zip(back.attention, ra.attention))
    text = str(ra)
    assert text.startswith(str(rep)) and "err_max" in text and "err_max" not in str(rep)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_production_error_on_gaussian_weights(dtype):
    """err_max <= 8 u v_absmax per launch with q_log2_scaled, u = 2^-11 (fp16) / 2^-8 (bf16): three roundings to the storage
    type (the probabilities, the denominator's share, the stored result) bound the error by 3 u v_absmax, fp16's flushed tail
    adds at most tk * 2^-25 * v_absmax, and 8 u leaves a factor of two."""
    ra = _probed(dtype)["rep_att"]
    scaled = [a for a in ra.attention if a.q_log2_scaled]
    assert len(scaled) > 4
    for a in scaled:
        print(f"#{a.seq} {a.module} {a.tq}x{a.tk} dh {a.dh}: err_max {a.err_max:.4g} = {a.err_max / (U[dtype] * a.v_absmax):.3g} u v_absmax, "
              f"rise_max {a.rise_max:.3g}, e_max {a.e_max:.3g}")
    for a in scaled:
        assert a.err_max <= 8 * U[dtype] * a.v_absmax, (a.seq, a.module, a.err_max, a.v_absmax)


def test_heavy_tailed_run():
    """health.heavy_tailed_ on the reduced UNet, bf16: whatever the first non-finite attention row is, its AttentionRow exists
    and agrees with it on out_nonfinite; at this size no attention row may be non-finite at all, and then that is asserted."""
    from mobi_amd import health
    model, net, i = _setup(torch.bfloat16)
    health.heavy_tailed_(net, 4)
    with health.probe(attention=True) as hp:
        _forward(net, i)
    torch.cuda.synchronize()
    rep = hp.report()
    launches = [x for x in rep.rows if x.kind == "attention"]
    assert len(rep.attention) == len(launches) > 4
    for x in launches:
        assert rep.attention_for(x.seq).out_nonfinite == x.inf + x.nan
    bad = next((x for x in launches if x.nonfinite), None)
    print(rep.summary())
    print(health.attention_section(rep))
    if bad is None:
        assert all(a.out_nonfinite == 0 for a in rep.attention)
    else:
        a = rep.attention_for(bad.seq)
        assert a is not None and a.out_nonfinite == bad.nonfinite > 0
