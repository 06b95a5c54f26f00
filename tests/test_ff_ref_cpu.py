"""tests/ff_ref.py on the CPU: the float64 reference against launch_shadow.ff_geglu_reference and against torch's own
F.linear / F.gelu / F.layer_norm, the restatement against criteria 2 and 3 of tests/test_gpu_ff_rows.py on every case of
tests/ff_cases.py (a condition on the inputs), other summation orders accepted, planted faults rejected, and the whole-tensor
figure shown to accept one wrong row among 4113.  Nothing is launched."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import ff_cases as FC
from tests import ff_ref as R
from tests.ff_ref import Case

DT = [torch.float16, torch.bfloat16]
# every launch of the GPU file, and hidden = 1280 (the product's size: one chunk is 1 / 40 of the second sum)
ALL = [c for _, c in FC.CASES] + [Case(FC.ROWS, 1280)]
ALL = list(dict.fromkeys(ALL))


@functools.lru_cache(maxsize=None)
def sides(case, dtype):
    o = R.host_operands(case, dtype)
    return o, R.reference(case, o), R.restated(case, o, dtype)


def rejected(dtype, got, ref, rest):
    """The criteria (2: rel-L2 below TOL; 3: row and channel measure within 2 x the restatement's) that reject `got`."""
    return set(R.judge(dtype, got, ref, rest)[1])


# ----------------------------------------------------------------------------------------------------------------------
# the reference is the contract
@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
@pytest.mark.parametrize("case", [Case(33, 96), Case(33, 64, residual="", b2=False), Case(35, 96, residual="x", ln="standard"),
                                  Case(35, 64, ln="off16")], ids=lambda c: c.form + "." + c.name)
def test_reference_equals_the_shadow_and_torch(case, dtype):
    from tests.launch_shadow import ff_geglu_reference
    o = R.host_operands(case, dtype)
    ref = R.reference(case, o)
    ln = (o["gamma"], o["beta"], R.LN_EPS) if case.ln else None
    shadow = ff_geglu_reference(dict(x=o["x"][None], residual=None if o["res"] is None else o["res"][None], b2=o["b2"], ln=ln,
                                     dec=o["dec"]))
    assert R.rel_l2(shadow.reshape(ref.shape), ref) < 1e-12
    w1, b1, w2 = (t.double() for t in o["dec"])
    x = o["x"].double()
    if case.ln:
        x = F.layer_norm(x, (case.c,), o["gamma"].double(), o["beta"].double(), R.LN_EPS)
    val, gate = F.linear(x, w1, b1).chunk(2, dim=-1)
    want = F.linear(val * F.gelu(gate), w2, None if o["b2"] is None else o["b2"].double())
    if o["res"] is not None:
        want = want + o["res"].double()
    assert R.rel_l2(want, ref) < 1e-12


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_decode_reads_back_what_was_packed(dtype):
    """The reference multiplies the decode of the packed buffer: it must be the rounded masters (b1 x B1_SCALE)."""
    w1, b1, w2, b2 = R._masters(96, R.C)
    _, (d1, db1, d2), pb2 = R.packed(96, dtype)
    assert torch.equal(d1, w1.to(dtype)) and torch.equal(d2, w2.to(dtype))
    assert torch.equal(db1, b1 * R.B1_SCALE) and torch.equal(pb2, b2)


def test_packed_bytes_is_61_kib_per_chunk():
    """A query, no launch: 40 W1 fragments + 20 W2 fragments + the b1 piece per chunk of 32 hidden units."""
    from mobi_amd import _lib
    lib = _lib.load()
    for h in (32, 96, 1280):
        assert lib.mobi_ff_geglu_packed_bytes(320, h) == (h // 32) * 61 * 1024 == R.packed(h, torch.float16)[0].numel()
    for c, h in ((0, 96), (-32, 96), (48, 96), (320, 0), (320, -32), (320, 48)):
        assert lib.mobi_ff_geglu_packed_bytes(c, h) == 0, (c, h)


def test_case_list_is_what_the_suite_promises():
    names = [FC.case_id(g, c, "fp16") for g, c in FC.CASES]
    assert len(set(names)) == len(names)
    chunk_counts = {c.chunks for g, c in FC.CASES if g == "chunks"}
    assert chunk_counts == {1, 2, 3, 4, 5, 6, 7, 8, 13, 40}
    for hidden in (96, 128):
        assert {c.rows for g, c in FC.CASES if g == "rows" and c.hidden == hidden} == {1, 31, 32, 33, 96, 127, 128, 129, 257}
    assert {(c.residual, c.b2) for g, c in FC.CASES if g == "forms" and not c.ln} == \
        {(r, b) for r in ("", "separate", "inplace") for b in (True, False)}
    assert any(c.ln and c.residual == "x" for g, c in FC.CASES if g == "forms")
    assert {c.ln for g, c in FC.CASES if g == "ln"} == set(R.LN_REGIMES)
    assert all(c.rows * c.c <= 257 * 320 and c.c == 320 for _, c in FC.CASES)


# ----------------------------------------------------------------------------------------------------------------------
# a condition on the inputs, not a measurement: the restatement itself meets criteria 2 and 3 with room to spare
@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_restatement_meets_the_criteria_on_every_case(dtype):
    bad = []
    for case in ALL:
        o, ref, rest = sides(case, dtype)
        fig, fails = R.judge(dtype, rest, ref, rest)
        if fails:
            bad.append(f"{case}: {fails}")
        _, gate = R.pre_activations(case, o)
        share = float((gate.abs() < 3).double().mean())
        if not share >= 0.5:
            bad.append(f"{case}: only {share:.2f} of the gate pre-activations inside |g| < 3")
        if o["res"] is not None and case.residual != "x":                   # the residual has to matter to be checked
            d = R.rel_l2(R.reference(case, dict(o, res=None)), ref)
            if not d > 10 * R.tolerance(dtype):
                bad.append(f"{case}: the residual moves the output by {d:.3e} only")
    assert not bad, "\n".join(bad)


def test_standard_inputs_measure_what_the_suite_was_planned_on():
    """rows = 161, hidden 32 / 96 / 256 / 1280: restated rel-L2 about 2.9e-4 (fp16) and 2.3e-3 (bf16) against TOL 5e-4 and
    4e-3 -- a correct kernel has room -- and the gate pre-activations have std about 2."""
    for dtype, lo, hi in ((torch.float16, 2.5e-4, 3.3e-4), (torch.bfloat16, 2.0e-3, 2.6e-3)):
        for hidden in (32, 96, 256, 1280):
            case = Case(FC.ROWS, hidden)
            o, ref, rest = sides(case, dtype)
            assert lo < R.rel_l2(rest, ref) < hi, (dtype, hidden)
            assert 1.8 < float(R.pre_activations(case, o)[1].std()) < 2.3


# ----------------------------------------------------------------------------------------------------------------------
# accepted: another summation order
@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
@pytest.mark.parametrize("order", ["reversed", "f64"])
def test_another_summation_order_is_accepted(order, dtype):
    bad = []
    for case in ALL:
        o, ref, rest = sides(case, dtype)
        fails = rejected(dtype, R.restated(case, o, dtype, order=order), ref, rest)
        if fails:
            bad.append(f"{case} {order}: {fails}")
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------------
# rejected: planted faults
def mutants(case):
    """name -> fault (ff_ref.restated) for every mutant that applies to `case`."""
    n, rows, c = case.chunks, case.rows, case.c
    mid, last = n // 2, n - 1
    tile = 128 if rows > 128 else 0                                      # the first wave tile of the last block
    r = torch.arange(rows)
    m = {
        "one chunk missing in one 32-row tile": dict(chunk_missing_in_tile={mid: tile}),
        "value and gate rows of one chunk exchanged": dict(swap_value_gate=(mid,)),
        "GELU skipped for one chunk": dict(no_gelu=(mid,)),
    }
    if n >= 2:
        m["chunk c formed with b1 of chunk c - 1"] = dict(b1_chunk={last: last - 1})
        m["chunk 1 formed with b1 of chunk 0"] = dict(b1_chunk={1: 0})
    if n % 2:
        m["odd count: last chunk dropped"] = dict(chunk_weight={last: 0.0})
        m["odd count: last chunk added twice"] = dict(chunk_weight={last: 2.0})
    if case.b2:
        m["b2 missing on channels 160 - 319"] = dict(b2_mask=torch.cat([torch.ones(160), torch.zeros(160)]))
    if case.residual and rows > 32:
        t0 = 32 * ((rows - 1) // 32)
        m["residual of row r + 32 in the last tile"] = dict(residual_rows=torch.where(r >= t0, (r + 32) % rows, r))
    if rows >= 64:
        perm = r.clone()
        perm[:32], perm[32:64] = r[32:64], r[:32]
        m["rows r and r + 32 exchanged in one block"] = dict(row_perm=perm)
    if case.ln:
        ch = torch.arange(c)
        m["gamma / beta of channels 8 - 15 of every 16 from channels 0 - 7"] = dict(gamma_index=torch.where(ch % 16 >= 8, ch - 8, ch))
    if case.ln in ("off128", "mixed"):
        m["LayerNorm variance as E[x^2] - mean^2"] = dict(ln_one_pass=True)
    if case.ln in ("const", "mixed"):
        m["LayerNorm without eps"] = dict(ln_no_eps=True)
    return m


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_every_mutant_is_rejected(dtype):
    """Each planted fault, on every case it applies to, fails criterion 2 or 3 (a NaN fails criterion 1 first)."""
    bad, seen = [], set()
    for case in ALL:
        o, ref, rest = sides(case, dtype)
        for name, fault in mutants(case).items():
            if name == "LayerNorm variance as E[x^2] - mean^2" and dtype == torch.bfloat16:
                continue                        # see test_one_pass_variance_is_below_the_resolution_of_bf16
            seen.add(name)
            got = R.restated(case, o, dtype, fault=fault)
            if not rejected(dtype, got, ref, rest):
                fig = R.judge(dtype, got, ref, rest)[0]
                bad.append(f"{case}: '{name}' passes: " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert len(seen) >= 13 - (dtype == torch.bfloat16), seen
    assert not bad, "\n".join(bad)


def test_one_pass_variance_is_below_the_resolution_of_bf16():
    """Why the E[x^2] - mean^2 mutant has no bf16 case.  At offset 128, the largest of tests/test_gpu_norm_stats.py, the fp32
    one-pass variance is off by a few 128^2 2^-24 ~ 1e-3 of a variance of 1 and rstd by 2.4e-3 in the worst row: below 2^-8, the
    unit roundoff with which LayerNorm's result is rounded to bf16 right afterwards, above fp16's 2^-11.  No criterion on a
    bf16 output can tell the two apart (measured: row measure 1.36 x the restatement's, rel-L2 3.5e-3 against 4e-3); fp16
    rejects the mutant on the off128 and the mixed rows (10 x and 6 x)."""
    case = Case(FC.ROWS, 96, ln="off128")
    for dtype, visible in ((torch.float16, True), (torch.bfloat16, False)):
        o, ref, rest = sides(case, dtype)
        x = o["x"].float()
        mean = x.sum(1) * torch.tensor(1.0 / case.c)
        one_pass = (x * x).sum(1) * torch.tensor(1.0 / case.c) - mean * mean
        exact = o["x"].double().var(1, unbiased=False)
        rstd_err = float(((one_pass.double() + R.LN_EPS).rsqrt() / (exact + R.LN_EPS).rsqrt() - 1).abs().max())
        assert 2.0 ** -11 < rstd_err < 2.0 ** -8, rstd_err
        fails = rejected(dtype, R.restated(case, o, dtype, fault=dict(ln_one_pass=True)), ref, rest)
        assert bool(fails) == visible, (dtype, fails)


def test_b1_scale_rejects_the_swap_with_room():
    """B1_SCALE: test_ff_geglu_fused's b1 needs no scaling up.  'chunk c formed with b1 of chunk c - 1' is rejected on every
    case in both storage types, and the narrowest case (bf16, hidden = 1280) exceeds the restatement's measure by more than
    twice the margin."""
    narrowest = float("inf")
    for dtype in DT:
        for case in ALL:
            if case.chunks < 2:
                continue
            o, ref, rest = sides(case, dtype)
            for fault in (dict(b1_chunk={case.chunks - 1: case.chunks - 2}), dict(b1_chunk={1: 0})):
                fig = R.judge(dtype, R.restated(case, o, dtype, fault=fault), ref, rest)[0]
                narrowest = min(narrowest, max(fig["row"] / fig["row.restated"], fig["channel"] / fig["channel.restated"]))
    assert narrowest > 2 * R.MARGIN, narrowest


# ----------------------------------------------------------------------------------------------------------------------
# the gap: a whole-tensor figure accepts one wrong row
ONE_ROW_MUTANTS = {
    torch.float16: ("chunk c formed with b1 of chunk c - 1", "chunk 1 formed with b1 of chunk 0", "b2 missing on channels 160 - 319"),
    torch.bfloat16: ("value and gate rows of one chunk exchanged", "GELU skipped for one chunk",
                     "chunk c formed with b1 of chunk c - 1", "chunk 1 formed with b1 of chunk 0"),
}


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_whole_tensor_check_accepts_one_wrong_row(dtype):
    """rows = 4113 (test_ff_geglu_fused's ragged size), hidden = 1280: the last row alone carries a mutant's result.  The
    whole-tensor rel-L2 stays below TOL -- test_ff_geglu_fused's criterion accepts it -- while the row measure rejects it.
    One wrong row among 4113 weighs 1 / 64 of its own relative error: in bf16 (TOL 4e-3) a row with a whole chunk's gate
    wrong passes (rel-L2 3.5e-3 - 3.7e-3 beside the restatement's 2.3e-3, row measure 50 x); in fp16 (TOL 5e-4) a row with
    another chunk's b1 or half of b2 missing does (3.1e-4 - 3.2e-4 beside 2.9e-4, row measure 15 - 20 x).  Grosser one-row
    faults (a chunk or the residual missing: 4e-3 - 5e-3) the whole-tensor figure does see at this row count."""
    rows, hidden = 4113, 1280
    case = Case(rows, hidden)
    o, ref, rest = sides(case, dtype)
    tail = Case(32, hidden)                                               # rows are independent: mutate the last 32 only
    ot = dict(o, x=o["x"][-32:], res=o["res"][-32:])
    assert torch.equal(R.restated(tail, ot, dtype), rest[-32:])
    for name in ONE_ROW_MUTANTS[dtype]:
        got = rest.clone()
        got[-1] = R.restated(tail, ot, dtype, fault=mutants(tail)[name])[-1]
        fig, fails = R.judge(dtype, got, ref, rest)
        assert fig["rel"] < R.tolerance(dtype), (name, fig)              # accepted by the whole-tensor figure
        assert "rel" not in fails and "row" in fails, (name, fig, fails)  # rejected per row
