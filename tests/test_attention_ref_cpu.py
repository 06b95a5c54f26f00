"""tests/attention_ref.py on its own (no GPU): the criteria of tests/test_gpu_attention_forward.py have teeth.  The storage
restatement on the standard inputs (n = 2, heads = 3, tq = 161, tk = 197) passes every criterion; each planted fault -- the
local faults a forward attention kernel can have -- is rejected by the ROW criterion (worst (image, query, head) row at most
2 x the restatement's, criterion 3 of the GPU file).  Two of them are sized so that the whole-tensor figure stays under its
bound, which is why the row measure exists: a share of a neighbour's row leaking into one row, and a key past the end in the
denominators of the last wave.  (A whole row replaced moves the whole tensor by sqrt(2 / 966) = 4.5e-2 at this shape: every
measure sees that.)  The key past the end has score 0; on the standard inputs it weighs less than the output's rounding and no
measure can see it, so it is planted on the 'negative' inputs too, where it must be -- and is -- rejected."""
import pytest
import torch

from tests import attention_ref as A

DT = [torch.float16, torch.bfloat16]
# tests/test_gpu_ops.py TOL (not imported: that module is the GPU suite's); asserted equal on the GPU side
TOL = {torch.float16: 5e-4, torch.bfloat16: 4e-3}
N, HEADS, TQ, TK = 2, 3, 161, 197
LAST_WAVE = 160                      # 32-query waves: queries 160 .. 191 are the last wave, one of them real


def case(dh, dtype, v_rows=True, kind=None):
    q, k, v = A.standard_inputs(N, HEADS, dh, TQ, TK, dtype)
    if kind:
        q, k = (t.to(dtype) for t in A.extremes(kind, q, k))
    r = A.route(dh, v_rows)
    ref = A.reference(q, k, v, HEADS, dh ** -0.5)
    args = (HEADS, dh ** -0.5, False, dtype) + A.restated_args(r)
    return q, k, v, ref, args


def criteria(out, ref, base, dtype, tol_factor):
    """(finite, whole-tensor rel-L2 under the bound, row measure within 2 x the restatement's)"""
    rel, row = A.rel_l2(out, ref), A.head_row_measure(out, ref, HEADS)
    return bool(torch.isfinite(out).all()), rel < TOL[dtype] * tol_factor, row <= 2 * base, rel, row


def test_route_table():
    """launch_attention_v, restated: the kernel body, who rounds Q', and where the denominator comes from."""
    rows = {dh: A.route(dh, True) for dh in range(8, 168, 8)}
    assert [dh for dh, r in rows.items() if r["kernel"] == "attention_rows_kernel"] == list(range(8, 88, 8))
    assert [dh for dh, r in rows.items() if r["qsh"]] == [8, 24, 40, 56, 72]
    assert [dh for dh, r in rows.items() if not r["ones"]] == [32, 64, 96, 128, 160]
    assert [rows[dh]["ks"] for dh in (88, 96, 104, 112, 120, 128, 136, 144, 152, 160)] == [6, 6, 8, 8, 8, 8, 10, 10, 10, 10]
    for dh in range(8, 168, 8):
        for r in (A.route(dh, False), A.route(dh, True, v3=False)):
            assert r["kernel"] == "attention_kernel" and not r["scales_q"] and r["ones"] == (dh % 32 != 0)
    assert A.route(40, False)["ks"] == 3 and A.route(72, False)["ks"] == 5 and A.route(8, False)["ks"] == 1


def test_measures():
    ref = torch.arange(2 * 5 * 12, dtype=torch.float64).reshape(2, 5, 12) + 1.0
    got = ref.clone()
    assert A.head_row_measure(got, ref, 3) == 0.0
    got[1, 2, 4:8] += 0.5                                       # one (image, query, head) row: |d|_2 = 1
    rms = float(ref.reshape(-1, 4).pow(2).sum(1).mean().sqrt())
    assert A.head_row_measure(got, ref, 3) == pytest.approx(1.0 / rms, rel=1e-12)
    assert A.head_row_measure(got, ref, 1) < A.head_row_measure(got, ref, 3)        # whole-token rows dilute it
    q = torch.zeros(1, 2, 8)
    k = torch.randn(1, 7, 8, generator=torch.Generator().manual_seed(0))
    assert torch.allclose(A.effective_keys(q, k, 2, 1.0), torch.full((1, 2, 2), 7.0, dtype=torch.float64))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dh", [8, 56, 104, 160])
def test_standard_inputs_exercise_pv_and_restatement_is_accepted(dh, dtype):
    for v_rows in (True, False):
        q, k, v, ref, args = case(dh, dtype, v_rows)
        out = A.restated(q, k, v, *args)
        factor = 1.5 if A.route(dh, v_rows)["scales_q"] else 1.0
        ok = criteria(out, ref, A.head_row_measure(out, ref, HEADS), dtype, factor)
        print(f"dh {dh} {dtype} v_rows {v_rows}: rel {ok[3]:.3e} row {ok[4]:.3e}")
        assert ok[:3] == (True, True, True), ok
        assert ok[4] > 0.0                                      # a restatement without rounding error restates nothing
    eff = A.effective_keys(q, k, HEADS, dh ** -0.5)
    s = (A._heads(q.double(), HEADS) @ A._heads(k.double(), HEADS).transpose(-1, -2)) * dh ** -0.5
    print(f"dh {dh}: median effective keys {float(eff.median()):.1f}, |score| <= {float(s.abs().max()):.1f}")
    assert float(eff.median()) >= 8.0
    # q_log2_scaled from the same rounded Q' is the same function of its inputs
    qs = A.log2_scaled(q, dh, dtype)
    ref2 = A.reference(qs, k, v, HEADS, 123.0, q_log2_scaled=True)
    out2 = A.restated(qs, k, v, HEADS, 123.0, True, dtype, *args[4:])
    assert A.rel_l2(out2, ref2) < TOL[dtype] and A.rel_l2(ref2, ref) < 1.5 * TOL[dtype]       # the allowance for rounding Q'


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kind", [None, "ramp", "huge", "negative", "spike"])
@pytest.mark.parametrize("dh,nw", [(40, 4), (40, 8), (64, 4)])
def test_rows_kernel_shift_schedule(dh, nw, kind, dtype):
    """Softmax is shift-invariant: attention_rows_kernel's shift schedule only moves where P is rounded.  The restatement under
    it stays finite on every score extreme (fp16 overflows in the untested first attempt at QSH head dims and must repeat the
    block with the test, as the kernel does), differs from the true-maximum restatement by rounding only, and -- where every
    half is tested -- keeps each rounded probability below 2.0 with the final shift at most BIAS above the row maximum."""
    q, k, v, ref, args = case(dh, dtype, kind=kind)
    qsh = A.route(dh, True)["qsh"]
    shifted = A.restated(q, k, v, *args[:6], (qsh, nw))
    plain = A.restated(q, k, v, *args[:6], None)
    assert bool(torch.isfinite(shifted).all())
    assert A.rel_l2(shifted, plain) < TOL[dtype], A.rel_l2(shifted, plain)
    t = (A._heads(q.float(), HEADS) * torch.tensor(dh ** -0.5 * A.LOG2E)).to(dtype).float() @ A._heads(k.float(), HEADS).transpose(-1, -2)
    skey, s = A.rows_kernel_shifts(t, dtype, qsh, nw)
    bias = 8.0 if dtype == torch.bfloat16 else 4.0
    p = torch.exp2(t - skey).to(dtype).float()
    assert bool(torch.isfinite(p).all()) and float(p.max()) <= (2.0 if not qsh else float("inf"))
    assert bool((skey <= s.unsqueeze(-1)).all())                                   # the shift only rises
    if not qsh:                                                                     # tested from the first tile on: P stays below 2.0
        assert bool((t.amax(-1) - s < 1.0).all()) and bool((s - t.amax(-1) <= bias + 1e-3).all())


def planted(name, dh, dtype, kind=None):
    """(faulty output, float64 reference, untouched restatement) of dh / dtype on the standard inputs or an extreme of them."""
    q, k, v, ref, args = case(dh, dtype, kind=kind)
    out = A.restated(q, k, v, *args)
    c0 = dh                                                     # head 1
    if name == "row_from_neighbour":
        out[1, 77, c0:c0 + dh] = out[1, 78, c0:c0 + dh]
    elif name == "row_leak":
        # the same fault at the size the criteria are about: a share of the neighbour's row that moves this row by 4 x the
        # restatement's own worst row error (twice the criterion's margin) -- 1 row of 966, so the whole tensor moves by
        # 4 / sqrt(966) = 0.13 of that error
        d = (out[1, 78, c0:c0 + dh] - out[1, 77, c0:c0 + dh]).double()
        rms = float(A.head_rows(ref, HEADS).pow(2).sum(1).mean().sqrt())
        out[1, 77, c0:c0 + dh] += (d * (4 * A.head_row_measure(out, ref, HEADS) * rms / float(d.norm()))).float()
    elif name == "last_key_dropped":
        out = A.restated(q, k[:, :TK - 1], v[:, :TK - 1], *args)
    elif name == "key_past_the_end_in_last_wave":
        # a key >= tk reads as zeros: score 0, value 0 -- it adds exp2(0 - m) to the denominator and nothing to P.V
        num, den, m = A.restated_parts(q, k, v, *args)
        den = den.clone()
        den[:, :, LAST_WAVE:] += torch.exp2(-m[:, :, LAST_WAVE:])
        out = A._tokens((num / den.unsqueeze(-1)).to(dtype).float())
    elif name == "heads_swapped":
        out[0, :, dh:2 * dh], out[0, :, 2 * dh:3 * dh] = out[0, :, 2 * dh:3 * dh].clone(), out[0, :, dh:2 * dh].clone()
    elif name == "channel_group_zeroed":
        out[0, 160, c0 + 4:c0 + 8] = 0.0
    return out, ref, A.restated(q, k, v, *args)


FAULTS = ["row_from_neighbour", "row_leak", "last_key_dropped", "key_past_the_end_in_last_wave", "heads_swapped", "channel_group_zeroed"]
# A whole row replaced, or four channels zeroed, moves the whole-tensor figure by sqrt(2 / 966) = 4.5e-2 resp. sqrt(4 / (966 dh))
# >= 5e-3 at these shapes -- above any bound; the faults below are the ones small enough for the whole-tensor figure to miss.
LOCAL = ("row_leak", "key_past_the_end_in_last_wave")
# A key past the end has score 0.  On the standard inputs a row's best score is ~6 nats, so that key weighs exp(-6) / l < 1e-3 of
# the denominator: less than the storage rounding of the output, and NO measure against float64 can see it (asserted below, with
# the whole-tensor figure under its bound as for every local fault).  It is a fault of the size of the result where a row's
# scores lie below zero -- the 'negative' construction -- and there the row criterion has to reject it; the GPU file therefore
# runs its tile-edge sweeps on those inputs as well.
ON_NEGATIVE = ("key_past_the_end_in_last_wave",)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dh", [40, 104])
@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_rejected_by_the_row_criterion(fault, dh, dtype):
    out, ref, clean = planted(fault, dh, dtype)
    base = A.head_row_measure(clean, ref, HEADS)
    factor = 1.5 if A.route(dh, True)["scales_q"] else 1.0
    finite, rel_ok, row_ok, rel, row = criteria(out, ref, base, dtype, factor)
    print(f"{fault} dh {dh} {dtype}: rel {rel:.3e} (bound {TOL[dtype] * factor:.1e}) row {row:.3e} restated {base:.3e}")
    assert criteria(clean, ref, base, dtype, factor)[:3] == (True, True, True)
    if fault in LOCAL:
        # one row of 2 x 161 x 3: the whole-tensor figure does not see it
        assert rel_ok, (rel, TOL[dtype] * factor)
    if fault in ON_NEGATIVE:
        out, ref, clean = planted(fault, dh, dtype, kind="negative")
        base = A.head_row_measure(clean, ref, HEADS)
        assert criteria(clean, ref, base, dtype, factor)[:3] == (True, True, True)
        finite, rel_ok, row_ok, rel, row = criteria(out, ref, base, dtype, factor)
        print(f"{fault} dh {dh} {dtype} on 'negative': rel {rel:.3e} row {row:.3e} restated {base:.3e}")
    assert finite and not row_ok, (rel, row, base)
