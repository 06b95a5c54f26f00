"""The fused GEGLU feed-forward (mobi_ff_geglu, csrc/ff.hip) per output row and channel on every chunk count and tile edge:
tests/ff_cases.py lists the launches (chunk counts 1 - 8, 13 and 40: both tails of the two-chunk loop, the one-chunk launch,
every phase of the two rings; 1 - 257 rows around the wave tile of 32 and the block of 128 at an odd and an even tail; b2
given / NULL, the residual absent / separate / the output itself, the in-kernel LayerNorm as ldm/modules/attention.py calls it
and on the offset, constant, small-variance, spike and interleaved rows of tests/test_gpu_norm_stats.py), tests/ff_ref.py holds
the float64 contract, the fp32 restatement, the measures and the operand builder, and tests/test_ff_ref_cpu.py shows on the
CPU what the criteria accept and reject.

Every launch goes through the C ABI (_lib.FfGegluParams): x, residual, out, b2, gamma and beta are views inside NaN-filled
allocations and the chunk images lie between NaN guard bytes, so a read past the last row or past the images pulls a NaN into
the output.

Criteria, for every launch (a test collects every case's figures before it fails):
  1. the output view is finite; nothing outside the output view changed; no input changed (an in-place residual is the output);
  2. whole-tensor rel-L2 against float64 below TOL of tests/test_gpu_ops.py;
  3. row measure and channel measure at most 2 x those of the fp32 restatement (ff_ref.restated) against the same reference;
  4. a second call returns the same bits; in place equals out of place; row r of a 161-row launch carries the bits of a
     one-row launch of that row;
  5. the refusals of mobi_ff_geglu return their code and leave the output untouched.
Figures go through MOBI_RECORD_ERRORS (golden_cases.record) as <group>.<form>.<dtype>.<case>.<figure>; profiles/ff_rows.txt
(tools/ff_rows_table.py) is the worst of them per <group>.<form>.<dtype>.

Measured on the MI355X (profiles/ff_rows.txt; 44 cases in both storage types, 232 launches, 4 s for the file): the worst
kernel / restated measure is 1.016 (fp16, the row measure of rows.b2+res.fp16.h128.r31) and 1.000 in bf16 -- no rounding point is
missing from the restatement, the one-row launches carry the bits of the 161-row launch, and no kernel fault was found."""
import ctypes as C

import pytest
import torch

from tests import ff_cases as FC
from tests import ff_ref as R
from tests.ff_ref import Case
from tests.golden_cases import record
from tests.test_gpu_ops import DT

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -4                # include/mobi_engine.h
_SIDES = {}


@pytest.fixture(scope="module")
def lib():
    from mobi_amd import _lib
    return _lib.load()


def sides(case, dtype):
    """(operands, float64 reference, fp32 restatement) of a case on the CPU: computed once, never written to."""
    if (case, dtype) not in _SIDES:
        o = R.host_operands(case, dtype)
        _SIDES[(case, dtype)] = (o, R.reference(case, o), R.restated(case, o, dtype))
    return _SIDES[(case, dtype)]


class Checker:
    def __init__(self):
        self.bad, self.launches = [], 0

    def true(self, name, cond):
        if not cond:
            self.bad.append(name)

    def same_bits(self, name, a, b):
        self.true(f"{name}: not bit-identical", a.shape == b.shape and torch.equal(R._bits(a.contiguous()), R._bits(b.contiguous())))

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def wait():
    """Wait for the launch; a device error ends the session (nothing more is started on a GPU that has faulted)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further launches: {e}", returncode=3)


def call(lib, p):
    rc = lib.mobi_ff_geglu(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    wait()
    return rc


class Launch:
    """One case on the device: operands and parameters."""

    def __init__(self, lib, case, dtype, o):
        from mobi_amd import _lib
        self.lib, self.case, self.dtype = lib, case, dtype
        self.od = R.Operands(case, dtype, o)
        self.p = R.fill_params(_lib.FfGegluParams(), case, dtype, self.od.pointers())

    def run(self, ck):
        """Reset the output, launch, return a copy of the output view [rows, c]."""
        self.od.reset_output()
        rc = call(self.lib, self.p)
        ck.launches += 1
        assert rc == OK, (self.case, rc)
        return self.od.out.view[0].clone()


def check_case(ck, lib, group, case, dtype):
    """Criteria 1 - 3 and the second call of one case; returns the output."""
    cid = FC.case_id(group, case, R.storage_name(dtype))
    o, ref, rest = sides(case, dtype)
    L = Launch(lib, case, dtype, o)
    y1 = L.run(ck)
    ck.true(f"{cid}: bytes outside the output view changed", L.od.outside_unchanged())
    ck.true(f"{cid}: an input changed", L.od.unchanged())
    y2 = L.run(ck)
    ck.same_bits(f"{cid}: second call", y1, y2)
    fig, fails = R.judge(dtype, y1, ref, rest)
    bounds = {"rel": R.tolerance(dtype), "row": R.MARGIN * fig["row.restated"], "channel": R.MARGIN * fig["channel.restated"]}
    for k, v in fig.items():
        record(f"{cid}.{k}", v, bounds.get(k, float("nan")))
    record(f"{cid}.launches", 2)
    print(f"{cid}: " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()), flush=True)
    ck.bad += [f"{cid}: {m}" for m in fails.values()]
    return y1


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
@pytest.mark.parametrize("group", ["chunks", "rows", "forms", "ln"])
def test_rows_and_channels(lib, group, dtype):
    """Every case of one group of tests/ff_cases.py."""
    ck = Checker()
    for g, case in FC.CASES:
        if g == group:
            check_case(ck, lib, group, case, dtype)
    assert ck.launches == 2 * sum(g == group for g, _ in FC.CASES)
    record(f"{group}.{R.storage_name(dtype)}.launches", ck.launches)
    ck.done()


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_in_place_equals_out_of_place(lib, dtype):
    """`residual` may alias `out` (include/mobi_engine.h): the same bits as with an output of its own."""
    ck = Checker()
    for inplace, separate in FC.INPLACE_PAIRS:
        a = Launch(lib, inplace, dtype, sides(inplace, dtype)[0])
        b = Launch(lib, separate, dtype, sides(separate, dtype)[0])
        assert a.od.out is a.od.res and torch.equal(sides(inplace, dtype)[0]["res"], sides(separate, dtype)[0]["res"])
        ck.same_bits(f"{inplace.form} {inplace.name}: in place against out of place", a.run(ck), b.run(ck))
        ck.true(f"{inplace.form}: bytes outside the in-place output changed", a.od.outside_unchanged())
    record(f"inplace.{R.storage_name(dtype)}.launches", ck.launches)
    ck.done()


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_a_row_does_not_depend_on_its_lane_or_block(lib, dtype):
    """Row r of a 161-row launch against a one-row launch of that row (every lane of the one-row launch computes row 0:
    `rowc = rows - 1`): the same bits, at an odd and an even tail and with the in-kernel LayerNorm on interleaved regimes."""
    ck = Checker()
    for case in FC.SINGLE_ROW_CASES:
        o = sides(case, dtype)[0]
        whole = Launch(lib, case, dtype, o).run(ck)
        one = Case(1, case.hidden, residual=case.residual, b2=case.b2, ln=case.ln)
        for r in FC.SINGLE_ROWS:
            o1 = dict(o, x=o["x"][r:r + 1].clone(), res=o["res"][r:r + 1].clone())
            L = Launch(lib, one, dtype, o1)
            y = L.run(ck)
            ck.same_bits(f"{case.form} {case.name} {R.storage_name(dtype)}: row {r} alone", y, whole[r:r + 1])
            ck.true(f"{case.name}: row {r} alone wrote outside its output", L.od.outside_unchanged())
    record(f"single_rows.{R.storage_name(dtype)}.launches", ck.launches)
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(lib):
    """Every `return MOBI_ERR_*` of mobi_ff_geglu that arguments can reach, on real operands: the code, and the NaN-filled
    output allocation bit for bit as it was."""
    case = Case(35, 96, ln="standard")
    bad = []
    for dtype in DT:
        L = Launch(lib, case, dtype, sides(case, dtype)[0])
        ptr = L.od.pointers()
        off = lambda name, n: {name: ptr[name] + n}
        cases = [("c = 640", dict(c=640), ERR_UNSUPPORTED),
                 ("hidden = 48", dict(hidden=48), ERR_ARG), ("hidden = 0", dict(hidden=0), ERR_ARG),
                 ("rows = 0", dict(rows=0), ERR_ARG), ("dtype 2", dict(dtype=2), ERR_ARG),
                 ("gamma without beta", dict(ln_beta=None), ERR_ARG),
                 ("no x", dict(x=None), ERR_ARG), ("no weights", dict(w_packed=None), ERR_ARG), ("no output", dict(out=None), ERR_ARG),
                 ("gamma + 4 bytes", off("ln_gamma", 4), ERR_ALIGN), ("beta + 4 bytes", off("ln_beta", 4), ERR_ALIGN)]
        for name in ("x", "out", "residual", "b2", "w_packed"):
            for n in (2, 4):
                if name == "b2" and n == 2:
                    continue                                               # an fp32 vector: 4 bytes is its smallest step
                cases.append((f"{name} + {n} bytes", off(name, n), ERR_ALIGN))
        for name, fields, want in cases:
            from mobi_amd import _lib
            p = R.fill_params(_lib.FfGegluParams(), case, dtype, ptr)
            for k, v in fields.items():
                setattr(p, k, v)
            rc = call(lib, p)
            if rc != want:
                bad.append(f"{R.storage_name(dtype)} {name}: returned {rc}, expected {want}")
            if not (L.od.output_untouched() and L.od.unchanged()):
                bad.append(f"{R.storage_name(dtype)} {name}: the refused call wrote something")
            if rc == OK:
                L.od.reset_output()
        assert call(lib, L.p) == OK and not L.od.output_untouched()      # the same operands, untampered, do launch
    assert not bad, "\n".join(bad)


def test_packed_bytes(lib):
    for h in (32, 96, 160, 1280):
        assert lib.mobi_ff_geglu_packed_bytes(320, h) == (h // 32) * 61 * 1024
    for c, h in ((0, 96), (-32, 96), (48, 96), (330, 96), (320, 0), (320, -32), (320, 48), (320, 100)):
        assert lib.mobi_ff_geglu_packed_bytes(c, h) == 0, (c, h)
