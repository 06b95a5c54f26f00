"""GroupNorm(32) (+ SiLU) and LayerNorm per (image, group) and per row on every kernel form and body: tests/norm_cases.py lists
the launches (every gn_regs_kernel instantiation a shape can reach, plain and from split-K slabs, the two-launch form and its
precise variants, the LDS form; the five layernorm_kernel bodies), each asserted with mobi_groupnorm_kernel_variant /
mobi_layernorm_kernel_variant under its knobs; tests/norm_ref.py holds the float64 contract, the fp32 restatement, the
measures and the operand builder; tests/test_norm_ref_cpu.py shows on the CPU what the criteria reject and that the margin
holds between two orders of summation.

Every launch goes through the C ABI on views inside NaN-filled allocations; every case runs with SiLU and without it, in both
storage types.  Criteria (a test collects every case's figures before it fails):
  1. the output view is finite everywhere (it starts as NaN; a read past the last image's last pixel pulls the guard's NaN into a
     group's statistics); nothing outside the output (and `finished`) views changed; no input changed;
  2. whole-tensor rel-L2 against float64 below TOL of tests/test_gpu_ops.py; 2e-6 for fp32 outputs;
  3. rel-L2 per (image, group) and per (image, channel) -- LayerNorm: per row, per channel over all rows -- at most 2 x the
     fp32 restatement's worst over the case;
  4. without SiLU: the statistics recovered from the rounded output (norm_ref.fitted), |rstd_fit / rstd - 1| and
     |mean_fit - mean| rstd per group / row, at most 2 x the restatement's worst over the case;
  5. a second call returns the same bits;
  6. slab bodies: `finished` is bit for bit the tensor the split source's contract gives on the host, and the output is bit
     for bit that of the plain register launch (the same body without slabs) on that tensor;
  7. out_mode 1 and 3: hi == T(y32) and lo == T(y32 - hi) bit for bit, y32 the same launch's out_mode 2 result.
Figures go through MOBI_RECORD_ERRORS (golden_cases.record) as <form>.<body>.<dtype>.<case>.<figure>;
profiles/norm_groups.txt is the worst of them per form and body (tools/norm_groups_table.py).

What the criteria found: on the fp32 outputs of the precise forms (out_mode 2) the kernel reached 10 x the restatement on
criteria 3 and 4 (precise.f32src.mode2: rstd 1.544e-06 against 1.517e-07, group 1.549e-06 against 1.653e-07) -- the shift of
the statistics' sums was the group's first element, which can lie far from the mean.  csrc/norm.hip now takes gn_shift_x for
those forms and folds in fp64: rstd 8.600e-08, group 9.636e-08.  Every other form agreed with the restatement to 1.05 x."""
import ctypes as C
import dataclasses
import functools

import pytest
import torch

from tests import norm_cases as NC
from tests import norm_ref as R
from tests.golden_cases import record
from tests.igemm_ref import _bits
from tests.test_gpu_ops import DT

pytestmark = pytest.mark.gpu
OK = 0


@pytest.fixture(scope="module")
def lib():
    from mobi_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=2)
def operands(case, dtype):
    return R.host_operands(case, dtype)


def set_knobs(tune, knobs):
    for name in R.KNOBS:
        tune.delenv(name)
    for k, v in knobs:
        tune.setenv(k, v)


class Checker:
    def __init__(self):
        self.bad, self.launches = [], 0

    def true(self, name, cond):
        if not cond:
            self.bad.append(name)

    def same_bits(self, name, a, b):
        self.true(f"{name}: not bit-identical", a.shape == b.shape and a.dtype == b.dtype and
                  torch.equal(_bits(a.contiguous()), _bits(b.contiguous())))

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def wait():
    """Wait for the launch; a device error ends the session (nothing more is started on a GPU that has faulted)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, no further launches: {e}", returncode=3)


class Launch:
    """One (case, dtype) on the device; run(with_silu) resets the outputs, launches and returns a copy of the output view."""

    def __init__(self, lib, case, dtype, o):
        self.lib, self.case, self.dtype = lib, case, dtype
        self.od = R.Operands(lib, case, dtype, o)

    def params(self, with_silu):
        return R.fill_params(self.case, self.dtype, self.od.ptr, with_silu)

    def plan(self):
        p, ss = self.params(True)
        return R.decode_plan(self.lib.mobi_groupnorm_kernel_variant(C.byref(p)))

    def run(self, ck, with_silu):
        self.od.reset_outputs()
        self.od.ws.fill_(float("nan"))
        p, ss = self.params(with_silu)
        rc = self.lib.mobi_groupnorm(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        wait()
        ck.launches += 1
        assert rc == OK, (self.case, rc)
        return self.od.out.view.clone()


def check_case(ck, lib, cid, key, form, body, case, dtype):
    """Criteria 1 - 7 of one case in one storage type, with and without SiLU."""
    o = operands(case, dtype)
    L = Launch(lib, case, dtype, o)
    plan = L.plan()
    assert R.FORM_NAMES[plan["form"]] == form and (body is None or R.body_of(plan) == body), \
        f"{cid}: runs on {R.FORM_NAMES[plan['form']]} {R.body_of(plan)}, the case list says {key}"
    name = f"{key}.{R.storage_name(dtype)}.{cid[len(key) + 1:]}"
    margin = NC.MARGINS.get(cid, R.MARGIN)
    partner = None
    if case.splits:                                                    # the plain register launch on the finished tensor
        plain = dataclasses.replace(case, splits=0, bias=False, rowvec="", residual="", finished=False, row_extra=0)
        partner = Launch(lib, plain, dtype, dict(o, slabs=None, bias=None, rowvec=None, res=None))
        pp = partner.plan()
        assert pp["form"] == R.REGS and R.body_of(pp) == body and pp["gb"] == plan["gb"], (cid, pp)
    y32 = None
    if case.out_mode in (1, 3):
        y32 = Launch(lib, dataclasses.replace(case, out_mode=2), dtype, o)
    for with_silu in (False, True):
        tag = "silu" if with_silu else "plain"
        y1 = L.run(ck, with_silu)
        ck.true(f"{cid} {tag}: bytes outside the output views changed", L.od.outside_unchanged())
        ck.true(f"{cid} {tag}: an input changed", L.od.unchanged())
        if case.finished:
            ck.same_bits(f"{cid} {tag}: finished against the contract on the host", L.od.finished.view.cpu(), o["x0"])
        y2 = L.run(ck, with_silu)
        ck.same_bits(f"{cid} {tag}: second call", y1, y2)
        if partner is not None:
            ck.same_bits(f"{cid} {tag}: slab launch against the plain launch on the finished tensor", y1, partner.run(ck, with_silu))
        if y32 is not None:
            f = y32.run(ck, with_silu)
            hi = f.to(dtype)
            ck.same_bits(f"{cid} {tag}: hi == T(y32)", y1[..., :case.C], hi)
            ck.same_bits(f"{cid} {tag}: lo == T(y32 - hi)", y1[..., case.C:2 * case.C], (f - hi.float()).to(dtype))
            if case.out_mode == 3:
                ck.same_bits(f"{cid} {tag}: third part == hi", y1[..., 2 * case.C:], hi)
        ref = R.reference(case, o, with_silu)
        rest_fig = R.figures(case, o, R.restated(case, o, dtype, with_silu), ref, with_silu)
        fig, fails = R.judge(case, dtype, y1, ref, rest_fig, o, with_silu, margin)
        for k, v in fig.items():
            bound = R.tolerance(dtype, case.f32_out) if k == "rel" else (margin * rest_fig[k] if k in rest_fig else float("nan"))
            record(f"{name}.{tag}.{k}", v, bound)
        print(f"{name} {tag}: " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()), flush=True)
        ck.bad += [f"{cid} {tag} [{R.storage_name(dtype)}]: {m}" for m in fails.values()]
    record(f"{name}.launches", ck.launches)


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
@pytest.mark.parametrize("key", NC.KEYS)
def test_groups_and_channels(lib, tune, key, dtype):
    """Every case of one form and body."""
    ck = Checker()
    for cid, form, body, case in NC.cases_of(key):
        set_knobs(tune, case.knobs)
        check_case(ck, lib, cid, key, form, body, case, dtype)
    ck.done()


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
@pytest.mark.parametrize("body", sorted(set(NC.LN_BODIES.values())), ids=lambda b: f"{b[0]}x{b[1]}")
def test_layernorm_rows(lib, body, dtype):
    """Every case of one layernorm_kernel body: criteria 1 - 5 per row and per channel."""
    ck = Checker()
    for cid, b, case in NC.LN_CASES:
        if b != body:
            continue
        o = R.ln_operands(case, dtype)
        od = R.LnOperands(case, dtype, o)
        p = R.ln_params(case, dtype, od.ptr, od.strides)
        assert R.decode_ln(lib.mobi_layernorm_kernel_variant(C.byref(p))) == body, cid
        outs = []
        for _ in range(2):
            od.reset_outputs()
            rc = lib.mobi_layernorm(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            wait()
            ck.launches += 1
            assert rc == OK, (cid, rc)
            outs.append(od.out.view.clone())
        ck.true(f"{cid}: bytes outside the output view changed", od.outside_unchanged())
        ck.true(f"{cid}: an input changed", od.unchanged())
        ck.same_bits(f"{cid}: second call", outs[0], outs[1])
        ref = R.ln_reference(case, o)
        rest_fig = R.ln_figures(case, o, R.ln_restated(case, o, dtype), ref)
        margin = NC.MARGINS.get(cid, R.MARGIN)
        fig, fails = R.ln_judge(case, dtype, outs[0], ref, rest_fig, o, margin)
        name = f"ln.{body[0]}x{body[1]}.{R.storage_name(dtype)}.{cid.split('.', 2)[2]}"
        for k, v in fig.items():
            bound = R.tolerance(dtype) if k == "rel" else (margin * rest_fig[k] if k in rest_fig else float("nan"))
            record(f"{name}.{k}", v, bound)
        print(f"{name}: " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()), flush=True)
        ck.bad += [f"{cid} [{R.storage_name(dtype)}]: {m}" for m in fails.values()]
    record(f"ln.{body[0]}x{body[1]}.{R.storage_name(dtype)}.launches", ck.launches)
    ck.done()
