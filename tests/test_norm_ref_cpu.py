"""CPU: what tests/test_gpu_norm_groups.py rests on, without a GPU.

  - every case of tests/norm_cases.py lands on the form and kernel body its id names, by mobi_groupnorm_kernel_variant /
    mobi_layernorm_kernel_variant (queries: no launch) under the case's knobs, and none lands on the chunks-through-memory form;
  - a sweep of the query (C = 256 .. 2560 in steps of 64, batch 1 / 2 / 3 / 8 / 16 / 32, hw = 1 .. 4200) reaches 18 of the 20
    gn_regs_kernel instantiations and 12 of the 13 slab instantiations: the case list covers every one of them;
    norm_cases.UNREACHABLE_REGS / UNREACHABLE_SLABS name the rest.  The same for the five LayerNorm bodies;
  - the criteria reject six seeded faults of the fp32 restatement, two of which the whole-tensor rel-L2 lets pass;
  - margin check: the restatement and a second one whose sums run over the pixels (LayerNorm: channels) in a permuted order
    satisfy every criterion against each other's figures on every case with the margin 2 of the GPU test -- no case needed a
    larger factor (norm_cases.MARGINS would hold it; it is empty).  The permutation moves the figures in the third digit at
    most: what they measure is the output rounding, not the order of the sums.  The cases above 4 M elements are checked in
    fp16 without SiLU only, to keep this file quick."""
import ctypes as C
import functools
import os

import pytest
import torch

from tests import norm_cases as NC
from tests import norm_ref as R

DT = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def lib():
    from mobi_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def set_knobs(tune, knobs):
    for name in R.KNOBS:
        tune.delenv(name)
    for k, v in knobs:
        tune.setenv(k, v)


def test_cases_land_on_the_bodies_their_ids_name(lib, tune):
    bad, gbs = [], set()
    for cid, form, body, case in NC.CASES:
        set_knobs(tune, case.knobs)
        v = R.query(lib, case)
        if v < 0:
            bad.append(f"{cid}: refused with {v}")
            continue
        plan = R.decode_plan(v)
        if R.FORM_NAMES[plan["form"]] != form or (body is not None and R.body_of(plan) != body):
            bad.append(f"{cid}: lands on {R.FORM_NAMES[plan['form']]} {R.body_of(plan)}")
        if body is None and R.body_of(plan) != (0, 0, 0):
            bad.append(f"{cid}: a form without a body reports {R.body_of(plan)}")
        if form == "regs":
            gbs.add(plan["gb"])
    assert not bad, "\n".join(bad)
    assert gbs == {1, 2, 4}, gbs
    set_knobs(tune, NC.BEYOND_LDS.knobs)
    assert R.decode_plan(R.query(lib, NC.LDS_FORM[0][1]))["form"] == R.LDS
    assert R.decode_plan(R.query(lib, NC.BEYOND_LDS))["form"] == R.TWO
    for cid, body, case in NC.LN_CASES:
        assert R.decode_ln(R.ln_query(lib, case.C)) == body, cid


def test_the_query_answers_what_the_launch_would(lib, tune):
    """Errors come back as mobi_groupnorm returns them (no launch is reached: there is no device here), the chunked form is
    reported only with arrival counters, and the knobs move the plan."""
    set_knobs(tune, ())
    base = R.Case(2, 64, 640)
    p, _ = R.fill_params(base, torch.float16, R.fake_pointers(base), True)
    q = lambda: lib.mobi_groupnorm_kernel_variant(C.byref(p))
    assert lib.mobi_groupnorm_kernel_variant(None) == -1
    want = R.decode_plan(q())
    assert want == dict(form=R.REGS, gb=2, pw=8, items=2, threads=256), want
    for field, value, err in (("c0", 48, -2), ("out", None, -1), ("dtype", 2, -1), ("batch", 0, -1), ("out", (1 << 20) + 8, -4),
                              ("out_mode", 4, -1), ("src_f32", 2, -1), ("sync", (1 << 20) + 2, -4)):
        old = getattr(p, field)
        setattr(p, field, value)
        assert q() == err == lib.mobi_groupnorm(C.byref(p), None), field
        setattr(p, field, old)
    p.out_mode = 2
    assert R.decode_plan(q()) == dict(form=R.PRECISE, gb=0, pw=0, items=0, threads=0)
    p.out_mode = 0
    split = R.Case(3, 1024, 2560, splits=2)
    ps, ss = R.fill_params(split, torch.float16, R.fake_pointers(split), True)
    assert lib.mobi_groupnorm_kernel_variant(C.byref(ps)) == -2 == lib.mobi_groupnorm(C.byref(ps), None)      # 12 pieces per thread
    assert lib.mobi_groupnorm_takes_split(2560, 0, 3, 1024) == 0
    pw4 = R.Case(1, 1429, 320, splits=3)
    assert R.query(lib, pw4) == -2
    set_knobs(tune, NC.SPLIT_PW4)
    assert R.decode_plan(R.query(lib, pw4)) == dict(form=R.SLABS, gb=2, pw=4, items=8, threads=1024)
    set_knobs(tune, (("MOBI_GN_COOP", "1"),))
    big = R.Case(16, 1024, 640)
    pc, _ = R.fill_params(big, torch.float16, R.fake_pointers(big), True)
    assert R.decode_plan(lib.mobi_groupnorm_kernel_variant(C.byref(pc)))["form"] == R.REGS                      # no counters
    pc.sync = 1 << 20
    chunks = R.decode_plan(lib.mobi_groupnorm_kernel_variant(C.byref(pc)))
    assert chunks["form"] == R.CHUNKS and chunks["threads"] == 1024 and chunks["pw"] == 8 and chunks["gb"] in (2, 4, 8, 16, 32)
    set_knobs(tune, NC.FUSED0)
    assert R.decode_plan(lib.mobi_groupnorm_kernel_variant(C.byref(pc)))["form"] == R.TWO
    set_knobs(tune, ())
    assert lib.mobi_layernorm_kernel_variant(None) == -1
    assert R.ln_query(lib, 2568) == -2 and R.ln_query(lib, 12) == -2
    a = 1 << 20
    lp = R.ln_params(R.LnCase(2, 4, 320), torch.float16, dict(x=a, out=a, gamma=a + 4, beta=a))
    assert lib.mobi_layernorm_kernel_variant(C.byref(lp)) == -4 == lib.mobi_layernorm(C.byref(lp), None)


INSTANTIATIONS = {(th, it, 8) for th in (256, 1024) for it in (1, 2, 3, 4, 6, 8, 12, 16)} | {(1024, it, 4) for it in (8, 12, 16, 24)}
SLAB_INSTANTIATIONS = {(th, it, 8) for th in (256, 1024) for it in (1, 2, 3, 4, 6, 8)} | {(1024, 8, 4)}


def _sweep(lib, batches, splits):
    """The bodies the query names over the grid, and the forms it names."""
    found, forms = set(), set()
    for n in batches:
        for ch in range(256, 2561, 64):
            case = R.Case(n, 1, ch, splits=splits)
            p, ss = R.fill_params(case, torch.float16, R.fake_pointers(case), True)
            ref = C.byref(p)
            for hw in range(1, 4201):
                p.hw = hw
                v = lib.mobi_groupnorm_kernel_variant(ref)
                if v >= 0 and v & 15 in (R.REGS, R.SLABS):
                    found.add(v >> 10)                                   # pw, items, threads
                forms.add(v & 15 if v >= 0 else v)
    return {(b >> 10 & 2047, b >> 4 & 63, b & 15) for b in found}, forms


def test_sweep_reaches_every_body_the_cases_cover(lib, tune):
    set_knobs(tune, ())
    regs, forms = _sweep(lib, (1, 2, 3, 8, 16, 32), 0)
    assert forms <= {R.REGS, R.LDS, R.TWO}, forms
    assert regs == set(NC.REGS), regs ^ set(NC.REGS)
    assert INSTANTIATIONS - regs == NC.UNREACHABLE_REGS
    slabs, forms = _sweep(lib, (1, 3, 32), 2)
    assert forms <= {R.SLABS, -2}, forms
    set_knobs(tune, NC.SPLIT_PW4)
    slabs |= _sweep(lib, (1, 16), 2)[0]
    assert slabs == set(NC.SLABS), slabs ^ set(NC.SLABS)
    assert SLAB_INSTANTIATIONS - slabs == NC.UNREACHABLE_SLABS
    ln = {R.decode_ln(R.ln_query(lib, ch)) for ch in range(8, 2561, 8)}
    assert ln == set(NC.LN_BODIES.values()) and len(ln) == 5, ln


# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def sides(cid, dtype, with_silu):
    case = next(c for i, _, _, c in NC.CASES if i == cid)
    o = R.host_operands(case, dtype)
    ref = R.reference(case, o, with_silu)
    return case, o, ref, R.figures(case, o, R.restated(case, o, dtype, with_silu), ref, with_silu)


def rejected(cid, dtype, hook):
    case, o, ref, rest_fig = sides(cid, dtype, False)
    fig, bad = R.judge(case, dtype, R.restated(case, o, dtype, False, hook=hook), ref, rest_fig, o, False)
    print(cid, R.storage_name(dtype), {k: f"{v:.3e}" for k, v in fig.items()}, sorted(bad))
    return fig, bad


WIDE = "regs.1024x8x4.batch16.1024x320"          # 16 images of 10-channel groups: columns straddle two groups
TWO_SOURCES = "regs.256x6x8.two.320+640"


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_one_group_variance_off_by_half_a_percent_is_rejected_where_rel_l2_passes(dtype):
    def stats(mean_c, var_c):
        var_c[5, 130:140] /= 1.005                                       # group 13 of image 5
    fig, bad = rejected(WIDE, dtype, dict(stats=stats))
    assert "rstd" in bad and "rel" not in bad and fig["rel"] < R.tolerance(dtype)
    assert fig["rstd"] > 5 * fig["rstd.restated"]


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_a_straddling_column_on_its_neighbours_statistics_is_rejected_where_rel_l2_passes(dtype):
    def stats(mean_c, var_c):                                            # column 8 .. 15: channels 10 .. 15 belong to group 1
        mean_c[3, 10:16] = mean_c[3, 9]
        var_c[3, 10:16] = var_c[3, 9]
    fig, bad = rejected(WIDE, dtype, dict(stats=stats))
    assert "channel" in bad and "rel" not in bad and fig["rel"] < R.tolerance(dtype)


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_shifted_affine_wrong_stride_and_missing_pixel_are_rejected(dtype):
    def affine(gamma_c, beta_c):                                         # one 8-channel column, every image
        gamma_c[:, 41:48] = gamma_c[:, 40:47].clone()
        beta_c[:, 41:48] = beta_c[:, 40:47].clone()
    fig, bad = rejected(TWO_SOURCES, dtype, dict(affine=affine))
    assert "channel" in bad, bad

    def wrong_stride(x):                                                 # image 1's second source read with c0 as its pixel stride
        case = sides(TWO_SOURCES, dtype, False)[0]
        x = x.clone()
        flat = x[1, :, case.c0:].reshape(-1)
        idx = (torch.arange(case.hw)[:, None] * case.c0 + torch.arange(case.c1)[None, :]) % flat.numel()
        x[1, :, case.c0:] = flat[idx]
        return x
    fig, bad = rejected(TWO_SOURCES, dtype, dict(x=wrong_stride))
    assert {"group", "channel", "rstd", "mean"} <= set(bad), bad

    def missing(out):
        out = out.clone()
        out[1, 76] = float("nan")                                        # the last pixel of the last image keeps its NaN
        return out
    fig, bad = rejected(TWO_SOURCES, dtype, dict(y=missing))
    assert "finite" in bad, bad


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_layernorm_last_row_on_the_previous_rows_statistics_is_rejected(dtype):
    cid, body, case = next(c for c in NC.LN_CASES if c[0] == "ln.5x16.c640.rows17")
    o = R.ln_operands(case, dtype)
    ref = R.ln_reference(case, o)
    rest_fig = R.ln_figures(case, o, R.ln_restated(case, o, dtype), ref)

    def stats(mean, var):
        mean[-1], var[-1] = mean[-2], var[-2]
    fig, bad = R.ln_judge(case, dtype, R.ln_restated(case, o, dtype, hook=dict(stats=stats)), ref, rest_fig, o)
    assert {"group", "rstd", "mean"} <= set(bad), bad
    assert not R.ln_judge(case, dtype, R.ln_restated(case, o, dtype), ref, rest_fig, o)[1]


# ----------------------------------------------------------------------------------------------------------------------
def _pair_fails(a, b, margin):
    return [f"{k}: {a[k]:.3e} against {b[k]:.3e}" for k in a if k != "rel" and not (a[k] <= margin * b[k] and b[k] <= margin * a[k])]


@pytest.mark.parametrize("key", NC.KEYS)
def test_margin_holds_between_two_orders_of_summation(key):
    bad = []
    for cid, form, body, case in NC.cases_of(key):
        large = case.n * case.hw * case.C > 4_000_000
        for dtype in DT[:1] if large else DT:
            o = R.host_operands(case, dtype)
            perm = torch.randperm(case.hw, generator=torch.Generator().manual_seed(case.hw))
            for with_silu in (False,) if large else (False, True):
                ref = R.reference(case, o, with_silu)
                a = R.figures(case, o, R.restated(case, o, dtype, with_silu), ref, with_silu)
                b = R.figures(case, o, R.restated(case, o, dtype, with_silu, perm=perm), ref, with_silu)
                tol = R.tolerance(dtype, case.f32_out)
                if not (a["rel"] < tol and b["rel"] < tol):
                    bad.append(f"{cid} {R.storage_name(dtype)}: whole-tensor rel-L2 {a['rel']:.3e} / {b['rel']:.3e} >= {tol:.1e}")
                bad += [f"{cid} {R.storage_name(dtype)} silu={with_silu}: {m}" for m in _pair_fails(a, b, NC.MARGINS.get(cid, R.MARGIN))]
    assert not bad, "\n".join(bad)


def test_margin_holds_for_layernorm():
    bad = []
    for cid, body, case in NC.LN_CASES:
        for dtype in DT:
            o = R.ln_operands(case, dtype)
            ref = R.ln_reference(case, o)
            perm = torch.randperm(case.C, generator=torch.Generator().manual_seed(case.C))
            a = R.ln_figures(case, o, R.ln_restated(case, o, dtype), ref)
            b = R.ln_figures(case, o, R.ln_restated(case, o, dtype, perm=perm), ref)
            if not (a["rel"] < R.tolerance(dtype) and b["rel"] < R.tolerance(dtype)):
                bad.append(f"{cid} {R.storage_name(dtype)}: whole-tensor rel-L2 {a['rel']:.3e} / {b['rel']:.3e}")
            bad += [f"{cid} {R.storage_name(dtype)}: {m}" for m in _pair_fails(a, b, NC.MARGINS.get(cid, R.MARGIN))]
    assert not bad, "\n".join(bad)


def test_split_source_contract_is_the_plain_sum_in_order():
    """finish_slabs against float64 on a case with every term, and the operand it feeds the reference is its rounding."""
    case = next(c for i, _, _, c in NC.CASES if i == "slabs.256x4x8.s5.all")
    o = R.host_operands(case, torch.float16)
    s = o["slabs"][..., :case.c0].double().sum(0) + o["bias"].double() + o["rowvec"].double()[:, None, :] + o["res"].double()
    assert torch.isfinite(o["x0"].float()).all()
    assert R.rel_l2(o["x0"], s) < 4e-4 and o["x0"].dtype == torch.float16
    assert float((o["x0"].double() - s).abs().max()) <= float(s.abs().max()) * 2.0 ** -11 * 1.01
