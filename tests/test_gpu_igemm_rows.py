"""The implicit GEMM (mobi_igemm) per output row and channel on every kernel body: tests/igemm_cases.py lists the launches
(every main loop launch_igemm can select, forced with the A/B environment and asserted with mobi_igemm_kernel_variant, on full
and ragged tiles, every gather / epilogue / weight / split form at the smallest sizes at which it can go wrong),
tests/igemm_ref.py holds the float64 contract, the fp32 restatement, the measures and the operand builder, and
tests/test_igemm_ref_cpu.py shows on the CPU what the criteria reject.

The body cases go through the C ABI (_lib.IgemmParams): each operand is a view inside a NaN-filled allocation, with image
strides beyond dense, a gap between per-group weight matrices, defer_finish + mobi_igemm_finish and the refusals, which
ops.igemm cannot all express; one path keeps the cases uniform.  test_wrapper_derives_strides_and_pointers runs the forms
the wrapper can express through ops.igemm on the same NaN-surrounded views.  Which launches of test_split_forms_are_bit_identical
finish inside the launch is igemm_ref.plan's reading of igemm_plan (the library does not report it); the sync8.* cases are
built so that both modes do, and the test refuses a fall-back for them.

Criteria, for every launch (a test collects every case's figures before it fails):
  1. the output view is finite everywhere (it starts as NaN; the NaN around every operand would be pulled in by a read past
     an image, a weight row past n_packed or a rowvec of the wrong image's gap); nothing outside the output view changed;
     no input changed (an in-place residual is the output);
  2. whole-tensor rel-L2 against float64 below TOL of tests/test_gpu_ops.py, 1.5 TOL for a LayerNorm-folded product;
  3. 16-bit outputs: row measure and channel measure at most 2 x those of the fp32 restatement (igemm_ref.restated);
  4. fp32 outputs and the slabs of a defer_finish launch: |got - ref| <= (k + 8) 2^-24 A element-wise (igemm_ref.f32_bound);
  5. a second call returns the same bits;
  6. bit-identical forms: the in-launch finish (MOBI_IGEMM_FUSED_SPLIT 1 and 2) and mobi_igemm_finish after defer_finish
     against the reduce launch; MOBI_IGEMM_SM64_OVL unset against 0; weight_tiled present against absent;
  7. the register epilogues against the LDS-staged epilogue of the same body: 2 ulp, as tests/test_gpu_ops.py has it.
Figures go through MOBI_RECORD_ERRORS (golden_cases.record) as <body>.<epilogue form>.<dtype>.<case>.<figure>;
profiles/igemm_rows.txt is the worst of them per such triple."""
import ctypes as C
import dataclasses
import functools
import os

import pytest
import torch

from tests import igemm_cases as IC
from tests import igemm_ref as R
from tests.golden_cases import record
from tests.igemm_ref import Case
from tests.test_gpu_ops import DT

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -4                # include/mobi_engine.h


@pytest.fixture(scope="module")
def lib():
    from mobi_amd import _lib
    return _lib.load()


@functools.lru_cache(maxsize=None)
def sides(case, dtype):
    """(operands, float64 reference, fp32 restatement) of a case on the CPU: computed once, never written to."""
    o = R.used(case, R.host_operands(case, dtype))
    return o, R.reference(case, o), R.restated(case, o, dtype)


def set_knobs(tune, knobs):
    for name in [k for k in os.environ if k.startswith("MOBI_IGEMM_")]:
        tune.delenv(name)
    for k, v in knobs.items():
        tune.setenv("MOBI_IGEMM_" + k, v)


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


class Launch:
    """One case on the device: operands, parameters, workspace."""

    def __init__(self, lib, case, dtype, knobs, key=None):
        from mobi_amd import _lib, ops
        self.lib, self.case, self.dtype = lib, case, dtype
        self.o, self.ref, self.rest = sides(case, dtype)
        self.plan = R.plan(case, knobs)
        self.od = od = R.Operands(case, dtype, self.o)
        ptr = dict(src0=od.x.view.data_ptr(), weight=od.w.view.data_ptr(), out=od.out.view.data_ptr())
        for name, placed in (("src1", od.x2), ("bias", od.bias), ("rowvec", od.rowvec), ("residual", od.res), ("ln_svec", od.svec)):
            if placed is not None:
                ptr[name] = placed.view.data_ptr()
        self.wt = None
        if case.w_tiled:
            self.wt = ops.tile_weights(od.w.view[0].contiguous())
            assert self.wt is not None
            ptr["weight_tiled"] = self.wt.data_ptr()
        self.p = p = R.fill_params(_lib.IgemmParams(), case, dtype, ptr,
                                   dict(src=od.src_img_stride, w=od.w_group_stride, rowvec=od.rowvec_stride,
                                        res=od.res_img_stride, out=od.out_img_stride))
        self.ws = self.sync = None
        if case.split_k > 1:
            nbytes = lib.mobi_igemm_workspace_bytes(C.byref(p), case.split_k)
            self.ws = torch.full((nbytes // 4 + 8,), float("nan"), dtype=torch.float32, device="cuda")
            p.ws = self.ws.data_ptr()
            self.sync = torch.zeros((lib.mobi_igemm_sync_bytes(C.byref(p), case.split_k) // 4 + 8,), dtype=torch.int32,
                                    device="cuda")
        # <body>.<epilogue form>.<dtype>; the body is the case list's key (ring64 and ring128s are both MOBI_IGEMM_RING_128)
        self.name = f"{key or self.plan['body_name']}.{self.plan['epilogue'].replace('.', '+')}.{R.storage_name(dtype)}"

    def variant(self):
        return self.lib.mobi_igemm_kernel_variant(C.byref(self.p))

    def run(self, ck, sync=False, defer=False):
        """Reset the output, launch, return a copy of the output view."""
        self.od.reset_output()
        self.p.sync = self.sync.data_ptr() if sync else None
        self.p.defer_finish = int(defer)
        rc = self.lib.mobi_igemm(C.byref(self.p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        wait()
        ck.launches += 1
        assert rc == OK, (self.case, rc)
        return self.od.out.view.clone()

    def finish(self):
        rc = self.lib.mobi_igemm_finish(C.byref(self.p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        wait()
        assert rc == OK, (self.case, rc)
        return self.od.out.view.clone()


def check_case(ck, lib, cid, key, knobs, case, dtype):
    """Criteria 1 - 5 of one case; returns (launch, output)."""
    L = Launch(lib, case, dtype, knobs, key)
    body = L.variant()
    assert body == L.plan["body"] and body in IC.EXPECTED_BODY[key], \
        f"{cid}: runs on {R.BODY_NAMES[body] if body >= 0 else body}, the case list says {key} ({L.plan['body_name']})"
    y1 = L.run(ck)
    ck.true(f"{cid}: bytes outside the output view changed", L.od.outside_unchanged())
    ck.true(f"{cid}: an input changed", L.od.unchanged())
    y2 = L.run(ck)
    ck.same_bits(f"{cid}: second call", y1, y2)
    fig, fails = R.judge(case, dtype, y1, L.ref, L.rest, L.o)
    bounds = {"rel": R.tolerance(case, dtype), "f32": 1.0, "row": R.MARGIN * fig.get("row.restated", 0.0),
              "channel": R.MARGIN * fig.get("channel.restated", 0.0)}
    for k, v in fig.items():
        record(f"{L.name}.{cid}.{k}", v, bounds.get(k, float("nan")))
    record(f"{L.name}.{cid}.launches", 2)
    print(f"{L.name} {cid}: " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()), flush=True)
    ck.bad += [f"{cid} [{L.name}]: {m}" for m in fails.values()]
    return L, y1


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
@pytest.mark.parametrize("key", list(IC.BODIES))
def test_rows_and_channels(lib, tune, key, dtype):
    """Every case of one body (split-K cases by the reduce launch; tests below add the other finishes)."""
    knobs = IC.BODIES[key][0]
    set_knobs(tune, knobs)
    ck = Checker()
    for cid, k, _, case in IC.CASES:
        if k == key:
            check_case(ck, lib, cid, key, knobs, case, dtype)
    record(f"{key}.{R.storage_name(dtype)}.launches", ck.launches)
    ck.done()


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_split_forms_are_bit_identical(lib, tune, dtype):
    """The reduce launch, the in-launch finish in modes 1 and 2 (arrival counters zero again afterwards), and
    mobi_igemm_finish after defer_finish (the output untouched until then, every slab within the fp32 bound of its k range)."""
    ck = Checker()
    taken_modes = set()
    for cid, key, knobs, case in IC.SPLIT_CASES:
        set_knobs(tune, knobs)
        L = Launch(lib, case, dtype, knobs, key)
        want = L.run(ck)
        for mode in (1, 2):
            set_knobs(tune, dict(knobs, FUSED_SPLIT=mode))
            assert L.variant() == L.plan["body"], cid
            # whether the launch finishes itself is plan()'s reading of igemm_plan (mode 2 needs tiles % 8 == 0, both need
            # <= 4 slabs); the cases built for it (sync8.*) must get the mode asked for, a fall-back to the reduce launch
            # would compare that launch with itself
            taken = IC.in_launch_mode(case, knobs, mode)
            taken_modes.add((mode, taken == mode))
            assert "sync8" not in cid or taken == mode, f"{cid}: mode {mode} falls back to the reduce launch"
            ck.same_bits(f"{cid}: in-launch finish mode {mode} ({'in the launch' if taken else 'reduce launch'})",
                         L.run(ck, sync=True), want)
            ck.true(f"{cid}: arrival counters not zero after mode {mode}", not bool(L.sync.any()))
            ck.true(f"{cid}: mode {mode} wrote outside the output view", L.od.outside_unchanged())
        set_knobs(tune, knobs)
        if case.out_mode != "rows":
            L.p.sync, L.p.defer_finish = None, 1
            ck.true(f"{cid}: defer_finish with an fp32 output is not refused", lib.mobi_igemm_slab_count(C.byref(L.p)) == ERR_UNSUPPORTED)
            continue
        L.ws.fill_(float("nan"))
        L.run(ck, defer=True)
        ck.true(f"{cid}: defer_finish wrote the output", L.od.output_untouched())
        count = lib.mobi_igemm_slab_count(C.byref(L.p))
        ck.true(f"{cid}: {count} slabs, expected {L.plan['splits']}", count == L.plan["splits"])
        slabs = L.ws[:count * case.m * case.n_packed].reshape(count, case.n, case.hw, case.n_packed).cpu()
        ck.true(f"{cid}: a slab element was not written", bool(torch.isfinite(slabs).all()))
        ck.true(f"{cid}: workspace past the slabs written", bool(torch.isnan(L.ws[count * case.m * case.n_packed:]).all()))
        ref = R.slab_products(case, L.o, case.split_k, torch.float64)
        mag = R.slab_products(case, L.o, case.split_k, torch.float64, absolute=True)
        worst = 0.0
        for s, (k0, k1) in enumerate(R.split_ranges(case, case.split_k)):
            worst = max(worst, R.bound_ratio(torch.nan_to_num(slabs[s]), ref[s], (k1 - k0 + 8) * R.U32 * mag[s]))
        record(f"{L.name}.{cid}.slab.f32", worst)
        ck.true(f"{cid}: a slab reaches {worst:.3f} x its fp32 bound", worst <= 1.0)
        L.p.defer_finish = 1
        ck.same_bits(f"{cid}: mobi_igemm_finish", L.finish(), want)
    record(f"split_forms.{R.storage_name(dtype)}.launches", ck.launches)
    assert {(1, True), (2, True)} <= taken_modes, taken_modes      # both modes really finished some launch in the launch
    ck.done()


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_sm64_overlap_and_tiled_weights_are_bit_identical(lib, tune, dtype):
    ck = Checker()
    for cid, key, knobs, case in IC.CASES:
        if key == "ring64seq":
            set_knobs(tune, knobs)
            seq = Launch(lib, case, dtype, knobs).run(ck)
            set_knobs(tune, IC.BODIES["ring64"][0])
            ck.same_bits(f"{cid}: MOBI_IGEMM_SM64_OVL unset against 0", Launch(lib, case, dtype, knobs).run(ck), seq)
    for cid, key, knobs, case in IC.WTILED_CASES:
        set_knobs(tune, knobs)
        with_t = Launch(lib, case, dtype, knobs)
        if not with_t.plan["w_tiled"]:
            continue                                               # (this body reads W only: both launches would be one)
        plain = dataclasses.replace(case, w_tiled=False)
        ck.same_bits(f"{cid}: weight_tiled against W alone", with_t.run(ck), Launch(lib, plain, dtype, knobs).run(ck))
    assert ck.launches >= 8
    record(f"bit_identical_forms.{R.storage_name(dtype)}.launches", ck.launches)
    ck.done()


STAGED_PARTNER = {"ring256r": dict(RING_DIRECT=0), "ring128r": dict(SM_DIRECT=0), "ring128w": dict(SM_DIRECT=0),
                  "ring64": dict(SM_DIRECT=0), "ring64seq": dict(SM_DIRECT=0)}


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_register_epilogues_within_two_ulp_of_the_staged_one(lib, tune, dtype):
    ulp = 2.0 ** (-7 if dtype == torch.bfloat16 else -10)
    ck = Checker()
    for cid, key, knobs, case in IC.CASES:
        if key not in STAGED_PARTNER or case.split_k > 1 or R.plan(case, knobs)["epilogue"] != "register":
            continue
        set_knobs(tune, knobs)
        reg = Launch(lib, case, dtype, knobs).run(ck).float()
        other = dict(knobs, **STAGED_PARTNER[key])
        assert R.plan(case, other)["epilogue"] == "staged" and R.plan(case, other)["kernel"] == R.plan(case, knobs)["kernel"], cid
        set_knobs(tune, other)
        st = Launch(lib, case, dtype, other).run(ck).float()
        d = float(((reg - st).abs() / st.abs().clamp_min(1.0)).max())
        record(f"{key}.register_vs_staged.{R.storage_name(dtype)}.{cid}", d, 2 * ulp)
        ck.true(f"{cid}: register and staged epilogue differ by {d:.3e} > 2 ulp", d <= 2 * ulp)
    assert ck.launches >= 16
    record(f"register_vs_staged.{R.storage_name(dtype)}.launches", ck.launches)
    ck.done()


WRAPPER_CASES = ("straddle.1x1.all", "w1.3x3", "s2.asym.two", "up.two", "geglu.ragged", "f32.ragged", "tr.hw43.coutQp1",
                 "mPp1.1x1.scale.inplace", "ln.ragged", "leaky.ragged.res", "rowvec.nobias.hw64", "mP.4x4.3x3.res.nt5")


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_wrapper_derives_strides_and_pointers(lib, tune, dtype):
    """The cases ops.igemm can express, through ops.igemm on the library's own route (no knobs): the wrapper's image strides
    (source, residual, output, rowvec), the in-place residual and the explicit output size come from the NaN-surrounded views,
    so a stride or pointer it derives wrongly is a NaN or a changed byte outside the view.  Criteria 1 - 4."""
    from mobi_amd import _lib, ops
    set_knobs(tune, {})
    ck = Checker()
    for cid, key, knobs, case in IC.CASES:
        if key != "ring128s" or cid.split(".", 1)[1] not in WRAPPER_CASES:
            continue
        o, ref, rest = sides(case, dtype)
        od = R.Operands(case, dtype, o)
        pw = ops.Packed(od.w.view[0], None if od.bias is None else od.bias.view[0], case.kh, case.kw, case.C, case.cout,
                        case.n_packed, geglu=case.geglu)
        if case.ln:
            pw.svec, pw.ln_eps = od.svec.view[0], R.LN_EPS
        as4 = lambda t: t.view(case.n, case.ho, case.wo, case.cout)
        out = od.out.view if case.out_mode == "tr" else as4(od.out.view)
        y = ops.igemm(od.x.view, pw, x2=None if od.x2 is None else od.x2.view, stride=case.stride, pad=(case.pad_h, case.pad_w),
                      upsample=case.upsample, hout=case.ho, wout=case.wo, rowvec=None if od.rowvec is None else od.rowvec.view,
                      rowvec_has_bias=False, residual=None if od.res is None else as4(od.res.view), out=out,
                      out_mode={"rows": _lib.OUT_ROWS, "tr": _lib.OUT_TRANSPOSED, "f32": _lib.OUT_ROWS_F32}[case.out_mode],
                      scale=case.scale, split_k=1, leaky=case.epilogue == "leaky")
        wait()
        ck.launches += 1
        ck.true(f"{cid}: the wrapper returned another tensor", y.data_ptr() == od.out.view.data_ptr())
        ck.true(f"{cid}: bytes outside the output view changed", od.outside_unchanged())
        ck.true(f"{cid}: an input changed", od.unchanged())
        fig, fails = R.judge(case, dtype, od.out.view, ref, rest, o)
        for k, v in fig.items():
            record(f"wrapper.ops_igemm.{R.storage_name(dtype)}.{cid}.{k}", v, R.tolerance(case, dtype) if k == "rel" else float("nan"))
        record(f"wrapper.ops_igemm.{R.storage_name(dtype)}.{cid}.launches", 1)
        ck.bad += [f"{cid} [ops.igemm]: {m}" for m in fails.values()]
    assert ck.launches == len(WRAPPER_CASES), ck.launches
    record(f"wrapper.{R.storage_name(dtype)}.launches", ck.launches)
    ck.done()


def test_every_instantiation_and_axis_value_has_a_case():
    """Closing check on the list the tests above ran: every (kernel, epilogue form) launch_igemm can select, with a ragged pixel and channel tile where its eligibility allows them, and every axis value on an LDS-DMA body
    and on a register-staged one (igemm_cases.missing names what is not there)."""
    assert not IC.missing(), "\n".join(IC.missing())


# ----------------------------------------------------------------------------------------------------------------------
def _query(lib, case, **fields):
    from mobi_amd import _lib
    p = R.fill_params(_lib.IgemmParams(), case, torch.float16, R.fake_pointers(case))
    for k, v in fields.items():
        setattr(p, k, v)
    return lib.mobi_igemm_kernel_variant(C.byref(p)), lib.mobi_igemm_slab_count(C.byref(p))


def test_refusals(lib, tune):
    """One case per `return MOBI_ERR_*` of igemm_plan that arguments alone can reach (csrc/igemm_plan.hip); no launch."""
    set_knobs(tune, {})
    base = Case(2, 4, 4, 64, 136, kh=3, kw=3, pad_h=1, pad_w=1)
    split = dataclasses.replace(base, split_k=2)
    ln = Case(2, 4, 4, 64, 136, ln=True)
    rep = dataclasses.replace
    cases = [
        ("no source", base, dict(src0=None), ERR_ARG),
        ("no weight", base, dict(weight=None), ERR_ARG),
        ("no output", base, dict(out=None), ERR_ARG),
        ("dtype", base, dict(dtype=2), ERR_ARG),
        ("c0 % 32", rep(base, c0=48), {}, ERR_UNSUPPORTED),
        ("c1 without src1", base, dict(c1=32), ERR_UNSUPPORTED),
        ("batch 0", base, dict(batch=0), ERR_ARG),
        ("hout 0", base, dict(hout=0), ERR_ARG),
        ("stride 0", base, dict(stride=0), ERR_ARG),
        ("groups do not divide the batch", rep(base, n=3, groups=2), {}, ERR_ARG),
        ("cout 0", base, dict(cout=0, n_packed=0), ERR_ARG),
        ("upsample 2", base, dict(upsample=2), ERR_ARG),
        ("unknown epilogue", base, dict(epilogue=3), ERR_ARG),
        ("leaky transposed", rep(base, epilogue="leaky", out_mode="tr"), {}, ERR_UNSUPPORTED),
        ("leaky split", rep(split, epilogue="leaky"), {}, ERR_UNSUPPORTED),
        ("out_mode 3", base, dict(out_mode=3), ERR_ARG),
        ("cout % 8 in rows", rep(base, cout=132), {}, ERR_UNSUPPORTED),
        ("GEGLU with residual", rep(base, cout=64, epilogue="geglu", residual="dense"), {}, ERR_UNSUPPORTED),
        ("GEGLU transposed", rep(base, cout=64, epilogue="geglu", out_mode="tr"), {}, ERR_UNSUPPORTED),
        ("n_packed != cout", base, dict(n_packed=144), ERR_ARG),
        ("GEGLU n_packed != 2 cout", rep(base, cout=64, epilogue="geglu"), dict(n_packed=64), ERR_ARG),
        ("transposed with rowvec", rep(base, out_mode="tr", rowvec=True), {}, ERR_UNSUPPORTED),
        ("bias alignment", base, dict(bias=(1 << 20) + 4), ERR_ALIGN),
        ("rowvec_stride % 4", rep(base, rowvec=True), dict(rowvec_stride=138), ERR_ALIGN),
        ("source alignment", base, dict(src0=(1 << 20) + 8), ERR_ALIGN),
        ("LayerNorm fold on 3 x 3", rep(base, ln=True), {}, ERR_UNSUPPORTED),
        ("LayerNorm fold with scale", rep(ln, scale=0.5), {}, ERR_UNSUPPORTED),
        ("LayerNorm fold with residual", rep(ln, residual="dense"), {}, ERR_UNSUPPORTED),
        ("ln_svec alignment", ln, dict(ln_svec=(1 << 20) + 4), ERR_ALIGN),
        ("strided source with two sources", rep(base, c1=64), dict(src_img_stride=64 * 20), ERR_UNSUPPORTED),
        ("src_img_stride % c0", base, dict(src_img_stride=64 * 16 + 8), ERR_UNSUPPORTED),
        ("k_order 2", base, dict(k_order=2), ERR_ARG),
        ("chunk-major k", base, dict(k_order=1), ERR_UNSUPPORTED),
        ("split without workspace", split, dict(ws=None), ERR_UNSUPPORTED),
        ("split with groups", rep(split, groups=2), {}, ERR_UNSUPPORTED),
        ("split transposed", rep(split, out_mode="tr"), {}, ERR_UNSUPPORTED),
        ("split_k 65", rep(split, split_k=65), {}, ERR_UNSUPPORTED),
        ("workspace alignment", split, dict(ws=(1 << 20) + 8), ERR_ALIGN),
        ("defer_finish 2", split, dict(defer_finish=2), ERR_ARG),
        ("defer_finish without split", base, dict(defer_finish=1), ERR_UNSUPPORTED),
        ("defer_finish with sync", rep(split, finish="sync"), dict(defer_finish=1), ERR_UNSUPPORTED),
        ("defer_finish fp32", rep(split, out_mode="f32"), dict(defer_finish=1), ERR_UNSUPPORTED),
        ("sync alignment", rep(split, finish="sync"), dict(sync=(1 << 20) + 2), ERR_ALIGN),
    ]
    bad = []
    for name, case, fields, want in cases:
        got = _query(lib, case, **fields)
        if got != (want, want):
            bad.append(f"{name}: kernel_variant / slab_count answer {got}, expected {want}")
    assert _query(lib, base)[0] >= 0 and _query(lib, split)[1] == 2
    assert not bad, "\n".join(bad)
