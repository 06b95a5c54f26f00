"""tests/igemm_ref.py on the CPU: the float64 reference against torch's own convolution / linear / LayerNorm, the restatement
against the criteria of tests/test_gpu_igemm_rows.py, planted faults against the criterion that has to reject each, the input
conditions of every GPU case, the launch plan against the library's own answer (a query: nothing is launched) and the
coverage of the case list."""
import ctypes as C
import dataclasses
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from tests import igemm_cases as IC
from tests import igemm_ref as R
from tests.igemm_ref import Case

DT = [torch.float16, torch.bfloat16]
C3 = dict(kh=3, kw=3, pad_h=1, pad_w=1)


@functools.lru_cache(maxsize=None)
def sides(case, dtype):
    o = R.used(case, R.host_operands(case, dtype))
    return o, R.reference(case, o), R.restated(case, o, dtype)


# ----------------------------------------------------------------------------------------------------------------------
# the reference is the contract
def _conv(case, o):
    """float64 F.conv2d composition of the gather: nearest x2 upsampling, top / left padding, zeros past the bottom / right
    edge (F.pad by what the last window reaches), stride, explicit output size."""
    x = o["x"] if o["x2"] is None else torch.cat([o["x"], o["x2"]], dim=3)
    x = x.double().permute(0, 3, 1, 2)
    if case.upsample:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    hl, wl = case.logical
    bottom = max(0, (case.ho - 1) * case.stride - case.pad_h + case.kh - hl)
    right = max(0, (case.wo - 1) * case.stride - case.pad_w + case.kw - wl)
    x = F.pad(x, (case.pad_w, right, case.pad_h, bottom))
    outs = []
    per = case.n // case.groups
    for g in range(case.groups):
        w = o["w"][g].double().reshape(case.n_packed, case.kh, case.kw, case.C).permute(0, 3, 1, 2)
        y = F.conv2d(x[g * per:(g + 1) * per], w, stride=case.stride)[:, :, :case.ho, :case.wo]
        outs.append(y.permute(0, 2, 3, 1).reshape(per, case.hw, case.n_packed))
    return torch.cat(outs)


GATHERS = [
    Case(2, 5, 7, 32, 24),
    Case(2, 5, 7, 32, 24, **C3),
    Case(2, 9, 7, 32, 24, stride=2, **C3),
    Case(2, 8, 6, 32, 24, kh=3, kw=3, stride=2, hout=4, wout=3),
    Case(2, 5, 3, 32, 24, upsample=True, **C3),
    Case(2, 1, 11, 32, 24, kh=1, kw=5, pad_w=2),
    Case(3, 1, 1, 32, 24, **C3),
    Case(3, 2, 2, 32, 24, **C3),
    Case(2, 1, 9, 32, 24, **C3),
    Case(2, 9, 1, 32, 24, **C3),
    Case(2, 5, 7, 96, 24, c1=32, **C3),
    Case(4, 3, 3, 32, 24, groups=2, **C3),
    Case(3, 3, 3, 32, 24, groups=3),
]


@pytest.mark.parametrize("case", GATHERS, ids=lambda c: f"{c.kh}x{c.kw}s{c.stride}p{c.pad_h}{c.pad_w}u{int(c.upsample)}_{c.hin}x{c.win}_g{c.groups}c{c.c1}")
def test_reference_gather_equals_conv2d(case):
    o = R.used(dataclasses.replace(case, bias=False), R.host_operands(case, torch.float16))
    assert R.rel_l2(R.product(case, o), _conv(case, o)) < 1e-12
    full = dataclasses.replace(case, rowvec=True, residual="dense", scale=0.5)
    o = R.used(full, R.host_operands(full, torch.float16))
    want = _conv(full, o) * 0.5 + o["bias"].double() + o["rowvec"].double()[:, None] + o["res"].double()
    assert R.rel_l2(R.reference(full, o), want) < 1e-12
    tr = dataclasses.replace(case, out_mode="tr")
    o = R.used(tr, R.host_operands(tr, torch.float16))
    assert R.rel_l2(R.reference(tr, o), (_conv(tr, o) + o["bias"].double()).transpose(1, 2)) < 1e-12


def test_reference_epilogues_equal_torch():
    leaky = Case(2, 4, 5, 64, 24, epilogue="leaky", rowvec=True, residual="dense", **C3)
    o = R.used(leaky, R.host_operands(leaky, torch.bfloat16))
    want = F.leaky_relu(_conv(leaky, o) + o["bias"].double() + o["rowvec"].double()[:, None], 0.1) + o["res"].double()
    assert R.rel_l2(R.reference(leaky, o), want) < 1e-12
    # GEGLU: unpack ops.pack_geglu's order (per 16 rows: 8 value rows, the 8 gate rows of the same outputs), F.linear, chunk
    g = Case(2, 1, 9, 64, 24, epilogue="geglu")
    o = R.used(g, R.host_operands(g, torch.float16))
    wp = o["w"][0].double().reshape(3, 2, 8, 64)
    bp = o["bias"].double().reshape(3, 2, 8)
    w = torch.cat([wp[:, 0].reshape(24, 64), wp[:, 1].reshape(24, 64)])
    b = torch.cat([bp[:, 0].reshape(24), bp[:, 1].reshape(24)])
    val, gate = F.linear(o["x"].double().reshape(2, 9, 64), w, b).chunk(2, dim=-1)
    assert R.rel_l2(R.reference(g, o), val * F.gelu(gate)) < 1e-12
    # the LayerNorm fold with exact row sums: Linear(LayerNorm(x)) of the folded matrix
    ln = Case(2, 1, 9, 64, 24, ln=True)
    o = R.used(ln, R.host_operands(ln, torch.float16))
    o = dict(o, svec=o["w"][0].double().sum(1))
    x = o["x"].double().reshape(2, 9, 64)
    want = F.linear(F.layer_norm(x, (64,), eps=R.LN_EPS), o["w"][0].double(), o["bias"].double())
    assert R.rel_l2(R.reference(ln, o), want) < 1e-12
    lg = Case(2, 1, 9, 64, 24, ln=True, epilogue="geglu")
    o = R.used(lg, R.host_operands(lg, torch.float16))
    o = dict(o, svec=o["w"][0].double().sum(1))
    val, gate = R.geglu_pairs(F.linear(F.layer_norm(o["x"].double().reshape(2, 9, 64), (64,), eps=R.LN_EPS), o["w"][0].double(),
                                       o["bias"].double()))
    assert R.rel_l2(R.reference(lg, o), val * F.gelu(gate)) < 1e-12


def test_split_ranges_and_slabs():
    case = Case(2, 4, 4, 64, 24, split_k=4, **C3)                  # 576 = 9 tiles of 64: 3 per range, three slabs
    assert R.split_ranges(case, 4) == [(0, 192), (192, 384), (384, 576)]
    assert R.split_ranges(dataclasses.replace(case, kh=1, kw=5, pad_h=0, pad_w=2, c0=128), 4) == \
        [(0, 192), (192, 384), (384, 576), (576, 640)]
    o = R.used(case, R.host_operands(case, torch.float16))
    assert R.rel_l2(R.slab_products(case, o, 4, torch.float64).sum(0), R.product(case, o)) < 1e-12


# ----------------------------------------------------------------------------------------------------------------------
# the restatement passes every criterion, with ratio 1 by construction
@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_restated_passes_every_criterion(dtype):
    bad = []
    for cid, key, knobs, case in IC.CASES:
        o, ref, rest = sides(case, dtype)
        fig, fails = R.judge(case, dtype, rest, ref, rest, o)
        bad += [f"{cid}: {m}" for m in fails.values()]
        for k in ("row", "channel"):
            assert k not in fig or fig[k] == fig[k + ".restated"]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_f32_restatement_is_far_inside_the_a_priori_bound(dtype):
    """fp32 outputs of 16-bit operands: products exact, sums fp32 -- the restatement stays below a tenth of (k + 8) u A."""
    for case in (Case(3, 1, 43, 64, 136, out_mode="f32", rowvec=True, residual="dense"),
                 Case(8, 4, 4, 64, 160, out_mode="f32", **C3), Case(8, 4, 4, 64, 128, out_mode="f32", split_k=2, **C3)):
        o, ref, rest = sides(case, dtype)
        fig, fails = R.judge(case, dtype, rest, ref, rest, o)
        assert not fails and fig["f32"] < 0.1, (case, fig)


# ----------------------------------------------------------------------------------------------------------------------
# planted faults: each is rejected by the criterion named
def _rejects(case, dtype, faulty, criterion, o=None):
    o0, ref, rest = sides(case, dtype)
    fig, fails = R.judge(case, dtype, faulty, ref, rest, o or o0)
    assert criterion in fails, (criterion, fig, fails)
    return fig


BIG = Case(6, 10, 10, 160, 320, rowvec=True, residual="dense", **C3)          # M = 600, N = 320, K = 1440


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_planted_row_faults(dtype):
    o, ref, rest = sides(BIG, dtype)
    # one pixel row replaced by its neighbour
    f = rest.clone()
    f[2, 37] = rest[2, 38]
    _rejects(BIG, dtype, f, "row")
    # the last k-step (32 of 1440) dropped for one 16-row block
    rows = slice(48, 64)

    def drop(acc):
        a = R.im2col(BIG, o["x"], o["x2"], torch.float32)[1, rows, -32:]
        acc = acc.clone()
        acc[1, rows] -= a @ o["w"][0].float()[:, -32:].T
        return acc
    _rejects(BIG, dtype, R.restated(BIG, o, dtype, acc_hook=drop), "row")
    # the padding tap of the first / last image column reads the neighbouring pixel instead of zero
    edge = (torch.arange(BIG.hw) % BIG.wo == 0) | (torch.arange(BIG.hw) % BIG.wo == BIG.wo - 1)

    def clamp(acc):
        acc = acc.clone()
        acc[:, edge] = R.product(BIG, o, torch.float32, clamp=True)[:, edge]
        return acc
    _rejects(BIG, dtype, R.restated(BIG, o, dtype, acc_hook=clamp), "row")
    # the residual of image i taken from image i - 1
    _rejects(BIG, dtype, R.restated(BIG, dict(o, res=o["res"].roll(1, 0)), dtype), "row")


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_planted_unwritten_ragged_row(dtype):
    case = Case(1, 1, 129, 64, 136)                                 # one row in the second 128-pixel tile
    o, ref, rest = sides(case, dtype)
    f = rest.clone()
    f[0, 128] = float("nan")
    fig = _rejects(case, dtype, f, "finite")
    assert set(R.judge(case, dtype, f, ref, rest, o)[1]) >= {"finite", "row"}, fig      # and the row stays wrong once zeroed


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_planted_channel_faults(dtype):
    o, ref, rest = sides(BIG, dtype)
    # one channel's bias taken from channel + 8
    b = o["bias"].clone()
    b[40] = o["bias"][48]
    fig = _rejects(BIG, dtype, R.restated(BIG, dict(o, bias=b), dtype), "channel")
    if dtype == torch.bfloat16:         # the point of the channel measure: the whole-tensor figure lets this one through
        assert fig["rel"] < R.tolerance(BIG, dtype), fig
    # GEGLU gate / value swapped within one 16-column tile
    g = Case(3, 1, 43, 96, 72, epilogue="geglu")
    og = sides(g, dtype)[0]

    def swap(acc):
        acc = acc.clone()
        acc[..., 32:40], acc[..., 40:48] = acc[..., 40:48].clone(), acc[..., 32:40].clone()
        return acc
    _rejects(g, dtype, R.restated(g, og, dtype, acc_hook=swap), "channel")
    # transposed output: pixel and channel offsets of one 16 x 16 tile exchanged
    t = Case(3, 1, 43, 96, 129, out_mode="tr")
    rt = sides(t, dtype)[2]
    f = rt.clone()
    f[1, 0:16, 16:32], f[1, 16:32, 0:16] = rt[1, 16:32, 0:16], rt[1, 0:16, 16:32]
    _rejects(t, dtype, f, "channel")
    _rejects(t, dtype, f, "row")


@pytest.mark.parametrize("dtype", DT, ids=R.storage_name)
def test_planted_epilogue_order_and_group_faults(dtype):
    # rowvec of group 1 taken from group 0
    g = Case(4, 1, 43, 96, 136, groups=2, w_gap=64, rowvec=True)
    o = sides(g, dtype)[0]
    rv = o["rowvec"].clone()
    rv[2:] = o["rowvec"][:2]
    _rejects(g, dtype, R.restated(g, dict(o, rowvec=rv), dtype), "row")
    # leaky slope applied after the residual
    lk = Case(3, 1, 43, 96, 136, epilogue="leaky", residual="strided")
    o = sides(lk, dtype)[0]
    _rejects(lk, dtype, R.restated(lk, o, dtype, leaky_after_residual=True), "row")
    assert R.rel_l2(R.reference(lk, o, leaky_after_residual=True), R.reference(lk, o)) > 10 * R.tolerance(lk, dtype)


def test_fp32_bound_rejects_a_rounded_intermediate():
    """An fp32 output whose sum went through bf16 once is far outside (k + 8) u A, and inside the old 2e-3 rel-L2 bound."""
    case = Case(3, 1, 43, 64, 136, out_mode="f32", rowvec=True, residual="dense")
    o, ref, rest = sides(case, torch.bfloat16)
    f = rest.to(torch.bfloat16).float()
    fig, fails = R.judge(case, torch.bfloat16, f, ref, rest, o)
    assert "f32" in fails and "rel" not in fails and fig["rel"] < 2e-3, fig


# ----------------------------------------------------------------------------------------------------------------------
# the GPU cases: sensitive data, the body the case list names, complete coverage
@pytest.mark.parametrize("key", sorted(IC.BODIES))
def test_input_conditions_of_every_gpu_case(key):
    bad = []
    for cid, k, knobs, case in IC.CASES:
        if k == key:
            for dtype in DT:
                o, ref, rest = sides(case, dtype)
                bad += [f"{cid} {R.storage_name(dtype)}: {m}" for m in R.input_conditions(case, dtype, o, ref, rest)]
    assert not bad, "\n".join(bad)


def test_plan_names_the_body_the_library_reports(monkeypatch):
    """igemm_ref.plan against mobi_igemm_kernel_variant / mobi_igemm_slab_count under each case's knobs.  The queries launch
    nothing and take any non-NULL aligned addresses; without a device the library counts 256 compute units, the MI355X's."""
    from mobi_amd import _lib
    lib = _lib.load()
    bad = []
    try:
        for cid, key, knobs, case in IC.CASES:
            for name in [k for k in os.environ if k.startswith("MOBI_IGEMM_")]:
                monkeypatch.delenv(name)
            for k, v in knobs.items():
                monkeypatch.setenv("MOBI_IGEMM_" + k, str(v))
            lib.mobi_tuning_reload()
            for finish in ("", "sync") if case.split_k > 1 else ("",):
                c = dataclasses.replace(case, finish=finish)
                p = R.fill_params(_lib.IgemmParams(), c, torch.float16, R.fake_pointers(c))
                body, slabs = lib.mobi_igemm_kernel_variant(C.byref(p)), lib.mobi_igemm_slab_count(C.byref(p))
                want = R.plan(c, knobs)
                if body != want["body"] or body not in IC.EXPECTED_BODY[key] or slabs != (1 if want["small"] else want["splits"]):
                    bad.append(f"{cid}: library body {body} slabs {slabs}, plan {want['body_name']} slabs {want['splits']}")
    finally:
        monkeypatch.undo()
        lib.mobi_tuning_reload()
    assert not bad, "\n".join(bad)


def test_case_list_covers_every_instantiation_and_axis_value():
    assert not IC.missing(), "\n".join(IC.missing())
    # and the check bites: without the transposed cases the list is incomplete
    assert IC.missing([c for c in IC.CASES if c[3].out_mode != "tr"])
    # without the cases whose tile count is a multiple of 8, no launch takes the default in-launch finish (mode 2)
    lost = IC.missing([c for c in IC.CASES if "sync8" not in c[0]])
    assert any("mode 2" in m for m in lost) and not any("mode 1" in m for m in lost), lost
    assert any("64+64" in m for m in IC.missing([c for c in IC.CASES if not c[0].endswith("two.64.64")]))
