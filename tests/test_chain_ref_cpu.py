"""tests/chain_ref.py (the fp64 interpreter of mobi_row_chain's contract) and the judge of tests/chain_cases.py, without a
device: the weight decoder against the packer, the interpreter on the three production programs against F.linear /
F.layer_norm / the adapter formula composed by hand, planted defects that the judge must fail, and -- for every case the
GPU tests run -- an fp32-accumulating emulation within HALF the bound the GPU test asserts (the reference alone leaves the
kernel at least the other half)."""
import pytest
import torch
import torch.nn.functional as F

from tests import chain_cases as cc, chain_ref
from tests.launch_shadow import two_key_adapter_reference

DT = [torch.float16, torch.bfloat16]
C = 320


def _dname(dtype):
    return "fp16" if dtype == torch.float16 else "bf16"


def _build(key, dtype):
    return cc.build_case(key, dtype, "cpu", chain_ref.ProgramDescription)


@pytest.mark.parametrize("dtype", DT, ids=_dname)
def test_chain_weight_decode_round_trips_the_packer(dtype):
    """decode_chain_weight restates the chunk-image layout of include/mobi_engine.h; the packer's image must decode to the
    storage-rounded matrix bit for bit, with and without a folded LayerNorm."""
    from mobi_amd import ops
    g = torch.Generator().manual_seed(3)
    w = torch.randn((C, C), generator=g) * 0.05
    w[7, 300], w[200, 13] = 1.25, -2.5                                     # two landmarks off the diagonal
    cw = ops.pack_chain_weight(w, None, dtype, "cpu")
    dec = chain_ref.decode_chain_weight(cw.image, dtype)
    assert dec.dtype == dtype and torch.equal(chain_ref.bits(dec), chain_ref.bits(w.to(dtype)))
    gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    cw = ops.pack_chain_weight(w, None, dtype, "cpu", ln=(gamma, beta), scale=0.25)
    want = (w.double() * 0.25 * gamma.double()[None, :]).float().to(dtype)
    dec = chain_ref.decode_chain_weight(cw.image, dtype)
    assert torch.equal(chain_ref.bits(dec), chain_ref.bits(want))
    assert torch.allclose(cw.svec.double(), want.double().sum(1), rtol=1e-6, atol=1e-7)
    assert torch.allclose(cw.bias.double(), 0.25 * (w.double() @ beta.double()), rtol=1e-6, atol=1e-7)


def _rounded(case, tag):
    """(W' in T as fp64, bias' fp64) of a master weight: scale W diag(gamma) rounded once, scale (W beta + b)."""
    w, b, ln, scale = case.masters[tag]
    wd = w.double() * scale
    bd = torch.zeros(C, dtype=torch.float64) if b is None else b.double() * scale
    if ln is not None:
        bd = bd + wd @ ln[1].double()
        wd = wd * ln[0].double()[None, :]
    return wd.float().to(case.dtype).double(), bd.float().double()


def _rt(v, dtype):
    return v.to(dtype).double()


def _ln_lin(case, x, tag):
    """linear(LayerNorm(x)) with the LayerNorm's affine folded into the rounded weight: what FOLD must equal."""
    w, b = _rounded(case, tag)
    return F.linear(F.layer_norm(x, (C,), None, None, cc.LN_EPS), w, b)


def _refs(case):
    res = chain_ref.run_launch(case.descs, case.images, case.rows, case.dtype, case.tables)
    return [chain_ref.as_images(r["ref"], case.rows) for r in res], res


def _close(a, b):
    return float((a - b).norm() / b.norm()) < 1e-6            # (svec and the folded bias are fp32 vectors of fp64 sums)


@pytest.mark.parametrize("dtype", DT, ids=_dname)
def test_interpreter_post_attn1_by_hand(dtype):
    case = _build("post_attn1-2x128", dtype)
    d = case.descs[0]
    a, x_in, ref_vec = d[0][1]["t"].double(), d[1][1]["t"].double(), d[2][1]["bias"].double()
    x1 = _rt(F.linear(a, _rounded(case, "to_out")[0]) + ref_vec[:, None, :] + x_in, dtype)
    tb = case.tables
    x2 = _rt(two_key_adapter_reference(x1, tb["a"], tb["a"].double().sum(-1), tb["c"], tb["u"], tb["b"], tb["eps"]), dtype)
    refs, res = _refs(case)
    assert [(r["prog"], r["code"]) for r in res] == [(0, "adapter"), (0, "product"), (1, "adapter"), (1, "product"), (1, "product"),
                                                    (1, "product")]
    assert torch.equal(refs[0], x2[0::2]) and torch.equal(refs[2], x2[1::2])
    assert _close(refs[1], _ln_lin(case, x2[0::2], "q_cam")) and _close(refs[3], _ln_lin(case, x2[1::2], "q_lid"))
    assert _close(refs[4], F.linear(x2[1::2], _rounded(case, "k_cam")[0])) and _close(refs[5], F.linear(x2[1::2], _rounded(case, "v_cam")[0]))
    assert all(r["div"] == (1 if r["code"] == "adapter" else 2) for r in res)
    assert res[3]["img"].unique().tolist() == [1] and res[1]["img"].unique().tolist() == [0]


@pytest.mark.parametrize("dtype", DT, ids=_dname)
def test_interpreter_post_cam_by_hand(dtype):
    case = _build("post_cam-2x128", dtype)
    d = case.descs[0]
    ac, xc = d[0][1]["t"].double(), d[1][1]["t"].double()
    assert xc.shape[0] == 2 and d[1][1]["t"].stride(0) == 2 * 128 * C           # the camera half of a batch of 4, in place
    wf, bf = _rounded(case, "fold_cam")
    x1 = F.linear(ac, wf, bf) + xc
    refs, _ = _refs(case)
    assert _close(refs[0], x1)
    s = _rt(x1, dtype)
    for ref, tag in ((refs[1], "k_lid"), (refs[2], "v_lid")):
        assert _close(ref, F.linear(s, _rounded(case, tag)[0]))


@pytest.mark.parametrize("dtype", DT, ids=_dname)
def test_interpreter_pre_attn1_by_hand(dtype):
    case = _build("pre_attn1-2x128", dtype)
    d = case.descs[0]
    x, scale, shift = d[0][1]["t"].double(), d[1][1]["scale"].double(), d[1][1]["shift"].double()
    s0 = _rt(x * scale[:, None, :] + shift[:, None, :], dtype)
    wp, bp = _rounded(case, "proj_in")
    t = F.linear(s0, wp, bp)
    refs, res = _refs(case)
    assert _close(refs[0], t)
    s = _rt(t, dtype)
    for ref, tag in zip(refs[1:], ("q", "k", "v")):
        assert _close(ref, _ln_lin(case, s, tag))
    # the three folded products land in the column thirds of one tensor
    assert [r["dst"].storage_offset() for r in res[1:]] == [0, C, 2 * C] and res[1]["dst"].stride(1) == 3 * C


@pytest.mark.parametrize("dtype", DT, ids=_dname)
def test_interpreter_selected_rows_equal_the_full_run(dtype):
    """sel = (image, row): the rows the shadow recomputes on the CPU are the rows of the full run."""
    case = _build("post_attn1-4x256", dtype)
    full = chain_ref.run_launch(case.descs, case.images, case.rows, dtype, case.tables)
    img, row = torch.tensor([0, 1, 1, 2, 3, 3]), torch.tensor([0, 5, 255, 128, 17, 200])
    part = chain_ref.run_launch(case.descs, case.images, case.rows, dtype, case.tables, sel=(img, row))
    assert len(part) == len(full)
    for p, f in zip(part, full):
        pos = [int(((f["img"] == i) & (f["row"] == r)).nonzero()[0]) for i, r in zip(p["img"].tolist(), p["row"].tolist())]
        assert torch.allclose(p["ref"], f["ref"][pos], rtol=1e-12, atol=1e-12)


# ---- the judge fails what a subtly wrong kernel would do -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT, ids=_dname)
def test_judge_passes_the_clean_emulation_and_fails_every_defect(dtype):
    key = "post_attn1-4x256"        # two programs, residual, per-image bias, adapter, fold, dst_img_div = 2, two tiles per image
    case = _build(key, dtype)
    assert cc.judge(case, lambda: cc.emulate(case)) == []
    for defect in cc.DEFECTS:
        case = _build(key, dtype)
        bad = cc.judge(case, lambda: cc.emulate(case, defect))
        assert bad, defect
        print(f"[{defect} {_dname(dtype)}] {bad[0]}")
    # a changed input and a launch that differs from run to run are failures of their own
    case = _build(key, dtype)
    flip = [0]

    def unstable():
        cc.emulate(case)
        flip[0] ^= 1
        case.containers[0].view(torch.int16)[1, 3, 7] ^= flip[0]         # one bit of one stored element, every other run
    assert any("second run" in m for m in cc.judge(case, unstable))
    case = _build(key, dtype)

    def touch_input():
        cc.emulate(case)
        case.descs[0][0][1]["t"].view(torch.int16)[0, 0, 0] ^= 1
    assert any(m.startswith("input changed") for m in cc.judge(case, touch_input, rerun=False))


@pytest.mark.parametrize("dtype", DT, ids=_dname)
def test_judge_sees_a_write_outside_the_destination_rows(dtype):
    """post_cam writes x[::2] in place: a row of an odd image, or a column past a destination's 320, must show."""
    case = _build("post_cam-2x128", dtype)
    x = case.containers[0]

    def odd_image():
        cc.emulate(case)
        x.view(torch.int16)[1, 0, 0] ^= 1
    assert any("outside the destination rows" in m for m in cc.judge(case, odd_image, rerun=False))
    case = _build("post_cam-2x128", dtype)
    assert cc.judge(case, lambda: cc.emulate(case)) == []


# ---- reference-alone margin: every GPU case, fp32 sums, within half the asserted bound ---------------------------------------------
@pytest.mark.parametrize("dtype", DT, ids=_dname)
@pytest.mark.parametrize("key", list(cc.CASES))
def test_reference_alone_margin(key, dtype):
    case = _build(key, dtype)
    worst = []
    bad = cc.judge(case, lambda: cc.emulate(case), bound_scale=0.5, rerun=False,
                   report=lambda name, rel, tile, bound: worst.append((rel / bound, tile / (4 * bound), name)))
    print(f"[margin {key} {_dname(dtype)}] worst rel / half bound {max(w[0] for w in worst):.2f}, tile {max(w[1] for w in worst):.2f}")
    assert not bad, "\n".join(bad)
