"""CPU: the attention probe's definition (`health.attention_health_ref`) on inputs whose records can be worked out by hand, the
report's JSON round trip with attention rows, the record's layout and `mobi_attention_health`'s argument checks (nothing is
launched: every call returns on the host)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

DTYPES = [torch.float16, torch.bfloat16]


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _planted(dtype, dh=8, tq=5, tk=48, late=40, amount=6.0):
    """2 images x 2 heads, all keys of a head equal, q_log2_scaled: every score is 2 * amount.  (image 1, head 0) has one key at
    index `late` >= 32 whose score is 3 * amount."""
    c = 2 * dh
    q, k = torch.zeros(2, tq, c), torch.zeros(2, tk, c)
    q[..., 0::dh] = 2.0
    k[..., 0::dh] = amount
    k[1, late, 0] = 1.5 * amount
    v = torch.arange(2 * tk * c, dtype=torch.float32).reshape(2, tk, c) % 7 - 3.0       # small integers: exact in both types
    return q.to(dtype), k.to(dtype), v.to(dtype)


def _exact_out(q, k, v, heads):
    """softmax(q k^T as exponents of two) v in fp64, rounded to the operands' type: a stand-in for the production result."""
    n, tq, c = q.shape
    dh = c // heads
    out = torch.zeros(n, tq, c, dtype=torch.float64)
    for h in range(heads):
        sl = slice(h * dh, (h + 1) * dh)
        e = q[..., sl].double() @ k[..., sl].double().transpose(1, 2)
        p = torch.exp2(e - e.amax(-1, keepdim=True))
        out[..., sl] = (p @ v[..., sl].double()) / p.sum(-1, keepdim=True)
    return out.to(q.dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_keys_equal(dtype):
    from mobi_amd import health
    q, k, v = _planted(dtype)
    k[1, 40, 0] = k[1, 0, 0]                                        # no plant
    out = _exact_out(q, k, v, 2)
    rec = health.attention_health_ref(q, k, v, out, 2, 1.0, v_rows=True, q_log2_scaled=True)
    assert rec.shape == (4,)
    assert (rec["rise_max"] == 0).all() and (rec["rows_rise_over"] == 0).all()
    assert (rec["e_max"] == 12.0).all() and (rec["e_min"] == 12.0).all()
    mean = v.double().reshape(2, 48, 2, 8).mean(1).abs().amax(-1).reshape(-1).numpy()      # uniform p: o is the mean of v
    assert np.allclose(rec["ref_absmax"], mean, rtol=0, atol=1e-12)
    assert (rec["in_nonfinite"] == 0).all() and (rec["out_nonfinite"] == 0).all()
    u = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    assert (rec["err_max"] <= u * rec["ref_absmax"]).all()          # out is the exact result rounded once
    assert (_f32(rec["q_absmax_bits"]) == 2.0).all() and (_f32(rec["k_absmax_bits"]) == 6.0).all()
    assert (_f32(rec["v_absmax_bits"]) == 3.0).all()
    # V^T is the same launch
    vt = health.attention_health_ref(q, k, v.transpose(1, 2).contiguous(), out, 2, 1.0, v_rows=False, q_log2_scaled=True)
    assert vt.tobytes() == rec.tobytes()
    # scale * log2(e) where q does not carry it
    un = health.attention_health_ref(q, k, v, out, 2, 0.5, v_rows=True, q_log2_scaled=False)
    assert np.allclose(un["e_max"], 12.0 * 0.5 * health.LOG2E, rtol=1e-15)


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_late_key(dtype):
    from mobi_amd import health
    q, k, v = _planted(dtype)
    out = _exact_out(q, k, v, 2)
    lo = health.attention_health_ref(q, k, v, out, 2, 1.0, True, True, rise_limit=5.5)
    hi = health.attention_health_ref(q, k, v, out, 2, 1.0, True, True, rise_limit=6.5)
    assert lo["rise_max"].tolist() == [0.0, 0.0, 6.0, 0.0] and hi["rise_max"].tolist() == lo["rise_max"].tolist()
    assert lo["rows_rise_over"].tolist() == [0, 0, 5, 0] and hi["rows_rise_over"].tolist() == [0, 0, 0, 0]
    assert lo["e_max"].tolist() == [12.0, 12.0, 18.0, 12.0]
    at = health.attention_health_ref(q, k, v, out, 2, 1.0, True, True, rise_limit=6.0)
    assert at["rows_rise_over"].tolist() == [0, 0, 0, 0]           # strictly over
    # the default limit is the storage type's
    assert health.attention_health_ref(q, k, v, out, 2, 1.0, True, True)["rows_rise_over"].sum() == 0
    assert health.RISE_LIMIT == {"fp16": 20.0, "bf16": 120.0}
    # p of the planted head: 47 keys at 2^-6 and one at 1
    w = np.full(48, 2.0 ** -6)
    w[40] = 1.0
    want = (w[:, None] * v[1, :, :8].double().numpy()).sum(0) / w.sum()
    assert abs(lo["ref_absmax"][2] - np.abs(want).max()) < 1e-12
    _, rises = health.attention_health_ref(q, k, v, out, 2, 1.0, True, True, rises=True)
    assert rises.shape == (4, 5) and (rises[2] == 6.0).all() and not rises[[0, 1, 3]].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_fewer_than_32_keys_never_rise(dtype):
    from mobi_amd import health
    q, k, v = _planted(dtype, tk=31, late=20)
    out = _exact_out(q, k, v, 2)
    rec = health.attention_health_ref(q, k, v, out, 2, 1.0, True, True, rise_limit=0.0)
    assert (rec["rise_max"] == 0).all() and (rec["rows_rise_over"] == 0).all() and rec["e_max"][2] == 18.0
    q, k, v = _planted(dtype, tk=33, late=32)                       # the first key that can
    rec = health.attention_health_ref(q, k, v, _exact_out(q, k, v, 2), 2, 1.0, True, True, rise_limit=0.0)
    assert rec["rise_max"].tolist() == [0.0, 0.0, 6.0, 0.0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_inf_and_nan(dtype):
    from mobi_amd import health
    q, k, v = _planted(dtype)
    out = _exact_out(q, k, v, 2)
    base = health.attention_health_ref(q, k, v, out, 2, 1.0, True, True)
    kb = k.clone()
    kb[0, 7, 8 + 3] = float("inf")                                  # image 0, head 1
    bad = health.attention_health_ref(q, kb, v, out, 2, 1.0, True, True)
    assert bad["in_nonfinite"].tolist() == [0, 1, 0, 0]
    for i in (0, 2, 3):
        assert bad[i].tobytes() == base[i].tobytes()
    for name in ("q_absmax_bits", "k_absmax_bits", "v_absmax_bits", "out_nonfinite"):
        assert bad[name][1] == base[name][1]
    ob = out.clone()
    ob[1, 3, 8 + 2] = float("nan")                                  # image 1, head 1
    rec = health.attention_health_ref(q, k, v, ob, 2, 1.0, True, True)
    assert rec["out_nonfinite"].tolist() == [0, 0, 0, 1]
    assert np.isfinite(rec["err_max"]).all() and rec["err_max"][3] <= base["err_max"][3]
    for i in (0, 1, 2):
        assert rec[i].tobytes() == base[i].tobytes()
    ob = out.clone()
    ob[0, :, :8] = float("inf")
    rec = health.attention_health_ref(q, k, v, ob, 2, 1.0, True, True)
    assert rec["err_row"][0] == -1 and rec["err_max"][0] == 0 and rec["out_nonfinite"][0] == 5 * 8
    # err_row: the smallest row that attains the maximum
    ob = out.clone().float()
    ob[1, 2, 1] += 0.5                                              # (the rows of a head are equal: the same error twice, bit for bit)
    ob[1, 4, 1] += 0.5
    rec = health.attention_health_ref(q, k, v, ob.to(dtype), 2, 1.0, True, True)
    assert rec["err_row"][2] == 2 and abs(rec["err_max"][2] - 0.5) < 0.01


def _report_with_attention():
    from mobi_amd import health, ops
    rows = [health.Row(0, "Net.a", "igemm", (2, 5, 16), "bf16", 3.0, 1e38, 0, 0, 0, 0),
            health.Row(1, "Net.a", "attention", (2, 5, 16), "bf16", 2.0, 1e38, 3, 1, 0, 0)]
    rec = np.zeros(4, dtype=ops.ATTENTION_HEALTH_DTYPE)
    rec["q_absmax_bits"] = np.array([2.0, 1.0, 4.0, 1.0], dtype=np.float32).view(np.uint32)
    rec["k_absmax_bits"] = rec["v_absmax_bits"] = rec["ref_absmax_bits"] = np.array([1.0, 8.0, 1.0, 1.0], dtype=np.float32).view(np.uint32)
    rec["out_nonfinite"] = [0, 4, 0, 0]
    rec["e_max"], rec["e_min"] = [1.0, 2.0, 9.5, -1.0], [-3.0, -2.0, -7.25, -1.0]
    rec["rise_max"], rec["rows_rise_over"] = [0.0, 130.0, 2.0, 0.0], [0, 2, 0, 0]
    rec["err_max"], rec["err_row"] = [0.25, 0.5, 0.75, 0.125], [4, 0, 3, 1]
    att = health.AttentionRow.from_records(1, "Net.a", (2, 2, 5, 40, 8), "bf16", True, 120.0, rec)
    return health.Report(rows, 0.5, [att]), rec


def test_report_round_trip_with_attention_rows():
    from mobi_amd import health
    rep, rec = _report_with_attention()
    a = rep.attention[0]
    assert (a.q_absmax, a.k_absmax, a.out_nonfinite, a.e_max, a.e_min, a.rise_max, a.rows_rise_over) == (4.0, 8.0, 4, 9.5, -7.25, 130.0, 2)
    assert (a.err_max, a.err_row, a.worst_head) == (0.75, 3, (1, 0)) and a.head(1, 0)["err_row"] == 3
    assert rep.attention_for(1) is a and rep.attention_for(0) is None
    text = rep.to_json()
    assert set(json.loads(text)) == {"near", "rows", "attention"}
    back = health.Report.from_json(text)
    assert back.rows == rep.rows and back.attention == rep.attention and back.near == rep.near
    assert back.attention[0].per_head.tobytes() == rec.tobytes()
    assert back.to_json() == text
    printed = str(rep)
    assert printed.startswith(str(health.Report(rep.rows, 0.5))) and "err_max" in printed and "(1, 0, 3)" in printed
    assert "operands non-finite" not in printed
    rec["in_nonfinite"][2] = 7
    bad = health.AttentionRow.from_records(1, "Net.a", (2, 2, 5, 40, 8), "bf16", True, 120.0, rec)
    assert "operands non-finite" in health.Report.attention_table([bad]) and "operands non-finite" in bad.worst_heads()
    assert "first attention launch with a non-finite result: #1" in health.attention_section(rep)


def test_report_without_attention_rows_serialises_as_before():
    from mobi_amd import health
    rep, _ = _report_with_attention()
    plain = health.Report(rep.rows, 0.5)
    d = json.loads(plain.to_json())
    assert set(d) == {"near", "rows"} and plain.attention == []
    assert plain.to_json() == json.dumps({"near": 0.5, "rows": d["rows"]})
    assert "err_max" not in str(plain)
    assert health.Report.from_json(plain.to_json()).attention == []
    assert health.probe().attention is False and health.probe(attention=True).attention is True
    args = health.build_parser().parse_args(["--config", "x.yaml", "--synthetic", "heavy"])
    assert args.attention is False
    assert health.build_parser().parse_args(["--config", "x.yaml", "--synthetic", "heavy", "--attention"]).attention is True


@pytest.fixture(scope="module")
def lib():
    from mobi_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_record_layout(lib):
    from mobi_amd import _lib, ops
    assert lib.mobi_struct_size(37) == C.sizeof(_lib.AttentionHealthRecord) == 48 == ops.ATTENTION_HEALTH_DTYPE.itemsize
    assert [n for n, _ in _lib.AttentionHealthRecord._fields_] == list(ops.ATTENTION_HEALTH_DTYPE.names)
    assert _lib.STRUCT_IDS[37] is _lib.AttentionHealthRecord and lib.mobi_abi_version() == 6


def test_argument_checks_match_mobi_attention(lib):
    """Every rejection comes before anything is enqueued: checkable without a GPU."""
    from mobi_amd import _lib
    OK_PTR = 4096

    def params(**kw):
        a = _lib.AttentionParams()
        a.q = a.k = a.vt = a.out = OK_PTR
        a.images = a.heads = a.tq = a.tk = 1
        a.dh, a.dtype, a.scale = 8, 0, 1.0
        a.q_row_stride = a.k_row_stride = a.vt_row_stride = a.out_row_stride = 8
        for key, v in kw.items():
            setattr(a, key, v)
        return a

    def both(a, rec=OK_PTR):
        return lib.mobi_attention_health(C.byref(a), 20.0, rec, None), lib.mobi_attention(C.byref(a), None)

    ARG, UNSUPPORTED, ALIGN = -1, -2, -4
    assert both(params(dh=12)) == (UNSUPPORTED, UNSUPPORTED)
    assert both(params(dh=168)) == (UNSUPPORTED, UNSUPPORTED)
    assert both(params(q=OK_PTR + 8)) == (ALIGN, ALIGN)
    assert both(params(k=OK_PTR + 2)) == (ALIGN, ALIGN)
    assert both(params(out=OK_PTR + 4)) == (ALIGN, ALIGN)
    assert both(params(v_layout=1, vt=OK_PTR + 8)) == (ALIGN, ALIGN)
    assert both(params(q_row_stride=12)) == (ALIGN, ALIGN)
    assert both(params(out_img_stride=2)) == (ALIGN, ALIGN)
    assert both(params(dtype=2)) == (ARG, ARG)
    assert both(params(tk=0)) == (ARG, ARG)
    assert both(params(v_layout=2)) == (ARG, ARG)
    assert both(params(q=None)) == (ARG, ARG)
    assert both(params(heads=65536)) == (UNSUPPORTED, UNSUPPORTED)
    assert lib.mobi_attention_health(None, 20.0, OK_PTR, None) == ARG
    assert lib.mobi_attention_health(C.byref(params()), 20.0, None, None) == ARG               # no record buffer
    assert lib.mobi_attention_health(C.byref(params()), 20.0, OK_PTR + 2, None) == ALIGN
    assert lib.mobi_attention_health(C.byref(params()), float("nan"), OK_PTR, None) == ARG
