"""CPU: numeric health's host side -- the ABI additions (struct ids 35, 36), `mobi_tensor_health`'s refusals (host checks: no
launch), the numpy definition on hand-written bit patterns, the report, the heavy-tailed stand-in and the two parsers."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import health_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from mobi_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_abi_additions(lib):
    from mobi_amd import _lib
    assert lib.mobi_abi_version() == 6
    assert lib.mobi_struct_size(35) == C.sizeof(_lib.HealthTensor) == 24
    assert lib.mobi_struct_size(36) == C.sizeof(_lib.HealthRecord) == 40
    assert _lib.STRUCT_IDS[35] is _lib.HealthTensor and _lib.STRUCT_IDS[36] is _lib.HealthRecord
    assert "mobi_tensor_health" in _lib.SYMBOLS and _lib.MOBI_F32 == 2
    with open(os.path.join(ROOT, "include", "mobi_engine.h")) as f:
        header = f.read()
    for word in ("int mobi_tensor_health(", "mobi_health_tensor;", "mobi_health_record;", "MOBI_F32 = 2"):
        assert word in header, word


def test_tensor_health_validates_before_any_launch(lib):
    """No GPU here: every call must return on the host."""
    from mobi_amd import _lib

    def call(n=1, x=4096, count=100, dtype=0, near=1.0, out=4096, table=True, edit=None):
        t = (_lib.HealthTensor * max(n, 1))()
        for e in t:
            e.x, e.n, e.dtype, e.near_abs = x, count, dtype, near
        if edit:
            edit(t)
        return lib.mobi_tensor_health(t if table else None, n, out, None)

    ARG, ALIGN = -1, -4
    assert call(table=False) == ARG and call(out=None) == ARG and call(x=None) == ARG
    assert call(n=0) == ARG and call(n=-1) == ARG and call(n=65) == ARG
    assert call(count=0) == ARG and call(count=-5) == ARG
    assert call(dtype=3) == ARG and call(dtype=-1) == ARG
    assert call(near=-1.0) == ARG and call(near=float("nan")) == ARG and call(near=-math.inf) == ARG
    assert call(x=4097) == ALIGN and call(x=4098, dtype=2) == ALIGN and call(x=4097, dtype=1) == ALIGN
    assert call(out=4100) == ALIGN
    # the last entry of a full table is checked like the first
    assert call(n=64, edit=lambda t: setattr(t[63], "n", 0)) == ARG
    assert call(n=64, edit=lambda t: setattr(t[63], "x", 4099)) == ALIGN


@pytest.mark.parametrize("name", ["fp16", "bf16", "fp32"])
def test_reference_on_hand_written_patterns(name):
    from mobi_amd import health
    _, _, ut = hc.LAYOUT[name]
    p = hc.patterns(name)
    near_pattern = p["max"] - 37                                   # a finite pattern: its value is the threshold
    near_abs = hc.value_of(name, near_pattern)
    lab = dict(hc.specials(name, near_pattern))
    mask = p["sign"] - 1

    def ref(labels):
        return health.tensor_health_ref(np.array([lab[k] for k in labels], dtype=ut), name, near_abs)

    zero = {"absmax_bits": 0, "absmax": 0.0, "inf": 0, "nan": 0, "near": 0, "subnormal": 0}
    assert ref(["+0", "-0"]) == zero
    assert ref(["+inf", "-inf", "+0"]) == {**zero, "inf": 2}
    assert ref(["nan_a", "nan_b"]) == {**zero, "nan": 2}           # an all-nan tensor: absmax_bits 0
    bits_of = lambda pat: int(np.array([hc.value_of(name, pat & mask)], dtype=np.float32).view(np.uint32)[0])
    r = ref(["+max", "-max", "nan_a", "+inf"])
    assert r == {"absmax_bits": bits_of(p["max"]), "absmax": hc.MAX[name], "inf": 1, "nan": 1, "near": 2, "subnormal": 0}
    r = ref(["at_near", "below_near", "-0"])
    assert r["near"] == 1 and r["absmax_bits"] == bits_of(near_pattern) and r["inf"] == r["nan"] == r["subnormal"] == 0
    r = ref(["sub_min", "sub_max", "+0", "-0"])
    assert r["subnormal"] == 2 and r["near"] == 0 and r["absmax_bits"] == bits_of(p["sub_max"]) and r["absmax"] > 0
    assert health.tensor_health_ref(np.array([p["min_normal"]], dtype=ut), name, near_abs)["subnormal"] == 0
    r = ref([k for k, _ in hc.specials(name, near_pattern)])        # all of them at once
    assert (r["inf"], r["nan"], r["near"], r["subnormal"], r["absmax"]) == (2, 2, 3, 2, hc.MAX[name])
    # a float array and a torch tensor are read by their bits
    if name != "bf16":
        arr = np.array([1.5, -2.5, np.inf, np.nan], dtype=np.float16 if name == "fp16" else np.float32)
        assert health.tensor_health_ref(arr, name, 2.0) == {"absmax_bits": bits_of(int(np.array([2.5], dtype=arr.dtype).view(ut)[0])),
                                                             "absmax": 2.5, "inf": 1, "nan": 1, "near": 1, "subnormal": 0}
    t = torch.tensor([1.5, -2.5, float("inf")], dtype=hc.TORCH[name])
    assert health.tensor_health_ref(t, t.dtype, 2.0)["absmax"] == 2.5


def _rows():
    from mobi_amd.health import Row
    rec = lambda amax, inf=0, nan=0: {"absmax": amax, "inf": inf, "nan": nan, "near": 0, "subnormal": 0}
    return [Row.from_record(0, "Net.a", "igemm", (2, 3), "fp16", rec(10.0)),
            Row.from_record(1, "Net.b", "groupnorm", (2, 3), "fp16", rec(0.0)),
            Row.from_record(2, "Net.c", "igemm", (4,), "fp16", rec(6550.4)),
            Row.from_record(3, "Net.d", "igemm", (4,), "fp16", rec(100.0, inf=2)),
            Row.from_record(4, "Net.e", "attention", (4,), "fp16", rec(1.0, nan=1)),
            Row.from_record(5, "Net.f", "sampler", (4,), "fp32", rec(2.0))]


def test_report():
    from mobi_amd.health import Report
    rep = Report(_rows(), near=0.25)
    assert [r.seq for r in rep.rows] == list(range(6))             # launch order
    assert rep.rows[0].headroom == 6550.4 and rep.rows[2].headroom == pytest.approx(10.0, rel=1e-12)
    assert rep.rows[1].headroom == math.inf                        # an all-zero tensor
    assert rep.first_nonfinite().module == "Net.d"
    assert [r.seq for r in rep.worst(3)] == [3, 4, 2] and len(rep.worst(100)) == 6
    assert Report(rep.rows[:3]).first_nonfinite() is None
    back = Report.from_json(rep.to_json())
    assert back.rows == rep.rows and back.near == 0.25
    text = str(rep)
    assert "Net.d" in text and "first non-finite: #3" in text and len(rep.summary().splitlines()) == 3


def test_probes_do_not_nest_and_leave_nothing_behind():
    from mobi_amd import health, ops
    assert ops._HEALTH is None
    with health.probe() as hp:
        assert ops._HEALTH is hp
        with pytest.raises(RuntimeError):
            with health.probe():
                pass
        assert ops._HEALTH is hp
        lin = torch.nn.Sequential(torch.nn.Linear(2, 2))
        lin(torch.zeros(1, 2))                                     # labels follow the modules called
        assert hp._stack == [] and hp._names[lin[0]] == "Sequential.0"
        with ops.health_scope("out"):
            assert hp.label() == "out"
    assert ops._HEALTH is None
    assert hp.report().rows == []
    with ops.health_scope("x") as s:                               # no probe: the shared empty scope
        assert s is ops._NO_SCOPE


def test_heavy_tailed_stand_in():
    from mobi_amd import health

    def net():
        return torch.nn.Sequential(torch.nn.Conv2d(8, 200, 3), torch.nn.GroupNorm(4, 200), torch.nn.Linear(200, 130),
                                   torch.nn.LayerNorm(130))

    a, b, c = (health.heavy_tailed_(net(), s) for s in (5, 5, 6))
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)                                  # the same seed: the same bits
    assert any(not torch.equal(pa, pc) for pa, pc in zip(a.parameters(), c.parameters()))
    assert health.outlier_channels(200, 64) == [32, 96, 160] and health.outlier_channels(130, 64) == [32, 96]
    # with sigma = 0 only the outlier channels stand out, by outlier_gain, exactly where the documentation says
    flat = health.heavy_tailed_(net(), 5, sigma=0.0, outlier_gain=1.0)
    out = health.heavy_tailed_(net(), 5, sigma=0.0, outlier_gain=30.0)
    for k in (0, 2):
        ratio = (out[k].weight / flat[k].weight).reshape(out[k].weight.shape[0], -1)
        want = torch.ones(ratio.shape[0])
        want[health.outlier_channels(ratio.shape[0], 64)] = 30.0
        assert torch.allclose(ratio, want[:, None].expand_as(ratio), rtol=1e-6, atol=0)
    for k in (1, 3):
        g = a[k].weight.detach()
        assert float(g.min()) >= 1.0 and float(g.max()) <= 10.0 and float(g.max()) > 3.0
    tight = health.heavy_tailed_(net(), 5, norm_gamma_max=2.0)
    assert float(tight[1].weight.max()) <= 2.0


def test_audit_weights_on_the_host():
    """Without a device the audit goes through the numpy definition."""
    from mobi_amd import health
    net = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2))
    with torch.no_grad():
        for p in net.parameters():
            p.fill_(0.5)
        net[1].weight[1, 2] = 1e5
    rep = health.audit_weights(net, torch.float16)
    assert [r.module for r in rep.rows] == ["0.weight", "0.bias", "1.weight", "1.bias"]
    hot = rep.rows[2]
    assert hot.near == 1 and hot.overflow == 1 and hot.headroom == pytest.approx(65504.0 / 1e5)
    assert all(r.near == r.overflow == r.inf == r.nan == 0 for r in rep.rows if r is not hot)
    bf = health.audit_weights(net, torch.bfloat16)
    assert all(r.near == r.overflow == 0 for r in bf.rows)


def test_first_batch_watch_probes_one_batch_and_restores_the_model():
    """What `python -m mobi_amd.health test_bench` puts on the loop's model: a probe from the first get_input to the end of the
    first log_data, nothing around later batches, and the model's own methods back afterwards."""
    from mobi_amd import health, ops

    class Model(torch.nn.Module):
        calls = []

        def get_input(self, batch):
            self.calls.append(("get_input", ops._HEALTH is not None))
            return batch

        def log_data(self, batch):
            self.calls.append(("log_data", ops._HEALTH is not None))
            return batch

    m = Model()
    watch = health._FirstBatch(m)
    assert ops._HEALTH is None and watch.report is None
    for b in (1, 2):
        assert m.log_data(m.get_input(b)) == b
        assert ops._HEALTH is None and watch.report is not None
    assert m.calls == [("get_input", True), ("log_data", True), ("get_input", False), ("log_data", False)]
    watch.remove()
    assert "get_input" not in m.__dict__ and "log_data" not in m.__dict__
    # a run that dies inside the first batch leaves no probe behind
    bad = health._FirstBatch(Model())
    bad.model.get_input(0)
    assert ops._HEALTH is bad.probe
    bad.remove()
    assert ops._HEALTH is None


def test_parsers():
    from mobi_amd import health
    opt = health.build_parser().parse_args(["--config", "c.yaml", "--synthetic", "heavy", "a.b=1"])
    assert (opt.synthetic, opt.dtype, opt.steps, opt.scale, opt.plms, opt.objects, opt.top, opt.json) == \
        ("heavy", "fp16", 2, 5, False, 2, 20, "")
    assert opt.overrides == ["a.b=1"]
    with pytest.raises(SystemExit):
        health.build_parser().parse_args(["--config", "c.yaml"])              # neither --ckpt nor --synthetic
    with pytest.raises(SystemExit):
        health.build_parser().parse_args(["--config", "c.yaml", "--ckpt", "k", "--synthetic", "gauss"])
