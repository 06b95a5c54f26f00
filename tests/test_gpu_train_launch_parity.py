"""Every launch of the training step against fp64, where it runs (`-m gpu`).

One `train.loss_and_gradients` call -- forward with a tape, `mobi_loss_grad`, the backward pass to all 432 adapter tensors and,
in fp16, the `lincomb4` unscale pass -- under the launch shadow (tests/launch_shadow.py) with TRAIN_KINDS and the extra kinds the
step uses: every launch is compared with the float64 restatement of its contract on the operands that launch read, within the
bound of its own unit test (TOL1, TOL_SUM, TOL_DGAMMA, REL, the igemm / linear_f32 / lincomb4 bounds of the forward shadow), its
worst tile within 4x that, finite, inputs untouched, nothing written outside an output view.  The census of library calls must
find no launch the shadow did not judge.  Two configurations, the smallest at which each path exists, each in fp16 (loss scale
`train.static_loss_scale`) and bf16 (1.0):
  * reduced_2pairs   the reduced UNet of test_unet_training_step_gradients_vs_autograd (model_channels 64) on n = 4, side 16: two
                     camera / lidar pairs, so every `x3[::2]` / `x4[::2]` / `dx3[1::2]` view has two images behind a doubled image
                     stride; levels of 1,024 / 256 / 64 / 16 token rows;
  * full_width_1pair the production net (tests/test_gpu_production.py::_full_width_net) on n = 2, side 16: the K = 23,040 split-k
                     data gradients, 1,280 channels, dh 40 / 80 / 160 attention backward, the 8-row level whose weight gradients
                     run on mobi_linear_f32.
A third case runs the 3-D box embedder's forward and backward on 4 boxes.  Side 64 (T = 4,096 attention backward, the 64 x 64
GroupNorm backward) stays with tests/test_gpu_backward_geometry.py, kernel by kernel: a shadowed step there would take minutes.
The optimizer's launches (grad_stats, adamw_multi, accum_multi, ema_multi) are outside the shadowed region: they have fp64 tests
of their own.  A routing change that removes one of the forms REQUIRED lists must edit that list explicitly.
"""
import collections
import functools
import os
import time

import pytest
import torch

from oracle import unet as ounet, weights as W
from tests.launch_shadow import TRAIN_KINDS, LaunchShadow

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
CONFIGS = ("reduced_2pairs", "full_width_1pair")
STEP_EXTRA = TRAIN_KINDS + ("skinny_linear", "linear_f32", "add")
JUDGED_EVERY_RUN = ("attention_bwd", "layernorm_bwd", "groupnorm_bwd", "geglu_bwd", "colsum", "transpose", "sumpool2", "loss_grad")
# Launches pinned by name ("<kind> #<ordinal among its kind> <output>") at TWICE the figure the storage restatement
# (backward_ref.attention_bwd_restated, matrix-core route: P and dS rounded to fp16 before their products) shows against the same
# float64 reference on the same operands -- never at the kernel's own figure.  A finding about `train.static_loss_scale`: at
# n = 2, side 16 it is 512, and in the lidar cross-modal attention of output blocks 11 / 10 / 9 (320 channels, dh 40, 256 keys
# whose common component is 4 - 5 x their spread) dS = P (dP - D) scale lies largely below fp16's smallest normal 6.1e-5; its
# rounding costs dq 1.6e-3 / 1.5e-3 / 2.7e-3 against TOL1 x 1.5 = 1.2e-3 (kernel and restatement agree to three digits).  The
# same restatement on dout x 256 -- dS back in the normal range -- shows 4.1e-4 / 3.4e-4 / 4.1e-4; the fp32 vector route 2.1e-4.
# dk, dv and every other launch of the step hold their unit tests' bounds; bf16 has fp32's range and no exception.
#   (configuration, dtype) -> {name: the restatement's rel-L2 on these operands, measured on the MI355X}
PINNED = {("full_width_1pair", torch.float16): {"attention_bwd #1 dq": 1.599e-3, "attention_bwd #5 dq": 1.498e-3,
                                                "attention_bwd #9 dq": 2.738e-3}}


def _dname(dtype):
    return "fp16" if dtype == torch.float16 else "bf16"


def _case(name):
    """(net, x, t, ctx, noise) on the device, the engine's storage type already set."""
    from tests.test_gpu_models import _unet
    from tests.test_gpu_production import _full_width_net
    if name == "reduced_2pairs":
        cfg = ounet.UNetConfig(model_channels=64)
        net = _unet(cfg, 16)
        net.load_state_dict(W.synth_state_dict(ounet.unet_param_shapes(cfg), 9))
        net, n, pre, t = net.cuda(), 4, "bw.unet", [741, 741, 21, 21]
    else:
        net, n, pre, t = _full_width_net(), 2, "bw.full16", [741, 741]
    x, ctx, noise = W.synth_input(pre + ".x", (n, 9, 16, 16)), W.synth_input(pre + ".ctx", (n, 2, 768)), W.synth_input(pre + ".noise", (n, 4, 16, 16))
    return net, x.cuda(), torch.tensor(t, dtype=torch.long).cuda(), ctx.cuda(), noise.cuda()


def _result(sh, sink, seconds, extra=None):
    return dict(failures=list(sh.failures), census=sh.census_failures(), counts=dict(sh.counts), calls=dict(sh.calls),
                kinds=dict(collections.Counter(r[0] for r in sink)), records=list(sh.records), seconds=seconds, **(extra or {}))


@functools.lru_cache(maxsize=None)
def _step(name, dtype):
    import mobi_amd
    from mobi_amd import ops, train
    mobi_amd.set_engine_dtype(dtype)
    net, x, t, ctx, noise = _case(name)
    scale = train.static_loss_scale(noise.numel()) if dtype == torch.float16 else 1.0
    sink = []
    t0 = time.time()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "_PROFILE", sink)
        pinned = {k: 2.0 * restated for k, restated in PINNED.get((name, dtype), {}).items()}
        with LaunchShadow(mp, label=f"{name} {_dname(dtype)}", extra=STEP_EXTRA, pinned=pinned) as sh:
            loss, grads = train.loss_and_gradients(net, x, t, ctx, noise, loss_scale=scale, unscale=True)
        torch.cuda.synchronize()
    seconds = time.time() - t0
    print(f"[train parity] {name} {_dname(dtype)}: {sum(sh.counts.values())} launches judged in {seconds:.1f} s (loss scale {scale:g})")
    finite = bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads.values())
    return _result(sh, sink, seconds, dict(tensors=len(grads), finite=finite, scale=scale))


@pytest.mark.parametrize("dtype", DT, ids=_dname)
@pytest.mark.parametrize("name", CONFIGS)
def test_training_step_launch_shadow(name, dtype):
    r = _step(name, dtype)
    assert not r["failures"], "\n".join(r["failures"][:40])
    assert not r["census"], "\n".join(r["census"])
    for kind, count in r["kinds"].items():
        assert r["counts"].get(kind, 0) == count, (kind, count, r["counts"])
    for kind in JUDGED_EVERY_RUN + ("igemm", "linear_f32", "add", "timestep_embedding", "geglu_fwd"):
        assert r["counts"].get(kind, 0) > 0, (kind, r["counts"])
    assert (r["counts"].get("lincomb4", 0) >= 433) == (dtype == torch.float16), r["counts"].get("lincomb4", 0)      # the unscale pass
    assert r["tensors"] == 433 and r["finite"]                                  # 432 adapter tensors and __dcontext__
    assert {rec["extra"] for rec in r["records"] if rec["kind"] == "attention_bwd"} == {"dq", "dk", "dv"}


def test_box_embedder_launch_shadow():
    """`bbox_embedder_forward` + `bbox_embedder_backward` on 4 boxes: four skinny_linear chains, eleven linear_f32 launches, two
    silu_bwd_f32."""
    import mobi_amd
    from mobi_amd import ops, train
    from mobi_amd.ldm.modules.encoders.modules import BBoxEmbedder
    mobi_amd.set_engine_dtype(torch.float16)
    emb = BBoxEmbedder()
    W.fill_module_(emb, seed=61)
    emb = emb.cuda()
    bbox = (W.synth_input("bw.bbox4", (4, 8, 3), kind="uniform") * 0.5 + 0.5).cuda()
    dtok = W.synth_input("bw.dtok4", (4, 1, 768)).cuda()
    sink = []
    t0 = time.time()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "_PROFILE", sink)
        with LaunchShadow(mp, verbose=True, label="bbox_embedder", extra=TRAIN_KINDS + ("skinny_linear", "linear_f32")) as sh:
            tok, tape = train.bbox_embedder_forward(emb, bbox)
            grads = train.bbox_embedder_backward(emb, tape, dtok)
        torch.cuda.synchronize()
    r = _result(sh, sink, time.time() - t0)
    print(f"[train parity] bbox_embedder: {sum(r['counts'].values())} launches judged in {r['seconds']:.1f} s")
    assert not r["failures"], "\n".join(r["failures"])
    assert not r["census"], "\n".join(r["census"])
    for kind, count in r["kinds"].items():
        assert r["counts"].get(kind, 0) == count, (kind, count, r["counts"])
    assert r["counts"] == {"skinny_linear": 4, "linear_f32": 11, "silu_bwd_f32": 2}, r["counts"]
    assert len(grads) == 8 and tok.shape == (4, 1, 768)


def _igemms(recs, **want):
    return [rec for rec in recs if rec["kind"] == "igemm" and all(rec["form"].get(k) == v for k, v in want.items())]


# what the step must reach somewhere across the runs (name -> predicate over one run's records)
REQUIRED = {
    "weight gradient on the matrix cores (igemm, OUT_ROWS_F32, k = token rows)": lambda name, recs, ops: _igemms(recs, out_mode=ops.OUT_ROWS_F32),
    "weight gradient on linear_f32 (8 token rows)": lambda name, recs, ops: name == "full_width_1pair" and [
        r for r in recs if r["kind"] == "linear_f32" and r["form"]["k"] == 8],
    "context-token weight gradient on linear_f32": lambda name, recs, ops: [
        r for r in recs if r["kind"] == "linear_f32" and r["form"]["n"] == 768 and r["form"]["k"] in (4, 8)],
    "split-k data gradient with K >= 23,040": lambda name, recs, ops: [
        r for r in _igemms(recs) if r["form"]["split"] > 1 and r["form"]["k"] >= 23040],
    "igemm on a strided source of two images": lambda name, recs, ops: name == "reduced_2pairs" and [
        r for r in _igemms(recs, src_strided=True) if r["form"]["images"] >= 2],
    "igemm into a strided output": lambda name, recs, ops: name == "reduced_2pairs" and _igemms(recs, out_strided=True),
    "igemm with a strided residual": lambda name, recs, ops: name == "reduced_2pairs" and _igemms(recs, res_strided=True),
    "stride-1 data gradient on a zero-spread input": lambda name, recs, ops: _igemms(recs, zero_spread=True, kh=3, stride=1),
    "the thin 32-channel head pack": lambda name, recs, ops: _igemms(recs, thin=1, cin=32, kh=3),
    "layernorm_bwd on a strided view of two images": lambda name, recs, ops: name == "reduced_2pairs" and [
        r for r in recs if r["kind"] == "layernorm_bwd" and r["form"]["x_strided"] and r["form"]["images"] >= 2],
    "attention_bwd with two context keys": lambda name, recs, ops: [r for r in recs if r["kind"] == "attention_bwd" and r["form"]["tk"] == 2],
    "attention_bwd at dh 40, 80 and 160 on the matrix cores": lambda name, recs, ops: name == "full_width_1pair" and {40, 80, 160} <= {
        r["form"]["dh"] for r in recs if r["kind"] == "attention_bwd" and r["form"]["route"] == "mfma"},
}


def _family(rec):
    fam = rec["kind"]
    if rec["kind"] == "igemm":
        f = rec["form"]
        fam += " wgrad (fp32 rows)" if f["out_mode"] == 2 else (" 3x3" if f["kh"] == 3 else " 1x1")
        fam += " split-k" if f["split"] > 1 else ""
    elif rec["kind"] == "attention_bwd":
        fam += f" {rec['extra']} {rec['form']['route']}" + (f" (pinned #{rec['pinned'].split('#')[1].split()[0]})" if rec.get("pinned") else "")
    elif rec["extra"] in ("dx", "dgamma", "dbeta", "per_sample", "terms", "dy (storage ulp)", "dy"):
        fam += " " + rec["extra"]
    return fam


def test_training_step_shadow_covers_the_paths():
    """Across the four runs every path of REQUIRED was judged at least once; prints launches, worst rel-L2, worst tile and bound
    per configuration, dtype and launch family (MOBI_TRAIN_PARITY_TABLE=<file> writes the table: profiles/train_launch_parity.txt)."""
    from mobi_amd import ops
    assert ops.OUT_ROWS_F32 == 2
    runs = {(name, dtype): _step(name, dtype) for name in CONFIGS for dtype in DT}
    for what, pred in REQUIRED.items():
        assert any(pred(name, r["records"], ops) for (name, _), r in runs.items()), what
    worst = {}
    for (name, dtype), r in runs.items():
        for rec in r["records"]:
            w = worst.setdefault((name, _dname(dtype), _family(rec)), [0.0, 0.0, 0, rec["bound"]])
            w[0], w[1], w[2], w[3] = max(w[0], rec["rel"]), max(w[1], rec["tile"]), w[2] + 1, max(w[3], rec["bound"])
    lines = [f"{'configuration':17s} {'dtype':5s} {'launch family':34s} {'judged':>6s} {'worst rel-L2':>12s} {'worst tile':>10s} {'bound':>7s}"]
    for (name, dn, fam), (rel, tile, cnt, bound) in sorted(worst.items()):
        lines.append(f"{name:17s} {dn:5s} {fam:34s} {cnt:6d} {rel:12.3e} {tile:10.3e} {bound:7.1e}")
    for (name, dtype), r in runs.items():
        lines.append(f"# {name} {_dname(dtype)}: {sum(r['counts'].values())} launches judged in {r['seconds']:.1f} s, loss scale {r['scale']:g}")
    for (name, dtype), r in runs.items():
        for rec in r["records"]:
            if rec.get("pinned"):
                now = rec["form"]["restated"][rec["extra"]]
                lines.append(f"# pinned by name: {name} {_dname(dtype)} {rec['pinned']}: kernel {rec['rel']:.3e}, storage restatement "
                             f"{now:.3e} on the same operands, bound {rec['bound']:.3e} = 2 x {PINNED[(name, dtype)][rec['pinned']]:.3e}")
                assert abs(now - PINNED[(name, dtype)][rec["pinned"]]) <= 0.02 * now, (rec["pinned"], now)      # the written figure is this run's
    print("\n".join(lines))
    path = os.environ.get("MOBI_TRAIN_PARITY_TABLE")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
