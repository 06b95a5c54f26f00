#!/usr/bin/env python3
"""Time the numeric health launch and the probe -- informational.

    python tools/health_bench.py [--config configs/mobi_nusc_512.yaml] [--reps 10] [--rounds 3] [--batch 16] [--out profiles/tensor_health.txt]

(a) `mobi_tensor_health` over the 432 trained fp32 tensors of the full-width UNet (fresh allocations filled with noise; 7 launches of
up to 64 tensors) against the bar, `mobi_snapshot_multi` without destinations over the same list (the existing read-only walker:
the same bytes, one launch), and over fp16 tensors of the same byte total (two halves per fp32 tensor).  Device events, median of
`--reps` after two warm-up launches, `--rounds` rounds with the sides alternating in one process.  Three forms, because a call
of `ops.tensor_health` also fills a 64-entry host table in Python per launch: "call" = `ops.tensor_health` as a user calls it;
"prebuilt" = the C function on tables and a record buffer made outside the timed window (what the device and the two commands per
launch cost); "one launch" = ONE launch over the 64 largest tensors, prebuilt, against the bar over the same 64 (the kernel's rate
with the launch count taken out).
(b) One UNet forward of the config at `--batch` images, N(0, 1 / fan_in) weights, fp16: eager without the probe, eager with it,
and the number of rows.  The captured-graph step is not measured here (bench.py measures it)."""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import mobi_amd  # noqa: E402
from mobi_amd import health, ops, train  # noqa: E402
from tools.ema_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(HERE, "configs", "mobi_nusc_512.yaml"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mobi_amd.ldm.util import instantiate_from_config, load_config
    ucfg = load_config(a.config, ["model.params.lidar_stage_config.params.ckpt_path=null"])["model"]["params"]["unet_config"]
    with torch.device("meta"):
        meta = instantiate_from_config(ucfg)
    numels = [p.numel() for k, p in sorted(meta.named_parameters()) if any(m in k for m in train.TRAINABLE_MARKERS)]
    src = [torch.randn(n, device="cuda") for n in numels]
    half = [torch.randn(n, device="cuda").half() for n in numels for _ in range(2)]
    n = sum(numels)
    stats = ops.MultiTensorTable([src, [None] * len(src)])
    lines = [f"{torch.cuda.get_device_name(0)}; device events, median (min .. max) of {a.reps}",
             f"-- (a) trained tensors: {len(src)} fp32 tensors, {n / 1e6:.1f} M elements, {n * 4 / 1e6:.0f} MB; "
             f"the same bytes as {len(half)} fp16 tensors"]
    print("\n".join(lines), flush=True)

    def row(what, fn, nbytes=n * 4):
        med, lo, hi = timed(fn, a.reps)
        lines.append(f"{what:<62s} {med:8.3f} ms ({lo:.3f} .. {hi:.3f})  -> {nbytes / med / 1e9:.2f} TB/s")
        print(lines[-1], flush=True)

    def prebuilt(tensors):
        """The launches of `ops.tensor_health(tensors)` with everything the host prepares made here, outside the timed window."""
        import ctypes as C
        from mobi_amd import _lib
        lib = _lib.load()
        rec = torch.empty((len(tensors), 5), dtype=torch.int64, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        calls = []
        for lo in range(0, len(tensors), _lib.HEALTH_MAX_TENSORS):
            part = tensors[lo:lo + _lib.HEALTH_MAX_TENSORS]
            table = (_lib.HealthTensor * len(part))()
            for e, t in zip(table, part):
                e.x, e.n, e.dtype, e.near_abs = t.data_ptr(), t.numel(), ops._HEALTH_DT[t.dtype], 0.5 * ops.HEALTH_DTYPE_MAX[t.dtype]
            calls.append((table, len(part), C.c_void_p(rec[lo:].data_ptr())))

        def run():
            for table, count, out in calls:
                _lib.check(lib.mobi_tensor_health(table, count, out, stream), "mobi_tensor_health")
        run.keep = (tensors, rec)
        return run

    pre32, pre16 = prebuilt(src), prebuilt(half)
    big = sorted(range(len(src)), key=lambda i: -numels[i])[:64]
    nbig = sum(numels[i] for i in big)
    big32, big16 = prebuilt([src[i] for i in big]), prebuilt([t for i in big for t in half[2 * i:2 * i + 1]])
    stats_big = ops.MultiTensorTable([[src[i] for i in big], [None] * len(big)])
    bar = "mobi_snapshot_multi (digest only, b = NULL), the bar"
    for r in range(a.rounds):
        lines.append(f"round {r + 1}")
        row("call:     ops.tensor_health, fp32 (7 launches)", lambda: ops.tensor_health(src))
        row("prebuilt: mobi_tensor_health, fp32 (7 launches)", pre32)
        row(bar, lambda: ops.snapshot_multi(stats))
        row("call:     ops.tensor_health, fp16, same bytes (14 launches)", lambda: ops.tensor_health(half))
        row("prebuilt: mobi_tensor_health, fp16, same bytes (14 launches)", pre16)
    lines.append(f"-- one launch: the 64 largest tensors, {nbig / 1e6:.1f} M elements (fp16: the first half of each, {nbig * 2 / 1e6:.0f} MB)")
    for r in range(a.rounds):
        lines.append(f"round {r + 1}")
        row("one launch: mobi_tensor_health, fp32, 64 tensors", big32, nbig * 4)
        row("one launch: the bar over the same 64 tensors", lambda: ops.snapshot_multi(stats_big), nbig * 4)
        row("one launch: mobi_tensor_health, fp16, 64 tensors", big16, nbig * 2)
    del src, half, stats, stats_big, pre32, pre16, big32, big16

    if not a.skip_forward:
        mobi_amd.set_engine_dtype(torch.float16)
        net = health.gauss_(instantiate_from_config(ucfg), 0).cuda().eval()
        p = ucfg["params"]
        side, b = int(p.get("image_size", 32)), a.batch
        g = torch.Generator().manual_seed(0)
        x = [torch.randn((b, 4, side, side), generator=g).cuda(), torch.randn((b, 4, side, side), generator=g).cuda(),
             (torch.randn((b, 1, side, side), generator=g) > 0).float().cuda()]
        cond = torch.randn((b, 2, int(p.get("context_dim", 768))), generator=g).cuda()
        t = torch.full((b,), 500, dtype=torch.long, device="cuda")
        fwd = lambda: net(x, t, context=cond)
        rows = [0]

        def probed():
            with health.probe() as hp:
                fwd()
            rows[0] = len(hp._pending)

        lines.append(f"-- (b) one UNet forward, batch {b}, latent {side} x {side}, fp16, eager")
        with torch.no_grad():
            for r in range(a.rounds):
                for what, fn in (("eager, no probe", fwd), ("eager under health.probe()", probed)):
                    m, lo, hi = timed(fn, a.reps)
                    lines.append(f"round {r + 1}  {what:<30s} {m:8.3f} ms ({lo:.3f} .. {hi:.3f})")
                    print(lines[-1], flush=True)
        lines.append(f"rows per forward: {rows[0]}; the captured-graph step: not measured here")
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
