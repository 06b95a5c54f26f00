#!/usr/bin/env python3
"""Time the attention probe's launch against the launch it judges -- informational, no bar.

    python tools/attention_health_bench.py [--config configs/mobi_nusc_512.yaml] [--reps 10] [--rounds 2] [--batch 16]
                                           [--out profiles/attention_health.txt]

(a) `mobi_attention_health` and `mobi_attention` on the same operands, alternating in one process: [16 images, 4096 x 4096 tokens,
8 heads x 40] (the first level's self-attention) and [16, 256 x 256, 8 x 160] (the 8 x 8 level's), fp16 and bf16, q | k | v
stacked as the UNet hands them over, q_log2_scaled.  Device events, median of `--reps` after two warm-up launches.
(b) One UNet forward of the config at `--batch` images, N(0, 1 / fan_in) weights, fp16, eager: under `health.probe()` and under
`health.probe(attention=True)`.
(c) The tolerance of tests/test_gpu_attention_health.py on ref_absmax / err_max: the kernel's algorithm restated in fp32 numpy
against fp64 over the test's cases (CPU arithmetic; tests/attention_health_cases.py), and 4 x that.
No hardware counters are collected."""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import mobi_amd  # noqa: E402
from mobi_amd import health, ops  # noqa: E402
from tools.ema_bench import timed  # noqa: E402

SHAPES = [(16, 4096, 4096, 8, 40), (16, 256, 256, 8, 160)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(HERE, "configs", "mobi_nusc_512.yaml"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--skip-forward", action="store_true")
    ap.add_argument("--skip-tolerance", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"{torch.cuda.get_device_name(0)}; device events, median (min .. max) of {a.reps}; no hardware counters collected",
             "-- (a) mobi_attention_health against mobi_attention on the same operands (stacked q | k | v, q_log2_scaled), alternating"]
    print("\n".join(lines), flush=True)
    g = torch.Generator().manual_seed(0)
    for n, tq, tk, heads, dh in SHAPES:
        c = heads * dh
        for dtype in (torch.float16, torch.bfloat16):
            qkv = torch.randn((n, max(tq, tk), 3 * c), generator=g).to(dtype).cuda()
            qkv[..., :c] *= dh ** -0.5 * ops.LOG2E
            q, k, v = qkv[:, :tq, :c], qkv[:, :tk, c:2 * c], qkv[:, :tk, 2 * c:]
            out = ops.attention(q, k, v, heads, dh ** -0.5, v_rows=True, q_log2_scaled=True)
            rec = ops.attention_health(q, k, v, out, heads, dh ** -0.5, v_rows=True, q_log2_scaled=True)
            name = health.DTYPE_NAMES[dtype]
            flop = 4.0 * n * heads * tq * tk * dh
            for r in range(a.rounds):
                for what, fn in (("mobi_attention", lambda: ops.attention(q, k, v, heads, dh ** -0.5, v_rows=True, q_log2_scaled=True)),
                                 ("mobi_attention_health", lambda: ops.attention_health(q, k, v, out, heads, dh ** -0.5, v_rows=True,
                                                                                        q_log2_scaled=True, records=rec))):
                    m, lo, hi = timed(fn, a.reps)
                    lines.append(f"[{n}, {tq} x {tk}, {heads} x {dh}] {name} round {r + 1}  {what:<22s} {m:9.3f} ms ({lo:.3f} .. {hi:.3f})"
                                 f"  {flop / m / 1e9:8.2f} TFLOP/s")
                    print(lines[-1], flush=True)
            del qkv, q, k, v, out, rec

    if not a.skip_forward:
        from mobi_amd.ldm.util import instantiate_from_config, load_config
        ucfg = load_config(a.config, ["model.params.lidar_stage_config.params.ckpt_path=null"])["model"]["params"]["unet_config"]
        mobi_amd.set_engine_dtype(torch.float16)
        net = health.gauss_(instantiate_from_config(ucfg), 0).cuda().eval()
        p = ucfg["params"]
        side, b = int(p.get("image_size", 32)), a.batch
        x = [torch.randn((b, 4, side, side), generator=g).cuda(), torch.randn((b, 4, side, side), generator=g).cuda(),
             (torch.randn((b, 1, side, side), generator=g) > 0).float().cuda()]
        cond = torch.randn((b, 2, int(p.get("context_dim", 768))), generator=g).cuda()
        t = torch.full((b,), 500, dtype=torch.long, device="cuda")
        counts = {}

        def probed(attention):
            def run():
                with health.probe(attention=attention) as hp:
                    net(x, t, context=cond)
                counts[attention] = (len(hp._pending), len(hp._att_pending))
            return run

        lines.append(f"-- (b) one UNet forward, batch {b}, latent {side} x {side}, fp16, eager")
        with torch.no_grad():
            for r in range(a.rounds):
                for what, fn in (("under health.probe()", probed(False)), ("under health.probe(attention=True)", probed(True))):
                    m, lo, hi = timed(fn, a.reps)
                    lines.append(f"round {r + 1}  {what:<36s} {m:9.3f} ms ({lo:.3f} .. {hi:.3f})")
                    print(lines[-1], flush=True)
        lines.append(f"rows per forward: {counts[True][0]}, of them probed attention launches: {counts[True][1]}")
        print(lines[-1], flush=True)

    if not a.skip_tolerance:
        from tests import attention_health_cases as AC
        worst, tol = AC.measured_tolerance()
        lines.append(f"-- (c) tolerance of tests/test_gpu_attention_health.py on ref_absmax and err_max, {len(AC.CASES)} cases (CPU arithmetic)")
        lines.append(f"the kernel's algorithm restated in fp32 numpy against fp64: worst |o32 - o64| = {worst:.6g}")
        lines.append(f"tolerance = 4 x that = {tol:.6g}")
        print("\n".join(lines[-3:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
