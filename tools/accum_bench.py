#!/usr/bin/env python3
"""Time the gradient-accumulation launch alone (`mobi_accum_multi`, one launch over every (gradient, accumulator) pair of a
micro-batch) -- informational.

    python tools/accum_bench.py [--config configs/mobi_nusc_512.yaml] [--reps 10] [--rounds 3] [--out profiles/accum_multi.txt]

The 432 trained tensors of the full-width UNet, accumulators laid out as `train.GradAccumulator` lays them out, gradients as
fresh allocations.  Device events, median of `--reps` after two warm-up launches, `--rounds` alternating rounds of: the ACCUM
launch (12 B per element), `mobi_ema_multi` over the same list (the bar: the same walker, the same three streams), the ASSIGN
launch (8 B per element), and what the launch replaces, the per-tensor torch loop `acc.add_(g, alpha=w)`.  Only the shapes of
the network are used (the tensors are filled with noise): the kernels' time does not depend on the values."""
import argparse
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from mobi_amd import _lib, dist as mdist, ops, train  # noqa: E402
from tools.ema_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(HERE, "configs", "mobi_nusc_512.yaml"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mobi_amd.ldm.util import instantiate_from_config, load_config
    ucfg = load_config(a.config, ["model.params.lidar_stage_config.params.ckpt_path=null"])["model"]["params"]["unet_config"]
    with torch.device("meta"):
        net = instantiate_from_config(ucfg)
    shapes = {k: tuple(p.shape) for k, p in net.named_parameters() if any(m in k for m in train.TRAINABLE_MARKERS)}
    names = sorted(shapes)
    layout, lengths = mdist.gradient_bucket_layout({k: math.prod(shapes[k]) for k in names})
    buckets = [torch.zeros(n, device="cuda") for n in lengths]
    acc = [buckets[layout[k][0]][layout[k][1]:layout[k][1] + layout[k][2]] for k in names]
    grads = [torch.randn(layout[k][2], device="cuda") for k in names]
    shadows = [torch.randn(layout[k][2], device="cuda") for k in names]
    n = sum(t.numel() for t in acc)
    table = ops.MultiTensorTable([ops.LIVE, acc])
    table.set_live(grads)
    pairs = ops.MultiTensorTable([grads, shadows])
    w = 0.25
    lines = [f"{torch.cuda.get_device_name(0)}; device events, median (min .. max) of {a.reps}; fp32",
             f"-- trained tensors: {len(names)} tensors, {n / 1e6:.1f} M elements, {table.n_chunks} chunks, {len(buckets)} buckets"]
    print("\n".join(lines), flush=True)

    def row(what, fn, bytes_per_elem):
        med, lo, hi = timed(fn, a.reps)
        lines.append(f"{what:<44s} {med:8.3f} ms ({lo:.3f} .. {hi:.3f})  {bytes_per_elem} B/element -> "
                     f"{n * bytes_per_elem / med / 1e9:.2f} TB/s")
        print(lines[-1], flush=True)

    def per_tensor():
        for b, g in zip(acc, grads):
            b.add_(g, alpha=w)
    for r in range(a.rounds):
        lines.append(f"round {r + 1}")
        row("mobi_accum_multi (ACCUM)", lambda: ops.accum_multi(table, w, _lib.MT_ACCUM), 12)
        row("mobi_ema_multi (update), the bar", lambda: ops.ema_multi(pairs, 1e-4), 12)
        row("mobi_accum_multi (ASSIGN)", lambda: ops.accum_multi(table, w, _lib.MT_ASSIGN), 8)
        row("torch, per tensor: acc.add_(g, alpha=w)", per_tensor, 12)
        ops.accum_multi(table, w, _lib.MT_ASSIGN)                 # (keeps the sums of the ACCUM rows finite from round to round)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
