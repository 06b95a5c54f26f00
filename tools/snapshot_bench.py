#!/usr/bin/env python3
"""Time the checkpoint snapshot launch alone (`mobi_snapshot_multi`: a word-for-word copy of every listed tensor plus a 64-bit
digest and a non-finite flag per tensor) -- informational.

    python tools/snapshot_bench.py [--config configs/mobi_nusc_512.yaml] [--reps 10] [--rounds 3] [--out profiles/snapshot_multi.txt]

The 432 trained tensors of the full-width UNet as fresh allocations, destinations laid out as `checkpoint.Checkpointer` lays its
staging buffer out (`dist.gradient_bucket_layout`: sorted names, 16-byte aligned starts).  Device events, median of `--reps` after
two warm-up launches, `--rounds` alternating rounds of: the snapshot with destinations (8 B per element), the bar --
`mobi_accum_multi` ASSIGN over the same list (the same walker, the same two streams, one multiply instead of the digest) -- and the
snapshot without destinations (statistics only, what `Checkpointer.load` runs: 4 B per element).  Only the shapes of the network are
used (the tensors are filled with noise): the kernels' time does not depend on the values."""
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
    layout, lengths = mdist.gradient_bucket_layout({k: math.prod(shapes[k]) for k in names}, 1 << 62)
    staging = torch.zeros(lengths[0], device="cuda")
    dst = [staging[layout[k][1]:layout[k][1] + layout[k][2]] for k in names]
    src = [torch.randn(layout[k][2], device="cuda") for k in names]
    n = sum(t.numel() for t in src)
    snap = ops.MultiTensorTable([src, dst])
    stats = ops.MultiTensorTable([src, [None] * len(src)])
    assign = ops.MultiTensorTable([ops.LIVE, dst])
    assign.set_live(src)
    lines = [f"{torch.cuda.get_device_name(0)}; device events, median (min .. max) of {a.reps}; fp32",
             f"-- trained tensors: {len(names)} tensors, {n / 1e6:.1f} M elements, {snap.n_chunks} chunks"]
    print("\n".join(lines), flush=True)

    def row(what, fn, bytes_per_elem):
        med, lo, hi = timed(fn, a.reps)
        lines.append(f"{what:<44s} {med:8.3f} ms ({lo:.3f} .. {hi:.3f})  {bytes_per_elem} B/element -> "
                     f"{n * bytes_per_elem / med / 1e9:.2f} TB/s")
        print(lines[-1], flush=True)

    for r in range(a.rounds):
        lines.append(f"round {r + 1}")
        row("mobi_snapshot_multi (copy + digest)", lambda: ops.snapshot_multi(snap), 8)
        row("mobi_accum_multi (ASSIGN, w = 1), the bar", lambda: ops.accum_multi(assign, 1.0, _lib.MT_ASSIGN), 8)
        row("mobi_snapshot_multi (digest only, b = NULL)", lambda: ops.snapshot_multi(stats), 4)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
