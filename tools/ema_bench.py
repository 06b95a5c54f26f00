#!/usr/bin/env python3
"""Time the EMA update of the shadow weights alone (`mobi_ema_multi`, one launch over every (parameter, shadow) pair) --
informational.

    python tools/ema_bench.py [--config configs/mobi_nusc_512.yaml] [--reps 10] [--out profiles/ema_multi.txt]

Two lists of the full-width UNet: every `requires_grad` tensor (what `LatentDiffusion(use_ema=True)` keeps shadows of) and the
432 trained tensors.  Device events, median of `--reps` after two warm-up launches.  Beside it, measured in the same process:
`mobi_adamw_multi` over the trained list (the same walker with seven fp32 streams instead of three), the swap, and the
per-tensor torch form of the same update, `s.sub_(omd * (s - p))` (three elementwise launches per tensor).  Only the shapes
of the network are used (the tensors are filled with noise): the kernels' time does not depend on the values."""
import argparse
import math
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from mobi_amd import ops, train  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(HERE, "configs", "mobi_nusc_512.yaml"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from mobi_amd.ldm.util import instantiate_from_config, load_config
    ucfg = load_config(a.config, ["model.params.lidar_stage_config.params.ckpt_path=null"])["model"]["params"]["unet_config"]
    with torch.device("meta"):
        net = instantiate_from_config(ucfg)
    shapes = [(k, tuple(p.shape)) for k, p in net.named_parameters() if p.requires_grad]
    lists = {"every requires_grad tensor": shapes,
             "trained tensors": [(k, s) for k, s in shapes if any(m in k for m in train.TRAINABLE_MARKERS)]}
    lines = [f"{torch.cuda.get_device_name(0)}; device events, median (min .. max) of {a.reps}; fp32"]
    omd = 1.0 - 0.9999
    for title, lst in lists.items():
        make = lambda: [torch.randn(math.prod(s), device="cuda") for _, s in lst]
        p, s = make(), make()
        n = sum(t.numel() for t in p)
        pairs = ops.MultiTensorTable([p, s])
        lines.append(f"-- {title}: {len(lst)} tensors, {n / 1e6:.1f} M elements, {pairs.n_chunks} chunks")

        def row(what, fn, bytes_per_elem):
            med, lo, hi = timed(fn, a.reps)
            lines.append(f"{what:<44s} {med:8.3f} ms ({lo:.3f} .. {hi:.3f})  {bytes_per_elem} B/element -> "
                         f"{n * bytes_per_elem / med / 1e9:.2f} TB/s")
            print(lines[-1], flush=True)

        print(lines[-1], flush=True)
        row("mobi_ema_multi (update)", lambda: ops.ema_multi(pairs, omd), 12)
        row("mobi_ema_multi (swap)", lambda: ops.swap_multi(pairs), 16)
        omd_t = torch.tensor(omd, device="cuda")

        def per_tensor():
            for pi, si in zip(p, s):
                si.sub_(omd_t * (si - pi))
        row("torch, per tensor: s.sub_(omd * (s - p))", per_tensor, 12)
        if title == "trained tensors":
            m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
            mt = ops.MultiTensorTable([p, ops.LIVE, m, v])
            mt.set_live([torch.randn_like(t) * 1e-3 for t in p])
            step = [0]

            def adamw():
                step[0] += 1
                ops.adamw_multi(mt, 1.0, step[0], 1e-5)
            row("mobi_adamw_multi (same walker, 7 streams)", adamw, 28)
        del p, s, pairs
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
