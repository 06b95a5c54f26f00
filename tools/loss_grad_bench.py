#!/usr/bin/env python3
"""Time the fused loss / entering-gradient launch (`mobi_loss_grad` + its finish pass) against the composition it replaced in
`train.loss_and_gradients`: the torch subtract, square and mean, `mobi_lincomb4`, `mobi_pack_nchw_sources` -- informational.

    python tools/loss_grad_bench.py [--reps 10] [--dtype fp16] [--out profiles/loss_grad.txt]

At the production shapes of the UNet's output ([4, 4, 64, 64]: mobi_nusc_512, two camera / lidar pairs; [40, 4, 32, 32]:
mobi_nusc_256 at its batch).  Device events around each side, the two sides alternating in one process, median (min .. max) of
`--reps` after two warm-up rounds.  About 1 MB moves: what is timed is launches, not bandwidth.  Not timed (it has no duration of
its own to take with events): the blocking `logvar[t]` read-back the old step made before these launches."""
import argparse
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from mobi_amd import ops  # noqa: E402


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    lines = [f"{torch.cuda.get_device_name(0)}; device events, the two sides alternating, median (min .. max) of {a.reps}; {a.dtype}"]
    print(lines[0], flush=True)
    for shape in ((4, 4, 64, 64), (40, 4, 32, 32)):
        g = torch.Generator(device="cuda").manual_seed(1)
        eps, target = torch.randn(shape, device="cuda", generator=g), torch.randn(shape, device="cuda", generator=g)
        t = torch.randint(0, 1000, (shape[0],), device="cuda", generator=g)
        logvar, lvlb = torch.zeros(1000, device="cuda"), torch.zeros(1000, device="cuda")
        scale = 2.0 ** 10
        k = 2.0 * scale / eps.numel()

        def new():
            return ops.loss_grad(eps, target, t, logvar, lvlb, loss_scale=scale, dtype=dt)

        def old():
            loss = torch.mean((eps - target) ** 2)
            return ops.pack_sources([ops.lincomb4([eps, target], [k, -k])], dt), loss
        dy_new, _, terms = new()
        dy_old, loss_old = old()
        same = torch.equal(dy_new.view(torch.int16), dy_old.view(torch.int16))
        ms = {"new": [], "old": []}
        for rep in range(a.reps + 2):
            for name, fn in (("new", new), ("old", old)):
                v = event_ms(fn)
                if rep >= 2:
                    ms[name].append(v)
        lines.append(f"-- eps {list(shape)}: dy bit-equal {same}; loss {float(terms[2])!r} (fused, fp64 sums) {float(loss_old)!r} (torch, fp32)")
        for name, what in (("new", "mobi_loss_grad + finish pass (2 launches)"),
                           ("old", "torch sub, pow, mean + lincomb4 + pack_sources")):
            v = ms[name]
            lines.append(f"{what:<50s} {statistics.median(v) * 1e3:8.1f} us ({min(v) * 1e3:.1f} .. {max(v) * 1e3:.1f})")
        print("\n".join(lines[-3:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
