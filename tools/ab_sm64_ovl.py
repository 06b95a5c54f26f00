#!/usr/bin/env python3
"""A/B of the 64-deep-step small-m loop (igemm_ring64_kernel): requests dealt out between the MFMAs (MOBI_IGEMM_SM64_OVL, the
default) against the sequential step (=0), on the production shapes of the C = 640 / 1280 transformer blocks; graph-timed
microseconds, interleaved in one process, best of three; the two outputs are compared bit for bit.
    python tools/ab_sm64_ovl.py              # timing table
    python tools/ab_sm64_ovl.py --race 150   # race screen of the overlapped loop instead (every repeat bit-equal to the
                                              # first and to the sequential loop, an HBM-thrashing copy between some repeats)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.sweep_split import timeit                       # noqa: E402

# (rows m, n, k, taps, split): 1 x 1 projections and one short split-K range
SHAPES = [(4096, 1280, 1280, 1, 1), (2048, 2560, 1280, 1, 1), (1024, 1280, 1280, 1, 1), (16384, 640, 640, 1, 1),
          (8192, 640, 640, 1, 1), (4096, 3840, 1280, 1, 1), (1024, 1280, 2560, 1, 4), (1024, 1280, 1280, 3, 4)]
FORCE = {"MOBI_IGEMM_WM": "2", "MOBI_IGEMM_WIDE": "0", "MOBI_IGEMM_SMALL": "0", "MOBI_IGEMM_SM64": "1"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--race", type=int, default=0)
    a = ap.parse_args()
    from mobi_amd import _lib, build, ops
    build.build(verbose=False)
    reload_ = _lib.load().mobi_tuning_reload
    os.environ.update(FORCE)
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(0)
    trash = torch.empty(256 << 20, dtype=torch.uint8, device="cuda") if a.race else None
    bad = 0
    for m, n, k, taps, split in SHAPES:
        hw = 16 if taps == 3 else 64
        side = int(hw ** 0.5)
        x = torch.randn(m // hw, side, side, k, generator=g).cuda().to(dt)
        pw = ops.pack_conv(torch.randn(n, k, taps, taps, generator=g) / (taps * k ** 0.5), torch.randn(n, generator=g) * 0.1, dt, "cuda")
        res = torch.randn(m // hw, side, side, n, generator=g).cuda().to(dt)
        fn = lambda: ops.igemm(x, pw, residual=res, split_k=split)
        variants = (("overlapped", {}), ("sequential", {"MOBI_IGEMM_SM64_OVL": "0"}))
        best, outs = {}, {}
        for rep in range(1 if a.race else 3):
            for tag, env in variants:
                os.environ.update(env)
                reload_()
                if rep == 0:
                    outs[tag] = fn().clone()
                if not a.race:
                    best[tag] = min(best.get(tag, 1e30), timeit(fn, 10, warm=1))
                for k_ in env:
                    os.environ.pop(k_, None)
        reload_()
        same = torch.equal(outs["overlapped"], outs["sequential"])
        what = f"m={m} n={n} k={k * taps * taps} ({taps}x{taps}) split={split}"
        if a.race:
            mism = 0
            for i in range(a.race):
                if i % 5 == 0:
                    trash.add_(1)                            # evict L2 / MALL, busy HBM
                mism += not torch.equal(fn(), outs["overlapped"])
            torch.cuda.synchronize()
            bad += mism + (not same)
            print(f"{what}: mismatching repeats {mism}/{a.race} | bit-equal to the sequential loop: {same}", flush=True)
        else:
            fl = 2.0 * m * n * k * taps * taps
            print(f"{what}: " + " | ".join(f"{t} {best[t]:6.1f} us {fl / best[t] / 1e6:5.0f} TFLOP/s" for t, _ in variants) +
                  f" | bit-equal {same}", flush=True)
            bad += not same
    if a.race:
        print("RACE SCREEN", "CLEAN" if bad == 0 else f"FAILED ({bad})")
    for k_ in FORCE:
        os.environ.pop(k_, None)
    reload_()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
