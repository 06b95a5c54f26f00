#!/usr/bin/env python3
"""Where a launch of the 64-deep-step small-m kernel (igemm_ring64_kernel) goes, per wave, in shader cycles: the phases of a
k-step  counted wait | barrier | fragment reads | request issue | LDS wait | MFMAs, the fixed cost in front of the first step
(entry, addresses, prologue requests) and behind the last one (drain + epilogue).  With the default loop
(MOBI_IGEMM_SM64_OVL) the requests are dealt out between the MFMAs: their columns are zero and `MFMAs` is the whole
stream; MOBI_IGEMM_SM64_OVL=0 is the sequential step.  Needs a library built with -DMOBI_STAMP=5 (MOBI_HIPCC_FLAGS; this
script builds it if the library at hand is another one, and does NOT build the plain library back).
    MOBI_HIPCC_FLAGS=-DMOBI_STAMP=5 python tools/phase_ring64.py"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (rows m, n, k, split)
SHAPES = [(4096, 1280, 1280, 1), (2048, 2560, 1280, 1), (16384, 640, 640, 1), (1024, 1280, 2560, 4)]


def main():
    if "-DMOBI_STAMP=5" not in os.environ.get("MOBI_HIPCC_FLAGS", ""):
        os.environ["MOBI_HIPCC_FLAGS"] = (os.environ.get("MOBI_HIPCC_FLAGS", "") + " -DMOBI_STAMP=5").strip()
    os.environ.update({"MOBI_IGEMM_WM": "2", "MOBI_IGEMM_WIDE": "0", "MOBI_IGEMM_SMALL": "0", "MOBI_IGEMM_SM64": "1"})
    from mobi_amd import build
    build.build(verbose=False)
    from mobi_amd import _lib, ops
    lib = _lib.load()
    lib.mobi_debug_set_phases.argtypes = [C.c_void_p]
    lib.mobi_debug_set_phases.restype = C.c_int
    g = torch.Generator().manual_seed(0)
    dt = torch.bfloat16
    cap = 1 << 12                                            # blocks
    buf = torch.zeros(cap * 8 * 8, dtype=torch.int64, device="cuda")
    for m, n, k, split in SHAPES:
        x = torch.randn(m // 64, 8, 8, k, generator=g).cuda().to(dt)
        pw = ops.pack_conv(torch.randn(n, k, 1, 1, generator=g) / k ** 0.5, torch.zeros(n), dt, "cuda")
        res = torch.randn(m // 64, 8, 8, n, generator=g).cuda().to(dt)
        run = lambda: ops.igemm(x, pw, residual=res, split_k=split)
        for tag, env in (("overlapped", None), ("sequential", "0")):
            if env is None:
                os.environ.pop("MOBI_IGEMM_SM64_OVL", None)
            else:
                os.environ["MOBI_IGEMM_SM64_OVL"] = env
            lib.mobi_tuning_reload()
            assert lib.mobi_debug_set_phases(None) == 0
            for _ in range(5):
                run()
            torch.cuda.synchronize()
            buf.zero_()
            assert lib.mobi_debug_set_phases(C.c_void_p(buf.data_ptr())) == 0
            run()
            torch.cuda.synchronize()
            assert lib.mobi_debug_set_phases(None) == 0
            d = buf.cpu().numpy().reshape(cap * 4, 16).astype("float64")       # [block x wave][2 rows of 8]
            d = d[d[:, 6] > 0]
            per = (d[:, :6] / d[:, 6:7]).mean(0)
            print(f"m={m} n={n} k={k} split={split} {tag}: {len(d)} waves x {int(d[:, 6].mean())} steps | cycles per step: wait {per[0]:.0f} | "
                  f"barrier {per[1]:.0f} | fragment reads {per[2]:.0f} | request issue {per[3]:.0f} | LDS wait {per[4]:.0f} | MFMAs {per[5]:.0f} | "
                  f"sum {per.sum():.0f} || per launch: before the first step {d[:, 8].mean():.0f} | drain + epilogue {d[:, 9].mean():.0f} | "
                  f"entry to end {d[:, 7].mean():.0f}", flush=True)
    os.environ.pop("MOBI_IGEMM_SM64_OVL", None)
    lib.mobi_tuning_reload()


if __name__ == "__main__":
    main()
