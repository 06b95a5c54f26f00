#!/usr/bin/env python3
"""Pairs per second of the engine's realism metrics at batch 64 against the fp32 torch restatement on the same GPU (what
the reference's eval tools run: torch ops, fp32 for LPIPS).

    python tools/realism_timing.py [--batch 64] [--dtype fp16|bf16] [--iters 20] [--warmup 5] [--out FILE]

LPIPS at 256 x 256 (AlexNet, seeded weights) and CLIP score at 224 x 224 (ViT-B/32, seeded weights).  Each figure is the
median over `iters` calls timed with device events after `warmup` calls; inputs are resident in HBM, so the numbers leave
out image decoding.  Prints one JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/realism_timing.py measures on the GPU"

    import realism_ref as R
    from mobi_amd import build, realism as M
    build.build()
    dt = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    n, dev = args.batch, "cuda"
    res = {"batch": n, "dtype": args.dtype}
    with torch.no_grad():
        convs, lins = M.lpips_state_from_dicts(*R.alex_state(13))
        lp = M.LPIPS(convs, lins, dtype=dt, device=dev)
        a = R.lpips_images("time.a", n, 256, 256).to(dev)
        b = R.lpips_images("time.b", n, 256, 256).to(dev)
        convs_d = [(w.to(dev), bb.to(dev)) for w, bb in convs]
        lins_d = [l.to(dev) for l in lins]
        ms = _median_ms(lambda: lp(a, b), args.iters, args.warmup)
        ms_t = _median_ms(lambda: R.lpips(a, b, convs_d, lins_d, dtype=torch.float32), args.iters, args.warmup)
        res["lpips_256"] = {"engine_ms": round(ms, 3), "engine_pairs_per_s": round(n / ms * 1e3, 1),
                            "torch_fp32_ms": round(ms_t, 3), "torch_fp32_pairs_per_s": round(n / ms_t * 1e3, 1)}

        sd = R.clip_b32_state(31)
        cs = M.CLIPScore.from_state_dict(sd, dtype=dt, device=dev)
        sd_d = {k: v.to(dev) for k, v in sd.items()}
        r = R.clip_images("time.r", n).to(dev)
        p = R.clip_images("time.p", n).to(dev)
        ms = _median_ms(lambda: cs(r, p), args.iters, args.warmup)
        ms_t = _median_ms(lambda: R.clip_score(r, p, sd_d, dtype=torch.float32), args.iters, args.warmup)
        res["clip_224"] = {"engine_ms": round(ms, 3), "engine_pairs_per_s": round(n / ms * 1e3, 1),
                           "torch_fp32_ms": round(ms_t, 3), "torch_fp32_pairs_per_s": round(n / ms_t * 1e3, 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
