#!/usr/bin/env python3
"""Throughput of the engine's Fréchet metrics against the fp32 torch restatement on the same GPU (what the reference's
eval tools run: torch ops, fp32 for RangeNet++).

    python tools/frechet_timing.py [--batch 64] [--iters 10] [--warmup 3] [--out FILE]

FRD: RangeNet++ features of 64 x 1024 range views (seeded weights; input kernel + 67 convolutions + band mean), fp16 and
bf16, in range views per second, and the fraction of the bf16 / fp16 dense MFMA peak (2.5 PFLOP/s) the 359 GFLOP per view
reach.  FID: CLIP ViT-B/32 embeddings plus the fp64 moments, images per second at 224 x 224.  Each figure is the median over
`iters` calls timed with device events after `warmup` calls; inputs are resident in HBM (no file decoding).  Prints one
JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VIEW_GFLOP = 359.0            # RangeNet++ (Darknet-53 + decoder) at 64 x 1024, 2 * MACs of the reference's convolutions
PEAK_TFLOPS = 2500.0          # MI355X dense fp16 / bf16 MFMA


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/frechet_timing.py measures on the GPU"

    import frd_ref
    import realism_ref as R
    from mobi_amd import build, realism as M
    build.build()
    n, dev = args.batch, "cuda"
    res = {"batch": n}
    views = torch.from_numpy(frd_ref.synthetic_views(n, 3)).float().to(dev)
    bb, dec = frd_ref.seeded_state_dicts(7)
    with torch.no_grad():
        for name, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            net = M.RangeNet.from_state_dicts(bb, dec, dtype=dt, device=dev)
            ms = _median_ms(lambda: net.features(views, n), args.iters, args.warmup)
            res[f"frd_{name}"] = {"ms": round(ms, 2), "views_per_s": round(n / ms * 1e3, 1),
                                  "tflops": round(VIEW_GFLOP * n / ms, 1),
                                  "peak_fraction": round(VIEW_GFLOP * n / ms / PEAK_TFLOPS, 3)}
        bb32 = {k: (v.float() if v.is_floating_point() else v).to(dev) for k, v in bb.items()}
        dec32 = {k: (v.float() if v.is_floating_point() else v).to(dev) for k, v in dec.items()}
        x32 = torch.stack([frd_ref.prepare(v) for v in views.double().cpu().numpy()]).to(dev)
        ms = _median_ms(lambda: frd_ref.forward(bb32, dec32, x32), max(2, args.iters // 2), 1)
        res["frd_torch_fp32"] = {"ms": round(ms, 2), "views_per_s": round(n / ms * 1e3, 1)}

        sd = R.clip_b32_state(31)
        fid = M.FID(M.CLIPScore.from_state_dict(sd, dtype=torch.float16, device=dev), batch_size=n)
        imgs = R.clip_images("time.fid", n).to(dev)
        ms = _median_ms(lambda: fid.stats(imgs), args.iters, args.warmup)
        res["fid_fp16"] = {"ms": round(ms, 2), "images_per_s": round(n / ms * 1e3, 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
