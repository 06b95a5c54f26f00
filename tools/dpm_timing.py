#!/usr/bin/env python3
"""What a sample costs with DPM-Solver++(2M) against DDIM and PLMS on the benched model (one GPU).

    python tools/dpm_timing.py [--workload mobi_nusc_512] [--objects B] [--dtype bf16|fp16] [--repeats R]
                               [--out FILE]

Same model and synthetic inputs as bench.py (random-init weights of the real architecture, UNet batch 2 * B
interleaved camera / lidar elements, inputs resident in HBM), every sampler on its graph path (one launch per step;
PLMS: one per UNet evaluation).  Each figure is the median over R whole `sample()` calls, host clock around a call
that ends in a device synchronise, the samplers alternated inside every repeat:
  * ms per step, DPM-20 vs DDIM-20, at guidance 1 and 5: the DPM update should cost what DDIM's does (a few MB of
    fp32 traffic next to a UNet evaluation);
  * ms per object batch at guidance 5: DPM-20 (20 UNet evaluations) vs PLMS-50 (51), the shipped invocation.
Prints one JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="mobi_nusc_512")
    ap.add_argument("--objects", type=int, default=None)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/dpm_timing.py measures on the GPU"

    import mobi_amd
    from bench import WORKLOADS, build_model
    from mobi_amd import build
    from mobi_amd.ldm.models.diffusion.ddim import DDIMSampler
    from mobi_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from mobi_amd.ldm.models.diffusion.plms import PLMSSampler
    build.build(verbose=False)
    mobi_amd.set_engine_dtype(torch.bfloat16 if args.dtype == "bf16" else torch.float16)
    device = torch.device("cuda", 0)
    wl = WORKLOADS[args.workload]
    B = args.objects or wl["objects"]
    side, N = wl["latent"], 2 * B
    model = build_model(args.workload).to(device)
    g = torch.Generator(device="cpu").manual_seed(1234)
    mk = lambda *s: torch.randn(*s, generator=g).to(device)
    x_T, inpaint, cond, uc = mk(N, 4, side, side), mk(N, 4, side, side), mk(N, 2, 768), mk(N, 2, 768)
    mask = torch.ones(N, 1, side, side)
    mask[:, :, side // 4: 3 * side // 4, side // 4: 3 * side // 4] = 0
    mask = mask.to(device)
    samplers = {"ddim": DDIMSampler(model), "dpm": DPMSolverSampler(model), "plms": PLMSSampler(model)}

    def run(name, S, scale):
        kw = dict(S=S, batch_size=N, shape=[4, side, side], conditioning=cond, verbose=False, x_T=x_T, eta=0.0,
                  unconditional_guidance_scale=scale, unconditional_conditioning=uc)
        if name == "ddim":
            kw["test_model_kwargs"] = {"inpaint_image": inpaint, "inpaint_mask": mask}
        else:
            kw.update(inpaint_image=inpaint, inpaint_mask=mask)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = samplers[name].sample(**kw)[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(out).all()), f"{name}-{S} at guidance {scale}: non-finite sample"
        return dt

    for scale in (1.0, 5.0):                 # captures every graph, then brings the clocks up
        for name in samplers:
            run(name, 4, scale)
    for name in ("ddim", "dpm"):
        run(name, 20, 5.0)

    times = {}
    for _ in range(args.repeats):
        for key, (name, S, scale) in {"ddim20_g1": ("ddim", 20, 1.0), "dpm20_g1": ("dpm", 20, 1.0),
                                      "ddim20_g5": ("ddim", 20, 5.0), "dpm20_g5": ("dpm", 20, 5.0),
                                      "plms50_g5": ("plms", 50, 5.0)}.items():
            times.setdefault(key, []).append(run(name, S, scale))
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = {k: round((max(v) - min(v)) / statistics.median(v), 4) for k, v in times.items()}
    rec = {
        "tool": "dpm_timing", "workload": args.workload, "objects": B, "unet_batch_elements": N, "latent": side,
        "dtype": args.dtype, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
        "ms_per_step": {"ddim_g1": round(med["ddim20_g1"] / 20 * 1e3, 3), "dpm_g1": round(med["dpm20_g1"] / 20 * 1e3, 3),
                        "ddim_g5": round(med["ddim20_g5"] / 20 * 1e3, 3), "dpm_g5": round(med["dpm20_g5"] / 20 * 1e3, 3),
                        "plms_g5_per_evaluation": round(med["plms50_g5"] / 51 * 1e3, 3)},
        "ms_per_object_batch_g5": {"dpm20": round(med["dpm20_g5"] * 1e3, 1), "plms50": round(med["plms50_g5"] * 1e3, 1),
                                   "plms50_over_dpm20": round(med["plms50_g5"] / med["dpm20_g5"], 3)},
        "spread_max_minus_min_over_median": spread,
    }
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
