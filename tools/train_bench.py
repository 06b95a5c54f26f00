#!/usr/bin/env python3
"""Time one training step of the adapter parameters (mobi_amd/train.py: forward with a tape + the backward pass through the
whole UNet + AdamW on the 432 adapter tensors) -- informational: the backward kernels are a first slice, not tuned.

    python tools/train_bench.py [--mc 320] [--side 32] [--n 4] [--dtype bf16] [--iters 3] [--scaler] [--ema] [--accumulate K] [--refresh]

--scaler: the gradients stay multiplied by a `train.GradScaler`'s scale and `AdamW.step_scaled` (two multi-tensor launches + one
read-back) replaces the per-tensor unscale and update launches; `--max-norm` adds gradient-norm clipping to it.
--ema: EMA shadows of every `requires_grad` tensor of the UNet (`ldm.modules.ema.LitEma`, what `LatentDiffusion(use_ema=True)`
keeps) and their update inside the timed step, after the optimizer's (what `on_train_batch_end` calls: one `mobi_ema_multi` launch).
--accumulate K: a timed iteration is K forward / backward passes, each added to a `train.GradAccumulator` (one `mobi_accum_multi`
launch), plus ONE optimizer step on the accumulated mean (`GradAccumulator.step` -> `AdamW.step_scaled`); the time printed is per
optimizer step.
--refresh: every optimizer step ends with one `train.WeightRefresher.refresh()` (`mobi_repack_multi`: the 16-bit copies of the
trained Linear weights in one launch) instead of the lazy per-tensor re-pack inside the next forward / backward."""
import argparse
import math
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import mobi_amd  # noqa: E402
from mobi_amd import ops, train  # noqa: E402
from tools import _synth as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mc", type=int, default=320)
    ap.add_argument("--side", type=int, default=32)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--scaler", action="store_true")
    ap.add_argument("--max-norm", type=float, default=None)
    ap.add_argument("--ema", action="store_true")
    ap.add_argument("--accumulate", type=int, default=0)
    ap.add_argument("--refresh", action="store_true")
    a = ap.parse_args()
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float16
    mobi_amd.set_engine_dtype(dt)
    from mobi_amd.ldm.util import instantiate_from_config, load_config
    ucfg = load_config(os.path.join(HERE, "configs", "mobi_nusc_512.yaml"),
                       ["model.params.lidar_stage_config.params.ckpt_path=null"])["model"]["params"]["unet_config"]
    ucfg["params"]["model_channels"] = a.mc                   # (the UNet of configs/mobi_nusc_512.yaml; --mc narrows it for quick runs)
    ucfg["params"]["image_size"] = a.side
    net = instantiate_from_config(ucfg)
    W.fill_module_(net, seed=3)
    net = net.cuda()
    x = W.synth_input("tb.x", (a.n, 9, a.side, a.side)).cuda()
    ctx = W.synth_input("tb.c", (a.n, 2, 768)).cuda()
    noise = W.synth_input("tb.n", (a.n, 4, a.side, a.side)).cuda()
    t = torch.full((a.n,), 500, dtype=torch.long, device="cuda")
    opt = train.AdamW({k: p for k, p in net.named_parameters() if any(m in k for m in train.TRAINABLE_MARKERS)}, lr=1e-5)
    refresh = train.WeightRefresher(net, list(opt.params)) if a.refresh else None
    ema = None
    if a.ema:
        from mobi_amd.ldm.modules.ema import LitEma
        ema = LitEma(net)
    sink = []
    scaler = train.GradScaler() if a.scaler else None
    if scaler is not None:
        scaler.first_use(noise.numel())

    acc = train.GradAccumulator(opt, a.accumulate) if a.accumulate else None
    static = 1.0 if dt == torch.bfloat16 else 2.0 ** round(math.log2(noise.numel() / 4))

    def step(profile=False):
        if profile:
            ops.set_profiler(sink)
        if acc is not None:
            for _ in range(a.accumulate):
                if scaler is not None:
                    loss, grads = train.loss_and_gradients(net, x, t, ctx, noise, loss_scale=scaler.scale, unscale=False)
                else:
                    loss, grads = train.loss_and_gradients(net, x, t, ctx, noise, loss_scale=static)
                grads.pop("__dcontext__", None)
                acc.add(grads, scale=1.0 if scaler is None else scaler.scale)
            acc.step(scaler=scaler, max_norm=a.max_norm, refresh=refresh)
            if ema is not None:
                ema(net)
            ops.set_profiler(None)
            return loss
        if scaler is not None:
            loss, grads = train.loss_and_gradients(net, x, t, ctx, noise, loss_scale=scaler.scale, unscale=False)
            grads.pop("__dcontext__", None)
            opt.step_scaled(grads, scaler=scaler, max_norm=a.max_norm, refresh=refresh)
            if ema is not None:
                ema(net)
            ops.set_profiler(None)
            return loss
        loss, grads = train.loss_and_gradients(net, x, t, ctx, noise, loss_scale=static)
        grads.pop("__dcontext__", None)
        opt.step(grads, refresh=refresh)
        if ema is not None:
            ema(net)
        ops.set_profiler(None)
        return loss
    with torch.no_grad():
        step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            loss = step()
        torch.cuda.synchronize()
        dt_s = (time.perf_counter() - t0) / a.iters
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
    n_par = sum(p.numel() for p in opt.params.values())
    if ema is not None:
        n_ema = sum(b.numel() for b in ema.buffers()) - 2
        print(f"--ema: shadows of {len(list(ema.buffers())) - 2} tensors / {n_ema / 1e6:.1f} M parameters ({n_ema * 4 / 2**30:.2f} GiB), "
              f"{int(ema.num_updates)} updates")
    if acc is not None:
        print(f"--accumulate: {a.accumulate} micro-batches of {a.n} per optimizer step, accumulators {sum(b.numel() for b in acc.buckets) * 4 / 2**30:.2f} GiB "
              f"in {len(acc.buckets)} buckets; the time below is per optimizer step")
    if refresh is not None:
        print(f"--refresh: {len(refresh.layers)} layers, {refresh.launches} launches of mobi_repack_multi")
    if scaler is not None:
        print(f"--scaler: loss scale {scaler.scale:g}, max_norm {a.max_norm}")
    print(f"training step, UNet model_channels {a.mc}, latent {a.side}x{a.side}, UNet batch {a.n}, {a.dtype}: {dt_s * 1e3:.1f} ms "
          f"(forward with tape + backward + AdamW on {len(opt.params)} tensors / {n_par / 1e6:.1f} M parameters), loss {float(loss):.4f}, "
          f"peak memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")


if __name__ == "__main__":
    main()
