#!/usr/bin/env python3
"""What sampling while training costs (train.ImageLogger), on ONE device in ONE process; every figure a median of --reps calls
after a warm-up call.

    python tools/image_logger_bench.py [--workload mobi_nusc_512] [--batch 4] [--ddim-steps 50] [--reps 10] [--out FILE]

1. One `ImageLogger` call in four parts (wall clock, the device drained after each): `get_input` (VAE encodes, CLIP, the two
   reconstructions), the sampling (DDIM, eta 1, under `ema_scope`), `decode_sample` + `log_data`, `ops.image_grid` + the PNG writes;
   the first call (graph capture, weight packing) apart; then the same with `use_ema` (two swaps per call: the packed 16-bit copies
   are rebuilt and the step graph is captured again).  Beside it one training step as tools/train_bench.py --dtype fp16 --scaler
   takes it (forward with tape + backward + `step_scaled`) on the same UNet at the same latent size and UNet batch.
2. `mobi_image_grid` against what it replaces, over the keys of that call's real `log_data` result: the torch composition on the
   device per key (slice, clamp, cat for C = 1, padded canvas copy, rescale, permute, `to(uint8)`, `.cpu()`), the two sides
   alternating, in device events and in wall clock (the point is launches and syncs)."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import mobi_amd  # noqa: E402
from mobi_amd import ops, train  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def make_batch(B, R, seed=0):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    hole = torch.ones(B, 1, R, R)
    hole[:, :, R // 4: 3 * R // 4, R // 4: 3 * R // 4] = 0
    img, rng, ref = u(B, 3, R, R), u(B, 2, R, R), u(B, 3, 224, 224) * 1.5
    b = {"image": {"GT": img, "inpaint_image": img * hole, "inpaint_mask": hole.clone(),
                   "cond": {"ref_image": ref, "ref_bbox": torch.rand(B, 8, 3, generator=g)}},
         "lidar": {"range_data": rng, "range_data_inpaint": rng * hole, "range_mask": hole.clone(),
                   "range_instance_mask": (torch.rand(B, 1, R, R, generator=g) > 0.8).float() * (1 - hole),
                   "min_depth_obj": torch.linspace(-0.8, -0.2, B), "max_depth_obj": torch.linspace(0.1, 0.7, B),
                   "width_crop": torch.full((B,), R // 2, dtype=torch.long),
                   "cond": {"ref_image": ref.clone(), "ref_bbox": torch.rand(B, 8, 3, generator=g)}}}
    move = lambda d: {k: move(v) if isinstance(v, dict) else v.cuda() for k, v in d.items()}
    return move(b)


def clone(x):
    return {k: clone(v) for k, v in x.items()} if isinstance(x, dict) else x.clone()


def one_call(model, logger, batch, steps, split_dir):
    """`ImageLogger.log_img`'s work, part by part -> ({part: ms}, the log dict)."""
    parts = {}
    b = clone(batch)
    data, parts["get_input"] = wall(lambda: model.get_input(b, model.first_stage_key, force_c_encode=True, return_vae_rec=True))

    def sample():
        with model.ema_scope():
            smp, _ = model.sample_log(cond=data["cond"], batch_size=data["z"].shape[0], ddim=True, ddim_steps=steps, eta=1.,
                                      rest=data["z"][:, 4:])
        return smp
    smp, parts["sampling"] = wall(sample)
    (log, _), parts["decode + log_data"] = wall(lambda: model.log_data(b, data, *model.decode_sample(smp, data.get("z_lidar")),
                                                                       log_metrics=True, split="train"))
    _, parts["image_grid + PNG"] = wall(lambda: logger.log_local(split_dir, logger.pictures(log), 0, 0, 0))
    parts["total"] = sum(parts.values())
    return parts, log


def torch_grid(x, max_images, nrow=4, padding=2):
    """What the reference's logger does per key, kept on the device until the final copy."""
    x = x[:max_images]
    if x.dtype != torch.uint8:
        x = x.clamp(-1., 1.)
    if x.shape[1] == 1:
        x = torch.cat([x, x, x], 1)
    n, _, h, w = x.shape
    if n > 1:
        xmaps = min(nrow, n)
        ymaps = -(-n // xmaps)
        canvas = x.new_zeros((3, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding))
        for k in range(n):
            y0, x0 = (k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding
            canvas[:, y0:y0 + h, x0:x0 + w].copy_(x[k])
    else:
        canvas = x[0]
    if canvas.dtype != torch.uint8:
        canvas = ((canvas + 1.0) / 2.0 * 255).to(torch.uint8)
    return canvas.permute(1, 2, 0).cpu().numpy()


def med(xs):
    return statistics.median(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="mobi_nusc_512")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from bench import WORKLOADS, build_model
    mobi_amd.set_engine_dtype(torch.float16)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    side = WORKLOADS[a.workload]["latent"]
    model = build_model(a.workload).cuda()
    batch = make_batch(a.batch, side * 8)
    tmp = tempfile.mkdtemp(prefix="image_logger_bench")
    logger = train.ImageLogger(tmp, max_images=8)
    say(f"== {a.workload}: full width, latent {side} x {side}, {a.batch} objects (UNet batch {2 * a.batch}), DDIM-{a.ddim_steps}, eta 1, fp16; "
        f"{torch.cuda.get_device_name(0)}; medians of {a.reps} after a warm-up call, ms")
    for ema in (False, True):
        if ema:
            from mobi_amd.ldm.modules.ema import LitEma
            model.use_ema, model.model_ema = True, LitEma(model.model).cuda()
        first, log = one_call(model, logger, batch, a.ddim_steps, "train")
        reps = [one_call(model, logger, batch, a.ddim_steps, "train")[0] for _ in range(a.reps)]
        say(f"-- one ImageLogger call, use_ema={ema}" + (" (two swaps: repack + re-capture in every call)" if ema else ""))
        for k in first:
            say(f"   {k:20s} {med([r[k] for r in reps]):9.1f}      first call {first[k]:9.1f}")
    model.use_ema = False
    keys = [k for k, v in log.items() if isinstance(v, torch.Tensor) and v.dim() == 4]
    say("   keys: " + ", ".join(f"{k} {tuple(log[k].shape)} {str(log[k].dtype).replace('torch.', '')}" for k in keys))
    # ---- the training step tools/train_bench.py --dtype fp16 --scaler times, on this UNet
    net, n = model.model.diffusion_model, 2 * a.batch
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(n, 9, side, side, device="cuda", generator=g)
    ctx = torch.randn(n, 2, 768, device="cuda", generator=g)
    noise = torch.randn(n, 4, side, side, device="cuda", generator=g)
    t = torch.full((n,), 500, dtype=torch.long, device="cuda")
    opt = train.AdamW({k: p for k, p in net.named_parameters() if any(m in k for m in train.TRAINABLE_MARKERS)}, lr=1e-5)
    scaler = train.GradScaler()
    scaler.first_use(noise.numel())

    def step():
        with torch.no_grad():
            _, grads = train.loss_and_gradients(net, x, t, ctx, noise, loss_scale=scaler.scale, unscale=False)
            grads.pop("__dcontext__", None)
            opt.step_scaled(grads, scaler=scaler)
    step()
    step_ms = med([wall(step)[1] for _ in range(a.reps)])
    say(f"-- one training step (tools/train_bench.py --dtype fp16 --scaler, this UNet, UNet batch {n}): {step_ms:.1f} ms")
    # ---- mobi_image_grid against the torch composition
    srcs = {k: log[k] for k in keys}
    ev = lambda: torch.cuda.Event(enable_timing=True)
    rows = {"mobi_image_grid": ([], []), "torch composition": ([], [])}
    sides = {"mobi_image_grid": lambda: ops.image_grid(srcs, 8), "torch composition": lambda: {k: torch_grid(v, 8) for k, v in srcs.items()}}
    mine, theirs = sides["mobi_image_grid"](), sides["torch composition"]()
    same = all((mine[k] == theirs[k]).all() for k in keys)
    for _ in range(a.reps):
        for name, fn in sides.items():
            e0, e1 = ev(), ev()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            rows[name][1].append((time.perf_counter() - t0) * 1e3)
            rows[name][0].append(e0.elapsed_time(e1))
    say(f"-- {len(keys)} keys -> uint8 HWC pictures on the host ({sum(v.size for v in mine.values()) / 1e6:.1f} MB), sides alternating; "
        f"pictures equal: {same}")
    for name, (dev, wl) in rows.items():
        say(f"   {name:20s} device events {med(dev):8.3f} ms      wall clock {med(wl):8.3f} ms")
    say()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
