#!/usr/bin/env python3
"""Time the weight refresh of a training step alone -- informational.

    python tools/repack_bench.py [--config configs/mobi_nusc_512.yaml] [--dtype fp16] [--reps 10] [--rounds 3] [--out profiles/repack_multi.txt]

The full-width UNet on the device (random weights: the kernels' time does not depend on the values) and the list
`train.WeightRefresher` makes of its trained Linear weights.  Median of `--reps` after two warm-up calls, `--rounds` alternating
rounds in one process of
  (a) `mobi_repack_multi`: every 16-bit image of every listed weight in one launch (device events);
  (b) what it replaces: `weights_changed` + one `packed()` / `_packed_t()` of every listed layer -- per image a cast, an allocation
      and a `mobi_tile_weights` launch -- as device events AND as wall clock ending in a synchronise (its cost is largely host time);
  (c) the bar for a streaming walker on this box in this process: `mobi_accum_multi` ASSIGN over the same masters (8 B / element).
The repack's bytes are computed from the shapes: 4 B read per element plus 2 B per element and image written (12 B where all four
images exist)."""
import argparse
import os
import statistics
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import mobi_amd  # noqa: E402
from mobi_amd import _lib, ops, train  # noqa: E402
from mobi_amd.ldm.modules.diffusionmodules.util import weights_changed  # noqa: E402
from tools.ema_bench import timed  # noqa: E402


def wall(fn, reps):
    for _ in range(2):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(HERE, "configs", "mobi_nusc_512.yaml"))
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
    ap.add_argument("--mc", type=int, default=None, help="narrow the UNet (quick runs)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mobi_amd.set_engine_dtype({"fp16": torch.float16, "bf16": torch.bfloat16}[a.dtype])
    from mobi_amd.ldm.util import instantiate_from_config, load_config
    ucfg = load_config(a.config, ["model.params.lidar_stage_config.params.ckpt_path=null"])["model"]["params"]["unet_config"]
    if a.mc:
        ucfg["params"]["model_channels"] = a.mc
    with torch.device("cuda"):
        net = instantiate_from_config(ucfg)
    names = train.trainable_names(net)
    params = [net.get_parameter(k) for k in names]
    r = train.WeightRefresher(net, names)
    r.refresh()
    table = r.table
    masters = [m.weight.data.reshape(-1) for m, _ in r.layers]
    n = sum(t.numel() for t in masters)
    images = sum(im[k] is not None for im in table.images for k in im)
    nbytes = sum(nk[0] * nk[1] * (4 + 2 * sum(im[k] is not None for k in im)) for nk, im in zip(table.shapes, table.images))
    assign = ops.MultiTensorTable([ops.LIVE, [torch.empty_like(t) for t in masters]])
    assign.set_live(masters)

    def lazy():
        weights_changed(params)
        for m, kind in r.layers:
            if kind == "skinny":
                m.skinny()
                continue
            m.packed()
            if kind == "mfma":
                train._packed_t(m)

    lines = [f"{torch.cuda.get_device_name(0)}; median (min .. max) of {a.reps}; {a.dtype}",
             f"-- trained Linear weights: {len(masters)} tensors, {n / 1e6:.1f} M elements, {images} images, {table.n_tiles} tiles, "
             f"{nbytes / 1e6:.1f} MB moved by the repack = {nbytes / n:.2f} B/element"]
    print("\n".join(lines), flush=True)

    def row(what, stat, nb=None):
        med, lo, hi = stat
        rate = f"  {nb / 1e6:.1f} MB -> {nb / med / 1e9:.2f} TB/s" if nb else ""
        lines.append(f"{what:<58s} {med:8.3f} ms ({lo:.3f} .. {hi:.3f}){rate}")
        print(lines[-1], flush=True)

    for i in range(a.rounds):
        lines.append(f"round {i + 1}")
        row("(a) mobi_repack_multi, device events", timed(lambda: ops.repack_multi(table), a.reps), nbytes)
        row("(b) lazy per-tensor path, device events", timed(lazy, a.reps))
        row("(b) lazy per-tensor path, wall clock + synchronise", wall(lazy, a.reps))
        row("(a) WeightRefresher.refresh(), wall clock + synchronise", wall(r.refresh, a.reps))
        row("(c) mobi_accum_multi (ASSIGN, w = 1), the bar", timed(lambda: ops.accum_multi(assign, 1.0, _lib.MT_ASSIGN), a.reps), 8 * n)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
