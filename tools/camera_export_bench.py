#!/usr/bin/env python3
"""The camera export against what it replaces, and one test-bench batch by stage (profiles/camera_export.txt).

    python tools/camera_export_bench.py [--out profiles/camera_export.txt] [--skip-batch | --only-batch]

1. `mobi_camera_export` (frames on / off) for 8 objects, 900 x 1600 frames, 512 x 512 patches, against the per-sample path:
   8 x (mobi_paste_patch, mobi_gaussian_blur, mobi_blend_frame) plus the torch form of the four pictures that had no kernel (the
   rounded crop window, the resized ground-truth patch, the object crop resized to 224 x 224 with F.interpolate -- not OpenCV's
   integer resize, which torch lacks -- and the un-normalised reference image).  Device events around a replayed graph of 20 calls,
   median of 10, inputs warmed, the sides alternating in one process.  The byte floor of frames on is one read of image and mask and
   one write of the uint8 frame per object, at the bandwidth `mobi_drop_context` reaches in the same run.  The same launch in
   copy-paste mode (`mobi_camera_copy_paste`, frames on / off) alternates with them; its bar is the export with frames on.
2. The wall clock of one batch of `python -m mobi_amd.bench_tree` at mobi_nusc_512 (8 objects, PLMS-50, scale 5, both save flags) on
   a synthetic database, by stage (`--timing`: a synchronise after every stage), in three variants on one model: without the
   lidar-on-camera overlays (`--no_overlays`) and with them, alternating twice, then one copy-paste batch
   (`python -m mobi_amd.copy_paste`: one sampling step), then six copy-paste batches in a row with every lap printed: whether the
   writer's `put` ever waits shows only in a run longer than its queue is deep.  (profiles/camera_copy_paste.txt)
"""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mobi_amd                                              # noqa: E402
from mobi_amd import ops                                     # noqa: E402
from mobi_amd.ldm.data import utils as du                    # noqa: E402

CALLS, REPS = 20, 10


def graph_of(fn):
    """fn CALLS times in one graph (after warm-up calls on a side stream, as capture wants)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            keep = fn()
    return g, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-batch", action="store_true")
    ap.add_argument("--only-batch", action="store_true")
    a = ap.parse_args()
    mobi_amd.set_engine_dtype(torch.float16)

    def say(s=""):
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")
    if a.only_batch:
        return batch_by_stage(say)
    B, H, W, S = 8, 900, 1600, 512
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: (torch.rand(*shape, device="cuda", generator=g) * 2 - 1).contiguous()
    patch_pred, patch_gt, image, ref = rnd(B, 3, S, S), rnd(B, 3, S, S), rnd(B, 3, H, W), rnd(B, 3, 224, 224) * 1.5
    rs = np.random.RandomState(0)
    crops, boxes = [], []
    mask = torch.ones(B, H, W, device="cuda")
    for b in range(B):
        cw = ch = int(rs.randint(200, 640))
        left, top = int(rs.randint(0, W - cw)), int(rs.randint(0, H - ch))
        crops.append((left, top, cw, ch))
        y1, y2, x1, x2 = top + ch // 4, top + 3 * ch // 4, left + cw // 4, left + 3 * cw // 4
        mask[b, y1:y2 + 1, x1:x2 + 1] = 0
        boxes.append((y1, y2, x1, x2))
    taps = torch.from_numpy(du.gaussian_kernel1d(15, 7.0)).cuda()

    def replaced():
        out = []
        for b, (left, top, cw, ch) in enumerate(crops):
            frame = torch.zeros((H, W, 3), device="cuda", dtype=torch.uint8)
            ops.paste_patch(patch_pred[b], frame, top, left, ch, cw)
            recon = ops.blend_frame(ops.gaussian_blur(mask[b], taps), image[b], frame)
            y1, y2, x1, x2 = boxes[b]
            u8 = lambda x: (((x + 1.0) / 2.0) * 255).clamp(0, 255).to(torch.uint8)
            out.append((recon[top:top + ch, left:left + cw].round().clamp(0, 255).to(torch.uint8),
                        u8(F.interpolate(patch_gt[b:b + 1], (ch, cw), mode="bilinear")[0].permute(1, 2, 0)),
                        F.interpolate(frame[y1:y2, x1:x2].permute(2, 0, 1)[None].float(), (224, 224), mode="bilinear").to(torch.uint8),
                        (du.un_norm_clip(ref[b:b + 1], size=(224, 224))[0].permute(1, 2, 0) * 255).clamp(0, 255).to(torch.uint8), recon))
        return out

    gt, inpaint = rnd(B, 3, H, W), rnd(B, 3, H, W)
    flags = torch.ones(B, dtype=torch.int32, device="cuda")
    sides = {"export, frames on": lambda: ops.camera_export(patch_pred, patch_gt, ref, image, mask, crops, taps, frames=True),
             "export, frames off": lambda: ops.camera_export(patch_pred, patch_gt, ref, image, mask, crops, taps, frames=False),
             "copy-paste, frames on": lambda: ops.camera_export(patch_pred, patch_gt, ref, image, mask, crops, None, frames=True,
                                                                copy_paste=True),
             "copy-paste, frames off": lambda: ops.camera_export(patch_pred, patch_gt, ref, image, mask, crops, None, frames=False,
                                                                 copy_paste=True),
             "replaced: 8 x paste_camera_patch + torch pictures": replaced,
             "mobi_drop_context [8, 3, 900, 1600]": lambda: ops.drop_context(gt, inpaint, mask[:, None], flags)}
    graphs = {k: graph_of(fn) for k, fn in sides.items()}
    times = {k: [] for k in sides}
    for _ in range(REPS):
        for k, (gr, _) in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / CALLS)
    med = {k: statistics.median(v) for k, v in times.items()}
    dc_bytes = B * H * W * 4 * (3 * 3 + 1)                   # per channel: gt read and written, inpaint written; the mask read once
    bw = dc_bytes / (med["mobi_drop_context [8, 3, 900, 1600]"] * 1e-3)
    floor_bytes = B * H * W * (3 * 4 + 4 + 3)
    say(f"== camera export: {B} objects, {H} x {W} frames, {S} x {S} patches, crops {[c[2] for c in crops]}; {torch.cuda.get_device_name(0)}; "
        f"device events around a replayed graph of {CALLS} calls, median of {REPS}, sides alternating; ms per call")
    for k, v in med.items():
        say(f"   {k:52s} {v:9.4f}   (min {min(times[k]):.4f}, max {max(times[k]):.4f})")
    say(f"   mobi_drop_context moves {dc_bytes / 1e6:.0f} MB: {bw / 1e12:.2f} TB/s")
    say(f"   byte floor of frames on: {floor_bytes / 1e6:.0f} MB at that bandwidth = {floor_bytes / bw * 1e3:.4f} ms; "
        f"export, frames on is {med['export, frames on'] / (floor_bytes / bw * 1e3):.2f} x the floor")
    say(f"   export, frames on / replaced = {med['export, frames on'] / med['replaced: 8 x paste_camera_patch + torch pictures']:.3f}; "
        f"frames off / replaced = {med['export, frames off'] / med['replaced: 8 x paste_camera_patch + torch pictures']:.3f}")
    say(f"   copy-paste, frames on / export, frames on = {med['copy-paste, frames on'] / med['export, frames on']:.3f}; "
        f"frames off / export, frames off = {med['copy-paste, frames off'] / med['export, frames off']:.3f}")
    if not a.skip_batch:
        batch_by_stage(say)
    say()


def batch_by_stage(say):
    from bench import build_model
    from mobi_amd import copy_paste as cp
    from mobi_amd import bench_tree as bt
    from mobi_amd import test_bench as tb
    from mobi_amd.ldm.util import load_config
    from tests import mini_db
    tmp = tempfile.mkdtemp(prefix="camera_export_bench")
    csv, pkl = mini_db.build(os.path.join(tmp, "db"), n_scenes=16, image_hw=(900, 1600))
    data = "data.params.test.params."
    overrides = ["model.params.lidar_stage_config.params.ckpt_path=null", "ref_mode=id-ref", "classes=[car]", f"{data}object_database_path={csv}",
                 f"{data}scene_database_path={pkl}", f"{data}num_samples_per_class=16", f"{data}min_lidar_points=8"]
    config_path = os.path.join(ROOT, "configs", "mobi_nusc_512.yaml")
    model = build_model("mobi_nusc_512").cuda().eval()
    common = ["--plms", "--ddim_steps", "50", "--scale", "5", "--n_samples", "8", "--n_workers", "0", "--save_samples",
              "--save_visualisations", "--timing"]
    say("-- one test-bench batch at mobi_nusc_512 (random weights, synthetic database, 8 objects, PLMS-50, scale 5, --save_samples "
        "--save_visualisations, 900 x 1600 frames), wall clock by stage, ms; 2 batches per run, the first of the first run includes "
        "graph capture; the runs in this order on one model")
    variants = [("without overlays (--no_overlays)", bt.build_parser().parse_args, ["--no_overlays"]),
                ("with overlays", bt.build_parser().parse_args, [])] * 2 + [("copy-paste (one step), with overlays", cp.parse, [])]
    at_the_end = "waiting for the writer at the end"                     # (once per run, not a stage of a batch)
    for k, (name, parse, extra) in enumerate(variants):
        opt = parse(["--outdir", os.path.join(tmp, f"out{k}")] + common + extra)
        tb.seed_everything(opt.seed)
        spent = bt.run(opt, load_config(config_path, overrides), model)
        say(f"   run {k + 1}: {name}")
        for stage, laps in spent.items():
            say(f"      {stage:36s} first {1e3 * laps[0]:9.1f}   last {1e3 * laps[-1]:9.1f}")
        whole = sum(stage_laps[-1] for stage, stage_laps in spent.items() if stage != at_the_end)
        say(f"      a whole batch (the last)             {1e3 * whole:9.1f}")
    # does `put` ever wait?  Two batches against a queue two batches deep cannot show it: six copy-paste batches, every lap printed
    csv, pkl = mini_db.build(os.path.join(tmp, "db48"), n_scenes=48, image_hw=(900, 1600))
    long_run = [o for o in overrides if "database_path" not in o and "num_samples_per_class" not in o]
    long_run += [f"{data}object_database_path={csv}", f"{data}scene_database_path={pkl}", f"{data}num_samples_per_class=48"]
    opt = cp.parse(["--outdir", os.path.join(tmp, "out_long")] + common)
    tb.seed_everything(opt.seed)
    spent = bt.run(opt, load_config(config_path, long_run), model)
    n = len(spent["sampling"])
    say(f"   run {len(variants) + 1}: copy-paste (one step), with overlays, {n} batches of 8 objects; every batch, ms")
    for stage, laps in spent.items():
        say(f"      {stage:36s} " + " ".join(f"{1e3 * t:8.1f}" for t in laps))


if __name__ == "__main__":
    main()
