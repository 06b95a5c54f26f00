#!/usr/bin/env python3
"""The lidar-on-camera overlays against their bar and against what they replace on the host (profiles/lidar_overlay.txt).

    python tools/lidar_overlay_bench.py [--out profiles/lidar_overlay.txt] [--skip-host]

1. `mobi_lidar_overlay` (the clear, both launches, the records) for 8 objects = 16 pictures on 900 x 1600 frames: 8 original sweeps on
   fp32 planar frames, 8 edited sweeps on the uint8 frames inside `mobi_camera_export`'s buffer, read in place.  The bar, in the same
   run, is `mobi_camera_export` with frames on (8 frames), per frame byte written.  Device events around a replayed graph of 20
   calls, median of 10, inputs warmed, the sides alternating in one process.  The byte floor is one read of every frame and one
   write of every picture at the bandwidth `mobi_drop_context` reaches in the same run.
2. What the call replaces on the host, per picture on one core: the numpy definition (`du.overlay_lidar_on_image`), and a
   matplotlib (Agg) scatter-and-savefig of the same points at the reference's figure size and dpi (12 x 8 in, dpi 200).
3. The copy of the 16 pictures to pinned host memory that follows the call (`du.overlay_lidar_batch`), by the host's clock around
   a synchronise, median of 10.
"""
import argparse
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

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


def synthetic_sweep(rng, empty=0.2, h0=32, w0=1096):
    """fp32 depth code, pitch, yaw [h0, w0]: nominal beam angles (pitch +10 .. -30 degrees down the rows, yaw pi .. -pi along the
    columns) plus small noise, depth codes uniform, about `empty` of them -1 (no return)."""
    pitch = np.deg2rad(np.linspace(10.0, -30.0, h0))[:, None] + rng.normal(0, 2e-3, (h0, w0))
    yaw = np.linspace(np.pi, -np.pi, w0, endpoint=False)[None, :] + rng.normal(0, 1e-3, (h0, w0))
    code = rng.uniform(-0.95, 1.0, (h0, w0))
    code[rng.uniform(size=(h0, w0)) < empty] = -1.0
    return code.astype(np.float32), pitch.astype(np.float32), yaw.astype(np.float32)


def front_camera(H, W, focal, shift):
    """4 x 4 lidar2image of a pinhole camera looking along +x of the lidar frame, `shift` metres from it, principal point centred."""
    ext = np.eye(4)
    ext[:3, :3] = [[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]            # camera x = right, y = down, z = ahead
    ext[:3, 3] = ext[:3, :3] @ -np.asarray(shift)
    k = np.eye(4)
    k[0, 0] = k[1, 1] = focal
    k[0, 2], k[1, 2] = W / 2.0, H / 2.0
    return k @ ext


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    mobi_amd.set_engine_dtype(torch.float16)

    def say(s=""):
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(s + "\n")
    the_call(say, host=not a.skip_host)
    say()


def the_call(say, host=True):
    B, H, W, S = 8, 900, 1600, 512
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: (torch.rand(*shape, device="cuda", generator=g) * 2 - 1).contiguous()
    patch_pred, patch_gt, image, ref = rnd(B, 3, S, S), rnd(B, 3, S, S), rnd(B, 3, H, W), rnd(B, 3, 224, 224) * 1.5
    rs = np.random.RandomState(0)
    crops = []
    mask = torch.ones(B, H, W, device="cuda")
    for b in range(B):
        cw = ch = int(rs.randint(200, 640))
        left, top = int(rs.randint(0, W - cw)), int(rs.randint(0, H - ch))
        crops.append((left, top, cw, ch))
        mask[b, top + ch // 4:top + 3 * ch // 4 + 1, left + cw // 4:left + 3 * cw // 4 + 1] = 0
    taps = torch.from_numpy(du.gaussian_kernel1d(15, 7.0)).cuda()
    cam_buf, cam_layout = ops.camera_export(patch_pred, patch_gt, ref, image, mask, crops, taps, frames=True)
    # 16 sweeps (original and edited) and a front camera of nuScenes' geometry: focal length 1266 px, the principal point centred
    rng = np.random.default_rng(0)
    host_sweeps = [synthetic_sweep(rng) for _ in range(2 * B)]
    sweeps = [tuple(torch.from_numpy(x).cuda() for x in s) for s in host_sweeps]
    matrices = [front_camera(H, W, 1266.0, shift=(0.5, 0.0, -0.3))] * (2 * B)
    frames = [image[b] for b in range(B)] + [(cam_buf, cam_layout["objects"][b]["frame"][0]) for b in range(B)]
    lut = torch.from_numpy(du.turbo_lut()).cuda()
    gt, inpaint = rnd(B, 3, H, W), rnd(B, 3, H, W)
    flags = torch.ones(B, dtype=torch.int32, device="cuda")
    sides = {"overlay, 16 pictures": lambda: ops.lidar_overlay(sweeps, matrices, frames, lut, H=H, W=W, point_size=3),
             "export, frames on": lambda: ops.camera_export(patch_pred, patch_gt, ref, image, mask, crops, taps, frames=True),
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
    out, layout = graphs["overlay, 16 pictures"][1]
    flat = out.cpu().numpy()
    rec = flat[layout["records"]:layout["bytes"]].view(np.uint32).reshape(2 * B, 4)
    dc_bytes = B * H * W * 4 * (3 * 3 + 1)                   # per channel: gt read and written, inpaint written; the mask read once
    bw = dc_bytes / (med["mobi_drop_context [8, 3, 900, 1600]"] * 1e-3)
    px = H * W
    floor_bytes = B * px * 12 + B * px * 3 + 2 * B * px * 3                       # fp32 frames and uint8 frames in, 16 pictures out
    own_bytes = 2 * B * px * 8                                                    # the keys: cleared, then read
    t_o, t_e = med["overlay, 16 pictures"], med["export, frames on"]
    per_byte = (t_o / (2 * B)) / (t_e / B)
    say(f"== lidar overlay: {B} objects = {2 * B} pictures, {H} x {W} frames, point_size 3, kept points per picture "
        f"{int(rec[:, 2].min())} .. {int(rec[:, 2].max())}; {torch.cuda.get_device_name(0)}; device events around a replayed graph of "
        f"{CALLS} calls, median of {REPS}, sides alternating; ms per call")
    for k, v in med.items():
        say(f"   {k:52s} {v:9.4f}   (min {min(times[k]):.4f}, max {max(times[k]):.4f})")
    say(f"   mobi_drop_context moves {dc_bytes / 1e6:.0f} MB: {bw / 1e12:.2f} TB/s")
    say(f"   overlay / export, frames on = {t_o / t_e:.3f} per call; per frame byte written (16 pictures against 8 frames) = {per_byte:.3f}")
    say(f"   every side replays the same inputs {CALLS} x {REPS} times (a captured call takes its output and workspace from the graph's "
        f"pool as the call before it returns them): steady state, not cold, and not cache-resident either -- the last-level cache "
        f"holds 256 MiB.  Per call the overlay touches "
        f"{(floor_bytes + own_bytes // 2) / 1e6:.0f} MB of distinct memory (frames, pictures, keys), the export about "
        f"{B * px * (12 + 4 + 3) / 1e6:.0f} MB, mobi_drop_context {B * px * 4 * 7 / 1e6:.0f} MB")
    say(f"   byte floor of the 16 pictures: {floor_bytes / 1e6:.0f} MB (frames in, pictures out) at that bandwidth = "
        f"{floor_bytes / bw * 1e3:.4f} ms; the overlay is {t_o / (floor_bytes / bw * 1e3):.2f} x the floor; its own key traffic "
        f"(cleared, then read) is another {own_bytes / 1e6:.0f} MB")
    depth, pitch, yaw = (torch.stack([sw[k] for sw in sweeps]) for k in range(3))
    f32 = [image[b] for b in range(B)] + [None] * B
    u8 = (cam_buf, [None] * B + [cam_layout["objects"][b]["frame"][0] for b in range(B)])
    whole = []
    for _ in range(REPS + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        du.overlay_lidar_batch(depth=depth, pitch=pitch, yaw=yaw, lidar2image=np.stack(matrices), frames_f32=f32, frames_u8=u8)
        whole.append(time.perf_counter() - t0)
    say(f"-- du.overlay_lidar_batch, the call and the copy of {layout['bytes'] / 1e6:.0f} MB into pinned host memory, host clock, "
        f"median of {REPS} after 2 warm-up calls: {1e3 * statistics.median(whole[2:]):.1f} ms")
    if not host:
        return
    # what the call replaces on the host, on one core
    from mobi_amd.ldm.data.lidar_converter import LidarConverter
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    affinity = os.sched_getaffinity(0)
    os.sched_setaffinity(0, {min(affinity)})
    torch.set_num_threads(1)
    try:
        frame = np.ascontiguousarray(flat[:px * 3].reshape(H, W, 3))
        t_np, t_mpl = [], []
        for k in range(3):
            points = LidarConverter().range2pcd(*host_sweeps[k])[0]
            t0 = time.perf_counter()
            du.overlay_lidar_on_image(points, matrices[k], frame, point_size=3)
            t_np.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            m = np.asarray(matrices[k])
            q = np.concatenate([points, np.ones((len(points), 1), dtype=np.float32)], axis=1) @ m.T
            q = q[q[:, 2] > 0]
            zc = np.clip(q[:, 2], 1e-5, 1e5)
            u, v = q[:, 0] / zc, q[:, 1] / zc
            ok = (u >= 0) & (u < W) & (v >= 0) & (v < H)
            fig, ax = plt.subplots(figsize=(12, 8))
            ax.imshow(frame)
            ax.scatter(u[ok], v[ok], c=zc[ok], s=2, cmap="turbo")
            ax.axis("off")
            fig.savefig(io.BytesIO(), format="png", bbox_inches="tight", dpi=200)
            plt.close(fig)
            t_mpl.append(time.perf_counter() - t0)
    finally:
        os.sched_setaffinity(0, affinity)
    say(f"-- on the host, one core, per picture, median of 3: the numpy definition {1e3 * statistics.median(t_np):.1f} ms; a matplotlib "
        f"(Agg) scatter + savefig at 12 x 8 in, dpi 200 {1e3 * statistics.median(t_mpl):.1f} ms (PNG encoding of the figure included); "
        f"the engine call is {t_o / (2 * B):.4f} ms per picture before its read-back")


if __name__ == "__main__":
    main()
