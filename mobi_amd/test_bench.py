"""The test bench: `python -m mobi_amd.test_bench --config C --ckpt K --outdir OUT [--plms | --dpm] [--save_samples]
[--save_visualisations] [key=value ...]` samples every object of the test split and writes the result tree the realism metrics
read (`python -m mobi_amd.realism lpips|clip|fid|frd`).

Command line and tree are those of the reference's scripts/inference_test_bench.py (written from its behaviour, none of its text):
    OUT/samples_seed{s}/<camera file_name>, <lidar file_name>.npy            the edited frame and point cloud [N, 5]
    OUT/camera/{object_pred,object_ref,patch_gt,patch_pred}/{id}_..._seed{s}.png
    OUT/lidar/{range_pred,range_orig}/{id}_range_..._seed{s}.npy             [4, H0, W0] = depth, intensity, pitch, yaw
    OUT/camera/grid, OUT/lidar/{point_clouds,range_depth_*,range_intensity_*}  pictures (--save_visualisations)
    OUT/metrics.csv                                                          mean lidar error scores
Every stage runs on the engine: the camera pictures of a batch are one `mobi_camera_export` launch and one read-back
(`du.export_camera_batch`), the range-view paste one `mobi_range_paste` launch (`du.paste_range_objects`).  Files are encoded by a
small pool of threads while the next batch samples.  One process, one GPU.  `--copy-paste` (the reference's baseline row) and its
lidar-on-camera overlays are not offered.
"""
import argparse
import csv
import os
import random
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

CAMERA_SAMPLE_FOLDERS = {"object_pred": "object_pred", "object_ref": "object_ref", "patch_gt": "gt", "patch_pred": "pred"}


def build_parser():
    """The reference's flags with its defaults; those it parses and never uses are accepted and ignored."""
    ap = argparse.ArgumentParser(prog="python -m mobi_amd.test_bench")
    ap.add_argument("--prompt", type=str, nargs="?", default="a photograph of an astronaut riding a horse", help="ignored")
    ap.add_argument("--outdir", type=str, nargs="?", default="outputs/txt2img-samples", help="folder the result tree is written to")
    ap.add_argument("--skip_grid", action="store_true", help="ignored")
    ap.add_argument("--skip_save", action="store_true", help="ignored")
    ap.add_argument("--ddim_steps", type=int, default=50, help="number of sampling steps")
    ap.add_argument("--plms", action="store_true", help="PLMS sampling")
    ap.add_argument("--dpm", action="store_true", help="DPM-Solver++(2M) sampling")
    ap.add_argument("--fixed_code", action="store_true", help="the same starting noise for every batch")
    ap.add_argument("--ddim_eta", type=float, default=0.0)
    ap.add_argument("--n_iter", type=int, default=2, help="ignored")
    ap.add_argument("--n_samples", type=int, default=4, help="batch size")
    ap.add_argument("--n_workers", type=int, default=4, help="DataLoader workers")
    ap.add_argument("--n_rows", type=int, default=0, help="ignored")
    ap.add_argument("--scale", type=float, default=1, help="classifier-free guidance scale")
    ap.add_argument("--from-file", type=str, help="ignored")
    ap.add_argument("--config", type=str, default="", help="the model's YAML config")
    ap.add_argument("--ckpt", type=str, default="", help="checkpoint holding `state_dict`")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--rank", type=int, default=0, help="ignored")
    ap.add_argument("--precision", type=str, choices=["full", "autocast"], default="autocast", help="ignored: see --dtype")
    ap.add_argument("--rotation_test", action="store_true", help="the rotation_test split, re-seeded per batch")
    ap.add_argument("--save_samples", action="store_true")
    ap.add_argument("--save_visualisations", action="store_true")
    ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16", help="engine storage type")
    ap.add_argument("--timing", action="store_true", help="print the wall clock per stage (synchronises after every stage)")
    ap.add_argument("overrides", nargs=argparse.REMAINDER, help="dot-list overrides of the config")
    return ap


def seed_everything(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


# --------------------------------------------------------------------------------------
# files
# --------------------------------------------------------------------------------------
def write_file(path, payload):
    """.npy: np.save; .png: PIL's defaults; .jpg / .jpeg: quality 95 (OpenCV's default).  payload: an array, or a callable making it
    (host work that belongs on a writer thread).  Pictures are HWC uint8 in RGB order, or HW / HW1 grey."""
    arr = payload() if callable(payload) else payload
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        with open(path, "wb") as f:
            np.save(f, arr)
        return
    from PIL import Image
    arr = np.ascontiguousarray(arr)
    if arr.ndim == 3 and arr.shape[2] == 1:
        arr = arr[:, :, 0]
    if ext in (".jpg", ".jpeg"):
        Image.fromarray(arr).save(path, quality=95)
    else:
        Image.fromarray(arr).save(path)


class TreeWriter:
    """Writes batch k's files while batch k + 1 samples: `put` takes one batch's (path, payload) jobs and blocks once `depth`
    batches are unfinished; a fixed pool of at most 8 threads encodes them; `wait` joins and re-raises the first error."""

    def __init__(self, threads=4, depth=2):
        self._pool = ThreadPoolExecutor(max_workers=max(1, min(8, int(threads))))
        self._slots = threading.BoundedSemaphore(depth)
        self._lock = threading.Lock()
        self._error = None
        self._last = {}                                     # path -> the future of the last job that writes it

    def put(self, jobs):
        jobs = list(jobs)
        if not jobs:
            return
        self._slots.acquire()
        left = [len(jobs)]

        def run(job, earlier):
            try:
                if earlier is not None:                     # two objects of one scene edit the same frame: the later one's file stays,
                    earlier.result()                        # as in the reference (the pool is first in, first out: no deadlock)
                if self._error is None:
                    write_file(*job)
            except BaseException as e:                      # noqa: BLE001 (kept for `wait`)
                with self._lock:
                    self._error = self._error or e
            finally:
                with self._lock:
                    left[0] -= 1
                    last = left[0] == 0
                if last:
                    self._slots.release()
        for job in jobs:
            self._last[job[0]] = self._pool.submit(run, job, self._last.get(job[0]))

    def wait(self):
        self._pool.shutdown(wait=True)
        if self._error is not None:
            raise self._error


def camera_sample_jobs(outdir, seed, ids, file_names, pictures):
    """pictures: `du.export_camera_batch`'s list of dicts (RGB)."""
    jobs = []
    for id_, file_name, pic in zip(ids, file_names, pictures):
        jobs.append((os.path.join(outdir, f"samples_seed{seed}", file_name), pic["frame"]))
        for name, tag in CAMERA_SAMPLE_FOLDERS.items():
            jobs.append((os.path.join(outdir, "camera", name, f"{id_}_{tag}_seed{seed}.png"), pic[name]))
    return jobs


def edited_point_cloud(depth, intensity, pitch, yaw):
    """[N, 5] = xyz, intensity, beam index of the valid pixels of one edited range view."""
    from .ldm.data.lidar_converter import LidarConverter
    xyz, inten, beam = LidarConverter().range2pcd(depth, pitch, yaw, intensity)
    return np.concatenate([xyz, inten[:, None], beam[:, None]], axis=1)


def lidar_sample_jobs(outdir, seed, ids, file_names, range_pred, range_orig):
    """range_pred / range_orig: [B, 4, H0, W0] = depth, intensity, pitch, yaw; the point cloud is made on the writer's thread."""
    jobs = []
    for i, (id_, file_name) in enumerate(zip(ids, file_names)):
        jobs.append((os.path.join(outdir, "lidar", "range_pred", f"{id_}_range_pred_seed{seed}.npy"), range_pred[i]))
        jobs.append((os.path.join(outdir, "lidar", "range_orig", f"{id_}_range_orig_seed{seed}.npy"), range_orig[i]))
        name = file_name if file_name.endswith(".npy") else file_name + ".npy"
        jobs.append((os.path.join(outdir, f"samples_seed{seed}", name), lambda v=range_pred[i]: edited_point_cloud(*v)))
    return jobs


def camera_vis_jobs(outdir, seed, ids, preds, preds_no_box):
    """preds / preds_no_box: uint8 [B, 3, Hg, W] collages; side by side."""
    return [(os.path.join(outdir, "camera", "grid", f"{id_}_grid_seed{seed}.jpg"),
             np.concatenate([preds[i].transpose(1, 2, 0), preds_no_box[i].transpose(1, 2, 0)], axis=1)) for i, id_ in enumerate(ids)]


def collage_u8(x):
    """fp32 [B, 1, 5 base, base] range collage -> uint8 [B, 5 base, base], numpy's ((x + 1) / 2 * 255).astype(uint8)."""
    return ((np.asarray(x, dtype=np.float32)[:, 0] + 1.0) / 2.0 * 255).astype(np.uint8)


def magma(grey):
    from matplotlib import cm                               # (lazily: matplotlib is only needed with --save_visualisations)
    return (cm.magma(grey / 255)[:, :, :3] * 255).astype(np.uint8)


def lidar_vis_jobs(outdir, seed, ids, point_clouds, depth, intensity):
    """point_clouds: uint8 [B, 3, H, W] or None; depth / intensity: `collage_u8` results.  Rows [3 base, 4 base) hold the sample, rows
    [0, base) the target."""
    jobs = []
    lid = os.path.join(outdir, "lidar")
    for i, id_ in enumerate(ids):
        if point_clouds is not None:
            jobs.append((os.path.join(lid, "point_clouds", f"{id_}_grid_pc_seed{seed}.jpg"), point_clouds[i].transpose(1, 2, 0)))
        for kind, col in (("depth", depth[i]), ("intensity", intensity[i])):
            base = col.shape[1]
            whole = (lambda c=col: magma(c)) if kind == "depth" else col
            jobs.append((os.path.join(lid, f"range_{kind}_collage", f"{id_}_grid_{kind}_seed{seed}.jpg"), whole))
            jobs.append((os.path.join(lid, f"range_{kind}_pred", f"{id_}_seed{seed}.png"), col[3 * base:4 * base]))
            jobs.append((os.path.join(lid, f"range_{kind}_target", f"{id_}_seed{seed}.png"), col[:base]))
    return jobs


def write_metrics_csv(outdir, metrics):
    """{score name: [values]} -> metrics.csv as pandas.DataFrame({"mse": {...}, "median_error": {...}}).to_csv lays it out: the
    means of the values per score, rows named by the score's last path component."""
    table = {"mse": {}, "median_error": {}}
    for name, values in metrics.items():
        mean = float(np.mean(values)) if len(values) else float("nan")
        for column in table:
            if column in name:
                table[column][name.split("/")[-1]] = mean
                break
    rows = list(table["mse"]) + [k for k in table["median_error"] if k not in table["mse"]]
    cell = lambda v: "" if v is None or v != v else repr(v)
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, "metrics.csv"), "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["", "mse", "median_error"])
        for r in rows:
            w.writerow([r, cell(table["mse"].get(r)), cell(table["median_error"].get(r))])


# --------------------------------------------------------------------------------------
# the loop
# --------------------------------------------------------------------------------------
def _to_device(batch, device):
    return {k: _to_device(v, device) if isinstance(v, dict) else (v.to(device) if isinstance(v, torch.Tensor) else v)
            for k, v in batch.items()}


class _Clock:
    def __init__(self, on):
        self.on, self.t, self.spent = on, 0.0, {}

    def start(self):
        import time
        if self.on:
            torch.cuda.synchronize()
            self.t = time.perf_counter()

    def lap(self, name):
        import time
        if self.on:
            torch.cuda.synchronize()
            now = time.perf_counter()
            self.spent.setdefault(name, []).append(now - self.t)
            self.t = now


def load_model(config, ckpt):
    from .ldm.util import instantiate_from_config
    sd = torch.load(ckpt, map_location="cpu")
    model = instantiate_from_config(config["model"])
    model.load_state_dict(sd["state_dict"], strict=False)
    return model.cuda().eval()


def main(argv=None):
    opt = build_parser().parse_args(argv)
    if opt.plms and opt.dpm:
        raise SystemExit("--plms and --dpm exclude each other")
    import mobi_amd
    from .ldm.util import load_config
    mobi_amd.set_engine_dtype({"fp16": torch.float16, "bf16": torch.bfloat16}[opt.dtype])
    seed_everything(opt.seed)
    config = load_config(opt.config, [o for o in opt.overrides if o != "--"])
    spent = run(opt, config)
    for name, laps in spent.items():
        print(f"{name}: median {1e3 * float(np.median(laps)):.1f} ms over {len(laps)} batches")
    print(f"The result tree is in {opt.outdir}")


def run(opt, config, model=None):
    """The loop of `main` for parsed options and a loaded config; model: built and on the device already (tools), else loaded from
    opt.ckpt.  Returns the wall clock per stage and batch in seconds (empty without opt.timing)."""
    from .ldm.data import utils as du
    from .ldm.models.diffusion.ddim import DDIMSampler
    from .ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from .ldm.models.diffusion.plms import PLMSSampler
    from .ldm.util import instantiate_from_config
    split = config["data"]["params"]["rotation_test" if opt.rotation_test else "test"]
    split["params"]["return_original_image"] = opt.save_samples
    dataset = instantiate_from_config(split)
    loader = torch.utils.data.DataLoader(dataset, batch_size=opt.n_samples, num_workers=opt.n_workers, pin_memory=True,
                                         shuffle=False, drop_last=False)
    model = load_model(config, opt.ckpt) if model is None else model
    sampler = (PLMSSampler if opt.plms else DPMSolverSampler if opt.dpm else DDIMSampler)(model)
    outdir, seed = opt.outdir, opt.seed
    for d in ("lidar", "camera", f"samples_seed{seed}"):
        os.makedirs(os.path.join(outdir, d), exist_ok=True)
    shape = [model.channels, model.image_size, model.image_size]
    start_code = torch.randn([opt.n_samples, *shape], device="cuda") if opt.fixed_code else None
    writer, clock, metrics = TreeWriter(threads=4, depth=2), _Clock(opt.timing), {}
    with torch.no_grad(), model.ema_scope():
        for cpu_batch in loader:
            if opt.rotation_test:
                seed_everything(seed)                       # (the starting noise decides much of a sample: the same for every angle)
            ids = list(cpu_batch["id_name"])
            clock.start()
            batch = _to_device(cpu_batch, "cuda")
            data = model.get_input(batch, model.first_stage_key, force_c_encode=True, return_vae_rec=True)
            n = data["z"].shape[0]
            clock.lap("get_input")
            uc = None
            if opt.scale != 1.0:
                uc = [model.learnable_vector.repeat(n, 1, 1)]
                if "ref_bbox" in model.cond_stage_key:
                    uc.append(model.bbox_uncond_vector.repeat(n, 1, 1))
                uc = torch.cat(uc, dim=1)
            common = dict(S=opt.ddim_steps, conditioning=data["cond"], batch_size=n, shape=shape, verbose=False,
                          unconditional_guidance_scale=opt.scale, unconditional_conditioning=uc, eta=opt.ddim_eta, x_T=start_code)
            if opt.plms:
                samples, _ = sampler.sample(inpaint_image=data["z"][:, 4:8], inpaint_mask=data["z"][:, [8]], **common)
            else:
                samples, _ = sampler.sample(test_model_kwargs={"inpaint_image": data["z"][:, 4:8], "inpaint_mask": data["z"][:, [8]]},
                                            **common)
            clock.lap("sampling")
            h_camera, h_lidar = model.decode_sample(samples, data.get("z_lidar"))
            log, lidar_metrics = model.log_data(batch, data, h_camera, h_lidar, log_metrics=False, return_sample=opt.save_samples,
                                                split="test")
            clock.lap("decode + log_data")
            count = len(batch["bbox_3d"])
            jobs = []
            if model.use_camera:
                if opt.save_samples:
                    orig = batch["image"]["orig"]
                    pictures = du.export_camera_batch(patch_pred=log["image_sample"], patch_gt=batch["image"]["GT"],
                                                      ref_image=batch["image"]["cond"]["ref_image"], image=orig["image"],
                                                      mask=orig["mask"], crop=cpu_batch["image"]["orig"]["crop"], frames=True)
                    jobs += camera_sample_jobs(outdir, seed, ids, list(orig["file_name"]), pictures)
                if opt.save_visualisations:
                    jobs += camera_vis_jobs(outdir, seed, ids, log["image_preds"].cpu().numpy(), log["image_preds_no_box"].cpu().numpy())
            if model.use_lidar:
                lid = batch["lidar"]
                if opt.save_samples:
                    out = du.paste_range_objects(range_depth=log["range_sample_depth"], range_int=log["range_sample_int"],
                                                 range_depth_orig=lid["range_depth_orig"], range_int_orig=lid["range_int_orig"],
                                                 crop_left=lid["range_shift_left"], width_crop=lid["width_crop"],
                                                 range_pitch=lid["range_pitch"], range_yaw=lid["range_yaw"], bbox_3d=batch["bbox_3d"],
                                                 gt_instance_mask=lid["range_instance_mask_orig"])
                    f32 = lambda t: t.to("cuda").float()
                    pitch, yaw = f32(lid["range_pitch"]), f32(lid["range_yaw"])
                    both = torch.stack([torch.stack([out["depth_final"], out["int_final"], pitch, yaw], dim=1),
                                        torch.stack([f32(lid["range_depth_orig"]), f32(lid["range_int_orig"]), pitch, yaw], dim=1)])
                    both = both.cpu().numpy()                                   # one read-back: [2, B, 4, H0, W0]
                    jobs += lidar_sample_jobs(outdir, seed, ids, list(lid["file_name"]), both[0], both[1])
                if opt.save_visualisations:
                    pcs = log["lidar_input-pred-rec"].cpu().numpy() if "lidar_input-pred-rec" in log else None
                    jobs += lidar_vis_jobs(outdir, seed, ids, pcs, collage_u8(log["range_depth_pred"].cpu().numpy()),
                                           collage_u8(log["range_int_pred"].cpu().numpy()))
                for k, v in (lidar_metrics or {}).items():                      # (once per object, as the reference weighs a batch)
                    metrics.setdefault(k, []).extend([float(v)] * count if not np.isnan(v) else [])
            clock.lap("export + read-back")
            writer.put(jobs)
            clock.lap("handing over the files")
    clock.start()
    writer.wait()
    clock.lap("waiting for the writer at the end")
    write_metrics_csv(outdir, metrics)
    return clock.spent


if __name__ == "__main__":
    main()
