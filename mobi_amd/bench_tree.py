"""The test bench with everything the reference's scripts/inference_test_bench.py writes: `python -m mobi_amd.bench_tree` takes the
arguments of `python -m mobi_amd.test_bench` and writes its result tree plus the lidar-on-camera overlays,
    OUT/lidar/overlay_orig/{id}.png      the original sweep on the original frame
    OUT/lidar/overlay_pred/{id}.png      the edited sweep on the recomposed frame
with `--save_samples` when the model has both camera and lidar, as the reference does; `--no_overlays` skips them (and keeps
matplotlib, whose `turbo` table colours them, out of the run).  The 2B overlays of a batch are ONE `mobi_lidar_overlay` call
(`du.overlay_lidar_batch`) after the range paste: the original sweep on `orig["image"]`, the edited sweep on the recomposed frame,
read in place from the camera export's device buffer.  They are drawn at the frame's own resolution, not as matplotlib's figure.

This module is also the loop of the copy-paste baseline (`python -m mobi_amd.copy_paste`, the reference's `--copy-paste`): `run`
hands `opt.copy_paste` to the camera export (`mobi_camera_copy_paste`), and the overlays are then drawn on the copy-paste frame.
scripts/inference_test_bench.py, the path the reference's shell drivers call, is a shim onto the two commands.

`mobi_amd/test_bench.py` is kept as it is -- its parser, its file jobs, its writer and its clock are used from here -- and its own
command writes the tree without the overlays, as before.
"""
import os

import numpy as np
import torch

from . import test_bench as tb


def build_parser():
    """`test_bench.build_parser()` (the reference's command line, which stays without `--copy-paste`) and `--no_overlays`."""
    ap = tb.build_parser()
    ap.prog = "python -m mobi_amd.bench_tree"
    ap.add_argument("--no_overlays", action="store_true", help="with --save_samples: skip lidar/overlay_orig and lidar/overlay_pred")
    return ap


def overlay_jobs(outdir, ids, overlay_orig, overlay_pred):
    """overlay_orig / overlay_pred: per object a uint8 [H, W, 3] picture (`du.overlay_lidar_batch`).  No seed in the name, as in the
    reference; two objects of one scene keep their own files."""
    jobs = []
    for id_, orig, pred in zip(ids, overlay_orig, overlay_pred):
        jobs.append((os.path.join(outdir, "lidar", "overlay_orig", f"{id_}.png"), orig))
        jobs.append((os.path.join(outdir, "lidar", "overlay_pred", f"{id_}.png"), pred))
    return jobs


def main(argv=None):
    run_command(build_parser().parse_args(argv))


def run_command(opt):
    """`main` for parsed options (`python -m mobi_amd.copy_paste` adds its own to them): what `test_bench.main` does around its loop."""
    if opt.plms and opt.dpm:
        raise SystemExit("--plms and --dpm exclude each other")
    import mobi_amd
    from .ldm.util import load_config
    mobi_amd.set_engine_dtype({"fp16": torch.float16, "bf16": torch.bfloat16}[opt.dtype])
    tb.seed_everything(opt.seed)
    config = load_config(opt.config, [o for o in opt.overrides if o != "--"])
    spent = run(opt, config)
    for name, laps in spent.items():
        print(f"{name}: median {1e3 * float(np.median(laps)):.1f} ms over {len(laps)} batches")
    print(f"The result tree is in {opt.outdir}")


def run(opt, config, model=None):
    """`test_bench.run` with the overlays and the baseline: the loop for parsed options and a loaded config; model: built and on the
    device already (tools), else loaded from opt.ckpt.  opt.copy_paste (set by `python -m mobi_amd.copy_paste`, no flag) goes to the
    camera export; nothing else in the loop differs for it.  Returns the wall clock per stage and batch in seconds (empty without
    opt.timing)."""
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
    model = tb.load_model(config, opt.ckpt) if model is None else model
    copy_paste = bool(getattr(opt, "copy_paste", False))
    overlays = opt.save_samples and model.use_camera and model.use_lidar and not getattr(opt, "no_overlays", False)
    sampler = (PLMSSampler if opt.plms else DPMSolverSampler if opt.dpm else DDIMSampler)(model)
    outdir, seed = opt.outdir, opt.seed
    for d in ("lidar", "camera", f"samples_seed{seed}"):
        os.makedirs(os.path.join(outdir, d), exist_ok=True)
    shape = [model.channels, model.image_size, model.image_size]
    start_code = torch.randn([opt.n_samples, *shape], device="cuda") if opt.fixed_code else None
    writer, clock, metrics = tb.TreeWriter(threads=4, depth=2), tb._Clock(opt.timing), {}
    with torch.no_grad(), model.ema_scope():
        for cpu_batch in loader:
            if opt.rotation_test:
                tb.seed_everything(seed)                    # (the starting noise decides much of a sample: the same for every angle)
            ids = list(cpu_batch["id_name"])
            clock.start()
            batch = tb._to_device(cpu_batch, "cuda")
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
                    pictures, frames_buf, layout = du.export_camera_batch(
                        patch_pred=log["image_sample"], patch_gt=batch["image"]["GT"], ref_image=batch["image"]["cond"]["ref_image"],
                        image=orig["image"], mask=orig["mask"], crop=cpu_batch["image"]["orig"]["crop"], frames=True,
                        return_device=True, copy_paste=copy_paste)
                    jobs += tb.camera_sample_jobs(outdir, seed, ids, list(orig["file_name"]), pictures)
                if opt.save_visualisations:
                    jobs += tb.camera_vis_jobs(outdir, seed, ids, log["image_preds"].cpu().numpy(), log["image_preds_no_box"].cpu().numpy())
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
                    jobs += tb.lidar_sample_jobs(outdir, seed, ids, list(lid["file_name"]), both[0], both[1])
                if opt.save_visualisations:
                    pcs = log["lidar_input-pred-rec"].cpu().numpy() if "lidar_input-pred-rec" in log else None
                    jobs += tb.lidar_vis_jobs(outdir, seed, ids, pcs, tb.collage_u8(log["range_depth_pred"].cpu().numpy()),
                                              tb.collage_u8(log["range_int_pred"].cpu().numpy()))
                for k, v in (lidar_metrics or {}).items():                      # (once per object, as the reference weighs a batch)
                    metrics.setdefault(k, []).extend([float(v)] * count if not np.isnan(v) else [])
            clock.lap("export + read-back")
            if overlays:                                                        # one call for 2B pictures: the original sweep on the
                orig = batch["image"]["orig"]                                   # original frame, the edited sweep (after the range paste)
                l2i = torch.as_tensor(np.asarray(cpu_batch["image"]["orig"]["lidar2image"]))      # on the recomposed frame, in place
                pics, _ = du.overlay_lidar_batch(
                    depth=torch.cat([f32(lid["range_depth_orig"]), out["depth_final"]]), pitch=torch.cat([pitch, pitch]),
                    yaw=torch.cat([yaw, yaw]), lidar2image=torch.cat([l2i, l2i]), frames_f32=list(orig["image"]) + [None] * count,
                    frames_u8=(frames_buf, [None] * count + [entry["frame"][0] for entry in layout["objects"]]),
                    size=tuple(orig["image"].shape[-2:]))
                jobs += overlay_jobs(outdir, ids, pics[:count], pics[count:])
            clock.lap("overlays")
            writer.put(jobs)
            clock.lap("handing over the files")
    clock.start()
    writer.wait()
    clock.lap("waiting for the writer at the end")
    tb.write_metrics_csv(outdir, metrics)
    return clock.spent


if __name__ == "__main__":
    main()
