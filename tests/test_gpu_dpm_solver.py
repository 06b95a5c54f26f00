"""DPM-Solver++(2M) on the MI355X (mobi_amd/ldm/models/diffusion/dpm_solver.py, include/mobi_engine.h mobi_dpm_step):

  * the update kernel is bit-identical to a torch fp32 restatement in the documented order;
  * on an analytic problem (Gaussian data, closed-form eps, exact ODE solution) its error falls as a second-order
    method's does, DDIM's as a first-order one's;
  * the graph path (one launch per step) is bit-identical to the eager path;
  * against the CPU oracle's UNet driven by an fp64-coefficient restatement of the solver;
  * as a drop-in for the reference harness's sampler call on the miniature database.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import sampler as osampler, unet as ounet, weights as W
from tests.golden_cases import check, rel_l2

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
# rel-L2 of the engine's DPM-20 vs the fp32 CPU oracle (width 64, 16 x 16, b = 4): the value measured on the MI355X
# + 20 %.  Measured fp16 4.15e-4 / 1.31e-3 and bf16 3.22e-3 / 1.03e-2 at guidance 1 / 5, next to DDIM-50's 3.9e-4 / 1.03e-3
# and 2.97e-3 / 9.2e-3 (tests/test_gpu_production.py): 20 steps accumulate no more storage rounding than 50
TOL_DPM20 = {(torch.float16, 1.0): 5.0e-4, (torch.float16, 5.0): 1.57e-3,
             (torch.bfloat16, 1.0): 3.9e-3, (torch.bfloat16, 5.0): 1.24e-2}


def _set(dtype):
    import mobi_amd
    mobi_amd.set_engine_dtype(dtype)


def _threads():
    torch.set_num_threads(max(1, min(os.cpu_count() or 1, 32)))


def _restate(x, e_c, e_u, hist, scale, row):
    """mobi_dpm_step in torch fp32, in the order of include/mobi_engine.h; row = {1/a_s, s_s/a_s, c_x, c_0, c_1}."""
    e = e_c if e_u is None else e_u + scale * (e_c - e_u)
    x0 = row[0] * x - row[1] * e
    xn = row[2] * x + row[3] * x0
    if row[4] != 0:
        xn = xn + row[4] * hist
    return xn, x0


# ---------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("shape", [(4, 4, 17, 19), (1, 4, 1024, 1027)], ids=["n5168", "grid_stride"])
@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg5"])
@pytest.mark.parametrize("order", [1, 2])
def test_dpm_step_kernel_bit_identical(shape, cfg, order):
    """n not a multiple of the 256-thread block; the larger case exceeds the 4096-block grid (grid-stride loop)."""
    from mobi_amd import ops
    from mobi_amd.ldm.models.diffusion.dpm_solver import dpm_coefficients, dpm_grid
    _, abar = dpm_grid(osampler.Schedule(1).buffers["alphas_cumprod"], 20, 1000)
    tab = dpm_coefficients(abar, False).astype(np.float32)
    row = [float(v) for v in tab[0 if order == 1 else 7]]
    assert (row[4] == 0) == (order == 1)
    tag = f"dpmk.{shape}.{cfg}.{order}"
    x, e_c = W.synth_input(tag + ".x", shape), W.synth_input(tag + ".ec", shape)
    e_u = W.synth_input(tag + ".eu", shape) if cfg else None
    hist = W.synth_input(tag + ".h", shape)
    scale = 5.0 if cfg else 1.0
    ref_x, ref_0 = _restate(x, e_c, e_u, hist, scale, row)
    h_dev = hist.cuda()
    xn, x0 = ops.dpm_step(x.cuda(), e_c.cuda(), h_dev, e_uncond=None if e_u is None else e_u.cuda(), cfg_scale=scale,
                          inv_alpha_s=row[0], sigma_over_alpha_s=row[1], c_x=row[2], c_0=row[3], c_1=row[4])
    assert torch.equal(xn.cpu(), ref_x) and torch.equal(x0.cpu(), ref_0)
    assert torch.equal(h_dev.cpu(), ref_0)                       # the history now holds this step's x0
    # the same row from device memory (the graph-captured form)
    h_dev = hist.cuda()
    xn2, x02 = ops.dpm_step(x.cuda(), e_c.cuda(), h_dev, e_uncond=None if e_u is None else e_u.cuda(), cfg_scale=scale,
                            coef_dev=torch.tensor(row, dtype=torch.float32, device="cuda"))
    assert torch.equal(xn2, xn) and torch.equal(x02, x0) and torch.equal(h_dev.cpu(), ref_0)


def test_dpm_step_first_order_ignores_nan_history():
    """A captured graph's history buffer holds the previous run's values: a first-order row must not read it
    (0 * NaN = NaN)."""
    from mobi_amd import ops
    from mobi_amd.ldm.models.diffusion.dpm_solver import dpm_coefficients, dpm_grid
    _, abar = dpm_grid(osampler.Schedule(1).buffers["alphas_cumprod"], 10, 1000)
    tab = dpm_coefficients(abar, True).astype(np.float32)
    shape = (2, 4, 9, 13)
    x, e_c, e_u = (W.synth_input("dpmnan." + k, shape) for k in ("x", "ec", "eu"))
    for i in (0, tab.shape[0] - 1):                              # both first-order rows of a 10-step run
        row = [float(v) for v in tab[i]]
        assert row[4] == 0
        hist = torch.full(shape, float("nan"), device="cuda")
        for c in (torch.tensor(row, device="cuda"), None):
            hist.fill_(float("nan"))
            kw = {"coef_dev": c} if c is not None else dict(inv_alpha_s=row[0], sigma_over_alpha_s=row[1], c_x=row[2],
                                                            c_0=row[3], c_1=row[4])
            xn, x0 = ops.dpm_step(x.cuda(), e_c.cuda(), hist, e_uncond=e_u.cuda(), cfg_scale=5.0, **kw)
            ref_x, ref_0 = _restate(x, e_c, e_u, None, 5.0, row)
            assert bool(torch.isfinite(xn).all()) and torch.equal(xn.cpu(), ref_x) and torch.equal(hist.cpu(), ref_0)


# ------------------------------------------------------------------------------------------- analytic convergence
class _GaussModel:
    """Data x ~ N(0, s^2 I): the exact eps-model is eps(x, t) = sigma_t x / (alpha_t^2 s^2 + sigma_t^2) (fp64, then
    fp32).  Not an nn.Module and no tensor conditioning: both samplers take their eager paths."""
    num_timesteps = 1000

    def __init__(self, s):
        buf = osampler.Schedule(1).buffers
        self.device = torch.device("cuda")
        self.s = s
        self.betas = torch.from_numpy(buf["betas"]).cuda()
        self.alphas_cumprod = torch.from_numpy(buf["alphas_cumprod"]).cuda()
        self.alphas_cumprod_prev = torch.from_numpy(buf["alphas_cumprod_prev"]).cuda()
        self.ac64 = self.alphas_cumprod.double()

    def apply_model(self, parts, t, c):
        ab = self.ac64[t].view(-1, 1, 1, 1)
        return (torch.sqrt(1 - ab) * parts[0].double() / (ab * self.s ** 2 + (1 - ab))).float()


def _gauss_error(kind, S, s):
    from mobi_amd.ldm.models.diffusion.ddim import DDIMSampler
    from mobi_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    m = _GaussModel(s)
    x_T = W.synth_input("dpm.gauss.xT", (4, 4, 32, 32)).cuda()
    rest = torch.zeros(4, 5, 32, 32, device="cuda")
    smp = (DPMSolverSampler if kind == "dpm" else DDIMSampler)(m)
    got, _ = smp.sample(S=S, batch_size=4, shape=[4, 32, 32], conditioning=None, verbose=False, eta=0.0, x_T=x_T,
                        log_every_t=1000, rest=rest)
    ac = [float(v) for v in osampler.Schedule(1).buffers["alphas_cumprod"]]
    a_T, a_end = ac[(1000 // S) * (S - 1) + 1], ac[0]                 # the grid's first point and DDIM's last a_prev
    k = math.sqrt((a_end * s * s + 1 - a_end) / (a_T * s * s + 1 - a_T))
    exact = x_T.double() * k
    return float((got.double() - exact).norm() / exact.norm())


def test_analytic_convergence_second_order():
    """s = 2: for s below 1 the uniform-t grid's step errors change sign from step to step and the per-doubling ratio is
    erratic at these lengths (fp64 model of both solvers: at s = 2 DPM falls 3.13x / 3.14x, DDIM 1.89x / 1.94x)."""
    s = 2.0
    dpm = [_gauss_error("dpm", S, s) for S in (10, 20, 40)]
    ddim = [_gauss_error("ddim", S, s) for S in (10, 20, 40)]
    print(f"analytic N(0, {s:g}^2): DPM {dpm}  DDIM {ddim}")
    assert dpm[0] / dpm[1] >= 3.0 and dpm[1] / dpm[2] >= 3.0, dpm                  # second order
    assert all(1.6 <= ddim[k] / ddim[k + 1] <= 2.4 for k in range(2)), ddim        # first order: ~2x
    assert dpm[1] < ddim[1]


# ------------------------------------------------------------------------------------ reduced UNet: graph / oracle
def _traj_case(S):
    cfg = ounet.UNetConfig(model_channels=64)
    sd = W.synth_state_dict(ounet.unet_param_shapes(cfg), 9)
    b, side = 4, 16
    inputs = dict(x_T=W.synth_input("smp.x_T", (b, 4, side, side)), inp=W.synth_input("smp.inpaint", (b, 4, side, side)),
                  msk=(W.synth_input("smp.mask", (b, 1, side, side)) > 0).float(),
                  cond=W.synth_input("smp.cond", (b, 2, 768)), uc=W.synth_input("smp.uc", (1, 2, 768)).repeat(b, 1, 1))
    return cfg, sd, inputs, osampler.Schedule(S)


def _unet(cfg, image_size):
    from mobi_amd.ldm.modules.diffusionmodules.openaimodel import UNetModel
    return UNetModel(image_size=image_size, in_channels=cfg.in_channels, out_channels=cfg.out_channels,
                     model_channels=cfg.model_channels, attention_resolutions=list(cfg.attention_resolutions),
                     num_res_blocks=cfg.num_res_blocks, channel_mult=list(cfg.channel_mult),
                     num_heads=cfg.num_heads, use_spatial_transformer=True, transformer_depth=1,
                     context_dim=cfg.context_dim, legacy=False, bbox_cond=cfg.bbox_cond,
                     use_camera=cfg.use_camera, use_lidar=cfg.use_lidar)


def _engine(S, scale, use_graph=True):
    from mobi_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    cfg, sd, i, sch = _traj_case(S)
    net = _unet(cfg, 16)
    net.load_state_dict(sd)
    net = net.cuda()

    class Model:
        num_timesteps = 1000
        device = torch.device("cuda")
        betas = torch.from_numpy(sch.buffers["betas"]).cuda()
        alphas_cumprod = torch.from_numpy(sch.buffers["alphas_cumprod"]).cuda()
        alphas_cumprod_prev = torch.from_numpy(sch.buffers["alphas_cumprod_prev"]).cuda()

        @staticmethod
        def apply_model(xx, tt, cc):
            return net(xx, tt, context=cc)

    s = DPMSolverSampler(Model(), graph=use_graph)
    got, _ = s.sample(S=S, batch_size=4, shape=[4, 16, 16], conditioning=i["cond"].cuda(), verbose=False, eta=0.0,
                      x_T=i["x_T"].cuda(), unconditional_guidance_scale=scale, unconditional_conditioning=i["uc"].cuda(),
                      log_every_t=1000, test_model_kwargs={"inpaint_image": i["inp"].cuda(),
                                                           "inpaint_mask": i["msk"].cuda()})
    return got, s


@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_graph_matches_eager(scale):
    _set(torch.float16)
    eager, se = _engine(10, scale, use_graph=False)
    got, sg = _engine(10, scale, use_graph=True)
    assert not se.__dict__.get("_step_graphs") and len(sg._step_graphs) == 1
    assert next(iter(sg._step_graphs))[0] == "dpm"
    assert torch.equal(got, eager)


@functools.lru_cache(maxsize=None)
def _oracle_dpm(S, scale):
    """§1 of the solver restated here: fp64 coefficients, fp32 tensors, the CPU oracle's UNet as the eps-model."""
    _threads()
    cfg, sd, i, sch = _traj_case(S)
    ac = [float(v) for v in sch.buffers["alphas_cumprod"]]
    ts = list(range(1, 1000, 1000 // S))[::-1]
    abar = [ac[t] for t in ts] + [ac[0]]
    al = [math.sqrt(v) for v in abar]
    sg = [math.sqrt(1 - v) for v in abar]
    lam = [math.log(al[k] / sg[k]) for k in range(len(abar))]
    rest = torch.cat([i["inp"], i["msk"]], 1)
    x, prev = i["x_T"], None
    n = len(ts)
    for k, t in enumerate(ts):
        xin = torch.cat([x, rest], 1)
        tt = torch.full((x.shape[0],), t, dtype=torch.long)
        if scale == 1.0:
            e = ounet.unet_forward(sd, cfg, xin, tt, i["cond"])
        else:
            e_u, e_c = ounet.unet_forward(sd, cfg, torch.cat([xin] * 2), torch.cat([tt] * 2),
                                          torch.cat([i["uc"], i["cond"]])).chunk(2)
            e = e_u + scale * (e_c - e_u)
        x0 = (x - sg[k] * e) / al[k]
        h = lam[k + 1] - lam[k]
        if k == 0 or (k == n - 1 and S < 15):
            D = x0
        else:
            r = (lam[k] - lam[k - 1]) / h
            D = (1 + 1 / (2 * r)) * x0 - (1 / (2 * r)) * prev
        x = (sg[k + 1] / sg[k]) * x - (al[k + 1] * (math.exp(-h) - 1)) * D
        prev = x0
    return x


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_dpm20_vs_oracle(dtype, scale):
    _set(dtype)
    got, s = _engine(20, scale)
    assert len(s._step_graphs) == 1
    err = rel_l2(got.cpu(), _oracle_dpm(20, scale))
    print(f"dpm20 cfg{scale:g} {dtype}: rel-L2 {err:.3e}")
    check(err, TOL_DPM20[(dtype, scale)], f"dpm20_cfg{scale:g}_{dtype}")


# ---------------------------------------------------------------------------------------------- harness drop-in
@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    from tests import mini_db
    root = str(tmp_path_factory.mktemp("mini_db_dpm"))
    return mini_db.build(root)


def _dataset(mini, **kw):
    from ldm.util import instantiate_from_config
    params = dict(state="test", use_lidar=True, use_camera=True, object_database_path=mini[0], scene_database_path=mini[1],
                  expand_mask_ratio=0.1, expand_ref_ratio=0, object_area_crop=0.2, num_samples_per_class=2, fixed_sampling=True,
                  object_random_crop=False, ref_aug=False, ref_mode="id-ref", image_height=128, image_width=128,
                  range_height=128, range_width=128, object_classes=["car", "pedestrian"], range_object_norm=True,
                  range_object_norm_scale=0.75, range_int_norm=True, min_lidar_points=8)
    params.update(kw)
    return instantiate_from_config({"target": "ldm.data.nuscenes.NuScenesDataset", "params": params})


def test_harness_loop_dpm_on_mini_db(mini, monkeypatch):
    """scripts/inference_test_bench.py's loop with the sampler swapped: dataset -> DataLoader -> get_input ->
    DPMSolverSampler (the PLMS branch's inpaint_image= / inpaint_mask= spelling, guidance 5) -> decode_sample -> log_data;
    every step one replay of one captured graph."""
    import mobi_amd
    from ldm.util import instantiate_from_config
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from mobi_amd import graph
    from mobi_amd.ldm.util import load_config
    mobi_amd.set_engine_dtype(torch.float16)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, "configs", "mobi_nusc_256.yaml"),
                      ["latent_size=16", "image_height=128", "use_lidar=True",
                       "model.params.lidar_stage_config.params.ckpt_path=null",
                       "model.params.unet_config.params.model_channels=64",
                       "model.params.first_stage_config.params.ddconfig.ch=32",
                       "model.params.lidar_stage_config.params.ddconfig.ch=32",
                       "model.params.cond_stage_config.params.clip_config.hidden_size=1024",
                       "model.params.cond_stage_config.params.clip_config.intermediate_size=256",
                       "model.params.cond_stage_config.params.clip_config.num_hidden_layers=1",
                       "model.params.cond_stage_config.params.clip_config.num_attention_heads=16"])
    model = instantiate_from_config(cfg["model"])
    W.fill_module_(model, seed=29)
    model = model.cuda().eval()
    sampler = DPMSolverSampler(model)
    counts = {"capture": 0, "replay": 0}
    init, run = graph.StepGraph.__init__, graph.StepGraph.run

    def counted_init(self, *a, **k):
        counts["capture"] += 1
        init(self, *a, **k)

    def counted_run(self, *a, **k):
        counts["replay"] += 1
        return run(self, *a, **k)

    monkeypatch.setattr(graph.StepGraph, "__init__", counted_init)
    monkeypatch.setattr(graph.StepGraph, "run", counted_run)
    ds = _dataset(mini, return_original_image=True)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, num_workers=0, pin_memory=True, shuffle=False, drop_last=False)
    move = lambda d: {k: move(v) if isinstance(v, dict) else (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    S, seen, sizes = 20, 0, set()
    with torch.no_grad(), model.ema_scope():
        for batch in loader:
            batch = move(batch)
            data = model.get_input(batch, model.first_stage_key, force_c_encode=True, return_vae_rec=True)
            n = data["z"].shape[0]
            uc = torch.cat([model.learnable_vector.repeat(n, 1, 1), model.bbox_uncond_vector.repeat(n, 1, 1)], dim=1)
            shape = [model.channels, model.image_size, model.image_size]
            before = dict(counts)
            samples, inter = sampler.sample(S=S, conditioning=data["cond"], batch_size=n, shape=shape, verbose=False,
                                            unconditional_guidance_scale=5.0, unconditional_conditioning=uc, eta=0.0,
                                            x_T=torch.randn([n, *shape], device="cuda"),
                                            inpaint_image=data["z"][:, 4:8], inpaint_mask=data["z"][:, [8]])
            assert counts["replay"] - before["replay"] == S                  # one launch per step
            assert counts["capture"] - before["capture"] == (0 if n in sizes else 1)
            sizes.add(n)
            assert samples.shape == (n, *shape) and bool(torch.isfinite(samples).all())
            assert len(inter["x_inter"]) == len(inter["pred_x0"]) == 3          # x_T, the first and the last step
            h_cam, h_lid = model.decode_sample(samples, data.get("z_lidar"))
            log, metrics = model.log_data(batch, data, h_cam, h_lid, log_metrics=False, return_sample=True, split="test")
            assert metrics is not None and all(np.isfinite(v) or np.isnan(v) for v in metrics.values())
            B = len(batch["id_name"])
            assert log["image_sample"].shape[0] == B and bool(torch.isfinite(log["image_sample"].float()).all())
            assert log["range_sample_depth"].shape[0] == B and bool(torch.isfinite(log["range_sample_depth"].float()).all())
            seen += B
    assert seen == len(ds) and counts["capture"] == len(sizes)
