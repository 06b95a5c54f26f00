"""GPU: `mobi_loss_grad` (the fused loss / entering-gradient launch, include/mobi_engine.h) against the fp64 restatement of its
contract (tests/loss_grad_ref.py), against the composition it replaces bit for bit, against the reference's own `p_losses` numbers
(tests/golden/losses.npz), and the training step built on it -- l2 with per-timestep weights, l1, and
`LatentDiffusion.training_step` with every setting it used to refuse -- against torch.autograd through the CPU oracle's UNet."""
import numpy as np
import pytest
import torch

from oracle import unet as ounet, weights as W
from tests.golden_cases import load, record
from tests.loss_grad_ref import loss_grad_ref, reference_formula, storage_ulp, to_storage

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
REL = 2e-6                      # per_sample / terms: the bound tests/test_gpu_models.py uses for the golden's loss numbers
# tests/test_gpu_backward.py TOL_UNET: (all 432 adapter gradients as one vector, the worst single tensor) of the reduced UNet
TOL_UNET = {torch.float16: (6e-3, 1.4e-2), torch.bfloat16: (3e-2, 7.8e-2)}
TOL_DX = {torch.float16: 1.9e-3, torch.bfloat16: 1.5e-2}        # the same file's bound on that test's loss value
ELBO = 0.25


@pytest.fixture(scope="module")
def ops():
    from mobi_amd import ops as o
    return o


@pytest.fixture(scope="module")
def tables():
    """(logvar: random in [-1, 1], lvlb: the reference's `lvlb_weights`), fp32 [1000]."""
    rng = np.random.default_rng(11)
    return torch.from_numpy(rng.uniform(-1.0, 1.0, 1000).astype(np.float32)), load("losses")["lvlb_weights"].float()


def _case(shape, seed):
    n = shape[0]
    rng = np.random.default_rng(seed)
    eps = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    target = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    eps[0, 0, 1, 2] = target[0, 0, 1, 2]                                  # an exact tie: the l1 zero
    eps[n - 1, shape[1] - 1, shape[2] - 1, shape[3] - 1] = target[n - 1, shape[1] - 1, shape[2] - 1, shape[3] - 1]
    t = torch.tensor({1: [999], 2: [1, 1], 3: [0, 1, 999], 4: [0, 999, 0, 1]}[n], dtype=torch.long)     # 0, 1, T - 1 and repeats
    return eps, target, t


def _run(ops, eps, target, t, logvar, lvlb, dtype, **kw):
    dy, per, terms = ops.loss_grad(eps.cuda(), target.cuda(), t.cuda(), logvar.cuda(), lvlb.cuda(), dtype=dtype, **kw)
    torch.cuda.synchronize()
    return dy.cpu(), per.cpu(), terms.cpu()


def _close(got, want, what):
    got, want = got.double(), want.double()
    err = float(((got - want).abs() / want.abs()).max())
    print(f"{what}: worst relative error {err:.3e}")
    assert err <= REL, (what, err)


# [3, 4, 5, 7]: fewer pixels than one wave; [2, 4, 16, 16]: exactly one 256-thread block per sample; [3, 4, 17, 17]: two partials
# per sample and a ragged tail; [1, 3, 9, 4]: a channel count other than 4
SHAPES = [(3, 4, 5, 7), (2, 4, 16, 16), (3, 4, 17, 17), (1, 3, 9, 4)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("loss_type", ["l2", "l1"])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_the_contract(ops, tables, shape, loss_type, dtype):
    logvar, lvlb = tables
    eps, target, t = _case(shape, seed=sum(shape))
    kw = dict(loss_type=loss_type, l_simple_weight=1.0, elbo_weight=ELBO, loss_scale=4.0)
    dy, per, terms = _run(ops, eps, target, t, logvar, lvlb, dtype, **kw)
    rdy, rper, rterms = loss_grad_ref(eps, target, t, logvar, lvlb, **kw)
    n, c, h, w = shape
    assert dy.shape == (n, h, w, 32) and dy.dtype == dtype
    assert bool((dy[..., c:] == 0).all()) and not bool(torch.signbit(dy[..., c:]).any())        # padding: exactly +0
    want = to_storage(rdy, dtype)
    if loss_type == "l1":
        assert torch.equal(dy.view(torch.int16), want.view(torch.int16))
        assert float(dy[0, 1, 2, 0]) == 0.0 and float(dy[n - 1, h - 1, w - 1, c - 1]) == 0.0   # the ties
        assert int((dy[..., :c] == 0).sum()) == 2
    else:
        got = dy[..., :c].permute(0, 3, 1, 2).double()
        over = (got - rdy).abs() / storage_ulp(rdy, dtype)
        print(f"l2 dy: worst distance {float(over.max()):.3f} storage ulp")
        assert float(over.max()) <= 1.0
        assert float(got[0, 0, 1, 2]) == 0.0
    _close(per, rper, "per_sample")
    _close(terms, rterms, "terms")
    again = _run(ops, eps, target, t, logvar, lvlb, dtype, **kw)
    assert torch.equal(again[0].view(torch.int16), dy.view(torch.int16)) and torch.equal(again[1], per) and torch.equal(again[2], terms)
    # a NaN in eps: a NaN in dy at that element under either loss, in that sample's loss and in the means; nothing else moves
    bad = eps.clone()
    bad[n - 1, 1, 2, 3] = float("nan")
    ndy, nper, nterms = _run(ops, bad, target, t, logvar, lvlb, dtype, **kw)
    assert bool(torch.isnan(ndy[n - 1, 2, 3, 1])) and int(torch.isnan(ndy).sum()) == 1
    keep = torch.ones_like(dy, dtype=torch.bool)
    keep[n - 1, 2, 3, 1] = False
    assert torch.equal(ndy[keep].view(torch.int16), dy[keep].view(torch.int16))
    assert bool(torch.isnan(nper[n - 1])) and torch.equal(nper[: n - 1], per[: n - 1]) and bool(torch.isnan(nterms).all())


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", [(4, 4, 16, 16), (3, 4, 17, 17)])
def test_default_settings_equal_the_composition_bit_for_bit(ops, shape, dtype):
    """Zero tables, weight 1, ELBO weight 0: dy is `pack_sources(lincomb4([eps, target], [k, -k]))`, k = 2 loss_scale / numel --
    what the training step computed before this launch existed -- bit for bit, and loss == loss_simple's mean."""
    eps, target, t = _case(shape, seed=3)
    z = torch.zeros(1)
    for loss_scale in (1.0, 256.0):
        dy, per, terms = _run(ops, eps, target, t, z, z, dtype, loss_scale=loss_scale)
        k = 2.0 * loss_scale / eps.numel()
        old = ops.pack_sources([ops.lincomb4([eps.cuda(), target.cuda()], [k, -k])], dtype).cpu()
        assert torch.equal(dy.view(torch.int16), old.view(torch.int16))
        assert float(terms[0]) == float(terms[2]) and float(terms[1]) == 0.0
        _close(terms[0], ((eps.double() - target.double()) ** 2).mean(), "mean squared error")


@pytest.mark.parametrize("loss_type,pre", [("l2", ""), ("l1", "l1_")])
def test_terms_equal_the_references_p_losses(ops, loss_type, pre):
    g = load("losses")
    logvar = torch.full((1000,), 0.3)
    _, per, terms = _run(ops, g["model_out"], g["noise"], g["t"], logvar, g["lvlb_weights"], torch.float16, loss_type=loss_type,
                         l_simple_weight=1.0, elbo_weight=ELBO)
    for i, key in enumerate(("val__loss_simple", "val__loss_vlb", "val__loss")):
        want = float(g[pre + key])
        print(f"{loss_type} {key}: {float(terms[i])!r} reference {want!r}")
        assert abs(float(terms[i]) - want) <= REL * abs(want), (loss_type, key)
    assert abs(float(terms[2]) - float(g[pre + "loss"])) <= REL * abs(float(g[pre + "loss"]))


# ----------------------------------------------------------------------------------------------------------------------
# End to end: the reduced UNet of tests/test_gpu_backward.py::test_unet_training_step_gradients_vs_autograd
# ----------------------------------------------------------------------------------------------------------------------
N, SIDE, LOSS_SCALE = 4, 16, 256.0


class _Oracle:
    """The CPU oracle's UNet on the test's inputs with its autograd graph kept: one forward, several backward passes."""

    def __init__(self):
        from mobi_amd import train
        from tests.test_gpu_models import _unet
        self.cfg = ounet.UNetConfig(model_channels=64)
        self.sd = W.synth_state_dict(ounet.unet_param_shapes(self.cfg), 9)
        self.x = W.synth_input("bw.unet.x", (N, 9, SIDE, SIDE))
        self.ctx = W.synth_input("bw.unet.ctx", (N, 2, 768))
        self.noise = W.synth_input("bw.unet.noise", (N, 4, SIDE, SIDE))
        self.t = torch.tensor([741, 741, 21, 21], dtype=torch.long)          # (a camera / lidar pair shares its t; the pairs differ)
        self.names = train.trainable_names(_unet(self.cfg, SIDE))
        assert len(self.names) == 432
        want = set(self.names)
        self.ps = {k: (v.clone().requires_grad_(True) if k in want else v) for k, v in self.sd.items()}
        self.eps = ounet.unet_forward(self.ps, self.cfg, self.x, self.t, self.ctx)

    def gradients(self, cotangent):
        """d <eps, cotangent> / d every adapter tensor -> one flat fp64 vector per name."""
        for k in self.names:
            self.ps[k].grad = None
        self.eps.backward(gradient=cotangent, retain_graph=True)
        return {k: self.ps[k].grad.detach().double().clone() for k in self.names}

    def net(self, dtype):
        import mobi_amd
        from tests.test_gpu_models import _unet
        mobi_amd.set_engine_dtype(dtype)
        net = _unet(self.cfg, SIDE)
        net.load_state_dict(self.sd)
        return net.cuda()


@pytest.fixture(scope="module")
def oracle():
    return _Oracle()


def _compare(grads, want, names, tag):
    errs = {}
    for k in names:
        a, b = grads[k].double().cpu().reshape(-1), want[k].reshape(-1)
        errs[k] = float((a - b).norm() / b.norm().clamp_min(1e-30))
    flat_g = torch.cat([grads[k].reshape(-1).double().cpu() for k in names])
    flat_r = torch.cat([want[k].reshape(-1) for k in names])
    whole = float((flat_g - flat_r).norm() / flat_r.norm())
    worst = max(errs.items(), key=lambda kv: kv[1])
    record(tag + "_all_adapter_gradients", whole)
    record(tag + "_worst_tensor", worst[1])
    print(f"{tag}: all 432 gradients {whole:.3e}, worst tensor {worst[1]:.3e} ({worst[0]})")
    return whole, worst


@pytest.mark.parametrize("dtype", DT)
def test_unet_l2_with_per_timestep_weights_vs_autograd(oracle, tables, dtype):
    """l2 with a non-zero logvar table and ELBO weight 0.25: the loss and all 432 gradients against torch.autograd of the
    reference's formula through the CPU oracle.  Bounds: TOL_UNET of tests/test_gpu_backward.py -- the per-sample weights only
    rescale, per sample, the cotangent that test already bounds."""
    from mobi_amd import train
    logvar, lvlb = tables
    o = oracle
    _, d = reference_formula(o.eps, o.noise, o.t, logvar, lvlb, "l2", 1.0, ELBO)
    cot, = torch.autograd.grad(d["loss"], o.eps, retain_graph=True)
    want = o.gradients(cot)
    net = o.net(dtype)
    loss, grads, (per, terms) = train.loss_and_gradients(net, o.x.cuda(), o.t.cuda(), o.ctx.cuda(), o.noise.cuda(), LOSS_SCALE,
                                                         t_weights=(logvar.cuda(), lvlb.cuda()), elbo_weight=ELBO, return_terms=True)
    grads.pop("__dcontext__")
    assert sorted(grads) == sorted(o.names) and float(loss) == float(terms[2]) and loss.dim() == 0
    for i, key in enumerate(("loss_simple", "loss_vlb", "loss")):
        ref = float(d[key].detach())
        assert abs(float(terms[i]) - ref) <= TOL_DX[dtype] * abs(ref), key
    whole, worst = _compare(grads, want, o.names, "l2_weighted")
    assert whole < TOL_UNET[dtype][0], whole
    assert worst[1] < TOL_UNET[dtype][1], worst


# the constant-magnitude cotangent measures INSIDE the l2 bounds on the MI355X (2.9e-3 / 6.4e-3 fp16, 1.6e-2 / 4.2e-2 bf16): they hold
L1_BOUND = TOL_UNET


@pytest.mark.parametrize("dtype", DT)
def test_unet_l1_backward_of_the_engines_own_cotangent(oracle, tables, dtype):
    """l1: the engine's own entering gradient (read back from `ops.loss_grad` on the engine's eps, loss scale divided out) is
    back-propagated through the oracle and the 432 gradients are compared -- NOT full autograd of the l1 loss: wherever the
    engine's eps and the oracle's straddle the target the sign differs, which is inherent to |.| and no backward error.
    Bounds: TOL_UNET of tests/test_gpu_backward.py (all gradients as one vector, the worst tensor), unchanged: measured on the
    MI355X 2.9e-3 / 6.4e-3 (fp16) and 1.6e-2 / 4.2e-2 (bf16), beside 2.7e-3 / 6.1e-3 and 1.4e-2 / 3.6e-2 for the weighted l2."""
    from mobi_amd import ops, train
    logvar, lvlb = tables
    o = oracle
    net = o.net(dtype)
    dev = lambda v: v.cuda()
    eps, tape = train.unet_forward(net, dev(o.x), dev(o.t), dev(o.ctx))
    dy, per, terms = ops.loss_grad(eps.contiguous(), dev(o.noise), dev(o.t), dev(logvar), dev(lvlb), loss_type="l1",
                                   elbo_weight=ELBO, loss_scale=LOSS_SCALE, dtype=dtype)
    grads = train.unet_backward(net, tape, dy=dy)
    grads.pop("__dcontext__")
    loss, grads2 = train.loss_and_gradients(net, dev(o.x), dev(o.t), dev(o.ctx), dev(o.noise), LOSS_SCALE, loss_type="l1",
                                            t_weights=(dev(logvar), dev(lvlb)), elbo_weight=ELBO)
    assert float(loss) == float(terms[2])
    assert all(torch.equal(grads[k] / LOSS_SCALE, grads2[k]) for k in o.names)          # (a power of two: exact)
    cot = dy[..., :4].permute(0, 3, 1, 2).float().cpu() / LOSS_SCALE
    assert int((cot == 0).sum()) == 0 and cot.abs().unique().numel() == 2              # +-k_i, one magnitude per pair
    want = o.gradients(cot)
    whole, worst = _compare(grads2, want, o.names, "l1")
    assert whole < L1_BOUND[dtype][0], whole
    assert worst[1] < L1_BOUND[dtype][1], worst
    # the loss against the oracle's forward (no sign involved)
    _, d = reference_formula(o.eps.detach(), o.noise, o.t, logvar, lvlb, "l1", 1.0, ELBO)
    assert abs(float(loss) - float(d["loss"])) <= TOL_DX[dtype] * abs(float(d["loss"]))


def test_training_step_trains_on_l1_elbo_and_logvar(oracle):
    """The public entry with every setting it used to refuse: loss_type l1, original_elbo_weight 0.25, logvar_init 0.3."""
    import mobi_amd
    from mobi_amd import train
    from mobi_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    mobi_amd.set_engine_dtype(torch.float16)
    cfg, o = oracle.cfg, oracle
    unet_cfg = {"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel",
                "params": dict(image_size=SIDE, in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=64,
                               attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks,
                               channel_mult=list(cfg.channel_mult), num_heads=cfg.num_heads, use_spatial_transformer=True,
                               transformer_depth=1, context_dim=cfg.context_dim, legacy=False, bbox_cond=True, use_camera=True,
                               use_lidar=True)}
    ld = LatentDiffusion(cond_stage_config="__is_unconditional__", unet_config=unet_cfg, linear_start=0.00085, linear_end=0.012,
                         timesteps=1000, first_stage_key="inpaint", loss_type="l1", cond_stage_key=["ref_image", "ref_bbox"],
                         image_size=SIDE, channels=4, conditioning_key="crossattn", use_ema=False, use_camera=True, use_lidar=True,
                         u_cond_percent=0.0, original_elbo_weight=ELBO, logvar_init=0.3)
    ld.model.diffusion_model.load_state_dict(o.sd)
    ld = ld.cuda().train()
    x, ctx, noise, t = o.x.cuda(), o.ctx.cuda(), o.noise.cuda(), o.t.cuda()
    ld.get_input = lambda batch, k, **kw: {"z": x, "cond": ctx}
    names = ["model.diffusion_model." + k for k in o.names]
    loss = ld.training_step({}, 0, t=t, noise=noise)
    assert loss.dim() == 0 and loss.is_cuda and bool(torch.isfinite(loss))
    assert sorted(ld.adapter_grads) == sorted(names)
    assert all(bool(torch.isfinite(v).all()) and v.dtype == torch.float32 for v in ld.adapter_grads.values())
    assert set(ld.loss_dict) == {"train/loss_simple", "train/loss_vlb", "train/loss"}
    assert all(v.dim() == 0 and v.is_cuda for v in ld.loss_dict.values())
    assert float(ld.loss_dict["train/loss"]) == float(loss) and ld.adapter_grads_scale == 1.0
    # the same numbers as the forward-only side (`p_losses`, pinned to the reference) on the same draw
    ld.eval()
    _, d = ld.p_losses(x, ctx, t, noise=noise)
    for key in ("loss_simple", "loss_vlb", "loss"):
        a, b = float(ld.loss_dict["train/" + key]), float(d["val/" + key])
        assert abs(a - b) <= 2 * 4e-3 * abs(b), (key, a, b)               # 2 TOL_NET[fp16] (tests/test_gpu_models.py): two forwards
    ld.train()
    # with a scaler: the gradients stay multiplied by its scale and `step_scaled` divides it out
    opt = train.AdamW({k: p for k, p in ld.named_parameters() if k in set(names)}, lr=1e-4)
    scaler = train.GradScaler(init_scale=None)
    before = {k: p.detach().clone() for k, p in opt.params.items()}
    unscaled = {k: v.clone() for k, v in ld.adapter_grads.items()}
    loss2 = ld.training_step({}, 0, t=t, noise=noise, scaler=scaler)
    assert float(loss2) == float(loss)
    assert ld.adapter_grads_scale == scaler.scale == train.static_loss_scale(noise.numel())
    assert all(torch.equal(ld.adapter_grads[k] / scaler.scale, unscaled[k]) for k in names)      # (a power of two: exact)
    res = opt.step_scaled(ld.adapter_grads, scaler=scaler)
    assert res.found_inf is False and res.grad_norm > 0.0 and opt.steps == 1
    assert sum(int(not torch.equal(p.detach(), before[k])) for k, p in opt.params.items()) >= 400
    # and a validation-mode call names its dict as the reference does
    ld.eval()
    ld.training_step({}, 0, t=t, noise=noise)
    assert set(ld.loss_dict) == {"val/loss_simple", "val/loss_vlb", "val/loss"}
