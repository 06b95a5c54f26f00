"""GPU: the multi-tensor kernels of the fp16 training step (`mobi_grad_stats`, `mobi_adamw_multi`) and what is built on them
(`train.AdamW.step_scaled`, `train.GradScaler`, `LatentDiffusion.training_step(..., scaler=)`).

One tensor-size list for the kernel tests, around the library's chunk length C: 1, 3, 255, 256, 257, C - 1, C, C + 1, 2 C + 5,
70001 -- single elements, the block width and its neighbours, one chunk and its neighbours, more than two chunks with a ragged
end, a tensor of several chunks.  Every tensor is a view of ONE flat buffer with sentinel-filled gaps between the views, so a
write outside a tensor shows.  The 257 tensor starts one element past a 16-byte boundary in all four buffers (head path of
the 16-byte walk); the gradient of the 2 C + 5 tensor alone is shifted as well (pointers that disagree: the 4-byte walk); an
eleventh tensor, `absent`, sits in the middle of the buffers and never has a gradient."""
import math

import numpy as np
import pytest
import torch

from oracle import unet as ounet, weights as W
from tests.backward_ref import adamw_ref
from tests.test_gpu_backward import rel
from tests.test_gpu_backward_geometry import TOL_ADAMW

pytestmark = pytest.mark.gpu

LR = 3e-3
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def ops():
    from mobi_amd import ops as o
    return o


def _layout(C, shifted=()):
    """[(name, offset, n)] in a flat buffer + its length: 16-byte aligned starts, `shifted` names one element further."""
    sizes = [1, 3, 255, 256, 257, C - 1, C, C + 1, 2 * C + 5, 70001]
    names = [f"t{n}" for n in sizes]
    order = list(zip(names[:5], sizes[:5])) + [("absent", 300)] + list(zip(names[5:], sizes[5:]))
    out, at = [], 8
    for name, n in order:
        at = (at + 3) // 4 * 4 + (1 if name in shifted else 0)
        out.append((name, at, n))
        at += n + 5
    return out, at + 8


def _carve(flat, lay):
    return {name: flat[off:off + n] for name, off, n in lay}


def _signed_log_uniform(rng, n, lo, hi):
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo, hi, n)).astype(np.float32)


class Case:
    """The shared inputs (CPU, never modified): layouts, initial parameters, three steps of gradients."""

    def __init__(self, C):
        self.C = C
        self.lay, self.total = _layout(C, shifted=("t257",))
        self.lay_g, self.total_g = _layout(C, shifted=("t257", f"t{2 * C + 5}"))
        self.names = [name for name, _, _ in self.lay if name != "absent"]
        rng = np.random.RandomState(1234)
        self.p0 = torch.full((self.total,), SENTINEL)
        for name, off, n in self.lay:                  # |p| in [0.5, 2]: the relative error of an update is well conditioned
            self.p0[off:off + n] = torch.from_numpy((rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)).astype(np.float32))
        self.grads = [{name: torch.from_numpy(_signed_log_uniform(rng, n, -3, 3)) for name, _, n in self.lay if name != "absent"}
                      for _ in range(3)]

    def grad_buffer(self, g, mul=1.0):
        """{name: fp32 CPU tensor} -> the device views of one flat gradient buffer (the gradient layout)."""
        flat = torch.full((self.total_g,), SENTINEL)
        for name, off, n in self.lay_g:
            if name in g:
                flat[off:off + n] = g[name] * mul
        flat = flat.cuda()
        return flat, _carve(flat, self.lay_g)

    def state(self):
        p, m, v = self.p0.cuda(), torch.full((self.total,), SENTINEL).cuda(), torch.full((self.total,), SENTINEL).cuda()
        for name, off, n in self.lay:
            m[off:off + n] = 0
            v[off:off + n] = 0
        return p, m, v


@pytest.fixture(scope="module")
def case(ops):
    return Case(ops.multi_tensor_chunk())


def _list(ops, case, p, m, v):
    pv, mv, vv = _carve(p, case.lay), _carve(m, case.lay), _carve(v, case.lay)
    return ops.MultiTensorTable([[pv[k] for k in case.names], ops.LIVE, [mv[k] for k in case.names], [vv[k] for k in case.names]])


def _stats(ops, case, g):
    p, m, v = case.state()
    mt = _list(ops, case, p, m, v)
    flat, views = case.grad_buffer(g)
    mt.set_live([views[k] for k in case.names])
    return ops.read_grad_stats(ops.grad_stats(mt)), ops.read_grad_stats(ops.grad_stats(mt))


def _wide_grads(case):
    rng = np.random.RandomState(99)
    return {name: torch.from_numpy(_signed_log_uniform(rng, n, -20, 19)) for name, _, n in case.lay if name != "absent"}


def test_grad_stats_value_in_fp64_and_reproducible(ops, case):
    """fp32 gradients of magnitude 1e-20 .. 1e19 over the size list, with and without one element of 3e38 (finite, its square is
    not an fp32 value: an fp32 accumulator would report an overflow).  Both sides are fp64 sums of exact fp64 products of fp32
    values: only the order of summation differs -> 1e-12; two runs are bit-equal."""
    assert case.C % 4 == 0 and case.C >= 512
    g = _wide_grads(case)
    for big in (False, True):
        if big:
            g[f"t{case.C}"][17] = 3e38
        want = sum(float(np.sum(t.numpy().astype(np.float64) ** 2)) for t in g.values())
        (sumsq, nonfinite), again = _stats(ops, case, g)
        print(f"grad_stats big={big}: sumsq {sumsq!r} numpy {want!r} rel {abs(sumsq - want) / want:.3e}")
        assert not nonfinite
        assert abs(sumsq - want) <= 1e-12 * want
        assert again == (sumsq, nonfinite)             # bit-equal: floats compared exactly


PLANT = {"first_of_first": lambda c: (c.names[0], 0),
         "last_of_last": lambda c: (c.names[-1], -1),
         "last_of_C_plus_1_tail_path": lambda c: (f"t{c.C + 1}", -1),
         "element_0_of_misaligned_view_head_path": lambda c: ("t257", 0)}


@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")], ids=["+inf", "-inf", "nan"])
@pytest.mark.parametrize("where", list(PLANT))
def test_grad_stats_flags_a_non_finite_value(ops, case, where, value):
    name, idx = PLANT[where](case)
    g = {k: t.clone() for k, t in case.grads[0].items()}
    (_, clean), _ = _stats(ops, case, g)
    assert clean is False
    g[name][idx] = value
    (sumsq, nonfinite), _ = _stats(ops, case, g)
    assert nonfinite is True, (where, value, sumsq)


def _run_multi(ops, case, grads, grad_mul, pre_mul=1.0):
    p, m, v = case.state()
    mt = _list(ops, case, p, m, v)
    for step, g in enumerate(grads, 1):
        flat, views = case.grad_buffer(g, pre_mul)
        mt.set_live([views[k] for k in case.names])
        ops.adamw_multi(mt, grad_mul, step, LR)
    return p.cpu(), m.cpu(), v.cpu()


@pytest.fixture(scope="module")
def per_tensor_loop(ops, case):
    """Three steps of `ops.adamw_step`, tensor by tensor, on the same buffers (computed once)."""
    p, m, v = case.state()
    pv, mv, vv = _carve(p, case.lay), _carve(m, case.lay), _carve(v, case.lay)
    for step, g in enumerate(case.grads, 1):
        for k in case.names:
            ops.adamw_step(pv[k], g[k].cuda(), mv[k], vv[k], step, LR)
    return p.cpu(), m.cpu(), v.cpu()


def _assert_same_buffers(case, got, want):
    for what, a, b in zip(("param", "exp_avg", "exp_avg_sq"), got, want):
        for name, off, n in case.lay:
            assert torch.equal(a[off:off + n], b[off:off + n]), (what, name)
        assert torch.equal(a, b), (what, "gaps")       # the sentinels between the tensors too


def test_adamw_multi_is_bit_equal_to_the_per_tensor_kernel(ops, case, per_tensor_loop):
    """grad_mul = 1, and gradients pre-multiplied by 2^13 with grad_mul = 2^-13 (magnitudes 1e-3 .. 1e3: the scaling is exact):
    parameters and both moments bit-equal to three loops of `ops.adamw_step`; `absent` and the gaps bit-unchanged."""
    _assert_same_buffers(case, _run_multi(ops, case, case.grads, 1.0), per_tensor_loop)
    _assert_same_buffers(case, _run_multi(ops, case, case.grads, 2.0 ** -13, pre_mul=2.0 ** 13), per_tensor_loop)
    off, n = next((o, n) for name, o, n in case.lay if name == "absent")
    assert torch.equal(per_tensor_loop[0][off:off + n], case.p0[off:off + n])
    assert not torch.equal(per_tensor_loop[0], case.p0)


def test_adamw_multi_grad_mul_against_fp64(ops, case):
    """grad_mul = 0.3: against `adamw_ref` (fp64) on the fp32-rounded g * 0.3, at the project's bound for AdamW."""
    p, _, _ = _run_multi(ops, case, case.grads, 0.3)
    for name, off, n in case.lay:
        if name == "absent":
            assert torch.equal(p[off:off + n], case.p0[off:off + n])
            continue
        gs = [torch.from_numpy(g[name].numpy() * np.float32(0.3)) for g in case.grads]
        assert gs[0].dtype == torch.float32
        want = adamw_ref(case.p0[off:off + n], gs, LR)[0]
        err = rel(p[off:off + n], want, "adamw_multi")
        assert err < TOL_ADAMW, (name, err)


def test_step_scaled_clips_then_skips_on_overflow(ops, case):
    from mobi_amd import train
    from mobi_amd.ldm.modules.diffusionmodules.util import WEIGHTS_EPOCH
    p, _, _ = case.state()
    params = _carve(p, case.lay)                       # 11 names; `absent` never has a gradient
    opt = train.AdamW(params, lr=LR)
    scaler = train.GradScaler(init_scale=1024.0, growth_interval=2000, enabled=True)
    g = case.grads[0]
    norm = math.sqrt(sum(float(np.sum(t.numpy().astype(np.float64) ** 2)) for t in g.values()))
    max_norm = 0.5 * norm
    flat, views = case.grad_buffer(g, 1024.0)          # still multiplied by the scale (exact)
    epoch, versions = WEIGHTS_EPOCH[0], {k: t._version for k, t in params.items()}
    res = opt.step_scaled({k: views[k] for k in case.names}, scaler=scaler, max_norm=max_norm)
    clip = min(1.0, max_norm / (norm + 1e-6))
    print(f"step_scaled: grad_norm {res.grad_norm!r} fp64 {norm!r} rel {abs(res.grad_norm - norm) / norm:.3e} clip {res.clip_coef!r}")
    assert res.found_inf is False and res.scale == 1024.0 and scaler.scale == 1024.0 and opt.steps == 1
    assert abs(res.grad_norm - norm) <= 1e-12 * norm
    assert abs(res.clip_coef - clip) <= 1e-12 and res.clip_coef < 1.0
    assert WEIGHTS_EPOCH[0] == epoch + 1
    assert all(params[k]._version > versions[k] for k in case.names)   # (views of one buffer share its version counter)
    got = p.cpu()
    for name, off, n in case.lay:
        if name == "absent":
            assert torch.equal(got[off:off + n], case.p0[off:off + n])
            continue
        want = adamw_ref(case.p0[off:off + n], [g[name].double() * clip], LR)[0]
        err = rel(got[off:off + n], want, "step_scaled")
        assert err < TOL_ADAMW, (name, err)
    assert "absent" not in opt.state
    # an inf in one gradient: nothing moves, the scale is halved
    before = (got, {k: (m.cpu(), v.cpu()) for k, (m, v) in opt.state.items()}, opt.steps, WEIGHTS_EPOCH[0])
    bad = {k: t.clone() for k, t in case.grads[1].items()}
    bad[f"t{case.C - 1}"][-1] = float("inf")
    flat, views = case.grad_buffer(bad, scaler.scale)
    res = opt.step_scaled({k: views[k] for k in case.names}, scaler=scaler, max_norm=max_norm)
    assert res.found_inf is True and res.scale == 1024.0 and scaler.scale == 512.0
    assert opt.steps == before[2] and WEIGHTS_EPOCH[0] == before[3]
    assert torch.equal(p.cpu(), before[0])
    for k, (m, v) in opt.state.items():
        assert torch.equal(m.cpu(), before[1][k][0]) and torch.equal(v.cpu(), before[1][k][1]), k


# ----------------------------------------------------------------------------------------------------------------------
# end to end: fp16, the reduced network of tests/test_gpu_backward.py (model_channels 64, latent 16 x 16, two camera / lidar pairs)
class _CondStage(torch.nn.Module):
    """The conditioning stage's trainable part alone: the 3-D box embedder; the image token is a constant."""

    def __init__(self, token):
        super().__init__()
        from mobi_amd.ldm.modules.encoders.modules import BBoxEmbedder
        self.bbox_embedder = BBoxEmbedder()
        W.fill_module_(self.bbox_embedder, seed=61)
        self.register_buffer("token", token)

    def encode(self, cond):
        return {"ref_image_token": self.token}


def test_training_with_a_scaler_end_to_end():
    """Two iterations of `training_step(scaler=s)` + `step_scaled` with s at today's static scale (a power of two: unscaling inside
    the update is exact) against two iterations of today's `training_step` + `step`: every trainable tensor bit-equal -- the
    432 UNet tensors, the box embedder's eight (iteration 1, a conditional draw) and `bbox_uncond_vector` (iteration 2, an
    unconditional draw): the conditioning stage's gradients carry the same factor.  Then one iteration at 2^40: the fp16
    backward pass saturates, the step is skipped, nothing moves and the scale is halved."""
    import mobi_amd
    from mobi_amd import train
    from mobi_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    mobi_amd.set_engine_dtype(torch.float16)
    cfg = ounet.UNetConfig(model_channels=64)
    n, side = 4, 16
    unet_cfg = {"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel",
                "params": dict(image_size=side, in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=64,
                               attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks,
                               channel_mult=list(cfg.channel_mult), num_heads=cfg.num_heads, use_spatial_transformer=True,
                               transformer_depth=1, context_dim=cfg.context_dim, legacy=False, bbox_cond=True, use_camera=True,
                               use_lidar=True)}
    torch.manual_seed(5)
    ld = LatentDiffusion(cond_stage_config="__is_unconditional__", unet_config=unet_cfg, linear_start=0.00085, linear_end=0.012,
                         timesteps=1000, first_stage_key="inpaint", loss_type="l2", cond_stage_key=["ref_image", "ref_bbox"],
                         image_size=side, channels=4, conditioning_key="crossattn", use_ema=False, use_camera=True, use_lidar=True,
                         u_cond_percent=0.0)
    ld.model.diffusion_model.load_state_dict(W.synth_state_dict(ounet.unet_param_shapes(cfg), 9))
    ld.cond_stage_model = _CondStage(W.synth_input("gs.tok", (n, 1, 1024)))
    ld.cond_stage_trainable = True
    ld = ld.cuda().eval()
    x = W.synth_input("tl.x", (n, 9, side, side)).cuda()
    noise = W.synth_input("tl.noise", (n, 4, side, side)).cuda()
    t = torch.tensor([741, 741, 21, 21], dtype=torch.long).cuda()
    bbox = (W.synth_input("gs.bbox", (n, 8, 3), kind="uniform") * 0.5 + 0.5).cuda()
    ld.get_input = lambda batch, k, **kw: {"z": x, "cond": {"ref_image": None, "ref_bbox": bbox.clone()}}
    start = {k: v.detach().clone() for k, v in ld.state_dict().items()}
    static = train.static_loss_scale(noise.numel())
    assert static == 1024.0

    def run(with_scaler):
        ld.load_state_dict(start)
        opt = ld.configure_optimizers()
        assert isinstance(opt, train.AdamW) and len(opt.params) == 432 + 8 + 1
        s = train.GradScaler(init_scale=None) if with_scaler else None
        seen = set()
        for it in range(2):
            ld.u_cond_percent = 0.0 if it == 0 else 2.0           # conditional, then unconditional (the draw is uniform in [0, 1))
            if with_scaler:
                ld.training_step({}, 0, t=t, noise=noise, scaler=s)
                assert ld.adapter_grads_scale == s.scale == static
                res = opt.step_scaled(ld.adapter_grads, scaler=s)
                assert res.found_inf is False and res.clip_coef == 1.0 and res.grad_norm > 0.0
            else:
                ld.training_step({}, 0, t=t, noise=noise)
                assert ld.adapter_grads_scale == 1.0
                opt.step(ld.adapter_grads)
            seen |= set(ld.adapter_grads)
        assert seen == set(opt.params)                             # every trainable tensor was stepped at least once
        return {k: p.detach().clone() for k, p in opt.params.items()}, opt, s

    today, _, _ = run(False)
    scaled, opt, s = run(True)
    moved = 0
    for k in today:
        assert torch.equal(today[k], scaled[k]), k
        moved += int(not torch.equal(today[k], start[k].to(today[k].device)))
    assert moved >= 432, moved
    # 2^40: 2 (eps - target) 2^40 / numel does not fit fp16 -- saturation is arithmetic, the step must be skipped
    s2 = train.GradScaler(init_scale=2.0 ** 40)
    steps = opt.steps
    ld.u_cond_percent = 0.0
    ld.training_step({}, 0, t=t, noise=noise, scaler=s2)
    res = opt.step_scaled(ld.adapter_grads, scaler=s2)
    assert res.found_inf is True, res
    assert s2.scale == 2.0 ** 39 and opt.steps == steps
    for k, p in opt.params.items():
        assert torch.equal(p.detach(), scaled[k]) and bool(torch.isfinite(p).all()), k
