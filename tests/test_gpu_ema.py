"""GPU: the EMA shadow weights -- the pair kernel `mobi_ema_multi` (update and swap) against what the reference's LitEma recorded
(tests/golden/ema.npz) and against torch's fp32 arithmetic on the host, and `LatentDiffusion(use_ema=True)` end to end.  Every
comparison is on bits.

Kernel tests: parameters (`a`) and shadows (`b`) are views of two flat device buffers with ONE guard float between neighbours
(a write outside a tensor shows).  `a` holds the tensors of tests/ema_cases.py in order from float offset 1, `b` in the order
1, 3, 255, 8191, 20001, 5, 8192, 8193 from float offset 3: the offsets of `a` cover all four 16-byte phases; the phases of `a`
and `b` agree for 5, 255, 8191, 8192, 8193 (16-byte body with a head of 1, 3, 3, 3, 2 elements) and disagree for 1, 3 and
20001 (the 4-byte walk, over three chunks for the last)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import unet as ounet, weights as W
from tests import ema_cases as E
from tests.golden_cases import load

pytestmark = pytest.mark.gpu

GUARD = 12345.0
B_ORDER = [0, 1, 3, 4, 7, 2, 5, 6]


@pytest.fixture(scope="module")
def ops():
    from mobi_amd import ops as o
    return o


@pytest.fixture(scope="module")
def golden():
    return load("ema")


def _offsets(order, start):
    out, at = {}, start
    for i in order:
        out[i] = at
        at += E.SIZES[i] + 1                           # one guard float between neighbours
    return [out[i] for i in range(len(E.SIZES))], at + 4


A_OFF, A_LEN = _offsets(range(len(E.SIZES)), 1)
B_OFF, B_LEN = _offsets(B_ORDER, 3)


def test_layout_has_the_phases_the_kernel_distinguishes(ops):
    assert ops.multi_tensor_chunk() == 8192            # 8191 / 8192 / 8193: one short chunk, one full chunk, a full chunk + 1 element
    assert {o % 4 for o in A_OFF} == {0, 1, 2, 3}
    differ = [n for n, a, b in zip(E.SIZES, A_OFF, B_OFF) if a % 4 != b % 4]
    assert differ == [1, 3, 20001]
    assert all(a % 4 for n, a, b in zip(E.SIZES, A_OFF, B_OFF) if n not in differ)     # every 16-byte walk has a head


class Buffers:
    """Two flat device buffers (guards everywhere, then the tensors) and the views into them."""

    def __init__(self, a_vals, b_vals):
        self.a, self.b = torch.full((A_LEN,), GUARD), torch.full((B_LEN,), GUARD)
        self.mask_a, self.mask_b = torch.ones(A_LEN, dtype=torch.bool), torch.ones(B_LEN, dtype=torch.bool)   # True: a guard
        for flat, mask, offs, vals in ((self.a, self.mask_a, A_OFF, a_vals), (self.b, self.mask_b, B_OFF, b_vals)):
            for o, n, v in zip(offs, E.SIZES, vals):
                flat[o:o + n] = torch.as_tensor(v)
                mask[o:o + n] = False
        self.a, self.b = self.a.cuda(), self.b.cuda()
        assert self.a.data_ptr() % 16 == 0 and self.b.data_ptr() % 16 == 0
        self.av = [self.a[o:o + n] for o, n in zip(A_OFF, E.SIZES)]
        self.bv = [self.b[o:o + n] for o, n in zip(B_OFF, E.SIZES)]

    def set_a(self, vals):
        for v, t in zip(vals, self.av):
            t.copy_(torch.as_tensor(v))

    def guards_intact(self):
        a, b = self.a.cpu(), self.b.cpu()
        return bool((a[self.mask_a] == GUARD).all()) and bool((b[self.mask_b] == GUARD).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(x, y):
    return torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("tag", list(E.DECAYS))
def test_update_equals_the_references_shadows_bit_for_bit(ops, golden, tag):
    """12 updates with fresh parameters before each, the coefficients the reference used: every shadow bit-equal to the
    reference's CPU result; guards and parameters untouched."""
    init, steps = E.draws(E.DECAYS[tag][1])
    buf = Buffers(init[:len(E.SIZES)], init[:len(E.SIZES)])          # a shadow starts as a copy of its parameter
    pairs = ops.MultiTensorTable([buf.av, buf.bv])
    assert pairs.n_chunks == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3
    omd = golden[f"{tag}_one_minus_decay"].numpy()
    for vals, c in zip(steps, omd):
        buf.set_a(vals)
        ops.ema_multi(pairs, c)
    names = [str(k) for k in golden["buffer_names"]][2:]
    for name, n, got, last in zip(names, E.SIZES, buf.bv, steps[-1]):
        want = golden[f"{tag}_shadow_{name}"]
        assert want.numel() == n and _same_bits(got, want), (tag, name, float((got.cpu() - want).abs().max()))
    assert buf.guards_intact()
    for got, last in zip(buf.av, steps[-1]):
        assert _same_bits(got, torch.from_numpy(last))


def test_degenerate_coefficients(ops):
    """1 - decay = 0: the shadows keep their bits.  = 1: b - (b - a) in three roundings, which is not always a."""
    init, steps = E.draws(77)
    buf = Buffers(steps[0], init[:len(E.SIZES)])
    pairs = ops.MultiTensorTable([buf.av, buf.bv])
    ops.ema_multi(pairs, 0.0)
    for got, v in zip(buf.bv, init):
        assert _same_bits(got, torch.from_numpy(v))
    ops.ema_multi(pairs, 1.0)
    inexact = 0
    for got, v, p in zip(buf.bv, init, steps[0]):
        b, a = torch.from_numpy(v), torch.from_numpy(p)
        want = b - torch.tensor(1.0) * (b - a)
        assert want.dtype == torch.float32 and _same_bits(got, want)
        inexact += int((want != a).sum())
    assert inexact > 0 and buf.guards_intact()


def test_swap_exchanges_and_restores(ops):
    init, steps = E.draws(78)
    a0, b0 = steps[0], init[:len(E.SIZES)]
    buf = Buffers(a0, b0)
    pairs = ops.MultiTensorTable([buf.av, buf.bv])
    ops.swap_multi(pairs)
    for ga, gb, va, vb in zip(buf.av, buf.bv, a0, b0):
        assert _same_bits(ga, torch.from_numpy(vb)) and _same_bits(gb, torch.from_numpy(va))
    assert buf.guards_intact()
    ops.swap_multi(pairs)
    for ga, gb, va, vb in zip(buf.av, buf.bv, a0, b0):
        assert _same_bits(ga, torch.from_numpy(va)) and _same_bits(gb, torch.from_numpy(vb))
    assert buf.guards_intact()


def test_entries_outside_their_tensor_are_skipped(ops):
    """A map that does not belong to the table: tensor indices -1 and `count`, offsets n (exactly one past the end, for the
    8192-element pair), 2^40 and -8192 -- all skipped, never accessed; every proper entry is processed as usual."""
    init, steps = E.draws(79)
    plain, foreign = Buffers(steps[0], init[:len(E.SIZES)]), Buffers(steps[0], init[:len(E.SIZES)])
    cmap = ops.multi_tensor_chunk_map(E.SIZES)
    bad = np.zeros(5, dtype=cmap.dtype)
    bad["tensor"] = [-1, len(E.SIZES), 5, 3, 7]
    bad["offset"] = [0, 0, 8192, 2 ** 40, -8192]
    assert E.SIZES[5] == 8192
    mixed = np.concatenate([bad[:2], cmap[:4], bad[2:4], cmap[4:], bad[4:]])
    ops.ema_multi(ops.MultiTensorTable([plain.av, plain.bv]), 0.25)
    ops.ema_multi(ops.MultiTensorTable([foreign.av, foreign.bv], chunk_map=mixed), 0.25)
    assert _same_bits(foreign.b, plain.b) and _same_bits(foreign.a, plain.a) and foreign.guards_intact()
    assert not _same_bits(plain.bv[-1], torch.from_numpy(init[len(E.SIZES) - 1]))      # (something was updated)
    ops.swap_multi(ops.MultiTensorTable([foreign.av, foreign.bv], chunk_map=mixed))
    for ga, gb, pa, pb in zip(foreign.av, foreign.bv, plain.av, plain.bv):
        assert _same_bits(ga, pb) and _same_bits(gb, pa)
    assert foreign.guards_intact()


def test_argument_errors_launch_nothing(ops):
    from mobi_amd import _lib
    lib = _lib.load()
    init, steps = E.draws(80)
    buf = Buffers(steps[0], init[:len(E.SIZES)])
    pairs = ops.MultiTensorTable([buf.av, buf.bv])
    before = (buf.a.clone(), buf.b.clone())
    tab, cm, st = C.c_void_p(pairs.rows.data_ptr()), C.c_void_p(pairs.chunks.data_ptr()), ops._stream()
    ERR_ARG = -1
    assert lib.mobi_ema_multi(None, pairs.count, cm, pairs.n_chunks, 0.5, _lib.MT_EMA, st) == ERR_ARG
    assert lib.mobi_ema_multi(tab, pairs.count, None, pairs.n_chunks, 0.5, _lib.MT_SWAP, st) == ERR_ARG
    assert lib.mobi_ema_multi(tab, 0, cm, pairs.n_chunks, 0.5, _lib.MT_EMA, st) == ERR_ARG
    assert lib.mobi_ema_multi(tab, pairs.count, cm, 0, 0.5, _lib.MT_SWAP, st) == ERR_ARG
    assert lib.mobi_ema_multi(tab, -1, cm, -1, 0.5, _lib.MT_EMA, st) == ERR_ARG
    for op in (2, -1):
        assert lib.mobi_ema_multi(tab, pairs.count, cm, pairs.n_chunks, 0.5, op, st) == ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(buf.a, before[0]) and torch.equal(buf.b, before[1])
    with pytest.raises(_lib.EngineUnavailable):
        ops.MultiTensorTable([[torch.zeros(4)], [torch.zeros(4)]])                     # no CPU path


# ----------------------------------------------------------------------------------------------------------------------
# end to end: fp16, the reduced network of tests/test_gpu_grad_scaler.py (model_channels 64, latent 16 x 16, two camera / lidar pairs)
N, SIDE = 4, 16


def _latent_diffusion(use_ema):
    from mobi_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    from tests.test_gpu_grad_scaler import _CondStage
    cfg = ounet.UNetConfig(model_channels=64)
    unet_cfg = {"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel",
                "params": dict(image_size=SIDE, in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=64,
                               attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks,
                               channel_mult=list(cfg.channel_mult), num_heads=cfg.num_heads, use_spatial_transformer=True,
                               transformer_depth=1, context_dim=cfg.context_dim, legacy=False, bbox_cond=True, use_camera=True,
                               use_lidar=True)}
    torch.manual_seed(5)
    ld = LatentDiffusion(cond_stage_config="__is_unconditional__", unet_config=unet_cfg, linear_start=0.00085, linear_end=0.012,
                         timesteps=1000, first_stage_key="inpaint", loss_type="l2", cond_stage_key=["ref_image", "ref_bbox"],
                         image_size=SIDE, channels=4, conditioning_key="crossattn", use_ema=use_ema, use_camera=True, use_lidar=True,
                         u_cond_percent=0.0)
    ld.model.diffusion_model.load_state_dict(W.synth_state_dict(ounet.unet_param_shapes(cfg), 9))
    if use_ema:                                        # (the shadows were cloned from the constructor's random initialisation)
        for k, p in ld.model.named_parameters():
            getattr(ld.model_ema, ld.model_ema.m_name2s_name[k]).copy_(p.detach())
    ld.cond_stage_model = _CondStage(W.synth_input("gs.tok", (N, 1, 1024)))
    ld.cond_stage_trainable = True
    return ld.cuda().eval()


def test_use_ema_end_to_end():
    """Three rounds of `training_step` + `step_scaled` + `on_train_batch_end`: after each, every shadow is s - omd (s - p) as
    torch computes it in fp32 on the host from snapshots of s and p.  Then `ema_scope`: the UNet inside the scope is bit-equal
    to a second model that carries the shadows as its weights, eagerly and through the DDIM sampler's captured step graph (the
    weights epoch moved: the graph is captured again); after the scope -- left normally or by an exception -- weights, shadows
    and results are back bit for bit."""
    import mobi_amd
    from mobi_amd import train
    from mobi_amd.ldm.models.diffusion.ddim import DDIMSampler
    from mobi_amd.ldm.modules.diffusionmodules.util import WEIGHTS_EPOCH
    mobi_amd.set_engine_dtype(torch.float16)
    ld = _latent_diffusion(True)
    ema = ld.model_ema
    x = W.synth_input("tl.x", (N, 9, SIDE, SIDE)).cuda()
    noise = W.synth_input("tl.noise", (N, 4, SIDE, SIDE)).cuda()
    t = torch.tensor([741, 741, 21, 21], dtype=torch.long).cuda()
    bbox = (W.synth_input("gs.bbox", (N, 8, 3), kind="uniform") * 0.5 + 0.5).cuda()
    ld.get_input = lambda batch, k, **kw: {"z": x, "cond": {"ref_image": None, "ref_bbox": bbox.clone()}}
    named = {k: p for k, p in ld.model.named_parameters() if p.requires_grad}
    shadow = lambda k: getattr(ema, ema.m_name2s_name[k])
    assert len(named) == len(list(ema.buffers())) - 2 and all(p.dtype == torch.float32 for p in named.values())
    opt = ld.configure_optimizers()
    scaler = train.GradScaler(init_scale=None)
    start = {k: p.detach().cpu() for k, p in named.items()}
    moved_shadows = set()
    for rnd in range(1, 4):
        ld.training_step({}, 0, t=t, noise=noise, scaler=scaler)
        res = opt.step_scaled(ld.adapter_grads, scaler=scaler)
        assert res.found_inf is False
        s0 = {k: shadow(k).cpu() for k in named}
        p0 = {k: p.detach().cpu() for k, p in named.items()}
        epoch, versions = WEIGHTS_EPOCH[0], [p._version for p in named.values()]
        ld.on_train_batch_end()
        assert WEIGHTS_EPOCH[0] == epoch and versions == [p._version for p in named.values()]      # shadows only
        omd = np.float32(1.0) - min(np.float32(0.9999), np.float32(1 + rnd) / np.float32(10 + rnd))
        omd_t = torch.tensor(omd, dtype=torch.float32)
        for k, p in named.items():
            want = s0[k] - omd_t * (s0[k] - p0[k])
            assert _same_bits(shadow(k), want), (rnd, k)
            assert _same_bits(p, p0[k]), (rnd, k)
            if not torch.equal(want, s0[k]):
                moved_shadows.add(k)
        assert int(ema.num_updates) == rnd
    # a shadow moved exactly where its weight did (1 - decay_t >= 0.69 here: no difference is too small to show), and that is
    # the trained tensors (tests/test_gpu_grad_scaler.py: at least 432 of the 432 + 9 move, at most 9 of them outside the UNet)
    assert moved_shadows == {k for k, p in named.items() if not torch.equal(p.detach().cpu(), start[k])}
    assert len(moved_shadows) >= 432 - 9, len(moved_shadows)

    # ---- ema_scope ----
    xin = W.synth_input("ema.x", (N, 9, SIDE, SIDE)).cuda()
    ctx = W.synth_input("ema.ctx", (N, 2, 768)).cuda()
    other = _latent_diffusion(False)                                 # (d): the shadows as plain weights
    ema.copy_to(other.model)
    for k, p in other.model.named_parameters():
        assert _same_bits(p, shadow(k)), k

    kw = {"test_model_kwargs": {"inpaint_image": xin[:, 4:8].contiguous(), "inpaint_mask": xin[:, 8:].contiguous()}}

    def ddim_step(sampler):
        ts = torch.full((N,), int(sampler.ddim_timesteps[-1]), device="cuda", dtype=torch.long)
        out = sampler.p_sample_ddim(xin[:, :4].contiguous(), ctx, ts, index=9, **kw)[0]
        assert sampler._last_step_was_graph
        return out

    sampler, sampler_d = DDIMSampler(ld, graph=True), DDIMSampler(other, graph=True)
    for s in (sampler, sampler_d):
        s.make_schedule(10, ddim_eta=0.0, verbose=False)
    with torch.no_grad():
        live = {k: p.detach().clone() for k, p in named.items()}
        kept = {k: shadow(k).clone() for k in named}
        a = ld.apply_model(xin, t, ctx).clone()
        a_ddim = ddim_step(sampler)
        d = other.apply_model(xin, t, ctx).clone()
        d_ddim = ddim_step(sampler_d)
        epoch, versions = WEIGHTS_EPOCH[0], [p._version for p in named.values()]
        with ld.ema_scope():
            assert WEIGHTS_EPOCH[0] == epoch + 1 and all(p._version > v for p, v in zip(named.values(), versions))
            for k, p in named.items():                               # the weights are the shadows, the shadows hold the weights
                assert _same_bits(p, kept[k]) and _same_bits(shadow(k), live[k]), k
            b = ld.apply_model(xin, t, ctx).clone()
            b_ddim = ddim_step(sampler)
        assert WEIGHTS_EPOCH[0] == epoch + 2
        c = ld.apply_model(xin, t, ctx).clone()
        c_ddim = ddim_step(sampler)
    assert torch.equal(b, d) and torch.equal(c, a) and not torch.equal(b, a)
    assert torch.equal(b_ddim, d_ddim) and torch.equal(c_ddim, a_ddim) and not torch.equal(b_ddim, a_ddim)
    for k, p in named.items():
        assert _same_bits(p, live[k]) and _same_bits(shadow(k), kept[k]), k
    # an exception inside the scope still restores
    with pytest.raises(ZeroDivisionError):
        with ld.ema_scope("test"):
            assert _same_bits(named[next(iter(named))], kept[next(iter(named))])
            1 / 0
    for k, p in named.items():
        assert _same_bits(p, live[k]) and _same_bits(shadow(k), kept[k]), k
    with torch.no_grad():
        assert torch.equal(ld.apply_model(xin, t, ctx), a)


def test_without_use_ema_the_scope_touches_nothing():
    from mobi_amd.ldm.modules.diffusionmodules.util import WEIGHTS_EPOCH
    ld = _latent_diffusion(False)
    assert not hasattr(ld, "model_ema")
    epoch, versions = WEIGHTS_EPOCH[0], [p._version for p in ld.parameters()]
    with ld.ema_scope("nothing"):
        assert WEIGHTS_EPOCH[0] == epoch
    ld.on_train_batch_end()
    assert WEIGHTS_EPOCH[0] == epoch and versions == [p._version for p in ld.parameters()]
