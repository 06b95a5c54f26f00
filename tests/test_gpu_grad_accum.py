"""GPU: gradient accumulation -- `mobi_accum_multi` (one multi-tensor launch per micro-batch) and `train.GradAccumulator`.

The kernel tests use the tensor-size list, layouts and gradients of tests/test_gpu_grad_scaler.py (`Case`): 1, 3, 255, 256, 257,
C - 1, C, C + 1, 2 C + 5, 70001 around the chunk length C, views of one flat buffer with sentinel-filled gaps, `t257` one element
past a 16-byte boundary in the accumulator AND the gradient buffer (head path), the 2 C + 5 gradient alone shifted (pointers that
disagree: the 4-byte walk), `absent` never given a gradient."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import unet as ounet, weights as W
from tests.golden_cases import record
from tests.test_gpu_backward import TOL_UNET
from tests.test_gpu_grad_scaler import SENTINEL, Case, _carve, _CondStage

pytestmark = pytest.mark.gpu

LR = 3e-3


@pytest.fixture(scope="module")
def ops():
    from mobi_amd import ops as o
    return o


@pytest.fixture(scope="module")
def case(ops):
    return Case(ops.multi_tensor_chunk())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(x, y):
    return torch.equal(_bits(x), _bits(y))


def _accumulators(case, fill):
    """The flat accumulator buffer in the parameter layout: `fill` inside the tensors, sentinels between them."""
    flat = torch.full((case.total,), SENTINEL)
    for _, off, n in case.lay:
        flat[off:off + n] = fill
    return flat.cuda()


def _launch_window(ops, case, acc, grad_sets, w, first_op):
    """One launch per gradient set over `case.names` (`first_op`, then ACCUM) -> the gradient buffers as (before, after)."""
    from mobi_amd import _lib
    views = _carve(acc, case.lay)
    table = ops.MultiTensorTable([ops.LIVE, [views[k] for k in case.names]])
    kept = []
    for i, g in enumerate(grad_sets):
        flat, gv = case.grad_buffer(g)
        before = flat.clone()
        table.set_live([gv[k] for k in case.names])
        ops.accum_multi(table, w, first_op if i == 0 else _lib.MT_ACCUM)
        kept.append((before, flat))
    torch.cuda.synchronize()
    return kept


def test_window_is_bit_equal_to_numpy_fp32(ops, case):
    """micro_batches = 3: ASSIGN, ACCUM, ACCUM with w = fp32(1/3) against `acc = w g0; acc = acc + w g1; acc = acc + w g2`, every
    numpy operation in float32 -- bit-equal; the gaps, `absent` and the gradient buffers bit-unchanged.  The inputs tell a
    contracted kernel (one rounding per accumulate) from a correct one in every tensor of 255 elements or more."""
    from mobi_amd import _lib
    w = np.float32(1.0) / np.float32(3.0)
    acc = _accumulators(case, 7.0)
    start = acc.clone()
    kept = _launch_window(ops, case, acc, case.grads, float(w), _lib.MT_ASSIGN)
    got = acc.cpu()
    want_flat = start.cpu().clone()
    for name, off, n in case.lay:
        if name == "absent":
            continue
        g = [gs[name].numpy() for gs in case.grads]
        ref = w * g[0]
        fused = ref.copy()
        for gi in g[1:]:
            ref = ref + w * gi
            fused = (fused.astype(np.float64) + np.float64(w) * gi.astype(np.float64)).astype(np.float32)
        assert ref.dtype == np.float32
        differ = int(np.sum(ref.view(np.int32) != fused.view(np.int32)))
        print(f"{name}: {differ} of {n} elements tell a contracted accumulate from the two-rounding one")
        if n >= 255:
            assert differ >= 1, name
        assert np.array_equal(got[off:off + n].numpy().view(np.int32), ref.view(np.int32)), name
        want_flat[off:off + n] = torch.from_numpy(ref)
    assert _same_bits(got, want_flat)                  # the sentinels between the tensors and `absent` (still 7.0) too
    for before, after in kept:
        assert _same_bits(before, after)


def test_assign_ignores_what_the_accumulator_held(ops, case):
    from mobi_amd import _lib
    w = np.float32(1.0) / np.float32(3.0)
    acc = _accumulators(case, float("nan"))
    start = acc.clone()
    _launch_window(ops, case, acc, case.grads[:1], float(w), _lib.MT_ASSIGN)
    got, want = acc.cpu(), start.cpu().clone()
    for name, off, n in case.lay:
        if name != "absent":
            assert bool(torch.isfinite(got[off:off + n]).all()), name
            want[off:off + n] = torch.from_numpy(w * case.grads[0][name].numpy())
    assert _same_bits(got, want)                       # `absent` keeps its nan, the gaps their sentinels


def _optimizer(case, micro_batches, scale):
    from mobi_amd import train
    p, _, _ = case.state()
    opt = train.AdamW(_carve(p, case.lay), lr=LR)     # 11 names; `absent` never has a gradient
    return p, opt, train.GradAccumulator(opt, micro_batches), train.GradScaler(init_scale=scale, enabled=True)


def _add(case, acc, g, scale):
    flat, views = case.grad_buffer(g, scale)           # still multiplied by the scale (a power of two: exact)
    acc.add({k: views[k] for k in case.names}, scale=scale)
    return flat


def test_non_finite_values_survive_the_window_and_the_next_window_is_clean(ops, case):
    """+inf in micro-batch 0 and -inf in the same element of micro-batch 1 (their sum is nan), one nan in the tail-path element
    of t{C+1}: the statistics over the accumulators flag it, the step is skipped, the scale halved -- and the next, clean window
    ends bit-equal to the first step of a run that never had the bad one."""
    name_inf, name_nan = f"t{case.C - 1}", f"t{case.C + 1}"
    bad = [{k: t.clone() for k, t in g.items()} for g in case.grads[:2]]
    bad[0][name_inf][11] = float("inf")
    bad[1][name_inf][11] = float("-inf")
    bad[1][name_nan][-1] = float("nan")
    p, opt, acc, s = _optimizer(case, 2, 1024.0)
    keep = [_add(case, acc, g, s.scale) for g in bad]
    assert bool(torch.isnan(acc.views[name_inf][11])) and bool(torch.isnan(acc.views[name_nan][-1]))
    assert bool(torch.isfinite(acc.views[name_inf][:11]).all()) and bool(torch.isfinite(acc.views[name_nan][:-1]).all())
    mt = ops.MultiTensorTable([[opt.params[k] for k in case.names], ops.LIVE, [torch.zeros_like(opt.params[k]) for k in case.names],
                               [torch.zeros_like(opt.params[k]) for k in case.names]])
    mt.set_live([acc.views[k] for k in case.names])
    assert ops.read_grad_stats(ops.grad_stats(mt))[1] is True
    res = acc.step(scaler=s)
    assert res.found_inf is True and res.scale == 1024.0 and s.scale == 512.0 and opt.steps == 0
    assert _same_bits(p, case.p0)
    for k, (m, v) in opt.state.items():
        assert not bool(m.any()) and not bool(v.any()), k
    keep += [_add(case, acc, g, s.scale) for g in case.grads[:2]]
    res = acc.step(scaler=s)
    assert res.found_inf is False and res.scale == 512.0 and opt.steps == 1
    # the run that never had the bad window
    p2, opt2, acc2, s2 = _optimizer(case, 2, 1024.0)
    keep += [_add(case, acc2, g, s2.scale) for g in case.grads[:2]]
    res2 = acc2.step(scaler=s2)
    assert res2.found_inf is False and opt2.steps == 1 and res2.grad_norm == res.grad_norm
    assert _same_bits(p, p2) and not _same_bits(p, case.p0)
    assert set(opt.state) == set(opt2.state) == set(case.names)
    for k in case.names:
        assert _same_bits(opt.state[k][0], opt2.state[k][0]) and _same_bits(opt.state[k][1], opt2.state[k][1]), k


def test_argument_errors_launch_nothing(ops, case):
    from mobi_amd import _lib
    lib = _lib.load()
    acc = _accumulators(case, 3.0)
    views = _carve(acc, case.lay)
    table = ops.MultiTensorTable([ops.LIVE, [views[k] for k in case.names]])
    flat, gv = case.grad_buffer(case.grads[0])
    table.set_live([gv[k] for k in case.names])
    before = (acc.clone(), flat.clone())
    tab, cm, st = C.c_void_p(table.rows.data_ptr()), C.c_void_p(table.chunks.data_ptr()), ops._stream()
    ERR_ARG = -1
    assert lib.mobi_accum_multi(None, table.count, cm, table.n_chunks, 0.5, _lib.MT_ACCUM, st) == ERR_ARG
    assert lib.mobi_accum_multi(tab, table.count, None, table.n_chunks, 0.5, _lib.MT_ASSIGN, st) == ERR_ARG
    assert lib.mobi_accum_multi(tab, 0, cm, table.n_chunks, 0.5, _lib.MT_ACCUM, st) == ERR_ARG
    assert lib.mobi_accum_multi(tab, table.count, cm, 0, 0.5, _lib.MT_ASSIGN, st) == ERR_ARG
    assert lib.mobi_accum_multi(tab, -1, cm, -1, 0.5, _lib.MT_ACCUM, st) == ERR_ARG
    for op in (2, -1):
        assert lib.mobi_accum_multi(tab, table.count, cm, table.n_chunks, 0.5, op, st) == ERR_ARG
    torch.cuda.synchronize()
    assert _same_bits(acc, before[0]) and _same_bits(flat, before[1])
    with pytest.raises(_lib.EngineUnavailable):
        ops.MultiTensorTable([ops.LIVE, [torch.zeros(4)]])                             # no CPU path


def test_misuse_raises(case):
    p, opt, acc, s = _optimizer(case, 2, 1024.0)
    keep = [_add(case, acc, case.grads[0], 1024.0)]
    with pytest.raises(RuntimeError):
        acc.step(scaler=s)                             # one of two
    flat, views = case.grad_buffer(case.grads[1], 512.0)
    with pytest.raises(ValueError):
        acc.add({k: views[k] for k in case.names}, scale=512.0)
    keep.append(_add(case, acc, case.grads[1], 1024.0))
    with pytest.raises(RuntimeError):
        _add(case, acc, case.grads[2], 1024.0)         # a third
    assert acc.step(scaler=s).found_inf is False and opt.steps == 1


# ----------------------------------------------------------------------------------------------------------------------
# end to end: fp16, the reduced network of tests/test_gpu_grad_scaler.py (model_channels 64, latent 16 x 16, two camera / lidar pairs)
def _latent_diffusion(n, side):
    from mobi_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    cfg = ounet.UNetConfig(model_channels=64)
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
    return ld.cuda().eval()


def test_one_micro_batch_equals_the_loop_without_accumulation():
    """micro_batches = 1 (w = 1: the product is exact): `training_step(scaler=s, allreduce=False)` + `add` + `step(scaler=s)`
    against `training_step(scaler=s)` + `step_scaled`, a conditional then an unconditional draw -- all 441 trainable tensors
    bit-equal; after the first iteration `bbox_uncond_vector` has no optimizer state (left out, not stepped with zeros)."""
    import mobi_amd
    from mobi_amd import train
    mobi_amd.set_engine_dtype(torch.float16)
    n, side = 4, 16
    ld = _latent_diffusion(n, side)
    x = W.synth_input("tl.x", (n, 9, side, side)).cuda()
    noise = W.synth_input("tl.noise", (n, 4, side, side)).cuda()
    t = torch.tensor([741, 741, 21, 21], dtype=torch.long).cuda()
    bbox = (W.synth_input("gs.bbox", (n, 8, 3), kind="uniform") * 0.5 + 0.5).cuda()
    ld.get_input = lambda batch, k, **kw: {"z": x, "cond": {"ref_image": None, "ref_bbox": bbox.clone()}}
    start = {k: v.detach().clone() for k, v in ld.state_dict().items()}

    def run(accumulate):
        ld.load_state_dict(start)
        opt = ld.configure_optimizers()
        assert isinstance(opt, train.AdamW) and len(opt.params) == 432 + 8 + 1
        s = train.GradScaler(init_scale=None)
        acc = train.GradAccumulator(opt, 1) if accumulate else None
        for it in range(2):
            ld.u_cond_percent = 0.0 if it == 0 else 2.0           # conditional, then unconditional
            if accumulate:
                ld.training_step({}, 0, t=t, noise=noise, scaler=s, allreduce=False)
                acc.add(ld.adapter_grads, scale=ld.adapter_grads_scale)
                res = acc.step(scaler=s)
            else:
                ld.training_step({}, 0, t=t, noise=noise, scaler=s)
                res = opt.step_scaled(ld.adapter_grads, scaler=s)
            assert res.found_inf is False and res.grad_norm > 0.0
            if it == 0:
                assert "bbox_uncond_vector" not in opt.state and len(opt.state) == 432 + 8
                assert torch.equal(opt.params["bbox_uncond_vector"].detach(), start["bbox_uncond_vector"].to("cuda"))
        assert opt.steps == 2 and len(opt.state) == 441
        return {k: p.detach().clone() for k, p in opt.params.items()}

    today, accumulated = run(False), run(True)
    assert len(today) == 441
    moved = 0
    for k in today:
        assert _same_bits(today[k], accumulated[k]), k
        moved += int(not torch.equal(today[k], start[k].to(today[k].device)))
    assert moved >= 432, moved


def test_two_micro_batches_against_autograd():
    """The network, inputs and fp16 setting of test_training_loop_follows_the_reference_trajectory, its batch of four as two
    micro-batches (images 0-1, 2-3): three windows of `loss_and_gradients` x 2 -> `add` x 2 -> `step` against the CPU oracle's
    `(loss / 2).backward()` x 2 + torch.optim.AdamW.  Every micro-batch loss within 1e-3 relative (that test's bound for this
    loop; measured 1.5e-4); the first window's accumulated gradient, all 432 tensors as one vector, within TOL_UNET[fp16][0]
    (6e-3; measured 3.8e-3)."""
    import mobi_amd
    from mobi_amd import train
    from tests.test_gpu_models import _unet
    mobi_amd.set_engine_dtype(torch.float16)
    cfg = ounet.UNetConfig(model_channels=64)
    sd = W.synth_state_dict(ounet.unet_param_shapes(cfg), 9)
    net = _unet(cfg, 16)
    net.load_state_dict(sd)
    net = net.cuda()
    n, side, lr = 4, 16, 2e-4
    x = W.synth_input("tl.x", (n, 9, side, side))
    ctx = W.synth_input("tl.ctx", (n, 2, 768))
    noise = W.synth_input("tl.noise", (n, 4, side, side))
    t = torch.tensor([741, 741, 21, 21], dtype=torch.long)
    names = train.trainable_names(net)
    assert len(names) == 432
    ps = {k: (v.clone().requires_grad_(True) if k in set(names) else v) for k, v in sd.items()}
    ref_opt = torch.optim.AdamW([ps[k] for k in names], lr=lr)
    eng_opt = train.AdamW({k: p for k, p in net.named_parameters() if k in set(names)}, lr=lr)
    acc = train.GradAccumulator(eng_opt, 2)
    micro = [slice(0, 2), slice(2, 4)]
    ref_losses, eng_losses, whole = [], [], None
    for window in range(3):
        ref_opt.zero_grad()
        for m in micro:
            loss = torch.mean((ounet.unet_forward(ps, cfg, x[m], t[m], ctx[m]) - noise[m]) ** 2)
            (loss / 2).backward()
            ref_losses.append(float(loss.detach()))
            el, grads = train.loss_and_gradients(net, x[m].cuda(), t[m].cuda(), ctx[m].cuda(), noise[m].cuda(), loss_scale=256.0)
            grads.pop("__dcontext__")
            acc.add(grads)
            eng_losses.append(float(el))
        if window == 0:
            flat_g = torch.cat([acc.views[k].reshape(-1).double().cpu() for k in names])
            flat_r = torch.cat([ps[k].grad.reshape(-1).double() for k in names])
            whole = float((flat_g - flat_r).norm() / flat_r.norm())
        ref_opt.step()
        res = acc.step()
        assert res.found_inf is False and eng_opt.steps == window + 1
    worst = max(abs(a - b) / abs(b) for a, b in zip(eng_losses, ref_losses))
    print(f"two micro-batches: accumulated gradient of window 0, 432 tensors as one vector, rel-L2 {whole:.3e}; "
          f"worst micro-batch loss rel diff {worst:.3e}; losses {eng_losses} reference {ref_losses}")
    record("accumulated_adapter_gradients", whole, TOL_UNET[torch.float16][0])
    record("accumulated_loop_worst_loss_rel_diff", worst, 1e-3)
    for a, b in zip(eng_losses, ref_losses):
        assert abs(a - b) <= 1e-3 * abs(b), (eng_losses, ref_losses)
    assert whole < TOL_UNET[torch.float16][0], whole
