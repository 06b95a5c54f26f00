"""GPU: checkpoints and resuming -- `mobi_snapshot_multi` (copy + digest + non-finite flag of every listed tensor in one launch),
`checkpoint.Checkpointer` (snapshot isolation, exact resume, refusals, the reference's readers) and `train.Trainer`.

Every comparison is bit-equality.  The end-to-end tests use the reduced network of tests/test_gpu_grad_accum.py (model_channels
64, latent 16 x 16, n = 4, fp16) with `use_ema=True`, a warm-up schedule and a trainable conditioning stage."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from oracle import unet as ounet, weights as W
from tests.test_gpu_grad_scaler import _CondStage

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(x, y):
    return x.shape == y.shape and torch.equal(_bits(x), _bits(y))


# ----------------------------------------------------------------------------------------------------------------------
# the kernel
class KernelCase:
    """Seven pairs around the chunk length c, sources and destinations carved out of one buffer each (sentinel words between
    them), some at a 4-byte and not a 16-byte boundary; pairs 3 and 5 with pointers whose alignment phases disagree.  Contents:
    random bits read as fp32 -- denormals, both zeros, +-inf and NaNs with payloads."""

    def __init__(self, c):
        self.sizes = [1, 3, c - 1, c, c + 1, 2 * c + 5, 5]
        src_shift, dst_shift = [1, 0, 2, 0, 3, 1, 0], [1, 0, 2, 1, 3, 0, 0]
        self.src_off, self.dst_off = self._offsets(src_shift), self._offsets(dst_shift)
        rng = np.random.RandomState(77)
        self.words = [rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32) for n in self.sizes]
        self.words[0][:] = [0x7F800000]                                     # +inf alone
        self.words[1][:] = [0x00000000, 0x80000000, 0x00000001]             # both zeros and the smallest denormal
        big = self.words[3]                                                 # a whole chunk WITHOUT a non-finite value
        big[((big >> 23) & 0xFF) == 0xFF] &= 0x807FFFFF                     # (exponent cleared: denormals instead)
        self.words[6][:] = [0x7FC00001, 0xFFC12345, 0x00000002, 0x3F800000, 0x807FFFFF]      # NaN payloads, denormals
        self.words[4][-1] = 0xFF800000                                      # -inf in the tail path
        self.nonfinite = [bool((((w >> 23) & 0xFF) == 0xFF).any()) for w in self.words]
        assert self.nonfinite == [True, False, True, False, True, True, True]
        self.total = max(o + n for o, n in zip(self.src_off + self.dst_off, self.sizes * 2)) + 16

    def _offsets(self, shifts):
        out, at = [], 8
        for n, s in zip(self.sizes, shifts):
            at = (at + 3) // 4 * 4 + s
            out.append(at)
            at += n + 5
        return out

    def source(self):
        flat = np.full(self.total, SENTINEL, dtype=np.uint32)
        for off, w in zip(self.src_off, self.words):
            flat[off:off + len(w)] = w
        return torch.from_numpy(flat.view(np.float32).copy()).cuda()

    def destination(self):
        return torch.from_numpy(np.full(self.total, SENTINEL, dtype=np.uint32).view(np.float32).copy()).cuda()

    def expected_destination(self, written):
        flat = np.full(self.total, SENTINEL, dtype=np.uint32)
        for j, (off, w) in enumerate(zip(self.dst_off, self.words)):
            if written[j]:
                flat[off:off + len(w)] = w
        return torch.from_numpy(flat.view(np.int32).copy())


@pytest.fixture(scope="module")
def ops():
    from mobi_amd import ops as o
    return o


@pytest.fixture(scope="module")
def kcase(ops):
    return KernelCase(ops.multi_tensor_chunk())


def _table(ops, kcase, src, dst, written):
    a = [src[o:o + n] for o, n in zip(kcase.src_off, kcase.sizes)]
    b = [dst[o:o + n] if w else None for o, n, w in zip(kcase.dst_off, kcase.sizes, written)]
    return ops.MultiTensorTable([a, b])


@pytest.mark.parametrize("written", [[True] * 7, [True, False] * 3 + [True], [False] * 7], ids=["all", "every_second_null", "all_null"])
def test_snapshot_copies_words_and_digests(ops, kcase, written):
    from mobi_amd.checkpoint import digest_host
    assert kcase.src_off[0] % 4 and kcase.src_off[2] % 4 and not kcase.src_off[1] % 4
    src, dst = kcase.source(), kcase.destination()
    src_before = src.clone()
    table = _table(ops, kcase, src, dst, written)
    first = ops.read_snapshot_records(ops.snapshot_multi(table))
    again = ops.read_snapshot_records(ops.snapshot_multi(table))
    torch.cuda.synchronize()
    assert torch.equal(_bits(dst), kcase.expected_destination(written))        # the copies, the sentinels, the NULL pairs' fill
    assert _same_bits(src, src_before)
    want = [(digest_host(w.view(np.float32)), nf) for w, nf in zip(kcase.words, kcase.nonfinite)]
    assert first == want
    assert again == first


def test_snapshot_argument_errors_launch_nothing(ops, kcase):
    from mobi_amd import _lib
    lib = _lib.load()
    src, dst = kcase.source(), kcase.destination()
    table = _table(ops, kcase, src, dst, [True] * 7)
    rec = torch.full((table.count * 2 + 1,), 0x77, dtype=torch.int64, device="cuda")
    before = (dst.clone(), rec.clone())
    tab, cm, out, st = C.c_void_p(table.rows.data_ptr()), C.c_void_p(table.chunks.data_ptr()), C.c_void_p(rec.data_ptr()), ops._stream()
    call = lib.mobi_snapshot_multi
    assert call(None, table.count, cm, table.n_chunks, None, out, st) == -1
    assert call(tab, table.count, None, table.n_chunks, None, out, st) == -1
    assert call(tab, table.count, cm, table.n_chunks, None, None, st) == -1
    assert call(tab, -1, cm, table.n_chunks, None, out, st) == -1
    assert call(tab, 0, cm, table.n_chunks, None, out, st) == -1
    assert call(tab, table.count, cm, 0, None, out, st) == -1
    assert call(tab, table.count, cm, -3, None, out, st) == -1
    assert call(tab, table.count, cm, table.n_chunks, None, C.c_void_p(rec.data_ptr() + 4), st) == -4
    torch.cuda.synchronize()
    assert _same_bits(dst, before[0]) and torch.equal(rec, before[1])


def test_snapshot_skips_map_entries_outside_their_pair(ops, kcase):
    """A chunk map with an entry past its tensor's end and entries of tensors the table does not have: skipped, and the records
    are those of the honest map."""
    src, dst = kcase.source(), kcase.destination()
    honest = _table(ops, kcase, src, dst, [True] * 7)
    want = ops.read_snapshot_records(ops.snapshot_multi(honest))
    cmap = ops.multi_tensor_chunk_map(kcase.sizes)
    extra = np.zeros(3, dtype=cmap.dtype)
    extra["tensor"], extra["offset"] = [6, 7, -1], [8, 0, 0]                 # offset 8 in a tensor of 5; tensors 7 and -1 of 7
    a = [src[o:o + n] for o, n in zip(kcase.src_off, kcase.sizes)]
    dst2 = kcase.destination()
    b = [dst2[o:o + n] for o, n in zip(kcase.dst_off, kcase.sizes)]
    table = ops.MultiTensorTable([a, b], chunk_map=np.concatenate([extra, cmap]))
    assert ops.read_snapshot_records(ops.snapshot_multi(table)) == want
    assert torch.equal(_bits(dst2), kcase.expected_destination([True] * 7))


def test_other_kernels_refuse_a_table_with_null_rows(ops, kcase):
    """A None in a column is `snapshot_multi`'s alone: `ema_multi`, `swap_multi` and `accum_multi` read every pointer, so they
    refuse such a table on the host and launch nothing."""
    from mobi_amd import _lib
    src, dst = kcase.source(), kcase.destination()
    table = _table(ops, kcase, src, dst, [True, False] * 3 + [True])
    assert table.has_null and not _table(ops, kcase, src, dst, [True] * 7).has_null
    before = (src.clone(), dst.clone())
    for launch in (lambda: ops.ema_multi(table, 0.5), lambda: ops.swap_multi(table), lambda: ops.accum_multi(table, 0.5, _lib.MT_ASSIGN),
                   lambda: ops.accum_multi(table, 0.5, _lib.MT_ACCUM)):
        with pytest.raises(AssertionError, match="None"):
            launch()
    torch.cuda.synchronize()
    assert _same_bits(src, before[0]) and _same_bits(dst, before[1])
    assert len(ops.read_snapshot_records(ops.snapshot_multi(table))) == 7      # (and the launch that tests for NULL takes it)


def _channels_last_net(seed):
    """A module whose trained weight and one frozen buffer are channels_last (fp32 tensors that are not dense), next to dense
    ones, and an optimizer with hand-made moments."""
    from mobi_amd import train
    torch.manual_seed(seed)
    net = torch.nn.Conv2d(4, 6, 3).cuda()
    net.weight.data = net.weight.data.contiguous(memory_format=torch.channels_last)
    net.register_buffer("frozen_cl", torch.randn(5, 4, 3, 3, device="cuda").contiguous(memory_format=torch.channels_last))
    net.register_buffer("frozen", torch.randn(7, device="cuda"))
    net.register_buffer("count", torch.tensor(seed, dtype=torch.int32, device="cuda"))
    assert not net.weight.is_contiguous() and not net.frozen_cl.is_contiguous()
    opt = train.AdamW({"weight": net.weight, "bias": net.bias}, lr=1e-3)
    opt.state["bias"] = (torch.randn(6, device="cuda"), torch.rand(6, device="cuda"))
    opt.steps = 2
    return net, opt


def test_tensors_that_are_not_dense_are_digested_and_staged(tmp_path):
    """A channels_last weight or buffer is digested, checked for inf / nan and snapshotted like every other fp32 tensor: `verify`
    passes on the file `save` wrote, the file holds the values of the moment of the save, and `load` finds its digests."""
    from mobi_amd import checkpoint
    path = str(tmp_path / "cl.ckpt")
    net, opt = _channels_last_net(3)
    ck = checkpoint.Checkpointer(net, opt)
    at_save = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ck.save(path, 2, 0, 2)
    net.weight.data.mul_(2.0)                          # before wait(): the file must not see it
    net.frozen_cl.add_(1.0)
    ck.wait()
    count, bad = checkpoint.verify_file(path)
    assert (count, bad) == (6, [])                     # weight, bias, frozen_cl, frozen and both moments of bias
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(ckpt["mobi_amd"]["digests"]) == ["bias", "frozen", "frozen_cl", "optimizer.1.exp_avg", "optimizer.1.exp_avg_sq", "weight"]
    for k, v in at_save.items():
        assert _same_bits(ckpt["state_dict"][k], v), k
    assert ckpt["mobi_amd"]["digests"]["weight"][0] == checkpoint.digest_host(at_save["weight"].cpu())
    before = open(path, "rb").read()
    net.weight.data[1, 2, 0, 1] = float("inf")
    with pytest.raises(checkpoint.NonFiniteState, match="'weight'"):
        ck.save(path, 3, 0, 3)
    ck.wait()
    assert open(path, "rb").read() == before
    other, other_opt = _channels_last_net(4)
    ck2 = checkpoint.Checkpointer(other, other_opt)
    assert ck2.load(path)["global_step"] == 2
    for k, v in at_save.items():
        assert _same_bits(other.state_dict()[k], v), k
    assert not other.weight.is_contiguous() and other_opt.steps == 2
    assert _same_bits(other_opt.state["bias"][0], opt.state["bias"][0])


# ----------------------------------------------------------------------------------------------------------------------
# end to end
N, SIDE, LR = 4, 16, 1e-3


class _CondStageWithBoxToken(_CondStage):
    """`_CondStage` that also serves `validation_step`, which asks the conditioning stage for the box token itself."""

    def encode(self, cond):
        from mobi_amd import train
        out = {"ref_image_token": self.token}
        if cond.get("ref_bbox") is not None:
            out["ref_bbox_token"] = train.bbox_embedder_forward(self.bbox_embedder, cond["ref_bbox"])[0]
        return out


def _model(seed=5, ckpt_path=None):
    from mobi_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    import mobi_amd
    mobi_amd.set_engine_dtype(torch.float16)
    cfg = ounet.UNetConfig(model_channels=64)
    unet_cfg = {"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel",
                "params": dict(image_size=SIDE, in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=64,
                               attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks,
                               channel_mult=list(cfg.channel_mult), num_heads=cfg.num_heads, use_spatial_transformer=True,
                               transformer_depth=1, context_dim=cfg.context_dim, legacy=False, bbox_cond=True, use_camera=True,
                               use_lidar=True)}
    sched = {"target": "ldm.lr_scheduler.LambdaLinearScheduler",
             "params": dict(warm_up_steps=[4], cycle_lengths=[10000000000000], f_start=[1.0e-2], f_max=[1.0], f_min=[1.0])}
    torch.manual_seed(seed)
    ld = LatentDiffusion(cond_stage_config="__is_unconditional__", unet_config=unet_cfg, linear_start=0.00085, linear_end=0.012,
                         timesteps=1000, first_stage_key="inpaint", loss_type="l2", cond_stage_key=["ref_image", "ref_bbox"],
                         image_size=SIDE, channels=4, conditioning_key="crossattn", use_ema=True, use_camera=True, use_lidar=True,
                         u_cond_percent=0.5, scheduler_config=sched, monitor="val/loss_simple_ema", ckpt_path=ckpt_path)
    if ckpt_path is None:
        ld.model.diffusion_model.load_state_dict(W.synth_state_dict(ounet.unet_param_shapes(cfg), 9 if seed == 5 else seed))
    ld.cond_stage_model = _CondStageWithBoxToken(W.synth_input("gs.tok", (N, 1, 1024)))
    ld.cond_stage_trainable = True
    ld.learning_rate = LR
    return ld.cuda().eval()


def _batches(count):
    return [{"z": W.synth_input(f"ck.x{i}", (N, 9, SIDE, SIDE)).cuda(),
             "bbox": (W.synth_input(f"ck.b{i}", (N, 8, 3), kind="uniform") * 0.5 + 0.5).cuda()} for i in range(count)]


def _wire(ld):
    """The grad-accum tests' synthetic `get_input` stand-in, reading the batch it is given."""
    ld.get_input = lambda batch, k, **kw: {"z": batch["z"], "cond": {"ref_image": None, "ref_bbox": batch["bbox"].clone()}}
    return ld


class Run:
    """One model with everything a loop holds, stepped by hand: `training_step(scaler=s)`, the optimizer (or the accumulator),
    the EMA hook, the schedule.  Step `bad_step` gets an inf planted in one gradient: skipped, the scaler backs off."""

    def __init__(self, seed=5, accumulate=1):
        from mobi_amd import checkpoint, train
        self.ld = _wire(_model(seed))
        (self.opt,), (sch,) = self.ld.configure_optimizers()
        self.sched = sch["scheduler"]
        self.scaler = train.GradScaler(init_scale=None)
        self.k = accumulate
        self.acc = train.GradAccumulator(self.opt, accumulate) if accumulate > 1 else None
        self.ck = checkpoint.Checkpointer(self.ld, self.opt, self.sched, self.scaler, self.acc)
        self.skipped = []

    def seed(self):
        random.seed(11)
        np.random.seed(11)
        torch.manual_seed(11)

    def steps(self, batches, first, count, bad_step=None):
        for s in range(first, first + count):
            for m in range(self.k):
                self.ld.training_step(batches[(s * self.k + m) % len(batches)], 0, scaler=self.scaler, allreduce=self.k == 1)
                if s == bad_step and m == 0:
                    g = self.ld.adapter_grads[sorted(self.ld.adapter_grads)[3]]
                    g.view(-1)[1] = float("inf")
                if self.acc is not None:
                    self.acc.add(self.ld.adapter_grads, scale=self.ld.adapter_grads_scale)
            res = self.acc.step(scaler=self.scaler) if self.acc is not None else \
                self.opt.step_scaled(self.ld.adapter_grads, scaler=self.scaler)
            self.skipped.append(res.found_inf)
            self.ld.on_train_batch_end()
            self.sched.step()

    def state(self):
        """Everything a resume must be exact about; draws from the python and the device generator last."""
        out = {"param/" + k: p.detach().clone() for k, p in self.opt.params.items()}
        for k, (m, v) in self.opt.state.items():
            out["exp_avg/" + k], out["exp_avg_sq/" + k] = m.clone(), v.clone()
        out.update({"ema/" + k: b.clone() for k, b in self.ld.model_ema.named_buffers()})
        host = {"scaler": self.scaler.state_dict(), "steps": self.opt.steps, "lr": self.opt.lr, "last_epoch": self.sched.last_epoch,
                "moments": sorted(self.opt.state), "random": random.random(), "numpy": float(np.random.rand()),
                "torch_cpu": float(torch.rand(1)), "device": float(torch.rand(1, device="cuda"))}
        return out, host


def _assert_same_state(got, want):
    (gt, gh), (wt, wh) = got, want
    assert gh == wh
    assert sorted(gt) == sorted(wt)
    for k in wt:
        assert _same_bits(gt[k], wt[k]), k


BAD_STEP = 1


@pytest.fixture(scope="module")
def batches():
    return _batches(4)


@pytest.fixture(scope="module")
def straight(batches):
    """Run A: six steps straight, step 1 skipped by an injected inf -> its final state."""
    a = Run()
    a.seed()
    a.steps(batches, 0, 6, bad_step=BAD_STEP)
    assert a.skipped == [False, True, False, False, False, False] and a.opt.steps == 5
    assert len(a.opt.params) == 441 and len(a.opt.state) == 441            # conditional and unconditional draws both occurred
    from mobi_amd import train
    assert a.scaler.scale == 0.5 * train.static_loss_scale(N * 4 * SIDE * SIDE) and a.scaler._growth_tracker == 4
    return a.state()


@pytest.fixture(scope="module")
def half(batches, tmp_path_factory):
    """Run B: two steps (one of them the skipped one), `save()` of iso.ckpt, the third step BEFORE `wait()`; then b.ckpt, saved and
    waited for -> (b.ckpt, the Run, iso.ckpt, clones of the state_dict and the moments taken just before iso.ckpt's save)."""
    d = tmp_path_factory.mktemp("ckpt")
    path, iso = str(d / "b.ckpt"), str(d / "iso.ckpt")
    b = Run()
    b.seed()
    b.steps(batches, 0, 2, bad_step=BAD_STEP)
    before = {k: v.detach().clone() for k, v in b.ld.state_dict().items()}
    moments = {k: (m.clone(), v.clone()) for k, (m, v) in b.opt.state.items()}
    b.ck.save(iso, global_step=2, epoch=0, batch_in_epoch=2)
    b.steps(batches, 2, 1)
    b.ck.wait()
    b.ck.save(path, global_step=3, epoch=0, batch_in_epoch=3, extra={"note": "half"})
    b.ck.wait()
    return path, b, iso, before, moments


def test_exact_resume(batches, straight, half):
    """Run B's file into a fresh model built from another seed, with a fresh optimizer, schedule and scaler, then three more
    steps: all 441 parameters, both moments, every shadow, `num_updates`, the scaler, the step count, the rate and the next
    draw of every generator equal run A's."""
    path = half[0]
    c = Run(seed=23)
    assert not _same_bits(c.opt.params["bbox_uncond_vector"], half[1].opt.params["bbox_uncond_vector"])
    random.seed(99)
    torch.manual_seed(99)
    at = c.ck.load(path)
    assert at == {"global_step": 3, "epoch": 0, "batch_in_epoch": 3, "extra": {"note": "half"}, "monitor": None}
    assert c.opt.steps == 2 and c.sched.last_epoch == 3 and c.scaler.state_dict() == half[1].scaler.state_dict()
    c.steps(batches, 3, 3)
    _assert_same_state(c.state(), straight)


def test_exact_resume_with_accumulation(batches, tmp_path):
    """The same with `GradAccumulator(opt, 2)`: four windows straight against two, a save between windows, a load into a fresh
    model and two more.  Inside a window `save` refuses."""
    a = Run(accumulate=2)
    a.seed()
    a.steps(batches, 0, 4, bad_step=BAD_STEP)
    assert a.skipped == [False, True, False, False]
    want = a.state()
    b = Run(accumulate=2)
    b.seed()
    b.steps(batches, 0, 2, bad_step=BAD_STEP)
    path = str(tmp_path / "acc.ckpt")
    b.ck.save(path, 2, 0, 4)
    b.ck.wait()
    c = Run(seed=23, accumulate=2)
    c.ck.load(path)
    c.steps(batches, 2, 2)
    _assert_same_state(c.state(), want)
    b.ld.training_step(batches[0], 0, scaler=b.scaler, allreduce=False)     # inside a window: no checkpoint
    b.acc.add(b.ld.adapter_grads, scale=b.ld.adapter_grads_scale)
    with pytest.raises(RuntimeError, match="between optimizer steps"):
        b.ck.save(str(tmp_path / "w.ckpt"), 2, 0)
    assert sorted(os.listdir(tmp_path)) == ["acc.ckpt"]


def test_snapshot_isolation(half):
    """`save()` after two steps, one more step BEFORE `wait()` (the `half` fixture): the file holds the state at the save, not
    the later one; `verify` passes on it."""
    from mobi_amd import checkpoint
    _, r, path, before, moments = half
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert "pytorch-lightning_version" not in ckpt and ckpt["global_step"] == 2 and ckpt["mobi_amd"]["format"] == 1
    assert list(ckpt["state_dict"]) == list(before)
    now = r.ld.state_dict()
    moved = 0
    for k, v in ckpt["state_dict"].items():
        assert not v.is_cuda and v.dtype == before[k].dtype and _same_bits(v, before[k]), k
        moved += int(not _same_bits(v, now[k]))
    assert moved >= 2 * 432                            # the trained tensors and their shadows went on
    assert int(ckpt["state_dict"]["model_ema.num_updates"]) == 2 and int(r.ld.model_ema.num_updates) == 3
    names = list(r.opt.params)
    opt_sd = ckpt["optimizer_states"][0]
    assert sorted(names[i] for i in opt_sd["state"]) == sorted(moments)
    moved = 0
    for i, e in opt_sd["state"].items():
        assert float(e["step"]) == 1.0                 # (two steps, one of them skipped)
        assert _same_bits(e["exp_avg"], moments[names[i]][0]) and _same_bits(e["exp_avg_sq"], moments[names[i]][1]), names[i]
        moved += int(not _same_bits(e["exp_avg"], r.opt.state[names[i]][0]))
    assert moved >= 432
    assert ckpt["lr_schedulers"] == [{"last_epoch": 2, "base_lrs": [LR]}]
    fp32 = [k for k, v in before.items() if v.dtype == torch.float32 and v.numel()]
    assert len(ckpt["mobi_amd"]["digests"]) == len(fp32) + 2 * len(moments)
    assert checkpoint.verify_file(path) == (len(fp32) + 2 * len(moments), [])


def test_refusals(batches, half, tmp_path):
    from mobi_amd import checkpoint
    path, b = half[0], half[1]
    mine = str(tmp_path / "r.ckpt")
    with open(path, "rb") as f:
        data = f.read()
    with open(mine, "wb") as f:
        f.write(data)
    # a non-finite moment: NonFiniteState names it, the file keeps its bytes
    name = list(b.opt.params)[7]
    index = 7
    keep = b.opt.state[name][0].view(-1)[2].clone()
    b.opt.state[name][0].view(-1)[2] = float("inf")
    try:
        with pytest.raises(checkpoint.NonFiniteState, match=rf"optimizer\.{index}\.exp_avg'"):
            b.ck.save(mine, 3, 0, 3)
        b.ck.wait()
    finally:
        b.opt.state[name][0].view(-1)[2] = keep
    assert open(mine, "rb").read() == data and os.listdir(tmp_path) == ["r.ckpt"]
    # inside ema_scope(): weights and shadows have traded places
    with b.ld.ema_scope():
        with pytest.raises(RuntimeError, match="ema_scope"):
            b.ck.save(mine, 3, 0, 3)
    b.ck.wait()
    assert open(mine, "rb").read() == data
    b.ck.save(mine, 3, 0, 3)                           # and outside again it saves: the same tensors, the same digests
    b.ck.wait()
    ckpt = torch.load(mine, map_location="cpu", weights_only=False)
    assert ckpt["mobi_amd"]["digests"] == torch.load(path, map_location="cpu", weights_only=False)["mobi_amd"]["digests"]
    # one corrupted element under the old digests
    victim = "model.diffusion_model.middle_block.1.transformer_blocks.0.cond_adapter_connector.weight"
    _bits_view = ckpt["state_dict"][victim].view(torch.int32)
    _bits_view.view(-1)[5] ^= 1
    torch.save(ckpt, mine)
    assert [n for n, _ in checkpoint.verify_file(mine)[1]] == [victim]
    c = Run(seed=23)
    with pytest.raises(checkpoint.DigestMismatch, match="cond_adapter_connector.weight"):
        c.ck.load(mine)
    assert c.ck.load(mine, strict_digests=False)["global_step"] == 3


def test_reader_compatibility(half):
    """A fresh `LatentDiffusion(ckpt_path=file)` -- `init_from_ckpt`, the path the sampling scripts take -- holds the trained
    weights and shadows bit for bit."""
    path, b = half[0], half[1]
    at_save = b.ld.state_dict()
    fresh = _model(seed=23, ckpt_path=path)
    sd = fresh.state_dict()
    checked = 0
    for k, v in at_save.items():
        if k.startswith(("model.", "model_ema.", "bbox_uncond_vector", "learnable_vector")):
            assert _same_bits(sd[k], v), k
            checked += 1
    assert checked > 2 * 432


class _TrainerCase:
    """Four batches per epoch in `train.epoch_order`, two epochs, save_top_k=1, every_n_steps=3, log_every=4."""

    def __init__(self, batches):
        self.batches = batches

    def train_batches(self, epoch, start_batch=0):
        from mobi_amd import train
        return [self.batches[j] for j in train.epoch_order(len(self.batches), 3, epoch)][start_batch:]

    def val_batches(self):
        return self.batches[:2]

    def trainer(self, seed, ckpt_dir, max_steps=None):
        from mobi_amd import train
        return train.Trainer(_wire(_model(seed)), max_epochs=2, scaler=train.GradScaler(init_scale=None), ckpt_dir=ckpt_dir,
                             every_n_steps=3, save_top_k=1, seed=3, log_every=4, max_steps=max_steps)

    @staticmethod
    def final(tr):
        out = {k: v.detach().clone() for k, v in tr.model.state_dict().items()}
        for k, (m, v) in tr.optimizer.state.items():
            out["exp_avg/" + k], out["exp_avg_sq/" + k] = m.clone(), v.clone()
        return out, {"scaler": tr.scaler.state_dict(), "steps": tr.optimizer.steps, "lr": tr.optimizer.lr,
                     "global_step": tr.global_step, "random": random.random(), "device": float(torch.rand(1, device="cuda"))}


@pytest.fixture(scope="module")
def full_run(batches, tmp_path_factory):
    """The uninterrupted run -> (the case, its final state, the name of the epoch file with the lower monitored value, what
    `test_trainer_keeps_last_and_the_best_epoch_file` asserts on)."""
    case = _TrainerCase(batches)
    d1 = str(tmp_path_factory.mktemp("full"))
    tr = case.trainer(5, d1).fit(case.train_batches, case.val_batches)
    want = case.final(tr)
    monitored = [v["val/loss_simple_ema"] for v in tr.val_history]
    best = f"epoch={int(np.argmin(monitored)):06d}.ckpt"
    seen = {"global_step": tr.global_step, "history": tr.history, "monitored": monitored, "files": sorted(os.listdir(d1)),
            "last": torch.load(os.path.join(d1, "last.ckpt"), map_location="cpu", weights_only=False)}
    return case, want, best, seen


@pytest.mark.parametrize("stop", [5, 7])
def test_trainer_resumes_exactly(full_run, tmp_path, stop):
    """A run stopped after step 5 (its `last.ckpt`: the end of epoch 0) or after step 7 (its `last.ckpt`: step 6, inside epoch 1),
    resumed by a second trainer over a fresh model from another seed, ends bit-equal to the uninterrupted run and keeps the same
    files."""
    case, want, best, _ = full_run
    d2 = str(tmp_path)
    case.trainer(5, d2, max_steps=stop).fit(case.train_batches, case.val_batches)
    assert sorted(os.listdir(d2)) == ["epoch=000000.ckpt", "last.ckpt"]
    at = torch.load(os.path.join(d2, "last.ckpt"), map_location="cpu", weights_only=False)
    assert (at["global_step"], at["epoch"], at["mobi_amd"]["batch_in_epoch"]) == ((4, 1, 0) if stop == 5 else (6, 1, 2))
    resumed = case.trainer(23, d2).fit(case.train_batches, case.val_batches, resume=os.path.join(d2, "last.ckpt"))
    _assert_same_state(case.final(resumed), want)
    assert sorted(os.listdir(d2)) == [best, "last.ckpt"]
    assert [r["step"] for r in resumed.history] == [8]


def test_trainer_keeps_last_and_the_best_epoch_file(full_run, batches):
    """Four batches per epoch, two epochs, save_top_k=1, every_n_steps=3, log_every=4: the directory holds `last.ckpt` plus exactly
    one `epoch=...` file, the one with the lower `val/loss_simple_ema`; `last.ckpt` is the end of the run whether or not the last
    epoch's own file was kept; `history` has one row per `log_every` steps."""
    from mobi_amd import train
    _, _, best, seen = full_run
    assert train.epoch_order(len(batches), 3, 0) != train.epoch_order(len(batches), 3, 1)
    assert seen["global_step"] == 8 and [r["step"] for r in seen["history"]] == [4, 8]
    assert all(set(r) == {"step", "train/loss", "train/loss_simple", "train/loss_vlb"} for r in seen["history"])
    monitored = seen["monitored"]
    assert len(monitored) == 2 and monitored[0] != monitored[1]
    assert seen["files"] == [best, "last.ckpt"]
    last = seen["last"]
    assert (last["global_step"], last["epoch"], last["mobi_amd"]["batch_in_epoch"]) == (8, 2, 0)
    assert list(last["mobi_amd"]["monitor"]["best"]) == [best]
    assert last["mobi_amd"]["monitor"]["best"][best]["value"] == min(monitored)
