"""GPU: sampling while training -- `mobi_image_grid` / `ops.image_grid` bit for bit against a numpy restatement of make_grid and
the logger's rescale; `LatentDiffusion.log_images` against the chain of calls it stands for; that the sampling path sees weights
the optimizer has just moved; that a run under `train.Trainer` with an `ImageLogger` ends bit-equal to the run without one, also
through gradient accumulation and a resume.

The network is the reduced one of tests/test_gpu_models.py::test_harness_flow_reference_spelling (mobi_nusc_256.yaml at
model_channels 64, VAEs at ch 32, a one-layer CLIP tower, 64 x 64 pictures, latent 8 x 8, two camera / lidar pairs, fp16)."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from oracle import weights as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2


# ----------------------------------------------------------------------------------------------------------------------
# mobi_image_grid
def grid_ref(x, max_images, nrow=4, padding=2, clamp=True, rescale=True):
    """The reference's chain (main.py:388-393, :357-362), restated in numpy: clamp, torchvision's make_grid (pad_value 0), the
    rescale of the WHOLE grid -- its frame included, which comes out as 127 --, * 255, astype(uint8), all in float32; a uint8
    source only goes through make_grid."""
    x = x[:max_images]
    if x.dtype == np.float32 and clamp:
        x = x.clip(-1, 1)
    n, c, h, w = x.shape
    if c == 1:
        x = np.concatenate([x, x, x], axis=1)
    if n == 1:
        grid = x[0]
    else:
        xmaps = min(nrow, n)
        ymaps = -(-n // xmaps)
        grid = np.zeros((3, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding), x.dtype)
        for k in range(n):
            y0, x0 = (k // xmaps) * (h + padding) + padding, (k % xmaps) * (w + padding) + padding
            grid[:, y0:y0 + h, x0:x0 + w] = x[k]
    if grid.dtype == np.float32:
        if rescale:
            grid = (grid + 1) / 2
        assert grid.dtype == np.float32
        grid = (grid * 255).astype(np.int32).astype(np.uint8)           # (through int32: values outside [0, 255] keep their low 8 bits)
    return np.ascontiguousarray(grid.transpose(1, 2, 0))


def _f32(shape, seed):
    """Uniform values in [-1.3, 1.3] with the rounding boundaries planted: -1, 1, +-1.5 and k / 127.5 - 1, k = 0 .. 255 (where
    (x + 1) / 2 * 255 lands on or next to an integer and a fused multiply-add would round the other way) -- as many as fit."""
    rng = np.random.RandomState(seed)
    a = rng.uniform(-1.3, 1.3, size=int(np.prod(shape))).astype(np.float32)
    special = np.concatenate([np.float32([-1, 1, 1.5, -1.5]), np.arange(256, dtype=np.float32) / np.float32(127.5) - np.float32(1)])
    if special.size > a.size:
        special = np.concatenate([special[:4], special[4::3]])
    a[rng.permutation(a.size)[:special.size]] = special[:a.size]
    return a.reshape(shape)


def _u8(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


SOURCES = {"single_f32": (lambda: _f32((1, 3, 5, 7), 1), 8),           # one image: no padding
           "gray_f32": (lambda: _f32((5, 1, 6, 9), 2), 8),             # C = 1, two rows, three empty cells, odd sizes
           "row_u8": (lambda: _u8((4, 3, 8, 8), 3), 8),                # exactly one row, pass-through
           "cut_u8": (lambda: _u8((8, 3, 16, 12), 4), 6),              # truncation to max_images
           "all_f32": (lambda: _f32((3, 3, 9, 11), 5), 8)}             # every planted value in one tensor (3 * 3 * 99 > 260)


@pytest.mark.parametrize("name", list(SOURCES))
def test_image_grid_single_source(name):
    from mobi_amd import ops
    make, max_images = SOURCES[name]
    x = make()
    if name == "gray_f32":
        assert {-1.0, 1.0, 1.5, -1.5} <= set(x.reshape(-1).tolist()) and x.size >= 260
    got = ops.image_grid({name: torch.from_numpy(x).cuda()}, max_images)
    want = grid_ref(x, max_images)
    assert list(got) == [name] and got[name].dtype == np.uint8 and got[name].shape == want.shape
    assert got[name].shape == ops.image_grid_shape(x.shape[0], x.shape[2], x.shape[3], max_images) + (3,)
    assert np.array_equal(got[name], want)


def test_image_grid_one_table_of_four_and_the_options():
    """The four sources of the single cases as ONE table (max_images = 6 for all: the offsets of four pictures of different sizes,
    none a multiple of 4 bytes apart by itself), then `clamp` / `rescale` off and other `nrow` / `padding`."""
    from mobi_amd import ops
    keys = ["single_f32", "gray_f32", "row_u8", "cut_u8"]
    xs = {k: SOURCES[k][0]() for k in keys}
    got = ops.image_grid({k: torch.from_numpy(v).cuda() for k, v in xs.items()}, 6)
    assert list(got) == keys
    for k in keys:
        assert np.array_equal(got[k], grid_ref(xs[k], 6)), k
    assert sum(1 for k in keys if got[k].size % 4) >= 1
    unit = np.random.RandomState(9).uniform(0, 1, size=(5, 3, 7, 5)).astype(np.float32)
    unit.reshape(-1)[:256] = np.arange(256, dtype=np.float32) / np.float32(255)
    wild = _f32((3, 1, 4, 6), 10)
    for kw in (dict(rescale=False), dict(clamp=False), dict(rescale=False, clamp=False)):
        for name, x in (("unit", unit), ("wild", wild)):
            got = ops.image_grid({name: torch.from_numpy(x).cuda()}, 8, nrow=3, padding=1, **kw)[name]
            assert np.array_equal(got, grid_ref(x, 8, nrow=3, padding=1, **kw)), (name, kw)
    assert np.array_equal(ops.image_grid({"p0": torch.from_numpy(wild).cuda()}, 2, nrow=1, padding=0)["p0"], grid_ref(wild, 2, 1, 0))


def test_image_grid_refusals_launch_nothing():
    """A 16-bit source and a 17-entry table are refused before the launch: the output buffer keeps its fill."""
    from mobi_amd import _lib, ops
    lib = _lib.load()
    x = torch.from_numpy(_f32((2, 3, 4, 4), 6)).cuda()
    with pytest.raises(_lib.EngineError, match="unsupported"):
        ops.image_grid({"half": x.half()}, 8)
    with pytest.raises(_lib.EngineError, match="unsupported"):
        ops.image_grid({f"k{i}": x for i in range(17)}, 8)
    assert len(ops.image_grid({f"k{i}": x for i in range(16)}, 8)) == 16
    hg, wg = ops.image_grid_shape(2, 4, 4, 8)
    each = (hg * wg * 3 + 3) // 4 * 4
    out = torch.full((17 * each,), 0x5A, dtype=torch.uint8, device="cuda")
    half = x.half()
    for count, src in ((1, half), (17, x)):
        t = (_lib.ImageGridSource * count)()
        for i, s in enumerate(t):
            s.data, s.elem_bytes, s.n, s.c, s.h, s.w, s.out_offset = src.data_ptr(), src.element_size(), 2, 3, 4, 4, i * each
        assert lib.mobi_image_grid(t, count, 8, 4, 2, 1, 1, C.c_void_p(out.data_ptr()), out.numel(), ops._stream()) == -2
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())


# ----------------------------------------------------------------------------------------------------------------------
# the model
_TEMPLATES = {}


def _template(use_ema):
    """The reduced model on the host, built once per module (instantiating and filling it takes longer than any test here)."""
    if use_ema not in _TEMPLATES:
        from mobi_amd.ldm.util import instantiate_from_config, load_config
        cfg = load_config(os.path.join(ROOT, "configs", "mobi_nusc_256.yaml"),
                          ["latent_size=8", "image_height=64", "use_lidar=True",
                           "model.params.lidar_stage_config.params.ckpt_path=null",
                           "model.params.unet_config.params.model_channels=64",
                           "model.params.first_stage_config.params.ddconfig.ch=32",
                           "model.params.lidar_stage_config.params.ddconfig.ch=32",
                           "model.params.cond_stage_config.params.clip_config.hidden_size=1024",
                           "model.params.cond_stage_config.params.clip_config.intermediate_size=256",
                           "model.params.cond_stage_config.params.clip_config.num_hidden_layers=1",
                           "model.params.cond_stage_config.params.clip_config.num_attention_heads=16",
                           "model.params.cond_stage_config.params.clip_config.image_size=28",
                           "model.params.cond_stage_config.params.clip_config.patch_size=14"])
        cfg["model"]["params"]["use_ema"] = use_ema
        torch.manual_seed(19)                                            # (the EMA shadows keep the constructor's random init)
        model = instantiate_from_config(cfg["model"])
        W.fill_module_(model, seed=19)
        model.learning_rate = 1e-3
        _TEMPLATES[use_ema] = model.eval()
    return _TEMPLATES[use_ema]


def _model(seed=19, use_ema=False):
    """A copy of the template on the device; another seed: the trainable UNet tensors, the box embedder, `bbox_uncond_vector` and
    every EMA shadow moved by noise of that seed (a generator of its own: the global streams are not touched)."""
    import copy
    import mobi_amd
    mobi_amd.set_engine_dtype(torch.float16)
    model = copy.deepcopy(_template(use_ema)).cuda().eval()
    if seed != 19:
        gen = torch.Generator(device="cuda").manual_seed(seed)
        opt = model.configure_optimizers()
        opt = opt[0][0] if isinstance(opt, tuple) else opt
        moved = list(opt.params.values()) + ([b for n, b in model.model_ema.named_buffers() if b.is_floating_point() and b.dim()]
                                             if use_ema else [])
        with torch.no_grad():
            for t in moved:
                t.add_(torch.randn(t.shape, generator=gen, device="cuda") * (0.05 * float(t.abs().mean()) + 1e-4))
    return model


def _batch(tag):
    s = lambda name, shape, **kw: W.synth_input(f"il.{tag}.{name}", shape, **kw)
    batch = {"image": {"GT": s("img", (B, 3, 64, 64), kind="uniform"), "inpaint_mask": torch.ones(B, 1, 64, 64),
                       "cond": {"ref_image": s("ref", (B, 3, 28, 28)), "ref_bbox": s("bbox", (B, 8, 3), kind="uniform") * 0.5 + 0.5}},
             "lidar": {"range_data": s("rng", (B, 2, 64, 64), kind="uniform"), "range_mask": torch.ones(B, 1, 64, 64),
                       "range_instance_mask": (s("inst", (B, 1, 64, 64)) > 1.0).float(),
                       "min_depth_obj": torch.tensor([-0.6, -0.3]), "max_depth_obj": torch.tensor([0.2, 0.5]),
                       "width_crop": torch.tensor([32, 64]),
                       "cond": {"ref_image": s("ref", (B, 3, 28, 28)), "ref_bbox": s("bbox2", (B, 8, 3), kind="uniform") * 0.5 + 0.5}}}
    batch["image"]["inpaint_mask"][:, :, 16:48, 16:48] = 0
    batch["lidar"]["range_mask"][:, :, 16:48, 16:48] = 0
    batch["image"]["inpaint_image"] = batch["image"]["GT"] * batch["image"]["inpaint_mask"]
    batch["lidar"]["range_data_inpaint"] = batch["lidar"]["range_data"] * batch["lidar"]["range_mask"]
    move = lambda d: {k: move(v) if isinstance(v, dict) else v.cuda() for k, v in d.items()}
    return move(batch)


def _clone(x):
    return {k: _clone(v) for k, v in x.items()} if isinstance(x, dict) else x.clone()


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _log(model, batch, seed, **kw):
    _seed(seed)
    return model.log_images(_clone(batch), **kw)


def _assert_same_log(got, want):
    assert list(got) == list(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def _same_metrics(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(np.float64(a[k]), np.float64(b[k]), equal_nan=True) for k in a)


SAMPLED_KEYS = ("range_depth_pred", "range_int_pred")                  # fp32 collages that hold the decoded sample


@pytest.mark.parametrize("use_ema", [False, True], ids=["live", "ema"])
def test_log_images_equals_its_parts(use_ema):
    """get_input -> DDIMSampler(model).sample(S, n, shape, cond, verbose=False, eta=1., rest=z[:, 4:]) -> decode_sample -> log_data,
    written out, under one seed: every entry `torch.equal` (both sides issue the same launches).  With `use_ema` the sampling runs
    on the shadows (the hand-written chain enters `ema_scope` as `log_images` does) and the exchange leaves every weight and shadow
    as it was.  A second call with unchanged weights reuses the model's one sampler and, without EMA swaps, its captured graph.
    S = 4, not 3: the uniform schedule of 3 steps is [1, 334, 667, 1000] (`make_ddim_timesteps`: 1000 // 3 = 333, so a fourth entry,
    plus one), which reads past the 1000-entry alpha table -- in the reference as here; 4 is the next count that divides 1000."""
    from mobi_amd.ldm.models.diffusion.ddim import DDIMSampler
    model, batch, S = _model(19, use_ema), _batch("a"), 4
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    _seed(7)
    mine = _clone(batch)
    data = model.get_input(mine, model.first_stage_key, force_c_encode=True, return_vae_rec=True)
    n = data["z"].shape[0]
    assert n == 2 * B
    with model.ema_scope():
        samples, _ = DDIMSampler(model).sample(S, n, (model.channels, model.image_size, model.image_size), data["cond"],
                                               verbose=False, eta=1., rest=data["z"][:, 4:])
        h_camera, h_lidar = model.decode_sample(samples, data.get("z_lidar"))
    want, want_metrics = model.log_data(mine, data, h_camera, h_lidar, log_metrics=True, split="train")
    assert {"image_preds", "image_input-rec", "range_depth_pred", "range_int_pred"} <= set(want) and len(want_metrics) == 16
    assert model.last_lidar_metrics is None
    got = _log(model, batch, 7, ddim_steps=S)
    _assert_same_log(got, want)
    assert _same_metrics(model.last_lidar_metrics, want_metrics) and all(k.startswith("train/") for k in want_metrics)
    sampler = model._log_sampler
    graphs = dict(sampler._step_graphs)
    _assert_same_log(_log(model, batch, 7, ddim_steps=S), want)
    assert model._log_sampler is sampler
    if not use_ema:
        assert list(sampler._step_graphs.values()) == list(graphs.values())      # nothing was captured again
    assert any(not torch.equal(_log(model, batch, 8, ddim_steps=S)[k], want[k]) for k in SAMPLED_KEYS)   # the seed is what it draws from
    after = model.state_dict()
    assert sorted(after) == sorted(before) and all(torch.equal(after[k], before[k]) for k in before)
    if use_ema:
        live, shadows = dict(model.model.named_parameters()), dict(model.model_ema.named_buffers())
        assert any(not torch.equal(shadows[s], live[m]) for m, s in model.model_ema.m_name2s_name.items())   # (the swap matters)
    with pytest.raises(NotImplementedError, match="9-channel"):
        model.sample_log(data["cond"], n, False, None)
    # log_metrics=False leaves the attribute alone
    model.last_lidar_metrics = "kept"
    _log(model, batch, 7, ddim_steps=S, log_metrics=False)
    assert model.last_lidar_metrics == "kept"


def test_sampling_sees_the_weights_the_optimizer_moved():
    """One `training_step` + `step_scaled`, then `log_images`: equal to a model built fresh and loaded with the stepped state_dict,
    different from what was logged before the step (else a folded table, a packed copy or the captured graph is stale)."""
    from mobi_amd import train
    a, batch = _model(19), _batch("a")
    before = _log(a, batch, 7, ddim_steps=2)
    opt = a.configure_optimizers()
    opt = opt[0][0] if isinstance(opt, tuple) else opt
    scaler = train.GradScaler(init_scale=None)
    a.train()
    _seed(3)
    a.training_step(_clone(batch), 0, scaler=scaler)
    res = opt.step_scaled(a.adapter_grads, scaler=scaler)
    assert not res.found_inf
    a.eval()
    after = _log(a, batch, 7, ddim_steps=2)
    fresh = _model(23)
    fresh.load_state_dict(a.state_dict())
    _assert_same_log(after, _log(fresh, batch, 7, ddim_steps=2))
    for k in SAMPLED_KEYS:
        assert not torch.equal(after[k], before[k]), k


# ----------------------------------------------------------------------------------------------------------------------
# under the Trainer
class _Case:
    """Two epochs of two optimizer steps each (k micro-batches per step), one validation batch, a checkpoint every 2 steps; the
    logger fires at steps 2 and 4, on the training batch and on the validation batch: DDIM-2."""

    def __init__(self, k):
        self.k = k
        self.train = [_batch(f"t{i}") for i in range(2 * k)]
        self.val = [_batch("v")]

    def train_batches(self, epoch, start_batch=0):
        return [_clone(b) for b in self.train][start_batch:]

    def val_batches(self):
        return [_clone(b) for b in self.val]

    def fit(self, seed, root=None, logger=True, max_steps=None, resume=None, max_images=8):
        from mobi_amd import train
        lg = train.ImageLogger(os.path.join(root, "pics"), batch_frequency=2, max_images=max_images, log_first_step=True, seed=11,
                               log_images_kwargs={"ddim_steps": 2}) if logger else None
        tr = train.Trainer(_model(seed, use_ema=True), max_epochs=2, accumulate_grad_batches=self.k,
                           scaler=train.GradScaler(init_scale=None), seed=3, log_every=2, max_steps=max_steps, image_logger=lg,
                           ckpt_dir=os.path.join(root, "ckpt") if root else None, every_n_steps=2 if root else None,
                           log_dir=os.path.join(root, "logs") if logger else None)
        return tr.fit(self.train_batches, self.val_batches, resume=resume)


def _final(tr):
    out = {"param/" + k: p.detach().clone() for k, p in tr.optimizer.params.items()}
    for k, (m, v) in tr.optimizer.state.items():
        out["exp_avg/" + k], out["exp_avg_sq/" + k] = m.clone(), v.clone()
    out.update({"ema/" + k: b.clone() for k, b in tr.model.model_ema.named_buffers()})
    np_state = np.random.get_state()
    out["rng/torch"], out["rng/device"] = torch.get_rng_state(), torch.cuda.get_rng_state()
    out["rng/numpy"] = torch.from_numpy(np_state[1].astype(np.int64))
    host = {"scaler": tr.scaler.state_dict(), "steps": tr.optimizer.steps, "lr": tr.optimizer.lr, "global_step": tr.global_step,
            "python": random.getstate(), "numpy": np_state[2:]}
    return out, host


def _assert_same_final(got, want):
    (gt, gh), (wt, wh) = got, want
    assert gh == wh
    assert sorted(gt) == sorted(wt)
    for k in wt:
        assert gt[k].dtype == wt[k].dtype and torch.equal(gt[k], wt[k]), k


def _names(split, key, step, epoch, b):
    return os.path.join("images", split, f"{key}_gs-{step:06d}_e-{epoch:06d}_b-{b:06d}.png")


@pytest.fixture(scope="module")
def logged_run(tmp_path_factory):
    case, root = _Case(1), str(tmp_path_factory.mktemp("logged"))
    tr = case.fit(5, root)
    return case, root, tr, _final(tr)


def test_the_logger_does_not_move_the_run(logged_run):
    """Every trained parameter, both moments, every EMA shadow, the scaler and the four generator states at the end of four optimizer
    steps are bit-equal with and without the logger; its files are there, decode to what `ops.image_grid` returned, and
    `image_history` / metrics.jsonl hold the lidar scores of the sampled objects."""
    import json
    from PIL import Image
    case, root, tr, final = logged_run
    assert tr.global_step == 4 and len([k for k in final[0] if k.startswith("param/")]) > 432
    _assert_same_final(_final(case.fit(5, logger=False)), final)
    rows = tr.image_history
    assert [(r["step"], r["epoch"], r["batch_idx"], r["split"]) for r in rows] == \
        [(2, 0, 1, "train"), (2, 0, 0, "val"), (4, 1, 1, "train"), (4, 1, 0, "val")]
    for r in rows:
        scores = {k for k in r if k not in ("step", "epoch", "batch_idx", "split")}
        assert len(scores) == 16 and all(k.startswith(r["split"] + "/") for k in scores)
        assert {r["split"] + "/mse/object_pred_depth", r["split"] + "/median_error/mask_rec_int"} <= scores
        assert all(isinstance(r[k], float) for k in scores) and np.isfinite(r[r["split"] + "/mse/mask_pred_depth"])
    pics = tr.image_logger.last_images
    assert {"image_preds", "image_preds_no_box", "image_input-rec", "range_depth_pred", "range_int_pred"} <= set(pics)
    for r in rows:
        for key in pics:
            assert os.path.exists(os.path.join(root, "pics", _names(r["split"], key, r["step"], r["epoch"], r["batch_idx"]))), (r, key)
    for key, arr in pics.items():                                        # the last call: the validation batch after step 4
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, "pics", _names("val", key, 4, 1, 0)))), arr), key
    assert pics["range_depth_pred"].shape == (5 * 64 + 4, B * (64 + 2) + 2, 3)          # B views side by side, 2 pixels of padding
    lines = [json.loads(x) for x in open(os.path.join(root, "logs", "metrics.jsonl"))]
    assert [x["kind"] for x in lines] == ["images", "train", "images", "val", "images", "train", "images", "val"]


def test_the_logger_does_not_move_a_run_with_accumulation(tmp_path):
    """accumulate_grad_batches = 2: the hook runs after the window's optimizer step only (batch indices 1 and 3), and the run ends
    bit-equal to the one without a logger.  (max_images = 1: the pictures are single images, a third of the PNG encoding.)"""
    case = _Case(2)
    tr = case.fit(5, str(tmp_path), max_images=1)
    assert tr.global_step == 4
    assert [(r["step"], r["batch_idx"], r["split"]) for r in tr.image_history] == [(2, 3, "train"), (2, 0, "val"), (4, 3, "train"), (4, 0, "val")]
    _assert_same_final(_final(case.fit(5, logger=False)), _final(tr))


def test_a_resumed_run_with_the_logger_ends_bit_equal(logged_run, tmp_path):
    """Stopped after step 2 (`last.ckpt`: step 2, the end of epoch 0's batches) and resumed by a second trainer over a fresh model from
    another seed: the same final state, and the pictures of step 4 are the same files byte for byte."""
    case, root, tr, final = logged_run
    mine = str(tmp_path)
    stopped = case.fit(5, mine, max_steps=2)
    assert stopped.global_step == 2
    at = torch.load(os.path.join(mine, "ckpt", "last.ckpt"), map_location="cpu", weights_only=False)
    assert (at["global_step"], at["epoch"], at["mobi_amd"]["batch_in_epoch"]) == (2, 0, 2)
    resumed = case.fit(23, mine, resume=os.path.join(mine, "ckpt", "last.ckpt"))
    _assert_same_final(_final(resumed), final)
    step4 = sorted(f for split in ("train", "val") for f in os.listdir(os.path.join(root, "pics", "images", split)) if "_gs-000004_" in f)
    assert len(step4) >= 2 * 5
    for split in ("train", "val"):
        for f in os.listdir(os.path.join(root, "pics", "images", split)):
            if "_gs-000004_" in f:
                a = open(os.path.join(root, "pics", "images", split, f), "rb").read()
                b = open(os.path.join(mine, "pics", "images", split, f), "rb").read()
                assert a == b, (split, f)
