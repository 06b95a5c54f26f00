"""CPU: the host side of sampling while training -- `LatentDiffusion.log_images` / `sample_log` and `train.ImageLogger` carry the
reference's signatures (tests/golden/reference_interfaces_logger.json, read from the reference with ast by
tests/golden/make_reference_interfaces_logger.py), `check_frequency` against a written-out table, the logger's RNG and mode
isolation around a `log_images` that raises, `Trainer`'s metrics.jsonl, and `mobi_image_grid`'s refusals (host checks: no launch)."""
import ctypes as C
import inspect
import json
import os
import random

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden():
    with open(os.path.join(HERE, "golden", "reference_interfaces_logger.json")) as f:
        return json.load(f)["signatures"]


def _mine(fn):
    ps = [p for p in inspect.signature(fn).parameters.values() if p.name != "self"]
    plain = [p for p in ps if p.kind == p.POSITIONAL_OR_KEYWORD]
    kw = [p.name for p in ps if p.kind == p.VAR_KEYWORD]
    return {"names": [p.name for p in plain], "defaults": [p.default for p in plain if p.default is not p.empty],
            "kwarg": kw[0] if kw else None}


@pytest.mark.parametrize("name", ["log_images", "sample_log"])
def test_model_signatures_equal_the_reference(name):
    from mobi_amd.ldm.models.diffusion.ddpm import LatentDiffusion
    assert _mine(getattr(LatentDiffusion, name)) == _golden()[f"LatentDiffusion.{name}"]


def test_image_logger_signature_is_the_reference_plus_save_dir_and_seed():
    from mobi_amd import train
    ref, mine = _golden()["ImageLogger.__init__"], _mine(train.ImageLogger.__init__)
    assert mine["names"] == ["save_dir"] + ref["names"] + ["seed"]
    assert mine["defaults"] == [400, 8] + ref["defaults"] + [0]          # (the two the reference leaves without a default: main.py:604-613)
    assert _mine(train.ImageLogger.check_frequency) == _golden()["ImageLogger.check_frequency"]


def _fired(logger, indices):
    return [i for i in indices if logger.check_frequency(i)]


def test_check_frequency_tables(tmp_path):
    from mobi_amd import train
    idx = [0, 1, 2, 399, 400, 401, 799, 800, 1200, 1201]
    # the reference's installation (main.py:604-613): every 400 batch indices, index 0 included
    ref = train.ImageLogger(str(tmp_path), batch_frequency=400, max_images=8, clamp=False, log_on_batch_idx=True, log_first_step=True)
    assert ref.log_steps == [] and _fired(ref, idx) == [0, 400, 800, 1200]
    assert _fired(train.ImageLogger(str(tmp_path), batch_frequency=400), idx) == [400, 800, 1200]          # index 0 without log_first_step
    # increase_log_steps=False: log_steps = [batch_frequency], popped by the first call that fires, whatever fired it
    lg = train.ImageLogger(str(tmp_path), batch_frequency=3, increase_log_steps=False, log_first_step=True)
    assert lg.log_steps == [3]
    assert _fired(lg, [0]) == [0] and lg.log_steps == []
    assert _fired(lg, [1, 2, 3, 4, 5, 6]) == [3, 6]
    lg = train.ImageLogger(str(tmp_path), batch_frequency=3, increase_log_steps=False)
    assert _fired(lg, [0, 1, 2]) == [] and lg.log_steps == [3]
    assert _fired(lg, [3, 3]) == [3, 3] and lg.log_steps == []            # (a pop from an empty list is swallowed, main.py:409-412)
    # batch_frequency 2: the GPU tests' setting
    assert _fired(train.ImageLogger(str(tmp_path), batch_frequency=2, log_first_step=True), range(0, 6)) == [0, 2, 4]


class _Trainer:
    global_step, current_epoch = 7, 1


class _RaisingModel(torch.nn.Module):
    """`log_images` draws from every host generator (and the device's, where there is one), then raises."""

    def __init__(self):
        super().__init__()
        self.seen = None

    def log_images(self, batch, split="train", **kw):
        self.seen = (self.training, split, kw, random.random(), float(np.random.rand()), float(torch.rand(1)))
        if torch.cuda.is_available():
            torch.rand(3, device="cuda")
        raise RuntimeError("no pictures today")


def _states():
    out = [random.getstate(), np.random.get_state()[1].tobytes(), np.random.get_state()[2], torch.get_rng_state().clone()]
    if torch.cuda.is_available():
        out.append(torch.cuda.get_rng_state().clone())
    return out


def _same(a, b):
    return all(torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y for x, y in zip(a, b))


def test_logger_restores_generators_and_mode_when_log_images_raises(tmp_path):
    from mobi_amd import train
    random.seed(3), np.random.seed(4), torch.manual_seed(5)
    np.random.randn()                                                   # (a cached gaussian is part of numpy's state)
    lg = train.ImageLogger(str(tmp_path), batch_frequency=7, log_images_kwargs={"ddim_steps": 2})
    seen = []
    for training in (True, False):
        model = _RaisingModel().train(training)
        before = _states()
        with pytest.raises(RuntimeError, match="no pictures today"):
            lg.on_train_batch_end(_Trainer(), model, {"x": torch.zeros(2)}, 3)
        assert _same(_states(), before)
        assert model.training is training
        assert model.seen[:3] == (False, "train", {"ddim_steps": 2})    # called in eval mode, with the kwargs
        seen.append(model.seen[3:])
    assert seen[0] == seen[1]                                           # the call's own stream: (seed, step, split, batch index)
    model = _RaisingModel()
    with pytest.raises(RuntimeError):
        lg.on_validation_batch_end(_Trainer(), model, {}, 3)
    assert model.seen[1] == "val" and model.seen[3:] != seen[0]
    other = train.ImageLogger(str(tmp_path), batch_frequency=7, seed=1)
    with pytest.raises(RuntimeError):
        other.on_train_batch_end(_Trainer(), model, {}, 3)
    assert model.seen[3:] != seen[0]
    # disabled, and step 0 without log_first_step: the model is not called
    model.seen = None
    assert train.ImageLogger(str(tmp_path), batch_frequency=7, disabled=True).on_train_batch_end(_Trainer(), model, {}, 3) is None
    first = _Trainer()
    first.global_step = 0
    assert lg.on_train_batch_end(first, model, {}, 0) is None and lg.on_validation_batch_end(first, model, {}, 0) is None
    assert model.seen is None
    assert train.ImageLogger(str(tmp_path), batch_frequency=5).on_train_batch_end(_Trainer(), _RaisingModel(), {}, 3) is None


def test_logger_row_and_files_from_a_stub(tmp_path, monkeypatch):
    """`log_img` end to end without a device: the stub's log dict has no tensor entry the launch would take, the pictures come from
    a patched `pictures`; file names follow `log_local`, a `/` in a key is a directory, the row carries the metrics as floats."""
    from PIL import Image
    from mobi_amd import train

    class Model(torch.nn.Module):
        last_lidar_metrics = None

        def log_images(self, batch, split="train", **kw):
            self.last_lidar_metrics = {f"{split}/mse/object_pred_depth": np.float64(1.5), f"{split}/median_error/mask_rec_int": np.float32(0.25)}
            return {"not_a_picture": 3}

    pics = {"range_depth_pred": np.arange(4 * 5 * 3, dtype=np.uint8).reshape(4, 5, 3), "a/b": np.full((2, 2, 3), 9, np.uint8)}
    lg = train.ImageLogger(str(tmp_path), batch_frequency=7)
    assert lg.pictures({"not_a_picture": 3, "flat": torch.zeros(3)}) == {}
    monkeypatch.setattr(lg, "pictures", lambda images: pics)
    row = lg.on_validation_batch_end(_Trainer(), Model(), {}, 2)
    assert row == {"step": 7, "epoch": 1, "batch_idx": 2, "split": "val", "val/mse/object_pred_depth": 1.5,
                   "val/median_error/mask_rec_int": 0.25}
    assert all(type(v) in (int, float, str) for v in row.values())
    root = tmp_path / "images" / "val"
    got = np.asarray(Image.open(root / "range_depth_pred_gs-000007_e-000001_b-000002.png"))
    assert np.array_equal(got, pics["range_depth_pred"])
    assert np.array_equal(np.asarray(Image.open(root / "a" / "b_gs-000007_e-000001_b-000002.png")), pics["a/b"])


class _StubOptimizer:
    def step_scaled(self, grads, scaler=None, max_norm=None):
        pass


class _StubLd(torch.nn.Module):
    learning_rate, monitor, adapter_grads, adapter_grads_scale = 1e-3, None, {}, 1.0
    last_lidar_metrics = None

    def __init__(self):
        super().__init__()
        self.steps = 0

    def configure_optimizers(self):
        return _StubOptimizer()

    def training_step(self, batch, i, scaler=None, allreduce=True):
        self.steps += 1
        self.loss_dict = {"train/loss": torch.tensor(float(self.steps))}

    def on_train_batch_end(self):
        pass

    def validation_step(self, batch, i):
        return {"val/loss": torch.tensor(0.5)}

    def log_images(self, batch, split="train", **kw):
        self.last_lidar_metrics = {f"{split}/mse/object_pred_depth": 2.0}
        return {}


def test_trainer_appends_metrics_jsonl_and_a_second_trainer_continues_it(tmp_path, monkeypatch):
    from mobi_amd import checkpoint, train

    class NoCheckpointer:
        def __init__(self, *a, **k):
            pass

        def wait(self):
            pass
    monkeypatch.setattr(checkpoint, "Checkpointer", NoCheckpointer)
    batches = lambda epoch, start=0: [{"i": j} for j in range(4)][start:]
    log_dir = str(tmp_path / "logs")

    def run(epochs):
        lg = train.ImageLogger(str(tmp_path), batch_frequency=2)
        return train.Trainer(_StubLd(), max_epochs=epochs, log_every=2, image_logger=lg, log_dir=log_dir).fit(batches, lambda: [{"v": 0}])
    tr = run(1)
    rows = [json.loads(line) for line in open(os.path.join(log_dir, "metrics.jsonl"))]
    assert [r["kind"] for r in rows] == ["images", "train", "images", "train", "images", "val"]       # (the hook runs before the log row is flushed)
    assert [r["step"] for r in rows if r["kind"] == "train"] == [2, 4] and rows[1]["train/loss"] == 1.5
    images = [r for r in rows if r["kind"] == "images"]
    assert [(r["step"], r["split"], r["batch_idx"]) for r in images] == [(2, "train", 1), (4, "train", 3), (4, "val", 0)]
    assert images[0]["train/mse/object_pred_depth"] == 2.0 and images[2]["val/mse/object_pred_depth"] == 2.0
    assert rows[-1] == {"kind": "val", "epoch": 0, "val/loss": 0.5}
    strip = lambda r: {k: v for k, v in r.items() if k != "kind"}
    assert [strip(r) for r in images] == tr.image_history and [strip(r) for r in rows if r["kind"] == "train"] == tr.history
    assert tr.current_epoch == 0
    run(1)                                                               # a second trainer: the file goes on
    again = [json.loads(line) for line in open(os.path.join(log_dir, "metrics.jsonl"))]
    assert again[:len(rows)] == rows and len(again) == 2 * len(rows)
    # without the two arguments: no file, no rows, and the hooks are not called
    plain = train.Trainer(_StubLd(), max_epochs=1, log_every=2).fit(batches, lambda: [{"v": 0}])
    assert plain.image_history == [] and plain.log_dir is None and len(plain.history) == 2


def test_image_grid_refusals_are_host_checks():
    """`mobi_image_grid` validates before its launch (no GPU here: every call must return): a 16-bit source and a 17-entry table are
    unsupported; null pointers, an offset past the buffer and a misaligned offset are refused."""
    from mobi_amd import _lib, build, ops
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.mobi_struct_size(30) == C.sizeof(_lib.ImageGridSource) == 40 and _lib.STRUCT_IDS[30] is _lib.ImageGridSource

    def table(count, **kw):
        t = (_lib.ImageGridSource * count)()
        for s in t:
            s.data, s.elem_bytes, s.n, s.c, s.h, s.w, s.out_offset = 4096, 4, 5, 1, 6, 9, 0
            for k, v in kw.items():
                setattr(s, k, v)
        return t
    hg, wg = ops.image_grid_shape(5, 6, 9, 8)
    assert (hg, wg) == (2 * 8 + 2, 4 * 11 + 2) and ops.image_grid_shape(1, 5, 7, 8) == (5, 7)
    assert ops.image_grid_shape(8, 16, 12, 6) == (2 * 18 + 2, 4 * 14 + 2) and ops.image_grid_shape(4, 8, 8, 8) == (1 * 10 + 2, 4 * 10 + 2)
    need = hg * wg * 3
    call = lambda t, n, out=8192, size=need, max_images=8, nrow=4, padding=2: lib.mobi_image_grid(t, n, max_images, nrow, padding, 1, 1, out, size, None)
    assert call(table(1, elem_bytes=2), 1) == -2                          # a 16-bit source
    assert call(table(17), 17) == -2                                      # 17 entries
    assert call(table(1, c=2), 1) == -2                                   # C = 1 | 3
    assert call(table(1, elem_bytes=8), 1) == -1
    assert call(None, 1) == -1 and call(table(1), 0) == -1 and call(table(1), 1, out=None) == -1
    assert call(table(1, data=None), 1) == -1 and call(table(1, h=0), 1) == -1
    assert call(table(1), 1, max_images=0) == -1 and call(table(1), 1, nrow=0) == -1 and call(table(1), 1, padding=-1) == -1
    assert call(table(1), 1, size=need - 1) == -1                         # the picture does not fit
    assert call(table(1, out_offset=4), 1, size=need + 3) == -1
    assert call(table(1, out_offset=2), 1, size=need + 8) == -4           # 4-byte offsets
    assert call(table(1, data=4098), 1) == -4
