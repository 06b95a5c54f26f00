"""CPU: the host side of checkpoints and resuming -- `train.AdamW` / `LambdaLR` / `GradAccumulator` state dicts, the digest's host
definition, the `verify` tool, the atomic writer and the epoch sampler.  All comparisons are bit-equality."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3,), (4, 5), (1,), (2, 3, 4), (7,), (16, 2), (5,), (1, 1, 9), (8,), (2, 2), (11,), (6, 3)]
WITH_STATE = (0, 1, 3, 4, 7, 10, 11)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _engine_adamw(steps=7, seed=0):
    from mobi_amd import train
    g = torch.Generator().manual_seed(seed)
    params = {f"p{i:02d}": torch.randn(s, generator=g) for i, s in enumerate(SHAPES)}
    opt = train.AdamW(params, lr=2.5e-4, betas=(0.8, 0.95), eps=1e-7, weight_decay=0.03)
    for i in WITH_STATE:
        n = f"p{i:02d}"
        opt.state[n] = (torch.randn(SHAPES[i], generator=g), torch.rand(SHAPES[i], generator=g))
    opt.steps = steps
    return opt


def test_adamw_state_interchanges_with_torch():
    """A torch.optim.AdamW over the same shapes accepts `state_dict()`; what it hands back loads with bit-equal moments and the
    same step count; a tensor without state stays without."""
    opt = _engine_adamw()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(WITH_STATE) and sd["param_groups"][0]["params"] == list(range(len(SHAPES)))
    for e in sd["state"].values():
        assert e["step"].dtype == torch.float32 and e["step"].dim() == 0 and float(e["step"]) == 7.0
    tparams = [torch.nn.Parameter(torch.zeros(s)) for s in SHAPES]
    topt = torch.optim.AdamW(tparams, lr=1.0)
    topt.load_state_dict(sd)
    g = topt.param_groups[0]
    assert g["lr"] == 2.5e-4 and tuple(g["betas"]) == (0.8, 0.95) and g["eps"] == 1e-7 and g["weight_decay"] == 0.03
    assert g["amsgrad"] is False
    assert sorted(i for i, p in enumerate(tparams) if p in topt.state) == list(WITH_STATE)
    back = topt.state_dict()
    fresh = _engine_adamw(steps=0, seed=1)
    del fresh.state["p04"]                             # created by the load
    fresh.state["p02"] = (torch.ones(SHAPES[2]), torch.ones(SHAPES[2]))     # not in the file: removed by the load
    kept = fresh.state["p00"]
    fresh._multi["sentinel"] = object()
    fresh.load_state_dict(back)
    assert fresh.steps == 7 and fresh.lr == 2.5e-4 and fresh.betas == (0.8, 0.95) and fresh.eps == 1e-7
    assert fresh.weight_decay == 0.03
    assert sorted(fresh.state) == [f"p{i:02d}" for i in WITH_STATE]
    assert fresh.state["p00"][0] is kept[0] and fresh.state["p00"][1] is kept[1]          # copied INTO the existing tensors
    assert len(fresh._multi) == 0                      # a moment tensor was created: the tables are dropped
    for n in fresh.state:
        for a, b in zip(fresh.state[n], opt.state[n]):
            assert torch.equal(_bits(a), _bits(b)), n


def test_adamw_load_keeps_the_tables_when_nothing_is_created():
    opt = _engine_adamw()
    sd = opt.state_dict()
    sd = {"state": {i: {k: v.clone() for k, v in e.items()} for i, e in sd["state"].items()}, "param_groups": sd["param_groups"]}
    other = _engine_adamw(steps=2, seed=3)
    other._multi["sentinel"] = object()
    other.load_state_dict(sd)
    assert "sentinel" in other._multi and other.steps == 7
    for n in opt.state:
        assert torch.equal(_bits(other.state[n][0]), _bits(opt.state[n][0]))


def test_adamw_mixed_step_counts_raise():
    opt = _engine_adamw()
    sd = opt.state_dict()
    sd["state"][3]["step"] = torch.tensor(6.0)
    with pytest.raises(ValueError, match="ONE step count"):
        _engine_adamw().load_state_dict(sd)
    sd = opt.state_dict()
    sd["param_groups"][0]["params"] = list(range(len(SHAPES) - 1))
    with pytest.raises(ValueError):
        _engine_adamw().load_state_dict(sd)


def test_lambda_lr_round_trip():
    from mobi_amd import train
    lam = lambda s: min(1.0, (s + 1) / 4.0) * 0.97 ** s
    a_opt, b_opt = _engine_adamw(), _engine_adamw()
    a = train.LambdaLR(a_opt, lam)
    for _ in range(3):
        a.step()
    sd = a.state_dict()
    assert sd == {"last_epoch": 3, "base_lrs": [2.5e-4]}
    b_opt.lr = 123.0                                   # (an optimizer built with another rate)
    b = train.LambdaLR(b_opt, lam)
    b.load_state_dict(sd)
    assert b_opt.lr == a_opt.lr
    for _ in range(5):
        a.step()
        b.step()
        assert b_opt.lr == a_opt.lr and b.last_epoch == a.last_epoch and b.get_last_lr() == a.get_last_lr()


def test_grad_accumulator_state_dict():
    from mobi_amd import train
    acc = train.GradAccumulator(_engine_adamw(), 2)
    assert acc.state_dict() == {}
    acc._adds = 1                                      # inside a window (`add` itself launches on the device: tests/test_gpu_checkpoint.py)
    with pytest.raises(RuntimeError, match="between optimizer steps"):
        acc.state_dict()
    acc._clear()
    acc.load_state_dict({})
    with pytest.raises(ValueError):
        acc.load_state_dict({"x": 1})


# ----------------------------------------------------------------------------------------------------------------------
def _from_bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32))


def test_digest_host_written_out_cases():
    from mobi_amd.checkpoint import digest_host
    K = 0x9E3779B9
    assert digest_host(torch.zeros(0)) == 0
    assert digest_host(_from_bits([0x3F800000])) == (0x3F800000 ^ K) * 1
    assert digest_host(torch.tensor([0.0, -0.0])) == ((0 ^ K) * 1 + (0x80000000 ^ K) * 3) % 2 ** 64
    assert digest_host(torch.tensor([-0.0, 0.0])) != digest_host(torch.tensor([0.0, -0.0]))
    assert digest_host(torch.tensor([0.0, 0.0])) != digest_host(torch.tensor([0.0, -0.0]))
    rng = np.random.RandomState(5)
    words = rng.randint(0, 2 ** 32, size=100, dtype=np.uint64).astype(np.uint32)
    t = _from_bits(words)
    want = 0
    for i, u in enumerate(words.tolist()):
        want = (want + (u ^ K) * ((2 * i + 1) % 2 ** 32)) % 2 ** 64
    assert digest_host(t) == want
    assert digest_host(t.numpy()) == want and digest_host(t.view(10, 10)) == want
    perm = torch.from_numpy(rng.permutation(100))
    assert digest_host(t[perm]) != want
    assert digest_host(_from_bits([0x7FC00000, 5])) != digest_host(_from_bits([0x7FC00001, 5]))       # two NaN payloads
    assert digest_host(_from_bits([0x7FC00000])) != digest_host(_from_bits([0xFFC00000]))             # and the NaN's sign


def _hand_built_file(path):
    from mobi_amd.checkpoint import FORMAT, digest_host
    g = torch.Generator().manual_seed(2)
    sd = {"model.w": torch.randn(5, 7, generator=g), "model.b": torch.randn(7, generator=g), "count": torch.tensor(3, dtype=torch.int32)}
    opt = {"state": {0: {"step": torch.tensor(2.0), "exp_avg": torch.randn(5, 7, generator=g), "exp_avg_sq": torch.rand(5, 7, generator=g)}},
           "param_groups": [{"params": [0, 1]}]}
    digests = {k: [digest_host(v), v.numel()] for k, v in sd.items() if v.dtype == torch.float32}
    digests["optimizer.0.exp_avg"] = [digest_host(opt["state"][0]["exp_avg"]), 35]
    digests["optimizer.0.exp_avg_sq"] = [digest_host(opt["state"][0]["exp_avg_sq"]), 35]
    ckpt = {"state_dict": sd, "optimizer_states": [opt], "lr_schedulers": [], "global_step": 2, "epoch": 0,
            "mobi_amd": {"format": FORMAT, "digests": digests}}
    torch.save(ckpt, path)
    return ckpt


def test_verify_tool(tmp_path):
    from mobi_amd import checkpoint
    path = str(tmp_path / "a.ckpt")
    ckpt = _hand_built_file(path)
    assert checkpoint.verify_file(path) == (4, [])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "mobi_amd.checkpoint", "verify", path], capture_output=True, text=True, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stdout + run.stderr
    _bits(ckpt["optimizer_states"][0]["state"][0]["exp_avg_sq"])[2, 3] ^= 1          # one mantissa bit
    torch.save(ckpt, path)
    count, bad = checkpoint.verify_file(path)
    assert count == 4 and [name for name, _ in bad] == ["optimizer.0.exp_avg_sq"]
    assert checkpoint.main(["verify", path]) == 1
    _bits(ckpt["optimizer_states"][0]["state"][0]["exp_avg_sq"])[2, 3] ^= 1
    _bits(ckpt["state_dict"]["model.b"])[6] ^= 1 << 22
    torch.save(ckpt, path)
    assert [name for name, _ in checkpoint.verify_file(path)[1]] == ["model.b"]


def test_writer_is_atomic(tmp_path, monkeypatch):
    """`torch.save` fails after it has created the tmp file: the target keeps its bytes, no tmp file remains, `wait()` raises."""
    from mobi_amd import checkpoint
    path = str(tmp_path / "last.ckpt")
    w = checkpoint.AtomicWriter()
    w.submit(lambda: {"x": torch.arange(4)}, path)
    w.wait()
    before = open(path, "rb").read()
    assert torch.equal(torch.load(path)["x"], torch.arange(4)) and not os.path.exists(path + ".tmp")
    seen = []

    def failing_save(obj, f, *a, **k):
        open(f, "wb").write(b"half a file")
        seen.append(os.path.exists(path + ".tmp"))
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", failing_save)
    w.submit(lambda: {"x": torch.arange(5)}, path)
    with pytest.raises(OSError, match="disk full"):
        w.wait()
    assert seen == [True]
    assert open(path, "rb").read() == before and not os.path.exists(path + ".tmp")
    w.wait()                                           # the error is raised once
    ck = checkpoint.Checkpointer(model=None, optimizer=None)                  # the Checkpointer's wait() is the writer's
    ck._writer.submit(lambda: {"x": 1}, path)
    with pytest.raises(OSError):
        ck.wait()
    assert open(path, "rb").read() == before and sorted(os.listdir(tmp_path)) == ["last.ckpt"]


def test_epoch_sampler():
    from mobi_amd import train
    n, bs = 23, 4
    a = list(train.EpochSampler(n, bs, seed=7, epoch=2))
    assert a == list(train.EpochSampler(n, bs, seed=7, epoch=2))
    assert len(a) == 5 and all(len(b) == bs for b in a) and len({i for b in a for i in b}) == 20
    assert sorted(train.epoch_order(n, 7, 2)) == list(range(n))
    assert a != list(train.EpochSampler(n, bs, seed=7, epoch=3)) and a != list(train.EpochSampler(n, bs, seed=8, epoch=3))
    assert list(train.EpochSampler(n, bs, seed=7, epoch=3)) == list(train.EpochSampler(n, bs, seed=8, epoch=2))   # seed + epoch
    for k in range(6):
        assert list(train.EpochSampler(n, bs, seed=7, epoch=2, start_batch=k)) == a[k:]
    ragged = list(train.EpochSampler(n, bs, seed=7, epoch=2, drop_last=False))
    assert ragged[:5] == a and len(ragged) == 6 and len(ragged[5]) == 3
    # through a DataLoader over a list: the items in front of start_batch are never built
    built = []

    class Items(torch.utils.data.Dataset):
        def __len__(self):
            return n

        def __getitem__(self, i):
            built.append(i)
            return i
    dl = torch.utils.data.DataLoader(Items(), batch_sampler=train.EpochSampler(n, bs, 7, 2, start_batch=3), collate_fn=list)
    assert [list(b) for b in dl] == a[3:] and built == [i for b in a[3:] for i in b]


@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    from tests import mini_db
    return mini_db.build(str(tmp_path_factory.mktemp("mini_db_ckpt")))


def _listing_dataset(mini):
    """The train split of the miniature database (augmentation draws on) whose `collate_device` only gathers what identifies a
    batch -- the items' names and augmentation draws -- so that `device_loader` iterates without a device."""
    from mobi_amd.ldm.data.nuscenes import NuScenesDataset

    class Listing(NuScenesDataset):
        def collate_device(self, items, device="cuda"):
            return [(it["id_name"], [it["ref_aug"][k].clone() for k in ("flags", "warp", "table")]) for it in items]
    np.random.seed(0)
    return Listing(state="train", use_lidar=True, use_camera=True, object_database_path=mini[0], scene_database_path=mini[1],
                   expand_mask_ratio=0.1, expand_ref_ratio=0, object_area_crop=0.2, num_samples_per_class=2, fixed_sampling=True,
                   object_random_crop=False, ref_aug=True, ref_mode="id-ref", image_height=128, image_width=128, range_height=128,
                   range_width=128, object_classes=["car", "pedestrian"], range_object_norm=True, range_object_norm_scale=0.75,
                   range_int_norm=True, min_lidar_points=8)


def _same_batch(x, y):
    return [n for n, _ in x] == [n for n, _ in y] and all(torch.equal(a, b) for (_, da), (_, db) in zip(x, y) for a, b in zip(da, db))


def test_epoch_loader_resumes_inside_an_epoch_with_the_generators_as_saved(mini):
    """`epoch_loader` -> `device_loader(sampler=)`: making the loader's iterator draws nothing from torch's global generator (a
    DataLoader without a generator of its own draws its base seed there, also without workers), so a run that restores the
    generators a checkpoint recorded after batch k and begins a new loader at k + 1 sees the batches, the augmentation draws and
    the next global draw (the posterior's noise in `get_input`) of the uninterrupted run."""
    import random
    from mobi_amd import train
    ds = _listing_dataset(mini)
    assert len(ds) == 4
    batches = train.epoch_loader(ds, batch_size=1, seed=7, num_workers=0, device="cpu")
    loader = batches(1, 0)
    assert len(loader) == 4
    torch.manual_seed(11)
    state = torch.get_rng_state()
    iter(loader.inner)
    assert torch.equal(torch.get_rng_state(), state)
    # the uninterrupted run: two batches, the generators as a checkpoint records them, the rest of the epoch, one global draw
    random.seed(5)
    np.random.seed(5)
    torch.manual_seed(5)
    it = iter(batches(1, 0))
    head = [next(it), next(it)]
    saved = (random.getstate(), np.random.get_state(), torch.get_rng_state())
    tail, noise = list(it), torch.randn(3)
    assert len(tail) == 2
    names = [ds.get_id_name(ds.objects_meta.loc[i]) for i in train.epoch_order(4, 7, 1)]
    assert [b[0][0] for b in head + tail] == names
    # the resumed run: other generators first, then the recorded ones; a new loader that begins at batch 2
    random.seed(99)
    np.random.seed(99)
    torch.manual_seed(99)
    list(batches(0, 0))
    random.setstate(saved[0])
    np.random.set_state(saved[1])
    torch.set_rng_state(saved[2])
    resumed = list(batches(1, 2))
    assert len(resumed) == 2 and all(_same_batch(x, y) for x, y in zip(resumed, tail))
    assert torch.equal(torch.randn(3), noise)
    assert not _same_batch(head[0], head[1])


def test_scaled_lr():
    from mobi_amd import train
    assert train.scaled_lr(1e-6, accumulate=2, nodes=1, gpus=8, batch_size=4) == 2 * 1 * 8 * 4 * 1e-6
