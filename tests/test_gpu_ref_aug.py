"""The training splits' data side on the device: `mobi_ref_augment` against the host restatement (`ldm.data.ref_aug`, itself
pinned stage by stage in tests/test_ref_aug_cpu.py) bit for bit, `mobi_drop_context` against torch's two operations,
`collate_device` over augmented / context-dropping raw items against the host items built from the same `random` state, and a
`state="train"` batch from `device_loader` through `get_input` and one `training_step`."""
import os
import random

import numpy as np
import pytest
import torch

from mobi_amd.ldm.data import ref_aug as RA
from mobi_amd.ldm.data.ref_aug import IDENTITY, RefAugDraw

pytestmark = pytest.mark.gpu

ALL = RefAugDraw(True, True, -30.0, True, 7, True, 0.7, -0.3)
# each stage alone, all together, all off; angles 0 / 30 / -30 / 17.3 / 90; box sides 3 / 5 / 7; both look-up extremes
DRAWS = [IDENTITY._replace(flip=True), IDENTITY._replace(rotate=True, angle=30.0), IDENTITY._replace(blur=True, k=3),
         IDENTITY._replace(bc=True, alpha=1.3, beta=0.3), ALL, IDENTITY,
         IDENTITY._replace(rotate=True, angle=17.3, blur=True, k=5), IDENTITY._replace(rotate=True, angle=90.0),
         RefAugDraw(True, True, 0.0, True, 3, True, 1.3, 0.3)]


@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    from tests import mini_db
    return mini_db.build(str(tmp_path_factory.mktemp("mini_db_aug_gpu")))


def _dataset(mini, **kw):
    from mobi_amd.ldm.data.nuscenes import NuScenesDataset
    params = dict(state="train", use_lidar=True, use_camera=True, object_database_path=mini[0], scene_database_path=mini[1],
                  expand_mask_ratio=0.1, expand_ref_ratio=0, object_area_crop=0.2, num_samples_per_class=2, fixed_sampling=True,
                  object_random_crop=False, ref_aug=True, ref_mode="id-ref", image_height=128, image_width=128,
                  range_height=128, range_width=128, object_classes=["car", "pedestrian"], range_object_norm=True,
                  range_object_norm_scale=0.75, range_int_norm=True, min_lidar_points=8)
    params.update(kw)
    np.random.seed(0)                                    # (the constructor samples the objects per class)
    return NuScenesDataset(**params)


def _patches(kind, b, s):
    if kind == "random":
        return np.random.default_rng(17).integers(0, 256, (b, s, s, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:s, 0:s]
    ramp = np.stack([(xx * 255) // (s - 1), (yy * 255) // (s - 1), ((xx + 2 * yy) * 3) % 256], -1).astype(np.uint8)
    return np.stack([np.roll(ramp, 5 * i, axis=1) for i in range(b)])


@pytest.mark.parametrize("kind", ["random", "ramp"])
@pytest.mark.parametrize("size,draws", [(224, DRAWS), (224, [ALL]), (45, [ALL, DRAWS[6]._replace(flip=True)])],
                         ids=["S224-B9", "S224-B1", "S45-B2"])
def test_ref_augment_equals_the_host_restatement(size, draws, kind):
    """One launch per case, a different draw per sample.  S = 45: partial tiles in both directions, and the reflected halo of
    the 7 x 7 box crosses the tile edge at 32."""
    from mobi_amd import ops
    from mobi_amd.ldm.data.nuscenes import get_tensor_clip
    patches = _patches(kind, len(draws), size)
    forms = [RA.device_form(d, size) for d in draws]
    got = ops.ref_augment(torch.from_numpy(patches).cuda(), torch.stack([f["flags"] for f in forms]),
                          torch.stack([f["warp"] for f in forms]), torch.stack([f["table"] for f in forms]))
    assert got.shape == (len(draws), 3, size, size) and got.dtype == torch.float32
    got = got.cpu()
    for b, d in enumerate(draws):
        want = get_tensor_clip()(RA.ref_augment_u8(patches[b], d))
        assert torch.equal(got[b], want), (b, d, int((got[b] != want).sum()))


def test_ref_augment_checks_its_arguments():
    from mobi_amd import _lib, ops
    f = RA.device_form(IDENTITY, 16)
    one = lambda k: f[k][None]
    p = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device="cuda")
    assert ops.ref_augment(p, one("flags"), one("warp"), one("table")).shape == (1, 3, 16, 16)
    with pytest.raises(ValueError):
        ops.ref_augment(p, torch.tensor([[0, 4]]), one("warp"), one("table"))     # an even box side
    with pytest.raises(ValueError):
        ops.ref_augment(p, torch.tensor([[4, 0]]), one("warp"), one("table"))     # an unknown stage bit
    with pytest.raises(AssertionError):
        ops.ref_augment(p, one("flags"), one("warp")[:, :, :8], one("table"))
    small = RA.device_form(IDENTITY, 4)
    with pytest.raises(_lib.EngineError):                                          # S >= 8: the reflected halo
        ops.ref_augment(p[:, :4, :4].contiguous(), small["flags"][None], small["warp"][None], small["table"][None])
    with pytest.raises(_lib.EngineUnavailable):
        ops.ref_augment(p.cpu(), one("flags"), one("warp"), one("table"))


@pytest.mark.parametrize("shape", [(3, 2, 5, 7), (3, 3, 8, 12)], ids=["scalar", "float4"])
def test_drop_context_is_torchs_two_operations(shape):
    from mobi_amd import ops
    g = torch.Generator().manual_seed(3)
    b, c, h, w = shape
    gt, inp = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    mask = torch.rand((b, 1, h, w), generator=g)
    mask[:, :, ::2] = (mask[:, :, ::2] > 0.5).float()
    flags = [True, False, True]
    d_gt, d_inp = gt.cuda(), inp.cuda()
    ops.drop_context(d_gt, d_inp, mask.cuda(), flags)
    for i, f in enumerate(flags):
        assert torch.equal(d_gt[i].cpu(), gt[i] * (1 - mask[i]) if f else gt[i]), i
        assert torch.equal(d_inp[i].cpu(), torch.zeros_like(inp[i]) if f else inp[i]), i


def _host_and_device(ds, seed):
    from torch.utils.data import default_collate
    random.seed(seed)
    host = default_collate([ds[i] for i in range(len(ds))])
    random.seed(seed)
    raw = [ds.raw_item(i) for i in range(len(ds))]
    return host, raw, ds.collate_device(raw)


def _assert_batches_agree(host, dev):
    """The bounds of tests/test_gpu_data_side.py::test_collate_device_equals_host_items (range_int_norm=True)."""
    hl, dl = host["lidar"], dev["lidar"]
    assert torch.equal(dl["range_mask"].cpu(), hl["range_mask"])
    assert torch.equal(dl["range_data"][:, :1].cpu(), hl["range_data"][:, :1])
    assert float((dl["range_data"][:, 1:].cpu() - hl["range_data"][:, 1:]).abs().max()) <= 2e-7
    assert float((dl["range_data_inpaint"].cpu() - hl["range_data_inpaint"]).abs().max()) <= 2e-7
    assert torch.equal(dl["range_instance_mask"].cpu(), hl["range_instance_mask"])
    for k in ("GT", "inpaint_image", "inpaint_mask"):
        assert float((dev["image"][k].cpu() - host["image"][k]).abs().max()) <= 1e-6, k
    assert torch.equal(dev["image"]["cond"]["ref_bbox"].cpu(), host["image"]["cond"]["ref_bbox"])
    assert torch.equal(dl["cond"]["ref_bbox"].cpu(), hl["cond"]["ref_bbox"]) and dev["id_name"] == host["id_name"]
    assert torch.equal(dev["image"]["cond"]["ref_image"].cpu(), host["image"]["cond"]["ref_image"])
    assert torch.equal(dl["cond"]["ref_image"].cpu(), hl["cond"]["ref_image"])
    assert set(dev) == set(host) and set(dev["image"]) == set(host["image"]) and set(dl) == set(hl)
    assert set(dev["image"]["cond"]) == set(host["image"]["cond"]) and set(dl["cond"]) == set(hl["cond"])
    assert dl["range_data"].is_cuda and dev["image"]["cond"]["ref_image"].is_cuda


def test_collate_device_equals_host_items_with_ref_aug(mini):
    ds = _dataset(mini)
    host, raw, dev = _host_and_device(ds, seed=3)
    stages = torch.stack([r["ref_aug"]["flags"] for r in raw])
    assert len({tuple(f) for f in stages.tolist()}) >= 2                           # the samples drew different chains
    _assert_batches_agree(host, dev)
    plain = _dataset(mini, ref_aug=False)
    assert not torch.equal(dev["image"]["cond"]["ref_image"].cpu(), torch.stack([plain[i]["image"]["cond"]["ref_image"] for i in range(4)]))


@pytest.mark.parametrize("prob,seed", [(1.0, 0), (0.5, 2)])
def test_collate_device_drops_context(mini, prob, seed):
    ds = _dataset(mini, prob_drop_context=prob)
    host, raw, dev = _host_and_device(ds, seed=seed)
    cam = [r["image"]["drop_context"] for r in raw]
    lid = [r["lidar"]["drop_context"] for r in raw]
    if prob == 1.0:
        assert all(cam) and all(lid)
    else:                                                                          # a mixed batch, the modalities apart
        assert any(cam) and not all(cam) and any(lid) and not all(lid) and cam != lid
    _assert_batches_agree(host, dev)
    for b in range(len(raw)):
        assert bool((dev["image"]["inpaint_image"][b] == 0).all()) == cam[b]
        assert bool((dev["lidar"]["range_data_inpaint"][b] == 0).all()) == lid[b]
    assert "drop_context" not in dev["image"] and "drop_context" not in dev["lidar"]


def test_train_split_batch_trains_one_step(mini):
    """`device_loader` over a `state="train"` dataset (augmentation and context drops on) -> `get_input` -> one
    `training_step` on the reduced network of tests/test_gpu_data_side.py::test_dataset_batch_feeds_get_input."""
    import copy
    import mobi_amd
    from mobi_amd.ldm.util import instantiate_from_config, load_config
    from oracle import weights as W
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
    W.fill_module_(model, seed=31)
    model = model.cuda().train()
    random.seed(5)
    ds = _dataset(mini, prob_drop_context=0.5)
    loader = ds.device_loader(batch_size=2)
    assert len(loader) == 2
    batch = next(iter(loader))
    assert batch["image"]["cond"]["ref_image"].shape == (2, 3, 224, 224) and batch["image"]["GT"].is_cuda
    data = model.get_input(copy.deepcopy(batch), model.first_stage_key)           # (get_input edits the lidar box token in place)
    assert data["z"].shape == (4, 9, 16, 16) and torch.isfinite(data["z"]).all()
    assert data["cond"]["ref_image"].shape == (4, 3, 224, 224) and data["cond"]["ref_bbox"].shape == (4, 8, 3)
    loss = model.training_step(batch, 0)
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    grads = model.adapter_grads
    opt = model.configure_optimizers()
    opt = opt[0][0] if isinstance(opt, tuple) else opt
    unet = [k for k in opt.params if k.startswith("model.diffusion_model.")]
    assert len(unet) == 432 and all(k in grads for k in unet)
    # the conditioning stage: the box embedder on a conditional draw, the learnt unconditional token otherwise
    cond = [k for k in opt.params if not k.startswith("model.diffusion_model.")]
    uncond = model.u_cond_prop < model.u_cond_percent
    assert cond and all(k in grads for k in cond if (k == "bbox_uncond_vector") == uncond)
    assert all(bool(torch.isfinite(v).all()) and v.dtype == torch.float32 for v in grads.values())
    assert sum(int(float(grads[k].abs().max()) > 0) for k in unet) >= 400
