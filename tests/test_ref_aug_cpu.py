"""CPU: the train / val splits' reference-image augmentation (`ldm.data.ref_aug`, `NuScenesDataset(ref_aug=True)`): every
stage against written-out numpy, the rotation's geometry against scipy in fp64, the draws, the draw-for-draw agreement of
`raw_item` with `__getitem__`, and `device_loader`'s worker processes staying off the GPU."""
import random

import numpy as np
import pytest
import torch

from mobi_amd.ldm.data import ref_aug as RA
from mobi_amd.ldm.data.ref_aug import IDENTITY, RefAugDraw


@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    from tests import mini_db
    return mini_db.build(str(tmp_path_factory.mktemp("mini_db_aug")))


def _dataset(mini, cls=None, **kw):
    from mobi_amd.ldm.data.nuscenes import NuScenesDataset
    params = dict(state="train", use_lidar=True, use_camera=True, object_database_path=mini[0], scene_database_path=mini[1],
                  expand_mask_ratio=0.1, expand_ref_ratio=0, object_area_crop=0.2, num_samples_per_class=2, fixed_sampling=True,
                  object_random_crop=False, ref_aug=True, ref_mode="id-ref", image_height=128, image_width=128,
                  range_height=128, range_width=128, object_classes=["car", "pedestrian"], range_object_norm=True,
                  range_object_norm_scale=0.75, range_int_norm=True, min_lidar_points=8)
    params.update(kw)
    np.random.seed(0)                                    # (the constructor samples the objects per class)
    return (cls or NuScenesDataset)(**params)


@pytest.fixture(scope="module")
def patch():
    return np.random.default_rng(11).integers(0, 256, (224, 224, 3)).astype(np.uint8)


def _only(**kw):
    return IDENTITY._replace(**kw)


def _shapes(x):
    if isinstance(x, dict):
        return {k: _shapes(v) for k, v in x.items()}
    if isinstance(x, torch.Tensor):
        return (tuple(x.shape), x.dtype)
    return type(x).__name__


# ---- the dataset ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["train", "val"])
def test_constructor_accepts_the_training_splits(mini, state):
    np.random.seed(0)
    random.seed(0)
    ds = _dataset(mini, state=state)
    item = ds[0]
    assert item["id_name"].endswith("-aug")
    for k in ("image", "lidar"):
        ref = item[k]["cond"]["ref_image"]
        assert ref.shape == (3, 224, 224) and ref.dtype == torch.float32
    with pytest.raises(NotImplementedError, match="train / val"):
        _dataset(mini, state="test")
    assert _dataset(mini, state="test", ref_aug=False)[0]["id_name"].endswith("rot-0")


@pytest.mark.parametrize("name", ["mobi_nusc-mini_256", "mobi_nusc-mini_512", "mobi_nusc_256", "mobi_nusc_512",
                                  "mobi_nusc_all-classes_256", "mobi_nusc_all-classes_512"])
def test_shipped_configs_build_their_training_splits(mini, name):
    """`data.params.train` / `.validation` of every shipped config, pointed at the miniature database."""
    import os
    from mobi_amd.ldm.util import instantiate_from_config, load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, "configs", f"{name}.yaml"), ["use_lidar=True"])
    for split, state in (("train", "train"), ("validation", "val")):
        node = cfg["data"]["params"][split]
        params = dict(node["params"], object_database_path=mini[0], scene_database_path=mini[1], num_samples_per_class=1,
                      min_lidar_points=8)
        assert params["ref_aug"] is True and params["state"] == state
        np.random.seed(0)
        ds = instantiate_from_config({"target": node["target"], "params": params})
        assert ds.ref_aug and ds.state == state and len(ds) == len(ds.object_classes)
    item = ds[0]
    assert item["id_name"].endswith("-aug") and item["image"]["cond"]["ref_image"].shape == (3, 224, 224)


def test_augmented_batches_have_the_schema_of_plain_ones(mini):
    np.random.seed(0)
    random.seed(0)
    load = lambda ds: next(iter(torch.utils.data.DataLoader(ds, batch_size=4, num_workers=0, shuffle=False)))
    aug, plain = load(_dataset(mini, return_original_image=True)), load(_dataset(mini, ref_aug=False, return_original_image=True))
    assert _shapes(aug) == _shapes(plain)
    assert aug["image"]["cond"]["ref_image"].shape == (4, 3, 224, 224) and aug["lidar"]["range_data"].shape == (4, 2, 128, 128)
    assert torch.equal(aug["image"]["inpaint_image"], aug["image"]["GT"] * aug["image"]["inpaint_mask"])
    assert all(n.endswith("-aug") for n in aug["id_name"]) and not any(n.endswith("-aug") for n in plain["id_name"])
    assert not torch.equal(aug["image"]["cond"]["ref_image"], plain["image"]["cond"]["ref_image"])


def test_identity_draw_gives_the_plain_item(mini, monkeypatch):
    from mobi_amd.ldm.data import nuscenes
    monkeypatch.setattr(nuscenes, "draw_ref_aug", lambda: IDENTITY)
    aug, plain = _dataset(mini), _dataset(mini, ref_aug=False)
    for i in range(len(aug)):
        assert torch.equal(aug[i]["image"]["cond"]["ref_image"], plain[i]["image"]["cond"]["ref_image"])
        raw = aug.raw_item(i)
        assert "ref_image" not in raw["image"]["cond"] and "ref_image" not in raw["lidar"]["cond"]
        assert raw["ref_aug"]["patch"].dtype == torch.uint8 and raw["ref_aug"]["patch"].shape == (224, 224, 3)
        assert raw["ref_aug"]["flags"].tolist() == [0, 0] and raw["ref_aug"]["warp"].shape == (4, 224)
        table = raw["ref_aug"]["table"]
        assert table.shape == (3, 256) and table.dtype == torch.float32
        p = raw["ref_aug"]["patch"].long()
        looked_up = torch.stack([table[c][p[..., c]] for c in range(3)])
        assert torch.equal(looked_up, plain[i]["image"]["cond"]["ref_image"])      # the table IS get_tensor_clip
    assert set(plain.raw_item(0)) == {"id_name", "bbox_3d", "ref_class", "image", "lidar", "erase"}
    assert "drop_context" not in plain.raw_item(0)["image"] and "drop_context" not in plain.raw_item(0)["lidar"]


def test_erase_patch_goes_through_the_chain(mini, monkeypatch):
    from mobi_amd.ldm.data import nuscenes
    from mobi_amd.ldm.data.nuscenes import get_tensor_clip
    monkeypatch.setattr(nuscenes, "draw_ref_aug", lambda: _only(bc=True, alpha=1.0, beta=0.2))
    it = _dataset(mini, ref_mode="erase-ref")[0]
    want = get_tensor_clip()(np.full((224, 224, 3), 51, dtype=np.uint8))           # 0 + float32(0.2 * 255) -> 51
    assert it["ref_class"] == "empty" and torch.equal(it["image"]["cond"]["ref_image"], want)


# ---- the stages ----------------------------------------------------------------------------------------------------------
def test_identity_and_flip(patch):
    assert np.array_equal(RA.ref_augment_u8(patch, IDENTITY), patch)
    assert np.array_equal(RA.ref_augment_u8(patch, _only(flip=True)), patch[:, ::-1])


def test_rotation_by_0_and_90_degrees(patch):
    assert np.array_equal(RA.ref_augment_u8(patch, _only(rotate=True, angle=0.0)), patch)
    # centre (112, 112): output (x, y) reads source (224 - y, x) -- column 224 does not exist, so row 0 is border, and
    # rows 1 .. 223 are rows 0 .. 222 of the counter-clockwise quarter turn (np.rot90(S)[i, j] = S[j, 223 - i])
    want = np.zeros_like(patch)
    want[1:] = np.rot90(patch)[:-1]
    assert np.array_equal(RA.ref_augment_u8(patch, _only(rotate=True, angle=90.0)), want)
    flipped_first = RA.ref_augment_u8(patch, _only(flip=True, rotate=True, angle=90.0))
    want[1:] = np.rot90(patch[:, ::-1])[:-1]
    assert np.array_equal(flipped_first, want)                                      # the rotation reads the FLIPPED patch


@pytest.mark.parametrize("angle", [30.0, -30.0, 17.3])
def test_rotation_geometry_against_scipy(angle):
    """Direction and centre, independently: scipy.ndimage.affine_transform (order 1, fp64) with the rotation about
    (112, 112) written in (row, column) coordinates.  Bound: the image's gradient is at most 8 levels per pixel and axis, the
    source position sits on a 1/32-pixel grid (<= 1/64 off per axis): 8 * 2 / 64 levels, plus one of rounding -> <= 2."""
    from scipy.ndimage import affine_transform
    yy, xx = np.mgrid[0:224, 0:224].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(xx / 20) * np.cos(yy / 25), 3 * xx / 4 + yy / 3, 255 - xx / 2 - yy / 2], -1)
    img = np.rint(img).astype(np.uint8)
    assert np.abs(np.diff(img.astype(int), axis=0)).max() <= 8 and np.abs(np.diff(img.astype(int), axis=1)).max() <= 8
    t = np.radians(angle)
    c, s = np.cos(t), np.sin(t)
    m = np.array([[c, s], [-s, c]])                                                 # (sy, sx) - centre = m @ ((y, x) - centre)
    centre = np.array([112.0, 112.0])
    want = np.stack([affine_transform(img[..., k].astype(np.float64), m, offset=centre - m @ centre, order=1,
                                      mode="constant", cval=0.0) for k in range(3)], -1)
    src = np.einsum("ij,jhw->ihw", m, np.stack([yy - 112, xx - 112])) + 112
    inner = (src >= 1).all(0) & (src <= 222).all(0)
    assert inner.mean() >= 0.75, inner.mean()
    got = RA.ref_augment_u8(img, _only(rotate=True, angle=angle)).astype(np.float64)
    worst = np.abs(got - want)[inner].max()
    print(f"angle {angle}: {inner.mean():.3f} of the pixels compared, worst deviation {worst:.3f} levels")
    assert worst <= 2.0, worst


@pytest.mark.parametrize("k,level", [(3, 28), (5, 10), (7, 5)])
def test_blur(patch, k, level):
    impulse = np.zeros((224, 224, 3), dtype=np.uint8)
    impulse[100, 50] = 255
    out = RA.ref_augment_u8(impulse, _only(blur=True, k=k))
    want = np.zeros_like(impulse)
    want[100 - k // 2:101 + k // 2, 50 - k // 2:51 + k // 2] = level
    assert np.array_equal(out, want)
    const = np.full((224, 224, 3), 201, dtype=np.uint8)
    assert np.array_equal(RA.ref_augment_u8(const, _only(blur=True, k=k)), const)  # also along the border
    r = k // 2
    padded = np.pad(patch.astype(np.int64), ((r, r), (r, r), (0, 0)), mode="reflect")
    got = RA.ref_augment_u8(patch, _only(blur=True, k=k))
    for y, x in ((0, 0), (0, 223), (223, 0), (223, 223), (1, 100), (100, 222), (57, 131)):
        total = padded[y:y + k, x:x + k].sum((0, 1))
        assert list(got[y, x]) == list((2 * total + k * k) // (2 * k * k)), (y, x)
        assert np.all(np.abs(got[y, x] - total / (k * k)) <= 0.5)                  # round to nearest, no ties (k * k odd)


@pytest.mark.parametrize("alpha,beta", [(1.3, 0.3), (0.7, -0.3)])
def test_brightness_contrast_lut(patch, alpha, beta):
    lut = RA.brightness_contrast_lut(alpha, beta)
    for v in range(256):
        f = np.float32(np.float32(v) * np.float32(alpha)) + np.float32(beta * 255)
        assert lut[v] == min(255, max(0, int(np.trunc(f)))), v
    assert lut.dtype == np.uint8 and (np.diff(lut.astype(int)) >= 0).all()
    assert np.array_equal(RA.ref_augment_u8(patch, _only(bc=True, alpha=alpha, beta=beta)), lut[patch])
    assert np.array_equal(RA.brightness_contrast_lut(1.0, 0.0), np.arange(256))


def test_stages_compose_in_the_reference_order(patch):
    d = RefAugDraw(True, True, -21.5, True, 5, True, 1.2, -0.1)
    want = RA.brightness_contrast_lut(1.2, -0.1)[RA.blur_u8(RA.rotate_u8(patch[:, ::-1], -21.5), 5)]
    assert np.array_equal(RA.ref_augment_u8(patch, d), want)
    form = RA.device_form(d)
    assert form["flags"].tolist() == [3, 5] and form["flags"].dtype == torch.int32
    assert np.array_equal(form["warp"].numpy(), RA.warp_tables(-21.5)) and form["warp"].dtype == torch.int32
    assert RA.device_form(_only(blur=True, k=7))["flags"].tolist() == [0, 7]


# ---- the draws -----------------------------------------------------------------------------------------------------------
def test_draws():
    random.seed(123)
    a = [RA.draw_ref_aug() for _ in range(4000)]
    random.seed(123)
    assert a == [RA.draw_ref_aug() for _ in range(4000)]
    for stage in ("flip", "rotate", "blur", "bc"):
        rate = np.mean([getattr(d, stage) for d in a])
        assert abs(rate - 0.5) <= 0.032, (stage, rate)                             # four binomial sigmas at n = 4,000
    assert all(-30 <= d.angle <= 30 and d.k in (3, 5, 7) and 0.7 <= d.alpha <= 1.3 and -0.3 <= d.beta <= 0.3 for d in a)
    assert {d.k for d in a if d.blur} == {3, 5, 7} and any(d.angle < -25 for d in a) and any(d.angle > 25 for d in a)
    off = [d for d in a if not (d.rotate or d.blur or d.bc)]
    assert off and all((d.angle, d.k, d.alpha, d.beta) == (0.0, 3, 1.0, 0.0) for d in off)
    random.seed(7)                                                                 # the order of the draws, written out
    flip = random.random() < 0.5
    rot = random.random() < 0.5
    angle = random.uniform(-30, 30) if rot else 0.0
    blur = random.random() < 0.5
    k = random.choice([3, 5, 7]) if blur else 3
    bc = random.random() < 0.5
    alpha = 1 + random.uniform(-0.3, 0.3) if bc else 1.0
    beta = random.uniform(-0.3, 0.3) if bc else 0.0
    random.seed(7)
    assert RA.draw_ref_aug() == RefAugDraw(flip, rot, angle, blur, k, bc, alpha, beta)


@pytest.mark.parametrize("kw", [dict(), dict(prob_drop_context=0.5), dict(ref_aug=False, prob_drop_context=0.5),
                                dict(prob_drop_context=0.5, prob_erase_box=0.5, random_range_crop=True)])
def test_raw_item_consumes_the_draws_of_getitem(mini, kw):
    ds = _dataset(mini, **kw)
    seen = set()
    for i in range(len(ds)):
        for seed in (0, 1, 2):
            random.seed(100 * i + seed)
            host = ds[i]
            after_host = random.getstate()
            random.seed(100 * i + seed)
            raw = ds.raw_item(i)
            assert random.getstate() == after_host, (i, seed)
            if kw.get("prob_drop_context"):
                cam, lid = raw["image"]["drop_context"], raw["lidar"]["drop_context"]
                assert cam == bool((host["image"]["inpaint_image"] == 0).all()) and lid == bool((host["lidar"]["range_data_inpaint"] == 0).all())
                seen.add((cam, lid))
    if kw.get("prob_drop_context"):
        assert len(seen) >= 3                                                      # the two modalities draw independently


# ---- the loader ----------------------------------------------------------------------------------------------------------
def _reporting_dataset():
    from mobi_amd.ldm.data.nuscenes import NuScenesDataset

    class Reporting(NuScenesDataset):
        def raw_item(self, index):
            item = super().raw_item(index)
            info = torch.utils.data.get_worker_info()
            item["worker"] = (-1 if info is None else info.id, torch.cuda.is_initialized())
            return item
    return Reporting


def test_device_loader_keeps_the_gpu_out_of_the_workers(mini):
    torch.manual_seed(0)
    ds = _dataset(mini, cls=_reporting_dataset())
    before = torch.cuda.is_initialized()                                           # (False in a process without GPU tests)
    loader = ds.device_loader(batch_size=1, num_workers=2)
    assert len(loader) == len(ds) == 4 and loader.inner.num_workers == 2
    lists = list(loader.inner)
    assert all(isinstance(items, list) and len(items) == 1 and isinstance(items[0], dict) for items in lists)
    items = [items[0] for items in lists]
    assert {it["worker"][0] for it in items} == {0, 1}
    assert not any(it["worker"][1] for it in items)                                # no worker has the device open
    assert torch.cuda.is_initialized() == before
    assert all("ref_aug" in it and "frame" in it["image"] and "range_mask_corners" in it["lidar"] for it in items)
    draws = {w: [it["ref_aug"][k] for it in items if it["worker"][0] == w for k in ("flags", "warp", "table")] for w in (0, 1)}
    assert len(draws[0]) == len(draws[1]) == 6                                     # two items each; torch seeds `random` per worker
    assert not all(torch.equal(a, b) for a, b in zip(draws[0], draws[1]))
    assert [it["id_name"] for it in items] == [ds.get_id_name(ds.objects_meta.loc[i]) for i in range(4)]


def test_entry_points_validate_before_any_launch():
    """`mobi_ref_augment` / `mobi_drop_context` refuse bad arguments on the host (no GPU here: every call must return)."""
    import ctypes as C
    from mobi_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    p = _lib.RefAugmentParams()
    assert lib.mobi_ref_augment(None, None) == -1 and lib.mobi_ref_augment(C.byref(p), None) == -1
    p.src = p.flags = p.warp = p.table = p.out = 4096
    p.batch, p.size = 1, 0
    assert lib.mobi_ref_augment(C.byref(p), None) == -1
    p.size = 7
    assert lib.mobi_ref_augment(C.byref(p), None) == -2                            # the reflected halo needs S >= 8
    p.batch, p.size = 0, 224
    assert lib.mobi_ref_augment(C.byref(p), None) == -1
    p.batch, p.table = 2, None
    assert lib.mobi_ref_augment(C.byref(p), None) == -1
    assert lib.mobi_drop_context(None, 4096, 4096, 4096, 1, 3, 64, None) == -1
    assert lib.mobi_drop_context(4096, 4096, 4096, None, 1, 3, 64, None) == -1
    assert lib.mobi_drop_context(4096, 4096, 4096, 4096, 0, 3, 64, None) == -1
    assert lib.mobi_drop_context(4096, 4096, 4096, 4096, 1, 3, 0, None) == -1
    assert lib.mobi_struct_size(28) == C.sizeof(_lib.RefAugmentParams) == 48
