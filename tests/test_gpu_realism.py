"""Realism metrics on the MI355X (mobi_amd/realism.py): the new kernels on the same stored operands, LPIPS end to end against
the fp64 restatement (tests/realism_ref.py), CLIP score against transformers' ViT-B/32 (tests/golden/realism_clip.npz), and
the file tool against the tensor API.

Measured errors (seeded weights, lins 0.1 |noise|) are printed by each test and recorded next to its bound."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import realism_ref as R                                                  # noqa: E402
from mobi_amd import ops, realism as M                                  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.float16, torch.bfloat16)

# LPIPS |delta| per pair / of the mean against fp64 (values 1e-4 .. 0.145 here).  fp16: the targets (LPIPS is reported to three
# decimals); measured on the MI355X at most 4.2e-6 / 1.7e-6.  bf16: measured 2.23e-5 / 6.5e-6, bound = measured + 20 %.
LPIPS_BOUND = {torch.float16: (2e-3, 5e-4), torch.bfloat16: (2.7e-5, 7.9e-6)}
# CLIP score |delta| per pair / of the mean against the golden (0-100 scale, reported to two decimals).  fp16: the targets;
# measured 6.5e-3 / 1.1e-3 (embedding rel-L2 1.2e-3).  bf16: measured 2.08e-2 / 4.5e-4 (rel-L2 9.2e-3), bound = measured + 20 %.
CLIP_BOUND = {torch.float16: (0.05, 0.01), torch.bfloat16: (0.025, 5.5e-4)}


@pytest.fixture(scope="module")
def alex():
    return M.lpips_state_from_dicts(*R.alex_state(13))


def _lpips(alex, dtype):
    return M.LPIPS(*alex, dtype=dtype, device=DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu", [False, True])
def test_maxpool_bit_identical(dtype, relu):
    x = torch.randn(3, 63, 47, 64, device=DEV).to(dtype)
    got = ops.maxpool3s2(x, relu=relu)
    src = torch.relu(x) if relu else x
    want = F.max_pool2d(src.permute(0, 3, 1, 2).float(), 3, 2).to(dtype).permute(0, 2, 3, 1)
    assert got.shape == want.shape == (3, 31, 23, 64)
    assert torch.equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("pairs,h,w,c", [(1, 63, 63, 64), (7, 15, 15, 384), (64, 15, 15, 256), (5, 31, 31, 192)])
def test_layer_distance_against_fp64(dtype, pairs, h, w, c):
    feat = (torch.randn(2 * pairs, h, w, c, device=DEV) * 3).to(dtype)
    feat[pairs - 1] = feat[2 * pairs - 1]                                 # one identical pair: exactly 0
    lin = torch.rand(c, device=DEV) * 0.2
    base = torch.rand(pairs, device=DEV)
    keep = feat.clone()
    out = ops.lpips_distance(feat, lin, base.clone(), relu_in_place=True)
    f64 = keep.double().permute(0, 3, 1, 2)
    want = base.double() + R.layer_distance(torch.relu(f64[:pairs]), torch.relu(f64[pairs:]), lin)
    rel = float(((out.double() - want).abs() / want.abs()).max())
    print(f"layer distance {dtype} pairs {pairs} {h}x{w}x{c}: max rel {rel:.2e}")
    assert rel <= 1e-6
    assert float(out[pairs - 1]) == float(base[pairs - 1])
    assert torch.equal(feat, torch.relu(keep))                            # relu written back in place
    out2 = ops.lpips_distance(keep.clone(), lin, base.clone())
    assert torch.equal(out2, out)                                         # bitwise reproducible


def test_row_cosine_against_fp64():
    a, b = torch.randn(64, 512, device=DEV), torch.randn(64, 512, device=DEV)
    b[:8] = a[:8] * 0.5 + b[:8] * 0.01
    a[63] = 0
    got = ops.row_cosine(a, b, eps=1e-8, scale=100.0)
    want = 100.0 * F.cosine_similarity(a.double(), b.double(), dim=-1, eps=1e-8)
    err = (got.double() - want).abs()
    assert float((err[:63] / want[:63].abs().clamp_min(1.0)).max()) <= 1e-6
    assert float(got[63]) == 0.0


def test_image_normalize_matches_torch():
    x = torch.rand(3, 3, 20, 24, device=DEV)
    got = ops.image_normalize(x, M.CLIP_MEAN, M.CLIP_STD)
    want = (x - torch.tensor(M.CLIP_MEAN, device=DEV).view(1, 3, 1, 1)) / torch.tensor(M.CLIP_STD, device=DEV).view(1, 3, 1, 1)
    assert torch.equal(got, want)
    for dtype in DTYPES:
        y = ops.image_normalize(x, M.LPIPS_SHIFT, M.LPIPS_SCALE, dtype=dtype, nhwc_channels=32)
        sh = torch.tensor(M.LPIPS_SHIFT, device=DEV).view(1, 3, 1, 1)
        sc = torch.tensor(M.LPIPS_SCALE, device=DEV).view(1, 3, 1, 1)
        assert torch.equal(y[..., :3], ((x - sh) / sc).to(dtype).permute(0, 2, 3, 1))
        assert not y[..., 3:].any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,h,w", [(1, 256, 256), (7, 256, 256), (64, 256, 256), (5, 200, 296)])
def test_lpips_end_to_end(alex, dtype, n, h, w):
    model = _lpips(alex, dtype)
    a = R.lpips_images(f"lp.a{n}", n, h, w)
    other = R.lpips_images(f"lp.b{n}", n, h, w)
    t = torch.linspace(0.02, 1.0, n).view(n, 1, 1, 1)                      # from near-identical to unrelated pairs
    b = ((1 - t) * a + t * other).clamp(-1, 1)
    got = model(a.to(DEV), b.to(DEV)).cpu().double()
    want = R.lpips(a, b, *alex)
    d = (got - want).abs()
    dm = abs(float(got.mean() - want.mean()))
    print(f"LPIPS {dtype} n={n} {h}x{w}: ref {float(want.min()):.4f}..{float(want.max()):.4f}  max |d| {float(d.max()):.2e}  "
          f"|d mean| {dm:.2e}")
    per, mean = LPIPS_BOUND[dtype]
    assert torch.isfinite(got).all()
    assert float(d.max()) <= per and dm <= mean


@pytest.mark.parametrize("dtype", DTYPES)
def test_lpips_identity_is_zero_and_repeatable(alex, dtype):
    model = _lpips(alex, dtype)
    a = R.lpips_images("lp.id", 9, 256, 256).to(DEV)
    b = R.lpips_images("lp.id2", 9, 256, 256).to(DEV)
    assert torch.equal(model(a, a), torch.zeros(9, device=DEV))
    r1, r2 = model(a, b), model(a, b)
    assert torch.equal(r1, r2)


def test_lpips_dead_conv5_is_finite(alex):
    convs, lins = alex
    convs = list(convs)
    convs[4] = (convs[4][0], torch.full_like(convs[4][1], -1e3))          # conv5 never fires: relu5 == 0 everywhere
    model = M.LPIPS(convs, lins, device=DEV)
    a = R.lpips_images("lp.dead.a", 3, 256, 256)
    b = R.lpips_images("lp.dead.b", 3, 256, 256)
    got = model(a.to(DEV), b.to(DEV)).cpu().double()
    want = R.lpips(a, b, convs, lins)
    assert torch.isfinite(got).all()
    assert float((got - want).abs().max()) <= LPIPS_BOUND[torch.float16][0]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "realism_clip.npz"))


@pytest.fixture(scope="module")
def clip_images(golden_dir):
    sys.path.insert(0, golden_dir)
    import make_golden_realism as MG
    return MG.images()


@pytest.mark.parametrize("dtype", DTYPES)
def test_clip_score_against_golden(golden, clip_images, dtype):
    model = M.CLIPScore.from_state_dict(R.clip_b32_state(int(golden["seed"])), dtype=dtype, device=DEV)
    ref, pred = clip_images
    er = model.embed(ref.to(DEV)).cpu().double().numpy()
    rel = np.linalg.norm(er - golden["embeds_ref"]) / np.linalg.norm(golden["embeds_ref"])
    got = model(ref.to(DEV), pred.to(DEV)).cpu().double().numpy()
    d = np.abs(got - golden["score"])
    dm = abs(got.mean() - golden["score"].mean())
    print(f"CLIP {dtype}: embedding rel-L2 {rel:.2e}  scores {np.round(got, 3)}  max |d| {d.max():.2e}  |d mean| {dm:.2e}")
    per, mean = CLIP_BOUND[dtype]
    assert d.max() <= per and dm <= mean
    self_score = model(ref.to(DEV), ref.to(DEV)).cpu()
    assert float((self_score - 100.0).abs().max()) <= 1e-3


def test_clip_score_ignores_engine_dtype(golden, clip_images):
    import mobi_amd
    model = M.CLIPScore.from_state_dict(R.clip_b32_state(int(golden["seed"])), device=DEV)
    ref, pred = clip_images
    prev = mobi_amd.engine_dtype()
    try:
        mobi_amd.set_engine_dtype(torch.float16)
        a = model(ref.to(DEV), pred.to(DEV))
        mobi_amd.set_engine_dtype(torch.bfloat16)
        b = model(ref.to(DEV), pred.to(DEV))
        assert mobi_amd.engine_dtype() == torch.bfloat16
    finally:
        mobi_amd.set_engine_dtype(prev)
    assert torch.equal(a, b)


def test_file_tools_match_tensor_api(tmp_path, alex, golden):
    from PIL import Image
    rng = np.random.default_rng(4)
    for d in ("t", "p"):
        (tmp_path / d).mkdir()
    n = 5
    for i in range(n):
        for d in ("t", "p"):
            Image.fromarray(rng.integers(0, 256, (240, 300, 3), dtype=np.uint8)).save(tmp_path / d / f"{i:03d}.png")
    pairs = M.paired_files(tmp_path / "t", tmp_path / "p")
    lp = _lpips(alex, torch.float16)
    mean, per = M.lpips_score_paths(tmp_path / "t", tmp_path / "p", lp)
    a = torch.stack([M.lpips_image(p) for p, _ in pairs])
    b = torch.stack([M.lpips_image(q) for _, q in pairs])
    assert torch.equal(per.cpu(), lp(a.to(DEV), b.to(DEV)).cpu())
    assert mean == per.mean().item()
    cs = M.CLIPScore.from_state_dict(R.clip_b32_state(int(golden["seed"])), device=DEV)
    mean, per = M.clip_score_paths(tmp_path / "t", tmp_path / "p", cs)
    a = torch.stack([M.clip_image(p) for p, _ in pairs])
    b = torch.stack([M.clip_image(q) for _, q in pairs])
    assert torch.equal(per.cpu(), cs(a.to(DEV), b.to(DEV)).cpu())
    assert mean == per.mean().item()
