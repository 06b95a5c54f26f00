"""Host side of the realism metrics (mobi_amd/realism.py): checkpoint key mapping, file pairing, the two resize rules, the
CLI's output line, the fp64 restatement's own properties and the igemm plan of the five AlexNet launches.  No GPU."""
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import realism_ref as R                                                  # noqa: E402
from mobi_amd import realism as M                                       # noqa: E402

SMALL = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, image_size=64, patch_size=32,
             projection_dim=16)


def _hf_to_openai(hf):
    """The inverse mapping written out independently: q, k, v concatenated into in_proj, proj transposed, `visual.` names."""
    hf = {k[len("vision_model."):] if k.startswith("vision_model.") else k: v for k, v in hf.items()}
    o = {"visual.conv1.weight": hf["embeddings.patch_embedding.weight"],
         "visual.class_embedding": hf["embeddings.class_embedding"],
         "visual.positional_embedding": hf["embeddings.position_embedding.weight"],
         "visual.ln_pre.weight": hf["pre_layrnorm.weight"], "visual.ln_pre.bias": hf["pre_layrnorm.bias"],
         "visual.ln_post.weight": hf["post_layernorm.weight"], "visual.ln_post.bias": hf["post_layernorm.bias"],
         "visual.proj": hf["visual_projection.weight"].t().contiguous(),
         "positional_embedding": torch.zeros(3, 4), "transformer.resblocks.0.ln_1.weight": torch.ones(4),   # text tower
         "logit_scale": torch.tensor(1.0)}
    n = 1 + max(int(k.split(".")[2]) for k in hf if k.startswith("encoder.layers."))
    for i in range(n):
        s, d = f"encoder.layers.{i}.", f"visual.transformer.resblocks.{i}."
        for leaf in ("weight", "bias"):
            o[d + "attn.in_proj_" + leaf] = torch.cat([hf[s + f"self_attn.{m}_proj.{leaf}"] for m in "qkv"], 0)
            o[d + "attn.out_proj." + leaf] = hf[s + "self_attn.out_proj." + leaf]
            o[d + "ln_1." + leaf] = hf[s + "layer_norm1." + leaf]
            o[d + "ln_2." + leaf] = hf[s + "layer_norm2." + leaf]
            o[d + "mlp.c_fc." + leaf] = hf[s + "mlp.fc1." + leaf]
            o[d + "mlp.c_proj." + leaf] = hf[s + "mlp.fc2." + leaf]
    return o


def test_openai_key_mapping_torch_save_and_scripted(tmp_path):
    hf = R.clip_b32_state(7, SMALL)
    oa = _hf_to_openai(hf)
    mapped = M.openai_to_hf(oa)
    want = {k[len("vision_model."):] if k.startswith("vision_model.") else k: v for k, v in hf.items()}
    assert set(mapped) == set(want)
    for k, v in want.items():
        assert torch.equal(mapped[k], v), k
    # both file forms load, and every parameter of the tower equals the original
    torch.save(oa, tmp_path / "plain.pt")

    class Scripted(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.visual = torch.nn.Module()
            for k, v in oa.items():
                mod, parts = self, k.split(".")
                for p in parts[:-1]:
                    if not hasattr(mod, p):
                        mod.add_module(p, torch.nn.Module())
                    mod = getattr(mod, p)
                mod.register_parameter(parts[-1], torch.nn.Parameter(v.clone(), requires_grad=False))

        def forward(self, x):
            return x

    torch.jit.save(torch.jit.script(Scripted()), str(tmp_path / "scripted.pt"))
    for name in ("plain.pt", "scripted.pt"):
        sd = M._read_checkpoint(str(tmp_path / name))
        hf2 = M.openai_to_hf(sd)
        proj = hf2.pop("visual_projection.weight")
        assert torch.equal(proj, want["visual_projection.weight"])
        from mobi_amd.ldm.modules.encoders.modules import CLIPVisionTower
        tower = CLIPVisionTower(**M._hf_config(hf2))
        tower.load_state_dict(hf2)
        got = dict(tower.named_parameters())
        assert set(got) == set(want) - {"visual_projection.weight"}
        for k, v in got.items():
            assert torch.equal(v.detach(), want[k]), (name, k)
    assert M._hf_config(M.openai_to_hf(oa)) == {k: SMALL[k] for k in SMALL if k != "projection_dim"} | {"num_attention_heads": 1}


def test_openai_mapping_rejects_unknown_visual_keys():
    with pytest.raises(KeyError):
        M.openai_to_hf({"visual.transformer.resblocks.0.attn.foo.weight": torch.zeros(1)})


def test_alexnet_and_lin_mapping(tmp_path):
    alex, lin = R.alex_state(3)
    alex = dict(alex, **{"classifier.1.weight": torch.zeros(4096, 9216), "classifier.1.bias": torch.zeros(4096)})
    torch.save(alex, tmp_path / "alexnet.pth")
    torch.save(lin, tmp_path / "alex.pth")
    convs, lins = M.lpips_state_from_dicts(torch.load(tmp_path / "alexnet.pth"), torch.load(tmp_path / "alex.pth"))
    for j, (idx, cin, cout, k, _, _) in enumerate(M.ALEX_CONVS):
        assert torch.equal(convs[j][0], alex[f"features.{idx}.weight"]) and convs[j][0].shape == (cout, cin, k, k)
        assert torch.equal(convs[j][1], alex[f"features.{idx}.bias"])
        assert torch.equal(lins[j], lin[f"lin{j}.model.1.weight"].reshape(-1))
    bad = dict(lin, **{"lin2.model.1.weight": torch.zeros(1, 383, 1, 1)})
    with pytest.raises(ValueError):
        M.lpips_state_from_dicts(alex, bad)


def _png(path, arr, mode="RGB"):
    from PIL import Image
    Image.fromarray(arr, mode).save(path)


def _rand_img(rng, h, w, c=3):
    return rng.integers(0, 256, size=(h, w, c) if c > 1 else (h, w), dtype=np.uint8)


def test_file_pairing_and_count_mismatch(tmp_path):
    rng = np.random.default_rng(0)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    names_a = ["2.png", "10.png", "1.jpg", "x.webp", "skip.txt"]
    names_b = ["b.png", "a.png", "c.jpeg", "d.bmp"]
    for n in names_a:
        if n.endswith(".txt"):
            (a / n).write_text("not an image")
        else:
            _png(a / n, _rand_img(rng, 8, 8))
    for n in names_b:
        _png(b / n, _rand_img(rng, 8, 8))
    pairs = M.paired_files(a, b)
    # the reference's rule: a glob per extension, then one sort of the paths (string order of the names)
    assert [p.name for p, _ in pairs] == ["1.jpg", "10.png", "2.png", "x.webp"]
    assert [q.name for _, q in pairs] == ["a.png", "b.png", "c.jpeg", "d.bmp"]
    _png(b / "e.png", _rand_img(rng, 8, 8))
    with pytest.raises(ValueError, match="should be same"):
        M.paired_files(a, b)


def test_lpips_resize_rule(tmp_path):
    """.convert('RGB') -> /255 -> bilinear (align_corners=False, no antialias) to 256 -> (x - .5) / .5, fp32 on the host."""
    rng = np.random.default_rng(1)
    for shape, mode in (((300, 200, 3), "RGB"), ((100, 90), "L"), ((256, 256, 3), "RGB")):
        arr = rng.integers(0, 256, size=shape, dtype=np.uint8)
        _png(tmp_path / "x.png", arr, mode)
        got = M.lpips_image(tmp_path / "x.png")
        rgb = np.repeat(arr[..., None], 3, 2) if arr.ndim == 2 else arr
        t = torch.from_numpy(rgb).permute(2, 0, 1).float() / 255
        want = F.interpolate(t[None], size=(256, 256), mode="bilinear", align_corners=False, antialias=False)[0] * 2 - 1
        assert got.dtype == torch.float32 and got.shape == (3, 256, 256)
        assert torch.equal(got, want), shape
    assert torch.equal(got, torch.from_numpy(rgb).permute(2, 0, 1).float() / 255 * 2 - 1)     # 256^2: the identity


def test_clip_resize_rule(tmp_path):
    """PIL bicubic resize of the short side to 224 (long side int(224 long / short)), centre crop at int(round((s - 224) / 2))."""
    from PIL import Image
    rng = np.random.default_rng(2)
    for h, w in ((300, 257), (224, 401), (500, 224), (224, 224), (100, 131)):
        arr = _rand_img(rng, h, w)
        _png(tmp_path / "y.png", arr)
        got = M.clip_image(tmp_path / "y.png")
        short, long = min(h, w), max(h, w)
        nl = int(224 * long / short)
        im = Image.fromarray(arr)
        if short != 224:
            im = im.resize((224, nl) if w <= h else (nl, 224), Image.BICUBIC)
        ww, hh = im.size
        top, left = int(round((hh - 224) / 2.0)), int(round((ww - 224) / 2.0))
        want = np.asarray(im)[top:top + 224, left:left + 224]
        assert got.shape == (3, 224, 224)
        assert torch.equal(got, torch.from_numpy(want.copy()).permute(2, 0, 1).float() / 255), (h, w)
        if (h, w) in ((224, 401), (224, 224)):
            assert torch.equal(got, torch.from_numpy(arr[:, left:left + 224].copy()).permute(2, 0, 1).float() / 255)


def test_cli_line_parses_with_the_reference_grep():
    """The reference's shell scripts read the number with grep -oP 'LPIPS:\\s*\\K[0-9.]+' (and CLIP likewise)."""
    for name, v in (("LPIPS", 0.123456789), ("CLIP", 87.65432)):
        buf = io.StringIO()
        print(f"{name}: ", v, file=buf)
        m = re.search(rf"{name}:\s*([0-9.]+)", buf.getvalue())
        assert m and float(m.group(1)) == v
    src = open(M.__file__).read()
    assert 'print("LPIPS: ", v)' in src and 'print("CLIP: ", v)' in src


def test_cli_refuses_mismatched_directories(tmp_path):
    from PIL import Image
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(a / "0.png")
    r = subprocess.run([sys.executable, "-m", "mobi_amd.realism", "lpips", "--path_target", str(a), "--path_pred", str(b),
                        "--alexnet", "none", "--lin", "none"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "LPIPS:" not in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 restatement itself
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_identity_symmetry_and_eps():
    convs, lins = M.lpips_state_from_dicts(*R.alex_state(11))
    x, y = R.lpips_images("ref.x", 3, 67, 75), R.lpips_images("ref.y", 3, 67, 75)
    assert torch.equal(R.lpips(x, x, convs, lins), torch.zeros(3, dtype=torch.float64))
    assert torch.allclose(R.lpips(x, y, convs, lins), R.lpips(y, x, convs, lins), rtol=1e-13, atol=0)
    d = R.lpips(x, y, convs, lins)
    assert (d > 0).all() and torch.isfinite(d).all()


def test_restatement_one_layer_by_hand():
    """Two 1 x 1 'images' with C = 2 channels: the term is sum_c w_c (a_c / (|a| + eps) - b_c / (|b| + eps))^2."""
    a = torch.tensor([3.0, 4.0], dtype=torch.float64).view(1, 2, 1, 1)
    b = torch.tensor([0.0, 2.0], dtype=torch.float64).view(1, 2, 1, 1)
    w = torch.tensor([0.5, 2.0], dtype=torch.float64)
    e = 1e-10
    want = 0.5 * (3 / (5 + e) - 0) ** 2 + 2.0 * (4 / (5 + e) - 2 / (2 + e)) ** 2
    assert abs(float(R.layer_distance(a, b, w)) - want) < 1e-12
    z = torch.zeros_like(a)
    assert float(R.layer_distance(z, z, w)) == 0.0 and torch.isfinite(R.layer_distance(z, b, w)).all()


def test_restatement_matches_transformers_clip():
    transformers = pytest.importorskip("transformers")
    cfg = transformers.CLIPVisionConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                                        image_size=64, patch_size=32, projection_dim=16, hidden_act="quick_gelu")
    model = transformers.CLIPVisionModelWithProjection(cfg).eval()
    from oracle import weights as W
    W.fill_module_(model, seed=5)
    names = {k for k, _ in model.named_parameters()}
    shapes = R.clip_b32_shapes(dict(SMALL, num_attention_heads=2))
    assert names == set(shapes) and all(tuple(p.shape) == shapes[k] for k, p in model.named_parameters())
    sd = {k: v.detach() for k, v in model.named_parameters()}
    imgs = R.clip_images("ref.clip", 3, 64)
    mean = torch.tensor(R.CLIP_MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(R.CLIP_STD, dtype=torch.float64).view(1, 3, 1, 1)
    with torch.no_grad():
        want = model.double()(pixel_values=(imgs.double() - mean) / std).image_embeds
    got = R.clip_embed(imgs, sd, heads=2)
    assert float((got - want).abs().max()) < 1e-12, float((got - want).abs().max())


def test_golden_matches_restatement_at_full_size(golden_dir):
    """The golden file's embeddings are what the restatement computes from the seed (ViT-B/32, fp64)."""
    g = np.load(os.path.join(golden_dir, "realism_clip.npz"))
    sys.path.insert(0, golden_dir)
    import make_golden_realism as MG
    ref, pred = MG.images()
    sd = R.clip_b32_state(int(g["seed"]))
    er = R.clip_embed(ref[:2], sd)
    assert np.allclose(er.numpy(), g["embeds_ref"][:2], rtol=1e-9, atol=1e-10)
    assert g["score"][0] == pytest.approx(100.0, abs=1e-9)


# ---------------------------------------------------------------------------------------------------------------------
# the launch plan
# ---------------------------------------------------------------------------------------------------------------------
def test_alexnet_igemm_plan(monkeypatch):
    """Which mobi_igemm main loop each AlexNet layer lands on (host logic, no launch), batch 64 pairs at 256^2 and 1 pair."""
    from mobi_amd import _lib
    for key in [k for k in os.environ if k.startswith("MOBI_")]:
        monkeypatch.delenv(key, raising=False)
    lib = _lib.load()
    lib.mobi_tuning_reload()
    RING128, RING256 = 4, 5
    assert M.alexnet_shapes(256, 256) == [(256, 256, 63, 63), (31, 31, 31, 31), (15, 15, 15, 15), (15, 15, 15, 15),
                                          (15, 15, 15, 15)]
    assert M.igemm_plan(256, 256, 64) == [(RING256, 1), (RING256, 1), (RING256, 1), (RING128, 1), (RING128, 1)]
    assert M.igemm_plan(256, 256, 1) == [(RING128, 4), (RING128, 3), (RING128, 3), (RING128, 4), (RING128, 4)]   # split-K fills the chip
    assert M.igemm_plan(256, 256, 64, torch.bfloat16) == M.igemm_plan(256, 256, 64)
