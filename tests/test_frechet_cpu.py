"""FID / FRD host side: the fp64 Fréchet distance against the reference's scipy form (golden), the RangeNet packing rewrites
against torch in fp64, the fp64 restatement against the reference model's golden features, strict key mapping, the CLI lines
and the igemm plan of the 67 RangeNet launches.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mobi_amd import _lib, realism as R
from tests import frd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "frd.npz")


def golden():
    return np.load(GOLDEN)


def golden_views():
    """The golden's six 512 x 512 range views, rebuilt from their stored codes."""
    gd = golden()
    return frd_ref.views_from_codes(gd["depth_codes"], gd["int_codes"])


# ---------------------------------------------------------------------------------------------------------------------
# the distance
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["well", "rankdef", "same", "one"])
def test_frechet_distance_matches_reference(case):
    a, b = frd_ref.frechet_cases()[case]
    stat = lambda f: (f.mean(0), np.cov(f, rowvar=False))
    got = R.frechet_distance(*stat(a), *stat(b))
    want = float(golden()[f"fd_{case}"])
    err = abs(got - want)
    print(f"{case}: ours {got!r} reference {want!r} abs err {err:.3e}")
    if case == "same":
        # 0 up to the rounding of tr S + tr S - 2 tr sqrtm(S S) with a singular S (rank 99): both forms land near -3e-5
        tr = np.trace(np.cov(a, rowvar=False))
        assert abs(got) < 1e-7 * tr and abs(want) < 1e-7 * tr
    elif case == "rankdef":
        # S1 S2 is singular (rank 99 of 512): scipy's Schur-based sqrtm is accurate to ~1e-8 there (measured 2.4e-8 relative)
        assert err <= 1e-7 * abs(want), (got, want)
    else:
        assert err <= 1e-9 * abs(want), (got, want)


def test_frechet_1d_by_hand():
    # 1-d: (m1 - m2)^2 + s1 + s2 - 2 sqrt(s1 s2) = (m1 - m2)^2 + (sqrt s1 - sqrt s2)^2
    assert R.frechet_distance([1.0], [[4.0]], [3.0], [[9.0]]) == pytest.approx(4.0 + 1.0, rel=1e-14)


def test_stats_refuse_fewer_than_two_rows():
    st = R.FrechetStats.__new__(R.FrechetStats)
    st.n = 1
    with pytest.raises(ValueError, match="at least 2"):
        st.mu_sigma()


# ---------------------------------------------------------------------------------------------------------------------
# packing rewrites (fp64 against torch)
# ---------------------------------------------------------------------------------------------------------------------
def _paired(x):
    """NCHW [N, C, H, W] -> the channels-last [H][W/2][2C] view, in NCHW: channel half * C + c of pair p = x[..., 2p + half]."""
    n, c, h, w = x.shape
    return x.reshape(n, c, h, w // 2, 2).permute(0, 4, 1, 2, 3).reshape(n, 2 * c, h, w // 2)


def test_stride2_rewrite_matches_conv2d():
    g = torch.Generator().manual_seed(0)
    x = torch.randn((2, 6, 5, 16), generator=g, dtype=torch.float64)
    w = torch.randn((7, 6, 3, 3), generator=g, dtype=torch.float64)
    want = F.conv2d(x, w, stride=(1, 2), padding=1)
    got = F.conv2d(F.pad(_paired(x), (1, 0, 1, 1)), R.stride2_weight(w))
    err = (got - want).abs().max().item()
    print(f"stride-(1, 2) rewrite max err {err:.2e}")
    assert got.shape == want.shape and err < 1e-12


def test_upconv_rewrite_matches_conv_transpose2d():
    g = torch.Generator().manual_seed(1)
    x = torch.randn((2, 6, 3, 8), generator=g, dtype=torch.float64)
    w = torch.randn((6, 5, 1, 4), generator=g, dtype=torch.float64)
    b = torch.randn((5,), generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(x, w, b, stride=(1, 2), padding=(0, 1))               # [N, 5, 3, 16]
    wc, bc = R.upconv_weight(w, b)
    y = F.conv2d(x, wc, bc, padding=(0, 1))                                          # [N, 10, 3, 8]: [H][W][2C] channels
    n, c2, h, wd = y.shape
    got = y.reshape(n, 2, c2 // 2, h, wd).permute(0, 2, 3, 4, 1).reshape(n, c2 // 2, h, 2 * wd)
    err = (got - want).abs().max().item()
    print(f"transpose rewrite max err {err:.2e}")
    assert err < 1e-12


def test_fold_bn_matches_batch_norm():
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 4, 5, 6), generator=g, dtype=torch.float64)
    w = torch.randn((3, 4, 3, 3), generator=g, dtype=torch.float64)
    sd = {"bn.weight": torch.rand(3, generator=g, dtype=torch.float64) + 0.5, "bn.bias": torch.randn(3, generator=g, dtype=torch.float64),
          "bn.running_mean": torch.randn(3, generator=g, dtype=torch.float64),
          "bn.running_var": torch.rand(3, generator=g, dtype=torch.float64) + 0.1}
    want = F.batch_norm(F.conv2d(x, w, padding=1), sd["bn.running_mean"], sd["bn.running_var"], sd["bn.weight"], sd["bn.bias"],
                        False, 0.0, 1e-5)
    wf, bf = R.fold_bn(w, sd, "bn")
    err = (F.conv2d(x, wf, bf, padding=1) - want).abs().max().item()
    print(f"BN fold max err {err:.2e}")
    assert err < 1e-12


def test_rangenet_layers_restate_the_model():
    """The 67 folded / rewritten layers, run in fp64 with torch on the channels-last views the engine uses, equal the fp64
    restatement -- on a small input (the layer graph, not the numbers, is what is checked)."""
    bb, dec = frd_ref.seeded_state_dicts(3)
    x = torch.randn((1, 5, 64, 64), generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    want = frd_ref.forward(bb, dec, x)
    layers = {name: (w, b, kind) for name, w, b, kind in R.rangenet_layers(bb, dec)}
    assert len(layers) == 67

    def conv(t, name, res=None):
        w, b, kind = layers[name]
        if kind == "down":
            y = F.conv2d(F.pad(_paired(t), (1, 0, 1, 1)), w, b)
        elif kind == "up":
            y = F.conv2d(t, w, b, padding=(0, 1))
            n, c2, h, wd = y.shape
            y = y.reshape(n, 2, c2 // 2, h, wd).permute(0, 2, 3, 4, 1).reshape(n, c2 // 2, h, 2 * wd)
        else:
            y = F.conv2d(t, w, b, padding=w.shape[-1] // 2)
        y = F.leaky_relu(y, 0.1)
        return y if res is None else y + res

    t = conv(x, "conv1")
    skips = [t]
    for i, nb in enumerate(R.RANGENET_BLOCKS, 1):
        t = conv(t, f"enc{i}.conv")
        for r in range(nb):
            t = conv(conv(t, f"enc{i}.residual_{r}.conv1"), f"enc{i}.residual_{r}.conv2", t)
        skips.append(t)
    skips.pop()
    for i in range(5, 0, -1):
        u = conv(t, f"dec{i}.upconv")
        t = conv(conv(u, f"dec{i}.residual.conv1"), f"dec{i}.residual.conv2", u) + skips.pop()
    got = t.reshape(1, 32, 16, 4, 64).mean((3, 4)).reshape(1, -1)
    err = ((got - want).norm() / want.norm()).item()
    print(f"folded layer graph vs restatement rel-L2 {err:.2e}")
    assert err < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 restatement against the reference (golden)
# ---------------------------------------------------------------------------------------------------------------------
def test_restated_prepare_matches_reference():
    gd = golden()
    prep = torch.stack([frd_ref.prepare(v) for v in golden_views()])
    mask = ~(prep == -1).all(1)
    assert np.array_equal(np.packbits(mask.numpy(), axis=-1), gd["mask"])
    assert np.array_equal(prep.reshape(6, 5, -1)[:, :, ::256].numpy(), gd["prep_sample"])
    # the boundary values are on the sampled rows: both sides of 1.4 m and of 54 m occur
    assert 0 < mask.float().mean() < 1


def test_restated_features_match_reference():
    gd = golden()
    x = torch.stack([frd_ref.prepare(v) for v in golden_views()]).double()
    bb, dec = frd_ref.seeded_state_dicts(int(gd["seeds"][0]), x)
    got = frd_ref.forward(bb, dec, x).numpy()
    want = gd["features"]
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"fp64 restatement vs reference features rel-L2 {err:.2e}")
    assert err < 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# key mapping, files, CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_rangenet_key_counts_and_strict_mapping():
    bb_keys, dec_keys = R.rangenet_keys()
    assert len(bb_keys) == 312 and len(dec_keys) == 95
    bb, dec = frd_ref.seeded_state_dicts(0)
    R._check_keys(bb, bb_keys, "backbone")
    R._check_keys(dec, dec_keys, "segmentation_decoder")
    missing = dict(bb)
    del missing["enc3.residual_5.conv2.weight"]
    with pytest.raises(KeyError, match="missing keys.*enc3.residual_5.conv2.weight"):
        R.RangeNet.from_state_dicts(missing, dec, device="cpu")
    extra = dict(dec)
    extra["dec5.residual.bn3.weight"] = torch.ones(3)
    with pytest.raises(KeyError, match="unexpected keys.*dec5.residual.bn3.weight"):
        R.RangeNet.from_state_dicts(bb, extra, device="cpu")


def test_cli_lines_parse_with_the_shipped_greps():
    for line, pat in (("FID:  12.5", r"FID:\s*\K[0-9.]+"), ("FRD:  0.031", r"FRD:\s*\K[0-9.]+")):
        m = re.search(pat.replace(r"\K", ""), line)      # python re has no \K: the lookbehind-free equivalent
        assert m and re.search(r"[0-9.]+$", line).group(0) in line
    out = subprocess.run(["grep", "-oP", r"FID:\s*\K[0-9.]+"], input="FID:  %s\n" % 3.25, capture_output=True, text=True)
    assert out.stdout.strip() == "3.25"


def test_cli_has_fid_and_frd_with_reference_flags():
    ap_help = subprocess.run([sys.executable, "-m", "mobi_amd.realism", "frd", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert "--path-target" in ap_help.stdout and "--path-pred" in ap_help.stdout and "--weights-dir" in ap_help.stdout
    ap_help = subprocess.run([sys.executable, "-m", "mobi_amd.realism", "fid", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert "--path_target" in ap_help.stdout and "--path_pred" in ap_help.stdout and "--weights" in ap_help.stdout


def test_fewer_than_two_files_refused(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    np.save(a / "0.npy", np.zeros((4, 8, 8), np.float32))
    for i in range(3):
        np.save(b / f"{i}.npy", np.zeros((4, 8, 8), np.float32))
    with pytest.raises(ValueError, match="at least 2 files"):
        R.frd_paths(a, b, model=None)


def test_unpaired_set_sizes_accepted(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    for i in range(2):
        np.save(a / f"{i}.npy", np.full((4, 8, 8), i, np.float32))
    for i in range(3):
        np.save(b / f"{i}.npy", np.full((4, 8, 8), i, np.float32))

    class Fake:
        def stats(self, batches):
            f = np.concatenate([x.reshape(x.shape[0], -1)[:, :2].numpy() for x in batches]).astype(np.float64)
            return f.mean(0), np.cov(f, rowvar=False)

    d = R.frd_paths(a, b, Fake(), batch_size=2)
    assert np.isfinite(d)


# ---------------------------------------------------------------------------------------------------------------------
# the igemm plan of the 67 launches (host logic, no launch)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [64, 37, 1])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_rangenet_igemm_plan_only_names_leaky_variants(batch, dtype):
    plans = R.rangenet_igemm_plan(batch, dtype)
    assert len(plans) == 67
    assert all(v in (4, 5) for v, _ in plans), plans          # MOBI_IGEMM_RING_128 / MOBI_IGEMM_RING_256
    assert all(s == 1 for _, s in plans), plans
    if batch == 64:
        assert {v for v, _ in plans} == {4, 5}


def test_leaky_epilogue_refuses_what_it_cannot_apply():
    lib = _lib.load()
    import ctypes as C
    from mobi_amd import ops
    q = _lib.IgemmParams()
    q.src0 = q.weight = q.out = q.bias = 4096
    q.c0, q.batch, q.hin, q.win, q.hout, q.wout = 64, 4, 16, 16, 16, 16
    q.kh = q.kw = 3
    q.stride, q.pad_h, q.pad_w, q.groups, q.n_packed, q.cout = 1, 1, 1, 1, 64, 64
    q.scale, q.dtype, q.epilogue = 1.0, ops._dt(torch.float16), _lib.EPI_LEAKY_RELU
    assert lib.mobi_igemm_kernel_variant(C.byref(q)) in (4, 5)
    assert lib.mobi_igemm_plan_splits(C.byref(q)) == 1
    UNSUPPORTED = -2
    for field, val in (("out_mode", 1), ("split_k", 2), ("ln_svec", 4096)):
        r = _lib.IgemmParams.from_buffer_copy(q)
        setattr(r, field, val)
        if field == "split_k":
            r.ws = 4096
        assert lib.mobi_igemm_kernel_variant(C.byref(r)) == UNSUPPORTED, field
