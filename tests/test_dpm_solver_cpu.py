"""DPM-Solver++(2M) without a GPU: the coefficient table against an fp64 restatement of the published algorithm, its
first-order rows against DDIM (eta = 0), the order of the last step, the sampler's argument rules and the host-side
checks of `mobi_dpm_step` (include/mobi_engine.h)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from oracle import sampler as osampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Model:
    """What the sampler reads of a LatentDiffusion for its schedule (the linear 0.00085 .. 0.012 betas, 1000 steps)."""
    num_timesteps = 1000
    device = torch.device("cpu")

    def __init__(self):
        buf = osampler.Schedule(1).buffers
        self.betas = torch.from_numpy(buf["betas"])
        self.alphas_cumprod = torch.from_numpy(buf["alphas_cumprod"])
        self.alphas_cumprod_prev = torch.from_numpy(buf["alphas_cumprod_prev"])


def _sampler(S):
    from mobi_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    s = DPMSolverSampler(_Model())
    s.make_schedule(S, verbose=False)
    return s


def _restated(S):
    """The issue's arithmetic, written out independently in fp64: rows {1/a_s, s_s/a_s, c_x, c_0, c_1} and the order."""
    ac = [float(v) for v in osampler.Schedule(1).buffers["alphas_cumprod"]]
    c = 1000 // S
    ts = list(range(1, 1000, c))[::-1]
    abar = [ac[t] for t in ts] + [ac[0]]
    a = [math.sqrt(v) for v in abar]
    sg = [math.sqrt(1 - v) for v in abar]
    lam = [math.log(a[k]) - math.log(sg[k]) for k in range(len(abar))]
    n = len(ts)
    rows, orders = [], []
    for i in range(n):
        h = lam[i + 1] - lam[i]
        m = -a[i + 1] * (math.exp(-h) - 1)               # x_t = sigma_t/sigma_s x + m D
        first = i == 0 or (i == n - 1 and S < 15)
        if first:
            c0, c1 = m, 0.0
        else:
            r = (lam[i] - lam[i - 1]) / h
            c0, c1 = m * (1 + 1 / (2 * r)), -m * (1 / (2 * r))
        rows.append([1 / a[i], sg[i] / a[i], sg[i + 1] / sg[i], c0, c1])
        orders.append(1 if first else 2)
    return ts, abar, np.array(rows), orders


@pytest.mark.parametrize("S", [10, 20, 50])
def test_coefficient_table_matches_fp64_restatement(S):
    s = _sampler(S)
    ts, abar, ref, orders = _restated(S)
    assert s.timesteps.tolist() == ts and s.timesteps.tolist() == np.flip(s.ddim_timesteps).tolist()
    np.testing.assert_allclose(s.abar, abar, rtol=0, atol=0)
    assert s.coef.dtype == np.float32 and s.coef.shape == (S, 5)
    # rounded once from fp64: within half an fp32 ulp of the restatement (relative 2^-24), signs and zeros included
    np.testing.assert_allclose(s.coef.astype(np.float64), ref, rtol=2.0 ** -24 * 1.01, atol=0)
    assert [1 if row[4] == 0 else 2 for row in s.coef] == orders
    assert s._coef_dev.dtype == torch.float32 and torch.equal(s._coef_dev, torch.from_numpy(s.coef))


@pytest.mark.parametrize("S", [10, 20, 50])
def test_first_order_rows_are_ddim_eta0(S):
    """DPM-Solver-1 is DDIM: x_t = sqrt(abar_t) x0 + sqrt(1 - abar_t) eps with eps = (x - alpha_s x0) / sigma_s, i.e.
    x_t = sigma_t/sigma_s x + (alpha_t - sigma_t alpha_s / sigma_s) x0; x0 = (x - sqrt(1 - a_t) e) / sqrt(a_t)."""
    from mobi_amd.ldm.models.diffusion.dpm_solver import dpm_coefficients, dpm_grid
    m = _Model()
    _, abar = dpm_grid(m.alphas_cumprod, S, 1000)
    tab = dpm_coefficients(abar, True)
    first = [i for i in range(tab.shape[0]) if tab[i, 4] == 0]
    assert 0 in first and tab.shape[0] - 1 in first
    for i in first:
        a_s, a_t = math.sqrt(abar[i]), math.sqrt(abar[i + 1])
        s_s, s_t = math.sqrt(1 - abar[i]), math.sqrt(1 - abar[i + 1])
        ddim = [1 / a_s, s_s / a_s, s_t / s_s, a_t - s_t * a_s / s_s]
        np.testing.assert_allclose(tab[i, :4], ddim, rtol=1e-12, atol=0)


@pytest.mark.parametrize("S", [5, 10, 14, 15, 20, 25, 50])
def test_last_step_first_order_exactly_below_15(S):
    s = _sampler(S)
    c1 = s.coef[:, 4]
    assert c1[0] == 0                                       # step 0 has no history
    assert (c1[-1] == 0) == (S < 15)
    assert all(v != 0 for v in c1[1:-1])                    # every other step is second order


def test_sampler_argument_rules():
    from mobi_amd.ldm.models.diffusion.dpm_solver import DPMSolverSampler
    from ldm.models.diffusion.dpm_solver import DPMSolverSampler as Aliased
    assert Aliased is DPMSolverSampler
    s = DPMSolverSampler(_Model())
    kw = dict(S=10, batch_size=1, shape=[4, 8, 8], verbose=False, rest=torch.zeros(1, 5, 8, 8))
    with pytest.raises(ValueError):
        s.sample(eta=0.5, **kw)
    with pytest.raises(NotImplementedError):
        s.sample(mask=torch.ones(1, 1, 8, 8), x0=torch.zeros(1, 4, 8, 8), **kw)
    with pytest.raises(NotImplementedError):
        s.sample(quantize_x0=True, **kw)
    with pytest.raises(Exception, match="test_model_kwargs"):
        s.sample(S=10, batch_size=1, shape=[4, 8, 8], verbose=False)


def test_dpm_step_host_argument_checks():
    """Null pointers or n <= 0: -1 before any launch (the fake addresses are never dereferenced)."""
    from mobi_amd import _lib
    lib = _lib.load()
    assert lib.mobi_abi_version() == 6
    assert lib.mobi_struct_size(20) == C.sizeof(_lib.DpmStepParams) and _lib.STRUCT_IDS[20] is _lib.DpmStepParams
    assert "mobi_dpm_step" in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "mobi_engine.h")) as f:
        assert "int mobi_dpm_step(const mobi_dpm_step_params* p, void* stream);" in f.read()
    assert lib.mobi_dpm_step(None, None) == -1
    fake = 0x1000
    required = ("x", "e_cond", "x0_hist", "x_next", "pred_x0")
    for missing in required:
        p = _lib.DpmStepParams()
        for name in required:
            if name != missing:
                setattr(p, name, fake)
        p.n = 16
        assert lib.mobi_dpm_step(C.byref(p), None) == -1, missing
    for n in (0, -5):
        p = _lib.DpmStepParams()
        for name in required:
            setattr(p, name, fake)
        p.n = n
        assert lib.mobi_dpm_step(C.byref(p), None) == -1
