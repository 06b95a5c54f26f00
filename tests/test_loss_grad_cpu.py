"""CPU: the fp64 restatement of `mobi_loss_grad`'s contract (tests/loss_grad_ref.py) against the reference's own `p_losses` numbers
(tests/golden/losses.npz) and against torch.autograd of the reference's formula; the new parameter struct's layout; the
unchanged positional signature of `train.loss_and_gradients`."""
import ctypes as C
import inspect

import pytest
import torch

from tests.golden_cases import load
from tests.loss_grad_ref import coefficients, loss_grad_ref, reference_formula

LOGVAR, ELBO = 0.3, 0.25            # what tests/golden/make_golden_losses.py set on the reference


@pytest.mark.parametrize("loss_type,pre", [("l2", ""), ("l1", "l1_")])
def test_helper_terms_equal_the_references_p_losses(loss_type, pre):
    """2e-6 relative: the bound tests/test_gpu_models.py uses for these numbers (the reference sums in fp32, the helper in fp64)."""
    g = load("losses")
    logvar = torch.full((1000,), LOGVAR)
    _, per, terms = loss_grad_ref(g["model_out"], g["noise"], g["t"], logvar, g["lvlb_weights"], loss_type, 1.0, ELBO)
    for i, key in enumerate(("val__loss_simple", "val__loss_vlb", "val__loss")):
        want = float(g[pre + key])
        assert abs(float(terms[i]) - want) <= 2e-6 * abs(want), (loss_type, key, float(terms[i]), want)
    assert abs(float(terms[2]) - float(g[pre + "loss"])) <= 2e-6 * abs(float(g[pre + "loss"]))
    assert abs(float(per.mean()) - float(terms[0])) <= 1e-15 * abs(float(terms[0]))


@pytest.mark.parametrize("loss_type", ["l2", "l1"])
@pytest.mark.parametrize("lsw,elbo", [(1.0, 0.0), (1.0, 0.25), (0.7, 0.25)])
def test_helper_gradient_equals_autograd_of_the_reference_formula(loss_type, lsw, elbo):
    """dy (before the storage rounding) against d(loss_scale * loss) / d eps from torch.autograd in fp64.  The helper's one
    departure from exact arithmetic is the contract's fp32 rounding of k_i: 2^-24 relative on k_i, on both products of l2."""
    g = load("losses")
    torch.manual_seed(5)
    n, c, h, w = 5, 4, 6, 7
    eps, target = torch.randn(n, c, h, w), torch.randn(n, c, h, w)
    eps[2, 1, 3, 4] = target[2, 1, 3, 4]                                      # a tie: |.|'s gradient is 0 there
    t = torch.tensor([0, 1, 999, 500, 1])
    logvar = torch.rand(1000) * 2 - 1
    lvlb, scale = g["lvlb_weights"], 256.0
    e64 = eps.double().requires_grad_(True)
    _, d = reference_formula(e64, target.double(), t, logvar.double(), lvlb.double(), loss_type, lsw, elbo)
    (scale * d["loss"]).backward()
    dy, per, terms = loss_grad_ref(eps, target, t, logvar, lvlb, loss_type, lsw, elbo, scale)
    k = coefficients(t, logvar, lvlb, loss_type, lsw, elbo, scale, eps.numel()).view(n, 1, 1, 1)
    bound = 2.0 ** -23 * k.abs() * (eps.double().abs() + target.double().abs() if loss_type == "l2" else 1.0)
    assert bool(((dy - e64.grad).abs() <= bound).all()), float((dy - e64.grad).abs().max())
    assert float(dy[2, 1, 3, 4]) == 0.0 and float(dy.abs().sum()) > 0
    # the terms are the formula's, in fp64 (the elements are formed in fp32: 2^-24 relative each)
    for i, key in enumerate(("loss_simple", "loss_vlb", "loss")):
        assert abs(float(terms[i]) - float(d[key].detach())) <= 1e-6 * abs(float(d[key].detach()))


def test_helper_defaults_and_out_of_range_t():
    """Zero tables, weight 1, ELBO weight 0: k = fp32(2 * loss_scale / numel) for every sample and loss == loss_simple's mean; a t
    outside the table reads its nearest end (mobi_q_sample's rule)."""
    import numpy as np
    torch.manual_seed(1)
    eps, target = torch.randn(3, 4, 5, 7), torch.randn(3, 4, 5, 7)
    z = torch.zeros(1)
    dy, per, terms = loss_grad_ref(eps, target, torch.tensor([7, 0, 900]), z, z, "l2", 1.0, 0.0, 256.0)
    k = float(np.float32(2.0 * 256.0 / eps.numel()))
    assert torch.equal(dy, k * eps.double() + (-k) * target.double())
    assert float(terms[0]) == float(terms[2]) and float(terms[1]) == 0.0
    tab = torch.tensor([0.5, -0.25, 0.125])
    a = loss_grad_ref(eps, target, torch.tensor([-4, 1, 17]), tab, tab.abs(), "l1", 1.0, 0.25, 2.0)
    b = loss_grad_ref(eps, target, torch.tensor([0, 1, 2]), tab, tab.abs(), "l1", 1.0, 0.25, 2.0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_loss_grad_struct_layout_and_validation():
    """`mobi_loss_grad_params` is struct id 27, 128 bytes, in the library and in the binding; the entry point validates on the
    host, before any launch."""
    from mobi_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.mobi_struct_size(27) == C.sizeof(_lib.LossGradParams) == 128 and _lib.STRUCT_IDS[27] is _lib.LossGradParams
    assert lib.mobi_abi_version() == 6
    assert [lib.mobi_loss_grad_blocks_per_sample(hw) for hw in (0, 1, 256, 257, 4096)] == [0, 1, 1, 2, 16]
    p = _lib.LossGradParams()
    assert lib.mobi_loss_grad(None, None) == -1 and lib.mobi_loss_grad(C.byref(p), None) == -1
    p.eps = p.target = p.t = p.logvar = p.lvlb = p.dy = p.per_sample = p.terms = p.workspace = 4096
    p.batch, p.channels, p.hw, p.table_len, p.c_pad = 2, 4, 64, 1000, 32
    p.dtype = 2
    assert lib.mobi_loss_grad(C.byref(p), None) == -1                     # storage type
    p.dtype, p.channels = 0, 33
    assert lib.mobi_loss_grad(C.byref(p), None) == -2                     # C > c_pad
    p.channels, p.loss_type = 4, 2
    assert lib.mobi_loss_grad(C.byref(p), None) == -2                     # unknown loss type
    p.loss_type, p.c_pad = 1, 12
    assert lib.mobi_loss_grad(C.byref(p), None) == -2                     # 16-byte stores: c_pad % 8
    p.c_pad, p.table_len = 32, 0
    assert lib.mobi_loss_grad(C.byref(p), None) == -1
    p.table_len, p.dy = 1000, 4104
    assert lib.mobi_loss_grad(C.byref(p), None) == -4                     # dy: 16-byte aligned


def test_loss_and_gradients_keeps_its_positional_signature():
    from mobi_amd import train
    params = list(inspect.signature(train.loss_and_gradients).parameters.values())
    positional = [(p.name, p.default) for p in params if p.kind is p.POSITIONAL_OR_KEYWORD]
    assert positional == [("net", inspect.Parameter.empty), ("x_noisy", inspect.Parameter.empty),
                          ("timesteps", inspect.Parameter.empty), ("context", inspect.Parameter.empty),
                          ("target", inspect.Parameter.empty), ("loss_scale", 1.0), ("unscale", True)]
    keyword = {p.name: p.default for p in params if p.kind is p.KEYWORD_ONLY}
    assert keyword == {"loss_type": "l2", "t_weights": None, "l_simple_weight": 1.0, "elbo_weight": 0.0, "return_terms": False}
    back = inspect.signature(train.unet_backward).parameters
    assert list(back)[:3] == ["net", "tape", "deps"] and back["dy"].default is None
