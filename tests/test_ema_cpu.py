"""CPU: the host side of the EMA shadow weights (`mobi_amd/ldm/modules/ema.py` LitEma, `LatentDiffusion(use_ema=True)`) against
what the reference's LitEma recorded (tests/golden/ema.npz, tests/golden/make_golden_ema.py).  Nothing here launches: the
update itself is tests/test_gpu_ema.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ema_cases as E
from tests.golden_cases import load


@pytest.fixture(scope="module")
def golden():
    return load("ema")


def _ema(decay, seed, **kw):
    from mobi_amd.ldm.modules.ema import LitEma
    net = E.Net()
    E.fill_(net, E.draws(seed)[0])
    return net, LitEma(net, decay=decay, **kw)


def test_buffers_are_the_references(golden):
    net, ema = _ema(*E.DECAYS["d9999"])
    names = [k for k, _ in ema.named_buffers()]
    assert names == [str(k) for k in golden["buffer_names"]]
    assert "outfrozen" not in names and "out.frozen" not in ema.m_name2s_name         # the frozen parameter has no shadow
    assert ema.m_name2s_name == {k: k.replace(".", "") for k, p in net.named_parameters() if p.requires_grad}
    assert ema.decay.dtype == torch.float32 and ema.decay.shape == () and ema.num_updates.dtype == torch.int32
    assert torch.equal(ema.decay, golden["d9999_decay"]) and int(ema.num_updates) == 0
    for k, p in net.named_parameters():
        if p.requires_grad:
            s = getattr(ema, ema.m_name2s_name[k])
            assert torch.equal(s, p) and s.data_ptr() != p.data_ptr() and not s.requires_grad


@pytest.mark.parametrize("tag", list(E.DECAYS))
def test_decay_sequence_in_fp32_equals_the_references(golden, tag):
    _, ema = _ema(*E.DECAYS[tag])
    got = [ema.advance() for _ in range(E.UPDATES)]
    assert all(type(x) is np.float32 for x in got)
    want = golden[f"{tag}_one_minus_decay"].numpy()
    assert want.dtype == np.float32 and np.array_equal(np.asarray(got).view(np.int32), want.view(np.int32)), (got, want)
    assert int(ema.num_updates) == int(golden[f"{tag}_num_updates"]) == E.UPDATES
    if tag == "d5":                                   # the cap takes over at n = 8: (1 + 8) / (10 + 8) = 0.5
        assert got[6] > 0.5 and all(x == 0.5 for x in got[7:])
    else:                                             # the warm-up is the minimum throughout
        assert all(a > b for a, b in zip(got, got[1:])) and got[-1] > 1e-4 * 1.01


def test_without_update_counting_the_decay_is_constant():
    _, ema = _ema(0.9999, 1, use_num_upates=False)
    assert int(ema.num_updates) == -1
    got = [ema.advance() for _ in range(3)]
    assert int(ema.num_updates) == -1
    assert got[0] == got[1] == got[2] == np.float32(1.0) - np.float32(0.9999)


@pytest.mark.parametrize("decay", [-0.01, 1.01])
def test_decay_outside_the_unit_interval_raises(decay):
    from mobi_amd.ldm.modules.ema import LitEma
    with pytest.raises(ValueError):
        LitEma(E.Net(), decay=decay)
    LitEma(E.Net(), decay=0.0), LitEma(E.Net(), decay=1.0)


def test_state_dict_round_trip():
    _, ema = _ema(0.5, 3)
    for _ in range(9):
        ema.advance()
    with torch.no_grad():
        ema.blocks1weight.mul_(3.0)
    sd = {k: v.clone() for k, v in ema.state_dict().items()}
    assert list(sd) == [k for k, _ in ema.named_buffers()]
    _, other = _ema(0.9999, 4)
    assert other.advance() == np.float32(1.0) - np.float32(2.0) / np.float32(11.0)    # (its host mirror is in use before the load)
    other.load_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())
    assert int(other.num_updates) == 9
    assert other.advance() == ema.advance() == 0.5 and int(other.num_updates) == 10   # decay and count came with the checkpoint


def test_store_copy_to_restore():
    net, ema = _ema(0.5, 5)
    init, steps = E.draws(5)
    E.fill_(net, steps[0], trainable_only=True)
    live = [p.detach().clone() for p in net.parameters()]
    ema.store(net.parameters())
    ema.copy_to(net)
    for (k, p), v in zip(net.named_parameters(), init):
        assert torch.equal(p.reshape(-1), torch.from_numpy(v)), k                       # the shadows are the initial values
    ema.restore(net.parameters())
    assert all(torch.equal(p, w) for p, w in zip(net.parameters(), live))


def test_argument_errors_return_before_any_launch():
    from mobi_amd import _lib
    lib = _lib.load()
    assert lib.mobi_struct_size(26) == C.sizeof(_lib.MtPair) == 24 and _lib.STRUCT_IDS[26] is _lib.MtPair
    assert lib.mobi_ema_multi(None, 1, 16, 1, 0.5, _lib.MT_EMA, None) == -1
    assert lib.mobi_ema_multi(16, 1, None, 1, 0.5, _lib.MT_EMA, None) == -1
    assert lib.mobi_ema_multi(16, 0, 16, 1, 0.5, _lib.MT_EMA, None) == -1
    assert lib.mobi_ema_multi(16, 1, 16, 0, 0.5, _lib.MT_SWAP, None) == -1
    assert lib.mobi_ema_multi(16, 1, 16, 1, 0.5, 2, None) == -1 and lib.mobi_ema_multi(16, 1, 16, 1, 0.5, -1, None) == -1


def _latent_diffusion(use_ema):
    """The model tests/test_dropin_cpu.py builds through the config flow, narrowed the same way (plain dicts: no omegaconf)."""
    import os
    from mobi_amd.ldm.util import instantiate_from_config, load_config
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, "configs", "mobi_nusc_256.yaml"),
                      ["ref_mode=id-ref", "use_lidar=True", "latent_size=8", "image_height=64",
                       "model.params.lidar_stage_config.params.ckpt_path=null",
                       "model.params.unet_config.params.model_channels=32",
                       "model.params.first_stage_config.params.ddconfig.ch=32",
                       "model.params.lidar_stage_config.params.ddconfig.ch=32",
                       "model.params.cond_stage_config=__is_unconditional__",
                       f"model.params.use_ema={use_ema}"])
    return instantiate_from_config(cfg["model"])


def test_latent_diffusion_keeps_shadows_of_exactly_its_trainable_unet_parameters(capsys):
    model = _latent_diffusion(True)
    assert model.use_ema is True
    want = {"model_ema." + k.replace(".", ""): p for k, p in model.model.named_parameters() if p.requires_grad}
    assert len(want) > 400
    assert f"Keeping EMAs of {len(want) + 2}." in capsys.readouterr().out
    sd = model.state_dict()
    got = [k for k in sd if k.startswith("model_ema.")]
    assert set(got) == set(want) | {"model_ema.decay", "model_ema.num_updates"} and len(got) == len(set(got))
    for k, p in want.items():
        assert sd[k].dtype == torch.float32 and torch.equal(sd[k], p), k
    # a checkpoint with model_ema.* keys loads key for key: nothing missing, nothing unexpected
    other = _latent_diffusion(True)
    missing, unexpected = other.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items() if k.startswith("model_ema."))
    # without use_ema: no shadows, and the hooks are no-ops (nothing to launch, so this runs without a device)
    capsys.readouterr()
    plain = _latent_diffusion(False)
    assert not any(k.startswith("model_ema") for k in plain.state_dict())
    plain.on_train_batch_end()
    with plain.ema_scope("x"):
        pass
    assert "EMA" not in capsys.readouterr().out
