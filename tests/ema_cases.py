"""The small module and the random draws shared by tests/golden/make_golden_ema.py (which ran the reference's LitEma on them)
and the EMA tests (which run the engine's): parameters of 1, 3, 5, 255, 8191, 8192, 8193 and 20 001 elements -- single
elements, fewer than one 16-byte access, the multi-tensor chunk length and its neighbours, more than two chunks -- under nested
names, plus one frozen parameter, which gets no shadow."""
import numpy as np
import torch
from torch import nn

UPDATES = 12
DECAYS = {"d9999": (0.9999, 20261), "d5": (0.5, 20262)}          # tag -> (decay, seed)


class Leaf(nn.Module):
    def __init__(self, **shapes):
        super().__init__()
        for name, shape in shapes.items():
            setattr(self, name, nn.Parameter(torch.zeros(shape)))


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.gain = nn.Parameter(torch.zeros(1))
        self.stem = Leaf(bias=(3,), scale=(5,))
        self.blocks = nn.ModuleList([Leaf(weight=(15, 17)), Leaf(weight=(8191,)), Leaf(weight=(64, 128)), Leaf(weight=(8193,))])
        self.out = Leaf(weight=(20001,), frozen=(7,))
        self.out.frozen.requires_grad_(False)


SIZES = [1, 3, 5, 255, 8191, 8192, 8193, 20001]                  # the trainable parameters, in named_parameters() order


def draws(seed):
    """-> (initial values of EVERY parameter in named_parameters() order, [per update: new values of the trainable ones])"""
    rng = np.random.default_rng(seed)
    net = Net()
    init = [rng.standard_normal(p.numel(), dtype=np.float32) for p in net.parameters()]
    steps = [[rng.standard_normal(n, dtype=np.float32) for n in SIZES] for _ in range(UPDATES)]
    return init, steps


def fill_(net, values, trainable_only=False):
    ps = [p for p in net.parameters() if p.requires_grad or not trainable_only]
    assert len(ps) == len(values)
    with torch.no_grad():
        for p, v in zip(ps, values):
            p.copy_(torch.from_numpy(v).reshape(p.shape))
