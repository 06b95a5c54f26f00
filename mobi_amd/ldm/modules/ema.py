"""EMA shadow weights (`use_ema`): the reference's `LitEma` interface (ldm/modules/ema.py) on the engine.

One fp32 shadow per `requires_grad` parameter of the wrapped model, kept as a buffer named by the parameter's name without
its dots (so `state_dict()` has the reference's `model_ema.*` keys), plus `decay` and `num_updates`.  An update is ONE
launch over all shadows (`ops.ema_multi` -> `mobi_ema_multi`) instead of three elementwise launches per tensor; `swap`
exchanges parameters and shadows in one launch (`LatentDiffusion.ema_scope`)."""
import numpy as np
import torch
from torch import nn

from ... import ops
from .diffusionmodules.util import weights_changed


class LitEma(nn.Module):
    def __init__(self, model, decay=0.9999, use_num_upates=True):
        super().__init__()
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        self.m_name2s_name = {}
        self.register_buffer("decay", torch.tensor(decay, dtype=torch.float32))
        self.register_buffer("num_updates", torch.tensor(0 if use_num_upates else -1, dtype=torch.int))
        for name, p in model.named_parameters():
            if p.requires_grad:
                s_name = name.replace(".", "")                    # (a buffer's name may not contain a dot)
                self.m_name2s_name[name] = s_name
                self.register_buffer(s_name, p.detach().clone())
        self.collected_params = []
        self._host = None               # (decay: np.float32, num_updates: int) as the buffers hold them, read once
        self._pairs = None              # ops.MultiTensorTable over (parameter, shadow), built at the first launch
        self.swapped = False            # True between the two swaps of an `ema_scope`: the buffers then hold the live weights

    def _load_from_state_dict(self, *args, **kwargs):
        self._host = None               # a checkpoint brings its own decay and update count
        return super()._load_from_state_dict(*args, **kwargs)

    def advance(self):
        """The host side of one update, nothing launched on the engine: counts the update (when counting is on) and returns
        this update's 1 - decay_t, decay_t = min(decay, (1 + n) / (10 + n)), in fp32 arithmetic throughout -- the values the
        reference's tensor expressions take (n is far below 2^24: its conversion to fp32 is exact).  `decay` and `num_updates`
        are read from their buffers once and mirrored on the host afterwards (no read-back per step); code that writes the
        buffers directly, other than `load_state_dict`, sets `self._host = None`."""
        if self._host is None:
            self._host = (np.float32(self.decay.item()), int(self.num_updates.item()))
        decay, n = self._host
        if n >= 0:
            n += 1
            self.num_updates += 1
            self._host = (decay, n)
            decay = min(decay, np.float32(1 + n) / np.float32(10 + n))
        return np.float32(1.0) - decay

    def _table(self, model):
        """The (parameter, shadow) table of `model`, rebuilt when a tensor of either side has moved."""
        m_param = dict(model.named_parameters())
        params, shadows = [], []
        for key, p in m_param.items():
            if p.requires_grad:
                params.append(p.data)
                shadows.append(self._buffers[self.m_name2s_name[key]])
            else:
                assert key not in self.m_name2s_name
        ptrs = tuple((p.data_ptr(), s.data_ptr()) for p, s in zip(params, shadows))
        if self._pairs is None or self._pairs.ptrs != ptrs:
            self._pairs = ops.MultiTensorTable([params, shadows])
        return self._pairs, [p for p in m_param.values() if p.requires_grad]

    @torch.no_grad()
    def forward(self, model):
        """shadow <- shadow - (1 - decay_t) (shadow - param) for every shadow, one launch.  Writes shadows only: no parameter
        version and no weights epoch moves."""
        ops.ema_multi(self._table(model)[0], self.advance())

    @torch.no_grad()
    def swap(self, model):
        """Exchange every parameter with its shadow, one launch, no copy of either.  The parameters change under the packed
        16-bit copies and captured step graphs that are keyed on them: every swapped parameter's version and the weights
        epoch are bumped, as `train.AdamW.step` does.  Every call toggles `swapped`, not only `ema_scope`'s two: after a single
        swap made on purpose the buffers hold the live weights, and `checkpoint.Checkpointer.save` refuses until a second
        swap puts them back."""
        pairs, params = self._table(model)
        ops.swap_multi(pairs)
        self.swapped = not self.swapped
        weights_changed(params)

    @torch.no_grad()
    def copy_to(self, model):
        for key, p in model.named_parameters():
            if p.requires_grad:
                p.copy_(self._buffers[self.m_name2s_name[key]])
            else:
                assert key not in self.m_name2s_name
        weights_changed()                               # (`copy_` has bumped the versions)

    def store(self, parameters):
        """Keep a copy of `parameters` (an iterable of `nn.Parameter`) for `restore`."""
        self.collected_params = [param.clone() for param in parameters]

    @torch.no_grad()
    def restore(self, parameters):
        """Write what `store` kept back into `parameters`."""
        for c_param, param in zip(self.collected_params, parameters):
            param.copy_(c_param)
        weights_changed()                               # (`copy_` has bumped the versions)
