#!/usr/bin/env python3
"""tests/golden/ema.npz: the REFERENCE's `LitEma` (its `ldm/modules/ema.py`, torch only: imported as it lies, nothing
copied) on the CPU over the small module of tests/ema_cases.py: 12 updates with fresh parameter values before each, for
decay 0.9999 (the warm-up (1 + n) / (10 + n) is the minimum throughout) and decay 0.5 (the cap takes over at n = 8).  Stored:
the seeds, the buffer names, `num_updates`, the fp32 1 - decay_t of every update (the reference's own tensor expression on its
own buffers) and the final shadows.  The tests regenerate the inputs from the seeds.   python tests/golden/make_golden_ema.py"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MOBI_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import ema_cases as E  # noqa: E402


def main():
    spec = importlib.util.spec_from_file_location("ref_ema", os.path.join(REF, "ldm", "modules", "ema.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for tag, (decay, seed) in E.DECAYS.items():
        init, steps = E.draws(seed)
        net = E.Net()
        E.fill_(net, init)
        ema = mod.LitEma(net, decay=decay)
        names = [k for k, _ in ema.named_buffers()]
        omd = []
        for vals in steps:
            E.fill_(net, vals, trainable_only=True)
            n = ema.num_updates + 1
            omd.append((1.0 - min(ema.decay, (1 + n) / (10 + n))).numpy().copy())
            assert omd[-1].dtype == np.float32
            ema(net)
        out[f"{tag}_seed"] = np.asarray(seed, dtype=np.int64)
        out[f"{tag}_decay"] = ema.decay.numpy().copy()
        out[f"{tag}_num_updates"] = ema.num_updates.numpy().copy()
        out[f"{tag}_one_minus_decay"] = np.asarray(omd, dtype=np.float32)
        for k, v in ema.named_buffers():
            if k not in ("decay", "num_updates"):
                out[f"{tag}_shadow_{k}"] = v.numpy().reshape(-1).copy()
        out["buffer_names"] = np.asarray(names)
        out["frozen_untouched"] = np.asarray(bool(torch.equal(net.out.frozen.reshape(-1), torch.from_numpy(init[-1]))))
    path = os.path.join(HERE, "ema.npz")
    np.savez(path, **out)
    print("wrote ema.npz:", os.path.getsize(path), "bytes;", list(out["buffer_names"]), out["d5_one_minus_decay"])


if __name__ == "__main__":
    main()
