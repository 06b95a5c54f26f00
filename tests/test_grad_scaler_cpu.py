"""CPU: `train.GradScaler`, the host-side state machine of dynamic loss scaling (the rules of torch.cuda.amp.GradScaler), and the
multi-tensor entry points' argument checks (validation happens before any launch)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch


def test_state_machine_backoff_growth_and_restart():
    from mobi_amd import train
    s = train.GradScaler(init_scale=1024.0, growth_interval=2, enabled=True)
    assert s.scale == 1024.0
    s.update(True)                                   # overflow: halves, counter reset
    assert s.scale == 512.0 and s.state_dict()["growth_tracker"] == 0
    s.update(False)
    assert s.scale == 512.0 and s.state_dict()["growth_tracker"] == 1
    s.update(False)                                  # two clean steps: doubles
    assert s.scale == 1024.0 and s.state_dict()["growth_tracker"] == 0
    s.update(False)
    s.update(True)                                   # an overflow between two clean steps restarts the count
    assert s.scale == 512.0 and s.state_dict()["growth_tracker"] == 0
    s.update(False)
    assert s.scale == 512.0
    s.update(False)
    assert s.scale == 1024.0
    s = train.GradScaler(init_scale=8.0, growth_factor=4.0, backoff_factor=0.25, growth_interval=1, enabled=True)
    s.update(False)
    assert s.scale == 32.0
    s.update(True)
    assert s.scale == 8.0


def test_state_dict_round_trip():
    from mobi_amd import train
    a = train.GradScaler(init_scale=4096.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=5, enabled=True)
    a.update(False)
    a.update(False)
    sd = a.state_dict()
    assert sd == {"scale": 4096.0, "growth_tracker": 2, "growth_factor": 3.0, "backoff_factor": 0.25, "growth_interval": 5}
    b = train.GradScaler(init_scale=1.0, enabled=True)
    b.load_state_dict(sd)
    assert b.state_dict() == sd and b.scale == 4096.0
    for _ in range(3):
        a.update(False)
        b.update(False)
    assert a.scale == b.scale == 3.0 * 4096.0 and a.state_dict() == b.state_dict()


def test_disabled_scale_is_one_and_never_moves():
    import mobi_amd
    from mobi_amd import train
    s = train.GradScaler(init_scale=1024.0, growth_interval=1, enabled=False)
    for found in (False, True, False, False):
        s.update(found)
        assert s.scale == 1.0
    assert s.first_use(1 << 16) == 1.0
    before = mobi_amd.engine_dtype()
    try:                                              # enabled=None follows the storage type: fp16 on, bf16 off
        mobi_amd.set_engine_dtype(torch.bfloat16)
        assert not train.GradScaler().enabled and train.GradScaler().scale == 1.0
        mobi_amd.set_engine_dtype(torch.float16)
        assert train.GradScaler().enabled
    finally:
        mobi_amd.set_engine_dtype(before)


@pytest.mark.parametrize("numel", [4 * 4 * 16 * 16, 8 * 4 * 64 * 64])
def test_default_init_scale_is_the_training_steps_rule(numel):
    """init_scale=None: 2 ** round(log2(max(4, numel) / 4)) of the first step's output, the static rule of `training_step`."""
    from mobi_amd import train
    s = train.GradScaler(init_scale=None, enabled=True)
    with pytest.raises(RuntimeError):
        s.scale                                       # not known before the first use
    want = 2.0 ** round(math.log2(max(4, numel) / 4))
    assert s.first_use(numel) == want == s.scale == train.static_loss_scale(numel)
    assert s.first_use(16 * numel) == want            # fixed at FIRST use
    assert train.static_loss_scale(1) == 1.0


def test_multi_tensor_entry_points_validate_on_the_host():
    from mobi_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    c = C.c_int32(0)
    ws = lib.mobi_multi_tensor_workspace_bytes(C.byref(c))
    assert c.value > 0 and c.value % 4 == 0 and ws > 0 and ws % 8 == 0
    assert lib.mobi_multi_tensor_workspace_bytes(None) == ws
    assert lib.mobi_grad_stats(None, 1, 16, 1, 16, 16, None) == -1
    assert lib.mobi_grad_stats(16, 0, 16, 1, 16, 16, None) == -1
    assert lib.mobi_grad_stats(16, 1, 16, 1, 20, 16, None) == -4          # fp64 partials: 8-byte alignment
    assert lib.mobi_adamw_multi(16, 1, None, 1, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1, None) == -1
    assert lib.mobi_adamw_multi(16, 1, 16, 1, 1.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0, None) == -1      # steps count from 1
    assert C.sizeof(_lib.MtTensor) == 40 and C.sizeof(_lib.MtChunk) == 16 and C.sizeof(_lib.GradStatsRecord) == 16


def test_table_rows_match_the_structs_field_by_field():
    """`ops.multi_tensor_rows` builds what the kernels read as `mobi_mt_tensor` / `mobi_mt_pair`: the bytes of a row equal the
    bytes of the ctypes struct filled, field by field, with the same distinct values (size AND field order)."""
    from mobi_amd import _lib, ops
    for cls in (_lib.MtTensor, _lib.MtPair):
        fields = [name for name, _ in cls._fields_]
        assert fields[-1] == "n"
        structs, columns, numels = [], [[] for _ in fields[:-1]], []
        for row in range(3):
            s = cls()
            for col, name in enumerate(fields[:-1]):
                value = 0x1000 * (row + 1) + 0x10 * (col + 1)             # distinct per row and per field
                setattr(s, name, value)
                columns[col].append(value)
            s.n = 7 + row
            numels.append(7 + row)
            structs.append(bytes(s))
        rows = ops.multi_tensor_rows(columns, numels)
        assert rows.dtype == np.int64 and rows.shape == (3, len(fields)) and rows.flags["C_CONTIGUOUS"]
        assert rows.tobytes() == b"".join(structs), cls.__name__
        live = ops.multi_tensor_rows([ops.LIVE] + columns[1:], numels)   # a live column: zeros until it is set, the rest in place
        assert (live[:, 0] == 0).all() and (live[:, 1:] == rows[:, 1:]).all()
