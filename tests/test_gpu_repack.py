"""GPU: `mobi_repack_multi` -- the 16-bit images of every listed fp32 master in ONE launch -- and `ops.RepackTable`.

Every comparison is exact: the launch rounds once, as torch's `.to()` does, and otherwise moves data.  The expected images are
what the lazy path builds tensor by tensor: `ops.pack_linear(src, ...)` (`.w`, `.wt`) and `ops.pack_linear(src.t().contiguous(),
...)` (the transposed pair), with `mobi_tile_weights` and with its torch restatement (`ops.TILE_WEIGHTS_TORCH`).

Shapes [n, k]: 16 x 32 one 1-KiB block and no tiled transposed image; 48 x 96 partial tiles both ways; 32 x 48 k % 32 != 0 (no
`wt`); 80 x 32 n % 32 != 0 (no `wt_t`); 320 x 768 and 1280 x 320 production shapes; 64 x 64 exactly one tile; 128 x 192.  All of
them, plus 30 x 21 with both directions (no 16-byte path applies: element-wise reads and writes) and one cast-only entry
(10 x 20: 16-byte reads, element-wise writes), sit in ONE table whose tile map is shuffled by a seeded
permutation; `GUARD` sentinel elements lie in front of, between and behind the images."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(16, 32), (48, 96), (32, 48), (80, 32), (320, 768), (1280, 320), (64, 64), (128, 192)]
ODD = (30, 21)
CAST_ONLY = (10, 20)
GUARD = 64
SENTINEL = 0x7b5a           # a 16-bit pattern no rounded value below takes by chance at every guard position
DTYPES = [torch.float16, torch.bfloat16]

# fp16: 65504 max, 65519.9 rounds down to it, 65520 (the tie) and 1e5 overflow to inf; 2^-24 x {0.5 (a tie: to even = 0), 0.50001
# (up to the smallest subnormal), 1.5 (a tie between subnormals 1 and 2: to even = 2)}; -0; bf16 ties 1 + 2^-8 (down, to even) and
# 1 + 3 2^-8 (up, to even); +-inf
SPECIAL = [65504.0, 65519.9, 65520.0, 1e5, -65520.0, 2.0 ** -24 * 0.5, 2.0 ** -24 * 0.50001, 2.0 ** -24 * 1.5, -0.0,
           1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, float("inf"), float("-inf")]


@pytest.fixture(scope="module")
def ops():
    from mobi_amd import ops as o
    return o


@pytest.fixture(scope="module")
def masters():
    """The fp32 masters (device) of SHAPES + ODD + CAST_ONLY; the rounding values are seeded into the first elements of every one."""
    g = torch.Generator().manual_seed(20)
    out = []
    for n, k in SHAPES + [ODD, CAST_ONLY]:
        t = torch.randn((n, k), generator=g) * 0.05
        t.view(-1)[:len(SPECIAL)] = torch.tensor(SPECIAL)
        t.view(-1)[-len(SPECIAL):] = torch.tensor(SPECIAL)
        out.append(t.cuda())
    return out


def _bits(t):
    return t.detach().contiguous().view(torch.int16).cpu()


def _items(masters):
    return [(m, True, True) for m in masters[:-1]] + [(masters[-1], "cast", False)]


def _table(ops, masters, dtype, seed=7):
    shapes = [tuple(m.shape) for m in masters]
    tmap = ops.repack_tile_map(shapes)
    tmap = tmap[np.random.default_rng(seed).permutation(len(tmap))].copy()
    table = ops.RepackTable(_items(masters), dtype, guard=GUARD, tile_map=tmap)
    table.buffer.view(torch.int16).fill_(SENTINEL)
    return table


@pytest.fixture(scope="module")
def launched(ops, masters):
    """{dtype: (table after one launch, the masters' bits before it)}: one launch per dtype, shared by the tests below."""
    out = {}
    for dtype in DTYPES:
        before = [m.clone() for m in masters]
        table = _table(ops, masters, dtype)
        ops.repack_multi(table)
        torch.cuda.synchronize()
        out[dtype] = (table, before)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
@pytest.mark.parametrize("torch_tiles", [False, True], ids=["tile_kernel", "tile_torch"])
def test_images_equal_the_lazy_path(ops, masters, launched, dtype, torch_tiles, monkeypatch):
    monkeypatch.setattr(ops, "TILE_WEIGHTS_TORCH", torch_tiles)
    table, _ = launched[dtype]
    for i, (m, (n, k)) in enumerate(zip(masters[:-1], SHAPES)):
        fwd = ops.pack_linear(m, None, dtype, m.device)
        tr = ops.pack_linear(m.t().contiguous(), None, dtype, m.device)
        im = table.images[i]
        assert torch.equal(_bits(im["w"]), _bits(fwd.w)), (n, k)
        assert torch.equal(_bits(im["w_t"]), _bits(tr.w)), (n, k)
        assert torch.equal(_bits(im["w"]), _bits(m.to(dtype))), (n, k)
        for got, want, tiled in ((im["wt"], fwd.wt, n % 16 == 0 and k % 32 == 0), (im["wt_t"], tr.wt, k % 16 == 0 and n % 32 == 0)):
            assert (got is not None) == tiled == (want is not None), (n, k)      # NULL exactly where tile_weights gives None
            if tiled:
                assert got.shape == want.shape and torch.equal(_bits(got), _bits(want)), (n, k)
    odd, m = table.images[-2], masters[-2]
    assert odd["wt"] is None and odd["wt_t"] is None
    assert torch.equal(_bits(odd["w"]), _bits(m.to(dtype))) and torch.equal(_bits(odd["w_t"]), _bits(m.t().contiguous().to(dtype)))
    cast = table.images[-1]
    assert cast["wt"] is None and cast["w_t"] is None and cast["wt_t"] is None
    assert torch.equal(_bits(cast["w"]), _bits(masters[-1].to(dtype)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_null_entries_where_no_tiled_image(ops, launched, dtype):
    table, _ = launched[dtype]
    rows = table.entries.cpu().numpy().view(np.dtype([("src", "<u8"), ("w", "<u8"), ("wt", "<u8"), ("w_t", "<u8"), ("wt_t", "<u8"),
                                                      ("n", "<i4"), ("k", "<i4")]))
    for row, (n, k) in zip(rows, SHAPES):
        assert (row["n"], row["k"]) == (n, k) and row["w"] and row["w_t"]
        assert bool(row["wt"]) == (n % 16 == 0 and k % 32 == 0)
        assert bool(row["wt_t"]) == (k % 16 == 0 and n % 32 == 0)
        assert all(int(row[f]) % 16 == 0 for f in ("w", "wt", "w_t", "wt_t"))
    assert not rows[-1]["wt"] and not rows[-1]["w_t"] and not rows[-1]["wt_t"] and rows[-1]["w"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_rounding_values(launched, masters, dtype):
    table, _ = launched[dtype]
    got = table.images[0]["w"].reshape(-1)[:len(SPECIAL)].cpu()
    want = torch.tensor(SPECIAL).to(dtype)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    if dtype == torch.float16:
        f = got.float()
        assert f[0] == 65504 and f[1] == 65504 and torch.isinf(f[2]) and torch.isinf(f[3]) and f[4] == float("-inf")
        assert f[5] == 0 and f[6] == 2.0 ** -24 and f[7] == 2.0 ** -23
    else:
        assert got[9].float() == 1.0 and got[10].float() == 1.0 + 2.0 ** -6
    assert got[8].view(torch.int16).item() == -0x8000                          # -0 keeps its sign
    # the same values at the far end of the cast-only entry, which no 16-byte path serves
    tail = table.images[-1]["w"].reshape(-1)[-len(SPECIAL):].cpu()
    assert torch.equal(tail.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp16", "bf16"])
def test_guards_and_sources_untouched(launched, masters, dtype):
    table, before = launched[dtype]
    inside = torch.zeros(table.buffer.numel(), dtype=torch.bool)
    for a, b in table.spans:
        assert a % 8 == 0 and not inside[a:b].any()                            # 16-byte boundaries, no overlap
        inside[a:b] = True
    flat = table.buffer.view(torch.int16).cpu()
    assert int((~inside).sum()) >= GUARD * (len(table.spans) + 1)
    assert bool((flat[~inside] == SENTINEL).all())
    for m, b in zip(masters, before):
        assert torch.equal(m.view(torch.int32).cpu(), b.view(torch.int32).cpu())


def test_tiles_outside_their_tensor_write_nothing(ops, masters):
    shapes = [tuple(m.shape) for m in masters]
    good = ops.repack_tile_map(shapes)
    bad = good.copy()
    for i, (n, k) in enumerate(shapes):                                         # every index past the tensor's last tile, or negative
        sel = bad["tensor"] == i
        tiles = ((n + 63) // 64) * ((k + 63) // 64)
        bad["offset"][sel] = np.where(np.arange(sel.sum()) % 2 == 0, tiles + np.arange(sel.sum()), -1 - np.arange(sel.sum()))
    bad["tensor"][::5] = np.where(np.arange(len(bad[::5])) % 2 == 0, len(shapes), -1)      # and entries past the table
    table = ops.RepackTable(_items(masters), torch.float16, guard=GUARD, tile_map=bad)
    table.buffer.view(torch.int16).fill_(SENTINEL)
    ops.repack_multi(table)
    torch.cuda.synchronize()
    assert bool((table.buffer.view(torch.int16) == SENTINEL).all())


def test_argument_errors(ops, masters):
    from mobi_amd import _lib
    lib = _lib.load()
    table = ops.RepackTable(_items(masters), torch.float16)
    e, t = C.c_void_p(table.entries.data_ptr()), C.c_void_p(table.tiles.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = _lib.load().mobi_error_string(-1)
    assert bad == b"invalid argument"
    assert lib.mobi_repack_multi(None, table.count, t, table.n_tiles, _lib.MOBI_F16, st) == -1
    assert lib.mobi_repack_multi(e, table.count, None, table.n_tiles, _lib.MOBI_F16, st) == -1
    assert lib.mobi_repack_multi(e, 0, t, table.n_tiles, _lib.MOBI_F16, st) == -1
    assert lib.mobi_repack_multi(e, table.count, t, 0, _lib.MOBI_F16, st) == -1
    assert lib.mobi_repack_multi(e, table.count, t, table.n_tiles, 2, st) == -1
    with pytest.raises(_lib.EngineError):
        _lib.check(lib.mobi_repack_multi(e, table.count, t, table.n_tiles, -1, st), "mobi_repack_multi")
    torch.cuda.synchronize()


def test_table_refuses_bad_sources(ops, masters):
    m = masters[4]
    with pytest.raises(ValueError):
        ops.RepackTable([(m.half(), True, True)], torch.float16)
    with pytest.raises(ValueError):
        ops.RepackTable([(m.t(), True, True)], torch.float16)                  # not dense
    with pytest.raises(ValueError):
        ops.RepackTable([(m[:, ::2], True, True)], torch.float16)
    with pytest.raises(ValueError):
        ops.RepackTable([(m, True, True), (m.cpu(), True, True)], torch.float16)          # another device
    with pytest.raises(ValueError):
        ops.RepackTable([(m.cpu(), True, True)], torch.float16)
    table = ops.RepackTable([(m, True, True)], torch.bfloat16)
    assert table.ptrs == (m.data_ptr(),)
