"""The backward kernels of csrc/backward.hip and the convolution data gradients of mobi_amd/train.py ONE BY ONE, at the training
step's shapes and across every launch limit of the file: the 64-block switch of the partials' fold and the 4,096-block cap of
`mobi_backward_partial_blocks`, the grid-stride caps, the MAXV buckets of LayerNorm backward, the routes and tiles of
attention backward, the piece / chunk geometry of the three-pass GroupNorm backward, the workspace sizes the header promises.

Every case asserts three things (tests/backward_ref.py):
  1. whole-tensor rel-L2 against float64 below the family's existing bound (tests/test_gpu_backward.py: TOL1, x 1.5 on the
     matrix-core attention route; 1e-5 / 1e-4 for the fp32 reductions; 1e-6 for AdamW);
  2. the ROW measure (worst row's error / rms row norm; 64-element blocks for fp32 vectors and matrices) at most 2 x what the
     storage restatement of the same operation -- fp32 torch with the kernel's documented rounding points -- shows against the
     same float64 reference, computed on the CPU beside the case;
  3. a second call returns the same bits.
Every restatement value and kernel value goes through MOBI_RECORD_ERRORS (tests/golden_cases.record).
A test collects all its cases' figures before it fails, so one run shows every finding."""
import ctypes as C
import time

import pytest
import torch

from oracle import weights as W
from tests import backward_ref as R
from tests.golden_cases import record
from tests.test_gpu_backward import TOL1
from tests.test_gpu_ops import DT

pytestmark = pytest.mark.gpu
TOL_SUM = 1e-5            # fp32 column sums / weight gradients / d beta (test_transpose_colsum_wgrad)
TOL_DGAMMA = 1e-4         # d gamma / d beta of LayerNorm backward (test_layernorm_backward)
TOL_ADAMW = 1e-6          # test_bbox_embedder_backward_and_adamw


@pytest.fixture(scope="module")
def ops():
    from mobi_amd import ops as o
    return o


def rnd(name, shape, dtype, scale=1.0):
    """deterministic input rounded to the storage type (a CPU tensor of that type)."""
    return (W.synth_input("bwg." + name, shape) * scale).to(dtype)


def tag(dtype):
    return "fp16" if dtype == torch.float16 else "bf16"


class Checker:
    """Collects (case, rel-L2, row measure of the kernel, of the restatement) and fails at the end with every miss."""

    def __init__(self):
        self.bad, self.worst_ratio = [], 0.0

    def check(self, name, got, ref, restated, tol, block=None):
        got = got.detach().cpu()
        e, rk, rr = R.rel_l2(got, ref), R.row_measure(got, ref, block), R.row_measure(restated, ref, block)
        record(name + ".rel", e, tol)
        record(name + ".row.restated", rr)
        record(name + ".row.kernel", rk, 2 * rr)
        ratio = rk / rr if rr > 0 else (0.0 if rk == 0 else float("inf"))
        self.worst_ratio = max(self.worst_ratio, ratio)
        print(f"{name}: rel {e:.3e} (< {tol:.1e})  row kernel {rk:.3e} restated {rr:.3e} ratio {ratio:.2f}", flush=True)
        if not e < tol:
            self.bad.append(f"{name}: rel-L2 {e:.3e} >= {tol:.1e}")
        if not rk <= 2 * rr:
            self.bad.append(f"{name}: row measure {rk:.3e} > 2 x restated {rr:.3e}")

    def equal(self, name, a, b):
        if not torch.equal(a, b):
            self.bad.append(f"{name}: not bit-identical")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def twice(ck, name, fn):
    a, b = fn(), fn()
    for i, (x, y) in enumerate(zip(a, b) if isinstance(a, tuple) else ((a, b),)):
        ck.equal(f"{name}: second call, output {i}", x, y)
    return a


# ----------------------------------------------------------------------------------------------------------------------
# the partials' fold: 64 / 65 blocks, the 4,096-block cap, empty trailing blocks
ROW_CASES = [(1024, 320), (1040, 320), (8192, 320), (8192, 1280), (65536, 320), (65537, 320), (131072, 320)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("rows,c", ROW_CASES)
def test_colsum_and_layernorm_bwd_rows(ops, dtype, rows, c):
    ck = Checker()
    x, dy = rnd(f"rows.x{c}", (rows, c), dtype, 2.0), rnd(f"rows.dy{c}", (rows, c), dtype)
    g = torch.from_numpy(W.synth_param(f"bwg.rows{c}.weight", (c,)))
    name = f"rows{rows}x{c}.{tag(dtype)}"
    got = twice(ck, name, lambda: ops.colsum(dy.cuda()))
    ck.check(name + ".colsum", got, R.colsum_ref(dy), R.colsum_restated(dy), TOL_SUM, block=64)
    dx, dg, db = twice(ck, name, lambda: ops.layernorm_bwd(x.cuda().view(1, rows, c), dy.cuda().view(1, rows, c), g.cuda(), 1e-5))
    rdx, rdg, rdb = R.layernorm_bwd_ref(x, dy, g, 1e-5)
    sdx, sdg, sdb = R.layernorm_bwd_restated(x, dy, g, 1e-5, dtype)
    ck.check(name + ".ln.dx", dx.view(rows, c), rdx, sdx, TOL1[dtype])
    ck.check(name + ".ln.dgamma", dg, rdg, sdg, TOL_DGAMMA, block=64)
    ck.check(name + ".ln.dbeta", db, rdb, sdb, TOL_DGAMMA, block=64)
    ck.done()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("c", [50, 320, 321, 640, 641, 1280, 1281, 1536])
def test_layernorm_bwd_widths(ops, dtype, c):
    """The MAXV buckets' borders and a width that is no multiple of 64; x and dy dense and as channel slices of a wider
    tensor (x_row_stride, dy_row_stride != C); with and without dx_add.  1,000 rows: 63 blocks, the last one of 8 rows."""
    ck = Checker()
    n, t, wide = 2, 500, c + 24
    xw, dyw = rnd(f"w.x{c}", (n, t, wide), dtype, 2.0), rnd(f"w.dy{c}", (n, t, wide), dtype)
    add = rnd(f"w.add{c}", (n, t, c), dtype)
    g = torch.from_numpy(W.synth_param(f"bwg.w{c}.weight", (c,)))
    x, dy = xw[..., 8:8 + c].contiguous(), dyw[..., 16:16 + c].contiguous()
    xd, dyd, xwd, dywd = x.cuda(), dy.cuda(), xw.cuda(), dyw.cuda()
    for with_add in (False, True):
        a = add if with_add else None
        rdx, rdg, rdb = R.layernorm_bwd_ref(x.view(-1, c), dy.view(-1, c), g, 1e-5, dx_add=None if a is None else a.view(-1, c))
        sdx, sdg, sdb = R.layernorm_bwd_restated(x.view(-1, c), dy.view(-1, c), g, 1e-5, dtype, dx_add=None if a is None else a.view(-1, c))
        outs = {}
        for layout in ("dense", "sliced"):
            xs, dys = (xd, dyd) if layout == "dense" else (xwd[..., 8:8 + c], dywd[..., 16:16 + c])
            name = f"lnw{c}.{tag(dtype)}.{layout}.add{int(with_add)}"
            dx, dg, db = twice(ck, name, lambda: ops.layernorm_bwd(xs, dys, g.cuda(), 1e-5, dx_add=None if a is None else a.cuda()))
            ck.check(name + ".dx", dx.view(-1, c), rdx, sdx, TOL1[dtype])
            ck.check(name + ".dgamma", dg, rdg, sdg, TOL_DGAMMA, block=64)
            ck.check(name + ".dbeta", db, rdb, sdb, TOL_DGAMMA, block=64)
            outs[layout] = (dx, dg, db)
        for i in range(3):
            ck.equal(f"lnw{c}: sliced vs dense, output {i}", outs["dense"][i], outs["sliced"][i])
    ck.done()


def test_layernorm_bwd_rejects_1537_channels(ops):
    from mobi_amd import _lib
    x = torch.zeros((1, 16, 1537), device="cuda", dtype=torch.float16)
    with pytest.raises(Exception) as ei:
        ops.layernorm_bwd(x, x, torch.ones(1537, device="cuda"), 1e-5)
    p = _lib.LayerNormBwdParams()
    buf = torch.zeros(1 << 20, device="cuda", dtype=torch.float32)
    p.x = p.dy = p.dx = C.c_void_p(x.data_ptr())
    p.gamma = p.partial = p.dgamma_dbeta = C.c_void_p(buf.data_ptr())
    p.eps, p.rows, p.channels, p.dtype = 1e-5, 16, 1537, 0
    assert _lib.load().mobi_layernorm_bwd(C.byref(p), None) == -2, ei.value      # MOBI_ERR_UNSUPPORTED


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("rows,n,k,strided", [(8192, 320, 320, False), (8192, 1280, 320, False), (8192, 320, 1280, False),
                                              (8200, 320, 320, False), (8192, 320, 320, True), (8200, 320, 320, True)])
def test_linear_wgrad(ops, dtype, rows, n, k, strided):
    ck = Checker()
    dyw, xw = rnd(f"wg.dy{n}", (rows, n + 16), dtype), rnd(f"wg.x{k}", (rows, k + 8), dtype)
    dy, x = dyw[:, 8:8 + n].contiguous(), xw[:, :k].contiguous()
    dyd, xd = (dyw.cuda()[:, 8:8 + n], xw.cuda()[:, :k]) if strided else (dy.cuda(), x.cuda())
    name = f"wgrad{rows}x{n}x{k}.{tag(dtype)}.{'strided' if strided else 'dense'}"
    got = twice(ck, name, lambda: ops.linear_wgrad(dyd, xd))
    ck.check(name, got, R.linear_wgrad_ref(dy, x), R.linear_wgrad_restated(dy, x), TOL_SUM, block=64)
    ck.done()


@pytest.mark.parametrize("dtype", DT)
def test_transpose_and_tile_weights_bit_exact(ops, dtype, monkeypatch):
    for rows, cols in ((8192, 1280), (63, 65), (1, 1)):
        x = rnd(f"tr.{rows}", (rows, cols + 8), dtype).cuda()
        assert torch.equal(ops.transpose(x[:, :cols].contiguous()), x[:, :cols].t())
        assert torch.equal(ops.transpose(x[:, 3:3 + cols]), x[:, 3:3 + cols].t())            # a strided source
    for n, k in ((2560, 10240), (16, 32)):                                                  # 12,800 blocks > the 8,192 cap; one block
        w = rnd(f"tile.{n}", (n, k), dtype).cuda()
        native = ops.tile_weights(w)
        monkeypatch.setattr(ops, "TILE_WEIGHTS_TORCH", True)
        restated = ops.tile_weights(w)
        monkeypatch.setattr(ops, "TILE_WEIGHTS_TORCH", False)
        assert native.shape == restated.shape == (n // 16, k // 32, 16, 4, 8) and torch.equal(native, restated)
        assert torch.equal(native, ops.tile_weights(w))


# ----------------------------------------------------------------------------------------------------------------------
# grid-stride caps
CAP = 65536 * 256


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("rows,inner", [(65535, 256), (65536, 256), (65537, 256), (8192, 1280), (512, 5120)])
def test_geglu_at_the_grid_cap(ops, dtype, rows, inner):
    ck = Checker()
    pre, dh = rnd(f"geglu.pre{inner}", (rows, 2 * inner), dtype, 1.5), rnd(f"geglu.dh{inner}", (rows, inner), dtype)
    name = f"geglu{rows}x{inner}.{tag(dtype)}"
    h = twice(ck, name, lambda: ops.geglu_fwd(pre.cuda()))
    ck.check(name + ".fwd", h, R.geglu_fwd_ref(pre), R.geglu_fwd_restated(pre, dtype), TOL1[dtype])
    d = twice(ck, name, lambda: ops.geglu_bwd(pre.cuda(), dh.cuda()))
    ck.check(name + ".bwd", d, R.geglu_bwd_ref(pre, dh), R.geglu_bwd_restated(pre, dh, dtype), TOL1[dtype])
    ck.done()


@pytest.mark.parametrize("dtype", DT)
def test_add_and_sumpool2_at_the_grid_cap(ops, dtype):
    ck = Checker()
    for n in (CAP - 8, CAP, CAP + 264):
        a, b = rnd("add.a", (n,), dtype), rnd("add.b", (n,), dtype)
        got = twice(ck, f"add{n}", lambda: ops.add(a.cuda(), b.cuda()))
        ck.equal(f"add{n}.{tag(dtype)} vs (a + b) rounded", got.cpu().float(), R.add_restated(a, b, dtype))
    for shape in ((2, 64, 64, 320), (4, 256, 208, 320), (1, 2, 2, 8)):                       # (4, 128, 104, 320) results: 65 K blocks + 1.5 %
        src = rnd(f"pool{shape[1]}", shape, dtype)
        name = f"sumpool2.{'x'.join(map(str, shape))}.{tag(dtype)}"
        got = twice(ck, name, lambda: ops.sumpool2(src.cuda()))
        ck.check(name, got, R.sumpool2_ref(src), R.sumpool2_restated(src, dtype), TOL1[dtype])
    ck.done()


def test_silu_bwd_f32_and_adamw_at_their_caps(ops):
    ck = Checker()
    for n in (4096 * 256 - 1, 4096 * 256, 4096 * 256 + 257):
        z, dy = rnd("silu.z", (n,), torch.float32, 2.0), rnd("silu.dy", (n,), torch.float32)
        got = twice(ck, f"silu{n}", lambda: ops.silu_bwd_f32(z.cuda(), dy.cuda()))
        ck.check(f"silu_bwd_f32.{n}", got, R.silu_bwd_ref(z, dy), R.silu_bwd_restated(z, dy), TOL_SUM, block=64)
    for shape in ((16384 * 256 - 1,), (16384 * 256,), (16384 * 256 + 257,), (1280, 1280)):
        p0 = rnd("adam.p", shape, torch.float32)
        grads = [rnd(f"adam.g{i}", shape, torch.float32) for i in range(3)]

        def run():
            p, m, v = p0.cuda().clone(), torch.zeros(shape, device="cuda"), torch.zeros(shape, device="cuda")
            for i, g in enumerate(grads, 1):
                ops.adamw_step(p, g.cuda(), m, v, i, 3e-3)
            return p, m, v
        p, m, v = twice(ck, f"adamw{shape}", run)
        ck.check(f"adamw.{'x'.join(map(str, shape))}", p, R.adamw_ref(p0, grads, 3e-3)[0], R.adamw_restated(p0, grads, 3e-3)[0],
                 TOL_ADAMW, block=64)
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
# attention backward
def _attn_views(layout, q, k, v, o, do):
    """device views of the five operands in the given layout (the values are the same)."""
    n, tq, c = q.shape
    tk = k.shape[1]
    dev = lambda t: t.cuda()
    if layout == "dense":
        return tuple(dev(t) for t in (q, k, v, o, do))
    if layout == "qkv_thirds":                   # q, k, v as thirds of one [N, T, 3C] buffer (self-attention's fused projection)
        buf = dev(torch.cat([q, k, v], 2))
        return buf[..., :c], buf[..., c:2 * c], buf[..., 2 * c:], dev(o), dev(do)
    if layout == "o_dout_wide":                  # o and dout as slices of a wider buffer
        buf = dev(torch.cat([o, do, o], 2))
        return dev(q), dev(k), dev(v), buf[..., :c], buf[..., c:2 * c]
    if layout == "image_strides":                # every operand a [:, :t] slice of a longer buffer: non-dense image strides
        pad = lambda t: dev(torch.cat([t, t[:, :8]], 1))[:, :t.shape[1]]
        return tuple(pad(t) for t in (q, k, v, o, do))
    if layout == "q_offset_8_bytes":             # q starts 8 bytes into a 16-byte aligned buffer: no 16-byte loads of its rows
        flat = torch.zeros(q.numel() + 8, dtype=q.dtype, device="cuda")
        flat[4:4 + q.numel()] = dev(q).reshape(-1)
        qv = flat[4:4 + q.numel()].view(n, tq, c)
        assert qv.data_ptr() % 16 == 8
        return qv, dev(k), dev(v), dev(o), dev(do)
    raise ValueError(layout)


def _attention_case(ops, ck, dtype, heads, dh, tq, tk, n=1, layout="dense", stored_o=False, vector_budget_s=None):
    """One shape in one layout, force_vector False and True.  Returns the route the host took with force_vector False."""
    c, scale = heads * dh, dh ** -0.5
    q, do = rnd(f"at.q{dh}.{tq}", (n, tq, c), dtype), rnd(f"at.do{dh}.{tq}", (n, tq, c), dtype)
    k, v = rnd(f"at.k{dh}.{tk}", (n, tk, c), dtype), rnd(f"at.v{dh}.{tk}", (n, tk, c), dtype)
    o = R.attention_fwd_ref(q, k, v, heads, scale).to(dtype)
    ref = R.attention_bwd_ref(q, k, v, do, heads, scale)
    views = _attn_views(layout, q, k, v, o, do)
    strides = [s for t in views for s in (t.stride(0), t.stride(1))]
    route = R.attention_bwd_route(dh, strides, [t.data_ptr() for t in views], False)
    restated, outs = {}, {}
    for force in (False, True):
        r = "vector" if force else route
        name = f"attn.h{heads}.dh{dh}.{tq}x{tk}.{layout}{'.stored_o' if stored_o else ''}.{tag(dtype)}.force{int(force)}.{r}"
        t0 = time.time()
        first = ops.attention_bwd(*views, heads, scale, force_vector=force)
        torch.cuda.synchronize()
        took = time.time() - t0
        if force and vector_budget_s is not None and took > vector_budget_s:
            print(f"{name}: the vector passes took {took:.0f} s > {vector_budget_s} s: force_vector=True not checked at this shape")
            record(name + ".skipped_seconds", took)
            continue
        second = ops.attention_bwd(*views, heads, scale, force_vector=force)
        if r not in restated:
            restated[r] = R.attention_bwd_restated(q, k, v, do, heads, scale, dtype, r, o_stored=o if stored_o else None)
        tol = TOL1[dtype] * (1.5 if r == "mfma" else 1.0)
        for got, again, want, rs, nm in zip(first, second, ref, restated[r], ("dq", "dk", "dv")):
            ck.equal(name + f".{nm}: second call", got, again)
            ck.check(name + "." + nm, got, want, rs, tol)
        outs[force] = first
    if len(outs) == 2:                           # the route taken is the route the host's rule gives
        same = all(torch.equal(a, b) for a, b in zip(outs[False], outs[True]))
        if same != (route == "vector"):
            ck.bad.append(f"attn dh{dh} {tq}x{tk} {layout}: expected the {route} route, outputs {'equal' if same else 'differ from'} the vector passes'")
    return route


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dh,tq,tk", [(40, 4096, 4096), (80, 1024, 1024), (160, 256, 256), (160, 64, 64), (40, 4096, 2), (80, 1024, 2)])
def test_attention_bwd_product_shapes(ops, dtype, dh, tq, tk):
    """The UNet's own attention shapes at a 64 x 64 latent, one image, 8 heads; tk = 2: the box adapter's two context tokens.
    At 4096 x 4096 force_vector=True is left out if the vector passes alone take more than a minute (the test says so)."""
    ck = Checker()
    assert _attention_case(ops, ck, dtype, 8, dh, tq, tk, vector_budget_s=60 if tq * tk == 4096 * 4096 else None) == "mfma"
    ck.done()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dh", [40, 64])
@pytest.mark.parametrize("tq", [127, 128, 129, 257])
def test_attention_bwd_tile_edges(ops, dtype, dh, tq):
    """The 128-row launch tile (queries in the dQ pass, keys in the dK | dV pass) and the 32-row staging tile."""
    ck = Checker()
    for tk in (31, 32, 33, 65):
        assert _attention_case(ops, ck, dtype, 2, dh, tq, tk, n=2) == "mfma"
        assert _attention_case(ops, ck, dtype, 2, dh, tk, tq, n=2) == "mfma"       # the same edges on the key side's launch tile
    ck.done()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dh,want", [(8, "mfma"), (24, "mfma"), (48, "mfma"), (72, "mfma"), (96, "vector"), (144, "vector"), (12, "vector")])
def test_attention_bwd_routing(ops, dtype, dh, want):
    """kd = ceil(dh / 16) in {1, 2, 3, 4, 5, 10} and dh % 8 == 0 -> matrix cores, else the vector passes (96 .. 144: kd 6 .. 9)."""
    ck = Checker()
    route = _attention_case(ops, ck, dtype, 4, dh, 130, 70, n=2)
    record(f"route.dh{dh}.{route}", 1.0 if route == "mfma" else 0.0)
    assert route == want
    ck.done()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("layout,want", [("qkv_thirds", "mfma"), ("o_dout_wide", "mfma"), ("image_strides", "mfma"),
                                         ("q_offset_8_bytes", "vector")])
def test_attention_bwd_strided_operands(ops, dtype, layout, want, tune):
    """Row and image strides of wider buffers (mobi_attention_bwd_params' strides, as train.py passes views), and a q pointer
    the matrix-core passes cannot load from: the host must take the vector passes, silently.  `o` is read only by the A/B form
    of the row term (MOBI_ATTN_BWD_EXACT_D=0: D = do . o on the stored output), so its strides are checked in that form too."""
    ck = Checker()
    heads, dh, t = 8, 40, 160
    route = _attention_case(ops, ck, dtype, heads, dh, t, t, n=2, layout=layout)
    record(f"route.{layout}.{route}", 1.0 if route == "mfma" else 0.0)
    assert route == want
    if layout in ("o_dout_wide", "image_strides"):
        tune.setenv("MOBI_ATTN_BWD_EXACT_D", 0)
        _attention_case(ops, ck, dtype, heads, dh, t, t, n=2, layout=layout, stored_o=True)
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
# GroupNorm backward: pieces = C / 8, R = 256 / pieces rows of threads, 256-pixel chunks
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("hw", [1, 257, 1024, 4096])
@pytest.mark.parametrize("c", [320, 640, 1280, 1920, 2048, 2080])
def test_groupnorm_bwd_geometry(ops, dtype, c, hw):
    ck = Checker()
    g = torch.from_numpy(W.synth_param(f"bwg.gn{c}.weight", (c,)))
    b = torch.from_numpy(W.synth_param(f"bwg.gn{c}.bias", (c,)))
    ran = 0
    for images in (1, 3):
        if images * hw * c > 2 * 4096 * 1920:
            continue
        ran += 1
        x, dy = rnd(f"gn.x{c}", (images, hw, c), dtype, 1.5), rnd(f"gn.dy{c}", (images, hw, c), dtype)
        add = rnd(f"gn.add{c}", (images, hw, c), dtype)
        xd, dyd, addd = (t.cuda().view(images, hw, 1, c) for t in (x, dy, add))
        for silu in (False, True):
            base = R._groupnorm_bwd(x, dy, g, b, 1e-5, silu, torch.float64)
            base32 = R._groupnorm_bwd(x, dy, g, b, 1e-5, silu, torch.float32)
            for with_add in (False, True):
                ref = base + add.double() if with_add else base
                restated = R.to_storage(base32 + add.float() if with_add else base32, dtype)
                outs = {}
                for obg in (False, True):
                    name = f"gn.c{c}.hw{hw}.n{images}.silu{int(silu)}.add{int(with_add)}.{'one_block' if obg else 'three_pass'}.{tag(dtype)}"
                    dx = twice(ck, name, lambda: ops.groupnorm_bwd(xd, dyd, g.cuda(), b.cuda(), 1e-5, silu, dx_add=addd if with_add else None,
                                                                   one_block_per_group=obg))
                    ck.check(name, dx.view(images, hw, c), ref, restated, TOL1[dtype])
                    outs[obg] = dx
                if c // 8 > 256:                     # more than 256 pieces: the workspace form falls back to one block per group
                    ck.equal(f"gn.c{c}.hw{hw}: the fallback is the one-block kernel", outs[False], outs[True])
    assert ran
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
# convolution data gradients as mobi_amd/train.py builds them
class _Conv(torch.nn.Module):
    def __init__(self, weight):
        super().__init__()
        self.weight = torch.nn.Parameter(weight)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("form", ["3x3", "1x1", "3x3_stride2", "nearest2_3x3"])
@pytest.mark.parametrize("cout,cin,side", [(320, 320, 64), (640, 320, 32), (1280, 2560, 16)])
def test_conv_data_gradients(ops, dtype, form, cout, cin, side):
    """dx of y = conv(x) (cin -> cout) at the latent size where the UNet has the pair: `side` is x's for 3 x 3 / 1 x 1 / stride 2
    (y at side / 2) and y's for nearest x2 + 3 x 3 (x at side / 2)."""
    import mobi_amd
    from mobi_amd import train
    mobi_amd.set_engine_dtype(dtype)
    ck = Checker()
    kh = 1 if form == "1x1" else 3
    w = rnd(f"conv.{form}.{cout}.{cin}", (cout, cin, kh, kh), dtype, (cin * kh * kh) ** -0.5).float()
    conv = _Conv(w.cuda())
    n = 2
    name = f"dgrad.{form}.{cout}x{cin}.side{side}.{tag(dtype)}"
    if form == "3x3_stride2":
        dy = rnd(f"conv.dy{cout}.{side}", (n, side // 2, side // 2, cout), dtype)

        def run():
            dz = torch.zeros((n, side, side, cout), device="cuda", dtype=dtype)
            dz[:, ::2, ::2] = dy.cuda()
            return ops.igemm(dz, train._conv_dgrad_pack(conv))
        ref, restated = R.conv_dgrad_ref(dy, w, (side, side), stride=2), R.conv_dgrad_restated(dy, w, (side, side), dtype, stride=2)
    elif form == "nearest2_3x3":
        dy = rnd(f"conv.dy{cout}.{side}", (n, side, side, cout), dtype)
        run = lambda: ops.sumpool2(ops.igemm(dy.cuda(), train._conv_dgrad_pack(conv)))
        ref = R.conv_dgrad_ref(dy, w, (side // 2, side // 2), upsample=True)
        restated = R.conv_dgrad_restated(dy, w, (side // 2, side // 2), dtype, upsample=True)
    else:
        dy = rnd(f"conv.dy{cout}.{side}", (n, side, side, cout), dtype)
        run = lambda: ops.igemm(dy.cuda(), train._conv_dgrad_pack(conv))
        ref, restated = R.conv_dgrad_ref(dy, w, (side, side)), R.conv_dgrad_restated(dy, w, (side, side), dtype)
    got = twice(ck, name, run)
    assert got.shape == ref.shape
    ck.check(name, got, ref, restated, TOL1[dtype])
    ck.done()


# ----------------------------------------------------------------------------------------------------------------------
# workspace contracts: every scratch and result buffer a slice of a larger OWNED tensor at exactly the documented size
GUARD = 8192              # elements on either side (an overrun lands in owned memory: detected, nothing faults)


class Guarded:
    def __init__(self, numel, dtype, sentinel, guard=GUARD):
        self.big = torch.full((numel + 2 * guard,), sentinel, device="cuda", dtype=dtype)
        self.t = self.big[guard:guard + numel]
        self.numel, self.guard, self.sentinel = numel, guard, sentinel
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool(torch.all(self.big[:self.guard] == self.sentinel)) and bool(torch.all(self.big[self.guard + self.numel:] == self.sentinel))

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("rows,c", [(1000, 320), (1040, 64), (65537, 320), (131072, 96)])
def test_workspace_contract_colsum_and_layernorm_bwd(ops, dtype, rows, c):
    """partial: f32 [mobi_backward_partial_blocks(rows) + 64][cols] (colsum), [..][2][channels] (LayerNorm backward), as
    include/mobi_engine.h states; x, dy and dx_add are the first `rows` rows of longer owned tensors, dx is guarded too."""
    from mobi_amd import _lib
    lib = _lib.load()
    dt = 0 if dtype == torch.float16 else 1
    nblk = lib.mobi_backward_partial_blocks(rows)
    assert nblk == R.partial_blocks(rows)
    slack = 4352                                                     # rows behind the tensors' end that are still owned memory
    mk = lambda nm, s=1.0: rnd(f"ws.{nm}{c}", (rows + slack, c), dtype, s).cuda()
    x, dy, add = mk("x", 2.0), mk("dy"), mk("add")
    g = torch.from_numpy(W.synth_param(f"bwg.ws{c}.weight", (c,))).cuda()
    want = ops.colsum(dy[:rows])
    part, out = Guarded((nblk + 64) * c, torch.float32, -7.0), Guarded(c, torch.float32, -7.0)
    assert lib.mobi_colsum(C.c_void_p(dy.data_ptr()), c, rows, c, dt, part.ptr, out.ptr, _stream()) == 0
    assert torch.equal(out.t, want)
    assert part.intact() and out.intact()
    wdx, wdg, wdb = ops.layernorm_bwd(x[:rows].view(1, rows, c), dy[:rows].view(1, rows, c), g, 1e-5, dx_add=add[:rows].view(1, rows, c))
    part, dgb = Guarded((nblk + 64) * 2 * c, torch.float32, -7.0), Guarded(2 * c, torch.float32, -7.0)
    dx = Guarded(rows * c, dtype, -7.0, guard=slack * c)              # (as long a tail as the inputs have)
    p = _lib.LayerNormBwdParams()
    p.x, p.dy, p.dx_add = C.c_void_p(x.data_ptr()), C.c_void_p(dy.data_ptr()), C.c_void_p(add.data_ptr())
    p.x_row_stride, p.dy_row_stride, p.gamma, p.eps = c, c, C.c_void_p(g.data_ptr()), 1e-5
    p.dx, p.partial, p.dgamma_dbeta, p.rows, p.channels, p.dtype = dx.ptr, part.ptr, dgb.ptr, rows, c, dt
    assert lib.mobi_layernorm_bwd(C.byref(p), _stream()) == 0
    assert torch.equal(dx.t.view(1, rows, c), wdx) and torch.equal(dgb.t[:c], wdg) and torch.equal(dgb.t[c:], wdb)
    assert part.intact() and dgb.intact() and dx.intact()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("images,hw,c", [(2, 257, 640), (1, 4096, 320), (3, 1, 2048), (2, 1024, 1920)])
def test_workspace_contract_groupnorm_bwd(ops, dtype, images, hw, c):
    """ws: mobi_groupnorm_bwd_workspace_floats(images, hw, channels) floats = images x 32 x 4 statistics + images x
    ceil(hw / 256) x 2 x channels chunk sums."""
    from mobi_amd import _lib
    lib = _lib.load()
    dt = 0 if dtype == torch.float16 else 1
    x, dy = rnd(f"ws.gn.x{c}", (images, hw, 1, c), dtype, 1.5).cuda(), rnd(f"ws.gn.dy{c}", (images, hw, 1, c), dtype).cuda()
    g = torch.from_numpy(W.synth_param(f"bwg.wsgn{c}.weight", (c,))).cuda()
    b = torch.from_numpy(W.synth_param(f"bwg.wsgn{c}.bias", (c,))).cuda()
    want = ops.groupnorm_bwd(x, dy, g, b, 1e-5, True)
    floats = lib.mobi_groupnorm_bwd_workspace_floats(images, hw, c)
    assert floats == images * 32 * 4 + images * ((hw + 255) // 256) * 2 * c
    ws, dx = Guarded(floats, torch.float32, -7.0), Guarded(images * hw * c, dtype, -7.0)
    vp = lambda t: C.c_void_p(t.data_ptr())
    assert lib.mobi_groupnorm_bwd(vp(x), vp(dy), vp(g), vp(b), 1e-5, 1, None, dx.ptr, images, hw, c, dt, ws.ptr, _stream()) == 0
    assert torch.equal(dx.t.view_as(want), want)
    assert ws.intact() and dx.intact()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("force_vector", [False, True], ids=["mfma", "vector"])
@pytest.mark.parametrize("heads,dh,tq,tk", [(8, 40, 129, 33), (2, 160, 65, 200), (8, 80, 1024, 2)])
def test_workspace_contract_attention_bwd(ops, dtype, force_vector, heads, dh, tq, tk):
    """lse, dvec: f32 [image][heads][tq] EACH (two separate buffers here; ops.attention_bwd passes two halves of one tensor);
    dq, dk, dv dense [image][t][heads * dh]."""
    from mobi_amd import _lib
    lib = _lib.load()
    n, c, scale = 2, heads * dh, dh ** -0.5
    q, do = rnd(f"ws.at.q{dh}", (n, tq, c), dtype).cuda(), rnd(f"ws.at.do{dh}", (n, tq, c), dtype).cuda()
    k, v = rnd(f"ws.at.k{dh}", (n, tk, c), dtype).cuda(), rnd(f"ws.at.v{dh}", (n, tk, c), dtype).cuda()
    o = torch.zeros_like(q)
    want = ops.attention_bwd(q, k, v, o, do, heads, scale, force_vector=force_vector)
    lse, dvec = Guarded(n * heads * tq, torch.float32, -7.0), Guarded(n * heads * tq, torch.float32, -7.0)
    dq, dk, dv = Guarded(n * tq * c, dtype, -7.0), Guarded(n * tk * c, dtype, -7.0), Guarded(n * tk * c, dtype, -7.0)
    p = _lib.AttentionBwdParams()
    for nm, t in (("q", q), ("k", k), ("v", v), ("o", o), ("dout", do)):
        setattr(p, nm, C.c_void_p(t.data_ptr()))
        setattr(p, nm + "_img_stride", t.stride(0))
        setattr(p, nm + "_row_stride", t.stride(1))
    p.dq, p.dk, p.dv, p.lse, p.dvec = dq.ptr, dk.ptr, dv.ptr, lse.ptr, dvec.ptr
    p.images, p.heads, p.dh, p.tq, p.tk, p.scale, p.dtype = n, heads, dh, tq, tk, scale, 0 if dtype == torch.float16 else 1
    p.force_vector = int(force_vector)
    assert lib.mobi_attention_bwd(C.byref(p), _stream()) == 0
    for got, w_ in zip((dq, dk, dv), want):
        assert torch.equal(got.t.view_as(w_), w_)
    assert all(t.intact() for t in (lse, dvec, dq, dk, dv))
    assert not torch.any(lse.t == -7.0)                                # every entry of the statistics was written
