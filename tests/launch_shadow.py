"""Launch shadow (TEST INFRASTRUCTURE, not a conftest): every launch of a UNet forward or a VAE encode / decode checked on its
own against a float64 restatement of its entry point's contract (include/mobi_engine.h, the docstrings of mobi_amd/ops.py).

`LaunchShadow(monkeypatch)` wraps the `mobi_amd.ops` entry points the model files call as `ops.<name>(...)`: igemm (and with it
`linear`, which calls the module's igemm), Deferred.finish, groupnorm, layernorm, attention, ctx_attention, ff_geglu,
two_key_adapter, row_chain (with chain_adapter_image and groupnorm_scale_shift) and the VAEs' softmax_rows, split_f32,
trunk_add, lincomb4, conv_small_cout, conv_small_cin and pack_sources.
A row_chain launch is judged per stored tensor against tests/chain_ref.py, the fp64 interpreter of mobi_row_chain_params'
contract: while a shadow runs, `ops.ChainProgram` is the recording subclass, so every program arrives with the plain description
of what it was asked to build; the adapter's fp32 tables are found by the CONTENT of the image the launch was given (the
transformer block copies the image into a persistent buffer) among the clones kept per chain_adapter_image call -- no match is
a failure.  Bounds: TOL for a product and the adapter, 1.5 TOL for a folded product (tests/test_gpu_chain.py); the tag is the
launch's note (post_attn1 / post_cam / pre_attn1).  groupnorm_scale_shift: x * scale + shift against fp64 GroupNorm within 1e-5
(test_spatial_transformer_pre_chain_equals_launches).
An igemm with per-image weights (the VAEs' mid attention) multiplies image i by slab i of the weight tensor's own shape; a
`w_group_stride` that disagrees with it is a failure.  The elementwise entry points are bit-exact where their contract is
(split_f32's hi and third part, trunk_add, the two-term coefficient-1 lincomb4, pack_sources).  Per call it snapshots the operands, runs the original with the same arguments, synchronises, computes the
fp64 reference on the device from the snapshots (the storage-rounded packed weights, the fp32 bias / rowvec / svec the launch
read) and compares:
  * whole-tensor rel-L2 within the bound the form's own unit test asserts (tests/test_gpu_ops.py);
  * the worst 128-row x 64-channel tile of an image within 4x that bound, a tile's error being
    |d| / max(|ref tile|, 0.1 x the norm a tile of the tensor's RMS would have);
  * every output element finite; the inputs unchanged (but a declared in-place residual); the bytes of `out`'s storage
    outside the view unchanged.
A split-K launch that returns an `ops.Deferred` stashes its fp64 product on it: the GroupNorm that sums its slabs is checked
against fp64 GroupNorm of that product (and, with `keep`, the tensor it writes against the product), a reduce launch
(`finish`) like any launch.  The first launch of every distinct variant tag also has 64 of its rows recomputed on the CPU
in fp64, which must agree with the device reference to 1e-9 (the device BLAS is not trusted blindly).

While a shadow runs, `mobi_amd._lib.load` returns a LibCensus that counts every `mobi_*` entry point called:
`census_failures()` lists a launching entry point called more often than the shadow judged its kind, and any entry point that
is neither shadowed nor query-only (LAUNCH_KINDS, QUERY_SUFFIXES): a new unwrapped launch cannot slip past.

`LaunchShadow(monkeypatch, extra=EXTRA_KINDS)` (or a subset) also wraps the entry points the conditioning producer and the
realism networks add (mobi_amd/ldm/modules/encoders/modules.py, mobi_amd/realism.py): skinny_linear (one ops call makes
ceil(m / 16) library calls, all counted), layernorm_rows_f32, linear_f32, quick_gelu, image_normalize, maxpool3s2, add,
lpips_distance, row_cosine, feature_moments, frd_input and band_mean, each against the fp64 (or, where the contract is
bit-exact, the torch) restatement its own unit test uses and within that test's bound; quick_gelu has no unit test: its output is
x sigmoid(1.702 x) in fp32 rounded once to T, so its rel-L2 AND its worst tile are bounded by the unit roundoff of T.  Without
`extra` the wrapped set is the UNet's and the VAEs' (WRAPPED), as before.  An igemm with `leaky` (MOBI_EPI_LEAKY_RELU) is judged
like any igemm: leaky_relu(., 0.1) after bias and rowvec, before the residual.

`LaunchShadow(monkeypatch, extra=TRAIN_KINDS + (...))` wraps the entry points the training step adds (mobi_amd/train.py:
unet_forward, unet_backward, loss_and_gradients, bbox_embedder_forward / _backward): transpose, colsum, layernorm_bwd,
groupnorm_bwd, geglu_fwd, geglu_bwd, attention_bwd, sumpool2, silu_bwd_f32, loss_grad and timestep_embedding.  Their references
are the ones the kernels' unit tests trust -- tests/backward_ref.py (`*_ref`, float64, on the CPU: every operand of a step at a
16 x 16 latent is small), tests/loss_grad_ref.py, oracle/unet.py's timestep_embedding -- and their bounds those tests' own (TOL1,
TOL_SUM, TOL_DGAMMA, REL; 1.5 TOL1 for an attention_bwd launch that backward_ref.attention_bwd_route sends to the matrix cores
with the strides and pointers the call passed).  The judgement of each kind is a plain function of CPU tensors (`*_checks`, as
check_split is) that returns Check records; the wrapper only snapshots, runs and records.  attention_bwd has one record per
output (dq, dk, dv); fp32 vectors / matrices are judged by rel-L2 with backward_ref.row_measure(block=64) recorded beside it.
`ops.linear_wgrad` and `ops.linear` need no wrapper: they call the MODULE's transpose / igemm / linear_f32 (`transpose(dy)`,
`igemm(...)`, `linear_f32(...)` are looked up in mobi_amd.ops' globals at call time), which are the patched ones -- a weight
gradient is a transpose pair and an OUT_ROWS_F32 igemm record (k = the token rows), or a linear_f32 record; the census proves it
(an unjudged mobi_transpose / mobi_igemm / mobi_linear_f32 call is a failure).  `add` stays bit-exact against the rounded fp32
sum (its unit test's own assertion; stricter than TOL1).  An igemm record's form says whether its source, its output and its
residual had a non-dense image stride (src_strided, out_strided, res_strided) and whether a 3 x 3 launch read a zero-spread
input (the stride-2 data gradient).

Nothing here calls a `mobi_*` entry point: the references are torch float64 (matmul per tap, attention per image and head).
"""
import collections
import math

import torch
import torch.nn.functional as F

from tests import backward_ref as R, chain_ref, loss_grad_ref
from tests.golden_cases import record
from tests.test_gpu_backward import TOL1
from tests.test_gpu_backward_geometry import TOL_DGAMMA, TOL_SUM
from tests.test_gpu_loss_grad import REL
from tests.test_gpu_ops import TOL

LN2 = math.log(2.0)
TILE_ROWS, TILE_COLS = 128, 64
TILE_FACTOR = 4.0
CPU_AGREE = 1e-9
CPU_ROWS = 64


def bound_f32_rows(dtype):
    """OUT_ROWS_F32 (fp32 output of 16-bit operands): test_igemm_epilogues' bound."""
    return 2e-5 * (100 if dtype == torch.bfloat16 else 1) + 1e-6


def bound_gn_f32(dtype):
    """GN_OUT_F32: test_groupnorm_fp32_source_and_precise_outputs."""
    return 2e-6


def bound_gn_split(dtype):
    """hi + lo of GN_OUT_SPLIT / SPLIT3 (and of split_f32): test_groupnorm_fp32_source_and_precise_outputs."""
    return 2e-6 if dtype == torch.float16 else 2e-5


BOUND_GN_SCALE_SHIFT = 1e-5     # test_spatial_transformer_pre_chain_equals_launches: x * scale + shift against GroupNorm
BOUND_LINCOMB = 1e-6            # test_sampler_arithmetic_bit_exact: lincomb4 against fp64
BOUND_SMALL_COUT = 2e-5         # test_conv_small_cout_matrix_core_form: fp32 NCHW output of 16-bit operands
BOUND_SMALL_CIN_F32 = 2e-6      # test_small_convs: conv_small_cin with out_f32_nchw

BOUND_SKINNY = 2e-6             # test_skinny_linear_and_timestep_embedding: against fp64, no activation / GELU behind
BOUND_SKINNY_SILU = 2e-5        # the same test's SiLU form
BOUND_F32_ROWS = 2e-6           # TOL_F32 of tests/test_gpu_norm_stats.py (layernorm_rows_f32); test_linear_f32
BOUND_LPIPS_DISTANCE = 1e-6     # test_layer_distance_against_fp64: max relative per pair
BOUND_ROW_COSINE = 1e-6         # test_row_cosine_against_fp64: |d| / max(|ref|, 1)
BOUND_MOMENTS = 1e-15           # test_moments_against_fp64_and_reproducible (fp64 sums)
BOUND_BAND_MEAN = 4.5e-7        # test_band_mean_against_fp64: max |d| / max |ref|
BOUND_TIMESTEP = 1e-6           # test_skinny_linear_and_timestep_embedding: rel-L2 against oracle/unet.py's fp32 restatement
UNIT_ROUNDOFF = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}      # quick_gelu: one rounding of an fp32 value to T
QUICK_GELU_ALPHA = 1.702

# entry points of the library that launch a kernel -> the shadow kind that judges each call
LAUNCH_KINDS = {"mobi_igemm": "igemm", "mobi_igemm_finish": "split_finish", "mobi_groupnorm": "groupnorm",
                "mobi_layernorm": "layernorm", "mobi_attention": "attention", "mobi_ctx_attention": "ctx_attention",
                "mobi_ff_geglu": "ff_geglu", "mobi_two_key_adapter": "two_key_adapter", "mobi_softmax_rows": "softmax_rows",
                "mobi_split_f32": "split_f32", "mobi_trunk_add": "trunk_add", "mobi_lincomb4": "lincomb4",
                "mobi_conv_small_cout": "conv_small_cout", "mobi_conv_small_cin": "conv_small_cin",
                "mobi_pack_nchw_sources": "pack_sources", "mobi_row_chain": "row_chain",
                "mobi_row_chain_adapter_image": "chain_adapter_image", "mobi_groupnorm_scale_shift": "groupnorm_scale_shift",
                # the conditioning producer's and the realism networks' (LaunchShadow(extra=...))
                "mobi_skinny_linear": "skinny_linear", "mobi_layernorm_rows_f32": "layernorm_rows_f32",
                "mobi_linear_f32": "linear_f32", "mobi_quick_gelu": "quick_gelu", "mobi_image_normalize": "image_normalize",
                "mobi_maxpool3s2": "maxpool3s2", "mobi_add": "add", "mobi_lpips_distance": "lpips_distance",
                "mobi_row_cosine": "row_cosine", "mobi_feature_moments": "feature_moments", "mobi_frd_input": "frd_input",
                "mobi_band_mean": "band_mean",
                # the training step's (LaunchShadow(extra=TRAIN_KINDS + ...))
                "mobi_transpose": "transpose", "mobi_colsum": "colsum", "mobi_layernorm_bwd": "layernorm_bwd",
                "mobi_groupnorm_bwd": "groupnorm_bwd", "mobi_geglu_fwd": "geglu_fwd", "mobi_geglu_bwd": "geglu_bwd",
                "mobi_attention_bwd": "attention_bwd", "mobi_sumpool2": "sumpool2", "mobi_silu_bwd_f32": "silu_bwd_f32",
                "mobi_loss_grad": "loss_grad", "mobi_timestep_embedding": "timestep_embedding"}
EXTRA_KINDS = ("skinny_linear", "layernorm_rows_f32", "linear_f32", "quick_gelu", "image_normalize", "maxpool3s2", "add",
               "lpips_distance", "row_cosine", "feature_moments", "frd_input", "band_mean")
TRAIN_KINDS = ("transpose", "colsum", "layernorm_bwd", "groupnorm_bwd", "geglu_fwd", "geglu_bwd", "attention_bwd", "sumpool2",
               "silu_bwd_f32", "loss_grad", "timestep_embedding")
# entry points that answer a question and launch nothing (mobi_tile_weights: the load-time weight image of a pack)
QUERY_SUFFIXES = ("_workspace_bytes", "_plan_splits", "_slab_count", "_kernel_variant", "_takes_split", "_sync_bytes",
                  "_supported", "_fuses_ln", "_packed_bytes", "_weight_bytes", "_image_bytes", "_ws_floats", "_workspace_floats")
QUERY_NAMES = ("mobi_tile_weights", "mobi_error_string", "mobi_build_info", "mobi_abi_version", "mobi_struct_size",
               "mobi_backward_partial_blocks", "mobi_loss_grad_blocks_per_sample")


def is_query_only(name):
    return name in QUERY_NAMES or name.endswith(QUERY_SUFFIXES)


class LibCensus:
    """Stands in for the loaded library while a shadow runs: counts every `mobi_*` entry point called through it."""

    def __init__(self, lib, calls):
        self._lib, self._calls, self._fns = lib, calls, {}

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            real = getattr(self._lib, name)
            if not name.startswith("mobi_") or not callable(real):
                return real
            calls = self._calls

            def fn(*a):
                calls[name] = calls.get(name, 0) + 1
                return real(*a)
            self._fns[name] = fn
        return fn


# ------------------------------------------------------------------------------------------------------------------
# metric
# ------------------------------------------------------------------------------------------------------------------
def compare(got, ref):
    """got, ref: [images, rows, channels] (any float type; compared in fp64 on ref's device) -> dict(rel, tile, where,
    finite): whole-tensor rel-L2, the worst tile's error and its (image, first row, first channel)."""
    g = got.to(device=ref.device, dtype=torch.float64)
    r = ref.double()
    finite = bool(torch.isfinite(g).all())
    d = g - r
    rel = float(d.norm() / r.norm().clamp_min(1e-30))
    n, rows, cols = r.shape
    pr, pc = (-rows) % TILE_ROWS, (-cols) % TILE_COLS

    def tiles(t):
        t = F.pad(t, (0, pc, 0, pr))
        return t.reshape(n, (rows + pr) // TILE_ROWS, TILE_ROWS, (cols + pc) // TILE_COLS, TILE_COLS).sum(dim=(2, 4))

    ed = tiles(d.square())
    er = tiles(r.square())
    cnt = tiles(torch.ones_like(r))
    rms2 = float(r.square().mean())
    floor = 0.01 * rms2 * cnt                                # (0.1 x RMS-equivalent tile norm)^2
    te = (ed / torch.maximum(er, floor).clamp_min(1e-300)).sqrt()
    te = torch.where(torch.isfinite(te), te, torch.full_like(te, float("inf")))
    flat = int(torch.argmax(te))
    tr, tc = te.shape[1], te.shape[2]
    where = (flat // (tr * tc), (flat // tc) % tr * TILE_ROWS, flat % tc * TILE_COLS)
    return dict(rel=rel, tile=float(te.max()), where=where, finite=finite)


def passes(res, bound):
    return res["finite"] and res["rel"] < bound and res["tile"] < TILE_FACTOR * bound


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


class OutsideView:
    """The elements of a view's storage that lie outside the view, kept to check that a launch wrote none of them."""

    def __init__(self, t):
        self.flat = torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage())
        idx = torch.arange(self.flat.numel(), device=t.device).as_strided(t.shape, t.stride(), t.storage_offset())
        self.mask = torch.ones(self.flat.numel(), dtype=torch.bool, device=t.device)
        self.mask[idx.reshape(-1)] = False
        self.any = bool(self.mask.any())
        self.before = _bits(self.flat)[self.mask].clone() if self.any else None

    def unchanged(self):
        return not self.any or torch.equal(_bits(self.flat)[self.mask], self.before)


def softmax_row_sums(got):
    """max over rows of |sum of the row - 1| of a softmax output [rows, cols] (fp64 on its device)."""
    return float((got.double().sum(dim=-1) - 1.0).abs().max())


def check_split(x32, out, parts, dtype):
    """split_f32's contract -> failure strings: hi == T(x) bit for bit, hi + lo within bound_gn_split, part 3 == hi bit for bit."""
    c = x32.shape[-1]
    bad = []
    if tuple(out.shape) != tuple(x32.shape[:-1]) + (parts * c,) or out.dtype != dtype:
        return [f"shape / dtype {tuple(out.shape)} {out.dtype}"]
    hi, lo = out[..., :c], out[..., c:2 * c]
    if not _same(hi, x32.to(dtype)):
        bad.append("hi is not the rounded input")
    res = compare((hi.double() + lo.double()).reshape(1, -1, c), x32.double().reshape(1, -1, c))
    if not passes(res, bound_gn_split(dtype)):
        bad.append(f"hi + lo rel-L2 {res['rel']:.3e} tile {res['tile']:.3e} (bound {bound_gn_split(dtype):.1e})")
    if parts == 3 and not _same(out[..., 2 * c:], hi):
        bad.append("the third part is not hi")
    return bad


def check_trunk_add(before, inc, after, x16, dtype):
    """trunk_add's contract -> failure strings: the fp32 trunk is before + inc (fp32 add, bit for bit; unchanged for inc None)
    and the returned copy is the updated trunk rounded to the storage type, bit for bit."""
    want = before if inc is None else before + inc.float()
    bad = []
    if not _same(after, want):
        bad.append("the fp32 trunk is not trunk + inc" if inc is not None else "the trunk changed without an increment")
    if x16.dtype != dtype or not _same(x16, want.to(dtype)):
        bad.append("the 16-bit copy is not the updated trunk rounded")
    return bad


def per_image_weights(w, n, n_packed, k, w_group_stride):
    """The slabs an igemm with weight_per_image multiplies image i by, taken from the weight tensor's own shape
    ([n, n_packed, k]); raises ValueError if the launch's w_group_stride says otherwise."""
    if w.numel() != n * n_packed * k:
        raise ValueError(f"per-image weights: {w.numel()} elements, not {n} images x {n_packed} x {k}")
    if w.dim() == 3 and w.stride(0) != n_packed * k:
        raise ValueError(f"per-image weights: the tensor's image stride {w.stride(0)} is not {n_packed * k}")
    if w_group_stride != n_packed * k:
        raise ValueError(f"per-image weights: w_group_stride {w_group_stride} disagrees with the tensor's slabs ({n_packed * k})")
    return w.reshape(n, n_packed, k)


def _snap(t):
    return None if t is None else t.detach().clone()


def _host(t):
    """The CPU copy of an operand: what the training kinds' references (tests/backward_ref.py: CPU torch) read."""
    return None if t is None else t.detach().cpu()


def _img_strided(t):
    """A batch-strided view (`x[::2]`): more than one image and an image stride that is not the dense one."""
    return t.shape[0] > 1 and t.stride(0) != t[0].numel()


def _tag_int(tag, key, default):
    """The integer after `key=` in a profiler tag (ops._Timed), or `default`."""
    for part in tag.split():
        if part.startswith(key + "="):
            return int(part[len(key) + 1:])
    return default


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


# ------------------------------------------------------------------------------------------------------------------
# references (fp64; `rows`: flattened output rows to compute, None = all; every operand is moved to `dev`)
# ------------------------------------------------------------------------------------------------------------------
def _chunks(total, rows, per):
    if rows is not None:
        yield rows
        return
    for r0 in range(0, total, per):
        yield torch.arange(r0, min(total, r0 + per))


def igemm_reference(op, rows=None, dev=None):
    """mobi_igemm's contract: out[m] = epilogue(scale * sum_taps A_tap[m] W_tap^T (+ bias) (+ rowvec[image]) (+ residual[m])),
    the LayerNorm fold as ((x - mean) rstd) W'^T + bias, GEGLU as value * gelu_erf(gate) of the packed row pairs,
    MOBI_EPI_LEAKY_RELU (op["leaky"]) as leaky_relu(., 0.1) after bias and rowvec and before the residual.
    -> fp64 [len(rows), cout] (or [images, hout * wout, cout] for rows=None)."""
    dev = op["x"].device if dev is None else dev
    to = lambda t: None if t is None else t.to(dev)
    src = to(op["x"]) if op["x2"] is None else torch.cat([to(op["x"]), to(op["x2"])], dim=3)
    n, hin, win, c = src.shape
    kh, kw, st, ph, pw = op["kh"], op["kw"], op["stride"], op["pad_h"], op["pad_w"]
    hl, wl = (2 * hin, 2 * win) if op["upsample"] else (hin, win)
    hout, wout, cout, npk, groups = op["hout"], op["wout"], op["cout"], op["n_packed"], op["groups"]
    w = to(op["w"]).double().reshape(groups, npk, kh * kw, c)          # k = tap * C + c
    bias = None if op["bias"] is None or op["rowvec_has_bias"] else to(op["bias"]).double()
    rowvec = None if op["rowvec"] is None else to(op["rowvec"]).double()
    res = None if op["residual"] is None else to(op["residual"]).double().reshape(-1, cout)
    hw = hout * wout
    total = n * hw
    per = max(256, (1 << 25) // max(kh * kw * c, npk))
    outs = []
    for r in _chunks(total, None if rows is None else rows.to(dev), per):
        r = r.to(dev)
        img, p = r // hw, r % hw
        oy, ox = p // wout, p % wout
        grp = img // (n // groups)
        acc = torch.zeros((r.numel(), npk), dtype=torch.float64, device=dev)
        for tap in range(kh * kw):
            ly, lx = oy * st - ph + tap // kw, ox * st - pw + tap % kw
            ok = (ly >= 0) & (ly < hl) & (lx >= 0) & (lx < wl)
            sy, sx = ly.clamp(0, hl - 1), lx.clamp(0, wl - 1)
            if op["upsample"]:
                sy, sx = sy // 2, sx // 2
            a = src[img, sy, sx].double() * ok[:, None]
            if op["ln"]:
                mean = a.mean(dim=1, keepdim=True)
                var = (a - mean).square().mean(dim=1, keepdim=True)
                a = (a - mean) * (var + op["ln_eps"]).rsqrt()
            for g in range(groups):
                sel = grp == g
                if groups == 1:
                    acc += a @ w[0, :, tap].T
                elif bool(sel.any()):
                    acc[sel] += a[sel] @ w[g, :, tap].T
        v = acc * op["scale"]
        if bias is not None:
            v = v + bias
        if op["geglu"]:
            t = v.reshape(r.numel(), npk // 16, 2, 8)
            v = (t[:, :, 0] * F.gelu(t[:, :, 1])).reshape(r.numel(), cout)
        if rowvec is not None:
            v = v + rowvec[img]
        if op.get("leaky"):
            v = F.leaky_relu(v, 0.1)
        if res is not None:
            v = v + res[r]
        outs.append(v)
    out = torch.cat(outs)
    return out if rows is not None else out.reshape(n, hw, cout)


def groupnorm_reference(op, rows=None, dev=None):
    """GroupNorm(32 groups, eps) (+ SiLU) over the channel concat of the sources, fp64 -> [images, hw, C] (rows: those rows,
    flattened over images)."""
    dev = op["x"].device if dev is None else dev
    x = op["x"].to(dev).double()
    n, c0 = x.shape[0], x.shape[-1]
    x = x.reshape(n, -1, c0)
    if op["x2"] is not None:
        x = torch.cat([x, op["x2"].to(dev).double().reshape(n, x.shape[1], -1)], dim=2)
    hw, c = x.shape[1], x.shape[2]
    imgs = torch.arange(n, device=dev) if rows is None else torch.unique(rows.to(dev) // hw)
    xs = x[imgs].reshape(imgs.numel(), hw, 32, c // 32)
    mean = xs.mean(dim=(1, 3), keepdim=True)
    var = (xs - mean).square().mean(dim=(1, 3), keepdim=True)
    y = ((xs - mean) * (var + op["eps"]).rsqrt()).reshape(imgs.numel(), hw, c)
    y = y * op["gamma"].to(dev).double() + op["beta"].to(dev).double()
    if op["silu"]:
        y = F.silu(y)
    if rows is None:
        return y
    pos = torch.searchsorted(imgs, rows.to(dev) // hw)
    return y[pos, rows.to(dev) % hw]


def layernorm_rows(x, gamma, beta, eps):
    x = x.double()
    mean = x.mean(dim=-1, keepdim=True)
    var = (x - mean).square().mean(dim=-1, keepdim=True)
    y = (x - mean) * (var + eps).rsqrt()
    return y if gamma is None else y * gamma.double() + beta.double()


def layernorm_reference(op, rows=None, dev=None):
    dev = op["x"].device if dev is None else dev
    x = op["x"].to(dev)
    n, t, c = x.shape
    sel = x.reshape(n * t, c) if rows is None else x.reshape(n * t, c)[rows.to(dev)]
    y = layernorm_rows(sel, op["gamma"].to(dev), op["beta"].to(dev), op["eps"])
    return y.reshape(n, t, c) if rows is None else y


def attention_reference(op, rows=None, dev=None):
    """softmax(q k^T * scale) v per image and head (q_log2_scaled: q carries scale * log2 e, the logits are q.k * ln 2);
    v_rows: v [N, Tk, C] like k, else V^T [N, C, Tk].  rows: flattened (image, query) rows."""
    dev = op["q"].device if dev is None else dev
    q, k, v = op["q"].to(dev), op["k"].to(dev), op["v"].to(dev)
    n, tq = q.shape[0], q.shape[1]
    h = op["heads"]
    c = v.shape[2] if op["v_rows"] else v.shape[1]
    dh = c // h
    mult = LN2 if op["q_log2_scaled"] else op["scale"]
    rsel = torch.arange(n * tq, device=dev) if rows is None else rows.to(dev)
    out = torch.empty((rsel.numel(), c), dtype=torch.float64, device=dev)
    for i in range(n):
        pos = (rsel // tq == i).nonzero().flatten()
        if pos.numel() == 0:
            continue
        kk = k[i, :, :c].double().reshape(-1, h, dh).transpose(0, 1)                  # [H, Tk, dh]
        vv = (v[i, :, :c].double().reshape(-1, h, dh) if op["v_rows"] else v[i].double().T.reshape(-1, h, dh)).transpose(0, 1)
        for p0 in range(0, pos.numel(), 1024):
            pp = pos[p0:p0 + 1024]
            qq = q[i, rsel[pp] % tq, :c].double().reshape(-1, h, dh).transpose(0, 1)    # [H, R, dh]
            # (softmax spelled out: torch.softmax in fp64 on the device is off by ~5e-8 rel-L2 over 4,096 keys, measured against
            #  the CPU; exp / max / sum / matmul agree to 1e-16)
            s = qq @ kk.transpose(1, 2) * mult
            e = torch.exp(s - s.amax(dim=-1, keepdim=True))
            out[pp] = ((e @ vv) / e.sum(dim=-1, keepdim=True)).transpose(0, 1).reshape(-1, c)
    return out if rows is not None else out.reshape(n, tq, c)


def ctx_attention_reference(op, rows=None, dev=None):
    dev = op["q"].device if dev is None else dev
    q, k, v = op["q"].to(dev), op["k"].to(dev), op["v"].to(dev)
    return attention_reference(dict(q=q, k=k, v=v, heads=op["heads"], scale=op["scale"], v_rows=True, q_log2_scaled=False),
                               rows, dev)


def decode_ff_geglu(buf, c, hidden, dtype):
    """The chunk images of mobi_ff_geglu (include/mobi_engine.h, the w_packed layout) -> (W1 [2 hidden, c], b1 [2 hidden]
    fp32, W2 [c, hidden]) as the storage type / fp32: index arithmetic on the documented formula, not the packer."""
    ks_n, mt_n, nch = c // 16, c // 32, hidden // 32
    dev = buf.device
    ar = lambda k: torch.arange(k, device=dev)
    n1 = nch * 2 * ks_n * 512
    img1 = buf[:2 * n1].view(dtype).reshape(nch, 2, ks_n, 64, 8)
    rest = buf[2 * n1:].reshape(nch, -1)
    img2 = rest[:, :2 * mt_n * 1024].contiguous().view(dtype).reshape(nch, mt_n, 2, 64, 8)
    bias = rest[:, 2 * mt_n * 1024:].contiguous().view(torch.float32).reshape(nch, 256)
    lane, j = ar(64), ar(8)
    # first product: element j of fragment (t, ks), lane l = W1[t hidden + 32 chunk + (l & 31)][16 ks + 8 (l >> 5) + j]
    r1 = ar(2)[None, :, None, None, None] * hidden + ar(nch)[:, None, None, None, None] * 32 + (lane & 31)[None, None, None, :, None]
    c1 = ar(ks_n)[None, None, :, None, None] * 16 + (lane >> 5)[None, None, None, :, None] * 8 + j[None, None, None, None, :]
    w1 = torch.zeros((2 * hidden, c), dtype=dtype, device=dev)
    w1[r1.expand_as(img1), c1.expand_as(img1)] = img1
    # second product: fragment 2 m + s: element j = W2[32 m + (l & 31)][32 chunk + 16 s + 8 (j >> 2) + 4 (l >> 5) + (j & 3)]
    r2 = ar(mt_n)[None, :, None, None, None] * 32 + (lane & 31)[None, None, None, :, None]
    c2 = (ar(nch)[:, None, None, None, None] * 32 + ar(2)[None, None, :, None, None] * 16 + (j >> 2)[None, None, None, None, :] * 8
          + (lane >> 5)[None, None, None, :, None] * 4 + (j & 3)[None, None, None, None, :])
    w2 = torch.zeros((c, hidden), dtype=dtype, device=dev)
    w2[r2.expand_as(img2), c2.expand_as(img2)] = img2
    b1 = torch.cat([bias[:, :32].reshape(hidden), bias[:, 32:64].reshape(hidden)])
    return w1, b1, w2


def ff_geglu_reference(op, rows=None, dev=None):
    """((x' W1v^T + b1v) * gelu_erf(x' W1g^T + b1g)) W2^T + b2 (+ residual), x' = x or LayerNorm(x) -> [images, T, c]."""
    dev = op["x"].device if dev is None else dev
    x = op["x"].to(dev)
    c = x.shape[-1]
    xr = x.reshape(-1, c)
    w1, b1, w2 = (t.to(dev).double() for t in op["dec"])
    hidden = w2.shape[1]
    b2 = None if op["b2"] is None else op["b2"].to(dev).double()
    res = None if op["residual"] is None else op["residual"].to(dev).reshape(-1, c)
    outs = []
    for r in _chunks(xr.shape[0], None if rows is None else rows.to(dev), 16384):
        r = r.to(dev)
        a = xr[r].double()
        if op["ln"] is not None:
            g, b, eps = op["ln"]
            a = layernorm_rows(a, g.to(dev), b.to(dev), eps)
        pre = a @ w1.T + b1
        y = (pre[:, :hidden] * F.gelu(pre[:, hidden:])) @ w2.T
        if b2 is not None:
            y = y + b2
        if res is not None:
            y = y + res[r].double()
        outs.append(y)
    out = torch.cat(outs)
    return out if rows is not None else out.reshape(x.shape[0], -1, c)


def two_key_adapter_reference(x, a, a_sum, c, u, b, eps):
    """mobi_two_key_adapter's contract, fp64: x + b + sum_h sigmoid(rstd (x . a_h - mean a_sum_h) + c_h) u_h with the token's
    LayerNorm statistics.  x [N, T, C]; a, u [N, H, C]; a_sum, c [N, H]; b [N, C] -> [N, T, C]."""
    x, a, a_sum, c, u, b = (t.double() for t in (x, a, a_sum, c, u, b))
    mean = x.mean(-1, keepdim=True)
    rstd = ((x - mean).square().mean(-1, keepdim=True) + eps).rsqrt()
    z = rstd * (torch.einsum("ntc,nhc->nth", x, a) - mean * a_sum[:, None, :]) + c[:, None, :]
    return x + b[:, None, :] + torch.einsum("nth,nhc->ntc", torch.sigmoid(z), u)


def two_key_adapter_op_reference(op, rows=None, dev=None):
    dev = op["x"].device if dev is None else dev
    x = op["x"].to(dev)
    n, t, ch = x.shape
    if rows is None:
        return two_key_adapter_reference(x, *(op[k].to(dev) for k in ("a", "a_sum", "c", "u", "b")), op["eps"])
    rows = rows.to(dev)
    img = rows // t
    y = two_key_adapter_reference(x.reshape(n * t, 1, ch)[rows], *(op[k].to(dev)[img] for k in ("a", "a_sum", "c", "u", "b")),
                                  op["eps"])
    return y.reshape(-1, ch)


def softmax_reference(op, rows=None, dev=None):
    """Row softmax of fp32 scores [rows, cols], spelled out in fp64 (see attention_reference) -> [rows, cols] (rows: those)."""
    dev = op["s"].device if dev is None else dev
    s = op["s"].to(dev)
    outs = []
    for r in _chunks(s.shape[0], None if rows is None else rows.to(dev), 4096):
        v = s[r.to(dev)].double()
        e = torch.exp(v - v.amax(dim=-1, keepdim=True))
        outs.append(e / e.sum(dim=-1, keepdim=True))
    return torch.cat(outs)


def conv_small_cout_reference(op, rows=None, dev=None):
    """mobi_conv_small_cout's contract: the convolution of the operands it read (T channels-last, T [cout][tap * C + c]) plus
    the fp32 bias in fp64, then the clamp -> [images, h * w, cout] (rows: flattened (image, pixel) rows)."""
    y = igemm_reference(op, rows, dev)
    return y if op["clamp"] is None else y.clamp(*op["clamp"])


def conv_small_cin_op(srcs, weight, bias, kh, kw, pad):
    """The operand record of a conv_small_cin launch as an igemm_reference form: the fp32 NCHW sources concatenated on channels
    as channels-last, the OIHW-flattened fp32 weight reordered to k = tap * C + c."""
    x = torch.cat(srcs, dim=1).permute(0, 2, 3, 1)
    n, h, w, cin = x.shape
    cout = weight.shape[0]
    wt = weight.reshape(cout, cin, kh, kw).permute(0, 2, 3, 1).reshape(cout, kh * kw * cin)
    return dict(x=x, x2=None, w=wt, bias=bias, kh=kh, kw=kw, stride=1, pad_h=pad[0], pad_w=pad[1], upsample=False,
                hout=h + 2 * pad[0] - kh + 1, wout=w + 2 * pad[1] - kw + 1, cout=cout, n_packed=cout, groups=1, geglu=False,
                ln=False, ln_eps=0.0, scale=1.0, rowvec=None, rowvec_has_bias=False, residual=None)


# ------------------------------------------------------------------------------------------------------------------
# the training step's launches: plain judgements of CPU tensors (the operands a launch read, what it wrote) -> Check records
# ------------------------------------------------------------------------------------------------------------------
# mode "tiles": got / ref [images, rows, channels] through `compare` (rel-L2 < bound, worst tile < 4x bound); "value": an fp32
# vector / matrix, rel-L2 < bound with backward_ref.row_measure(block=64) beside it; "exact": bit for bit; "figure": `got` is an
# error figure already (<= bound); "fault": a broken contract, `got` says which
Check = collections.namedtuple("Check", "what mode got ref bound")


def evaluate(ck):
    """-> dict(rel, tile, where, finite, row, ok) of one Check."""
    if ck.mode == "tiles":
        res = compare(ck.got, ck.ref)
        return dict(res, row=None, ok=passes(res, ck.bound))
    if ck.mode == "value":
        finite = bool(torch.isfinite(ck.got).all())
        rel = R.rel_l2(ck.got, ck.ref) if finite else float("inf")
        row = R.row_measure(ck.got, ck.ref, block=64) if finite else float("inf")
        return dict(rel=rel, tile=rel, where=(0, 0, 0), finite=finite, row=row, ok=finite and rel < ck.bound)
    if ck.mode == "exact":
        ok = ck.got.dtype == ck.ref.dtype and _same(ck.got, ck.ref)
        err = 0.0 if ok else float("inf")
        return dict(rel=err, tile=err, where=(0, 0, 0), finite=bool(torch.isfinite(ck.got.float()).all()), row=None, ok=ok)
    if ck.mode == "figure":
        ok = ck.got <= ck.bound                                   # (a NaN figure fails)
        return dict(rel=ck.got, tile=ck.got, where=(0, 0, 0), finite=math.isfinite(ck.got), row=None, ok=ok)
    return dict(rel=float("inf"), tile=float("inf"), where=(0, 0, 0), finite=True, row=None, ok=False)      # "fault"


def check_failures(kind, tag, checks):
    """The failure strings of a launch's checks, each naming the launch (kind, tag) and the output."""
    bad = []
    for ck in checks:
        res = evaluate(ck)
        if res["ok"]:
            continue
        if ck.mode == "fault":
            bad.append(f"{kind} {tag}: {ck.got}")
        elif ck.mode == "exact":
            bad.append(f"{kind} {tag} {ck.what}: not the restatement bit for bit")
        else:
            bad.append(f"{kind} {tag} {ck.what}: rel-L2 {res['rel']:.3e}, worst tile {res['tile']:.3e} at {res['where']}, finite "
                       f"{res['finite']} (bound {ck.bound:.1e})")
    return bad


def describe(**tensors):
    """name=shape/strides of every tensor given: what a failure string says about the operands."""
    return " ".join(f"{k}={tuple(t.shape)}/{tuple(t.stride())}" for k, t in tensors.items() if t is not None)


def _images(t):
    return t.reshape(t.shape[0], -1, t.shape[-1])


def transpose_checks(x, out):
    """mobi_transpose: out == x^T bit for bit (tests/test_gpu_backward_geometry.py::test_transpose_and_tile_weights_bit_exact)."""
    if tuple(out.shape) != (x.shape[1], x.shape[0]):
        return [Check("out", "fault", f"shape {tuple(out.shape)}", None, 0.0)]
    return [Check("out", "exact", out, x.t().contiguous(), 0.0)]


def colsum_checks(dy, out):
    return [Check("out", "value", out, R.colsum_ref(dy), TOL_SUM)]


def layernorm_bwd_checks(x, dy, gamma, eps, dx_add, dx, dgamma, dbeta):
    """x, dy, dx_add, dx [N, T, C]; gamma, dgamma, dbeta [C]."""
    c = x.shape[-1]
    rows = lambda t: None if t is None else t.reshape(-1, c)
    rdx, rdg, rdb = R.layernorm_bwd_ref(rows(x), rows(dy), gamma, eps, dx_add=rows(dx_add))
    return [Check("dx", "tiles", dx, rdx.reshape(x.shape), TOL1[x.dtype]), Check("dgamma", "value", dgamma, rdg, TOL_DGAMMA),
            Check("dbeta", "value", dbeta, rdb, TOL_DGAMMA)]


def groupnorm_bwd_checks(x, dy, gamma, beta, eps, silu, dx_add, dx):
    """x, dy, dx_add, dx [N, H, W, C]."""
    ref = R.groupnorm_bwd_ref(_images(x), _images(dy), gamma, beta, eps, silu, dx_add=None if dx_add is None else _images(dx_add))
    return [Check("dx", "tiles", _images(dx), ref, TOL1[x.dtype])]


def geglu_fwd_checks(pre, h):
    return [Check("h", "tiles", _images(h), _images(R.geglu_fwd_ref(pre)), TOL1[pre.dtype])]


def geglu_bwd_checks(pre, dh, dpre):
    return [Check("dpre", "tiles", _images(dpre), _images(R.geglu_bwd_ref(pre, dh)), TOL1[pre.dtype])]


def attention_bwd_checks(q, k, v, dout, heads, scale, route, dq, dk, dv):
    """q, dout, dq [N, Tq, C]; k, v, dk, dv [N, Tk, C]; route: what backward_ref.attention_bwd_route says of the call."""
    bound = TOL1[q.dtype] * (1.5 if route == "mfma" else 1.0)
    ref = R.attention_bwd_ref(q, k, v, dout, heads, scale)
    return [Check(nm, "tiles", got, want, bound) for nm, got, want in zip(("dq", "dk", "dv"), (dq, dk, dv), ref)]


def attention_bwd_diagnosis(q, k, v, dout, heads, scale, dtype, ref):
    """For a failure string: rel-L2 of both storage restatements (backward_ref.attention_bwd_restated) against the same float64
    reference, the share of dout and of the reference dq below the smallest fp16 normal, and the keys' common component."""
    parts = []
    for route in ("mfma", "vector"):
        rs = R.attention_bwd_restated(q, k, v, dout, heads, scale, dtype, route)
        parts.append(f"restated {route}: " + " ".join(f"{nm} {R.rel_l2(g, w):.3e}" for nm, g, w in zip(("dq", "dk", "dv"), rs, ref)))
    # the same restatement with dout x 256 (a power of two: exact) and the result / 256: what dS would keep above fp16's subnormals
    rs = R.attention_bwd_restated(q, k, v, (dout.float() * 256.0).to(dtype), heads, scale, dtype, "mfma")
    parts.append("restated mfma on dout x 256: " + " ".join(f"{nm} {R.rel_l2(g / 256.0, w):.3e}" for nm, g, w in zip(("dq", "dk", "dv"), rs, ref)))
    tiny = lambda t: float((t.double().abs() < 2.0 ** -14).double().mean())
    kd = k.double()
    offset = float(kd.mean(1).norm() / (kd - kd.mean(1, keepdim=True)).pow(2).mean(1).sum(-1).sqrt().mean().clamp_min(1e-300))
    parts.append(f"below 2^-14: dout {tiny(dout):.2f} dq {tiny(ref[0]):.2f}; rms dout {float(dout.double().pow(2).mean().sqrt()):.2e}; "
                 f"keys' common component / spread {offset:.2f}")
    return "; ".join(parts)


def sumpool2_checks(src, out):
    return [Check("out", "tiles", _images(out), _images(R.sumpool2_ref(src)), TOL1[src.dtype])]


def silu_bwd_f32_checks(z, dy, dx):
    return [Check("dx", "value", dx, R.silu_bwd_ref(z, dy), TOL_SUM)]


def _max_relative(got, want):
    """max |got - want| / |want|, 0 where both are exactly 0 (loss_vlb of the default objective's zero tables)."""
    got, want = got.double(), want.double()
    err = (got - want).abs() / want.abs()
    err = torch.where((got == 0) & (want == 0), torch.zeros_like(err), err)
    return float(err.max()) if bool(torch.isfinite(err).all()) else float("inf")


def loss_grad_checks(eps, target, t, logvar, lvlb, kw, dtype, c_pad, dy, per_sample, terms):
    """mobi_loss_grad as tests/test_gpu_loss_grad.py::test_kernel_against_the_contract asserts it: dy [N, H, W, c_pad] of the
    storage type, exactly +0 beyond the channels; l1: the fp64 contract rounded once, bit for bit; l2: within one storage ulp of
    the fp64 contract (the kernel forms k e - k g in fp32 before its one rounding); per_sample and terms within REL.
    kw: loss_type, l_simple_weight, elbo_weight, loss_scale."""
    n, c, h, w = eps.shape
    if tuple(dy.shape) != (n, h, w, c_pad) or dy.dtype != dtype:
        return [Check("dy", "fault", f"dy shape / dtype {tuple(dy.shape)} {dy.dtype}", None, 0.0)]
    rdy, rper, rterms = loss_grad_ref.loss_grad_ref(eps, target, t, logvar, lvlb, **kw)
    out = []
    pad = dy[..., c:]
    if bool((pad != 0).any()) or bool(torch.signbit(pad).any()):
        out.append(Check("dy", "fault", f"dy is not +0 beyond the {c} out_channels", None, 0.0))
    if kw["loss_type"] == "l1":
        out.append(Check("dy", "exact", dy, loss_grad_ref.to_storage(rdy, dtype, c_pad), 0.0))
    else:
        over = (dy[..., :c].permute(0, 3, 1, 2).double() - rdy).abs() / loss_grad_ref.storage_ulp(rdy, dtype)
        out.append(Check("dy (storage ulp)", "figure", float(over.max()) if bool(torch.isfinite(over).all()) else float("inf"), None, 1.0))
    out.append(Check("per_sample", "figure", _max_relative(per_sample, rper), None, REL))
    out.append(Check("terms", "figure", _max_relative(terms, rterms), None, REL))
    return out


def timestep_embedding_checks(t, freqs, out):
    """As test_skinny_linear_and_timestep_embedding: rel-L2 against oracle/unet.py's timestep_embedding (fp32, max_period
    10,000; it forms its own frequencies, so a wrong table shows)."""
    from oracle.unet import timestep_embedding as ref_temb
    return [Check("out", "value", out, ref_temb(t, 2 * freqs.shape[0]), BOUND_TIMESTEP)]


# ------------------------------------------------------------------------------------------------------------------
# the shadow
# ------------------------------------------------------------------------------------------------------------------
class LaunchShadow:
    """Context manager: `with LaunchShadow(monkeypatch) as sh: net(...)`; then `sh.failures` (strings), `sh.records` (one
    dict per compared launch), `sh.counts` (launches shadowed per profiler kind), `sh.calls` (every `mobi_*` entry point called
    through the library while the shadow ran) and `sh.census_failures()`."""

    WRAPPED = ("igemm", "groupnorm", "layernorm", "attention", "ctx_attention", "ff_geglu", "two_key_adapter", "softmax_rows",
               "split_f32", "trunk_add", "lincomb4", "conv_small_cout", "conv_small_cin", "pack_sources", "row_chain",
               "chain_adapter_image", "groupnorm_scale_shift")

    def __init__(self, monkeypatch, verbose=False, label="", cpu_check=True, seed=0, extra=(), pinned=None):
        from mobi_amd import ops
        self.ops, self.mp, self.verbose, self.label, self.cpu_check = ops, monkeypatch, verbose, label, cpu_check
        unknown = [k for k in extra if k not in EXTRA_KINDS + TRAIN_KINDS]
        if unknown:
            raise ValueError(f"launch shadow: no extra kinds {unknown} (EXTRA_KINDS, TRAIN_KINDS)")
        self.wrapped = self.WRAPPED + tuple(k for k in EXTRA_KINDS + TRAIN_KINDS if k in extra)
        self.records, self.failures, self.counts, self.calls = [], [], {}, {}
        # {"<kind> #<ordinal of the launch among its kind> <output>": bound}: launches judged at a bound written down by name
        # (an fp16 operand range finding; twice the storage restatement's own figure on the same operands)
        self.pinned, self.pins_used = dict(pinned or {}), set()
        self.cpu_checked = set()
        self.pending = {}
        self.thin = {}                  # data_ptr of a pack_sources output -> its number of sources
        self.adapter_images = []        # per chain_adapter_image call: clones of the fp32 tables and of the returned image
        self.gen = torch.Generator().manual_seed(seed)

    def census_failures(self):
        """Every launching entry point called as often as the shadow judged its kind; no call of an entry point that is
        neither shadowed nor query-only."""
        bad = []
        for name, cnt in sorted(self.calls.items()):
            kind = LAUNCH_KINDS.get(name)
            if kind is not None:
                if self.counts.get(kind, 0) != cnt:
                    bad.append(f"{name}: {cnt} calls, {self.counts.get(kind, 0)} judged by the shadow")
            elif not is_query_only(name):
                bad.append(f"{name}: {cnt} launches no wrapper of the shadow saw")
        return bad

    # -- plumbing ------------------------------------------------------------------------------------------------------
    def __enter__(self):
        ops = self.ops
        if ops._PROFILE is None:
            self.sink = []
            self.mp.setattr(ops, "_PROFILE", self.sink)
        else:
            self.sink = ops._PROFILE
        from mobi_amd import _lib
        orig = {k: getattr(ops, k) for k in self.wrapped}
        orig_finish = ops.Deferred.finish
        self.orig = orig
        sh = self
        for k in self.wrapped:
            self.mp.setattr(ops, k, (lambda name: lambda *a, **kw: getattr(sh, "_" + name)(orig[name], *a, **kw))(k))
        self.mp.setattr(ops.Deferred, "finish", lambda d: sh._finish(orig_finish, d))
        self.mp.setattr(ops, "ChainProgram", chain_ref.recording_program())      # (builds what ops.ChainProgram builds)
        census = LibCensus(_lib.load(), self.calls)
        self.mp.setattr(_lib, "load", lambda: census)
        return self

    def __exit__(self, *exc):
        self.mp.undo()
        if exc[0] is None and self.pending:
            self.failures.append(f"{len(self.pending)} split-K launches whose partial sums nobody consumed")
        for name in sorted(set(self.pinned) - self.pins_used) if exc[0] is None else ():
            self._fail(f"pinned launch '{name}' did not run")
        return False

    def _tag(self, n0, kind):
        """The profiler record the original appended (ops._Timed), or ''."""
        for rec in self.sink[n0:]:
            if rec[0] == kind:
                return rec[5]
        return ""

    def _count(self, kind, calls=1):
        self.counts[kind] = self.counts.get(kind, 0) + calls

    def _fail(self, msg):
        self.failures.append(f"{self.label} {msg}")

    def _inputs_unchanged(self, what, pairs):
        for name, live, snap in pairs:
            if live is not None and not _same(live, snap):
                self._fail(f"{what}: input {name} changed")

    def _cpu_agree(self, key, fn, op, dev_ref, total):
        """First launch of a variant: 64 rows (first, last, 62 random) in fp64 on the CPU against the device reference."""
        if not self.cpu_check or key in self.cpu_checked:
            return
        self.cpu_checked.add(key)
        rnd = torch.randperm(max(total - 2, 1), generator=self.gen)[:CPU_ROWS - 2] + 1
        rows = torch.unique(torch.cat([torch.tensor([0, total - 1]), rnd.clamp(max=total - 1)]))
        cpu = fn(op, rows=rows, dev=torch.device("cpu"))
        dev = dev_ref.reshape(total, -1)[rows.to(dev_ref.device)].cpu()
        err = float((cpu - dev).norm() / cpu.norm().clamp_min(1e-300))
        if not err <= CPU_AGREE:
            self._fail(f"{key}: device fp64 reference disagrees with the CPU on {rows.numel()} rows: {err:.3e}")

    def _judge(self, kind, tag, got, ref, bound, extra="", form=None, tile_factor=TILE_FACTOR, detail=""):
        res = compare(got, ref)
        ok = res["finite"] and res["rel"] < bound and res["tile"] < tile_factor * bound
        rec = dict(kind=kind, tag=tag, bound=bound, extra=extra, form=form or {}, **res)
        self.records.append(rec)
        name = f"{kind} {tag} {extra}".strip()
        record(f"shadow {self.label} {name}", res["rel"], bound)
        record(f"shadow {self.label} {name} worst_tile", res["tile"], tile_factor * bound)
        if self.verbose:
            print(f"[shadow {self.label}] {kind:16s} {tag} {extra} rel={res['rel']:.3e} tile={res['tile']:.3e} "
                  f"at(img,row,col)={res['where']} bound={bound:.1e}{'' if ok else '  FAIL'}")
        if not ok:
            self._fail(f"{name}: rel-L2 {res['rel']:.3e}, worst tile {res['tile']:.3e} at {res['where']}, finite "
                       f"{res['finite']} (bound {bound:.1e}, tile bound {tile_factor * bound:.1e})" + (f" [{detail}]" if detail else ""))
        return res

    # -- igemm ---------------------------------------------------------------------------------------------------------
    def _igemm(self, orig, x, pw, *, x2=None, stride=1, pad=None, upsample=False, hout=None, wout=None, rowvec=None,
               rowvec_has_bias=False, residual=None, out=None, out_mode=0, scale=1.0, weight_per_image=False,
               w_group_stride=0, split_k=None, groups=1, defer=None, leaky=False):
        ops = self.ops
        x, x2, residual = ops.finished(x), ops.finished(x2), ops.finished(residual)
        if w_group_stride and not weight_per_image and groups == 1:
            raise NotImplementedError("launch shadow: a weight group stride without per-image weights or groups")
        n, hin, win, _ = x.shape
        ph, pw_ = (pw.kh // 2, pw.kw // 2) if pad is None else pad
        hl, wl = (hin * 2, win * 2) if upsample else (hin, win)
        ho = (hl + 2 * ph - pw.kh) // stride + 1 if hout is None else hout
        wo = (wl + 2 * pw_ - pw.kw) // stride + 1 if wout is None else wout
        cout, npk = (pw.cout // groups, pw.n_packed // groups) if groups > 1 else (pw.cout, pw.n_packed)
        w, ref_groups = pw.w, groups
        if weight_per_image:                 # image i times slab i of the tensor's own shape, not of the stride argument
            ref_groups = n
            try:
                w = per_image_weights(pw.w, n, npk, pw.kh * pw.kw * pw.cin, w_group_stride)
            except ValueError as e:
                self._fail(str(e))
                w = pw.w.reshape(n, npk, -1)
        op = dict(x=_snap(x), x2=_snap(x2), w=w, bias=pw.bias, kh=pw.kh, kw=pw.kw, stride=stride, pad_h=ph, pad_w=pw_,
                  upsample=upsample, hout=ho, wout=wo, cout=cout, n_packed=npk, groups=ref_groups, geglu=pw.geglu,
                  ln=pw.svec is not None, ln_eps=pw.ln_eps, scale=scale, rowvec=_snap(rowvec), rowvec_has_bias=rowvec_has_bias,
                  residual=None if residual is None else residual.detach().reshape(n, ho * wo, cout).clone(), leaky=leaky)
        ins = [("x", x, op["x"]), ("x2", x2, op["x2"]), ("rowvec", rowvec, op["rowvec"])]
        in_place = residual is not None and out is not None and residual.data_ptr() == out.data_ptr()
        if residual is not None and not in_place:
            ins.append(("residual", residual, residual.detach().clone()))
        wsnap = [pw.w.clone(), None if pw.bias is None else pw.bias.clone(), None if pw.svec is None else pw.svec.clone()]
        outside = OutsideView(out) if out is not None else None
        n0 = len(self.sink)
        y = orig(x, pw, x2=x2, stride=stride, pad=pad, upsample=upsample, hout=hout, wout=wout, rowvec=rowvec,
                 rowvec_has_bias=rowvec_has_bias, residual=residual, out=out, out_mode=out_mode, scale=scale, split_k=split_k,
                 groups=groups, defer=defer, weight_per_image=weight_per_image, w_group_stride=w_group_stride,
                 **({"leaky": True} if leaky else {}))
        torch.cuda.synchronize()
        self._count("igemm")
        tag = self._tag(n0, "igemm") + (" per_image" if weight_per_image else "")
        self._inputs_unchanged(tag, ins + [("weight", pw.w, wsnap[0]), ("bias", pw.bias, wsnap[1]), ("svec", pw.svec, wsnap[2])])
        if outside is not None and not outside.unchanged():
            self._fail(f"{tag}: wrote outside its out view")
        ref = igemm_reference(op)
        self._cpu_agree(tag, igemm_reference, op, ref, ref.shape[0] * ref.shape[1])
        dtype = x.dtype
        bound = bound_f32_rows(dtype) if out_mode == ops.OUT_ROWS_F32 else TOL[dtype]
        if isinstance(y, ops.Deferred):
            y._shadow = dict(ref=ref, tag=tag, bound=bound)
            self.pending[id(y)] = y
            return y
        got = y.transpose(1, 2) if out_mode == ops.OUT_TRANSPOSED else y.reshape(n, ho * wo, cout)
        form = dict(per_image=weight_per_image, out_mode=out_mode, upsample=upsample, stride=stride, pad=(ph, pw_), hin=hin,
                    win=win, hout=ho, wout=wo, cin=pw.cin, kh=pw.kh, kw=pw.kw, thin=self.thin.pop(x.data_ptr(), 0), leaky=leaky,
                    residual=residual is not None, k=pw.kh * pw.kw * pw.cin, m=n * ho * wo, images=n, split=_tag_int(tag, "split", 1),
                    src_strided=_img_strided(x), out_strided=out is not None and _img_strided(out),
                    res_strided=residual is not None and _img_strided(residual),
                    zero_spread=pw.kh == 3 and stride == 1 and min(hin, win) >= 2 and not bool(x[:, 1::2].any())
                    and not bool(x[:, :, 1::2].any()) and bool(x.any()))
        self._judge("igemm", tag, got, ref, bound, form=form,
                    detail=describe(x=x, x2=x2, w=pw.w, residual=residual, out=y) + f" images={n}")
        return y

    def _finish(self, orig, d):
        if d.done:
            return orig(d)
        n0 = len(self.sink)
        t = orig(d)
        torch.cuda.synchronize()
        self._count("split_finish")
        if self.pending.pop(id(d), None) is None:
            self._fail("a reduce launch of a split-K launch the shadow did not see")
            return t
        s = d._shadow
        d._shadow_finished = True
        self._judge("split_finish", self._tag(n0, "split_finish"), t.reshape(t.shape[0], -1, t.shape[3]), s["ref"], s["bound"],
                    extra=f"of [{s['tag']}]")
        return t

    # -- normalisation -------------------------------------------------------------------------------------------------
    def _groupnorm(self, orig, x, gamma, beta, eps, silu, x2=None, out_mode=0, dtype=None):
        ops = self.ops
        x2 = ops.finished(x2)
        d = x if isinstance(x, ops.Deferred) else None
        d_shape, d_dtype = (tuple(d.shape), d.dtype) if d is not None else (None, None)     # (tensor is dropped after "drop")
        snap = None if d is not None else _snap(x)
        x2s = _snap(x2)
        n0 = len(self.sink)
        y = orig(x, gamma, beta, eps, silu, x2=x2, out_mode=out_mode, dtype=dtype)
        torch.cuda.synchronize()
        self._count("groupnorm")
        tag = self._tag(n0, "groupnorm")
        extra = ""
        if d is not None:
            s = d._shadow
            if getattr(d, "_shadow_finished", False):          # the GroupNorm ran the reduce launch first (checked there)
                src = d.tensor
            else:                                              # it summed the slabs: against GroupNorm of the fp64 product
                self.pending.pop(id(d), None)
                src = s["ref"].reshape(d_shape)
                extra = f"slabs of [{s['tag']}]"
                if d.keep:
                    self._judge("igemm", s["tag"], d.tensor.reshape(s["ref"].shape), s["ref"], s["bound"], extra="summed by groupnorm")
            t_dtype = d_dtype
        else:
            src = x
            self._inputs_unchanged(tag, [("x", x, snap)])
            t_dtype = dtype if x.dtype == torch.float32 else x.dtype
        self._inputs_unchanged(tag, [("x2", x2, x2s)])
        op = dict(x=src, x2=x2s, gamma=gamma, beta=beta, eps=eps, silu=silu)
        ref = groupnorm_reference(op)
        self._cpu_agree(f"groupnorm {tag} {out_mode} {silu}", groupnorm_reference, op, ref, ref.shape[0] * ref.shape[1])
        n, c = ref.shape[0], ref.shape[2]
        y3 = y.reshape(n, ref.shape[1], -1)
        form = dict(out_mode=out_mode)
        if out_mode == ops.GN_OUT_T:
            self._judge("groupnorm", tag, y3, ref, TOL[t_dtype], extra, form=form)
        elif out_mode == ops.GN_OUT_F32:
            self._judge("groupnorm", tag, y3, ref, bound_gn_f32(t_dtype), extra + " f32", form=form)
        else:
            self._judge("groupnorm", tag, y3[..., :c].double() + y3[..., c:2 * c].double(), ref, bound_gn_split(t_dtype),
                        extra + " hi+lo", form=form)
            self._judge("groupnorm", tag, y3[..., :c], ref, TOL[t_dtype], extra + " hi", form=form)
            if out_mode == ops.GN_OUT_SPLIT3 and not torch.equal(y3[..., 2 * c:], y3[..., :c]):
                self._fail(f"groupnorm {tag}: SPLIT3's third part is not hi")
        return y

    def _layernorm(self, orig, x, gamma, beta, eps=1e-5):
        snap = _snap(x)
        y = orig(x, gamma, beta, eps)
        torch.cuda.synchronize()
        self._count("layernorm")
        tag = f"n={x.shape[0]} t={x.shape[1]} c={x.shape[2]} strided={int(not x.is_contiguous())}"
        self._inputs_unchanged(tag, [("x", x, snap)])
        op = dict(x=snap, gamma=gamma, beta=beta, eps=eps)
        ref = layernorm_reference(op)
        self._cpu_agree("layernorm " + tag, layernorm_reference, op, ref, ref.shape[0] * ref.shape[1])
        self._judge("layernorm", tag, y, ref, TOL[x.dtype])
        return y

    # -- attention -----------------------------------------------------------------------------------------------------
    def _attention(self, orig, q, k, v, heads, scale, v_rows=False, q_log2_scaled=False):
        snaps = [_snap(t) for t in (q, k, v)]
        n0 = len(self.sink)
        y = orig(q, k, v, heads, scale, v_rows=v_rows, q_log2_scaled=q_log2_scaled)
        torch.cuda.synchronize()
        self._count("attention")
        tag = self._tag(n0, "attention") + f" v_rows={int(v_rows)} log2q={int(q_log2_scaled)}"
        self._inputs_unchanged(tag, [("q", q, snaps[0]), ("k", k, snaps[1]), ("v", v, snaps[2])])
        op = dict(q=snaps[0], k=snaps[1], v=snaps[2], heads=heads, scale=scale, v_rows=v_rows, q_log2_scaled=q_log2_scaled)
        ref = attention_reference(op)
        self._cpu_agree("attention " + tag, attention_reference, op, ref, ref.shape[0] * ref.shape[1])
        self._judge("attention", tag, y, ref, TOL[q.dtype] * (1.0 if q_log2_scaled else 1.5))
        return y

    def _ctx_attention(self, orig, q, k, v, heads, scale):
        snaps = [_snap(t) for t in (q, k, v)]
        y = orig(q, k, v, heads, scale)
        torch.cuda.synchronize()
        self._count("ctx_attention")
        tag = f"n={q.shape[0]} tq={q.shape[1]} tk={k.shape[1]} heads={heads}"
        self._inputs_unchanged(tag, [("q", q, snaps[0]), ("k", k, snaps[1]), ("v", v, snaps[2])])
        op = dict(q=snaps[0], k=snaps[1], v=snaps[2], heads=heads, scale=scale)
        ref = ctx_attention_reference(op)
        self._cpu_agree("ctx_attention " + tag, ctx_attention_reference, op, ref, ref.shape[0] * ref.shape[1])
        self._judge("ctx_attention", tag, y, ref, TOL[q.dtype])
        return y

    # -- fused feed-forward, adapter -----------------------------------------------------------------------------------
    def _ff_geglu(self, orig, x, pf, residual=None, out=None, ln=None):
        xs = _snap(x)
        rs = xs if residual is not None and residual.data_ptr() == x.data_ptr() else _snap(residual)
        in_place = residual is not None and out is not None and residual.data_ptr() == out.data_ptr()
        bufs = pf.buf.clone()
        n0 = len(self.sink)
        y = orig(x, pf, residual=residual, out=out, ln=ln)
        torch.cuda.synchronize()
        self._count("ff_geglu")
        tag = self._tag(n0, "ff_geglu") + f" ln={int(ln is not None)} residual={int(residual is not None)}"
        ins = [("w_packed", pf.buf, bufs)]
        if not (out is not None and out.data_ptr() == x.data_ptr()):
            ins.append(("x", x, xs))
        if residual is not None and not in_place:
            ins.append(("residual", residual, rs))
        self._inputs_unchanged(tag, ins)
        op = dict(x=xs, residual=rs, b2=pf.b2, ln=ln, dec=decode_ff_geglu(bufs, pf.c, pf.hidden, pf.dtype))
        ref = ff_geglu_reference(op)
        self._cpu_agree("ff_geglu " + tag, ff_geglu_reference, op, ref, ref.shape[0] * ref.shape[1])
        self._judge("ff_geglu", tag, y.reshape(ref.shape), ref, TOL[x.dtype])
        return y

    def _two_key_adapter(self, orig, x, a, a_sum, c, u, b, eps, out=None, ln_pair=None):
        snaps = {k: _snap(t) for k, t in (("x", x), ("a", a), ("a_sum", a_sum), ("c", c), ("u", u), ("b", b))}
        outside = OutsideView(out) if out is not None else None
        r = orig(x, a, a_sum, c, u, b, eps, out=out, ln_pair=ln_pair)
        torch.cuda.synchronize()
        self._count("two_key_adapter")
        y, lns = (r, None) if ln_pair is None else r
        tag = f"n={x.shape[0]} t={x.shape[1]} c={x.shape[2]} in_place={int(out is not None)} ln_pair={int(ln_pair is not None)}"
        live = {"x": x, "a": a, "a_sum": a_sum, "c": c, "u": u, "b": b}
        self._inputs_unchanged(tag, [(k, live[k], snaps[k]) for k in snaps if not (k == "x" and out is not None
                                                                                      and out.data_ptr() == x.data_ptr())])
        if outside is not None and not outside.unchanged():
            self._fail(f"two_key_adapter {tag}: wrote outside its out view")
        op = dict(snaps, eps=eps)
        ref = two_key_adapter_op_reference(op)
        self._cpu_agree("two_key_adapter " + tag, two_key_adapter_op_reference, op, ref, ref.shape[0] * ref.shape[1])
        self._judge("two_key_adapter", tag, y, ref, TOL[x.dtype])
        if lns is not None:
            (g0, b0), (g1, b1), ln_eps = ln_pair
            for i, (got, g, bb) in enumerate(((lns[0], g0, b0), (lns[1], g1, b1))):
                want = layernorm_rows(ref[i::2], g, bb, ln_eps)
                self._judge("two_key_adapter", tag, got, want, TOL[x.dtype], extra=f"ln_pair[{i}]")
        return r

    # -- row chains ------------------------------------------------------------------------------------------------------
    def _chain_adapter_image(self, orig, a, c, u, b, dtype, out=None):
        snaps = dict(a=_snap(a), c=_snap(c), u=_snap(u), b=_snap(b))
        outside = OutsideView(out) if out is not None else None
        image = orig(a, c, u, b, dtype, out=out)
        torch.cuda.synchronize()
        self._count("chain_adapter_image")
        tag = f"chain_adapter_image n={a.shape[0]} heads={a.shape[1]}"
        self._inputs_unchanged(tag, [(k, t, snaps[k]) for k, t in (("a", a), ("c", c), ("u", u), ("b", b))])
        if outside is not None and not outside.unchanged():
            self._fail(f"{tag}: wrote outside its out view")
        self.adapter_images.append(dict(snaps, image=image.detach().clone(), dtype=dtype))      # judged through the launches that use it
        return image

    def adapter_tables(self, image, dtype):
        """The fp32 tables of the chain_adapter_image call whose image has this content (latest first), or None."""
        for rec in reversed(self.adapter_images):
            if rec["dtype"] == dtype and rec["image"].shape == image.shape and torch.equal(rec["image"], image):
                return rec
        return None

    def _groupnorm_scale_shift(self, orig, x, gamma, beta, eps):
        snap = _snap(x)
        scale, shift = orig(x, gamma, beta, eps)
        torch.cuda.synchronize()
        self._count("groupnorm_scale_shift")
        n, c = x.shape[0], x.shape[-1]
        tag = f"n={n} hw={x.numel() // (n * c)} c={c}"
        self._inputs_unchanged("groupnorm_scale_shift " + tag, [("x", x, snap)])
        op = dict(x=snap, x2=None, gamma=gamma, beta=beta, eps=eps, silu=False)
        ref = groupnorm_reference(op)
        self._cpu_agree("groupnorm_scale_shift " + tag, groupnorm_reference, op, ref, ref.shape[0] * ref.shape[1])
        got = snap.double().reshape(n, -1, c) * scale.double()[:, None, :] + shift.double()[:, None, :]
        self._judge("groupnorm_scale_shift", tag, got, ref, BOUND_GN_SCALE_SHIFT)
        return scale, shift

    def _row_chain(self, orig, programs, images, rows_per_image, dtype, adapter=None, flops=0.0, nbytes=0.0, note=""):
        what = f"row_chain {note}".strip()
        descs = [getattr(p, "desc", None) for p in programs]
        if any(d is None for d in descs):
            self._fail(f"{what}: a program that was not built through ops.ChainProgram while the shadow ran")
            descs = None
        tables = None
        if descs is not None:
            snaps, memo = chain_ref.snapshot(descs)
            if adapter is not None:
                image_before = adapter[0].detach().clone()
                rec = self.adapter_tables(image_before, dtype)
                if rec is None:
                    self._fail(f"{what}: the adapter image matches no chain_adapter_image call the shadow saw")
                else:
                    tables = dict(a=rec["a"], c=rec["c"], u=rec["u"], b=rec["b"], eps=adapter[1])
        orig(programs, images, rows_per_image, dtype, adapter=adapter, flops=flops, nbytes=nbytes, note=note)
        torch.cuda.synchronize()
        self._count("row_chain")
        if descs is None or (adapter is not None and tables is None):
            return
        tag = note.split()[0] if note.split() else "unnamed"
        dev = next(v.device for desc in descs for _, kw in desc for v in kw.values() if torch.is_tensor(v))
        results = chain_ref.run_launch(snaps, images, rows_per_image, dtype, tables, dev=dev)
        if not results:
            self._fail(f"{what}: the launch stores nothing")
        key = f"row_chain {tag} {len(descs)} programs"
        if self.cpu_check and key not in self.cpu_checked:
            self.cpu_checked.add(key)
            self._chain_cpu_agree(key, snaps, images, rows_per_image, dtype, tables, results)
        for rec in results:
            form = f"prog{rec['prog']} op{rec['index']} {rec['code']}"
            if rec["code"] == "product":
                form += " " + chain_ref.flag_name(rec["flags"])
            bound = TOL[dtype] * (1.5 if rec["code"] == "product" and rec["flags"] & 1 else 1.0)
            self._judge("row_chain", f"{tag} rows={images * rows_per_image}", chain_ref.as_images(chain_ref.stored_rows(rec), rows_per_image),
                        chain_ref.as_images(rec["ref"], rows_per_image), bound, extra=form,
                        form=dict(note=tag, code=rec["code"], flags=rec["flags"], programs=len(descs), images=images, rows=rows_per_image))
        for msg in chain_ref.changed_inputs(descs, snaps):
            self._fail(f"{what}: input changed: {msg}")
        for msg in chain_ref.touched_outside(results, memo):
            self._fail(f"{what}: {msg}")
        if adapter is not None and not torch.equal(adapter[0], image_before):
            self._fail(f"{what}: the adapter image changed")

    def _chain_cpu_agree(self, key, snaps, images, rows_per_image, dtype, tables, results):
        """First launch of a tag: 64 (image, row) pairs (first, last, 62 random) through the interpreter on the CPU."""
        total = images * rows_per_image
        rnd = torch.randperm(max(total - 2, 1), generator=self.gen)[:CPU_ROWS - 2] + 1
        flat = torch.unique(torch.cat([torch.tensor([0, total - 1]), rnd.clamp(max=total - 1)]))
        cpu = chain_ref.run_launch(snaps, images, rows_per_image, dtype, tables, sel=(flat // rows_per_image, flat % rows_per_image),
                                   dev=torch.device("cpu"))
        step = 1 if len(snaps) == 1 else 2
        for c, d in zip(cpu, results):
            pos = (c["img"] // step) * rows_per_image + c["row"]           # image-major over the images the program ran
            dref = d["ref"][pos.to(d["ref"].device)].cpu()
            err = float((c["ref"] - dref).norm() / c["ref"].norm().clamp_min(1e-300))
            if not err <= CPU_AGREE:
                self._fail(f"{key} prog{c['prog']} op{c['index']}: device fp64 reference disagrees with the CPU on {pos.numel()} rows: "
                           f"{err:.3e}")

    # -- the VAEs' entry points ------------------------------------------------------------------------------------------
    def _softmax_rows(self, orig, s, dtype):
        snap = _snap(s)
        y = orig(s, dtype)
        torch.cuda.synchronize()
        self._count("softmax_rows")
        rows, cols = snap.numel() // snap.shape[-1], snap.shape[-1]
        tag = f"rows={rows} cols={cols}"
        self._inputs_unchanged("softmax_rows " + tag, [("s", s, snap)])
        op = dict(s=snap.reshape(rows, cols))
        ref = softmax_reference(op)
        self._cpu_agree("softmax_rows " + tag, softmax_reference, op, ref, rows)
        got = y.reshape(rows, cols)
        self._judge("softmax_rows", tag, got.reshape(1, rows, cols), ref.reshape(1, rows, cols), TOL[dtype])
        dev = softmax_row_sums(got)
        if not dev < TOL[dtype]:
            self._fail(f"softmax_rows {tag}: a row sums to 1 +- {dev:.3e} (bound {TOL[dtype]:.1e})")
        return y

    def _split_f32(self, orig, x32, dtype, parts=2):
        snap = _snap(x32)
        y = orig(x32, dtype, parts)
        torch.cuda.synchronize()
        self._count("split_f32")
        c = snap.shape[-1]
        tag = f"rows={snap.numel() // c} c={c} parts={parts}"
        self._inputs_unchanged("split_f32 " + tag, [("x", x32, snap)])
        for msg in check_split(snap, y, parts, dtype):
            self._fail(f"split_f32 {tag}: {msg}")
        self._judge("split_f32", tag, (y[..., :c].double() + y[..., c:2 * c].double()).reshape(1, -1, c), snap.reshape(1, -1, c),
                    bound_gn_split(dtype), extra="hi+lo", form=dict(parts=parts))
        return y

    def _trunk_add(self, orig, trunk, inc, dtype):
        before, incs = _snap(trunk), _snap(inc)
        y = orig(trunk, inc, dtype)
        torch.cuda.synchronize()
        self._count("trunk_add")
        c = trunk.shape[-1]
        tag = f"n={trunk.numel()} inc={int(inc is not None)}"
        self._inputs_unchanged("trunk_add " + tag, [("inc", inc, incs)])
        for msg in check_trunk_add(before, incs, trunk, y, dtype):
            self._fail(f"trunk_add {tag}: {msg}")
        want = before.double() if incs is None else before.double() + incs.double()
        self._judge("trunk_add", tag, y.reshape(1, -1, c), want.reshape(1, -1, c), TOL[dtype], extra="16-bit copy")
        return y

    def _lincomb4(self, orig, es, cs):
        snaps = [_snap(e) for e in es]
        y = orig(es, cs)
        torch.cuda.synchronize()
        self._count("lincomb4")
        terms = [(e, float(c)) for e, c in zip(snaps, cs) if e is not None]
        tag = f"n={y.numel()} terms={len(terms)}"
        self._inputs_unchanged("lincomb4 " + tag, [(f"e{i}", e, s) for i, (e, s) in enumerate(zip(es, snaps))])
        if len(terms) == 2 and terms[0][1] == 1.0 and terms[1][1] == 1.0 and not _same(y, terms[0][0] + terms[1][0]):
            self._fail(f"lincomb4 {tag}: e0 + e1 is not the fp32 sum bit for bit")
        ref = sum(e.double() * c for e, c in terms)
        c = y.shape[-1]
        self._judge("lincomb4", tag, y.reshape(1, -1, c), ref.reshape(1, -1, c), BOUND_LINCOMB)
        return y

    def _conv_small_cout(self, orig, x, pw, pad=None, clamp=None):
        xs, ws, bs = _snap(x), pw.w.clone(), _snap(pw.bias)
        y = orig(x, pw, pad=pad, clamp=clamp)
        torch.cuda.synchronize()
        self._count("conv_small_cout")
        n, h, w, cin = x.shape
        ph, pw_ = (pw.kh // 2, pw.kw // 2) if pad is None else pad
        taps = ws.reshape(pw.cout, pw.kh * pw.kw, cin)
        dup = cin % 2 == 0 and torch.equal(taps[..., :cin // 2], taps[..., cin // 2:])
        tag = f"n={n} h={h} w={w} cin={cin} cout={pw.cout} tap={pw.kh}x{pw.kw} clamp={int(clamp is not None)} dup={int(dup)}"
        self._inputs_unchanged("conv_small_cout " + tag, [("x", x, xs), ("weight", pw.w, ws), ("bias", pw.bias, bs)])
        op = dict(x=xs, x2=None, w=ws, bias=bs, kh=pw.kh, kw=pw.kw, stride=1, pad_h=ph, pad_w=pw_, upsample=False, hout=h, wout=w,
                  cout=pw.cout, n_packed=pw.cout, groups=1, geglu=False, ln=False, ln_eps=0.0, scale=1.0, rowvec=None,
                  rowvec_has_bias=False, residual=None, clamp=clamp)
        ref = conv_small_cout_reference(op)
        self._cpu_agree("conv_small_cout " + tag, conv_small_cout_reference, op, ref, n * h * w)
        self._judge("conv_small_cout", tag, y.reshape(n, pw.cout, h * w).transpose(1, 2), ref, BOUND_SMALL_COUT,
                    form=dict(dup=dup, kh=pw.kh, kw=pw.kw, clamp=clamp is not None))
        return y

    def _conv_small_cin(self, orig, srcs, weight, bias, kh, kw, pad, dtype, out_f32_nchw=False):
        snaps = [_snap(s) for s in srcs]
        y = orig(srcs, weight, bias, kh, kw, pad, dtype, out_f32_nchw=out_f32_nchw)
        torch.cuda.synchronize()
        self._count("conv_small_cin")
        op = conv_small_cin_op(snaps, _snap(weight), _snap(bias), kh, kw, pad)
        n, h, w = op["x"].shape[:3]
        cout = weight.shape[0]
        tag = f"n={n} h={h} w={w} cin={op['x'].shape[3]} cout={cout} tap={kh}x{kw} f32_nchw={int(out_f32_nchw)}"
        self._inputs_unchanged("conv_small_cin " + tag, [(f"src{i}", s, t) for i, (s, t) in enumerate(zip(srcs, snaps))])
        ref = igemm_reference(op)
        self._cpu_agree("conv_small_cin " + tag, igemm_reference, op, ref, n * op["hout"] * op["wout"])
        got = y.reshape(n, cout, -1).transpose(1, 2) if out_f32_nchw else y.reshape(n, -1, cout)
        self._judge("conv_small_cin", tag, got, ref, BOUND_SMALL_CIN_F32 if out_f32_nchw else TOL[dtype])
        return y

    def _pack_sources(self, orig, srcs, dtype, c_pad=32):
        snaps = [_snap(s) for s in srcs]
        y = orig(srcs, dtype, c_pad)
        torch.cuda.synchronize()
        self._count("pack_sources")
        cat = torch.cat(snaps, dim=1).permute(0, 2, 3, 1)
        c = cat.shape[3]
        tag = f"n={cat.shape[0]} hw={cat.shape[1] * cat.shape[2]} sources={len(srcs)} c={c} c_pad={c_pad}"
        self._inputs_unchanged("pack_sources " + tag, [(f"src{i}", s, t) for i, (s, t) in enumerate(zip(srcs, snaps))])
        if not (_same(y[..., :c], cat.to(dtype)) and not bool(y[..., c:].any())):
            self._fail(f"pack_sources {tag}: not the rounded sources followed by zeros, bit for bit")
        self.thin[y.data_ptr()] = len(srcs)
        self._judge("pack_sources", tag, y.reshape(1, -1, c_pad), F.pad(cat, (0, c_pad - c)).reshape(1, -1, c_pad), TOL[dtype])
        return y

    # -- the conditioning producer's and the realism networks' entry points (extra=...) ------------------------------------
    def _judge_value(self, kind, tag, err, bound, finite=True, form=None):
        """A launch whose unit test bounds one figure (a maximum over its outputs), not a rel-L2 over tiles."""
        ok = finite and err <= bound
        self.records.append(dict(kind=kind, tag=tag, bound=bound, extra="", form=form or {}, rel=err, tile=err, where=(0, 0, 0),
                                 finite=finite))
        record(f"shadow {self.label} {kind} {tag}", err, bound)
        if self.verbose:
            print(f"[shadow {self.label}] {kind:16s} {tag} err={err:.3e} bound={bound:.1e}{'' if ok else '  FAIL'}")
        if not ok:
            self._fail(f"{kind} {tag}: error {err:.3e}, finite {finite} (bound {bound:.1e})")

    def _judge_exact(self, kind, tag, got, want, form=None):
        """A launch whose contract is bit-exact: torch.equal against the torch restatement its unit test uses."""
        ok = got.shape == want.shape and got.dtype == want.dtype and torch.equal(got, want)
        self.records.append(dict(kind=kind, tag=tag, bound=0.0, extra="", form=form or {}, rel=0.0 if ok else float("inf"),
                                 tile=0.0 if ok else float("inf"), where=(0, 0, 0), finite=bool(torch.isfinite(got).all())))
        if self.verbose:
            print(f"[shadow {self.label}] {kind:16s} {tag} bit-exact{'' if ok else '  FAIL'}")
        if not ok:
            diff = int((got != want).sum()) if got.shape == want.shape else -1
            self._fail(f"{kind} {tag}: not the torch restatement bit for bit ({diff} elements differ)")

    def _skinny_linear(self, orig, x, w, bias=None, pre_act=0, post_act=0, out=None):
        xs, ws, bs = _snap(x), _snap(w), _snap(bias)
        outside = OutsideView(out) if out is not None else None
        y = orig(x, w, bias=bias, pre_act=pre_act, post_act=post_act, out=out)
        torch.cuda.synchronize()
        m, k = xs.shape
        n = ws.shape[0]
        self._count("skinny_linear", (m + 15) // 16)                  # one library call per 16 rows
        tag = f"m={m} k={k} n={n} pre={pre_act} post={post_act} bias={int(bias is not None)}"
        self._inputs_unchanged("skinny_linear " + tag, [("x", x, xs), ("weight", w, ws), ("bias", bias, bs)])
        if outside is not None and not outside.unchanged():
            self._fail(f"skinny_linear {tag}: wrote outside its out view")
        act = {0: lambda t: t, 1: F.silu, 2: F.gelu}
        ref = act[pre_act](xs.double()) @ ws.double().T
        if bs is not None:
            ref = ref + bs.double()
        ref = act[post_act](ref)
        bound = BOUND_SKINNY_SILU if 1 in (pre_act, post_act) else BOUND_SKINNY
        self._judge("skinny_linear", tag, y.reshape(1, m, n), ref.reshape(1, m, n), bound,
                    form=dict(m=m, k=k, n=n, remainder=m % 16, calls=(m + 15) // 16))
        return y

    def _layernorm_rows_f32(self, orig, x, gamma, beta, eps=1e-5):
        xs, gs, bs = _snap(x), _snap(gamma), _snap(beta)
        y = orig(x, gamma, beta, eps)
        torch.cuda.synchronize()
        self._count("layernorm_rows_f32")
        tag = f"rows={xs.shape[0]} cols={xs.shape[1]}"
        self._inputs_unchanged("layernorm_rows_f32 " + tag, [("x", x, xs), ("gamma", gamma, gs), ("beta", beta, bs)])
        ref = layernorm_rows(xs, gs, bs, eps)
        self._judge("layernorm_rows_f32", tag, y.reshape(1, *y.shape), ref.reshape(1, *ref.shape), BOUND_F32_ROWS)
        return y

    def _linear_f32(self, orig, x, w, bias=None):
        xs, ws, bs = _snap(x), _snap(w), _snap(bias)
        y = orig(x, w, bias)
        torch.cuda.synchronize()
        self._count("linear_f32")
        tag = f"m={xs.shape[0]} k={xs.shape[1]} n={ws.shape[0]} bias={int(bias is not None)}"
        self._inputs_unchanged("linear_f32 " + tag, [("x", x, xs), ("weight", w, ws), ("bias", bias, bs)])
        ref = xs.double() @ ws.double().T
        if bs is not None:
            ref = ref + bs.double()
        self._judge("linear_f32", tag, y.reshape(1, *y.shape), ref.reshape(1, *ref.shape), BOUND_F32_ROWS,
                    form=dict(m=xs.shape[0], k=xs.shape[1], n=ws.shape[0]))
        return y

    def _quick_gelu(self, orig, x):
        xs = _snap(x)
        y = orig(x)
        torch.cuda.synchronize()
        self._count("quick_gelu")
        c = xs.shape[-1]
        tag = f"n={xs.numel()} c={c}"
        self._inputs_unchanged("quick_gelu " + tag, [("x", x, xs)])
        if y.shape != xs.shape or y.dtype != xs.dtype:
            self._fail(f"quick_gelu {tag}: shape / dtype {tuple(y.shape)} {y.dtype}")
            return y
        x64 = xs.double()
        ref = x64 * torch.sigmoid(QUICK_GELU_ALPHA * x64)
        # one rounding of the fp32 value to T: every element within the unit roundoff, hence the whole tensor and every tile
        self._judge("quick_gelu", tag, y.reshape(1, -1, c), ref.reshape(1, -1, c), UNIT_ROUNDOFF[xs.dtype], tile_factor=1.0,
                    form=dict(n=xs.numel()))
        return y

    def _image_normalize(self, orig, x, shift, scale, dtype=None, nhwc_channels=0):
        xs = _snap(x)
        y = orig(x, shift, scale, dtype=dtype, nhwc_channels=nhwc_channels)
        torch.cuda.synchronize()
        self._count("image_normalize")
        n, c, h, w = xs.shape
        tag = f"n={n} c={c} hw={h}x{w} nhwc={nhwc_channels}"
        self._inputs_unchanged("image_normalize " + tag, [("x", x, xs)])
        sh = torch.tensor(shift, device=xs.device).view(1, c, 1, 1)
        sc = torch.tensor(scale, device=xs.device).view(1, c, 1, 1)
        want = (xs - sh) / sc
        if nhwc_channels:
            want = F.pad(want.to(dtype).permute(0, 2, 3, 1), (0, nhwc_channels - c)).contiguous()
        self._judge_exact("image_normalize", tag, y, want, form=dict(nhwc=nhwc_channels))
        return y

    def _maxpool3s2(self, orig, x, relu=False):
        xs = _snap(x)
        y = orig(x, relu=relu)
        torch.cuda.synchronize()
        self._count("maxpool3s2")
        tag = f"n={xs.shape[0]} hw={xs.shape[1]}x{xs.shape[2]} c={xs.shape[3]} relu={int(relu)}"
        self._inputs_unchanged("maxpool3s2 " + tag, [("x", x, xs)])
        src = torch.relu(xs) if relu else xs
        want = F.max_pool2d(src.permute(0, 3, 1, 2).float(), 3, 2).to(xs.dtype).permute(0, 2, 3, 1).contiguous()
        self._judge_exact("maxpool3s2", tag, y, want, form=dict(relu=relu))
        return y

    def _add(self, orig, a, b):
        sa, sb = _snap(a), _snap(b)
        y = orig(a, b)
        torch.cuda.synchronize()
        self._count("add")
        tag = f"n={sa.numel()}"
        self._inputs_unchanged("add " + tag, [("a", a, sa), ("b", b, sb)])
        self._judge_exact("add", tag, y, (sa.float() + sb.float()).to(sa.dtype))
        return y

    def _lpips_distance(self, orig, feat, lin, out, eps=1e-10, relu_in_place=False):
        fs, ls_, base = _snap(feat), _snap(lin), _snap(out)
        outside = OutsideView(out)
        y = orig(feat, lin, out, eps, relu_in_place=relu_in_place)
        torch.cuda.synchronize()
        self._count("lpips_distance")
        n2, h, w, c = fs.shape
        p = n2 // 2
        tag = f"pairs={p} hw={h}x{w} c={c} relu_in_place={int(relu_in_place)}"
        self._inputs_unchanged("lpips_distance " + tag, [("lin", lin, ls_)])
        if not _same(feat, torch.relu(fs) if relu_in_place else fs):
            self._fail(f"lpips_distance {tag}: the features are not " + ("relu(features) bit for bit" if relu_in_place else "unchanged"))
        if not outside.unchanged():
            self._fail(f"lpips_distance {tag}: wrote outside its out view")
        f64 = torch.relu(fs.double()).permute(0, 3, 1, 2)

        def unit(f):
            return f / (torch.sqrt((f * f).sum(dim=1, keepdim=True)) + eps)
        d = (unit(f64[:p]) - unit(f64[p:])).square() * ls_.double().view(1, -1, 1, 1)
        want = base.double() + d.sum(1).mean(dim=(1, 2))
        got = y.double()
        err = (got - want).abs() / want.abs().clamp_min(1e-300)
        err = torch.where((want == 0) & (got == 0), torch.zeros_like(err), err)
        self._judge_value("lpips_distance", tag, float(err.max()), BOUND_LPIPS_DISTANCE, bool(torch.isfinite(got).all()),
                          form=dict(relu_in_place=relu_in_place, pairs=p))
        return y

    def _row_cosine(self, orig, a, b, eps=1e-8, scale=1.0):
        sa, sb = _snap(a), _snap(b)
        y = orig(a, b, eps=eps, scale=scale)
        torch.cuda.synchronize()
        self._count("row_cosine")
        tag = f"rows={sa.shape[0]} d={sa.shape[1]}"
        self._inputs_unchanged("row_cosine " + tag, [("a", a, sa), ("b", b, sb)])
        want = scale * F.cosine_similarity(sa.double(), sb.double(), dim=-1, eps=eps)
        err = ((y.double() - want).abs() / want.abs().clamp_min(1.0)).max()
        self._judge_value("row_cosine", tag, float(err), BOUND_ROW_COSINE, bool(torch.isfinite(y).all()))
        return y

    def _feature_moments(self, orig, feat, shift, sum_, cross=None):
        fs, ss, s0, c0 = _snap(feat), _snap(shift), _snap(sum_), _snap(cross)
        r = orig(feat, shift, sum_, cross)
        torch.cuda.synchronize()
        self._count("feature_moments")
        rows, d = fs.shape
        tag = f"rows={rows} d={d} shift={int(shift is not None)} cross={int(cross is not None)}"
        self._inputs_unchanged("feature_moments " + tag, [("feat", feat, fs), ("shift", shift, ss)])
        x = fs.double() if ss is None else fs.double() - ss
        # increments against fp64, each relative to the size of what was summed (the shifted sum itself is near 0)
        e_sum = float(((sum_ - s0) - x.sum(0)).abs().max() / x.abs().sum(0).max().clamp_min(1e-300))
        finite = bool(torch.isfinite(sum_).all())
        self._judge_value("feature_moments", tag + " sum", e_sum, BOUND_MOMENTS, finite, form=dict(shift=shift is not None))
        if cross is not None:
            want = x.T @ x
            e_cross = float(((cross.reshape(d, d) - c0.reshape(d, d)) - want).abs().max() / want.abs().max().clamp_min(1e-300))
            self._judge_value("feature_moments", tag + " cross", e_cross, BOUND_MOMENTS, bool(torch.isfinite(cross).all()),
                              form=dict(shift=shift is not None))
        return r

    def _frd_input(self, orig, raw, dtype, hout=64, wout=1024, cpad=32, depth_min=1.4, depth_max=54.0):
        from tests import frd_ref
        rs = _snap(raw)
        y = orig(raw, dtype, hout, wout, cpad, depth_min, depth_max)
        torch.cuda.synchronize()
        self._count("frd_input")
        n = rs.shape[0]
        tag = f"n={n} hw={rs.shape[2]}x{rs.shape[3]} -> {hout}x{wout}x{cpad}"
        self._inputs_unchanged("frd_input " + tag, [("raw", raw, rs)])
        if (depth_min, depth_max) != tuple(frd_ref.FRD_DEPTH):
            self._fail(f"frd_input {tag}: depth range {(depth_min, depth_max)} is not the reference's {frd_ref.FRD_DEPTH}")
            return y
        want = torch.stack([frd_ref.prepare(v, hout, wout) for v in rs.cpu().double().numpy()])       # f32 [n, 5, hout, wout]
        got = y.cpu()
        g5 = got[..., :5].permute(0, 3, 1, 2)
        bad = []
        if tuple(got.shape) != (n, hout, wout, cpad) or got.dtype != dtype:
            bad.append(f"shape / dtype {tuple(got.shape)} {got.dtype}")
        elif bool(got[..., 5:].any()):
            bad.append("the padding channels are not zero")
        elif not torch.equal(~(g5 == -1).all(1), ~(want == -1).all(1)):
            bad.append("the validity mask differs from the reference's")
        ulps = float("inf")
        if not bad:
            wt = want.to(dtype)
            ulp = torch.nextafter(wt.float().abs().to(dtype), torch.tensor(float("inf")).to(dtype)).float() - wt.float().abs()
            ulps = float(((g5.float() - wt.float()).abs() / ulp).max())
        for msg in bad:
            self._fail(f"frd_input {tag}: {msg}")
        self._judge_value("frd_input", tag, ulps, 1.0, bool(torch.isfinite(got.float()).all()))
        return y

    def _band_mean(self, orig, x, skip=None, bands=16):
        xs, ss = _snap(x), _snap(skip)
        y = orig(x, skip, bands)
        torch.cuda.synchronize()
        self._count("band_mean")
        n, h, w, c = xs.shape
        tag = f"n={n} hw={h}x{w} c={c} bands={bands} skip={int(skip is not None)}"
        self._inputs_unchanged("band_mean " + tag, [("x", x, xs), ("skip", skip, ss)])
        t = xs.double() if ss is None else xs.double() + ss.double()
        want = t.permute(0, 3, 1, 2).reshape(n, c, bands, h // bands, w).mean((3, 4)).reshape(n, -1)
        err = float((y.double() - want).abs().max() / want.abs().max().clamp_min(1e-300))
        self._judge_value("band_mean", tag, err, BOUND_BAND_MEAN, bool(torch.isfinite(y).all()), form=dict(skip=skip is not None))
        return y


    # -- the training step's entry points (extra=TRAIN_KINDS) --------------------------------------------------------------
    def _apply(self, kind, tag, checks, form=None):
        """Records and judges the Check records of one launch (one record per output)."""
        ordinal = self.counts.get(kind, 0)
        checks = list(checks)
        for i, ck in enumerate(checks):
            name = f"{kind} #{ordinal} {ck.what}"
            if name in self.pinned:
                self.pins_used.add(name)
                checks[i] = ck = ck._replace(bound=self.pinned[name])
            res = evaluate(ck)
            self.records.append(dict(kind=kind, tag=tag, bound=ck.bound, extra=ck.what, form=form or {}, rel=res["rel"], tile=res["tile"],
                                     where=res["where"], finite=res["finite"], row=res["row"], pinned=name if name in self.pinned else None))
            if ck.mode in ("tiles", "value", "figure"):
                record(f"shadow {self.label} {kind} {tag} {ck.what}", res["rel"], ck.bound)
            if res["row"] is not None:
                record(f"shadow {self.label} {kind} {tag} {ck.what} row_measure", res["row"])
            if self.verbose:
                row = "" if res["row"] is None else f" row={res['row']:.3e}"
                print(f"[shadow {self.label}] {kind:16s} {tag} {ck.what} rel={res['rel']:.3e} tile={res['tile']:.3e}{row} "
                      f"bound={ck.bound:.1e}{'' if res['ok'] else '  FAIL'}")
        for msg in check_failures(kind, tag, checks):
            self._fail(msg)

    def _host_unchanged(self, what, pairs):
        for name, live, snap in pairs:
            if live is not None and not _same(live.detach().cpu(), snap):
                self._fail(f"{what}: input {name} changed")

    def _transpose(self, orig, x):
        xs = _host(x)
        y = orig(x)
        torch.cuda.synchronize()
        self._count("transpose")
        tag = describe(x=x)
        self._host_unchanged("transpose " + tag, [("x", x, xs)])
        self._apply("transpose", tag, transpose_checks(xs, _host(y)), form=dict(rows=x.shape[0], cols=x.shape[1]))
        return y

    def _colsum(self, orig, dy):
        ds = _host(dy)
        y = orig(dy)
        torch.cuda.synchronize()
        self._count("colsum")
        tag = describe(dy=dy)
        self._host_unchanged("colsum " + tag, [("dy", dy, ds)])
        self._apply("colsum", tag, colsum_checks(ds, _host(y)), form=dict(rows=dy.shape[0], blocks=R.partial_blocks(dy.shape[0])))
        return y

    def _layernorm_bwd(self, orig, x, dy, gamma, eps, dx_add=None):
        xs, ds, gs, adds = _host(x), _host(dy), _host(gamma), _host(dx_add)
        dx, dg, db = orig(x, dy, gamma, eps, dx_add=dx_add)
        torch.cuda.synchronize()
        self._count("layernorm_bwd")
        tag = describe(x=x, dy=dy, dx_add=dx_add)
        self._host_unchanged("layernorm_bwd " + tag, [("x", x, xs), ("dy", dy, ds), ("gamma", gamma, gs), ("dx_add", dx_add, adds)])
        self._apply("layernorm_bwd", tag, layernorm_bwd_checks(xs, ds, gs, eps, adds, _host(dx), _host(dg), _host(db)),
                    form=dict(images=x.shape[0], x_strided=_img_strided(x), dy_strided=_img_strided(dy), dx_add=dx_add is not None))
        return dx, dg, db

    def _groupnorm_bwd(self, orig, x, dy, gamma, beta, eps, silu, dx_add=None, one_block_per_group=False):
        xs, ds, gs, bs, adds = _host(x), _host(dy), _host(gamma), _host(beta), _host(dx_add)
        dx = orig(x, dy, gamma, beta, eps, silu, dx_add=dx_add, one_block_per_group=one_block_per_group)
        torch.cuda.synchronize()
        self._count("groupnorm_bwd")
        tag = describe(x=x, dx_add=dx_add) + f" silu={int(silu)} one_block={int(one_block_per_group)}"
        self._host_unchanged("groupnorm_bwd " + tag, [("x", x, xs), ("dy", dy, ds), ("gamma", gamma, gs), ("beta", beta, bs),
                                                      ("dx_add", dx_add, adds)])
        self._apply("groupnorm_bwd", tag, groupnorm_bwd_checks(xs, ds, gs, bs, eps, silu, adds, _host(dx)),
                    form=dict(silu=bool(silu), dx_add=dx_add is not None, c=x.shape[-1]))
        return dx

    def _geglu_fwd(self, orig, pre):
        ps = _host(pre)
        h = orig(pre)
        torch.cuda.synchronize()
        self._count("geglu_fwd")
        tag = describe(pre=pre)
        self._host_unchanged("geglu_fwd " + tag, [("pre", pre, ps)])
        self._apply("geglu_fwd", tag, geglu_fwd_checks(ps, _host(h)))
        return h

    def _geglu_bwd(self, orig, pre, dh):
        ps, ds = _host(pre), _host(dh)
        dpre = orig(pre, dh)
        torch.cuda.synchronize()
        self._count("geglu_bwd")
        tag = describe(pre=pre, dh=dh)
        self._host_unchanged("geglu_bwd " + tag, [("pre", pre, ps), ("dh", dh, ds)])
        self._apply("geglu_bwd", tag, geglu_bwd_checks(ps, ds, _host(dpre)))
        return dpre

    def _attention_bwd(self, orig, q, k, v, o, dout, heads, scale, force_vector=False):
        live = dict(q=q, k=k, v=v, o=o, dout=dout)
        snaps = {nm: _host(t) for nm, t in live.items()}
        dq, dk, dv = orig(q, k, v, o, dout, heads, scale, force_vector=force_vector)
        torch.cuda.synchronize()
        self._count("attention_bwd")
        c = o.shape[2]
        dh = c // heads
        route = R.attention_bwd_route(dh, [s for t in live.values() for s in (t.stride(0), t.stride(1))],
                                      [t.data_ptr() for t in live.values()], force_vector)
        tag = f"#{self.counts['attention_bwd']} heads={heads} dh={dh} route={route} " + describe(**live)
        self._host_unchanged("attention_bwd " + tag, [(nm, live[nm], snaps[nm]) for nm in live])
        ops_ = (snaps["q"][..., :c], snaps["k"][..., :c], snaps["v"][..., :c], snaps["dout"])
        checks = attention_bwd_checks(*ops_, heads, scale, route, _host(dq), _host(dk), _host(dv))
        nfail = len(self.failures)
        form = dict(route=route, dh=dh, tq=q.shape[1], tk=k.shape[1], images=q.shape[0])
        if any(name.startswith(f"attention_bwd #{self.counts['attention_bwd']} ") for name in self.pinned):
            rs = R.attention_bwd_restated(*ops_, heads, scale, q.dtype, route)           # recorded beside the pinned bound
            form["restated"] = {ck.what: R.rel_l2(g, ck.ref) for ck, g in zip(checks, rs)}
        self._apply("attention_bwd", tag, checks, form=form)
        if len(self.failures) > nfail:              # what the operands say: the storage restatements on them, their range, the keys' offset
            self.failures[-1] += " [" + attention_bwd_diagnosis(*ops_, heads, scale, q.dtype, [ck.ref for ck in checks]) + "]"
        return dq, dk, dv

    def _sumpool2(self, orig, src):
        ss = _host(src)
        y = orig(src)
        torch.cuda.synchronize()
        self._count("sumpool2")
        tag = describe(src=src)
        self._host_unchanged("sumpool2 " + tag, [("src", src, ss)])
        self._apply("sumpool2", tag, sumpool2_checks(ss, _host(y)))
        return y

    def _silu_bwd_f32(self, orig, z, dy):
        zs, ds = _host(z), _host(dy)
        dx = orig(z, dy)
        torch.cuda.synchronize()
        self._count("silu_bwd_f32")
        tag = describe(z=z)
        self._host_unchanged("silu_bwd_f32 " + tag, [("z", z, zs), ("dy", dy, ds)])
        self._apply("silu_bwd_f32", tag, silu_bwd_f32_checks(zs, ds, _host(dx)))
        return dx

    def _loss_grad(self, orig, eps, target, t, logvar, lvlb, loss_type="l2", l_simple_weight=1.0, elbo_weight=0.0, loss_scale=1.0,
                   dtype=None, c_pad=32):
        from mobi_amd import engine_dtype
        live = dict(eps=eps, target=target, t=t, logvar=logvar, lvlb=lvlb)
        snaps = {nm: _host(v) for nm, v in live.items()}
        kw = dict(loss_type=loss_type, l_simple_weight=l_simple_weight, elbo_weight=elbo_weight, loss_scale=loss_scale)
        dy, per_sample, terms = orig(eps, target, t, logvar, lvlb, dtype=dtype, c_pad=c_pad, **kw)
        torch.cuda.synchronize()
        self._count("loss_grad")
        dtype = engine_dtype() if dtype is None else dtype
        tag = f"{loss_type} scale={loss_scale:g} " + describe(eps=eps)
        self._host_unchanged("loss_grad " + tag, [(nm, live[nm], snaps[nm]) for nm in live])
        self._apply("loss_grad", tag, loss_grad_checks(*(snaps[nm] for nm in ("eps", "target", "t", "logvar", "lvlb")), kw, dtype, c_pad,
                                                       _host(dy), _host(per_sample), _host(terms)),
                    form=dict(loss_type=loss_type, loss_scale=loss_scale))
        self.thin[dy.data_ptr()] = 1                # (the thin 32-channel pack the head's data gradient reads)
        return dy, per_sample, terms

    def _timestep_embedding(self, orig, t, freqs):
        ts, fs = _host(t), _host(freqs)
        y = orig(t, freqs)
        torch.cuda.synchronize()
        self._count("timestep_embedding")
        tag = f"n={t.shape[0]} dim={2 * freqs.shape[0]}"
        self._host_unchanged("timestep_embedding " + tag, [("t", t, ts), ("freqs", freqs, fs)])
        self._apply("timestep_embedding", tag, timestep_embedding_checks(ts, fs, _host(y)))
        return y
