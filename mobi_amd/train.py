"""The training step of the adapter parameters on the engine: forward WITH a tape and the backward
pass through the WHOLE UNet -- every tensor the reference's optimizer filter selects (`cond_adapter*`, `cross_modal*`:
ldm/models/diffusion/ddpm.py:1616-1629 of the reference; 27 tensors in each of the 16 transformer blocks = 432 tensors,
180 M parameters at full width) gets its gradient.  ldm/modules/attention.py:230-266 and
ldm/modules/diffusionmodules/openaimodel.py:255-275, 861-898 are what is differentiated; torch.autograd does this for the
reference, Lightning's DDP all-reduces the result (main.py:510).

What runs where: the products -- y = x W^T, dx = dy W, dW = dy^T x, and the data gradients of the 3 x 3 / strided /
upsampling convolutions (the kernel rotated by 180 degrees with its in / out axes swapped; stride 2: dy spread onto the even
pixels first; nearest x2: 2 x 2 sums after) -- are mobi_igemm launches; LayerNorm, GroupNorm (+ SiLU), GEGLU and attention
have backward kernels of their own (csrc/backward.hip: correct and bit-reproducible, NOT tuned: fp32 vector arithmetic).
The training forward is the UN-folded sequence: the sampling path's algebra (two-key adapter tables, connector o to_out,
LayerNorm folded into to_q, the row chains, the un-materialised skip concat) bakes trainable weights into per-run constants
or hides tensors the backward pass needs, and has no place here.  Frozen layers only pass the data gradient on.

Pinned to torch.autograd through the CPU oracle (tests/test_gpu_backward.py): one block, and the reduced UNet end to end.
Also here: the conditioning stage's trainable part (the 3-D box embedder, `bbox_uncond_vector`: ddpm.py:1635-1647) and AdamW.
The objective is every one `p_losses` can express with the eps-parameterisation (ddpm.py:1189-1216): l2 or l1, `l_simple_weight`,
the variational-bound term (`original_elbo_weight` x `lvlb_weights[t]`) and a per-timestep `logvar` table -- `mobi_loss_grad`
(csrc/loss.hip) reads eps and the target once and writes the three loss terms and the gradient that enters `unet_backward`, in the
layout its first launch reads, gathering the tables by the device-resident t: no torch arithmetic, no read-back.
Not built: optimising `logvar` (`learn_logvar`: the table is fixed, honoured but not trained), the x0 parameterisation, activation
checkpointing (the tape of a full-width step at 64 x 64 x 4 is 17 GB: fine in 288 GB).
`mobi_amd.dist.allreduce_gradients` is the gradient collective (bucketed, RCCL; gloo on CPU in the tests).
"""
import math

import torch

from . import engine_dtype, ops
from .ops import Packed
from .ldm.modules.diffusionmodules.util import weights_changed

TRAINABLE_MARKERS = ("cond_adapter", "lidar", "cross_modal")          # ddpm.py:1622-1626 of the reference


def trainable_names(module):
    """Parameter names the reference's `configure_optimizers` would hand to AdamW (ddpm.py:1616-1633), relative to `module`."""
    return [n for n, _ in module.named_parameters() if any(m in n for m in TRAINABLE_MARKERS)]


def _packed_t(lin):
    """The layer's weight read as [in][out]: `dx = dy W` is then an ordinary linear launch (no bias)."""
    key = (lin.weight._version, lin.weight.data_ptr(), engine_dtype())
    c = lin.__dict__.setdefault("_packed_t", {})
    if c.get("key") != key:
        c["key"], c["val"] = key, ops.pack_linear(lin.weight.detach().t().contiguous(), None, engine_dtype(), lin.weight.device)
    return c["val"]


# `block_backward` sends the data gradient of the bbox adapter's to_k / to_v (a handful of context rows) through fp32 chains
# on the master weight: their `_packed_t` is never read
_NO_PACKED_T = ("cond_adapter_attn.to_k", "cond_adapter_attn.to_v")


class WeightRefresher:
    """The 16-bit copies of every trained Linear weight, rebuilt by ONE launch after an optimizer update (`mobi_repack_multi`)
    instead of lazily, tensor by tensor, by the next forward / backward (`ops.pack_linear`, `_packed_t`: a cast, an allocation
    and a `mobi_tile_weights` launch each, twice per layer).  names: the parameter names an optimizer steps, relative to `model`.
    Of those, every `Linear` weight is listed with the copies the training step reads: inside a `BBoxEmbedder` the cast alone
    (`Linear.skinny()`), elsewhere `Linear.packed()` (w, wt, the fp32 bias alias) and `_packed_t` (the transposed pair; not for
    `_NO_PACKED_T`, whose data gradient never reads one).
    `refresh()` launches on the current stream and then re-keys the layers' caches (`_Holder._install`, the `_packed_t` dict) on
    the parameters' current versions: the next `packed()` / `_packed_t()` is a hit that returns `ops.Packed` objects over the
    table's persistent buffers.  The table is rebuilt when the engine dtype or a parameter's address has moved.  A cache
    something else invalidates later (an `ema_scope` swap) is rebuilt lazily by the old path and re-installed at the next
    `refresh()`; the sampling path's folded tables are not touched."""

    def __init__(self, model, names):
        from .ldm.modules.diffusionmodules.util import Linear
        from .ldm.modules.encoders.modules import BBoxEmbedder
        skinny = {id(m) for e in model.modules() if isinstance(e, BBoxEmbedder) for m in e.modules()}
        self.layers = []                              # (Linear, "mfma" | "forward" | "skinny")
        for name in names:
            prefix, _, leaf = name.rpartition(".")
            if leaf != "weight" or not prefix:
                continue
            mod = model.get_submodule(prefix)
            if isinstance(mod, Linear):
                kind = "skinny" if id(mod) in skinny else "forward" if prefix.endswith(_NO_PACKED_T) else "mfma"
                self.layers.append((mod, kind))
        self.table = self._key = None
        self.launches = 0

    def _now(self):
        return (engine_dtype(),) + tuple(m.weight.data_ptr() for m, _ in self.layers)

    def refresh(self):
        if not self.layers:
            return
        key = self._now()
        if self.table is None or key != self._key:
            want = {"mfma": (True, True), "forward": (True, False), "skinny": ("cast", False)}
            self.table = ops.RepackTable([(m.weight.data, *want[kind]) for m, kind in self.layers], engine_dtype())
            self._key = key
        ops.repack_multi(self.table)
        self.launches += 1
        dt = engine_dtype()
        for (m, kind), im in zip(self.layers, self.table.images):
            w = m.weight
            b = None if m.bias is None else m.bias.detach().float().contiguous()
            if kind == "skinny":
                m._install("skinny", (im["w"], b))
                continue
            n, k = w.shape
            m._install("mfma", Packed(im["w"], b, 1, 1, k, n, n, wt=im["wt"]))
            if kind == "forward":
                continue
            c = m.__dict__.setdefault("_packed_t", {})
            c["key"], c["val"] = (w._version, w.data_ptr(), dt), Packed(im["w_t"], None, 1, 1, n, k, k, wt=im["wt_t"])


def _rows(t):
    return t.reshape(-1, t.shape[-1])


def _dgrad(dy, lin, residual=None, out=None):
    return ops.linear(dy, _packed_t(lin), residual=residual, out=out)


def _wgrad(grads, name, lin, dy, x):
    """dW (and db) of `y = lin(x)` into grads[name + '.weight' / '.bias'] (fp32)."""
    grads[name + ".weight"] = ops.linear_wgrad(_rows(dy), _rows(x))
    if lin.bias is not None:
        grads[name + ".bias"] = ops.colsum(_rows(dy))


class BlockTape:
    """Activations one block's backward pass reads (kept in the engine's 16-bit storage type, as the forward wrote them)."""


def block_forward(blk, x, context):
    """BasicTransformerBlock._forward for training: x T [N, T, C] dense, context fp32 [N, 2, ctx_dim] -> (out, tape)."""
    assert blk.bbox_cond and blk.multimodal and x.shape[0] % 2 == 0 and context.shape[1] == 2
    t = BlockTape()
    n, tok, c = x.shape
    ln = lambda norm, v: ops.layernorm(v, *norm.affine(), norm.eps)
    a1m = blk.attn1
    t.x = x
    t.xn1 = ln(blk.norm1, x)
    t.q1, t.k1, t.v1 = (ops.linear(t.xn1, m.packed()) for m in (a1m.to_q, a1m.to_k, a1m.to_v))
    t.a1 = ops.attention(t.q1, t.k1, t.v1, a1m.heads, a1m.scale, v_rows=True)
    ctx = context.float().contiguous()
    vec = blk.attn2.single_token_vector(ctx[:, 0])               # one key: softmax == 1 (frozen; no gradient path to x)
    t.x2 = ops.linear(t.a1, a1m.to_out[0].packed(), residual=x, rowvec=vec)
    # bbox adapter (trainable)
    ca = blk.cond_adapter_attn
    t.ctx_t = ctx.to(x.dtype)
    t.xn_a = ln(blk.cond_adapter_norm, t.x2)
    t.q_a = ops.linear(t.xn_a, ca.to_q.packed())
    t.k_a, t.v_a = ops.linear(t.ctx_t, ca.to_k.packed()), ops.linear(t.ctx_t, ca.to_v.packed())
    t.a_a = ops.ctx_attention(t.q_a, t.k_a.float().contiguous(), t.v_a.float().contiguous(), ca.heads, ca.scale)
    t.y_a = ops.linear(t.a_a, ca.to_out[0].packed())
    t.x3 = ops.linear(t.y_a, blk.cond_adapter_connector.packed(), residual=t.x2)
    # cross-modal: camera rows attend to the lidar rows, then lidar rows to the UPDATED camera rows (attention.py:249-261)
    xc, xl = t.x3[::2], t.x3[1::2]
    t.x4 = torch.empty_like(t.x3)
    cam, lid = blk.cross_modal_attn_camera, blk.cross_modal_attn_lidar
    t.xn_c = ln(blk.cross_modal_norm_camera, xc)
    t.q_c, t.k_c, t.v_c = ops.linear(t.xn_c, cam.to_q.packed()), ops.linear(xl, cam.to_k.packed()), ops.linear(xl, cam.to_v.packed())
    t.a_c = ops.attention(t.q_c, t.k_c, t.v_c, cam.heads, cam.scale, v_rows=True)
    t.y_c = ops.linear(t.a_c, cam.to_out[0].packed())
    ops.linear(t.y_c, blk.cross_modal_connector_camera.packed(), residual=xc, out=t.x4[::2])
    xc2 = t.x4[::2]
    t.xn_l = ln(blk.cross_modal_norm_lidar, xl)
    t.q_l, t.k_l, t.v_l = ops.linear(t.xn_l, lid.to_q.packed()), ops.linear(xc2, lid.to_k.packed()), ops.linear(xc2, lid.to_v.packed())
    t.a_l = ops.attention(t.q_l, t.k_l, t.v_l, lid.heads, lid.scale, v_rows=True)
    t.y_l = ops.linear(t.a_l, lid.to_out[0].packed())
    ops.linear(t.y_l, blk.cross_modal_connector_lidar.packed(), residual=xl, out=t.x4[1::2])
    # feed-forward (frozen), GEGLU un-fused so that its inputs are on the tape
    t.xn3 = ln(blk.norm3, t.x4)
    t.pre = ops.linear(t.xn3, blk.ff.net[0].proj.packed())
    t.h = ops.geglu_fwd(t.pre)
    out = ops.linear(t.h, blk.ff.net[2].packed(), residual=t.x4)
    return out, t


def _attn_grads(grads, name, attn, connector, cname, dres, t_q_in, t_kv_in, q, k, v, a, y, scale_heads):
    """Backward of `res + connector(to_out(attention(to_q(q_in), to_k(kv_in), to_v(kv_in))))` given d(res + ...) = dres
    (a [n, T, C] view): parameter gradients into `grads`, returns (d q_in, dk, dv) -- the key / value data gradients still
    as gradients of the projections' OUTPUTS (the caller pushes them through to_k / to_v and into the right rows)."""
    heads, scale = scale_heads
    dy = _dgrad(dres, connector)
    _wgrad(grads, cname, connector, dres, y)
    da = _dgrad(dy, attn.to_out[0])
    _wgrad(grads, name + ".to_out.0", attn.to_out[0], dy, a)
    dq, dk, dv = ops.attention_bwd(q, k, v, a, da, heads, scale)
    _wgrad(grads, name + ".to_q", attn.to_q, dq, t_q_in)
    return _dgrad(dq, attn.to_q), dk, dv


def block_backward(blk, tape, dout):
    """dout: T [N, T, C] dense, the gradient of the loss w.r.t. `block_forward`'s output -> (dx T [N, T, C], grads):
    grads = {parameter name relative to the block: fp32 tensor} for every name of `trainable_names(blk)`, plus
    `__dcontext__`: fp32 [N, 2, ctx_dim], the gradient w.r.t. the context tokens through the bbox adapter's to_k / to_v
    (what the conditioning stage's trainable tensors receive; attn2's path to token 0 ends in frozen tensors only)."""
    t, g = tape, {}
    n, tok, c = dout.shape
    ff = blk.ff
    # ---- feed-forward (frozen): out = W2 geglu(W1 LN3(x4)) + x4
    dh = _dgrad(dout, ff.net[2])
    dpre = ops.geglu_bwd(t.pre, dh)
    dxn3 = _dgrad(dpre, ff.net[0].proj)
    dx4, _, _ = ops.layernorm_bwd(t.x4, dxn3, blk.norm3.affine()[0], blk.norm3.eps, dx_add=dout)
    xc, xl, xc2 = t.x3[::2], t.x3[1::2], t.x4[::2]
    cam, lid = blk.cross_modal_attn_camera, blk.cross_modal_attn_lidar
    # ---- lidar rows: xl' = xl + connector(attn(LN_l(xl), context = xc'))
    dxl2 = dx4[1::2]
    dxn_l, dk_l, dv_l = _attn_grads(g, "cross_modal_attn_lidar", lid, blk.cross_modal_connector_lidar, "cross_modal_connector_lidar",
                                    dxl2, t.xn_l, xc2, t.q_l, t.k_l, t.v_l, t.a_l, t.y_l, (lid.heads, lid.scale))
    _wgrad(g, "cross_modal_attn_lidar.to_k", lid.to_k, dk_l, xc2)
    _wgrad(g, "cross_modal_attn_lidar.to_v", lid.to_v, dv_l, xc2)
    dxl, g["cross_modal_norm_lidar.weight"], g["cross_modal_norm_lidar.bias"] = ops.layernorm_bwd(
        xl, dxn_l, blk.cross_modal_norm_lidar.affine()[0], blk.cross_modal_norm_lidar.eps, dx_add=dxl2.contiguous())
    # ---- camera rows: xc' = xc + connector(attn(LN_c(xc), context = xl)); d xc' = its own rows of dx4 + what the lidar's keys / values send back
    dxc2 = _dgrad(dv_l, lid.to_v, residual=_dgrad(dk_l, lid.to_k, residual=dx4[::2]))
    dxn_c, dk_c, dv_c = _attn_grads(g, "cross_modal_attn_camera", cam, blk.cross_modal_connector_camera, "cross_modal_connector_camera",
                                    dxc2, t.xn_c, xl, t.q_c, t.k_c, t.v_c, t.a_c, t.y_c, (cam.heads, cam.scale))
    _wgrad(g, "cross_modal_attn_camera.to_k", cam.to_k, dk_c, xl)
    _wgrad(g, "cross_modal_attn_camera.to_v", cam.to_v, dv_c, xl)
    dxc, g["cross_modal_norm_camera.weight"], g["cross_modal_norm_camera.bias"] = ops.layernorm_bwd(
        xc, dxn_c, blk.cross_modal_norm_camera.affine()[0], blk.cross_modal_norm_camera.eps, dx_add=dxc2)
    dx3 = torch.empty((n, tok, c), device=dout.device, dtype=dout.dtype)
    _dgrad(dv_c, cam.to_v, residual=_dgrad(dk_c, cam.to_k, residual=dxl), out=dx3[1::2])      # lidar rows: own + the camera's keys / values
    dx3[::2].copy_(dxc)                                                                        # (placement, not arithmetic)
    # ---- bbox adapter: x3 = x2 + connector(attn(LN_a(x2), context tokens))
    ca = blk.cond_adapter_attn
    dxn_a, dk_a, dv_a = _attn_grads(g, "cond_adapter_attn", ca, blk.cond_adapter_connector, "cond_adapter_connector", dx3, t.xn_a,
                                    None, t.q_a, t.k_a, t.v_a, t.a_a, t.y_a, (ca.heads, ca.scale))
    # to_k / to_v saw the 2 N context tokens: a handful of rows -> fp32 FMA chains (mobi_linear_f32) instead of the matrix cores
    ctx32 = _rows(t.ctx_t).float()
    dctx = None                                  # d loss / d context tokens [2 N, ctx_dim] fp32, through to_k and to_v
    for nm, dd, lin in (("to_k", dk_a, ca.to_k), ("to_v", dv_a, ca.to_v)):
        d32 = _rows(dd).float().contiguous()
        g[f"cond_adapter_attn.{nm}.weight"] = ops.linear_f32(d32.t().contiguous(), ctx32.t().contiguous())
        part = ops.linear_f32(d32, lin.weight.detach().float().t().contiguous())
        dctx = part if dctx is None else ops.lincomb4([dctx, part], [1.0, 1.0])
    g["__dcontext__"] = dctx.view(n, 2, -1)
    dx2, g["cond_adapter_norm.weight"], g["cond_adapter_norm.bias"] = ops.layernorm_bwd(
        t.x2, dxn_a, blk.cond_adapter_norm.affine()[0], blk.cond_adapter_norm.eps, dx_add=dx3)
    # ---- attn2 adds a per-image constant: identity for the data gradient.  attn1 (frozen): x2 = to_out(attention(qkv(LN1(x)))) + x
    a1m = blk.attn1
    da1 = _dgrad(dx2, a1m.to_out[0])
    dq, dk, dv = ops.attention_bwd(t.q1, t.k1, t.v1, t.a1, da1, a1m.heads, a1m.scale)
    dxn1 = _dgrad(dv, a1m.to_v, residual=_dgrad(dk, a1m.to_k, residual=_dgrad(dq, a1m.to_q)))
    dx, _, _ = ops.layernorm_bwd(t.x, dxn1, blk.norm1.affine()[0], blk.norm1.eps, dx_add=dx2)
    return dx, g


# ======================================================================================================================
# The whole UNet (openaimodel.py:861-898 of the reference): forward with a tape, backward to every adapter tensor
# ======================================================================================================================
def _conv_dgrad_pack(conv):
    """Data gradient of a stride-1 convolution = the convolution of dy with the kernel rotated by 180 degrees and its
    in / out axes swapped (the same padding for the odd kernels used here): packed once like any other weight."""
    key = (conv.weight._version, conv.weight.data_ptr(), engine_dtype())
    c = conv.__dict__.setdefault("_dgrad_pack", {})
    if c.get("key") != key:
        w = conv.weight.detach().flip(2, 3).transpose(0, 1).contiguous()
        c["key"], c["val"] = key, ops.pack_conv(w, None, engine_dtype(), conv.weight.device)
    return c["val"]


def _res_forward(rb, x, embd, skip):
    lo, hi = rb._emb_slice
    emb_out = embd["proj"][:, lo:hi]                           # (carries conv1's bias: UNetModel._emb_projection)
    xin = x if skip is None else torch.cat([x, skip], dim=3)  # the concat IS materialised here: its gradient is split below
    n1, n2 = rb.in_layers[0], rb.out_layers[0]
    a1 = ops.groupnorm(xin, *n1.affine(), n1.eps, silu=True)
    h1 = ops.igemm(a1, rb.in_layers[2].packed(), rowvec=emb_out, rowvec_has_bias=True)
    a2 = ops.groupnorm(h1, *n2.affine(), n2.eps, silu=True)
    has_conv = not isinstance(rb.skip_connection, torch.nn.Identity) and hasattr(rb.skip_connection, "weight")
    xs = ops.igemm(xin, rb.skip_connection.packed()) if has_conv else xin
    out = ops.igemm(a2, rb.out_layers[3].packed(), residual=xs)
    return out, (xin, h1, x.shape[3], has_conv)


def _res_backward(rb, tape, dout):
    xin, h1, c0, has_conv = tape
    n1, n2 = rb.in_layers[0], rb.out_layers[0]
    da2 = ops.igemm(dout, _conv_dgrad_pack(rb.out_layers[3]))
    dh1 = ops.groupnorm_bwd(h1, da2, *n2.affine(), n2.eps, True)
    da1 = ops.igemm(dh1, _conv_dgrad_pack(rb.in_layers[2]))
    dside = ops.igemm(dout, _conv_dgrad_pack(rb.skip_connection)) if has_conv else dout
    dxin = ops.groupnorm_bwd(xin, da1, *n1.affine(), n1.eps, True, dx_add=dside)
    if c0 < xin.shape[3]:
        return dxin[..., :c0].contiguous(), dxin[..., c0:].contiguous()
    return dxin, None


def _st_forward(st, x, context):
    n, h, w, c = x.shape
    g, b = st.norm.affine()
    t = ops.igemm(ops.groupnorm(x, g, b, st.norm.eps, silu=False), st.proj_in.packed())
    t = t.view(n, h * w, t.shape[3])
    tapes = []
    for blk in st.transformer_blocks:
        t, tp = block_forward(blk, t, context)
        tapes.append(tp)
    return ops.igemm(t.view(n, h, w, t.shape[2]), st.proj_out.packed(), residual=x), (x, tapes)


def _st_backward(st, tape, dout, grads, prefix):
    x, tapes = tape
    n, h, w, c = x.shape
    dt = ops.igemm(dout, _conv_dgrad_pack(st.proj_out))
    dt = dt.view(n, h * w, dt.shape[3])
    for i in reversed(range(len(tapes))):
        dt, g = block_backward(st.transformer_blocks[i], tapes[i], dt)
        dc = g.pop("__dcontext__")
        grads["__dcontext__"] = dc if "__dcontext__" not in grads else ops.lincomb4([grads["__dcontext__"], dc], [1.0, 1.0])
        grads.update({f"{prefix}.transformer_blocks.{i}.{k}": v for k, v in g.items()})
    dxn = ops.igemm(dt.view(n, h, w, dt.shape[2]), _conv_dgrad_pack(st.proj_in))
    g, b = st.norm.affine()
    return ops.groupnorm_bwd(x, dxn, g, b, st.norm.eps, False, dx_add=dout)


def _seq_forward(seq, h, embd, context, skip=None):
    from .ldm.modules.attention import SpatialTransformer
    from .ldm.modules.diffusionmodules.openaimodel import Downsample, ResBlock, Upsample, _plain_conv
    tapes = []
    for layer in seq:
        if isinstance(layer, ResBlock):
            h, tp = _res_forward(layer, h, embd, skip)
            skip = None
        elif isinstance(layer, SpatialTransformer):
            h, tp = _st_forward(layer, h, context)
        elif isinstance(layer, (Downsample, Upsample)):
            tp, h = tuple(h.shape), layer(h)
        else:
            h, tp = _plain_conv(layer, h), None          # input_blocks.0: nothing trainable in front of it, the gradient stops
        tapes.append(tp)
    return h, tapes


def _seq_backward(seq, tapes, dh, grads, prefix):
    from .ldm.modules.attention import SpatialTransformer
    from .ldm.modules.diffusionmodules.openaimodel import Downsample, ResBlock, Upsample
    dskip = None
    for i in reversed(range(len(seq))):
        layer, tp = seq[i], tapes[i]
        if isinstance(layer, ResBlock):
            dh, dskip = _res_backward(layer, tp, dh)
        elif isinstance(layer, SpatialTransformer):
            dh = _st_backward(layer, tp, dh, grads, f"{prefix}.{i}")
        elif isinstance(layer, Upsample):
            dh = ops.sumpool2(ops.igemm(dh, _conv_dgrad_pack(layer.conv)))       # nearest x2, then the convolution
        elif isinstance(layer, Downsample):
            # stride 2: dy spread onto the even pixels of the input grid (placement), then the stride-1 data gradient
            n, ho, wo, c = dh.shape
            dz = torch.zeros((n, tp[1], tp[2], c), device=dh.device, dtype=dh.dtype)
            dz[:, : 2 * ho: 2, : 2 * wo: 2] = dh
            dh = ops.igemm(dz, _conv_dgrad_pack(layer.op))
        else:
            dh = None
    return dh, dskip


def unet_forward(net, x, timesteps, context):
    """UNetModel.forward for training: x fp32 [N, in_channels, h, w] -> (eps fp32 [N, out_channels, h, w], tape)."""
    from ._lib import ACT_SILU
    from .ldm.modules.diffusionmodules.util import timestep_embedding
    t_emb = timestep_embedding(timesteps, net.model_channels)
    w0, b0 = net.time_embed[0].skinny()
    w2, b2 = net.time_embed[2].skinny()
    emb = ops.skinny_linear(ops.skinny_linear(t_emb, w0, b0, post_act=ACT_SILU), w2, b2)
    we, be = net._emb_projection()
    embd = {"emb": emb, "proj": ops.skinny_linear(emb, we, be, pre_act=ACT_SILU)}
    context = context.float().contiguous()
    tape = {"in": [], "out": []}
    hs, h = [], x
    for module in net.input_blocks:
        h, tp = _seq_forward(module, h, embd, context)
        hs.append(h)
        tape["in"].append(tp)
    h, tape["mid"] = _seq_forward(net.middle_block, h, embd, context)
    for module in net.output_blocks:
        h, tp = _seq_forward(module, h, embd, context, skip=hs.pop())
        tape["out"].append(tp)
    n0 = net.out[0]
    tape["head"] = h
    a = ops.groupnorm(h, *n0.affine(), n0.eps, silu=True)
    return ops.conv_small_cout(a, net.out[2].packed_tap_major(), pad=net.out[2].padding), tape


def unet_backward(net, tape, deps=None, dy=None):
    """deps: fp32 [N, out_channels, h, w], the gradient of the loss w.r.t. `unet_forward`'s result -- or dy: the same gradient
    already as T [N, h, w, 32] channels-last, zero beyond out_channels (what `ops.loss_grad` writes) -> {parameter name relative
    to the UNet: fp32 gradient} for every tensor of `trainable_names(net)` (ddpm.py:1616-1629 of the reference)."""
    assert (deps is None) != (dy is None), "one of deps (plain fp32 gradient) and dy (packed by ops.loss_grad)"
    grads = {}
    conv = net.out[2]
    key = (conv.weight._version, conv.weight.data_ptr(), engine_dtype())
    c = conv.__dict__.setdefault("_dgrad_thin", {})
    if c.get("key") != key:                       # 4 -> 320 channels: the thin side zero-padded to 32 like the input convolution's
        w = conv.weight.detach().flip(2, 3).transpose(0, 1).contiguous()
        c["key"], c["val"] = key, ops.pack_conv_padded_cin(w, None, engine_dtype(), conv.weight.device)
    if dy is None:
        dy = ops.pack_sources([deps.float().contiguous()], engine_dtype())
    assert dy.dtype == engine_dtype() and dy.is_contiguous() and dy.shape[3] == 32
    n0 = net.out[0]
    dh = ops.groupnorm_bwd(tape["head"], ops.igemm(dy, c["val"]), *n0.affine(), n0.eps, True)
    nin = len(net.input_blocks)
    dhs = {}
    for i in reversed(range(len(net.output_blocks))):
        dh, dskip = _seq_backward(net.output_blocks[i], tape["out"][i], dh, grads, f"output_blocks.{i}")
        dhs[nin - 1 - i] = dskip                   # output block i consumed hs.pop() = the result of input block nin - 1 - i
    dh, _ = _seq_backward(net.middle_block, tape["mid"], dh, grads, "middle_block")
    for j in reversed(range(1, nin)):              # input_blocks.0 is the bare input convolution: nothing trainable before it
        dh = ops.add(dh, dhs[j])
        dh, _ = _seq_backward(net.input_blocks[j], tape["in"][j], dh, grads, f"input_blocks.{j}")
    return grads


_ZERO_TABLES = {}


def _zero_tables(device):
    """(logvar, lvlb) of the default objective, one entry each, cached per device: `mobi_loss_grad` clamps t into the tables, so
    every t reads logvar 0 and weight 0."""
    if device not in _ZERO_TABLES:
        _ZERO_TABLES[device] = (torch.zeros(1, dtype=torch.float32, device=device), torch.zeros(1, dtype=torch.float32, device=device))
    return _ZERO_TABLES[device]


def loss_and_gradients(net, x_noisy, timesteps, context, target, loss_scale=1.0, unscale=True, *, loss_type="l2", t_weights=None,
                       l_simple_weight=1.0, elbo_weight=0.0, return_terms=False):
    """The eps-parameterised loss of `p_losses` (ddpm.py:1177-1217 of the reference) and its gradient w.r.t. every adapter tensor:
    loss = l_simple_weight * mean_i(loss_simple_i / exp(logvar[t_i]) + logvar[t_i]) + elbo_weight * mean_i(lvlb[t_i] * loss_simple_i),
    loss_simple_i the per-sample mean of (eps - target)^2 (loss_type "l2") or |eps - target| ("l1").  t_weights: the device
    tables (logvar, lvlb), fp32 [T]; None: logvar 0 and weight 0 at every t (with the default weights: the mean squared error).
    One launch (`ops.loss_grad`) forms the loss terms and the gradient that enters the backward pass, in the layout its first
    launch reads; nothing is read back.  loss_scale multiplies that gradient and is divided out of the fp32 results (fp16
    storage underflows without it at production sizes); with unscale=False that per-tensor pass is skipped and every gradient
    (`__dcontext__` too) comes back still multiplied by loss_scale, for `AdamW.step_scaled` to divide out inside its one update
    launch.  -> (loss: 0-d fp32 device tensor, grads); return_terms=True: (loss, grads, (per_sample fp32 [N], terms fp32 [3] =
    loss_simple's mean, loss_vlb, loss))."""
    eps, tape = unet_forward(net, x_noisy, timesteps, context)
    eps, target = eps.contiguous(), target.float().contiguous()
    logvar, lvlb = _zero_tables(eps.device) if t_weights is None else t_weights
    t = timesteps.to(device=eps.device, dtype=torch.int64).contiguous()
    dy, per_sample, terms = ops.loss_grad(eps, target, t, logvar.float().contiguous(), lvlb.float().contiguous(), loss_type=loss_type,
                                          l_simple_weight=l_simple_weight, elbo_weight=elbo_weight, loss_scale=loss_scale,
                                          dtype=engine_dtype())
    grads = unet_backward(net, tape, dy=dy)
    if unscale and loss_scale != 1.0:
        grads = {name: ops.lincomb4([g.contiguous()], [1.0 / loss_scale]) for name, g in grads.items()}
    loss = terms[2]                               # (grads["__dcontext__"]: the gradient w.r.t. the context tokens)
    return (loss, grads, (per_sample, terms)) if return_terms else (loss, grads)


# ======================================================================================================================
# The conditioning stage's trainable part (ddpm.py:1635-1647 of the reference): the 3-D box embedder and `bbox_uncond_vector`
# ======================================================================================================================
def bbox_embedder_forward(emb, bbox):
    """BBoxEmbedder.forward (ldm/modules/encoders/modules.py:85-91 of the reference) with a tape: bbox fp32 [B, 8, 3] ->
    (token fp32 [B, 1, 768], tape).  Fourier features, then Linear -> Linear, SiLU, Linear, SiLU, Linear as fp32 GEMV chains."""
    from ._lib import ACT_SILU
    from .ldm.modules.encoders.modules import fourier_features
    e = fourier_features(bbox.float(), emb.num_freqs).reshape(bbox.shape[0], -1).contiguous()
    gemv = lambda lin, x, pre=0: ops.skinny_linear(x.contiguous(), *lin.skinny(), pre_act=pre)
    h0 = gemv(emb.bbox_proj, e)
    z1 = gemv(emb.second_linear[0], h0)
    z2 = gemv(emb.second_linear[2], z1, ACT_SILU)
    out = gemv(emb.second_linear[4], z2, ACT_SILU)
    return out.unsqueeze(1), (e, h0, z1, z2)


def bbox_embedder_backward(emb, tape, dtoken):
    """dtoken: fp32 [B, 1, 768] -> {`bbox_proj.weight`, ..., `second_linear.4.bias`: fp32 gradient} (8 tensors).  A handful of rows:
    every product is an fp32 FMA chain (mobi_linear_f32)."""
    e, h0, z1, z2 = tape
    silu = lambda z: z * torch.sigmoid(z)          # (recomputed activations: [B, 512] fp32 elementwise, the GEMV's pre-activation)
    g = {}
    ones = torch.ones((1, dtoken.shape[0]), device=dtoken.device, dtype=torch.float32)

    def layer(name, lin, dy, x, need_dx=True):
        g[name + ".weight"] = ops.linear_f32(dy.t().contiguous(), x.t().contiguous())
        g[name + ".bias"] = ops.linear_f32(dy.t().contiguous(), ones).reshape(-1)
        return ops.linear_f32(dy, lin.weight.detach().float().t().contiguous()) if need_dx else None
    dy = dtoken.reshape(dtoken.shape[0], -1).float().contiguous()
    da2 = layer("second_linear.4", emb.second_linear[4], dy, silu(z2))
    dz2 = ops.silu_bwd_f32(z2.contiguous(), da2)
    da1 = layer("second_linear.2", emb.second_linear[2], dz2, silu(z1))
    dz1 = ops.silu_bwd_f32(z1.contiguous(), da1)
    dh0 = layer("second_linear.0", emb.second_linear[0], dz1, h0)
    layer("bbox_proj", emb.bbox_proj, dh0, e, need_dx=False)
    return g


class LambdaLR:
    """torch.optim.lr_scheduler.LambdaLR for the engine's optimizer (ddpm.py:1662): the rate is the optimizer's initial rate times
    `lr_lambda(step)`, set at construction (step 0) and after every `step()`."""

    def __init__(self, optimizer, lr_lambda):
        self.optimizer, self.lr_lambda = optimizer, lr_lambda
        self.base_lrs = [optimizer.lr]
        self.last_epoch = 0
        optimizer.lr = self.base_lrs[0] * lr_lambda(0)

    def step(self):
        self.last_epoch += 1
        self.optimizer.lr = self.base_lrs[0] * self.lr_lambda(self.last_epoch)

    def get_last_lr(self):
        return [self.optimizer.lr]

    def state_dict(self):
        """`last_epoch` and `base_lrs` (the schedule function itself is code, rebuilt by `configure_optimizers`)."""
        return {"last_epoch": int(self.last_epoch), "base_lrs": [float(x) for x in self.base_lrs]}

    def load_state_dict(self, sd):
        """Restores the position and re-applies `optimizer.lr = base_lr * lr_lambda(last_epoch)`."""
        self.last_epoch, self.base_lrs = int(sd["last_epoch"]), [float(x) for x in sd["base_lrs"]]
        self.optimizer.lr = self.base_lrs[0] * self.lr_lambda(self.last_epoch)


def static_loss_scale(numel):
    """The loss scale `training_step` picks for fp16 from the element count of the UNet's output: a power of two near numel / 4
    (the gradient that enters the network is 2 (eps - target) / numel)."""
    return 2.0 ** round(math.log2(max(4, numel) / 4))


class GradScaler:
    """Dynamic loss scaling with the rules of torch.cuda.amp.GradScaler, the scale kept as a host float: `update(found_inf)`
    multiplies it by `backoff_factor` on an overflow (and restarts the count of clean steps), by `growth_factor` after
    `growth_interval` consecutive clean steps.  enabled=None: on for fp16 storage only (bf16 has fp32's range: the scale is 1.0
    and never moves).  init_scale=None: `static_loss_scale(numel)` of the first step (`first_use`), so that a run starts at the
    scale `training_step` uses without a scaler."""

    def __init__(self, init_scale=None, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=None):
        self.enabled = (engine_dtype() == torch.float16) if enabled is None else bool(enabled)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._scale = None if init_scale is None else float(init_scale)
        self._growth_tracker = 0

    def first_use(self, numel):
        """Fixes the scale left open by init_scale=None from the element count of the UNet's output; returns the scale."""
        if self.enabled and self._scale is None:
            self._scale = static_loss_scale(numel)
        return self.scale

    @property
    def scale(self):
        if not self.enabled:
            return 1.0
        if self._scale is None:
            raise RuntimeError("GradScaler(init_scale=None): the scale is set at first use (first_use(numel), training_step)")
        return self._scale

    def update(self, found_inf):
        if not self.enabled:
            return
        if found_inf:
            self._scale = self.scale * self.backoff_factor
            self._growth_tracker = 0
            return
        self._growth_tracker += 1
        if self._growth_tracker >= self.growth_interval:
            self._scale = self.scale * self.growth_factor
            self._growth_tracker = 0

    def state_dict(self):
        return {"scale": self._scale, "growth_tracker": self._growth_tracker, "growth_factor": self.growth_factor,
                "backoff_factor": self.backoff_factor, "growth_interval": self.growth_interval}

    def load_state_dict(self, sd):
        self._scale = None if sd["scale"] is None else float(sd["scale"])
        self._growth_tracker = int(sd["growth_tracker"])
        self.growth_factor, self.backoff_factor = float(sd["growth_factor"]), float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])


class StepResult:
    """What `AdamW.step_scaled` did: found_inf (the step was skipped), grad_norm (the UNscaled global L2 norm), clip_coef (what
    the gradients were multiplied by besides 1 / scale), scale (the loss scale the gradients carried)."""

    def __init__(self, found_inf, grad_norm, clip_coef, scale):
        self.found_inf, self.grad_norm, self.clip_coef, self.scale = found_inf, grad_norm, clip_coef, scale

    def __repr__(self):
        return f"StepResult(found_inf={self.found_inf}, grad_norm={self.grad_norm}, clip_coef={self.clip_coef}, scale={self.scale})"


class _TableCache(dict):
    """Multi-tensor tables per tuple of names, built at first use: `cache.get_or_build(names, build)`."""

    def get_or_build(self, names, build):
        table = self.get(names)
        if table is None:
            table = self[names] = build()
        return table


class AdamW:
    """torch.optim.AdamW's update (what `configure_optimizers` returns, ddpm.py:1649) on the engine: fp32 master parameters
    updated in place by `mobi_adamw_step`, moments kept per parameter name."""

    def __init__(self, named_params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        self.params = dict(named_params)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.state, self.steps = {}, 0
        self._multi = _TableCache()                   # step_scaled's tables, per set of names that had a gradient (built lazily)

    def step(self, grads, refresh=None):
        """grads: {name: fp32 tensor}; names without an entry are left alone.  refresh: a `WeightRefresher`, called after the
        update (None: the 16-bit copies are rebuilt lazily, as ever)."""
        self.steps += 1
        stepped = {name: p for name, p in self.params.items() if name in grads}
        for name, p in stepped.items():
            st = self.state.setdefault(name, (torch.zeros_like(p.data, dtype=torch.float32), torch.zeros_like(p.data, dtype=torch.float32)))
            ops.adamw_step(p.data, grads[name].reshape(p.shape).contiguous(), st[0], st[1], self.steps, self.lr, self.betas, self.eps,
                           self.weight_decay)
        weights_changed(stepped.values())
        if refresh is not None:
            refresh.refresh()
        return self

    def state_dict(self):
        """torch.optim.AdamW's format: {"state": {index: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [one group]}, the
        index a tensor's position in `self.params` (`configure_optimizers`' order, the reference's).  The moments are the live
        tensors, not copies.  A tensor that never had a gradient has no entry, as in torch.  The engine keeps ONE step count:
        `self.steps` goes into every entry (an fp32 0-d tensor, as torch writes it)."""
        state = {i: {"step": torch.tensor(float(self.steps)), "exp_avg": self.state[n][0], "exp_avg_sq": self.state[n][1]}
                 for i, n in enumerate(self.params) if n in self.state}
        group = {"lr": float(self.lr), "betas": tuple(float(b) for b in self.betas), "eps": float(self.eps),
                 "weight_decay": float(self.weight_decay), "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        """The inverse of `state_dict`, also for a torch.optim.AdamW's over the same tensors in the same order.  All entries must
        carry the same step count (ValueError otherwise: per-tensor counts have no place in one launch over all tensors).  Moments
        are copied INTO the existing tensors where there are some -- the multi-tensor tables hold their addresses; where one is
        created or removed the tables are dropped and rebuilt at the next step."""
        groups = sd["param_groups"]
        names = list(self.params)
        if len(groups) != 1 or len(groups[0]["params"]) != len(names):
            raise ValueError(f"an optimizer state of {len(groups)} groups / {sum(len(g['params']) for g in groups)} tensors where "
                             f"this optimizer holds one group of {len(names)}")
        group = groups[0]
        if group.get("amsgrad", False):
            raise ValueError("amsgrad=True: the engine's AdamW keeps no running maximum")
        position = {pid: k for k, pid in enumerate(group["params"])}
        entries = {names[position[pid]]: e for pid, e in sd["state"].items()}
        steps = sorted({float(e["step"]) for e in entries.values()})
        if len(steps) > 1:
            raise ValueError(f"the optimizer state carries {len(steps)} different step counts ({steps[:4]} ...): the engine keeps "
                             "ONE step count for all tensors and cannot load per-tensor counts")
        if steps and (steps[0] != int(steps[0]) or steps[0] < 0):
            raise ValueError(f"step count {steps[0]!r}")
        for n, e in entries.items():
            for key in ("exp_avg", "exp_avg_sq"):
                if tuple(e[key].shape) != tuple(self.params[n].shape):
                    raise ValueError(f"{n}: {key} of shape {tuple(e[key].shape)} for a tensor of shape {tuple(self.params[n].shape)}")
        rebuilt = False
        for n in [k for k in self.state if k not in entries]:
            del self.state[n]
            rebuilt = True
        for n, e in entries.items():
            if n in self.state:
                self.state[n][0].copy_(e["exp_avg"])
                self.state[n][1].copy_(e["exp_avg_sq"])
            else:
                dev = self.params[n].device
                self.state[n] = tuple(e[key].detach().to(device=dev, dtype=torch.float32, copy=True).contiguous()
                                      for key in ("exp_avg", "exp_avg_sq"))
                rebuilt = True
        if rebuilt:
            self._multi = _TableCache()
        self.steps = int(steps[0]) if steps else 0
        self.lr, self.betas = float(group["lr"]), tuple(float(b) for b in group["betas"])
        self.eps, self.weight_decay = float(group["eps"]), float(group["weight_decay"])

    def step_scaled(self, grads, scaler=None, max_norm=None, refresh=None):
        """`step()` for gradients that are still multiplied by `scaler.scale` (`training_step(..., scaler=s)`), with overflow
        skipping and gradient-norm clipping, in two launches whatever the number of tensors: `mobi_grad_stats` (fp64 sum of squares
        + non-finite flag over every gradient), ONE read-back of its 16-byte record -- the single host sync of a step: it keeps
        `steps`, the bias corrections and the scale on the host, where `step()` keeps them -- then `mobi_adamw_multi` on
        g * clip_coef / scale.  norm = sqrt(sumsq) / scale (host fp64); clip_coef = min(1, max_norm / (norm + 1e-6)) as
        torch.nn.utils.clip_grad_norm_.  A non-finite gradient launches nothing more: `steps`, every parameter and both moments
        stay as they are and the scaler backs off.  Names without an entry in `grads` are left alone.  refresh: a `WeightRefresher`,
        called after an update that took place (a skipped step launches nothing).  -> StepResult."""
        names = tuple(n for n in self.params if n in grads)
        scale = 1.0 if scaler is None else scaler.scale
        if not names:
            return StepResult(False, 0.0, 1.0, scale)
        def build():
            for n in names:
                p = self.params[n]
                self.state.setdefault(n, (torch.zeros_like(p.data, dtype=torch.float32), torch.zeros_like(p.data, dtype=torch.float32)))
            return ops.MultiTensorTable([[self.params[n].data for n in names], ops.LIVE, [self.state[n][0] for n in names],
                                         [self.state[n][1] for n in names]])
        mt = self._multi.get_or_build(names, build)
        mt.set_live([grads[n].reshape(self.params[n].shape) for n in names])
        sumsq, found_inf = ops.read_grad_stats(ops.grad_stats(mt))
        if found_inf:
            if scaler is not None:
                scaler.update(True)
            return StepResult(True, float("inf"), 0.0, scale)
        norm = math.sqrt(sumsq) / scale
        clip = 1.0 if max_norm is None else min(1.0, float(max_norm) / (norm + 1e-6))
        self.steps += 1
        ops.adamw_multi(mt, clip / scale, self.steps, self.lr, self.betas, self.eps, self.weight_decay)
        weights_changed(self.params[n] for n in names)
        if refresh is not None:
            refresh.refresh()
        if scaler is not None:
            scaler.update(False)
        return StepResult(False, norm, clip, scale)


class GradAccumulator:
    """Gradient accumulation over a window of `micro_batches` forward / backward passes per optimizer step (the reference's
    `lightning.trainer.accumulate_grad_batches`, main.py:675-694): `add` after every `training_step(..., allreduce=False)`, `step`
    after the last.  The accumulators are views of flat fp32 buffers -- one fp32 copy of `optimizer.params`, laid out by
    `dist.gradient_bucket_layout` (sorted names, the buckets of `allreduce_gradients`, 16-byte aligned starts) -- and hold the MEAN
    over the window: every micro-batch enters with the weight w = fp32(1 / micro_batches), in ONE launch (`mobi_accum_multi`), as
    b <- w g for a name's first gradient of the window (the accumulator is not read: nothing of an earlier window, skipped or
    not, is seen; no zero-fill) and b <- b + (w g) after -- two launches only where a micro-batch brings both new and known names
    (a conditional draw after an unconditional one).  With more than one process the collective runs once per window, on the
    buffers in place (`dist.allreduce_accumulated`).  inf / nan of any micro-batch survive the sums; `step_scaled` finds them."""

    def __init__(self, optimizer, micro_batches, bucket_bytes=256 << 20):
        import numpy as np
        from . import dist as mdist
        if int(micro_batches) != micro_batches or micro_batches < 1:
            raise ValueError(f"micro_batches must be a positive integer, not {micro_batches!r}")
        self.optimizer, self.micro_batches = optimizer, int(micro_batches)
        self.weight = float(np.float32(1.0) / np.float32(self.micro_batches))
        self.names = sorted(optimizer.params)
        numels = {k: optimizer.params[k].numel() for k in self.names}
        self.layout, lengths = mdist.gradient_bucket_layout(numels, bucket_bytes)
        device = optimizer.params[self.names[0]].device
        mdist.check_same_layout(self.names, [numels[k] for k in self.names], device)      # once: the layout cannot diverge later
        self.buckets = [torch.zeros(n, dtype=torch.float32, device=device) for n in lengths]
        self.views = {k: self.buckets[b][off:off + n].view(optimizer.params[k].shape) for k, (b, off, n) in self.layout.items()}
        self._tables = _TableCache()                  # per tuple of names, as AdamW._multi
        self._clear()

    def _clear(self):
        self._seen, self._adds, self._scale = set(), 0, None

    def _launch(self, names, grads, op):
        if not names:
            return
        table = self._tables.get_or_build(names, lambda: ops.MultiTensorTable([ops.LIVE, [self.views[k] for k in names]]))
        table.set_live([grads[k].reshape(self.views[k].shape) for k in names])
        ops.accum_multi(table, self.weight, op)

    def add(self, grads, scale=1.0):
        """grads: {name: fp32 tensor} of one micro-batch (`model.adapter_grads`: any subset of the optimizer's names), still
        multiplied by `scale` (`model.adapter_grads_scale`) -- the same for every micro-batch of a window."""
        from ._lib import MT_ACCUM, MT_ASSIGN
        if self._adds >= self.micro_batches:
            raise RuntimeError(f"add() number {self._adds + 1} in a window of {self.micro_batches} micro-batches: step() first")
        unknown = [k for k in grads if k not in self.views]
        if unknown:
            raise KeyError(f"gradients of tensors the optimizer does not hold: {unknown[:3]}")
        if self._adds and float(scale) != self._scale:
            raise ValueError(f"this micro-batch's gradients carry the loss scale {scale!r}, the window's first {self._scale!r}")
        first = tuple(k for k in self.names if k in grads and k not in self._seen)
        again = tuple(k for k in self.names if k in grads and k in self._seen)
        self._launch(first, grads, MT_ASSIGN)
        self._launch(again, grads, MT_ACCUM)
        self._seen.update(first)
        self._adds, self._scale = self._adds + 1, float(scale)

    def state_dict(self):
        """Between windows the accumulator holds nothing a later window reads (its first add is an ASSIGN): {}.  Inside a window
        it raises: a checkpoint is taken between optimizer steps."""
        if self._adds != 0:
            raise RuntimeError(f"state_dict() after {self._adds} of {self.micro_batches} micro-batches of a window: a checkpoint is "
                               "taken between optimizer steps")
        return {}

    def load_state_dict(self, sd):
        if sd:
            raise ValueError(f"a GradAccumulator has no state between windows, got keys {sorted(sd)[:4]}")
        self._clear()

    def step(self, scaler=None, max_norm=None, refresh=None):
        """The optimizer step of the window (refresh: handed on to `step_scaled`): `optimizer.step_scaled` on the accumulators of every tensor some rank saw (a tensor
        nobody saw is left out and so left alone -- no weight decay, no decay of its moments), after the one collective of the
        window where there is more than one process.  The window is cleared whether or not the step was skipped.  -> StepResult."""
        from . import dist as mdist
        if self._adds != self.micro_batches:
            raise RuntimeError(f"step() after {self._adds} of {self.micro_batches} micro-batches")
        want = 1.0 if scaler is None else float(scaler.scale)
        if self._scale != want:
            raise ValueError(f"the window's gradients carry the loss scale {self._scale!r}, the step would divide by {want!r}")
        try:
            present = mdist.allreduce_accumulated(self.buckets, self.layout, self._seen)
            return self.optimizer.step_scaled({k: self.views[k] for k in present}, scaler=scaler, max_norm=max_norm, refresh=refresh)
        finally:
            self._clear()


# ======================================================================================================================
# The loop (main.py of the reference: Lightning's Trainer + ModelCheckpoint, `scripts/train.sh`)
# ======================================================================================================================
def scaled_lr(base_lr, accumulate=1, nodes=1, gpus=1, batch_size=1):
    """The reference's `--scale_lr` arithmetic (main.py:690-694): accumulate * nodes * gpus * batch_size * base_lr."""
    return accumulate * nodes * gpus * batch_size * base_lr


def epoch_order(n, seed, epoch):
    """The order in which epoch `epoch` visits a dataset of n items: a permutation that depends on (seed, epoch) only."""
    return torch.randperm(n, generator=torch.Generator().manual_seed(int(seed) + int(epoch))).tolist()


class EpochSampler:
    """A batch sampler for one (seed, epoch): `epoch_order` cut into batches of `batch_size`, beginning at batch `start_batch`
    -- the indices in front of it are dropped here, their items are never built.  `loader_seed` is what `device_loader` seeds
    its DataLoader's own generator with (the base seed of worker processes): (seed, epoch) again, nothing of the global state."""

    def __init__(self, n, batch_size, seed, epoch, start_batch=0, drop_last=True):
        self.loader_seed = int(seed) + int(epoch)
        order = epoch_order(n, seed, epoch)
        if drop_last:
            order = order[:len(order) // batch_size * batch_size]
        order = order[start_batch * batch_size:]
        self.batches = [order[i:i + batch_size] for i in range(0, len(order), batch_size)]

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def epoch_loader(dataset, batch_size, seed, num_workers=0, drop_last=True, device="cuda"):
    """`train_batches` for `Trainer.fit` over a `NuScenesDataset`: (epoch, start_batch) -> its `device_loader` under an
    `EpochSampler`.  The order depends on (seed, epoch) only and a resumed epoch begins at `start_batch`."""
    def train_batches(epoch, start_batch=0):
        sampler = EpochSampler(len(dataset), batch_size, seed, epoch, start_batch, drop_last)
        return dataset.device_loader(batch_size, num_workers=num_workers, device=device, sampler=sampler)
    return train_batches


def _clone_tensors(x):
    if isinstance(x, dict):
        return {k: _clone_tensors(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_clone_tensors(v) for v in x)
    return x.clone() if isinstance(x, torch.Tensor) else x


class ImageLogger:
    """The reference's `ImageLogger` callback (main.py:319-422; always installed there with batch_frequency=400, max_images=8,
    clamp=False, log_on_batch_idx=True, log_first_step=True, main.py:604-613) for `Trainer`: every `batch_frequency` batches, and
    on validation batches, `model.log_images(batch, split=split, **log_images_kwargs)` samples the batch again (DDIM, under the EMA
    weights) and the tensor entries of its log dict become pictures under
    `save_dir/images/<split>/<key>_gs-<global_step:06>_e-<epoch:06>_b-<batch_idx:06>.png` (`log_local`'s naming) -- all keys
    through ONE `ops.image_grid` launch and one read-back, with `max_images`, `clamp` and `rescale` honoured by that launch
    (`rescale=False`: an fp32 entry is taken as [0, 1]; uint8 entries, `log_data`'s camera collages, pass through, where the
    reference's rescale would destroy them).  `log_img` returns {"step", "epoch", "batch_idx", "split",
    **model.last_lidar_metrics} in Python floats: the lidar error scores of the SAMPLED objects.

    A logging call does not move the run: the four generator states `checkpoint.Checkpointer` saves (Python, numpy, torch CPU,
    torch device) are captured before the call, all four are seeded from (seed, global_step, split == "val", batch_idx) -- the VAE
    posteriors `get_input` samples and the noise DDIM draws at every step with eta = 1 come from that stream -- and put back
    after it, also when it raises; so does the model's train / eval mode.  The model sees a copy of the batch (`get_input` edits
    `ref_bbox` in place).  As in the reference the hook runs AFTER the training step has made that edit once already.
    More than one process: every rank runs the call (no collective inside it, the ranks stay in step), rank 0 alone writes files
    (not run on more than one GPU)."""

    def __init__(self, save_dir, batch_frequency=400, max_images=8, clamp=True, increase_log_steps=True, rescale=True,
                 disabled=False, log_on_batch_idx=False, log_first_step=False, log_images_kwargs=None, seed=0):
        self.save_dir, self.batch_freq, self.max_images = save_dir, int(batch_frequency), int(max_images)
        self.clamp, self.rescale, self.disabled = clamp, rescale, disabled
        self.log_steps = []                       # (the reference's doubling steps are commented out there, main.py:330)
        if not increase_log_steps:
            self.log_steps = [self.batch_freq]
        self.log_on_batch_idx, self.log_first_step = log_on_batch_idx, log_first_step
        self.log_images_kwargs = log_images_kwargs if log_images_kwargs else {}
        self.seed = int(seed)
        self.last_images = None                   # {key: uint8 [Hg, Wg, 3]} of the last call

    def check_frequency(self, check_idx):
        """main.py:406-414 as it stands."""
        if (check_idx % self.batch_freq == 0 or check_idx in self.log_steps) and (check_idx > 0 or self.log_first_step):
            if self.log_steps:
                self.log_steps.pop(0)
            return True
        return False

    def _seed(self, global_step, split, batch_idx, device):
        import random
        import numpy as np
        words = np.random.SeedSequence([self.seed, int(global_step), int(split == "val"), int(batch_idx)]).generate_state(4)
        random.seed(int(words[0]))
        np.random.seed(int(words[1]))
        torch.default_generator.manual_seed(int(words[2]))
        if device is not None:
            index = device.index if device.index is not None else torch.cuda.current_device()
            torch.cuda.default_generators[index].manual_seed(int(words[3]))

    def pictures(self, images):
        """The tensor entries of a log dict -> {key: uint8 [Hg, Wg, 3]}: one launch per 16 keys."""
        keys = [k for k, v in images.items() if isinstance(v, torch.Tensor) and v.dim() == 4]
        out = {}
        for i in range(0, len(keys), 16):
            out.update(ops.image_grid({k: images[k] for k in keys[i:i + 16]}, self.max_images, nrow=4, padding=2,
                                      clamp=self.clamp, rescale=self.rescale))
        return out

    def log_local(self, split, pictures, global_step, current_epoch, batch_idx):
        import os
        from PIL import Image
        root = os.path.join(self.save_dir, "images", split)
        for k, grid in pictures.items():
            path = os.path.join(root, "{}_gs-{:06}_e-{:06}_b-{:06}.png".format(k, global_step, current_epoch, batch_idx))
            os.makedirs(os.path.split(path)[0], exist_ok=True)             # (a `/` in a key is a directory, as in the reference)
            Image.fromarray(grid).save(path)

    def log_img(self, trainer, model, batch, batch_idx, split="train"):
        from . import checkpoint
        from . import dist as mdist
        global_step, epoch = int(trainer.global_step), int(getattr(trainer, "current_epoch", 0))
        check_idx = batch_idx if self.log_on_batch_idx else global_step
        if not (self.check_frequency(check_idx) and callable(getattr(model, "log_images", None)) and self.max_images > 0):
            return None
        if getattr(trainer, "checkpointer", None) is not None:
            trainer.checkpointer.wait()           # (a step graph may be captured below: not while the writer thread copies)
        device = getattr(model, "device", None)
        device = device if isinstance(device, torch.device) and device.type == "cuda" else None
        was_training, rng = model.training, checkpoint.rng_get(device)
        try:
            self._seed(global_step, split, batch_idx, device)
            model.eval()
            with torch.no_grad():
                images = model.log_images(_clone_tensors(batch), split=split, **self.log_images_kwargs)
                self.last_images = self.pictures(images)
        finally:
            model.train(was_training)
            checkpoint.rng_set(rng, device)
        if mdist.world()[0] == 0:
            self.log_local(split, self.last_images, global_step, epoch, batch_idx)
        metrics = getattr(model, "last_lidar_metrics", None) or {}
        return {"step": global_step, "epoch": epoch, "batch_idx": int(batch_idx), "split": split,
                **{k: float(v) for k, v in metrics.items()}}

    def on_train_batch_end(self, trainer, model, batch, batch_idx):
        if not self.disabled and (trainer.global_step > 0 or self.log_first_step):
            return self.log_img(trainer, model, batch, batch_idx, split="train")
        return None

    def on_validation_batch_end(self, trainer, model, batch, batch_idx):
        if not self.disabled and (trainer.global_step > 0 or self.log_first_step):
            return self.log_img(trainer, model, batch, batch_idx, split="val")
        return None


class Trainer:
    """The loop the reference runs under Lightning (main.py; `scripts/train.sh`: `--save_top_k`, `--resume`), for ONE model on the
    engine: `training_step(batch, scaler=s, allreduce=k == 1)`, `acc.add` / `acc.step` (or `opt.step_scaled` directly),
    `model.on_train_batch_end()`, `scheduler.step()`; at the end of every epoch `validation_step` over `val_batches`, every key
    averaged, `epoch=NNNNNN.ckpt` saved and the `save_top_k` best by `model.monitor` (lower is better; -1 keeps all; without a
    monitored value: the most recent) kept next to `last.ckpt`, which is always there; `every_n_steps` adds `last.ckpt` saves
    inside an epoch.  Only files this trainer wrote are pruned; an epoch outside the top k is written once, as `last.ckpt`.  The optimizer, the schedule and the rate come from
    `model.configure_optimizers()` / `model.learning_rate`.

    train_batches(epoch, start_batch) -> an iterable of batch dicts whose order depends on (seed, epoch) only and which begins
    at batch `start_batch` (`epoch_loader`); val_batches() -> an iterable of batch dicts, or None.  With
    accumulate_grad_batches = k > 1 an optimizer step takes k consecutive batches; batches at an epoch's end that do not fill a
    window are not used.  A checkpoint's (`epoch`, `batch_in_epoch`) is the position the run continues at: `resume=path`
    loads through `checkpoint.Checkpointer.load` and continues there.  `max_steps` ends `fit` after that many optimizer steps
    (nothing is saved at that point).

    `model.loss_dict` stays on the device: the 0-d tensors of `log_every` steps are read back together, once, into one row of
    `history` ({"step": the last of them, key: the mean over them}); what is left at the end of `fit` makes a last, shorter row.
    More than one process: every rank loads, rank 0 alone writes, a barrier follows `wait()` (not run on more than one GPU).

    `image_logger` (an `ImageLogger`) is called after every optimizer step (`on_train_batch_end(self, model, batch, i)`, once
    `global_step` has moved; in an accumulation window after the window's step only) and after every `validation_step`; the rows it
    returns go to `image_history`.  `log_dir`: every row of `history`, `val_history` and `image_history` is also appended to
    `log_dir/metrics.jsonl` as it is made.  `current_epoch` is the epoch `fit` is in.  With neither, nothing changes.

    `refresh_weights`: every optimizer step ends with one `WeightRefresher.refresh()` over the optimizer's tensors (the same
    numbers; off by default).  `request_save()` asks for a `last.ckpt` after the optimizer step in progress (it only sets a flag:
    safe to call from a signal handler)."""

    def __init__(self, model, max_epochs, accumulate_grad_batches=1, max_norm=None, scaler=None, ckpt_dir=None, every_n_steps=None,
                 save_top_k=3, seed=0, log_every=50, max_steps=None, image_logger=None, log_dir=None, refresh_weights=False):
        self.refresh_weights, self.refresher, self._save_requested = bool(refresh_weights), None, False
        self.image_logger, self.log_dir, self.image_history, self.current_epoch = image_logger, log_dir, [], 0
        self.model, self.max_epochs, self.accumulate = model, int(max_epochs), int(accumulate_grad_batches)
        self.max_norm, self.scaler, self.ckpt_dir, self.every_n_steps = max_norm, scaler, ckpt_dir, every_n_steps
        self.save_top_k, self.seed, self.log_every, self.max_steps = int(save_top_k), int(seed), int(log_every), max_steps
        self.monitor = getattr(model, "monitor", None)
        self.history, self.val_history = [], []
        self.global_step = 0
        self.best = {}                                # {file name: monitored value (None without one), epoch} of the epoch files kept
        self._pending = []

    # -- logging
    def _emit(self, kind, row):
        """One JSON line per row of `history` / `val_history` / `image_history` ("kind": train | val | images), appended to
        `log_dir/metrics.jsonl` when the row is made: a resumed run continues the file.  Rank 0 alone writes."""
        if self.log_dir is None:
            return
        import json
        import os
        from . import dist as mdist
        if mdist.world()[0] != 0:
            return
        os.makedirs(self.log_dir, exist_ok=True)
        with open(os.path.join(self.log_dir, "metrics.jsonl"), "a") as f:
            f.write(json.dumps({"kind": kind, **row}) + "\n")

    def _log_images(self, hook, batch, batch_idx):
        if self.image_logger is None:
            return
        row = getattr(self.image_logger, hook)(self, self.model, batch, batch_idx)
        if row is not None:
            self.image_history.append(row)
            self._emit("images", row)

    def _flush_log(self):
        if not self._pending:
            return
        keys = sorted(self._pending[0][1])
        vals = torch.stack([torch.stack([d[k].detach().float().reshape(()) for k in keys]) for _, d in self._pending]).cpu()
        row = {"step": self._pending[-1][0]}
        row.update({k: float(vals[:, j].double().mean()) for j, k in enumerate(keys)})
        self.history.append(row)
        self._emit("train", row)
        self._pending = []

    # -- checkpoints
    def request_save(self):
        self._save_requested = True

    def _save(self, name, epoch, batch_in_epoch):
        import os
        from . import dist as mdist
        path = os.path.join(self.ckpt_dir, name)
        if mdist.world()[0] == 0:
            self.checkpointer.save(path, self.global_step, epoch, batch_in_epoch, monitor={"name": self.monitor, "best": dict(self.best)})
        return path

    def _wait(self):
        from . import dist as mdist
        self.checkpointer.wait()
        if mdist.world()[1] > 1:
            import torch.distributed as tdist
            tdist.barrier()

    def _end_of_epoch(self, epoch, val_batches):
        import os
        import shutil
        from . import dist as mdist
        metrics = {}
        if val_batches is not None:
            self.model.eval()
            sums, count = {}, 0
            for batch in val_batches():
                out = self.model.validation_step(batch, count)
                self._log_images("on_validation_batch_end", batch, count)
                for k, v in out.items():
                    sums[k] = v.detach().double() if k not in sums else sums[k] + v.detach().double()
                count += 1
            if count:
                keys = sorted(sums)
                vals = (torch.stack([sums[k].reshape(()) for k in keys]) / count).cpu()
                metrics = {k: float(v) for k, v in zip(keys, vals)}
            self.model.train()
        self.val_history.append({"epoch": epoch, **metrics})
        self._emit("val", self.val_history[-1])
        if self.ckpt_dir is None:
            return
        name = f"epoch={epoch:06d}.ckpt"
        value = metrics.get(self.monitor)
        self.best[name] = {"value": value, "epoch": epoch}
        drop = []
        if self.save_top_k >= 0:
            rank_of = lambda kv: (kv[1]["value"] is None, kv[1]["value"] if kv[1]["value"] is not None else 0.0, -kv[1]["epoch"])
            ranked = sorted(self.best.items(), key=rank_of)
            drop = [k for k, _ in ranked[self.save_top_k:]]
            for k in drop:
                del self.best[k]
        kept = name not in drop                        # (an epoch outside the top k is written once, as `last.ckpt`)
        path = self._save(name if kept else "last.ckpt", epoch + 1, 0)
        self._wait()
        if mdist.world()[0] == 0:
            if kept:
                last = os.path.join(self.ckpt_dir, "last.ckpt")
                shutil.copyfile(path, last + ".tmp")
                os.replace(last + ".tmp", last)
            for k in drop:
                if os.path.exists(os.path.join(self.ckpt_dir, k)):
                    os.remove(os.path.join(self.ckpt_dir, k))

    def fit(self, train_batches, val_batches=None, resume=None):
        import os
        import random
        import numpy as np
        from . import checkpoint
        model, k = self.model, self.accumulate
        if not hasattr(model, "learning_rate"):
            raise AttributeError("set model.learning_rate first (`scaled_lr` is the reference's --scale_lr arithmetic)")
        made = model.configure_optimizers()
        self.optimizer, self.scheduler = (made[0][0], made[1][0]["scheduler"]) if isinstance(made, tuple) else (made, None)
        self.accumulator = GradAccumulator(self.optimizer, k) if k > 1 else None
        self.refresher = WeightRefresher(model, list(self.optimizer.params)) if self.refresh_weights else None
        refresh = {} if self.refresher is None else {"refresh": self.refresher}      # (off: the calls are what they always were)
        self.checkpointer = checkpoint.Checkpointer(model, self.optimizer, self.scheduler, self.scaler, self.accumulator)
        if self.ckpt_dir is not None:
            os.makedirs(self.ckpt_dir, exist_ok=True)
        epoch0 = batch0 = 0
        if resume is not None:
            at = self.checkpointer.load(resume)
            self.global_step, epoch0, batch0 = at["global_step"], at["epoch"], at["batch_in_epoch"]
            self.best = dict((at.get("monitor") or {}).get("best") or {})
        else:
            random.seed(self.seed)
            np.random.seed(self.seed)
            torch.manual_seed(self.seed)
        model.train()
        done = lambda: self.max_steps is not None and self.global_step >= self.max_steps
        for epoch in range(epoch0, self.max_epochs):
            self.current_epoch = epoch
            start = batch0 if epoch == epoch0 else 0
            for i, batch in enumerate(train_batches(epoch, start), start):
                if done():
                    break
                model.training_step(batch, i, scaler=self.scaler, allreduce=k == 1)
                self._pending.append((self.global_step + 1, dict(model.loss_dict)))
                if self.accumulator is not None:
                    self.accumulator.add(model.adapter_grads, scale=model.adapter_grads_scale)
                    if (i + 1) % k:
                        self._pending.pop()            # (a row of the log is an optimizer step: the window's last micro-batch)
                        continue
                    self.accumulator.step(scaler=self.scaler, max_norm=self.max_norm, **refresh)
                else:
                    self.optimizer.step_scaled(model.adapter_grads, scaler=self.scaler, max_norm=self.max_norm, **refresh)
                model.on_train_batch_end()
                if self.scheduler is not None:
                    self.scheduler.step()
                self.global_step += 1
                self._log_images("on_train_batch_end", batch, i)       # (in a window: after its optimizer step only)
                if len(self._pending) >= self.log_every:
                    self._flush_log()
                due = bool(self.every_n_steps) and self.global_step % self.every_n_steps == 0
                if (due or self._save_requested) and self.ckpt_dir is not None:
                    self._save_requested = False
                    self._save("last.ckpt", epoch, i + 1)
            if done():
                break
            if self.accumulator is not None:
                self.accumulator._clear()              # (batches that did not fill a window)
            self._end_of_epoch(epoch, val_batches)
        self._flush_log()
        self._wait()
        return self
