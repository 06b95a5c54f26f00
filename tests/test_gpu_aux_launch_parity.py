"""Every launch and every block of the conditioning producer and the three realism networks against fp64 (`-m gpu`).

The four networks that run on the UNet's and the VAEs' kernels but were judged by one number at their very end:
  * the conditioning producer (FrozenCLIPImageEmbedder: true ViT-L/14 geometry, width 1024, 16 heads x 64, 224 x 224 -> 257 tokens,
    inner 4096, depth 2 -- launch shapes repeat per layer; full depth stays with tests/test_gpu_cond_producer.py): `encode()` with
    ref_image and ref_bbox at batch 3 (ragged 771 rows, 4-wave attention), at the product's batches 8 (8-wave attention from here
    on; its five igemm plans are neither batch 3's nor batch 16's) and 16 (quick_gelu past its 16,777,216-element grid cap), and
    the mapper + bbox MLP alone at 17 rows (skinny_linear's 16-row split plus a 1-row remainder);
  * CLIP score / FID (CLIPScore: ViT-B/32 geometry, 50 tokens, 12 heads x 64, k = 3072 patch product, depth 2): 3 pairs, 32 pairs
    (64 images, FID's batch) and 64 pairs (128 images: 8-wave attention at tq = 50, quick_gelu past the cap), each followed by one
    FrechetStats.update on the embeddings;
  * LPIPS at 256 x 256: 1 pair (the split-K plan), 7 pairs, the tool's 64 pairs (RING256 / RING128 without a split; no batch
    below 55 pairs has these five plans), and 5 pairs of 200 x 296;
  * RangeNet++ (all 67 leaky-ReLU launches, 64 x 1024) at batch 3 and at batch 8, the smallest batch that routes all 67 launches
    as the tool's batch of 64 does (batch 3 differs at 40 of them); inputs through frd_input from frd_ref.synthetic_views.
Every image of a batch is a distinct input; fp16 and bf16.  Per leg, in one pass:
  * launch shadow (tests/launch_shadow.py with extra=EXTRA_KINDS): every launch against the fp64 restatement of its contract within
    its unit test's bound; the census of library calls finds no launch the shadow did not judge;
  * block shadow: each AlexNet tap (F.conv2d / max_pool2d as tests/realism_ref.alexnet_taps), each CLIP encoder layer
    (realism_ref.clip_layer) and each RangeNet stem / down conv / BasicBlock / upconv (frd_ref._cbl / _block) in fp64 with the fp32
    master weights on the stage's own engine input, per image and for the whole batch.  A wrong weight rewrite (padded cin, the
    stride-(1, 2) and transposed-convolution rewrites, the stacked q / k / v matrix) shows here, not in the launch shadow, which
    reads the matrix the kernel reads.
A leg that stands in for a larger production batch (64 pairs for LPIPS, 64 images for RangeNet and the CLIP metrics) must route
every igemm as that batch does: (mobi_igemm_kernel_variant, mobi_igemm_plan_splits) from the query-only entry points, asserted.
Block bounds are per family and dtype, at most 2x the worst measured on the MI355X (BLOCK_BOUND).  Two mutation cases show that
the checks fail: realism.stride2_weight with its two taps swapped (block shadow), and the last ragged 128-row tile of AlexNet
conv1's output overwritten with the tile before it (launch shadow).
MOBI_AUX_LAUNCH_PARITY_TABLE=<file> writes the per-family table (profiles/aux_launch_parity.txt).
"""
import ctypes as C
import functools
import os
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import weights as W
from tests import frd_ref, realism_ref as R
from tests.golden_cases import record
from tests.launch_shadow import EXTRA_KINDS, TILE_ROWS, LaunchShadow, compare

pytestmark = pytest.mark.gpu

T_START = []
DEV = "cuda"
F16, BF16 = torch.float16, torch.bfloat16
DTYPES = {"fp16": F16, "bf16": BF16}
SEED = 29
KERNELS = ("staged128", "staged256", "direct_lds", "pingpong", "ring128", "ring256", "ring128w", "small")   # ops.igemm's tag

VIT_L14_DEPTH2 = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=2, num_attention_heads=16, image_size=224,
                      patch_size=14, projection_dim=768, hidden_act="quick_gelu", layer_norm_eps=1e-5)
CLIP_B32_DEPTH2 = dict(R.CLIP_B32, num_hidden_layers=2)
LPIPS_PRODUCT_PAIRS, METRIC_PRODUCT_IMAGES = 64, 64      # the batches the metric tools run (--batch-size 64)
RANGENET_STANDIN_BATCH = 8                                # smallest batch whose 67 plans are the 64-image batch's (asserted)

# name -> (network, arguments)
LEGS = {"cond_b3": ("cond", dict(batch=3)), "cond_b8": ("cond", dict(batch=8)), "cond_b16": ("cond", dict(batch=16)),
        "cond_rows17": ("cond_rows", dict(rows=17)),
        "clip_p3": ("clip", dict(pairs=3)), "clip_p32": ("clip", dict(pairs=32)), "clip_p64": ("clip", dict(pairs=64)),
        "lpips_p1": ("lpips", dict(pairs=1, h=256, w=256)), "lpips_p7": ("lpips", dict(pairs=7, h=256, w=256)),
        "lpips_p64": ("lpips", dict(pairs=LPIPS_PRODUCT_PAIRS, h=256, w=256)),
        "lpips_p5_200x296": ("lpips", dict(pairs=5, h=200, w=296)),
        "rangenet_b3": ("rangenet", dict(batch=3)),
        f"rangenet_b{RANGENET_STANDIN_BATCH}": ("rangenet", dict(batch=RANGENET_STANDIN_BATCH))}
CASES = [(leg, dn) for leg in LEGS for dn in DTYPES]
CASE_IDS = [f"{leg}-{dn}" for leg, dn in CASES]

# Worst per-image (and whole-batch) rel-L2 of a stage against fp64 with the fp32 master weights, per family and dtype: at most 2x
# the MI355X measurement (profiles/aux_launch_parity.txt; the measured worst is the comment).  "conv" = the AlexNet taps,
# "attn" = the CLIP encoder layers of both towers, "leaky" = RangeNet's stem, down convolutions, BasicBlocks and upconvs.
# Measured worst: fp16 conv 3.44e-4, attn 4.30e-4, leaky 4.44e-4; bf16 conv 2.54e-3, attn 3.46e-3, leaky 3.54e-3.
BLOCK_BOUND = {F16: dict(conv=6.8e-4, attn=8.5e-4, leaky=8.8e-4),
               BF16: dict(conv=5.0e-3, attn=6.9e-3, leaky=7.0e-3)}


def _set(dtype):
    import mobi_amd
    mobi_amd.set_engine_dtype(dtype)


def _rows(t):
    """fp64 NCHW -> [1, n h w, c] for compare()"""
    return t.permute(0, 2, 3, 1).reshape(1, -1, t.shape[1])


# ---- routing (query-only entry points: nothing is launched) --------------------------------------------------------------
def _linear_plan(images, tokens, k, n, dtype, bias=True, residual=False):
    """(kernel variant, split count) of ops.linear on [images, tokens, k] tokens -> n, as ops.igemm fills mobi_igemm_params: the
    split count the library plans is set before the variant is asked (a split launch may take another kernel: fc2 of 128
    ViT-B/32 images is RING128 unsplit and RING256 once split in two)."""
    from mobi_amd import _lib, ops
    q = _lib.IgemmParams()
    q.src0 = q.weight = q.out = q.weight_tiled = 4096                             # placeholders: nothing is launched
    q.bias = 4096 if bias else None
    q.residual = 4096 if residual else None
    q.c0, q.batch, q.hin, q.win, q.hout, q.wout = k, images, tokens, 1, tokens, 1
    q.kh = q.kw = q.stride = q.groups = 1
    q.n_packed = q.cout = n
    q.scale, q.dtype = 1.0, ops._dt(dtype)
    lib = _lib.load()
    splits = lib.mobi_igemm_plan_splits(C.byref(q))
    if splits > 1:
        q.split_k, q.ws = splits, 4096
    return lib.mobi_igemm_kernel_variant(C.byref(q)), splits


def clip_igemm_plan(images, cfg, dtype):
    """The plans of a CLIPVisionTower.pooled pass in launch order: the patch product, then per layer the stacked q / k / v
    projection, out_proj (+ residual), fc1, fc2 (+ residual)."""
    w, inner, p = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"]
    grid = cfg["image_size"] // p
    t = grid * grid + 1
    kp = (3 * p * p + 31) // 32 * 32
    plans = [_linear_plan(images, t - 1, kp, w, dtype, bias=False)]
    for _ in range(cfg["num_hidden_layers"]):
        plans += [_linear_plan(images, t, w, 3 * w, dtype), _linear_plan(images, t, w, w, dtype, residual=True),
                  _linear_plan(images, t, w, inner, dtype), _linear_plan(images, t, inner, w, dtype, residual=True)]
    return plans


def _plan_of(leg, dtype):
    """(the leg's own plan, the plan of the production batch it stands in for or None) from the query-only entry points."""
    from mobi_amd import realism as M
    net, a = LEGS[leg]
    if net == "lpips":
        return M.igemm_plan(a["h"], a["w"], a["pairs"], dtype), None
    if net == "rangenet":
        product = M.rangenet_igemm_plan(METRIC_PRODUCT_IMAGES, dtype) if a["batch"] == RANGENET_STANDIN_BATCH else None
        return M.rangenet_igemm_plan(a["batch"], dtype), product
    if net == "clip":
        return clip_igemm_plan(2 * a["pairs"], CLIP_B32_DEPTH2, dtype), None
    if net == "cond":
        return clip_igemm_plan(a["batch"], VIT_L14_DEPTH2, dtype), None
    return [], None


# ---- models and inputs (built once, shared by the dtypes: packed weights are cached per storage type) ----------------------
@functools.lru_cache(maxsize=None)
def _cond_model():
    from mobi_amd.ldm.modules.encoders.modules import FrozenCLIPImageEmbedder
    enc = FrozenCLIPImageEmbedder(["ref_image", "ref_bbox"], clip_config=VIT_L14_DEPTH2)
    W.fill_module_(enc, seed=SEED)
    return enc.cuda()


@functools.lru_cache(maxsize=None)
def _clip_state():
    return R.clip_b32_state(SEED, CLIP_B32_DEPTH2)


@functools.lru_cache(maxsize=None)
def _clip_model(dn):
    from mobi_amd import realism as M
    return M.CLIPScore.from_state_dict(dict(_clip_state()), dtype=DTYPES[dn], device=DEV)


@functools.lru_cache(maxsize=None)
def _alex():
    from mobi_amd import realism as M
    return M.lpips_state_from_dicts(*R.alex_state(SEED))


@functools.lru_cache(maxsize=None)
def _lpips_model(dn):
    from mobi_amd import realism as M
    return M.LPIPS(*_alex(), dtype=DTYPES[dn], device=DEV)


@functools.lru_cache(maxsize=None)
def _range_views(batch):
    return torch.from_numpy(frd_ref.synthetic_views(batch, seed=SEED)).float()


@functools.lru_cache(maxsize=None)
def _range_state():
    """Seeded RangeNet++ state dicts (fp64, on the device) with the BatchNorm statistics calibrated on the leg's own views, so
    that every layer's activations stay O(1)."""
    bb, dec = frd_ref.seeded_state_dicts(SEED)
    bb, dec = ({k: v.cuda() for k, v in sd.items()} for sd in (bb, dec))
    from mobi_amd.realism import RANGENET_H, RANGENET_W
    x = torch.stack([frd_ref.prepare(v, RANGENET_H, RANGENET_W) for v in _range_views(3).double().numpy()]).double().cuda()
    with torch.backends.cudnn.flags(enabled=False), torch.no_grad():
        frd_ref.forward(bb, dec, x, calib=True)
    return bb, dec


def _build_range_model(dn):
    from mobi_amd import realism as M
    return M.RangeNet.from_state_dicts(*_range_state(), dtype=DTYPES[dn], device=DEV)


_range_model = functools.lru_cache(maxsize=None)(_build_range_model)


# ---- block shadow -----------------------------------------------------------------------------------------------------------
class BlockShadow:
    """Each stage's engine output against fp64 with the fp32 master weights on the stage's own engine input: `results` holds one
    dict(block, family, rel, worst_image, image, finite) per stage call."""

    def __init__(self, mp):
        self.mp, self.results = mp, []

    def _judge(self, name, family, got64, ref64):
        """got64, ref64: fp64 [images, rows, channels]"""
        per = [compare(got64[i:i + 1], ref64[i:i + 1]) for i in range(got64.shape[0])]
        whole = compare(got64.reshape(1, -1, got64.shape[-1]), ref64.reshape(1, -1, ref64.shape[-1]))
        worst = max(range(len(per)), key=lambda i: per[i]["rel"])
        self.results.append(dict(block=name, family=family, rel=whole["rel"], worst_image=per[worst]["rel"], image=worst,
                                 finite=whole["finite"] and all(p["finite"] for p in per)))

    # CLIP encoder layers (both towers)
    def install_clip(self, tower, prefix):
        from mobi_amd.ldm.modules.encoders import modules as E
        sd = {k: v.detach().double() for k, v in tower.state_dict().items()}
        names = {id(m): n for n, m in tower.named_modules()}
        orig, sh = E._EncoderLayer.forward, self

        def forward(mod, x):
            torch.cuda.synchronize()
            x64 = x.double()
            y = orig(mod, x)
            torch.cuda.synchronize()
            with torch.no_grad():
                ref = torch.cat([R.clip_layer(x64[i:i + 1], sd, names[id(mod)] + ".", mod.heads) for i in range(x64.shape[0])])
            sh._judge(f"{prefix}.{names[id(mod)]}", "attn", y.double(), ref)
            return y
        self.mp.setattr(E._EncoderLayer, "forward", forward)
        return self

    # AlexNet taps: relu(conv_j(max_pool(relu(input)))) on the tensor the stage received
    def install_alex(self, model):
        from mobi_amd import ops
        convs = [(w.double().cuda(), b.double().cuda()) for w, b in model.convs]
        index = {id(pw): j for j, pw in enumerate(model.packed)}
        orig_igemm, orig_pool, sh = ops.igemm, ops.maxpool3s2, self
        pooled = {}

        def maxpool(x, relu=False):
            y = orig_pool(x, relu=relu)
            pooled.clear()
            pooled[y.data_ptr()] = x
            return y

        def igemm(x, pw, **kw):
            j = index.get(id(pw))
            if j is None:
                return orig_igemm(x, pw, **kw)
            torch.cuda.synchronize()
            src = pooled.pop(x.data_ptr(), None)
            x64 = (x if src is None else src).double().permute(0, 3, 1, 2)
            if j == 0:
                x64 = x64[:, :3]                                                # conv1's source is zero-padded to 32 channels
            else:
                x64 = torch.relu(x64)
                if src is not None:
                    x64 = F.max_pool2d(x64, 3, 2)
            y = orig_igemm(x, pw, **kw)
            torch.cuda.synchronize()
            s, p = R._ALEX[j]
            with torch.backends.cudnn.flags(enabled=False), torch.no_grad():
                ref = torch.cat([torch.relu(F.conv2d(x64[i:i + 1], *convs[j], stride=s, padding=p)) for i in range(x64.shape[0])])
            n, c = y.shape[0], y.shape[3]
            sh._judge(f"alex.relu{j + 1}", "conv", torch.relu(y.double()).reshape(n, -1, c), ref.permute(0, 2, 3, 1).reshape(n, -1, c))
            return y
        self.mp.setattr(ops, "igemm", igemm)
        self.mp.setattr(ops, "maxpool3s2", maxpool)
        return self

    # RangeNet: stem, down convolutions, BasicBlocks, upconvs
    def install_rangenet(self, bb, dec):
        from mobi_amd import realism as M
        orig_conv, orig_block, sh = M.RangeNet._conv, M.RangeNet._block, self
        inside = []

        def sd_of(name):
            return dec if name.startswith("dec") else bb

        def judge(name, y, ref):
            n, c = ref.shape[0], ref.shape[1]
            sh._judge(name, "leaky", y.double().reshape(n, -1, c), ref.permute(0, 2, 3, 1).reshape(n, -1, c))

        def stage(fn, x64):
            with torch.backends.cudnn.flags(enabled=False), torch.no_grad():
                return torch.cat([fn(x64[i:i + 1]) for i in range(x64.shape[0])])

        def conv(net, x, name, residual=None, **kw):
            if inside:
                return orig_conv(net, x, name, residual=residual, **kw)
            torch.cuda.synchronize()
            n, h, w, c = x.shape
            sd = sd_of(name)
            if name == "conv1":
                x64 = x.double().permute(0, 3, 1, 2)[:, :5]
                fn = lambda v: frd_ref._cbl(v, sd, "conv1", "bn1", False, padding=1)
            elif name.endswith(".upconv"):
                x64 = x.double().permute(0, 3, 1, 2)
                pre = name[:-len(".upconv")]
                fn = lambda v: frd_ref._cbl(v, sd, name, f"{pre}.bn", False, fn=F.conv_transpose2d, stride=(1, 2), padding=(0, 1))
            else:                                                               # enc<i>.conv on the paired view [H][W/2][2C]
                x64 = x.double().reshape(n, h, 2 * w, c // 2).permute(0, 3, 1, 2)
                pre = name[:-len(".conv")]
                fn = lambda v: frd_ref._cbl(v, sd, name, f"{pre}.bn", False, stride=(1, 2), padding=1)
            y = orig_conv(net, x, name, residual=residual, **kw)
            torch.cuda.synchronize()
            judge(name, y, stage(fn, x64))
            return y

        def block(net, x, pre):
            torch.cuda.synchronize()
            x64 = x.double().permute(0, 3, 1, 2)
            inside.append(pre)
            try:
                y = orig_block(net, x, pre)
            finally:
                inside.pop()
            torch.cuda.synchronize()
            judge(pre, y, stage(lambda v: frd_ref._block(v, sd_of(pre), pre, False), x64))
            return y
        self.mp.setattr(M.RangeNet, "_conv", conv)
        self.mp.setattr(M.RangeNet, "_block", block)
        return self


# ---- one pass per leg ---------------------------------------------------------------------------------------------------------
def _cond_inputs(batch):
    """`batch` distinct reference images (fp32 NCHW) and boxes (8 corners x 3) on the device."""
    side = VIT_L14_DEPTH2["image_size"]
    img = torch.cat([W.synth_input(f"auxlp.cond.image.{i}", (1, 3, side, side)) for i in range(batch)])
    box = torch.cat([W.synth_input(f"auxlp.cond.bbox.{i}", (1, 8, 3)) for i in range(batch)])
    return img.cuda(), box.cuda()


def _lpips_inputs(pairs, h, w):
    """`pairs` distinct image pairs in [-1, 1] (fp32 NCHW on the CPU), from near-identical to unrelated."""
    x = R.lpips_images(f"auxlp.lpips.a.{pairs}", pairs, h, w)
    other = R.lpips_images(f"auxlp.lpips.b.{pairs}", pairs, h, w)
    t = torch.linspace(0.05, 1.0, pairs).view(-1, 1, 1, 1)
    return x, ((1 - t) * x + t * other).clamp(-1, 1)


def _run(leg, dn, install=None, mutate=None):
    """One shadowed pass of a leg -> (LaunchShadow, BlockShadow, result of the forward).  `install(mp)`: further patches below
    the shadows (the mutation cases); `mutate`: a model to run in place of the cached one."""
    from mobi_amd import realism as M
    from mobi_amd.ldm.modules.encoders import modules as E
    net, a = LEGS[leg]
    dtype = DTYPES[dn]
    _set(dtype)
    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        if install is not None:
            install(mp)
        bs = BlockShadow(mp)
        if net in ("cond", "cond_rows"):
            enc = _cond_model()
            enc.__dict__.pop("_pooled_cache", None)
            bs.install_clip(enc.transformer, "cond")
            if net == "cond":
                img, box = _cond_inputs(a["batch"])
                fwd = lambda: enc.encode({"ref_image": img, "ref_bbox": box})
            else:
                pooled = W.synth_input("auxlp.cond.pooled", (a["rows"], enc.transformer.width)).cuda()
                box = _cond_inputs(a["rows"])[1]
                fwd = lambda: (E._rows(enc.final_ln, enc.mapper(pooled)), enc.bbox_embedder(box))
        elif net == "clip":
            model = _clip_model(dn)
            bs.install_clip(model.tower, "clip")
            ref = R.clip_images("auxlp.clip.ref", a["pairs"], CLIP_B32_DEPTH2["image_size"]).cuda()
            pred = R.clip_images("auxlp.clip.pred", a["pairs"], CLIP_B32_DEPTH2["image_size"]).cuda()
            embeds, embed = [], model.embed
            mp.setattr(model, "embed", lambda im: (embeds.append(embed(im)), embeds[-1])[1], raising=False)

            def fwd():
                score = model(ref, pred)
                st = M.FrechetStats(embeds[0].shape[1], DEV).update(embeds[0])
                return score, st.sum, st.cross
        elif net == "lpips":
            model = mutate or _lpips_model(dn)
            bs.install_alex(model)
            x, y = (t.cuda() for t in _lpips_inputs(a["pairs"], a["h"], a["w"]))
            fwd = lambda: model(x, y)
        else:
            model = mutate or _range_model(dn)
            bs.install_rangenet(*_range_state())
            views = _range_views(a["batch"])
            fwd = lambda: model.features(views)
        with pytest.MonkeyPatch.context() as mp2:
            with LaunchShadow(mp2, label=f"{leg} {dn}", extra=EXTRA_KINDS) as sh:
                out = fwd()
        torch.cuda.synchronize()
    return sh, bs, out


@functools.lru_cache(maxsize=None)
def _leg(leg, dn):
    t0 = time.time()
    T_START[:] = T_START or [t0]
    sh, bs, _ = _run(leg, dn)
    sec = time.time() - t0
    print(f"[aux {leg} {dn}] one shadowed pass {sec:.1f} s")
    return dict(failures=list(sh.failures), census=sh.census_failures(), counts=dict(sh.counts), calls=dict(sh.calls),
                records=list(sh.records), blocks=list(bs.results), seconds=sec)


@pytest.mark.parametrize("leg,dn", CASES, ids=CASE_IDS)
def test_launch_shadow(leg, dn):
    r = _leg(leg, dn)
    print(f"[aux {leg} {dn}] launches judged {r['counts']}")
    assert sum(r["counts"].values()) > 0
    assert not r["census"], "\n".join(r["census"])
    assert not r["failures"], "\n".join(r["failures"][:40])


def _bad_blocks(blocks, dtype):
    return [b for b in blocks if not (b["finite"] and b["rel"] < BLOCK_BOUND[dtype][b["family"]]
                                      and b["worst_image"] < BLOCK_BOUND[dtype][b["family"]])]


@pytest.mark.parametrize("leg,dn", [c for c in CASES if LEGS[c[0]][0] != "cond_rows"],
                         ids=[i for i, c in zip(CASE_IDS, CASES) if LEGS[c[0]][0] != "cond_rows"])
def test_block_shadow(leg, dn):
    r = _leg(leg, dn)
    net = LEGS[leg][0]
    seen = [b["block"] for b in r["blocks"]]
    if net == "lpips":
        assert seen == [f"alex.relu{j}" for j in range(1, 6)], seen
    elif net in ("cond", "clip"):
        assert seen == [f"{net}.encoder.layers.{i}" for i in range(2)], seen
    else:
        from mobi_amd.realism import RANGENET_BLOCKS
        want = ["conv1"]
        for i, nb in enumerate(RANGENET_BLOCKS, 1):
            want += [f"enc{i}.conv"] + [f"enc{i}.residual_{k}" for k in range(nb)]
        for i in range(5, 0, -1):
            want += [f"dec{i}.upconv", f"dec{i}.residual"]
        assert seen == want, seen
    for b in r["blocks"]:
        tol = BLOCK_BOUND[DTYPES[dn]][b["family"]]
        print(f"[block {leg} {dn}] {b['block']:28s} rel={b['rel']:.3e} worst image={b['worst_image']:.3e} (image {b['image']}) "
              f"bound {tol:.1e}")
        record(f"aux block {leg} {dn} {b['block']}", b["rel"], tol)
        record(f"aux block {leg} {dn} {b['block']} worst_image", b["worst_image"], tol)
    bad = _bad_blocks(r["blocks"], DTYPES[dn])
    assert not bad, bad


def _launched_plan(records):
    """(kernel variant, split count) of a leg's igemm launches in order, from the tags ops.igemm gave the profiler."""
    out = []
    for rec in records:
        if rec["kind"] == "igemm":
            kern = rec["tag"].split()[0][len("kern="):]
            out.append((KERNELS.index(kern), rec["form"]["split"]))
    return out


@pytest.mark.parametrize("dn", list(DTYPES))
def test_routing_is_the_production_batch(dn):
    """The plans of the query-only entry points describe what the legs launched; a leg that stands in for a production batch
    routes every igemm as that batch does; every launch of the production batches' plans is judged in some leg."""
    from mobi_amd import realism as M
    dtype = DTYPES[dn]
    for leg, (net, a) in LEGS.items():
        own, product = _plan_of(leg, dtype)
        if net != "cond_rows":
            assert _launched_plan(_leg(leg, dn)["records"]) == own, leg
        if product is not None:
            assert own == product, (leg, [j for j in range(len(own)) if own[j] != product[j]])
    # the smallest stand-in: no smaller RangeNet batch has the 64-image plans (batch 3 is a leg of its own)
    product = M.rangenet_igemm_plan(METRIC_PRODUCT_IMAGES, dtype)
    assert all(M.rangenet_igemm_plan(b, dtype) != product for b in range(1, RANGENET_STANDIN_BATCH))
    # LPIPS: the tool's 64 pairs are a leg themselves
    product = M.igemm_plan(256, 256, LPIPS_PRODUCT_PAIRS, dtype)
    assert _plan_of("lpips_p64", dtype)[0] == product
    # the CLIP metrics: 64 images (FID, the clip_p32 leg) and 64 pairs (CLIP score, the clip_p64 leg) are legs themselves
    assert _plan_of("clip_p32", dtype)[0] == clip_igemm_plan(METRIC_PRODUCT_IMAGES, CLIP_B32_DEPTH2, dtype)
    assert _plan_of("clip_p64", dtype)[0] == clip_igemm_plan(2 * METRIC_PRODUCT_IMAGES, CLIP_B32_DEPTH2, dtype)
    # LPIPS: the plans of test_realism_cpu (64 pairs without a split, 1 pair with split-K)
    assert all(s == 1 for _, s in product) and any(s > 1 for _, s in _plan_of("lpips_p1", dtype)[0])


def _ig(r):
    return r["kind"] == "igemm"


# kernel forms the legs must route to somewhere: a routing change that removes one must update this list explicitly.
# (A split-K igemm here is reduced inside its own library call -- no GroupNorm consumes it, so no Deferred and no separate
# `split_finish` record -- and is judged after the reduction, as the launch and its finish together.)
REQUIRED_FORMS = {
    "igemm stride 4, 11 x 11 on a padded-cin source": lambda r: (_ig(r) and r["form"]["stride"] == 4 and r["form"]["kh"] == 11
                                                                  and r["form"]["kw"] == 11 and r["form"]["cin"] == 32),
    "igemm 5 x 5 pad 2": lambda r: _ig(r) and (r["form"]["kh"], r["form"]["kw"]) == (5, 5) and r["form"]["pad"] == (2, 2),
    "igemm split-K with its reduction": lambda r: (_ig(r) and r["form"]["split"] > 1) or r["kind"] == "split_finish",
    "igemm leaky 3 x 2 on the paired view": lambda r: _ig(r) and r["form"]["leaky"] and (r["form"]["kh"], r["form"]["kw"]) == (3, 2),
    "igemm leaky 1 x 3 (upconv)": lambda r: _ig(r) and r["form"]["leaky"] and (r["form"]["kh"], r["form"]["kw"]) == (1, 3),
    "igemm leaky with residual": lambda r: _ig(r) and r["form"]["leaky"] and r["form"]["residual"],
    "igemm k = 608 (the padded 588 patch product)": lambda r: _ig(r) and r["form"]["k"] == 608,
    "attention 4-wave blocks": lambda r: r["kind"] == "attention" and _attention_blocks(r) < 256,
    "attention 8-wave blocks, dh = 64, tk = 257": lambda r: (r["kind"] == "attention" and _attention_blocks(r) >= 256
                                                            and " dh=64" in r["tag"] and " tk=257 " in r["tag"]),
    "attention 8-wave blocks, tq = 50": lambda r: (r["kind"] == "attention" and _attention_blocks(r) >= 256
                                                  and " tq=50 " in r["tag"]),
    "quick_gelu past 16,777,216 elements": lambda r: r["kind"] == "quick_gelu" and r["form"]["n"] > 16777216,
    "skinny_linear with a 1-row remainder": lambda r: r["kind"] == "skinny_linear" and r["form"]["remainder"] == 1
                                                       and r["form"]["calls"] == 2,
    "lpips_distance with relu_in_place": lambda r: r["kind"] == "lpips_distance" and r["form"]["relu_in_place"],
    "lpips_distance without relu_in_place": lambda r: r["kind"] == "lpips_distance" and not r["form"]["relu_in_place"],
    "band_mean with a skip": lambda r: r["kind"] == "band_mean" and r["form"]["skip"],
    "feature_moments with a shift": lambda r: r["kind"] == "feature_moments" and r["form"]["shift"],
    "feature_moments without a shift": lambda r: r["kind"] == "feature_moments" and not r["form"]["shift"],
}


def _attention_blocks(rec):
    """The blocks of 128 queries a launch_attention_v launch would have with 4 waves (2 per 257- or 50-token image and head):
    from 256 on the library takes 8-wave blocks (mobi_amd/csrc: launch_attention_v)."""
    f = {k: int(v) for k, v in (p.split("=") for p in rec["tag"].split() if "=" in p)}
    return (f["tq"] + 127) // 128 * f["heads"] * f["n"]


def test_launch_shadow_covers_the_routing():
    """Every REQUIRED_FORMS entry judged at least once across the legs; the worst rel-L2 / tile per launch kind, leg and dtype and
    the worst block per family printed (and written to MOBI_AUX_LAUNCH_PARITY_TABLE), with the file's wall time so far."""
    recs = [rec for leg, dn in CASES for rec in _leg(leg, dn)["records"]]
    for form, pred in REQUIRED_FORMS.items():
        assert any(pred(rec) for rec in recs), form
    lines = [f"{'leg':24s} {'launch kind':20s} {'launches':>8s} {'worst rel-L2':>12s} {'worst tile':>10s} {'bound':>7s}"]
    for leg, dn in CASES:
        worst = {}
        for rec in _leg(leg, dn)["records"]:
            fam = rec["kind"] + (" leaky" if rec["form"].get("leaky") else "")
            w = worst.setdefault(fam, [0.0, 0.0, 0, rec["bound"]])
            w[0], w[1], w[2], w[3] = max(w[0], rec["rel"]), max(w[1], rec["tile"]), w[2] + 1, max(w[3], rec["bound"])
        for fam, (rel, tile, cnt, bound) in sorted(worst.items()):
            lines.append(f"{leg + ' ' + dn:24s} {fam:20s} {cnt:8d} {rel:12.3e} {tile:10.3e} {bound:7.1e}")
    lines.append("")
    lines.append(f"{'leg':24s} {'block family':>12s} {'blocks':>6s} {'worst (image or batch)':>22s} {'bound':>7s} {'pass':>6s}")
    family_worst = {}
    for leg, dn in CASES:
        r = _leg(leg, dn)
        for fam in ("conv", "attn", "leaky"):
            bs = [max(b["worst_image"], b["rel"]) for b in r["blocks"] if b["family"] == fam]
            if bs:
                lines.append(f"{leg + ' ' + dn:24s} {fam:>12s} {len(bs):6d} {max(bs):22.3e} {BLOCK_BOUND[DTYPES[dn]][fam]:7.1e} "
                             f"{r['seconds']:5.1f}s")
                family_worst[(fam, dn)] = max(family_worst.get((fam, dn), 0.0), max(bs))
    lines.append("")
    for (fam, dn), v in sorted(family_worst.items()):
        lines.append(f"worst {fam:5s} {dn}: {v:.3e} (bound {BLOCK_BOUND[DTYPES[dn]][fam]:.1e})")
    lines.append(f"wall time of the file so far: {time.time() - T_START[0]:.0f} s")
    print("\n".join(lines))
    path = os.environ.get("MOBI_AUX_LAUNCH_PARITY_TABLE")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


# ---- the checks can fail ---------------------------------------------------------------------------------------------------
def test_block_shadow_fails_on_swapped_stride2_taps():
    """realism.stride2_weight with its two taps swapped: every launch is right on the matrix it reads, the enc*.conv stages are
    not the stride-(1, 2) convolutions of the master weights."""
    from mobi_amd import realism as M
    leg, dn = "rangenet_b3", "fp16"
    orig = M.stride2_weight
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(M, "stride2_weight", lambda w: orig(w).flip(3))
        model = _build_range_model(dn)
    sh, bs, _ = _run(leg, dn, mutate=model)
    bad = {b["block"] for b in _bad_blocks(bs.results, DTYPES[dn])}
    print(f"[mutation stride2] {len(bad)} of {len(bs.results)} stages fail: {sorted(bad)}")
    assert {f"enc{i}.conv" for i in range(1, 6)} <= bad, "the block shadow passed a down convolution with swapped taps"
    assert not sh.failures, sh.failures[:8]                                     # the launches are right on what they read
    r = _leg(leg, dn)
    assert not _bad_blocks(r["blocks"], DTYPES[dn]) and not r["failures"]       # and passes without the fault


def test_launch_shadow_fails_on_a_repeated_tile():
    """The last, ragged 128-row tile of AlexNet conv1's output overwritten with the tile before it after the launch: a wrong
    number, in bounds; the launch shadow must name that launch's worst tile.  Whether the end-to-end LPIPS still lies within
    its bound is printed (information, not an assertion)."""
    from mobi_amd import ops
    from tests.test_gpu_realism import LPIPS_BOUND
    leg, dn = "lpips_p1", "fp16"
    conv1 = _lpips_model(dn).packed[0]
    orig = ops.igemm

    def repeat_tile(x, pw, **kw):
        y = orig(x, pw, **kw)
        if pw is conv1:
            rows = y.reshape(-1, y.shape[-1])
            last = (rows.shape[0] - 1) // TILE_ROWS * TILE_ROWS
            rows[last:] = rows[last - TILE_ROWS:last - TILE_ROWS + rows.shape[0] - last].clone()
        return y
    sh, _, got = _run(leg, dn, install=lambda mp: mp.setattr(ops, "igemm", repeat_tile))
    print("[mutation tile] " + "\n".join(sh.failures[:4]))
    # conv1's output is [2, 63 x 63, 64]: flat rows 7936, 7937 are rows 3967, 3968 of image 1; the one-row tile at 3968 is all wrong
    hit = [f for f in sh.failures if "tap=11x11" in f and "worst tile" in f and "at (1, 3968, 0)" in f]
    assert hit, sh.failures
    a = LEGS[leg][1]
    want = R.lpips(*_lpips_inputs(a["pairs"], a["h"], a["w"]), *_alex())
    d = float((got.cpu().double() - want).abs().max())
    print(f"[mutation tile] end-to-end LPIPS is off fp64 by {d:.2e}: {'within' if d <= LPIPS_BOUND[F16][0] else 'outside'} "
          f"LPIPS_BOUND {LPIPS_BOUND[F16][0]:.0e} per pair")
    assert not _leg(leg, dn)["failures"]                                        # and passes without the fault
