"""Every launch and every block of the VAEs against fp64, at the batch the product runs (`-m gpu`).

The full-width VAEs of tests/test_gpu_production.py (ch = 128, seed 23), camera and lidar:
  * decode, latent 64 x 64 -> 512 x 512, batch 8 (the objects of one GPU), fp16 and bf16 with their default routing (fp16: fp32
    streams, precise level 2, precise tail; bf16: the 16-bit path), clamped to [-1, 1] as decode_first_stage does;
  * encode, 512 x 512 -> moments 64 x 64, batch 8, fp16 and bf16;
  * decode, latent 32 x 32 -> 256 x 256, batch 3, fp16 forced through every decoder routing (module globals, as
    test_vae_decoder_precision_levels sets them): level 2, level 1, level 0 on fp32 streams, the fp32 trunk without streams,
    the plain 16-bit path.
Every image of a batch is a distinct input.  Per leg, in one pass:
  * launch shadow (tests/launch_shadow.py): every launch against the fp64 restatement of its contract within its unit test's
    bound; the census of library calls finds no launch the shadow did not judge;
  * block shadow: every ResnetBlock / AttnBlock / Upsample / Downsample call, conv_in and the encoder's and decoder's tails
    against oracle/vae.py in fp64 on the device, on the block's engine input, with the fp32 master weights; each image on its
    own and the whole batch.  A wrong packed_dup3 / packed_dup / thin-split weight shows here, not in the launch shadow (which
    reads the matrix the kernel reads);
  * output: each decoded picture / range view and each image's moments against the oracle run on that image alone.
Block and output bounds are per routing and dtype, at most 2x the worst measured on the MI355X (BLOCK_BOUND / OUT_BOUND).
Two mutation cases show that the checks fail: decoder weights [W ; W ; 0] in place of [W ; W ; W - T(W)] (block shadow), and
the mid attention's score launch with w_group_stride = 0 (launch shadow).
MOBI_VAE_LAUNCH_PARITY_TABLE=<file> writes the per-family table (profiles/vae_launch_parity.txt).
"""
import functools
import os
import time

import pytest
import torch
import torch.nn.functional as F

from oracle import vae as ovae, weights as W
from tests.golden_cases import record
from tests.launch_shadow import LaunchShadow, compare
from tests.test_gpu_models import _set, _vae

pytestmark = pytest.mark.gpu

T_START = []                    # when the first leg ran: the file's wall time is reported from there
SEED = 23
F16, BF16 = torch.float16, torch.bfloat16
# routing -> (_TRUNK_ENV, _STREAMS_ENV, _PRECISE_ENV, _TAIL_ENV) of mobi_amd/ldm/modules/diffusionmodules/model.py
ROUTINGS = {"level2": ("1", "1", "2", ""), "level1": ("1", "1", "1", ""), "level0": ("1", "1", "0", "0"),
            "trunk": ("1", "0", "", ""), "plain": ("0", "0", "", "0"), "default": None}
# name -> (decode | encode, lidar, image side, batch, dtype, routing)
LEGS = {}
for _lid, _mod in ((False, "camera"), (True, "lidar")):
    for _dt, _dn in ((F16, "fp16"), (BF16, "bf16")):
        LEGS[f"decode512_b8_{_mod}_{_dn}"] = ("decode", _lid, 512, 8, _dt, "default")
        LEGS[f"encode512_b8_{_mod}_{_dn}"] = ("encode", _lid, 512, 8, _dt, "default")
    for _r in ("level2", "level1", "level0", "trunk", "plain"):
        LEGS[f"decode256_b3_{_mod}_{_r}"] = ("decode", _lid, 256, 3, F16, _r)


def _routing_key(leg):
    kind, _, _, _, dtype, routing = LEGS[leg]
    if kind == "encode":
        return ("encode", "-", dtype)
    if routing == "default":
        routing = "level2" if dtype == F16 else "plain"
    return ("decode", routing, dtype)


# Worst per-image (and whole-batch) rel-L2 per routing and dtype, at most 2x the MI355X measurement (profiles/vae_launch_parity.txt).
# Blocks by family: "conv" = ResnetBlocks, up / downsampling, conv_in, norm_out_lidar1; "attn" = mid.attn_1 (q / k / v, the scores
# and P in the storage type at every level); "tail" = norm_out + swish + conv_out (its weights rounded once, [W ; W] at level 2).
# At level 2 a ResnetBlock is ~1e-6: a weight form wrong by 1e-3 per convolution fails by orders of magnitude.
BLOCK_BOUND = {("decode", "level2", F16): dict(conv=2.8e-6, attn=2.0e-4, tail=4.4e-4),
               ("decode", "level1", F16): dict(conv=4.3e-4, attn=1.9e-4, tail=4.4e-4),
               ("decode", "level0", F16): dict(conv=6.0e-4, attn=1.9e-4, tail=6.1e-4),
               ("decode", "trunk", F16): dict(conv=6.4e-4, attn=2.2e-4, tail=8.1e-4),
               ("decode", "plain", F16): dict(conv=8.1e-4, attn=4.6e-4, tail=6.1e-4),
               ("decode", "plain", BF16): dict(conv=6.5e-3, attn=3.6e-3, tail=4.9e-3),
               ("encode", "-", F16): dict(conv=8.5e-4, attn=4.5e-4, tail=7.0e-4),
               ("encode", "-", BF16): dict(conv=6.8e-3, attn=3.6e-3, tail=5.7e-3)}
OUT_BOUND = {("decode", "level2", F16): 5.5e-4, ("decode", "level1", F16): 1.7e-3, ("decode", "level0", F16): 2.5e-3,
             ("decode", "trunk", F16): 2.8e-3, ("decode", "plain", F16): 3.9e-3, ("decode", "plain", BF16): 3.1e-2,
             ("encode", "-", F16): 3.5e-3, ("encode", "-", BF16): 2.8e-2}


def _family(block):
    return "attn" if block.endswith("attn_1") else "tail" if block.endswith(".tail") else "conv"


def _dname(dtype):
    return "fp16" if dtype == F16 else "bf16"


def _cfg(lidar):
    return ovae.VAEConfig(in_channels=2 if lidar else 3, out_ch=2 if lidar else 3, ch=128, lidar_adapter=lidar)


@functools.lru_cache(maxsize=None)
def _model(lidar):
    vae = _vae(_cfg(lidar), res=512)
    vae.load_state_dict(W.synth_state_dict(ovae.vae_param_shapes(_cfg(lidar)), SEED))
    return vae.cuda()


@functools.lru_cache(maxsize=None)
def _sd64(lidar):
    return {k: v.detach().double() for k, v in _model(lidar).state_dict().items()}


def _input(kind, lidar, side, batch):
    """fp32 NCHW on the CPU: `batch` distinct images (one synth_input name per image), never a repeated one."""
    if kind == "decode":
        parts = [W.synth_input(f"vaelp.z.{int(lidar)}.{side}.{i}", (1, 4, side // 8, side // 8)) for i in range(batch)]
    else:
        parts = [W.synth_input(f"vaelp.x.{int(lidar)}.{side}.{i}", (1, _cfg(lidar).in_channels, side, side), kind="uniform")
                 for i in range(batch)]
    return torch.cat(parts)


@functools.lru_cache(maxsize=None)
def _oracle_out(kind, lidar, side, batch):
    """The oracle on each image alone, fp64 on the device (dtype-independent: shared by the legs)."""
    sd, cfg = _sd64(lidar), _cfg(lidar)
    x = _input(kind, lidar, side, batch).double().cuda()
    with torch.backends.cudnn.flags(enabled=False), torch.no_grad():
        if kind == "decode":
            return torch.cat([ovae.decode(sd, cfg, x[i:i + 1]).clamp(-1.0, 1.0) for i in range(batch)])
        return torch.cat([ovae.encode_moments(sd, cfg, x[i:i + 1]) for i in range(batch)])


# ---- block shadow -----------------------------------------------------------------------------------------------------
def _nchw64(t):
    """an engine tensor (channels-last, 16-bit or fp32) -> fp64 NCHW"""
    return t.double().permute(0, 3, 1, 2)


def _rows(t):
    """fp64 NCHW -> [1, n h w, c] for compare()"""
    return t.permute(0, 2, 3, 1).reshape(1, -1, t.shape[1])


class BlockShadow:
    """Wraps the VAE's block methods (monkeypatch): each call's output against oracle/vae.py on the call's engine input; the
    stages that run inline between block calls (conv_in, the decoder's upsampling convolutions on the fp32 stream / trunk, the
    lidar decoder's norm_out_lidar1, the tails) against the oracle on the previous block's output."""

    def __init__(self, mp, vae, sd):
        from mobi_amd.ldm.modules.diffusionmodules import model as M
        self.M, self.mp, self.sd = M, mp, sd
        self.names = {id(m): name for name, m in vae.named_modules()}
        self.results, self.pending, self.last = [], None, None

    def install(self):
        M, sh = self.M, self
        for cls, meths in ((M.ResnetBlock, ("forward", "forward_trunk", "forward_stream", "forward_precise")),
                           (M.AttnBlock, ("forward", "forward_stream")), (M.Upsample, ("forward",)), (M.Downsample, ("forward",)),
                           (M.Encoder, ("forward",)), (M.Decoder, ("forward",))):
            for meth in meths:
                orig = getattr(cls, meth)
                self.mp.setattr(cls, meth, (lambda o, m: lambda mod, *a, **k: sh._call(o, m, mod, *a, **k))(orig, meth))
        return self

    def _judge(self, name, got64, ref64):
        per = [compare(_rows(got64[i:i + 1]), _rows(ref64[i:i + 1])) for i in range(got64.shape[0])]
        whole = compare(_rows(got64), _rows(ref64))
        worst = max(range(len(per)), key=lambda i: per[i]["rel"])
        self.results.append(dict(block=name, rel=whole["rel"], worst_image=per[worst]["rel"], image=worst,
                                 finite=whole["finite"] and all(p["finite"] for p in per)))

    def _ref_block(self, name, x64):
        fn = ovae.attn_block if name.endswith("attn_1") else ovae.resnet_block
        with torch.backends.cudnn.flags(enabled=False):
            return torch.cat([fn(self.sd, name, x64[i:i + 1]) for i in range(x64.shape[0])])

    def _stage(self, fn, x64):
        with torch.backends.cudnn.flags(enabled=False):
            return torch.cat([fn(x64[i:i + 1]) for i in range(x64.shape[0])])

    def _gn_swish(self, p, x):
        return ovae._swish(ovae._gn(self.sd, p, x))

    def _check_pending(self, x64):
        if self.pending is not None:
            name, ref = self.pending
            self._judge(name, x64, ref)
            self.pending = None

    def _call(self, orig, meth, mod, *a, **k):
        M, sd = self.M, self.sd
        name = self.names[id(mod)]
        torch.cuda.synchronize()
        if isinstance(mod, M.Encoder) or isinstance(mod, M.Decoder):
            x64 = a[0].double()
            cin = [c for c in ("conv_in", "conv_in_lidar") if hasattr(mod, c)][0]
            self.pending = (f"{name}.{cin}", self._stage(lambda v: ovae._conv(sd, f"{name}.{cin}", v), x64))
            y = orig(mod, *a, **k)
            torch.cuda.synchronize()
            last = self.last
            if isinstance(mod, M.Decoder):
                norm, conv = ("norm_out_lidar2", "conv_out_lidar") if mod.lidar_adapter else ("norm_out", "conv_out")
            else:
                norm, conv = "norm_out", "conv_out"
            ref = self._stage(lambda v: ovae._conv(sd, f"{name}.{conv}", self._gn_swish(f"{name}.{norm}", v)), last)
            clamp = k.get("clamp", a[1] if len(a) > 1 else None) if isinstance(mod, M.Decoder) else None
            if clamp is not None:
                ref = ref.clamp(*clamp)
            self._judge(f"{name}.tail", y.double(), ref)
            self.last = self.pending = None
            return y
        trunk_in = meth == "forward_trunk" or (meth == "forward" and isinstance(mod, M.AttnBlock) and k.get("trunk") is not None)
        if trunk_in:
            x64 = _nchw64(k["trunk"] if "trunk" in k else a[1]).clone()
        else:
            x64 = _nchw64(a[0])
        if isinstance(mod, (M.Upsample, M.Downsample)):
            self.pending = None
            y = orig(mod, *a, **k)
            torch.cuda.synchronize()
            if isinstance(mod, M.Upsample):
                ref = self._stage(lambda v: ovae._conv(sd, f"{name}.conv", F.interpolate(v, scale_factor=2.0, mode="nearest")), x64)
            else:
                ref = self._stage(lambda v: ovae._conv(sd, f"{name}.conv", F.pad(v, (0, 1, 0, 1)), stride=2, padding=0), x64)
            out64 = _nchw64(y)
            self._judge(name, out64, ref)
            self.last = out64
            return y
        self._check_pending(x64)
        y = orig(mod, *a, **k)
        torch.cuda.synchronize()
        out64 = _nchw64(y[1] if trunk_in else y).clone()
        self._judge(name, out64, self._ref_block(name, x64))
        self.last = out64
        self._set_next(name, out64)
        return y

    def _set_next(self, name, out64):
        """the inline stage after this block, judged on the next block's input"""
        sd = self.sd
        parts = name.split(".")
        if parts[0] == "decoder" and parts[1] == "up" and parts[2] != "0":
            lvl, blk = int(parts[2]), int(parts[4])
            if f"decoder.up.{lvl}.block.{blk + 1}.norm1.weight" not in sd:
                p = f"decoder.up.{lvl}.upsample"
                self.pending = (p, self._stage(lambda v: ovae._conv(sd, f"{p}.conv", F.interpolate(v, scale_factor=2.0,
                                                                                                      mode="nearest")), out64))
        elif name == "decoder.res_block_lidar1":
            self.pending = ("decoder.norm_out_lidar1", self._stage(lambda v: self._gn_swish("decoder.norm_out_lidar1", v),
                                                                   out64))


# ---- one pass per leg ---------------------------------------------------------------------------------------------------
def _route(mp, routing):
    from mobi_amd.ldm.modules.diffusionmodules import model as M
    if ROUTINGS[routing] is not None:
        for attr, val in zip(("_TRUNK_ENV", "_STREAMS_ENV", "_PRECISE_ENV", "_TAIL_ENV"), ROUTINGS[routing]):
            mp.setattr(M, attr, val)


def _forward(vae, kind, x):
    if kind == "decode":
        return vae.decode(x, clamp=(-1.0, 1.0))
    return vae.encode(x).parameters


@functools.lru_cache(maxsize=None)
def _leg(leg):
    kind, lidar, side, batch, dtype, routing = LEGS[leg]
    t0 = time.time()
    T_START[:] = T_START or [t0]
    _set(dtype)
    vae, sd = _model(lidar), _sd64(lidar)
    x = _input(kind, lidar, side, batch).cuda()
    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        _route(mp, routing)
        bs = BlockShadow(mp, vae, sd).install()
        with pytest.MonkeyPatch.context() as mp2:
            with LaunchShadow(mp2, label=leg) as sh:
                y = _forward(vae, kind, x)
        torch.cuda.synchronize()
    want = _oracle_out(kind, lidar, side, batch)
    per = [compare(_rows(y[i:i + 1].double()), _rows(want[i:i + 1])) for i in range(batch)]
    print(f"[vae {leg}] one shadowed pass {time.time() - t0:.1f} s")
    return dict(failures=list(sh.failures), census=sh.census_failures(), counts=dict(sh.counts), calls=dict(sh.calls),
                records=list(sh.records), blocks=list(bs.results), out=[p["rel"] for p in per],
                out_finite=all(p["finite"] for p in per))


@pytest.mark.parametrize("leg", list(LEGS))
def test_launch_shadow(leg):
    r = _leg(leg)
    print(f"[vae {leg}] launches judged {r['counts']}")
    assert r["counts"].get("igemm", 0) > 0 and r["counts"].get("groupnorm", 0) > 0 and r["counts"].get("softmax_rows", 0) > 0
    assert not r["census"], "\n".join(r["census"])
    assert not r["failures"], "\n".join(r["failures"][:40])


@pytest.mark.parametrize("leg", list(LEGS))
def test_block_shadow(leg):
    r = _leg(leg)
    bounds = BLOCK_BOUND[_routing_key(leg)]
    vae = _model(LEGS[leg][1])
    want = {n for n, m in vae.named_modules() if type(m).__name__ in ("ResnetBlock", "AttnBlock")
            and n.startswith("decoder" if LEGS[leg][0] == "decode" else "encoder")}
    seen = {b["block"] for b in r["blocks"]}
    assert want <= seen, sorted(want - seen)
    assert any(b["block"].endswith(".tail") for b in r["blocks"]) and any(b["block"].endswith("conv_in") or
                                                                          b["block"].endswith("conv_in_lidar") for b in r["blocks"])
    bad = []
    for b in r["blocks"]:
        tol = bounds[_family(b["block"])]
        print(f"[block {leg}] {b['block']:32s} rel={b['rel']:.3e} worst image={b['worst_image']:.3e} (image {b['image']}) "
              f"bound {tol:.1e}")
        record(f"vae block {leg} {b['block']}", b["rel"], tol)
        record(f"vae block {leg} {b['block']} worst_image", b["worst_image"], tol)
        if not (b["finite"] and b["rel"] < tol and b["worst_image"] < tol):
            bad.append(b)
    assert not bad, bad


@pytest.mark.parametrize("leg", list(LEGS))
def test_output_per_image(leg):
    r = _leg(leg)
    tol = OUT_BOUND[_routing_key(leg)]
    for i, e in enumerate(r["out"]):
        print(f"[output {leg}] image {i} rel={e:.3e}")
        record(f"vae output {leg} image {i}", e, tol)
    assert r["out_finite"] and max(r["out"]) < tol, (r["out"], tol)


# kernel forms the legs must route to somewhere: a routing change that removes one must update this list explicitly
REQUIRED_FORMS = {
    "igemm per-image S (OUT_ROWS_F32)": lambda r: r["kind"] == "igemm" and r["form"].get("per_image") and r["form"]["out_mode"] == 2,
    "igemm per-image PV": lambda r: r["kind"] == "igemm" and r["form"].get("per_image") and r["form"]["out_mode"] == 0,
    "igemm OUT_TRANSPOSED": lambda r: r["kind"] == "igemm" and r["form"].get("out_mode") == 1,
    "igemm upsample": lambda r: r["kind"] == "igemm" and r["form"].get("upsample"),
    "igemm stride 2, pad (0, 1, 0, 1)": lambda r: (r["kind"] == "igemm" and r["form"].get("stride") == 2 and r["form"]["pad"] == (0, 0)
                                                  and r["form"]["hout"] == (r["form"]["hin"] + 1 - 3) // 2 + 1),
    "igemm thin input conv": lambda r: r["kind"] == "igemm" and r["form"].get("thin") == 1,
    "igemm thin split-latent conv": lambda r: r["kind"] == "igemm" and r["form"].get("thin", 0) >= 2,
    "groupnorm GN_OUT_SPLIT3": lambda r: r["kind"] == "groupnorm" and r["form"].get("out_mode") == 3,
    "groupnorm GN_OUT_SPLIT": lambda r: r["kind"] == "groupnorm" and r["form"].get("out_mode") == 1,
    "groupnorm GN_OUT_F32": lambda r: r["kind"] == "groupnorm" and r["form"].get("out_mode") == 2,
    "split_f32 2 parts": lambda r: r["kind"] == "split_f32" and r["form"]["parts"] == 2,
    "split_f32 3 parts": lambda r: r["kind"] == "split_f32" and r["form"]["parts"] == 3,
    "conv_small_cout tap-major": lambda r: r["kind"] == "conv_small_cout" and not r["form"]["dup"],
    "conv_small_cout packed_dup + clamp 3x3": lambda r: (r["kind"] == "conv_small_cout" and r["form"]["dup"] and r["form"]["clamp"]
                                                        and r["form"]["kh"] == 3),
    "conv_small_cout packed_dup + clamp 1x5": lambda r: (r["kind"] == "conv_small_cout" and r["form"]["dup"] and r["form"]["clamp"]
                                                        and (r["form"]["kh"], r["form"]["kw"]) == (1, 5)),
    "conv_small_cin": lambda r: r["kind"] == "conv_small_cin",
}


def test_launch_shadow_covers_the_routing():
    """Every REQUIRED_FORMS entry judged at least once across the legs; the worst rel-L2 / tile per launch family, leg and dtype
    printed (and written to MOBI_VAE_LAUNCH_PARITY_TABLE), with the file's wall time so far."""
    recs = [(leg, rec) for leg in LEGS for rec in _leg(leg)["records"]]
    for form, pred in REQUIRED_FORMS.items():
        assert any(pred(rec) for _, rec in recs), form
    worst = {}
    for leg, rec in recs:
        fam = rec["kind"]
        if rec["kind"] == "igemm":
            fam += " " + rec["tag"].split()[0][5:] + (" per_image" if rec["form"].get("per_image") else "") + \
                f" mode={rec['form'].get('out_mode')}"
        elif rec["kind"] == "groupnorm":
            fam += f" out_mode={rec['form'].get('out_mode')}{rec['extra']}"
        elif rec["kind"] in ("conv_small_cout", "split_f32"):
            fam += " " + " ".join(f"{k}={int(v)}" for k, v in sorted(rec["form"].items()))
        w = worst.setdefault((leg, fam), [0.0, 0.0, 0, rec["bound"]])
        w[0], w[1], w[2] = max(w[0], rec["rel"]), max(w[1], rec["tile"]), w[2] + 1
    lines = [f"{'leg':32s} {'launch family':44s} {'launches':>8s} {'worst rel-L2':>12s} {'worst tile':>10s} {'bound':>7s}"]
    for (leg, fam), (rel, tile, cnt, bound) in sorted(worst.items()):
        lines.append(f"{leg:32s} {fam:44s} {cnt:8d} {rel:12.3e} {tile:10.3e} {bound:7.1e}")
    lines.append("")
    lines.append(f"{'leg':32s} {'routing':20s} {'block family':>12s} {'blocks':>6s} {'worst (image)':>13s} {'bound':>7s}")
    for leg in LEGS:
        r = _leg(leg)
        key = _routing_key(leg)
        route = f"{key[0]} {key[1]} {_dname(key[2])}"
        for fam in ("conv", "attn", "tail"):
            bs = [max(b["worst_image"], b["rel"]) for b in r["blocks"] if _family(b["block"]) == fam]
            lines.append(f"{leg:32s} {route:20s} {fam:>12s} {len(bs):6d} {max(bs):13.3e} {BLOCK_BOUND[key][fam]:7.1e}")
        lines.append(f"{leg:32s} {route:20s} {'output':>12s} {len(r['out']):6d} {max(r['out']):13.3e} {OUT_BOUND[key]:7.1e}")
    lines.append(f"wall time of the file so far: {time.time() - T_START[0]:.0f} s")
    print("\n".join(lines))
    path = os.environ.get("MOBI_VAE_LAUNCH_PARITY_TABLE")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


# ---- the checks can fail ---------------------------------------------------------------------------------------------------
MUT_LEG = "decode256_b3_camera_level2"


def test_block_shadow_fails_on_zeroed_weight_correction(monkeypatch):
    """Conv2d.packed_dup3 returning [W ; W ; 0] (the weights' rounding left uncorrected): the launches are all right on the
    matrix they read, the block shadow is not."""
    from mobi_amd import ops
    from mobi_amd.ldm.modules.diffusionmodules.util import Conv2d
    kind, lidar, side, batch, dtype, routing = LEGS[MUT_LEG]
    _set(dtype)
    vae, sd = _model(lidar), _sd64(lidar)

    def zero_third(self):
        def build():
            w = self.weight.detach().float()
            return ops.pack_conv(torch.cat([w, w, torch.zeros_like(w)], dim=1), self.bias, dtype, self.weight.device)
        return self._cached("dup3_zero_third", build)

    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        _route(mp, routing)
        mp.setattr(Conv2d, "packed_dup3", zero_third)
        bs = BlockShadow(mp, vae, sd).install()
        _forward(vae, kind, _input(kind, lidar, side, batch).cuda())
    bounds = BLOCK_BOUND[_routing_key(MUT_LEG)]
    bad = [(b["block"], f"{b['worst_image']:.1e}") for b in bs.results if not b["worst_image"] < bounds[_family(b["block"])]]
    print(f"[mutation dup3] {len(bad)} of {len(bs.results)} blocks fail: {bad[:8]}")
    assert len(bad) >= 10, "the block shadow passed decoder weights [W ; W ; 0]"
    assert all(b["worst_image"] < bounds[_family(b["block"])] for b in _leg(MUT_LEG)["blocks"])   # and passes without the fault


def test_launch_shadow_fails_on_zero_weight_group_stride():
    """The mid attention's S = q k^T launch with w_group_stride = 0 (every image reading image 0's keys): a wrong number, in
    bounds; the launch shadow must fail it."""
    from mobi_amd import ops
    kind, lidar, side, batch, dtype, routing = LEGS[MUT_LEG]
    _set(dtype)
    vae = _model(lidar)
    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        _route(mp, routing)
        with pytest.MonkeyPatch.context() as mp2:
            with LaunchShadow(mp2, label="mutation stride0", cpu_check=False) as sh:
                shadowed = ops.igemm

                def stride0(*a, **k):
                    if k.get("weight_per_image") and k.get("out_mode") == ops.OUT_ROWS_F32:
                        k["w_group_stride"] = 0
                    return shadowed(*a, **k)
                mp2.setattr(ops, "igemm", stride0)
                _forward(vae, kind, _input(kind, lidar, side, batch).cuda())
    print("[mutation stride0] " + "\n".join(sh.failures[:6]))
    assert any("w_group_stride 0 disagrees" in f for f in sh.failures)
    assert any("per_image" in f and "rel-L2" in f for f in sh.failures), sh.failures
    assert not _leg(MUT_LEG)["failures"]                                       # and passes without the fault
