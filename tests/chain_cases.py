"""Row-chain launches for the kernel-level parity tests (TEST INFRASTRUCTURE): the case list shared by the GPU tests
(tests/test_gpu_chain_programs.py: the kernel against tests/chain_ref.py) and the CPU tests (tests/test_chain_ref_cpu.py: an
fp32-accumulating emulation of the same launches against the same reference, clean and with planted defects).

A case builds its operands from seeded noise (distinct weights per product, distinct rows per image), its destinations as
containers pre-filled with a fixed bit pattern, and its programs through the builder class it is given: the recording
subclass of ops.ChainProgram on the device, chain_ref.ProgramDescription without one.  `judge` runs a launch callable and
applies every check of the issue: rel-L2 and worst 128 x 64 tile per stored tensor against the fp64 interpreter, finite,
inputs bit-unchanged, nothing outside the destination rows touched, a second run bit-equal.
"""
import types

import torch

from oracle import weights as W
from tests import chain_ref
from tests.launch_shadow import TILE_FACTOR, compare
from tests.test_gpu_ops import TOL

C = 320
FILL = 0x5A5A                      # the 16-bit pattern every destination container holds before a launch (finite in both types)
LN_EPS = 1e-5


class Weight:
    """What ops.ChainWeight holds (image, bias, svec)."""

    def __init__(self, image, bias, svec=None):
        self.image, self.bias, self.svec = image, bias, svec


class Builder:
    """Operands of one case: seeded, rounded to the storage type, on `device`; containers filled with FILL."""

    def __init__(self, name, dtype, device, program):
        self.name, self.dtype, self.device, self.Program = name, dtype, device, program
        self.containers, self.masters = [], {}

    def rows(self, tag, shape, scale=1.0, offset=0.0):
        x = W.synth_input(f"{self.name}.{tag}", shape) * scale + offset
        # distinct rows per image and per row: a slow ramp on top of the noise
        x = x + 0.05 * torch.arange(shape[0]).view(-1, 1, 1) + 0.1 * torch.linspace(-1, 1, shape[1]).view(1, -1, 1)
        return x.to(self.dtype).to(self.device)

    def f32(self, tag, shape, scale=1.0, offset=0.0):
        return (W.synth_input(f"{self.name}.{tag}", shape) * scale + offset).contiguous().to(self.device)

    def weight(self, tag, ln=False, scale=1.0, bias=True):
        from mobi_amd import ops
        w = torch.from_numpy(W.synth_param(f"{self.name}.{tag}.weight", (C, C)))
        b = torch.from_numpy(W.synth_param(f"{self.name}.{tag}.bias", (C,))) if bias else None
        lnp = None
        if ln:
            lnp = (torch.from_numpy(W.synth_param(f"{self.name}.{tag}.ln.weight", (C,))),
                   torch.from_numpy(W.synth_param(f"{self.name}.{tag}.ln.bias", (C,))))
        self.masters[tag] = (w, b, lnp, scale)
        cw = ops.pack_chain_weight(w, b, self.dtype, self.device, ln=lnp, scale=scale)       # (host arithmetic + one query call)
        return Weight(cw.image, cw.bias, cw.svec) if self.device == "cpu" else cw

    def container(self, *shape):
        t = torch.full(shape, FILL, dtype=torch.int16).view(self.dtype).to(self.device)
        self.containers.append(t)
        return t

    def tables(self, n, heads):
        """The two-key adapter's fp32 tables (the scales of test_chain_adapter)."""
        return dict(a=self.f32("ad.a", (n, heads, C), 0.05), c=self.f32("ad.c", (n, heads)), u=self.f32("ad.u", (n, heads, C)),
                    b=self.f32("ad.b", (n, C)), eps=LN_EPS)


def _case(b, programs, images, rows, tables=None):
    return types.SimpleNamespace(name=b.name, dtype=b.dtype, device=b.device, programs=programs, images=images, rows=rows,
                                 tables=tables, containers=b.containers, descs=[p.desc for p in programs], masters=b.masters)


# ---- the production programs, built with the calls of BasicTransformerBlock._forward_chained / SpatialTransformer.forward ------
def post_attn1(b, n, t):
    a, x_in = b.rows("a", (n, t, C)), b.rows("x", (n, t, C))
    ref_vec = b.f32("ref_vec", (n, C), 0.3)
    cw = {k: b.weight(k, bias=False) for k in ("to_out", "k_cam", "v_cam")}
    cw["q_cam"], cw["q_lid"] = b.weight("q_cam", ln=True, scale=0.23, bias=False), b.weight("q_lid", ln=True, scale=0.23, bias=False)
    x = b.container(n, t, C)
    q_cam, q_lid, kv_l = b.container(n // 2, t, C), b.container(n // 2, t, C), b.container(n // 2, t, 2 * C)
    c = C

    def head(prog):
        return prog.load(a, "s").load(x_in, "r").product(cw["to_out"], resid=True, to_s=True, bias=ref_vec,
                                                         bias_img_stride=c).adapter(dst=x)
    p_cam = head(b.Program()).rowstats(LN_EPS).product(cw["q_cam"], fold=True, dst=q_cam, dst_img_div=2)
    p_lid = head(b.Program()).rowstats(LN_EPS).product(cw["q_lid"], fold=True, dst=q_lid, dst_img_div=2)
    p_lid.product(cw["k_cam"], dst=kv_l[..., :c], dst_img_div=2).product(cw["v_cam"], dst=kv_l[..., c:], dst_img_div=2)
    return _case(b, [p_cam, p_lid], n, t, b.tables(n, 8))


def post_cam(b, n, t):
    """`n` images in the launch: the camera half x[::2] of a 2 n batch, updated in place."""
    x = b.rows("x", (2 * n, t, C))
    b.containers.append(x)
    ac = b.rows("ac", (n, t, C))
    cw = {k: b.weight(k) for k in ("fold_cam",)}
    cw.update({k: b.weight(k, bias=False) for k in ("k_lid", "v_lid")})
    kv_c = b.container(n, t, 2 * C)
    c = C
    xc = x[::2]
    p = b.Program().load(ac, "s").load(xc, "r").product(cw["fold_cam"], resid=True, to_s=True, dst=xc)
    p.product(cw["k_lid"], dst=kv_c[..., :c]).product(cw["v_lid"], dst=kv_c[..., c:])
    return _case(b, [p], n, t)


def pre_attn1(b, n, t):
    x = b.rows("x", (n, t, C), 1.5)
    scale, shift = b.f32("scale", (n, C), 0.2, 1.0), b.f32("shift", (n, C), 0.2)
    cw = {"proj_in": b.weight("proj_in"), "q": b.weight("q", ln=True, scale=0.23, bias=False), "k": b.weight("k", ln=True, bias=False),
          "v": b.weight("v", ln=True, bias=False)}
    tt, qkv = b.container(n, t, C), b.container(n, t, 3 * C)
    c = C
    prog = b.Program().load(x.view(n, t, c), "s").affine(scale, shift).product(cw["proj_in"], to_s=True, dst=tt)
    prog.rowstats(LN_EPS).product(cw["q"], fold=True, dst=qkv[..., :c]).product(cw["k"], fold=True, dst=qkv[..., c:2 * c])
    prog.product(cw["v"], fold=True, dst=qkv[..., 2 * c:])
    return _case(b, [prog], n, t)


# ---- every accepted product form, programs of 1 .. 4 products -------------------------------------------------------------------
def form_store(b, n, t):
    """STORE as the first and only product."""
    p = b.Program().load(b.rows("x", (n, t, C)), "s").product(b.weight("w0"), dst=b.container(n, t, C))
    return _case(b, [p], n, t)


def form_fold(b, n, t):
    """FOLD | STORE as the first and only product (behind ROWSTATS: not the straight-line head)."""
    p = b.Program().load(b.rows("x", (n, t, C), 2.0, 0.7), "s").rowstats(LN_EPS)
    p.product(b.weight("w0", ln=True, scale=0.25), fold=True, dst=b.container(n, t, C))
    return _case(b, [p], n, t)


def form_resid_to_s(b, n, t):
    """RESID | TO_S (no store) as the only product, then STORE_S of the new row state."""
    p = b.Program().load(b.rows("x", (n, t, C)), "s").load(b.rows("r", (n, t, C)), "r")
    p.product(b.weight("w0"), resid=True, to_s=True).store(b.container(n, t, C))
    return _case(b, [p], n, t)


def form_resid_to_s_store(b, n, t):
    """RESID | TO_S | STORE first, STORE later (2 products)."""
    p = b.Program().load(b.rows("x", (n, t, C)), "s").load(b.rows("r", (n, t, C)), "r")
    p.product(b.weight("w0"), resid=True, to_s=True, dst=b.container(n, t, C)).product(b.weight("w1"), dst=b.container(n, t, C))
    return _case(b, [p], n, t)


def form_resid_store(b, n, t):
    """RESID | STORE first (the residual loaded before the state; the state stays the loaded rows), TO_S | STORE and
    FOLD | STORE later (3 products)."""
    p = b.Program().load(b.rows("r", (n, t, C)), "r").load(b.rows("x", (n, t, C)), "s")
    p.product(b.weight("w0"), resid=True, dst=b.container(n, t, C)).product(b.weight("w1"), to_s=True, dst=b.container(n, t, C))
    p.rowstats(LN_EPS).product(b.weight("w2", ln=True), fold=True, dst=b.container(n, t, C))
    return _case(b, [p], n, t)


def form_to_s_store(b, n, t):
    """TO_S | STORE first and later, FOLD | STORE and STORE later (4 products)."""
    p = b.Program().load(b.rows("x", (n, t, C)), "s").product(b.weight("w0"), to_s=True, dst=b.container(n, t, C))
    p.product(b.weight("w1"), to_s=True, dst=b.container(n, t, C)).rowstats(LN_EPS)
    p.product(b.weight("w2", ln=True), fold=True, dst=b.container(n, t, C)).product(b.weight("w3"), dst=b.container(n, t, C))
    return _case(b, [p], n, t)


def two_programs_1_and_4(b, n, t):
    """Even images: one product; odd images: four (the first takes the residual); every store into half-batch tensors."""
    x, r = b.rows("x", (n, t, C)), b.rows("r", (n, t, C))
    o0, o1 = b.container(n // 2, t, C), b.container(n // 2, t, 4 * C)
    p0 = b.Program().load(x, "s").product(b.weight("w0"), dst=o0, dst_img_div=2)
    p1 = b.Program().load(x, "s").load(r, "r").product(b.weight("w1"), resid=True, to_s=True, dst=o1[..., :C], dst_img_div=2)
    for k in (1, 2, 3):
        p1.product(b.weight(f"w{k + 1}"), dst=o1[..., k * C:(k + 1) * C], dst_img_div=2)
    return _case(b, [p0, p1], n, t)


def mid_load(b, n, t):
    """A second LOAD_S between two products."""
    p = b.Program().load(b.rows("x", (n, t, C)), "s").product(b.weight("w0"), dst=b.container(n, t, C))
    p.load(b.rows("y", (n, t, C)), "s").product(b.weight("w1"), dst=b.container(n, t, C))
    return _case(b, [p], n, t)


def mid_load_after_resid(b, n, t):
    """RESID | TO_S first (residual rows in flight while the ring runs), a second LOAD_S, two more products."""
    p = b.Program().load(b.rows("x", (n, t, C)), "s").load(b.rows("r", (n, t, C)), "r").product(b.weight("w0"), resid=True, to_s=True)
    p.store(b.container(n, t, C)).load(b.rows("y", (n, t, C)), "s").product(b.weight("w1"), to_s=True, dst=b.container(n, t, C))
    p.product(b.weight("w2"), dst=b.container(n, t, C))
    return _case(b, [p], n, t)


def strided_loads(b, n, t):
    """LOAD_S and LOAD_R from row-strided views: the column halves of one [n, t, 640] tensor."""
    big = b.rows("xr", (n, t, 2 * C))
    p = b.Program().load(big[..., :C], "s").load(big[..., C:], "r").product(b.weight("w0"), resid=True, dst=b.container(n, t, C))
    return _case(b, [p], n, t)


def load_img_div(b, n, t):
    """LOAD_S with img_div = 2 (images 2 i and 2 i + 1 read the same rows), a full-batch residual."""
    p = b.Program().load(b.rows("x", (n // 2, t, C)), "s", img_div=2).load(b.rows("r", (n, t, C)), "r")
    p.product(b.weight("w0"), resid=True, dst=b.container(n, t, C))
    return _case(b, [p], n, t)


def bias_img_div(b, n, t):
    """A per-pair bias: [n / 2, 320] with bias_img_stride = 320 and bias_img_div = 2."""
    bias = b.f32("bias", (n // 2, C), 0.5)
    p = b.Program().load(b.rows("x", (n, t, C)), "s")
    p.product(b.weight("w0"), dst=b.container(n, t, C), bias=bias, bias_img_stride=C, bias_img_div=2)
    return _case(b, [p], n, t)


def adapter_heads(heads):
    def build(b, n, t):
        p = b.Program().load(b.rows("x", (n, t, C), 2.0), "s").adapter(dst=b.container(n, t, C))
        return _case(b, [p], n, t, b.tables(n, heads))
    build.__name__ = f"adapter_h{heads}"
    return build


SMALL, TWO_TILES, MANY_BLOCKS = (2, 128), (4, 256), (4, 8320)          # 1 tile per image; 2 tiles and img / 2; 260 workgroups
CASES = {}
for fn, shapes in ((post_attn1, (SMALL, TWO_TILES, MANY_BLOCKS)), (post_cam, (SMALL, TWO_TILES)), (pre_attn1, (SMALL, TWO_TILES)),
                   (form_store, (SMALL,)), (form_fold, (SMALL,)), (form_resid_to_s, (SMALL, TWO_TILES)),
                   (form_resid_to_s_store, (SMALL,)), (form_resid_store, (SMALL, TWO_TILES)), (form_to_s_store, (SMALL, TWO_TILES)),
                   (two_programs_1_and_4, (SMALL, TWO_TILES)), (mid_load, (SMALL,)), (mid_load_after_resid, (SMALL, TWO_TILES)),
                   (strided_loads, (SMALL, TWO_TILES)), (load_img_div, (TWO_TILES,)), (bias_img_div, (TWO_TILES,)),
                   (adapter_heads(1), (SMALL,)), (adapter_heads(2), (SMALL,)), (adapter_heads(5), (TWO_TILES,)),
                   (adapter_heads(8), (SMALL, TWO_TILES))):
    for n_, t_ in shapes:
        CASES[f"{fn.__name__}-{n_}x{t_}"] = (fn, n_, t_)


def build_case(key, dtype, device, program):
    fn, n, t = CASES[key]
    return fn(Builder(f"chainprog.{fn.__name__}.{n}.{t}", dtype, device, program), n, t)


def bound_of(rec, dtype):
    """The bound tests/test_gpu_chain.py asserts for the form: TOL for products and the adapter, 1.5 TOL for a folded product."""
    return TOL[dtype] * (1.5 if rec["code"] == "product" and rec["flags"] & 1 else 1.0)


def result_name(rec):
    return f"prog{rec['prog']} op{rec['index']} {rec['code']}" + (f" {chain_ref.flag_name(rec['flags'])}" if rec["code"] == "product" else "")


def judge(case, launch, bound_scale=1.0, rerun=True, report=None):
    """Run `launch()` (which writes the case's destinations) and check it against the fp64 interpreter on the operands it read
    -> list of failure strings.  report(name, rel, tile, bound) is called per stored tensor before anything is judged."""
    dev = case.containers[0].device
    snaps, memo = chain_ref.snapshot(case.descs)
    before = [c.clone() for c in case.containers]
    launch()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    bad = []
    results = chain_ref.run_launch(snaps, case.images, case.rows, case.dtype, case.tables, dev=dev)
    if not results:
        bad.append("the launch stores nothing")
    for rec in results:
        got = chain_ref.as_images(chain_ref.stored_rows(rec), case.rows)
        res = compare(got, chain_ref.as_images(rec["ref"], case.rows))
        bound = bound_of(rec, case.dtype) * bound_scale
        if report is not None:
            report(result_name(rec), res["rel"], res["tile"], bound)
        if not (res["finite"] and res["rel"] < bound and res["tile"] < TILE_FACTOR * bound):
            bad.append(f"{result_name(rec)}: rel-L2 {res['rel']:.3e}, worst tile {res['tile']:.3e} at {res['where']}, finite "
                       f"{res['finite']} (bound {bound:.2e}, tile bound {TILE_FACTOR * bound:.2e})")
    bad += [f"input changed: {m}" for m in chain_ref.changed_inputs(case.descs, snaps)]
    bad += chain_ref.touched_outside(results, memo)
    if rerun:
        first = [c.clone() for c in case.containers]
        for c, b0 in zip(case.containers, before):
            c.copy_(b0)
        launch()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        if not all(torch.equal(chain_ref.bits(c), chain_ref.bits(f)) for c, f in zip(case.containers, first)):
            bad.append("a second run of the same launch is not bit-equal to the first")
    return bad


# ---- fp32-accumulating emulation of a launch (the CPU tests' stand-in for the kernel; defects planted one at a time) ------------
DEFECTS = ("swap_weights", "drop_residual", "ignore_dst_img_div", "skip_wave", "drop_cs_svec", "bias_stride_0")


def emulate(case, defect=None):
    """What a correct kernel computes, in fp32 torch with the contract's rounding points: fp32 sums, the state rounded to T
    after AFFINE_S / TO_S / ADAPTER, stores rounded once -- written into the case's destinations image by image.  `defect`:
      swap_weights        products 0 and 1 of a program read each other's weights
      drop_residual       RESID adds nothing
      ignore_dst_img_div  a store goes to image img, not img / div (what falls outside the tensor is lost)
      skip_wave           rows 160 .. 191 (wave 1 of tile 1) of the last image are not written by one store
      drop_cs_svec        FOLD applies rs only
      bias_stride_0       every image reads the first bias vector"""
    dt = case.dtype
    rt = lambda v: v.to(dt).float()
    for k, desc in enumerate(case.descs):
        imgs = range(case.images) if len(case.descs) == 1 else range(k, case.images, 2)
        weights = [chain_ref.decode_chain_weight(kw["image"], dt).float() for code, kw in desc if code == "product"]
        if defect == "swap_weights" and len(weights) > 1:
            weights[0], weights[1] = weights[1], weights[0]
        n_store = sum(1 for code, kw in desc if kw.get("dst") is not None)
        for img in imgs:
            s = r = torch.zeros((case.rows, C))
            rs, cs = torch.ones((case.rows, 1)), torch.zeros((case.rows, 1))
            pk = stores = 0

            def store(kw, v):
                nonlocal stores
                stores += 1
                dst = kw["dst"]
                div = max(kw["dst_img_div"], 1)
                di = img if defect == "ignore_dst_img_div" else img // div
                if di >= dst.shape[0]:
                    return
                v = v.to(dt)
                if defect == "skip_wave" and img == imgs[-1] and stores == n_store and case.rows >= 192:
                    keep = torch.ones(case.rows, dtype=torch.bool)
                    keep[160:192] = False
                    dst[di, keep, :C] = v[keep]
                else:
                    dst[di, :, :C] = v

            for code, kw in desc:
                if code in ("load_s", "load_r"):
                    v = kw["t"][img // max(kw["img_div"], 1), :, :C].float()
                    s, r = (v, r) if code == "load_s" else (s, v)
                elif code == "affine":
                    s = rt(s * kw["scale"][img] + kw["shift"][img])
                elif code == "rowstats":
                    mean = s.mean(-1, keepdim=True)
                    rs = ((s - mean).square().mean(-1, keepdim=True) + kw["eps"]).rsqrt()
                    cs = -rs * mean
                elif code == "product":
                    v = s @ weights[pk].T
                    pk += 1
                    if kw["fold"]:
                        v = rs * v + (0.0 if defect == "drop_cs_svec" else cs * kw["svec"])
                    stride = 0 if defect == "bias_stride_0" else kw["bias_img_stride"]
                    off = (img // max(kw["bias_img_div"], 1)) * stride
                    v = v + kw["bias"].reshape(-1)[off:off + C]
                    if kw["resid"]:
                        v = v if defect == "drop_residual" else v + r
                    if kw["to_s"]:
                        s = rt(v)
                    if kw["dst"] is not None:
                        store(kw, v)
                elif code == "adapter":
                    tb = case.tables
                    mean = s.mean(-1, keepdim=True)
                    rstd = ((s - mean).square().mean(-1, keepdim=True) + tb["eps"]).rsqrt()
                    z = rstd * (s @ tb["a"][img].T - mean * tb["a"][img].sum(-1)) + tb["c"][img]
                    s = rt(s + tb["b"][img] + torch.sigmoid(z) @ tb["u"][img])
                    store(kw, s)
                elif code == "store":
                    store(kw, s)
