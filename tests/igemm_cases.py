"""The launches of tests/test_gpu_igemm_rows.py: (id, body key, MOBI_IGEMM_* knobs, Case).  Shared with
tests/test_igemm_ref_cpu.py, which checks on the CPU that every case lands on its body (igemm_ref.plan against
mobi_igemm_kernel_variant -- a query, no launch), that its data is sensitive (igemm_ref.input_conditions) and that the
list covers what it promises (`missing`).

A body is forced with the A/B environment of csrc/tuning.hip:
  staged128   SM=0 WM=2 WIDE=0            igemm_kernel<.., WM 2>
  staged256   WM=4 WIDE=0 PP=0            igemm_kernel<.., WM 4> (Body::Staged256; reported as direct_lds where C % 64 == 0:
                                          mobi_engine.h says why)
  pingpong    WM=4 WIDE=0                 igemm_pp_kernel (eligible shapes only)
  ring256s    WM=4 WIDE=2 RING_DIRECT=0       igemm_ring_kernel<.., 8, 8>, LDS-staged epilogue
  ring256r    WM=4 WIDE=2 RING_DIRECT=1       the same, register epilogue where it applies
  ring128w    WIDE=1                      igemm_ring_kernel<.., 8, 4>
  ring128s    WM=2 WIDE=0 SM64=0 SM_DIRECT=0    igemm_ring_kernel<.., 4, 4>, staged epilogue
  ring128r    WM=2 WIDE=0 SM64=0 SM_DIRECT=1    the same, register epilogue / register slab stores where they apply
  ring64      WM=2 WIDE=0 SM64=1          igemm_ring64_kernel, overlapped step; ring64seq: SM64_OVL=0
  small       SMALL=32                    csrc/igemm_small.hip
P is the body's pixel tile (128 / 256), Q its channel tile for n_packed % 160 != 0 (128 / 256), Q5 for % 160 == 0 (160 / 320)."""
import itertools

from tests import igemm_ref as R
from tests.igemm_ref import Case

BODIES = {
    "staged128": (dict(SM=0, WM=2, WIDE=0, SMALL=0), 128, 128, 160),
    "staged256": (dict(WM=4, WIDE=0, PP=0, SMALL=0), 256, 128, 160),
    "pingpong": (dict(WM=4, WIDE=0, SMALL=0), 256, 128, 160),
    "ring256s": (dict(WM=4, WIDE=2, RING_DIRECT=0, SMALL=0), 256, 256, 320),
    "ring256r": (dict(WM=4, WIDE=2, RING_DIRECT=1, SMALL=0), 256, 256, 320),
    "ring128w": (dict(WIDE=1, SMALL=0), 128, 256, 320),
    "ring128s": (dict(WM=2, WIDE=0, SM64=0, SM_DIRECT=0, SMALL=0), 128, 128, 160),
    "ring128r": (dict(WM=2, WIDE=0, SM64=0, SM_DIRECT=1, SMALL=0), 128, 128, 160),
    "ring64": (dict(WM=2, WIDE=0, SM64=1, SMALL=0), 128, 128, 160),
    "ring64seq": (dict(WM=2, WIDE=0, SM64=1, SM64_OVL=0, SMALL=0), 128, 128, 160),
    "small": (dict(SMALL=32), 32, 32, 32),
}
EXPECTED_BODY = {"staged128": (R.STAGED_128,), "staged256": (R.STAGED_256, R.DIRECT_LDS), "pingpong": (R.PINGPONG,),
                 "ring256s": (R.RING_256,), "ring256r": (R.RING_256,), "ring128w": (R.RING_128W,), "ring128s": (R.RING_128,),
                 "ring128r": (R.RING_128,), "ring64": (R.RING_128,), "ring64seq": (R.RING_128,), "small": (R.SMALL,)}
GENERAL = ("staged128", "staged256", "ring256s", "ring128s", "ring64")      # bodies that take every row-major form
LDS_DMA = ("pingpong", "ring256s", "ring256r", "ring128w", "ring128s", "ring128r", "ring64", "ring64seq")
STAGED = ("staged128", "staged256")

C3 = dict(kh=3, kw=3, pad_h=1, pad_w=1)


def _general(key, P, Q, Q5):
    """The forms every general body takes; k: 64-deep bodies (ring64) need channel runs of 64."""
    deep = key.startswith("ring64")
    c32, c96, c160 = (64, 128, 192) if deep else (32, 96, 160)
    two_a, two_b = ((64, 64), (128, 64)) if deep else ((32, 32), (96, 32))
    full = P // 16
    out = [
        # ---- pixel rows: 1, P - 1, P, P + 1, tiles that straddle images -----------------------------------------------
        ("m1.3x3.nobias", Case(1, 1, 1, c32, 8, bias=False, **C3)),
        ("mPm1.1x5.rowvec", Case(1, 1, P - 1, c32, Q - 8, kh=1, kw=5, pad_w=2, bias=False, rowvec=True)),
        ("mP.4x4.3x3.res", Case(full, 4, 4, 64, Q, residual="dense", **C3)),
        ("mP.4x4.3x3.res.nt5", Case(full, 4, 4, 64, Q5, residual="dense", w_tiled=True, **C3)),
        ("mPp1.1x1.scale.inplace", Case(1, 1, P + 1, c160, Q, scale=0.5, residual="inplace")),
        ("straddle.1x1.all", Case(3, 1, 43, c96, Q + 8, rowvec=True, residual="strided", src_strided=True, out_strided=True,
                                  rowvec_strided=True)),
        ("straddle.nt5", Case(3, 1, 43, c96, Q5 + 160, rowvec=True, residual="dense", w_tiled=True)),
        # ---- gather ----------------------------------------------------------------------------------------------------
        ("s2.pad1", Case(2, 9, 9, 64, Q5, stride=2, **C3)),
        ("s2.asym.two", Case(2, 8, 8, two_a[0], Q + 8, c1=two_a[1], kh=3, kw=3, stride=2, hout=4, wout=4)),
        ("up.two", Case(2, 5, 3, two_b[0], 136, c1=two_b[1], upsample=True, residual="dense", **C3)),
        ("img1x1.3x3", Case(4, 1, 1, c32, 24, **C3)),
        ("img2x2.3x3", Case(3, 2, 2, c32, 136, rowvec=True, **C3)),
        ("h1.3x3", Case(2, 1, 9, c32, 40, **C3)),
        ("w1.3x3", Case(2, 9, 1, c32, 40, src_strided=True, **C3)),
        ("tap.straddle.3x3", Case(2, 6, 6, c96, Q, residual="dense", **C3)),
        # ---- epilogue ---------------------------------------------------------------------------------------------------
        ("rowvec.nobias.hw64", Case(2, 8, 8, 64, Q, bias=False, rowvec=True)),
        ("rowvec.bias.res", Case(2, 8, 8, 64, Q5, rowvec=True, residual="dense")),
        ("geglu.full", Case(full, 4, 4, 64, Q // 2, epilogue="geglu")),
        ("geglu.full.nt5", Case(full, 4, 4, 64, Q5 // 2, epilogue="geglu")),
        ("geglu.ragged", Case(3, 1, 43, c96, Q // 2 + 8, epilogue="geglu", out_strided=True)),
        ("f32.ragged", Case(3, 1, 43, 64, Q + 8, out_mode="f32", rowvec=True, residual="dense")),
        ("f32.full.nt5", Case(full, 4, 4, 64, Q5, out_mode="f32", **C3)),
        ("tr.hw8.cout3", Case(2, 4, 4, c32, 3, out_mode="tr", **C3)),
        ("tr.hw43.coutQp1", Case(3, 1, 43, c96, Q + 1, out_mode="tr", out_strided=True)),
        ("tr.full.nt5", Case(full, 4, 4, 64, Q5, out_mode="tr")),
        ("tr.full", Case(full, 4, 4, 64, Q, out_mode="tr", out_strided=True)),
        # ---- weights ----------------------------------------------------------------------------------------------------
        ("groups2.full", Case(2 * full, 4, 4, 64, Q, groups=2, residual="dense")),
        ("groups2.ragged.gap", Case(4, 1, 43, c96, Q + 8, groups=2, w_gap=64, rowvec=True)),
        ("groupsN.dense", Case(3, 1, 43, 64, 136, groups=3, bias=False)),
        ("groupsN.gap.tr", Case(3, 1, 43, 64, 136, groups=3, w_gap=72, bias=False, out_mode="tr")),
        # ---- split-K ----------------------------------------------------------------------------------------------------
        ("split2.uneven.full", Case(full, 4, 4, 64, Q, split_k=2, residual="dense", rowvec=True, **C3)),                 # 9 tiles: 5 + 4
        ("split4.fewer.ragged", Case(3, 1, 43, 64, Q + 8, split_k=4, residual="strided", **C3)),                          # 9 tiles: 3 slabs
        ("split4.uneven.ragged.f32", Case(1, 1, P + 1, 128, Q + 8, kh=1, kw=5, pad_w=2, split_k=4, out_mode="f32")),     # 10: 3, 3, 3, 1
        ("split2.uneven.ragged", Case(3, 1, 43, 64, Q + 8, split_k=2, rowvec=True, **C3)),
        ("split4.fewer.full", Case(full, 4, 4, 64, Q, split_k=4, residual="dense", **C3)),
        ("split4.uneven.full.nt5", Case(full, 4, 4, 128, Q5, kh=1, kw=5, pad_w=2, split_k=4, rowvec=True)),
        ("split8.reduce.full.nt5", Case(full, 4, 4, 512, Q5, split_k=8, residual="dense")),
        ("split8.reduce.ragged", Case(3, 1, 43, 512, 136, split_k=8, rowvec=True)),
    ]
    return out


def _ln(P, Q, Q5):
    full = P // 16
    return [("ln.full", Case(full, 4, 4, 128, Q, ln=True)),
            ("ln.full.nt5", Case(full, 4, 4, 128, Q5, ln=True)),
            ("ln.ragged", Case(3, 1, 43, 192, Q + 8, ln=True, out_strided=True)),
            ("ln.ragged.nt5", Case(1, 1, P + 1, 64, Q5 + 160, ln=True)),
            ("ln.geglu.full.nt5", Case(full, 4, 4, 128, Q5 // 2, ln=True, epilogue="geglu")),
            ("ln.geglu.ragged", Case(3, 1, 43, 128, Q // 2 + 8, ln=True, epilogue="geglu")),
            ("ln.f32.ragged", Case(3, 1, 43, 128, Q + 8, ln=True, out_mode="f32"))]


def _leaky(P, Q, Q5):
    full = P // 16
    lo = 256 if P == 256 else 0                   # the 256 x 256 (320) tiles take leaky launches of >= 256 channels only
    return [("leaky.full", Case(full, 4, 4, 64, max(Q, lo), epilogue="leaky", **C3)),
            ("leaky.full.nt5.res.rowvec", Case(full, 4, 4, 64, 320, epilogue="leaky", residual="dense", rowvec=True, **C3)),
            ("leaky.ragged.res", Case(3, 1, 43, 96, max(Q, lo) + 8, epilogue="leaky", residual="strided")),
            ("leaky.ragged.nt5.f32", Case(1, 1, P + 1, 64, 480, epilogue="leaky", rowvec=True, out_mode="f32"))]


def _register(P, Q, Q5, hw_rowvec):
    """Full tiles only: what the register epilogues take (bias | rowvec without bias, residual, GEGLU), 3+ k-steps."""
    n = P // 64
    return [("reg.bias.res", Case(n, 8, 8, 64, Q, residual="dense", **C3)),
            ("reg.bias.res.nt5", Case(n, 8, 8, 64, Q5, residual="strided", out_strided=True, **C3)),
            ("reg.rowvec", Case(max(1, P // hw_rowvec), hw_rowvec // 8, 8, 192, Q, bias=False, rowvec=True, rowvec_strided=True)),
            ("reg.rowvec.nt5.res", Case(max(1, P // hw_rowvec), hw_rowvec // 8, 8, 192, Q5, bias=False, rowvec=True,
                                        residual="dense")),
            ("reg.nobias.two", Case(n, 8, 8, 64, Q, c1=64, bias=False, **C3)),
            ("reg.geglu", Case(n, 8, 8, 192, Q // 2, epilogue="geglu")),
            ("reg.geglu.nt5", Case(n, 8, 8, 192, Q5 // 2, epilogue="geglu")),
            ("reg.inplace", Case(n, 8, 8, 256, Q5, residual="inplace"))]


def build():
    cases = []
    add = lambda key, name, case: cases.append((f"{key}.{name}", key, BODIES[key][0], case))
    for key in GENERAL:
        _, P, Q, Q5 = BODIES[key]
        for name, case in _general(key, P, Q, Q5):
            add(key, name, case)
    for key in ("staged128", "ring128s", "ring64", "ring256s"):      # 256 + 64 channels: the source changes inside every tap
        add(key, "two.256.64", Case(3, 1, 43, 256, 136, c1=64, kh=1, kw=3, pad_w=1, residual="dense"))
    add("ring128s", "three.column.tiles", Case(1, 1, 129, 32, 2 * 128 + 8, rowvec=True))
    add("staged128", "three.column.tiles", Case(1, 1, 129, 32, 2 * 128 + 8, rowvec=True))
    for key in ("staged128", "staged256"):                            # 64 + 64: the register-staged bodies' own case
        add(key, "two.64.64", Case(2, 6, 6, 64, 136, c1=64, **C3))
    # the ring's prologue (four k-slots, requests three steps ahead): 1, 2, 3 and depth + 1 = 4 k-steps, and 5 (the ring wraps)
    for key, chans in (("ring128s", (32, 64, 96, 128, 160)), ("ring256s", (32, 64, 96, 128, 160)),
                       ("ring128w", (32, 64, 96, 128, 160)), ("ring64", (64, 128, 192, 256, 320)),
                       ("ring64seq", (64, 128, 192, 256, 320))):
        for c in chans:
            add(key, f"steps.c{c}", Case(3, 1, 43, c, 136, residual="dense"))
    for key in ("ring256s", "ring128s", "ring64", "ring64seq"):
        _, P, Q, Q5 = BODIES[key]
        for name, case in _ln(P, Q, Q5):
            add(key, name, case)
    for key in ("ring256s", "ring128s"):
        _, P, Q, Q5 = BODIES[key]
        for name, case in _leaky(P, Q, Q5):
            add(key, name, case)
    for key, hw_rowvec in (("pingpong", 64), ("ring256r", 128), ("ring128r", 64), ("ring128w", 64), ("ring64", 64),
                           ("ring64seq", 64)):
        _, P, Q, Q5 = BODIES[key]
        for name, case in _register(P, Q, Q5, hw_rowvec):
            if key == "ring256r" and case.c1:
                case = Case(**{**case.__dict__, "c0": 128, "c1": 64})
            add(key, name, case)
    # the remaining forms of the bodies above
    add("ring256r", "ln.full.nt5", Case(16, 4, 4, 128, 320, ln=True))
    add("ring256r", "ln.geglu.full", Case(16, 4, 4, 128, 128, ln=True, epilogue="geglu"))
    add("ring128r", "ln.full", Case(8, 4, 4, 128, 128, ln=True))
    add("ring128r", "ln.full.nt5", Case(8, 4, 4, 128, 160, ln=True))
    for key in GENERAL + ("ring64seq",):                      # transposed output on 160 (320)-wide tiles, ragged pixel tile
        _, P, Q, Q5 = BODIES[key]
        add(key, "tr.ragged.nt5", Case(3, 1, 43, 64, Q5 + (160 if Q5 == 320 else 0), out_mode="tr"))
    for key in ("ring128w", "ring64seq"):
        _, P, Q, Q5 = BODIES[key]
        add(key, "ragged.all", Case(3, 1, 43, 64, Q + 8, rowvec=True, residual="strided", out_strided=True))
        add(key, "ragged.nt5.f32", Case(1, 1, P + 1, 64, Q5 + 160 if key == "ring128w" else 320, out_mode="f32", **C3))
        add(key, "s2.asym", Case(2, 8, 8, 64, Q, c1=64, kh=3, kw=3, stride=2, hout=4, wout=4))
    add("ring64seq", "tr.hw43", Case(3, 1, 43, 64, 129, out_mode="tr"))
    add("ring64seq", "tr.full.nt5", Case(8, 4, 4, 64, 160, out_mode="tr"))
    # split-K finished inside the launch (modes 1 and 2) and by mobi_igemm_finish: test_split_forms runs every finish of these
    # the ping-pong kernel's slab stores: 256-pixel tiles, >= 3 k-tiles per range
    add("pingpong", "slab.split2", Case(4, 8, 8, 64, 128, split_k=2, residual="dense", **C3))
    add("pingpong", "slab.split2.nt5", Case(4, 8, 8, 64, 160, split_k=2, rowvec=True, **C3))
    add("ring128r", "slab.split2", Case(8, 4, 4, 64, 128, split_k=2, residual="dense", **C3))
    add("ring128r", "slab.split4.nt5", Case(8, 4, 4, 128, 160, split_k=4, kh=1, kw=5, pad_w=2, rowvec=True))
    add("ring128w", "slab.split2", Case(8, 4, 4, 64, 256, split_k=2, residual="dense", **C3))
    add("ring64", "slab.split2.f32", Case(8, 4, 4, 64, 128, split_k=2, out_mode="f32", **C3))
    # the in-launch finish in its same-XCD form (MOBI_IGEMM_FUSED_SPLIT 2, the default) needs a tile count that is a multiple
    # of 8 (in_launch_finish, csrc/igemm_plan.hip: `mode == 1 || tiles % 8 == 0`): 4 x 2 tiles of 128 x 128 / 160 / 256, 2 x 4 of 256 x 128 / 160 on the
    # ping-pong kernel, 4 x 2 of 256 x 256 (M = 1,024: the one shape beyond the suite's usual 600 rows)
    sync8 = Case(8, 8, 8, 64, 256, split_k=2, residual="dense", rowvec=True, **C3)
    add("ring128s", "sync8.split2", sync8)                            # staged slab stores
    add("ring128r", "sync8.split2", sync8)                            # register slab stores
    add("ring64", "sync8.split2", sync8)
    add("ring64seq", "sync8.split2", sync8)
    add("ring128r", "sync8.split4.nt5", Case(8, 8, 8, 128, 320, split_k=4, kh=1, kw=5, pad_w=2, residual="dense"))
    add("ring128s", "sync8.split4.nt5", Case(8, 8, 8, 128, 320, split_k=4, kh=1, kw=5, pad_w=2, residual="dense"))
    add("ring64", "sync8.split4.nt5", Case(8, 8, 8, 128, 320, split_k=4, kh=1, kw=5, pad_w=2, residual="dense"))
    add("ring128w", "sync8.split2", Case(8, 8, 8, 64, 512, split_k=2, residual="dense", **C3))
    add("ring128w", "sync8.split2.nt5", Case(8, 8, 8, 64, 640, split_k=2, rowvec=True, **C3))
    add("pingpong", "sync8.split2", Case(8, 8, 8, 64, 512, split_k=2, residual="dense", **C3))
    add("pingpong", "sync8.split2.nt5", Case(8, 8, 8, 64, 640, split_k=2, rowvec=True, **C3))
    add("ring256s", "sync8.split2", Case(16, 8, 8, 64, 512, split_k=2, residual="dense", **C3))
    # the slab stores the cases above leave out: ragged tiles (LDS-staged stores) on the 128 x 256 (320) ring and on ring64
    add("ring128w", "slab.ragged", Case(3, 1, 43, 64, 264, split_k=2, rowvec=True, **C3))
    add("ring128w", "slab.ragged.nt5", Case(3, 1, 43, 64, 480, split_k=2, residual="strided", **C3))
    for key in ("ring64", "ring64seq"):
        add(key, "slab.ragged", Case(3, 1, 43, 64, 136, split_k=2, rowvec=True, **C3))
        add(key, "slab.ragged.nt5", Case(3, 1, 43, 64, 160, split_k=2, residual="strided", **C3))
    add("ring64seq", "slab.split4.nt5", Case(8, 4, 4, 128, 160, split_k=4, kh=1, kw=5, pad_w=2, rowvec=True))
    # the small kernel: 1 x 1 and 3 x 3 pad 1, C % 320 == 0, n % 32 == 0, row-major T / fp32 output
    for name, case in (("m1", Case(1, 1, 1, 320, 32)), ("m31", Case(1, 1, 31, 320, 64, rowvec=True, residual="strided",
                                                                   src_strided=True, out_strided=True)),
                       ("m33.f32", Case(3, 1, 11, 320, 96, out_mode="f32", residual="dense")),
                       ("m32.two", Case(2, 4, 4, 160, 32, c1=160, scale=0.5)),
                       ("3x3", Case(3, 3, 5, 320, 64, bias=False, rowvec=True, **C3)),
                       ("3x3.inplace", Case(2, 2, 2, 320, 160, residual="inplace", **C3))):
        add("small", name, case)
    return cases


CASES = build()
SPLIT_CASES = [c for c in CASES if c[3].split_k > 1]
WTILED_CASES = [c for c in CASES if c[3].w_tiled]


def _axes(case, p):
    """The axis values of the issue a case exercises on its body."""
    P, Qt = p["pixel_tile"], p["channel_tile"]
    M = (case.n // case.groups) * case.hw
    a = set()
    for name, val in (("m=1", 1), ("m=P-1", P - 1), ("m=P", P), ("m=P+1", P + 1)):
        if M == val:
            a.add(name)
    if case.hw < P and case.n > 1 and P % case.hw:
        a.add("tile straddles images")
    for name, val in (("n=8", 8), ("n=Q-8", Qt - 8), ("n=Q", Qt), ("n=Q+8", Qt + 8), ("n=2Q+8", 2 * Qt + 8)):
        if case.n_packed == val:
            a.add(name)
    if case.out_mode == "tr":
        a.add("tr.hw%8==0" if case.hw % 8 == 0 else "tr.hw%8!=0")
        if case.cout % 8:
            a.add("tr.cout%8!=0")
    if case.c1:
        a.add("two sources")
        a.add(f"{case.c0}+{case.c1}")
    else:
        a.add(f"C={case.c0}")
    if p["kernel"].startswith("ring") and case.split_k <= 1:         # k-steps of the LDS ring: 32 deep, 64 on ring64
        deep = p["kernel"].startswith("ring64")
        steps = -(-case.ktot // (64 if deep else 32))
        a.add(f"{'ring64' if deep else 'ring32'}.k-steps={steps}")
    g = (case.kh, case.kw, case.stride, case.pad_h, case.upsample)
    for name, val in (("1x1", (1, 1, 1, 0, False)), ("3x3", (3, 3, 1, 1, False)), ("3x3.s2", (3, 3, 2, 1, False)),
                      ("3x3.s2.asym", (3, 3, 2, 0, False)), ("3x3.up", (3, 3, 1, 1, True)), ("1x5", (1, 5, 1, 0, False))):
        if g == val:
            a.add(name)
    if case.kh == 3 and (case.hin, case.win) in ((1, 1), (2, 2)):
        a.add("3x3 on a tiny image")
    if case.kh == 3 and case.hin == 1 and case.win > 2:
        a.add("h=1")
    if case.kh == 3 and case.win == 1 and case.hin > 2:
        a.add("w=1")
    flags = (("no bias", not case.bias and not case.rowvec), ("rowvec+bias", case.rowvec and case.bias),
             ("rowvec no bias", case.rowvec and not case.bias), ("strided rowvec", case.rowvec_strided),
             ("residual dense", case.residual == "dense"), ("residual strided", case.residual == "strided"),
             ("in-place residual", case.residual == "inplace"), ("scale", case.scale != 1.0),
             ("leaky", case.epilogue == "leaky"), ("geglu", case.geglu), ("fp32 rows", case.out_mode == "f32"),
             ("LayerNorm fold", case.ln), ("groups 2", case.groups == 2), ("groups = batch", case.groups == case.n > 1),
             ("w_group_stride gap", case.w_gap > 0), ("strided source", case.src_strided), ("strided output", case.out_strided),
             ("split_k", case.split_k > 1))
    a.update(name for name, on in flags if on)
    return a


# every axis value below appears on at least one LDS-DMA body and on at least one register-staged body
AXES_BOTH = ("m=1", "m=P-1", "m=P", "m=P+1", "tile straddles images", "n=8", "n=Q-8", "n=Q", "n=Q+8", "tr.hw%8==0",
             "tr.hw%8!=0", "tr.cout%8!=0", "two sources", "1x1", "3x3", "3x3.s2", "3x3.s2.asym", "3x3.up", "1x5",
             "3x3 on a tiny image", "h=1", "w=1", "no bias", "rowvec+bias", "rowvec no bias", "strided rowvec", "residual dense",
             "residual strided", "in-place residual", "scale", "geglu", "fp32 rows", "groups 2", "groups = batch",
             "w_group_stride gap", "strided source", "strided output", "split_k",
             "C=32", "C=64", "C=96", "C=160", "32+32", "96+32", "64+64", "256+64")
# forms only the ring kernels have; three column tiles on one body; the ring's step counts 1, 2, 3, depth + 1 = 4 (and 5)
AXES_LDS_ONLY = ("leaky", "LayerNorm fold", "n=2Q+8") + tuple(f"{r}.k-steps={s}" for r in ("ring32", "ring64") for s in (1, 2, 3, 4, 5))


def split_kind(case):
    """The split-K kinds of the issue: more than four slabs (the reduce launch whatever `sync` says), a slab count below
    split_k, an uneven last range, or even ranges."""
    ranges = R.split_ranges(case, case.split_k)
    if len(ranges) > 4:
        return "more than four slabs"
    if len(ranges) < case.split_k:
        return "fewer slabs than split_k"
    uneven = ranges[-1][1] - ranges[-1][0] != ranges[0][1] - ranges[0][0]
    return f"split_k {case.split_k}, {'uneven last range' if uneven else 'even ranges'}"


SPLIT_KINDS = ("more than four slabs", "fewer slabs than split_k", "split_k 2, uneven last range", "split_k 4, uneven last range")


def in_launch_mode(case, knobs, mode):
    """sync_mode igemm_ref.plan expects of the case launched with `sync` under MOBI_IGEMM_FUSED_SPLIT = mode."""
    import dataclasses
    return R.plan(dataclasses.replace(case, finish="sync"), dict(knobs, FUSED_SPLIT=mode))["sync_mode"]


def expected_instantiations():
    """(kernel, epilogue form) of igemm_ref.plan for everything launch_igemm (csrc/igemm.hip) can select
    -> (its eligibility allows a ragged pixel tile, a ragged channel tile)."""
    want = {}
    for nt, tr, wm in itertools.product((4, 5), (0, 1), (2, 4)):
        want[(f"staged<{nt},{tr},{wm}>", "staged")] = True
    for nt in (4, 5):
        want[(f"pp<{nt},geglu0,slab0>", "register")] = False
        want[(f"pp<{nt},geglu1,slab0>", "register")] = False
        for shape in ("8,8", "4,4"):
            want[(f"ring<{nt},0,{shape},lnf0,leaky0>", "staged")] = True
            want[(f"ring<{nt},0,{shape},lnf0,leaky0>", "register")] = False
            want[(f"ring<{nt},1,{shape},lnf0,leaky0>", "staged")] = True
            want[(f"ring<{nt},0,{shape},lnf1,leaky0>", "staged")] = True
            want[(f"ring<{nt},0,{shape},lnf1,leaky0>", "register")] = False
            want[(f"ring<{nt},0,{shape},lnf0,leaky1>", "staged")] = True
        want[(f"ring<{nt},0,8,4,lnf0,leaky0>", "staged")] = True
        want[(f"ring<{nt},0,8,4,lnf0,leaky0>", "register")] = False
        for ovl in (0, 1):
            want[(f"ring64<{nt},0,lnf0,ovl{ovl}>", "staged")] = True
            want[(f"ring64<{nt},0,lnf0,ovl{ovl}>", "register")] = False
            want[(f"ring64<{nt},1,lnf0,ovl{ovl}>", "staged")] = True
            want[(f"ring64<{nt},0,lnf1,ovl{ovl}>", "staged")] = True
            want[(f"ring64<{nt},0,lnf1,ovl{ovl}>", "register")] = False
        # split-K: the slab stores of each main loop on their own (fp32 partial sums; full or ragged is the split kinds' matter)
        want[(f"pp<{nt},geglu0,slab1>", "slab")] = False
        for wm in (2, 4):
            want[(f"staged<{nt},0,{wm}>", "staged.slab")] = False
        want[(f"ring<{nt},0,8,8,lnf0,leaky0>", "staged.slab")] = False
        for kernel in [f"ring<{nt},0,4,4,lnf0,leaky0>", f"ring<{nt},0,8,4,lnf0,leaky0>", f"ring64<{nt},0,lnf0,ovl0>",
                       f"ring64<{nt},0,lnf0,ovl1>"]:
            want[(kernel, "staged.slab")] = False
            want[(kernel, "register.slab")] = False
    want[("small_gemm", "small")] = True
    # ragged N: never on 160-wide tiles (n_packed % 160 == 0 selects them) nor on the small kernel (n % 32 == 0)
    narrow5 = lambda kernel: kernel.startswith(("staged<5", "ring64<5")) or (kernel.startswith("ring<5") and ",4,4," in kernel)
    return {k: (ok, ok and not narrow5(k[0]) and k[0] != "small_gemm") for k, ok in want.items()}


def missing(cases=None):
    """What the list of cases does not cover -> list of strings (empty: complete)."""
    cases = CASES if cases is None else cases
    seen, axes_lds, axes_staged = {}, set(), set()
    kinds, modes = set(), set()
    for cid, key, knobs, case in cases:
        p = R.plan(case, knobs)
        form = p["epilogue"].split(".")[0]
        if case.split_k > 1 and form != "slab":
            form += ".slab"
        s = seen.setdefault((p["kernel"], form), [False, False])
        s[0] |= p["ragged_m"]
        s[1] |= p["ragged_n"]
        (axes_lds if key in LDS_DMA else axes_staged if key in STAGED else set()).update(_axes(case, p))
        if case.split_k > 1:
            kinds.add((split_kind(case), p["ragged_m"] or p["ragged_n"]))
            for mode in (1, 2):
                if in_launch_mode(case, knobs, mode) == mode:
                    modes.add((mode, "pingpong" if key == "pingpong" else form))
    out = []
    for (kernel, form), (m_ok, n_ok) in expected_instantiations().items():
        s = seen.get((kernel, form))
        if s is None:
            out.append(f"instantiation {kernel} / {form} has no case")
            continue
        if m_ok and not s[0]:
            out.append(f"instantiation {kernel} / {form} has no case with ragged M")
        if n_ok and not s[1]:
            out.append(f"instantiation {kernel} / {form} has no case with ragged N")
    for a in AXES_BOTH:
        if a not in axes_lds:
            out.append(f"axis value '{a}' on no LDS-DMA body")
        if a not in axes_staged:
            out.append(f"axis value '{a}' on no register-staged body")
    for a in AXES_LDS_ONLY:
        if a not in axes_lds:
            out.append(f"axis value '{a}' on no LDS-DMA body")
    for kind in SPLIT_KINDS:
        for ragged in (False, True):
            if (kind, ragged) not in kinds:
                out.append(f"split kind '{kind}' on no {'ragged' if ragged else 'full-tile'} shape")
    # the in-launch finish: each mode on the ring's staged slab stores, its register slab stores and the ping-pong kernel
    for mode in (1, 2):
        for form in ("staged.slab", "register.slab", "pingpong"):
            if (mode, form) not in modes:
                out.append(f"no split case finishes in the launch in mode {mode} on {form}")
    return out
