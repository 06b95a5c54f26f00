"""A helper, not a test: the launches of tests/test_gpu_norm_groups.py.  Every GroupNorm case names the form and, for the
register forms, the kernel body gn_regs_kernel<T, threads, items, pw> it is there for; tests/test_norm_ref_cpu.py asserts with
mobi_groupnorm_kernel_variant (a query, no launch) that it lands there under its knobs, and that the list covers every body
a sweep of the query can reach.  Shapes are the smallest found with the query at batch 1: `ragged` has hw no multiple of the
pixel slots with the last item partly filled, `full` has hw = slots x items (where that is reachable: the 256-thread body with
12 items only exists in the window below 2048 pieces, the 1024-thread body with 2 items only at exactly 2048).

  CASES        (id, form, body or None, Case): plain register bodies, two sources, production shapes at batch 3, both sides
               of the batch rule that switches the piece width; the slab bodies with 2 / 3 / 4 / 5 / 9 slabs, with and without
               bias / rowvec / strided residual / `finished`, row_stride > c0, a second source behind the split one; the
               two-launch form and its precise variants; the LDS form and the first shape beyond it;
  LN_CASES     (id, body (MAXV, LPR), LnCase): all five bodies, full and ragged last lanes, row counts around a block and
               inside a wave, strided source and output images.
The chunks-through-memory form keeps its own tests (it spins on its siblings): no case here may land on it."""
from tests.norm_ref import Case, LnCase

# case id -> margin of criteria 3 and 4 where the restatement and its permuted twin need more than norm_ref.MARGIN against
# each other (tests/test_norm_ref_cpu.py's margin check).  None does.
MARGINS = {}

FUSED0 = (("MOBI_GN_FUSED", "0"),)
FUSED1 = (("MOBI_GN_FUSED", "1"),)
SPLIT_PW4 = (("MOBI_GN_SPLIT_PW4", "1"),)

# ---- plain register bodies: body -> [(tag, Case)] --------------------------------------------------------------------
REGS = {
    (256, 1, 8): [("ragged", Case(1, 1, 256)), ("full", Case(1, 64, 256))],
    (256, 2, 8): [("ragged", Case(1, 65, 256)), ("full", Case(1, 102, 640)), ("two.320+320", Case(2, 52, 320, 320))],
    (256, 3, 8): [("ragged", Case(1, 103, 320)), ("full", Case(1, 153, 1280))],
    (256, 4, 8): [("ragged", Case(1, 154, 320)), ("full", Case(1, 68, 960)), ("prod.64x960.b3", Case(3, 64, 960))],
    (256, 6, 8): [("ragged", Case(1, 256, 320)), ("full", Case(1, 102, 1920)), ("two.320+640", Case(2, 77, 320, 640)),
                  ("two.1280+640", Case(2, 77, 1280, 640)), ("two.960+960", Case(2, 77, 960, 960))],
    (256, 8, 8): [("ragged", Case(1, 358, 320)), ("full", Case(1, 408, 320))],
    (256, 12, 8): [("ragged", Case(1, 409, 320))],
    (1024, 2, 8): [("full", Case(1, 512, 256))],
    (1024, 3, 8): [("ragged", Case(1, 513, 256)), ("full", Case(1, 612, 1280)), ("prod.256x2560.b3", Case(3, 256, 2560))],
    (1024, 4, 8): [("ragged", Case(1, 769, 256)), ("full", Case(1, 816, 1280))],
    (1024, 6, 8): [("ragged", Case(1, 1021, 1280)), ("full", Case(1, 612, 2560)), ("prod.1024x1280.b3", Case(3, 1024, 1280)),
                   ("batch32.1024x320", Case(32, 1024, 320))],
    (1024, 8, 8): [("ragged", Case(1, 1429, 1280)), ("full", Case(1, 816, 2560))],
    (1024, 12, 8): [("ragged", Case(1, 2245, 1280)), ("full", Case(1, 1224, 2560)), ("prod.1024x2560.b3", Case(3, 1024, 2560))],
    (1024, 16, 8): [("ragged", Case(1, 3061, 1280)), ("full", Case(1, 1632, 2560))],
    (1024, 8, 4): [("ragged", Case(1, 1429, 320)), ("full", Case(1, 1632, 640)), ("prod.256x1920.b3", Case(3, 256, 1920)),
                   ("batch16.1024x320", Case(16, 1024, 320))],
    (1024, 12, 4): [("ragged", Case(1, 2245, 320)), ("full", Case(1, 816, 960))],
    (1024, 16, 4): [("ragged", Case(1, 3061, 320)), ("full", Case(1, 1088, 960)), ("prod.4096x512.b3", Case(3, 4096, 512))],
    (1024, 24, 4): [("ragged", Case(1, 1565, 960)), ("full", Case(1, 1632, 1920))],
}
# gn_regs_kernel instantiations no shape reaches (tests/test_norm_ref_cpu.py's sweep): 16 items need 256 threads and at least
# 2048 pieces at once; one item of 1024 threads is at most 1024 pieces, which takes 256 threads
UNREACHABLE_REGS = {(256, 16, 8), (1024, 1, 8)}

# ---- slab bodies (src0 from split-K slabs, C ABI with synthetic slabs) ------------------------------------------------
SLABS = {
    (256, 1, 8): [("s2.bias", Case(2, 33, 256, splits=2, bias=True))],
    (256, 2, 8): [("s3.rowvec", Case(1, 65, 256, splits=3, rowvec="dense")),
                  ("s2.two.320+320", Case(2, 52, 320, 320, splits=2, finished=True))],
    (256, 3, 8): [("s4.res", Case(1, 103, 320, splits=4, residual="dense"))],
    (256, 4, 8): [("s5.all", Case(2, 154, 320, splits=5, bias=True, rowvec="strided", residual="strided", finished=True))],
    (256, 6, 8): [("s9.finished", Case(1, 256, 320, splits=9, finished=True))],
    (256, 8, 8): [("s2.rowstride.bias", Case(1, 358, 320, splits=2, bias=True, row_extra=64))],
    (1024, 2, 8): [("s4.all", Case(2, 512, 256, splits=4, bias=True, rowvec="dense", residual="strided", finished=True))],
    (1024, 3, 8): [("s5.two.640+640", Case(1, 410, 640, 640, splits=5, bias=True, finished=True)),
                   ("s3.res", Case(1, 513, 256, splits=3, residual="dense"))],
    (1024, 4, 8): [("s2.plain", Case(1, 769, 256, splits=2))],
    (1024, 6, 8): [("s4.bias.rowvec", Case(1, 1021, 1280, splits=4, bias=True, rowvec="strided"))],
    (1024, 8, 8): [("s9.res.finished.rowstride", Case(1, 1429, 1280, splits=9, residual="strided", finished=True, row_extra=32))],
    (1024, 8, 4): [("s3.pw4", Case(1, 1429, 320, knobs=SPLIT_PW4, splits=3, bias=True, finished=True))],
}
UNREACHABLE_SLABS = {(1024, 1, 8)}

# ---- two launches (MOBI_GN_FUSED=0), the precise variants, the LDS form (MOBI_GN_FUSED=1) -----------------------------
CAP_CASE = Case(16, 3277, 320, knobs=FUSED0)       # 129 blocks of 1024 pieces per image against a cap of 2048 / 16 = 128
TWO = [("c32.hw1", Case(2, 1, 32, knobs=FUSED0)), ("c96.hw31", Case(2, 31, 96, knobs=FUSED0)),
       ("c128.hw32", Case(2, 32, 128, knobs=FUSED0)), ("c2560.hw33", Case(2, 33, 2560, knobs=FUSED0)),
       ("c96.hw2049", Case(2, 2049, 96, knobs=FUSED0)), ("c2560.hw1", Case(1, 1, 2560, knobs=FUSED0)),
       ("two.64+32.hw33", Case(2, 33, 64, 32, knobs=FUSED0)), ("two.320+640.hw31", Case(2, 31, 320, 640, knobs=FUSED0)),
       ("cap.16x3277x320", CAP_CASE)]
PRECISE = [(f"f32src.mode{m}", Case(2, 33, 128, src_f32=True, out_mode=m, eps=1e-6)) for m in range(4)] + \
          [(f"tsrc.mode{m}", Case(2, 2049, 96, out_mode=m, eps=1e-6)) for m in (1, 2, 3)] + \
          [("tsrc.two.64+32.mode2", Case(2, 31, 64, 32, out_mode=2))]
LDS_FORM = [("exact32768", Case(1, 1024, 1024, knobs=FUSED1)), ("hw1", Case(2, 1, 64, knobs=FUSED1)),
            ("two.320+640", Case(2, 100, 320, 640, knobs=FUSED1))]
BEYOND_LDS = Case(1, 1025, 1024, knobs=FUSED1)     # one pixel more than the LDS slab holds: two launches


def body_key(form, body):
    return form if body is None else f"{form}.{body[0]}x{body[1]}x{body[2]}"


CASES = []
for _body, _lst in REGS.items():
    CASES += [(f"{body_key('regs', _body)}.{tag}", "regs", _body, case) for tag, case in _lst]
for _body, _lst in SLABS.items():
    CASES += [(f"{body_key('slabs', _body)}.{tag}", "slabs", _body, case) for tag, case in _lst]
CASES += [(f"two.{tag}", "two", None, case) for tag, case in TWO]
CASES += [(f"precise.{tag}", "precise", None, case) for tag, case in PRECISE]
CASES += [(f"lds.{tag}", "lds", None, case) for tag, case in LDS_FORM]
CASES.append(("two.beyond_lds", "two", None, BEYOND_LDS))
KEYS = list(dict.fromkeys(body_key(form, body) for _, form, body, _ in CASES))
assert len({cid for cid, *_ in CASES}) == len(CASES)


def cases_of(key):
    return [(cid, form, body, case) for cid, form, body, case in CASES if body_key(form, body) == key]


# ---- LayerNorm --------------------------------------------------------------------------------------------------------
LN_BODIES = {8: (1, 8), 64: (1, 8), 72: (5, 8), 200: (5, 8), 320: (5, 8), 328: (5, 16), 640: (5, 16), 648: (5, 32),
             1280: (5, 32), 1288: (5, 64), 2560: (5, 64)}


def ln_row_counts(lpr):
    """1, one short of a block, one past it, and a count that ends inside the second wave of the second block (LPR = 64 has
    one row per wave: there it ends between two waves)."""
    rpw = 64 // lpr
    return [1, 4 * rpw - 1, 4 * rpw + 1, 5 * rpw + max(rpw // 2, 1)]


LN_CASES = []
for _c, _b in LN_BODIES.items():
    for _r in ln_row_counts(_b[1]):
        LN_CASES.append((f"ln.{_b[0]}x{_b[1]}.c{_c}.rows{_r}", _b, LnCase(1, _r, _c)))
    _r = ln_row_counts(_b[1])[2]
    LN_CASES.append((f"ln.{_b[0]}x{_b[1]}.c{_c}.strided", _b, LnCase(3, _r, _c, src_gap=8 * 3, out_gap=8 * 5)))
