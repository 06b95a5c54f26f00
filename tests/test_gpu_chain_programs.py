"""GPU parity of mobi_row_chain (csrc/chain.hip) per launch and program form (`-m gpu`): every case of tests/chain_cases.py
-- the three production programs built with the calls of ldm/modules/attention.py, each of the six accepted product flag
sets as a form of its own, programs of 1 .. 4 products, two programs of 1 and 4 products, STORE_S, a LOAD_S in the middle of
a program, row-strided sources, img_div on a load and on a bias, the adapter with 1 / 2 / 5 / 8 heads -- against the fp64
interpreter of the header's contract (tests/chain_ref.py) on the operands the launch read:
  whole-tensor rel-L2 within the bound tests/test_gpu_chain.py asserts for the form (TOL; 1.5 TOL for a folded product), the
  worst 128 x 64 tile within 4x that, finite, inputs bit-unchanged, the destinations' storage outside the written rows
  bit-unchanged (containers pre-filled with a fixed pattern), a second run bit-equal.
Shapes (images, rows per image): (2, 128) one tile per image; (4, 256) two tiles and img / 2; (4, 8320) = 260 workgroups for
the production two-program form.  tests/test_chain_ref_cpu.py holds an fp32 emulation of every case within half these bounds.

The rejection matrix needs no launch: every rule of mobi_row_chain is checked on the host in front of the launch; each
program the kernel cannot run must come back with its documented error code and leave the destination untouched."""
import ctypes

import pytest
import torch

from tests import chain_cases as cc, chain_ref
from tests.golden_cases import record
from tests.launch_shadow import TILE_FACTOR

pytestmark = pytest.mark.gpu
DT = [torch.float16, torch.bfloat16]
C = 320
OK, ERR_ARG, ERR_UNSUPPORTED, ERR_ALIGN = 0, -1, -2, -4          # include/mobi_engine.h


def _dname(dtype):
    return "fp16" if dtype == torch.float16 else "bf16"


@pytest.mark.parametrize("dtype", DT, ids=_dname)
@pytest.mark.parametrize("key", list(cc.CASES))
def test_chain_program(key, dtype):
    from mobi_amd import ops
    case = cc.build_case(key, dtype, "cuda", chain_ref.recording_program())
    adapter = None
    if case.tables is not None:
        tb = case.tables
        adapter = (ops.chain_adapter_image(tb["a"], tb["c"], tb["u"], tb["b"], dtype), tb["eps"])

    def report(name, rel, tile, bound):
        print(f"[chain {key} {_dname(dtype)}] {name:40s} rel={rel:.3e} tile={tile:.3e} bound={bound:.1e}")
        record(f"chain {key} {name}", rel, bound)
        record(f"chain {key} {name} worst_tile", tile, TILE_FACTOR * bound)

    bad = cc.judge(case, lambda: ops.row_chain(case.programs, case.images, case.rows, dtype, adapter=adapter), report=report)
    assert not bad, "\n".join(bad)


# ---- rejection matrix ---------------------------------------------------------------------------------------------------
class _Params:
    """A valid two-product program (LOAD_S, LOAD_R, PRODUCT RESID | TO_S | STORE, PRODUCT STORE) as a raw RowChainParams that a
    case then breaks in one place."""

    def __init__(self):
        from mobi_amd import _lib
        L = self.L = _lib
        dt = torch.float16
        z = lambda *s: torch.zeros(s, device="cuda", dtype=dt)
        self.x, self.r = z(2, 128, C), z(2, 128, C)
        self.dst = torch.full((2, 2, 128, C), cc.FILL, dtype=torch.int16, device="cuda").view(dt)
        self.w = torch.zeros((3, 204800), device="cuda", dtype=torch.uint8)
        self.bias = torch.zeros((2, C), device="cuda", dtype=torch.float32)
        self.ad = torch.zeros((2, L.load().mobi_row_chain_adapter_image_bytes(C)), device="cuda", dtype=torch.uint8)
        p = self.p = L.RowChainParams()
        p.dtype, p.channels, p.images, p.rows_per_image, p.nprog = L.MOBI_F16, C, 2, 128, 1
        ops_ = [self.load(L.CH_LOAD_S, self.x), self.load(L.CH_LOAD_R, self.r),
                self.product(0, L.CH_RESID | L.CH_TO_S | L.CH_STORE, 0, nxt=1), self.product(1, L.CH_STORE, 1)]
        self.set(0, ops_)

    def set(self, k, ops_):
        self.p.nops[k] = len(ops_)
        for i, o in enumerate(ops_):
            self.p.prog[k][i] = o

    def op(self, code, flags=0):
        o = self.L.ChainOp()
        o.code, o.flags = code, flags
        return o

    def load(self, code, t):
        o = self.op(code)
        o.p0, o.img_stride, o.row_stride, o.img_div = t.data_ptr(), t.stride(0), t.stride(1), 1
        return o

    def to_dst(self, o, slot):
        d = self.dst[slot]
        o.dst, o.dst_img_stride, o.dst_row_stride, o.dst_img_div = d.data_ptr(), d.stride(0), d.stride(1), 1
        return o

    def product(self, wi, flags, slot, nxt=None):
        o = self.op(self.L.CH_PRODUCT, flags)
        o.p0 = self.w[wi].data_ptr()
        o.p1 = None if nxt is None else self.w[nxt].data_ptr()
        o.bias = self.bias.data_ptr()
        o.svec = self.bias.data_ptr()
        return self.to_dst(o, slot) if flags & self.L.CH_STORE else o

    def run(self):
        code = self.L.load().mobi_row_chain(ctypes.byref(self.p), None)
        torch.cuda.synchronize()
        return code, bool((self.dst.view(torch.int16) == cc.FILL).all())


def _five_products(q):
    L = q.L
    q.set(0, [q.load(L.CH_LOAD_S, q.x)] + [q.product(0, L.CH_STORE, 0, nxt=0) for _ in range(4)] + [q.product(0, L.CH_STORE, 0)])


def _resid_later(q):
    q.p.prog[0][3].flags = q.L.CH_RESID | q.L.CH_STORE


def _load_r_late(q):
    L = q.L
    q.set(0, [q.load(L.CH_LOAD_S, q.x), q.product(0, L.CH_STORE, 0), q.load(L.CH_LOAD_R, q.r)])


def _load_r_behind_a_product(q):
    """In the first two places, but not among the leading loads: the kernel would never issue it."""
    L = q.L
    q.set(0, [q.product(0, L.CH_STORE, 0), q.load(L.CH_LOAD_R, q.r)])


def _affine_late(q):
    L = q.L
    a = q.op(L.CH_AFFINE_S)
    a.bias = a.svec = q.bias.data_ptr()
    q.set(0, [q.load(L.CH_LOAD_S, q.x), q.product(0, L.CH_STORE, 0), a])


def _p1_wrong(q):
    q.p.prog[0][2].p1 = q.w[2].data_ptr()


def _p1_on_last(q):
    q.p.prog[0][3].p1 = q.w[0].data_ptr()


def _flags(f):
    def brk(q):
        o = q.product(0, f, 0, nxt=1)
        q.to_dst(o, 0)                              # (a destination is there whatever the flags say)
        q.p.prog[0][2] = o
    brk.__name__ = f"flags_{f}"
    return brk


def _fold_no_svec(q):
    L = q.L
    o = q.product(1, L.CH_FOLD | L.CH_STORE, 1)
    o.svec = None
    q.p.prog[0][3] = o


def _adapter(no_image=False, no_store=False, no_dst=False):
    def brk(q):
        L = q.L
        o = q.op(L.CH_ADAPTER, 0 if no_store else L.CH_STORE)
        if not no_dst:
            q.to_dst(o, 0)
        q.set(0, [q.load(L.CH_LOAD_S, q.x), o])
        if not no_image:
            q.p.ad_image, q.p.ad_eps = q.ad.data_ptr(), 1e-5
    brk.__name__ = f"adapter_image{int(not no_image)}_store{int(not no_store)}_dst{int(not no_dst)}"
    return brk


def _misalign(field, index):
    def brk(q):
        o = q.p.prog[0][index]
        setattr(o, field, getattr(o, field) + 8)
        if field == "p0" and index == 3:
            q.p.prog[0][2].p1 = o.p0                # (keep the prefetch pointer consistent: the alignment rule is what must fire)
    brk.__name__ = f"misaligned_{field}_op{index}"
    return brk


def _stride(field, index, value):
    def brk(q):
        setattr(q.p.prog[0][index], field, value)
    brk.__name__ = f"{field}_op{index}_{value}"
    return brk


def _two_programs_odd(q):
    q.p.nprog, q.p.images = 2, 3
    q.set(1, [q.p.prog[0][i] for i in range(4)])


def _nops(n):
    def brk(q):
        q.p.nops[0] = n
    brk.__name__ = f"nops_{n}"
    return brk


SIX = (8, 9, 6, 14, 10, 12)      # STORE, FOLD|STORE, RESID|TO_S, RESID|TO_S|STORE, RESID|STORE, TO_S|STORE
REJECTED = ([(_five_products, ERR_UNSUPPORTED), (_resid_later, ERR_UNSUPPORTED), (_load_r_late, ERR_UNSUPPORTED),
             (_load_r_behind_a_product, ERR_UNSUPPORTED),
             (_affine_late, ERR_UNSUPPORTED), (_p1_wrong, ERR_ARG), (_p1_on_last, ERR_ARG)]
            + [(_flags(f), ERR_UNSUPPORTED) for f in range(16) if f not in SIX]
            + [(_fold_no_svec, ERR_ARG), (_adapter(no_image=True), ERR_ARG), (_adapter(no_store=True), ERR_ARG),
               (_adapter(no_dst=True), ERR_ARG)]
            + [(_misalign(f, i), ERR_ALIGN) for f, i in (("p0", 0), ("p0", 1), ("p0", 3), ("dst", 2), ("dst", 3), ("bias", 2))]
            + [(_stride(f, i, v), ERR_ALIGN) for f, i, v in (("img_stride", 0, 128 * C + 4), ("row_stride", 1, C + 4), ("row_stride", 0, 312),
                                                            ("dst_img_stride", 2, 128 * C + 4), ("dst_row_stride", 3, C + 4),
                                                            ("dst_row_stride", 2, 312), ("bias_img_stride", 2, 322))]
            + [(_two_programs_odd, ERR_ARG), (_nops(0), ERR_ARG), (_nops(11), ERR_ARG)])


def test_the_matrix_base_program_is_accepted_and_the_six_forms_named():
    """The program every rejection case breaks in one place runs as it stands (zeros in, zeros out): a case's error code is its
    own defect's.  The six accepted flag sets are the ones the header names."""
    from mobi_amd import _lib as L
    assert set(SIX) == {L.CH_STORE, L.CH_FOLD | L.CH_STORE, L.CH_RESID | L.CH_TO_S, L.CH_RESID | L.CH_TO_S | L.CH_STORE,
                        L.CH_RESID | L.CH_STORE, L.CH_TO_S | L.CH_STORE}
    q = _Params()
    code, untouched = q.run()
    assert code == OK and not untouched and not bool(q.dst.any())
    q = _Params()
    _adapter()(q)
    assert q.run()[0] == OK


@pytest.mark.parametrize("brk,want", REJECTED, ids=[b.__name__.lstrip("_") for b, _ in REJECTED])
def test_chain_rejects(brk, want):
    q = _Params()
    brk(q)
    code, untouched = q.run()
    assert code == want, (code, want)
    assert untouched
