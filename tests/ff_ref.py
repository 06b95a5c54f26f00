"""The fused GEGLU feed-forward (mobi_ff_geglu, csrc/ff.hip) in plain torch on the CPU: the float64 reference of the contract
in include/mobi_engine.h, the fp32 restatement with the kernel's rounding points, the row / channel measures, the criteria and
the operand builder of tests/test_gpu_ff_rows.py.  Nothing here launches anything or needs a GPU (tests/test_ff_ref_cpu.py
runs it alone); the builder only needs one when asked for device views.

A case is a `Case`; its host operands (`host_operands`) are ALREADY what the kernel reads:
  x [rows, c] T   res [rows, c] T | None (`x` itself for residual == "x")   buf uint8: the packed chunk images
  dec = (W1 [2 hidden, c] T, b1 [2 hidden] f32, W2 [c, hidden] T): launch_shadow.decode_ff_geglu of `buf`, the header's formula
  b2 f32 [c] | None   gamma, beta f32 [c] | None
The reference and the restatement multiply `dec`, i.e. what the packed buffer really holds."""
import dataclasses
import functools
import math

import torch

from oracle import weights as W
from tests.backward_ref import rel_l2, row_measure  # noqa: F401  (the suite's row measure, as it is)
from tests.igemm_ref import MARGIN, Placed, _bits, place, storage_name  # noqa: F401

C = 320
LN_EPS = 1e-5
# b1 = B1_SCALE x synth_param's bias (0.05 z) beside pre-activations of std 2.  Scale 1 (test_ff_geglu_fused's) is enough: the
# CPU mutant that forms chunk c with b1 of chunk c - 1 is rejected on every case; the narrowest is bf16 at hidden = 1280 (one
# chunk of 40), where its worst row is 4.6 x the restatement's against the margin of 2 (37 x in fp16); at 0.5 it would be
# 2.6 x (tests/test_ff_ref_cpu.py test_b1_scale_rejects_the_swap_with_room).
B1_SCALE = 1.0
LN_REGIMES = ("standard", "off16", "off128", "small", "small_off", "const", "spike", "mixed")


@dataclasses.dataclass(frozen=True)
class Case:
    rows: int
    hidden: int
    residual: str = "separate"          # "" | "separate" | "inplace" (out IS the residual) | "x" (the residual IS x: norm3's call)
    b2: bool = True
    ln: str = ""                        # "" | one of LN_REGIMES: LayerNorm inside the kernel, x drawn from that regime
    c: int = C

    @property
    def chunks(self):
        return self.hidden // 32

    @property
    def form(self):
        res = {"": "nores", "separate": "res", "inplace": "inplace", "x": "resx"}[self.residual]
        return ("ln+" if self.ln else "") + ("b2" if self.b2 else "nob2") + "+" + res

    @property
    def name(self):
        return f"h{self.hidden}.r{self.rows}" + (f".{self.ln}" if self.ln else "")


# ----------------------------------------------------------------------------------------------------------------------
# data
def ln_rows(regime, rows, c=C):
    """fp64 rows of one LayerNorm regime, not yet rounded: the generators and magnitudes of tests/test_gpu_norm_stats.py
    (regime_data: offsets 16 and 128, spread 2 sqrt(eps), the -1 fill and the 10.3 constant) on 7 'images' of rows / 7 rows;
    'standard' is test_ff_geglu_fused's 1.7 z + 0.4; 'spike' puts that file's offset 16 on one channel of each row (another
    channel per row: half the row's variance in one channel; at 128 the first product is that one channel's term and its
    single rounding, and the restatement itself misses TOL); 'mixed' takes row r from regime r mod 7, so neighbours in a wave
    tile differ."""
    from tests.test_gpu_norm_stats import EPS_UNET, OFFSETS, regime_data
    assert EPS_UNET == LN_EPS and rows % 7 == 0
    shape = (7, rows // 7, c)
    if regime == "standard":
        return (1.7 * W.synth_input("ffr.ln.standard", (rows, c)).double() + 0.4)
    if regime == "spike":
        x = W.synth_input("ffr.ln.spike", (rows, c)).double()
        r = torch.arange(rows)
        x[r, (37 * r + 5) % c] = OFFSETS[0]
        return x
    if regime == "mixed":
        parts = [ln_rows(k, rows, c) for k in LN_REGIMES[:-1]]
        x = parts[0].clone()
        for i, p in enumerate(parts):
            x[i::len(parts)] = p[i::len(parts)]
        return x
    return regime_data(regime, "ffr.ln." + regime, shape, LN_EPS)[0].reshape(rows, c)


@functools.lru_cache(maxsize=None)
def _masters(hidden, c):
    """fp32 masters with the names and scales of test_ff_geglu_fused (W1 and W2 x 2), b1 x B1_SCALE."""
    p = lambda name, shape: torch.from_numpy(W.synth_param(name, shape))
    return (p("ff.w1.weight", (2 * hidden, c)) * 2.0, p("ff.w1.bias", (2 * hidden,)), p("ff.w2.weight", (c, hidden)) * 2.0,
            p("ff.w2.bias", (c,)))


@functools.lru_cache(maxsize=None)
def packed(hidden, dtype, b1_scale=B1_SCALE, c=C):
    """(buf uint8 on the CPU, decode of buf, b2): ops.pack_ff_geglu's images and what launch_shadow.decode_ff_geglu reads back."""
    from mobi_amd import ops
    from tests.launch_shadow import decode_ff_geglu
    w1, b1, w2, b2 = _masters(hidden, c)
    pf = ops.pack_ff_geglu(w1, b1 * b1_scale, w2, b2, dtype, "cpu")
    return pf.buf, decode_ff_geglu(pf.buf, c, hidden, dtype), pf.b2


def host_operands(case, dtype, b1_scale=B1_SCALE):
    """Deterministic in the case: x and the residual N(0, 1) (x of a LayerNorm case: `ln_rows`), rounded to T; gamma, beta
    from synth_param (1 + 0.1 z, 0.05 z)."""
    buf, dec, b2 = packed(case.hidden, dtype, b1_scale, case.c)
    if case.ln:
        x = ln_rows(case.ln, case.rows, case.c).to(dtype)
    else:
        x = W.synth_input(f"ffr.x{case.rows}", (case.rows, case.c)).to(dtype)
    res = {"": None, "x": x}.get(case.residual, W.synth_input(f"ffr.r{case.rows}", (case.rows, case.c)).to(dtype))
    gamma = torch.from_numpy(W.synth_param("ffr.ln.weight", (case.c,))) if case.ln else None
    beta = torch.from_numpy(W.synth_param("ffr.ln.bias", (case.c,))) if case.ln else None
    return dict(x=x, res=res, buf=buf, dec=dec, b2=b2 if case.b2 else None, gamma=gamma, beta=beta)


# ----------------------------------------------------------------------------------------------------------------------
# the contract
def gelu_erf(g):
    return 0.5 * g * (1.0 + torch.special.erf(g * (1.0 / math.sqrt(2.0))))


def layernorm64(x, gamma, beta, eps=LN_EPS):
    x = x.double()
    mean = x.mean(dim=1, keepdim=True)
    var = (x - mean).square().mean(dim=1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def pre_activations(case, o):
    """float64 (value, gate) pre-activations [rows, hidden] each."""
    w1, b1, _ = o["dec"]
    x = layernorm64(o["x"], o["gamma"], o["beta"]) if case.ln else o["x"].double()
    pre = x @ w1.double().T + b1.double()
    return pre[:, :case.hidden], pre[:, case.hidden:]


def reference(case, o):
    """float64: ((x' W1v^T + b1v) * gelu_erf(x' W1g^T + b1g)) W2^T + b2 + residual, x' = x or LayerNorm(x); the hidden
    activation is not rounded, erf is exact."""
    val, gate = pre_activations(case, o)
    y = (val * gelu_erf(gate)) @ o["dec"][2].double().T
    if o["b2"] is not None:
        y = y + o["b2"].double()
    if o["res"] is not None:
        y = y + o["res"].double()
    return y


# ----------------------------------------------------------------------------------------------------------------------
# the kernel's arithmetic
def restated(case, o, dtype, fault=None, order="kernel"):
    """The same operation in fp32 torch with the rounding points csrc/ff.hip documents and nothing else (ff_geglu_kernel,
    cited as a phrase of the line):
      * LayerNorm: `s1 += (float)xf[ks][j]` and `const float mean = s1 * (1.0f / C)`: an fp32 mean; `const float d =
        (float)xf[ks][j] - mean; q += d * d`: the variance about the mean; `rsqrtf(q * (1.0f / C) + a.ln_eps)`; the result
        rounded to T: `xf[ks][j] = (T)(((float)xf[ks][j] - mean) * rstd * g0[j] + h0[j])`;
      * first product: operands T, an fp32 sum that starts from b1 (`nv[4 * q + j] = v[j]`, `va[4 * q + j] = v[j]`, then
        `nv = mfma32(f, xf[ks], nv)`);
      * the gate in fp32: `hv[e] * gelu_erf_f(hg[e])`;
      * H rounded to T: `v2[0] = (T)he[0]` (step) and `v[0] = (T)h0` (gate2);
      * second product: an fp32 sum over the chunks in ascending order, `o[m] = mfma32(f, __builtin_bit_cast(frag_t, pu), o[m])`
        from `o[m][r] = 0.f`;
      * epilogue: `v += b` (b2, fp32), `f[j] += rf[j]` (the residual read as T), ONE rounding `st16(outp + off, pack8<T>(f))`.
    torch.erf stands for gelu_erf_f (a polynomial within ~1.5e-7 of it, far below the rounding of H).
    order: "kernel" | "reversed" (every k sum in the opposite order) | "f64" (sums in float64, rounded to fp32 at the same
    points).  `fault` plants one of the mutants of tests/test_ff_ref_cpu.py (a dict; a launch has none).  Returns fp32."""
    f32 = torch.float32
    fault = fault or {}
    acc_t = torch.float64 if order == "f64" else f32
    flip = (lambda t: t.flip(-1)) if order == "reversed" else (lambda t: t)
    w1, b1, w2 = o["dec"]
    w1, w2 = w1.float(), w2.float()
    hid, nch, rows = case.hidden, case.chunks, case.rows
    x = o["x"].float()
    if case.ln:
        gi = fault.get("gamma_index", torch.arange(case.c))
        gamma, beta = o["gamma"][gi], o["beta"][gi]
        inv_c = torch.tensor(1.0 / case.c, dtype=f32)
        eps = torch.tensor(0.0 if fault.get("ln_no_eps") else LN_EPS, dtype=f32)
        mean = flip(x).to(acc_t).sum(dim=1, keepdim=True).to(f32) * inv_c
        if fault.get("ln_one_pass"):
            var = flip(x * x).to(acc_t).sum(dim=1, keepdim=True).to(f32) * inv_c - mean * mean
        else:
            d = x - mean
            var = flip(d * d).to(acc_t).sum(dim=1, keepdim=True).to(f32) * inv_c
        x = ((x - mean) * torch.rsqrt(var + eps) * gamma + beta).to(dtype).float()
    mm = lambda a, b: (flip(a).to(acc_t) @ flip(b).to(acc_t).T)
    order_c = list(range(nch))[::-1] if order == "reversed" else list(range(nch))
    out = torch.zeros((rows, case.c), dtype=acc_t)
    for ch in order_c:
        sl = slice(32 * ch, 32 * ch + 32)
        bc = fault.get("b1_chunk", {}).get(ch, ch)
        bsl = slice(32 * bc, 32 * bc + 32)
        val = (b1[bsl].to(acc_t) + mm(x, w1[sl])).to(f32)
        gate = (b1[hid:][bsl].to(acc_t) + mm(x, w1[hid:][sl])).to(f32)
        if ch in fault.get("swap_value_gate", ()):
            val, gate = gate, val
        h = val * (gate if ch in fault.get("no_gelu", ()) else gelu_erf(gate))
        h = h.to(dtype).float()
        part = mm(h, w2[:, sl]) * fault.get("chunk_weight", {}).get(ch, 1.0)
        if ch in fault.get("chunk_missing_in_tile", {}):
            r0 = fault["chunk_missing_in_tile"][ch]
            part[r0:r0 + 32] = 0.0
        out = out + part
    out = out.to(f32)
    if o["b2"] is not None:
        out = out + o["b2"] * fault.get("b2_mask", 1.0)
    if o["res"] is not None:
        res = o["res"].float()
        out = out + (res[fault["residual_rows"]] if "residual_rows" in fault else res)
    out = out.to(dtype).float()
    return out[fault["row_perm"]] if "row_perm" in fault else out


# ----------------------------------------------------------------------------------------------------------------------
# measures and criteria (all on [rows, c])
def channel_measure(got, ref):
    """igemm_ref.channel_measure's definition on [rows, c]: the worst channel's |got - ref|_2 over its rows, over the rms of
    the reference's channel norms."""
    return row_measure(got.detach().double().cpu().T, ref.detach().double().cpu().T)


def tolerance(dtype):
    from tests.test_gpu_ops import TOL
    return TOL[dtype]


def judge(dtype, got, ref, rest):
    """Criteria 2 and 3 of tests/test_gpu_ff_rows.py (and the finiteness of criterion 1) on one output -> (figures, failures);
    the keys of `failures` name the criterion: finite, rel, row, channel."""
    got = got.detach().cpu()
    fig, bad = {}, {}
    nonfinite = int((~torch.isfinite(got)).sum())
    if nonfinite:
        bad["finite"] = f"{nonfinite} non-finite outputs"
        got = torch.nan_to_num(got.float(), nan=0.0, posinf=0.0, neginf=0.0)
    tol = tolerance(dtype)
    fig["rel"], fig["rel.restated"] = rel_l2(got, ref), rel_l2(rest, ref)
    if not fig["rel"] < tol:
        bad["rel"] = f"rel-L2 {fig['rel']:.3e} >= {tol:.1e}"
    for key, measure in (("row", row_measure), ("channel", channel_measure)):
        k, r = measure(got, ref), measure(rest, ref)
        fig[key], fig[key + ".restated"] = k, r
        if not k <= MARGIN * r:
            bad[key] = f"{key} measure {k:.3e} > {MARGIN:g} x restated {r:.3e}"
    return fig, bad


# ----------------------------------------------------------------------------------------------------------------------
# operands on the device
WEIGHT_GUARD = 64 * 1024                # bytes in front of and behind the chunk images: more than one image (61 KiB)
NAN_BYTES = (0xC0, 0x7F)                # 0x7FC0 per 16 bits: a NaN as fp16, as bf16 and (0x7FC07FC0) as fp32


def place_weights(buf, device):
    """The packed images inside a larger byte allocation whose every other 16-bit word is a NaN pattern; the view starts at a
    multiple of 16 bytes."""
    assert buf.dtype == torch.uint8 and buf.numel() % 16 == 0 and WEIGHT_GUARD % 16 == 0
    whole = torch.tensor(NAN_BYTES, dtype=torch.uint8).repeat((2 * WEIGHT_GUARD + buf.numel()) // 2)
    whole[WEIGHT_GUARD:WEIGHT_GUARD + buf.numel()] = buf
    d = whole.to(device)
    assert d.data_ptr() % 16 == 0
    return Placed(d, d[WEIGHT_GUARD:WEIGHT_GUARD + buf.numel()])


class Operands:
    """The device side of one (case, dtype): x, residual, out, b2, gamma, beta each a view inside a NaN-filled allocation
    (igemm_ref.place), the chunk images between NaN guard bytes, the output view NaN before the launch (or the residual, in
    place).  `unchanged()`: the input allocations are bit for bit what was uploaded; `outside_unchanged()`: nothing outside
    the output view was written (launch_shadow.OutsideView)."""

    def __init__(self, case, dtype, o, device="cuda"):
        from tests.launch_shadow import OutsideView
        self.case, self.dtype = case, dtype
        c = case.c
        guard = 8 * (c // 8 + 2)                                     # more than one row
        rows2d = lambda t: place(t.reshape(1, -1, c), t.numel(), device, guard)
        f32p = lambda t: None if t is None else place(t.reshape(1, -1), t.numel(), device, 8)
        self.x = rows2d(o["x"])
        self.w = place_weights(o["buf"], device)
        self.b2, self.gamma, self.beta = f32p(o["b2"]), f32p(o["gamma"]), f32p(o["beta"])
        self.res = self.x if case.residual == "x" else (None if o["res"] is None else rows2d(o["res"]))
        if case.residual == "inplace":
            self.out = self.res
        else:
            self.out = rows2d(torch.full((case.rows, c), float("nan"), dtype=dtype))
        self.inputs = [p for p in (self.x, self.w, self.b2, self.gamma, self.beta,
                                   None if case.residual in ("inplace", "x") else self.res) if p is not None]
        self._bits = [self._raw(p.buffer).clone() for p in self.inputs]
        self.outside = OutsideView(self.out.view)
        self._out0 = _bits(self.out.buffer).clone()

    @staticmethod
    def _raw(t):
        return t if t.dtype == torch.uint8 else _bits(t)

    def pointers(self):
        """Field name of mobi_ff_geglu_params -> address (absent: NULL)."""
        ptr = dict(x=self.x.view.data_ptr(), w_packed=self.w.view.data_ptr(), out=self.out.view.data_ptr())
        for name, p in (("b2", self.b2), ("residual", self.res), ("ln_gamma", self.gamma), ("ln_beta", self.beta)):
            if p is not None:
                ptr[name] = p.view.data_ptr()
        return ptr

    def reset_output(self):
        """The output allocation as it was before the first launch (NaN, or the residual of an in-place case)."""
        _bits(self.out.buffer).copy_(self._out0)

    def output_untouched(self):
        return torch.equal(_bits(self.out.buffer), self._out0)

    def unchanged(self):
        return all(torch.equal(self._raw(p.buffer), b) for p, b in zip(self.inputs, self._bits))

    def outside_unchanged(self):
        return self.outside.unchanged()


def fill_params(p, case, dtype, ptr):
    """Set the fields of a mobi_ff_geglu_params-shaped object `p` (mobi_amd._lib.FfGegluParams); ptr: addresses by field name."""
    for name in ("x", "w_packed", "b2", "residual", "out", "ln_gamma", "ln_beta"):
        setattr(p, name, ptr.get(name))
    p.rows, p.c, p.hidden = case.rows, case.c, case.hidden
    p.dtype = 0 if dtype == torch.float16 else 1                    # MOBI_F16 / MOBI_BF16
    p.ln_eps = LN_EPS if case.ln else 0.0
    return p
