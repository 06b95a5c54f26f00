"""Numeric health: where in fp16's (bf16's, fp32's) range every tensor of a run lies, and the launch at which it left it.

    with health.probe(near=0.5) as hp:
        ...any eager engine work...
    rep = hp.report()            # ONE read-back of all records
    rep.first_nonfinite()        # the first row in launch order with inf + nan > 0, or None
    rep.worst(5)                 # the rows with the least headroom
    print(rep)

A row is one tensor that a launch has just written, measured by `mobi_tensor_health` on the same stream right behind the launch
(`ops._HEALTH`, tested inside the functions of ops.py that return activations): nothing is held pending, so a later in-place
writer cannot change what a row saw, and the probe keeps no activation alive (`keep=True`, for tests, keeps a clone).  While a
probe is active `graph.usable()` is False (samplers run their eager path) and `ops.concurrently` runs serially; with no probe
active nothing changes.  The module path of a row comes from forward hooks on every `nn.Module.__call__`: `<root class>.<path>`,
the root being the outermost module called; `ops.health_scope(name)` appends a name for launches a module issues for a child it
never calls (`UNetModel.out`, the autoencoders' `conv_in` / `conv_out`), and a block body that its owner calls as a method, not
through `module(...)`, is decorated with `ops.health_labelled` and carries its own path (the autoencoders' stream / trunk bodies).

Per element, by bit pattern (a = |x| as fp32, exact for both 16-bit types) -- `tensor_health_ref` is the definition in numpy,
include/mobi_engine.h (mobi_tensor_health) and DESIGN.md state it:
    nan          all exponent bits set, mantissa != 0          inf   all exponent bits set, mantissa == 0
    absmax       the largest a over the finite elements (0 without one)
    near         finite and a >= near_abs (fp32 compare)       subnormal   exponent bits zero, mantissa != 0
    headroom     dtype max / absmax (inf for an all-zero tensor)

`probe(attention=True)` looks inside the attention launches as well: every `ops.attention` launch is followed, on the same stream,
by one `mobi_attention_health` launch (csrc/attention_health.hip) that recomputes it from its own operands with the exact row
maximum as the shift and fp32 probabilities, into the probe's own record buffers (still ONE read-back, in `report()`):
    rep.attention              one AttentionRow per launch; rep.rows is what it is without the flag, seq for seq
    rep.attention_for(seq)     the AttentionRow of the launch whose own row is rep.rows[seq], or None
An AttentionRow says whether the operands were already bad (in_nonfinite), where the scores lie as exponents of two (e_max, e_min),
how far they rise behind the first 32 keys (rise_max; rows_rise_over counts the rows past RISE_LIMIT), and how far the production
result is from the exact one (err_max at err_row of worst_head, against ref_absmax; out_nonfinite).  `attention_health_ref` is the
definition in fp64 numpy (DESIGN.md 5a states it).  RISE_LIMIT only LABELS rows: it is what the comments of csrc/attention.hip
state for the first pass of attention_rows_kernel and does not claim to predict which branch that kernel takes.  `ctx_attention`
and `attention_bwd` launches are not probed.

`audit_weights` measures a model's parameters as they will be rounded to a storage type, `heavy_tailed_` is a deterministic
stand-in for trained weights, and `python -m mobi_amd.health` runs both on the model a config describes (see `main`).
"""
import argparse
import json
import math
import sys
import weakref
from dataclasses import dataclass, field, fields

import numpy as np
import torch

DTYPE_NAMES = {torch.float16: "fp16", torch.bfloat16: "bf16", torch.float32: "fp32"}
DTYPE_MAX = {"fp16": 65504.0, "bf16": 3.3895313892515355e38, "fp32": 3.4028234663852886e38}
# the smallest magnitude that rounds (to nearest even) to inf: max + half an ulp of max
OVERFLOW_FROM = {"fp16": 65520.0, "bf16": float(np.array([0x7f7f8000], dtype=np.uint32).view(np.float32)[0]), "fp32": math.inf}
# bits: (storage bits, mantissa bits)
_LAYOUT = {"fp16": (16, 10), "bf16": (16, 7), "fp32": (32, 23)}


def dtype_name(dtype):
    if isinstance(dtype, str):
        if dtype not in DTYPE_MAX:
            raise ValueError(f"unknown dtype {dtype!r}: fp16, bf16 or fp32")
        return dtype
    return DTYPE_NAMES[dtype]


def _bits(array_or_bits, name):
    """-> the bit patterns as uint16 / uint32, flat."""
    a = array_or_bits
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().contiguous()
        a = a.view(torch.int16 if a.element_size() == 2 else torch.int32).numpy() if a.is_floating_point() else a.numpy()
    a = np.ascontiguousarray(a)
    want = np.uint16 if _LAYOUT[name][0] == 16 else np.uint32
    if a.dtype.kind == "f":
        if a.dtype.itemsize != want().itemsize or name == "bf16":
            raise TypeError(f"a {a.dtype} array does not hold {name} values: pass the bit patterns")
        return a.view(want).reshape(-1)
    if a.dtype.itemsize != want().itemsize:
        raise TypeError(f"{name} bit patterns are {want.__name__}, got {a.dtype}")
    return a.view(want).reshape(-1)


def tensor_health_ref(array_or_bits, dtype, near_abs):
    """The definition of a health record in numpy, on bit patterns.  array_or_bits: a float16 / float32 array (or torch tensor of
    the dtype itself) or the patterns as uint16 / uint32 (bf16: always patterns, or a torch.bfloat16 tensor); dtype: "fp16",
    "bf16", "fp32" or the torch dtype.  -> {absmax_bits, absmax, inf, nan, near, subnormal}.  The slow path on a machine
    without a GPU."""
    name = dtype_name(dtype)
    bits = _bits(array_or_bits, name)
    width, mant = _LAYOUT[name]
    h = bits & bits.dtype.type((1 << (width - 1)) - 1)             # the magnitude pattern
    man = h & h.dtype.type((1 << mant) - 1)
    exp = h >> h.dtype.type(mant)
    exp_all = (1 << (width - 1 - mant)) - 1
    if name == "fp16":
        a = h.view(np.float16).astype(np.float32)                  # exact
    elif name == "bf16":
        a = (h.astype(np.uint32) << np.uint32(16)).view(np.float32)
    else:
        a = h.view(np.float32)
    nan = (exp == exp_all) & (man != 0)
    inf = (exp == exp_all) & (man == 0)
    finite = exp != exp_all
    abits = a.view(np.uint32)
    absmax_bits = int(abits[finite].max()) if finite.any() else 0
    with np.errstate(invalid="ignore"):
        near = finite & (a >= np.float32(near_abs))
    sub = (exp == 0) & (man != 0)
    return {"absmax_bits": absmax_bits, "absmax": float(np.array([absmax_bits], dtype=np.uint32).view(np.float32)[0]),
            "inf": int(inf.sum()), "nan": int(nan.sum()), "near": int(near.sum()), "subnormal": int(sub.sum())}


# --------------------------------------------------------------------------------------
# the attention probe: the definition and its rows
# --------------------------------------------------------------------------------------
LOG2E = 1.4426950408889634
# octaves a row's scores may rise above the maximum of its first 32 keys before the row is counted in rows_rise_over: the reach
# csrc/attention.hip's comments give the first pass of attention_rows_kernel, which keeps the first 32 keys' shift (2^-24 is the
# last fp16 probability that is not flushed, bf16 has fp32's exponent).  A label for rows, not a prediction of the kernel's branch.
RISE_LIMIT = {"fp16": 20.0, "bf16": 120.0}
_FLOAT_FIELDS = ("e_max", "e_min", "rise_max", "err_max")
ATTENTION_REF_DTYPE = np.dtype([("q_absmax_bits", "<u4"), ("k_absmax_bits", "<u4"), ("v_absmax_bits", "<u4"), ("in_nonfinite", "<i4"),
                                ("out_nonfinite", "<i4"), ("e_max", "<f8"), ("e_min", "<f8"), ("rise_max", "<f8"),
                                ("rows_rise_over", "<i4"), ("ref_absmax_bits", "<u4"), ("err_max", "<f8"), ("err_row", "<i4"),
                                ("ref_absmax", "<f8"), ("dot_abs_max", "<f8")])


def _f32_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def _bits_f32(b):
    return float(np.array([b], dtype=np.uint32).view(np.float32)[0])


def attention_health_ref(q, k, v, out, heads, scale, v_rows=False, q_log2_scaled=False, rise_limit=None, rises=False):
    """The definition of `mobi_attention_health`'s record in fp64 numpy.  q [n, tq, C], k [n, tk, C], v [n, tk, C] (v_rows) or
    V^T [n, C, tk], out [n, tq, C]: torch tensors of one 16-bit storage type, any device, any strides.  On the stored values,
    with cexp = 1 if q_log2_scaled else float32(scale) * log2(e) (the launch holds `scale` as fp32):
        e_ij = cexp * sum_c q_ic k_jc,   m_i = max_j e_ij,   f_i = max_{j < min(32, tk)} e_ij,   rise_i = m_i - f_i
        p_ij = 2^(e_ij - m_i),   l_i = sum_j p_ij,   o_i = sum_j p_ij v_j / l_i
    -> a structured array, one element per (image, head), image-major: the record's fields (floats as fp64; ref_absmax_bits
    is the pattern of ref_absmax rounded to fp32) plus ref_absmax and dot_abs_max = cexp * max_ij sum_c |q_ic k_jc| (what an
    fp32 dot-product error bound scales with).  rise_limit: RISE_LIMIT of the storage type by default.  With in_nonfinite > 0
    the fields behind the two counts are whatever numpy makes of the non-finite values: unspecified.  rises=True: also the
    rise of every row, [n * heads, tq]."""
    name = dtype_name(q.dtype)
    if rise_limit is None:
        rise_limit = RISE_LIMIT[name]
    f64 = lambda t: t.detach().cpu().double().numpy()
    qd, kd, od = f64(q), f64(k), f64(out)
    vd = f64(v) if v_rows else f64(v).transpose(0, 2, 1)
    n, tq, c = qd.shape
    tk, dh = kd.shape[1], c // heads
    cexp = 1.0 if q_log2_scaled else float(np.float32(scale)) * LOG2E
    rec = np.zeros(n * heads, dtype=ATTENTION_REF_DTYPE)
    all_rises = np.zeros((n * heads, tq))
    with np.errstate(all="ignore"):
        for i in range(n):
            for h in range(heads):
                r = rec[i * heads + h]
                sl = slice(h * dh, (h + 1) * dh)
                qh, kh, vh, oh = qd[i, :, sl], kd[i, :, sl], vd[i, :, sl], od[i, :, sl]
                for tag, x in (("q", qh), ("k", kh), ("v", vh)):
                    fin = np.isfinite(x)
                    r[tag + "_absmax_bits"] = _f32_bits(np.abs(x[fin]).max()) if fin.any() else 0
                    r["in_nonfinite"] += int((~fin).sum())
                e = cexp * (qh @ kh.T)
                m, f = e.max(1), e[:, :min(32, tk)].max(1)
                rise = m - f
                pr = np.exp2(e - m[:, None])
                o = (pr @ vh) / pr.sum(1)[:, None]
                fin = np.isfinite(oh)
                r["out_nonfinite"] = int((~fin).sum())
                r["e_max"], r["e_min"], r["rise_max"] = e.max(), e.min(), rise.max()
                r["rows_rise_over"] = int((rise > rise_limit).sum())
                r["ref_absmax"] = np.abs(o).max()
                r["ref_absmax_bits"] = _f32_bits(r["ref_absmax"])
                r["dot_abs_max"] = cexp * (np.abs(qh) @ np.abs(kh).T).max()
                if fin.any():
                    err = np.where(fin, np.abs(np.where(fin, oh, 0.0) - o), -1.0).max(1)
                    r["err_max"] = err.max()
                    r["err_row"] = int(np.argmax(err == err.max()))
                else:
                    r["err_max"], r["err_row"] = 0.0, -1
                all_rises[i * heads + h] = rise
    return (rec, all_rises) if rises else rec


@dataclass
class AttentionRow:
    """One probed `ops.attention` launch: the records of its heads merged (max / min / sum) and the records themselves."""
    seq: int                     # of the launch's own row in Report.rows
    module: str
    images: int
    heads: int
    tq: int
    tk: int
    dh: int
    dtype: str
    q_log2_scaled: bool
    rise_limit: float
    q_absmax: float
    k_absmax: float
    v_absmax: float
    in_nonfinite: int
    out_nonfinite: int
    e_max: float
    e_min: float
    rise_max: float
    rows_rise_over: int
    ref_absmax: float
    err_max: float
    err_row: int                 # in worst_head
    worst_head: tuple            # (image, head) of err_max
    per_head: np.ndarray = field(default=None, repr=False, compare=False)   # ops.ATTENTION_HEALTH_DTYPE, [images * heads], image-major
    kept: dict = field(default=None, repr=False, compare=False)             # keep=True: clones of q, k, v, out and the launch's arguments

    @staticmethod
    def from_records(seq, module, shape, dtype, q_log2_scaled, rise_limit, rec, kept=None):
        images, heads, tq, tk, dh = shape
        f32 = lambda bits: _bits_f32(int(bits.max()))
        # the head with the largest error; a head whose record is unspecified (nan) never wins against a number
        err = np.where(np.isnan(rec["err_max"]) | (rec["err_row"] < 0), -1.0, rec["err_max"])
        w = int(np.argmax(err))
        return AttentionRow(seq, module, images, heads, tq, tk, dh, dtype, bool(q_log2_scaled), float(rise_limit),
                            f32(rec["q_absmax_bits"]), f32(rec["k_absmax_bits"]), f32(rec["v_absmax_bits"]),
                            int(rec["in_nonfinite"].sum()), int(rec["out_nonfinite"].sum()), float(rec["e_max"].max()),
                            float(rec["e_min"].min()), float(rec["rise_max"].max()), int(rec["rows_rise_over"].sum()),
                            f32(rec["ref_absmax_bits"]), float(rec["err_max"][w]), int(rec["err_row"][w]), (w // heads, w % heads),
                            rec, kept)

    def head(self, image, head):
        return self.per_head[image * self.heads + head]

    def to_dict(self):
        d = {f.name: getattr(self, f.name) for f in fields(self) if f.name not in ("per_head", "kept")}
        d["worst_head"] = list(self.worst_head)
        d["per_head"] = [[r[name].item() for name in self.per_head.dtype.names] for r in self.per_head]
        return d

    @staticmethod
    def from_dict(d):
        from . import ops
        rec = np.zeros(len(d["per_head"]), dtype=ops.ATTENTION_HEALTH_DTYPE)
        for i, values in enumerate(d["per_head"]):
            rec[i] = tuple(values)
        return AttentionRow(**{**d, "worst_head": tuple(d["worst_head"]), "per_head": rec})

    @staticmethod
    def head_lines(rec, heads, order):
        lines = [f"{'img':>4} {'head':>4} {'q absmax':>10} {'k absmax':>10} {'v absmax':>10} {'in bad':>7} {'out bad':>8} {'e_max':>10} "
                 f"{'e_min':>10} {'rise_max':>9} {'over':>6} {'ref absmax':>10} {'err_max':>10} {'err_row':>7}"]
        for i in order:
            r = rec[i]
            tail = (f"{r['e_max']:>10.4g} {r['e_min']:>10.4g} {r['rise_max']:>9.4g} {r['rows_rise_over']:>6} "
                    f"{_bits_f32(r['ref_absmax_bits']):>10.4g} {r['err_max']:>10.4g} {r['err_row']:>7}") if r["in_nonfinite"] == 0 \
                else "operands non-finite"
            lines.append(f"{i // heads:>4} {i % heads:>4} {_bits_f32(r['q_absmax_bits']):>10.4g} {_bits_f32(r['k_absmax_bits']):>10.4g} "
                         f"{_bits_f32(r['v_absmax_bits']):>10.4g} {r['in_nonfinite']:>7} {r['out_nonfinite']:>8} {tail}")
        return "\n".join(lines)

    def worst_heads(self, k=4):
        """The k heads with the most non-finite results (then by error), printed in full."""
        err = np.where(np.isnan(self.per_head["err_max"]), np.inf, self.per_head["err_max"])
        order = sorted(range(len(self.per_head)), key=lambda i: (-int(self.per_head["out_nonfinite"][i]), -err[i], i))[:k]
        return self.head_lines(self.per_head, self.heads, order)


def _merge(records):
    """One row over several tensors (the sampler's x and pred_x0): the max and the sums."""
    out = dict(records[0])
    for r in records[1:]:
        out["absmax_bits"] = max(out["absmax_bits"], r["absmax_bits"])
        for k in ("inf", "nan", "near", "subnormal"):
            out[k] += r[k]
    out["absmax"] = float(np.array([out["absmax_bits"]], dtype=np.uint32).view(np.float32)[0])
    return out


@dataclass
class Row:
    seq: int
    module: str
    kind: str
    shape: tuple
    dtype: str
    absmax: float
    headroom: float
    inf: int
    nan: int
    near: int
    subnormal: int
    overflow: int = 0            # audit_weights only: elements of an fp32 master that round to inf in the audited storage type
    kept: list = field(default=None, repr=False, compare=False)     # keep=True: clones of the measured tensors

    @property
    def nonfinite(self):
        return self.inf + self.nan

    @staticmethod
    def from_record(seq, module, kind, shape, dtype, rec, range_of=None, overflow=0, kept=None):
        """range_of: the storage type whose maximum the headroom is taken against (the row's own by default)."""
        amax = rec["absmax"]
        return Row(seq, module, kind, tuple(shape), dtype, amax, DTYPE_MAX[range_of or dtype] / amax if amax > 0 else math.inf,
                   rec["inf"], rec["nan"], rec["near"], rec["subnormal"], overflow, kept)


class Report:
    def __init__(self, rows, near=0.5, attention=()):
        self.rows, self.near, self.attention = list(rows), near, list(attention)

    def attention_for(self, seq):
        """The AttentionRow of the launch whose own row is rows[seq] (probe(attention=True)), or None."""
        for a in self.attention:
            if a.seq == seq:
                return a
        return None

    def first_nonfinite(self):
        for r in self.rows:
            if r.nonfinite > 0:
                return r
        return None

    def worst(self, k=20):
        """The k rows with the least headroom (rows that hold inf or nan first, then by headroom; ties in launch order)."""
        return sorted(self.rows, key=lambda r: (r.nonfinite == 0, r.headroom, r.seq))[:k]

    def to_json(self):
        rows = []
        for r in self.rows:
            d = {f.name: getattr(r, f.name) for f in fields(r) if f.name != "kept"}
            d["shape"] = list(r.shape)
            rows.append(d)
        d = {"near": self.near, "rows": rows}
        if self.attention:
            d["attention"] = [a.to_dict() for a in self.attention]
        return json.dumps(d)

    @staticmethod
    def from_json(text):
        d = json.loads(text)
        return Report([Row(**{**r, "shape": tuple(r["shape"])}) for r in d["rows"]], d["near"],
                      [AttentionRow.from_dict(a) for a in d.get("attention", [])])

    @staticmethod
    def attention_table(rows):
        lines = [f"{'seq':>5} {'n x h':>7} {'tq x tk':>11} {'dh':>4} {'dtype':>5} {'in bad':>7} {'out bad':>8} {'e_max':>10} {'e_min':>10} "
                 f"{'rise_max':>9} {'over':>6} {'ref absmax':>10} {'err_max':>10} {'at (img, head, row)':>19}  module"]
        for a in rows:
            at = f"({a.worst_head[0]}, {a.worst_head[1]}, {a.err_row})"
            tail = (f"{a.e_max:>10.4g} {a.e_min:>10.4g} {a.rise_max:>9.4g} {a.rows_rise_over:>6} {a.ref_absmax:>10.4g} {a.err_max:>10.4g} "
                    f"{at:>19}") if a.in_nonfinite == 0 else f"{'operands non-finite':>79}"
            lines.append(f"{a.seq:>5} {f'{a.images}x{a.heads}':>7} {f'{a.tq}x{a.tk}':>11} {a.dh:>4} {a.dtype:>5} {a.in_nonfinite:>7} "
                         f"{a.out_nonfinite:>8} {tail}  {a.module}")
        return "\n".join(lines)

    @staticmethod
    def table(rows, extra=None):
        head = f"{'seq':>5} {'absmax':>11} {'headroom':>10} {'inf':>7} {'nan':>7} {'near':>8} {'subnorm':>8} {'dtype':>5}  kind / module / shape"
        if extra:
            head = head.replace("  kind", f" {extra[0]:>11}  kind")
        lines = [head]
        for r in rows:
            x = f" {extra[1].get(r.seq, float('nan')):>11.4g}" if extra else ""
            lines.append(f"{r.seq:>5} {r.absmax:>11.4g} {r.headroom:>10.4g} {r.inf:>7} {r.nan:>7} {r.near:>8} {r.subnormal:>8} "
                         f"{r.dtype:>5}{x}  {r.kind}  {r.module}  {list(r.shape)}")
        return "\n".join(lines)

    def summary(self):
        """Three lines: the size of the report, the row with the least headroom, the first non-finite row."""
        w = self.worst(1)
        bad = self.first_nonfinite()
        return "\n".join([
            f"numeric health: {len(self.rows)} rows, near = {self.near:g} of the dtype maximum",
            "least headroom: " + (f"{w[0].headroom:.4g} x (absmax {w[0].absmax:.4g} {w[0].dtype}) at #{w[0].seq} {w[0].kind} {w[0].module}"
                                  if w else "no rows"),
            "first non-finite: " + (f"#{bad.seq} {bad.kind} {bad.module} (inf {bad.inf}, nan {bad.nan})" if bad else "none")])

    def __str__(self):
        text = self.table(self.rows) + "\n" + self.summary()
        if self.attention:
            text += "\n" + self.attention_table(self.attention)
        return text


# --------------------------------------------------------------------------------------
# the probe
# --------------------------------------------------------------------------------------
_ACTIVE = [None]
_SLOTS = 4096          # records per device buffer; a probe adds buffers as it fills them


class _Scope:
    def __init__(self, probe, name):
        self.probe, self.name = probe, name

    def __enter__(self):
        self.probe._stack.append(self.name)
        return self

    def __exit__(self, *exc):
        self.probe._stack.pop()
        return False


class Probe:
    """The sink behind `ops._HEALTH` (see the module's documentation); made by `probe()`."""

    def __init__(self, near=0.5, keep=False, attention=False):
        self.near, self.keep, self.attention = float(near), bool(keep), bool(attention)
        self._att_pending = []    # (seq, module, (images, heads, tq, tk, dh), dtype, q_log2_scaled, rise limit, buffer index, first slot, kept)
        self._att_buffers, self._att_used = [], 0
        self._pending = []        # (module, kind, shapes, dtypes, buffer index, first slot, count, kept)
        self._buffers, self._used = [], _SLOTS
        self._stack, self._names = [], weakref.WeakKeyDictionary()  # module -> path (weak: a freed module's address may be reused)
        self._hooks = []
        self._report = None

    # -- labels
    def _name(self, module):
        """A module seen for the first time is a root: it and everything under it get `<its class>.<path>`."""
        if module not in self._names:
            root = type(module).__name__
            for name, m in module.named_modules():
                self._names.setdefault(m, root + ("." + name if name else ""))

    def _pre(self, module, args):
        self._name(module)
        self._stack.append(module)

    def _post(self, module, args, output):
        while self._stack:
            if self._stack.pop() is module:
                break

    def scope(self, name):
        """name: a string appended to the current path, or a module whose own path takes over (ops.health_labelled)."""
        if not isinstance(name, str):
            self._name(name)
        return _Scope(self, name)

    def label(self):
        tail = []
        for e in reversed(self._stack):
            if isinstance(e, str):
                tail.append(e)
            else:
                return ".".join([self._names[e]] + tail[::-1])
        return ".".join(tail[::-1])

    # -- the sink
    def measure(self, kind, *tensors, label=None):
        """One row over `tensors` (usually one), measured now on the current stream.  label: the module path to record instead of
        the current one (an ops.Deferred's producer, whose result a later GroupNorm sums and writes)."""
        from . import ops
        ts = []
        for t in tensors:
            if t is None or t.numel() == 0 or t.dtype not in DTYPE_NAMES:
                continue
            # a strided view (a channel slice, a row-chain destination inside a wider buffer) is measured through a dense copy: one
            # more launch and the view's bytes for the time of the measurement, under a probe only
            ts.append(t if t.is_contiguous() else t.contiguous())
        if not ts:
            return
        if self._used + len(ts) > _SLOTS:
            self._buffers.append(torch.empty((_SLOTS, 5), dtype=torch.int64, device=ts[0].device))
            self._used = 0
        buf = self._buffers[-1]
        ops.tensor_health(ts, self.near, out=buf[self._used:])
        kept = [t.clone() for t in ts] if self.keep else None
        self._pending.append((self.label() if label is None else label, kind, [tuple(t.shape) for t in ts], [DTYPE_NAMES[t.dtype] for t in ts],
                              len(self._buffers) - 1, self._used, len(ts), kept))
        self._used += len(ts)

    def measure_attention(self, q, k, v, out, heads, scale, v_rows, q_log2_scaled):
        """ops.attention calls this right behind `measure("attention", out)` when `attention` is set: one mobi_attention_health
        launch on the current stream into the probe's own record buffer, tied to the row just made."""
        from . import ops
        if not self._pending or out.numel() == 0:
            return
        count = q.shape[0] * heads
        if not self._att_buffers or self._att_used + count > self._att_buffers[-1].shape[0]:
            self._att_buffers.append(torch.empty((max(_SLOTS, count), ops.ATTENTION_HEALTH_DTYPE.itemsize // 4), dtype=torch.int32,
                                                 device=q.device))
            self._att_used = 0
        name = DTYPE_NAMES[q.dtype]
        ops.attention_health(q, k, v, out, heads, scale, v_rows, q_log2_scaled, RISE_LIMIT[name],
                             records=self._att_buffers[-1][self._att_used:])
        kept = dict(q=q.clone(), k=k.clone(), v=v.clone(), out=out.clone(), heads=heads, scale=scale, v_rows=v_rows,
                    q_log2_scaled=q_log2_scaled) if self.keep else None
        c = v.shape[2] if v_rows else v.shape[1]
        self._att_pending.append((len(self._pending) - 1, self._pending[-1][0], (q.shape[0], heads, q.shape[1], k.shape[1], c // heads),
                                  name, bool(q_log2_scaled), RISE_LIMIT[name], len(self._att_buffers) - 1, self._att_used, kept))
        self._att_used += count

    # -- context
    def __enter__(self):
        from . import ops
        if _ACTIVE[0] is not None or ops._HEALTH is not None:
            raise RuntimeError("health probes do not nest")
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("a health probe cannot start during stream capture")
        from torch.nn.modules import module as M
        self._hooks = [M.register_module_forward_pre_hook(self._pre), M.register_module_forward_hook(self._post, always_call=True)]
        _ACTIVE[0] = self
        ops.set_health(self)
        return self

    def __exit__(self, *exc):
        from . import ops
        ops.set_health(None)
        _ACTIVE[0] = None
        for h in self._hooks:
            h.remove()
        self._hooks, self._stack = [], []
        return False

    def report(self):
        """The rows so far; one copy of all records to the host."""
        from . import ops
        if self._report is not None and self._report[0] == len(self._pending):
            return self._report[1]
        rows = []
        if self._pending:
            used = [(_SLOTS if i + 1 < len(self._buffers) else self._used) for i in range(len(self._buffers))]
            allrec = ops.read_tensor_health(torch.cat([b[:u] for b, u in zip(self._buffers, used)]) if len(self._buffers) > 1
                                            else self._buffers[0][:used[0]])
            starts = np.concatenate([[0], np.cumsum(used)])
            for seq, (module, kind, shapes, dtypes, bi, slot, count, kept) in enumerate(self._pending):
                lo = int(starts[bi]) + slot
                rows.append(Row.from_record(seq, module, kind, shapes[0], dtypes[0], _merge(allrec[lo:lo + count]), kept=kept))
        att = []
        if self._att_pending:
            host = [ops.read_attention_health(b if i + 1 < len(self._att_buffers) else b[:self._att_used])
                    for i, b in enumerate(self._att_buffers)]
            for seq, module, shape, dtype, log2, limit, bi, slot, kept in self._att_pending:
                att.append(AttentionRow.from_records(seq, module, shape, dtype, log2, limit, host[bi][slot:slot + shape[0] * shape[1]].copy(),
                                                     kept))
        rep = Report(rows, self.near, att)
        self._report = (len(self._pending), rep)
        return rep


def probe(near=0.5, keep=False, attention=False):
    return Probe(near, keep, attention)


# --------------------------------------------------------------------------------------
# the weight audit
# --------------------------------------------------------------------------------------
def _sixteen_bit_tensors(value, out, seen):
    """Every 16-bit tensor inside a cached pack (ops.Packed and its kin, tuples, lists)."""
    if isinstance(value, torch.Tensor):
        if value.dtype in (torch.float16, torch.bfloat16) and id(value) not in seen:
            seen.add(id(value))
            out.append(value)
    elif isinstance(value, (tuple, list)):
        for v in value:
            _sixteen_bit_tensors(v, out, seen)
    elif hasattr(value, "__dict__") and not isinstance(value, torch.nn.Module):
        for v in vars(value).values():
            _sixteen_bit_tensors(v, out, seen)


def _measure_many(tensors, near_abs):
    """records of tensors on any device: the engine's launches for device tensors, the numpy definition otherwise."""
    from . import ops
    recs = [None] * len(tensors)
    dev = [i for i, t in enumerate(tensors) if t.is_cuda]
    if dev:
        got = ops.read_tensor_health(ops.tensor_health([tensors[i].detach().contiguous() for i in dev],
                                                       near_abs=[near_abs[i] for i in dev]))
        for i, r in zip(dev, got):
            recs[i] = r
    for i, t in enumerate(tensors):
        if recs[i] is None:
            recs[i] = tensor_health_ref(t.detach(), t.dtype, near_abs[i])
    return recs


def audit_weights(model, dtype=torch.float16, near=0.5):
    """One row per fp32 parameter and per packed 16-bit image that already exists (the modules' pack caches) -> a Report.
    A parameter is measured as it will be rounded to `dtype`: `near` counts its elements from near x the maximum of `dtype`,
    `overflow` those that round to inf, and the headroom is taken against the maximum of `dtype`; a 16-bit image is measured
    directly.  Answers "does any weight of this checkpoint leave the storage type's range" before anything runs."""
    name = dtype_name(dtype)
    entries = []                                                   # (module, kind, tensor, near_abs)
    for pname, p in model.named_parameters():
        if p.dtype == torch.float32 and p.numel() > 0:
            entries.append((pname, "param", p, near * DTYPE_MAX[name]))
    n_params = len(entries)
    seen = set()
    for mname, m in model.named_modules():
        for tag, hit in sorted(m.__dict__.get("_pack_cache", {}).items(), key=lambda kv: str(kv[0])):
            found = []
            _sixteen_bit_tensors(hit[1], found, seen)
            for k, t in enumerate(found):
                entries.append((f"{mname}[{tag}].{k}", "image", t, near * DTYPE_MAX[DTYPE_NAMES[t.dtype]]))
    # the overflow count of a parameter is the `near` of a second entry of the same tensor in the same launch list, with the
    # threshold from which a value rounds to inf
    counted = math.isfinite(OVERFLOW_FROM[name])
    extra = entries[:n_params] if counted else []
    recs = _measure_many([e[2] for e in entries + extra], [e[3] for e in entries] + [OVERFLOW_FROM[name]] * len(extra))
    over = [r["near"] for r in recs[len(entries):]] + [0] * (len(entries) - len(extra))
    recs = recs[:len(entries)]
    rows = [Row.from_record(i, e[0], e[1], e[2].shape, DTYPE_NAMES[e[2].dtype], r, range_of=name if e[1] == "param" else None,
                            overflow=over[i]) for i, (e, r) in enumerate(zip(entries, recs))]
    return Report(rows, near)


# --------------------------------------------------------------------------------------
# trained-like weights
# --------------------------------------------------------------------------------------
def outlier_channels(n_out, outlier_every=64):
    """The output channels `heavy_tailed_` multiplies by outlier_gain: outlier_every // 2 + k * outlier_every."""
    return list(range(outlier_every // 2, n_out, outlier_every))


def heavy_tailed_(module, seed, sigma=1.0, outlier_every=64, outlier_gain=30.0, norm_gamma_max=10.0):
    """Fills `module`'s parameters in place with a deterministic stand-in for trained weights (torch CPU generator streams):
      matrices / filters   N(0, 1 / fan_in), every output channel c times exp(sigma z_c - sigma^2 / 2) (log-normal, mean 1);
                           the channels `outlier_channels(n_out, outlier_every)` times outlier_gain on top
      LayerNorm / GroupNorm weights (1-D `weight` of a module whose class name holds "Norm")
                           norm_gamma_max ** u, u uniform in [0, 1): between 1 and norm_gamma_max
      other 1-D weights    1 + 0.1 z;      biases   0.05 z
    norm_gamma_max=None leaves the norm weights at 1 + 0.1 z (with sigma = 0 and outlier_gain = 1: the plain synthetic recipe).
    One generator seeded with `seed` walks named_parameters() in order: the same seed gives the same bits."""
    g = torch.Generator().manual_seed(int(seed))
    owners = {}
    for m in module.modules():
        for p in m.parameters(recurse=False):
            owners[id(p)] = m
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() >= 2:
                w = torch.randn(p.shape, generator=g) / math.sqrt(p[0].numel())
                scale = torch.exp(sigma * torch.randn(p.shape[0], generator=g) - 0.5 * sigma * sigma)
                scale[outlier_channels(p.shape[0], outlier_every)] *= outlier_gain
                p.copy_(w * scale.view(-1, *([1] * (p.dim() - 1))))
            elif norm_gamma_max is not None and name.endswith("weight") and "norm" in type(owners[id(p)]).__name__.lower():
                p.copy_(float(norm_gamma_max) ** torch.rand(p.shape, generator=g))
            elif name.endswith("weight"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.05 * torch.randn(p.shape, generator=g))
    return module


# --------------------------------------------------------------------------------------
# the command
# --------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m mobi_amd.health",
                                 description="Weight audit and a probed sampling run of a config's UNet; exit status 3 when a row holds inf or nan.")
    ap.add_argument("--config", type=str, required=True, help="the model's YAML config")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt", type=str, default="", help="checkpoint holding `state_dict`")
    src.add_argument("--synthetic", choices=("gauss", "heavy"), help="seeded weights: N(0, 1 / fan_in), or heavy_tailed_")
    ap.add_argument("--dtype", choices=("fp16", "bf16", "both"), default="fp16")
    ap.add_argument("--steps", type=int, default=2, help="sampler steps")
    ap.add_argument("--scale", type=float, default=5, help="classifier-free guidance scale")
    ap.add_argument("--plms", action="store_true", help="PLMS instead of DDIM")
    ap.add_argument("--objects", type=int, default=2)
    ap.add_argument("--top", type=int, default=20, help="rows of the worst-headroom table")
    ap.add_argument("--json", type=str, default="", help="write the reports here")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--attention", action="store_true", help="probe inside every attention launch as well (mobi_attention_health)")
    ap.add_argument("overrides", nargs=argparse.REMAINDER, help="dot-list overrides of the config")
    return ap


def gauss_(module, seed):
    """The plain synthetic weights (bench.py's recipe, as tools/_synth.py: N(0, 1 / fan_in) matrices, 1 + 0.1 z norm scales,
    0.05 z biases); `heavy_tailed_` is laid over the same distribution."""
    return heavy_tailed_(module, seed, sigma=0.0, outlier_gain=1.0, norm_gamma_max=None)


def synthetic_batch(objects, size, seed=0):
    """One seeded batch as the data side hands it to `get_input`, camera and lidar (uniform pictures with a square hole; no
    database): `size` = the pixel size of the pictures (8 x the latent)."""
    g = torch.Generator().manual_seed(int(seed))
    B, R = int(objects), int(size)
    u = lambda *shape: torch.rand(*shape, generator=g) * 2 - 1
    hole = torch.ones(B, 1, R, R)
    hole[:, :, R // 4: 3 * R // 4, R // 4: 3 * R // 4] = 0
    img, rng, ref = u(B, 3, R, R), u(B, 2, R, R), u(B, 3, 224, 224) * 1.5
    b = {"image": {"GT": img, "inpaint_image": img * hole, "inpaint_mask": hole.clone(),
                   "cond": {"ref_image": ref, "ref_bbox": torch.rand(B, 8, 3, generator=g)}},
         "lidar": {"range_data": rng, "range_data_inpaint": rng * hole, "range_mask": hole.clone(),
                   "range_instance_mask": (torch.rand(B, 1, R, R, generator=g) > 0.8).float() * (1 - hole),
                   "min_depth_obj": torch.linspace(-0.8, -0.2, B), "max_depth_obj": torch.linspace(0.1, 0.7, B),
                   "width_crop": torch.full((B,), R // 2, dtype=torch.long),
                   "cond": {"ref_image": ref.clone(), "ref_bbox": torch.rand(B, 8, 3, generator=g)}}}
    move = lambda d: {k: move(v) if isinstance(v, dict) else v.cuda() for k, v in d.items()}
    return move(b)


def probed_model_run(model, dtype, *, objects=2, steps=2, scale=5.0, plms=False, seed=0, near=0.5, keep=False, attention=False):
    """One synthetic batch through `get_input` -> `steps` sampler steps -> `decode_sample` + `log_data` of a LatentDiffusion model
    under a probe -> the Report: the conditioning producer, both autoencoders in encode and decode, the UNet and the sampler."""
    import mobi_amd
    from .ldm.models.diffusion.ddim import DDIMSampler
    from .ldm.models.diffusion.plms import PLMSSampler
    mobi_amd.set_engine_dtype(dtype)
    batch = synthetic_batch(objects, model.image_size * 8, seed)
    shape = [model.channels, model.image_size, model.image_size]
    sampler = (PLMSSampler if plms else DDIMSampler)(model)
    with torch.no_grad(), model.ema_scope(), probe(near=near, keep=keep, attention=attention) as hp:
        data = model.get_input(batch, model.first_stage_key, force_c_encode=True, return_vae_rec=True)
        n = data["z"].shape[0]
        x_T = torch.randn([n, *shape], generator=torch.Generator().manual_seed(int(seed) + 1)).cuda()
        uc = None
        if scale != 1.0:
            uc = [model.learnable_vector.repeat(n, 1, 1)]
            if "ref_bbox" in model.cond_stage_key:
                uc.append(model.bbox_uncond_vector.repeat(n, 1, 1))
            uc = torch.cat(uc, dim=1)
        common = dict(S=steps, conditioning=data["cond"], batch_size=n, shape=shape, verbose=False, x_T=x_T, eta=0.0,
                      unconditional_guidance_scale=scale, unconditional_conditioning=uc)
        if plms:
            samples, _ = sampler.sample(inpaint_image=data["z"][:, 4:8], inpaint_mask=data["z"][:, [8]], **common)
        else:
            samples, _ = sampler.sample(test_model_kwargs={"inpaint_image": data["z"][:, 4:8], "inpaint_mask": data["z"][:, [8]]},
                                        **common)
        h_camera, h_lidar = model.decode_sample(samples, data.get("z_lidar"))
        model.log_data(batch, data, h_camera, h_lidar, log_metrics=True, split="train")
    return hp.report()


class _FirstBatch:
    """Opens a probe at a model's first `get_input` and closes it when its first `log_data` returns: one test-bench batch
    (get_input, sampling, decode_sample, log_data) runs under the probe, eagerly, once; later batches run as always."""

    def __init__(self, model, near=0.5, attention=False):
        self.model, self.probe, self.report = model, Probe(near, attention=attention), None
        self._state = 0                                            # 0 not started, 1 probing, 2 done
        get_input, log_data = model.get_input, model.log_data

        def probed_get_input(*a, **k):
            if self._state == 0:
                self._state = 1
                self.probe.__enter__()
            return get_input(*a, **k)

        def probed_log_data(*a, **k):
            try:
                return log_data(*a, **k)
            finally:
                self.close()
        model.get_input, model.log_data = probed_get_input, probed_log_data      # (instance attributes over the class's methods)

    def close(self):
        if self._state == 1:
            self.probe.__exit__(None, None, None)
            self.report = self.probe.report()
        self._state = 2

    def remove(self):
        self.close()
        del self.model.get_input, self.model.log_data


def test_bench_main(argv=None):
    """`python -m mobi_amd.health test_bench <the arguments of python -m mobi_amd.test_bench>`: the test-bench command with its
    first batch under the probe.  Writes OUT/health.json beside the result tree and prints a three-line summary; every other file
    is byte-equal to what `python -m mobi_amd.test_bench` writes with the same arguments (the model is loaded where that command
    loads it, so every random draw falls where it fell).  Exit status 3 when a row holds inf or nan."""
    import os
    from . import set_engine_dtype, test_bench as tb
    from .ldm.util import load_config
    argv = sys.argv[2:] if argv is None else list(argv)
    attention = "--attention" in argv                              # the probe's own flag; the rest is the test bench's
    opt = tb.build_parser().parse_args([a for a in argv if a != "--attention"])
    if opt.plms and opt.dpm:
        raise SystemExit("--plms and --dpm exclude each other")
    set_engine_dtype({"fp16": torch.float16, "bf16": torch.bfloat16}[opt.dtype])
    tb.seed_everything(opt.seed)
    config = load_config(opt.config, [o for o in opt.overrides if o != "--"])
    load_model, first = tb.load_model, []

    def load_and_watch(cfg, ckpt):
        first.append(_FirstBatch(load_model(cfg, ckpt), attention=attention))
        return first[0].model

    tb.load_model = load_and_watch                                 # the loop loads its model through this name, after the split is built
    try:
        spent = tb.run(opt, config)
    finally:
        tb.load_model = load_model
        for f in first:
            f.remove()
    rep = first[0].report if first else None
    if rep is None:
        raise SystemExit("the test split is empty: nothing ran under the probe")
    with open(os.path.join(opt.outdir, "health.json"), "w") as f:
        f.write(rep.to_json())
    for name, laps in spent.items():                               # (--timing, as the test-bench command prints it)
        print(f"{name}: median {1e3 * float(np.median(laps)):.1f} ms over {len(laps)} batches")
    print(rep.summary())
    if attention:
        print(attention_section(rep))
    print(f"The result tree is in {opt.outdir}")
    return 3 if rep.first_nonfinite() is not None else 0


def attention_section(rep):
    """What `--attention` adds to the output: the attention table and, for the first launch whose production result holds inf or
    nan, its worst heads in full."""
    lines = [f"attention probe: {len(rep.attention)} launches", Report.attention_table(rep.attention)]
    bad = next((a for a in rep.attention if a.out_nonfinite > 0), None)
    if bad is not None:
        lines += [f"first attention launch with a non-finite result: #{bad.seq} {bad.module} ({bad.images} x {bad.heads} heads, "
                  f"{bad.tq} x {bad.tk}, dh {bad.dh}, {bad.dtype}, rise limit {bad.rise_limit:g}): its worst heads", bad.worst_heads()]
    else:
        lines.append("no attention launch stored inf or nan")
    return "\n".join(lines)


def main(argv=None):
    """Builds the config's model (UNet, both autoencoders, the conditioning producer), loads or fills its weights, audits every
    one of them and runs one seeded synthetic batch through get_input -> `--steps` sampler steps -> decode_sample + log_data under
    the probe.  `python -m mobi_amd.health test_bench ...` is `test_bench_main`."""
    argv = sys.argv[1:] if argv is None else list(argv)
    if argv and argv[0] == "test_bench":
        return test_bench_main(argv[1:])
    opt = build_parser().parse_args(argv)
    from .ldm.util import instantiate_from_config, load_config
    config = load_config(opt.config, [o for o in opt.overrides if o != "--"])
    model = instantiate_from_config(config["model"])
    if opt.ckpt:
        sd = torch.load(opt.ckpt, map_location="cpu")
        sd = sd.get("state_dict", sd)
        own = model.state_dict()
        missing, unexpected = model.load_state_dict(sd, strict=False)
        loaded = len(own) - len(missing)
        print(f"== checkpoint {opt.ckpt}: {loaded} of {len(own)} tensors loaded, {len(missing)} missing, {len(unexpected)} unexpected")
        for k in list(missing)[:10]:
            print(f"   missing    {k}")
        for k in list(unexpected)[:10]:
            print(f"   unexpected {k}")
        if loaded == 0:
            raise SystemExit("no tensor of the checkpoint matches the model: nothing to report on")
    elif opt.synthetic == "heavy":
        heavy_tailed_(model, opt.seed)
    else:
        gauss_(model, opt.seed)
    model = model.cuda().eval()
    names = ["fp16", "bf16"] if opt.dtype == "both" else [opt.dtype]
    torch_dt = {"fp16": torch.float16, "bf16": torch.bfloat16}
    out, bad = {}, False
    for name in names:
        audit = audit_weights(model, torch_dt[name])
        print(f"== weight audit, {name}: {len(audit.rows)} tensors")
        print(Report.table(audit.worst(min(opt.top, 5))))
        out[f"audit_{name}"] = json.loads(audit.to_json())
        bad |= any(r.nonfinite or r.overflow for r in audit.rows)
    reports = {name: probed_model_run(model, torch_dt[name], objects=opt.objects, steps=opt.steps, scale=opt.scale, plms=opt.plms,
                                      seed=opt.seed, attention=opt.attention) for name in names}
    first = reports[names[0]]
    extra = None
    if len(names) == 2:
        # the two runs need not have the same launches (the fp16 decoders run their fp32-stream paths): a row's partner is the
        # bf16 row with the same module, kind and shape at the same occurrence; a row without one prints nan
        def keyed(rows):
            seen = {}
            for r in rows:
                k = (r.module, r.kind, r.shape)
                seen[k] = seen.get(k, 0) + 1
                yield k + (seen[k],), r
        partner = {k: r.absmax for k, r in keyed(reports["bf16"].rows)}
        extra = ("bf16 absmax", {r.seq: partner[k] for k, r in keyed(first.rows) if k in partner})
    print(f"== probed run, {names[0]}: the {opt.top} rows with the least headroom")
    print(Report.table(first.worst(opt.top), extra))
    for name in names:
        print(f"-- {name}")
        print(reports[name].summary())
        if opt.attention:
            print(attention_section(reports[name]))
        out[f"run_{name}"] = json.loads(reports[name].to_json())
        bad |= reports[name].first_nonfinite() is not None
    if opt.json:
        with open(opt.json, "w") as f:
            json.dump(out, f)
    return 3 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
