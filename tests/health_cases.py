"""Shared by tests/test_health_cpu.py and tests/test_gpu_health.py: the special bit patterns of the three storage types and the
torch restatement of a health row on a kept clone."""
import numpy as np
import torch

# (storage bits, mantissa bits, numpy pattern type)
LAYOUT = {"fp16": (16, 10, np.uint16), "bf16": (16, 7, np.uint16), "fp32": (32, 23, np.uint32)}
TORCH = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
MAX = {"fp16": 65504.0, "bf16": 3.3895313892515355e38, "fp32": 3.4028234663852886e38}


def patterns(name):
    """The magnitude patterns of the special values of a format."""
    width, mant, _ = LAYOUT[name]
    inf = ((1 << (width - 1 - mant)) - 1) << mant
    return {"inf": inf, "nan_a": inf | 1, "nan_b": inf | (1 << (mant - 1)) | 5, "max": inf - 1, "sub_min": 1,
            "sub_max": (1 << mant) - 1, "min_normal": 1 << mant, "zero": 0, "sign": 1 << (width - 1)}


def value_of(name, pattern):
    """The fp32 value of a magnitude pattern (exact)."""
    _, _, ut = LAYOUT[name]
    p = np.array([pattern], dtype=ut)
    if name == "fp16":
        return np.float32(p.view(np.float16)[0])
    if name == "bf16":
        return (p.astype(np.uint32) << np.uint32(16)).view(np.float32)[0]
    return p.view(np.float32)[0]


def specials(name, near_pattern):
    """[(label, pattern with sign)] : +-inf, two nan payloads, +-max, a value exactly at the near threshold and one ulp below,
    the smallest and largest subnormal, +-0."""
    p = patterns(name)
    s = p["sign"]
    return [("+inf", p["inf"]), ("-inf", p["inf"] | s), ("nan_a", p["nan_a"]), ("nan_b", p["nan_b"] | s), ("+max", p["max"]),
            ("-max", p["max"] | s), ("at_near", near_pattern), ("below_near", near_pattern - 1), ("sub_min", p["sub_min"]),
            ("sub_max", p["sub_max"] | s), ("+0", 0), ("-0", s)]


def torch_from_bits(name, bits):
    """numpy patterns -> a torch CPU tensor of the storage type."""
    bits = np.ascontiguousarray(bits)
    signed = bits.view(np.int16 if bits.dtype.itemsize == 2 else np.int32)
    return torch.from_numpy(signed.copy()).view(TORCH[name])


def torch_row(kept, near):
    """What torch computes on the kept clones of a row: (absmax, inf, nan, near, subnormal).  Float arithmetic in fp32 on the host
    (|x| of a 16-bit value is exact in fp32); the subnormal test is on magnitudes: 0 < |x| < the smallest normal."""
    amax, n_inf, n_nan, n_near, n_sub = 0.0, 0, 0, 0, 0
    for t in kept:
        tiny = torch.finfo(t.dtype).tiny
        thr = np.float32(near * MAX[{torch.float16: "fp16", torch.bfloat16: "bf16", torch.float32: "fp32"}[t.dtype]])
        a = t.detach().cpu().float().abs().reshape(-1)
        finite = torch.isfinite(a)
        if bool(finite.any()):
            amax = max(amax, float(a[finite].max()))
        n_inf += int(torch.isinf(a).sum())
        n_nan += int(torch.isnan(a).sum())
        n_near += int((finite & (a >= float(thr))).sum())
        n_sub += int(((a > 0) & (a < tiny)).sum())
    return amax, n_inf, n_nan, n_near, n_sub


def assert_rows_match_torch(report):
    assert len(report.rows) > 0
    for r in report.rows:
        assert r.kept, r
        want = torch_row(r.kept, report.near)
        assert (r.absmax, r.inf, r.nan, r.near, r.subnormal) == want, (r.seq, r.kind, r.module, want)
