"""The cases of tests/test_gpu_attention_health.py and the fp32 restatement of csrc/attention_health.hip that sets the test's
tolerance on `ref_absmax` and `err_max`.  Nothing here needs a GPU:

    python -m tests.attention_health_cases        # prints the restatement's worst error against fp64 and the tolerance

The selection covers, without being the full product: both storage types, dh in {8, 40, 64, 160} (one per instantiation of the
kernel: 16, 48, 80 and 160 padded channels), (tq, tk) in {(1, 1), (33, 31), (65, 100), (96, 257)} (one row; a ragged tile below
32 keys, where the rise is 0 by definition; more than one key tile; more than one wave's rows and a ragged fifth key tile), the
operand forms dense / stacked / partner, the V forms rows / vt / vt_ragged and q_log2_scaled 0 and 1, on 2 images x 2 heads."""
import functools

import numpy as np
import torch

from tests import attention_ref as AR

IMAGES, HEADS = 2, 2
DTYPES = (torch.float16, torch.bfloat16)
DHS = (8, 40, 64, 160)
SHAPES = ((1, 1), (33, 31), (65, 100), (96, 257))
FORMS = ("dense", "stacked", "partner")
V_FORMS = ("rows", "vt", "vt_ragged")
TILE = 64                                   # keys per tile of the kernel (kAhKeys)


def _cases():
    out, i = [], 0
    for dtype in DTYPES:
        for dh in DHS:
            for tq, tk in SHAPES:
                out.append((dtype, dh, tq, tk, FORMS[i % 3], V_FORMS[(i // 3) % 3], (i // 9 + i) % 2))
                i += 1
    for dtype in DTYPES:                    # pairs the walk above leaves out at the largest shapes
        out += [(dtype, 160, 96, 257, "stacked", "rows", 1), (dtype, 40, 96, 257, "partner", "vt_ragged", 1),
                (dtype, 8, 1, 1, "dense", "vt", 0), (dtype, 64, 65, 100, "stacked", "vt_ragged", 0)]
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = _cases()


def case_id(c):
    return f"{'fp16' if c[0] == torch.float16 else 'bf16'}-dh{c[1]}-{c[2]}x{c[3]}-{c[4]}-{c[5]}-log2{c[6]}"


@functools.lru_cache(maxsize=None)
def inputs(dtype, dh, tq, tk, log2):
    """(q, k, v) CPU tensors of the storage type, [n, t, C] (v as rows), and the scale of the launch."""
    q, k, v = AR.standard_inputs(IMAGES, HEADS, dh, tq, tk, dtype)
    if log2:
        q = AR.log2_scaled(q, dh, dtype)
    return q, k, v, dh ** -0.5


def restated32(q, k, v, heads, scale, q_log2_scaled):
    """The kernel's algorithm in fp32 numpy: fp32 scores, the running maximum raised once per tile of 64 keys, l and o rescaled
    by exp2(m_old - m_new), then p = exp2(e - m_new) added key by key in order.  q, k, v: [n, t, C] tensors (v as rows).
    -> o [n, heads, tq, dh] fp32."""
    f32 = lambda t: t.detach().cpu().float().numpy()
    qd, kd, vd = f32(q), f32(k), f32(v)
    n, tq, c = qd.shape
    tk, dh = kd.shape[1], c // heads
    cexp = np.float32(1.0) if q_log2_scaled else np.float32(scale) * np.float32(1.4426950408889634)
    out = np.zeros((n, heads, tq, dh), dtype=np.float32)
    for i in range(n):
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            e = (qd[i, :, sl] @ kd[i, :, sl].T) * cexp
            vh = vd[i, :, sl]
            m = np.full(tq, -np.inf, dtype=np.float32)
            l = np.zeros(tq, dtype=np.float32)
            o = np.zeros((tq, dh), dtype=np.float32)
            for k0 in range(0, tk, TILE):
                m_new = np.maximum(m, e[:, k0:k0 + TILE].max(1))
                alpha = np.exp2(m - m_new)
                l, o = l * alpha, o * alpha[:, None]
                for j in range(k0, min(tk, k0 + TILE)):
                    p = np.exp2(e[:, j] - m_new)
                    l = l + p
                    o = o + p[:, None] * vh[j][None, :]
                m = m_new
            out[i, h] = o / l[:, None]
    return out


def exact64(q, k, v, heads, scale, q_log2_scaled):
    """o of the definition in fp64, [n, heads, tq, dh]."""
    f64 = lambda t: t.detach().cpu().double().numpy()
    qd, kd, vd = f64(q), f64(k), f64(v)
    n, tq, c = qd.shape
    dh = c // heads
    cexp = 1.0 if q_log2_scaled else float(np.float32(scale)) * 1.4426950408889634
    out = np.zeros((n, heads, tq, dh))
    for i in range(n):
        for h in range(heads):
            sl = slice(h * dh, (h + 1) * dh)
            e = cexp * (qd[i, :, sl] @ kd[i, :, sl].T)
            p = np.exp2(e - e.max(1, keepdims=True))
            out[i, h] = (p @ vd[i, :, sl]) / p.sum(1, keepdims=True)
    return out


@functools.lru_cache(maxsize=None)
def measured_tolerance():
    """(the restatement's worst |o32 - o64| over the distinct inputs of CASES, 4 x that): the tolerance of the GPU test on
    ref_absmax and err_max.  The factor 4 is the kernel's freedom in summation order (the MFMA's inside a dot product, the
    block's over channels) and in exp2's last place."""
    worst = 0.0
    for key in sorted({(c[0], c[1], c[2], c[3], c[6]) for c in CASES}, key=str):
        q, k, v, scale = inputs(*key)
        worst = max(worst, float(np.abs(restated32(q, k, v, HEADS, scale, key[4]) - exact64(q, k, v, HEADS, scale, key[4])).max()))
    return worst, 4.0 * worst


if __name__ == "__main__":
    w, tol = measured_tolerance()
    print(f"{len(CASES)} cases; fp32 restatement against fp64: worst |o32 - o64| = {w:.6g}; tolerance (x 4) = {tol:.6g}")
