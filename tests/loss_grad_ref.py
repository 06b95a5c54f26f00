"""The contract of `mobi_loss_grad` (include/mobi_engine.h) restated in fp64 numpy / torch on the CPU: the reference the kernel's
tests compare against, itself pinned to the reference's own `p_losses` numbers (tests/golden/losses.npz) and to torch.autograd of
the reference's formula (tests/test_loss_grad_cpu.py)."""
import numpy as np
import torch

STORAGE_BITS = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}        # (mantissa bits, smallest normal exponent)


def clamp_t(t, table_len):
    """t outside [0, table_len) is clamped into it, as `mobi_q_sample` does."""
    return t.long().clamp(0, table_len - 1)


def coefficients(t, logvar, lvlb, loss_type, l_simple_weight, elbo_weight, loss_scale, numel):
    """k_i = fp32(loss_scale * g_i * (l2 ? 2 : 1) / numel), g_i = l_simple_weight * exp(-logvar[t_i]) + elbo_weight * lvlb[t_i]
    in fp64 from the fp32 table entries -> fp64 [N] holding fp32 values."""
    ti = clamp_t(t, logvar.numel())
    g = l_simple_weight * torch.exp(-logvar.float().double()[ti]) + elbo_weight * lvlb.float().double()[ti]
    k = loss_scale * g * (2.0 if loss_type == "l2" else 1.0) / numel
    return k.float().double()


def loss_grad_ref(eps, target, t, logvar, lvlb, loss_type="l2", l_simple_weight=1.0, elbo_weight=0.0, loss_scale=1.0):
    """eps, target: fp32 [N, C, H, W]; t: int64 [N]; logvar, lvlb: fp32 [T] -> (dy fp64 [N, C, H, W] BEFORE the rounding to the
    storage type, per_sample fp64 [N], terms fp64 [3] = {mean loss_simple, loss_vlb, loss})."""
    assert loss_type in ("l2", "l1") and eps.dtype == target.dtype == torch.float32
    n = eps.shape[0]
    k = coefficients(t, logvar, lvlb, loss_type, l_simple_weight, elbo_weight, loss_scale, eps.numel()).view(n, 1, 1, 1)
    e, g = eps.double(), target.double()
    d32 = eps - target                                                       # every element is formed in fp32 ...
    if loss_type == "l2":
        dy = k * e + (-k) * g
        elem = (d32 * d32).double()
    else:
        dy = torch.where(eps > target, k, torch.where(eps < target, -k, torch.zeros_like(k))).expand_as(e).clone()
        dy[torch.isnan(d32)] = float("nan")
        elem = d32.abs().double()
    per_sample = elem.sum(dim=(1, 2, 3)) / (eps[0].numel())                  # ... and summed in fp64
    ti = clamp_t(t, logvar.numel())
    lv, w = logvar.float().double()[ti], lvlb.float().double()[ti]
    simple = per_sample.mean()
    vlb = (w * per_sample).mean()
    loss = l_simple_weight * (per_sample * torch.exp(-lv) + lv).mean() + elbo_weight * vlb
    return dy, per_sample, torch.stack([simple, vlb, loss])


def to_storage(dy, dtype, c_pad=32):
    """fp64 [N, C, H, W] -> the kernel's layout: `dtype` [N, H, W, c_pad], one rounding, channels >= C zero."""
    n, c, h, w = dy.shape
    out = torch.zeros((n, h, w, c_pad), dtype=dtype)
    out[..., :c] = dy.permute(0, 2, 3, 1).to(dtype)
    return out


def storage_ulp(x, dtype):
    """The spacing of `dtype` at |x| (fp64 tensor), subnormal spacing below the smallest normal."""
    mant, emin = STORAGE_BITS[dtype]
    ax = x.abs().double().numpy()
    e = np.floor(np.log2(np.where(ax > 0, ax, 1.0)))
    e = np.where(ax > 0, np.maximum(e, emin), emin)
    return torch.from_numpy(np.exp2(e - mant))


def reference_formula(eps, target, t, logvar, lvlb, loss_type, l_simple_weight, elbo_weight):
    """ddpm.py:1189-1216 of the reference written out on whatever dtype `eps` has (differentiable): -> (loss_simple [N], dict)."""
    d = target - eps
    loss_simple = (d.abs() if loss_type == "l1" else d * d).mean([1, 2, 3])
    ti = clamp_t(t, logvar.numel())
    logvar_t = logvar.to(eps.dtype)[ti]
    loss_vlb = (lvlb.to(eps.dtype)[ti] * loss_simple).mean()
    loss = l_simple_weight * (loss_simple / torch.exp(logvar_t) + logvar_t).mean() + elbo_weight * loss_vlb
    return loss_simple, {"loss_simple": loss_simple.mean(), "loss_vlb": loss_vlb, "loss": loss}
