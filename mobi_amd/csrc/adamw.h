// The AdamW update of one element (torch.optim.AdamW's update, ddpm.py:1649 of the reference), shared by the per-tensor kernel
// (backward.hip: mobi_adamw_step) and the multi-tensor kernel (multi_tensor.hip: mobi_adamw_multi):
//   p *= 1 - lr wd;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)
// Which products the compiler fuses into an FMA depends on the code around an expression, so the fusions are spelled out here and
// contraction is off for the rest: both kernels perform the SAME sequence of fp32 operations, bit for bit -- the one
// mobi_adamw_step has performed since it was written (1 - lr wd and the first moment fused, the second moment and the final
// subtraction not).
#pragma once
#include "common.h"

namespace mobi {

__device__ __forceinline__ void adamw_update(float& p, const float gi, float& m, float& v, float lr, float b1, float b2, float eps,
                                             float wd, float bc1, float bc2_sqrt) {
#pragma clang fp contract(off)
  float pi = p * __builtin_fmaf(-lr, wd, 1.0f);
  const float mi = __builtin_fmaf(1.0f - b1, gi, b1 * m);
  const float vi = b2 * v + ((1.0f - b2) * gi) * gi;
  m = mi;
  v = vi;
  pi -= ((lr / bc1) * mi) / (sqrtf(vi) / bc2_sqrt + eps);
  p = pi;
}

}  // namespace mobi
