// Where the training loss meets the network (include/mobi_engine.h, mobi_loss_grad; mobi_amd/train.py loss_and_gradients): the
// three loss terms of p_losses (ddpm.py:1189-1216 of the reference) and the gradient that enters unet_backward, in the layout its
// first launch reads, from ONE pass over eps and target.  About 1 MB moves at the production shapes: what the launch buys is
// launches and a host sync removed and one arithmetic definition, not bandwidth.  One thread per pixel: a wave reads 64
// consecutive floats of a channel plane (coalesced), and writes its pixel's c_pad * 2-byte row with 16-byte stores.  Blocks never
// straddle samples (grid = blocks per sample x batch); every block writes one fp64 partial, the one-block finish pass adds a
// sample's partials in ascending order and the samples in ascending order: no atomics, two runs are bit-equal.
// This file is compiled with -ffp-contract=off (mobi_amd/build.py), as sampler_ops.hip is: the l2 gradient is lincomb4_kernel's
// expression, product and sum each rounded to fp32.
#include "common.h"

namespace mobi {

constexpr int kLossBlock = 256;

// t[b] clamped into the tables, as q_sample_kernel does (torch's indexing would raise; never read out of range)
__device__ __forceinline__ long long loss_table_index(const long long* __restrict__ t, int b, int table_len) {
  const long long ti = t[b];
  return ti < 0 ? 0 : (ti >= table_len ? table_len - 1 : ti);
}

template <typename T>
__global__ __launch_bounds__(kLossBlock) void loss_grad_kernel(const mobi_loss_grad_params a) {
  __shared__ double wave_part[kLossBlock / 64];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int p = blockIdx.x * kLossBlock + tid;
  const bool live = p < a.hw;
  const long long ti = loss_table_index(reinterpret_cast<const long long*>(a.t), b, a.table_len);
  const double g = a.l_simple_weight * exp(-(double)a.logvar[ti]) + a.elbo_weight * (double)a.lvlb[ti];
  const double numel = (double)a.batch * (double)a.channels * (double)a.hw;
  const bool l2 = a.loss_type == MOBI_LOSS_L2;
  const float k = (float)(a.loss_scale * g * (l2 ? 2.0 : 1.0) / numel), nk = -k;
  const float* __restrict__ e = a.eps + (long long)b * a.channels * a.hw + p;
  const float* __restrict__ tg = a.target + (long long)b * a.channels * a.hw + p;
  T* __restrict__ row = static_cast<T*>(a.dy) + ((long long)b * a.hw + p) * a.c_pad;
  double sum = 0.0;
  if (live) {
    for (int v = 0; v < (a.c_pad >> 3); ++v) {
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = v * 8 + j;
        float val = 0.f;
        if (c < a.channels) {
          const float x = e[(long long)c * a.hw], y = tg[(long long)c * a.hw];
          const float d = x - y;
          if (l2) {
            val = k * x;
            val += nk * y;
            sum += (double)(d * d);
          } else {
            val = x > y ? k : (x < y ? nk : (x == y ? 0.f : d));      // (unordered: d is the NaN)
            sum += (double)fabsf(d);
          }
        }
        f[j] = val;
      }
      st16(row + v * 8, pack8<T>(f));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if ((tid & 63) == 0) wave_part[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) a.workspace[(long long)b * gridDim.x + blockIdx.x] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

// one block: thread i takes sample base + i (its partials in ascending order), thread 0 adds the samples in ascending order
__global__ __launch_bounds__(kLossBlock) void loss_grad_finish_kernel(const mobi_loss_grad_params a, int blocks_per_sample) {
  __shared__ double s_simple[kLossBlock], s_vlb[kLossBlock], s_weighted[kLossBlock];
  const int tid = threadIdx.x;
  const double per = (double)a.channels * (double)a.hw;
  double simple = 0.0, vlb = 0.0, weighted = 0.0;          // (thread 0's running sums)
  for (int base = 0; base < a.batch; base += kLossBlock) {
    const int i = base + tid;
    if (i < a.batch) {
      const double* __restrict__ part = a.workspace + (long long)i * blocks_per_sample;
      double s = 0.0;
      for (int j = 0; j < blocks_per_sample; ++j) s += part[j];
      const double ls = s / per;
      const long long ti = loss_table_index(reinterpret_cast<const long long*>(a.t), i, a.table_len);
      const double lv = (double)a.logvar[ti];
      a.per_sample[i] = (float)ls;
      s_simple[tid] = ls;
      s_vlb[tid] = (double)a.lvlb[ti] * ls;
      s_weighted[tid] = ls * exp(-lv) + lv;
    }
    __syncthreads();
    if (tid == 0) {
      const int n = a.batch - base < kLossBlock ? a.batch - base : kLossBlock;
      for (int j = 0; j < n; ++j) {
        simple += s_simple[j];
        vlb += s_vlb[j];
        weighted += s_weighted[j];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double n = (double)a.batch, loss_vlb = vlb / n;
    a.terms[0] = (float)(simple / n);
    a.terms[1] = (float)loss_vlb;
    a.terms[2] = (float)(a.l_simple_weight * (weighted / n) + a.elbo_weight * loss_vlb);
  }
}

}  // namespace mobi

using namespace mobi;
#define ST(stream) reinterpret_cast<hipStream_t>(stream)

extern "C" int32_t mobi_loss_grad_blocks_per_sample(int32_t hw) { return hw <= 0 ? 0 : (hw + kLossBlock - 1) / kLossBlock; }

extern "C" int mobi_loss_grad(const mobi_loss_grad_params* p, void* stream) {
  if (!p || !p->eps || !p->target || !p->t || !p->logvar || !p->lvlb || !p->dy || !p->per_sample || !p->terms || !p->workspace)
    return MOBI_ERR_ARG;
  if (p->batch <= 0 || p->channels <= 0 || p->hw <= 0 || p->table_len <= 0 || p->c_pad <= 0) return MOBI_ERR_ARG;
  if (p->dtype != MOBI_F16 && p->dtype != MOBI_BF16) return MOBI_ERR_ARG;
  if (p->channels > p->c_pad || (p->c_pad & 7) || p->batch > 65535) return MOBI_ERR_UNSUPPORTED;
  if (p->loss_type != MOBI_LOSS_L2 && p->loss_type != MOBI_LOSS_L1) return MOBI_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(p->dy) & 15) || (reinterpret_cast<uintptr_t>(p->workspace) & 7)) return MOBI_ERR_ALIGN;
  const int bps = mobi_loss_grad_blocks_per_sample(p->hw);
  const dim3 grid((unsigned)bps, (unsigned)p->batch);
  if (p->dtype == MOBI_F16) hipLaunchKernelGGL((loss_grad_kernel<f16_t>), grid, dim3(kLossBlock), 0, ST(stream), *p);
  else hipLaunchKernelGGL((loss_grad_kernel<bf16_t>), grid, dim3(kLossBlock), 0, ST(stream), *p);
  MOBI_CHECK_LAUNCH();
  hipLaunchKernelGGL(loss_grad_finish_kernel, dim3(1), dim3(kLossBlock), 0, ST(stream), *p, bps);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}
