// Numeric health of up to 64 dense tensors in one launch (include/mobi_engine.h, mobi_tensor_health; mobi_amd/health.py holds the
// numpy definition): per tensor the largest finite magnitude as fp32 bits and exact counts of inf, nan, "near the ceiling" and
// subnormal elements.  Read only, pure streaming.
//
// Everything is decided on the MAGNITUDE PATTERN h = the element's bits without the sign.  For an IEEE-style format the finite
// magnitudes are ordered as their patterns are, INF = the pattern with all exponent bits set and a zero mantissa, so
//   nan  h > INF      inf  h == INF      subnormal  0 < h < MINNORM      finite  h < INF
// and the largest finite magnitude is the largest finite pattern: the kernel keeps a max of patterns and converts it to fp32
// bits once, at the flush.  "a >= near_abs as an fp32 compare" becomes h >= near_h with near_h = the smallest pattern whose
// fp32 value is >= near_abs (INF if no finite one is): the host finds it, exactly, per tensor.  A thread counts
// #(h >= near_h), #(h >= INF), #(h > INF) and the subnormals; near = the first minus the second, inf = the second minus the third.
//
// The host cuts every tensor into blocks of `per_block` elements (one figure for the launch, a multiple of 8192, sized so that
// the grid is about eight blocks a CU) and passes the running block count as a prefix array in the argument block beside the
// table; a block finds its tensor by a binary search of the prefix.  Every block of a tensor starts at a multiple of 8192 elements,
// so all of them have the tensor's alignment phase: element loads in front of the first 16-byte boundary and behind the last,
// 16-byte loads between them.  Every wave adds its lanes up and lane 0 issues one vector atomic per field that is not zero.
#include "common.h"

namespace mobi {

constexpr int kHealthBlock = 256;
constexpr int kHealthMax = MOBI_HEALTH_MAX_TENSORS;
constexpr long long kHealthGrain = 8192;               // per_block is a multiple of it
constexpr long long kHealthMaxPerBlock = 1LL << 30;    // a thread's 32-bit counts hold per_block / 256, a wave's sum 64 of them
constexpr int kHealthBlocksPerCu = 8;

struct health_entry {
  const void* x;
  long long n;
  uint32_t near_h;                                     // smallest magnitude pattern that counts as near (<= INF)
  int32_t dtype;
};
struct health_args {
  health_entry t[kHealthMax];
  uint32_t first_block[kHealthMax + 1];                // tensor i owns blocks [first_block[i], first_block[i + 1])
  long long per_block;
  int32_t n_tensors;
};

struct health_acc {
  uint32_t m = 0, ge_near = 0, ge_inf = 0, gt_inf = 0, sub = 0;
};

template <uint32_t INF, uint32_t MINNORM>
__device__ __forceinline__ void health_one(uint32_t h, uint32_t near_h, health_acc& a) {
  a.ge_near += h >= near_h;
  a.ge_inf += h >= INF;
  a.gt_inf += h > INF;
  a.sub += (h - 1u) < (MINNORM - 1u);
  const uint32_t f = h < INF ? h : 0u;
  a.m = f > a.m ? f : a.m;
}

// 16-bit storage: x is 2-byte aligned
template <uint32_t INF, uint32_t MINNORM>
__device__ __forceinline__ void health_block16(const uint16_t* __restrict__ x, int len, uint32_t near_h, health_acc& a) {
  const int tid = threadIdx.x;
  const int ph = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) >> 1;
  const int head = ph < len ? ph : len;
  const int nvec = (len - head) >> 3, tail0 = head + (nvec << 3);
  if (tid < head) health_one<INF, MINNORM>(x[tid] & 0x7fffu, near_h, a);
  if (tid < len - tail0) health_one<INF, MINNORM>(x[tail0 + tid] & 0x7fffu, near_h, a);
  const u32x4* __restrict__ xv = reinterpret_cast<const u32x4*>(x + head);
#pragma unroll 4
  for (int i = tid; i < nvec; i += kHealthBlock) {
    const u32x4 q = xv[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      health_one<INF, MINNORM>(q[j] & 0x7fffu, near_h, a);
      health_one<INF, MINNORM>((q[j] >> 16) & 0x7fffu, near_h, a);
    }
  }
}

// fp32: x is 4-byte aligned
__device__ __forceinline__ void health_block32(const uint32_t* __restrict__ x, int len, uint32_t near_h, health_acc& a) {
  constexpr uint32_t INF = 0x7f800000u, MINNORM = 0x00800000u;
  const int tid = threadIdx.x;
  const int ph = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) >> 2;
  const int head = ph < len ? ph : len;
  const int nvec = (len - head) >> 2, tail0 = head + (nvec << 2);
  if (tid < head) health_one<INF, MINNORM>(x[tid] & 0x7fffffffu, near_h, a);
  if (tid < len - tail0) health_one<INF, MINNORM>(x[tail0 + tid] & 0x7fffffffu, near_h, a);
  const u32x4* __restrict__ xv = reinterpret_cast<const u32x4*>(x + head);
#pragma unroll 4
  for (int i = tid; i < nvec; i += kHealthBlock) {
    const u32x4 q = xv[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) health_one<INF, MINNORM>(q[j] & 0x7fffffffu, near_h, a);
  }
}

// the fp32 bit pattern of a finite fp16 magnitude pattern (exact: a subnormal is mantissa * 2^-24)
__host__ __device__ inline uint32_t health_f16_to_f32_bits(uint32_t h) {
  if (h >= 0x0400u) return (h << 13) + 0x38000000u;
  const float v = (float)h * 5.9604644775390625e-08f;
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  return u;
}

__global__ __launch_bounds__(kHealthBlock) void tensor_health_kernel(const health_args a, mobi_health_record* __restrict__ out) {
  // the tensor of this block: the last i with first_block[i] <= blockIdx.x (uniform: scalar loads from the argument block)
  const uint32_t b = blockIdx.x;
  int lo = 0, hi = a.n_tensors;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.first_block[mid] <= b) lo = mid; else hi = mid;
  }
  if (b >= a.first_block[a.n_tensors]) return;
  const health_entry t = a.t[lo];
  const long long off = (long long)(b - a.first_block[lo]) * a.per_block;
  if (off >= t.n) return;
  const long long left = t.n - off;
  const int len = (int)(left < a.per_block ? left : a.per_block);
  health_acc acc;
  uint32_t m32;
  if (t.dtype == MOBI_F16) {
    health_block16<0x7c00u, 0x0400u>(reinterpret_cast<const uint16_t*>(t.x) + off, len, t.near_h, acc);
    m32 = health_f16_to_f32_bits(acc.m);
  } else if (t.dtype == MOBI_BF16) {
    health_block16<0x7f80u, 0x0080u>(reinterpret_cast<const uint16_t*>(t.x) + off, len, t.near_h, acc);
    m32 = acc.m << 16;
  } else {
    health_block32(reinterpret_cast<const uint32_t*>(t.x) + off, len, t.near_h, acc);
    m32 = acc.m;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t mo = (uint32_t)__shfl_xor((int)m32, o, 64);
    m32 = mo > m32 ? mo : m32;
    acc.ge_near += (uint32_t)__shfl_xor((int)acc.ge_near, o, 64);
    acc.ge_inf += (uint32_t)__shfl_xor((int)acc.ge_inf, o, 64);
    acc.gt_inf += (uint32_t)__shfl_xor((int)acc.gt_inf, o, 64);
    acc.sub += (uint32_t)__shfl_xor((int)acc.sub, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    mobi_health_record* r = out + lo;
    const uint32_t n_inf = acc.ge_inf - acc.gt_inf, n_near = acc.ge_near - acc.ge_inf;
    if (m32) atomicMax(&r->absmax_bits, m32);
    if (n_inf) atomicAdd(reinterpret_cast<unsigned long long*>(&r->inf), (unsigned long long)n_inf);
    if (acc.gt_inf) atomicAdd(reinterpret_cast<unsigned long long*>(&r->nan), (unsigned long long)acc.gt_inf);
    if (n_near) atomicAdd(reinterpret_cast<unsigned long long*>(&r->near), (unsigned long long)n_near);
    if (acc.sub) atomicAdd(reinterpret_cast<unsigned long long*>(&r->subnormal), (unsigned long long)acc.sub);
  }
}

static inline uint32_t f32_bits(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  return u;
}

// the smallest magnitude pattern of `dtype` whose fp32 value is >= near_abs (near_abs >= 0, not nan); INF where no finite one is
static uint32_t health_near_pattern(int dtype, float near_abs) {
  const uint32_t nb = f32_bits(near_abs) & 0x7fffffffu;                         // (-0 counts as 0)
  if (dtype == MOBI_F32) return nb < 0x7f800000u ? nb : 0x7f800000u;
  if (dtype == MOBI_BF16) {
    const uint32_t p = (nb >> 16) + ((nb & 0xffffu) ? 1u : 0u);                 // round up to a pattern of 16 bits
    return p < 0x7f80u ? p : 0x7f80u;
  }
  uint32_t lo = 0, hi = 0x7c00u;                                                // fp16: patterns and fp32 bits are both monotone
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (health_f16_to_f32_bits(mid) >= nb) hi = mid; else lo = mid + 1;
  }
  return lo;
}

static int health_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus = n;
  }
  return cus;
}

}  // namespace mobi

using namespace mobi;
#define ST(stream) reinterpret_cast<hipStream_t>(stream)

extern "C" int mobi_tensor_health(const mobi_health_tensor* tensors, int32_t n_tensors, mobi_health_record* out, void* stream) {
  if (!tensors || !out || n_tensors <= 0 || n_tensors > kHealthMax) return MOBI_ERR_ARG;
  double total = 0.0;
  for (int i = 0; i < n_tensors; ++i) {
    const mobi_health_tensor& t = tensors[i];
    if (!t.x || t.n <= 0) return MOBI_ERR_ARG;
    if (t.dtype != MOBI_F16 && t.dtype != MOBI_BF16 && t.dtype != MOBI_F32) return MOBI_ERR_ARG;
    if (!(t.near_abs >= 0.0f)) return MOBI_ERR_ARG;                             // negative or nan
    total += (double)t.n;
  }
  for (int i = 0; i < n_tensors; ++i)
    if (reinterpret_cast<uintptr_t>(tensors[i].x) & (tensors[i].dtype == MOBI_F32 ? 3u : 1u)) return MOBI_ERR_ALIGN;
  if (reinterpret_cast<uintptr_t>(out) & 7) return MOBI_ERR_ALIGN;

  health_args a = {};
  const double want = total / (double)(health_cus() * kHealthBlocksPerCu);
  long long per_block = want >= (double)kHealthMaxPerBlock ? kHealthMaxPerBlock
                                                           : (((long long)want + kHealthGrain) / kHealthGrain) * kHealthGrain;
  if (per_block > kHealthMaxPerBlock) per_block = kHealthMaxPerBlock;
  a.per_block = per_block;
  a.n_tensors = n_tensors;
  long long blocks = 0;
  for (int i = 0; i < n_tensors; ++i) {
    a.t[i] = {tensors[i].x, (long long)tensors[i].n, health_near_pattern(tensors[i].dtype, tensors[i].near_abs), tensors[i].dtype};
    a.first_block[i] = (uint32_t)blocks;
    blocks += (tensors[i].n - 1) / per_block + 1;
    if (blocks > 0x7fffffffLL) return MOBI_ERR_UNSUPPORTED;                     // (beyond 2^61 elements)
  }
  for (int i = n_tensors; i <= kHealthMax; ++i) a.first_block[i] = (uint32_t)blocks;
  if (hipMemsetAsync(out, 0, (size_t)n_tensors * sizeof(mobi_health_record), ST(stream)) != hipSuccess) return MOBI_ERR_LAUNCH;
  hipLaunchKernelGGL(tensor_health_kernel, dim3((unsigned)blocks), dim3(kHealthBlock), 0, ST(stream), a, out);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}
