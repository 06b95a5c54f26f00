// The attention probe (include/mobi_engine.h, mobi_attention_health; mobi_amd/health.py holds the fp64 numpy definition,
// attention_health_ref): a second, independent attention launch that recomputes softmax(q k^T) v of one mobi_attention launch
// from the launch's own operands with the exact row maximum as the shift and fp32 probabilities, and records per (image, head)
// where the operands and the scores lie, how far the scores rise behind the first 32 keys and how far the production result
// (p->out, already written) is from the exact one.  Read only: the records are the only bytes it writes.  Runs under a
// health probe only; nothing here is tuned.
//
// One block of four waves per (image, head) walks the query rows in tiles of 128 (32 a wave) and, per tile, the keys in tiles
// of 64 staged through LDS.  Per key tile:
//   S = Q K^T     32x32x16 MFMAs on the stored 16-bit operands (products of two 16-bit values are exact in fp32, the sums are
//                 fp32), times cexp, into the wave's own [32][64] fp32 slab of LDS
//   softmax, P V  lane (row r = lane & 31, channel half = lane >> 5) reads its row's 64 scores in key order, raises the running
//                 maximum m, rescales l and o by 2^(m_old - m_new) and adds p_j = 2^(e_j - m_new) to l and p_j v_j to its
//                 channels with fp32 FMAs: p is never rounded to the storage type.
// A row's sums therefore run in key order, tile after tile, whatever the grid or the batch holds: no atomics, and two launches
// give bit-equal records.  Keys beyond tk, rows beyond tq and channels beyond dh are zeros in LDS (nothing is read out of
// bounds), masked scores are -inf and no loop reaches them.  Every field is a maximum, a minimum or an integer count; the block
// reduces them through shuffles and LDS and thread 0 writes the record.
//
// The operand measures (absmax, inf + nan) are taken where an element is staged: q in every query tile (each row is staged
// once), k and v during the first query tile only.
#include "common.h"

namespace mobi {

constexpr int kAhThreads = 256, kAhWaves = 4, kAhRows = 128, kAhKeys = 64, kAhSld = 65;   // kAhSld: fp32 words per score row

struct AhArgs {
  const void* q; long long q_img; int q_row;
  const void* k; long long k_img; int k_row;
  const void* vt; long long vt_img; int vt_row;
  const void* out; long long out_img; int out_row;
  int heads, dh, tq, tk;
  float cexp, rise_limit;
  int v_rows;
};

template <typename T> struct AhFmt;
template <> struct AhFmt<f16_t> { static constexpr uint32_t INF = 0x7c00u; };
template <> struct AhFmt<bf16_t> { static constexpr uint32_t INF = 0x7f80u; };

// the fp32 bit pattern of a finite magnitude pattern of T (exact)
template <typename T>
__device__ __forceinline__ uint32_t ah_f32_bits(uint32_t h) {
  const float v = (float)__builtin_bit_cast(T, (uint16_t)h);
  return __builtin_bit_cast(uint32_t, v);
}

struct AhScan {
  uint32_t m = 0;       // the largest finite magnitude pattern
  int bad = 0;          // inf + nan
};

template <uint32_t INF>
__device__ __forceinline__ void ah_scan1(uint32_t h, AhScan& s) {
  s.bad += h >= INF;
  const uint32_t f = h < INF ? h : 0u;
  s.m = f > s.m ? f : s.m;
}

template <uint32_t INF>
__device__ __forceinline__ void ah_scan8(const u32x4& v, AhScan& s) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ah_scan1<INF>(v[i] & 0x7fffu, s);
    ah_scan1<INF>((v[i] >> 16) & 0x7fffu, s);
  }
}

// rows [row0, row0 + ROWS) of a row-major operand (this head's dh columns, 16-byte aligned) -> dst[ROWS][LD]; rows from
// `limit` on and the channels from dh to DHP are zeros
template <uint32_t INF, int ROWS, int DHP, int LD>
__device__ __forceinline__ void ah_stage_rows(uint16_t* dst, const uint16_t* src, long long row_stride, int row0, int limit, int dh,
                                              bool count, AhScan& s) {
  constexpr int CH = DHP / 8;
  for (int idx = threadIdx.x; idx < ROWS * CH; idx += kAhThreads) {
    const int r = idx / CH, c8 = idx - r * CH;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row0 + r < limit && c8 * 8 < dh) {
      v = ld16(src + (long long)(row0 + r) * row_stride + c8 * 8);
      if (count) ah_scan8<INF>(v, s);
    }
    st16(dst + r * LD + c8 * 8, v);
  }
}

// keys [k0, k0 + 64) of this head's V^T rows ([channel][key], any row stride, element loads) -> dst[key][LD]
template <uint32_t INF, int DHP, int LD>
__device__ __forceinline__ void ah_stage_vt(uint16_t* dst, const uint16_t* src, long long row_stride, int k0, int tk, int dh, bool count,
                                            AhScan& s) {
  for (int idx = threadIdx.x; idx < DHP * kAhKeys; idx += kAhThreads) {
    const int c = idx >> 6, j = idx & 63;
    uint16_t v = 0;
    if (c < dh && k0 + j < tk) {
      v = src[(long long)c * row_stride + k0 + j];
      if (count) ah_scan1<INF>(v & 0x7fffu, s);
    }
    dst[j * LD + c] = v;
  }
}

// NT: the block holds head dims up to 16 NT (a lane keeps 8 NT fp32 output channels)
template <typename T, int NT>
__global__ __launch_bounds__(kAhThreads) void attention_health_kernel(const AhArgs a, mobi_attention_health_record* __restrict__ rec) {
  typedef typename Vec8<T>::type V8;
  constexpr uint32_t INF = AhFmt<T>::INF;
  constexpr int DHP = NT * 16, LD = DHP + 8;                        // LD: 16-bit elements per staged row (a multiple of 8)
  __shared__ __attribute__((aligned(16))) uint16_t Qs[kAhRows * LD];
  __shared__ __attribute__((aligned(16))) uint16_t Ks[kAhKeys * LD];
  __shared__ __attribute__((aligned(16))) uint16_t Vs[kAhKeys * LD];
  __shared__ float Ss[kAhWaves * 32 * kAhSld];

  const int head = blockIdx.x, img = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, half = lane >> 5;
  const int dh = a.dh, tq = a.tq, tk = a.tk;
  const int nks = (dh + 15) >> 4;                                  // MFMA k-steps (16 channels each)
  const uint16_t* qg = reinterpret_cast<const uint16_t*>(a.q) + (long long)img * a.q_img + (long long)head * dh;
  const uint16_t* kg = reinterpret_cast<const uint16_t*>(a.k) + (long long)img * a.k_img + (long long)head * dh;
  const uint16_t* vg = reinterpret_cast<const uint16_t*>(a.vt) + (long long)img * a.vt_img +
                       (a.v_rows ? (long long)head * dh : (long long)head * dh * a.vt_row);
  const uint16_t* og = reinterpret_cast<const uint16_t*>(a.out) + (long long)img * a.out_img + (long long)head * dh;

  AhScan sq, sk, sv;
  int out_bad = 0, over = 0, err_row = -1;
  float e_max = -INFINITY, e_min = INFINITY, rise_max = 0.0f, ref_max = 0.0f, err_max = 0.0f;

  for (int q0 = 0; q0 < tq; q0 += kAhRows) {
    ah_stage_rows<INF, kAhRows, DHP, LD>(Qs, qg, a.q_row, q0, tq, dh, true, sq);
    const int grow = q0 + wave * 32 + r;
    const bool valid = grow < tq;
    float m = -INFINITY, l = 0.0f, f = -INFINITY;
    float o[8 * NT];
#pragma unroll
    for (int i = 0; i < 8 * NT; ++i) o[i] = 0.0f;

    for (int k0 = 0; k0 < tk; k0 += kAhKeys) {
      __syncthreads();                                             // the last tile's K, V and scores are read
      ah_stage_rows<INF, kAhKeys, DHP, LD>(Ks, kg, a.k_row, k0, tk, dh, q0 == 0, sk);
      if (a.v_rows) ah_stage_rows<INF, kAhKeys, DHP, LD>(Vs, vg, a.vt_row, k0, tk, dh, q0 == 0, sv);
      else ah_stage_vt<INF, DHP, LD>(Vs, vg, a.vt_row, k0, tk, dh, q0 == 0, sv);
      __syncthreads();

      // S = Q K^T: A = Q[row r][8 half + j], B = K^T[8 half + j][key r]; D: key on the lane, rows in the registers
      f32x16 acc0, acc1;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.0f;
      for (int ks = 0; ks < nks; ++ks) {
        const int c = ks * 16 + half * 8;
        const V8 fa = *reinterpret_cast<const V8*>(Qs + (wave * 32 + r) * LD + c);
        const V8 fb0 = *reinterpret_cast<const V8*>(Ks + r * LD + c);
        const V8 fb1 = *reinterpret_cast<const V8*>(Ks + (32 + r) * LD + c);
        acc0 = mfma32(fa, fb0, acc0);
        acc1 = mfma32(fa, fb1, acc1);
      }
      float* sw = Ss + wave * 32 * kAhSld;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * half;
        sw[row * kAhSld + r] = k0 + r < tk ? acc0[i] * a.cexp : -INFINITY;
        sw[row * kAhSld + 32 + r] = k0 + 32 + r < tk ? acc1[i] * a.cexp : -INFINITY;
      }
      __syncthreads();

      // this lane's row: the tile's extremes, then the online step
      const float* srow = sw + r * kAhSld;
      const int jn = tk - k0 < kAhKeys ? tk - k0 : kAhKeys;
      float tmax = -INFINITY, tmin = INFINITY;
      for (int j = 0; j < jn; ++j) {
        const float s = srow[j];
        tmax = fmaxf(tmax, s);
        tmin = fminf(tmin, s);
        if (k0 == 0 && j == 31) f = tmax;
      }
      if (k0 == 0 && jn < 32) f = tmax;
      if (valid) {
        e_max = fmaxf(e_max, tmax);
        e_min = fminf(e_min, tmin);
      }
      const float m_new = fmaxf(m, tmax);
      const float alpha = exp2f(m - m_new);
      l *= alpha;
#pragma unroll
      for (int i = 0; i < 8 * NT; ++i) o[i] *= alpha;
      for (int j = 0; j < jn; ++j) {
        const float p = exp2f(srow[j] - m_new);
        l += p;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (t < nks) {
            float v[8];
            unpack8<T>(ld16(Vs + j * LD + t * 16 + half * 8), v);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[t * 8 + e] = __builtin_fmaf(p, v[e], o[t * 8 + e]);
          }
        }
      }
      m = m_new;
    }

    // the tile's rows against the production result
    if (valid) {
      if (half == 0) {
        const float rise = m - f;
        rise_max = fmaxf(rise_max, rise);
        over += rise > a.rise_limit;
      }
      const uint16_t* orow = og + (long long)grow * a.out_row;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int c = t * 16 + half * 8 + e;
          if (c < dh) {
            const float ref = o[t * 8 + e] / l;
            ref_max = fmaxf(ref_max, fabsf(ref));
            const uint16_t bits = orow[c];
            if ((bits & 0x7fffu) >= INF) {
              ++out_bad;
            } else {
              const float err = fabsf((float)__builtin_bit_cast(T, bits) - ref);
              if (err_row < 0 || err > err_max) {
                err_max = err;
                err_row = grow;
              }
            }
          }
        }
      }
    }
  }

  // the block's record: shuffles inside a wave, LDS across the four
  uint32_t mq = ah_f32_bits<T>(sq.m), mk = ah_f32_bits<T>(sk.m), mv = ah_f32_bits<T>(sv.m);
  int in_bad = sq.bad + sk.bad + sv.bad;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t oq = (uint32_t)__shfl_xor((int)mq, d, 64), ok = (uint32_t)__shfl_xor((int)mk, d, 64),
                   ov = (uint32_t)__shfl_xor((int)mv, d, 64);
    mq = oq > mq ? oq : mq;
    mk = ok > mk ? ok : mk;
    mv = ov > mv ? ov : mv;
    in_bad += __shfl_xor(in_bad, d, 64);
    out_bad += __shfl_xor(out_bad, d, 64);
    over += __shfl_xor(over, d, 64);
    e_max = fmaxf(e_max, __shfl_xor(e_max, d, 64));
    e_min = fminf(e_min, __shfl_xor(e_min, d, 64));
    rise_max = fmaxf(rise_max, __shfl_xor(rise_max, d, 64));
    ref_max = fmaxf(ref_max, __shfl_xor(ref_max, d, 64));
    const float oe = __shfl_xor(err_max, d, 64);
    const int orw = __shfl_xor(err_row, d, 64);
    if (orw >= 0 && (err_row < 0 || oe > err_max || (oe == err_max && orw < err_row))) {
      err_max = oe;
      err_row = orw;
    }
  }
  __syncthreads();                                                 // (the score slabs are free: the record's partials go there)
  uint32_t* red = reinterpret_cast<uint32_t*>(Ss);
  if (lane == 0) {
    uint32_t* w = red + wave * 12;
    w[0] = mq; w[1] = mk; w[2] = mv; w[3] = (uint32_t)in_bad; w[4] = (uint32_t)out_bad;
    w[5] = __builtin_bit_cast(uint32_t, e_max); w[6] = __builtin_bit_cast(uint32_t, e_min);
    w[7] = __builtin_bit_cast(uint32_t, rise_max); w[8] = (uint32_t)over; w[9] = __builtin_bit_cast(uint32_t, ref_max);
    w[10] = __builtin_bit_cast(uint32_t, err_max); w[11] = (uint32_t)err_row;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kAhWaves; ++w) {
      const uint32_t* x = red + w * 12;
      mq = x[0] > mq ? x[0] : mq;
      mk = x[1] > mk ? x[1] : mk;
      mv = x[2] > mv ? x[2] : mv;
      in_bad += (int)x[3];
      out_bad += (int)x[4];
      e_max = fmaxf(e_max, __builtin_bit_cast(float, x[5]));
      e_min = fminf(e_min, __builtin_bit_cast(float, x[6]));
      rise_max = fmaxf(rise_max, __builtin_bit_cast(float, x[7]));
      over += (int)x[8];
      ref_max = fmaxf(ref_max, __builtin_bit_cast(float, x[9]));
      const float oe = __builtin_bit_cast(float, x[10]);
      const int orw = (int)x[11];
      if (orw >= 0 && (err_row < 0 || oe > err_max || (oe == err_max && orw < err_row))) {
        err_max = oe;
        err_row = orw;
      }
    }
    mobi_attention_health_record o;
    o.q_absmax_bits = mq; o.k_absmax_bits = mk; o.v_absmax_bits = mv;
    o.in_nonfinite = in_bad; o.out_nonfinite = out_bad;
    o.e_max = e_max; o.e_min = e_min; o.rise_max = rise_max; o.rows_rise_over = over;
    o.ref_absmax_bits = __builtin_bit_cast(uint32_t, ref_max);
    o.err_max = err_max; o.err_row = err_row;
    rec[(long long)img * a.heads + head] = o;
  }
}

template <typename T>
static int launch_attention_health(const AhArgs& a, int images, mobi_attention_health_record* out, hipStream_t st) {
  const dim3 grid((unsigned)a.heads, (unsigned)images), block(kAhThreads);
  if (a.dh <= 16) hipLaunchKernelGGL((attention_health_kernel<T, 1>), grid, block, 0, st, a, out);
  else if (a.dh <= 48) hipLaunchKernelGGL((attention_health_kernel<T, 3>), grid, block, 0, st, a, out);
  else if (a.dh <= 80) hipLaunchKernelGGL((attention_health_kernel<T, 5>), grid, block, 0, st, a, out);
  else hipLaunchKernelGGL((attention_health_kernel<T, 10>), grid, block, 0, st, a, out);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

}  // namespace mobi

extern "C" int mobi_attention_health(const mobi_attention_params* p, float rise_limit, mobi_attention_health_record* out, void* stream) {
  using namespace mobi;
  // mobi_attention's checks, in its order
  if (!p || !p->q || !p->k || !p->vt || !p->out || !out) return MOBI_ERR_ARG;
  if (p->dtype != MOBI_F16 && p->dtype != MOBI_BF16) return MOBI_ERR_ARG;
  if (p->images <= 0 || p->heads <= 0 || p->tq <= 0 || p->tk <= 0 || p->dh <= 0) return MOBI_ERR_ARG;
  if (!(rise_limit == rise_limit)) return MOBI_ERR_ARG;                           // nan
  if ((p->dh & 7) || p->dh > 160) return MOBI_ERR_UNSUPPORTED;
  if (p->v_layout != 0 && p->v_layout != 1) return MOBI_ERR_ARG;
  if (p->v_layout == 1 && ((p->vt_row_stride & 7) || (p->vt_img_stride & 7) ||
                           (reinterpret_cast<uintptr_t>(p->vt) & 15))) return MOBI_ERR_ALIGN;
  if ((p->q_row_stride & 7) || (p->k_row_stride & 7) || (p->out_row_stride & 3)) return MOBI_ERR_ALIGN;
  if ((p->q_img_stride & 7) || (p->k_img_stride & 7) || (p->out_img_stride & 3)) return MOBI_ERR_ALIGN;
  if ((reinterpret_cast<uintptr_t>(p->q) | reinterpret_cast<uintptr_t>(p->k) |
       reinterpret_cast<uintptr_t>(p->out)) & 15) return MOBI_ERR_ALIGN;
  if (reinterpret_cast<uintptr_t>(out) & 3) return MOBI_ERR_ALIGN;
  if (p->heads > 65535 || p->images > 65535) return MOBI_ERR_UNSUPPORTED;
  AhArgs a;
  a.q = p->q; a.q_img = p->q_img_stride; a.q_row = p->q_row_stride;
  a.k = p->k; a.k_img = p->k_img_stride; a.k_row = p->k_row_stride;
  a.vt = p->vt; a.vt_img = p->vt_img_stride; a.vt_row = p->vt_row_stride;
  a.out = p->out; a.out_img = p->out_img_stride; a.out_row = p->out_row_stride;
  a.heads = p->heads; a.dh = p->dh; a.tq = p->tq; a.tk = p->tk;
  a.cexp = p->q_log2_scaled ? 1.0f : p->scale * 1.4426950408889634f;           // (mobi_attention's own expression)
  a.rise_limit = rise_limit;
  a.v_rows = p->v_layout == 1;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return p->dtype == MOBI_F16 ? launch_attention_health<f16_t>(a, p->images, out, st)
                              : launch_attention_health<bf16_t>(a, p->images, out, st);
}
