// Multi-tensor passes of the fp16 training step (include/mobi_engine.h, "Multi-tensor passes"; mobi_amd/train.py GradScaler /
// AdamW.step_scaled): the gradient statistics (sum of squares + non-finite flag) and the AdamW update of EVERY listed tensor in one
// launch each, instead of one launch per tensor (432 adapter tensors + the conditioning stage's: ~880 launches of a few hundred KB
// to a few MB each); the EMA update / swap of every (parameter, shadow) pair (mobi_amd/ldm/modules/ema.py); and the gradient
// accumulation of a window of micro-batches (mobi_amd/train.py GradAccumulator); and the checkpoint snapshot (mobi_amd/checkpoint.py): a
// word-for-word copy of every mutable tensor with a 64-bit digest and a non-finite flag per tensor.  All kernels walk a device-resident table of tensors through a device-resident chunk map: every tensor is cut
// into chunks of kMtChunk elements, one 256-thread block takes chunks in a grid-stride walk, the grid follows the CU count.  Pure
// streaming: 16-byte accesses on the 16-byte-aligned body of a chunk, 4-byte accesses on its head and tail (a tensor may start at
// any 4-byte boundary); no atomics, LDS only for the block reduction of the statistics -- except the snapshot,
// whose per-tensor integer sums meet by one 64-bit vector atomic add per wave and tensor (order-free: wrapping sums commute).
#include "adamw.h"
#include "common.h"

namespace mobi {

constexpr int kMtChunk = 8192;        // elements per chunk (a multiple of 4: every chunk of a tensor has the tensor's alignment phase)
constexpr int kMtBlock = 256;
constexpr int kMtMaxBlocks = 2048;    // the workspace holds one fp64 partial per block
constexpr int kMtBlocksPerCu = 4;

// elements in front of the next 16-byte boundary (0 .. 3; the pointer is 4-byte aligned)
__device__ __forceinline__ int mt_phase(const void* p) { return (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2; }

// chunk c of the map -> (tensor entry, element offset, length); false for an entry that does not lie inside its tensor (a map that
// does not belong to the table must never turn into an out-of-bounds access)
// (Entry: mobi_mt_tensor or mobi_mt_pair -- a table row with its element count in `n`)
template <class Entry>
__device__ __forceinline__ bool mt_chunk(const Entry* __restrict__ tensors, int n_tensors, const mobi_mt_chunk* __restrict__ chunks,
                                         int c, Entry& t, long long& off, int& len) {
  const mobi_mt_chunk ch = chunks[c];
  if (ch.tensor < 0 || ch.tensor >= n_tensors) return false;
  t = tensors[ch.tensor];
  off = ch.offset;
  if (off < 0 || off >= t.n) return false;
  const long long left = t.n - off;
  len = left < kMtChunk ? (int)left : kMtChunk;
  return true;
}

// ---------------------------------------------------------------------------------------------------------------------
// Gradient statistics.  Squares and sums in fp64 from the first add upward: the square of a finite fp32 value (up to 1.2e77) is
// exact in fp64 and a sum of them cannot overflow, so the sum is non-finite exactly when some gradient is inf or nan -- the flag
// is read off the sum, no per-element test.  Fixed order: a thread adds its elements in ascending order into four accumulators
// (one per lane of the 16-byte access), lanes and waves are combined by a fixed tree, every block writes one partial and the
// finish pass adds the partials in ascending block order.  Bit-reproducible for a given grid (= for a given device).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMtBlock) void grad_stats_kernel(const mobi_mt_tensor* __restrict__ tensors, int n_tensors,
                                                              const mobi_mt_chunk* __restrict__ chunks, int n_chunks,
                                                              double* __restrict__ partial) {
  __shared__ double wave_part[kMtBlock / 64];
  const int tid = threadIdx.x;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    mobi_mt_tensor t;
    long long off;
    int len;
    if (!mt_chunk(tensors, n_tensors, chunks, c, t, off, len)) continue;
    const float* __restrict__ g = t.grad + off;
    const int ph = mt_phase(g), head = ph < len ? ph : len;
    const int nvec = (len - head) >> 2, tail0 = head + (nvec << 2);
    if (tid < head) {
      const double x = (double)g[tid];
      a0 = fma(x, x, a0);
    }
    if (tid < len - tail0) {
      const double x = (double)g[tail0 + tid];
      a1 = fma(x, x, a1);
    }
    const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + head);
#pragma unroll 4
    for (int i = tid; i < nvec; i += kMtBlock) {
      const f32x4 x = gv[i];
      const double x0 = (double)x[0], x1 = (double)x[1], x2 = (double)x[2], x3 = (double)x[3];
      a0 = fma(x0, x0, a0);
      a1 = fma(x1, x1, a1);
      a2 = fma(x2, x2, a2);
      a3 = fma(x3, x3, a3);
    }
  }
  double s = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((tid & 63) == 0) wave_part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

__global__ __launch_bounds__(kMtBlock) void grad_stats_finish_kernel(const double* __restrict__ partial, int blocks,
                                                                     mobi_grad_stats_record* __restrict__ out) {
  __shared__ double part[kMtMaxBlocks];
  for (int i = threadIdx.x; i < blocks; i += kMtBlock) part[i] = partial[i];
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < blocks; ++i) s += part[i];
    out->sumsq = s;
    out->nonfinite = ((__double_as_longlong(s) >> 52) & 0x7ff) == 0x7ff ? 1 : 0;      // exponent all ones: inf or nan
    out->reserved = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// AdamW over the whole list: g * grad_mul (1 / loss scale times the clip coefficient), then the update of adamw.h.  The 16-byte
// path needs param, grad and both moments at the same alignment phase; a tensor whose four pointers disagree takes the 4-byte
// path for all of its elements.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMtBlock) void adamw_multi_kernel(const mobi_mt_tensor* __restrict__ tensors, int n_tensors,
                                                               const mobi_mt_chunk* __restrict__ chunks, int n_chunks, float grad_mul,
                                                               float lr, float b1, float b2, float eps, float wd, float bc1,
                                                               float bc2_sqrt) {
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    mobi_mt_tensor t;
    long long off;
    int len;
    if (!mt_chunk(tensors, n_tensors, chunks, c, t, off, len)) continue;
    float* __restrict__ p = t.param + off;
    const float* __restrict__ g = t.grad + off;
    float* __restrict__ m = t.exp_avg + off;
    float* __restrict__ v = t.exp_avg_sq + off;
    const int ph = mt_phase(g);
    const bool same = ph == mt_phase(p) && ph == mt_phase(m) && ph == mt_phase(v);
    const int head = same && ph < len ? ph : len;
    const int nvec = (len - head) >> 2, tail0 = head + (nvec << 2);
    // head [0, head) and tail [tail0, len): at most 3 elements each, or the whole chunk where the pointers disagree
    auto one = [&](int i) {
      float pi = p[i], mi = m[i], vi = v[i];
      adamw_update(pi, g[i] * grad_mul, mi, vi, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
      m[i] = mi;
      v[i] = vi;
      p[i] = pi;
    };
    for (int i = tid; i < head; i += kMtBlock) one(i);
    for (int i = tail0 + tid; i < len; i += kMtBlock) one(i);
    f32x4* __restrict__ pv = reinterpret_cast<f32x4*>(p + head);
    const f32x4* __restrict__ gv = reinterpret_cast<const f32x4*>(g + head);
    f32x4* __restrict__ mv = reinterpret_cast<f32x4*>(m + head);
    f32x4* __restrict__ vv = reinterpret_cast<f32x4*>(v + head);
#pragma unroll 2
    for (int i = tid; i < nvec; i += kMtBlock) {
      f32x4 pq = pv[i], mq = mv[i], vq = vv[i];
      const f32x4 gq = gv[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pi = pq[j], mi = mq[j], vi = vq[j];
        adamw_update(pi, gq[j] * grad_mul, mi, vi, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
        pq[j] = pi;
        mq[j] = mi;
        vq[j] = vi;
      }
      mv[i] = mq;
      vv[i] = vq;
      pv[i] = pq;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Tensor pairs: the EMA update of the shadows (b <- b - omd (b - a): subtract, multiply, subtract, each rounded to fp32 -- what
// torch's shadow.sub_(omd * (shadow - param)) computes; a contracted b - omd d differs in the last bit) or the exchange of a
// and b; or one micro-batch's gradient a into the accumulator b (b <- b + w a: multiply, add, each rounded to fp32 -- the
// numpy / torch fp32 sequence, no contraction into one rounding; or b <- w a WITHOUT reading b: a window's first contribution
// never meets what an earlier window left in the accumulator, nan included).  One walker for all four (OP, below).  The 16-byte
// path needs both pointers at the same alignment phase, as above.
// ---------------------------------------------------------------------------------------------------------------------
// the walker's OPs: the two of mobi_ema_multi carry their public values, the two of mobi_accum_multi follow
enum { kPairEma = MOBI_MT_EMA, kPairSwap = MOBI_MT_SWAP, kPairAccum = 2, kPairAssign = 3 };

__device__ __forceinline__ float ema_update(float b, float a, float omd) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float s = omd * d;
  return b - s;
}

__device__ __forceinline__ float accum_update(float b, float a, float w) {
#pragma clang fp contract(off)
  const float s = w * a;
  return b + s;
}

// `w`: one_minus_decay (EMA), the micro-batch weight (ACCUM, ASSIGN), not read (SWAP).  a is read only except under SWAP.
template <int OP>
__global__ __launch_bounds__(kMtBlock) void pair_multi_kernel(const mobi_mt_pair* __restrict__ pairs, int n_pairs,
                                                              const mobi_mt_chunk* __restrict__ chunks, int n_chunks, float w) {
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    mobi_mt_pair t;
    long long off;
    int len;
    if (!mt_chunk(pairs, n_pairs, chunks, c, t, off, len)) continue;
    float* __restrict__ a = t.a + off;
    float* __restrict__ b = t.b + off;
    const int ph = mt_phase(b);
    const bool same = ph == mt_phase(a);
    const int head = same && ph < len ? ph : len;
    const int nvec = (len - head) >> 2, tail0 = head + (nvec << 2);
    auto one = [&](int i) {
      const float ai = a[i];
      if (OP == kPairAssign) {
        b[i] = w * ai;
      } else if (OP == kPairAccum) {
        b[i] = accum_update(b[i], ai, w);
      } else if (OP == kPairEma) {
        b[i] = ema_update(b[i], ai, w);
      } else {
        a[i] = b[i];
        b[i] = ai;
      }
    };
    for (int i = tid; i < head; i += kMtBlock) one(i);
    for (int i = tail0 + tid; i < len; i += kMtBlock) one(i);
    f32x4* __restrict__ av = reinterpret_cast<f32x4*>(a + head);
    f32x4* __restrict__ bv = reinterpret_cast<f32x4*>(b + head);
#pragma unroll 4
    for (int i = tid; i < nvec; i += kMtBlock) {
      const f32x4 aq = av[i];
      if (OP == kPairAssign) {                       // b is not read
        f32x4 bq;
#pragma unroll
        for (int j = 0; j < 4; ++j) bq[j] = w * aq[j];
        bv[i] = bq;
      } else if (OP == kPairSwap) {
        const f32x4 bq = bv[i];
        av[i] = bq;
        bv[i] = aq;
      } else {
        f32x4 bq = bv[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) bq[j] = OP == kPairEma ? ema_update(bq[j], aq[j], w) : accum_update(bq[j], aq[j], w);
        bv[i] = bq;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Snapshot: b <- a as a move of 32-bit words (no arithmetic: denormals, both zeros and NaN payloads arrive as they left; where
// b is NULL nothing is written) while every word enters its tensor's digest, sum_i uint64(u_i ^ 0x9E3779B9) * uint64((2 i + 1)
// mod 2^32) mod 2^64 (i: the element's index in its tensor), and the non-finite flag (exponent bits all set).  One 32 x 32 -> 64
// multiply-add per element.  A thread keeps its sum across the chunks of its walk for as long as they belong to one tensor;
// when the tensor changes, and at the end, every wave adds its lanes up and lane 0 issues ONE 64-bit vector atomic add into
// the tensor's record (and one atomic or of the flag, only where it is set).  Wrapping integer sums commute: the records do
// not depend on the grid, the order of the map or the order in which the atomics land.  The records are zeroed on the stream
// in front of the launch.
// ---------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kDigestXor = 0x9E3779B9u;

__device__ __forceinline__ void snapshot_flush(mobi_snapshot_record* __restrict__ out, int tensor, unsigned long long s, int bad) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += (unsigned long long)__shfl_xor((long long)s, o, 64);
    bad |= __shfl_xor(bad, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (s) atomicAdd(reinterpret_cast<unsigned long long*>(&out[tensor].digest), s);
    if (bad) atomicOr(&out[tensor].nonfinite, 1);
  }
}

// one chunk: [0, head) and [tail0, len) word by word, the 16-byte aligned body between them four words at a time.  COPY is
// decided per chunk, outside the loops: with the test inside, every store waits for its load before the next load is issued
template <bool COPY>
__device__ __forceinline__ void snapshot_chunk(const uint32_t* __restrict__ a, uint32_t* __restrict__ b, long long off, int len,
                                               int head, unsigned long long& s, int& bad) {
  const int tid = threadIdx.x;
  const int nvec = (len - head) >> 2, tail0 = head + (nvec << 2);
  auto word = [&](uint32_t u, long long i) {         // i: the index in the tensor
    s += (unsigned long long)(u ^ kDigestXor) * (unsigned long long)(uint32_t)(2ull * (unsigned long long)i + 1ull);
    bad |= (u & 0x7f800000u) == 0x7f800000u;
  };
  auto one = [&](int i) {
    const uint32_t u = a[i];
    if (COPY) b[i] = u;
    word(u, off + i);
  };
  for (int i = tid; i < head; i += kMtBlock) one(i);
  for (int i = tail0 + tid; i < len; i += kMtBlock) one(i);
  const u32x4* __restrict__ av = reinterpret_cast<const u32x4*>(a + head);
  u32x4* __restrict__ bv = COPY ? reinterpret_cast<u32x4*>(b + head) : nullptr;
#pragma unroll 4
  for (int i = tid; i < nvec; i += kMtBlock) {
    const u32x4 q = av[i];
    if (COPY) bv[i] = q;
    const long long i0 = off + head + ((long long)i << 2);
#pragma unroll
    for (int j = 0; j < 4; ++j) word(q[j], i0 + j);
  }
}

__global__ __launch_bounds__(kMtBlock) void snapshot_multi_kernel(const mobi_mt_pair* __restrict__ pairs, int n_pairs,
                                                                  const mobi_mt_chunk* __restrict__ chunks, int n_chunks,
                                                                  mobi_snapshot_record* __restrict__ out) {
  const int tid = threadIdx.x;
  unsigned long long s = 0;
  int bad = 0, cur = -1;                             // cur: the tensor `s` and `bad` belong to (the same for every thread of the block)
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    mobi_mt_pair t;
    long long off;
    int len;
    if (!mt_chunk(pairs, n_pairs, chunks, c, t, off, len)) continue;
    const int tensor = chunks[c].tensor;
    if (tensor != cur) {
      if (cur >= 0) snapshot_flush(out, cur, s, bad);
      s = 0, bad = 0, cur = tensor;
    }
    const uint32_t* __restrict__ a = reinterpret_cast<const uint32_t*>(t.a) + off;
    uint32_t* __restrict__ b = t.b ? reinterpret_cast<uint32_t*>(t.b) + off : nullptr;
    const int ph = mt_phase(a);
    const bool same = !b || ph == mt_phase(b);
    const int head = same && ph < len ? ph : len;
    if (b) {
      snapshot_chunk<true>(a, b, off, len, head, s, bad);
    } else {
      snapshot_chunk<false>(a, b, off, len, head, s, bad);
    }
  }
  if (cur >= 0) snapshot_flush(out, cur, s, bad);
}

// ---------------------------------------------------------------------------------------------------------------------
// Repack: the 16-bit images of every listed fp32 master weight W [n][k] in one launch (mobi_engine.h mobi_repack_multi; what
// ops.pack_linear / train._packed_t build tensor by tensor after an optimizer update): w = round(W), wt = its 1-KiB request
// images (tile_weights_kernel's index map), w_t = round(W)^T, wt_t = the images of that.  One rounding (the cast, round to
// nearest even as torch's .to()), everything else is placement.  One block per 64 x 64 tile of W: 16-byte reads along k,
// the rounded tile in LDS, then row reads for w / wt and column reads for w_t / wt_t, 16-byte stores.
// LDS: a row is 32 dwords (64 values) and every 8 rows are followed by 4 dwords of padding, dword (r, d) at
// 32 r + 4 (r >> 3) + d.
//   stores  ds_write_b64, 16 lanes = one row = 32 consecutive dwords: conflict-free
//   rows    ds_read_b128 of (row = idx >> 3, chunk = idx & 7): a wave reads 8 rows of one 8-row group; each 16-lane group of
//           the instruction holds four half rows, two of even and two of odd rows, one in each 64-byte half: 64 distinct banks
//           (mod 64)
//   columns ds_read_b32 of dword kp (two neighbouring k) of rows 8 nc + j, lane = (kp, nc) with nc = lane & 7: a 32-lane half
//           holds nc = 0..7 and four consecutive kp from a multiple of 4; bank = (32 row + 4 nc + kp) mod 32 = 4 nc + kp - kp0:
//           32 distinct banks.  (Without the padding the eight nc would meet on four banks.)  One thread turns its 8 dwords
//           into the two 16-byte chunks w_t[k][8 nc ..] and w_t[k + 1][8 nc ..]: 8 lanes write 128 contiguous bytes.
// Shapes the 16-byte paths cannot take (k % 8 / n % 8 non-zero, a source off the 16-byte grid) go element by element.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kRpTile = 64;
constexpr int kRpLdsDwords = kRpTile * 32 + (kRpTile / 8) * 4;

__device__ __forceinline__ int rp_lds(int r, int d) { return r * 32 + (r >> 3) * 4 + d; }

// chunk (row R, 16-byte chunk kc of that row) of a matrix of `steps` 32-deep steps -> its chunk index in the tiled image
__device__ __forceinline__ long long rp_tiled_chunk(int R, int kc, int steps) {
  const int rr = R & 15, perm = (0x1320 >> (4 * ((rr >> 2) & 3))) & 3;          // P[(r >> 2) & 3] of {0, 2, 3, 1}
  return (((long long)(R >> 4) * steps + (kc >> 2)) * 16 + rr) * 4 + ((kc & 3) ^ perm);
}

template <typename T>
__global__ __launch_bounds__(kMtBlock) void repack_multi_kernel(const mobi_repack_entry* __restrict__ entries, int n_entries,
                                                                const mobi_mt_chunk* __restrict__ tiles) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kRpLdsDwords];
  const int tid = threadIdx.x;
  const mobi_mt_chunk tl = tiles[blockIdx.x];
  if (tl.tensor < 0 || tl.tensor >= n_entries) return;
  const mobi_repack_entry e = entries[tl.tensor];
  const int n = e.n, k = e.k;
  if (!e.src || n <= 0 || k <= 0) return;
  const long long tk = (k + kRpTile - 1) / kRpTile, tn = (n + kRpTile - 1) / kRpTile;
  if (tl.offset < 0 || tl.offset >= tn * tk) return;                             // (all returns above are block-uniform)
  const int n0 = (int)(tl.offset / tk) * kRpTile, k0 = (int)(tl.offset % tk) * kRpTile;
  const float* __restrict__ src = e.src;

  // fp32 tile -> rounded tile in LDS; what lies outside the tensor is written as zero and never stored
  const bool vld = !(k & 3) && !(reinterpret_cast<uintptr_t>(src) & 15);
  f32x4 v[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = it * kMtBlock + tid, gr = n0 + (idx >> 4), gc = k0 + 4 * (idx & 15);
    v[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (gr < n && gc < k) {
      const float* p = src + (long long)gr * k + gc;
      if (vld) {
        v[it] = *reinterpret_cast<const f32x4*>(p);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (gc + j < k) v[it][j] = p[j];
      }
    }
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = it * kMtBlock + tid;
    const float f[4] = {v[it][0], v[it][1], v[it][2], v[it][3]};
    *reinterpret_cast<u32x2*>(&lds[rp_lds(idx >> 4, 2 * (idx & 15))]) = pack4<T>(f);
  }
  __syncthreads();
  const uint16_t* lds16 = reinterpret_cast<const uint16_t*>(lds);

  // rows: w and wt
  uint16_t* __restrict__ w = static_cast<uint16_t*>(e.w);
  u32x4* __restrict__ wt = !(n & 15) && !(k & 31) ? static_cast<u32x4*>(e.wt) : nullptr;
  if (!(k & 7)) {
    if (w || wt) {
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int idx = it * kMtBlock + tid, r = idx >> 3, c8 = idx & 7, gr = n0 + r, gc = k0 + 8 * c8;
        if (gr < n && gc < k) {
          const u32x4 q = *reinterpret_cast<const u32x4*>(&lds[rp_lds(r, 4 * c8)]);
          if (w) st16(w + (long long)gr * k + gc, q);
          if (wt) wt[rp_tiled_chunk(gr, gc >> 3, k >> 5)] = q;
        }
      }
    }
  } else if (w) {
    for (int i = tid; i < kRpTile * kRpTile; i += kMtBlock) {
      const int r = i >> 6, c = i & 63;
      if (n0 + r < n && k0 + c < k) w[(long long)(n0 + r) * k + k0 + c] = lds16[2 * rp_lds(r, 0) + c];
    }
  }

  // columns: w_t and wt_t (the matrix [k][n])
  uint16_t* __restrict__ w_t = static_cast<uint16_t*>(e.w_t);
  u32x4* __restrict__ wt_t = !(k & 15) && !(n & 31) ? static_cast<u32x4*>(e.wt_t) : nullptr;
  if (!(n & 7)) {
    const int nc = tid & 7, kp = tid >> 3, gn = n0 + 8 * nc, gk = k0 + 2 * kp;
    if ((w_t || wt_t) && gn < n && gk < k) {
      uint32_t d[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = lds[rp_lds(8 * nc + j, kp)];
      u32x4 lo, hi;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        lo[j] = (d[2 * j] & 0xffffu) | (d[2 * j + 1] << 16);
        hi[j] = (d[2 * j] >> 16) | (d[2 * j + 1] & 0xffff0000u);
      }
      if (w_t) st16(w_t + (long long)gk * n + gn, lo);
      if (wt_t) wt_t[rp_tiled_chunk(gk, gn >> 3, n >> 5)] = lo;
      if (gk + 1 < k) {
        if (w_t) st16(w_t + (long long)(gk + 1) * n + gn, hi);
        if (wt_t) wt_t[rp_tiled_chunk(gk + 1, gn >> 3, n >> 5)] = hi;
      }
    }
  } else if (w_t) {
    for (int i = tid; i < kRpTile * kRpTile; i += kMtBlock) {
      const int c = i >> 6, r = i & 63;
      if (n0 + r < n && k0 + c < k) w_t[(long long)(k0 + c) * n + n0 + r] = lds16[2 * rp_lds(r, 0) + c];
    }
  }
}

static int mt_grid(int n_chunks) {
  static int cus = 0;
  if (!cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus = n;
  }
  int g = cus * kMtBlocksPerCu;
  if (g > kMtMaxBlocks) g = kMtMaxBlocks;
  return n_chunks < g ? n_chunks : g;
}

}  // namespace mobi

using namespace mobi;
#define ST(stream) reinterpret_cast<hipStream_t>(stream)

extern "C" size_t mobi_multi_tensor_workspace_bytes(int32_t* chunk_elems) {
  if (chunk_elems) *chunk_elems = kMtChunk;
  return (size_t)kMtMaxBlocks * sizeof(double);
}

extern "C" int mobi_grad_stats(const mobi_mt_tensor* tensors, int32_t n_tensors, const mobi_mt_chunk* chunks, int32_t n_chunks,
                               void* workspace, mobi_grad_stats_record* out, void* stream) {
  if (!tensors || !chunks || !workspace || !out || n_tensors <= 0 || n_chunks <= 0) return MOBI_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7) || (reinterpret_cast<uintptr_t>(out) & 7)) return MOBI_ERR_ALIGN;
  const int blocks = mt_grid(n_chunks);
  hipLaunchKernelGGL(grad_stats_kernel, dim3(blocks), dim3(kMtBlock), 0, ST(stream), tensors, n_tensors, chunks, n_chunks,
                     static_cast<double*>(workspace));
  MOBI_CHECK_LAUNCH();
  hipLaunchKernelGGL(grad_stats_finish_kernel, dim3(1), dim3(kMtBlock), 0, ST(stream), static_cast<const double*>(workspace), blocks, out);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_adamw_multi(const mobi_mt_tensor* tensors, int32_t n_tensors, const mobi_mt_chunk* chunks, int32_t n_chunks,
                                float grad_mul, float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                                void* stream) {
  if (!tensors || !chunks || n_tensors <= 0 || n_chunks <= 0 || step <= 0) return MOBI_ERR_ARG;
  const float bc1 = 1.0f - powf(beta1, (float)step), bc2 = 1.0f - powf(beta2, (float)step);
  hipLaunchKernelGGL(adamw_multi_kernel, dim3(mt_grid(n_chunks)), dim3(kMtBlock), 0, ST(stream), tensors, n_tensors, chunks, n_chunks,
                     grad_mul, lr, beta1, beta2, eps, weight_decay, bc1, sqrtf(bc2));
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

static bool pairs_args_ok(const mobi_mt_pair* pairs, int32_t n_pairs, const mobi_mt_chunk* chunks, int32_t n_chunks) {
  return pairs && chunks && n_pairs > 0 && n_chunks > 0;
}

template <int OP>
static int launch_pairs(const mobi_mt_pair* pairs, int32_t n_pairs, const mobi_mt_chunk* chunks, int32_t n_chunks, float scalar,
                        void* stream) {
  hipLaunchKernelGGL(pair_multi_kernel<OP>, dim3(mt_grid(n_chunks)), dim3(kMtBlock), 0, ST(stream), pairs, n_pairs, chunks, n_chunks,
                     scalar);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_ema_multi(const mobi_mt_pair* pairs, int32_t n_pairs, const mobi_mt_chunk* chunks, int32_t n_chunks,
                              float one_minus_decay, int32_t op, void* stream) {
  if (!pairs_args_ok(pairs, n_pairs, chunks, n_chunks)) return MOBI_ERR_ARG;
  if (op == MOBI_MT_EMA) return launch_pairs<kPairEma>(pairs, n_pairs, chunks, n_chunks, one_minus_decay, stream);
  if (op == MOBI_MT_SWAP) return launch_pairs<kPairSwap>(pairs, n_pairs, chunks, n_chunks, one_minus_decay, stream);
  return MOBI_ERR_ARG;
}

extern "C" int mobi_accum_multi(const mobi_mt_pair* pairs, int32_t n_pairs, const mobi_mt_chunk* chunks, int32_t n_chunks, float w,
                                int32_t op, void* stream) {
  if (!pairs_args_ok(pairs, n_pairs, chunks, n_chunks)) return MOBI_ERR_ARG;
  if (op == MOBI_MT_ACCUM) return launch_pairs<kPairAccum>(pairs, n_pairs, chunks, n_chunks, w, stream);
  if (op == MOBI_MT_ASSIGN) return launch_pairs<kPairAssign>(pairs, n_pairs, chunks, n_chunks, w, stream);
  return MOBI_ERR_ARG;
}

extern "C" int mobi_snapshot_multi(const mobi_mt_pair* pairs, int32_t n_pairs, const mobi_mt_chunk* chunks, int32_t n_chunks,
                                   void* workspace, mobi_snapshot_record* out, void* stream) {
  (void)workspace;                                   // the per-tensor sums meet by atomics: nothing is staged
  if (!pairs_args_ok(pairs, n_pairs, chunks, n_chunks) || !out) return MOBI_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(out) & 7) return MOBI_ERR_ALIGN;
  if (hipMemsetAsync(out, 0, (size_t)n_pairs * sizeof(mobi_snapshot_record), ST(stream)) != hipSuccess) return MOBI_ERR_LAUNCH;
  hipLaunchKernelGGL(snapshot_multi_kernel, dim3(mt_grid(n_chunks)), dim3(kMtBlock), 0, ST(stream), pairs, n_pairs, chunks, n_chunks, out);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_repack_multi(const mobi_repack_entry* entries, int32_t n_entries, const mobi_mt_chunk* tiles, int32_t n_tiles,
                                 int32_t dtype, void* stream) {
  if (!entries || !tiles || n_entries <= 0 || n_tiles <= 0) return MOBI_ERR_ARG;
  if (dtype == MOBI_F16) {
    hipLaunchKernelGGL(repack_multi_kernel<f16_t>, dim3((unsigned)n_tiles), dim3(kMtBlock), 0, ST(stream), entries, n_entries, tiles);
  } else if (dtype == MOBI_BF16) {
    hipLaunchKernelGGL(repack_multi_kernel<bf16_t>, dim3((unsigned)n_tiles), dim3(kMtBlock), 0, ST(stream), entries, n_entries, tiles);
  } else {
    return MOBI_ERR_ARG;
  }
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}
