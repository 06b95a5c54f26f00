// Realism metrics (include/mobi_engine.h, "Realism metrics"; mobi_amd/realism.py): the pieces of LPIPS-alex and CLIP score
// that are not convolutions or transformer layers -- AlexNet's max-pool (with its ReLU), the LPIPS layer distance, the input
// normalisations and the final cosine.  The convolutions run on mobi_igemm, the ViT-B/32 tower on the CLIP tower's launches.
#include "common.h"

namespace mobi {

// ---------------------------------------------------------------------------------------------------------------------
// 3 x 3 / stride 2 max-pool, optional ReLU on read.  One thread = one output pixel x 8 channels (one 16-byte access per
// window tap).  Every input index is inside the image: 2 * (hout - 1) + 2 <= h - 1 by floor mode.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void maxpool3s2_kernel(const T* __restrict__ src, T* __restrict__ out, int batch, int h, int w, int c, int relu) {
  const int hout = (h - 3) / 2 + 1, wout = (w - 3) / 2 + 1, c8 = c >> 3;
  const long long total = (long long)batch * hout * wout * c8;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int cv = (int)(i % c8);
    long long r = i / c8;
    const int x = (int)(r % wout);
    r /= wout;
    const int y = (int)(r % hout);
    const long long n = r / hout;
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = relu ? 0.0f : -INFINITY;
    const T* base = src + ((n * h + 2 * y) * w + 2 * x) * c + cv * 8;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        float f[8];
        unpack8<T>(ld16(base + ((long long)dy * w + dx) * c), f);
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = f[j] > m[j] ? f[j] : m[j];
      }
    st16(out + i * 8, pack8<T>(m));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// LPIPS layer distance.  Grid (blocks, pairs), one wave per block; thread t of block b handles pixels
// b * 64 + t, + blocks * 64, ... of its pair.  Pass 1 sums relu(a)^2 and relu(b)^2 over the channels (and writes relu back
// when asked); pass 2 sums lin_c (a_c / na - b_c / nb)^2.  The wave's sum goes to ws[pair][block]; the finish launch adds
// a pair's partials in ascending block order.  Identical images give identical rows, so d(x, x) is exactly 0.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kLpipsMaxBlocks = 64;

static inline int lpips_blocks(int hw) {
  const int b = (hw + 63) / 64;
  return b < 1 ? 1 : (b > kLpipsMaxBlocks ? kLpipsMaxBlocks : b);
}

template <typename T>
__global__ __launch_bounds__(64) void lpips_distance_kernel(const mobi_lpips_distance_params p, int blocks) {
  const int pair = blockIdx.y, t = threadIdx.x, C = p.channels;
  T* fa = reinterpret_cast<T*>(p.feat) + (long long)pair * p.hw * C;
  T* fb = reinterpret_cast<T*>(p.feat) + ((long long)pair + p.pairs) * p.hw * C;
  float acc = 0.0f;
  for (int px = blockIdx.x * 64 + t; px < p.hw; px += blocks * 64) {
    T* ra = fa + (long long)px * C;
    T* rb = fb + (long long)px * C;
    float qa = 0.0f, qb = 0.0f;
    for (int c = 0; c < C; c += 8) {
      float a[8], b[8];
      unpack8<T>(ld16(ra + c), a);
      unpack8<T>(ld16(rb + c), b);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a[j] = a[j] > 0.0f ? a[j] : 0.0f;
        b[j] = b[j] > 0.0f ? b[j] : 0.0f;
        qa += a[j] * a[j];
        qb += b[j] * b[j];
      }
      if (p.relu_in_place) {
        st16(ra + c, pack8<T>(a));
        st16(rb + c, pack8<T>(b));
      }
    }
    const float na = sqrtf(qa) + p.eps, nb = sqrtf(qb) + p.eps;
    float d = 0.0f;
    for (int c = 0; c < C; c += 8) {
      float a[8], b[8], wl[8];
      unpack8<T>(ld16(ra + c), a);
      unpack8<T>(ld16(rb + c), b);
      ld8f(p.lin + c, wl);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float e = (a[j] > 0.0f ? a[j] : 0.0f) / na - (b[j] > 0.0f ? b[j] : 0.0f) / nb;
        d += wl[j] * (e * e);
      }
    }
    acc += d;
  }
  acc = wave_sum(acc);
  if (t == 0) p.ws[(long long)pair * kLpipsMaxBlocks + blockIdx.x] = acc;
}

__global__ void lpips_finish_kernel(const float* __restrict__ ws, float* __restrict__ out, int pairs, int blocks, int hw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pairs) return;
  float s = 0.0f;
  for (int b = 0; b < blocks; ++b) s += ws[(long long)i * kLpipsMaxBlocks + b];
  out[i] += s / (float)hw;
}

// ---------------------------------------------------------------------------------------------------------------------
// (x - shift) / scale per channel; one thread per pixel.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void image_normalize_kernel(const mobi_image_normalize_params p) {
  const long long total = (long long)p.batch * p.hw;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / p.hw, px = i % p.hw;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < p.channels; ++c) v[c] = (p.src[(n * p.channels + c) * p.hw + px] - p.shift[c]) / p.scale[c];
    if (p.nhwc_channels == 0) {
      float* o = reinterpret_cast<float*>(p.out);
      for (int c = 0; c < p.channels; ++c) o[(n * p.channels + c) * p.hw + px] = v[c];
    } else {
      T* o = reinterpret_cast<T*>(p.out) + i * p.nhwc_channels;
      float f[8] = {v[0], v[1], v[2], v[3], 0.0f, 0.0f, 0.0f, 0.0f};
      st16(o, pack8<T>(f));
      const float z[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      for (int c = 8; c < p.nhwc_channels; c += 8) st16(o + c, pack8<T>(z));
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Row cosine: one 256-thread block per row; the three sums reduced by waves, then across the four waves in order.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void row_cosine_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         float* __restrict__ out, int dim, float eps, float scale) {
  __shared__ float part[3][4];
  const long long row = blockIdx.x;
  const float* ra = a + row * dim;
  const float* rb = b + row * dim;
  float sab = 0.0f, saa = 0.0f, sbb = 0.0f;
  for (int d = threadIdx.x; d < dim; d += 256) {
    const float x = ra[d], y = rb[d];
    sab += x * y;
    saa += x * x;
    sbb += y * y;
  }
  sab = wave_sum(sab); saa = wave_sum(saa); sbb = wave_sum(sbb);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[0][wv] = sab; part[1][wv] = saa; part[2][wv] = sbb; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s[3];
    for (int k = 0; k < 3; ++k) s[k] = ((part[k][0] + part[k][1]) + part[k][2]) + part[k][3];
    const float na = fmaxf(sqrtf(s[1]), eps), nb = fmaxf(sqrtf(s[2]), eps);
    out[row] = scale * (s[0] / (na * nb));
  }
}

static inline unsigned rgrid(long long n) {
  long long g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace mobi

using namespace mobi;
#define ST(stream) reinterpret_cast<hipStream_t>(stream)

static inline bool misaligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) & 15; }

extern "C" int mobi_maxpool3s2(const void* src, void* out, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t relu,
                               int32_t dtype, void* stream) {
  if (!src || !out || batch <= 0 || h < 3 || w < 3 || c <= 0 || (relu != 0 && relu != 1)) return MOBI_ERR_ARG;
  if (dtype != MOBI_F16 && dtype != MOBI_BF16) return MOBI_ERR_ARG;
  if (c & 7) return MOBI_ERR_UNSUPPORTED;
  if (misaligned16(src) || misaligned16(out)) return MOBI_ERR_ALIGN;
  const long long total = (long long)batch * ((h - 3) / 2 + 1) * ((w - 3) / 2 + 1) * (c / 8);
  if (dtype == MOBI_F16)
    hipLaunchKernelGGL((maxpool3s2_kernel<f16_t>), dim3(rgrid(total)), dim3(256), 0, ST(stream),
                       static_cast<const f16_t*>(src), static_cast<f16_t*>(out), batch, h, w, c, relu);
  else
    hipLaunchKernelGGL((maxpool3s2_kernel<bf16_t>), dim3(rgrid(total)), dim3(256), 0, ST(stream),
                       static_cast<const bf16_t*>(src), static_cast<bf16_t*>(out), batch, h, w, c, relu);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" size_t mobi_lpips_distance_ws_floats(int32_t pairs, int32_t hw) {
  (void)hw;
  return pairs > 0 ? (size_t)pairs * kLpipsMaxBlocks : 0;
}

extern "C" int mobi_lpips_distance(const mobi_lpips_distance_params* p, void* stream) {
  if (!p || !p->feat || !p->lin || !p->out || !p->ws) return MOBI_ERR_ARG;
  if (p->pairs <= 0 || p->pairs > 65535 || p->hw <= 0 || p->channels <= 0 || !(p->eps >= 0.0f)) return MOBI_ERR_ARG;
  if (p->relu_in_place != 0 && p->relu_in_place != 1) return MOBI_ERR_ARG;
  if (p->dtype != MOBI_F16 && p->dtype != MOBI_BF16) return MOBI_ERR_ARG;
  if (p->channels & 7) return MOBI_ERR_UNSUPPORTED;
  if (misaligned16(p->feat) || misaligned16(p->lin)) return MOBI_ERR_ALIGN;
  const int blocks = lpips_blocks(p->hw);
  const dim3 grid(blocks, p->pairs);
  if (p->dtype == MOBI_F16) hipLaunchKernelGGL((lpips_distance_kernel<f16_t>), grid, dim3(64), 0, ST(stream), *p, blocks);
  else hipLaunchKernelGGL((lpips_distance_kernel<bf16_t>), grid, dim3(64), 0, ST(stream), *p, blocks);
  MOBI_CHECK_LAUNCH();
  hipLaunchKernelGGL(lpips_finish_kernel, dim3((p->pairs + 63) / 64), dim3(64), 0, ST(stream), p->ws, p->out, p->pairs, blocks,
                     p->hw);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_image_normalize(const mobi_image_normalize_params* p, void* stream) {
  if (!p || !p->src || !p->out || p->batch <= 0 || p->hw <= 0 || p->channels < 1 || p->channels > 4) return MOBI_ERR_ARG;
  if (p->nhwc_channels != 0) {
    if (p->dtype != MOBI_F16 && p->dtype != MOBI_BF16) return MOBI_ERR_ARG;
    if (p->nhwc_channels < p->channels || (p->nhwc_channels & 7)) return MOBI_ERR_UNSUPPORTED;
    if (misaligned16(p->out)) return MOBI_ERR_ALIGN;
  }
  for (int c = 0; c < p->channels; ++c)
    if (!(p->scale[c] != 0.0f)) return MOBI_ERR_ARG;
  const long long total = (long long)p->batch * p->hw;
  if (p->dtype == MOBI_BF16 && p->nhwc_channels)
    hipLaunchKernelGGL((image_normalize_kernel<bf16_t>), dim3(rgrid(total)), dim3(256), 0, ST(stream), *p);
  else
    hipLaunchKernelGGL((image_normalize_kernel<f16_t>), dim3(rgrid(total)), dim3(256), 0, ST(stream), *p);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_row_cosine(const float* a, const float* b, float* out, int32_t rows, int32_t dim, float eps, float scale,
                               void* stream) {
  if (!a || !b || !out || rows <= 0 || dim <= 0 || !(eps >= 0.0f)) return MOBI_ERR_ARG;
  hipLaunchKernelGGL(row_cosine_kernel, dim3(rows), dim3(256), 0, ST(stream), a, b, out, dim, eps, scale);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}
