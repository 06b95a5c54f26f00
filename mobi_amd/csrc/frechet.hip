// Fréchet realism metrics (include/mobi_engine.h, "Fréchet realism metrics"; mobi_amd/realism.py): the pieces of FID and FRD
// that are not convolutions or transformer layers -- the fp64 moments of a stream of feature batches, the RangeNet++ input
// (range view -> 5 channels at 64 x 1024) and the final band mean of RangeNet's last decoder stage (with its skip).
// RangeNet's 67 convolutions run on mobi_igemm (MOBI_EPI_LEAKY_RELU), CLIP's tower on the conditioning producer's launches.
// Built with -ffp-contract=off (mobi_amd/build.py): the depth arithmetic mirrors numpy's separate fp64 operations.
#include "common.h"

namespace mobi {

// ---------------------------------------------------------------------------------------------------------------------
// Moments: sum[i] += sum_r (x_ri - shift_i), cross[i][j] += sum_r (x_ri - shift_i)(x_rj - shift_j), fp64.  One thread per
// (i, j) of a 16 x 16 tile of `cross`; rows go through LDS 16 at a time and every thread adds them in ascending row order, so
// the result is one fixed sequence of fp64 operations per element: reproducible bit for bit, no atomics.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kMomTile = 16;

__global__ __launch_bounds__(256) void moments_cross_kernel(const float* __restrict__ x, int rows, int dim,
                                                            const double* __restrict__ shift, double* __restrict__ cross) {
  __shared__ double xi[kMomTile][kMomTile + 1], xj[kMomTile][kMomTile + 1];
  const int tx = threadIdx.x % kMomTile, ty = threadIdx.x / kMomTile;
  const int i0 = blockIdx.y * kMomTile, j0 = blockIdx.x * kMomTile;
  const int i = i0 + ty, j = j0 + tx;
  double acc = 0.0;
  for (int r0 = 0; r0 < rows; r0 += kMomTile) {
    // thread (ty, tx) stages row r0 + ty, columns i0 + tx and j0 + tx
    const int r = r0 + ty;
    double a = 0.0, b = 0.0;
    if (r < rows) {
      if (i0 + tx < dim) a = (double)x[(long long)r * dim + i0 + tx] - (shift ? shift[i0 + tx] : 0.0);
      if (j0 + tx < dim) b = (double)x[(long long)r * dim + j0 + tx] - (shift ? shift[j0 + tx] : 0.0);
    }
    xi[ty][tx] = a;
    xj[ty][tx] = b;
    __syncthreads();
    const int n = rows - r0 < kMomTile ? rows - r0 : kMomTile;
    for (int k = 0; k < n; ++k) acc += xi[k][ty] * xj[k][tx];
    __syncthreads();
  }
  if (i < dim && j < dim) cross[(long long)i * dim + j] += acc;
}

__global__ void moments_sum_kernel(const float* __restrict__ x, int rows, int dim, const double* __restrict__ shift,
                                   double* __restrict__ sum) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= dim) return;
  const double s = shift ? shift[i] : 0.0;
  double acc = 0.0;
  for (int r = 0; r < rows; ++r) acc += (double)x[(long long)r * dim + i] - s;
  sum[i] += acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// RangeNet++ input (eval_tool/lidar/frd_score.py RangePathDataset.__getitem__ + the model's input): one thread per output
// pixel.  depth = (d + 1) / 2 * dmax and the mask dmin < depth < dmax in fp64, the operations numpy performs (bit-exact
// mask); x, y, z from fp64 cos / sin; the five values rounded to f32 (the reference's .float()) and then to T; every
// channel -1 where the point is invalid; channels 5 .. cpad - 1 zero.  Nearest resize: source index dst * in / out (torch's
// floor(dst * scale) for the exact ratios of the range views).
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void frd_input_kernel(const float* __restrict__ raw, T* __restrict__ out, int batch, int h, int w, int hout,
                                 int wout, int cpad, double dmin, double dmax) {
  const long long total = (long long)batch * hout * wout;
  for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long long)gridDim.x * blockDim.x) {
    const int x = (int)(p % wout);
    const long long r = p / wout;
    const int y = (int)(r % hout);
    const long long n = r / hout;
    const int sy = (int)(((long long)y * h) / hout), sx = (int)(((long long)x * w) / wout);
    const long long plane = (long long)h * w, at = n * 4 * plane + (long long)sy * w + sx;
    const double d = (double)raw[at], inten = (double)raw[at + plane];
    const double pitch = (double)raw[at + 2 * plane], yaw = (double)raw[at + 3 * plane];
    const double depth = (d + 1.0) / 2.0 * dmax;
    const bool valid = depth > dmin && depth < dmax;
    float v[8] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
      const double cp = cos(pitch);
      v[0] = (float)depth;
      v[1] = (float)inten;
      v[2] = (float)(cos(yaw) * cp * depth);
      v[3] = (float)(-sin(yaw) * cp * depth);
      v[4] = (float)(sin(pitch) * depth);
    }
    T* o = out + p * cpad;
    st16(o, pack8<T>(v));
    const float z[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 8; c < cpad; c += 8) st16(o + c, pack8<T>(z));
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Band mean (Model.forward, return_final_logits, agg_type 'depth'): out[n][c * bands + b] = mean over the rows of band b and
// every column of (src + skip)[n][.][.][c], fp32.  One 256-thread block per (image, band); thread t sums channels
// 8 (t % G) .. + 7 (G = c / 8 channel groups) of pixels t / G, + 256 / G, ... in order; the partials of one channel group are
// then added in ascending thread order.  No atomics: reproducible bit for bit.
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void band_mean_kernel(const T* __restrict__ src, const T* __restrict__ skip,
                                                        float* __restrict__ out, int h, int w, int c, int bands) {
  __shared__ float part[256][9];
  const int n = blockIdx.y, band = blockIdx.x, t = threadIdx.x;
  const int G = c >> 3, g = t % G, step = 256 / G;
  const int rows = h / bands;
  const long long npx = (long long)rows * w;
  const long long base = ((long long)n * h + (long long)band * rows) * w * c;
  float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (long long px = t / G; px < npx; px += step) {
    float a[8];
    const long long off = base + px * c + 8 * g;
    unpack8<T>(ld16(src + off), a);
    if (skip) {
      float b[8];
      unpack8<T>(ld16(skip + off), b);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += b[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += a[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) part[t][j] = acc[j];
  __syncthreads();
  if (t < c) {
    const int gg = t >> 3, j = t & 7;
    float s = 0.0f;
    for (int k = gg; k < 256; k += G) s += part[k][j];
    out[(long long)n * c * bands + (long long)t * bands + band] = s / (float)npx;
  }
}

static inline unsigned fgrid(long long n) {
  long long g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

}  // namespace mobi

using namespace mobi;
#define ST(stream) reinterpret_cast<hipStream_t>(stream)

static inline bool misaligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) & 15; }

extern "C" int mobi_feature_moments(const float* feat, int32_t rows, int32_t dim, const double* shift, double* sum,
                                    double* cross, void* stream) {
  if (!feat || !sum || rows <= 0 || dim <= 0 || dim > 65535 * kMomTile) return MOBI_ERR_ARG;
  hipLaunchKernelGGL(moments_sum_kernel, dim3((dim + 255) / 256), dim3(256), 0, ST(stream), feat, rows, dim, shift, sum);
  MOBI_CHECK_LAUNCH();
  if (cross) {
    const int tiles = (dim + kMomTile - 1) / kMomTile;
    hipLaunchKernelGGL(moments_cross_kernel, dim3(tiles, tiles), dim3(256), 0, ST(stream), feat, rows, dim, shift, cross);
    MOBI_CHECK_LAUNCH();
  }
  return MOBI_OK;
}

extern "C" int mobi_frd_input(const float* raw, void* out, int32_t batch, int32_t h, int32_t w, int32_t hout, int32_t wout,
                              int32_t cpad, double depth_min, double depth_max, int32_t dtype, void* stream) {
  if (!raw || !out || batch <= 0 || h <= 0 || w <= 0 || hout <= 0 || wout <= 0 || !(depth_max > 0.0)) return MOBI_ERR_ARG;
  if (dtype != MOBI_F16 && dtype != MOBI_BF16) return MOBI_ERR_ARG;
  if (cpad < 8 || (cpad & 7)) return MOBI_ERR_UNSUPPORTED;
  if (misaligned16(out)) return MOBI_ERR_ALIGN;
  const long long total = (long long)batch * hout * wout;
  if (dtype == MOBI_F16)
    hipLaunchKernelGGL((frd_input_kernel<f16_t>), dim3(fgrid(total)), dim3(256), 0, ST(stream), raw, static_cast<f16_t*>(out),
                       batch, h, w, hout, wout, cpad, depth_min, depth_max);
  else
    hipLaunchKernelGGL((frd_input_kernel<bf16_t>), dim3(fgrid(total)), dim3(256), 0, ST(stream), raw, static_cast<bf16_t*>(out),
                       batch, h, w, hout, wout, cpad, depth_min, depth_max);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_band_mean(const void* src, const void* skip, float* out, int32_t batch, int32_t h, int32_t w, int32_t c,
                              int32_t bands, int32_t dtype, void* stream) {
  if (!src || !out || batch <= 0 || batch > 65535 || h <= 0 || w <= 0 || c <= 0 || bands <= 0 || h % bands) return MOBI_ERR_ARG;
  if (dtype != MOBI_F16 && dtype != MOBI_BF16) return MOBI_ERR_ARG;
  if ((c & 7) || c > 256 || 256 % (c >> 3)) return MOBI_ERR_UNSUPPORTED;      // channel groups must tile the 256 threads
  if (misaligned16(src) || misaligned16(skip)) return MOBI_ERR_ALIGN;
  const dim3 grid(bands, batch);
  if (dtype == MOBI_F16)
    hipLaunchKernelGGL((band_mean_kernel<f16_t>), grid, dim3(256), 0, ST(stream), static_cast<const f16_t*>(src),
                       static_cast<const f16_t*>(skip), out, h, w, c, bands);
  else
    hipLaunchKernelGGL((band_mean_kernel<bf16_t>), grid, dim3(256), 0, ST(stream), static_cast<const bf16_t*>(src),
                       static_cast<const bf16_t*>(skip), out, h, w, c, bands);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}
