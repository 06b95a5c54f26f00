// Harness post-processing on the device: what scripts/inference_test_bench.py and
// LatentDiffusion.log_data do with numpy / cv2 / torch-CPU after decoding, one D2H hop per sample today:
//   range view   un-crop of the 512 x 512 sample back into the 32 x 1096 sweep (avg-pool resize + wrap-around paste),
//                points-in-box instance mask of the predicted object, np.where paste          -> range_paste_kernel
//   metrics      avg / max pooled per-sample RMSE and (lower) median error over the object and mask regions,
//                written to a device table (one read-back per batch instead of ~100 .item() syncs) -> lidar_metrics_kernel
//   camera       bilinear patch resize + uint8 conversion + paste, 15 x 15 Gaussian blur of the mask
//                (BORDER_REFLECT_101), blend                                                  -> paste / blur / blend kernels
// Compiled with -ffp-contract=off: the fp32 expressions are evaluated in the reference's order without FMA fusion.
#include "common.h"

namespace mobi {

// avg_pool2d with kernel = stride = (kh, kw), as torch-CPU evaluates it: a sequential fp32 sum over the window in
// (row, column) order, then one division by the window size (lidar_converter.py:8-19 -> F.avg_pool2d)
__device__ __forceinline__ float avg_window(const float* img, int w, int y0, int x0, int kh, int kw) {
  float sum = 0.f;
  for (int dy = 0; dy < kh; ++dy)
    for (int dx = 0; dx < kw; ++dx) sum += img[(long long)(y0 + dy) * w + x0 + dx];
  return sum / (float)(kh * kw);
}
__device__ __forceinline__ float max_window(const float* img, int w, int y0, int x0, int kh, int kw) {
  float m = -INFINITY;
  for (int dy = 0; dy < kh; ++dy)
    for (int dx = 0; dx < kw; ++dx) m = fmaxf(m, img[(long long)(y0 + dy) * w + x0 + dx]);
  return m;
}

__global__ void range_paste_kernel(const mobi_range_paste_params a) {
  const long long per = (long long)a.h0 * a.w0;
  const long long total = (long long)a.batch * per;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / per);
    const int p = (int)(i - (long long)b * per);
    const int y = p / a.w0, x = p - y * a.w0;
    // LidarConverter.undo_default_transforms (lidar_converter.py:436-485): the crop window [crop_left, crop_left + wc)
    // wraps around the sweep; inside it the sample is avg-pooled from (hc, wc_in) to (h0, wc)
    // (the wrappers validate host-resident windows; a device-resident one is clamped to what the sample and the sweep
    // hold, and an empty one pastes nothing, rather than dividing by it)
    int wc = a.width_crop[b];
    wc = wc > a.wc ? a.wc : wc;
    wc = wc > a.w0 ? a.w0 : wc;
    int cl = a.crop_left[b] % a.w0;
    if (cl < 0) cl += a.w0;                                   // Python's % is non-negative
    int rel = x - cl;
    if (rel < 0) rel += a.w0;
    const bool inside = rel < wc;
    float d = a.depth_orig[i], it = a.int_orig ? a.int_orig[i] : 0.f;
    if (inside) {
      const int kh = a.hc / a.h0, kw = a.wc / wc;
      d = avg_window(a.sample_depth + (long long)b * a.hc * a.wc, a.wc, y * kh, rel * kw, kh, kw);
      if (a.sample_int) it = avg_window(a.sample_int + (long long)b * a.hc * a.wc, a.wc, y * kh, rel * kw, kh, kw);
    }
    if (a.depth_unc) a.depth_unc[i] = d;
    if (a.int_unc) a.int_unc[i] = it;
    if (!a.planes) continue;
    // LidarConverter.range2pcd (:122-172): metric depth, validity window, spherical -> Cartesian
    float dm = (d + 1.0f) / 2.0f;
    dm = dm * a.depth_max;
    const bool valid = dm > a.depth_min && dm < a.depth_max;
    const float yaw = a.yaw[i], pitch = a.pitch[i];
    const float cp = cosf(pitch);
    const float px = cosf(yaw) * cp * dm;
    const float py = -sinf(yaw) * cp * dm;
    const float pz = sinf(pitch) * dm;
    // points_in_convex_polygon_3d_jit (box_np_ops.py:736-771): inside iff every surface's sign is negative
    bool in_box = valid;
    const float* pl = a.planes + (long long)b * 24;
    for (int k = 0; k < 6 && in_box; ++k) {
      const float sign = px * pl[4 * k] + py * pl[4 * k + 1] + pz * pl[4 * k + 2] + pl[4 * k + 3];
      if (sign >= 0.f) in_box = false;
    }
    if (a.pred_mask) a.pred_mask[i] = in_box ? 1 : 0;
    const bool paste = in_box || (a.gt_mask && a.gt_mask[i] != 0);       // np.logical_or(pred, gt)
    if (a.depth_final) a.depth_final[i] = paste ? d : a.depth_orig[i];
    if (a.int_final) a.int_final[i] = paste ? it : (a.int_orig ? a.int_orig[i] : 0.f);
  }
}

// one block per (sample, region): region 0 = object (instance mask), 1 = inpainting mask
__global__ __launch_bounds__(1024) void lidar_metrics_kernel(const mobi_lidar_metrics_params a) {
  __shared__ float vals[16384];                              // absolute errors of the region (<= 32 x 512 cells), then sorted
  __shared__ unsigned n_vals;
  __shared__ double red[1024];
  const int b = blockIdx.x, region = blockIdx.y, tid = threadIdx.x;
  // (a device-resident window the wrapper could not validate: clamped to the sort space the launch was sized for;
  // an empty one selects no cell -> NaN, NaN, 0)
  int wc = a.width_crop[b];
  wc = wc > a.max_width ? a.max_width : wc;
  const int kh = a.h / a.pool_h, kw = wc > 0 ? a.w / wc : 1;
  const int cells = wc > 0 ? a.pool_h * wc : 0;
  const float* pred = a.pred + (long long)b * a.h * a.w;
  const float* gt = a.gt + (long long)b * a.h * a.w;
  const float* msk = (region == 0 ? a.inst_mask : a.box_mask) + (long long)b * a.h * a.w;
  if (tid == 0) n_vals = 0;
  __syncthreads();
  double sq = 0.0;
  for (int c = tid; c < cells; c += blockDim.x) {
    const int y = c / wc, x = c - y * wc;
    if (max_window(msk, a.w, y * kh, x * kw, kh, kw) != 1.0f) continue;      // `mask_ == 1` after max pooling
    const float e = avg_window(pred, a.w, y * kh, x * kw, kh, kw) - avg_window(gt, a.w, y * kh, x * kw, kh, kw);
    sq += (double)e * (double)e;
    vals[atomicAdd(&n_vals, 1u)] = fabsf(e);
  }
  red[tid] = sq;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {                        // fixed-order tree: deterministic
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const unsigned n = n_vals;
  unsigned cap = 1;
  while (cap < n) cap <<= 1;
  for (unsigned i = n + tid; i < cap; i += blockDim.x) vals[i] = INFINITY;
  __syncthreads();
  for (unsigned k = 2; k <= cap; k <<= 1)                    // bitonic sort (ascending)
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      for (unsigned i = tid; i < cap; i += blockDim.x) {
        const unsigned l = i ^ j;
        if (l > i) {
          const float x = vals[i], y = vals[l];
          const bool up = (i & k) == 0;
          if ((x > y) == up) { vals[i] = y; vals[l] = x; }
        }
      }
      __syncthreads();
    }
  if (tid == 0) {
    float* o = a.out + ((long long)b * 2 + region) * 3;
    o[0] = n ? (float)sqrt(red[0] / (double)n) : NAN;        // (((pred - gt) ** 2).mean() ** 0.5), ddpm.py:1576-1584
    o[1] = n ? vals[(n - 1) >> 1] : NAN;                     // torch.median: the lower of the two middle values
    o[2] = (float)n;
  }
}

// F.interpolate(patch, (crop_h, crop_w), mode="bilinear") [align_corners=False], then the harness's
// (((x + 1) / 2) * 255).astype(uint8) in BGR order, written into the frame at (top, left)
__global__ void paste_patch_kernel(const float* patch, int hs, int ws, unsigned char* frame, int H, int W, int top,
                                   int left, int crop_h, int crop_w) {
  const float sy = (float)hs / (float)crop_h, sx = (float)ws / (float)crop_w;
  const long long total = (long long)crop_h * crop_w;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int y = (int)(i / crop_w), x = (int)(i - (long long)y * crop_w);
    const int fy = top + y, fx = left + x;
    if (fy < 0 || fy >= H || fx < 0 || fx >= W) continue;
    float syf = sy * ((float)y + 0.5f) - 0.5f;
    if (syf < 0.f) syf = 0.f;
    float sxf = sx * ((float)x + 0.5f) - 0.5f;
    if (sxf < 0.f) sxf = 0.f;
    const int y0 = (int)syf, x0 = (int)sxf;
    const int y1 = y0 + (y0 < hs - 1 ? 1 : 0), x1 = x0 + (x0 < ws - 1 ? 1 : 0);
    const float ly = syf - (float)y0, lx = sxf - (float)x0;
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    for (int c = 0; c < 3; ++c) {
      const float* pc = patch + (long long)c * hs * ws;
      const float v = hy * (hx * pc[(long long)y0 * ws + x0] + lx * pc[(long long)y0 * ws + x1]) +
                      ly * (hx * pc[(long long)y1 * ws + x0] + lx * pc[(long long)y1 * ws + x1]);
      float u = ((v + 1.0f) / 2.0f) * 255.0f;
      u = u < 0.f ? 0.f : (u > 255.f ? 255.f : u);           // (astype wraps out-of-range values; the sample is clamped to [-1, 1])
      frame[((long long)fy * W + fx) * 3 + (2 - c)] = (unsigned char)(int)u;     // RGB plane c -> BGR byte 2 - c
    }
  }
}

// one pass of the separable blur along x (horizontal = 1) or y; BORDER_REFLECT_101: index -i -> i, n - 1 + i -> n - 1 - i
__global__ void blur_pass_kernel(const float* src, float* dst, int H, int W, const float* kern, int ksize, int horizontal) {
  const int r = ksize >> 1;
  const long long total = (long long)H * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const int n = horizontal ? W : H, p = horizontal ? x : y;
    float acc = 0.f;
    for (int k = 0; k < ksize; ++k) {
      int q = p + k - r;
      if (n == 1) q = 0;
      else {
        while (q < 0 || q >= n) q = q < 0 ? -q : 2 * (n - 1) - q;
      }
      acc += kern[k] * (horizontal ? src[(long long)y * W + q] : src[(long long)q * W + x]);
    }
    dst[i] = acc;
  }
}

// image_recon = m * image_u8 + (1 - m) * image_pred  (inference_test_bench.py:508-509); image: f32 [3][H][W] RGB in
// [-1, 1] (converted to uint8 BGR as the harness does), pred: u8 [H][W][3] BGR, out: f32 [H][W][3] BGR
__global__ void blend_kernel(const float* mask_blur, const float* image, const unsigned char* pred, float* out, int H,
                             int W) {
  const long long total = (long long)H * W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const float m = mask_blur[i];
    for (int c = 0; c < 3; ++c) {
      float u = ((image[(long long)(2 - c) * total + i] + 1.0f) / 2.0f) * 255.0f;
      u = u < 0.f ? 0.f : (u > 255.f ? 255.f : u);
      const float iu = (float)(unsigned char)(int)u;
      out[i * 3 + c] = m * iu + (1.0f - m) * (float)pred[i * 3 + c];
    }
  }
}

static inline int egrid_pp(long long n) {
  long long b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}


// ---------------------------------------------------------------------------------------------------------
// Dataset side, one launch per batch (ldm/data/nuscenes.py:418-470 with lidar_converter.py:387-434): the object's view
// of the sweep -- three sweeps side by side, a window of width_crop columns from column crop_left, nearest-neighbour
// resize to (height, width) -- then the depth / intensity normalisation and the edit-mask product.  The tiled array
// is never built: column (crop_left + sx) mod w0 of the sweep is the same pixel.  Nearest index as OpenCV's resizeNN:
// min(floor(d * (1 / (dst / src))), src - 1) in double.  Float expressions in the reference's operation order
// (this file is compiled without FMA contraction).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void range_prepare_kernel(const mobi_range_prepare_params a) {
  const long long total = (long long)a.batch * a.height * a.width;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % a.width);
    const int r = (int)((i / a.width) % a.height);
    const int b = (int)(i / ((long long)a.width * a.height));
    const int wc = a.width_crop[b];
    int sy = (int)floor((double)r * (1.0 / ((double)a.height / (double)a.h0)));
    int sx = (int)floor((double)c * (1.0 / ((double)a.width / (double)wc)));
    sy = sy < a.h0 - 1 ? sy : a.h0 - 1;
    sx = sx < wc - 1 ? sx : wc - 1;
    int col = (a.crop_left[b] + sx) % a.w0;
    if (col < 0) col += a.w0;
    const long long src = ((long long)b * a.h0 + sy) * a.w0 + col;
    float d = a.depth_orig[src];
    if (a.object_norm) {
      const float lo = a.min_depth[b], hi = a.max_depth[b], al = a.alpha;
      const float two_al = (float)(2.0 * (double)a.alpha), rest = (float)(-((double)a.alpha - 1.0)), rest_hi = (float)(1.0 - (double)a.alpha);
      float o = 0.f;
      if (d >= lo && d <= hi) o = -al + (two_al * (d - lo)) / (hi - lo);
      else if (d >= -1.f && d < lo) o = -1.f + (rest * (d + 1.f)) / (lo + 1.f);
      else if (d > hi && d <= 1.f) o = al + (rest_hi * (d - hi)) / (1.f - hi);
      d = o;
    }
    float v = ((a.int_orig[src] / 255.f) - 0.5f) * 2.f;
    if (a.int_norm) {
      v = 1.f - expf(-2.f * (v + 1.f));
      v = 2.f * v - 1.f;
      v = v < -1.f ? -1.f : (v > 1.f ? 1.f : v);
    }
    const long long hw = (long long)a.height * a.width, px = (long long)r * a.width + c;
    const float m = a.edit_mask[b * hw + px];
    a.range_data[(b * 2 + 0) * hw + px] = d;
    a.range_data[(b * 2 + 1) * hw + px] = v;
    a.range_data_inpaint[(b * 2 + 0) * hw + px] = d * m;
    a.range_data_inpaint[(b * 2 + 1) * hw + px] = v * m;
    if (a.inst_out) a.inst_out[b * hw + px] = a.inst_orig[src];
  }
}

// Edit region of a projected box (ldm/data/utils.py:146-198; cv2.fillPoly restated, see
// mobi_amd/ldm/data/utils.py:fill_box_faces): a pixel belongs to it when its centre is inside one of the six faces
// (integer corner coordinates) or within half a pixel of a face's outline.  Double arithmetic, the host restatement's
// own expressions.
__device__ __forceinline__ bool in_box_faces(const int* __restrict__ q, int x, int y) {
  const int FACES[6][4] = {{0, 1, 2, 3}, {4, 5, 6, 7}, {0, 1, 5, 4}, {2, 3, 7, 6}, {0, 4, 7, 3}, {1, 5, 6, 2}};
  for (int f = 0; f < 6; ++f) {
    double px[4], py[4];
    for (int k = 0; k < 4; ++k) { px[k] = (double)q[FACES[f][k] * 2]; py[k] = (double)q[FACES[f][k] * 2 + 1]; }
    bool pos = true, neg = true, near = false;
    double lox = px[0], hix = px[0], loy = py[0], hiy = py[0];
    for (int k = 1; k < 4; ++k) {
      lox = px[k] < lox ? px[k] : lox; hix = px[k] > hix ? px[k] : hix;
      loy = py[k] < loy ? py[k] : loy; hiy = py[k] > hiy ? py[k] : hiy;
    }
    if ((double)x < lox - 1 || (double)x > hix + 1 || (double)y < loy - 1 || (double)y > hiy + 1) continue;
    const bool box = (double)x >= lox && (double)x <= hix && (double)y >= loy && (double)y <= hiy;
    for (int k = 0; k < 4; ++k) {
      const double ax = px[k], ay = py[k], ex = px[(k + 1) & 3] - ax, ey = py[(k + 1) & 3] - ay;
      const double cross = ex * ((double)y - ay) - ey * ((double)x - ax);
      pos = pos && cross >= 0; neg = neg && cross <= 0;
      const double ll = ex * ex + ey * ey;
      double t = ll > 0 ? (((double)x - ax) * ex + ((double)y - ay) * ey) / ll : 0.0;
      t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
      const double dx = (double)x - (ax + t * ex), dy = (double)y - (ay + t * ey);
      near = near || dx * dx + dy * dy <= 0.25;
    }
    if (((pos || neg) && box) || near) return true;
  }
  return false;
}

// out = 0 inside the edit region, 1 elsewhere; stats (optional): per box {pixels inside, min x, max x, min y, max y},
// pre-set by the caller to {0, W, -1, H, -1}
__global__ __launch_bounds__(256) void box_mask_kernel(const int* __restrict__ corners_xy, float* __restrict__ out,
                                                        int* __restrict__ stats, int batch, int H, int W) {
  const long long per = (long long)H * W;
  const int b = blockIdx.y;
  const int* q = corners_xy + (long long)b * 16;
  int cnt = 0, lox = W, hix = -1, loy = H, hiy = -1;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % W), y = (int)(i / W);
    const bool hit = in_box_faces(q, x, y);
    if (out) out[b * per + i] = hit ? 0.f : 1.f;
    if (hit) { ++cnt; lox = x < lox ? x : lox; hix = x > hix ? x : hix; loy = y < loy ? y : loy; hiy = y > hiy ? y : hiy; }
  }
  if (stats) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cnt += __shfl_xor(cnt, o, 64);
      const int a = __shfl_xor(lox, o, 64), c = __shfl_xor(hix, o, 64), d = __shfl_xor(loy, o, 64), e = __shfl_xor(hiy, o, 64);
      lox = a < lox ? a : lox; hix = c > hix ? c : hix; loy = d < loy ? d : loy; hiy = e > hiy ? e : hiy;
    }
    if ((threadIdx.x & 63) == 0 && cnt) {
      atomicAdd(stats + b * 5, cnt);
      atomicMin(stats + b * 5 + 1, lox); atomicMax(stats + b * 5 + 2, hix);
      atomicMin(stats + b * 5 + 3, loy); atomicMax(stats + b * 5 + 4, hiy);
    }
  }
}

// Camera side of a batch in one launch (ldm/data/nuscenes.py:495-594): frame pixels ((u8 / 255) - 0.5) / 0.5, the edit
// mask evaluated at the source pixels, both cropped to (left, top, crop_w, crop_h) and resized to (height, width) as
// torchvision 0.11's tensor Resize does (F.interpolate bilinear, align_corners=False, no antialias);
// GT = image, inpaint_image = image * mask.  invert[b]: the mask had no edit pixel and was flipped (:513-515).
__global__ __launch_bounds__(256) void image_prepare_kernel(const mobi_image_prepare_params a) {
  const long long hw = (long long)a.height * a.width, total = (long long)a.batch * hw;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int x = (int)(i % a.width), y = (int)((i / a.width) % a.height), b = (int)(i / hw);
    const int left = a.crop[b * 4], top = a.crop[b * 4 + 1], cw = a.crop[b * 4 + 2], ch = a.crop[b * 4 + 3];
    const float sy = (float)ch / (float)a.height, sx = (float)cw / (float)a.width;
    float fy = sy * ((float)y + 0.5f) - 0.5f, fx = sx * ((float)x + 0.5f) - 0.5f;
    fy = fy < 0.f ? 0.f : fy; fx = fx < 0.f ? 0.f : fx;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < ch - 1 ? 1 : 0), x1 = x0 + (x0 < cw - 1 ? 1 : 0);
    const float ly1 = fy - (float)y0, lx1 = fx - (float)x0, ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const unsigned char* fr = a.frames + (long long)b * a.H * a.W * 3;
    const int* q = a.corners_xy + (long long)b * 16;
    const int Y[2] = {top + y0, top + y1}, X[2] = {left + x0, left + x1};
    float m[2][2];
    for (int r = 0; r < 2; ++r)
      for (int c = 0; c < 2; ++c) {
        const bool hit = in_box_faces(q, X[c], Y[r]);
        m[r][c] = (hit != (a.invert[b] != 0)) ? 0.f : 1.f;
      }
    const float mk = ly0 * (lx0 * m[0][0] + lx1 * m[0][1]) + ly1 * (lx0 * m[1][0] + lx1 * m[1][1]);
    a.mask[b * hw + (long long)y * a.width + x] = mk;
    for (int ch3 = 0; ch3 < 3; ++ch3) {
      float v[2][2];
      for (int r = 0; r < 2; ++r)
        for (int c = 0; c < 2; ++c) {
          const float u = (float)fr[((long long)Y[r] * a.W + X[c]) * 3 + ch3] / 255.f;
          v[r][c] = (u - 0.5f) / 0.5f;
        }
      const float g = ly0 * (lx0 * v[0][0] + lx1 * v[0][1]) + ly1 * (lx0 * v[1][0] + lx1 * v[1][1]);
      const long long o = ((long long)b * 3 + ch3) * hw + (long long)y * a.width + x;
      a.gt[o] = g;
      a.inpaint[o] = g * mk;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Reference-image augmentation of a batch in one launch (ldm/data/nuscenes.py:239-250: albumentations 0.4.3
// HorizontalFlip -> Rotate(border_mode=0) -> Blur -> RandomBrightnessContrast on the resized uint8 patch, then
// get_tensor_clip), every stage on or off per sample.  Integer arithmetic up to the table look-up, the expressions of
// mobi_amd/ldm/data/ref_aug.py (the host builds the warp tables and the [3][256] output table).
// One block per 32 x 32 output tile: the flipped / rotated tile with a halo of the blur radius goes to LDS as one
// packed dword per pixel (r | g << 8 | b << 16), one barrier, then the box sums are taken from LDS.
// ---------------------------------------------------------------------------------------------------------
constexpr int RA_TILE = 32, RA_HALO = 3, RA_SIDE = RA_TILE + 2 * RA_HALO;

// pixel (y, x) of the flipped patch, 0 outside it
__device__ __forceinline__ unsigned ra_source(const unsigned char* __restrict__ img, int S, int flip, int y, int x) {
  if ((unsigned)y >= (unsigned)S || (unsigned)x >= (unsigned)S) return 0u;
  const unsigned char* p = img + ((long long)y * S + (flip ? S - 1 - x : x)) * 3;
  return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}

// pixel (y, x), 0 <= y, x < S, of the flipped and rotated patch
__device__ __forceinline__ unsigned ra_rotated(const unsigned char* __restrict__ img, const int* __restrict__ warp, int S,
                                               int flip, int rotate, int y, int x) {
  if (!rotate) return ra_source(img, S, flip, y, x);
  const int X = (warp[2 * S + y] + warp[x]) >> 5, Y = (warp[3 * S + y] + warp[S + x]) >> 5;
  const int sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31;
  const unsigned w00 = (32 - fy) * (32 - fx), w01 = (32 - fy) * fx, w10 = fy * (32 - fx), w11 = fy * fx;
  const unsigned p00 = ra_source(img, S, flip, sy, sx), p01 = ra_source(img, S, flip, sy, sx + 1);
  const unsigned p10 = ra_source(img, S, flip, sy + 1, sx), p11 = ra_source(img, S, flip, sy + 1, sx + 1);
  unsigned out = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int sh = 8 * c;
    const unsigned v = (w00 * ((p00 >> sh) & 255u) + w01 * ((p01 >> sh) & 255u) + w10 * ((p10 >> sh) & 255u) +
                        w11 * ((p11 >> sh) & 255u) + 512u) >> 10;
    out |= v << sh;
  }
  return out;
}

// box sums of side 2 R + 1 around tile pixel (ly, lx): r and b in the 16-bit halves of one word (49 * 255 < 2^16), g apart
template <int R>
__device__ __forceinline__ void ra_box(const unsigned* __restrict__ tile, int ly, int lx, unsigned& r, unsigned& g, unsigned& b) {
  unsigned rb = 0, gg = 0;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy)
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      const unsigned v = tile[(ly + RA_HALO + dy) * RA_SIDE + lx + RA_HALO + dx];
      rb += v & 0x00ff00ffu;
      gg += (v >> 8) & 255u;
    }
  constexpr unsigned K2 = (2 * R + 1) * (2 * R + 1);
  r = (2 * (rb & 0xffffu) + K2) / (2 * K2);
  g = (2 * gg + K2) / (2 * K2);
  b = (2 * (rb >> 16) + K2) / (2 * K2);
}

__global__ __launch_bounds__(256) void ref_augment_kernel(const mobi_ref_augment_params a) {
  __shared__ unsigned tile[RA_SIDE * RA_SIDE];
  __shared__ float table[3 * 256];
  const int S = a.size, b = blockIdx.z, ty0 = blockIdx.y * RA_TILE, tx0 = blockIdx.x * RA_TILE;
  const int flip = a.flags[b * 2] & 1, rotate = (a.flags[b * 2] >> 1) & 1;
  int rad = a.flags[b * 2 + 1] >> 1;                                    // box side 0 (off) | 3 | 5 | 7 -> radius 0 .. 3
  rad = rad < 0 ? 0 : (rad > RA_HALO ? RA_HALO : rad);
  const unsigned char* img = a.src + (long long)b * S * S * 3;
  const int* warp = a.warp + (long long)b * 4 * S;
  for (int i = threadIdx.x; i < 3 * 256; i += 256) table[i] = a.table[(long long)b * 3 * 256 + i];
  const int side = RA_TILE + 2 * rad;
  for (int i = threadIdx.x; i < side * side; i += 256) {
    const int py = i / side - rad, px = i % side - rad;                // tile-relative, -rad .. 31 + rad
    int y = ty0 + py, x = tx0 + px;
    unsigned v = 0;
    if (y < S + rad && x < S + rad) {                                   // (beyond: no output pixel of the patch reads it)
      y = y < 0 ? -y : (y >= S ? 2 * S - 2 - y : y);                    // BORDER_REFLECT_101 (S >= 8 > rad)
      x = x < 0 ? -x : (x >= S ? 2 * S - 2 - x : x);
      v = ra_rotated(img, warp, S, flip, rotate, y, x);
    }
    tile[(py + RA_HALO) * RA_SIDE + px + RA_HALO] = v;
  }
  __syncthreads();
  const long long plane = (long long)S * S;
  float* out = a.out + (long long)b * 3 * plane;
  for (int i = threadIdx.x; i < RA_TILE * RA_TILE; i += 256) {
    const int ly = i / RA_TILE, lx = i % RA_TILE, y = ty0 + ly, x = tx0 + lx;
    if (y >= S || x >= S) continue;
    unsigned r, g, bl;
    if (rad == 1) ra_box<1>(tile, ly, lx, r, g, bl);
    else if (rad == 2) ra_box<2>(tile, ly, lx, r, g, bl);
    else if (rad == 3) ra_box<3>(tile, ly, lx, r, g, bl);
    else ra_box<0>(tile, ly, lx, r, g, bl);
    const long long o = (long long)y * S + x;
    out[o] = table[r];
    out[plane + o] = table[256 + g];
    out[2 * plane + o] = table[512 + bl];
  }
}

// Context drop of the flagged samples (ldm/data/nuscenes.py:463-466 / :588-591): inpaint = 0, gt = gt * (1 - mask), the mask
// [batch][1][hw] broadcast over the channels; two fp32 operations as torch computes them (no contraction in this file).
__device__ __forceinline__ float dc_keep(float v, float m) { return v * (1.0f - m); }
__device__ __forceinline__ float4 dc_keep(float4 v, float4 m) {
  return make_float4(dc_keep(v.x, m.x), dc_keep(v.y, m.y), dc_keep(v.z, m.z), dc_keep(v.w, m.w));
}
__device__ __forceinline__ void dc_zero(float& z) { z = 0.0f; }
__device__ __forceinline__ void dc_zero(float4& z) { z = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

template <typename V>                                                    // V = float4 (hw % 4 == 0, aligned) | float
__global__ __launch_bounds__(256) void drop_context_kernel(float* __restrict__ gt, float* __restrict__ inpaint,
                                                            const float* __restrict__ mask, const int* __restrict__ flag,
                                                            int channels, long long hw) {
  const int b = blockIdx.y;
  if (!flag[b]) return;
  const long long nv = hw / (long long)(sizeof(V) / sizeof(float));
  V zero;
  dc_zero(zero);
  const V* m = reinterpret_cast<const V*>(mask + b * hw);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long long)gridDim.x * 256) {
    const V keep = m[i];
    for (int c = 0; c < channels; ++c) {
      const long long plane = ((long long)b * channels + c) * hw;
      V* g = reinterpret_cast<V*>(gt + plane) + i;
      *g = dc_keep(*g, keep);
      reinterpret_cast<V*>(inpaint + plane)[i] = zero;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// The image logger's pictures (main.py:353-370: make_grid(nrow), (g + 1) / 2, two transposes, * 255, astype(uint8) per key):
// every key of a log dict in one launch.  blockIdx.y = the source, so its table entry -- part of the launch's argument block --
// is read with scalar loads; a thread writes one dword (4 bytes, 1 1/3 pixels) of the source's HWC picture, a plain gather.
// ---------------------------------------------------------------------------------------------------------
constexpr int IG_MAX_SOURCES = 16;
struct ig_entry {
  const void* data;
  int n, c, h, w;                                            // n: images used (<= max_images)
  int hg, wg, xmaps, is_u8;
  long long out_offset;
};
struct ig_table {
  ig_entry e[IG_MAX_SOURCES];
  int padding, clamp, rescale;
};

// byte gb of the picture [hg][wg][3] of source s.  The canvas between and around the cells holds the SOURCE value 0, as make_grid
// fills it, and goes through the same conversion as the images: 127 in a rescaled fp32 picture (the reference's grey frame), else 0.
__device__ __forceinline__ unsigned ig_byte(const ig_entry& s, int padding, int clamp, int rescale, int gb) {
  const int pix = gb / 3, ch = gb - pix * 3;
  int y = pix / s.wg, x = pix - y * s.wg, k = 0;
  bool inside = true;
  if (s.n > 1) {                                             // (one image: the picture is the image)
    const int cell_h = s.h + padding, cell_w = s.w + padding;
    y -= padding;
    x -= padding;
    const int cy = y / cell_h, cx = x / cell_w;
    y -= cy * cell_h;
    x -= cx * cell_w;
    k = cy * s.xmaps + cx;
    inside = y >= 0 && x >= 0 && y < s.h && x < s.w && k < s.n;    // not: the frame, the gaps, the cells past the last image
  }
  const long long i = (((long long)k * s.c + (s.c == 3 ? ch : 0)) * s.h + y) * s.w + x;
  if (s.is_u8) return inside ? (unsigned)static_cast<const unsigned char*>(s.data)[i] : 0u;
  float v = inside ? static_cast<const float*>(s.data)[i] : 0.0f;
  if (clamp) v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
  if (rescale) v = (v + 1.0f) / 2.0f;
  v = v * 255.0f;
  return (unsigned)(int)v & 255u;                            // astype(uint8): towards zero, the low 8 bits
}

__global__ __launch_bounds__(256) void image_grid_kernel(const ig_table t, unsigned char* __restrict__ out) {
  const ig_entry& s = t.e[blockIdx.y];
  const int bytes = s.hg * s.wg * 3, words = (bytes + 3) >> 2;
  unsigned char* dst = out + s.out_offset;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < words; i += gridDim.x * 256) {
    const int b0 = i * 4;
    if (b0 + 3 < bytes) {
      unsigned word = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) word |= ig_byte(s, t.padding, t.clamp, t.rescale, b0 + j) << (8 * j);
      reinterpret_cast<unsigned*>(dst)[i] = word;
    } else {
      for (int b = b0; b < bytes; ++b) dst[b] = (unsigned char)ig_byte(s, t.padding, t.clamp, t.rescale, b);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// The test bench's camera pictures of a sampled batch (scripts/inference_test_bench.py:478-527) in one launch: per object the
// recomposed frame, its crop window, the resized ground-truth patch, the object crop of the pasted prediction at 224 x 224 and
// the un-normalised reference image, all HWC uint8 RGB in one buffer (include/mobi_engine.h, mobi_camera_export).
// blockIdx.y = the object; a block walks that object's 64 x 32 pixel tiles, of four kinds, and leaves each tile's bytes in LDS,
// from where whole rows go out as dwords (single bytes only up to a row's first and after its last 4-byte boundary).
// The blend tile holds the mask with its 7-pixel halo in LDS and takes both blur passes from there.  The expressions are those
// of paste_patch_kernel / blur_pass_kernel / blend_kernel above; this file is compiled without FMA contraction.
// The copy-paste baseline (mobi_camera_copy_paste) is a second kernel over the same walk and the same tile bodies, templated on
// the mode: the mask dilated 5 x 5 in place of the blur, the reference resized onto the mask's box in pred.
// ---------------------------------------------------------------------------------------------------------
constexpr int CE_TW = 64, CE_TH = 32, CE_R = 7, CE_K = 15;
constexpr int CE_MW = CE_TW + 16, CE_MH = CE_TH + 2 * CE_R;          // mask tile: columns x0 - 8 .. x0 + 71, rows y0 - 7 .. y0 + 38
constexpr int CE_OBW = CE_TW * 3;
constexpr int CE_MAX_OBJECTS = 32, CE_BOX_PARTS = 64, CE_REF = 224;
constexpr int CE_EXPORT = 0, CE_COPY_PASTE = 1, CE_DR = 2;  // the two modes of the export launch; the 5 x 5 dilation's radius
struct ce_object {
  int left, top, cw, ch;
  long long off[5];                                          // frame, patch_pred, patch_gt, object_pred, object_ref
};
struct ce_table { ce_object o[CE_MAX_OBJECTS]; };
struct ce_args {
  const float* patch_pred; const float* patch_gt; const float* ref; const float* image; const float* mask; const float* taps;
  int* box_ws; unsigned char* out; int* status;
  int hs, ws, H, W, frames;
};

// rows / columns of the pixels with 1 - mask != 0: block (j, b) reduces its stripe of rows to {min x, max x, min y, max y}
// (W, -1, H, -1 when it has none); the export launch folds an object's CE_BOX_PARTS records.  No atomics, nothing to pre-set.
__global__ __launch_bounds__(256) void camera_box_kernel(const float* __restrict__ mask, int* __restrict__ box_ws, int H, int W) {
  __shared__ int part[4][4];
  const int b = blockIdx.y, rows = (H + CE_BOX_PARTS - 1) / CE_BOX_PARTS;
  const int r0 = blockIdx.x * rows, r1 = r0 + rows < H ? r0 + rows : H;
  const float* m = mask + (long long)b * H * W;
  int lox = W, hix = -1, loy = H, hiy = -1;
  const long long i0 = (long long)r0 * W, i1 = (long long)(r1 > r0 ? r1 : r0) * W;
  for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
    if (1.0f - m[i] != 0.0f) {
      const int y = (int)(i / W), x = (int)(i - (long long)y * W);
      lox = x < lox ? x : lox; hix = x > hix ? x : hix; loy = y < loy ? y : loy; hiy = y > hiy ? y : hiy;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int a = __shfl_xor(lox, o, 64), c = __shfl_xor(hix, o, 64), d = __shfl_xor(loy, o, 64), e = __shfl_xor(hiy, o, 64);
    lox = a < lox ? a : lox; hix = c > hix ? c : hix; loy = d < loy ? d : loy; hiy = e > hiy ? e : hiy;
  }
  if ((threadIdx.x & 63) == 0) {
    int* p = part[threadIdx.x >> 6];
    p[0] = lox; p[1] = hix; p[2] = loy; p[3] = hiy;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      lox = part[w][0] < lox ? part[w][0] : lox; hix = part[w][1] > hix ? part[w][1] : hix;
      loy = part[w][2] < loy ? part[w][2] : loy; hiy = part[w][3] > hiy ? part[w][3] : hiy;
    }
    int* o = box_ws + ((long long)b * CE_BOX_PARTS + blockIdx.x) * 4;
    o[0] = lox; o[1] = hix; o[2] = loy; o[3] = hiy;
  }
}

__device__ __forceinline__ int ce_reflect(int q, int n) {    // BORDER_REFLECT_101, as blur_pass_kernel
  if (n == 1) return 0;
  while (q < 0 || q >= n) q = q < 0 ? -q : 2 * (n - 1) - q;
  return q;
}

// source taps of output index d of the align_corners = False resize, as paste_patch_kernel
__device__ __forceinline__ void ce_taps(float scale, int d, int n, int& i0, int& i1, float& l) {
  float f = scale * ((float)d + 0.5f) - 0.5f;
  if (f < 0.f) f = 0.f;
  i0 = (int)f;
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
  l = f - (float)i0;
}

// P: one channel of the resized patch as a byte value, as paste_patch_kernel
__device__ __forceinline__ int ce_patch_byte(const float* __restrict__ pc, int ws, int y0, int y1, int x0, int x1, float ly,
                                             float lx) {
  const float hy = 1.0f - ly, hx = 1.0f - lx;
  const float v = hy * (hx * pc[(long long)y0 * ws + x0] + lx * pc[(long long)y0 * ws + x1]) +
                  ly * (hx * pc[(long long)y1 * ws + x0] + lx * pc[(long long)y1 * ws + x1]);
  float u = ((v + 1.0f) / 2.0f) * 255.0f;
  u = u < 0.f ? 0.f : (u > 255.f ? 255.f : u);
  return (int)u;
}

// rows [ry0, ry1) x columns [rx0, rx1) of the tile at (tx0, ty0) -> the picture at dst whose pixel (0, 0) is (ox, oy) of the
// same coordinates and whose rows are `pitch` bytes; dst is 4-byte aligned.  One wave per row, at most 48 dwords.
__device__ __forceinline__ void ce_store(const unsigned char* ob, int tx0, int ty0, int rx0, int ry0, int rx1, int ry1,
                                         unsigned char* dst, long long pitch, int ox, int oy) {
  if (rx1 <= rx0) return;
  const int lane = threadIdx.x & 63, nb = (rx1 - rx0) * 3;
  for (int y = ry0 + (threadIdx.x >> 6); y < ry1; y += 4) {
    const unsigned char* src = ob + (y - ty0) * CE_OBW + (rx0 - tx0) * 3;
    const long long g0 = (long long)(y - oy) * pitch + (long long)(rx0 - ox) * 3;
    int head = (int)((4 - (g0 & 3)) & 3);
    head = head > nb ? nb : head;
    const int ndw = (nb - head) >> 2, tail = nb - head - ndw * 4;
    if (lane < ndw) {
      const unsigned char* s = src + head + lane * 4;
      const unsigned word = (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16) | ((unsigned)s[3] << 24);
      *reinterpret_cast<unsigned*>(dst + g0 + head + lane * 4) = word;
    } else if (lane >= 56 && lane < 56 + head) {
      dst[g0 + (lane - 56)] = src[lane - 56];
    } else if (lane >= 60 && lane < 60 + tail) {
      const int k = head + ndw * 4 + (lane - 60);
      dst[g0 + k] = src[k];
    }
  }
}

// taps of OpenCV's 8-bit INTER_LINEAR resize (ldm/data/nuscenes.py:resize_linear_u8): position in fp64, every operation
// rounded on its own, the fraction rounded to fp32, 11-bit integer weights
__device__ __forceinline__ void ce_cv_taps(int d, int n_dst, int n_src, int& i0, int& i1, int& w0, int& w1) {
  const double scale = (double)n_src / (double)n_dst;
  const double f = __dsub_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), 0.5);
  const double fl = floor(f);
  i0 = (int)fl;
  float frac = (float)__dsub_rn(f, fl);
  if (i0 < 0) { i0 = 0; frac = 0.f; }
  if (i0 >= n_src - 1) { i0 = n_src - 1; frac = 0.f; }
  i1 = i0 + 1 < n_src - 1 ? i0 + 1 : n_src - 1;
  w1 = (int)rintf(frac * 2048.0f);
  w0 = (int)rintf((1.0f - frac) * 2048.0f);
}

// one byte of the object_ref picture: (ref * std[c] + mean[c]) * 255, each operation rounded, clamped, truncated (CLIP's constants)
__device__ __forceinline__ int ce_ref_byte(const float* __restrict__ ref, int c, int y, int x) {
  const float stdv[3] = {(float)0.26862954, (float)0.26130258, (float)0.27577711};
  const float mean[3] = {(float)0.48145466, (float)0.4578275, (float)0.40821073};
  float u = ref[((long long)c * CE_REF + y) * CE_REF + x] * stdv[c];
  u = u + mean[c];
  u = u * 255.0f;
  u = u < 0.f ? 0.f : (u > 255.f ? 255.f : u);
  return (int)u;
}

// the copy-paste baseline's paste: one byte of the object_ref picture resized to the mask's box, from the taps of its row and
// column -- computed from `ref`, never read from the picture this launch writes
__device__ __forceinline__ int ce_paste_byte(const float* __restrict__ ref, int c, int y0, int y1, int b0, int b1, int x0, int x1,
                                             int a0, int a1) {
  const int r0 = ce_ref_byte(ref, c, y0, x0) * a0 + ce_ref_byte(ref, c, y0, x1) * a1;
  const int r1 = ce_ref_byte(ref, c, y1, x0) * a0 + ce_ref_byte(ref, c, y1, x1) * a1;
  const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// the copy-paste baseline's m on a blend tile, up to the vertical maximum: mt = the mask of one object with a 2-pixel halo around
// the tile's part [ax0, ax1) x [ay0, ay1) of the region (what lies outside the frame, or is not needed, holds -inf and never wins),
// hb = its horizontal 5-pixel maximum on the rows the vertical one reads.  Laid out as the blur's tiles.
__device__ __forceinline__ void ce_dilate_rows(const ce_args& a, const float* __restrict__ mask, bool vec, int x0, int y0, int ax0,
                                               int ax1, int ay0, int ay1, float* mt, float* hb) {
  const int tid = threadIdx.x;
  const float out = -__builtin_inff();
  for (int i = tid; i < CE_MH * (CE_MW / 4); i += 256) {                 // the mask and its 2-pixel halo, 16 bytes a lane where whole
    const int j = i / (CE_MW / 4), c4 = (i - j * (CE_MW / 4)) * 4;
    const int y = y0 - CE_R + j, q0 = x0 - 8 + c4;
    float4 v = make_float4(out, out, out, out);
    if (y >= ay0 - CE_DR && y < ay1 + CE_DR && y >= 0 && y < a.H) {
      const float* row = mask + (long long)y * a.W;
      if (vec && q0 >= 0 && q0 + 3 < a.W && q0 >= ax0 - CE_DR && q0 + 3 < ax1 + CE_DR) {
        v = *reinterpret_cast<const float4*>(row + q0);
      } else {
        const int lo = ax0 - CE_DR > 0 ? ax0 - CE_DR : 0, hi = ax1 + CE_DR < a.W ? ax1 + CE_DR : a.W;
        v.x = (q0 >= lo && q0 < hi) ? row[q0] : out;
        v.y = (q0 + 1 >= lo && q0 + 1 < hi) ? row[q0 + 1] : out;
        v.z = (q0 + 2 >= lo && q0 + 2 < hi) ? row[q0 + 2] : out;
        v.w = (q0 + 3 >= lo && q0 + 3 < hi) ? row[q0 + 3] : out;
      }
    }
    *reinterpret_cast<float4*>(mt + j * CE_MW + c4) = v;
  }
  __syncthreads();
  // horizontal maximum of the rows the vertical one reads: pixel lx of row j reads mask columns lx + 6 .. lx + 10
  for (int i = tid; i < (CE_TH + 2 * CE_DR) * (CE_TW / 4); i += 256) {
    const int j = CE_R - CE_DR + i / (CE_TW / 4), i4 = (i & (CE_TW / 4 - 1)) * 4;
    float s[12];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float4 t = *reinterpret_cast<const float4*>(mt + j * CE_MW + i4 + 4 + 4 * q);
      s[4 * q] = t.x; s[4 * q + 1] = t.y; s[4 * q + 2] = t.z; s[4 * q + 3] = t.w;
    }
    float acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[e] = s[e + 2];
#pragma unroll
      for (int k = 1; k < 2 * CE_DR + 1; ++k) acc[e] = s[e + 2 + k] > acc[e] ? s[e + 2 + k] : acc[e];
    }
    *reinterpret_cast<float4*>(hb + j * CE_TW + i4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  }
}

// tile kind 0: recon = m * I + (1 - m) * pred on the tile at (x0, y0) of the frame, x0 % 64 == 0; written to the frame picture
// (frames) and, where the tile meets the crop window, to patch_pred.  Only what the tile's part of the region (the frame, or the
// crop window when no frame is written) needs is read: its pixels of image, its pixels and a 7-pixel halo of mask.
// MODE CE_COPY_PASTE: m is the 5 x 5 maximum of mask over the pixels inside the frame (a 2-pixel halo; what lies outside the frame
// or is not read holds -inf and never wins) and pred carries the resized reference on the mask's box.
template <int MODE>
__device__ __forceinline__ void ce_tile_blend(const ce_args& a, const ce_object& o, int b, int x0, int y0, const int* box, float* mt,
                                              float* hb, unsigned char* ob) {
  const int tid = threadIdx.x;
  const int gx0 = a.frames ? 0 : o.left, gy0 = a.frames ? 0 : o.top;
  const int gx1 = a.frames ? a.W : o.left + o.cw, gy1 = a.frames ? a.H : o.top + o.ch;
  const int ax0 = x0 > gx0 ? x0 : gx0, ax1 = x0 + CE_TW < gx1 ? x0 + CE_TW : gx1;
  const int ay0 = y0 > gy0 ? y0 : gy0, ay1 = y0 + CE_TH < gy1 ? y0 + CE_TH : gy1;
  const long long plane = (long long)a.H * a.W;
  const float* mask = a.mask + (long long)b * plane;
  const float* image = a.image + (long long)b * 3 * plane;
  const bool vec = (a.W & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.mask) | reinterpret_cast<uintptr_t>(a.image)) & 15) == 0;
  if constexpr (MODE == CE_COPY_PASTE) {
    ce_dilate_rows(a, mask, vec, x0, y0, ax0, ax1, ay0, ay1, mt, hb);
  } else {
    for (int i = tid; i < CE_MH * (CE_MW / 4); i += 256) {                 // the mask and its halo, 16 bytes a lane where whole
      const int j = i / (CE_MW / 4), c4 = (i - j * (CE_MW / 4)) * 4;
      const int y = y0 - CE_R + j, q0 = x0 - 8 + c4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (y >= ay0 - CE_R && y < ay1 + CE_R) {
        const float* row = mask + (long long)ce_reflect(y, a.H) * a.W;
        if (vec && q0 >= 0 && q0 + 3 < a.W && q0 >= ax0 - CE_R && q0 + 3 < ax1 + CE_R) {
          v = *reinterpret_cast<const float4*>(row + q0);
        } else {
          v.x = (q0 >= ax0 - CE_R && q0 < ax1 + CE_R) ? row[ce_reflect(q0, a.W)] : 0.f;
          v.y = (q0 + 1 >= ax0 - CE_R && q0 + 1 < ax1 + CE_R) ? row[ce_reflect(q0 + 1, a.W)] : 0.f;
          v.z = (q0 + 2 >= ax0 - CE_R && q0 + 2 < ax1 + CE_R) ? row[ce_reflect(q0 + 2, a.W)] : 0.f;
          v.w = (q0 + 3 >= ax0 - CE_R && q0 + 3 < ax1 + CE_R) ? row[ce_reflect(q0 + 3, a.W)] : 0.f;
        }
      }
      *reinterpret_cast<float4*>(mt + j * CE_MW + c4) = v;
    }
    __syncthreads();
    for (int i = tid; i < CE_MH * (CE_TW / 4); i += 256) {                 // horizontal pass: pixel lx reads mask columns lx + 1 + k
      const int j = i / (CE_TW / 4), i4 = (i - j * (CE_TW / 4)) * 4;
      float s[20];
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        const float4 t = *reinterpret_cast<const float4*>(mt + j * CE_MW + i4 + 4 * q);
        s[4 * q] = t.x; s[4 * q + 1] = t.y; s[4 * q + 2] = t.z; s[4 * q + 3] = t.w;
      }
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < CE_K; ++k) {
        const float t = a.taps[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += t * s[e + k + 1];
      }
      *reinterpret_cast<float4*>(hb + j * CE_TW + i4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
  }
  __syncthreads();
  const float sy = (float)a.hs / (float)o.ch, sx = (float)a.ws / (float)o.cw;
  const float* patch = a.patch_pred + (long long)b * 3 * a.hs * a.ws;
  const int bx1 = box[0], by1 = box[2], sw = box[1] - bx1, sh = box[3] - by1;       // (read in copy-paste mode only)
  const float* ref = a.ref + (long long)b * 3 * CE_REF * CE_REF;
  for (int p = 0; p < 2; ++p) {                                          // vertical pass and the blend, four pixels a lane
    const int ly = (tid >> 4) + 16 * p, lx4 = (tid & 15) * 4, y = y0 + ly, x = x0 + lx4;
    if (y < ay0 || y >= ay1 || x >= ax1 || x + 3 < ax0) continue;
    float m[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (MODE == CE_COPY_PASTE) {
      const float4 h0 = *reinterpret_cast<const float4*>(hb + (ly + CE_R - CE_DR) * CE_TW + lx4);
      m[0] = h0.x; m[1] = h0.y; m[2] = h0.z; m[3] = h0.w;
#pragma unroll
      for (int k = 1; k < 2 * CE_DR + 1; ++k) {
        const float4 h = *reinterpret_cast<const float4*>(hb + (ly + CE_R - CE_DR + k) * CE_TW + lx4);
        m[0] = h.x > m[0] ? h.x : m[0]; m[1] = h.y > m[1] ? h.y : m[1]; m[2] = h.z > m[2] ? h.z : m[2]; m[3] = h.w > m[3] ? h.w : m[3];
      }
    } else {
#pragma unroll
      for (int k = 0; k < CE_K; ++k) {
        const float t = a.taps[k];
        const float4 h = *reinterpret_cast<const float4*>(hb + (ly + k) * CE_TW + lx4);
        m[0] += t * h.x; m[1] += t * h.y; m[2] += t * h.z; m[3] += t * h.w;
      }
    }
    const bool whole = vec && x >= ax0 && x + 3 < ax1;
    const int cy = y - o.top;
    const bool row_in = cy >= 0 && cy < o.ch;
    int py0 = 0, py1 = 0;
    float ply = 0.f;
    if (row_in) ce_taps(sy, cy, a.hs, py0, py1, ply);
    const bool paste_row = MODE == CE_COPY_PASTE && sw > 0 && sh > 0 && y >= by1 && y < by1 + sh;
    int ry0 = 0, ry1 = 0, rb0 = 0, rb1 = 0;
    int rx0[4] = {0, 0, 0, 0}, rx1[4] = {0, 0, 0, 0}, ra0[4] = {0, 0, 0, 0}, ra1[4] = {0, 0, 0, 0};
    bool paste[4] = {false, false, false, false};                        // the paste's taps: one set per row and per column, not per channel
    if (paste_row) {
      ce_cv_taps(y - by1, sh, CE_REF, ry0, ry1, rb0, rb1);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        paste[e] = x + e >= bx1 && x + e < bx1 + sw;
        if (paste[e]) ce_cv_taps(x + e - bx1, sw, CE_REF, rx0[e], rx1[e], ra0[e], ra1[e]);
      }
    }
    unsigned bytes[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* ic = image + c * plane + (long long)y * a.W + x;
      float v[4];
      if (whole) {
        const float4 t = *reinterpret_cast<const float4*>(ic);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (x + e >= ax0 && x + e < ax1) ? ic[e] : 0.f;
      }
      const float* pc = patch + (long long)c * a.hs * a.ws;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float u = ((v[e] + 1.0f) / 2.0f) * 255.0f;
        u = u < 0.f ? 0.f : (u > 255.f ? 255.f : u);
        const float iu = (float)(unsigned char)(int)u;
        const int cx = x + e - o.left;
        float pred = 0.f;
        if (row_in && cx >= 0 && cx < o.cw) {
          int px0, px1;
          float plx;
          ce_taps(sx, cx, a.ws, px0, px1, plx);
          pred = (float)ce_patch_byte(pc, a.ws, py0, py1, px0, px1, ply, plx);
        }
        if (paste[e]) pred = (float)ce_paste_byte(ref, c, ry0, ry1, rb0, rb1, rx0[e], rx1[e], ra0[e], ra1[e]);
        const float r = m[e] * iu + (1.0f - m[e]) * pred;
        int q = __float2int_rn(r);                                       // nearest even, saturating
        q = q < 0 ? 0 : (q > 255 ? 255 : q);
        bytes[e * 3 + c] = (unsigned)q;
      }
    }
    unsigned* w = reinterpret_cast<unsigned*>(ob + ly * CE_OBW + lx4 * 3);
#pragma unroll
    for (int q = 0; q < 3; ++q)
      w[q] = bytes[4 * q] | (bytes[4 * q + 1] << 8) | (bytes[4 * q + 2] << 16) | (bytes[4 * q + 3] << 24);
  }
  __syncthreads();
  if (a.frames) ce_store(ob, x0, y0, ax0, ay0, ax1, ay1, a.out + o.off[0], (long long)a.W * 3, 0, 0);
  const int cx0 = ax0 > o.left ? ax0 : o.left, cx1 = ax1 < o.left + o.cw ? ax1 : o.left + o.cw;
  const int cy0 = ay0 > o.top ? ay0 : o.top, cy1 = ay1 < o.top + o.ch ? ay1 : o.top + o.ch;
  ce_store(ob, x0, y0, cx0, cy0, cx1, cy1, a.out + o.off[1], (long long)o.cw * 3, o.left, o.top);
}

// tile kind 1: P(patch_gt) on the tile at (x0, y0) of the crop window's own coordinates
__device__ __forceinline__ void ce_tile_patch(const ce_args& a, const ce_object& o, int b, int x0, int y0, unsigned char* ob) {
  const float sy = (float)a.hs / (float)o.ch, sx = (float)a.ws / (float)o.cw;
  const float* patch = a.patch_gt + (long long)b * 3 * a.hs * a.ws;
  const int lx = threadIdx.x & 63, x = x0 + lx;
  int px0 = 0, px1 = 0;
  float plx = 0.f;
  if (x < o.cw) ce_taps(sx, x, a.ws, px0, px1, plx);
  for (int ly = threadIdx.x >> 6; ly < CE_TH; ly += 4) {
    const int y = y0 + ly;
    if (x >= o.cw || y >= o.ch) continue;
    int py0, py1;
    float ply;
    ce_taps(sy, y, a.hs, py0, py1, ply);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      ob[ly * CE_OBW + lx * 3 + c] = (unsigned char)ce_patch_byte(patch + (long long)c * a.hs * a.ws, a.ws, py0, py1, px0, px1, ply, plx);
  }
  __syncthreads();
  const int x1 = x0 + CE_TW < o.cw ? x0 + CE_TW : o.cw, y1 = y0 + CE_TH < o.ch ? y0 + CE_TH : o.ch;
  ce_store(ob, x0, y0, x0, y0, x1, y1, a.out + o.off[2], (long long)o.cw * 3, 0, 0);
}

// pred at frame pixel (y, x): P(patch_pred) inside the crop window, 0 elsewhere -- recomputed, not read from another block's tile
__device__ __forceinline__ int ce_pred_at(const ce_args& a, const ce_object& o, const float* __restrict__ pc, float sy, float sx,
                                          int y, int x) {
  const int cy = y - o.top, cx = x - o.left;
  if (cy < 0 || cy >= o.ch || cx < 0 || cx >= o.cw) return 0;
  int py0, py1, px0, px1;
  float ply, plx;
  ce_taps(sy, cy, a.hs, py0, py1, ply);
  ce_taps(sx, cx, a.ws, px0, px1, plx);
  return ce_patch_byte(pc, a.ws, py0, py1, px0, px1, ply, plx);
}

// tile kind 2: object_pred = cv2.resize(pred[y1:y2, x1:x2], (224, 224)) on the tile at (x0, y0) of the 224 x 224 picture
// MODE CE_COPY_PASTE: the box of pred holds the pasted reference and nothing else, so every tap is a `ce_paste_byte`
template <int MODE>
__device__ __forceinline__ void ce_tile_object(const ce_args& a, const ce_object& o, int b, int x0, int y0, const int* box,
                                               unsigned char* ob) {
  const int bx1 = box[0], bx2 = box[1], by1 = box[2], by2 = box[3];
  const int sw = bx2 - bx1, sh = by2 - by1;                              // the slice excludes the last row and column
  if (sw <= 0 || sh <= 0) return;                                        // (block-uniform: the status word reports it)
  const float sy = (float)a.hs / (float)o.ch, sx = (float)a.ws / (float)o.cw;
  const float* patch = a.patch_pred + (long long)b * 3 * a.hs * a.ws;
  const int lx = threadIdx.x & 63, x = x0 + lx;
  int xi0 = 0, xi1 = 0, a0 = 0, a1 = 0;
  if (x < CE_REF) ce_cv_taps(x, CE_REF, sw, xi0, xi1, a0, a1);
  const float* ref = a.ref + (long long)b * 3 * CE_REF * CE_REF;
  int tx[2][4] = {}, ty[2][4] = {};                                      // copy-paste: the paste's taps at box columns xi0, xi1 / rows yi0, yi1
  if (MODE == CE_COPY_PASTE && x < CE_REF) {
    ce_cv_taps(xi0, sw, CE_REF, tx[0][0], tx[0][1], tx[0][2], tx[0][3]);
    ce_cv_taps(xi1, sw, CE_REF, tx[1][0], tx[1][1], tx[1][2], tx[1][3]);
  }
  for (int ly = threadIdx.x >> 6; ly < CE_TH; ly += 4) {
    const int y = y0 + ly;
    if (x >= CE_REF || y >= CE_REF) continue;
    int yi0, yi1, b0, b1;
    ce_cv_taps(y, CE_REF, sh, yi0, yi1, b0, b1);
    if constexpr (MODE == CE_COPY_PASTE) {
      ce_cv_taps(yi0, sh, CE_REF, ty[0][0], ty[0][1], ty[0][2], ty[0][3]);
      ce_cv_taps(yi1, sh, CE_REF, ty[1][0], ty[1][1], ty[1][2], ty[1][3]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int r0, r1;
      if constexpr (MODE == CE_COPY_PASTE) {
        r0 = ce_paste_byte(ref, c, ty[0][0], ty[0][1], ty[0][2], ty[0][3], tx[0][0], tx[0][1], tx[0][2], tx[0][3]) * a0 +
             ce_paste_byte(ref, c, ty[0][0], ty[0][1], ty[0][2], ty[0][3], tx[1][0], tx[1][1], tx[1][2], tx[1][3]) * a1;
        r1 = ce_paste_byte(ref, c, ty[1][0], ty[1][1], ty[1][2], ty[1][3], tx[0][0], tx[0][1], tx[0][2], tx[0][3]) * a0 +
             ce_paste_byte(ref, c, ty[1][0], ty[1][1], ty[1][2], ty[1][3], tx[1][0], tx[1][1], tx[1][2], tx[1][3]) * a1;
      } else {
        const float* pc = patch + (long long)c * a.hs * a.ws;
        r0 = ce_pred_at(a, o, pc, sy, sx, by1 + yi0, bx1 + xi0) * a0 + ce_pred_at(a, o, pc, sy, sx, by1 + yi0, bx1 + xi1) * a1;
        r1 = ce_pred_at(a, o, pc, sy, sx, by1 + yi1, bx1 + xi0) * a0 + ce_pred_at(a, o, pc, sy, sx, by1 + yi1, bx1 + xi1) * a1;
      }
      int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      ob[ly * CE_OBW + lx * 3 + c] = (unsigned char)v;
    }
  }
  __syncthreads();
  const int x1 = x0 + CE_TW < CE_REF ? x0 + CE_TW : CE_REF, y1 = y0 + CE_TH < CE_REF ? y0 + CE_TH : CE_REF;
  ce_store(ob, x0, y0, x0, y0, x1, y1, a.out + o.off[3], (long long)CE_REF * 3, 0, 0);
}

// tile kind 3: object_ref = un_norm_clip(ref) * 255 on the tile at (x0, y0) of the 224 x 224 picture
__device__ __forceinline__ void ce_tile_ref(const ce_args& a, const ce_object& o, int b, int x0, int y0, unsigned char* ob) {
  const float* ref = a.ref + (long long)b * 3 * CE_REF * CE_REF;
  const int lx = threadIdx.x & 63, x = x0 + lx;
  for (int ly = threadIdx.x >> 6; ly < CE_TH; ly += 4) {
    const int y = y0 + ly;
    if (x >= CE_REF || y >= CE_REF) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) ob[ly * CE_OBW + lx * 3 + c] = (unsigned char)ce_ref_byte(ref, c, y, x);
  }
  __syncthreads();
  const int x1 = x0 + CE_TW < CE_REF ? x0 + CE_TW : CE_REF, y1 = y0 + CE_TH < CE_REF ? y0 + CE_TH : CE_REF;
  ce_store(ob, x0, y0, x0, y0, x1, y1, a.out + o.off[4], (long long)CE_REF * 3, 0, 0);
}

// the walk of both export kernels: MODE picks the form of the blend and object tiles
template <int MODE>
__device__ __forceinline__ void ce_walk(const ce_args& a, const ce_table& t) {
  __shared__ __attribute__((aligned(16))) float mt[CE_MH * CE_MW];
  __shared__ __attribute__((aligned(16))) float hb[CE_MH * CE_TW];
  __shared__ __attribute__((aligned(16))) unsigned char ob[CE_TH * CE_OBW];
  __shared__ int box[4];
  const int b = blockIdx.y;
  const ce_object& o = t.o[b];
  // the blend tiles lie on the frame's 64 x 32 grid (so that rows of four floats stay 16-byte aligned), the others on their picture's
  const int bx0 = a.frames ? 0 : o.left / CE_TW, bx1 = a.frames ? (a.W + CE_TW - 1) / CE_TW : (o.left + o.cw - 1) / CE_TW + 1;
  const int by0 = a.frames ? 0 : o.top / CE_TH, by1 = a.frames ? (a.H + CE_TH - 1) / CE_TH : (o.top + o.ch - 1) / CE_TH + 1;
  const int nbx = bx1 - bx0, n_blend = nbx * (by1 - by0);
  const int npx = (o.cw + CE_TW - 1) / CE_TW, n_patch = npx * ((o.ch + CE_TH - 1) / CE_TH);
  constexpr int NRX = (CE_REF + CE_TW - 1) / CE_TW, N_REF = NRX * ((CE_REF + CE_TH - 1) / CE_TH);
  const int total = n_blend + n_patch + 2 * N_REF;
  if (threadIdx.x < 64) {                                                // the object's box: 1 KiB of partial records
    const int* p = a.box_ws + ((long long)b * CE_BOX_PARTS + threadIdx.x) * 4;
    int lox = p[0], hix = p[1], loy = p[2], hiy = p[3];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const int c = __shfl_xor(lox, s, 64), d = __shfl_xor(hix, s, 64), e = __shfl_xor(loy, s, 64), f = __shfl_xor(hiy, s, 64);
      lox = c < lox ? c : lox; hix = d > hix ? d : hix; loy = e < loy ? e : loy; hiy = f > hiy ? f : hiy;
    }
    if (threadIdx.x == 0) { box[0] = lox; box[1] = hix; box[2] = loy; box[3] = hiy; }
  }
  __syncthreads();
  for (int i = blockIdx.x; i < total; i += gridDim.x) {
    if (i < n_blend) {
      ce_tile_blend<MODE>(a, o, b, (bx0 + i % nbx) * CE_TW, (by0 + i / nbx) * CE_TH, box, mt, hb, ob);
    } else if (i < n_blend + n_patch) {
      const int k = i - n_blend;
      ce_tile_patch(a, o, b, (k % npx) * CE_TW, (k / npx) * CE_TH, ob);
    } else if (i < n_blend + n_patch + N_REF) {
      const int k = i - n_blend - n_patch;
      if (k == 0 && threadIdx.x == 0) a.status[b] = (box[1] - box[0] <= 0 || box[3] - box[2] <= 0) ? 1 : 0;
      ce_tile_object<MODE>(a, o, b, (k % NRX) * CE_TW, (k / NRX) * CE_TH, box, ob);
    } else {
      const int k = i - n_blend - n_patch - N_REF;
      ce_tile_ref(a, o, b, (k % NRX) * CE_TW, (k / NRX) * CE_TH, ob);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void camera_export_kernel(const ce_args a, const ce_table t) { ce_walk<CE_EXPORT>(a, t); }

// the copy-paste baseline (include/mobi_engine.h, mobi_camera_copy_paste): the same tiles, with the dilated mask and the pasted reference
__global__ __launch_bounds__(256) void camera_copy_paste_kernel(const ce_args a, const ce_table t) { ce_walk<CE_COPY_PASTE>(a, t); }

// ---------------------------------------------------------------------------------------------------------
// Lidar-on-camera overlays of a batch (include/mobi_engine.h, mobi_lidar_overlay): a sweep's points projected into a frame and
// drawn over it as round markers coloured by depth, every picture HWC uint8 in one buffer.  Two launches over a cleared
// workspace of one u32 key per frame pixel: the splat launch projects every sweep pixel, folds the picture's depth range into
// its record and leaves `sweep index + 1` under its marker with atomicMax (the higher index wins, as matplotlib paints in array
// order, whatever the thread order); the resolve launch walks the frame four pixels a lane, converts or copies the frame's
// pixel where the key is 0 and otherwise projects that point again (the same expressions: the same bits) for its colour.
// blockIdx.y = the picture; its table entry travels in the launch's argument block.  No FMA contraction in this file.
// ---------------------------------------------------------------------------------------------------------
constexpr int LO_MAX_PICTURES = 64, LO_LAUNCH = 32;          // per call; per launch (what fits the argument block)
constexpr int LO_REC = 4;                                    // u32 per record: ~min bits, max bits, kept count, 0
struct lo_picture {
  const float* depth; const float* pitch; const float* yaw;
  const unsigned char* frame;                                // the frame source with its byte offset added
  long long out_off;
  float m[12];
  int kind, pad;
};
struct lo_table { lo_picture p[LO_LAUNCH]; };
struct lo_args {
  unsigned* keys; unsigned* rec;                             // of this launch's first picture
  const unsigned char* lut; unsigned char* out;
  long long out_bytes, rec_off, key_stride;                  // rec_off: this launch's first record in `out`
  int h0, w0, H, W, point_size;
};

// sweep pixel i of picture s -> kept?, the clipped camera depth and the marker's centre pixel
__device__ __forceinline__ bool lo_project(const lo_picture& s, int i, int H, int W, float& zc, int& px, int& py) {
  float d = (s.depth[i] + 1.0f) / 2.0f;
  d = d * 54.0f;
  if (!(d > 1.4f && d < 54.0f)) return false;                // LidarConverter.range2pcd's validity window
  const float yaw = s.yaw[i], pitch = s.pitch[i];
  const float cp = cosf(pitch);
  const float x = cosf(yaw) * cp * d;
  const float y = -sinf(yaw) * cp * d;
  const float z = sinf(pitch) * d;
  const float qx = s.m[0] * x + s.m[1] * y + s.m[2] * z + s.m[3];
  const float qy = s.m[4] * x + s.m[5] * y + s.m[6] * z + s.m[7];
  const float qz = s.m[8] * x + s.m[9] * y + s.m[10] * z + s.m[11];
  if (!(qz > 0.0f)) return false;
  zc = qz < 1e-5f ? 1e-5f : (qz > 1e5f ? 1e5f : qz);
  const float u = qx / zc, v = qy / zc;
  if (!(u >= 0.0f && u < (float)W && v >= 0.0f && v < (float)H)) return false;
  px = (int)u, py = (int)v;
  return true;
}

__global__ __launch_bounds__(256) void lidar_overlay_splat_kernel(const lo_args a, const lo_table t) {
  const int p = blockIdx.y;
  const lo_picture& s = t.p[p];
  const int n = a.h0 * a.w0, i = blockIdx.x * 256 + threadIdx.x;
  float zc = 0.f;
  int px = 0, py = 0;
  const bool kept = i < n && lo_project(s, i, a.H, a.W, zc, px, py);
  if (kept) {
    unsigned* keys = a.keys + (long long)p * a.key_stride;
    const int r = a.point_size >> 1, d2 = a.point_size * a.point_size;           // dx^2 + dy^2 <= (point_size / 2)^2
    for (int dy = -r; dy <= r; ++dy) {
      const int y = py + dy;
      if (y < 0 || y >= a.H) continue;
      for (int dx = -r; dx <= r; ++dx) {
        const int x = px + dx;
        if (4 * (dx * dx + dy * dy) > d2 || x < 0 || x >= a.W) continue;
        atomicMax(keys + (long long)y * a.W + x, (unsigned)i + 1u);
      }
    }
  }
  // zc > 0: its bits order as unsigned integers; the minimum is kept as the maximum of the complement, so that 0 means "none"
  unsigned lo = kept ? ~__float_as_uint(zc) : 0u, hi = kept ? __float_as_uint(zc) : 0u, cnt = kept ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
    lo = l2 > lo ? l2 : lo, hi = h2 > hi ? h2 : hi, cnt += __shfl_xor(cnt, o, 64);
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    unsigned* rec = a.rec + p * LO_REC;
    atomicMax(rec, lo);
    atomicMax(rec + 1, hi);
    atomicAdd(rec + 2, cnt);
  }
}

// one frame pixel as 0x00BBGGRR: the marker's colour under a key, else the frame's own pixel `under`
__device__ __forceinline__ unsigned lo_pixel(const lo_args& a, const lo_picture& s, unsigned key, float zmin, float zmax, unsigned under) {
  if (key == 0u || key > (unsigned)(a.h0 * a.w0)) return under;
  float zc = 0.f;
  int px, py;
  if (!lo_project(s, (int)(key - 1u), a.H, a.W, zc, px, py)) return under;       // (cannot be: the splat launch kept it)
  float tt = 0.f;
  if (zmax != zmin) tt = (zc - zmin) / (zmax - zmin);
  int li = (int)(tt * 256.0f);
  li = li < 0 ? 0 : (li > 255 ? 255 : li);
  const unsigned char* c = a.lut + li * 3;
  return (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
}

__device__ __forceinline__ unsigned lo_byte(float x) {        // ((x + 1) / 2 * 255) clamped to [0, 255], truncated
  float u = ((x + 1.0f) / 2.0f) * 255.0f;
  u = u < 0.f ? 0.f : (u > 255.f ? 255.f : u);
  return (unsigned)(int)u;
}

__global__ __launch_bounds__(256) void lidar_overlay_resolve_kernel(const lo_args a, const lo_table t) {
  const int p = blockIdx.y;
  const lo_picture& s = t.p[p];
  const long long N = (long long)a.H * a.W, groups = (N + 3) >> 2;
  const unsigned* rec = a.rec + p * LO_REC;
  const unsigned count = rec[2];
  const float zmin = count ? __uint_as_float(~rec[0]) : 0.f, zmax = count ? __uint_as_float(rec[1]) : 0.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) {                 // the record, behind the pictures
    const long long ro = a.rec_off + (long long)p * LO_REC * 4;
    if (ro >= 0 && ro + LO_REC * 4 <= a.out_bytes) {
      unsigned* o = reinterpret_cast<unsigned*>(a.out + ro);
      o[0] = __float_as_uint(zmin), o[1] = __float_as_uint(zmax), o[2] = count, o[3] = 0u;
    }
  }
  const unsigned* keys = a.keys + (long long)p * a.key_stride;
  const float* f32 = reinterpret_cast<const float*>(s.frame);
  const bool vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(s.frame) & 15) == 0;
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < groups; j += (long long)gridDim.x * 256) {
    const long long q0 = j * 4, ob = s.out_off + q0 * 3;
    const int m = N - q0 < 4 ? (int)(N - q0) : 4;            // pixels of this group
    const uint4 k4 = *reinterpret_cast<const uint4*>(keys + q0);                 // (key rows are padded to whole groups)
    const unsigned key[4] = {k4.x, k4.y, k4.z, k4.w};
    unsigned under[4] = {0u, 0u, 0u, 0u};
    if (s.kind == 1) {                                       // uint8 HWC: 12 bytes of 4 pixels
      if (m == 4) {
        const unsigned* w = reinterpret_cast<const unsigned*>(s.frame + q0 * 3);
        const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
        under[0] = w0 & 0xffffffu, under[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
        under[2] = (w1 >> 16) | ((w2 & 0xffu) << 16), under[3] = w2 >> 8;
      } else {
#pragma unroll
        for (int e = 0; e < 3; ++e) {                        // (the picture's last, short group)
          if (e >= m) continue;
          const unsigned char* c = s.frame + (q0 + e) * 3;
          under[e] = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
        }
      }
    } else {                                                 // fp32 planar in [-1, 1]
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* pc = f32 + c * N + q0;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
          const float4 f = *reinterpret_cast<const float4*>(pc);
          v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = e < m ? pc[e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) under[e] |= lo_byte(v[e]) << (8 * c);
      }
    }
    unsigned px[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) px[e] = lo_pixel(a, s, e < m ? key[e] : 0u, zmin, zmax, under[e]);
    if (ob < 0 || ob + m * 3 > a.out_bytes) continue;        // (the host placed every picture inside the buffer)
    if (m == 4) {
      unsigned* w = reinterpret_cast<unsigned*>(a.out + ob);                     // out, out_off and 12 j: 4-byte aligned
      w[0] = px[0] | (px[1] << 24);
      w[1] = (px[1] >> 8) | (px[2] << 16);
      w[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
#pragma unroll
      for (int e = 0; e < 3; ++e)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (e < m) a.out[ob + e * 3 + c] = (unsigned char)(px[e] >> (8 * c));
      // the bytes up to the next 4-byte boundary are nobody else's (every offset is a multiple of 4): 0, so that a buffer is
      // defined to its last byte
      for (long long b = ob + m * 3; (b & 3) && b < a.out_bytes; ++b) a.out[b] = 0;
    }
  }
}

}  // namespace mobi

using namespace mobi;
#define ST(stream) reinterpret_cast<hipStream_t>(stream)

extern "C" int mobi_range_paste(const mobi_range_paste_params* p, void* stream) {
  if (!p || !p->sample_depth || !p->depth_orig || !p->crop_left || !p->width_crop) return MOBI_ERR_ARG;
  if (p->batch <= 0 || p->hc <= 0 || p->wc <= 0 || p->h0 <= 0 || p->w0 <= 0 || p->hc % p->h0) return MOBI_ERR_ARG;
  if (p->planes && (!p->pitch || !p->yaw)) return MOBI_ERR_ARG;
  if ((p->sample_int != nullptr) != (p->int_orig != nullptr)) return MOBI_ERR_ARG;
  hipLaunchKernelGGL(range_paste_kernel, dim3(egrid_pp((long long)p->batch * p->h0 * p->w0)), dim3(256), 0, ST(stream), *p);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_lidar_metrics(const mobi_lidar_metrics_params* p, void* stream) {
  if (!p || !p->pred || !p->gt || !p->inst_mask || !p->box_mask || !p->width_crop || !p->out) return MOBI_ERR_ARG;
  if (p->batch <= 0 || p->h <= 0 || p->w <= 0 || p->pool_h <= 0 || p->h % p->pool_h || p->max_width <= 0) return MOBI_ERR_ARG;
  if (p->max_width > p->w) return MOBI_ERR_ARG;                                      // a window wider than the view
  if ((long long)p->pool_h * p->max_width > 16384) return MOBI_ERR_UNSUPPORTED;      // the sort space in LDS
  hipLaunchKernelGGL(lidar_metrics_kernel, dim3(p->batch, 2), dim3(1024), 0, ST(stream), *p);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_image_grid(const mobi_image_grid_source* sources, int32_t n_sources, int32_t max_images, int32_t nrow,
                               int32_t padding, int32_t clamp, int32_t rescale, uint8_t* out, int64_t out_bytes, void* stream) {
  if (!sources || !out || n_sources <= 0 || max_images <= 0 || nrow <= 0 || padding < 0 || out_bytes <= 0) return MOBI_ERR_ARG;
  if (n_sources > IG_MAX_SOURCES) return MOBI_ERR_UNSUPPORTED;
  ig_table t = {};
  t.padding = padding, t.clamp = clamp != 0, t.rescale = rescale != 0;
  long long most = 0;
  for (int i = 0; i < n_sources; ++i) {
    const mobi_image_grid_source& s = sources[i];
    if (!s.data || s.n <= 0 || s.c <= 0 || s.h <= 0 || s.w <= 0) return MOBI_ERR_ARG;
    if (s.elem_bytes == 2 || (s.c != 1 && s.c != 3)) return MOBI_ERR_UNSUPPORTED;
    if (s.elem_bytes != 1 && s.elem_bytes != 4) return MOBI_ERR_ARG;
    ig_entry& e = t.e[i];
    e.data = s.data, e.n = s.n < max_images ? s.n : max_images, e.c = s.c, e.h = s.h, e.w = s.w, e.is_u8 = s.elem_bytes == 1;
    e.xmaps = e.n < nrow ? e.n : nrow;
    const long long ymaps = (e.n + e.xmaps - 1) / e.xmaps;
    const long long hg = e.n == 1 ? s.h : ymaps * ((long long)s.h + padding) + padding;
    const long long wg = e.n == 1 ? s.w : e.xmaps * ((long long)s.w + padding) + padding;
    const long long bytes = hg * wg * 3;
    if (hg > 0x7fffffffLL || wg > 0x7fffffffLL || bytes > 0x7ffffff0LL) return MOBI_ERR_UNSUPPORTED;   // (32-bit byte index)
    if (s.out_offset < 0 || s.out_offset > out_bytes || bytes > out_bytes - s.out_offset) return MOBI_ERR_ARG;
    if ((s.out_offset & 3) || (reinterpret_cast<uintptr_t>(out) & 3)) return MOBI_ERR_ALIGN;
    if (s.elem_bytes == 4 && (reinterpret_cast<uintptr_t>(s.data) & 3)) return MOBI_ERR_ALIGN;
    e.hg = (int)hg, e.wg = (int)wg, e.out_offset = s.out_offset;
    most = bytes > most ? bytes : most;
  }
  hipLaunchKernelGGL(image_grid_kernel, dim3(egrid_pp((most + 3) / 4), n_sources), dim3(256), 0, ST(stream), t, out);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

static int camera_export_launch(const mobi_camera_export_params* p, void* stream, int mode) {
  if (!p || !p->patch_pred || !p->patch_gt || !p->ref || !p->image || !p->mask || (mode == CE_EXPORT && !p->taps) || !p->crop ||
      !p->offsets || !p->box_ws || !p->out) return MOBI_ERR_ARG;
  if (p->batch <= 0 || p->hs <= 0 || p->ws <= 0 || p->ref_h <= 0 || p->ref_w <= 0 || p->H <= 0 || p->W <= 0 || p->out_bytes <= 0)
    return MOBI_ERR_ARG;
  if (p->ref_h != CE_REF || p->ref_w != CE_REF || p->batch > CE_MAX_OBJECTS) return MOBI_ERR_UNSUPPORTED;
  if ((long long)p->H * p->W > 0x7fffffffLL / 3) return MOBI_ERR_UNSUPPORTED;                  // (32-bit pixel indices)
  // one picture: inside the buffer, on a 4-byte boundary
  auto place = [&](long long off, long long bytes) {
    if (off < 0 || off > p->out_bytes || bytes > p->out_bytes - off) return (int)MOBI_ERR_ARG;
    return (off & 3) ? (int)MOBI_ERR_ALIGN : (int)MOBI_OK;
  };
  if (reinterpret_cast<uintptr_t>(p->out) & 3) return MOBI_ERR_ALIGN;
  int rc = place(p->status_offset, 4LL * p->batch);
  if (rc != MOBI_OK) return rc;
  ce_table t = {};
  int most = 0;
  const int n_ref = ((CE_REF + CE_TW - 1) / CE_TW) * ((CE_REF + CE_TH - 1) / CE_TH);
  for (int b = 0; b < p->batch; ++b) {
    ce_object& o = t.o[b];
    o.left = p->crop[b * 4], o.top = p->crop[b * 4 + 1], o.cw = p->crop[b * 4 + 2], o.ch = p->crop[b * 4 + 3];
    if (o.left < 0 || o.top < 0 || o.cw <= 0 || o.ch <= 0 || o.cw > p->W - o.left || o.ch > p->H - o.top) return MOBI_ERR_ARG;
    const long long sizes[5] = {p->frames ? 3LL * p->H * p->W : 0, 3LL * o.cw * o.ch, 3LL * o.cw * o.ch, 3LL * CE_REF * CE_REF,
                                3LL * CE_REF * CE_REF};
    for (int k = p->frames ? 0 : 1; k < 5; ++k) {
      o.off[k] = p->offsets[b * 5 + k];
      if ((rc = place(o.off[k], sizes[k])) != MOBI_OK) return rc;
    }
    const int tiles_x = p->frames ? (p->W + CE_TW - 1) / CE_TW : (o.left + o.cw - 1) / CE_TW - o.left / CE_TW + 1;
    const int tiles_y = p->frames ? (p->H + CE_TH - 1) / CE_TH : (o.top + o.ch - 1) / CE_TH - o.top / CE_TH + 1;
    const int total = tiles_x * tiles_y + ((o.cw + CE_TW - 1) / CE_TW) * ((o.ch + CE_TH - 1) / CE_TH) + 2 * n_ref;
    most = total > most ? total : most;
  }
  ce_args a = {p->patch_pred, p->patch_gt, p->ref, p->image, p->mask, p->taps, p->box_ws, p->out,
               reinterpret_cast<int*>(p->out + p->status_offset), p->hs, p->ws, p->H, p->W, p->frames != 0};
  hipLaunchKernelGGL(camera_box_kernel, dim3(CE_BOX_PARTS, p->batch), dim3(256), 0, ST(stream), p->mask, p->box_ws, p->H, p->W);
  const dim3 grid(most > 2048 ? 2048 : most, p->batch);
  if (mode == CE_COPY_PASTE) hipLaunchKernelGGL(camera_copy_paste_kernel, grid, dim3(256), 0, ST(stream), a, t);
  else hipLaunchKernelGGL(camera_export_kernel, grid, dim3(256), 0, ST(stream), a, t);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_camera_export(const mobi_camera_export_params* p, void* stream) { return camera_export_launch(p, stream, CE_EXPORT); }

extern "C" int mobi_camera_copy_paste(const mobi_camera_export_params* p, void* stream) {
  return camera_export_launch(p, stream, CE_COPY_PASTE);
}

static inline long long lo_key_stride(long long H, long long W) { return (H * W + 3) & ~3LL; }

extern "C" size_t mobi_lidar_overlay_workspace_bytes(int32_t n_pictures, int32_t H, int32_t W) {
  if (n_pictures <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)n_pictures * ((size_t)lo_key_stride(H, W) * 4 + LO_REC * 4);
}

extern "C" int mobi_lidar_overlay(const mobi_lidar_overlay_params* p, void* stream) {
  if (!p || !p->pictures || !p->lut || !p->out || !p->workspace) return MOBI_ERR_ARG;
  if (p->n_pictures <= 0 || p->h0 <= 0 || p->w0 <= 0 || p->H <= 0 || p->W <= 0 || p->out_bytes <= 0) return MOBI_ERR_ARG;
  if (p->n_pictures > LO_MAX_PICTURES) return MOBI_ERR_UNSUPPORTED;
  if (p->point_size != 1 && p->point_size != 3 && p->point_size != 5) return MOBI_ERR_UNSUPPORTED;
  if ((long long)p->H * p->W > 0x7fffffffLL / 3 || (long long)p->h0 * p->w0 > 0x7ffffff0LL) return MOBI_ERR_UNSUPPORTED;   // (32-bit indices)
  if (p->workspace_bytes < 0 || (size_t)p->workspace_bytes < mobi_lidar_overlay_workspace_bytes(p->n_pictures, p->H, p->W))
    return MOBI_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(p->out) & 3) || (reinterpret_cast<uintptr_t>(p->workspace) & 15)) return MOBI_ERR_ALIGN;
  auto place = [&](long long off, long long bytes) {         // inside the buffer, on a 4-byte boundary
    if (off < 0 || off > p->out_bytes || bytes > p->out_bytes - off) return (int)MOBI_ERR_ARG;
    return (off & 3) ? (int)MOBI_ERR_ALIGN : (int)MOBI_OK;
  };
  int rc = place(p->records_offset, 4LL * LO_REC * p->n_pictures);
  if (rc != MOBI_OK) return rc;
  const long long N = (long long)p->H * p->W, stride = lo_key_stride(p->H, p->W);
  lo_table t[LO_MAX_PICTURES / LO_LAUNCH] = {};
  for (int i = 0; i < p->n_pictures; ++i) {
    const mobi_lidar_overlay_picture& s = p->pictures[i];
    if (!s.depth || !s.pitch || !s.yaw || !s.frame || s.frame_offset < 0) return MOBI_ERR_ARG;
    if (s.frame_kind != MOBI_OVERLAY_FRAME_F32_PLANAR && s.frame_kind != MOBI_OVERLAY_FRAME_U8_HWC) return MOBI_ERR_ARG;
    if ((rc = place(s.out_offset, 3 * N)) != MOBI_OK) return rc;
    const uintptr_t frame = reinterpret_cast<uintptr_t>(s.frame) + (uintptr_t)s.frame_offset;
    // a picture owns its bytes up to the next multiple of 4 (the resolve launch zeroes them): it may share none of them with the
    // records or with an earlier picture, and no frame source may lie in the buffer the pictures are written to
    const long long end = (s.out_offset + 3 * N + 3) & ~3LL;
    if (s.out_offset < p->records_offset + 4LL * LO_REC * p->n_pictures && p->records_offset < end) return MOBI_ERR_ARG;
    for (int j = 0; j < i; ++j) {
      const long long oj = p->pictures[j].out_offset;
      if (s.out_offset < ((oj + 3 * N + 3) & ~3LL) && oj < end) return MOBI_ERR_ARG;
    }
    const uintptr_t frame_bytes = (uintptr_t)(s.frame_kind == MOBI_OVERLAY_FRAME_U8_HWC ? 3 * N : 12 * N);
    const uintptr_t out0 = reinterpret_cast<uintptr_t>(p->out);
    if (frame < out0 + (uintptr_t)p->out_bytes && out0 < frame + frame_bytes) return MOBI_ERR_ARG;
    if ((frame & 3) || ((reinterpret_cast<uintptr_t>(s.depth) | reinterpret_cast<uintptr_t>(s.pitch) | reinterpret_cast<uintptr_t>(s.yaw)) & 3))
      return MOBI_ERR_ALIGN;
    lo_picture& o = t[i / LO_LAUNCH].p[i % LO_LAUNCH];
    o.depth = s.depth, o.pitch = s.pitch, o.yaw = s.yaw, o.frame = reinterpret_cast<const unsigned char*>(frame);
    o.out_off = s.out_offset, o.kind = s.frame_kind;
    for (int k = 0; k < 12; ++k) o.m[k] = s.matrix[k];
  }
  unsigned* keys = reinterpret_cast<unsigned*>(p->workspace);
  unsigned* rec = keys + (long long)p->n_pictures * stride;
  if (hipMemsetAsync(p->workspace, 0, mobi_lidar_overlay_workspace_bytes(p->n_pictures, p->H, p->W), ST(stream)) != hipSuccess)
    return MOBI_ERR_LAUNCH;
  const int sweep_blocks = (int)(((long long)p->h0 * p->w0 + 255) / 256);
  const long long groups = (N + 3) / 4;
  const int frame_blocks = (int)((groups + 255) / 256 > 4096 ? 4096 : (groups + 255) / 256);
  for (int lo = 0; lo < p->n_pictures; lo += LO_LAUNCH) {
    const int n = p->n_pictures - lo < LO_LAUNCH ? p->n_pictures - lo : LO_LAUNCH;
    const lo_args a = {keys + (long long)lo * stride, rec + lo * LO_REC, p->lut, p->out, p->out_bytes,
                       p->records_offset + 4LL * LO_REC * lo, stride, p->h0, p->w0, p->H, p->W, p->point_size};
    hipLaunchKernelGGL(lidar_overlay_splat_kernel, dim3(sweep_blocks, n), dim3(256), 0, ST(stream), a, t[lo / LO_LAUNCH]);
    hipLaunchKernelGGL(lidar_overlay_resolve_kernel, dim3(frame_blocks, n), dim3(256), 0, ST(stream), a, t[lo / LO_LAUNCH]);
  }
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_paste_patch(const float* patch, int32_t hs, int32_t ws, uint8_t* frame, int32_t H, int32_t W,
                                int32_t top, int32_t left, int32_t crop_h, int32_t crop_w, void* stream) {
  if (!patch || !frame || hs <= 0 || ws <= 0 || H <= 0 || W <= 0 || crop_h <= 0 || crop_w <= 0) return MOBI_ERR_ARG;
  hipLaunchKernelGGL(paste_patch_kernel, dim3(egrid_pp((long long)crop_h * crop_w)), dim3(256), 0, ST(stream), patch, hs,
                     ws, frame, H, W, top, left, crop_h, crop_w);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_gaussian_blur(const float* src, float* tmp, float* dst, int32_t H, int32_t W, const float* kern,
                                  int32_t ksize, void* stream) {
  if (!src || !tmp || !dst || !kern || H <= 0 || W <= 0 || ksize <= 0 || !(ksize & 1)) return MOBI_ERR_ARG;
  const int g = egrid_pp((long long)H * W);
  hipLaunchKernelGGL(blur_pass_kernel, dim3(g), dim3(256), 0, ST(stream), src, tmp, H, W, kern, ksize, 1);
  hipLaunchKernelGGL(blur_pass_kernel, dim3(g), dim3(256), 0, ST(stream), (const float*)tmp, dst, H, W, kern, ksize, 0);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_blend_frame(const float* mask_blur, const float* image, const uint8_t* pred, float* out, int32_t H,
                                int32_t W, void* stream) {
  if (!mask_blur || !image || !pred || !out || H <= 0 || W <= 0) return MOBI_ERR_ARG;
  hipLaunchKernelGGL(blend_kernel, dim3(egrid_pp((long long)H * W)), dim3(256), 0, ST(stream), mask_blur, image, pred, out,
                     H, W);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_range_prepare(const mobi_range_prepare_params* p, void* stream) {
  if (!p || !p->depth_orig || !p->int_orig || !p->crop_left || !p->width_crop || !p->edit_mask || !p->range_data ||
      !p->range_data_inpaint) return MOBI_ERR_ARG;
  if ((p->inst_orig != nullptr) != (p->inst_out != nullptr)) return MOBI_ERR_ARG;
  if (p->object_norm && (!p->min_depth || !p->max_depth)) return MOBI_ERR_ARG;
  if (p->batch <= 0 || p->h0 <= 0 || p->w0 <= 0 || p->height <= 0 || p->width <= 0) return MOBI_ERR_ARG;
  // (whole-factor REDUCTIONS take the reference's pooling branch, lidar_converter.py:262-267; MObI's views enlarge)
  if (p->height < p->h0) return MOBI_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(range_prepare_kernel, dim3(egrid_pp((long long)p->batch * p->height * p->width)), dim3(256), 0,
                     ST(stream), *p);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_box_mask(const int32_t* corners_xy, float* out, int32_t* stats, int32_t batch, int32_t H, int32_t W,
                             void* stream) {
  if (!corners_xy || (!out && !stats) || batch <= 0 || H <= 0 || W <= 0) return MOBI_ERR_ARG;
  int gx = egrid_pp((long long)H * W);
  gx = gx > 256 ? 256 : gx;
  hipLaunchKernelGGL(box_mask_kernel, dim3(gx, batch), dim3(256), 0, ST(stream), corners_xy, out, stats, batch, H, W);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_image_prepare(const mobi_image_prepare_params* p, void* stream) {
  if (!p || !p->frames || !p->corners_xy || !p->invert || !p->crop || !p->gt || !p->inpaint || !p->mask) return MOBI_ERR_ARG;
  if (p->batch <= 0 || p->H <= 0 || p->W <= 0 || p->height <= 0 || p->width <= 0) return MOBI_ERR_ARG;
  hipLaunchKernelGGL(image_prepare_kernel, dim3(egrid_pp((long long)p->batch * p->height * p->width)), dim3(256), 0,
                     ST(stream), *p);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_ref_augment(const mobi_ref_augment_params* p, void* stream) {
  if (!p || !p->src || !p->flags || !p->warp || !p->table || !p->out) return MOBI_ERR_ARG;
  if (p->batch <= 0 || p->size <= 0) return MOBI_ERR_ARG;
  if (p->size < 8 || p->size > 4096 || p->batch > 65535) return MOBI_ERR_UNSUPPORTED;   // (reflection needs size > halo)
  const int tiles = (p->size + RA_TILE - 1) / RA_TILE;
  hipLaunchKernelGGL(ref_augment_kernel, dim3(tiles, tiles, p->batch), dim3(256), 0, ST(stream), *p);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}

extern "C" int mobi_drop_context(float* gt, float* inpaint, const float* mask, const int32_t* flag, int32_t batch,
                                 int32_t channels, int64_t hw, void* stream) {
  if (!gt || !inpaint || !mask || !flag || batch <= 0 || channels <= 0 || hw <= 0) return MOBI_ERR_ARG;
  if (batch > 65535) return MOBI_ERR_UNSUPPORTED;
  const bool wide = hw % 4 == 0 && ((reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(inpaint) |
                                     reinterpret_cast<uintptr_t>(mask)) & 15) == 0;
  int gx = egrid_pp(wide ? hw / 4 : hw);
  gx = gx > 256 ? 256 : gx;
  if (wide)
    hipLaunchKernelGGL(drop_context_kernel<float4>, dim3(gx, batch), dim3(256), 0, ST(stream), gt, inpaint, mask, flag,
                       channels, (long long)hw);
  else
    hipLaunchKernelGGL(drop_context_kernel<float>, dim3(gx, batch), dim3(256), 0, ST(stream), gt, inpaint, mask, flag,
                       channels, (long long)hw);
  MOBI_CHECK_LAUNCH();
  return MOBI_OK;
}
