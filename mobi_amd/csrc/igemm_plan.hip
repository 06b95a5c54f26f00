// The launch plan of mobi_igemm, decided once per call: checks, geometry, route (igemm_plan), and the entry points that launch
// nothing.  Host code only: csrc/igemm.hip launches what IgemmPlan says (bodies, tiles and conditions: DESIGN.md section 4).
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "igemm_plan.h"
#include "tuning.h"

namespace mobi {
namespace {

constexpr long long I32_MAX = 0x7fffffffLL;

// CUs of the current device (cached per device ordinal); 256 on MI355X.  MOBI_IGEMM_PERSIST_BLOCKS overrides the
// persistent grid size (tests: few blocks walk many output tiles).
int compute_units() {
  if (tuning().persist_blocks > 0) return tuning().persist_blocks;
  static int cached[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cached[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

// Small problems go to csrc/igemm_small.hip (coalesced loads, a wave-private LDS transposition, k split over the block's four
// waves, no slabs): returns its tile (32), or 0.  Rules (tools/small_lab.py, graph-timed on cold operands,
// profiles/r04_small_lab.txt):
//   1 x 1: up to 1.8 GFLOP of 2 M N K -- 1.0 GFLOP at K = 320, where a wave has a single batch and the LDS kernels' launch is a
//          10-step loop (8192 x 320 x 320: 16.6 against 12.6 us; 4096 x 320 x 320: 9.9 against 11.8);
//   3 x 3 (pad 1, stride 1): NOT routed (MOBI_IGEMM_SMALL_CONV_M output pixels, default 0) -- built for the 4 x 4 levels of
//          `mobi_nusc_256` (128 pixels, 30-60 MB of weights per launch) and measured SLOWER there: 36.1 against 24.7 us
//          (1280 -> 1280), 66 against 35 (2560 -> 1280): a wave walks 36-72 batches one HBM latency after the other, and 160
//          blocks of four waves are 2.5 waves per CU (profiles/r04_small_lab_conv.txt).  Kept for tests and the A/B.
// MOBI_IGEMM_SMALL_MFLOP overrides the 1 x 1 cap; MOBI_IGEMM_SMALL=0 never; 32: every eligible launch whatever its size (A/B, tests).
constexpr int SMALL_MFLOP_DEFAULT = 1800, SMALL_MFLOP_K320 = 1000, SMALL_CONV_M_DEFAULT = 0;
int small_tile(const mobi_igemm_params* p) {
  if (tuning().small == 0) return 0;
  // a forced tile geometry (the A/B knobs of the LDS kernels) keeps the launch on them unless this kernel is forced too
  if (tuning().small < 0 && (tuning().wm == 2 || tuning().wm == 4 || tuning().wide >= 0 || tuning().sm == 0)) return 0;
  const bool conv3 = p->kh == 3 && p->kw == 3 && p->pad_h == 1 && p->pad_w == 1;
  if (!(p->kh == 1 && p->kw == 1) && !conv3) return 0;
  if (p->stride != 1 || p->upsample || p->groups != 1 || p->epilogue != MOBI_EPI_NONE || p->k_order != 0 || p->split_k > 1) return 0;
  if (p->out_mode != MOBI_OUT_ROWS && p->out_mode != MOBI_OUT_ROWS_F32) return 0;
  if (p->hout != p->hin || p->wout != p->win) return 0;
  const int ct = p->c0 + p->c1, N = p->n_packed;
  const long long K = (long long)ct * p->kh * p->kw;
  if (ct % 320 || (p->c1 > 0 && p->c0 % 80) || N != p->cout || N % 32) return 0;
  const long long hw = (long long)p->hin * p->win, M = (long long)p->batch * hw;
  const long long ips = p->src_img_stride ? p->src_img_stride / p->c0 : hw;
  const long long cmax = p->c0 > p->c1 ? p->c0 : p->c1;
  if ((((long long)p->batch - 1) * ips + hw) * cmax * 2 >= I32_MAX || (long long)N * K * 2 >= I32_MAX) return 0;
  if (tuning().small > 0) return 32;
  if (conv3) {
    const int cap_m = tuning().small_conv_m >= 0 ? tuning().small_conv_m : SMALL_CONV_M_DEFAULT;
    return M <= cap_m ? 32 : 0;
  }
  const int cap = tuning().small_mflop >= 0 ? tuning().small_mflop : (K == 320 ? SMALL_MFLOP_K320 : SMALL_MFLOP_DEFAULT);
  if (2.0 * (double)M * N * (double)K > 1e6 * cap) return 0;
  return 32;
}

// split-K plan: only when the tile grid cannot fill the chip and k is long
int plan_splits(long long M, int n_packed, int ktot) {
  const int bn = (n_packed % 160) == 0 ? 160 : 128;
  const long long tiles = ((M + 127) / 128) * ((n_packed + bn - 1) / bn);
  const int nk = (ktot + 63) / 64;
  // round 5 (profiles/r05_split_sweep.txt, slabs + reduce launch timed together): 20 k-tiles never pay for a second launch
  // ([2048 | 1024 x 1280 x 1280] 22.2 / 20.7 us unsplit against 23.3 / 21.1 split in two; [8192 x 320 x 1280] 21.9 against 23.3)
  const bool r5 = tuning().split_round4 != 0;   // MOBI_IGEMM_SPLIT_ROUND4=0: round 4's plan (A/B)
  if (tiles >= 384 || nk < (r5 ? 24 : 16)) return 1;
  if (tiles >= 256 && (r5 ? nk <= 40 : nk < 40)) return 1;   // one full wave of blocks, short k ([4096 x 1280 x 2560]: 40.3 us unsplit, 44.1 in two)
  const long long target = tuning().split_target > 0 ? tuning().split_target : 512;      // MOBI_IGEMM_SPLIT_TARGET (sweeps)
  long long s = (target + tiles - 1) / tiles;
  const long long cap = tiles <= 16 ? 16 : 8;               // a handful of tiles (the 4x4 / 8x8 levels): measured best at 16
  if (s > cap) s = cap;
  if (s > nk / 8) s = nk / 8;
  // the reduce launch sums four slabs per round: 5 .. 7 splits buy a second round for little more parallelism ([1024 x 1280 x 2560]
  // 23.6 us at 4 against 29.5 at 5; [2048 x 640 x 2560] 23.0 against 28.3), and so do 8 on 64 tiles or more with at most 96 k-tiles
  // ([1024 x 1280 x 5120] 31.3 against 35.7, [2048 x 640 x 5760] 32.6 against 35.7; fewer tiles still want 8: [512 x 1280 x 5120])
  if (r5) {
    if (s > 4 && s < 8) s = 4;
    if (s == 8 && nk <= 96 && tiles >= 64) s = 4;
  }
  // one round of 128-pixel tiles and a very long k range per split (the 16 x 16 level's 1280 -> 1280 and 2560 -> 1280 3 x 3
  // convolutions: 90 / 180 k-tiles per split at s = 2): twice the splits -- 114.7 against 126.3 us and 198.8 against 225.3
  // (tools/sweep_split.py), -0.08 ms per step; MOBI_IGEMM_SPLIT_LONGK=0 keeps the old plan (A/B)
  if (tiles >= 128 && tiles <= 256 && s >= 2 && nk / s >= 80 && tuning().split_longk != 0) s *= 2;
  return s < 2 ? 1 : (int)s;
}

long long image_pixel_stride(const mobi_igemm_params* p) {
  return p->src_img_stride ? p->src_img_stride / p->c0 : (long long)p->hin * p->win;
}
bool misaligned(const void* q, uintptr_t mask = 15) { return (reinterpret_cast<uintptr_t>(q) & mask) != 0; }

// ---- step 1, checks: what the parameters alone decide.  The first rule broken gives the error (the order is the contract's)
int check_args(const mobi_igemm_params* p) {
  if (!p || !p->src0 || !p->weight || !p->out) return MOBI_ERR_ARG;
  if (p->dtype != MOBI_F16 && p->dtype != MOBI_BF16) return MOBI_ERR_ARG;
  if (p->c0 <= 0 || (p->c0 & 31) || p->c1 < 0 || (p->c1 & 31) || (p->c1 > 0 && !p->src1)) return MOBI_ERR_UNSUPPORTED;
  if (p->batch <= 0 || p->hin <= 0 || p->win <= 0 || p->hout <= 0 || p->wout <= 0) return MOBI_ERR_ARG;
  if (p->kh <= 0 || p->kw <= 0 || p->stride <= 0 || p->groups <= 0 || p->batch % p->groups) return MOBI_ERR_ARG;
  if (p->cout <= 0 || p->n_packed <= 0) return MOBI_ERR_ARG;
  if (p->upsample != 0 && p->upsample != 1) return MOBI_ERR_ARG;
  const bool geglu = p->epilogue == MOBI_EPI_GEGLU;
  const bool leaky = p->epilogue == MOBI_EPI_LEAKY_RELU;
  const bool tr = p->out_mode == MOBI_OUT_TRANSPOSED;
  if (p->epilogue != MOBI_EPI_NONE && !geglu && !leaky) return MOBI_ERR_ARG;
  // leaky ReLU: row-major output, one pass, no LayerNorm fold, tap-major k (the ring kernels' staged epilogue applies it)
  if (leaky && (tr || p->ln_svec || p->split_k > 1 || p->k_order != 0)) return MOBI_ERR_UNSUPPORTED;
  if (p->out_mode < 0 || p->out_mode > 2) return MOBI_ERR_ARG;
  if (!tr && (p->cout & 7)) return MOBI_ERR_UNSUPPORTED;
  if (geglu && (p->out_mode != MOBI_OUT_ROWS || p->rowvec || p->residual)) return MOBI_ERR_UNSUPPORTED;
  if (p->n_packed != (geglu ? 2 * p->cout : p->cout)) return MOBI_ERR_ARG;
  if (tr && (p->rowvec || p->residual)) return MOBI_ERR_UNSUPPORTED;
  if (misaligned(p->bias) || misaligned(p->rowvec)) return MOBI_ERR_ALIGN;
  if (p->rowvec && (p->rowvec_stride & 3)) return MOBI_ERR_ALIGN;
  if (misaligned(p->src0) || misaligned(p->src1) || misaligned(p->weight) || misaligned(p->out) || misaligned(p->residual))
    return MOBI_ERR_ALIGN;
  // LayerNorm folded into the launch (ln_fold_acc): a 1 x 1 product of ONE source whose block sweeps all of k
  if (p->ln_svec) {
    if (p->kh != 1 || p->kw != 1 || p->c1 || p->stride != 1 || p->upsample || p->groups != 1 || p->split_k > 1 || p->rowvec ||
        p->residual || tr || p->scale != 1.0f || p->k_order != 0 || p->hout != p->hin || p->wout != p->win)
      return MOBI_ERR_UNSUPPORTED;
    if (misaligned(p->ln_svec)) return MOBI_ERR_ALIGN;
  }
  if (p->src_img_stride && (p->c1 || p->src_img_stride % p->c0)) return MOBI_ERR_UNSUPPORTED;
  if (image_pixel_stride(p) * p->batch > I32_MAX) return MOBI_ERR_UNSUPPORTED;
  // tap-major k only: the chunk-major order (1) measured slower and no kernel is routed for it any more
  if (p->k_order != 0) return p->k_order == 1 ? MOBI_ERR_UNSUPPORTED : MOBI_ERR_ARG;
  return MOBI_OK;
}

struct Geometry {
  bool ring_ok;   // the 32-bit buffer offsets of the LDS-DMA kernels reach every operand byte (each operand below 2 GB)
  bool k64;       // channel runs of 64: a 64-deep k-tile never straddles a tap or a source
  bool nt5;       // n_packed % 160 == 0: channel tiles of 160 (320), five 16-channel MFMA tiles per wave, instead of 128 (256)
  int bn;         // 160 | 128
};

// ---- step 2, geometry: the operands as the kernels address them, M, k-tiles, byte extents
Geometry geometry(const mobi_igemm_params* p, IgemmArgs& a) {
  a.ln_svec = p->ln_svec; a.ln_eps = p->ln_eps;
  a.src0 = p->src0; a.src1 = p->src1;
  a.c0 = p->c0; a.c1 = p->c1; a.C = p->c0 + p->c1;
  a.hin = p->hin; a.win = p->win; a.up = p->upsample;
  a.hout = p->hout; a.wout = p->wout; a.hw_out = p->hout * p->wout;
  a.kh = p->kh; a.kw = p->kw; a.stride = p->stride; a.pad_h = p->pad_h; a.pad_w = p->pad_w;
  const long long ips = image_pixel_stride(p);
  a.img_pix_stride = (int)ips;
  a.weight = p->weight; a.w_group_stride = p->groups > 1 ? p->w_group_stride : 0;
  a.n_packed = p->n_packed; a.cout = p->cout;
  a.ktot = p->kh * p->kw * a.C;
  a.nk = (a.ktot + 63) / 64;
  a.imgs_per_group = p->batch / p->groups;
  a.M = a.imgs_per_group * a.hw_out;
  a.bias = p->bias; a.rowvec = p->rowvec; a.residual = p->residual;
  a.rowvec_stride = p->rowvec_stride ? p->rowvec_stride : p->cout;
  a.res_img_stride = p->res_img_stride ? p->res_img_stride : (long long)a.hw_out * p->cout;
  a.out = p->out;
  a.out_img_stride = p->out_img_stride ? p->out_img_stride : (long long)a.hw_out * p->cout;
  a.out_mode = p->out_mode; a.epilogue = p->epilogue; a.scale = p->scale;
  a.k_order = 0;
  auto log2_exact = [](int v) { int s = 0; while ((1 << s) < v) ++s; return (1 << s) == v ? s : -1; };
  a.hw_shift = log2_exact(a.hw_out); a.w_shift = log2_exact(a.wout);
  const long long span = ((long long)p->batch - 1) * ips + (long long)p->hin * p->win;   // pixels from the first image's to the last's end
  const long long ext0 = span * p->c0 * 2, ext1 = p->c1 ? span * p->c1 * 2 : 0, wext = (long long)p->n_packed * a.ktot * 2;
  Geometry g;
  g.ring_ok = ext0 < I32_MAX && ext1 < I32_MAX && wext < I32_MAX;
  g.k64 = a.C % 64 == 0 && (p->c1 == 0 || p->c0 % 64 == 0);
  g.nt5 = p->n_packed % 160 == 0;
  g.bn = g.nt5 ? 160 : 128;
  a.src0_bytes = (int)(ext0 < I32_MAX ? ext0 : 0);
  a.src1_bytes = (int)(ext1 < I32_MAX ? ext1 : 0);
  a.w_bytes = (int)(wext < I32_MAX ? wext : 0);
  return g;
}

// ... and the split ranges: blockIdx.y owns k-tiles [y * nk_per, (y + 1) * nk_per)
int split_ranges(const mobi_igemm_params* p, IgemmArgs& a) {
  a.splits = 1; a.nk_per = a.nk; a.split_ws = nullptr;
  if (p->split_k > 1) {
    if (!p->ws || p->groups != 1 || p->epilogue == MOBI_EPI_GEGLU || p->out_mode == MOBI_OUT_TRANSPOSED || p->split_k > 64)
      return MOBI_ERR_UNSUPPORTED;
    if (misaligned(p->ws)) return MOBI_ERR_ALIGN;
    a.nk_per = (a.nk + p->split_k - 1) / p->split_k;
    a.splits = (a.nk + a.nk_per - 1) / a.nk_per;            // no empty k ranges: every slab that is summed is written
    a.split_ws = reinterpret_cast<float*>(p->ws);
  }
  if (p->defer_finish != 0 && p->defer_finish != 1) return MOBI_ERR_ARG;
  // deferred finish: the slabs are the launch's result -- T rows only (what a consumer reconstructs), never with `sync`
  if (p->defer_finish && (!a.split_ws || p->sync || p->out_mode != MOBI_OUT_ROWS)) return MOBI_ERR_UNSUPPORTED;
  return MOBI_OK;
}

// ---- step 3, route.  First the waves along the pixel axis (block tile = 64 * wm pixels): 256-pixel tiles (4) when that still
// gives every CU a block; MOBI_IGEMM_WM overrides
int pixel_waves(const mobi_igemm_params* p, const IgemmArgs& a, const Geometry& g) {
  const long long tiles256 = ((a.M + 255) / 256) * (long long)((p->n_packed + g.bn - 1) / g.bn);
  int wm = tiles256 >= 256 ? 4 : 2;
  // split-K launches with long k ranges: 256-pixel tiles (ping-pong kernel) once tiles x splits fill the chip
  if (p->split_k > 1 && a.M % 256 == 0 && tiles256 * p->split_k >= 256 && a.nk / p->split_k >= 16) wm = 4;
  if (tuning().pp_split == 0 && p->split_k > 1 && tiles256 < 256) wm = 2;
  if (tuning().wm == 2 || tuning().wm == 4) wm = tuning().wm;
  return wm;
}

// The eight-wave ring kernel's tiles for a launch of the generic rules: 2 = 256 x 320 (256), 1 = 128 x 320 (256), 0 = neither.
// (measured, tools/ab_wide.py: 3x3 convolutions at 64x64 x 16: 1071-1245 vs 813-976 TFLOP/s on the ping-pong kernel;
//  it needs about one block per CU: with 128 tiles -- the 32x32 level at N = 640 -- half the chip idles and it loses;
//  the 128 x 320 tile (twice the blocks at the ping-pong tile's bytes per FLOP) measured 829-965 TFLOP/s there against
//  982-1085 on the ping-pong kernel: kept for A/B (MOBI_IGEMM_WIDE128=1), not routed)
// pp: the ping-pong kernel would take the launch.  MOBI_IGEMM_WIDE: 0 never, 1 | 2 always that tile.
int wide_tiles(const mobi_igemm_params* p, const IgemmArgs& a, const Geometry& g, int wm, bool pp) {
  const int knob = tuning().wide;
  if (!((wm == 4 || knob > 0) && g.ring_ok && knob != 0)) return 0;
  if (p->ln_svec) return wm == 4 ? 2 : 0;                  // the LayerNorm fold lives in the 256 x 320 / 128 x 160 ring tiles
  if (knob > 0) return knob == 1 ? 1 : 2;
  const int bnw = 2 * g.bn;
  const long long tn = (p->n_packed + bnw - 1) / bnw;
  auto fills = [&](long long blocks) {
    const long long rounds = (blocks + 255) / 256;
    return blocks >= 190 && blocks * 5 >= rounds * 256 * 4 - 64 * (rounds == 1);   // rounds about 80 % full on average
                                                                     // (192 blocks, 1280 -> 3840 at 16 x 16 x 16: 43.4 vs 51.7 us)
  };
  const long long t256 = ((a.M + 255) / 256) * tn * a.splits, t128 = ((a.M + 127) / 128) * tn * a.splits;
  int pick = fills(t256) ? 2 : (fills(t128) && tuning().wide128 == 1 ? 1 : 0);
  // a channel tile that is half padding or more (128 output channels in a 256-wide tile: the VAEs' 128-channel levels)
  // loses to the ping-pong kernel's 256 x 128 tile: 878 vs 1160 us on 128 -> 128 3x3 at 512 x 512 x 8 (tools/kbench.py conv)
  if (pick == 2 && p->n_packed * 2 <= bnw && pp) pick = 0;
  // launches of the 256-pixel geometry that the ping-pong kernel's register epilogue does not take (transposed / fp32
  // output, ragged tiles, bias AND per-image vector, per-image weights): the ring kernel's LDS-staged epilogue does
  // (a source of fewer than 64 channels into a wide layer -- the UNet's 9-channel input, padded to 32: a tap per k-step --
  //  stays on the register-staged kernel: 38 against 104 us on 9 -> 320 at 64 x 64 x 16)
  if (!pick && wm == 4 && !pp && (a.C >= 64 || p->out_mode != MOBI_OUT_ROWS || p->n_packed < 256)) pick = 2;
  return pick;
}

// Split-K finished inside the launch: the LDS-DMA kernels (ring tiles of every geometry; the ping-pong kernel when every
// block owns exactly one output tile -- its epilogue is deferred into the next tile's loop otherwise); the register-staged
// fallback keeps the reduce launch.  At most FOUR splits (splitk_finish_tile).  MOBI_IGEMM_FUSED_SPLIT: 0 never (A/B);
// 1 device-coherent slab traffic; 2 (default) the same-XCD form where the grid's x extent (the tile count: one tile per block)
// is a multiple of 8, the reduce launch elsewhere.  Returns the mode, 0 for the reduce launch.
int in_launch_finish(const IgemmArgs& a, Body body, bool ring) {
  const long long tiles = (long long)a.tiles_m * a.tiles_n;
  const int mode = tuning().fused_split == 1 ? 1 : 2;
  const bool can = ring || (body == Body::PingPong && tiles <= (long long)compute_units());
  return can && (mode == 1 || tiles % 8 == 0) ? mode : 0;
}

int route(const mobi_igemm_params* p, const Geometry& g, const int wm, IgemmPlan& pl) {
  IgemmArgs& a = pl.a;
  const Tuning& t = tuning();
  const bool rows = p->out_mode == MOBI_OUT_ROWS, tr = p->out_mode == MOBI_OUT_TRANSPOSED, split = a.split_ws != nullptr;
  const bool lnf = p->ln_svec != nullptr, leaky = p->epilogue == MOBI_EPI_LEAKY_RELU;
  const int npk = p->n_packed, bn = g.bn, bnw = 2 * g.bn;
  // a per-image vector takes a register epilogue's bias registers: never both, and every wave's pixels inside one image
  auto vec_ok = [&](int wave_pixels) { return !p->rowvec || (!p->bias && a.hw_out % wave_pixels == 0); };
  // the ping-pong kernel: k-tiles that never straddle a tap or a source (fast), every tile full, >= 3 k-tiles per range, window
  // pixels linear in the tap (no scale, image sides powers of two) -- with its register epilogue (row-major T output, no
  // per-image vector beside a bias) or, split, fp32 slabs from the registers, finished by the reduce launch
  const bool fast = g.k64 && g.ring_ok && t.fast != 0, glds = t.glds != 0;
  const bool pp_tiles = wm == 4 && fast && glds && a.M % 256 == 0 && npk % bn == 0 && a.nk_per >= 3;
  const bool pp_window = p->scale == 1.0f && a.hw_shift >= 6 && a.w_shift >= 0 && a.hout < 32768 && a.wout < 32768;
  const bool epi_direct = pp_tiles && rows && !split && vec_ok(64) && t.epi_direct != 0;
  const bool pp = (split ? pp_tiles && !tr : epi_direct) && pp_window && t.pp != 0;
  const int wide = wide_tiles(p, a, g, wm, pp);
  const bool pix256 = wide ? wide == 2 : wm == 4;
  Body body;
  if (leaky) {
    // MOBI_EPI_LEAKY_RELU lives in the ring kernels' LDS-staged epilogue only: 256 x 256 (320) tiles for launches of the
    // 256-pixel geometry with at least 256 output channels, 128 x 128 (160) tiles otherwise; the register epilogues, the
    // ping-pong / direct / small kernels and the 64-deep ring never see it.  Operands beyond the ring's 2 GB: unsupported.
    if (!g.ring_ok) return MOBI_ERR_UNSUPPORTED;
    body = pix256 && npk >= 256 ? Body::Ring256 : Body::Ring128;
  }
  else if (wide) body = wide == 2 ? Body::Ring256 : Body::Ring128W;
  else if (pp) body = Body::PingPong;
  else if (wm == 4) body = Body::Staged256;
  // 128-pixel tiles: the LDS-DMA ring kernel whenever the 32-bit buffer offsets reach every operand byte
  // (k-steps are 32 deep there: channel counts are multiples of 32 by the ABI's own rule)
  else body = g.ring_ok && t.sm != 0 ? Body::Ring128 : Body::Staged128;
  pl.tile_m = body == Body::Ring256 || body == Body::PingPong || body == Body::Staged256 ? 256 : 128;
  pl.tile_n = body == Body::Ring256 || body == Body::Ring128W ? bnw : bn;
  a.tiles_m = (a.M + pl.tile_m - 1) / pl.tile_m;
  a.tiles_n = (npk + pl.tile_n - 1) / pl.tile_n;
  if ((long long)a.tiles_m * a.tiles_n > I32_MAX) return MOBI_ERR_UNSUPPORTED;
  // 64-deep steps for the 128-pixel geometry: channel runs of 64 (a k-step never straddles a tap or a source), >= 3 steps
  // (one block per CU: only grids of at most one round of blocks -- with more, two co-resident blocks of the 32-deep ring win:
  //  36.2 vs 45.3 us on 320 -> 320 3x3 at 32 x 32 x 8 split 4, tools/ab_sm64.py); MOBI_IGEMM_SM64: 0 never, 1 every grid
  const long long blocks = (long long)a.tiles_m * a.tiles_n * a.splits * p->groups;
  if (body == Body::Ring128 && !leaky && g.k64 &&
      (t.sm64 == 1 || (a.nk_per >= 1 && blocks <= (long long)compute_units() && t.sm64 != 0)))
    body = Body::Ring64;
  const bool ring = body != Body::PingPong && body != Body::Staged256 && body != Body::Staged128;
  if (lnf && !ring) return MOBI_ERR_UNSUPPORTED;            // (operands beyond the ring kernels' 2 GB: LayerNorm as a launch)
  // order of the work list (tile_of): by channel tile when a 1 x 1 launch's weights outweigh the activations it reads --
  // every XCD's L2 then fetches its slice of the weights and all of the (smaller) activations instead of all of the weights
  // and its slice of the activations.  Measured (tools/ab_nmajor.sh): the 16 x 16 level's GEGLU projection (26 MB of weights,
  // 10.5 MB of activations) 219-223 against 233-237 us; 3 x 3 convolutions LOSE 3-6 % (143.7 vs 139.5 us at 1280 -> 1280,
  // 16 x 16: nine taps re-read the whole activation tensor through every L2), so they keep the pixel-major order.
  // (never the ping-pong kernel, which always walks pixel-major, nor a leaky launch)
  const long long wbytes = (long long)npk * a.ktot * 2, abytes = (long long)p->batch * p->hin * p->win * a.C * 2;
  a.n_major = body != Body::PingPong && !leaky && p->groups == 1 &&
              (t.n_major == 1 || (a.tiles_n >= 2 && p->kh * p->kw == 1 && wbytes > abytes && t.n_major != 0));
  a.w_tiled = (p->weight_tiled && ring && body != Body::Ring64 &&
               (p->groups == 1 || p->w_group_stride == (long long)npk * a.ktot) && npk % 16 == 0 && a.ktot % 32 == 0 &&
               !misaligned(p->weight_tiled) && t.w_tiled != 0) ? p->weight_tiled : nullptr;
  // 128-pixel ring tiles: register epilogue / slab stores when every tile is full (the staged epilogue keeps ragged tiles,
  // transposed / fp32 output, bias AND per-image vector)
  // (groups: every group's rows are whole tiles -- a.M is the rows of ONE group -- and the epilogue addresses rows, residual and
  //  per-image vector through the group's first image; the bias is shared by the groups)
  a.sm_direct = ring && body != Body::Ring256 && !leaky && (rows || split) && !tr && a.M % 128 == 0 && npk % pl.tile_n == 0 &&
                (split || vec_ok(64)) && t.sm_direct != 0;
  // 256 x 320 ring tiles: the same, one k pass, one weight matrix
  // (with a residual the staged epilogue is as fast or a microsecond faster: 28.1 vs 29.2 us on 320 -> 320 1x1 at 64 x 64 x 16,
  //  98.9 vs 100.2 on the 3x3; MOBI_IGEMM_RING_DIRECT=1 forces the register epilogue there too)
  a.ring_direct = body == Body::Ring256 && !leaky && rows && !split && p->groups == 1 && vec_ok(128) && a.M % 256 == 0 &&
                  npk % bnw == 0 && p->scale == 1.0f && (p->residual ? t.ring_direct == 1 : t.ring_direct != 0);
  const int small = lnf || leaky ? 0 : small_tile(p);
  a.sync = nullptr; a.sync_mode = 0;
  if (split && p->sync && !small && t.fused_split != 0 && a.splits <= 4 && (long long)a.splits * a.M * npk * 4 < I32_MAX) {
    if (misaligned(p->sync, 3)) return MOBI_ERR_ALIGN;
    a.sync_mode = in_launch_finish(a, body, ring);
    if (a.sync_mode) a.sync = reinterpret_cast<int*>(p->sync);
  }
  a.fast = fast; a.glds = glds; a.wm = pl.tile_m / 64; a.lin_window = 0; a.small = small;   // (the flags no kernel reads)
  a.epi_direct = epi_direct && !leaky; a.pp = pp && !leaky;
  a.sm = body == Body::Ring128 || body == Body::Ring64; a.sm64 = body == Body::Ring64;
  a.wide = body == Body::Ring256 ? 2 : body == Body::Ring128W ? 1 : 0;
  static const int variant[] = {MOBI_IGEMM_STAGED_128, MOBI_IGEMM_STAGED_256, MOBI_IGEMM_PINGPONG, MOBI_IGEMM_RING_128,
                                MOBI_IGEMM_RING_128, MOBI_IGEMM_RING_256, MOBI_IGEMM_RING_128W, MOBI_IGEMM_SMALL};
  pl.body = small ? Body::Small : body;
  if (small) pl.tile_m = pl.tile_n = small;
  // (MOBI_IGEMM_DIRECT_LDS: the register-staged 256-pixel kernel on a launch the former direct-to-LDS kernel would have taken)
  pl.variant = pl.body == Body::Staged256 && fast && glds ? MOBI_IGEMM_DIRECT_LDS : variant[(int)pl.body];
  return MOBI_OK;
}

}  // namespace

int igemm_plan(const mobi_igemm_params* p, IgemmPlan& pl) {
  IgemmArgs& a = pl.a;
  int rc = check_args(p);
  if (rc != MOBI_OK) return rc;
  const Geometry g = geometry(p, a);
  const int wm = pixel_waves(p, a, g);
  if ((long long)((a.M + 64 * wm - 1) / (64 * wm)) * ((p->n_packed + g.bn - 1) / g.bn) > I32_MAX) return MOBI_ERR_UNSUPPORTED;
  if ((rc = split_ranges(p, a)) != MOBI_OK) return rc;
  if ((rc = route(p, g, wm, pl)) != MOBI_OK) return rc;
  // the launch: template arguments, grid (ping-pong kernel: persistent, at most one 156-KB-LDS block per CU), block, and whether a
  // second launch sums the slabs (with `sync` the tile's last block has; with defer_finish the consumer or mobi_igemm_finish does)
  const bool small = pl.body == Body::Small;
  pl.nt5 = g.nt5; pl.tr = p->out_mode == MOBI_OUT_TRANSPOSED; pl.lnf = p->ln_svec != nullptr;
  pl.leaky = p->epilogue == MOBI_EPI_LEAKY_RELU; pl.geglu = p->epilogue == MOBI_EPI_GEGLU; pl.slab = a.split_ws != nullptr;
  pl.ovl = tuning().sm64_ovl != 0;           // Ring64: requests dealt out between the MFMAs (MOBI_IGEMM_SM64_OVL=0: the sequential step, the A/B partner)
  const unsigned tiles = (unsigned)(a.tiles_m * a.tiles_n), cus = (unsigned)compute_units();
  pl.grid[0] = pl.body == Body::PingPong && tiles > cus ? cus : tiles;
  pl.grid[1] = (unsigned)a.splits; pl.grid[2] = (unsigned)p->groups;
  pl.block = pl.body == Body::Ring128 || pl.body == Body::Ring64 || pl.body == Body::Staged128 ? 256 : 512;
  pl.reduce_after = !small && a.split_ws && !a.sync && !p->defer_finish;
  return MOBI_OK;
}

}  // namespace mobi

extern "C" int mobi_igemm_plan_splits(const mobi_igemm_params* p) {
  // (GEGLU and MOBI_EPI_LEAKY_RELU launches never split)
  if (!p || p->groups != 1 || p->epilogue != MOBI_EPI_NONE || p->out_mode == MOBI_OUT_TRANSPOSED || p->ln_svec) return 1;
  {
    mobi_igemm_params q = *p;
    q.split_k = 0;
    if (mobi::small_tile(&q)) return 1;
  }
  return mobi::plan_splits((long long)p->batch * p->hout * p->wout, p->n_packed, p->kh * p->kw * (p->c0 + p->c1));
}

extern "C" size_t mobi_igemm_workspace_bytes(const mobi_igemm_params* p, int32_t splits) {
  if (!p || splits <= 1) return 0;
  return (size_t)splits * p->batch * p->hout * p->wout * p->n_packed * sizeof(float);
}

// arrival counters of a split launch that finishes itself: one int per output tile of the SMALLEST tile geometry (128 pixels
// x 128 channels), whichever kernel runs it
extern "C" size_t mobi_igemm_sync_bytes(const mobi_igemm_params* p, int32_t splits) {
  if (!p || splits <= 1) return 0;
  const size_t m = (size_t)p->batch * p->hout * p->wout;
  return ((m + 127) / 128) * (((size_t)p->n_packed + 127) / 128) * sizeof(int32_t);
}

extern "C" int32_t mobi_igemm_slab_count(const mobi_igemm_params* p) {
  mobi::IgemmPlan pl;
  const int rc = mobi::igemm_plan(p, pl);
  if (rc != MOBI_OK) return rc;
  return pl.body == mobi::Body::Small ? 1 : pl.a.splits;
}

extern "C" int mobi_igemm_kernel_variant(const mobi_igemm_params* p) {
  mobi::IgemmPlan pl;
  const int rc = mobi::igemm_plan(p, pl);
  return rc != MOBI_OK ? rc : pl.variant;
}
