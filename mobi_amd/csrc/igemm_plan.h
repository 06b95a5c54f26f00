// The launch plan of mobi_igemm (csrc/igemm_plan.hip decides it, csrc/igemm.hip launches it) and the kernels' argument block.
// Host-only C++: nothing here or in igemm_plan.hip is device code, so the plan builds and runs without the kernels.
#pragma once
#include <stdint.h>

#include "../../include/mobi_engine.h"

namespace mobi {

struct IgemmArgs {
  const void* src0; const void* src1;
  int c0, c1, C;
  int hin, win, up, hout, wout, hw_out;
  int kh, kw, stride, pad_h, pad_w;
  int img_pix_stride;      // pixels between images of the sources (elements / channels)
  const void* weight; long long w_group_stride;
  int n_packed, cout, ktot, nk;
  int M;                 // rows per group
  int imgs_per_group;
  const float* bias; const float* rowvec; int rowvec_stride;
  const void* residual; long long res_img_stride;
  void* out; long long out_img_stride;
  int out_mode, epilogue;
  float scale;
  int tiles_m, tiles_n;
  int n_major;             // work list walks the pixel tiles of one channel tile first (launches whose weights outweigh their activations)
  int src0_bytes, src1_bytes, w_bytes, fast, glds;
  int k_order;             // always 0 (k = tap*C + c); igemm_pp_kernel still tests it (the field is part of the argument block)
  int wm;
  int splits, nk_per;      // split-K: blockIdx.y owns k-tiles [y*nk_per, (y+1)*nk_per)
  float* split_ws;         // f32 [splits][M][n_packed] partial sums (NULL: single pass)
  const float* ln_svec;    // LayerNorm folded into this 1 x 1 launch (see ln_fold_acc): row sums of the packed W diag(gamma), or NULL
  float ln_eps;
  int sync_mode;           // 0: no `sync`; 1: device-coherent slab traffic; 2: a tile's blocks share one XCD's L2 (see splitk_arrive_and_finish)
  int* sync;               // split-K finished inside the launch: one arrival counter per output tile (zero before and after
                           // the launch), or NULL: the slabs are summed by igemm_splitk_reduce_kernel (a second launch)
  int ring_direct;         // 256 x 320 ring tiles: register epilogue (full tiles, row-major T output, bias OR per-image vector)
  int sm_direct;           // 128 x 160 ring tiles: register epilogue / register slab stores (full tiles)
  const void* w_tiled;     // W as 1-KiB request images (ring kernels), or NULL
  int sm64;
  int lin_window;
  int epi_direct;
  int pp;
  int sm;
  int wide;
  int hw_shift, w_shift;   // log2(hw_out), log2(wout) when both are powers of two (ping-pong kernel), else -1
  int small;
  // NO KERNEL READS fast, glds, wm, sm64, lin_window, epi_direct, pp, sm, wide, small: the route's working flags of an earlier
  // plan.  igemm_plan() still writes the values that plan gave them (lin_window 0), so the block a kernel receives is
  // unchanged, and no host code reads them back -- the route is IgemmPlan::body.  They leave with the struct's next layout change.
};

// The main loop of a launch: its tile, kernel and conditions are the table of DESIGN.md section 4.  Small: csrc/igemm_small.hip
// runs, and `a` holds what the launch would have had on the kernels of csrc/igemm.hip.
enum class Body { Staged128, Staged256, PingPong, Ring128, Ring64, Ring256, Ring128W, Small };

struct IgemmPlan {
  Body body;
  int variant;                     // what mobi_igemm_kernel_variant answers (MOBI_IGEMM_*), decided with the body
  int tile_m, tile_n;              // the body's pixel and channel tile
  bool nt5, tr, lnf, leaky, geglu, slab, ovl;   // the template arguments launch_igemm picks the instantiation by
  unsigned grid[3], block;
  bool reduce_after;               // the slabs are summed by a second launch (igemm_splitk_reduce_kernel)
  IgemmArgs a;                     // what the kernel reads
};

// Argument checks + plan: MOBI_OK, or the error mobi_igemm returns for these parameters (nothing is launched).
int igemm_plan(const mobi_igemm_params* p, IgemmPlan& pl);

}  // namespace mobi
