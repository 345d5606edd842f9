// What the split-K weight-gradient launchers share: the planner that cuts the pixel (K) range into chunks, and the deterministic-mode
// wrapper around a launch (det.h).  A launcher is: plan, grid, wgrad_launch([&](dst, group_stride, slice_stride) { kernel launch }).
#pragma once
#include <math.h>
#include "conv_launch.h"
#include "det.h"

struct SplitK {
  int chunks, chunk_len;
};

static inline SplitK split_k_lengths(int P, int chunks, int k_step) {
  const int chunk_len = ((cdiv(P, chunks) + k_step - 1) / k_step) * k_step;
  return SplitK{cdiv(P, chunk_len), chunk_len};
}

// Split the P pixels of the contraction (chunks of >= 512 pixels, at most 64, whole K-steps; fp32 atomics or det.h combine them) so that
// the launch fills the chip in whole "rounds": `slots` workgroups are resident at once (LDS-limited, a constant of each kernel), and e.g.
// 1152 workgroups on 1024 slots leave 7/8 of the CUs idle for the last ninth of the work (measured -10 % on the 3x3 layers).  Take the
// smallest split whose last round is >= 93 % full, else the best one.  work = tiles * images: the workgroups of an unsplit launch.
// chunk_cap > 0: at most that many chunks (a grid-dimension limit), applied to the choice, before the lengths are rounded.
static inline SplitK plan_split_k(i64 work, int P, int slots, int k_step, int chunk_cap = 0) {
  int chunks = 1;
  double best = -1.0;
  for (int c = 1; c <= 64 && (c == 1 || P / c >= 512); ++c) {
    const double rounds = (double)work * c / (double)slots;
    const double eff = rounds < 2.0 ? 0.45 * rounds : rounds / ceil(rounds);    // want >= 2 rounds: 1x1 layers measured best there
    if (eff > best + 0.02) { best = eff; chunks = c; }
    if (eff >= 0.93) break;
  }
  if (chunk_cap > 0 && chunks > chunk_cap) chunks = chunk_cap;
  return split_k_lengths(P, chunks, k_step);
}

// The rule of the generic bf16x6 weight gradient (launch_wgrad_split): double the chunks while the launch has fewer than 1024 workgroups
static inline SplitK plan_split_k_doubling(i64 work, int P) {
  int chunks = 1;
  while (work * chunks < 1024 && P / (chunks * 2) >= 512) chunks *= 2;
  return split_k_lengths(P, chunks, 16);
}

// One split-K launch of groups * slices_per_group grid slices (slice = (group * N + image) * chunks + chunk) that add into dw[group * dw_gs].
// launch(dst, group_stride, slice_stride) enqueues the kernel: it accumulates at `dst`, and gets whichever stride argument its family
// takes -- the flat-grid kernels group_stride (dw_gs; in deterministic mode -elems: one scratch tile-set per slice), the 3-D-grid kernels
// slice_stride (0; in deterministic mode elems).  In deterministic mode the slices are then added into dw in index order.
template <class Launch>
static inline int wgrad_launch(float* dw, i64 elems, int groups, int slices_per_group, i64 dw_gs, hipStream_t s, Launch&& launch) {
  bool det_ok;
  float* const ws = wgrad_det_scratch(elems, (i64)groups * slices_per_group, s, det_ok);
  PFST_CHECK_DET(det_ok);
  launch(ws ? ws : dw, ws ? -elems : dw_gs, ws ? elems : (i64)0);
  if (ws) wgrad_det_reduce(ws, dw, elems, groups, slices_per_group, dw_gs, s);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
