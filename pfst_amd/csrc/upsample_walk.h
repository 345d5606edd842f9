// The pixel walks of the fused up-sampling losses (loss.hip: cross-entropy, dice_loss.hip, sigmoid_loss.hip), ONE text each -- but for
// ce_fwd_blocks_kernel and ce_bwd_blocks_kernel, which keep a twin of the two block frames for what the compiler makes of them (loss.hip).
// Every loss
// kernel walks the full-resolution pixels and interpolates their C logits from the low-resolution map in registers; the families differ
// only in what they read per pixel and in the per-pixel term, which a small functor supplies.  A kernel sets up its image's pointers,
// builds its functor and calls a frame.  The interpolation, the class order, the arg-max and the order of a cell's terms are therefore the
// same bits in every family: acc_seg does not depend on which losses a head lists, and Dice reads CE's log-sum-exp.
//
//   fwd_blocks_walk<S, TILES>   forward, x4 / x8 inter-cell blocks (C <= 8)
//   bwd_blocks_walk<S>          backward, inter-cell blocks whose corner sums meet in LDS (C <= 8)
//   bwd_cells_gather            backward, one thread per low-resolution cell, all classes (C <= 8)    } one text,
//   bwd_class_gather            backward, one thread per (cell, class)                               } bwd_gather<8 / 1>
//
// The frames round every + - * on its own whatever the including file's contraction mode (a template's mode is fixed where it is parsed):
// `#pragma clang fp contract(off)` opens each body, and every fused multiply-add is written as one.  A functor keeps its own file's mode.
#pragma once
#include "bilin.h"

// the logits of the four cells that every pixel of one inter-cell block interpolates from (what bilin_src returns for each of them)
struct Corners {
  float v[2][2][8];
  __device__ __forceinline__ void load(const float* __restrict__ lp, int C, int hw, int w, int xl, int xr, int yt, int yb) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float* q = lp + (i64)(c < C ? c : 0) * hw;
      v[0][0][c] = q[yt * w + xl];
      v[0][1][c] = q[yt * w + xr];
      v[1][0][c] = q[yb * w + xl];
      v[1][1][c] = q[yb * w + xr];
    }
  }
  __device__ __forceinline__ float blend(int c, float lx0, float lx1, float ly0, float ly1) const {
    return bilin_blend(v[0][0][c], v[0][1][c], v[1][0][c], v[1][1][c], lx0, lx1, ly0, ly1);
  }
};
// a pixel's interpolated logit of class c, handed to the backward functors: evaluated when (and if) the functor asks
struct BlockZ {
  const Corners& q;
  float lx0, lx1, ly0, ly1;
  __device__ __forceinline__ float operator()(int c) const { return q.blend(c, lx0, lx1, ly0, ly1); }
};
struct CellZ {
  const float* __restrict__ lp;
  int hw, w;
  const Bilin& b;
  __device__ __forceinline__ float operator()(int c) const { return interp(lp + (i64)c * hw, w, b); }
};

// Forward, the x4 / x8 cases (H == S h, W == S w, S = 4: the decode head's logits at 1/4 resolution, 8: the auxiliary head's at 1/8; C <= 8)
// by inter-cell blocks, as bwd_blocks_walk below: one thread per S x S block of full-resolution pixels that interpolate from the same four
// cells -- their 4 x C logits are loaded once instead of once per pixel.  Per pixel the arithmetic is the generic kernels' (same coordinates
// and weights from bilin_src, same class order): bit-identical logits, the same arg-max.  TILES tiles of 16 x 16 blocks per workgroup.
//   px.pair(p)                        before a pixel pair: load what the family reads per pair (p: the pair's first pixel, even)
//   px.pixel(k, l, zc, mx, arg)       pixel k of the pair: label, logits (-inf beyond C), their maximum and its first index
//   px.pair_end(p)                    after the pair: store what the family writes per pair
// The workgroup's reduction of what px gathered stays with the kernel.
// grid: (ceil((w + 1) / 16), ceil((h + 1) / (16 TILES)), N), 16 x 16 threads
template <int S, int TILES, class Px>
__device__ __forceinline__ void fwd_blocks_walk(const float* __restrict__ lp, int C, int h, int w, const unsigned char* __restrict__ lab, Px& px) {
#pragma clang fp contract(off)
  const int H = S * h, W = S * w, hw = h * w;
  const int bx = blockIdx.x * 16 + (threadIdx.x & 15) - 1;
  for (int it = 0; it < TILES; ++it) {
    const int by = (blockIdx.y * TILES + it) * 16 + (threadIdx.x >> 4) - 1;
    if (bx > w - 1 || by > h - 1) continue;
    const int xl = max(bx, 0), xr = min(xl + 1, w - 1), yt = max(by, 0), yb = min(yt + 1, h - 1);
    Corners q;
    q.load(lp, C, hw, w, xl, xr, yt, yb);
    float lx0[S], lx1[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const int ox = S * bx + S / 2 + j;
      int x0, x1;
      lx0[j] = lx1[j] = 0.f;
      if (ox >= 0 && ox < W) bilin_src(ox, 1.f / S, w, x0, x1, lx0[j], lx1[j]);
    }
#pragma unroll
    for (int r = 0; r < S; ++r) {
      const int oy = S * by + S / 2 + r;
      if (oy < 0 || oy >= H) continue;
      int y0, y1;
      float ly0, ly1;
      bilin_src(oy, 1.f / S, h, y0, y1, ly0, ly1);
#pragma unroll
      for (int half = 0; half < S / 2; ++half) {
        const int ox = S * bx + S / 2 + 2 * half;                  // pixel pairs are inside the image together (W = S w, ox even)
        if (ox < 0 || ox >= W) continue;
        const i64 p = (i64)oy * W + ox;
        const unsigned short l2 = *reinterpret_cast<const unsigned short*>(lab + p);
        px.pair(p);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int j = 2 * half + k;
          const int l = k ? (l2 >> 8) : (l2 & 255);
          float mx = -INFINITY;
          int arg = 0;
          float zc[8];
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            zc[c] = c < C ? q.blend(c, lx0[j], lx1[j], ly0, ly1) : -INFINITY;
            if (c < C && zc[c] > mx) { mx = zc[c]; arg = c; }
          }
          px.pixel(k, l, zc, mx, arg);
        }
        px.pair_end(p);
      }
    }
  }
}

// Backward, the x4 / x8 cases (H == S h, W == S w; C <= 8) by INTER-CELL BLOCKS instead of cells.  The S x S full-resolution pixels between
// four neighbouring cell centres -- pixels S b + S/2 ... S b + 3S/2 - 1 of block b in each direction (4b+2 ... 4b+5 at S = 4),
// b = -1 ... w-1 (the outermost blocks are the half-width borders whose taps are clamped) -- all interpolate from the same four cells:
// one thread loads those 4 x C logits ONCE, evaluates each pixel's terms once (the per-cell gather below evaluates every pixel in each
// of the up to four cells it touches: 4x the exponentials, 16x the logit loads), and keeps the 4 x C corner sums in registers.  A
// workgroup is 16 x 16 blocks; the corner sums meet in LDS in four conflict-free phases (in a phase every thread adds to a different
// cell), and the 15 x 15 cells whose four blocks all lie inside the workgroup are written out -- neighbouring workgroups overlap by one
// block row / column.  Per pixel and tap the term is the one of bwd_cells_gather (same source coordinates, weights, interpolation and
// fma); the ORDER of a cell's <= 64 terms differs (block by block instead of raster order), deterministically.
//   px.pair(p)                        before a pixel pair: load what the family reads per pair (p: the pair's first pixel, even)
//   px.skip(k, l) -> bool             pixel k of the pair, with label l, adds nothing
//   px.weight(k, l, z) -> float       otherwise: the multiplier of its tap weights (and whatever of the pixel its terms share: z(c) is
//                                     its logit of class c, evaluated when asked for)
//   px.term(c, z) -> float            that pixel's term of class c < C, asked for in class order
// (skip apart from weight: a hook is optimised on its own before it is inlined, and one that returned both would hand the weight out
// through selects on the skip condition)
// grid: (ceil(w / 15), ceil(h / 15), N), 16 x 16 threads
template <int S, class Px>
__device__ __forceinline__ void bwd_blocks_walk(const float* __restrict__ lp, int C, int h, int w, const unsigned char* __restrict__ lab,
                                                float scale, float* __restrict__ dp, int accumulate, Px& px) {
#pragma clang fp contract(off)
  constexpr int TB = 16, OWN = TB - 1;
  __shared__ float cell[8][TB + 1][TB + 1];
  const int H = S * h, W = S * w, hw = h * w;
  const int tx = threadIdx.x & (TB - 1), ty = threadIdx.x >> 4;
  const int cx0 = blockIdx.x * OWN, cy0 = blockIdx.y * OWN;        // first cell this workgroup owns
  const int bx = cx0 - 1 + tx, by = cy0 - 1 + ty;                  // this thread's block: taps (b, b + 1), clamped at the borders
  for (int i = threadIdx.x; i < 8 * (TB + 1) * (TB + 1); i += 256) (&cell[0][0][0])[i] = 0.f;
  float acc[2][2][8];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[a][b][c] = 0.f;
  if (bx <= w - 1 && by <= h - 1) {
    const int xl = max(bx, 0), xr = min(xl + 1, w - 1), yt = max(by, 0), yb = min(yt + 1, h - 1);
    Corners q;
    q.load(lp, C, hw, w, xl, xr, yt, yb);
    // column taps of the block's pixel columns: weight towards cell bx (L) and cell bx + 1 (R)
    float lx0[S], lx1[S], wxl[S], wxr[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const int ox = S * bx + S / 2 + j;
      int x0 = 0, x1 = 0;
      lx0[j] = lx1[j] = 0.f;
      if (ox >= 0 && ox < W) bilin_src(ox, 1.f / S, w, x0, x1, lx0[j], lx1[j]);
      wxl[j] = (x0 == bx ? lx0[j] : 0.f) + (x1 == bx ? lx1[j] : 0.f);
      wxr[j] = (x0 == bx + 1 ? lx0[j] : 0.f) + (x1 == bx + 1 ? lx1[j] : 0.f);
    }
#pragma unroll
    for (int r = 0; r < S; ++r) {
      const int oy = S * by + S / 2 + r;
      if (oy < 0 || oy >= H) continue;
      int y0, y1;
      float ly0, ly1;
      bilin_src(oy, 1.f / S, h, y0, y1, ly0, ly1);
      const float wyt = (y0 == by ? ly0 : 0.f) + (y1 == by ? ly1 : 0.f);
      const float wyb = (y0 == by + 1 ? ly0 : 0.f) + (y1 == by + 1 ? ly1 : 0.f);
#pragma unroll
      for (int half = 0; half < S / 2; ++half) {
        const int ox = S * bx + S / 2 + 2 * half;                  // pixel pairs are inside the image together (W = S w, ox even)
        if (ox < 0 || ox >= W) continue;
        const i64 p = (i64)oy * W + ox;
        const unsigned short l2 = *reinterpret_cast<const unsigned short*>(lab + p);
        px.pair(p);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int j = 2 * half + k;
          const int l = k ? (l2 >> 8) : (l2 & 255);
          if (px.skip(k, l)) continue;
          const BlockZ z{q, lx0[j], lx1[j], ly0, ly1};
          const float g = px.weight(k, l, z);
          const float wtl = wyt * wxl[j] * g, wtr = wyt * wxr[j] * g, wbl = wyb * wxl[j] * g, wbr = wyb * wxr[j] * g;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            if (c < C) {
              const float d = px.term(c, z);
              acc[0][0][c] = fmaf(wtl, d, acc[0][0][c]);
              acc[0][1][c] = fmaf(wtr, d, acc[0][1][c]);
              acc[1][0][c] = fmaf(wbl, d, acc[1][0][c]);
              acc[1][1][c] = fmaf(wbr, d, acc[1][1][c]);
            }
          }
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < C) cell[c][ty + a][tx + b] += acc[a][b][c];
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < OWN * OWN; i += 256) {
    const int u = i / OWN, v = i - u * OWN;
    const int gy = cy0 + u, gx = cx0 + v;
    if (gy >= h || gx >= w) continue;
    for (int c = 0; c < C; ++c) {
      const float a = cell[c][u + 1][v + 1] * scale;
      float* o = dp + (i64)c * hw + gy * w + gx;
      *o = accumulate ? *o + a : a;
    }
  }
}

// Backward at any ratio: one thread per low-resolution cell gathers the full-resolution pixels whose taps reach it (bilin_footprint's
// window, a tap's weight towards the cell from bilin_src), deterministic and without atomics.
//   bwd_cells_gather    ALL classes in one thread (C <= 8): the per-pixel work that does not depend on the class -- source coordinates and
//                       weights, label, what px reads -- is done once instead of C times, the C accumulators live in registers.
//                       grid: (blocks over h*w, 1, N)
//   bwd_class_gather    one thread per low-resolution logit of ONE class (any C: a launch row per class); lp and dp are that class's
//                       planes, px's class 0 is that class.  grid: (blocks over h*w, C, N)
// Per class the terms and their order are the same in both: bit-identical gradients.
//   px.cell_skip(p, l) -> bool        pixel p, with label l, adds nothing
//   px.cell_weight(p, l, z) -> float  as px.weight of bwd_blocks_walk for the single pixel p, which loads what it reads itself
//   px.term(c, z) -> float            that pixel's term of class c, asked for in class order
template <int NC, class Px>
__device__ __forceinline__ void bwd_gather(const float* __restrict__ lp, int C, int h, int w, const unsigned char* __restrict__ lab, int H, int W,
                                           float sh, float sw, float scale, float* __restrict__ dp, int accumulate, Px& px) {
#pragma clang fp contract(off)
  const int hw = h * w;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
    const int iy = i / w, ix = i - iy * w;
    int oy_lo, oy_hi, ox_lo, ox_hi;
    bilin_footprint(iy, ix, sh, sw, H, W, oy_lo, oy_hi, ox_lo, ox_hi);
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      int y0, y1; float ly0, ly1;
      bilin_src(oy, sh, h, y0, y1, ly0, ly1);
      const float wy = (y0 == iy ? ly0 : 0.f) + (y1 == iy ? ly1 : 0.f);
      if (wy == 0.f) continue;
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        Bilin b;
        b.y0 = y0; b.y1 = y1; b.ly0 = ly0; b.ly1 = ly1;
        bilin_src(ox, sw, w, b.x0, b.x1, b.lx0, b.lx1);
        const float wx = (b.x0 == ix ? b.lx0 : 0.f) + (b.x1 == ix ? b.lx1 : 0.f);
        if (wx == 0.f) continue;
        const int p = oy * W + ox;
        const int l = lab[p];
        if (px.cell_skip(p, l)) continue;
        const CellZ z{lp, hw, w, b};
        const float wg = wy * wx * px.cell_weight(p, l, z);
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c < C) acc[c] = fmaf(wg, px.term(c, z), acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < C) {
        const float a = acc[c] * scale;
        dp[(i64)c * hw + i] = accumulate ? dp[(i64)c * hw + i] + a : a;
      }
    }
  }
}
template <class Px>
__device__ __forceinline__ void bwd_cells_gather(const float* __restrict__ lp, int C, int h, int w, const unsigned char* __restrict__ lab, int H,
                                                 int W, float sh, float sw, float scale, float* __restrict__ dp, int accumulate, Px& px) {
  bwd_gather<8>(lp, C, h, w, lab, H, W, sh, sw, scale, dp, accumulate, px);
}
template <class Px>
__device__ __forceinline__ void bwd_class_gather(const float* __restrict__ lp, int h, int w, const unsigned char* __restrict__ lab, int H, int W,
                                                 float sh, float sw, float scale, float* __restrict__ dp, int accumulate, Px& px) {
  bwd_gather<1>(lp, 1, h, w, lab, H, W, sh, sw, scale, dp, accumulate, px);
}
