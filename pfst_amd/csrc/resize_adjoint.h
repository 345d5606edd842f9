// The adjoint of the bilinear resize (align_corners=False) as a gather over the SOURCE pixels of one plane, shared by fpn.hip (concat_bwd) and
// hrnet.hip (the exchange unit's backward): the two gather forms of pfst_resize_bilinear_bwd (spatial.hip: resize_bilinear_bwd_kernel for any
// ratio, resize_bilinear2x_bwd_q_kernel for x2 on even grids), term for term -- a rounded product, then one fused multiply-add per further
// tap in ascending column order, rows likewise; a zero-weight tap adds nothing.  Every value is bit-identical to pfst_resize_bilinear_bwd's.
#pragma once
#include "common.h"

namespace pfst_adj {
// grid.x of a grid-stride launch over `items` work items of one plane (256 threads, up to four passes each)
inline int px_grid(i64 items) {
  i64 g = (items + 1023) / 1024;
  return g < 1 ? 1 : (g > 65535 ? 65535 : (int)g);
}
inline bool al(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }
// the x2 form of the adjoint applies: an exact x2 on even grids with aligned planes -- pfst_resize_bilinear_bwd's own rule for its 2 x 2 block kernel
inline bool adjoint2x_q_ok(const float* dy_plane, long long dy_bs, const float* d_src, long long src_bs, int Hc, int Wc, int Hf, int Wf) {
  return Hf == 2 * Hc && Wf == 2 * Wc && Hc > 1 && Wc > 1 && (Hc & 1) == 0 && (Wc & 1) == 0 && (dy_bs & 3) == 0 && (src_bs & 1) == 0 &&
         al(dy_plane, 15) && al(d_src, 7);
}
// do two strided NCHW operands ([N] images of `plane` floats, batch stride bs) share memory?
inline bool overlap(const float* a, long long a_bs, const float* b, long long b_bs, int N, long long a_plane, long long b_plane) {
  const float* ae = a + (long long)(N - 1) * a_bs + a_plane;
  const float* be = b + (long long)(N - 1) * b_bs + b_plane;
  return a < be && b < ae;
}
}  // namespace pfst_adj

__device__ __forceinline__ float bilin_row4(const float (&wx)[4], float v0, float v1, float v2, float v3) {
  return __fmaf_rn(wx[3], v3, __fmaf_rn(wx[2], v2, __fmaf_rn(wx[1], v1, __fmul_rn(wx[0], v0))));
}
__device__ __forceinline__ void adjoint_generic(const float* __restrict__ gp, float* __restrict__ dp, int Hi, int Wi, int Ho, int Wo, float sh,
                                                float sw, int accumulate) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Hi * Wi; i += gridDim.x * blockDim.x) {
    const int iy = i / Wi, ix = i - iy * Wi;
    int oy_lo, oy_hi, ox_lo, ox_hi;
    bilin_footprint(iy, ix, sh, sw, Ho, Wo, oy_lo, oy_hi, ox_lo, ox_hi);
    float acc = 0.f;
    for (int oy = oy_lo; oy <= oy_hi; ++oy) {
      int y0, y1; float ly0, ly1;
      bilin_src(oy, sh, Hi, y0, y1, ly0, ly1);
      const float wy = (y0 == iy ? ly0 : 0.f) + (y1 == iy ? ly1 : 0.f);
      if (wy == 0.f) continue;
      float row = 0.f;
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        int x0, x1; float lx0, lx1;
        bilin_src(ox, sw, Wi, x0, x1, lx0, lx1);
        const float wx = (x0 == ix ? lx0 : 0.f) + (x1 == ix ? lx1 : 0.f);
        if (wx != 0.f) row = fmaf(wx, gp[(i64)oy * Wo + ox], row);
      }
      acc = fmaf(wy, row, acc);
    }
    dp[i] = accumulate ? dp[i] + acc : acc;
  }
}
// x2, a 2 x 2 block of source pixels per thread (Hi, Wi even, 16-byte aligned dy rows, 8-byte aligned dx rows)
__device__ __forceinline__ void adjoint2x_q(const float* __restrict__ gp, float* __restrict__ dp, int Hi, int Wi, int accumulate) {
  const int Wo = 2 * Wi, Ho = 2 * Hi, W2 = Wi >> 1, H2 = Hi >> 1;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < H2 * W2; b += gridDim.x * blockDim.x) {
    const int by = b / W2, bx = b - by * W2;
    const int iy0 = 2 * by, ix0 = 2 * bx;
    float v[6][6];                 // columns 2 ix0 - 1 .. 2 ix0 + 4 of dy rows 2 iy0 - 1 .. 2 iy0 + 4 (clamped: those taps carry weight 0)
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const int oy = min(max(2 * iy0 - 1 + r, 0), Ho - 1);
      const float* row = gp + (i64)oy * Wo + 2 * ix0;
      const float4 mid = *reinterpret_cast<const float4*>(row);
      v[r][0] = row[ix0 > 0 ? -1 : 0];
      v[r][1] = mid.x; v[r][2] = mid.y; v[r][3] = mid.z; v[r][4] = mid.w;
      v[r][5] = row[ix0 + 1 < Wi - 1 ? 4 : 3];
    }
    float o[2][2];
#pragma unroll
    for (int dyi = 0; dyi < 2; ++dyi) {
      const int iy = iy0 + dyi;
      float wy[4];
      wy[0] = iy > 0 ? 0.25f : 0.f;  wy[1] = iy > 0 ? 0.75f : 1.f;  wy[2] = iy < Hi - 1 ? 0.75f : 1.f;  wy[3] = iy < Hi - 1 ? 0.25f : 0.f;
#pragma unroll
      for (int dxi = 0; dxi < 2; ++dxi) {
        const int ix = ix0 + dxi;
        float wx[4];
        wx[0] = ix > 0 ? 0.25f : 0.f;  wx[1] = ix > 0 ? 0.75f : 1.f;  wx[2] = ix < Wi - 1 ? 0.75f : 1.f;  wx[3] = ix < Wi - 1 ? 0.25f : 0.f;
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float* q = &v[2 * dyi + t][2 * dxi];
          acc = __fmaf_rn(wy[t], bilin_row4(wx, q[0], q[1], q[2], q[3]), acc);
        }
        o[dyi][dxi] = acc;
      }
    }
#pragma unroll
    for (int dyi = 0; dyi < 2; ++dyi) {
      float2* d2 = reinterpret_cast<float2*>(dp + (i64)(iy0 + dyi) * Wi + ix0);
      float2 w2 = make_float2(o[dyi][0], o[dyi][1]);
      if (accumulate) { const float2 old = *d2; w2.x = old.x + w2.x; w2.y = old.y + w2.y; }
      *d2 = w2;
    }
  }
}
