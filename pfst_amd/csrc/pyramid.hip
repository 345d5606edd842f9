// Plane <-> pyramid-of-small-grids kernels: the pyramid pooling module of PSPHead (psp_head.py:9-50) both ways.
//
// nn.AdaptiveAvgPool2d(s) and the bilinear resize from s x s (align_corners=False) are separable linear maps between an H x W plane and an
// s x s grid.  With a per-axis operator D_k (s_k x H rows, s_k x W columns; the host builds the tables once per (H, W, scales),
// hip_ops.pyramid_operator) both directions of both operations are
//   reduce:  out_k = Dh_k . X . Dw_k^T          (pool forward: D = the bin averages;  resize backward: D = A^T, the bilinear adjoint)
//   expand:  Y (+)= Dh_k^T . G_k . Dw_k         (pool backward, summed over the scales;  resize forward, scale k into its channel slice)
// Every row of D_k is non-zero on one contiguous span, and so is every column: the tables carry the dense operator (sum_k s_k rows per
// axis) and the two kinds of spans.  No atomics between or inside workgroups, every sum in one fixed order: bit-identical run to run.
#include "amax.h"
#include "common.h"
#include "../../include/pfst_hip.h"

namespace {

constexpr int MAXK = PFST_PYR_MAX_SCALES;                      // scales per launch
constexpr int MAXS = PFST_PYR_MAX_SCALE;                       // largest grid
constexpr int MAXJ = MAXK * MAXS;                              // rows of a per-axis operator table at most (48)
constexpr int MAXO = MAXK * MAXS * MAXS;                       // grid cells of all scales at most (384)

struct PyrArgs {
  int K;
  int s[MAXK];
  int off1[MAXK + 1];          // prefix sums of s_k: scale k owns the operator rows [off1[k], off1[k+1])
  int off2[MAXK + 1];          // prefix sums of s_k^2: its cells in the flat cell order
  int coff[MAXK];              // channel offset of the scale's plane slice (the sliced forms)
  float* grid[MAXK];           // dense [N][C][s_k][s_k]
};

// ---- reduce.  One workgroup per (n, c); the plane is staged through LDS RED_ROWS rows at a time (row stride W | 1: the partial step walks
// a column of the tile, odd strides keep its lanes on different banks), each chunk gives per-row column partials P[J][r] = sum_x X[r][x]
// Dw[J][x] for the sum_k s_k operator rows J, and the thread that owns cell (k, i, j) adds sum_r Dh[k,i][r] P[off1[k] + j][r] to its
// accumulator -- rows in ascending order across the chunks.  shared: every scale reads the same plane (staged once for all of them); else
// scale k reads the plane of channel coff[k] + c and only its own operator rows.
constexpr int RED_ROWS = 64;
constexpr int RED_TILE = 8320;                                 // floats: 64 rows of a 128-wide plane (stride 129) and a little more
constexpr int PSTR = RED_ROWS + 1;

__global__ __launch_bounds__(256) void pyramid_reduce_kernel(const float* __restrict__ x, i64 x_bs, int C, int H, int W, PyrArgs a, int shared,
                                                             const float* __restrict__ op_h, const float* __restrict__ op_w,
                                                             const int* __restrict__ span_h, const int* __restrict__ span_w) {
  __shared__ float tile[RED_TILE];
  __shared__ float part[MAXJ * PSTR];
  const int c = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const int ws = W | 1;
  int rc = RED_TILE / ws;
  rc = rc > RED_ROWS ? RED_ROWS : rc;
  rc = rc > H ? H : rc;
  const int groups = shared ? 1 : a.K;
  for (int g = 0; g < groups; ++g) {
    const int k0 = shared ? 0 : g, k1 = shared ? a.K : g + 1;
    int J0 = 0, J1 = 0, O0 = 0, O1 = 0, ch = 0;
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      if (k == k0) { J0 = a.off1[k]; O0 = a.off2[k]; ch = a.coff[k]; }
      if (k + 1 == k1) { J1 = a.off1[k + 1]; O1 = a.off2[k + 1]; }
    }
    const float* plane = x + (i64)n * x_bs + (i64)(ch + c) * H * W;
    const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(plane) & 15) == 0;
    // the (at most two) cells of this group that the thread owns
    int oI[2], oJ[2], oS[2], oL[2];
    float* oP[2];
    float acc[2] = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int o = O0 + tid + 256 * q;
      oI[q] = -1; oJ[q] = 0; oS[q] = 1; oL[q] = 0; oP[q] = nullptr;
#pragma unroll
      for (int k = 0; k < MAXK; ++k)
        if (k >= k0 && k < k1 && o >= a.off2[k] && o < a.off2[k + 1]) {
          const int l = o - a.off2[k], i = l / a.s[k];
          oI[q] = a.off1[k] + i; oJ[q] = a.off1[k] + (l - i * a.s[k]) - J0; oS[q] = a.s[k]; oL[q] = l; oP[q] = a.grid[k];
        }
    }
    const int nJ = J1 - J0;
    for (int y0 = 0; y0 < H; y0 += rc) {
      const int rows = H - y0 < rc ? H - y0 : rc;
      const float* src = plane + (i64)y0 * W;
      const int cnt = rows * W;
      if (vec) {
        const float4* src4 = reinterpret_cast<const float4*>(src);
        for (int e = tid; e < (cnt >> 2); e += 256) {
          const float4 v = src4[e];
          const int r = (4 * e) / W, xx = 4 * e - r * W;
          float* t = tile + r * ws + xx;
          t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
        }
      } else {
        for (int e = tid; e < cnt; e += 256) {
          const int r = e / W;
          tile[r * ws + (e - r * W)] = src[e];
        }
      }
      __syncthreads();
      for (int t = tid; t < nJ * rows; t += 256) {
        const int jl = t / rows, r = t - jl * rows, J = J0 + jl;
        const int xa = span_w[2 * J], xb = span_w[2 * J + 1];
        const float* wrow = op_w + (i64)J * W;
        const float* trow = tile + r * ws;
        float s = 0.f;
#pragma unroll 8
        for (int xx = xa; xx < xb; ++xx) s = fmaf(trow[xx], wrow[xx], s);          // (unrolled: the loads of eight terms in flight, the sum in order)
        part[jl * PSTR + r] = s;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (oI[q] >= 0) {
          int ya = span_h[2 * oI[q]], yb = span_h[2 * oI[q] + 1];
          ya = ya < y0 ? y0 : ya;
          yb = yb > y0 + rows ? y0 + rows : yb;
          const float* hrow = op_h + (i64)oI[q] * H;
          const float* prow = part + oJ[q] * PSTR - y0;
          float s = acc[q];
#pragma unroll 8
          for (int yy = ya; yy < yb; ++yy) s = fmaf(hrow[yy], prow[yy], s);
          acc[q] = s;
        }
      __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (oI[q] >= 0) oP[q][((i64)n * C + c) * (oS[q] * oS[q]) + oL[q]] = acc[q];
  }
}

// ---- expand.  One workgroup per EXP_ROWS rows of an output plane.  The grids of the plane's scales go to LDS, then U[r][J] = sum_i Dh[k,i][y0 + r]
// G_k[i][j] for the operator rows J = off1[k] + j, then every thread walks columns: the column's span and its first two weights per scale stay in
// registers (a pooling bin pair, the two bilinear taps; a longer span -- a plane narrower than the grid -- reads the rest from the table), a wave
// holds one output row, so the U reads are broadcasts and the stores 256 contiguous bytes.
// sliced = 0: y[n][c] (+)= [add[n][c] +] the sum over all scales;  sliced = 1: scale k alone into the plane of channel coff[k] + c.
constexpr int EXP_ROWS = 64;
constexpr int USTR = MAXJ + 1;

__global__ __launch_bounds__(256) void pyramid_expand_kernel(PyrArgs a, float* __restrict__ y, i64 y_bs, const float* __restrict__ add, i64 add_bs,
                                                             int C, int H, int W, int sliced, int accumulate, const float* __restrict__ op_h,
                                                             const float* __restrict__ op_w, const int* __restrict__ tspan_h,
                                                             const int* __restrict__ tspan_w, float* __restrict__ amax) {
  __shared__ float G[MAXO];
  __shared__ float U[EXP_ROWS * USTR];
  const int tid = threadIdx.x, n = blockIdx.z;
  const int slot = sliced ? blockIdx.y / C : 0, c = sliced ? blockIdx.y - slot * C : blockIdx.y;
  const int k0 = sliced ? slot : 0, k1 = sliced ? slot + 1 : a.K;
  const int y0 = blockIdx.x * EXP_ROWS;
  const int rows = H - y0 < EXP_ROWS ? H - y0 : EXP_ROWS;
  int J0 = 0, J1 = 0, O0 = 0, O1 = 0, ch = 0;
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    if (k == k0) { J0 = a.off1[k]; O0 = a.off2[k]; ch = a.coff[k]; }
    if (k + 1 == k1) { J1 = a.off1[k + 1]; O1 = a.off2[k + 1]; }
  }
  for (int o = tid; o < O1 - O0; o += 256) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
      if (k >= k0 && k < k1 && O0 + o >= a.off2[k] && O0 + o < a.off2[k + 1])
        v = a.grid[k][((i64)n * C + c) * (a.s[k] * a.s[k]) + (O0 + o - a.off2[k])];
    G[o] = v;
  }
  __syncthreads();
  const int nJ = J1 - J0;
  for (int t = tid; t < rows * nJ; t += 256) {
    const int r = t / nJ, jl = t - r * nJ, J = J0 + jl, yy = y0 + r;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < MAXK; ++k)
      if (k >= k0 && k < k1 && J >= a.off1[k] && J < a.off1[k + 1]) {
        const int j = J - a.off1[k], sk = a.s[k];
        const int ilo = tspan_h[2 * (k * H + yy)], ihi = tspan_h[2 * (k * H + yy) + 1];
        const float* g = G + (a.off2[k] - O0) + j;
        const float* d = op_h + (i64)a.off1[k] * H + yy;
        for (int i = ilo; i < ihi; ++i) s = fmaf(d[(i64)i * H], g[i * sk], s);
      }
    U[r * USTR + jl] = s;
  }
  __syncthreads();
  float* plane = y + (i64)n * y_bs + (i64)((sliced ? ch : 0) + c) * H * W;
  const float* addp = add ? add + (i64)n * add_bs + (i64)c * H * W : nullptr;
  const int lane = tid & 63, wv = tid >> 6;
  float m = 0.f;
  for (int xx = lane; xx < W; xx += 64) {
    int jl[MAXK], lo[MAXK], cn[MAXK];
    float wa[MAXK], wb[MAXK];
#pragma unroll
    for (int k = 0; k < MAXK; ++k) {
      cn[k] = 0; jl[k] = 0; lo[k] = 0; wa[k] = 0.f; wb[k] = 0.f;
      if (k >= k0 && k < k1) {
        lo[k] = tspan_w[2 * (k * W + xx)];
        cn[k] = tspan_w[2 * (k * W + xx) + 1] - lo[k];
        jl[k] = a.off1[k] - J0 + lo[k];
        // (every pixel touches at least one cell; a single one: its second term is 0 x the same cell)
        wa[k] = op_w[(i64)(a.off1[k] + lo[k]) * W + xx];
        if (cn[k] > 1) wb[k] = op_w[(i64)(a.off1[k] + lo[k] + 1) * W + xx];
      }
    }
#pragma unroll 4
    for (int r = wv; r < rows; r += 4) {
      float v = 0.f;
#pragma unroll
      for (int k = 0; k < MAXK; ++k)
        if (k >= k0 && k < k1) {
          const float* u = U + r * USTR + jl[k];
          v = fmaf(u[0], wa[k], v);
          v = fmaf(u[cn[k] > 1 ? 1 : 0], wb[k], v);
          for (int jj = 2; jj < cn[k]; ++jj) v = fmaf(u[jj], op_w[(i64)(a.off1[k] + lo[k] + jj) * W + xx], v);
        }
      const i64 idx = (i64)(y0 + r) * W + xx;
      if (addp) v += addp[idx];
      if (accumulate) v += plane[idx];
      plane[idx] = v;
      m = fmaxf(m, fabsf(v));
    }
  }
  if (amax) amax_publish(amax, m);
}

// ---- a dense-plane view into (or, in backward, added to) another: the identity slice of a concat; max |y| published when asked
__global__ __launch_bounds__(256) void copy_planes_kernel(const float* __restrict__ x, i64 x_bs, float* __restrict__ y, i64 y_bs, i64 chw, int vec,
                                                          int accumulate, float* __restrict__ amax) {
  const int n = blockIdx.y;
  const float* xp = x + (i64)n * x_bs;
  float* yp = y + (i64)n * y_bs;
  float m = 0.f;
  const i64 step = (i64)gridDim.x * blockDim.x, first = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec) {
    const float4* x4 = reinterpret_cast<const float4*>(xp);
    float4* y4 = reinterpret_cast<float4*>(yp);
    for (i64 i = first; i < (chw >> 2); i += step) {
      float4 v = x4[i];
      if (accumulate) {
        const float4 o = y4[i];
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
      }
      y4[i] = v;
      m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
  } else {
    for (i64 i = first; i < chw; i += step) {
      const float v = accumulate ? yp[i] + xp[i] : xp[i];
      yp[i] = v;
      m = fmaxf(m, fabsf(v));
    }
  }
  if (amax) amax_publish(amax, m);
}

bool fill_args(PyrArgs& a, int K, const int* scales, const int* chan_off, float* const* grids) {
  if (K < 1 || K > MAXK || !scales || !grids) return false;
  a.K = K;
  a.off1[0] = a.off2[0] = 0;
  for (int k = 0; k < MAXK; ++k) {
    const bool on = k < K;
    if (on && (scales[k] < 1 || scales[k] > MAXS || !grids[k] || (chan_off && chan_off[k] < 0))) return false;
    a.s[k] = on ? scales[k] : 0;
    a.coff[k] = on && chan_off ? chan_off[k] : 0;
    a.grid[k] = on ? grids[k] : nullptr;
    a.off1[k + 1] = a.off1[k] + a.s[k];
    a.off2[k + 1] = a.off2[k] + a.s[k] * a.s[k];
  }
  return true;
}

}  // namespace

extern "C" int pfst_pyramid_reduce(const float* x, long long x_bs, int N, int C, int H, int W, int K, const int* scales, const int* chan_off,
                                   int shared, const float* op_h, const float* op_w, const int* span_h, const int* span_w, float* const* outs,
                                   pfst_stream_t stream) {
  PyrArgs a;
  PFST_CHECK_ARG(x && op_h && op_w && span_h && span_w && N > 0 && C > 0 && H > 0 && W > 0 && N <= 65535);
  PFST_CHECK_ARG((W | 1) <= RED_TILE && (long long)H * W < (1ll << 31));
  PFST_CHECK_ARG(fill_args(a, K, scales, chan_off, outs));
  if (shared)
    for (int k = 1; k < K; ++k) PFST_CHECK_ARG(a.coff[k] == a.coff[0]);
  hipLaunchKernelGGL(pyramid_reduce_kernel, dim3(C, N), dim3(256), 0, (hipStream_t)stream, x, (i64)x_bs, C, H, W, a, shared ? 1 : 0, op_h, op_w,
                     span_h, span_w);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_pyramid_expand(const float* const* grids, int N, int C, int H, int W, int K, const int* scales, const int* chan_off, int sliced,
                                   float* y, long long y_bs, const float* add, long long add_bs, int accumulate, const float* op_h,
                                   const float* op_w, const int* tspan_h, const int* tspan_w, float* y_amax, pfst_stream_t stream) {
  PyrArgs a;
  PFST_CHECK_ARG(y && op_h && op_w && tspan_h && tspan_w && N > 0 && C > 0 && H > 0 && W > 0 && N <= 65535);
  PFST_CHECK_ARG((long long)H * W < (1ll << 31) && (!y_amax || !accumulate) && (!sliced || !add));
  PFST_CHECK_ARG(fill_args(a, K, scales, chan_off, const_cast<float* const*>(reinterpret_cast<const float* const*>(grids))));
  PFST_CHECK_ARG((long long)C * (sliced ? K : 1) <= 65535);
  hipLaunchKernelGGL(pyramid_expand_kernel, dim3(cdiv(H, EXP_ROWS), C * (sliced ? K : 1), N), dim3(256), 0, (hipStream_t)stream, a, y, (i64)y_bs,
                     add, (i64)add_bs, C, H, W, sliced ? 1 : 0, accumulate ? 1 : 0, op_h, op_w, tspan_h, tspan_w, y_amax);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_copy_planes(const float* x, long long x_bs, float* y, long long y_bs, int N, long long CHW, int accumulate, float* y_amax,
                                pfst_stream_t stream) {
  PFST_CHECK_ARG(x && y && N > 0 && N <= 65535 && CHW > 0 && (!y_amax || !accumulate));
  const int vec = (CHW & 3) == 0 && (x_bs & 3) == 0 && (y_bs & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  hipLaunchKernelGGL(copy_planes_kernel, dim3(ew_grid(vec ? CHW / 4 : CHW), N), dim3(256), 0, (hipStream_t)stream, x, (i64)x_bs, y, (i64)y_bs,
                     (i64)CHW, vec, accumulate ? 1 : 0, y_amax);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
