// The top-down path of a feature pyramid (UPerHead, uper_head.py:108-132) as fused streaming kernels:
//   merge:       out[n][c] = lat[n][c] + bilinear(coarse[n][c] -> Hf x Wf), with max |out| published        (2.25 instead of 4.25 map sizes)
//   concat:      K <= 3 coarser maps resized into K channel slices of one buffer in one launch, max |.| published over all of them
//   concat_bwd:  the adjoint of that, every level in one launch, as a gather over the source pixels
// All of them: align_corners=False, dense planes with batch strides (operands may be channel slices of wider buffers), no atomics and one
// fixed summation order -- deterministic mode needs no second path.  The interpolation is bilin.h's (bilin_src / bilin_blend, pinned
// roundings): a value is bit-identical to what pfst_resize_bilinear stores, the merge adds the lateral with ONE rounded fp32 add, the
// adjoint sums in the order of pfst_resize_bilinear_bwd's kernels (spatial.hip, whose three forms agree bit for bit).  The fine map moves in
// 16-byte accesses where its rows allow it; the coarse source is gathered and re-read from L2.
#include "amax.h"
#include "bilin.h"
#include "common.h"
#include "../../include/pfst_hip.h"

namespace {

constexpr int MAXL = PFST_FPN_MAX_LEVELS;

struct FpnArgs {
  int h[MAXL], w[MAXL];          // the level's own grid
  int coff[MAXL];                // first channel of its slice of the wide buffer
  int route[MAXL];               // concat_bwd: 0 generic gather, 1 the x2 form on 2 x 2 blocks
  int acc[MAXL];                 // concat_bwd: add to the level's gradient instead of writing it
  float sh[MAXL], sw[MAXL];      // h / Hf, w / Wf as pfst_resize_bilinear forms them (on the host)
  i64 bs[MAXL];
  float* p[MAXL];
};

inline int px_grid(i64 items) {
  i64 g = (items + 1023) / 1024;
  return g < 1 ? 1 : (g > 65535 ? 65535 : (int)g);
}

// four consecutive pixels of output row oy from column ox0: one pair of source rows, four column tap pairs
__device__ __forceinline__ float4 resize_quad(const float* __restrict__ cp, int Hc, int Wc, int oy, int ox0, float sh, float sw) {
  int y0, y1;
  float ly0, ly1;
  bilin_src(oy, sh, Hc, y0, y1, ly0, ly1);
  const float* r0 = cp + (i64)y0 * Wc;
  const float* r1 = cp + (i64)y1 * Wc;
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int x0, x1;
    float lx0, lx1;
    bilin_src(ox0 + k, sw, Wc, x0, x1, lx0, lx1);
    v[k] = bilin_blend(r0[x0], r0[x1], r1[x0], r1[x1], lx0, lx1, ly0, ly1);
  }
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ float amax4(float m, const float4& v) {
  return fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}

// ---- merge, any ratio.  grid: (blocks over the fine plane, C, N).  VEC: Wf % 4 == 0 and 16-byte aligned lat / out planes, four pixels per thread
template <bool VEC>
__global__ __launch_bounds__(256) void topdown_merge_kernel(const float* __restrict__ lat, i64 lat_bs, const float* __restrict__ coarse, i64 c_bs,
                                                            float* __restrict__ out, i64 out_bs, int Hc, int Wc, int Hf, int Wf, float sh,
                                                            float sw, float* __restrict__ amax) {
  const int c = blockIdx.y, n = blockIdx.z;
  const float* cp = coarse + (i64)n * c_bs + (i64)c * Hc * Wc;
  const float* lp = lat + (i64)n * lat_bs + (i64)c * Hf * Wf;
  float* op = out + (i64)n * out_bs + (i64)c * Hf * Wf;
  float m = 0.f;
  if (VEC) {
    const int W4 = Wf >> 2;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < Hf * W4; q += gridDim.x * blockDim.x) {
      const int oy = q / W4, ox0 = 4 * (q - oy * W4);
      float4 v = resize_quad(cp, Hc, Wc, oy, ox0, sh, sw);
      const float4 l = reinterpret_cast<const float4*>(lp)[q];
      v.x = __fadd_rn(l.x, v.x); v.y = __fadd_rn(l.y, v.y); v.z = __fadd_rn(l.z, v.z); v.w = __fadd_rn(l.w, v.w);
      reinterpret_cast<float4*>(op)[q] = v;
      m = amax4(m, v);
    }
  } else {
    for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < Hf * Wf; o += gridDim.x * blockDim.x) {
      const int oy = o / Wf, ox = o - oy * Wf;
      const Bilin b = make_bilin(oy, ox, sh, sw, Hc, Wc);
      const float v = __fadd_rn(lp[o], interp(cp, Wc, b));
      op[o] = v;
      m = fmaxf(m, fabsf(v));
    }
  }
  if (amax) amax_publish(amax, m);
}

// ---- merge at the exact scale 1/2: the walk of spatial.hip's resize_bilinear2x_kernel (outputs 4j .. 4j+3 of a row blend the source column
// pairs (2j-1, 2j), (2j, 2j+1), (2j, 2j+1), (2j+1, 2j+2) with the weights bilin_src returns there; output rows 2p-1 and 2p blend source rows
// p-1, p), the same expressions, plus the lateral's 16-byte load and the add.  grid: ((Hc + 1) / 4 rounded up, C, N); Wc even
__global__ __launch_bounds__(256) void topdown_merge2x_kernel(const float* __restrict__ lat, i64 lat_bs, const float* __restrict__ coarse, i64 c_bs,
                                                              float* __restrict__ out, i64 out_bs, int Hc, int Wc, float* __restrict__ amax) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int Hf = 2 * Hc, Wf = 2 * Wc, W4 = Wf >> 2;
  const float* cp = coarse + (i64)n * c_bs + (i64)c * Hc * Wc;
  const float* lp = lat + (i64)n * lat_bs + (i64)c * Hf * Wf;
  float* op = out + (i64)n * out_bs + (i64)c * Hf * Wf;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);            // output rows 2p-1 (p >= 1) and 2p (p <= Hc-1) from source rows p-1, p
  float m = 0.f;
  if (p <= Hc) {
    const int ra = max(p - 1, 0), rb = min(p, Hc - 1);
    const float* r0 = cp + (i64)ra * Wc;
    const float* r1 = cp + (i64)rb * Wc;
    const bool hasA = p >= 1, hasB = p <= Hc - 1;
    int y0, y1;
    float la0 = 0.f, la1 = 0.f, lb0 = 0.f, lb1 = 0.f;
    if (hasA) bilin_src(2 * p - 1, 0.5f, Hc, y0, y1, la0, la1);
    if (hasB) bilin_src(2 * p, 0.5f, Hc, y0, y1, lb0, lb1);
    const i64 offA = (i64)(2 * p - 1) * Wf, offB = (i64)(2 * p) * Wf;
    for (int j = threadIdx.x & 63; j < W4; j += 64) {
      const int cl = max(2 * j - 1, 0), cr = min(2 * j + 2, Wc - 1);
      const float2 m0 = *reinterpret_cast<const float2*>(r0 + 2 * j), m1 = *reinterpret_cast<const float2*>(r1 + 2 * j);
      const float l0 = r0[cl], l1 = r1[cl], g0 = r0[cr], g1 = r1[cr];
      auto row = [&](float ly0, float ly1, i64 off) {
        const float4 l = reinterpret_cast<const float4*>(lp + off)[j];
        float4 o;
        o.x = j > 0 ? bilin_blend(l0, m0.x, l1, m1.x, 0.25f, 0.75f, ly0, ly1) : bilin_blend(m0.x, m0.y, m1.x, m1.y, 1.f, 0.f, ly0, ly1);
        o.y = bilin_blend(m0.x, m0.y, m1.x, m1.y, 0.75f, 0.25f, ly0, ly1);
        o.z = bilin_blend(m0.x, m0.y, m1.x, m1.y, 0.25f, 0.75f, ly0, ly1);
        o.w = bilin_blend(m0.y, g0, m1.y, g1, 0.75f, 0.25f, ly0, ly1);
        o.x = __fadd_rn(l.x, o.x); o.y = __fadd_rn(l.y, o.y); o.z = __fadd_rn(l.z, o.z); o.w = __fadd_rn(l.w, o.w);
        reinterpret_cast<float4*>(op + off)[j] = o;
        m = amax4(m, o);
      };
      if (hasA) row(la0, la1, offA);
      if (hasB) row(lb0, lb1, offB);
    }
  }
  if (amax) amax_publish(amax, m);
}

// ---- concat.  grid: (blocks over the fine plane, K C, N): plane blockIdx.y = k C + c is level k's channel c, into channel coff[k] + c of y
template <bool VEC>
__global__ __launch_bounds__(256) void fpn_resize_concat_kernel(FpnArgs a, float* __restrict__ y, i64 y_bs, int C, int Hf, int Wf,
                                                                float* __restrict__ amax) {
  const int lvl = blockIdx.y / C, c = blockIdx.y - lvl * C, n = blockIdx.z;
  int Hc = 1, Wc = 1, coff = 0;
  float sh = 1.f, sw = 1.f;
  i64 bs = 0;
  const float* src = nullptr;
#pragma unroll
  for (int k = 0; k < MAXL; ++k)
    if (k == lvl) { Hc = a.h[k]; Wc = a.w[k]; coff = a.coff[k]; sh = a.sh[k]; sw = a.sw[k]; bs = a.bs[k]; src = a.p[k]; }
  const float* cp = src + (i64)n * bs + (i64)c * Hc * Wc;
  float* op = y + (i64)n * y_bs + (i64)(coff + c) * Hf * Wf;
  float m = 0.f;
  if (VEC) {
    const int W4 = Wf >> 2;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < Hf * W4; q += gridDim.x * blockDim.x) {
      const int oy = q / W4, ox0 = 4 * (q - oy * W4);
      const float4 v = resize_quad(cp, Hc, Wc, oy, ox0, sh, sw);
      reinterpret_cast<float4*>(op)[q] = v;
      m = amax4(m, v);
    }
  } else {
    for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < Hf * Wf; o += gridDim.x * blockDim.x) {
      const int oy = o / Wf, ox = o - oy * Wf;
      const Bilin b = make_bilin(oy, ox, sh, sw, Hc, Wc);
      const float v = interp(cp, Wc, b);
      op[o] = v;
      m = fmaxf(m, fabsf(v));
    }
  }
  if (amax) amax_publish(amax, m);
}

// ---- concat_bwd: the two gather forms of pfst_resize_bilinear_bwd (spatial.hip: resize_bilinear_bwd_kernel for any ratio,
// resize_bilinear2x_bwd_q_kernel for x2 on even grids), term for term -- a rounded product, then one fused multiply-add per further tap in
// ascending column order, rows likewise; a zero-weight tap adds nothing
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
// grid: (blocks over the largest level's work, K C, N); a workgroup beyond its level's work finds its loop empty
__global__ __launch_bounds__(256) void fpn_resize_concat_bwd_kernel(const float* __restrict__ dy, i64 dy_bs, FpnArgs a, int C, int Hf, int Wf) {
  const int lvl = blockIdx.y / C, c = blockIdx.y - lvl * C, n = blockIdx.z;
  int Hc = 1, Wc = 1, coff = 0, route = 0, acc = 0;
  float sh = 1.f, sw = 1.f;
  i64 bs = 0;
  float* dst = nullptr;
#pragma unroll
  for (int k = 0; k < MAXL; ++k)
    if (k == lvl) {
      Hc = a.h[k]; Wc = a.w[k]; coff = a.coff[k]; route = a.route[k]; acc = a.acc[k]; sh = a.sh[k]; sw = a.sw[k]; bs = a.bs[k]; dst = a.p[k];
    }
  const float* gp = dy + (i64)n * dy_bs + (i64)(coff + c) * Hf * Wf;
  float* dp = dst + (i64)n * bs + (i64)c * Hc * Wc;
  if (route == 1) adjoint2x_q(gp, dp, Hc, Wc, acc);
  else adjoint_generic(gp, dp, Hc, Wc, Hf, Wf, sh, sw, acc);
}

inline bool al(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

bool fill_levels(FpnArgs& a, int K, float* const* ptrs, const long long* bs, const int* hs, const int* ws, const int* chan_off, int C, int Hf,
                 int Wf) {
  if (K < 1 || K > MAXL || !ptrs || !bs || !hs || !ws || !chan_off) return false;
  for (int k = 0; k < MAXL; ++k) {
    const bool on = k < K;
    if (on && (!ptrs[k] || hs[k] < 1 || ws[k] < 1 || hs[k] > Hf || ws[k] > Wf || chan_off[k] < 0 || bs[k] < (long long)C * hs[k] * ws[k])) return false;
    a.h[k] = on ? hs[k] : 1;
    a.w[k] = on ? ws[k] : 1;
    a.coff[k] = on ? chan_off[k] : 0;
    a.route[k] = a.acc[k] = 0;
    a.sh[k] = on ? (float)hs[k] / (float)Hf : 1.f;
    a.sw[k] = on ? (float)ws[k] / (float)Wf : 1.f;
    a.bs[k] = on ? bs[k] : 0;
    a.p[k] = on ? ptrs[k] : nullptr;
  }
  // the slices must not overlap: level k owns channels [coff, coff + C)
  for (int k = 0; k < K; ++k)
    for (int j = 0; j < k; ++j)
      if (a.coff[k] < a.coff[j] + C && a.coff[j] < a.coff[k] + C) return false;
  return true;
}

}  // namespace

// ---- which form a launch takes: the launchers below ask these, and so can a test
extern "C" int pfst_topdown_merge_route(const float* lat, long long lat_bs, const float* coarse, long long coarse_bs, const float* out,
                                        long long out_bs, int Hc, int Wc, int Hf, int Wf) {
  const bool quads = (Wf & 3) == 0 && (lat_bs & 3) == 0 && (out_bs & 3) == 0 && al(lat, 15) && al(out, 15);
  if (quads && Hf == 2 * Hc && Wf == 2 * Wc && Hc > 1 && Wc > 1 && (Wc & 1) == 0 && (coarse_bs & 1) == 0 && al(coarse, 7)) return 2;
  return quads ? 1 : 0;
}
extern "C" int pfst_fpn_resize_concat_route(const float* y, long long y_bs, int Hf, int Wf) {
  return (Wf & 3) == 0 && (y_bs & 3) == 0 && al(y, 15) ? 1 : 0;
}
extern "C" int pfst_fpn_resize_concat_bwd_route(const float* dy_plane, long long dy_bs, const float* d_src, long long src_bs, int Hc, int Wc,
                                                int Hf, int Wf) {
  return Hf == 2 * Hc && Wf == 2 * Wc && Hc > 1 && Wc > 1 && (Hc & 1) == 0 && (Wc & 1) == 0 && (dy_bs & 3) == 0 && (src_bs & 1) == 0 &&
                 al(dy_plane, 15) && al(d_src, 7)
             ? 1
             : 0;
}

extern "C" int pfst_topdown_merge(const float* lat, long long lat_bs, const float* coarse, long long coarse_bs, float* out, long long out_bs,
                                  int N, int C, int Hc, int Wc, int Hf, int Wf, float* y_amax, pfst_stream_t stream) {
  PFST_CHECK_ARG(lat && coarse && out && out != lat && out != coarse && N > 0 && C > 0 && Hc > 0 && Wc > 0 && C <= 65535 && N <= 65535);
  PFST_CHECK_ARG(Hf >= Hc && Wf >= Wc && (long long)Hf * Wf < (1ll << 31));
  PFST_CHECK_ARG(lat_bs >= (long long)C * Hf * Wf && out_bs >= (long long)C * Hf * Wf && coarse_bs >= (long long)C * Hc * Wc);
  const int route = pfst_topdown_merge_route(lat, lat_bs, coarse, coarse_bs, out, out_bs, Hc, Wc, Hf, Wf);
  const float sh = (float)Hc / (float)Hf, sw = (float)Wc / (float)Wf;          // = pfst_resize_bilinear's
  if (route == 2)
    hipLaunchKernelGGL(topdown_merge2x_kernel, dim3(cdiv(Hc + 1, 4), C, N), dim3(256), 0, (hipStream_t)stream, lat, (i64)lat_bs, coarse,
                       (i64)coarse_bs, out, (i64)out_bs, Hc, Wc, y_amax);
  else if (route == 1)
    hipLaunchKernelGGL(topdown_merge_kernel<true>, dim3(px_grid((i64)Hf * Wf / 4), C, N), dim3(256), 0, (hipStream_t)stream, lat, (i64)lat_bs,
                       coarse, (i64)coarse_bs, out, (i64)out_bs, Hc, Wc, Hf, Wf, sh, sw, y_amax);
  else
    hipLaunchKernelGGL(topdown_merge_kernel<false>, dim3(px_grid((i64)Hf * Wf), C, N), dim3(256), 0, (hipStream_t)stream, lat, (i64)lat_bs,
                       coarse, (i64)coarse_bs, out, (i64)out_bs, Hc, Wc, Hf, Wf, sh, sw, y_amax);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_fpn_resize_concat(const float* const* srcs, const long long* src_bs, const int* src_h, const int* src_w, const int* chan_off,
                                      int K, float* y, long long y_bs, int N, int C, int Hf, int Wf, float* y_amax, pfst_stream_t stream) {
  FpnArgs a;
  PFST_CHECK_ARG(y && N > 0 && C > 0 && Hf > 0 && Wf > 0 && N <= 65535 && (long long)Hf * Wf < (1ll << 31));
  PFST_CHECK_ARG(fill_levels(a, K, const_cast<float* const*>(reinterpret_cast<const float* const*>(srcs)), src_bs, src_h, src_w, chan_off, C, Hf, Wf));
  PFST_CHECK_ARG((long long)C * K <= 65535);
  for (int k = 0; k < K; ++k) PFST_CHECK_ARG(y_bs >= (long long)(a.coff[k] + C) * Hf * Wf);
  if (pfst_fpn_resize_concat_route(y, y_bs, Hf, Wf))
    hipLaunchKernelGGL(fpn_resize_concat_kernel<true>, dim3(px_grid((i64)Hf * Wf / 4), C * K, N), dim3(256), 0, (hipStream_t)stream, a, y,
                       (i64)y_bs, C, Hf, Wf, y_amax);
  else
    hipLaunchKernelGGL(fpn_resize_concat_kernel<false>, dim3(px_grid((i64)Hf * Wf), C * K, N), dim3(256), 0, (hipStream_t)stream, a, y,
                       (i64)y_bs, C, Hf, Wf, y_amax);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_fpn_resize_concat_bwd(const float* dy, long long dy_bs, float* const* d_srcs, const long long* src_bs, const int* src_h,
                                          const int* src_w, const int* chan_off, const int* accumulate, int K, int N, int C, int Hf, int Wf,
                                          pfst_stream_t stream) {
  FpnArgs a;
  PFST_CHECK_ARG(dy && accumulate && N > 0 && C > 0 && Hf > 0 && Wf > 0 && N <= 65535 && (long long)Hf * Wf < (1ll << 31));
  PFST_CHECK_ARG(fill_levels(a, K, d_srcs, src_bs, src_h, src_w, chan_off, C, Hf, Wf));
  PFST_CHECK_ARG((long long)C * K <= 65535);
  i64 work = 1;
  for (int k = 0; k < K; ++k) {
    PFST_CHECK_ARG(dy_bs >= (long long)(a.coff[k] + C) * Hf * Wf);
    a.acc[k] = accumulate[k] ? 1 : 0;
    a.route[k] = pfst_fpn_resize_concat_bwd_route(dy + (i64)a.coff[k] * Hf * Wf, dy_bs, a.p[k], a.bs[k], a.h[k], a.w[k], Hf, Wf);
    const i64 items = (i64)a.h[k] * a.w[k] / (a.route[k] ? 4 : 1);
    work = items > work ? items : work;
  }
  hipLaunchKernelGGL(fpn_resize_concat_bwd_kernel, dim3(px_grid(work), C * K, N), dim3(256), 0, (hipStream_t)stream, dy, (i64)dy_bs, a, C, Hf, Wf);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
