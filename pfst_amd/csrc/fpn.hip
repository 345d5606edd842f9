// The top-down path of a feature pyramid (UPerHead, uper_head.py:108-132) as fused streaming kernels; the Semantic FPN
// kernels (FPN neck, FPNHead; section 8q) follow further down:
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
#include "resize_adjoint.h"
#include "../../include/pfst_hip.h"

namespace {

using pfst_adj::adjoint2x_q_ok;
using pfst_adj::al;
using pfst_adj::px_grid;

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

// ---- concat_bwd: the two gather forms of pfst_resize_bilinear_bwd per level (resize_adjoint.h)
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
  return adjoint2x_q_ok(dy_plane, dy_bs, d_src, src_bs, Hc, Wc, Hf, Wf) ? 1 : 0;
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

// =====================================================================================================================================
// Semantic FPN (necks/fpn.py, decode_heads/fpn_head.py):
//   merge_nearest:      out = lat + coarse[sy(y)][sx(x)], torch's legacy 'nearest' for a given output size, max |out| published
//   nearest_resize_bwd: its adjoint as a gather over the (contiguous) pre-image of every source pixel
//   upsample2x_norm:    out = bilinear_x2(act(pre)), act(v) = max(fma(v, sc, sh), 0) from the lazy record of conv_bn_act, max |out| published
//   fpn_level_sum:      out = act0(pre0) + bilinear_x2((act1(pre1) + act2(pre2)) + act3(pre3)) [+ addend], max |out| published
// The conventions of the kernels above hold: dense planes with batch strides, no atomics, one summation order, pinned roundings.
namespace {

// ---- torch's legacy 'nearest' (UpSample.h, nearest_neighbor_compute_source_index): scale = (float)in / (float)out, formed on the host
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
  const int s = (int)floorf(__fmul_rn((float)dst, scale));
  return s < in - 1 ? s : in - 1;
}
// the first output index whose source is >= t under that (monotone) rule; `out` if there is none.  A division only places a window of five
// candidates (t / scale is off by far less than one index at these sizes); which of them it is, the forward's own expression decides
__device__ __forceinline__ int nearest_first(int t, float scale, int in, int out) {
  if (t >= in) return out;
  const int g = (int)ceilf((float)t / scale);
  int first = out;
#pragma unroll
  for (int d = 2; d >= -2; --d) {
    const int c = g + d;
    if (c >= 0 && c < out && nearest_src(c, scale, in) >= t) first = c;
  }
  return first;
}
// the pre-image [lo, hi) of source index s: a contiguous range
__device__ __forceinline__ void nearest_preimage(int s, float scale, int in, int out, int& lo, int& hi) {
  lo = nearest_first(s, scale, in, out);
  hi = nearest_first(s + 1, scale, in, out);
}

// ---- nearest merge, any ratio.  grid: (blocks over the fine plane, C, N).  VEC: four pixels per thread, 16-byte lat / out accesses
template <bool VEC>
__global__ __launch_bounds__(256) void merge_nearest_kernel(const float* __restrict__ lat, i64 lat_bs, const float* __restrict__ coarse, i64 c_bs,
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
      const float* r = cp + (i64)nearest_src(oy, sh, Hc) * Wc;
      const float4 l = reinterpret_cast<const float4*>(lp)[q];
      float4 v;
      v.x = __fadd_rn(l.x, r[nearest_src(ox0, sw, Wc)]);
      v.y = __fadd_rn(l.y, r[nearest_src(ox0 + 1, sw, Wc)]);
      v.z = __fadd_rn(l.z, r[nearest_src(ox0 + 2, sw, Wc)]);
      v.w = __fadd_rn(l.w, r[nearest_src(ox0 + 3, sw, Wc)]);
      reinterpret_cast<float4*>(op)[q] = v;
      m = amax4(m, v);
    }
  } else {
    for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < Hf * Wf; o += gridDim.x * blockDim.x) {
      const int oy = o / Wf, ox = o - oy * Wf;
      const float v = __fadd_rn(lp[o], cp[(i64)nearest_src(oy, sh, Hc) * Wc + nearest_src(ox, sw, Wc)]);
      op[o] = v;
      m = fmaxf(m, fabsf(v));
    }
  }
  if (amax) amax_publish(amax, m);
}
// the exact x2 form (scale 1/2: the source of dst is dst >> 1): one 8-byte coarse load feeds a 2 x 4 block of the fine map.  Wc even
__global__ __launch_bounds__(256) void merge_nearest2x_kernel(const float* __restrict__ lat, i64 lat_bs, const float* __restrict__ coarse, i64 c_bs,
                                                              float* __restrict__ out, i64 out_bs, int Hc, int Wc, float* __restrict__ amax) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int W2 = Wc >> 1;                                  // = float4s per fine row
  const float* cp = coarse + (i64)n * c_bs + (i64)c * Hc * Wc;
  const float* lp = lat + (i64)n * lat_bs + (i64)c * 4 * Hc * Wc;
  float* op = out + (i64)n * out_bs + (i64)c * 4 * Hc * Wc;
  float m = 0.f;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < Hc * W2; q += gridDim.x * blockDim.x) {
    const int cy = q / W2, j = q - cy * W2;
    const float2 s = *reinterpret_cast<const float2*>(cp + (i64)cy * Wc + 2 * j);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const i64 f = (i64)(2 * cy + r) * W2 + j;
      const float4 l = reinterpret_cast<const float4*>(lp)[f];
      float4 v;
      v.x = __fadd_rn(l.x, s.x); v.y = __fadd_rn(l.y, s.x); v.z = __fadd_rn(l.z, s.y); v.w = __fadd_rn(l.w, s.y);
      reinterpret_cast<float4*>(op)[f] = v;
      m = amax4(m, v);
    }
  }
  if (amax) amax_publish(amax, m);
}

// ---- the adjoint of the nearest resize: a plain sum over the pre-image, rows ascending, columns ascending within a row
__global__ __launch_bounds__(256) void nearest_resize_bwd_kernel(const float* __restrict__ dy, i64 dy_bs, float* __restrict__ dx, i64 dx_bs, int Hc,
                                                                 int Wc, int Hf, int Wf, float sh, float sw, int accumulate) {
  const int c = blockIdx.y, n = blockIdx.z;
  const float* gp = dy + (i64)n * dy_bs + (i64)c * Hf * Wf;
  float* dp = dx + (i64)n * dx_bs + (i64)c * Hc * Wc;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Hc * Wc; i += gridDim.x * blockDim.x) {
    const int iy = i / Wc, ix = i - iy * Wc;
    int y_lo, y_hi, x_lo, x_hi;
    nearest_preimage(iy, sh, Hc, Hf, y_lo, y_hi);
    nearest_preimage(ix, sw, Wc, Wf, x_lo, x_hi);
    float acc = 0.f;
    for (int oy = y_lo; oy < y_hi; ++oy)
      for (int ox = x_lo; ox < x_hi; ++ox) acc = __fadd_rn(acc, gp[(i64)oy * Wf + ox]);
    dp[i] = accumulate ? __fadd_rn(dp[i], acc) : acc;
  }
}
// x2: two source pixels per thread from two 16-byte loads, the same order of terms (0 + a is a)
__global__ __launch_bounds__(256) void nearest_resize2x_bwd_kernel(const float* __restrict__ dy, i64 dy_bs, float* __restrict__ dx, i64 dx_bs, int Hc,
                                                                   int Wc, int accumulate) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int W2 = Wc >> 1;
  const float* gp = dy + (i64)n * dy_bs + (i64)c * 4 * Hc * Wc;
  float* dp = dx + (i64)n * dx_bs + (i64)c * Hc * Wc;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < Hc * W2; q += gridDim.x * blockDim.x) {
    const int cy = q / W2, j = q - cy * W2;
    const float4 a = reinterpret_cast<const float4*>(gp)[(i64)(2 * cy) * W2 + j], b = reinterpret_cast<const float4*>(gp)[(i64)(2 * cy + 1) * W2 + j];
    float2 v = make_float2(__fadd_rn(__fadd_rn(__fadd_rn(a.x, a.y), b.x), b.y), __fadd_rn(__fadd_rn(__fadd_rn(a.z, a.w), b.z), b.w));
    float2* d2 = reinterpret_cast<float2*>(dp + (i64)cy * Wc + 2 * j);
    if (accumulate) { const float2 old = *d2; v.x = __fadd_rn(old.x, v.x); v.y = __fadd_rn(old.y, v.y); }
    *d2 = v;
  }
}

// ---- normalise on load: row c of a [C, 4] table (mean, invstd, sc, sh) as conv_bn_act leaves it; a null table: the values are final
struct Act {
  float sc, sh;
  bool on;
};
__device__ __forceinline__ Act load_act(const float* __restrict__ coef, int c) {
  Act a;
  a.on = coef != nullptr;
  a.sc = a.on ? coef[4 * c + 2] : 1.f;
  a.sh = a.on ? coef[4 * c + 3] : 0.f;
  return a;
}
__device__ __forceinline__ float act(const Act& a, float v) { return a.on ? fmaxf(__fmaf_rn(v, a.sc, a.sh), 0.f) : v; }

// ---- upsample2x_norm, the pixel form: any Hc x Wc -> 2 Hc x 2 Wc.  grid: (blocks over the fine plane, C, N)
__global__ __launch_bounds__(256) void upsample2x_norm_kernel(const float* __restrict__ pre, i64 pre_bs, const float* __restrict__ coef,
                                                              float* __restrict__ out, i64 out_bs, int Hc, int Wc, float* __restrict__ amax) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int Hf = 2 * Hc, Wf = 2 * Wc;
  const float* p = pre + (i64)n * pre_bs + (i64)c * Hc * Wc;
  float* op = out + (i64)n * out_bs + (i64)c * Hf * Wf;
  const Act a = load_act(coef, c);
  float m = 0.f;
  for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < Hf * Wf; o += gridDim.x * blockDim.x) {
    const int oy = o / Wf, ox = o - oy * Wf;
    const Bilin b = make_bilin(oy, ox, 0.5f, 0.5f, Hc, Wc);
    const float v = bilin_blend(act(a, p[b.y0 * Wc + b.x0]), act(a, p[b.y0 * Wc + b.x1]), act(a, p[b.y1 * Wc + b.x0]), act(a, p[b.y1 * Wc + b.x1]),
                                b.lx0, b.lx1, b.ly0, b.ly1);
    op[o] = v;
    m = fmaxf(m, fabsf(v));
  }
  if (amax) amax_publish(amax, m);
}

// the eight source values one thread of the x2 walk blends (resize_bilinear2x_kernel): columns 2j, 2j+1 and the clamped 2j-1, 2j+2 of two rows
struct Walk8 {
  float2 m0, m1;
  float l0, l1, g0, g1;
};
__device__ __forceinline__ Walk8 walk_load(const float* __restrict__ r0, const float* __restrict__ r1, int j, int Wc, const Act& a) {
  const int cl = max(2 * j - 1, 0), cr = min(2 * j + 2, Wc - 1);
  Walk8 w;
  w.m0 = *reinterpret_cast<const float2*>(r0 + 2 * j);
  w.m1 = *reinterpret_cast<const float2*>(r1 + 2 * j);
  w.l0 = r0[cl]; w.l1 = r1[cl]; w.g0 = r0[cr]; w.g1 = r1[cr];
  w.m0.x = act(a, w.m0.x); w.m0.y = act(a, w.m0.y); w.m1.x = act(a, w.m1.x); w.m1.y = act(a, w.m1.y);
  w.l0 = act(a, w.l0); w.l1 = act(a, w.l1); w.g0 = act(a, w.g0); w.g1 = act(a, w.g1);
  return w;
}
__device__ __forceinline__ void walk_add(Walk8& s, const Walk8& w) {
  s.m0.x = __fadd_rn(s.m0.x, w.m0.x); s.m0.y = __fadd_rn(s.m0.y, w.m0.y); s.m1.x = __fadd_rn(s.m1.x, w.m1.x); s.m1.y = __fadd_rn(s.m1.y, w.m1.y);
  s.l0 = __fadd_rn(s.l0, w.l0); s.l1 = __fadd_rn(s.l1, w.l1); s.g0 = __fadd_rn(s.g0, w.g0); s.g1 = __fadd_rn(s.g1, w.g1);
}
__device__ __forceinline__ float4 walk_row(const Walk8& w, int j, float ly0, float ly1) {
  float4 o;
  o.x = j > 0 ? bilin_blend(w.l0, w.m0.x, w.l1, w.m1.x, 0.25f, 0.75f, ly0, ly1) : bilin_blend(w.m0.x, w.m0.y, w.m1.x, w.m1.y, 1.f, 0.f, ly0, ly1);
  o.y = bilin_blend(w.m0.x, w.m0.y, w.m1.x, w.m1.y, 0.75f, 0.25f, ly0, ly1);
  o.z = bilin_blend(w.m0.x, w.m0.y, w.m1.x, w.m1.y, 0.25f, 0.75f, ly0, ly1);
  o.w = bilin_blend(w.m0.y, w.g0, w.m1.y, w.g1, 0.75f, 0.25f, ly0, ly1);
  return o;
}
// the row pair a wave of the walk owns: output rows 2p-1 (p >= 1) and 2p (p <= Hc-1) from source rows p-1, p
struct WalkRows {
  int ra, rb;
  bool hasA, hasB;
  float la0, la1, lb0, lb1;
};
__device__ __forceinline__ WalkRows walk_rows(int p, int Hc) {
  WalkRows r;
  r.ra = max(p - 1, 0); r.rb = min(p, Hc - 1);
  r.hasA = p >= 1; r.hasB = p <= Hc - 1;
  r.la0 = r.la1 = r.lb0 = r.lb1 = 0.f;
  int y0, y1;
  if (r.hasA) bilin_src(2 * p - 1, 0.5f, Hc, y0, y1, r.la0, r.la1);
  if (r.hasB) bilin_src(2 * p, 0.5f, Hc, y0, y1, r.lb0, r.lb1);
  return r;
}

// ---- upsample2x_norm, the x2 walk.  grid: ((Hc + 1) / 4 rounded up, C, N), 256 threads = four row pairs; Wc even
__global__ __launch_bounds__(256) void upsample2x_norm_walk_kernel(const float* __restrict__ pre, i64 pre_bs, const float* __restrict__ coef,
                                                                   float* __restrict__ out, i64 out_bs, int Hc, int Wc, float* __restrict__ amax) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int Wf = 2 * Wc, W4 = Wf >> 2;
  const float* p0 = pre + (i64)n * pre_bs + (i64)c * Hc * Wc;
  float* op = out + (i64)n * out_bs + (i64)c * 4 * Hc * Wc;
  const Act a = load_act(coef, c);
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  float m = 0.f;
  if (p <= Hc) {
    const WalkRows r = walk_rows(p, Hc);
    const float* r0 = p0 + (i64)r.ra * Wc;
    const float* r1 = p0 + (i64)r.rb * Wc;
    float4* outA = reinterpret_cast<float4*>(op + (i64)(2 * p - 1) * Wf);
    float4* outB = reinterpret_cast<float4*>(op + (i64)(2 * p) * Wf);
    for (int j = threadIdx.x & 63; j < W4; j += 64) {
      const Walk8 w = walk_load(r0, r1, j, Wc, a);
      if (r.hasA) { const float4 o = walk_row(w, j, r.la0, r.la1); outA[j] = o; m = amax4(m, o); }
      if (r.hasB) { const float4 o = walk_row(w, j, r.lb0, r.lb1); outB[j] = o; m = amax4(m, o); }
    }
  }
  if (amax) amax_publish(amax, m);
}

// ---- fpn_level_sum.  The members come by value
constexpr int MAXM = PFST_FPN_MAX_LEVELS;
struct LevelSumArgs {
  const float* pre0; i64 bs0; const float* coef0;
  const float* p[MAXM]; i64 bs[MAXM]; const float* coef[MAXM];
  const float* addend; i64 add_bs;
  int K;
};
// the pixel form: any H0 x W0 (K = 0), or H0 = 2 Hh, W0 = 2 Wh.  VEC0: K = 0 only, a flat pass in 16-byte accesses (H0 W0 % 4 == 0)
template <bool VEC0>
__global__ __launch_bounds__(256) void fpn_level_sum_kernel(LevelSumArgs a, float* __restrict__ out, i64 out_bs, int H0, int W0,
                                                            float* __restrict__ amax) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int HW = H0 * W0, Hh = H0 >> 1, Wh = W0 >> 1;
  const float* p0 = a.pre0 + (i64)n * a.bs0 + (i64)c * HW;
  const float* ap = a.addend ? a.addend + (i64)n * a.add_bs + (i64)c * HW : nullptr;
  float* op = out + (i64)n * out_bs + (i64)c * HW;
  const Act a0 = load_act(a.coef0, c);
  float m = 0.f;
  if (VEC0) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < (HW >> 2); q += gridDim.x * blockDim.x) {
      float4 v = reinterpret_cast<const float4*>(p0)[q];
      v.x = act(a0, v.x); v.y = act(a0, v.y); v.z = act(a0, v.z); v.w = act(a0, v.w);
      if (ap) {
        const float4 d = reinterpret_cast<const float4*>(ap)[q];
        v.x = __fadd_rn(v.x, d.x); v.y = __fadd_rn(v.y, d.y); v.z = __fadd_rn(v.z, d.z); v.w = __fadd_rn(v.w, d.w);
      }
      reinterpret_cast<float4*>(op)[q] = v;
      m = amax4(m, v);
    }
  } else {
    const float* pk[MAXM];
    Act ak[MAXM];
#pragma unroll
    for (int k = 0; k < MAXM; ++k) {
      const bool on = k < a.K;
      pk[k] = on ? a.p[k] + (i64)n * a.bs[k] + (i64)c * Hh * Wh : nullptr;
      ak[k] = load_act(on ? a.coef[k] : nullptr, c);
    }
    for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < HW; o += gridDim.x * blockDim.x) {
      float v = act(a0, p0[o]);
      if (a.K > 0) {
        const int oy = o / W0, ox = o - oy * W0;
        const Bilin b = make_bilin(oy, ox, 0.5f, 0.5f, Hh, Wh);
        const int i00 = b.y0 * Wh + b.x0, i01 = b.y0 * Wh + b.x1, i10 = b.y1 * Wh + b.x0, i11 = b.y1 * Wh + b.x1;
        float t00 = act(ak[0], pk[0][i00]), t01 = act(ak[0], pk[0][i01]), t10 = act(ak[0], pk[0][i10]), t11 = act(ak[0], pk[0][i11]);
#pragma unroll
        for (int k = 1; k < MAXM; ++k)
          if (k < a.K) {
            t00 = __fadd_rn(t00, act(ak[k], pk[k][i00])); t01 = __fadd_rn(t01, act(ak[k], pk[k][i01]));
            t10 = __fadd_rn(t10, act(ak[k], pk[k][i10])); t11 = __fadd_rn(t11, act(ak[k], pk[k][i11]));
          }
        v = __fadd_rn(v, bilin_blend(t00, t01, t10, t11, b.lx0, b.lx1, b.ly0, b.ly1));
      }
      if (ap) v = __fadd_rn(v, ap[o]);
      op[o] = v;
      m = fmaxf(m, fabsf(v));
    }
  }
  if (amax) amax_publish(amax, m);
}
// the x2 walk, K >= 1.  grid: ((Hh + 1) / 4 rounded up, C, N); Wh even
__global__ __launch_bounds__(256) void fpn_level_sum_walk_kernel(LevelSumArgs a, float* __restrict__ out, i64 out_bs, int Hh, int Wh,
                                                                 float* __restrict__ amax) {
  const int c = blockIdx.y, n = blockIdx.z;
  const int W0 = 2 * Wh, W4 = W0 >> 2;
  const i64 HW = (i64)4 * Hh * Wh;
  const float* p0 = a.pre0 + (i64)n * a.bs0 + (i64)c * HW;
  const float* ap = a.addend ? a.addend + (i64)n * a.add_bs + (i64)c * HW : nullptr;
  float* op = out + (i64)n * out_bs + (i64)c * HW;
  const Act a0 = load_act(a.coef0, c);
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  float m = 0.f;
  if (p <= Hh) {
    const WalkRows r = walk_rows(p, Hh);
    const float* r0[MAXM];
    const float* r1[MAXM];
    Act ak[MAXM];
#pragma unroll
    for (int k = 0; k < MAXM; ++k) {
      const bool on = k < a.K;
      const float* base = on ? a.p[k] + (i64)n * a.bs[k] + (i64)c * Hh * Wh : nullptr;
      r0[k] = on ? base + (i64)r.ra * Wh : nullptr;
      r1[k] = on ? base + (i64)r.rb * Wh : nullptr;
      ak[k] = load_act(on ? a.coef[k] : nullptr, c);
    }
    for (int j = threadIdx.x & 63; j < W4; j += 64) {
      Walk8 s = walk_load(r0[0], r1[0], j, Wh, ak[0]);
#pragma unroll
      for (int k = 1; k < MAXM; ++k)
        if (k < a.K) walk_add(s, walk_load(r0[k], r1[k], j, Wh, ak[k]));
      auto row = [&](float ly0, float ly1, i64 off) {
        float4 v = reinterpret_cast<const float4*>(p0 + off)[j];
        const float4 u = walk_row(s, j, ly0, ly1);
        v.x = __fadd_rn(act(a0, v.x), u.x); v.y = __fadd_rn(act(a0, v.y), u.y); v.z = __fadd_rn(act(a0, v.z), u.z); v.w = __fadd_rn(act(a0, v.w), u.w);
        if (ap) {
          const float4 d = reinterpret_cast<const float4*>(ap + off)[j];
          v.x = __fadd_rn(v.x, d.x); v.y = __fadd_rn(v.y, d.y); v.z = __fadd_rn(v.z, d.z); v.w = __fadd_rn(v.w, d.w);
        }
        reinterpret_cast<float4*>(op + off)[j] = v;
        m = amax4(m, v);
      };
      if (r.hasA) row(r.la0, r.la1, (i64)(2 * p - 1) * W0);
      if (r.hasB) row(r.lb0, r.lb1, (i64)(2 * p) * W0);
    }
  }
  if (amax) amax_publish(amax, m);
}

inline bool quads_ok(const void* p, long long bs) { return al(p, 15) && (bs & 3) == 0; }
inline bool pairs_ok(const void* p, long long bs) { return al(p, 7) && (bs & 1) == 0; }

}  // namespace

extern "C" int pfst_topdown_merge_nearest_route(const float* lat, long long lat_bs, const float* coarse, long long coarse_bs, const float* out,
                                                long long out_bs, int Hc, int Wc, int Hf, int Wf) {
  const bool quads = (Wf & 3) == 0 && quads_ok(lat, lat_bs) && quads_ok(out, out_bs);
  if (quads && Hf == 2 * Hc && Wf == 2 * Wc && (Wc & 1) == 0 && pairs_ok(coarse, coarse_bs)) return 2;
  return quads ? 1 : 0;
}
extern "C" int pfst_nearest_resize_bwd_route(const float* dy, long long dy_bs, const float* dx, long long dx_bs, int Hc, int Wc, int Hf, int Wf) {
  return Hf == 2 * Hc && Wf == 2 * Wc && (Wc & 1) == 0 && quads_ok(dy, dy_bs) && pairs_ok(dx, dx_bs) ? 1 : 0;
}
extern "C" int pfst_upsample2x_norm_route(const float* pre, long long pre_bs, const float* out, long long out_bs, int Hc, int Wc) {
  return Hc > 1 && Wc > 1 && (Wc & 1) == 0 && pairs_ok(pre, pre_bs) && quads_ok(out, out_bs) ? 1 : 0;
}
extern "C" int pfst_fpn_level_sum_route(const float* pre0, long long pre0_bs, const float* const* members, const long long* member_bs, int K,
                                        const float* addend, long long addend_bs, const float* out, long long out_bs, int H0, int W0) {
  if (!(quads_ok(pre0, pre0_bs) && quads_ok(out, out_bs) && (!addend || quads_ok(addend, addend_bs)))) return 0;
  if (K <= 0) return (((long long)H0 * W0) & 3) == 0 ? 1 : 0;
  const int Hh = H0 >> 1, Wh = W0 >> 1;
  if (!(Hh > 1 && Wh > 1 && (Wh & 1) == 0) || !members || !member_bs) return 0;
  for (int k = 0; k < K && k < MAXM; ++k)
    if (!pairs_ok(members[k], member_bs[k])) return 0;
  return 1;
}

extern "C" int pfst_topdown_merge_nearest(const float* lat, long long lat_bs, const float* coarse, long long coarse_bs, float* out, long long out_bs,
                                          int N, int C, int Hc, int Wc, int Hf, int Wf, float* y_amax, pfst_stream_t stream) {
  PFST_CHECK_ARG(lat && coarse && out && out != lat && out != coarse && N > 0 && C > 0 && Hc > 0 && Wc > 0 && C <= 65535 && N <= 65535);
  PFST_CHECK_ARG(Hf >= Hc && Wf >= Wc && (long long)Hf * Wf < (1ll << 31));
  PFST_CHECK_ARG(lat_bs >= (long long)C * Hf * Wf && out_bs >= (long long)C * Hf * Wf && coarse_bs >= (long long)C * Hc * Wc);
  const int route = pfst_topdown_merge_nearest_route(lat, lat_bs, coarse, coarse_bs, out, out_bs, Hc, Wc, Hf, Wf);
  const float sh = (float)Hc / (float)Hf, sw = (float)Wc / (float)Wf;
  if (route == 2)
    hipLaunchKernelGGL(merge_nearest2x_kernel, dim3(px_grid((i64)Hc * Wc / 2), C, N), dim3(256), 0, (hipStream_t)stream, lat, (i64)lat_bs, coarse,
                       (i64)coarse_bs, out, (i64)out_bs, Hc, Wc, y_amax);
  else if (route == 1)
    hipLaunchKernelGGL(merge_nearest_kernel<true>, dim3(px_grid((i64)Hf * Wf / 4), C, N), dim3(256), 0, (hipStream_t)stream, lat, (i64)lat_bs,
                       coarse, (i64)coarse_bs, out, (i64)out_bs, Hc, Wc, Hf, Wf, sh, sw, y_amax);
  else
    hipLaunchKernelGGL(merge_nearest_kernel<false>, dim3(px_grid((i64)Hf * Wf), C, N), dim3(256), 0, (hipStream_t)stream, lat, (i64)lat_bs,
                       coarse, (i64)coarse_bs, out, (i64)out_bs, Hc, Wc, Hf, Wf, sh, sw, y_amax);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_nearest_resize_bwd(const float* dy, long long dy_bs, float* dx, long long dx_bs, int N, int C, int Hc, int Wc, int Hf, int Wf,
                                       int accumulate, pfst_stream_t stream) {
  PFST_CHECK_ARG(dy && dx && dx != dy && N > 0 && C > 0 && Hc > 0 && Wc > 0 && C <= 65535 && N <= 65535);
  PFST_CHECK_ARG(Hf >= Hc && Wf >= Wc && (long long)Hf * Wf < (1ll << 31));
  PFST_CHECK_ARG(dy_bs >= (long long)C * Hf * Wf && dx_bs >= (long long)C * Hc * Wc);
  if (pfst_nearest_resize_bwd_route(dy, dy_bs, dx, dx_bs, Hc, Wc, Hf, Wf))
    hipLaunchKernelGGL(nearest_resize2x_bwd_kernel, dim3(px_grid((i64)Hc * Wc / 2), C, N), dim3(256), 0, (hipStream_t)stream, dy, (i64)dy_bs, dx,
                       (i64)dx_bs, Hc, Wc, accumulate ? 1 : 0);
  else
    hipLaunchKernelGGL(nearest_resize_bwd_kernel, dim3(px_grid((i64)Hc * Wc), C, N), dim3(256), 0, (hipStream_t)stream, dy, (i64)dy_bs, dx,
                       (i64)dx_bs, Hc, Wc, Hf, Wf, (float)Hc / (float)Hf, (float)Wc / (float)Wf, accumulate ? 1 : 0);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_upsample2x_norm(const float* pre, long long pre_bs, const float* coef, float* out, long long out_bs, int N, int C, int Hc,
                                    int Wc, float* y_amax, pfst_stream_t stream) {
  PFST_CHECK_ARG(pre && out && out != pre && N > 0 && C > 0 && Hc > 0 && Wc > 0 && C <= 65535 && N <= 65535);
  PFST_CHECK_ARG((long long)Hc * Wc * 4 < (1ll << 31));
  PFST_CHECK_ARG(pre_bs >= (long long)C * Hc * Wc && out_bs >= (long long)C * Hc * Wc * 4);
  if (pfst_upsample2x_norm_route(pre, pre_bs, out, out_bs, Hc, Wc))
    hipLaunchKernelGGL(upsample2x_norm_walk_kernel, dim3(cdiv(Hc + 1, 4), C, N), dim3(256), 0, (hipStream_t)stream, pre, (i64)pre_bs, coef, out,
                       (i64)out_bs, Hc, Wc, y_amax);
  else
    hipLaunchKernelGGL(upsample2x_norm_kernel, dim3(px_grid((i64)Hc * Wc * 4), C, N), dim3(256), 0, (hipStream_t)stream, pre, (i64)pre_bs, coef, out,
                       (i64)out_bs, Hc, Wc, y_amax);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_fpn_level_sum(const float* pre0, long long pre0_bs, const float* coef0, const float* const* members,
                                  const long long* member_bs, const float* const* member_coef, int K, const float* addend, long long addend_bs,
                                  float* out, long long out_bs, int N, int C, int H0, int W0, float* y_amax, pfst_stream_t stream) {
  PFST_CHECK_ARG(pre0 && out && out != pre0 && out != addend && N > 0 && C > 0 && H0 > 0 && W0 > 0 && C <= 65535 && N <= 65535);
  PFST_CHECK_ARG(K >= 0 && K <= MAXM && (long long)H0 * W0 < (1ll << 31));
  PFST_CHECK_ARG(K == 0 || (members && member_bs && member_coef && (H0 & 1) == 0 && (W0 & 1) == 0));
  const long long plane = (long long)C * H0 * W0;
  PFST_CHECK_ARG(pre0_bs >= plane && out_bs >= plane && (!addend || addend_bs >= plane));
  LevelSumArgs a;
  a.pre0 = pre0; a.bs0 = pre0_bs; a.coef0 = coef0;
  a.addend = addend; a.add_bs = addend ? addend_bs : 0;
  a.K = K;
  for (int k = 0; k < MAXM; ++k) {
    const bool on = k < K;
    if (on) PFST_CHECK_ARG(members[k] && members[k] != out && member_bs[k] >= plane / 4);
    a.p[k] = on ? members[k] : nullptr;
    a.bs[k] = on ? member_bs[k] : 0;
    a.coef[k] = on ? member_coef[k] : nullptr;
  }
  const int route = pfst_fpn_level_sum_route(pre0, pre0_bs, members, member_bs, K, addend, addend_bs, out, out_bs, H0, W0);
  if (route && K > 0)
    hipLaunchKernelGGL(fpn_level_sum_walk_kernel, dim3(cdiv(H0 / 2 + 1, 4), C, N), dim3(256), 0, (hipStream_t)stream, a, out, (i64)out_bs, H0 / 2,
                       W0 / 2, y_amax);
  else if (route)
    hipLaunchKernelGGL(fpn_level_sum_kernel<true>, dim3(px_grid((i64)H0 * W0 / 4), C, N), dim3(256), 0, (hipStream_t)stream, a, out, (i64)out_bs,
                       H0, W0, y_amax);
  else
    hipLaunchKernelGGL(fpn_level_sum_kernel<false>, dim3(px_grid((i64)H0 * W0), C, N), dim3(256), 0, (hipStream_t)stream, a, out, (i64)out_bs, H0,
                       W0, y_amax);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
