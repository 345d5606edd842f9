// The exchange unit that ends every HRModule (backbones/hrnet.py:199-213) as fused streaming kernels:
//   hr_fuse:      out[n][c] = max(((t_0 + t_1) + t_2) + t_3, 0) over B <= 4 operands in branch order, max |out| published.  An operand is
//                   - on the output grid: final values (NULL table), or the PRE-normalisation output of a deferred conv -> BN layer with its
//                     [C, 4] table (mean, invstd, sc, sh): t = fma(v, sc, sh), no ReLU (the fuse layers' BN has no activation);
//                   - on a grid coarser by exactly 2, 4 or 8: t = bilinear(normalised coarse values -> Hf x Wf), at most PFST_FPN_MAX_LEVELS of them
//   hr_fuse_bwd:  gy = (out > 0 ? d_out : 0), the upstream gradient of every output-grid operand, then ONE gather launch that gives every
//                 coarser operand resize^T(gy) on its own grid
// The conventions of fpn.hip hold: align_corners=False, dense planes with batch strides (operands may be views), no atomics but amax_publish
// and one fixed summation order -- deterministic mode needs no second path.  Roundings are pinned: the normalisation is pfst_bn_apply's fma,
// the interpolation bilin.h's (bit-identical to pfst_resize_bilinear), every add one __fadd_rn, the adjoint resize_adjoint.h's (bit-identical
// to pfst_resize_bilinear_bwd).  The fine map moves in 16-byte accesses where its rows allow it; the coarse sources are gathered and re-read
// from L2 (1/4 + 1/16 + 1/64 of a map for the three coarser members of a stage-4 output).
#include "amax.h"
#include "bilin.h"
#include "common.h"
#include "resize_adjoint.h"
#include "../../include/pfst_hip.h"

namespace {

using pfst_adj::adjoint2x_q_ok;
using pfst_adj::al;
using pfst_adj::overlap;
using pfst_adj::px_grid;

constexpr int MAXB = PFST_HR_MAX_BRANCHES;
constexpr int MAXL = PFST_FPN_MAX_LEVELS;

struct HrArgs {
  const float* p[MAXB];
  i64 bs[MAXB];
  const float* coef[MAXB];       // [C, 4] table, or null: the values are final
  int h[MAXB], w[MAXB];          // the operand's own grid
  float sh[MAXB], sw[MAXB];      // h / Hf, w / Wf as pfst_resize_bilinear forms them (on the host)
  int B;
};

// one operand's plane as a thread sees it
struct HrOp {
  const float* p;
  float sc, sh;
  bool on, coarse;
};
__device__ __forceinline__ float norm(const HrOp& o, float v) { return o.on ? __fmaf_rn(v, o.sc, o.sh) : v; }

// four consecutive pixels of output row oy from column ox0, interpolated from the NORMALISED coarse plane
__device__ __forceinline__ float4 norm_quad(const HrOp& o, int Hc, int Wc, int oy, int ox0, float sh, float sw) {
  int y0, y1;
  float ly0, ly1;
  bilin_src(oy, sh, Hc, y0, y1, ly0, ly1);
  const float* r0 = o.p + (i64)y0 * Wc;
  const float* r1 = o.p + (i64)y1 * Wc;
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int x0, x1;
    float lx0, lx1;
    bilin_src(ox0 + k, sw, Wc, x0, x1, lx0, lx1);
    v[k] = bilin_blend(norm(o, r0[x0]), norm(o, r0[x1]), norm(o, r1[x0]), norm(o, r1[x1]), lx0, lx1, ly0, ly1);
  }
  return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ float amax4(float m, const float4& v) {
  return fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}

// grid: (blocks over the fine plane, C, N).  VEC: Wf % 4 == 0 and 16-byte aligned planes of out and of every output-grid operand
template <bool VEC>
__global__ __launch_bounds__(256) void hr_fuse_kernel(HrArgs a, float* __restrict__ out, i64 out_bs, int Hf, int Wf, float* __restrict__ amax) {
  const int c = blockIdx.y, n = blockIdx.z;
  HrOp op[MAXB];
#pragma unroll
  for (int j = 0; j < MAXB; ++j) {
    const bool live = j < a.B;
    op[j].p = live ? a.p[j] + (i64)n * a.bs[j] + (i64)c * a.h[j] * a.w[j] : nullptr;
    op[j].on = live && a.coef[j] != nullptr;
    op[j].sc = op[j].on ? a.coef[j][4 * c + 2] : 1.f;
    op[j].sh = op[j].on ? a.coef[j][4 * c + 3] : 0.f;
    op[j].coarse = live && (a.h[j] != Hf || a.w[j] != Wf);
  }
  float* o = out + (i64)n * out_bs + (i64)c * Hf * Wf;
  float m = 0.f;
  if (VEC) {
    const int W4 = Wf >> 2;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < Hf * W4; q += gridDim.x * blockDim.x) {
      const int oy = q / W4, ox0 = 4 * (q - oy * W4);
      float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int j = 0; j < MAXB; ++j)
        if (j < a.B) {
          float4 t;
          if (op[j].coarse) {
            t = norm_quad(op[j], a.h[j], a.w[j], oy, ox0, a.sh[j], a.sw[j]);
          } else {
            t = reinterpret_cast<const float4*>(op[j].p)[q];
            t.x = norm(op[j], t.x); t.y = norm(op[j], t.y); t.z = norm(op[j], t.z); t.w = norm(op[j], t.w);
          }
          if (j == 0) s = t;
          else { s.x = __fadd_rn(s.x, t.x); s.y = __fadd_rn(s.y, t.y); s.z = __fadd_rn(s.z, t.z); s.w = __fadd_rn(s.w, t.w); }
        }
      s.x = fmaxf(s.x, 0.f); s.y = fmaxf(s.y, 0.f); s.z = fmaxf(s.z, 0.f); s.w = fmaxf(s.w, 0.f);
      reinterpret_cast<float4*>(o)[q] = s;
      m = amax4(m, s);
    }
  } else {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < Hf * Wf; i += gridDim.x * blockDim.x) {
      const int oy = i / Wf, ox = i - oy * Wf;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < MAXB; ++j)
        if (j < a.B) {
          float t;
          if (op[j].coarse) {
            const Bilin b = make_bilin(oy, ox, a.sh[j], a.sw[j], a.h[j], a.w[j]);
            const float* p = op[j].p;
            const int w = a.w[j];
            t = bilin_blend(norm(op[j], p[b.y0 * w + b.x0]), norm(op[j], p[b.y0 * w + b.x1]), norm(op[j], p[b.y1 * w + b.x0]),
                            norm(op[j], p[b.y1 * w + b.x1]), b.lx0, b.lx1, b.ly0, b.ly1);
          } else {
            t = norm(op[j], op[j].p[i]);
          }
          s = j == 0 ? t : __fadd_rn(s, t);
        }
      s = fmaxf(s, 0.f);
      o[i] = s;
      m = fmaxf(m, s);
    }
  }
  if (amax) amax_publish(amax, m);
}

// ---- backward, the gate pass: gy = out > 0 ? d_out : 0.  grid: (blocks over the plane, C, N); gy may be d_out itself (element for element)
template <bool VEC>
__global__ __launch_bounds__(256) void hr_gate_kernel(const float* d_out, i64 d_bs, const float* __restrict__ out, i64 out_bs, float* gy, i64 gy_bs,
                                                      int HW) {
  const int c = blockIdx.y, n = blockIdx.z;
  const float* dp = d_out + (i64)n * d_bs + (i64)c * HW;
  const float* op = out + (i64)n * out_bs + (i64)c * HW;
  float* gp = gy + (i64)n * gy_bs + (i64)c * HW;
  if (VEC) {
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < (HW >> 2); q += gridDim.x * blockDim.x) {
      const float4 d = reinterpret_cast<const float4*>(dp)[q], y = reinterpret_cast<const float4*>(op)[q];
      reinterpret_cast<float4*>(gp)[q] = make_float4(y.x > 0.f ? d.x : 0.f, y.y > 0.f ? d.y : 0.f, y.z > 0.f ? d.z : 0.f, y.w > 0.f ? d.w : 0.f);
    }
  } else {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += gridDim.x * blockDim.x) gp[i] = op[i] > 0.f ? dp[i] : 0.f;
  }
}

// ---- backward, the gather: every coarser member in one launch.  grid: (blocks over the largest level's work, K C, N); a workgroup beyond its
// level's work finds its loop empty
struct HrBwdArgs {
  int h[MAXL], w[MAXL];
  int route[MAXL];               // 0 generic gather, 1 the x2 form on 2 x 2 blocks
  int acc[MAXL];
  float sh[MAXL], sw[MAXL];
  i64 bs[MAXL];
  float* p[MAXL];
};
__global__ __launch_bounds__(256) void hr_fuse_gather_kernel(const float* __restrict__ gy, i64 gy_bs, HrBwdArgs a, int C, int Hf, int Wf) {
  const int lvl = blockIdx.y / C, c = blockIdx.y - lvl * C, n = blockIdx.z;
  int Hc = 1, Wc = 1, route = 0, acc = 0;
  float sh = 1.f, sw = 1.f;
  i64 bs = 0;
  float* dst = nullptr;
#pragma unroll
  for (int k = 0; k < MAXL; ++k)
    if (k == lvl) { Hc = a.h[k]; Wc = a.w[k]; route = a.route[k]; acc = a.acc[k]; sh = a.sh[k]; sw = a.sw[k]; bs = a.bs[k]; dst = a.p[k]; }
  const float* gp = gy + (i64)n * gy_bs + (i64)c * Hf * Wf;
  float* dp = dst + (i64)n * bs + (i64)c * Hc * Wc;
  if (route == 1) adjoint2x_q(gp, dp, Hc, Wc, acc);
  else adjoint_generic(gp, dp, Hc, Wc, Hf, Wf, sh, sw, acc);
}

inline bool quads_ok(const void* p, long long bs) { return al(p, 15) && (bs & 3) == 0; }
// the ratio of an operand's grid to the output grid: 1 (the output grid), 2, 4, 8, or 0 (anything else: not an operand of the fused form)
inline int grid_ratio(int h, int w, int Hf, int Wf) {
  for (int r = 1; r <= 8; r *= 2)
    if (h > 0 && w > 0 && (long long)h * r == Hf && (long long)w * r == Wf) return r;
  return 0;
}

}  // namespace

extern "C" int pfst_hr_fuse_route(const float* const* ops, const long long* op_bs, const int* op_h, const int* op_w, int B, const float* out,
                                  long long out_bs, int Hf, int Wf) {
  if (!ops || !op_bs || !op_h || !op_w || B < 1 || B > MAXB || (Wf & 3) != 0 || !quads_ok(out, out_bs)) return 0;
  for (int j = 0; j < B; ++j)
    if (op_h[j] == Hf && op_w[j] == Wf && !quads_ok(ops[j], op_bs[j])) return 0;
  return 1;
}

extern "C" int pfst_hr_fuse(const float* const* ops, const long long* op_bs, const float* const* op_coef, const int* op_h, const int* op_w, int B,
                            float* out, long long out_bs, int N, int C, int Hf, int Wf, float* y_amax, pfst_stream_t stream) {
  PFST_CHECK_ARG(ops && op_bs && op_coef && op_h && op_w && out && B >= 1 && B <= MAXB);
  PFST_CHECK_ARG(N > 0 && C > 0 && Hf > 0 && Wf > 0 && C <= 65535 && N <= 65535 && (long long)Hf * Wf < (1ll << 31));
  PFST_CHECK_ARG(out_bs >= (long long)C * Hf * Wf);
  HrArgs a;
  int coarser = 0;
  for (int j = 0; j < MAXB; ++j) {
    const bool live = j < B;
    if (live) {
      const int r = grid_ratio(op_h[j], op_w[j], Hf, Wf);
      PFST_CHECK_ARG(ops[j] && r != 0 && op_bs[j] >= (long long)C * op_h[j] * op_w[j]);
      PFST_CHECK_ARG(!overlap(ops[j], op_bs[j], out, out_bs, N, (long long)C * op_h[j] * op_w[j], (long long)C * Hf * Wf));
      coarser += r > 1;
    }
    a.p[j] = live ? ops[j] : nullptr;
    a.bs[j] = live ? op_bs[j] : 0;
    a.coef[j] = live ? op_coef[j] : nullptr;
    a.h[j] = live ? op_h[j] : 1;
    a.w[j] = live ? op_w[j] : 1;
    a.sh[j] = live ? (float)op_h[j] / (float)Hf : 1.f;          // = pfst_resize_bilinear's
    a.sw[j] = live ? (float)op_w[j] / (float)Wf : 1.f;
  }
  a.B = B;
  PFST_CHECK_ARG(coarser <= MAXL);
  if (pfst_hr_fuse_route(ops, op_bs, op_h, op_w, B, out, out_bs, Hf, Wf))
    hipLaunchKernelGGL(hr_fuse_kernel<true>, dim3(px_grid((i64)Hf * Wf / 4), C, N), dim3(256), 0, (hipStream_t)stream, a, out, (i64)out_bs, Hf, Wf,
                       y_amax);
  else
    hipLaunchKernelGGL(hr_fuse_kernel<false>, dim3(px_grid((i64)Hf * Wf), C, N), dim3(256), 0, (hipStream_t)stream, a, out, (i64)out_bs, Hf, Wf,
                       y_amax);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_hr_fuse_bwd(const float* d_out, long long d_out_bs, const float* out, long long out_bs, float* gy, long long gy_bs,
                                float* const* d_coarse, const long long* coarse_bs, const int* coarse_h, const int* coarse_w,
                                const int* accumulate, int K, int N, int C, int Hf, int Wf, pfst_stream_t stream) {
  PFST_CHECK_ARG(d_out && out && gy && N > 0 && C > 0 && Hf > 0 && Wf > 0 && N <= 65535 && (long long)Hf * Wf < (1ll << 31));
  PFST_CHECK_ARG(K >= 0 && K <= MAXL && (long long)C * (K > 0 ? K : 1) <= 65535);
  PFST_CHECK_ARG(K == 0 || (d_coarse && coarse_bs && coarse_h && coarse_w && accumulate));
  const long long plane = (long long)C * Hf * Wf;
  PFST_CHECK_ARG(d_out_bs >= plane && out_bs >= plane && gy_bs >= plane);
  // gy is d_out itself (element for element) or a buffer of its own; it never touches the saved output
  PFST_CHECK_ARG(gy == d_out ? gy_bs == d_out_bs : !overlap(gy, gy_bs, d_out, d_out_bs, N, plane, plane));
  PFST_CHECK_ARG(!overlap(gy, gy_bs, out, out_bs, N, plane, plane));
  HrBwdArgs a;
  i64 work = 1;
  for (int k = 0; k < MAXL; ++k) {
    const bool live = k < K;
    if (live) {
      PFST_CHECK_ARG(d_coarse[k] && d_coarse[k] != gy && grid_ratio(coarse_h[k], coarse_w[k], Hf, Wf) > 1);
      const long long cp = (long long)C * coarse_h[k] * coarse_w[k];
      PFST_CHECK_ARG(coarse_bs[k] >= cp);
      PFST_CHECK_ARG(!overlap(d_coarse[k], coarse_bs[k], gy, gy_bs, N, cp, plane) && !overlap(d_coarse[k], coarse_bs[k], d_out, d_out_bs, N, cp, plane) &&
                     !overlap(d_coarse[k], coarse_bs[k], out, out_bs, N, cp, plane));
      for (int q = 0; q < k; ++q)
        PFST_CHECK_ARG(!overlap(d_coarse[k], coarse_bs[k], d_coarse[q], coarse_bs[q], N, cp, (long long)C * coarse_h[q] * coarse_w[q]));
    }
    a.h[k] = live ? coarse_h[k] : 1;
    a.w[k] = live ? coarse_w[k] : 1;
    a.acc[k] = live && accumulate[k] ? 1 : 0;
    a.sh[k] = live ? (float)coarse_h[k] / (float)Hf : 1.f;
    a.sw[k] = live ? (float)coarse_w[k] / (float)Wf : 1.f;
    a.bs[k] = live ? coarse_bs[k] : 0;
    a.p[k] = live ? d_coarse[k] : nullptr;
    a.route[k] = live && adjoint2x_q_ok(gy, gy_bs, a.p[k], a.bs[k], a.h[k], a.w[k], Hf, Wf) ? 1 : 0;
    if (live) {
      const i64 items = (i64)a.h[k] * a.w[k] / (a.route[k] ? 4 : 1);
      work = items > work ? items : work;
    }
  }
  const i64 HW = (i64)Hf * Wf;
  if ((HW & 3) == 0 && quads_ok(d_out, d_out_bs) && quads_ok(out, out_bs) && quads_ok(gy, gy_bs))
    hipLaunchKernelGGL(hr_gate_kernel<true>, dim3(px_grid(HW / 4), C, N), dim3(256), 0, (hipStream_t)stream, d_out, (i64)d_out_bs, out, (i64)out_bs,
                       gy, (i64)gy_bs, (int)HW);
  else
    hipLaunchKernelGGL(hr_gate_kernel<false>, dim3(px_grid(HW), C, N), dim3(256), 0, (hipStream_t)stream, d_out, (i64)d_out_bs, out, (i64)out_bs, gy,
                       (i64)gy_bs, (int)HW);
  PFST_CHECK_LAUNCH();
  if (K > 0) {
    hipLaunchKernelGGL(hr_fuse_gather_kernel, dim3(px_grid(work), C * K, N), dim3(256), 0, (hipStream_t)stream, gy, (i64)gy_bs, a, C, Hf, Wf);
    PFST_CHECK_LAUNCH();
  }
  return PFST_OK;
}
