// EntropyLoss on the student's low-resolution logits of the mixed pass: entropy minimisation (MinEnt) and the
// max-squares loss, forward and backward.  Reference: rsiseg/models/losses/entropy_loss.py:27-42.
//
//   p = softmax_c(z) as torch forms it: exp(z - max) / sum
//   kind 0 (entropy):    e = -sum_c p_c log2(p_c + 1e-30) / log2(C)      loss =  weight * sum_px e / (N h w)
//   kind 1 (max_square): s =  sum_c p_c^2                                loss = -weight * sum_px s / (2 N C h w)
//
// One pixel per thread, no up-sampling, nothing kept between forward and backward: the backward forms p again from the logits.  A workgroup
// reduces its 256 per-pixel values (fp32 each, added in fp64) by wave shuffles and LDS and STORES one fp64 partial; a single workgroup adds
// the partials in a fixed order.  No atomics anywhere: the result has the same bits run to run in every mode.
//
// The file is compiled with contraction off, and what is meant as one fma is an explicit builtin (entropy_labels.hip gives the reason): the
// register form (C <= 8) and the generic form then perform the same operations on the same values in the same order, and
// `accumulate` adds exactly the value that a plain store writes.
#include <limits.h>
#include "common.h"
#include "../../include/pfst_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int REG_C = 8;                              // classes the register form holds per thread
constexpr float ENT_EPS = 1e-30f;                     // entropy_loss.py:29
constexpr float INV_LN2 = 1.44269504088896340736f;

// a pixel's term of the forward sum from one class
template <int KIND>
__device__ __forceinline__ float fwd_term(float pc, float acc) {
  return KIND == 0 ? __builtin_fmaf(pc, log2f(pc + ENT_EPS), acc) : __builtin_fmaf(pc, pc, acc);
}
// g_c = dL/dp_c as autograd forms it for the reference expression; k = weight / (N h w log2 C) (entropy), weight / (N C h w) (max_square)
template <int KIND>
__device__ __forceinline__ float seed(float pc, float k) {
  if (KIND == 0) {
    const float q = pc + ENT_EPS;
    return -(log2f(q) + (pc / q) * INV_LN2) * k;
  }
  return -pc * k;
}

// The class walk of one pixel.  REG: the logits are read once into registers (class arrays indexed by compile-time constants only) and
// turned into the probabilities in place; else the classes are read again in every pass (the second and later reads hit the cache) and
// every pass forms exp(z - max) / sum again.  Both forms: the maximum, the sum of exponentials and the class terms in class order, by the
// same operations on the same values -- the same bits.  zp: the pixel's class-0 logit, hw: the class stride.
template <bool REG>
struct PxLogits {
  const float* __restrict__ zp;
  i64 hw;
  int C;
  float mx, se;
  float z[REG_C];
  // f(c, z_c) for c = 0 .. C-1
  template <class F>
  __device__ __forceinline__ void each_logit(F&& f) const {
    if (REG) {
#pragma unroll
      for (int c = 0; c < REG_C; ++c)
        if (c < C) f(c, z[c]);
    } else {
      for (int c = 0; c < C; ++c) f(c, zp[c * hw]);
    }
  }
  // p_c = exp(z_c - max) / sum: a division, as torch's softmax
  __device__ __forceinline__ void softmax() {
    if (REG) {
#pragma unroll
      for (int c = 0; c < REG_C; ++c) z[c] = c < C ? zp[c * hw] : -INFINITY;
    }
    float m = -INFINITY, s = 0.f;
    each_logit([&](int, float zc) { m = zc > m ? zc : m; });
    if (REG) {
#pragma unroll
      for (int c = 0; c < REG_C; ++c)
        if (c < C) z[c] = expf(z[c] - m);
#pragma unroll
      for (int c = 0; c < REG_C; ++c)
        if (c < C) s = s + z[c];
#pragma unroll
      for (int c = 0; c < REG_C; ++c)
        if (c < C) z[c] = z[c] / s;
    } else {
      each_logit([&](int, float zc) { s = s + expf(zc - m); });
    }
    mx = m;
    se = s;
  }
  // f(c, p_c) for c = 0 .. C-1, after softmax()
  template <class F>
  __device__ __forceinline__ void each(F&& f) const {
    if (REG) {
#pragma unroll
      for (int c = 0; c < REG_C; ++c)
        if (c < C) f(c, z[c]);
    } else {
      for (int c = 0; c < C; ++c) f(c, expf(zp[c * hw] - mx) / se);
    }
  }
};

// grid: (ceil(HW / 256), N); partial[n * gridDim.x + blockIdx.x] = the workgroup's sum of per-pixel values (e resp. s above, unscaled
// but for 1 / log2 C)
template <bool REG, int KIND>
__global__ __launch_bounds__(256) void entropy_fwd_kernel(const float* __restrict__ logits, int C, i64 HW, float inv_log2c,
                                                          double* __restrict__ partial) {
  __shared__ double sm[16];
  const i64 n = blockIdx.y, p = (i64)blockIdx.x * 256 + threadIdx.x;
  float v = 0.f;
  if (p < HW) {
    PxLogits<REG> px{logits + n * C * HW + p, HW, C};
    px.softmax();
    float acc = 0.f;
    px.each([&](int, float pc) { acc = fwd_term<KIND>(pc, acc); });
    v = KIND == 0 ? -acc * inv_log2c : acc;
  }
  const double tot = block_sum_d((double)v, sm);
  if (threadIdx.x == 0) partial[n * gridDim.x + blockIdx.x] = tot;
}

// One workgroup: thread t adds partials t, t + 1024, ... in index order, then the fixed tree of block_sum_d.  out[0] = (float)(scale * sum)
__global__ __launch_bounds__(1024) void entropy_finalize_kernel(const double* __restrict__ partial, i64 count, double scale,
                                                                float* __restrict__ out) {
  __shared__ double sm[16];
  double a = 0.0;
  for (i64 i = threadIdx.x; i < count; i += 1024) a += partial[i];
  a = block_sum_d(a, sm);
  if (threadIdx.x == 0) out[0] = (float)(scale * a);
}

// dz_j (+)= grad_scale * (p_j * (g_j - sum_c p_c g_c)).                                                  grid: (ceil(HW / 256), N)
template <bool REG, int KIND>
__global__ __launch_bounds__(256) void entropy_bwd_kernel(const float* __restrict__ logits, int C, i64 HW, float k, float grad_scale,
                                                          float* __restrict__ dlogits, int accumulate) {
  const i64 n = blockIdx.y, p = (i64)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  PxLogits<REG> px{logits + n * C * HW + p, HW, C};
  px.softmax();
  float s = 0.f;
  float g[REG_C];                // the register form keeps the seeds; the class loop forms them again
  px.each([&](int c, float pc) {
    const float gc = seed<KIND>(pc, k);
    if (REG) g[c] = gc;
    s = __builtin_fmaf(pc, gc, s);
  });
  float* dp = dlogits + n * C * HW + p;
  px.each([&](int c, float pc) {
    const float gc = REG ? g[c] : seed<KIND>(pc, k);
    const float d = grad_scale * (pc * (gc - s));
    dp[c * HW] = accumulate ? dp[c * HW] + d : d;
  });
}

inline bool shape_ok(const void* logits, int N, int C, i64 HW, int kind, int form) {
  return logits && N > 0 && N <= 65535 && C >= 2 && C <= 255 && HW > 0 && HW < (i64)INT_MAX * 256 && (kind == 0 || kind == 1) &&
         (form == 0 || form == 1);
}

}  // namespace

extern "C" int pfst_softmax_entropy_workspace_bytes(int N, long long HW, long long* bytes) {
  PFST_CHECK_ARG(bytes && N > 0 && N <= 65535 && HW > 0 && HW < (i64)INT_MAX * 256);
  *bytes = (i64)N * cdiv(HW, 256) * (i64)sizeof(double);
  return PFST_OK;
}

#define PFST_ENT_DISPATCH(KERNEL, ...)                                                                        \
  do {                                                                                                        \
    const bool reg_ = form == 0 && C <= REG_C;                                                                \
    if (reg_ && kind == 0) hipLaunchKernelGGL((KERNEL<true, 0>), grid, dim3(256), 0, s, __VA_ARGS__);         \
    else if (reg_) hipLaunchKernelGGL((KERNEL<true, 1>), grid, dim3(256), 0, s, __VA_ARGS__);                 \
    else if (kind == 0) hipLaunchKernelGGL((KERNEL<false, 0>), grid, dim3(256), 0, s, __VA_ARGS__);           \
    else hipLaunchKernelGGL((KERNEL<false, 1>), grid, dim3(256), 0, s, __VA_ARGS__);                          \
  } while (0)

extern "C" int pfst_softmax_entropy_fwd(const float* logits, int N, int C, long long HW, int kind, int form, double weight, double* workspace,
                                        float* out, pfst_stream_t stream) {
  PFST_CHECK_ARG(C >= 2);                      // log2(1) = 0: the reference's normaliser divides by zero
  PFST_CHECK_ARG(shape_ok(logits, N, C, HW, kind, form) && workspace && out);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(HW, 256), N);
  const double log2c = log2((double)C);
  const float inv_log2c = (float)(1.0 / log2c);
  PFST_ENT_DISPATCH(entropy_fwd_kernel, logits, C, (i64)HW, inv_log2c, workspace);
  PFST_CHECK_LAUNCH();
  const double px = (double)N * (double)HW;
  const double scale = kind == 0 ? weight / px : -weight / (2.0 * px * (double)C);
  hipLaunchKernelGGL(entropy_finalize_kernel, dim3(1), dim3(1024), 0, s, workspace, (i64)N * grid.x, scale, out);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_softmax_entropy_bwd(const float* logits, int N, int C, long long HW, int kind, int form, double weight, float grad_scale,
                                        float* dlogits, int accumulate, pfst_stream_t stream) {
  PFST_CHECK_ARG(C >= 2);
  PFST_CHECK_ARG(shape_ok(logits, N, C, HW, kind, form) && dlogits && (accumulate == 0 || accumulate == 1));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(HW, 256), N);
  const double px = (double)N * (double)HW;
  const float k = (float)(kind == 0 ? weight / (px * log2((double)C)) : weight / (px * (double)C));
  PFST_ENT_DISPATCH(entropy_bwd_kernel, logits, C, (i64)HW, k, grad_scale, dlogits, accumulate);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
#undef PFST_ENT_DISPATCH
