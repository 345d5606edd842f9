// EntropyLoss on the student's low-resolution logits of the mixed pass: entropy minimisation (MinEnt) and the
// max-squares loss, forward and backward.  Reference: rsiseg/models/losses/entropy_loss.py:27-42.
//
//   p = softmax_c(z) as torch forms it: exp(z - max) / sum
//   kind 0 (entropy):    e = -sum_c p_c log2(p_c + 1e-30) / log2(C)      loss =  weight * sum_px e / (N h w)
//   kind 1 (max_square): s =  sum_c p_c^2                                loss = -weight * sum_px s / (2 N C h w)
//
// The same file holds the per-class entropy MAP of the adversarial baseline (adv_loss.py:47-50) and its adjoint: the same
// class walk (entropy_walk.h), not summed over the classes.
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
#include "entropy_walk.h"
#include "../../include/pfst_hip.h"

#pragma clang fp contract(off)

namespace {

// a pixel's term of the forward sum from one class
template <int KIND>
__device__ __forceinline__ float fwd_term(float pc, float acc) {
  return KIND == 0 ? __builtin_fmaf(pc, log2f(pc + ENT_EPS), acc) : __builtin_fmaf(pc, pc, acc);
}

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

// The per-class entropy map that the adversarial baseline's discriminator reads (adv_loss.py:47-50): e_c = -p_c log2(p_c + 1e-30) / log2(C),
// not summed over the classes.                                                                             grid: (ceil(HW / 256), N)
template <bool REG>
__global__ __launch_bounds__(256) void entropy_map_fwd_kernel(const float* __restrict__ logits, int C, i64 HW, float inv_log2c,
                                                              float* __restrict__ ent) {
  const i64 n = blockIdx.y, p = (i64)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  PxLogits<REG> px{logits + n * C * HW + p, HW, C};
  px.softmax();
  float* ep = ent + n * C * HW + p;
  px.each([&](int c, float pc) { ep[c * HW] = -(pc * log2f(pc + ENT_EPS)) * inv_log2c; });
}

// Its adjoint: with G_c = g_e[c] * de_c/dp_c (seed<0> with k = 1 / log2 C), dz_j (+)= p_j * (G_j - sum_c p_c G_c)
template <bool REG>
__global__ __launch_bounds__(256) void entropy_map_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ gent, int C, i64 HW,
                                                              float inv_log2c, float* __restrict__ dlogits, int accumulate) {
  const i64 n = blockIdx.y, p = (i64)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  PxLogits<REG> px{logits + n * C * HW + p, HW, C};
  px.softmax();
  const float* gp = gent + n * C * HW + p;
  float s = 0.f;
  float g[REG_C];                // the register form keeps G; the class loop forms it again
  px.each([&](int c, float pc) {
    const float gc = gp[c * HW] * seed<0>(pc, inv_log2c);
    if (REG) g[c] = gc;
    s = __builtin_fmaf(pc, gc, s);
  });
  float* dp = dlogits + n * C * HW + p;
  px.each([&](int c, float pc) {
    const float gc = REG ? g[c] : gp[c * HW] * seed<0>(pc, inv_log2c);
    const float d = pc * (gc - s);
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

extern "C" int pfst_entropy_map(const float* logits, int N, int C, long long HW, int form, float* ent, pfst_stream_t stream) {
  PFST_CHECK_ARG(shape_ok(logits, N, C, HW, 0, form) && ent);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(HW, 256), N);
  const float inv_log2c = (float)(1.0 / log2((double)C));
  if (form == 0 && C <= REG_C) hipLaunchKernelGGL(entropy_map_fwd_kernel<true>, grid, dim3(256), 0, s, logits, C, (i64)HW, inv_log2c, ent);
  else hipLaunchKernelGGL(entropy_map_fwd_kernel<false>, grid, dim3(256), 0, s, logits, C, (i64)HW, inv_log2c, ent);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_entropy_map_bwd(const float* logits, const float* grad_ent, int N, int C, long long HW, int form, float* dlogits,
                                    int accumulate, pfst_stream_t stream) {
  PFST_CHECK_ARG(shape_ok(logits, N, C, HW, 0, form) && grad_ent && dlogits && (accumulate == 0 || accumulate == 1));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(HW, 256), N);
  const float inv_log2c = (float)(1.0 / log2((double)C));
  if (form == 0 && C <= REG_C)
    hipLaunchKernelGGL(entropy_map_bwd_kernel<true>, grid, dim3(256), 0, s, logits, grad_ent, C, (i64)HW, inv_log2c, dlogits, accumulate);
  else
    hipLaunchKernelGGL(entropy_map_bwd_kernel<false>, grid, dim3(256), 0, s, logits, grad_ent, C, (i64)HW, inv_log2c, dlogits, accumulate);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
