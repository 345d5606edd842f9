// The class walk of one pixel's softmax that the entropy kernels share (entropy_loss.hip: EntropyLoss and the per-class entropy map of the
// adversarial baseline): the constants, the probabilities as torch forms them and the seed dL/dp_c of the entropy term -- one copy, so that
// every user performs the same operations on the same values in the same order.  Include it in a file compiled with contraction off.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int REG_C = 8;                              // classes the register form holds per thread
constexpr float ENT_EPS = 1e-30f;                     // entropy_loss.py:29
constexpr float INV_LN2 = 1.44269504088896340736f;

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

}  // namespace
