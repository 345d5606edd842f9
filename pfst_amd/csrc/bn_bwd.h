// BatchNorm backward of ONE element, one definition of each step for every kernel that evaluates it -- the single-layer and the two-layer
// passes (bn.hip), the depthwise backward that forms dL/dpre while it stages its rows (dwconv.hip): the gated gradient dz (BnGate), the terms
// of (sum dz, sum dz * xhat), the projection dx = gs * (dz - m1 - xhat * m2), and the ReLU bitmask that bn_apply writes and the gates read.
#pragma once
#include "common.h"
#include "../../include/pfst_hip.h"

// THE ReLU bitmask: [N][C][HW / 64] 64-bit words, HW % 256 == 0.  A plane's 256-element group q owns words 4q ... 4q + 3; word k, bit l <-> element
// 256 q + 4 l + k: component k of float4 number i4 = 64 q + l of the plane, which is what lane l of a wave holds in bn_apply.
template <typename W>
__device__ __forceinline__ W* relu_mask_plane(W* mask, int n, int c, int C, int HW) { return mask + ((i64)n * C + c) * (HW >> 6); }
// word (within its plane) of component k of float4 number i4; its bit there is i4 & 63
__device__ __forceinline__ int relu_mask_word(int i4, int k) { return (i4 >> 6) * 4 + k; }

// ReLU gate of element i of a plane: from the bitmask plane mp, else from the saved output y, else (no residual) recomputed from x exactly
// as bn_apply decided it
__device__ __forceinline__ bool relu_on(const unsigned long long* __restrict__ mp, const float* __restrict__ yp, int i, float xv,
                                        float sc, float sh) {
  if (mp) return (mp[relu_mask_word(i >> 2, i & 3)] >> ((i >> 2) & 63)) & 1ull;
  return (yp ? yp[i] : __fmaf_rn(xv, sc, sh)) > 0.f;
}

// ReLU gates of the 4 elements of float4 number i4 of a plane (same sources as relu_on)
__device__ __forceinline__ void relu_on4(const unsigned long long* __restrict__ mp, const float* __restrict__ yp, int i4, const float4& xv,
                                         float sc, float sh, bool (&on)[4]) {
  if (mp) {
    const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(mp + relu_mask_word(i4, 0));       // wave-uniform address: broadcast loads
    const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(mp + relu_mask_word(i4, 2));
    const int l = i4 & 63;
    on[0] = (a.x >> l) & 1ull; on[1] = (a.y >> l) & 1ull; on[2] = (b.x >> l) & 1ull; on[3] = (b.y >> l) & 1ull;
  } else if (yp) {
    const float4 yv = reinterpret_cast<const float4*>(yp)[i4];
    on[0] = yv.x > 0.f; on[1] = yv.y > 0.f; on[2] = yv.z > 0.f; on[3] = yv.w > 0.f;
  } else {
    on[0] = __fmaf_rn(xv.x, sc, sh) > 0.f; on[1] = __fmaf_rn(xv.y, sc, sh) > 0.f; on[2] = __fmaf_rn(xv.z, sc, sh) > 0.f; on[3] = __fmaf_rn(xv.w, sc, sh) > 0.f;
  }
}

// dz of one plane's elements: bn_apply's folded Dropout2d factor first (the incoming gradient is that of y * post[n][c]), then the ReLU gate
struct BnGate {
  bool relu;                              // false: every gate is open
  const unsigned long long* mp;           // the plane's bitmask words, else
  const float* yp;                        // the plane of the saved output, else
  float sc, sh;                           // recomputed from x (bn_affine of the layer)
  bool post;
  float pm;                               // post[n][c]

  __device__ __forceinline__ float dz(float g, int i, float xv) const {
    if (post) g *= pm;
    return relu && !relu_on(mp, yp, i, xv, sc, sh) ? 0.f : g;
  }
  // float4 number i4.  The factor stays ONE uniform branch around four products: four selects would need g before the gate's loads are issued
  __device__ __forceinline__ float4 dz4(float4 g, int i4, const float4& xv) const {
    if (post) { g.x *= pm; g.y *= pm; g.z *= pm; g.w *= pm; }
    if (relu) {
      bool on[4];
      relu_on4(mp, yp, i4, xv, sc, sh, on);
      if (!on[0]) g.x = 0.f;
      if (!on[1]) g.y = 0.f;
      if (!on[2]) g.z = 0.f;
      if (!on[3]) g.w = 0.f;
    }
    return g;
  }
};

// xhat is formed in fp32 here; the products of two fp32 values are exact in fp64, so a fused multiply-add changes nothing in these sums.
// A scalar loop adds its terms one by one (s += dz; sx += bn_bwd_dot(...)), a float4 loop adds the four of a float4 pairwise first: the
// two orders differ, and deterministic mode keeps each (tests/test_batchnorm_edges_gpu.py: test_f_deterministic_routes).
__device__ __forceinline__ double bn_bwd_dot(float dz, float xv, float mu, float is) { return (double)dz * (double)((xv - mu) * is); }
__device__ __forceinline__ double bn_bwd_sum4(const float4& dz) { return ((double)dz.x + (double)dz.y) + ((double)dz.z + (double)dz.w); }
__device__ __forceinline__ double bn_bwd_dot4(const float4& dz, const float4& xv, float mu, float is) {
  return (bn_bwd_dot(dz.x, xv.x, mu, is) + bn_bwd_dot(dz.y, xv.y, mu, is)) + (bn_bwd_dot(dz.z, xv.z, mu, is) + bn_bwd_dot(dz.w, xv.w, mu, is));
}

// dx = gs * (dz - m1 - xhat * m2) in fp64: dz - mean(dz) cancels heavily when dz has a large common mode.  Five roundings, in this order:
// x - mu, (.) * is, dz - m1, ONE fused multiply-add for -(m2 * xhat) + (dz - m1), the product with gs; then the rounding to fp32.  Every
// kernel that writes a BatchNorm input gradient calls this, so two routes to the same dx agree bit for bit.  Contraction is off in the
// body: which product meets which difference is written out, not left to the compiler (the __d*_rn intrinsics are plain operators here and
// would inherit the translation unit's contraction).
__device__ __forceinline__ float bn_bwd_dx(float dz, float xv, const pfst_bn_bwd_rec_t& r) {
#pragma clang fp contract(off)
  const double xh = ((double)xv - (double)r.mu) * (double)r.is;
  return (float)(r.gs * fma(-xh, r.m2, (double)dz - r.m1));
}
__device__ __forceinline__ float4 bn_bwd_dx4(const float4& dz, const float4& xv, const pfst_bn_bwd_rec_t& r) {
  return make_float4(bn_bwd_dx(dz.x, xv.x, r), bn_bwd_dx(dz.y, xv.y, r), bn_bwd_dx(dz.z, xv.z, r), bn_bwd_dx(dz.w, xv.w, r));
}

// the per-channel record of the projection from the two sums ws[2c] = sum dz, ws[2c + 1] = sum dz * xhat (beta NULL: sh from beta = 0)
__device__ __forceinline__ pfst_bn_bwd_rec_t bn_bwd_rec(const double* __restrict__ ws, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, int c, double inv_count) {
  const float mu = mean[c], is = invstd[c];
  pfst_bn_bwd_rec_t r{ws[2 * c] * inv_count, ws[2 * c + 1] * inv_count, (double)gamma[c] * (double)is, mu, is, 0.f, 0.f};
  bn_affine(r.mu, r.is, gamma[c], beta ? beta[c] : 0.f, r.sc, r.sh);
  return r;
}
