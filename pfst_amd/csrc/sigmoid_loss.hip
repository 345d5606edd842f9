// Fused bilinear-upsample + per-(pixel, class) logistic losses (+ accuracy), forward and backward: FocalLoss and CrossEntropyLoss(use_sigmoid).
// As in loss.hip the full-resolution logits are never materialised: every full-resolution pixel interpolates its C logits from the
// low-resolution map in registers, with the helpers and the class order of the CE kernels (the arg-max, hence acc_seg, has the CE path's bits).
// Reference: rsiseg/models/losses/focal_loss.py:13-68, cross_entropy_loss.py:68-156 (the closed form is in DESIGN.md section 8k).
//
//   y = t_c ? -x_c : x_c      q = sigmoid(y)      b = softplus(y) = max(y, 0) + log1p(exp(-|y|))      k = coef[c][t_c ? 0 : 1]
//   l_c = k q^gamma b         dl/dx_c = (t_c ? -1 : 1) k q^gamma (q + gamma (1 - q) b)
//
// with 1 - q = sigmoid(-y) formed as such (never by subtraction) and q^gamma = exp(-gamma softplus(-y)): no negative power, finite everywhere.
// A pixel counts with its weight where label != ignore_index and label < C.  The summation order is fixed in every mode: a workgroup reduces
// by wave shuffles and LDS and STORES one row of partials; pfst_sigloss_finalize adds the rows in a fixed order.  No atomics anywhere.
#include <limits.h>
#include <algorithm>
#include "common.h"
#include "bilin.h"
#include "../../include/pfst_hip.h"

// plain + - * round one by one; every fused multiply-add below is written as one
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// exp(-a), a >= 0, on the hardware's base-2 exponential (v_exp_f32).  libm's expf spends its instructions on the range reduction of an
// argument of either sign and on denormal results; here the argument is never positive and a result below 2^-126 may be 0.  The rounding
// error of the product a log2(e) is carried along (log2(e) in two floats, one fma for the product's error): -a log2(e) = t + r,
// 2^(t + r) = 2^t (1 + r ln 2); the result stays within 2 ulp for every a.  a above 126 (the result is 0 in fp32) is clamped (t stays within
// the instruction's range); a NaN compares false and passes through.
__device__ __forceinline__ float exp_neg(float a) {
  a = a > 126.f ? 126.f : a;
  const float t = a * -1.44269502162933349609375f;
  const float r = fmaf(a, -1.925963033500011e-8f, fmaf(a, -1.44269502162933349609375f, -t));
  const float v = __builtin_amdgcn_exp2f(t);
  return fmaf(v, r * 0.693147182464599609375f, v);
}
// log1p(e) for e in [0, 1], given u = 1 + e (rounded) and r = 1 / u: ln(u) on the hardware's base-2 logarithm (v_log_f32, u in [1, 2]) plus
// the first-order term of what the rounding of 1 + e lost, (e - (u - 1)) / u -- exact differences; log1p(e) -> e as e -> 0, where libm's
// log1pf needs about four times the instructions (profiles/sigmoid_losses.txt)
__device__ __forceinline__ float log1p_unit(float e, float u, float r) {
  return fmaf(__builtin_amdgcn_logf(u), 0.693147182464599609375f, (e - (u - 1.f)) * r);
}

// GM: 0 = gamma == 0 (q^0 = 1, also at q = 0), 2 = gamma == 2 (q q), 1 = any other gamma > 0 (one more exponential, no powf)
// The two sigmoids and the two softpluses of y share ONE exponential, ONE reciprocal and ONE logarithm: e = exp(-|y|), r = 1 / (1 + e).
// What a caller does not read (the forward: p; the gamma = 0 gradient: b) the compiler drops.
template <int GM>
struct SigTerm {
  float q, p, b, qg;      // sigmoid(y), sigmoid(-y), softplus(y), q^gamma
  __device__ __forceinline__ SigTerm(float x, bool hit, float gamma) {
    const float y = hit ? -x : x;
    const float e = exp_neg(fabsf(y)), u = 1.f + e, r = __frcp_rn(u), er = e * r;
    q = y >= 0.f ? r : er;
    p = y >= 0.f ? er : r;
    const float L = log1p_unit(e, u, r);
    b = fmaxf(y, 0.f) + L;
    qg = GM == 0 ? 1.f : GM == 2 ? q * q : exp_neg(gamma * (fmaxf(-y, 0.f) + L));       // q = exp(-softplus(-y))
  }
};

// k q^gamma b
template <int GM>
__device__ __forceinline__ float sig_loss(float x, bool hit, float kpos, float kneg, float gamma) {
  const SigTerm<GM> s(x, hit, gamma);
  const float k = hit ? kpos : kneg;
  return GM == 0 ? k * s.b : k * (s.qg * s.b);
}
// (t ? -1 : 1) k q^gamma (q + gamma (1 - q) b)
template <int GM>
__device__ __forceinline__ float sig_grad(float x, bool hit, float kpos, float kneg, float gamma) {
  const SigTerm<GM> s(x, hit, gamma);
  const float k = hit ? -kpos : kneg;
  if (GM == 0) return k * s.q;
  return k * (s.qg * fmaf(gamma * s.p, s.b, s.q));
}

constexpr int GPIX = 4;   // pixels per thread of the generic forward kernel: a workgroup owns 1024 consecutive pixels of one image

// Any H x W, any C <= 255.  A thread keeps the taps, the label and the weight of its GPIX pixels in registers and walks the classes once:
// the running arg-max (ce_fwd_kernel's comparison in its order) and the class's loss, one block reduction per class.
// grid: (ceil(H W / 1024), N)
template <int GM>
__global__ __launch_bounds__(256) void sig_fwd_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                      const unsigned char* __restrict__ label, const float* __restrict__ pw, int H, int W,
                                                      int ign, float sh, float sw, const float* __restrict__ coef, float gamma,
                                                      double* __restrict__ slab, long long* __restrict__ cnt) {
  __shared__ double sm[16];
  const int n = blockIdx.y, hw = h * w, HW = H * W;
  const float* lp = logits + (i64)n * C * hw;
  Bilin b[GPIX];
  int lab[GPIX], arg[GPIX];
  float wgt[GPIX], mx[GPIX];
  bool in[GPIX];
#pragma unroll
  for (int k = 0; k < GPIX; ++k) {
    const int p = blockIdx.x * (256 * GPIX) + k * 256 + threadIdx.x;
    in[k] = p < HW;
    const int q = in[k] ? p : 0;
    const int oy = q / W, ox = q - oy * W;
    b[k] = make_bilin(oy, ox, sh, sw, h, w);
    lab[k] = in[k] ? label[(i64)n * HW + p] : ign;
    wgt[k] = in[k] && pw ? pw[(i64)n * HW + p] : 1.f;
    mx[k] = -INFINITY;
    arg[k] = 0;
  }
  const i64 row = (i64)n * gridDim.x + blockIdx.x;
  for (int c = 0; c < C; ++c) {
    const float kpos = coef[2 * c], kneg = coef[2 * c + 1];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < GPIX; ++k) {
      if (in[k]) {
        const float x = interp(lp + (i64)c * hw, w, b[k]);
        if (x > mx[k]) { mx[k] = x; arg[k] = c; }
        if (lab[k] != ign && lab[k] < C && wgt[k] != 0.f) s += (double)(wgt[k] * sig_loss<GM>(x, lab[k] == c, kpos, kneg, gamma));
      }
    }
    s = block_sum_d(s, sm);
    if (threadIdx.x == 0) slab[row * C + c] = s;
  }
  double correct = 0.0, valid = 0.0, bad = 0.0;
#pragma unroll
  for (int k = 0; k < GPIX; ++k) {
    if (in[k]) {
      if (lab[k] != ign && lab[k] < C) {
        valid += 1.0;
        if (arg[k] == lab[k]) correct += 1.0;
      } else if (lab[k] != ign) {
        bad += 1.0;
      }
    }
  }
  correct = block_sum_d(correct, sm);
  valid = block_sum_d(valid, sm);
  bad = block_sum_d(bad, sm);
  if (threadIdx.x == 0) {
    cnt[row * 3] = (long long)correct;
    cnt[row * 3 + 1] = (long long)valid;
    cnt[row * 3 + 2] = (long long)bad;
  }
}

// The x4 / x8 cases (H == S h, W == S w, C <= 8) by inter-cell blocks, as ce_fwd_blocks_kernel: one thread per S x S block of
// full-resolution pixels that interpolate from the same four cells, whose 4 x C logits are loaded once.  Per pixel the interpolation and the
// arg-max are ce_fwd_blocks_kernel's (same coordinates, weights, class order).
// grid: (ceil((w + 1) / 16), ceil((h + 1) / (16 TILES)), N), 16 x 16 threads
template <int S, int TILES, int GM>
__global__ __launch_bounds__(256) void sig_fwd_blocks_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                             const unsigned char* __restrict__ label, const float* __restrict__ pw, int ign,
                                                             const float* __restrict__ coef, float gamma, double* __restrict__ slab,
                                                             long long* __restrict__ cnt) {
  __shared__ double smd[4][8];
  __shared__ int smi[4][4];
  const int n = blockIdx.z, H = S * h, W = S * w, hw = h * w;
  const int bx = blockIdx.x * 16 + (threadIdx.x & 15) - 1;
  const float* lp = logits + (i64)n * C * hw;
  const unsigned char* lab = label + (i64)n * H * W;
  const float* pwp = pw ? pw + (i64)n * H * W : nullptr;
  float kpos[8], kneg[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    kpos[c] = c < C ? coef[2 * c] : 0.f;
    kneg[c] = c < C ? coef[2 * c + 1] : 0.f;
  }
  double sum[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) sum[c] = 0.0;
  int correct = 0, valid = 0, bad = 0;
  for (int it = 0; it < TILES; ++it) {
    const int by = (blockIdx.y * TILES + it) * 16 + (threadIdx.x >> 4) - 1;
    if (bx > w - 1 || by > h - 1) continue;
    const int xl = max(bx, 0), xr = min(xl + 1, w - 1), yt = max(by, 0), yb = min(yt + 1, h - 1);
    float v[2][2][8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float* q = lp + (i64)(c < C ? c : 0) * hw;
      v[0][0][c] = q[yt * w + xl];
      v[0][1][c] = q[yt * w + xr];
      v[1][0][c] = q[yb * w + xl];
      v[1][1][c] = q[yb * w + xr];
    }
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
        float2 g2 = make_float2(1.f, 1.f);
        if (pwp) g2 = *reinterpret_cast<const float2*>(pwp + p);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int j = 2 * half + k;
          const int l = k ? (l2 >> 8) : (l2 & 255);
          const float wgt = k ? g2.y : g2.x;
          float mx = -INFINITY;
          int arg = 0;
          float zc[8];
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            zc[c] = c < C ? bilin_blend(v[0][0][c], v[0][1][c], v[1][0][c], v[1][1][c], lx0[j], lx1[j], ly0, ly1) : -INFINITY;
            if (c < C && zc[c] > mx) { mx = zc[c]; arg = c; }
          }
          if (l != ign && l < C) {
            valid += 1;
            if (arg == l) correct += 1;
            if (wgt != 0.f) {
#pragma unroll
              for (int c = 0; c < 8; ++c)
                if (c < C) sum[c] += (double)(wgt * sig_loss<GM>(zc[c], c == l, kpos[c], kneg[c], gamma));
            }
          } else if (l != ign) {
            bad += 1;
          }
        }
      }
    }
  }
  // one row of partials per workgroup: lanes by shuffles, the four waves through LDS in wave order
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (c < C) sum[c] = wave_sum_d(sum[c]);
  correct = wave_sum_i(correct);
  valid = wave_sum_i(valid);
  bad = wave_sum_i(bad);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 8; ++c) smd[wid][c] = sum[c];
    smi[wid][0] = correct;
    smi[wid][1] = valid;
    smi[wid][2] = bad;
  }
  __syncthreads();
  const i64 row = ((i64)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const int t = threadIdx.x;
  if (t < C) {
    slab[row * C + t] = ((smd[0][t] + smd[1][t]) + smd[2][t]) + smd[3][t];
  } else if (t >= 64 && t < 64 + 3) {
    const int j = t - 64;
    cnt[row * 3 + j] = (long long)smi[0][j] + smi[1][j] + smi[2][j] + smi[3][j];
  }
}

// One workgroup of 16 waves.  Phase 1: a wave per (n, c) adds that pair's `blocks` partials -- lane l takes rows l, l + 64, ... in order,
// then the shuffle tree: one fixed order (dice_finalize_kernel's scheme).  Phase 2: the pairs in index order, the loss and the accuracy.
__global__ __launch_bounds__(1024) void sig_finalize_kernel(const double* __restrict__ slab, const long long* __restrict__ cnt, int N, int C,
                                                            int blocks, double divisor, double loss_weight, double* __restrict__ sums,
                                                            float* __restrict__ out) {
  __shared__ double sm[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int NC = N * C;
  for (int pair = wid; pair < NC + 3; pair += 16) {
    double a = 0.0;
    if (pair < NC) {
      const int n = pair / C, c = pair - n * C;
      for (int k = lane; k < blocks; k += 64) a += slab[((i64)n * blocks + k) * C + c];
    } else {                                 // the three counts, over every row of every image (integers: exact in any order)
      const int j = pair - NC;
      for (i64 row = lane; row < (i64)N * blocks; row += 64) a += (double)cnt[row * 3 + j];
    }
    a = wave_sum_d(a);
    if (lane == 0) sums[pair] = a;
  }
  __syncthreads();
  double part = 0.0;
  for (int pair = threadIdx.x; pair < NC; pair += 1024) part += sums[pair];
  part = block_sum_d(part, sm);
  if (threadIdx.x == 0) {
    const double eps = 1.1920928955078125e-07;  // torch.finfo(float32).eps, as ce_finalize_kernel
    const double* tot = sums + NC;
    out[0] = (float)(loss_weight * (part / divisor));
    out[1] = (float)((tot[0] + eps) * (100.0 / (tot[1] + eps)));
    out[2] = (float)tot[2];
  }
}

// grid: (blocks over h*w, C, N).  One thread per low-resolution logit; gathers its full-res footprint (ce_bwd_kernel's gather).  The gradient
// is separable per class, so any C runs without a per-pixel work map.
template <int GM>
__global__ __launch_bounds__(256) void sig_bwd_kernel(const float* __restrict__ logits, int C, int h, int w, const unsigned char* __restrict__ label,
                                                      const float* __restrict__ pw, int H, int W, int ign, float sh, float sw,
                                                      const float* __restrict__ coef, float gamma, float scale, float* __restrict__ dlogits,
                                                      int accumulate) {
  const int c = blockIdx.y, n = blockIdx.z;
  const float* lp = logits + ((i64)n * C + c) * h * w;
  const unsigned char* lab = label + (i64)n * H * W;
  const float* pwp = pw ? pw + (i64)n * H * W : nullptr;
  const float kpos = coef[2 * c], kneg = coef[2 * c + 1];
  float* dp = dlogits + ((i64)n * C + c) * h * w;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < h * w; i += gridDim.x * blockDim.x) {
    const int iy = i / w, ix = i - iy * w;
    int oy_lo = (int)floorf(((float)iy - 0.5f) / sh - 0.5f) - 1, oy_hi = (int)ceilf(((float)iy + 1.5f) / sh - 0.5f) + 1;
    int ox_lo = (int)floorf(((float)ix - 0.5f) / sw - 0.5f) - 1, ox_hi = (int)ceilf(((float)ix + 1.5f) / sw - 0.5f) + 1;
    oy_lo = max(oy_lo, 0); oy_hi = min(oy_hi, H - 1);
    ox_lo = max(ox_lo, 0); ox_hi = min(ox_hi, W - 1);
    float acc = 0.f;
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
        if (l == ign || l >= C) continue;
        const float g = pwp ? pwp[p] : 1.f;
        if (g == 0.f) continue;
        acc = fmaf(wy * wx * g, sig_grad<GM>(interp(lp, w, b), l == c, kpos, kneg, gamma), acc);
      }
    }
    acc *= scale;
    dp[i] = accumulate ? dp[i] + acc : acc;
  }
}

// The same gather with ONE thread per low-resolution cell for all classes (C <= 8), as ce_bwd_cells_kernel: the per-pixel work that does not
// depend on the class is done once.                                                                        grid: (blocks over h*w, 1, N)
template <int GM>
__global__ __launch_bounds__(256) void sig_bwd_cells_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                            const unsigned char* __restrict__ label, const float* __restrict__ pw, int H, int W,
                                                            int ign, float sh, float sw, const float* __restrict__ coef, float gamma,
                                                            float scale, float* __restrict__ dlogits, int accumulate) {
  const int n = blockIdx.z;
  const int hw = h * w;
  const float* lp = logits + (i64)n * C * hw;
  const unsigned char* lab = label + (i64)n * H * W;
  const float* pwp = pw ? pw + (i64)n * H * W : nullptr;
  float* dp = dlogits + (i64)n * C * hw;
  float kpos[8], kneg[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    kpos[c] = c < C ? coef[2 * c] : 0.f;
    kneg[c] = c < C ? coef[2 * c + 1] : 0.f;
  }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += gridDim.x * blockDim.x) {
    const int iy = i / w, ix = i - iy * w;
    int oy_lo = (int)floorf(((float)iy - 0.5f) / sh - 0.5f) - 1, oy_hi = (int)ceilf(((float)iy + 1.5f) / sh - 0.5f) + 1;
    int ox_lo = (int)floorf(((float)ix - 0.5f) / sw - 0.5f) - 1, ox_hi = (int)ceilf(((float)ix + 1.5f) / sw - 0.5f) + 1;
    oy_lo = max(oy_lo, 0); oy_hi = min(oy_hi, H - 1);
    ox_lo = max(ox_lo, 0); ox_hi = min(ox_hi, W - 1);
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.f;
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
        if (l == ign || l >= C) continue;
        const float g = pwp ? pwp[p] : 1.f;
        if (g == 0.f) continue;
        const float wg = wy * wx * g;
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c < C) acc[c] = fmaf(wg, sig_grad<GM>(interp(lp + (i64)c * hw, w, b), l == c, kpos[c], kneg[c], gamma), acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {
        const float a = acc[c] * scale;
        dp[(i64)c * hw + i] = accumulate ? dp[(i64)c * hw + i] + a : a;
      }
    }
  }
}

// The x4 / x8 cases by inter-cell blocks, ce_bwd_blocks_kernel's scheme: one thread loads the 4 x C corner logits of its S x S block once,
// evaluates each pixel's C terms once and keeps the 4 x C corner sums in registers; the corner sums of a 16 x 16 tile of blocks meet in LDS
// in four conflict-free phases and the 15 x 15 cells whose four blocks lie inside the workgroup are written out.
// grid: (ceil(w / 15), ceil(h / 15), N)
template <int S, int GM>
__global__ __launch_bounds__(256) void sig_bwd_blocks_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                             const unsigned char* __restrict__ label, const float* __restrict__ pw, int ign,
                                                             const float* __restrict__ coef, float gamma, float scale,
                                                             float* __restrict__ dlogits, int accumulate) {
  constexpr int TB = 16, OWN = TB - 1;
  __shared__ float cell[8][TB + 1][TB + 1];
  const int n = blockIdx.z, H = S * h, W = S * w, hw = h * w;
  const int tx = threadIdx.x & (TB - 1), ty = threadIdx.x >> 4;
  const int cx0 = blockIdx.x * OWN, cy0 = blockIdx.y * OWN;        // first cell this workgroup owns
  const int bx = cx0 - 1 + tx, by = cy0 - 1 + ty;                  // this thread's block: taps (b, b + 1), clamped at the borders
  const float* lp = logits + (i64)n * C * hw;
  const unsigned char* lab = label + (i64)n * H * W;
  const float* pwp = pw ? pw + (i64)n * H * W : nullptr;
  for (int i = threadIdx.x; i < 8 * (TB + 1) * (TB + 1); i += 256) (&cell[0][0][0])[i] = 0.f;
  float kpos[8], kneg[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    kpos[c] = c < C ? coef[2 * c] : 0.f;
    kneg[c] = c < C ? coef[2 * c + 1] : 0.f;
  }
  float acc[2][2][8];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[a][b][c] = 0.f;
  if (bx <= w - 1 && by <= h - 1) {
    const int xl = max(bx, 0), xr = min(xl + 1, w - 1), yt = max(by, 0), yb = min(yt + 1, h - 1);
    float v[2][2][8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float* q = lp + (i64)(c < C ? c : 0) * hw;
      v[0][0][c] = q[yt * w + xl];
      v[0][1][c] = q[yt * w + xr];
      v[1][0][c] = q[yb * w + xl];
      v[1][1][c] = q[yb * w + xr];
    }
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
        float2 g2 = make_float2(1.f, 1.f);
        if (pwp) g2 = *reinterpret_cast<const float2*>(pwp + p);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int j = 2 * half + k;
          const int l = k ? (l2 >> 8) : (l2 & 255);
          const float g = k ? g2.y : g2.x;
          if (l == ign || l >= C || g == 0.f) continue;
          const float wtl = wyt * wxl[j] * g, wtr = wyt * wxr[j] * g, wbl = wyb * wxl[j] * g, wbr = wyb * wxr[j] * g;
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            if (c < C) {
              const float z = bilin_blend(v[0][0][c], v[0][1][c], v[1][0][c], v[1][1][c], lx0[j], lx1[j], ly0, ly1);
              const float d = sig_grad<GM>(z, l == c, kpos[c], kneg[c], gamma);
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
  float* dp = dlogits + (i64)n * C * hw;
  for (int i = threadIdx.x; i < OWN * OWN; i += 256) {
    const int u = i / OWN, q = i - u * OWN;
    const int gy = cy0 + u, gx = cx0 + q;
    if (gy >= h || gx >= w) continue;
    for (int c = 0; c < C; ++c) {
      const float a = cell[c][u + 1][q + 1] * scale;
      float* o = dp + (i64)c * hw + gy * w + gx;
      *o = accumulate ? *o + a : a;
    }
  }
}

// form: 0 = the generic kernels, 4 / 8 = the inter-cell block kernels of that ratio (the caller chooses, the library checks)
inline bool form_ok(int form, int C, int h, int w, int H, int W, const void* pw, const void* label) {
  if (form == 0) return true;
  return (form == 4 || form == 8) && C <= 8 && H == form * h && W == form * w && ((uintptr_t)pw & 7) == 0 && ((uintptr_t)label & 1) == 0 &&
         h < 65535 * 15;
}
inline bool shape_ok(int N, int C, int h, int w, int H, int W) {
  return N > 0 && N <= 65535 && C > 0 && C <= 255 && h > 0 && w > 0 && H > 0 && W > 0 && (i64)H * W < INT_MAX - 2048 && (i64)h * w < INT_MAX - 2048;
}
inline int gamma_mode(float gamma) { return gamma == 0.f ? 0 : gamma == 2.f ? 2 : 1; }

}  // namespace

#define PFST_SIG_GM(gm, LAUNCH) \
  do {                          \
    if ((gm) == 0) LAUNCH(0);   \
    else if ((gm) == 2) LAUNCH(2); \
    else LAUNCH(1);             \
  } while (0)

extern "C" int pfst_sigloss_upsample_fwd(const float* logits, int N, int C, int h, int w, const unsigned char* label, const float* pix_weight,
                                         int H, int W, int ignore_index, const float* coef, float gamma, int form, double* slab,
                                         long long* counts, int blocks, pfst_stream_t stream) {
  PFST_CHECK_ARG(logits && label && coef && slab && counts && shape_ok(N, C, h, w, H, W));
  PFST_CHECK_ARG(gamma >= 0.f && form_ok(form, C, h, w, H, W, pix_weight, label));
  hipStream_t s = (hipStream_t)stream;
  const int gm = gamma_mode(gamma);
  if (form == 0) {
    const int gx = cdiv((i64)H * W, 256 * GPIX);
    PFST_CHECK_ARG(blocks == gx);
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
#define PFST_SIG_FWD(GM)                                                                                                                  \
  hipLaunchKernelGGL(sig_fwd_kernel<GM>, dim3(gx, N), dim3(256), 0, s, logits, C, h, w, label, pix_weight, H, W, ignore_index, sh, sw, coef, \
                     gamma, slab, counts)
    PFST_SIG_GM(gm, PFST_SIG_FWD);
#undef PFST_SIG_FWD
  } else {
    // tiles per workgroup as pfst_ce_upsample_fwd: two at x4, one at x8 (64 pixels per thread)
    const int gx = cdiv(w + 1, 16), gy = cdiv(h + 1, form == 4 ? 32 : 16);
    PFST_CHECK_ARG(blocks == gx * gy);
    const dim3 grid(gx, gy, N);
#define PFST_SIG_FWD4(GM)                                                                                                              \
  hipLaunchKernelGGL((sig_fwd_blocks_kernel<4, 2, GM>), grid, dim3(256), 0, s, logits, C, h, w, label, pix_weight, ignore_index, coef, gamma, \
                     slab, counts)
#define PFST_SIG_FWD8(GM)                                                                                                              \
  hipLaunchKernelGGL((sig_fwd_blocks_kernel<8, 1, GM>), grid, dim3(256), 0, s, logits, C, h, w, label, pix_weight, ignore_index, coef, gamma, \
                     slab, counts)
    if (form == 4) PFST_SIG_GM(gm, PFST_SIG_FWD4);
    else PFST_SIG_GM(gm, PFST_SIG_FWD8);
#undef PFST_SIG_FWD4
#undef PFST_SIG_FWD8
  }
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_sigloss_finalize(const double* slab, const long long* counts, int N, int C, int blocks, double divisor, double loss_weight,
                                     double* sums, float* out, pfst_stream_t stream) {
  PFST_CHECK_ARG(slab && counts && sums && out && N > 0 && N <= 65535 && C > 0 && C <= 255 && blocks > 0 && divisor > 0.0);
  hipLaunchKernelGGL(sig_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, slab, counts, N, C, blocks, divisor, loss_weight, sums,
                     out);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_sigloss_upsample_bwd(const float* logits, int N, int C, int h, int w, const unsigned char* label, const float* pix_weight,
                                         int H, int W, int ignore_index, const float* coef, float gamma, int form, float scale, float* dlogits,
                                         int accumulate, pfst_stream_t stream) {
  PFST_CHECK_ARG(logits && label && coef && dlogits && shape_ok(N, C, h, w, H, W));
  PFST_CHECK_ARG(gamma >= 0.f && form_ok(form, C, h, w, H, W, pix_weight, label));
  hipStream_t s = (hipStream_t)stream;
  const int gm = gamma_mode(gamma);
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  const int gx = cdiv((i64)h * w, 256);
  if (form != 0) {
    const dim3 grid(cdiv(w, 15), cdiv(h, 15), N);
#define PFST_SIG_BWD4(GM)                                                                                                                 \
  hipLaunchKernelGGL((sig_bwd_blocks_kernel<4, GM>), grid, dim3(256), 0, s, logits, C, h, w, label, pix_weight, ignore_index, coef, gamma, scale, \
                     dlogits, accumulate)
#define PFST_SIG_BWD8(GM)                                                                                                                 \
  hipLaunchKernelGGL((sig_bwd_blocks_kernel<8, GM>), grid, dim3(256), 0, s, logits, C, h, w, label, pix_weight, ignore_index, coef, gamma, scale, \
                     dlogits, accumulate)
    if (form == 4) PFST_SIG_GM(gm, PFST_SIG_BWD4);
    else PFST_SIG_GM(gm, PFST_SIG_BWD8);
#undef PFST_SIG_BWD4
#undef PFST_SIG_BWD8
  } else if (C <= 8) {
#define PFST_SIG_BWDC(GM)                                                                                                                   \
  hipLaunchKernelGGL(sig_bwd_cells_kernel<GM>, dim3(gx, 1, N), dim3(256), 0, s, logits, C, h, w, label, pix_weight, H, W, ignore_index, sh, sw, \
                     coef, gamma, scale, dlogits, accumulate)
    PFST_SIG_GM(gm, PFST_SIG_BWDC);
#undef PFST_SIG_BWDC
  } else {
#define PFST_SIG_BWDG(GM)                                                                                                                \
  hipLaunchKernelGGL(sig_bwd_kernel<GM>, dim3(gx, C, N), dim3(256), 0, s, logits, C, h, w, label, pix_weight, H, W, ignore_index, sh, sw, coef, \
                     gamma, scale, dlogits, accumulate)
    PFST_SIG_GM(gm, PFST_SIG_BWDG);
#undef PFST_SIG_BWDG
  }
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
