// Fused bilinear-upsample + softmax + Dice loss (+ accuracy), forward and backward.
// As in loss.hip the full-resolution logits are never materialised: every full-resolution pixel interpolates its C logits from the
// low-resolution map in registers, with the helpers and the class order of the CE kernels, so p = exp(z - lse) has the CE path's bits and
// a Dice term that follows a CE term reads that term's log-sum-exp instead of forming its own.
// Reference: rsiseg/models/losses/dice_loss.py (the closed form is in DESIGN.md section 8h), decode_heads/decode_head.py:249-283.
//
//   I[n,c] = sum_px valid * t_c * p_c     P[n,c] = sum_px p_c^e (every pixel)     T[n,c] = sum_px t_c (every pixel)
//   t = one_hot(min(label, C - 1)), valid = label != the LOSS's ignore_index
//
// I and P feed the gradient, so their summation order is fixed in every mode: a workgroup reduces by wave shuffles and LDS and STORES one
// row of partials (fp64 I, P; integer T and accuracy counts); pfst_dice_finalize adds the rows in a fixed order.  No atomics anywhere.
#include <limits.h>
#include <algorithm>
#include "common.h"
#include "upsample_walk.h"
#include "../../include/pfst_hip.h"

namespace {

// three block-wide sums at once; results valid in thread 0.  smem: 12 doubles.
__device__ __forceinline__ void block_sum3_d(double& a, double& b, double& c, double* smem) {
  a = wave_sum_d(a);
  b = wave_sum_d(b);
  c = wave_sum_d(c);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) { smem[wid] = a; smem[4 + wid] = b; smem[8 + wid] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = ((smem[0] + smem[1]) + smem[2]) + smem[3];
    b = ((smem[4] + smem[5]) + smem[6]) + smem[7];
    c = ((smem[8] + smem[9]) + smem[10]) + smem[11];
  }
}

// p^q for p = exp(x) as exp(q x): ONE exponential where powf costs a logarithm, an exponential and their range reductions (about ten times
// the instructions; the e = 3 kernels ran at 3.3 - 4.5 times their CE counterparts with it, profiles/dice_loss.txt).  The rounding error of the
// product q x would enter the result relatively, so it is carried along: q x = t + r exactly (r from one fma), exp(t + r) = exp(t) (1 + r).
__device__ __forceinline__ float exp_scaled(float x, float q) {
  const float t = q * x, r = fmaf(q, x, -t), v = expf(t);
  return fmaf(v, r, v);
}
// p = exp(x), x = z - lse
template <bool E2>
__device__ __forceinline__ float pow_e(float p, float x, float e) { return E2 ? p * p : exp_scaled(x, e); }          // p^e
template <bool E2>
__device__ __forceinline__ float pow_e1(float p, float x, float e1) { return E2 ? p : exp_scaled(x, e1); }           // p^(e-1), e1 = e - 1 >= 0
// dL/dp_c up to the common scale: -a * valid * t_c + b * p_c^(e-1)    (a, b: pfst_dice_finalize's table)
template <bool E2>
__device__ __forceinline__ float dice_g(float p, float x, float a, float b, bool hit, float e1) {
  return fmaf(b, pow_e1<E2>(p, x, e1), hit ? -a : 0.f);
}

constexpr int GPIX = 4;   // pixels per thread of the generic forward kernel: a workgroup owns 1024 consecutive pixels of one image

// Any H x W, any C <= 255.  A thread keeps the taps, the label and the log-sum-exp of its GPIX pixels in registers; the classes are walked
// twice for the log-sum-exp (maximum / arg-max, then the sum: ce_fwd_kernel's arithmetic in ce_fwd_kernel's order, bit-identical lse) and
// once more for the sums, one block reduction per class.                                      grid: (ceil(H W / 1024), N)
template <bool E2>
__global__ __launch_bounds__(256) void dice_fwd_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                       const unsigned char* __restrict__ label, int H, int W, int ign, int hign, float sh,
                                                       float sw, float expo, const float* __restrict__ lse_in, float* __restrict__ lse_out,
                                                       double* __restrict__ slab, long long* __restrict__ cnt) {
  __shared__ double sm[12];
  const int n = blockIdx.y, hw = h * w, HW = H * W;
  const float* lp = logits + (i64)n * C * hw;
  Bilin b[GPIX];
  float ls[GPIX];
  int lab[GPIX];
  bool in[GPIX];
  double correct = 0.0, valid = 0.0, bad = 0.0;
#pragma unroll
  for (int k = 0; k < GPIX; ++k) {
    const int p = blockIdx.x * (256 * GPIX) + k * 256 + threadIdx.x;
    in[k] = p < HW;
    const int q = in[k] ? p : 0;
    const int oy = q / W, ox = q - oy * W;
    b[k] = make_bilin(oy, ox, sh, sw, h, w);
    lab[k] = 0;
    ls[k] = 0.f;
    if (in[k]) {
      const int l = lab[k] = label[(i64)n * HW + p];
      float mx = -INFINITY;
      int arg = 0;
      for (int c = 0; c < C; ++c) {
        const float z = interp(lp + (i64)c * hw, w, b[k]);
        if (z > mx) { mx = z; arg = c; }
      }
      if (lse_in) {
        ls[k] = lse_in[(i64)n * HW + p];
      } else {
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(interp(lp + (i64)c * hw, w, b[k]) - mx);
        ls[k] = mx + logf(se);
        lse_out[(i64)n * HW + p] = ls[k];
      }
      // the head's accuracy and label check, as ce_fwd_kernel counts them (hign: the HEAD's ignore_index)
      if (l != hign && l < C) {
        valid += 1.0;
        if (arg == l) correct += 1.0;
      } else if (l != hign && l != ign) {
        bad += 1.0;
      }
    }
  }
  const i64 row = (i64)n * gridDim.x + blockIdx.x;
  for (int c = 0; c < C; ++c) {
    double I = 0.0, P = 0.0, T = 0.0;
#pragma unroll
    for (int k = 0; k < GPIX; ++k) {
      if (in[k]) {
        const float x = interp(lp + (i64)c * hw, w, b[k]) - ls[k], p = expf(x);
        if (min(lab[k], C - 1) == c) {
          T += 1.0;
          if (lab[k] != ign) I += (double)p;
        }
        P += (double)pow_e<E2>(p, x, expo);
      }
    }
    block_sum3_d(I, P, T, sm);
    if (threadIdx.x == 0) {
      slab[(row * C + c) * 2] = I;
      slab[(row * C + c) * 2 + 1] = P;
      cnt[row * (C + 3) + c] = (long long)T;
    }
  }
  block_sum3_d(correct, valid, bad, sm);
  if (threadIdx.x == 0) {
    cnt[row * (C + 3) + C] = (long long)correct;
    cnt[row * (C + 3) + C + 1] = (long long)valid;
    cnt[row * (C + 3) + C + 2] = (long long)bad;
  }
}

// What the Dice forward does with a pixel of fwd_blocks_walk (upsample_walk.h): the log-sum-exp, read or formed -- with ce_fwd_kernel's
// arithmetic on the frame's logits, so the same bits either way -- and stored in pairs, the pixel's terms of I, P, T and the head's accuracy
// counts.  The sums are the kernel's own arrays: a functor that is indexed by a loop variable would stay in memory until that loop is unrolled.
template <bool E2>
struct DiceFwdPx {
  const float* __restrict__ li;
  float* __restrict__ ls;
  int C, ign, hign;
  float expo;
  double (&I)[8], (&P)[8];
  int (&T)[8];
  int correct, valid, bad;
  float2 e2, lo;
  __device__ __forceinline__ void pair(i64 p) {
    e2 = make_float2(0.f, 0.f);
    if (li) e2 = *reinterpret_cast<const float2*>(li + p);
  }
  __device__ __forceinline__ void pixel(int k, int l, const float (&zc)[8], float mx, int arg) {
    float e = k ? e2.y : e2.x;
    if (!li) {
      float se = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (c < C) se += expf(zc[c] - mx);
      e = mx + logf(se);
    }
    lo.x = k ? lo.x : e;
    lo.y = k ? e : lo.y;
    const int tl = min(l, C - 1);
    const bool ok = l != ign;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {
        const float x = zc[c] - e, pc = expf(x);
        const bool hit = c == tl;
        T[c] += hit ? 1 : 0;
        I[c] += (double)(hit && ok ? pc : 0.f);
        P[c] += (double)pow_e<E2>(pc, x, expo);
      }
    }
    // the head's accuracy and label check, as ce_fwd_kernel counts them (hign: the HEAD's ignore_index); on copies that are stored back
    // unconditionally, since updates of the members under the branches would be merged into one store through a selected address
    int co = correct, va = valid, ba = bad;
    if (l != hign && l < C) {
      va += 1;
      if (arg == l) co += 1;
    } else if (l != hign && l != ign) {
      ba += 1;
    }
    correct = co; valid = va; bad = ba;
  }
  __device__ __forceinline__ void pair_end(i64 p) {
    if (ls) *reinterpret_cast<float2*>(ls + p) = lo;
  }
};

// The x4 / x8 cases (H == S h, W == S w, C <= 8) by inter-cell blocks.
// grid: (ceil((w + 1) / 16), ceil((h + 1) / (16 TILES)), N), 16 x 16 threads
template <int S, int TILES, bool E2>
__global__ __launch_bounds__(256) void dice_fwd_blocks_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                              const unsigned char* __restrict__ label, int ign, int hign, float expo,
                                                              const float* __restrict__ lse_in, float* __restrict__ lse_out,
                                                              double* __restrict__ slab, long long* __restrict__ cnt) {
  __shared__ double smd[4][16];
  __shared__ int smi[4][12];
  const i64 n = blockIdx.z, HW = (i64)S * h * S * w;
  double I[8], P[8];
  int T[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) { I[c] = 0.0; P[c] = 0.0; T[c] = 0; }
  DiceFwdPx<E2> px{lse_in ? lse_in + n * HW : nullptr, lse_in ? nullptr : lse_out + n * HW, C, ign, hign, expo, I, P, T, 0, 0, 0};
  fwd_blocks_walk<S, TILES>(logits + n * C * h * w, C, h, w, label + n * HW, px);
  int correct = px.correct, valid = px.valid, bad = px.bad;
  // one row of partials per workgroup: lanes by shuffles, the four waves through LDS in wave order
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    if (c < C) {
      I[c] = wave_sum_d(I[c]);
      P[c] = wave_sum_d(P[c]);
      T[c] = wave_sum_i(T[c]);
    }
  }
  correct = wave_sum_i(correct);
  valid = wave_sum_i(valid);
  bad = wave_sum_i(bad);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      smd[wid][2 * c] = I[c];
      smd[wid][2 * c + 1] = P[c];
      smi[wid][c] = T[c];
    }
    smi[wid][8] = correct;
    smi[wid][9] = valid;
    smi[wid][10] = bad;
  }
  __syncthreads();
  const i64 row = ((i64)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const int t = threadIdx.x;
  if (t < 2 * C) {
    slab[row * (2 * C) + t] = ((smd[0][t] + smd[1][t]) + smd[2][t]) + smd[3][t];
  } else if (t >= 64 && t < 64 + C + 3) {
    const int j = t - 64, src = j < C ? j : 8 + (j - C);
    cnt[row * (C + 3) + j] = (long long)smi[0][src] + smi[1][src] + smi[2][src] + smi[3][src];
  }
}

// One workgroup of 16 waves.  Phase 1: a wave per (n, c) adds that pair's `blocks` partials -- lane l takes rows l, l + 64, ... in order,
// then the shuffle tree: one fixed order.  Phase 2: the coefficient table and the loss.
__global__ __launch_bounds__(1024) void dice_finalize_kernel(const double* __restrict__ slab, const long long* __restrict__ cnt, int N, int C,
                                                             int blocks, const float* __restrict__ cw, int ign, double smooth, double expo,
                                                             double loss_weight, double* __restrict__ sums, float* __restrict__ coef,
                                                             float* __restrict__ out) {
  __shared__ double sm[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int NC = N * C;
  for (int pair = wid; pair < NC + 3; pair += 16) {
    double a = 0.0, b = 0.0, c3 = 0.0;
    if (pair < NC) {
      const int n = pair / C, c = pair - n * C;
      for (int k = lane; k < blocks; k += 64) {
        const i64 row = (i64)n * blocks + k;
        a += slab[(row * C + c) * 2];
        b += slab[(row * C + c) * 2 + 1];
        c3 += (double)cnt[row * (C + 3) + c];
      }
    } else {                                 // the three accuracy counts, over every row of every image (integers: exact in any order)
      const int j = pair - NC;
      for (i64 row = lane; row < (i64)N * blocks; row += 64) a += (double)cnt[row * (C + 3) + C + j];
    }
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    c3 = wave_sum_d(c3);
    if (lane == 0) {
      if (pair < NC) {
        sums[(i64)pair * 3] = a;
        sums[(i64)pair * 3 + 1] = b;
        sums[(i64)pair * 3 + 2] = c3;
      } else {
        sums[(i64)NC * 3 + (pair - NC)] = a;
      }
    }
  }
  __syncthreads();
  double part = 0.0;
  for (int pair = threadIdx.x; pair < NC; pair += 1024) {
    const int n = pair / C, c = pair - n * C;
    float fa = 0.f, fb = 0.f;
    if (c != ign) {
      const double w = cw ? (double)cw[c] : 1.0;
      const double num = 2.0 * sums[(i64)pair * 3] + smooth;
      const double den = sums[(i64)pair * 3 + 1] + sums[(i64)pair * 3 + 2] + smooth;
      const double k = w / ((double)C * (double)N);
      fa = (float)(k * 2.0 / den);
      fb = (float)(k * expo * num / (den * den));
      part += w * (1.0 - num / den) / (double)N;
    }
    coef[(i64)pair * 2] = fa;
    coef[(i64)pair * 2 + 1] = fb;
  }
  part = block_sum_d(part, sm);
  if (threadIdx.x == 0) {
    const double eps = 1.1920928955078125e-07;  // torch.finfo(float32).eps, as ce_finalize_kernel
    const double* tot = sums + (i64)NC * 3;
    out[0] = (float)(loss_weight * (part / (double)C));
    out[1] = (float)((tot[0] + eps) * (100.0 / (tot[1] + eps)));
    out[2] = (float)tot[2];
  }
}

// C > 8: s[p] = sum_k g_k p_k of every full-resolution pixel, so that the per-class gather below is O(C) per pixel.  grid: (blocks, N)
template <bool E2>
__global__ __launch_bounds__(256) void dice_s_kernel(const float* __restrict__ logits, int C, int h, int w, const unsigned char* __restrict__ label,
                                                     int H, int W, int ign, float sh, float sw, float e1, const float* __restrict__ lse,
                                                     const float* __restrict__ coef, float* __restrict__ s_out) {
  const int n = blockIdx.y, hw = h * w;
  const float* lp = logits + (i64)n * C * hw;
  const float* cf = coef + (i64)n * C * 2;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < H * W; p += gridDim.x * blockDim.x) {
    const int oy = p / W, ox = p - oy * W;
    const Bilin b = make_bilin(oy, ox, sh, sw, h, w);
    const int l = label[(i64)n * H * W + p];
    const int tl = min(l, C - 1);
    const bool ok = l != ign;
    const float lsp = lse[(i64)n * H * W + p];
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
      const float x = interp(lp + (i64)c * hw, w, b) - lsp, pc = expf(x);
      s = fmaf(dice_g<E2>(pc, x, cf[2 * c], cf[2 * c + 1], ok && c == tl, e1), pc, s);
    }
    s_out[(i64)n * H * W + p] = s;
  }
}

// The Dice gradient's term of one class for bwd_class_gather (upsample_walk.h): p_c (g_c - s) with s = sum_k g_k p_k from dice_s_kernel.
// No pixel is skipped (an ignored pixel still carries the b p^(e-1) term) and the tap weights have no multiplier.
template <bool E2>
struct DiceClassPx {
  const float* __restrict__ ls;
  const float* __restrict__ sp;
  int C, ign, c;
  float e1, ca, cb;
  float d;
  __device__ __forceinline__ bool cell_skip(int, int) const { return false; }
  template <class Z>
  __device__ __forceinline__ float cell_weight(int p, int l, const Z& z) {
    const float x = z(0) - ls[p], pc = expf(x);
    d = pc * (dice_g<E2>(pc, x, ca, cb, l != ign && min(l, C - 1) == c, e1) - sp[p]);
    return 1.f;
  }
  template <class Z>
  __device__ __forceinline__ float term(int, const Z&) const { return d; }
};

// grid: (blocks over h*w, C, N).  One thread per low-resolution logit; gathers its full-res footprint.
template <bool E2>
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* __restrict__ logits, int C, int h, int w, const unsigned char* __restrict__ label,
                                                       int H, int W, int ign, float sh, float sw, float e1, const float* __restrict__ lse,
                                                       const float* __restrict__ coef, const float* __restrict__ s_in, float scale,
                                                       float* __restrict__ dlogits, int accumulate) {
  const int c = blockIdx.y;
  const i64 n = blockIdx.z, HW = (i64)H * W, nc = n * C + c, plane = nc * h * w;
  DiceClassPx<E2> px{lse + n * HW, s_in + n * HW, C, ign, c, e1, coef[nc * 2], coef[nc * 2 + 1]};
  bwd_class_gather(logits + plane, h, w, label + n * HW, H, W, sh, sw, scale, dlogits + plane, accumulate, px);
}

// The Dice gradient's terms of all classes (C <= 8) for bwd_blocks_walk and bwd_cells_gather: a pixel's soft-max, its g and
// s = sum_k g_k p_k are formed once, in registers (the kernel's own arrays, as in DiceFwdPx); the term of class c is p_c (g_c - s).
// No pixel is skipped and the tap weights have no multiplier.
template <bool E2>
struct DiceBwdPx {
  const float* __restrict__ ls;
  int C, ign;
  float e1;
  const float (&ca)[8], (&cb)[8];
  float (&pc)[8], (&g)[8];
  float2 ls2;
  float s;
  __device__ __forceinline__ void pair(i64 p) { ls2 = *reinterpret_cast<const float2*>(ls + p); }
  template <class Z>
  __device__ __forceinline__ void softmax(int l, float lsp, const Z& z) {
    const int tl = min(l, C - 1);
    const bool ok = l != ign;
    s = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {               // pc, g beyond C stay unset: term() is asked for c < C only
        const float x = z(c) - lsp;
        pc[c] = expf(x);
        g[c] = dice_g<E2>(pc[c], x, ca[c], cb[c], ok && c == tl, e1);
        s = fmaf(g[c], pc[c], s);
      }
    }
  }
  __device__ __forceinline__ bool skip(int, int) const { return false; }
  __device__ __forceinline__ bool cell_skip(int, int) const { return false; }
  template <class Z>
  __device__ __forceinline__ float weight(int k, int l, const Z& z) {
    softmax(l, k ? ls2.y : ls2.x, z);
    return 1.f;
  }
  template <class Z>
  __device__ __forceinline__ float cell_weight(int p, int l, const Z& z) {
    softmax(l, ls[p], z);
    return 1.f;
  }
  template <class Z>
  __device__ __forceinline__ float term(int c, const Z&) const { return pc[c] * (g[c] - s); }
};
// an image's (a, b) of pfst_dice_finalize's table, by class
__device__ __forceinline__ void dice_coef(const float* __restrict__ coef, i64 n, int C, float (&ca)[8], float (&cb)[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    ca[c] = c < C ? coef[(n * C + c) * 2] : 0.f;
    cb[c] = c < C ? coef[(n * C + c) * 2 + 1] : 0.f;
  }
}

// ONE thread per low-resolution cell for all classes (C <= 8).                                          grid: (blocks over h*w, 1, N)
template <bool E2>
__global__ __launch_bounds__(256) void dice_bwd_cells_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                             const unsigned char* __restrict__ label, int H, int W, int ign, float sh, float sw,
                                                             float e1, const float* __restrict__ lse, const float* __restrict__ coef,
                                                             float scale, float* __restrict__ dlogits, int accumulate) {
  const i64 n = blockIdx.z, HW = (i64)H * W, img = n * C * h * w;
  float ca[8], cb[8], pc[8], g[8];
  dice_coef(coef, n, C, ca, cb);
  DiceBwdPx<E2> px{lse + n * HW, C, ign, e1, ca, cb, pc, g};
  bwd_cells_gather(logits + img, C, h, w, label + n * HW, H, W, sh, sw, scale, dlogits + img, accumulate, px);
}

// The x4 / x8 cases by inter-cell blocks.                                                        grid: (ceil(w / 15), ceil(h / 15), N)
template <int S, bool E2>
__global__ __launch_bounds__(256) void dice_bwd_blocks_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                              const unsigned char* __restrict__ label, int ign, float e1,
                                                              const float* __restrict__ lse, const float* __restrict__ coef, float scale,
                                                              float* __restrict__ dlogits, int accumulate) {
  const i64 n = blockIdx.z, HW = (i64)S * h * S * w, img = n * C * h * w;
  float ca[8], cb[8], pc[8], g[8];
  dice_coef(coef, n, C, ca, cb);
  DiceBwdPx<E2> px{lse + n * HW, C, ign, e1, ca, cb, pc, g};
  bwd_blocks_walk<S>(logits + img, C, h, w, label + n * HW, scale, dlogits + img, accumulate, px);
}

}  // namespace

extern "C" int pfst_dice_upsample_fwd(const float* logits, int N, int C, int h, int w, const unsigned char* label, int H, int W,
                                      int ignore_index, int head_ignore_index, float exponent, int form, const float* lse_in, float* lse_out,
                                      double* slab, long long* counts, int blocks, pfst_stream_t stream) {
  PFST_CHECK_ARG(logits && label && slab && counts && N > 0 && C > 0 && C <= 255 && h > 0 && w > 0 && H > 0 && W > 0 && N <= 65535);
  PFST_CHECK_ARG((lse_in != nullptr) != (lse_out != nullptr) && exponent >= 1.f && (i64)H * W < INT_MAX - 2048);
  const void* lse = lse_in ? (const void*)lse_in : (const void*)lse_out;
  PFST_CHECK_ARG(form == 0 || blocks_form_ok(form, C, h, w, H, W, label, (uintptr_t)lse));
  hipStream_t s = (hipStream_t)stream;
  const bool e2 = exponent == 2.f;
  if (form == 0) {
    const int gx = cdiv((i64)H * W, 256 * GPIX);
    PFST_CHECK_ARG(blocks == gx);
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    if (e2)
      hipLaunchKernelGGL(dice_fwd_kernel<true>, dim3(gx, N), dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, head_ignore_index, sh,
                         sw, exponent, lse_in, lse_out, slab, counts);
    else
      hipLaunchKernelGGL(dice_fwd_kernel<false>, dim3(gx, N), dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, head_ignore_index, sh,
                         sw, exponent, lse_in, lse_out, slab, counts);
  } else {
    const dim3 grid = fwd_blocks_grid(form, h, w, N);
    PFST_CHECK_ARG(blocks == (int)(grid.x * grid.y));
#define PFST_DICE_FWD(S, TILES, E2)                                                                                                         \
  hipLaunchKernelGGL((dice_fwd_blocks_kernel<S, TILES, E2>), grid, dim3(256), 0, s, logits, C, h, w, label, ignore_index, head_ignore_index, \
                     exponent, lse_in, lse_out, slab, counts)
    if (form == 4 && e2) PFST_DICE_FWD(4, 2, true);
    else if (form == 4) PFST_DICE_FWD(4, 2, false);
    else if (e2) PFST_DICE_FWD(8, 1, true);
    else PFST_DICE_FWD(8, 1, false);
#undef PFST_DICE_FWD
  }
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_dice_finalize(const double* slab, const long long* counts, int N, int C, int blocks, const float* class_weight,
                                  int ignore_index, double smooth, double exponent, double loss_weight, double* sums, float* coef, float* out,
                                  pfst_stream_t stream) {
  PFST_CHECK_ARG(slab && counts && sums && coef && out && N > 0 && N <= 65535 && C > 0 && C <= 255 && blocks > 0 && exponent >= 1.0);
  hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, slab, counts, N, C, blocks, class_weight, ignore_index,
                     smooth, exponent, loss_weight, sums, coef, out);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_dice_upsample_bwd(const float* logits, int N, int C, int h, int w, const unsigned char* label, int H, int W,
                                      int ignore_index, float exponent, int form, const float* lse, const float* coef, float scale,
                                      float* work, float* dlogits, int accumulate, pfst_stream_t stream) {
  PFST_CHECK_ARG(logits && label && lse && coef && dlogits && N > 0 && C > 0 && C <= 255 && h > 0 && w > 0 && H > 0 && W > 0 && N <= 65535);
  PFST_CHECK_ARG(exponent >= 1.f && (i64)H * W < INT_MAX - 2048 && (form == 0 || blocks_form_ok(form, C, h, w, H, W, label, (uintptr_t)lse)) && (form != 0 || C <= 8 || work));
  hipStream_t s = (hipStream_t)stream;
  const bool e2 = exponent == 2.f;
  const float e1 = exponent - 1.f, sh = (float)h / (float)H, sw = (float)w / (float)W;
  const int gx = cdiv((i64)h * w, 256);
  if (form != 0) {
    const dim3 grid = bwd_blocks_grid(h, w, N);
#define PFST_DICE_BWD(S, E2)                                                                                                          \
  hipLaunchKernelGGL((dice_bwd_blocks_kernel<S, E2>), grid, dim3(256), 0, s, logits, C, h, w, label, ignore_index, e1, lse, coef, scale, \
                     dlogits, accumulate)
    if (form == 4 && e2) PFST_DICE_BWD(4, true);
    else if (form == 4) PFST_DICE_BWD(4, false);
    else if (e2) PFST_DICE_BWD(8, true);
    else PFST_DICE_BWD(8, false);
#undef PFST_DICE_BWD
  } else if (C <= 8) {
    if (e2)
      hipLaunchKernelGGL(dice_bwd_cells_kernel<true>, dim3(gx, 1, N), dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, sh, sw, e1,
                         lse, coef, scale, dlogits, accumulate);
    else
      hipLaunchKernelGGL(dice_bwd_cells_kernel<false>, dim3(gx, 1, N), dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, sh, sw, e1,
                         lse, coef, scale, dlogits, accumulate);
  } else {
    const dim3 gs(px_blocks((i64)H * W), N), gb(gx, C, N);
    if (e2) {
      hipLaunchKernelGGL(dice_s_kernel<true>, gs, dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, sh, sw, e1, lse, coef, work);
      hipLaunchKernelGGL(dice_bwd_kernel<true>, gb, dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, sh, sw, e1, lse, coef, work,
                         scale, dlogits, accumulate);
    } else {
      hipLaunchKernelGGL(dice_s_kernel<false>, gs, dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, sh, sw, e1, lse, coef, work);
      hipLaunchKernelGGL(dice_bwd_kernel<false>, gb, dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, sh, sw, e1, lse, coef, work,
                         scale, dlogits, accumulate);
    }
  }
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
