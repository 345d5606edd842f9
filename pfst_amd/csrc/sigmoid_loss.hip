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
#include "upsample_walk.h"
#include "../../include/pfst_hip.h"

// plain + - * round one by one; every fused multiply-add below is written as one
#pragma clang fp contract(off)

namespace {

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

// an image-independent (k_pos, k_neg) table, by class
__device__ __forceinline__ void sig_coef(const float* __restrict__ coef, int C, float (&kpos)[8], float (&kneg)[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    kpos[c] = c < C ? coef[2 * c] : 0.f;
    kneg[c] = c < C ? coef[2 * c + 1] : 0.f;
  }
}

// What the sigmoid losses' forward does with a pixel of fwd_blocks_walk (upsample_walk.h): the accuracy counts from the frame's arg-max
// and, where the pixel counts and its weight is not zero, its C weighted loss terms.  The tables and sums are the kernel's own arrays: a
// functor that is indexed by a loop variable would stay in memory until that loop is unrolled.
template <int GM>
struct SigFwdPx {
  const float* __restrict__ pwp;
  int C, ign;
  float gamma;
  const float (&kpos)[8], (&kneg)[8];
  double (&sum)[8];
  int correct, valid, bad;
  float2 g2;
  __device__ __forceinline__ void pair(i64 p) {
    g2 = make_float2(1.f, 1.f);
    if (pwp) g2 = *reinterpret_cast<const float2*>(pwp + p);
  }
  __device__ __forceinline__ void pixel(int k, int l, const float (&zc)[8], float, int arg) {
    const float wgt = k ? g2.y : g2.x;
    // on copies that are stored back unconditionally: updates of the members under the branches would be merged into one store through a
    // selected address
    int co = correct, va = valid, ba = bad;
    if (l != ign && l < C) {
      va += 1;
      if (arg == l) co += 1;
      if (wgt != 0.f) {
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (c < C) sum[c] += (double)(wgt * sig_loss<GM>(zc[c], c == l, kpos[c], kneg[c], gamma));
      }
    } else if (l != ign) {
      ba += 1;
    }
    correct = co; valid = va; bad = ba;
  }
  __device__ __forceinline__ void pair_end(i64) {}
};

// The x4 / x8 cases (H == S h, W == S w, C <= 8) by inter-cell blocks.
// grid: (ceil((w + 1) / 16), ceil((h + 1) / (16 TILES)), N), 16 x 16 threads
template <int S, int TILES, int GM>
__global__ __launch_bounds__(256) void sig_fwd_blocks_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                             const unsigned char* __restrict__ label, const float* __restrict__ pw, int ign,
                                                             const float* __restrict__ coef, float gamma, double* __restrict__ slab,
                                                             long long* __restrict__ cnt) {
  __shared__ double smd[4][8];
  __shared__ int smi[4][4];
  const i64 n = blockIdx.z, HW = (i64)S * h * S * w;
  float kpos[8], kneg[8];
  sig_coef(coef, C, kpos, kneg);
  double sum[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) sum[c] = 0.0;
  SigFwdPx<GM> px{pw ? pw + n * HW : nullptr, C, ign, gamma, kpos, kneg, sum, 0, 0, 0};
  fwd_blocks_walk<S, TILES>(logits + n * C * h * w, C, h, w, label + n * HW, px);
  int correct = px.correct, valid = px.valid, bad = px.bad;
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

// What the sigmoid losses' gradient reads per pixel and its terms for the backward frames of upsample_walk.h: sig_grad of each class,
// weighted by the pixel weight; an ignored or out-of-range label or a zero weight adds nothing.  The gradient is separable per class, so
// any C runs (bwd_class_gather) without a per-pixel work map.  kpos / kneg: the kernel's own arrays, as in SigFwdPx.
template <int GM>
struct SigBwdPx {
  const float* __restrict__ pwp;
  int C, ign;
  float gamma;
  const float (&kpos)[8], (&kneg)[8];
  int c0;                        // the class that the frame calls 0: the launch row's in bwd_class_gather (its table entry is [0]), else 0
  float2 g2;
  int l;                         // the current pixel's label
  __device__ __forceinline__ void pair(i64 p) {
    g2 = make_float2(1.f, 1.f);
    if (pwp) g2 = *reinterpret_cast<const float2*>(pwp + p);
  }
  __device__ __forceinline__ bool skip(int k, int l_) const { return l_ == ign || l_ >= C || (k ? g2.y : g2.x) == 0.f; }
  __device__ __forceinline__ bool cell_skip(int p, int l_) const {
    if (l_ == ign || l_ >= C) return true;
    return (pwp ? pwp[p] : 1.f) == 0.f;
  }
  template <class Z>
  __device__ __forceinline__ float weight(int k, int l_, const Z&) {
    l = l_;
    return k ? g2.y : g2.x;
  }
  template <class Z>
  __device__ __forceinline__ float cell_weight(int p, int l_, const Z&) {
    l = l_;
    return pwp ? pwp[p] : 1.f;
  }
  template <class Z>
  __device__ __forceinline__ float term(int c, const Z& z) const { return sig_grad<GM>(z(c), l == c0 + c, kpos[c], kneg[c], gamma); }
};

// grid: (blocks over h*w, C, N).  One thread per low-resolution logit; gathers its full-res footprint.
template <int GM>
__global__ __launch_bounds__(256) void sig_bwd_kernel(const float* __restrict__ logits, int C, int h, int w, const unsigned char* __restrict__ label,
                                                      const float* __restrict__ pw, int H, int W, int ign, float sh, float sw,
                                                      const float* __restrict__ coef, float gamma, float scale, float* __restrict__ dlogits,
                                                      int accumulate) {
  const int c = blockIdx.y;
  const i64 n = blockIdx.z, HW = (i64)H * W, plane = (n * C + c) * h * w;
  const float kpos[8] = {coef[2 * c]}, kneg[8] = {coef[2 * c + 1]};
  SigBwdPx<GM> px{pw ? pw + n * HW : nullptr, C, ign, gamma, kpos, kneg, c};
  bwd_class_gather(logits + plane, h, w, label + n * HW, H, W, sh, sw, scale, dlogits + plane, accumulate, px);
}

// ONE thread per low-resolution cell for all classes (C <= 8).                                          grid: (blocks over h*w, 1, N)
template <int GM>
__global__ __launch_bounds__(256) void sig_bwd_cells_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                            const unsigned char* __restrict__ label, const float* __restrict__ pw, int H, int W,
                                                            int ign, float sh, float sw, const float* __restrict__ coef, float gamma,
                                                            float scale, float* __restrict__ dlogits, int accumulate) {
  const i64 n = blockIdx.z, HW = (i64)H * W, img = n * C * h * w;
  float kpos[8], kneg[8];
  sig_coef(coef, C, kpos, kneg);
  SigBwdPx<GM> px{pw ? pw + n * HW : nullptr, C, ign, gamma, kpos, kneg, 0};
  bwd_cells_gather(logits + img, C, h, w, label + n * HW, H, W, sh, sw, scale, dlogits + img, accumulate, px);
}

// The x4 / x8 cases by inter-cell blocks.                                                        grid: (ceil(w / 15), ceil(h / 15), N)
template <int S, int GM>
__global__ __launch_bounds__(256) void sig_bwd_blocks_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                             const unsigned char* __restrict__ label, const float* __restrict__ pw, int ign,
                                                             const float* __restrict__ coef, float gamma, float scale,
                                                             float* __restrict__ dlogits, int accumulate) {
  const i64 n = blockIdx.z, HW = (i64)S * h * S * w, img = n * C * h * w;
  float kpos[8], kneg[8];
  sig_coef(coef, C, kpos, kneg);
  SigBwdPx<GM> px{pw ? pw + n * HW : nullptr, C, ign, gamma, kpos, kneg, 0};
  bwd_blocks_walk<S>(logits + img, C, h, w, label + n * HW, scale, dlogits + img, accumulate, px);
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
  PFST_CHECK_ARG(gamma >= 0.f && (form == 0 || blocks_form_ok(form, C, h, w, H, W, label, (uintptr_t)pix_weight)));
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
    const dim3 grid = fwd_blocks_grid(form, h, w, N);
    PFST_CHECK_ARG(blocks == (int)(grid.x * grid.y));
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
  PFST_CHECK_ARG(gamma >= 0.f && (form == 0 || blocks_form_ok(form, C, h, w, H, W, label, (uintptr_t)pix_weight)));
  hipStream_t s = (hipStream_t)stream;
  const int gm = gamma_mode(gamma);
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  const int gx = cdiv((i64)h * w, 256);
  if (form != 0) {
    const dim3 grid = bwd_blocks_grid(h, w, N);
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
