// Offline pseudo-labels with class-wise entropy thresholds: the reference's PseudoLabelingHookV4._cal_threshold
// (rsiseg/core/hook/pseudo_labeling_hookv4.py:173-205) and LoadAnnotationsPseudoLabelsV2 (rsiseg/datasets/pipelines/loading.py:475-494).
// As in loss.hip / dice_loss.hip the full-resolution logits are never materialised: every full-resolution pixel interpolates its C logits
// from the low-resolution map with bilin.h's helpers in the CE kernels' class order, and nothing per pixel is kept between the passes of the
// radix select -- every pass forms the pixel's entropy again, with ONE device function (px_eval) in which no rounding is left to the
// compiler's choice, so that the three entry points (and the register and the generic form of each) see the same bits for the same pixel:
// the file is compiled with contraction off (plain + - * / round on their own; the __f*_rn intrinsics would NOT do that here, they are
// inline functions made of plain operators under the default, fusable after inlining), and the one product-and-sum of the entropy is an
// explicit fma.  The resize's arithmetic is bilin.h's explicit fmas.
//
//   mode 0 (thresholds): p = exp(z - max) / sum (torch's softmax), pred = the first class whose ROUNDED p is maximal (pfst_pseudo_label's
//                        rule), H = -sum_c p_c log p_c with the term of p_c == 0 taken as 0
//   mode 1 (labels):     pred' = the first maximal LOGIT, H' = -sum_c p_c log(p_c + 1e-8)
//
// Both entropies are >= +0 (never -0: formed as 0 - s, and clamped), so the unsigned order of their bit patterns is their order as values.
#include <limits.h>
#include "common.h"
#include "bilin.h"
#include "../../include/pfst_hip.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int REG_C = 8;            // classes the register form holds per thread
constexpr int LDS_ENTRIES = 12288;  // 48 KB of 32-bit counters: the privatised histogram of one workgroup

__device__ __forceinline__ void ent_terms(int mode, float pc, float& s) {
  // s += p log p as ONE fma in every instantiation (an explicit builtin: nothing for the compiler to decide)
  if (mode == 0) {
    if (pc > 0.f) s = __builtin_fmaf(pc, logf(pc), s);
  } else {
    s = __builtin_fmaf(pc, logf(pc + 1e-8f), s);
  }
}
__device__ __forceinline__ float ent_finish(float s) {
  const float e = 0.f - s;                    // s <= 0 (p <= 1); 0 - (+-0) = +0
  return e > 0.f ? e : 0.f;
}

// REG: C <= 8, the pixel's logits in registers (class arrays indexed by compile-time constants only); else the classes are walked three times
// and interpolated again each time, as pseudo_label_kernel does.  The arithmetic per class is the same in both forms, in the same order.
template <bool REG>
__device__ __forceinline__ void px_eval(const float* __restrict__ lp, int C, int hw, int w, const Bilin& b, int mode, float& ent, int& pred) {
  float mx = -INFINITY, se = 0.f, s = 0.f, pmax = -1.f;
  int argz = 0, argp = 0;
  if (REG) {
    float z[REG_C];
#pragma unroll
    for (int c = 0; c < REG_C; ++c) {
      z[c] = c < C ? interp(lp + (i64)c * hw, w, b) : -INFINITY;
      if (c < C && z[c] > mx) { mx = z[c]; argz = c; }
    }
#pragma unroll
    for (int c = 0; c < REG_C; ++c)
      if (c < C) se = se + expf(z[c] - mx);
#pragma unroll
    for (int c = 0; c < REG_C; ++c) {
      if (c < C) {
        const float pc = expf(z[c] - mx) / se;
        if (pc > pmax) { pmax = pc; argp = c; }
        ent_terms(mode, pc, s);
      }
    }
  } else {
    for (int c = 0; c < C; ++c) {
      const float z = interp(lp + (i64)c * hw, w, b);
      if (z > mx) { mx = z; argz = c; }
    }
    for (int c = 0; c < C; ++c) se = se + expf(interp(lp + (i64)c * hw, w, b) - mx);
    for (int c = 0; c < C; ++c) {
      const float pc = expf(interp(lp + (i64)c * hw, w, b) - mx) / se;
      if (pc > pmax) { pmax = pc; argp = c; }
      ent_terms(mode, pc, s);
    }
  }
  ent = ent_finish(s);
  pred = mode == 0 ? argp : argz;
}

// grid: (blocks over H*W, N)
template <bool REG>
__global__ __launch_bounds__(256) void entropy_upsample_kernel(const float* __restrict__ logits, int C, int h, int w, int H, int W, float sh,
                                                               float sw, int mode, float* __restrict__ ent, unsigned char* __restrict__ pred) {
  const int n = blockIdx.y, hw = h * w, HW = H * W;
  const float* lp = logits + (i64)n * C * hw;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    const int oy = p / W, ox = p - oy * W;
    const Bilin b = make_bilin(oy, ox, sh, sw, h, w);
    float e;
    int a;
    px_eval<REG>(lp, C, hw, w, b, mode, e, a);
    if (ent) ent[(i64)n * HW + p] = e;
    if (pred) pred[(i64)n * HW + p] = (unsigned char)a;
  }
}

// One count per pixel at hist[pred][(key >> shift) & mask], key = the bit pattern of the mode-0 entropy; with a prefix table only the pixels
// whose higher key bits equal prefix[pred].  LDS: the workgroup counts into its own 32-bit table (a workgroup sees fewer than 2^31 pixels) and
// adds the non-zero entries to the 64-bit table at the end; else every pixel is one 64-bit atomic in global memory.  Integer adds: the table
// does not depend on any order.                                                              grid: (blocks over H*W, N); smem: LDS ? C << bits : 0
template <bool REG, bool LDS>
__global__ __launch_bounds__(256) void entropy_hist_kernel(const float* __restrict__ logits, int C, int h, int w, int H, int W, float sh, float sw,
                                                           int shift, int bits, const unsigned int* __restrict__ prefix, u64* __restrict__ hist) {
  extern __shared__ unsigned int sm[];
  const int n = blockIdx.y, hw = h * w, HW = H * W, entries = C << bits;
  const unsigned int mask = (1u << bits) - 1u;
  const float* lp = logits + (i64)n * C * hw;
  if (LDS) {
    for (int i = threadIdx.x; i < entries; i += blockDim.x) sm[i] = 0u;
    __syncthreads();
  }
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    const int oy = p / W, ox = p - oy * W;
    const Bilin b = make_bilin(oy, ox, sh, sw, h, w);
    float e;
    int a;
    px_eval<REG>(lp, C, hw, w, b, 0, e, a);
    const unsigned int key = __float_as_uint(e);
    if (prefix && (key >> (shift + bits)) != prefix[a]) continue;      // shift + bits < 32 with a prefix (checked on the host side)
    const int slot = (a << bits) + (int)((key >> shift) & mask);
    if (LDS) atomicAdd(&sm[slot], 1u);
    else atomicAdd(&hist[slot], (u64)1);
  }
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < entries; i += blockDim.x) {
      const unsigned int v = sm[i];
      if (v) atomicAdd(&hist[i], (u64)v);
    }
  }
}

// label = pred' where H' < thr[pred'], else ignored; annotation space: pred' + 1 and 0 (what LoadAnnotations(reduce_zero_label=True) turns
// back into pred' and 255).  counts[c] += (pixels predicted c, pixels kept as c).                                grid: (blocks over H*W, N)
template <bool REG>
__global__ __launch_bounds__(256) void entropy_label_kernel(const float* __restrict__ logits, int C, int h, int w, int H, int W, float sh, float sw,
                                                            const float* __restrict__ thr, int ann, unsigned char* __restrict__ label,
                                                            u64* __restrict__ counts) {
  __shared__ unsigned int sm[2 * 255];
  const int n = blockIdx.y, hw = h * w, HW = H * W;
  const float* lp = logits + (i64)n * C * hw;
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) sm[i] = 0u;
  __syncthreads();
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    const int oy = p / W, ox = p - oy * W;
    const Bilin b = make_bilin(oy, ox, sh, sw, h, w);
    float e;
    int a;
    px_eval<REG>(lp, C, hw, w, b, 1, e, a);
    const bool keep = e < thr[a];
    label[(i64)n * HW + p] = (unsigned char)(keep ? a + ann : (ann ? 0 : 255));
    atomicAdd(&sm[2 * a], 1u);
    if (keep) atomicAdd(&sm[2 * a + 1], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
    const unsigned int v = sm[i];
    if (v) atomicAdd(&counts[i], (u64)v);
  }
}

inline bool shape_ok(const void* logits, int N, int C, int h, int w, int H, int W) {
  return logits && N > 0 && N <= 65535 && C > 0 && C <= 255 && h > 0 && w > 0 && H > 0 && W > 0 && (i64)H * W < INT_MAX - 2048 * 4096 &&
         (i64)h * w * C < INT_MAX;
}

}  // namespace

extern "C" int pfst_entropy_upsample(const float* logits, int N, int C, int h, int w, int H, int W, int mode, float* ent, unsigned char* pred,
                                     pfst_stream_t stream) {
  PFST_CHECK_ARG(shape_ok(logits, N, C, h, w, H, W) && (mode == 0 || mode == 1) && (ent || pred));
  const dim3 grid(px_blocks((i64)H * W), N);
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  if (C <= REG_C)
    hipLaunchKernelGGL(entropy_upsample_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, logits, C, h, w, H, W, sh, sw, mode, ent, pred);
  else
    hipLaunchKernelGGL(entropy_upsample_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, logits, C, h, w, H, W, sh, sw, mode, ent, pred);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_entropy_class_hist(const float* logits, int N, int C, int h, int w, int H, int W, int shift, int bits,
                                       const unsigned int* prefix, unsigned long long* hist, pfst_stream_t stream) {
  PFST_CHECK_ARG(shape_ok(logits, N, C, h, w, H, W) && hist && shift >= 0 && bits >= 1 && bits <= 16 && shift + bits <= 32);
  PFST_CHECK_ARG(!prefix || shift + bits < 32);
  const dim3 grid(px_blocks((i64)H * W), N);
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  hipStream_t s = (hipStream_t)stream;
  const int entries = C << bits;
  const bool lds = entries <= LDS_ENTRIES;
  const size_t smem = lds ? (size_t)entries * sizeof(unsigned int) : 0;
#define PFST_ENT_HIST(REG, LDS) \
  hipLaunchKernelGGL((entropy_hist_kernel<REG, LDS>), grid, dim3(256), smem, s, logits, C, h, w, H, W, sh, sw, shift, bits, prefix, hist)
  if (C <= REG_C && lds) PFST_ENT_HIST(true, true);
  else if (C <= REG_C) PFST_ENT_HIST(true, false);
  else if (lds) PFST_ENT_HIST(false, true);
  else PFST_ENT_HIST(false, false);
#undef PFST_ENT_HIST
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_entropy_pseudo_label(const float* logits, int N, int C, int h, int w, int H, int W, const float* thr, int annotation_space,
                                         unsigned char* label, unsigned long long* counts, pfst_stream_t stream) {
  PFST_CHECK_ARG(shape_ok(logits, N, C, h, w, H, W) && thr && label && counts && (annotation_space == 0 || annotation_space == 1));
  const dim3 grid(px_blocks((i64)H * W), N);
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  if (C <= REG_C)
    hipLaunchKernelGGL(entropy_label_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, logits, C, h, w, H, W, sh, sw, thr, annotation_space,
                       label, counts);
  else
    hipLaunchKernelGGL(entropy_label_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, logits, C, h, w, H, W, sh, sw, thr,
                       annotation_space, label, counts);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
