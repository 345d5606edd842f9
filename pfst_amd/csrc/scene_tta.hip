// Test-time augmentation on whole scenes (pfst_amd/scene.py predict_scene_tta): aug_test (encoder_decoder.py:355-372) over slide_inference
// (:220-263) with the views of MultiScaleFlipAug (test_time_aug.py:98-126, img_scale=None).  Per view the scene is resized (and mirrored) on the
// device, goes through the scene path of scene.hip unchanged, and its window sums are folded into the scene-sized sum of probabilities in one
// pass; after the last view one pass makes labels (+ confidence, + probabilities).  Three streaming kernels in the style of scene.hip: one
// thread owns 4 consecutive pixels of a row (16-byte / dword accesses where the alignment allows, scalar otherwise), grid-stride, no LDS, no
// atomics.  Every value is formed with the operations of the chain it replaces, in the same order: bit-identical.
#include "common.h"
#include "../../include/pfst_hip.h"

static inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// ---- out[oy][ox] = resize(src, (Hr, Wr))[vflip ? Hr - 1 - oy : oy][hflip ? Wr - 1 - ox : ox]: the bilinear resize of pipeline.resize_bilinear_u8
// / pfst_cpu_resize_window_u8 (pipeline_cpu.c), mirrored on the way out as the pipeline's RandomFlip after Resize does.  Source indices and the
// weight of the upper index come per axis from the host (pipeline._src_index: yi / xi = [2][n] lo then hi, fy / fx = [n]), so the geometry keeps
// its one definition; the arithmetic is the C loop's: w0 = 1 - f, every product and every sum rounded on its own, rint half-to-even, clamp.
// With equal sizes the tables are the identity with weight 0 and the result is an exact (mirrored) copy.  A thread writes the 12 bytes of
// its four pixels as three dwords when they start on a 4-byte boundary; the source bytes are gathered (cache-resident rows).
__global__ __launch_bounds__(256) void scene_resize_u8_kernel(const unsigned char* __restrict__ src, int h, int w, const int* __restrict__ yi,
                                                              const float* __restrict__ fy, const int* __restrict__ xi,
                                                              const float* __restrict__ fx, int Hr, int Wr, int hflip, int vflip,
                                                              unsigned char* __restrict__ out) {
  // Plain * and + with contraction off for this body (the __f*_rn intrinsics are inline functions compiled under the default, which lets the
  // compiler fuse a product into the sum that follows it: one rounding fewer than the C loop, and a byte that differs wherever the blend
  // lies within an ulp of a half)
#pragma clang fp contract(off)
  const int w4 = (Wr + 3) >> 2;
  const i64 items = (i64)Hr * w4;
  for (i64 it = (i64)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (i64)gridDim.x * blockDim.x) {
    const int oy = (int)(it / w4), ox = (int)(it - (i64)oy * w4) * 4;
    const int nk = min(4, Wr - ox);
    const int vy = vflip ? Hr - 1 - oy : oy;
    const int y0 = min(max(yi[vy], 0), h - 1), y1 = min(max(yi[Hr + vy], 0), h - 1);       // the tables are the host's; never read outside src
    const float wy1 = fy[vy], wy0 = 1.0f - wy1;
    const unsigned char* r0 = src + (i64)y0 * w * 3;
    const unsigned char* r1 = src + (i64)y1 * w * 3;
    unsigned char o[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < nk) {
        const int vx = hflip ? Wr - 1 - (ox + k) : ox + k;
        const int x0 = min(max(xi[vx], 0), w - 1), x1 = min(max(xi[Wr + vx], 0), w - 1);
        const float wx1 = fx[vx], wx0 = 1.0f - wx1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float a = (float)r0[x0 * 3 + ch], b = (float)r0[x1 * 3 + ch], c = (float)r1[x0 * 3 + ch], d = (float)r1[x1 * 3 + ch];
          const float top = a * wx0 + b * wx1;
          const float bot = c * wx0 + d * wx1;
          float r = rintf(top * wy0 + bot * wy1);
          r = r < 0.f ? 0.f : r;
          r = r > 255.f ? 255.f : r;
          o[3 * k + ch] = (unsigned char)r;
        }
      } else {
        o[3 * k] = o[3 * k + 1] = o[3 * k + 2] = 0;
      }
    }
    unsigned char* op = out + ((i64)oy * Wr + ox) * 3;
    if (nk == 4 && (reinterpret_cast<uintptr_t>(op) & 3) == 0) {
      uint32_t* o4 = reinterpret_cast<uint32_t*>(op);
#pragma unroll
      for (int q = 0; q < 3; ++q)
        o4[q] = (uint32_t)o[4 * q] | ((uint32_t)o[4 * q + 1] << 8) | ((uint32_t)o[4 * q + 2] << 16) | ((uint32_t)o[4 * q + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if (k < 3 * nk) op[k] = o[k];
    }
  }
}

// ---- one view's window sums -> the scene-sized sum of probabilities: acc[c][ay][ax] = (accumulate ? acc : 0) + softmax_c(resize(sums / count,
// (H, W)))[c][vy][vx], (vy, vx) the view's pixel that lands on (ay, ax) after the un-flip.  The chain it replaces: window_normalize_ (a count
// plane), resize_bilinear (skipped when the sizes are equal), softmax_nchw, flip_planes, axpy_ (a store for the first view).  Each tap of the
// bilinear sample is __fdiv_rn(sum, (float)(rows[ys] * cols[xs])), the fp32 value window_normalize_kernel would have stored -- no Hr x Wr count
// plane and no normalised copy of the sums exist; the sample is bilin_src / bilin_blend at pfst_resize_bilinear's scales, the softmax
// softmax_nchw_kernel's max / sequential sum of expf / __fdiv_rn, the sum axpy_kernel's fmaf(1, p, acc): what tta_accumulate_kernel (spatial.hip)
// does for a tile, with the division in front of the taps.  CM classes in registers, PX pixels per thread (C <= 8: 4; up to PFST_TTA_MAX_C: 1).
// The view sums are read once per tap (neighbouring pixels share them in cache); the HBM traffic is the read-modify-write of acc.
template <int CM, int PX>
__global__ __launch_bounds__(256) void scene_tta_accumulate_kernel(const float* __restrict__ sums, int C, int Hr, int Wr,
                                                                   const int* __restrict__ rows, const int* __restrict__ cols, float sh, float sw,
                                                                   int skip, int hflip, int vflip, float* __restrict__ acc, int H, int W,
                                                                   int accumulate, int vec) {
  const int wg = (W + PX - 1) / PX;
  const i64 items = (i64)H * wg, HW = (i64)H * W, plane = (i64)Hr * Wr;
  for (i64 it = (i64)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (i64)gridDim.x * blockDim.x) {
    const int ay = (int)(it / wg), ax0 = (int)(it - (i64)ay * wg) * PX;
    const int nk = min(PX, W - ax0);
    const int vy = vflip ? H - 1 - ay : ay;
    int y0 = vy, y1 = vy;
    float ly0 = 1.f, ly1 = 0.f;
    if (!skip) bilin_src(vy, sh, Hr, y0, y1, ly0, ly1);
    const int rc0 = rows[y0], rc1 = rows[y1];
    float prob[PX][CM];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      if (k >= nk) continue;
      const int vx = hflip ? W - 1 - (ax0 + k) : ax0 + k;
      float mx = -INFINITY;
      if (skip) {
        const float cnt = (float)(rc0 * cols[vx]);
        const float* sp = sums + (i64)vy * Wr + vx;
#pragma unroll
        for (int c = 0; c < CM; ++c) {
          if (c < C) {
            prob[k][c] = __fdiv_rn(sp[(i64)c * plane], cnt);
            mx = fmaxf(mx, prob[k][c]);
          }
        }
      } else {
        int x0, x1;
        float lx0, lx1;
        bilin_src(vx, sw, Wr, x0, x1, lx0, lx1);
        const int cc0 = cols[x0], cc1 = cols[x1];
        const float n00 = (float)(rc0 * cc0), n01 = (float)(rc0 * cc1), n10 = (float)(rc1 * cc0), n11 = (float)(rc1 * cc1);
        const i64 o00 = (i64)y0 * Wr + x0, o01 = (i64)y0 * Wr + x1, o10 = (i64)y1 * Wr + x0, o11 = (i64)y1 * Wr + x1;
#pragma unroll
        for (int c = 0; c < CM; ++c) {
          if (c < C) {
            const float* cp = sums + (i64)c * plane;
            prob[k][c] = bilin_blend(__fdiv_rn(cp[o00], n00), __fdiv_rn(cp[o01], n01), __fdiv_rn(cp[o10], n10), __fdiv_rn(cp[o11], n11), lx0,
                                     lx1, ly0, ly1);
            mx = fmaxf(mx, prob[k][c]);
          }
        }
      }
      float se = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c < C) {
          prob[k][c] = expf(prob[k][c] - mx);
          se += prob[k][c];
        }
      }
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) prob[k][c] = __fdiv_rn(prob[k][c], se);
    }
    float* ap = acc + (i64)ay * W + ax0;
    const bool v4 = PX == 4 && vec && nk == 4;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c >= C) break;
      float* cp = ap + (i64)c * HW;
      if constexpr (PX == 4) {
        if (v4) {
          float4 a;
          if (accumulate) {
            a = *reinterpret_cast<const float4*>(cp);
            a.x = fmaf(1.f, prob[0][c], a.x); a.y = fmaf(1.f, prob[1][c], a.y); a.z = fmaf(1.f, prob[2][c], a.z); a.w = fmaf(1.f, prob[3][c], a.w);
          } else {
            a = make_float4(prob[0][c], prob[1][c], prob[2][c], prob[3][c]);
          }
          *reinterpret_cast<float4*>(cp) = a;
          continue;
        }
      }
#pragma unroll
      for (int k = 0; k < PX; ++k)
        if (k < nk) cp[k] = accumulate ? fmaf(1.f, prob[k][c], cp[k]) : prob[k][c];
    }
  }
}

// ---- the sum of the views -> labels (+ confidence, + probabilities): p = __fdiv_rn(acc, views) (div_scalar_kernel; BEFORE the comparison, ties
// made by the rounding resolve as in div + argmax), the first maximal class (argmax_nchw_kernel), confidence = rint(p_max * 255).  Unlike
// scene_finalize_kernel there is no softmax here, so nothing is needed twice: ONE loop over the classes serves every C (no register array, no
// separate generic kernel), each value read once and, when asked for, written once.  A thread owns four pixels of the flat map.
__global__ __launch_bounds__(256) void scene_tta_finalize_kernel(const float* __restrict__ acc, int C, i64 HW, float views,
                                                                 unsigned char* __restrict__ lab, unsigned char* __restrict__ conf,
                                                                 float* __restrict__ probs, int vec) {
  const i64 groups = (HW + 3) >> 2;
  for (i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (i64)gridDim.x * blockDim.x) {
    const i64 p = g * 4;
    const int nk = (int)(HW - p < 4 ? HW - p : 4);
    const bool v4 = vec && nk == 4;
    float best[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned char arg[4] = {0, 0, 0, 0};
    for (int c = 0; c < C; ++c) {
      const float* cp = acc + (i64)c * HW + p;
      float v[4];
      if (v4) {
        const float4 a = *reinterpret_cast<const float4*>(cp);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < nk ? cp[k] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = __fdiv_rn(v[k], views);
        if (c == 0) best[k] = v[k];
        else if (v[k] > best[k] || (v[k] != v[k] && best[k] == best[k])) { best[k] = v[k]; arg[k] = (unsigned char)c; }   // the first NaN wins
      }
      if (probs) {
        float* qp = probs + (i64)c * HW + p;
        if (v4) {
          *reinterpret_cast<float4*>(qp) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (k < nk) qp[k] = v[k];
        }
      }
    }
    unsigned char cf[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float r = rintf(__fmul_rn(best[k], 255.f));                 // NaN sums (never from this path) would give 0, not an undefined conversion
      r = r > 0.f ? r : 0.f;
      cf[k] = (unsigned char)(r > 255.f ? 255.f : r);
    }
    if (v4) {
      *reinterpret_cast<uchar4*>(lab + p) = make_uchar4(arg[0], arg[1], arg[2], arg[3]);
      if (conf) *reinterpret_cast<uchar4*>(conf + p) = make_uchar4(cf[0], cf[1], cf[2], cf[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < nk) {
          lab[p + k] = arg[k];
          if (conf) conf[p + k] = cf[k];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ C ABI
extern "C" int pfst_scene_resize_u8(const unsigned char* src_u8, int h, int w, const int* y_index, const float* y_frac, const int* x_index,
                                    const float* x_frac, int Hr, int Wr, int hflip, int vflip, unsigned char* out_u8, pfst_stream_t stream) {
  PFST_CHECK_ARG(src_u8 && out_u8 && y_index && y_frac && x_index && x_frac && src_u8 != out_u8);
  PFST_CHECK_ARG(h >= 1 && w >= 1 && Hr >= 1 && Wr >= 1 && (i64)h * w <= 0x7fffffffLL / 3 && (i64)Hr * Wr <= 0x7fffffffLL / 3);
  hipLaunchKernelGGL(scene_resize_u8_kernel, dim3(ew_grid((i64)Hr * ((Wr + 3) >> 2))), dim3(256), 0, (hipStream_t)stream, src_u8, h, w, y_index,
                     y_frac, x_index, x_frac, Hr, Wr, hflip ? 1 : 0, vflip ? 1 : 0, out_u8);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_scene_tta_accumulate(const float* sums, int C, int Hr, int Wr, const int* row_count, const int* col_count, int hflip, int vflip,
                                         float* acc, int H, int W, int accumulate, pfst_stream_t stream) {
  PFST_CHECK_ARG(sums && acc && row_count && col_count && sums != acc && C >= 1 && C <= PFST_TTA_MAX_C);
  PFST_CHECK_ARG(Hr >= 1 && Wr >= 1 && H >= 1 && W >= 1 && (i64)Hr * Wr <= 0x7fffffffLL && (i64)H * W <= 0x7fffffffLL);
  const int skip = Hr == H && Wr == W;
  const float sh = (float)Hr / (float)H, sw = (float)Wr / (float)W;          // = pfst_resize_bilinear's
  const int vec = (W & 3) == 0 && aligned(acc, 16);
  hipStream_t s = (hipStream_t)stream;
  if (C <= 8)
    hipLaunchKernelGGL((scene_tta_accumulate_kernel<8, 4>), dim3(ew_grid((i64)H * ((W + 3) >> 2))), dim3(256), 0, s, sums, C, Hr, Wr, row_count,
                       col_count, sh, sw, skip, hflip ? 1 : 0, vflip ? 1 : 0, acc, H, W, accumulate ? 1 : 0, vec);
  else
    hipLaunchKernelGGL((scene_tta_accumulate_kernel<PFST_TTA_MAX_C, 1>), dim3(ew_grid((i64)H * W)), dim3(256), 0, s, sums, C, Hr, Wr, row_count,
                       col_count, sh, sw, skip, hflip ? 1 : 0, vflip ? 1 : 0, acc, H, W, accumulate ? 1 : 0, 0);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_scene_tta_finalize(const float* acc, int C, int H, int W, int views, unsigned char* label_u8, unsigned char* conf_u8,
                                       float* probs, pfst_stream_t stream) {
  PFST_CHECK_ARG(acc && label_u8 && acc != probs && C >= 1 && C <= 255 && H >= 1 && W >= 1 && views >= 1);
  const i64 HW = (i64)H * W;
  const int vec = (HW & 3) == 0 && aligned(acc, 16) && aligned(label_u8, 4) && (!conf_u8 || aligned(conf_u8, 4)) && (!probs || aligned(probs, 16));
  hipLaunchKernelGGL(scene_tta_finalize_kernel, dim3(ew_grid((HW + 3) >> 2)), dim3(256), 0, (hipStream_t)stream, acc, C, HW, (float)views,
                     label_u8, conf_u8, probs, vec);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
