// Whole-scene prediction (pfst_amd/scene.py): a uint8 scene resident on the device is covered with overlapping windows, the windows are
// forwarded in batches, their low-resolution logits summed into place and the sums turned into labels -- slide_inference
// (encoder_decoder.py:220-263) + softmax + arg-max, and the painting of BaseSegmentor.show_result (segmentors/base.py:227-300).
// Four streaming kernels: one thread owns 4 consecutive pixels of a row (16-byte accesses where the alignment allows, scalar otherwise),
// grid-stride, no LDS, no atomics.  Every value is formed with the operations of the chain it replaces, in the same order: bit-identical.
#include "common.h"
#include "../../include/pfst_hip.h"

#define SCENE_MAX_WINDOWS 16
static_assert(SCENE_MAX_WINDOWS == PFST_SCENE_MAX_WINDOWS, "header and kernels disagree");

struct SceneWins {       // the windows of one batch, by value in the kernel arguments: no host-to-device copy, nothing to synchronise
  int n;
  int y[SCENE_MAX_WINDOWS], x[SCENE_MAX_WINDOWS];
};
struct SceneNorm {
  float mean[3], std[3];
};

static bool scene_wins(SceneWins& wins, const int* win_yx, int B, int h, int w, int H, int W) {
  if (!win_yx || B < 1 || B > SCENE_MAX_WINDOWS || h < 1 || w < 1 || H < 1 || W < 1) return false;
  wins.n = B;
  for (int b = 0; b < SCENE_MAX_WINDOWS; ++b) {
    const int y = b < B ? win_yx[2 * b] : 0, x = b < B ? win_yx[2 * b + 1] : 0;
    if (y < 0 || x < 0 || (i64)y + h > H || (i64)x + w > W) return false;          // every window lies inside the scene
    wins.y[b] = y;
    wins.x[b] = x;
  }
  return true;
}
static inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// ---- out[b][c][i][j] = (scene[y_b + i][x_b + j][to_rgb ? 2 - c : c] - mean[c]) / std[c]: pipeline.normalize (mmcv.imnormalize) of the
// window's pixels, transposed to CHW -- fp32 subtract, fp32 IEEE divide, as pfst_cpu_normalize_u8.  A thread reads the 12 bytes of its four
// pixels (three dwords when they start on a 4-byte boundary: x_b is arbitrary) and writes one float4 per channel.  grid: (blocks, B)
__global__ __launch_bounds__(256) void scene_windows_kernel(const unsigned char* __restrict__ scene, int W, SceneWins wins, int h, int w,
                                                            SceneNorm nm, int to_rgb, float* __restrict__ out, int vec) {
  const int b = blockIdx.y, w4 = (w + 3) >> 2;
  const i64 items = (i64)h * w4, plane = (i64)h * w;
  const unsigned char* sb = scene + ((i64)wins.y[b] * W + wins.x[b]) * 3;
  float* ob = out + (i64)b * 3 * plane;
  for (i64 it = (i64)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (i64)gridDim.x * blockDim.x) {
    const int y = (int)(it / w4), x = (int)(it - (i64)y * w4) * 4;
    const int nk = min(4, w - x);
    const unsigned char* sp = sb + ((i64)y * W + x) * 3;
    unsigned char px[12];
    if (nk == 4 && (reinterpret_cast<uintptr_t>(sp) & 3) == 0) {
      const uint32_t* s4 = reinterpret_cast<const uint32_t*>(sp);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const uint32_t v = s4[q];
        px[4 * q] = (unsigned char)(v & 255u); px[4 * q + 1] = (unsigned char)((v >> 8) & 255u);
        px[4 * q + 2] = (unsigned char)((v >> 16) & 255u); px[4 * q + 3] = (unsigned char)(v >> 24);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) px[k] = k < 3 * nk ? sp[k] : (unsigned char)0;
    }
    float* op = ob + (i64)y * w + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int sc = to_rgb ? 2 - c : c;
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = __fdiv_rn(__fsub_rn((float)px[3 * k + sc], nm.mean[c]), nm.std[c]);
      if (vec && nk == 4) {
        *reinterpret_cast<float4*>(op + c * plane) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < nk) op[c * plane + k] = v[k];
      }
    }
  }
}

// ---- sums[c][y][x] += for every window b of the batch that covers (y, x), in index order: resize_bilinear(logits[b], (h, w))[c][y - y_b][x - x_b]
// -- what B x (pfst_resize_bilinear to the window size, then pfst_window_accumulate) leaves in preds.  A thread owns four scene pixels of a row
// inside the batch's bounding box (columns from a multiple of 4) and gathers: the windows of a batch overlap, and the gather fixes the order
// of the additions to the sequential chain's whatever B is.  The value is bilin_src / bilin_blend at pfst_resize_bilinear's scales, the fp32
// value that kernel would have stored; the addition is window_accumulate_kernel's fp32 add.  Pixels no window of the batch covers are neither
// read nor written (a float4 access needs all four covered).  Classes go in chunks of CM registers per pixel, any C.  logits are small
// (B x 1.5 MB at 1024^2, C = 6): cache-resident; the HBM traffic is the read-modify-write of the covered sums.
template <int CM>
__global__ __launch_bounds__(256) void scene_accumulate_kernel(const float* __restrict__ logits, i64 lbs, SceneWins wins, int C, int hl, int wl,
                                                               int h, int w, float sh, float sw, float* __restrict__ sums, int H, int W, int by0,
                                                               int bx0, int bh, int bw4, int vec) {
  const i64 items = (i64)bh * bw4, HW = (i64)H * W, lplane = (i64)hl * wl;
  for (i64 it = (i64)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (i64)gridDim.x * blockDim.x) {
    const int r = (int)(it / bw4);
    const int y = by0 + r, x = bx0 + (int)(it - (i64)r * bw4) * 4;
    unsigned cov = 0;
    for (int b = 0; b < wins.n; ++b) {
      if (y < wins.y[b] || y >= wins.y[b] + h) continue;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k >= wins.x[b] && x + k < wins.x[b] + w) cov |= 1u << k;
    }
    if (!cov) continue;
    float* sp = sums + (i64)y * W + x;
    const bool v4 = vec && cov == 15u;
    for (int c0 = 0; c0 < C; c0 += CM) {
      float acc[CM][4];
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c0 + c < C) {
          const float* cp = sp + (i64)(c0 + c) * HW;
          if (v4) {
            const float4 a = *reinterpret_cast<const float4*>(cp);
            acc[c][0] = a.x; acc[c][1] = a.y; acc[c][2] = a.z; acc[c][3] = a.w;
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[c][k] = (cov >> k) & 1u ? cp[k] : 0.f;
          }
        }
      }
      for (int b = 0; b < wins.n; ++b) {
        const int wy = wins.y[b], wx = wins.x[b];
        if (y < wy || y >= wy + h) continue;
        int y0, y1;
        float ly0, ly1;
        bilin_src(y - wy, sh, hl, y0, y1, ly0, ly1);
        const float* lp = logits + (i64)b * lbs + (i64)c0 * lplane;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (x + k >= wx && x + k < wx + w) {
            int x0, x1;
            float lx0, lx1;
            bilin_src(x + k - wx, sw, wl, x0, x1, lx0, lx1);
#pragma unroll
            for (int c = 0; c < CM; ++c) {
              if (c0 + c < C) {
                const float* cp = lp + (i64)c * lplane;
                const float v = bilin_blend(cp[y0 * wl + x0], cp[y0 * wl + x1], cp[y1 * wl + x0], cp[y1 * wl + x1], lx0, lx1, ly0, ly1);
                acc[c][k] = __fadd_rn(acc[c][k], v);
              }
            }
          }
        }
      }
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c0 + c < C) {
          float* cp = sp + (i64)(c0 + c) * HW;
          if (v4) {
            *reinterpret_cast<float4*>(cp) = make_float4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if ((cov >> k) & 1u) cp[k] = acc[c][k];
          }
        }
      }
    }
  }
}

// ---- sums -> labels (+ confidence, + probabilities): window_normalize_kernel's __fdiv_rn(sum, count), softmax_nchw_kernel's max / sequential
// sum of expf / __fdiv_rn, argmax_nchw_kernel's first maximal class OF THE PROBABILITIES (ties made by the roundings resolve as in the chain).
// The cover count of (y, x) is rows[y] * cols[x] (windows covering the row x windows covering the column: the window grid is a product), two
// small tables instead of an H x W plane.  confidence = rint(p_max * 255).  CM classes in registers, PX pixels per thread.
template <int CM, int PX>
__global__ __launch_bounds__(256) void scene_finalize_kernel(const float* __restrict__ sums, int C, int H, int W, const int* __restrict__ rows,
                                                             const int* __restrict__ cols, unsigned char* __restrict__ lab,
                                                             unsigned char* __restrict__ conf, float* __restrict__ probs, int vec) {
  const int wg = (W + PX - 1) / PX;
  const i64 items = (i64)H * wg, HW = (i64)H * W;
  for (i64 it = (i64)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (i64)gridDim.x * blockDim.x) {
    const int y = (int)(it / wg), x = (int)(it - (i64)y * wg) * PX;
    const int nk = min(PX, W - x);
    const i64 p = (i64)y * W + x;
    const bool v4 = PX == 4 && vec && nk == 4;
    const int rc = rows[y];
    float val[CM][PX];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c < C) {
        const float* cp = sums + (i64)c * HW + p;
        if constexpr (PX == 4) {
          if (v4) {
            const float4 a = *reinterpret_cast<const float4*>(cp);
            val[c][0] = a.x; val[c][1] = a.y; val[c][2] = a.z; val[c][3] = a.w;
            continue;
          }
        }
#pragma unroll
        for (int k = 0; k < PX; ++k) val[c][k] = k < nk ? cp[k] : 0.f;
      }
    }
    unsigned char arg[PX], cf[PX];
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      arg[k] = 0; cf[k] = 0;
      if (k >= nk) continue;
      const float cnt = (float)(rc * cols[x + k]);
      float mx = -INFINITY;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c < C) {
          val[c][k] = __fdiv_rn(val[c][k], cnt);
          mx = fmaxf(mx, val[c][k]);
        }
      }
      float se = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c < C) {
          val[c][k] = expf(val[c][k] - mx);
          se += val[c][k];
        }
      }
      float best = 0.f;
      int a = 0;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c < C) {
          val[c][k] = __fdiv_rn(val[c][k], se);
          if (c == 0) best = val[c][k];
          else if (val[c][k] > best) { best = val[c][k]; a = c; }
        }
      }
      arg[k] = (unsigned char)a;
      cf[k] = (unsigned char)__float2int_rn(__fmul_rn(best, 255.f));
    }
    if constexpr (PX == 4) {
      if (v4) {
        *reinterpret_cast<uchar4*>(lab + p) = make_uchar4(arg[0], arg[1], arg[2], arg[3]);
        if (conf) *reinterpret_cast<uchar4*>(conf + p) = make_uchar4(cf[0], cf[1], cf[2], cf[3]);
        if (probs) {
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (c < C) *reinterpret_cast<float4*>(probs + (i64)c * HW + p) = make_float4(val[c][0], val[c][1], val[c][2], val[c][3]);
        }
        continue;
      }
    }
#pragma unroll
    for (int k = 0; k < PX; ++k) {
      if (k < nk) {
        lab[p + k] = arg[k];
        if (conf) conf[p + k] = cf[k];
        if (probs) {
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (c < C) probs[(i64)c * HW + p + k] = val[c][k];
        }
      }
    }
  }
}
// more classes than registers hold: the same arithmetic, the sums read again in every pass (as the three kernels of the chain do)
__global__ __launch_bounds__(256) void scene_finalize_generic_kernel(const float* __restrict__ sums, int C, int H, int W,
                                                                     const int* __restrict__ rows, const int* __restrict__ cols,
                                                                     unsigned char* __restrict__ lab, unsigned char* __restrict__ conf,
                                                                     float* __restrict__ probs) {
  const i64 HW = (i64)H * W;
  for (i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += (i64)gridDim.x * blockDim.x) {
    const int y = (int)(p / W), x = (int)(p - (i64)y * W);
    const float cnt = (float)(rows[y] * cols[x]);
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmaxf(mx, __fdiv_rn(sums[(i64)c * HW + p], cnt));
    float se = 0.f;
    for (int c = 0; c < C; ++c) {
      const float e = expf(__fdiv_rn(sums[(i64)c * HW + p], cnt) - mx);
      se += e;
    }
    float best = 0.f;
    int a = 0;
    for (int c = 0; c < C; ++c) {
      const float e = expf(__fdiv_rn(sums[(i64)c * HW + p], cnt) - mx);
      const float q = __fdiv_rn(e, se);
      if (probs) probs[(i64)c * HW + p] = q;
      if (c == 0) best = q;
      else if (q > best) { best = q; a = c; }
    }
    lab[p] = (unsigned char)a;
    if (conf) conf[p] = (unsigned char)__float2int_rn(__fmul_rn(best, 255.f));
  }
}

// ---- out[p][ch] = palette[lab[p]][ch] (RGB), or with a scene uint8(img * keep + colour * opacity) per channel as show_result (base.py:278-285)
// does in NumPy: img the scene's pixel (stored BGR, read in RGB order), DOUBLE products and sum without contraction, truncation toward zero;
// keep = 1 - opacity formed in double by the caller as Python forms it.  Labels beyond the palette keep colour 0 (`color_seg = np.zeros`).
// A thread owns four pixels of the flat map: one 4-byte label load, 12 bytes of scene and of output as three dwords.
__global__ __launch_bounds__(256) void paint_labels_kernel(const unsigned char* __restrict__ lab, i64 HW, const unsigned char* __restrict__ pal,
                                                           int colours, const unsigned char* __restrict__ scene, double keep, double opacity,
                                                           unsigned char* __restrict__ out, int vec) {
  const i64 groups = (HW + 3) >> 2;
  for (i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (i64)gridDim.x * blockDim.x) {
    const i64 p = g * 4;
    const int nk = (int)(HW - p < 4 ? HW - p : 4);
    const bool v4 = vec && nk == 4;
    unsigned char l[4] = {0, 0, 0, 0}, s[12], o[12];
    if (v4) {
      const uchar4 q = *reinterpret_cast<const uchar4*>(lab + p);
      l[0] = q.x; l[1] = q.y; l[2] = q.z; l[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nk) l[k] = lab[p + k];
    }
    if (scene) {
      if (v4) {
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(scene + 3 * p);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const uint32_t v = s4[q];
          s[4 * q] = (unsigned char)(v & 255u); s[4 * q + 1] = (unsigned char)((v >> 8) & 255u);
          s[4 * q + 2] = (unsigned char)((v >> 16) & 255u); s[4 * q + 3] = (unsigned char)(v >> 24);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) s[k] = k < 3 * nk ? scene[3 * p + k] : (unsigned char)0;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const unsigned char col = (int)l[k] < colours ? pal[3 * (int)l[k] + ch] : (unsigned char)0;
        if (scene) {
          const double d = __dadd_rn(__dmul_rn((double)s[3 * k + 2 - ch], keep), __dmul_rn((double)col, opacity));
          o[3 * k + ch] = (unsigned char)(int)d;
        } else {
          o[3 * k + ch] = col;
        }
      }
    }
    if (v4) {
      uint32_t* o4 = reinterpret_cast<uint32_t*>(out + 3 * p);
#pragma unroll
      for (int q = 0; q < 3; ++q)
        o4[q] = (uint32_t)o[4 * q] | ((uint32_t)o[4 * q + 1] << 8) | ((uint32_t)o[4 * q + 2] << 16) | ((uint32_t)o[4 * q + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if (k < 3 * nk) out[3 * p + k] = o[k];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ C ABI
extern "C" int pfst_scene_windows(const unsigned char* scene_u8, int H, int W, const int* win_yx, int B, int h, int w, float mean0, float mean1,
                                  float mean2, float std0, float std1, float std2, int to_rgb, float* out, pfst_stream_t stream) {
  PFST_CHECK_ARG(scene_u8 && out && win_yx);
  SceneWins wins;
  PFST_CHECK_ARG(scene_wins(wins, win_yx, B, h, w, H, W));
  PFST_CHECK_ARG(std0 != 0.f && std1 != 0.f && std2 != 0.f);
  SceneNorm nm = {{mean0, mean1, mean2}, {std0, std1, std2}};
  const int vec = (w & 3) == 0 && aligned(out, 16);
  const i64 items = (i64)h * ((w + 3) >> 2);
  hipLaunchKernelGGL(scene_windows_kernel, dim3(ew_grid(items), B), dim3(256), 0, (hipStream_t)stream, scene_u8, W, wins, h, w, nm,
                     to_rgb ? 1 : 0, out, vec);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_scene_accumulate(const float* logits, long long logits_bs, int B, int C, int hl, int wl, const int* win_yx, int h, int w,
                                     float* sums, int H, int W, pfst_stream_t stream) {
  PFST_CHECK_ARG(logits && sums && win_yx && C >= 1 && hl >= 1 && wl >= 1 && logits_bs >= (i64)C * hl * wl);
  PFST_CHECK_ARG((i64)hl * wl <= 0x7fffffffLL);
  SceneWins wins;
  PFST_CHECK_ARG(scene_wins(wins, win_yx, B, h, w, H, W));
  int y0 = H, x0 = W, y1 = 0, x1 = 0;                      // bounding box of the batch's windows
  for (int b = 0; b < B; ++b) {
    y0 = wins.y[b] < y0 ? wins.y[b] : y0;
    x0 = wins.x[b] < x0 ? wins.x[b] : x0;
    y1 = wins.y[b] + h > y1 ? wins.y[b] + h : y1;
    x1 = wins.x[b] + w > x1 ? wins.x[b] + w : x1;
  }
  x0 &= ~3;                                                // pixel groups start at a multiple of 4: 16-byte aligned when W % 4 == 0
  const int bh = y1 - y0, bw4 = (x1 - x0 + 3) >> 2;
  const int vec = (W & 3) == 0 && aligned(sums, 16);
  const float sh = (float)hl / (float)h, sw = (float)wl / (float)w;          // = pfst_resize_bilinear's
  hipLaunchKernelGGL((scene_accumulate_kernel<8>), dim3(ew_grid((i64)bh * bw4)), dim3(256), 0, (hipStream_t)stream, logits, (i64)logits_bs,
                     wins, C, hl, wl, h, w, sh, sw, sums, H, W, y0, x0, bh, bw4, vec);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_scene_finalize(const float* sums, int C, int H, int W, const int* row_count, const int* col_count, unsigned char* label_u8,
                                   unsigned char* conf_u8, float* probs, pfst_stream_t stream) {
  PFST_CHECK_ARG(sums && row_count && col_count && label_u8 && C >= 1 && C <= 255 && H >= 1 && W >= 1);
  const int vec = (W & 3) == 0 && aligned(sums, 16) && aligned(label_u8, 4) && (!conf_u8 || aligned(conf_u8, 4)) && (!probs || aligned(probs, 16));
  hipStream_t s = (hipStream_t)stream;
  if (C <= 8)
    hipLaunchKernelGGL((scene_finalize_kernel<8, 4>), dim3(ew_grid((i64)H * ((W + 3) >> 2))), dim3(256), 0, s, sums, C, H, W, row_count,
                       col_count, label_u8, conf_u8, probs, vec);
  else if (C <= PFST_TTA_MAX_C)
    hipLaunchKernelGGL((scene_finalize_kernel<PFST_TTA_MAX_C, 1>), dim3(ew_grid((i64)H * W)), dim3(256), 0, s, sums, C, H, W, row_count,
                       col_count, label_u8, conf_u8, probs, 0);
  else
    hipLaunchKernelGGL(scene_finalize_generic_kernel, dim3(ew_grid((i64)H * W)), dim3(256), 0, s, sums, C, H, W, row_count, col_count,
                       label_u8, conf_u8, probs);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_paint_labels(const unsigned char* label_u8, int H, int W, const unsigned char* palette_rgb, int colours,
                                 const unsigned char* scene_bgr, double keep, double opacity, unsigned char* out_rgb, pfst_stream_t stream) {
  PFST_CHECK_ARG(label_u8 && palette_rgb && out_rgb && H >= 1 && W >= 1 && colours >= 1 && colours <= 256);
  PFST_CHECK_ARG(!scene_bgr || (opacity >= 0.0 && opacity <= 1.0 && keep >= 0.0 && keep <= 1.0));
  const i64 HW = (i64)H * W;
  const int vec = aligned(label_u8, 4) && aligned(out_rgb, 4) && (!scene_bgr || aligned(scene_bgr, 4));
  hipLaunchKernelGGL(paint_labels_kernel, dim3(ew_grid((HW + 3) >> 2)), dim3(256), 0, (hipStream_t)stream, label_u8, HW, palette_rgb, colours,
                     scene_bgr, keep, opacity, out_rgb, vec);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
