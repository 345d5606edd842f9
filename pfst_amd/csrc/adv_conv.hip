// The convolution family of the adversarial baseline's discriminator: 4x4 kernels, stride 2, padding 1, bias, dense
// NCHW fp32 -- forward with a fused LeakyReLU, data gradient with the LeakyReLU gate of the layer below, weight + bias gradient.  The
// streaming end of the network (the forward pass of a one-channel layer, the mean / L1 tail) is adv_tail.hip.
// Reference: rsiseg/models/discriminators/fc_discriminator.py:8-19 (five such layers).
//
// All three products are implicit GEMMs on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate), tiled like conv_mfma.hip's generic
// kernels: a 256-thread workgroup owns BM x 128 outputs, each wave 32x32 accumulators, K advances 16 per step through a double-buffered LDS
// tile with register-staged prefetch.  The weights are read in their torch layout w[Cout][Cin][4][4]: nothing is packed per step.
//
//   forward        y[co][oy][ox] = b[co] + sum_{ci,ty,tx} w[co][ci][ty][tx] x[ci][2 oy + ty - 1][2 ox + tx - 1]        K = (ci, tap): 16 Cin
//   data gradient  dx[ci][iy][ix] = sum_{co} sum_{ty = iy + 1 (mod 2), tx = ix + 1 (mod 2)} w[co][ci][ty][tx] dy[co][(iy + 1 - ty) / 2][(ix + 1 - tx) / 2]
//                  By the parity of (iy, ix) exactly 2 x 2 of the 16 taps reach an input element, so the launch is four sub-convolutions, one
//                  per parity class (grid z), each with K = (co, 2 x 2 taps): 4 Cout -- a quarter of the products of a gather over all 16 taps.
//                  Every element of dx belongs to one class and is written, border rows (fewer valid taps) included.
//   weight grad    dw[co][ci][tap] += sum_{n,oy,ox} dy[n][co][oy][ox] x[n][ci][2 oy + ty - 1][2 ox + tx - 1]            K = pixels, split over images
//                  and pixel chunks (wgrad_launch.h: fp32 atomics, or per-slice scratch + ordered sum in deterministic mode)
//
// Out-of-range rows, pixels and taps are loaded from a clamped (valid) address and zeroed on their way into LDS; stores are guarded.
#include "wgrad_launch.h"
#include "adv_conv.h"
#include "../../include/pfst_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int BK = 16, BN = 128;

template <int BM>
struct Tile {
  static constexpr int WM = BM >= 64 ? 64 : 32;
  static constexpr int WAVES_M = BM / WM;
  static constexpr int WAVES_N = 4 / WAVES_M;
  static constexpr int WN = BN / WAVES_N;
  static constexpr int TM = WM / 32, TN = WN / 32;
};

// MODE 0 (forward): in = x[Cin][Hi][Wi], out = y[Cout][Ho][Wo], rows = Cout, k = ci * 16 + tap.
// MODE 1 (data gradient): in = dy[Cout][Ho][Wo], out = dx[Cin][Hi][Wi], rows = Cin, k = co * 4 + a * 2 + b (ty = ty0 + 2 a, tx = tx0 + 2 b);
//   `gate` (or null) is x[Cin][Hi][Wi], the stored LeakyReLU output of the layer below: dx *= x > 0 ? 1 : slope.
// grid: (pixel tiles, row tiles, N) resp. (pixel tiles of the largest parity class, row tiles, 4 N)
template <int BM, int MODE>
__global__ __launch_bounds__(256) void adv_igemm_kernel(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
                                                        const float* __restrict__ gate, float* __restrict__ out, int Cin, int Hi, int Wi,
                                                        int Cout, int Ho, int Wo, int act, float slope, int accumulate) {
  using TL = Tile<BM>;
  constexpr int TM = TL::TM, TN = TL::TN;
  constexpr int A_N = BM / 16;      // A loads per thread and step: k = tid % 16 (contiguous in w), rows tid / 16 + 16 i
  constexpr int B_N = BK / 2;       // B loads per thread and step: pixel tid % 128, k = tid / 128 + 2 i
  constexpr int ALD = BM + 4;       // row pitch of the A tile: the 16 k of a store land in 16 different banks

  __shared__ float As[2][BK][ALD];
  __shared__ float Bs[2][BK][BN];

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wid / TL::WAVES_N) * TL::WM, wn0 = (wid % TL::WAVES_N) * TL::WN;
  const int M = MODE == 0 ? Cout : Cin;
  const int K = MODE == 0 ? Cin * 16 : Cout * 4;
  int n = blockIdx.z, py = 0, px = 0, Wp = Wo, P = Ho * Wo;
  if (MODE == 1) {
    const int q = blockIdx.z & 3;
    n = blockIdx.z >> 2;
    py = q >> 1;
    px = q & 1;
    Wp = (Wi - px + 1) >> 1;
    P = ((Hi - py + 1) >> 1) * Wp;
  }
  const int p0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
  if (p0 >= P) return;              // (a smaller parity class; the whole workgroup leaves before any barrier)
  const int ty0 = (py + 1) & 1, tx0 = (px + 1) & 1;
  const i64 in_img = MODE == 0 ? (i64)Cin * Hi * Wi : (i64)Cout * Ho * Wo;
  const i64 out_img = MODE == 0 ? (i64)Cout * Ho * Wo : (i64)Cin * Hi * Wi;
  in += (i64)n * in_img;
  out += (i64)n * out_img;

  // this thread's pixel of the B tile
  const int bj = tid % BN, br0 = tid / BN;
  const int p = p0 + bj;
  const bool pvalid = p < P;
  const int qy = pvalid ? p / Wp : 0, qx = pvalid ? p - qy * Wp : 0;
  // this thread's k and rows of the A tile
  const int ak = tid & 15, ar0 = tid >> 4;

  float areg[A_N], breg[B_N];
  unsigned a_mask = 0, b_mask = 0;
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto load_tile = [&](int kt) {
    const int k0 = kt * BK;
    a_mask = 0;
    b_mask = 0;
    {
      const int k = k0 + ak, kc = min(k, K - 1);
#pragma unroll
      for (int i = 0; i < A_N; ++i) {
        const int m = m0 + ar0 + 16 * i, mc = min(m, M - 1);
        i64 off;
        if (MODE == 0) {
          off = (i64)mc * K + kc;                                  // w[co = m][ci][tap], k = ci * 16 + tap
        } else {
          const int co = kc >> 2, a = (kc >> 1) & 1, b = kc & 1;
          off = ((i64)co * Cin + mc) * 16 + (ty0 + 2 * a) * 4 + tx0 + 2 * b;
        }
        areg[i] = w[off];
        a_mask |= (unsigned)(m < M && k < K) << i;
      }
    }
#pragma unroll
    for (int i = 0; i < B_N; ++i) {
      const int k = k0 + br0 + 2 * i, kc = min(k, K - 1);
      int ch, sy, sx, Hs, Ws;
      bool ok = pvalid && k < K;
      if (MODE == 0) {
        ch = kc >> 4;
        const int tap = kc & 15;
        sy = 2 * qy + (tap >> 2) - 1;
        sx = 2 * qx + (tap & 3) - 1;
        Hs = Hi;
        Ws = Wi;
      } else {
        ch = kc >> 2;
        // iy = py + 2 qy, ty = ty0 + 2 a: oy = (iy + 1 - ty) / 2 = qy + (py + 1 - ty0) / 2 - a, and (py + 1 - ty0) / 2 = py
        sy = qy + py - ((kc >> 1) & 1);
        sx = qx + px - (kc & 1);
        Hs = Ho;
        Ws = Wo;
      }
      ok = ok && (unsigned)sy < (unsigned)Hs && (unsigned)sx < (unsigned)Ws;
      breg[i] = in[ok ? ((i64)ch * Hs + sy) * Ws + sx : 0];
      b_mask |= (unsigned)ok << i;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_N; ++i) As[buf][ak][ar0 + 16 * i] = ((a_mask >> i) & 1u) ? areg[i] : 0.f;
#pragma unroll
    for (int i = 0; i < B_N; ++i) Bs[buf][br0 + 2 * i][bj] = ((b_mask >> i) & 1u) ? breg[i] : 0.f;
  };

  const int KT = (K + BK - 1) / BK;
  load_tile(0);
  store_tile(0);
  __syncthreads();

  const int l31 = lane & 31, lh = lane >> 5;
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < KT) load_tile(kt + 1);
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      const int krow = kk * 2 + lh;
      float af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = As[cur][krow][wm0 + i * 32 + l31];
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = Bs[cur][krow][wn0 + j * 32 + l31];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < KT) store_tile(cur ^ 1);
    __syncthreads();
  }

  // accumulator register r of lane (l31, lh): row (r & 3) + 8 (r >> 2) + 4 lh, column l31
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int pp = p0 + wn0 + j * 32 + l31;
    if (pp >= P) continue;
    int opix;
    if (MODE == 0) {
      opix = pp;
    } else {
      const int ry = pp / Wp, rx = pp - ry * Wp;
      opix = (py + 2 * ry) * Wi + px + 2 * rx;
    }
    const int plane = MODE == 0 ? Ho * Wo : Hi * Wi;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m >= M) continue;
        const i64 o = (i64)m * plane + opix;
        float v = acc[i][j][r];
        if (MODE == 0) {
          if (bias) v += bias[m];
          if (act) v = v > 0.f ? v : v * slope;
        } else if (gate) {
          v = gate[(i64)n * out_img + o] > 0.f ? v : v * slope;
        }
        out[o] = accumulate ? out[o] + v : v;
      }
    }
  }
}

// Weight gradient: rows = Cout (dy), columns j = ci * 16 + tap (dw's own order), K = the output pixels [pbeg, pend) of image n.
// grid: (ceil(16 Cin / 128), ceil(Cout / BM), N * chunks); dw += slice * det_stride in deterministic mode (one scratch tile-set per slice)
template <int BM>
__global__ __launch_bounds__(256) void adv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dw, int Cin,
                                                        int Hi, int Wi, int Cout, int Ho, int Wo, int chunks, int chunk_len, i64 det_stride) {
  using TL = Tile<BM>;
  constexpr int TM = TL::TM, TN = TL::TN;
  constexpr int WLD = BK + 1;
  constexpr int A_N = BM / 16, B_N = BN / 16;     // tile rows tid / 16 + 16 i, pixel tid % 16

  __shared__ float As[2][BM][WLD];
  __shared__ float Bs[2][BN][WLD];

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wid / TL::WAVES_N) * TL::WM, wn0 = (wid % TL::WAVES_N) * TL::WN;
  const int P = Ho * Wo, J = Cin * 16;
  const int j0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
  const int n = blockIdx.z / chunks, chunk = blockIdx.z - n * chunks;
  const int pbeg = chunk * chunk_len, pend = min(P, pbeg + chunk_len);
  if (pbeg >= pend) return;
  x += (i64)n * Cin * Hi * Wi;
  dy += (i64)n * Cout * P;
  dw += (i64)blockIdx.z * det_stride;

  const int kcol = tid & 15, r0 = tid >> 4;
  // column j0 + r0 + 16 i: tap r0 (j0 is a multiple of 16), channel j0 / 16 + i
  const int ty = r0 >> 2, tx = r0 & 3, ci0 = j0 >> 4;

  float areg[A_N], breg[B_N];
  bool pv = false, bv = false;
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto load_tile = [&](int pk0) {
    const int p = pk0 + kcol;
    pv = p < pend;
    const int pc = pv ? p : pend - 1;
    const int oy = pc / Wo, ox = pc - oy * Wo;
    const int sy = 2 * oy + ty - 1, sx = 2 * ox + tx - 1;
    bv = pv && (unsigned)sy < (unsigned)Hi && (unsigned)sx < (unsigned)Wi;
    const int spix = bv ? sy * Wi + sx : 0;
#pragma unroll
    for (int i = 0; i < A_N; ++i) areg[i] = dy[(i64)min(m0 + r0 + 16 * i, Cout - 1) * P + pc];
#pragma unroll
    for (int i = 0; i < B_N; ++i) breg[i] = x[(i64)min(ci0 + i, Cin - 1) * Hi * Wi + spix];
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_N; ++i) As[buf][r0 + 16 * i][kcol] = (pv && m0 + r0 + 16 * i < Cout) ? areg[i] : 0.f;
#pragma unroll
    for (int i = 0; i < B_N; ++i) Bs[buf][r0 + 16 * i][kcol] = (bv && ci0 + i < Cin) ? breg[i] : 0.f;
  };

  const int KT = (pend - pbeg + BK - 1) / BK;
  load_tile(pbeg);
  store_tile(0);
  __syncthreads();
  const int l31 = lane & 31, lh = lane >> 5;
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < KT) load_tile(pbeg + (kt + 1) * BK);
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      const int kc = kk * 2 + lh;
      float af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = As[cur][wm0 + i * 32 + l31][kc];
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = Bs[cur][wn0 + j * 32 + l31][kc];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < KT) store_tile(cur ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int jj = j0 + wn0 + j * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < Cout && jj < J) atomicAdd(&dw[(i64)m * J + jj], acc[i][j][r]);      // (deterministic mode: the slice's own scratch, one writer)
      }
    }
  }
}

inline bool adv_shape_ok(int N, int Cin, int Hi, int Wi, int Cout) {
  // 32-bit element offsets inside one image and one weight tensor; grid z carries 4 N (data gradient) or N * chunks; Cout within what
  // pfst_bias_grad takes, so that the weight gradient refuses a shape before anything is accumulated
  return N > 0 && N <= 16383 && Cin > 0 && Cout > 0 && Hi >= 2 && Wi >= 2 && (i64)Cin * Hi * Wi < (1ll << 29) &&
         (i64)Cout * (Hi / 2) * (Wi / 2) < (1ll << 29) && (i64)Cin * Cout * 16 < (1ll << 29) && Cin <= (1 << 20) && Cout <= 65535;
}

}  // namespace

extern "C" int pfst_adv_conv_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Hi, int Wi, int Cout, int act,
                                 float slope, pfst_stream_t stream) {
  PFST_CHECK_ARG(x && w && y && adv_shape_ok(N, Cin, Hi, Wi, Cout) && (act == 0 || act == 1));
  const int Ho = Hi / 2, Wo = Wi / 2;
  hipStream_t s = (hipStream_t)stream;
  if (Cout == 1) return adv_conv1_fwd_launch(x, w, bias, y, N, Cin, Hi, Wi, act, slope, s);      // a reduction per pixel, not a matrix product
  return with_row_tile(Cout, [&](auto bm) {
    constexpr int BM = decltype(bm)::value;
    const dim3 grid(cdiv((i64)Ho * Wo, BN), cdiv(Cout, BM), N);
    hipLaunchKernelGGL((adv_igemm_kernel<BM, 0>), grid, dim3(256), 0, s, x, w, bias, (const float*)nullptr, y, Cin, Hi, Wi, Cout, Ho, Wo, act, slope, 0);
    PFST_CHECK_LAUNCH();
    return PFST_OK;
  });
}

extern "C" int pfst_adv_conv_dgrad(const float* dy, const float* w, const float* x_gate, float* dx, int N, int Cin, int Hi, int Wi, int Cout,
                                   float slope, int accumulate, pfst_stream_t stream) {
  PFST_CHECK_ARG(dy && w && dx && adv_shape_ok(N, Cin, Hi, Wi, Cout) && (accumulate == 0 || accumulate == 1));
  const int Ho = Hi / 2, Wo = Wi / 2;
  hipStream_t s = (hipStream_t)stream;
  return with_row_tile(Cin, [&](auto bm) {
    constexpr int BM = decltype(bm)::value;
    const i64 pmax = (i64)((Hi + 1) / 2) * ((Wi + 1) / 2);          // the even-even class is the largest
    const dim3 grid(cdiv(pmax, BN), cdiv(Cin, BM), 4 * N);
    hipLaunchKernelGGL((adv_igemm_kernel<BM, 1>), grid, dim3(256), 0, s, dy, w, (const float*)nullptr, x_gate, dx, Cin, Hi, Wi, Cout, Ho, Wo, 0, slope,
                       accumulate);
    PFST_CHECK_LAUNCH();
    return PFST_OK;
  });
}

extern "C" int pfst_adv_conv_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int Cin, int Hi, int Wi, int Cout,
                                   pfst_stream_t stream) {
  PFST_CHECK_ARG(x && dy && dw && adv_shape_ok(N, Cin, Hi, Wi, Cout));
  const int Ho = Hi / 2, Wo = Wi / 2, P = Ho * Wo, J = Cin * 16;
  hipStream_t s = (hipStream_t)stream;
  const int rc = with_row_tile(Cout, [&](auto bm) {
    constexpr int BM = decltype(bm)::value;
    const int tiles = cdiv(J, BN) * cdiv(Cout, BM);
    const SplitK k = plan_split_k((i64)tiles * N, P, 256 * 2, BK, 65535 / N);
    const dim3 grid(cdiv(J, BN), cdiv(Cout, BM), N * k.chunks);
    return wgrad_launch(dw, (i64)Cout * J, 1, N * k.chunks, 0, s, [&](float* dst, i64, i64 slice_stride) {
      hipLaunchKernelGGL((adv_wgrad_kernel<BM>), grid, dim3(256), 0, s, x, dy, dst, Cin, Hi, Wi, Cout, Ho, Wo, k.chunks, k.chunk_len, slice_stride);
    });
  });
  if (rc != PFST_OK || !db) return rc;
  return pfst_bias_grad(dy, (i64)Cout * P, db, N, Cout, P, stream);
}
