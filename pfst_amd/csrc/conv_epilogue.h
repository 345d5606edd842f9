// Shared epilogue of the implicit-GEMM convolution kernels (fp32-MFMA, K-quad and bf16x6-split): optional fused BatchNorm
// statistics, bias, accumulate, store.  C/D layout of the 32x32 MFMA accumulator: column = lane & 31 (pixel),
// row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (output channel).
#pragma once
#include <type_traits>
#include <utility>
#include "common.h"
#ifndef PFST_BNB_LOAD_AUX
#define PFST_BNB_LOAD_AUX 0      // cache policy of the fused BatchNorm-backward epilogue's x / y loads (read once): A/B builds
#endif
#include "../../include/pfst_hip.h"

typedef float pfst_f32x16 __attribute__((ext_vector_type(16)));

// source coordinate of output index o for tap t: (o*a + t*b + c0) / div, div in {1,2}; branch-free validity.  (a, b, c0, div) come from
// conv_geometry (conv_launch.h): forward (stride, dil, -pad, 1), data gradient (1, -dil, pad, stride).
__device__ __forceinline__ bool src_coord(int o, int t, int a, int b, int c0, int div, int lim, int& s) {
  const int v = o * a + t * b + c0;
  const int odd = v & (div - 1);
  s = v >> (div >> 1);
  return (odd == 0) & (s >= 0) & (s < lim);
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), always unrolled: the pinned instruction schedules of the pipelined K loops
template <int... Is, class F>
__device__ __forceinline__ void static_for_seq(std::integer_sequence<int, Is...>, F&& f) {
  (f(std::integral_constant<int, Is>()), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_seq(std::make_integer_sequence<int, N>(), static_cast<F&&>(f));
}

// Fused BatchNorm-BACKWARD statistics (data-gradient launches).  When the tensor this launch writes is the COMPLETE gradient dL/dy
// of a conv -> BN(train) -> [+res] -> ReLU layer's output y (the launch is the last writer into that gradient buffer), the epilogue
// also emits per-block partials of the two reductions BatchNorm backward needs,
//     S1[c] = sum dz,   S2[c] = sum dz * xhat,     dz = dy * [ReLU gate],  xhat = (x - mean[c]) * invstd[c],
// from the final (accumulated) values it holds in registers, so the separate two-tensor reduction pass of pfst_bn_backward is
// dropped (its 2N of HBM reads move into an MFMA-bound kernel whose HBM is idle).  x = the layer's pre-BN tensor; the gate comes
// from y (> 0) for residual layers, else it is recomputed from x exactly as bn_apply computed it (bn_affine below).
typedef pfst_bnb_fuse_t PfstBnbArgs;      // include/pfst_hip.h (plain C struct of the ABI); value-initialised = off

// Transposing butterfly over the 32 lanes of each half-wave: every lane enters with NV values (one per accumulator row) and
// leaves with ONE fully reduced value, lane l holding value index l & (NV-1).  Each step exchanges half of the remaining
// values with the partner lane l ^ mask and adds, so the whole reduction costs NV-1 exchanges instead of 5 NV.  The partner
// permutations are XORs the DPP unit (or one ds_swizzle) provides: 16 | 15 = row mirror | 7 = half-row mirror | 2, 1 = quad
// perms; they are independent over GF(2) and the kept half is chosen by the top bit of each mask, which the lower masks
// leave alone, so partners always hold the same value subset and every lane's data is counted exactly once.
template <int CTRL>
__device__ __forceinline__ float lane_xchg(float v) {
  if (CTRL == 0) return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));   // lane ^ 16
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// OP: 0 sum, 1 minimum, 2 maximum (the per-channel extrema of the pre-BatchNorm tensor: pfst_bn_finalize_partials predicts max |y| from them)
template <int OP>
__device__ __forceinline__ float lane_combine(float a, float b) {
  return OP == 0 ? a + b : (OP == 1 ? fminf(a, b) : fmaxf(a, b));
}
template <int H, int CTRL, int OP = 0>
__device__ __forceinline__ void butterfly_step(float* a, bool upper) {   // 2H values -> H values
#pragma unroll
  for (int k = 0; k < H; ++k) {
    const float send = upper ? a[k] : a[k + H];
    const float keep = upper ? a[k + H] : a[k];
    a[k] = lane_combine<OP>(keep, lane_xchg<CTRL>(send));
  }
}
template <int NV, int OP = 0>
__device__ __forceinline__ float half_wave_transpose_reduce(float (&a)[NV], int l31) {
  static_assert(NV == 32 || NV == 16, "one value per accumulator row of a 64- or 32-row wave tile");
  if (NV == 32) {
    butterfly_step<16, 0, OP>(a, (l31 & 16) != 0);
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = lane_combine<OP>(a[k], lane_xchg<0>(a[k]));      // both 16-lane rows need all 16 values: plain combine
  }
  butterfly_step<8, 0x140, OP>(a, (l31 & 8) != 0);     // row_mirror      (lane ^ 15)
  butterfly_step<4, 0x141, OP>(a, (l31 & 4) != 0);     // row_half_mirror (lane ^ 7)
  butterfly_step<2, 0x4E, OP>(a, (l31 & 2) != 0);      // quad_perm [2,3,0,1]
  butterfly_step<1, 0xB1, OP>(a, (l31 & 1) != 0);      // quad_perm [1,0,3,2]
  return a[0];
}
template <int NV>
__device__ __forceinline__ float half_wave_transpose_sum(float (&a)[NV], int l31) { return half_wave_transpose_reduce<NV, 0>(a, l31); }

// The same reduction through LDS (16 values per lane = the rows of one 32x32 accumulator block): fp32 MFMA and VALU share the
// vector pipe, so the butterfly's ~3 VALU instructions per exchange come out of the co-resident waves' matrix throughput; LDS
// traffic does not.  Each lane writes its 16 values as 4 ds_write_b128 (lane stride 20 floats: the 16 lanes of a b128 group hit 16
// distinct bank quads), then lane (l31, lh) adds value (l31 & 15) of the 16 even (l31 < 16) or odd (l31 >= 16) lanes of its
// half-wave (16 conflict-free ds_read_b32: value index and lane parity spread over disjoint banks) and the two halves are
// combined with one lane ^ 16 exchange.  Same contract as half_wave_transpose_sum<16>.  `ws`: this wave's 64 * 20 floats; the
// caller has put a workgroup barrier between the main loop's last LDS reads and the first call.
constexpr int PFST_ROWSUM_LDS_FLOATS = 64 * 20;
// Lanes of ONE wave exchange values through LDS: the hardware completes a wave's LDS operations in order, but the compiler may
// move may-alias accesses; a wavefront-scope release/acquire fence + wave barrier (no instructions at run time) pins the order
// between a store phase and the loads of other lanes' values (and between a load phase and the next store phase).
__device__ __forceinline__ void wave_lds_phase_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float half_wave_rowsum_lds(const float (&v)[16], float* __restrict__ ws, int lane) {
  float4* wr = reinterpret_cast<float4*>(ws + lane * 20);
  wave_lds_phase_fence();        // a previous call's reads of `ws` (sv, then sq on the same scratch) come before these stores
  wr[0] = make_float4(v[0], v[1], v[2], v[3]);
  wr[1] = make_float4(v[4], v[5], v[6], v[7]);
  wr[2] = make_float4(v[8], v[9], v[10], v[11]);
  wr[3] = make_float4(v[12], v[13], v[14], v[15]);
  wave_lds_phase_fence();        // every lane's values are in LDS before any lane reads its neighbours'
  const int l31 = lane & 31;
  const float* rd = ws + ((lane & 32) + (l31 >> 4)) * 20 + (l31 & 15);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) s += rd[i * 40];
  return s + lane_xchg<0>(s);
}

// BNB: 0 = off; fused BatchNorm-backward sums with the ReLU gate 1 = recomputed from x, 2 = read from y, 3 = none (layer without ReLU),
// 4 = from bn_apply's bitmask of y (residual layers; P % 256 == 0)
// LDSRED: the per-row sums are reduced through the LDS scratch `lds` (half_wave_rowsum_lds) instead of the DPP butterfly
template <int TM, int TN, int WAVES_N, int BN, int BNB = 0, bool LDSRED = false>
__device__ __forceinline__ void conv_epilogue(pfst_f32x16 (&acc)[TM][TN], float* __restrict__ out, const float* __restrict__ bias,
                                              float* __restrict__ stats, int stats_T, int accumulate, int M, int P, int m0, int p0,
                                              int wm0, int wn0, int bx, int n, int wid, int lane, const PfstBnbArgs& bnb = PfstBnbArgs(),
                                              float* __restrict__ lds = nullptr, const float* __restrict__ gsrc = nullptr,
                                              const unsigned long long* __restrict__ gmask = nullptr, float* __restrict__ stats_mm = nullptr,
                                              bool nt_store = false) {
  // nt_store (wave-uniform): the plain output stores carry the streaming (nt) cache policy -- see conv_f16x3.hip
  // stats_mm (with stats, plain path): [M][stats_T][2] = per-channel (minimum, maximum) of this wave's output values -- BatchNorm + ReLU is a
  // monotone map of the pre-activation per channel, so max |y| of the NORMALISED tensor is attained at one of the two and is known (exactly:
  // pfst_bn_finalize_partials evaluates the same fma) before y is written: the consumer that normalises as it loads has its f16x3 scale
  // gsrc / gmask (this image's planes; whole row tiles, P % 256 == 0, no bias, accumulate = 0: checked on the host): out = acc + (bit ? gsrc : 0)
  // -- the identity branch of a residual block, dL/d(block input) = conv1's data gradient + dL/d(block output) gated by the block's final
  // ReLU (bn_apply's bitmask: word [row][p >> 8][p & 3], bit (p & 255) >> 2): the gated tensor is never written by BatchNorm backward
  const int l31 = lane & 31, lh = lane >> 5;
  // Fused BatchNorm statistics: per-row (output channel) sum / sum of squares over this wave's pixels, reduced across
  // the 32 lanes of each half-wave (transposing butterfly) and written (no atomics) to stats[m][slot][2]; pfst_bn_finalize_partials
  // reduces the slots in fp64.  Saves the separate full-tensor read of bn_stats.
  if (BNB == 0 && stats) {           // (the fused-backward variants are launched without forward statistics)
    const int gx = (P + BN - 1) / BN;
    const int slot = (n * gx + bx) * WAVES_N + (wid % WAVES_N);
    if constexpr (LDSRED) {
      // reduction through LDS, one 32-row block at a time (see half_wave_rowsum_lds)
      float* ws = lds + wid * PFST_ROWSUM_LDS_FLOATS;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        float sv[16], sq[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float a = 0.f, b = 0.f;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int pp = p0 + wn0 + j * 32 + l31;
            const float v = pp < P ? acc[i][j][r] : 0.f;
            a += v;
            b = fmaf(v, v, b);
          }
          sv[r] = a;
          sq[r] = b;
        }
        const float ts = half_wave_rowsum_lds(sv, ws, lane);
        const float tq = half_wave_rowsum_lds(sq, ws, lane);
        const int r = l31 & 15;
        const int m = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (l31 < 16 && m < M) reinterpret_cast<float2*>(stats)[(i64)m * stats_T + slot] = make_float2(ts, tq);
      }
    } else {
    constexpr int NV = TM * 16;
    float sv[NV], sq[NV];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int pp = p0 + wn0 + j * 32 + l31;
          const float v = pp < P ? acc[i][j][r] : 0.f;
          a += v;
          b = fmaf(v, v, b);
        }
        sv[i * 16 + r] = a;
        sq[i * 16 + r] = b;
      }
    }
    const float ts = half_wave_transpose_sum<NV>(sv, l31);
    const float tq = half_wave_transpose_sum<NV>(sq, l31);
    // lane l31 now owns value index e = l31 & (NV-1) = i*16 + r of its half-wave: one 8-byte store per lane
    const int e = l31 & (NV - 1), r = e & 15;
    const int m = m0 + wm0 + (e >> 4) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    if (l31 < NV && m < M) {
      float2* dst = reinterpret_cast<float2*>(stats) + ((i64)m * stats_T + slot);
      *dst = make_float2(ts, tq);
    }
    if (stats_mm) {
      const float inf = __builtin_inff();
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
          float lo = inf, hi = -inf;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const int pp = p0 + wn0 + j * 32 + l31;
            const float v = acc[i][j][rr];
            lo = pp < P ? fminf(lo, v) : lo;
            hi = pp < P ? fmaxf(hi, v) : hi;
          }
          sv[i * 16 + rr] = lo;
          sq[i * 16 + rr] = hi;
        }
      }
      const float tlo = half_wave_transpose_reduce<NV, 1>(sv, l31);
      const float thi = half_wave_transpose_reduce<NV, 2>(sq, l31);
      if (l31 < NV && m < M) reinterpret_cast<float2*>(stats_mm)[(i64)m * stats_T + slot] = make_float2(tlo, thi);
    }
    }
  }
  // Store.  fp32 MFMA and VALU share the vector pipe, so per-element address arithmetic and bounds checks in a 64-store
  // epilogue cost the co-resident waves real matrix throughput (measured: 10-17 % on tiles that live only 16-32 K-steps).
  // Fast path (all rows of this wave's sub-tile inside M, no bias): BUFFER stores -- one voffset per lane and column block
  // (pixel + the half-wave's 4-row shift; ragged pixel tiles use an out-of-range offset that the hardware drops), the row as
  // a SCALAR soffset: no vector arithmetic per element at all.
  if (BNB != 0 || (!bias && m0 + wm0 + TM * 32 <= M)) {     // BNB launches: whole row tiles and no bias (checked on the host)
    constexpr unsigned OOB = 0x80000000u;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(out, 0, M * P * 4, 0x00020000);
    unsigned voff[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int pp = p0 + wn0 + j * 32 + l31;
      voff[j] = pp < P ? 4u * ((unsigned)pp + 4u * (unsigned)lh * (unsigned)P) : OOB;
    }
    // NOTE for callers: wm0 must be provably wave-uniform (derive the wave id with __builtin_amdgcn_readfirstlane(tid >> 6));
    // otherwise every store below (and every accumulate load, each with its own vmcnt(0) wait) is wrapped in a waterfall
    // loop over the 'divergent' soffset -- measured 120-300 k cycles per workgroup.
    const int row0 = m0 + wm0;
    const bool gated = gsrc != nullptr;
    // what is added to a 32x32 block: the old values of `out`, or the gated tensor (16 loads issued back to back: one latency per block).
    // Gate bits (layout: relu_mask_plane / relu_mask_word in bn_bwd.h, restated by hand in mvoff below): the 64 pixel columns of a wave
    // tile start at a multiple of 64, so a lane's bits for both column blocks (pixel pp and
    // pp + 32: bit + 8) sit in the SAME 32-bit half of the same mask word -- one 4-byte load per accumulator row serves the row's two
    // blocks, and a sign-extending bit-field extract turns the bit into an AND mask (two vector instructions per element).
    static_assert(TN <= 2, "the gate words are shared by the column blocks of a 64-pixel wave tile");
    const __amdgpu_buffer_rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gated ? gsrc : out), 0, M * P * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t mrs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned long long*>(gmask), 0, gated ? M * (P >> 6) * 8 : 0, 0x00020000);
    const int gpp = p0 + wn0 + l31, gbit = (gpp & 255) >> 2;           // column block 0 (block 1: gbit + 8)
    const unsigned mvoff = 8u * (unsigned)((gpp >> 8) * 4 + (gpp & 3)) + 4u * (unsigned)(gbit >> 5) + 32u * (unsigned)lh * (unsigned)(P >> 6);
    auto load_gate = [&](int i, int (&gw)[16]) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        gw[r] = gated ? __builtin_amdgcn_raw_buffer_load_b32(mrs, mvoff, 8 * (P >> 6) * (row0 + i * 32 + (r & 3) + 8 * (r >> 2)), 0) : 0;
    };
    auto load_addend = [&](int i, int j, const int (&gw)[16], float (&old)[16]) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        old[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(grs, voff[j], 4 * P * (row0 + i * 32 + (r & 3) + 8 * (r >> 2)), 0));
      if (gated) {
        const unsigned sh = (unsigned)((gbit & 31) + 8 * j);
#pragma unroll
        for (int r = 0; r < 16; ++r)
          old[r] = __builtin_bit_cast(float, __builtin_bit_cast(int, old[r]) & __builtin_amdgcn_sbfe(gw[r], sh, 1u));
      }
    };
    if (BNB && (accumulate || gated)) {
      // the fused BatchNorm-backward sums below need the FINAL gradient: fold the addend into the accumulators first, then take the plain
      // store path
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        int gw[16];
        load_gate(i, gw);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          float old[16];
          load_addend(i, j, gw, old);
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] += old[r];
        }
      }
    }
    if (BNB || !(accumulate || gated)) {
      auto store_all = [&](auto aux_c) {
        constexpr int AUX = decltype(aux_c)::value;         // raw_buffer_store aux bits on gfx950: 2 = nt
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float v = acc[i][j][r];       // (a float temporary: __builtin_bit_cast of the vector-element lvalue reads element 0)
#ifdef PFST_DIAG_NO_STORE                         // timing-only build (WRONG results): what the output stores of the plain path cost
              if (v != 1.2345e-30f) continue;
#endif
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc, voff[j],
                                                    4 * P * (row0 + i * 32 + (r & 3) + 8 * (r >> 2)), AUX);
            }
          }
      };
#ifdef PFST_BNB_NT_STORE
      if (nt_store) store_all(std::integral_constant<int, 2>());
#else
      if (BNB == 0 && nt_store) store_all(std::integral_constant<int, 2>());
#endif
      else store_all(std::integral_constant<int, 0>());
    } else {
      // accumulate: the 16 loads of a 32x32 block are issued back to back, then added and stored (one latency per block, not 64)
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        int gw[16];
        load_gate(i, gw);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          float old[16];
          load_addend(i, j, gw, old);
#pragma unroll
          for (int r = 0; r < 16; ++r)
          {
            const float v = acc[i][j][r] + old[r];
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrc, voff[j],
                                                  4 * P * (row0 + i * 32 + (r & 3) + 8 * (r >> 2)), 0);
          }
        }
      }
    }
    if (BNB) {
      // S1 = sum dz and the RAW second sum S2' = sum dz * x of the layer that owns this gradient (pfst_bnb_fuse_t); pfst_bn_backward turns
      // them into sum dz * xhat = invstd * (S2' - mean * S1) in fp64.  Loads mirror the stores: the pixel (+ half-wave row shift) on the
      // voffset, the row on the scalar soffset; the ReLU gate is recomputed from x with the layer's (sc, sh) -- coef[row] holds
      // (mean, invstd, sc, sh) as bn_affine produced them in the forward pass -- or read from y for residual layers.
      const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bnb.x) + (i64)n * bnb.x_bs, 0, M * P * 4, 0x00020000);
      const __amdgpu_buffer_rsrc_t yr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bnb.y ? bnb.y + (i64)n * bnb.y_bs : bnb.x), 0,
                                                                          M * P * 4, 0x00020000);
      const __amdgpu_buffer_rsrc_t cr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bnb.coef), 0, M * 16, 0x00020000);
      constexpr bool gate_x = BNB == 1, gate_y = BNB == 2, gate_m = BNB == 4;
      // gate_m: one 4-byte mask word per accumulator row serves both column blocks (as for the gated addend above)
      const __amdgpu_buffer_rsrc_t ymr = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<unsigned long long*>(gate_m ? bnb.y_mask + (i64)n * M * (P >> 6) : nullptr), 0, gate_m ? M * (P >> 6) * 8 : 0, 0x00020000);
      const unsigned cvoff = 64u * (unsigned)lh + 8u;           // row + 4 lh, fields (sc, sh)
      const int gxp = (P + BN - 1) / BN;
      const int slot = (n * gxp + bx) * WAVES_N + (wid % WAVES_N);
      // one 32-row block of the wave tile at a time (16 values per lane and sum): keeps the live set at acc + 32 registers
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        float sv[16], sq[16];
        int yw[gate_m ? 16 : 1];
        if constexpr (gate_m) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            yw[r] = __builtin_amdgcn_raw_buffer_load_b32(ymr, mvoff, 8 * (P >> 6) * (row0 + i * 32 + (r & 3) + 8 * (r >> 2)), 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = row0 + i * 32 + (r & 3) + 8 * (r >> 2);
          float sc = 0.f, sh = 0.f;
          if (gate_x) {
            const float2 c2 = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(cr, cvoff, 16 * row, 0));
            sc = c2.x; sh = c2.y;
          }
          float a = 0.f, b = 0.f;
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const float xv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xr, voff[j], 4 * P * row, PFST_BNB_LOAD_AUX));
            float dz = voff[j] != OOB ? acc[i][j][r] : 0.f;
            if (gate_y) {
              const float yv = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(yr, voff[j], 4 * P * row, PFST_BNB_LOAD_AUX));
              dz = yv > 0.f ? dz : 0.f;
            } else if (gate_x) {
              dz = __fmaf_rn(xv, sc, sh) > 0.f ? dz : 0.f;
            } else if constexpr (gate_m) {
              dz = __builtin_bit_cast(float, __builtin_bit_cast(int, dz) & __builtin_amdgcn_sbfe(yw[r], (unsigned)((gbit & 31) + 8 * j), 1u));
            }
            a += dz;
            b = fmaf(dz, xv, b);
          }
          sv[r] = a;
          sq[r] = b;
          if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);     // 4 rows of loads in flight (register budget; 8 / 16 measured: same time)
        }
        float* ws = lds + wid * PFST_ROWSUM_LDS_FLOATS;
        const float ts = LDSRED ? half_wave_rowsum_lds(sv, ws, lane) : half_wave_transpose_sum<16>(sv, l31);
        const float tq = LDSRED ? half_wave_rowsum_lds(sq, ws, lane) : half_wave_transpose_sum<16>(sq, l31);
        // lane l31 (both 16-lane rows hold the same sums) owns accumulator row r = l31 & 15 of block i
        const int r = l31 & 15;
        const int m = row0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (l31 < 16) reinterpret_cast<float2*>(bnb.partials)[(i64)m * stats_T + slot] = make_float2(ts, tq);
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int pp = p0 + wn0 + j * 32 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < M && pp < P) {
          float v = acc[i][j][r];
          if (bias) v += bias[m];
          const i64 idx = (i64)m * P + pp;
          if (accumulate) v += out[idx];
          out[idx] = v;
        }
      }
    }
  }
}
