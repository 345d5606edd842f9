// Fused bilinear-upsample + softmax + Lovasz-Softmax loss (+ accuracy), forward and backward.
// Reference: rsiseg/models/losses/lovasz_loss.py (lovasz_softmax_flat, lovasz_grad) behind decode_heads/decode_head.py:249-283; DESIGN.md 8m.
// As in loss.hip / dice_loss.hip the full-resolution logits are never materialised; unlike every other term the loss is no per-pixel sum:
// per class it needs every valid pixel's rank among the errors e = |fg - p_c|.  Stages, all on the caller's stream:
//
//   keys      the pixel walk of upsample_walk.h (x4 / x8 block frames for C <= 8, a generic kernel otherwise): acc_seg and bad-label counts,
//             the log-sum-exp map (read when a CE term left it, the same bits either way) and, per class of the class set, one
//             (key, value) pair per pixel.  key = 0x3F800000 - bits(e): e in [0, 1] orders as its fp32 bits, so ASCENDING keys are descending
//             errors; a pixel under ignore_index gets LOVASZ_INVALID, above every valid key -- it sorts behind all valid pixels and moves no
//             valid pixel's rank.  value = the pixel's index in its segment's pixel order (n, y, x), bit 31 = foreground.
//             Segments: one per class slot (per_image = 0, N H W elements) or per (image, slot) (per_image = 1, H W elements).
//   sort      a stable segmented LSD radix sort, 8-bit digits, 4 passes, segments on grid.y.  A pass = per-workgroup digit histograms, an
//             exclusive scan per segment in (digit, workgroup) order (a workgroup per digit scans its row of counts; the 256 digit totals
//             are scanned by every scatter workgroup), and a scatter that ranks equal digits in input order (ballots inside a wave, a
//             wave's running digit counters in LDS, waves in order).  Integer counting only, no tickets: the permutation does not
//             depend on launch, wave or stream order.  Equal keys keep ascending pixel index.
//   gradient  over the sorted order: the inclusive integer scan of the foreground flags (per-tile counts, then in-tile ballots),
//             g_k = J_k - J_{k-1} in fp64, the coefficient sign(fg - p) cw g_k scattered to map[n][slot][pixel], and sum e_k g_k per tile in
//             fp64 in a fixed order (no atomics: bit-identical run to run in either mode).
//   finalize  one workgroup: present mask, class mean, per_image reduction, loss_weight -> out[3] and the scale block of the backward.
//   backward  the backward frames of upsample_walk.h: dz_j = p_j (d_j - sum_c d_c p_c), d_c = scale[n][slot] map[n][slot][pixel].
#include <limits.h>
#include <algorithm>
#include "common.h"
#include "upsample_walk.h"
#include "../../include/pfst_hip.h"

namespace {

constexpr unsigned LOVASZ_ONE = 0x3F800000u;       // bits(1.0f)
constexpr unsigned LOVASZ_INVALID = LOVASZ_ONE + 1u;
constexpr int SORT_ITEMS = 16, SORT_TILE = 256 * SORT_ITEMS;   // elements per workgroup of the sort and gradient kernels
constexpr int GPIX = 4;                                       // pixels per thread of the generic key kernel

// counters (unsigned 64-bit, zeroed per call): [0] #correct, [1] #valid for acc_seg, [2] #bad labels, [3 + n K + k] foreground count
__device__ __forceinline__ void count_add(unsigned long long* cnt, int v) {
  v = wave_sum_i(v);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(cnt, (unsigned long long)v);      // integers: exact in any order
}

__device__ __forceinline__ unsigned lovasz_key(float p, bool fg, bool valid) {
  float e = fg ? 1.f - p : p;
  e = fminf(fmaxf(e, 0.f), 1.f);                   // (a NaN becomes 0: the key stays inside the range the sort is sized for)
  return valid ? LOVASZ_ONE - __float_as_uint(e) : LOVASZ_INVALID;
}
__device__ __forceinline__ float lovasz_prob(float x) { return fminf(expf(x), 1.f); }

// -------------------------------------------------------------------------------------------------------------------- keys
// Any H x W, any C <= 255: dice_fwd_kernel's walk (ce_fwd_kernel's arithmetic and order: bit-identical lse and arg-max).  grid: (ceil(H W / 1024), N)
__global__ __launch_bounds__(256) void lovasz_keys_kernel(const float* __restrict__ logits, int C, int h, int w, const unsigned char* __restrict__ label,
                                                          int H, int W, int ign, float sh, float sw, const int* __restrict__ slot, int K,
                                                          i64 sn, i64 sk, int per_image, const float* __restrict__ lse_in,
                                                          float* __restrict__ lse_out, unsigned* __restrict__ keys, unsigned* __restrict__ vals,
                                                          unsigned long long* __restrict__ cnt) {
  const int n = blockIdx.y, hw = h * w, HW = H * W;
  const float* lp = logits + (i64)n * C * hw;
  Bilin b[GPIX];
  float ls[GPIX];
  int lab[GPIX];
  bool in[GPIX];
  int correct = 0, valid = 0, bad = 0;
#pragma unroll
  for (int k = 0; k < GPIX; ++k) {
    const int p = blockIdx.x * (256 * GPIX) + k * 256 + threadIdx.x;
    in[k] = p < HW;
    const int q = in[k] ? p : 0;
    const int oy = q / W, ox = q - oy * W;
    b[k] = make_bilin(oy, ox, sh, sw, h, w);
    lab[k] = ign;
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
      if (l != ign && l < C) {
        valid += 1;
        if (arg == l) correct += 1;
      } else if (l != ign) {
        bad += 1;
      }
    }
  }
  for (int c = 0; c < C; ++c) {
    const int s = slot[c];
    if (s < 0 || s >= K) continue;                 // (uniform: the class is not in the class set)
    int G = 0;
#pragma unroll
    for (int k = 0; k < GPIX; ++k) {
      if (in[k]) {
        const int p = blockIdx.x * (256 * GPIX) + k * 256 + threadIdx.x;
        const bool ok = lab[k] != ign, fg = ok && lab[k] == c;
        const float pc = lovasz_prob(interp(lp + (i64)c * hw, w, b[k]) - ls[k]);
        const i64 at = (i64)n * sn + (i64)s * sk + p;
        keys[at] = lovasz_key(pc, fg, ok);
        vals[at] = (unsigned)(per_image ? p : n * HW + p) | (fg ? 0x80000000u : 0u);
        G += fg ? 1 : 0;
      }
    }
    count_add(cnt + 3 + (i64)n * K + s, G);
  }
  count_add(cnt, correct);
  count_add(cnt + 1, valid);
  count_add(cnt + 2, bad);
}

// What the key pass does with a pixel of fwd_blocks_walk: the log-sum-exp as DiceFwdPx has it, the keys of the class set -- stored in
// pixel pairs -- and the counts.  Arrays are the kernel's own (see DiceFwdPx).
struct LovaszKeyPx {
  const float* __restrict__ li;
  float* __restrict__ ls;
  unsigned* __restrict__ keys;      // the image's first element of slot 0
  unsigned* __restrict__ vals;
  i64 sk;
  unsigned vbase;                   // value of the image's pixel 0
  int C, ign;
  const int (&slot)[8];
  int (&G)[8];
  unsigned (&kx)[8], (&ky)[8];
  int correct, valid, bad;
  unsigned fgx, fgy;
  float2 e2, lo;
  __device__ __forceinline__ void pair(i64 p) {
    e2 = make_float2(0.f, 0.f);
    if (li) e2 = *reinterpret_cast<const float2*>(li + p);
    fgx = fgy = 0u;
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
    const bool ok = l != ign;
    unsigned fgm = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {
        const bool fg = ok && l == c;
        const unsigned key = lovasz_key(lovasz_prob(zc[c] - e), fg, ok);
        kx[c] = k ? kx[c] : key;
        ky[c] = k ? key : ky[c];
        fgm |= fg ? (1u << c) : 0u;
        G[c] += fg ? 1 : 0;
      }
    }
    fgx = k ? fgx : fgm;
    fgy = k ? fgm : fgy;
    int co = correct, va = valid, ba = bad;
    if (ok && l < C) {
      va += 1;
      if (arg == l) co += 1;
    } else if (ok) {
      ba += 1;
    }
    correct = co; valid = va; bad = ba;
  }
  __device__ __forceinline__ void pair_end(i64 p) {
    if (ls) *reinterpret_cast<float2*>(ls + p) = lo;
    const unsigned v = vbase + (unsigned)p;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C && slot[c] >= 0) {
        const i64 at = (i64)slot[c] * sk + p;
        *reinterpret_cast<uint2*>(keys + at) = make_uint2(kx[c], ky[c]);
        *reinterpret_cast<uint2*>(vals + at) = make_uint2(v | ((fgx >> c) & 1u) << 31, (v + 1u) | ((fgy >> c) & 1u) << 31);
      }
    }
  }
};

__device__ __forceinline__ void load_slots(const int* __restrict__ slot, int C, int K, int (&sl)[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int s = c < C ? slot[c] : -1;
    sl[c] = s < K ? s : -1;
  }
}

// grid: fwd_blocks_grid, 16 x 16 threads
template <int S, int TILES>
__global__ __launch_bounds__(256) void lovasz_keys_blocks_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                                 const unsigned char* __restrict__ label, int ign, const int* __restrict__ slot,
                                                                 int K, i64 sn, i64 sk, int per_image, const float* __restrict__ lse_in,
                                                                 float* __restrict__ lse_out, unsigned* __restrict__ keys,
                                                                 unsigned* __restrict__ vals, unsigned long long* __restrict__ cnt) {
  const i64 n = blockIdx.z, HW = (i64)S * h * S * w;
  int sl[8], G[8];
  unsigned kx[8], ky[8];
  load_slots(slot, C, K, sl);
#pragma unroll
  for (int c = 0; c < 8; ++c) { G[c] = 0; kx[c] = ky[c] = 0u; }
  LovaszKeyPx px{lse_in ? lse_in + n * HW : nullptr, lse_in ? nullptr : lse_out + n * HW, keys + n * sn, vals + n * sn, sk,
                 per_image ? 0u : (unsigned)(n * HW), C, ign, sl, G, kx, ky, 0, 0, 0, 0u, 0u};
  fwd_blocks_walk<S, TILES>(logits + n * C * h * w, C, h, w, label + n * HW, px);
#pragma unroll
  for (int c = 0; c < 8; ++c)
    if (c < C && sl[c] >= 0) count_add(cnt + 3 + n * K + sl[c], G[c]);
  count_add(cnt, px.correct);
  count_add(cnt + 1, px.valid);
  count_add(cnt + 2, px.bad);
}

// -------------------------------------------------------------------------------------------------------------------- sort
// segment s holds elements [s stride, s stride + len_s), len_s = seg_len[s] clamped to [0, L] (seg_len null: L)
__device__ __forceinline__ int seg_length(const int* __restrict__ seg_len, int s, int L) { return seg_len ? min(max(seg_len[s], 0), L) : L; }

// hist[s][digit][workgroup]: the digit counts of a workgroup's tile.  LDS integer atomics: the counts do not depend on their order.
// grid: (nblk, S)
__global__ __launch_bounds__(256) void sort_hist_kernel(const unsigned* __restrict__ keys, i64 stride, const int* __restrict__ seg_len, int L,
                                                        int shift, int nblk, int* __restrict__ hist) {
  __shared__ int hs[256];
  const int s = blockIdx.y, blk = blockIdx.x, len = seg_length(seg_len, s, L);
  hs[threadIdx.x] = 0;
  __syncthreads();
  const unsigned* kp = keys + (i64)s * stride;
  const i64 base = (i64)blk * SORT_TILE;
#pragma unroll 4
  for (int i = 0; i < SORT_ITEMS; ++i) {
    const i64 idx = base + i * 256 + threadIdx.x;
    if (idx < len) atomicAdd(&hs[(kp[idx] >> shift) & 255u], 1);
  }
  __syncthreads();
  hist[((i64)s * 256 + threadIdx.x) * nblk + blk] = hs[threadIdx.x];
}

// exclusive scan of one int per thread across a workgroup of 256 threads; `total` is their sum.  sm: 4 ints
__device__ __forceinline__ int block_excl_scan_256(int v, int* sm, int& total) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  __syncthreads();
  if (lane == 63) sm[wid] = inc;
  __syncthreads();
  int pre = 0;
  for (int i = 0; i < wid; ++i) pre += sm[i];
  total = sm[0] + sm[1] + sm[2] + sm[3];
  return pre + inc - v;
}

// in place: the exclusive prefix sums of one digit's nblk counts (workgroup order), and the digit's total; the scatter adds the totals of
// the lower digits itself.  A thread takes 4 consecutive counts of a 1024-count chunk.  grid: (256 digits, S)
__global__ __launch_bounds__(256) void sort_scan_kernel(int* __restrict__ hist, int nblk, int* __restrict__ tot) {
  __shared__ int sm[4];
  const i64 row = (i64)blockIdx.y * 256 + blockIdx.x;
  int* hp = hist + row * nblk;
  int carry = 0;
  for (int c0 = 0; c0 < nblk; c0 += 1024) {
    const int i0 = c0 + (int)threadIdx.x * 4;
    int v[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = i0 + j < nblk ? hp[i0 + j] : 0;
      sum += v[j];
    }
    int total;
    int pre = carry + block_excl_scan_256(sum, sm, total);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j < nblk) hp[i0 + j] = pre;
      pre += v[j];
    }
    carry += total;
  }
  if (threadIdx.x == 0) tot[row] = carry;
}

// A wave owns 1024 consecutive elements of the workgroup's tile, 64 at a time.  An element's place among the tile's elements of its digit:
// those in earlier waves (phase 2), those in earlier rounds of its wave (the wave's LDS counter), those in lower lanes of its round (ballots).
// The tile is first ordered by digit in LDS (phase 3), then stored (phase 4): consecutive threads store consecutive elements of a digit's
// run, so a wave instruction writes a few contiguous pieces instead of up to 64 single words.
// IDENT: the value is the element's index in its segment.  grid: (nblk, S)
template <bool IDENT>
__global__ __launch_bounds__(256) void sort_scatter_kernel(const unsigned* __restrict__ kin, const unsigned* __restrict__ vin,
                                                           unsigned* __restrict__ kout, unsigned* __restrict__ vout, i64 stride,
                                                           const int* __restrict__ seg_len, int L, int shift, int nblk,
                                                           const int* __restrict__ hist, const int* __restrict__ tot) {
  __shared__ int cnt[4][256];
  __shared__ int lbase[4][256];     // place in the ordered tile of wave w's first element of digit d
  __shared__ int gofs[256];         // a digit's place in the segment minus its place in the ordered tile
  __shared__ unsigned sk[SORT_TILE], sv[SORT_TILE];
  __shared__ int sm[4];
  const int s = blockIdx.y, blk = blockIdx.x, len = seg_length(seg_len, s, L);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < 4 * 256; i += 256) (&cnt[0][0])[i] = 0;
  __syncthreads();
  const unsigned* kp = kin + (i64)s * stride;
  const unsigned* vp = IDENT ? nullptr : vin + (i64)s * stride;
  const i64 wbase = (i64)blk * SORT_TILE + wid * (SORT_TILE / 4);
  const unsigned long long below = (1ull << lane) - 1ull;
  volatile int* wc = cnt[wid];
  unsigned key[SORT_ITEMS], val[SORT_ITEMS];
  int rk[SORT_ITEMS];
#pragma unroll
  for (int i = 0; i < SORT_ITEMS; ++i) {
    const i64 idx = wbase + i * 64 + lane;
    const bool ok = idx < len;
    key[i] = ok ? kp[idx] : 0u;
    val[i] = ok ? (IDENT ? (unsigned)idx : vp[idx]) : 0u;
    const unsigned d = (key[i] >> shift) & 255u;
    unsigned long long peers = __ballot(ok);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(ok && bit);
      peers &= bit ? m : ~m;
    }
    const int leader = ok ? __ffsll((long long)peers) - 1 : lane;        // (an element is its own peer: peers != 0 where ok)
    int old = 0;
    if (ok && lane == leader) {
      old = wc[d];
      wc[d] = old + __popcll(peers);
    }
    old = __shfl(old, leader, 64);
    rk[i] = old + __popcll(peers & below);
  }
  __syncthreads();
  {
    // thread d: the tile's digits ahead of d (their place in the ordered tile); the segment's elements of lower digits + those of digit d
    // in earlier workgroups (their place in the segment)
    const int d = threadIdx.x;
    const int c0 = cnt[0][d], c1 = cnt[1][d], c2 = cnt[2][d], c3 = cnt[3][d];
    int total;
    const int lex = block_excl_scan_256(c0 + c1 + c2 + c3, sm, total);
    const int gex = block_excl_scan_256(tot[(i64)s * 256 + d], sm, total) + hist[((i64)s * 256 + d) * nblk + blk];
    lbase[0][d] = lex;
    lbase[1][d] = lex + c0;
    lbase[2][d] = lex + c0 + c1;
    lbase[3][d] = lex + c0 + c1 + c2;
    gofs[d] = gex - lex;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < SORT_ITEMS; ++i) {
    const i64 idx = wbase + i * 64 + lane;
    if (idx < len) {
      const int at = lbase[wid][(key[i] >> shift) & 255u] + rk[i];
      if ((unsigned)at < (unsigned)SORT_TILE) {        // always true for consistent counts
        sk[at] = key[i];
        sv[at] = val[i];
      }
    }
  }
  __syncthreads();
  const i64 left = (i64)len - (i64)blk * SORT_TILE;
  const int here = left < 0 ? 0 : left > SORT_TILE ? SORT_TILE : (int)left;      // the tile's elements inside the segment
  unsigned* ko = kout + (i64)s * stride;
  unsigned* vo = vout + (i64)s * stride;
#pragma unroll 4
  for (int i = 0; i < SORT_ITEMS; ++i) {
    const int j = i * 256 + (int)threadIdx.x;
    if (j < here) {
      const unsigned k = sk[j];
      const int o = gofs[(k >> shift) & 255u] + j;
      if ((unsigned)o < (unsigned)len) {             // always true for consistent counts; never store outside the segment
        ko[o] = k;
        vo[o] = sv[j];
      }
    }
  }
}

// 4 passes over 32-bit keys: in -> tmp -> out -> tmp -> out (in == out is fine: `in` is dead after the first pass)
void sort_launch(const unsigned* kin, const unsigned* vin, unsigned* kout, unsigned* vout, unsigned* ktmp, unsigned* vtmp, int* hist, int* tot,
                 int S, i64 stride, int L, const int* seg_len, hipStream_t s) {
  const int nblk = cdiv(L, SORT_TILE);
  const dim3 grid(nblk, S);
  for (int pass = 0; pass < 4; ++pass) {
    const unsigned* ki = pass == 0 ? kin : (pass & 1) ? ktmp : kout;
    const unsigned* vi = pass == 0 ? vin : (pass & 1) ? vtmp : vout;
    unsigned* ko = (pass & 1) ? kout : ktmp;
    unsigned* vo = (pass & 1) ? vout : vtmp;
    hipLaunchKernelGGL(sort_hist_kernel, grid, dim3(256), 0, s, ki, stride, seg_len, L, 8 * pass, nblk, hist);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(256, S), dim3(256), 0, s, hist, nblk, tot);
    if (vi)
      hipLaunchKernelGGL(sort_scatter_kernel<false>, grid, dim3(256), 0, s, ki, vi, ko, vo, stride, seg_len, L, 8 * pass, nblk, hist, tot);
    else
      hipLaunchKernelGGL(sort_scatter_kernel<true>, grid, dim3(256), 0, s, ki, vi, ko, vo, stride, seg_len, L, 8 * pass, nblk, hist, tot);
  }
}

struct LovaszWs {
  unsigned *kA, *vA, *kB, *vB;
  int *hist, *tot, *bcount;
  double* partial;
  size_t bytes;
};
inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
LovaszWs lovasz_ws(void* base, i64 S, i64 stride) {
  const size_t nblk = (size_t)cdiv(stride, SORT_TILE), kv = up16(sizeof(unsigned) * (size_t)S * (size_t)stride);
  char* p = static_cast<char*>(base);
  LovaszWs w;
  size_t off = 0;
  w.kA = reinterpret_cast<unsigned*>(p + off); off += kv;
  w.vA = reinterpret_cast<unsigned*>(p + off); off += kv;
  w.kB = reinterpret_cast<unsigned*>(p + off); off += kv;
  w.vB = reinterpret_cast<unsigned*>(p + off); off += kv;
  w.partial = reinterpret_cast<double*>(p + off); off += up16(sizeof(double) * (size_t)S * nblk);
  w.hist = reinterpret_cast<int*>(p + off); off += up16(sizeof(int) * (size_t)S * 256 * nblk);
  w.tot = reinterpret_cast<int*>(p + off); off += up16(sizeof(int) * (size_t)S * 256);
  w.bcount = reinterpret_cast<int*>(p + off); off += up16(sizeof(int) * (size_t)S * nblk);
  w.bytes = off;
  return w;
}

// -------------------------------------------------------------------------------------------------------------------- gradient
// bcount[s][workgroup]: the foreground flags in a tile of the sorted order.  grid: (nblk, S)
__global__ __launch_bounds__(256) void lovasz_fgcount_kernel(const unsigned* __restrict__ vals, int L, int nblk, int* __restrict__ bcount) {
  __shared__ int sm[4];
  const int s = blockIdx.y, blk = blockIdx.x;
  const unsigned* vp = vals + (i64)s * L;
  int c = 0;
#pragma unroll 4
  for (int i = 0; i < SORT_ITEMS; ++i) {
    const i64 idx = (i64)blk * SORT_TILE + i * 256 + threadIdx.x;
    if (idx < L) c += (int)(vp[idx] >> 31);
  }
  c = wave_sum_i(c);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) bcount[(i64)s * nblk + blk] = sm[0] + sm[1] + sm[2] + sm[3];
}

// Position k (1-based) of a segment's sorted order, cum = the inclusive count of foreground flags up to k, G the segment's foreground count:
//   I = G - cum, U = G + k - cum, J_k = 1 - I / U, g_k = J_k - J_{k-1}, J_0 = 0, J_{k-1} from cum - fg_k.
// A foreground element leaves U and lowers I by one, a background one leaves I and raises U by one, so for k > 1 the difference is
// g_k = fg ? 1 / U : I / (U (U - 1)) -- exact integers below 2^53 and one division, no cancellation.  U >= 1 always (G = 0 under 'all').
// grid: (nblk, S)
__global__ __launch_bounds__(256) void lovasz_grad_kernel(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals, int L, int nblk,
                                                          int N, int K, i64 HW, int per_image, const unsigned long long* __restrict__ cnt,
                                                          const float* __restrict__ cw, const int* __restrict__ bcount,
                                                          float* __restrict__ map, double* __restrict__ partial) {
  __shared__ int wc[SORT_ITEMS][4], wp[SORT_ITEMS][4];
  __shared__ long long sG, sPre;
  __shared__ int spre[4];
  __shared__ double sd[4];
  const int s = blockIdx.y, blk = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned* kp = keys + (i64)s * L;
  const unsigned* vp = vals + (i64)s * L;
  // the foreground flags ahead of this tile (integers: any order), and the segment's G
  int pre = 0;
  for (int i = threadIdx.x; i < blk; i += 256) pre += bcount[(i64)s * nblk + i];
  pre = wave_sum_i(pre);
  if (lane == 0) spre[wid] = pre;
  if (threadIdx.x == 0) {
    unsigned long long g = 0;
    if (per_image) {
      g = cnt[3 + s];
    } else {
      for (int n = 0; n < N; ++n) g += cnt[3 + (i64)n * K + s];
    }
    sG = (long long)g;
  }
  unsigned key[SORT_ITEMS], val[SORT_ITEMS];
  int lower[SORT_ITEMS];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int i = 0; i < SORT_ITEMS; ++i) {
    const i64 idx = (i64)blk * SORT_TILE + i * 256 + threadIdx.x;
    const bool ok = idx < L;
    key[i] = ok ? kp[idx] : LOVASZ_INVALID;
    val[i] = ok ? vp[idx] : 0u;
    const unsigned long long f = __ballot(ok && (val[i] >> 31));
    lower[i] = __popcll(f & below);
    if (lane == 0) wc[i][wid] = __popcll(f);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < SORT_ITEMS; ++i)
      for (int v = 0; v < 4; ++v) {
        wp[i][v] = run;
        run += wc[i][v];
      }
    sPre = (long long)spre[0] + spre[1] + spre[2] + spre[3];
  }
  __syncthreads();
  const long long G = sG, tile_pre = sPre;
  const int k_slot = per_image ? s % K : s;
  const float w = cw ? cw[k_slot] : 1.f;
  const i64 total = per_image ? HW : (i64)N * HW;
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < SORT_ITEMS; ++i) {
    if (key[i] <= LOVASZ_ONE) {                    // a valid pixel (the tail beyond L carries LOVASZ_INVALID as well)
      const long long k = (i64)blk * SORT_TILE + i * 256 + threadIdx.x + 1;
      const int fg = (int)(val[i] >> 31);
      const long long cum = tile_pre + wp[i][wid] + lower[i] + fg;
      const long long I = G - cum, U = G + k - cum;
      double g;
      if (k == 1) g = 1.0 - (double)I / (double)U;
      else g = fg ? 1.0 / (double)U : (double)I / ((double)U * (double)(U - 1));
      const float e = __uint_as_float(LOVASZ_ONE - key[i]);
      acc += (double)e * g;
      const i64 idx = (i64)(val[i] & 0x7FFFFFFFu);
      if (idx < total) {                           // always true for values the key pass wrote
        i64 at;
        if (per_image) {
          at = (i64)s * HW + idx;
        } else {
          const i64 n = idx / HW;
          at = (n * K + s) * HW + (idx - n * HW);
        }
        const float gw = (float)g * w;
        map[at] = e == 0.f ? 0.f : (fg ? gw : -gw);     // d|fg - p|/dp = -sign(fg - p), sign(0) = 0: stored as dL/d(fg - p) -> see the backward
      }
    }
  }
  acc = wave_sum_d(acc);
  if (lane == 0) sd[wid] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(i64)s * nblk + blk] = ((sd[0] + sd[1]) + sd[2]) + sd[3];
}

// One workgroup of 16 waves.  Phase 1: a wave per segment adds its nblk partials (lane l takes l, l + 64, ... in order, then the shuffle tree).
// Phase 2 (thread 0): the present mask, the class mean per image or per batch, the reduction, and the backward's scale block.
// mode_present: a class with no foreground among the segment's valid pixels is skipped.  reduction (per_image only): 0 mean (and 'none',
// logged as its mean), 1 sum.
__global__ __launch_bounds__(1024) void lovasz_finalize_kernel(const double* __restrict__ partial, int nblk, const unsigned long long* __restrict__ cnt,
                                                               int N, int K, int per_image, int mode_present, int reduction,
                                                               const float* __restrict__ cw, double loss_weight, double* __restrict__ sums,
                                                               float* __restrict__ scale, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int S = per_image ? N * K : K;
  for (int s = wid; s < S; s += 16) {
    double a = 0.0;
    for (int k = lane; k < nblk; k += 64) a += partial[(i64)s * nblk + k];
    a = wave_sum_d(a);
    if (lane == 0) sums[s] = a;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
  const int groups = per_image ? N : 1;
  const double rscale = per_image && reduction == 0 ? 1.0 / (double)N : 1.0;
  for (int g = 0; g < groups; ++g) {
    int kept = 0;
    double v = 0.0;
    for (int k = 0; k < K; ++k) {
      unsigned long long G = 0;
      if (per_image) {
        G = cnt[3 + (i64)g * K + k];
      } else {
        for (int n = 0; n < N; ++n) G += cnt[3 + (i64)n * K + k];
      }
      const bool present = !mode_present || G > 0;
      if (present) {
        kept += 1;
        v += (cw ? (double)cw[k] : 1.0) * sums[g * K + k];
      }
      const float m = present ? 1.f : 0.f;
      if (per_image) {
        scale[g * K + k] = m;
      } else {
        for (int n = 0; n < N; ++n) scale[n * K + k] = m;
      }
    }
    const double f = kept ? rscale / (double)kept : 0.0;
    total += v * f;
    if (per_image) {
      for (int k = 0; k < K; ++k) scale[g * K + k] *= (float)f;
    } else {
      for (int i = 0; i < N * K; ++i) scale[i] *= (float)f;
    }
  }
  const double eps = 1.1920928955078125e-07;     // torch.finfo(float32).eps, as ce_finalize_kernel
  out[0] = (float)(loss_weight * total);
  out[1] = (float)(((double)cnt[0] + eps) * (100.0 / ((double)cnt[1] + eps)));
  out[2] = (float)cnt[2];
}

// -------------------------------------------------------------------------------------------------------------------- backward
// L = sum_c sum_k e_k g_k with e = |fg - p_c|: dL/dp_c = -sign(fg - p_c) g.  The map holds m = sign(fg - p_c) cw g, so d_c = -scale m.
// All classes (C <= 8) for bwd_blocks_walk and bwd_cells_gather; a pixel under ignore_index adds nothing.
struct LovaszBwdPx {
  const float* __restrict__ ls;
  const float* __restrict__ map;    // the image's plane of slot 0
  i64 HW;
  int C, ign;
  const int (&slot)[8];
  const float (&sc)[8];
  float (&pc)[8], (&d)[8], (&mx)[8], (&my)[8];
  float2 ls2;
  float s;
  __device__ __forceinline__ void pair(i64 p) {
    ls2 = *reinterpret_cast<const float2*>(ls + p);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C && slot[c] >= 0) {
        const float2 m = *reinterpret_cast<const float2*>(map + (i64)slot[c] * HW + p);
        mx[c] = m.x;
        my[c] = m.y;
      }
    }
  }
  template <class Z>
  __device__ __forceinline__ void softmax(float lsp, const Z& z, const float (&m)[8]) {
    s = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c < C) {
        pc[c] = lovasz_prob(z(c) - lsp);
        d[c] = slot[c] >= 0 ? -sc[c] * m[c] : 0.f;
        s = fmaf(d[c], pc[c], s);
      }
    }
  }
  __device__ __forceinline__ bool skip(int, int l) const { return l == ign; }
  __device__ __forceinline__ bool cell_skip(int, int l) const { return l == ign; }
  template <class Z>
  __device__ __forceinline__ float weight(int k, int, const Z& z) {
    if (k) softmax(ls2.y, z, my);
    else softmax(ls2.x, z, mx);
    return 1.f;
  }
  template <class Z>
  __device__ __forceinline__ float cell_weight(int p, int, const Z& z) {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < C && slot[c] >= 0) mx[c] = map[(i64)slot[c] * HW + p];
    softmax(ls[p], z, mx);
    return 1.f;
  }
  template <class Z>
  __device__ __forceinline__ float term(int c, const Z&) const { return pc[c] * (d[c] - s); }
};

__device__ __forceinline__ void load_scales(const float* __restrict__ scale, i64 n, int K, const int (&sl)[8], float (&sc)[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) sc[c] = sl[c] >= 0 ? scale[n * K + sl[c]] : 0.f;
}

// grid: bwd_blocks_grid, 16 x 16 threads
template <int S>
__global__ __launch_bounds__(256) void lovasz_bwd_blocks_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                                const unsigned char* __restrict__ label, int ign, const int* __restrict__ slot,
                                                                int K, const float* __restrict__ lse, const float* __restrict__ map,
                                                                const float* __restrict__ scale, float gscale, float* __restrict__ dlogits,
                                                                int accumulate) {
  const i64 n = blockIdx.z, HW = (i64)S * h * S * w, img = n * C * h * w;
  int sl[8];
  float sc[8], pc[8], d[8], mx[8], my[8];
  load_slots(slot, C, K, sl);
  load_scales(scale, n, K, sl, sc);
#pragma unroll
  for (int c = 0; c < 8; ++c) mx[c] = my[c] = 0.f;
  LovaszBwdPx px{lse + n * HW, map + n * K * HW, HW, C, ign, sl, sc, pc, d, mx, my};
  bwd_blocks_walk<S>(logits + img, C, h, w, label + n * HW, gscale, dlogits + img, accumulate, px);
}

// ONE thread per low-resolution cell for all classes (C <= 8).  grid: (blocks over h*w, 1, N)
__global__ __launch_bounds__(256) void lovasz_bwd_cells_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                               const unsigned char* __restrict__ label, int H, int W, int ign, float sh, float sw,
                                                               const int* __restrict__ slot, int K, const float* __restrict__ lse,
                                                               const float* __restrict__ map, const float* __restrict__ scale, float gscale,
                                                               float* __restrict__ dlogits, int accumulate) {
  const i64 n = blockIdx.z, HW = (i64)H * W, img = n * C * h * w;
  int sl[8];
  float sc[8], pc[8], d[8], mx[8], my[8];
  load_slots(slot, C, K, sl);
  load_scales(scale, n, K, sl, sc);
#pragma unroll
  for (int c = 0; c < 8; ++c) mx[c] = my[c] = 0.f;
  LovaszBwdPx px{lse + n * HW, map + n * K * HW, HW, C, ign, sl, sc, pc, d, mx, my};
  bwd_cells_gather(logits + img, C, h, w, label + n * HW, H, W, sh, sw, gscale, dlogits + img, accumulate, px);
}

// C > 8: s[p] = sum_c d_c p_c of every valid full-resolution pixel, over the class set (cls[k]: the class of slot k).  grid: (blocks, N)
__global__ __launch_bounds__(256) void lovasz_s_kernel(const float* __restrict__ logits, int C, int h, int w, const unsigned char* __restrict__ label,
                                                       int H, int W, int ign, float sh, float sw, const int* __restrict__ cls, int K,
                                                       const float* __restrict__ lse, const float* __restrict__ map,
                                                       const float* __restrict__ scale, float* __restrict__ s_out) {
  const int n = blockIdx.y, hw = h * w;
  const i64 HW = (i64)H * W;
  const float* lp = logits + (i64)n * C * hw;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < H * W; p += gridDim.x * blockDim.x) {
    float s = 0.f;
    if (label[n * HW + p] != ign) {
      const int oy = p / W, ox = p - oy * W;
      const Bilin b = make_bilin(oy, ox, sh, sw, h, w);
      const float lsp = lse[n * HW + p];
      for (int k = 0; k < K; ++k) {
        const int c = cls[k];
        if (c < 0 || c >= C) continue;
        const float pc = lovasz_prob(interp(lp + (i64)c * hw, w, b) - lsp);
        s = fmaf(-scale[(i64)n * K + k] * map[((i64)n * K + k) * HW + p], pc, s);
      }
    }
    s_out[n * HW + p] = s;
  }
}

// one class for bwd_class_gather: p_c (d_c - s)
struct LovaszClassPx {
  const float* __restrict__ ls;
  const float* __restrict__ sp;
  const float* __restrict__ map;    // this class's plane of the image, or null: the class is not in the class set
  int ign;
  float sc;
  float d;
  __device__ __forceinline__ bool cell_skip(int, int l) const { return l == ign; }
  template <class Z>
  __device__ __forceinline__ float cell_weight(int p, int, const Z& z) {
    const float pc = lovasz_prob(z(0) - ls[p]);
    d = pc * ((map ? -sc * map[p] : 0.f) - sp[p]);
    return 1.f;
  }
  template <class Z>
  __device__ __forceinline__ float term(int, const Z&) const { return d; }
};

// grid: (blocks over h*w, C, N)
__global__ __launch_bounds__(256) void lovasz_bwd_class_kernel(const float* __restrict__ logits, int C, int h, int w,
                                                               const unsigned char* __restrict__ label, int H, int W, int ign, float sh, float sw,
                                                               const int* __restrict__ slot, int K, const float* __restrict__ lse,
                                                               const float* __restrict__ map, const float* __restrict__ scale,
                                                               const float* __restrict__ s_in, float gscale, float* __restrict__ dlogits,
                                                               int accumulate) {
  const int c = blockIdx.y;
  const i64 n = blockIdx.z, HW = (i64)H * W, plane = (n * C + c) * h * w;
  const int s = slot[c];
  const bool in = s >= 0 && s < K;
  LovaszClassPx px{lse + n * HW, s_in + n * HW, in ? map + (n * K + s) * HW : nullptr, ign, in ? scale[n * K + s] : 0.f, 0.f};
  bwd_class_gather(logits + plane, h, w, label + n * HW, H, W, sh, sw, gscale, dlogits + plane, accumulate, px);
}

}  // namespace

extern "C" int pfst_lovasz_workspace_bytes(int segments, long long seg_stride, long long* bytes) {
  PFST_CHECK_ARG(bytes && segments > 0 && segments <= 65535 && seg_stride > 0 && seg_stride <= INT_MAX - SORT_TILE);
  *bytes = (long long)lovasz_ws(nullptr, segments, seg_stride).bytes;
  return PFST_OK;
}

extern "C" int pfst_lovasz_sort(const unsigned int* keys_in, const unsigned int* vals_in, int segments, long long seg_stride, const int* seg_len,
                                void* workspace, unsigned int* keys_out, unsigned int* vals_out, pfst_stream_t stream) {
  PFST_CHECK_ARG(keys_in && keys_out && vals_out && workspace && ((uintptr_t)workspace & 15) == 0);
  PFST_CHECK_ARG(segments > 0 && segments <= 65535 && seg_stride > 0 && seg_stride <= INT_MAX - SORT_TILE);
  const LovaszWs ws = lovasz_ws(workspace, segments, seg_stride);
  sort_launch(keys_in, vals_in, keys_out, vals_out, ws.kB, ws.vB, ws.hist, ws.tot, segments, seg_stride, (int)seg_stride, seg_len, (hipStream_t)stream);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_lovasz_keys(const float* logits, int N, int C, int h, int w, const unsigned char* label, int H, int W, int ignore_index,
                                int form, const int* slot, int K, int per_image, const float* lse_in, float* lse_out, void* workspace,
                                long long* counters, pfst_stream_t stream) {
  PFST_CHECK_ARG(logits && label && slot && workspace && counters && N > 0 && C > 0 && C <= 255 && h > 0 && w > 0 && H > 0 && W > 0 && N <= 65535);
  PFST_CHECK_ARG((lse_in != nullptr) != (lse_out != nullptr) && K > 0 && K <= C && (i64)N * H * W < INT_MAX - SORT_TILE && (i64)N * K <= 65535);
  PFST_CHECK_ARG(((uintptr_t)workspace & 15) == 0);
  const void* lse = lse_in ? (const void*)lse_in : (const void*)lse_out;
  PFST_CHECK_ARG(form == 0 || blocks_form_ok(form, C, h, w, H, W, label, (uintptr_t)lse));
  hipStream_t s = (hipStream_t)stream;
  const i64 HW = (i64)H * W, L = per_image ? HW : (i64)N * HW;
  const int S = per_image ? N * K : K;
  const LovaszWs ws = lovasz_ws(workspace, S, L);
  const i64 sn = per_image ? (i64)K * HW : HW, sk = per_image ? HW : (i64)N * HW;
  if (hipMemsetAsync(counters, 0, sizeof(long long) * (3 + (size_t)N * K), s) != hipSuccess) {
    pfst_set_error(__FILE__, __LINE__, "hipMemsetAsync failed");
    return PFST_ERR_LAUNCH;
  }
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counters);
  if (form == 0) {
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    hipLaunchKernelGGL(lovasz_keys_kernel, dim3(cdiv(HW, 256 * GPIX), N), dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, sh, sw,
                       slot, K, sn, sk, per_image, lse_in, lse_out, ws.kA, ws.vA, cnt);
  } else {
    const dim3 grid = fwd_blocks_grid(form, h, w, N);
    if (form == 4)
      hipLaunchKernelGGL((lovasz_keys_blocks_kernel<4, 2>), grid, dim3(256), 0, s, logits, C, h, w, label, ignore_index, slot, K, sn, sk,
                         per_image, lse_in, lse_out, ws.kA, ws.vA, cnt);
    else
      hipLaunchKernelGGL((lovasz_keys_blocks_kernel<8, 1>), grid, dim3(256), 0, s, logits, C, h, w, label, ignore_index, slot, K, sn, sk,
                         per_image, lse_in, lse_out, ws.kA, ws.vA, cnt);
  }
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_lovasz_sort_keys(int N, int H, int W, int K, int per_image, void* workspace, pfst_stream_t stream) {
  PFST_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && N > 0 && H > 0 && W > 0 && K > 0 && (i64)N * H * W < INT_MAX - SORT_TILE && (i64)N * K <= 65535);
  const i64 HW = (i64)H * W, L = per_image ? HW : (i64)N * HW;
  const int S = per_image ? N * K : K;
  const LovaszWs ws = lovasz_ws(workspace, S, L);
  sort_launch(ws.kA, ws.vA, ws.kA, ws.vA, ws.kB, ws.vB, ws.hist, ws.tot, S, L, (int)L, nullptr, (hipStream_t)stream);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_lovasz_grad(int N, int H, int W, int K, int per_image, const long long* counters, const float* slot_weight, void* workspace,
                                float* coef_map, pfst_stream_t stream) {
  PFST_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && counters && coef_map && N > 0 && H > 0 && W > 0 && K > 0);
  PFST_CHECK_ARG((i64)N * H * W < INT_MAX - SORT_TILE && (i64)N * K <= 65535);
  hipStream_t s = (hipStream_t)stream;
  const i64 HW = (i64)H * W, L = per_image ? HW : (i64)N * HW;
  const int S = per_image ? N * K : K, nblk = cdiv(L, SORT_TILE);
  const LovaszWs ws = lovasz_ws(workspace, S, L);
  const unsigned long long* cnt = reinterpret_cast<const unsigned long long*>(counters);
  hipLaunchKernelGGL(lovasz_fgcount_kernel, dim3(nblk, S), dim3(256), 0, s, ws.vA, (int)L, nblk, ws.bcount);
  hipLaunchKernelGGL(lovasz_grad_kernel, dim3(nblk, S), dim3(256), 0, s, ws.kA, ws.vA, (int)L, nblk, N, K, HW, per_image, cnt, slot_weight,
                     ws.bcount, coef_map, ws.partial);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_lovasz_finalize(int N, int H, int W, int K, int per_image, int mode_present, int reduction, const long long* counters,
                                    const float* slot_weight, double loss_weight, void* workspace, double* sums, float* scale, float* out,
                                    pfst_stream_t stream) {
  PFST_CHECK_ARG(workspace && ((uintptr_t)workspace & 15) == 0 && counters && sums && scale && out && N > 0 && H > 0 && W > 0 && K > 0);
  PFST_CHECK_ARG((i64)N * H * W < INT_MAX - SORT_TILE && (i64)N * K <= 65535 && (reduction == 0 || reduction == 1));
  const i64 HW = (i64)H * W, L = per_image ? HW : (i64)N * HW;
  const int S = per_image ? N * K : K, nblk = cdiv(L, SORT_TILE);
  const LovaszWs ws = lovasz_ws(workspace, S, L);
  hipLaunchKernelGGL(lovasz_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, ws.partial, nblk,
                     reinterpret_cast<const unsigned long long*>(counters), N, K, per_image, mode_present, reduction, slot_weight, loss_weight,
                     sums, scale, out);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_lovasz_upsample_bwd(const float* logits, int N, int C, int h, int w, const unsigned char* label, int H, int W,
                                        int ignore_index, int form, const int* slot, const int* cls, int K, const float* lse,
                                        const float* coef_map, const float* scale, float grad_scale, float* work, float* dlogits,
                                        int accumulate, pfst_stream_t stream) {
  PFST_CHECK_ARG(logits && label && slot && cls && lse && coef_map && scale && dlogits && N > 0 && C > 0 && C <= 255 && h > 0 && w > 0 && H > 0 && W > 0);
  PFST_CHECK_ARG(N <= 65535 && K > 0 && K <= C && (i64)N * H * W < INT_MAX - SORT_TILE && ((uintptr_t)coef_map & 7) == 0);
  PFST_CHECK_ARG((form == 0 || blocks_form_ok(form, C, h, w, H, W, label, (uintptr_t)lse)) && (form != 0 || C <= 8 || work));
  hipStream_t s = (hipStream_t)stream;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  const int gx = cdiv((i64)h * w, 256);
  if (form != 0) {
    const dim3 grid = bwd_blocks_grid(h, w, N);
    if (form == 4)
      hipLaunchKernelGGL(lovasz_bwd_blocks_kernel<4>, grid, dim3(256), 0, s, logits, C, h, w, label, ignore_index, slot, K, lse, coef_map, scale,
                         grad_scale, dlogits, accumulate);
    else
      hipLaunchKernelGGL(lovasz_bwd_blocks_kernel<8>, grid, dim3(256), 0, s, logits, C, h, w, label, ignore_index, slot, K, lse, coef_map, scale,
                         grad_scale, dlogits, accumulate);
  } else if (C <= 8) {
    hipLaunchKernelGGL(lovasz_bwd_cells_kernel, dim3(gx, 1, N), dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, sh, sw, slot, K, lse,
                       coef_map, scale, grad_scale, dlogits, accumulate);
  } else {
    hipLaunchKernelGGL(lovasz_s_kernel, dim3(px_blocks((i64)H * W), N), dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, sh, sw, cls,
                       K, lse, coef_map, scale, work);
    hipLaunchKernelGGL(lovasz_bwd_class_kernel, dim3(gx, C, N), dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, sh, sw, slot, K, lse,
                       coef_map, scale, work, grad_scale, dlogits, accumulate);
  }
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
