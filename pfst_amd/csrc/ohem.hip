// OHEMPixelSampler (rsiseg/core/seg/sampler/ohem_pixel_sampler.py): the 0/1 pixel-weight map of online hard example
// mining, from the LOW-resolution logits, without the reference's full-resolution softmax and global sort and without a host read.
//
//   key pass     one thread per full-resolution pixel interpolates its C logits (bilin.h, the CE kernels' class order) and writes the pixel's
//                KEY into the [N][H][W] float map that becomes the weight map: with a threshold p_label = exp(z_y - max) / sum (torch's softmax
//                arithmetic), without one coef[y] * max(lse - z_y, 0), the head's unreduced CE.  A pixel whose label is the ignore index or lies
//                outside [0, C) gets the sentinel -1.  The pass counts the valid pixels, and those with p <= thresh.
//   select       keys are >= +0, so the unsigned order of their 31 low bits is their order as values: an exact radix select in three levels of
//                11 + 10 + 10 bits.  A level is a histogram pass over the key map (restricted to the prefix found so far) and a one-workgroup
//                kernel that scans the table, picks the digit that holds the wanted rank and updates prefix and rank in the STATE block on the
//                device.  The rank itself is formed on the device from the counts of the key pass.
//   weight pass  key -> 0/1 in place.  With a threshold: valid and key < max(s[k], thresh).  Without: the min(batch_kept, n_valid) largest keys;
//                pixels equal to the cut value are kept in raster order (n, y, x) until the count is exact -- per-workgroup tie counts over
//                fixed contiguous chunks, an exclusive scan across the workgroups, a scan inside the workgroup; no ticket counters.
//
// All counting is in integers, so the map does not depend on launch, wave or stream order; nothing is read on the host.  The file is compiled
// with contraction off (entropy_labels.hip explains why): a key has the same bits wherever it is formed.
#include <limits.h>
#include "common.h"
#include "bilin.h"
#include "../../include/pfst_hip.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int REG_C = 8;                      // classes the register form holds per thread
constexpr int L0_BITS = 11, L1_BITS = 10, L2_BITS = 10;
constexpr int HIST_MAX = 1 << L0_BITS;        // entries of the largest level
constexpr int MAX_CHUNKS = 2048;              // workgroups of the tie-count / weight passes (one contiguous chunk of the map each)
constexpr unsigned int KEY_INF = 0x7f800000u;

// the state block: 64-bit words at the head of the workspace
enum {
  ST_NVALID = 0,   // valid pixels
  ST_NLE,          // valid pixels with p <= thresh (threshold mode)
  ST_DONE,         // 1: the cut is known without a select (early-out, or nothing to select from): the level kernels return at once
  ST_RANK,         // ascending 0-based rank wanted among the keys that share ST_PREFIX
  ST_PREFIX,       // the key's high bits found so far
  ST_CUT,          // bit pattern of the threshold (threshold mode) / the cut value (top-k mode)
  ST_TIE_MODE,     // top-k mode, pixels equal to the cut: 0 none kept, 1 all kept, 2 the first ST_TIE_TAKE in raster order
  ST_TIE_TAKE,
  ST_WORDS = 16
};
constexpr size_t HIST_OFF = ST_WORDS * sizeof(u64);
constexpr size_t TIECNT_OFF = HIST_OFF + HIST_MAX * sizeof(u64);            // unsigned int [MAX_CHUNKS]
constexpr size_t TIEBASE_OFF = TIECNT_OFF + MAX_CHUNKS * sizeof(unsigned int);   // u64 [MAX_CHUNKS]
constexpr size_t WS_BYTES = TIEBASE_OFF + MAX_CHUNKS * sizeof(u64);

// sum of v over the 256 threads of the workgroup, valid in every thread
__device__ __forceinline__ unsigned int block_count(unsigned int v, unsigned int* sm /* >= 4 */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}

// exclusive prefix sum of v over the 256 threads (thread order)
__device__ __forceinline__ u64 block_excl_scan(u64 v, u64* sm /* >= 256 */) {
  const int t = threadIdx.x;
  sm[t] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const u64 add = t >= o ? sm[t - o] : 0;
    __syncthreads();
    sm[t] += add;
    __syncthreads();
  }
  return sm[t] - v;
}

// REG: C <= 8, the pixel's logits in registers; else the classes are walked twice and interpolated again, as px_eval of entropy_labels.hip
// does.  The arithmetic per class is the same in both forms, in the same order.  lab < C.
template <bool REG>
__device__ __forceinline__ float px_key(const float* __restrict__ lp, int C, int hw, int w, const Bilin& b, int lab, bool has_thresh,
                                        const float* __restrict__ coef) {
  float mx = -INFINITY, se = 0.f, zl = 0.f;
  if (REG) {
    float z[REG_C];
#pragma unroll
    for (int c = 0; c < REG_C; ++c) {
      z[c] = c < C ? interp(lp + (i64)c * hw, w, b) : -INFINITY;
      if (c < C && z[c] > mx) mx = z[c];
      if (c == lab) zl = z[c];
    }
#pragma unroll
    for (int c = 0; c < REG_C; ++c)
      if (c < C) se = se + expf(z[c] - mx);
  } else {
    for (int c = 0; c < C; ++c) {
      const float z = interp(lp + (i64)c * hw, w, b);
      if (z > mx) mx = z;
      if (c == lab) zl = z;
    }
    for (int c = 0; c < C; ++c) se = se + expf(interp(lp + (i64)c * hw, w, b) - mx);
  }
  float key;
  if (has_thresh) {
    key = expf(zl - mx) / se;
  } else {
    const float nll = (mx + logf(se)) - zl;
    key = coef[lab] * (nll > 0.f ? nll : 0.f);
  }
  return key >= 0.f ? key : __uint_as_float(KEY_INF);      // a NaN (non-finite logits) ranks above everything, as torch's sort has it
}

// grid: (blocks over H*W, N)
template <bool REG>
__global__ __launch_bounds__(256) void ohem_key_kernel(const float* __restrict__ logits, int C, int h, int w, const unsigned char* __restrict__ label,
                                                       int H, int W, int ignore, float sh, float sw, int has_thresh, float thresh,
                                                       const float* __restrict__ coef, float* __restrict__ keys, u64* __restrict__ st) {
  __shared__ unsigned int sm[4];
  const int n = blockIdx.y, hw = h * w, HW = H * W;
  const float* lp = logits + (i64)n * C * hw;
  unsigned int nvalid = 0, nle = 0;
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
    const int lab = label[(i64)n * HW + p];
    float key = -1.f;
    if (lab != ignore && lab < C) {
      const int oy = p / W, ox = p - oy * W;
      const Bilin b = make_bilin(oy, ox, sh, sw, h, w);
      key = px_key<REG>(lp, C, hw, w, b, lab, has_thresh != 0, coef);
      ++nvalid;
      if (has_thresh && key <= thresh) ++nle;
    }
    keys[(i64)n * HW + p] = key;
  }
  nvalid = block_count(nvalid, sm);
  nle = block_count(nle, sm);
  if (threadIdx.x == 0) {
    if (nvalid) atomicAdd(&st[ST_NVALID], (u64)nvalid);
    if (nle) atomicAdd(&st[ST_NLE], (u64)nle);
  }
}

// one thread: the rank to select, or the cut itself where no select is needed.  info: (cut bits, n_valid, n_kept, k)
__global__ void ohem_plan_kernel(u64* __restrict__ st, long long batch_kept, int has_thresh, float thresh, long long* __restrict__ info) {
  const u64 nv = st[ST_NVALID], bk = (u64)batch_kept;
  u64 k, done = 0, rank = 0, cut = 0;
  if (has_thresh) {
    // s = the ascending sort: threshold = max(s[k], thresh), k = min(batch_kept, n_valid - 1); s[k] <= thresh exactly when at least k + 1
    // keys are <= thresh, and then the threshold is thresh
    k = nv == 0 ? 0 : (bk < nv - 1 ? bk : nv - 1);
    if (nv == 0 || st[ST_NLE] >= k + 1) { done = 1; cut = __float_as_uint(thresh); }
    rank = k;
  } else {
    // the k = min(batch_kept, n_valid) largest: the cut value is the ascending rank n_valid - k
    k = bk < nv ? bk : nv;
    if (k == 0) { done = 1; cut = KEY_INF; }
    rank = nv - k;
  }
  st[ST_DONE] = done;
  st[ST_RANK] = rank;
  st[ST_PREFIX] = 0;
  st[ST_CUT] = cut;
  st[ST_TIE_MODE] = 0;
  st[ST_TIE_TAKE] = 0;
  info[0] = (long long)cut;
  info[1] = (long long)nv;
  info[2] = 0;
  info[3] = (long long)k;
}

// One key into the workgroup's table; every lane of the wave calls this (live = the lane has a key to count).  The top-level digits
// concentrate in a few buckets (every p in [0.5, 1) shares one exponent), where 64 lanes would queue on one LDS counter: up to four rounds of
// "the lanes that share the first live lane's digit add their count once", then the rest go one by one.
__device__ __forceinline__ void hist_add(unsigned int* sm, bool live, unsigned int digit) {
  const int lane = threadIdx.x & 63;
#pragma unroll 1
  for (int r = 0; r < 4; ++r) {
    const u64 act = __ballot(live);
    if (act == 0) return;                                  // the same in every lane
    const int first = __ffsll((long long)act) - 1;
    const unsigned int d = (unsigned int)__shfl((int)digit, first, 64);
    const bool same = live && digit == d;
    const u64 m = __ballot(same);
    if (lane == first) atomicAdd(&sm[d], (unsigned int)__popcll(m));
    live = live && !same;
  }
  if (live) atomicAdd(&sm[digit], 1u);
}

// One radix level: counts digit (key >> SHIFT) & (2^BITS - 1) of the keys whose higher bits equal the prefix found so far (level 0: prefix 0
// over bit 31, which drops the sentinels) in a 32-bit LDS table, and adds the non-zero entries to the global one.      grid: blocks over total / 4
template <int SHIFT, int BITS>
__global__ __launch_bounds__(256) void ohem_hist_kernel(const float* __restrict__ keys, i64 total, const u64* __restrict__ st, u64* __restrict__ hist) {
  __shared__ unsigned int sm[1 << BITS];
  if (st[ST_DONE]) return;
  const unsigned int prefix = (unsigned int)st[ST_PREFIX], mask = (1u << BITS) - 1u;
  for (int i = threadIdx.x; i < (1 << BITS); i += 256) sm[i] = 0u;
  __syncthreads();
  const uint4* kv = reinterpret_cast<const uint4*>(keys);
  const i64 nvec = total >> 2;
  for (i64 base = (i64)blockIdx.x * 256; base < nvec; base += (i64)gridDim.x * 256) {      // whole waves walk the loop: hist_add votes
    const i64 i = base + threadIdx.x;
    const bool in = i < nvec;
    const uint4 v = in ? kv[i] : make_uint4(~0u, ~0u, ~0u, ~0u);
    hist_add(sm, in && (v.x >> (SHIFT + BITS)) == prefix, (v.x >> SHIFT) & mask);
    hist_add(sm, in && (v.y >> (SHIFT + BITS)) == prefix, (v.y >> SHIFT) & mask);
    hist_add(sm, in && (v.z >> (SHIFT + BITS)) == prefix, (v.z >> SHIFT) & mask);
    hist_add(sm, in && (v.w >> (SHIFT + BITS)) == prefix, (v.w >> SHIFT) & mask);
  }
  if (blockIdx.x == 0) {                                                                     // the last total % 4 keys
    const i64 i = (nvec << 2) + threadIdx.x;
    const bool in = i < total;
    const unsigned int k = in ? __float_as_uint(keys[i]) : ~0u;
    hist_add(sm, in && (k >> (SHIFT + BITS)) == prefix, (k >> SHIFT) & mask);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < (1 << BITS); i += 256) {
    const unsigned int v = sm[i];
    if (v) atomicAdd(&hist[i], (u64)v);
  }
}

// One workgroup: scans the level's table, finds the digit that holds the wanted rank, extends the prefix, leaves the rank inside that digit and
// clears the table for the next level.  LAST: the prefix is the whole key -- the cut; in top-k mode the digit's count is the number of pixels
// equal to the cut, of which count - rank are kept.
template <int BITS, bool LAST>
__global__ __launch_bounds__(256) void ohem_select_kernel(u64* __restrict__ st, u64* __restrict__ hist, int has_thresh, long long* __restrict__ info) {
  __shared__ u64 sm[256];
  if (st[ST_DONE]) return;
  constexpr int PER = (1 << BITS) / 256;
  const int t = threadIdx.x;
  u64 hv[PER], sum = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    hv[j] = hist[t * PER + j];
    hist[t * PER + j] = 0;
    sum += hv[j];
  }
  const u64 rank = st[ST_RANK], prefix = st[ST_PREFIX];
  u64 before = block_excl_scan(sum, sm);                  // its barriers: every thread has read the state before one of them writes it
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (rank >= before && rank < before + hv[j]) {
      const u64 np = (prefix << BITS) | (u64)(t * PER + j), nr = rank - before;
      st[ST_PREFIX] = np;
      st[ST_RANK] = nr;
      if (LAST) {
        st[ST_CUT] = np;
        info[0] = (long long)np;
        if (!has_thresh) {
          const u64 take = hv[j] - nr;
          st[ST_TIE_TAKE] = take;
          st[ST_TIE_MODE] = take == hv[j] ? 1 : 2;
        }
      }
    }
    before += hv[j];
  }
}

// pixels equal to the cut in each workgroup's chunk of the map (only where some but not all of them are kept)     grid: chunks
__global__ __launch_bounds__(256) void ohem_tie_count_kernel(const float* __restrict__ keys, i64 total, i64 chunk, const u64* __restrict__ st,
                                                             unsigned int* __restrict__ tiecnt) {
  __shared__ unsigned int sm[4];
  if (st[ST_TIE_MODE] != 2) return;
  const unsigned int cut = (unsigned int)st[ST_CUT];
  const i64 lo = (i64)blockIdx.x * chunk, hi = lo + chunk < total ? lo + chunk : total;
  unsigned int c = 0;
  for (i64 i = lo + threadIdx.x; i < hi; i += 256) c += __float_as_uint(keys[i]) == cut ? 1u : 0u;
  c = block_count(c, sm);
  if (threadIdx.x == 0) tiecnt[blockIdx.x] = c;
}

// one workgroup: tiebase[b] = pixels equal to the cut in the chunks before b, added in chunk order
__global__ __launch_bounds__(256) void ohem_tie_scan_kernel(const u64* __restrict__ st, const unsigned int* __restrict__ tiecnt, int chunks,
                                                            u64* __restrict__ tiebase) {
  __shared__ u64 sm[256];
  if (st[ST_TIE_MODE] != 2) return;
  constexpr int PER = MAX_CHUNKS / 256;
  const int t = threadIdx.x;
  u64 v[PER], sum = 0;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    v[j] = t * PER + j < chunks ? tiecnt[t * PER + j] : 0;
    sum += v[j];
  }
  u64 before = block_excl_scan(sum, sm);
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    if (t * PER + j < chunks) tiebase[t * PER + j] = before;
    before += v[j];
  }
}

// key -> 0 / 1 in place, and info[2] += pixels kept.  TOPK: keys above the cut, and of the keys equal to it none, all, or -- tie mode 2 --
// those whose index among the equal ones, counted in raster order (chunks in order, 256-pixel tiles in order, lanes in order), is below
// ST_TIE_TAKE.                                                                                                        grid: chunks
template <bool TOPK>
__global__ __launch_bounds__(256) void ohem_weight_kernel(float* __restrict__ keys, i64 total, i64 chunk, const u64* __restrict__ st,
                                                          const u64* __restrict__ tiebase, long long* __restrict__ info) {
  __shared__ unsigned int sm[4];
  __shared__ unsigned int wv[4];
  const unsigned int cut = (unsigned int)st[ST_CUT];
  const i64 lo = (i64)blockIdx.x * chunk, hi = lo + chunk < total ? lo + chunk : total;
  unsigned int kept = 0;
  if (!TOPK) {
    const float thr = __uint_as_float(cut);
    for (i64 i = lo + threadIdx.x; i < hi; i += 256) {
      const float k = keys[i];
      const bool keep = k >= 0.f && k < thr;
      keys[i] = keep ? 1.f : 0.f;
      kept += keep ? 1u : 0u;
    }
  } else {
    const int mode = (int)st[ST_TIE_MODE], lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const u64 take = st[ST_TIE_TAKE];
    u64 run = mode == 2 ? tiebase[blockIdx.x] : 0;
    for (i64 base = lo; base < hi; base += 256) {                                            // whole workgroups walk the loop: votes and barriers
      const i64 i = base + threadIdx.x;
      const bool in = i < hi;
      const unsigned int k = in ? __float_as_uint(keys[i]) : ~0u;                            // a sentinel has bit 31 set
      const bool valid = (k >> 31) == 0, tie = valid && k == cut;
      bool keep = valid && k > cut;
      if (mode == 1) {
        keep = keep || tie;
      } else if (mode == 2) {
        const u64 m = __ballot(tie);
        if (lane == 0) wv[wid] = (unsigned int)__popcll(m);
        __syncthreads();
        u64 idx = run + (u64)__popcll(m & ((1ull << lane) - 1ull));
        for (int q = 0; q < wid; ++q) idx += wv[q];
        keep = keep || (tie && idx < take);
        run += wv[0] + wv[1] + wv[2] + wv[3];
        __syncthreads();
      }
      if (in) keys[i] = keep ? 1.f : 0.f;
      kept += keep ? 1u : 0u;
    }
  }
  kept = block_count(kept, sm);
  if (threadIdx.x == 0 && kept) atomicAdd(reinterpret_cast<u64*>(&info[2]), (u64)kept);
}

}  // namespace

extern "C" int pfst_ohem_workspace_bytes(int N, int H, int W, long long* bytes) {
  PFST_CHECK_ARG(N > 0 && H > 0 && W > 0 && bytes);
  *bytes = (long long)WS_BYTES;               // the state block, one level's table and the per-chunk tie counts: the same for every shape
  return PFST_OK;
}

extern "C" int pfst_ohem_sample(const float* logits, int N, int C, int h, int w, const unsigned char* label, int H, int W, int ignore_index,
                                int has_thresh, float thresh, long long batch_kept, const float* coef, void* workspace, float* weight,
                                long long* info, float* keys_out, pfst_stream_t stream) {
  PFST_CHECK_ARG(logits && label && workspace && weight && info && N > 0 && N <= 65535 && C > 0 && C <= 255 && h > 0 && w > 0 && H > 0 && W > 0);
  PFST_CHECK_ARG((i64)H * W < INT_MAX - 2048 * 4096 && (i64)h * w * C < INT_MAX);
  PFST_CHECK_ARG((has_thresh == 0 || has_thresh == 1) && batch_kept >= 0 && (has_thresh ? thresh == thresh : coef != nullptr));
  PFST_CHECK_ARG(((uintptr_t)weight & 15) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)info & 7) == 0);
  hipStream_t s = (hipStream_t)stream;
  char* ws = static_cast<char*>(workspace);
  u64* st = reinterpret_cast<u64*>(ws);
  u64* hist = reinterpret_cast<u64*>(ws + HIST_OFF);
  unsigned int* tiecnt = reinterpret_cast<unsigned int*>(ws + TIECNT_OFF);
  u64* tiebase = reinterpret_cast<u64*>(ws + TIEBASE_OFF);
  const i64 total = (i64)N * H * W;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  if (hipMemsetAsync(ws, 0, TIECNT_OFF, s) != hipSuccess) {              // the state block and the table
    pfst_set_error(__FILE__, __LINE__, "hipMemsetAsync of the workspace failed");
    return PFST_ERR_LAUNCH;
  }
  const dim3 pgrid(px_blocks((i64)H * W), N);
  if (C <= REG_C)
    hipLaunchKernelGGL(ohem_key_kernel<true>, pgrid, dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, sh, sw, has_thresh, thresh, coef,
                       weight, st);
  else
    hipLaunchKernelGGL(ohem_key_kernel<false>, pgrid, dim3(256), 0, s, logits, C, h, w, label, H, W, ignore_index, sh, sw, has_thresh, thresh, coef,
                       weight, st);
  PFST_CHECK_LAUNCH();
  if (keys_out && hipMemcpyAsync(keys_out, weight, (size_t)total * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
    pfst_set_error(__FILE__, __LINE__, "hipMemcpyAsync of the key map failed");
    return PFST_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(ohem_plan_kernel, dim3(1), dim3(1), 0, s, st, batch_kept, has_thresh, thresh, info);
  i64 hg = ((total >> 2) + 255) / 256;
  hg = hg > 1024 ? 1024 : (hg < 1 ? 1 : hg);
  const dim3 hgrid((unsigned int)hg);
  hipLaunchKernelGGL((ohem_hist_kernel<L1_BITS + L2_BITS, L0_BITS>), hgrid, dim3(256), 0, s, weight, total, st, hist);
  hipLaunchKernelGGL((ohem_select_kernel<L0_BITS, false>), dim3(1), dim3(256), 0, s, st, hist, has_thresh, info);
  hipLaunchKernelGGL((ohem_hist_kernel<L2_BITS, L1_BITS>), hgrid, dim3(256), 0, s, weight, total, st, hist);
  hipLaunchKernelGGL((ohem_select_kernel<L1_BITS, false>), dim3(1), dim3(256), 0, s, st, hist, has_thresh, info);
  hipLaunchKernelGGL((ohem_hist_kernel<0, L2_BITS>), hgrid, dim3(256), 0, s, weight, total, st, hist);
  hipLaunchKernelGGL((ohem_select_kernel<L2_BITS, true>), dim3(1), dim3(256), 0, s, st, hist, has_thresh, info);
  PFST_CHECK_LAUNCH();
  // fixed contiguous chunks of the map, whole 256-pixel tiles each: the raster order of the tie fill
  i64 chunks = (total + 1023) / 1024;
  chunks = chunks > MAX_CHUNKS ? MAX_CHUNKS : chunks;
  const i64 chunk = ((total + chunks - 1) / chunks + 255) / 256 * 256;
  chunks = (total + chunk - 1) / chunk;
  const dim3 cgrid((unsigned int)chunks);
  if (has_thresh) {
    hipLaunchKernelGGL(ohem_weight_kernel<false>, cgrid, dim3(256), 0, s, weight, total, chunk, st, tiebase, info);
  } else {
    hipLaunchKernelGGL(ohem_tie_count_kernel, cgrid, dim3(256), 0, s, weight, total, chunk, st, tiecnt);
    hipLaunchKernelGGL(ohem_tie_scan_kernel, dim3(1), dim3(256), 0, s, st, tiecnt, (int)chunks, tiebase);
    hipLaunchKernelGGL(ohem_weight_kernel<true>, cgrid, dim3(256), 0, s, weight, total, chunk, st, tiebase, info);
  }
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
