// EMA teacher update, AdamW and SGD on FLAT parameter arenas: one launch each instead of the reference's
// ~850 tiny kernels (pfgst.py:105-127 loops over ~214 tensors) / torch.optim.AdamW's and torch.optim.SGD's per-tensor loops.
// All student parameters live in one contiguous fp32 buffer (same for grads, Adam moments and the
// teacher), which is also what RCCL all-reduces.
#include "common.h"
#include "../../include/pfst_hip.h"

namespace {

__global__ void ema_kernel(float* __restrict__ t, const float* __restrict__ s, i64 n, float alpha) {
  const float one_m = 1.f - alpha;
  const i64 stride = (i64)gridDim.x * blockDim.x;
  const i64 n4 = n >> 2;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 a = reinterpret_cast<float4*>(t)[i];
    const float4 b = reinterpret_cast<const float4*>(s)[i];
    // the reference's expression alpha*ema + (1-alpha)*param; as compiled (contraction is on) each element is ONE rounded product one_m*b and
    // ONE fused multiply-add alpha*a + that (v_mul_f32, v_fmac_f32), and one_m = 1 - alpha is formed in fp32 from the rounded alpha (at 0.999
    // it is 1.3e-5 relative away from the rounded double 1 - alpha).  Bound and measurement: tests/test_optimizer_edges_gpu.py, part C
    a.x = alpha * a.x + one_m * b.x; a.y = alpha * a.y + one_m * b.y;
    a.z = alpha * a.z + one_m * b.z; a.w = alpha * a.w + one_m * b.w;
    reinterpret_cast<float4*>(t)[i] = a;
  }
  for (i64 i = (n4 << 2) + (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) t[i] = alpha * t[i] + one_m * s[i];
}

// torch.optim.AdamW (amsgrad=False, maximize=False), single-tensor formulation
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, i64 n,
                             float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt, float gscale) {
  const i64 stride = (i64)gridDim.x * blockDim.x;
  const float step_size = lr / bc1;
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gi = g[i] * gscale;
    float pi = p[i] * (1.f - lr * wd);
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi -= step_size * (mi / denom);
    p[i] = pi; m[i] = mi; v[i] = vi;
  }
}

// torch.optim.SGD (maximize=False), single-tensor formulation, one element, with torch's roundings: each of its `x.add(y, alpha=a)` calls
// (grad.add(p, alpha=wd); buf.mul_(momentum).add_(d, alpha=1-dampening); d.add(buf, alpha=momentum); p.add_(d, alpha=-lr)) is ONE fused
// multiply-add in torch's CPU and GPU kernels, and `mul_` rounds on its own -- so exactly these fmaf calls and nothing else fused (contraction
// off), and a checkpoint stepped here stays on the trajectory of one stepped by torch (bit for bit against torch's CPU kernels).
template <bool MOM>
__device__ __forceinline__ void sgd_elem(float& p, const float g, float& b, float lr, float mom, float one_m_damp, float wd, bool nesterov,
                                         bool first, float gscale) {
#pragma clang fp contract(off)
  float d = __builtin_fmaf(p, wd, g * gscale);
  if (MOM) {
    b = first ? d : __builtin_fmaf(d, one_m_damp, mom * b);
    d = nesterov ? __builtin_fmaf(b, mom, d) : b;
  }
  p = __builtin_fmaf(d, -lr, p);
}

// Memory-bound: three reads (p, g, buf) and two writes (p, buf) of n floats -- two and one without momentum.  float4 body over n / 4, scalar
// tail; the arena keeps every tensor 16-byte aligned, loose tensors that are not go through the scalar loop alone (vec = 0).
template <bool MOM>
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, i64 n, int vec, float lr, float mom,
                           float one_m_damp, float wd, int nesterov, int first, float gscale) {
  const i64 stride = (i64)gridDim.x * blockDim.x;
  const i64 tid = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  const i64 n4 = vec ? (n >> 2) : 0;
  const bool nest = nesterov != 0, fst = first != 0;
  for (i64 i = tid; i < n4; i += stride) {
    float4 pi = reinterpret_cast<float4*>(p)[i];
    const float4 gi = reinterpret_cast<const float4*>(g)[i];
    float4 bi = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MOM && !fst) bi = reinterpret_cast<float4*>(buf)[i];          // the first step writes the buffer without reading it
    sgd_elem<MOM>(pi.x, gi.x, bi.x, lr, mom, one_m_damp, wd, nest, fst, gscale);
    sgd_elem<MOM>(pi.y, gi.y, bi.y, lr, mom, one_m_damp, wd, nest, fst, gscale);
    sgd_elem<MOM>(pi.z, gi.z, bi.z, lr, mom, one_m_damp, wd, nest, fst, gscale);
    sgd_elem<MOM>(pi.w, gi.w, bi.w, lr, mom, one_m_damp, wd, nest, fst, gscale);
    reinterpret_cast<float4*>(p)[i] = pi;
    if (MOM) reinterpret_cast<float4*>(buf)[i] = bi;
  }
  for (i64 i = (n4 << 2) + tid; i < n; i += stride) {
    float pi = p[i], bi = 0.f;
    if (MOM && !fst) bi = buf[i];
    sgd_elem<MOM>(pi, g[i], bi, lr, mom, one_m_damp, wd, nest, fst, gscale);
    p[i] = pi;
    if (MOM) buf[i] = bi;
  }
}

}  // namespace

extern "C" int pfst_ema_update(float* teacher, const float* student, long long n, float alpha, pfst_stream_t stream) {
  PFST_CHECK_ARG(teacher && student && n > 0);
  PFST_CHECK_ARG(((((uintptr_t)teacher) | ((uintptr_t)student)) & 15) == 0);
  hipLaunchKernelGGL(ema_kernel, dim3(ew_grid(n / 4 + 1)), dim3(256), 0, (hipStream_t)stream, teacher, student, (i64)n, alpha);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_adamw_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                               float eps, float weight_decay, int step, float grad_scale, pfst_stream_t stream) {
  PFST_CHECK_ARG(p && g && m && v && n > 0 && step >= 1);
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adamw_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (i64)n, lr, beta1, beta2, eps,
                     weight_decay, (float)bc1, (float)sqrt(bc2), grad_scale);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_sgd_step(float* p, const float* g, float* buf, long long n, float lr, float momentum, float dampening,
                             float weight_decay, int nesterov, int first_step, float grad_scale, pfst_stream_t stream) {
  PFST_CHECK_ARG(p && g && n > 0);
  PFST_CHECK_ARG((buf != nullptr) == (momentum != 0.f));
  PFST_CHECK_ARG(((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)buf)) & 3) == 0);
  // torch.optim.SGD's own condition: nesterov needs a momentum and no dampening
  PFST_CHECK_ARG(!nesterov || (momentum > 0.f && dampening == 0.f));
  const int vec = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)buf)) & 15) == 0;
  const float one_m_damp = (float)(1.0 - (double)dampening);          // torch forms 1 - dampening in double
  const dim3 grid(ew_grid(vec ? n / 4 + 1 : n)), block(256);
  if (momentum != 0.f)
    hipLaunchKernelGGL(sgd_kernel<true>, grid, block, 0, (hipStream_t)stream, p, g, buf, (i64)n, vec, lr, momentum, one_m_damp, weight_decay,
                       nesterov, first_step, grad_scale);
  else
    hipLaunchKernelGGL(sgd_kernel<false>, grid, block, 0, (hipStream_t)stream, p, g, buf, (i64)n, vec, lr, momentum, one_m_damp, weight_decay,
                       nesterov, first_step, grad_scale);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
