// The streaming end of the adversarial baseline's discriminator: the forward pass of its last layer -- 4x4, stride 2,
// padding 1, ONE output channel: a reduction, not a matrix product -- and the tail of the network: global mean, L1 against a constant label,
// and that loss's gradient spread back over the plane.  Built without the SLP vectoriser like every streaming file (build.py NO_SLP).
// Reference: rsiseg/models/discriminators/fc_discriminator.py:17-18, losses/adv_loss.py:58-63.
#include "adv_conv.h"
#include "../../include/pfst_hip.h"

namespace {

// One workgroup per output pixel (grid: (Ho Wo, N)).  Thread t owns tap t % 16 and the channels t / 16 + 16 i: its 16 neighbours read one
// w row of 16 floats; the per-thread partials (Cin / 16 fp32 terms) are added in fp64 in a fixed order.  Taps outside the image add nothing.
__global__ __launch_bounds__(256) void adv_conv1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ y, int Cin, int Hi, int Wi, int Ho, int Wo, int act, float slope) {
  __shared__ double sm[16];
  const int p = blockIdx.x, n = blockIdx.y;
  const int oy = p / Wo, ox = p - oy * Wo;
  const int tap = threadIdx.x & 15, c0 = threadIdx.x >> 4;
  const int sy = 2 * oy + (tap >> 2) - 1, sx = 2 * ox + (tap & 3) - 1;
  const i64 plane = (i64)Hi * Wi;
  float s = 0.f;
  if ((unsigned)sy < (unsigned)Hi && (unsigned)sx < (unsigned)Wi) {
    const float* xp = x + (i64)n * Cin * plane + (i64)sy * Wi + sx;
    for (int ci = c0; ci < Cin; ci += 16) s += w[ci * 16 + tap] * xp[ci * plane];
  }
  const double tot = block_sum_d((double)s, sm);
  if (threadIdx.x == 0) {
    float v = (float)tot;
    if (bias) v += bias[0];
    if (act) v = v > 0.f ? v : v * slope;
    y[(i64)n * Ho * Wo + p] = v;
  }
}

// One workgroup.  d[n] = mean of y[n][0 .. HW), each plane added in fp64 in a fixed order; loss[0] = weight * mean_n |d_n - label|;
// gy[n][i] (if given) = grad_scale * weight * sign(d_n - label) / (N HW)
__global__ __launch_bounds__(256) void adv_tail_kernel(const float* __restrict__ y, int N, int HW, float label, double weight, float grad_scale,
                                                       float* __restrict__ d, float* __restrict__ loss, float* __restrict__ gy) {
  __shared__ double sm[16];
  __shared__ float dn_s;
  double tot = 0.0;
  for (int n = 0; n < N; ++n) {
    double s = 0.0;
    for (int i = threadIdx.x; i < HW; i += 256) s += (double)y[(i64)n * HW + i];
    s = block_sum_d(s, sm);
    if (threadIdx.x == 0) dn_s = (float)(s / (double)HW);
    __syncthreads();
    const float dn = dn_s;
    const float diff = dn - label;
    tot += (double)fabsf(diff);
    if (threadIdx.x == 0 && d) d[n] = dn;
    if (gy) {
      const float sg = diff > 0.f ? 1.f : diff < 0.f ? -1.f : 0.f;
      const float g = grad_scale * (float)(weight * (double)sg / ((double)N * (double)HW));
      for (int i = threadIdx.x; i < HW; i += 256) gy[(i64)n * HW + i] = g;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && loss) loss[0] = (float)(weight * tot / (double)N);
}

}  // namespace

int adv_conv1_fwd_launch(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Hi, int Wi, int act, float slope,
                         hipStream_t s) {
  const int Ho = Hi / 2, Wo = Wi / 2;
  hipLaunchKernelGGL(adv_conv1_fwd_kernel, dim3(Ho * Wo, N), dim3(256), 0, s, x, w, bias, y, Cin, Hi, Wi, Ho, Wo, act, slope);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}

extern "C" int pfst_adv_tail(const float* y, int N, int HW, float label, double weight, float grad_scale, float* d, float* loss, float* gy,
                             pfst_stream_t stream) {
  PFST_CHECK_ARG(y && N > 0 && HW > 0 && (i64)N * HW < (1ll << 31) && (d || loss || gy));
  hipLaunchKernelGGL(adv_tail_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, y, N, HW, label, weight, grad_scale, d, loss, gy);
  PFST_CHECK_LAUNCH();
  return PFST_OK;
}
