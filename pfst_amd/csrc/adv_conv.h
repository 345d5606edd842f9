// What adv_conv.hip (the matrix kernels of the discriminator's convolutions) and adv_tail.hip (its streaming end) share.
#pragma once
#include "common.h"

// The forward pass of a layer with ONE output channel (the discriminator's last): y[n][0][oy][ox] = b[0] + sum_{ci,tap} w[0][ci][tap] x[...],
// optionally through the LeakyReLU.  A reduction over K = 16 Cin per output pixel, one workgroup each: on the 32-row MFMA tile 31 rows idle
// and a handful of workgroups walk K serially (adv_tail.hip).  The caller has checked the shapes (adv_shape_ok).
int adv_conv1_fwd_launch(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Hi, int Wi, int act, float slope,
                         hipStream_t s);
