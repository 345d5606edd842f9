// The four-tap source of one full-resolution pixel of a bilinear resize (align_corners=False) and its blend: shared by every kernel that
// interpolates a pixel's logits in registers -- the fused up-sampling losses (loss.hip, dice_loss.hip, sigmoid_loss.hip through
// upsample_walk.h), entropy_labels.hip and ohem.hip -- so that all of them use the same arithmetic, bit for bit.
#pragma once
#include "common.h"

struct Bilin {
  int y0, y1, x0, x1;
  float ly0, ly1, lx0, lx1;
};
__device__ __forceinline__ Bilin make_bilin(int oy, int ox, float sh, float sw, int h, int w) {
  Bilin b;
  bilin_src(oy, sh, h, b.y0, b.y1, b.ly0, b.ly1);
  bilin_src(ox, sw, w, b.x0, b.x1, b.lx0, b.lx1);
  return b;
}
__device__ __forceinline__ float interp(const float* __restrict__ p, int w, const Bilin& b) {
  return bilin_blend(p[b.y0 * w + b.x0], p[b.y0 * w + b.x1], p[b.y1 * w + b.x0], p[b.y1 * w + b.x1], b.lx0, b.lx1, b.ly0, b.ly1);
}
