// Host-side launch rules shared by the matrix-kernel files (conv_mfma, conv_igemm_q, conv_wgrad_q, conv_split, conv_f16x3): the geometry
// of a forward / data-gradient launch, the row tile of a launch and the epilogue mode of the fused BatchNorm-backward sums -- each once.
#pragma once
#include <type_traits>
#include "common.h"
#include "../../include/pfst_hip.h"

// the kernels' source-coordinate map (src_coord in conv_epilogue.h): input = (out * a + tap * b + c) / d
struct ConvGeom {
  int a, b, c, d;
};

// Validates the geometry of an implicit-GEMM launch and yields its coordinate map.  mode 0 (forward, and the weight gradients, which walk
// the forward map): Hi x Wi is the input, Ho x Wo the output.  mode 1 (data gradient): `in` is dy (Hi x Wi = the forward OUTPUT) and `out`
// is dx (Ho x Wo = the forward input).
static inline int conv_geometry(int Hi, int Wi, int Ho, int Wo, int ksize, int stride, int dil, int pad, int mode, ConvGeom& g) {
  PFST_CHECK_ARG((ksize == 1 || ksize == 3) && (stride == 1 || stride == 2) && dil >= 1 && pad >= 0 && (mode == 0 || mode == 1));
  const int span = (ksize - 1) * dil;
  if (mode == 0) {
    PFST_CHECK_ARG(Ho == (Hi + 2 * pad - span - 1) / stride + 1 && Wo == (Wi + 2 * pad - span - 1) / stride + 1);
    g = ConvGeom{stride, dil, -pad, 1};
  } else {
    PFST_CHECK_ARG(Hi == (Ho + 2 * pad - span - 1) / stride + 1 && Wi == (Wo + 2 * pad - span - 1) / stride + 1);
    g = ConvGeom{1, -dil, pad, stride};
  }
  return PFST_OK;
}

// The row tile of a launch with M output rows: f(integral_constant<int, BM>) with BM = 128 for M > 64, 64 for M > 32, else 32
template <class F>
static inline int with_row_tile(int M, F&& f) {
  if (M > 64) return f(std::integral_constant<int, 128>());
  if (M > 32) return f(std::integral_constant<int, 64>());
  return f(std::integral_constant<int, 32>());
}

// Epilogue mode of the fused BatchNorm-backward sums (the BNB template argument, conv_epilogue.h): 3 no ReLU, 4 the gate bits of y_mask,
// 2 the gate from y, 1 the gate recomputed from x.  GATE_BITS: the kernel family has mode 4 (f16x3 only; the others read y).
template <bool GATE_BITS>
static inline int bnb_mode(const pfst_bnb_fuse_t& bnb) {
  return !bnb.relu ? 3 : (GATE_BITS && bnb.y_mask) ? 4 : bnb.y ? 2 : 1;
}
// f(integral_constant<int, MODE>) for that mode
template <bool GATE_BITS, class F>
static inline void with_bnb_mode(const pfst_bnb_fuse_t& bnb, F&& f) {
  switch (bnb_mode<GATE_BITS>(bnb)) {
    case 3: f(std::integral_constant<int, 3>()); break;
    case 4: if constexpr (GATE_BITS) f(std::integral_constant<int, 4>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    default: f(std::integral_constant<int, 1>()); break;
  }
}
