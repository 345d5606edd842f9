/* pfst_hip.h -- C ABI of libpfst_hip.so: the MI355X (gfx950) kernels of the PFST train step.
 *
 * The reference (zhu-xlab/PFST, `rsiseg`) has no native layer: every op below is, in the
 * reference, a PyTorch/mmcv call inside PFGST.train_step (rsiseg/models/uda/pfgst.py:129-356).
 * Each entry point names the reference call it replaces.  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (torch allocates); no hidden state,
 *     no allocation, no synchronisation inside; work is enqueued on `stream` (a hipStream_t);
 *   - tensors are fp32 NCHW; `*_bs` arguments are batch strides in elements so a channel slice of
 *     a bigger tensor can be passed (concatenations are never materialised);
 *   - return 0 on success, <0 on error (-1 bad argument, -2 launch failure, -3 unsupported);
 *     pfst_last_error() returns a static description of the last failure of the calling process;
 *   - re-entrant per stream.
 * The parser in pfst_amd/_lib.py reads this file to build the ctypes signatures, so keep one
 * declaration per statement and only the scalar types used below.
 */
#ifndef PFST_HIP_H
#define PFST_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

typedef void* pfst_stream_t; /* hipStream_t */

int pfst_abi_version(void);
const char* pfst_last_error(void);
/* Deterministic mode, the counterpart of torch.backends.cudnn.deterministic = True that the reference's `--deterministic` sets
 * (rsiseg/apis/train.py:52-68): weight gradients, BatchNorm-backward sums and depthwise weight gradients are summed in a fixed order instead of
 * by atomic adds of several workgroups -- the gradient of a step is bit-identical run to run; slower.  Process-wide, read at every launch. */
int pfst_set_deterministic(int on);
int pfst_get_deterministic(void);

/* ---- elementwise utilities -------------------------------------------------------------- */
int pfst_fill_f32(float* p, long long n, float value, pfst_stream_t stream);
/* y[i] += alpha * x[i]   (autograd's gradient accumulation) */
int pfst_axpy_f32(float* y, const float* x, float alpha, long long n, pfst_stream_t stream);
/* int64 / uint8 label conversions (decode_head.py:209 `.type(torch.LongTensor)`) */
int pfst_i64_to_u8(const long long* src, unsigned char* dst, long long n, pfst_stream_t stream);
int pfst_u8_to_i64(const unsigned char* src, long long* dst, long long n, pfst_stream_t stream);

/* fused BatchNorm-backward sums of a data-gradient launch, see pfst_conv_igemm */
typedef struct pfst_bnb_fuse {
  const float* x;            /* pre-BN tensor [N][M][P] of the layer that owns the gradient being written */
  long long x_bs;            /* its batch stride (elements) */
  const float* y;            /* that layer's output: ReLU gate = y > 0 (residual layers); NULL: gate recomputed from x as bn_apply did */
  long long y_bs;
  const float* coef;         /* [M][4] = (mean, invstd, sc, sh) of that layer as pfst_bn_finalize_partials / pfst_bn_stats wrote them */
  float* partials;           /* out: [M][T][2] = (sum dz, sum dz * x) per channel and slot */
  int relu;
  const unsigned long long* y_mask; /* optional, with y: pfst_bn_apply's ReLU bitmask of y ([N][M][HW / 64] words, HW % 256 == 0) -- the f16x3
                                      kernel then takes a residual layer's gate bits from it instead of reading y */
} pfst_bnb_fuse_t;

/* What a kernel needs to apply the SECOND pass of BatchNorm backward on the fly, per channel: dx = gs * (dz - m1 - xhat * m2) with
 * dz = dy * [x * sc + sh > 0], xhat = (x - mu) * is, in the arithmetic of pfst_bn_backward's apply pass (fp64 projections).  Written by
 * pfst_bn_backward_sums, read by pfst_dwconv3x3_bwd / pfst_dwconv3x3_multi_bwd (the depthwise layers' backward forms dL/dpre itself). */
typedef struct pfst_bn_bwd_rec {
  double m1, m2, gs;
  float mu, is, sc, sh;
} pfst_bn_bwd_rec_t;

/* ---- dense convolution as implicit GEMM on fp32 MFMA (F.conv2d, groups=1) ---------------
 * resnet.py:169-209 (Bottleneck 1x1/3x3), resnet.py:593-624 (stem), aspp_head.py:32-42,85-92,
 * fcn_head.py:40-49, decode_head.py:242-247 (conv_seg), mmcv pointwise convs. */
/* w[Cout][Cin][T] -> wk_fprop[(t*Cin+ci)][Cout] and wk_dgrad[(t*Cout+co)][Cin] (either may be NULL) */
int pfst_conv_pack_weight(const float* w, float* wk_fprop, float* wk_dgrad, int Cout, int Cin, int T, pfst_stream_t stream);
/* out[n][m][oy][ox] (+)= bias[m] + sum_{t,c} wk[(t*C+c)][m] * in[n][c][sy][sx]
 *   mode 0 (fprop): sy = oy*stride + ty*dil - pad          in = x,  C = Cin,  M = Cout
 *   mode 1 (dgrad): sy = (oy + pad - ty*dil) / stride      in = dy, C = Cout, M = Cin  (exact division only)
 * ksize in {1,3}; accumulate != 0 adds into `out`. */
int pfst_conv_igemm(const float* in, long long in_bs, const float* wk, const float* bias, float* out, long long out_bs,
                    int N, int C, int Hi, int Wi, int M, int Ho, int Wo, int ksize, int stride, int dil, int pad,
                    int mode, int accumulate, float* stats, const pfst_bnb_fuse_t* bnb, pfst_stream_t stream);
/* Fused BatchNorm-BACKWARD sums (bnb != NULL, data-gradient launches): when `out` is the COMPLETE gradient dL/dy of a
 * conv -> BN(train) -> [+residual] -> ReLU layer's output (this launch is the last writer of that buffer; with accumulate != 0 the
 * sums are taken over old + new), the epilogue also writes per-channel partials of  S1 = sum dz,  S2' = sum dz * x  (dz = dy * ReLU gate)
 * to bnb->partials[M][N * pfst_conv_stats_slots(M, Ho, Wo)][2]; pfst_bn_backward then skips its reduction pass (torch's
 * native_batch_norm_backward makes the same two sums).  Needs C % 16 == 0, M a multiple of the row tile (128 for M > 64, else 64 / 32),
 * no bias, stats == NULL; returns PFST_ERR_ARG otherwise (the caller then simply does not fuse). */
/* Fused BatchNorm statistics: if `stats` != NULL the epilogue also writes per-channel partial (sum, sum of squares)
 * pairs to stats[M][N * pfst_conv_stats_slots(M, Ho, Wo)][2] (fp32, no atomics); reduce them with
 * pfst_bn_finalize_partials.  Saves the separate full-tensor read of pfst_bn_stats. */
int pfst_conv_stats_slots(int M, int Ho, int Wo);
/* The same convolution on the bf16 matrix cores with fp32-faithful arithmetic: operands are split exactly into three
 * bf16 pieces and the six piece-products >= 2^-16 are accumulated in fp32 (csrc/conv_split.hip).  Needs C % 16 == 0
 * (returns -3 otherwise).  wk6_*: pfst_conv_pack_weight_split images, 6*Cout*Cin*T bytes each. */
int pfst_conv_pack_weight_split(const float* w, void* wk6_fprop, void* wk6_dgrad, int Cout, int Cin, int T, pfst_stream_t stream);
int pfst_conv_igemm_split(const float* in, long long in_bs, const void* wk6, const float* bias, float* out, long long out_bs,
                          int N, int C, int Hi, int Wi, int M, int Ho, int Wo, int ksize, int stride, int dil, int pad,
                          int mode, int accumulate, float* stats, const pfst_bnb_fuse_t* bnb, pfst_stream_t stream);
int pfst_conv_wgrad_split(const float* x, long long x_bs, const float* dy, long long dy_bs, float* dw,
                          int N, int Cin, int Hi, int Wi, int Cout, int Ho, int Wo, int ksize, int stride, int dil, int pad,
                          pfst_stream_t stream);
/* dw[co][ci][t] += sum_{n,oy,ox} dy[n][co][oy][ox] * x[n][ci][oy*stride+ty*dil-pad][...]   (atomic fp32 adds) */
int pfst_conv_wgrad(const float* x, long long x_bs, const float* dy, long long dy_bs, float* dw,
                    int N, int Cin, int Hi, int Wi, int Cout, int Ho, int Wo, int ksize, int stride, int dil, int pad,
                    pfst_stream_t stream);
/* Occupancy cap of the K-quad weight-gradient kernels: `bytes` of unused dynamic LDS per workgroup (0 = off, the default).  With
 * 24000 two instead of four workgroups fit per CU (the fp32-MFMA pipe stays saturated: -0.3 % on the step) and an HBM-bound kernel
 * of ANOTHER stream -- the BatchNorm-backward chain, when the host runs weight gradients on a side stream -- can be co-resident. */
int pfst_conv_wgrad_set_lds_pad(int bytes);
/* The split-K plan of the weight-gradient launchers (csrc/wgrad_launch.h), host arithmetic only -- no device is touched: a launch of
 * `work` workgroups (tiles x images x groups) over P pixels is cut into *chunks pixel chunks of *chunk_len (a multiple of k_step; the last
 * one may be shorter), so that whole rounds of `slots` resident workgroups fill the chip.  chunk_cap > 0: at most that many chunks.
 * doubling != 0: the doubling rule of the generic bf16x6 weight gradient instead (slots, k_step and chunk_cap are ignored). */
int pfst_wgrad_split_k(long long work, int P, int slots, int k_step, int chunk_cap, int doubling, int* chunks, int* chunk_len);
/* db[c] += sum_{n,hw} dy[n][c][hw] */
int pfst_bias_grad(const float* dy, long long dy_bs, float* db, int N, int C, int HW, pfst_stream_t stream);

/* ---- Winograd F(m x m, 3x3), m = 2 or 4, for wide stride-1 'same' 3x3 convolutions (csrc/conv_winograd.hip): the same F.conv2d /
 * autograd results with 2.25x (m = 2) or 4x (m = 4) fewer MACs.  X = (m+2)^2 transform indices; transform-domain tensors
 * V [X][N][C][T], U [X][K/4][M][4], Mbuf [X][N][M][T], T = pfst_wino_tiles(H, W, dil, m) tiles per image (dilation d = d*d
 * interleaved sub-grids).  fp32 error vs an fp64 direct convolution: 3e-6 (m = 2), 3e-5 (m = 4) of the mean |y|.
 *   fprop : pfst_wino_input(x) -> V;   pfst_wino_gemm(V, U_fprop) -> Mbuf;   pfst_wino_output(Mbuf) -> y
 *   dgrad : the same on dy with U_dgrad (flipped, transposed filter), pfst_wino_output(..., accumulate)
 *   wgrad : pfst_wino_input(x) -> V;  pfst_wino_dy(dy) -> dM;  pfst_wino_wgrad(V, dM, scratch dU[X*Cout*Cin]) : dw += ... */
int pfst_wino_tiles(int H, int W, int dil, int m);
int pfst_wino_pack_weight(const float* w, float* U_fprop, float* U_dgrad, int Cout, int Cin, int m, pfst_stream_t stream);
int pfst_wino_input(const float* x, long long x_bs, float* V, int N, int C, int H, int W, int dil, int m, float* v_amax,
                    const float* pack_x_amax, const float* bnl, pfst_stream_t stream);
/* bnl != NULL: coef [C][4] = (mean, invstd, sc, sh) of the conv -> BN -> ReLU layer whose PRE-normalisation output x is (Bottleneck conv1 ->
 * bn1 -> relu -> conv2, resnet.py:273-281): elements are normalised as they are loaded, the normalised tensor is never written; pack_x_amax
 * then is the slot group pfst_bn_finalize_partials published the predicted max |relu(bn(x))| to */
/* v_amax: NULL, or the slot group (1024 floats, zeroed; csrc/amax.h) that receives max |V| (f16x3 scale).  pack_x_amax != NULL: V is
 * written PRE-SPLIT for the f16x3 GEMMs (one dword per element: the two fp16 pieces of V s), scaled from the slot group holding max |x|
 * through the transform's norm bound, and v_amax receives that bound (pass v_packed = 1 / packed = 1 to the consumers) */
int pfst_wino_gemm(const float* V, const float* U, float* Mbuf, int N, int K, int M, int T, int m, pfst_stream_t stream);
int pfst_wino_output(const float* Mbuf, float* y, long long y_bs, int N, int Cout, int H, int W, int dil, int accumulate,
                     float* stats, int stats_minmax, const float* bnb_x, long long bnb_x_bs, const float* bnb_coef, int bnb_relu, int m,
                     pfst_stream_t stream);
/* bnb_x != NULL (the output transform of a DATA-GRADIENT launch whose `y` is the complete gradient of a conv -> BN [-> ReLU] layer's output,
 * no residual -- Bottleneck bn1 behind a Winograd conv2): bnb_x = that layer's pre-BN tensor, bnb_coef its coef [Cout][4]; `stats` then
 * receives the layer's BatchNorm-backward partials (sum dz, sum dz * x) [Cout][N * pfst_wino_stats_slots][2] for pfst_bn_backward(bwd_partials),
 * as pfst_conv_igemm's bnb does for the GEMM data gradients: the layer's reduction pass is not launched */
/* stats != NULL: BatchNorm partials of the output, stats[Cout][N * pfst_wino_stats_slots(H, W, dil, m)][2]; stats_minmax != 0: `stats` has room
 * for twice that and also receives the per-channel (minimum, maximum) partials behind the sums (as pfst_conv_igemm_f16x3's stats_minmax) */
int pfst_wino_stats_slots(int H, int W, int dil, int m);
int pfst_wino_dy(const float* dy, long long dy_bs, float* dM, int N, int Cout, int H, int W, int dil, int m, float* dm_amax,
                 const float* pack_dy_amax, pfst_stream_t stream);
/* the data gradient from the weight gradient's transform (f16x3): P [X][N][Cin][T] = pfst_wino_gemm_f16x3(dM packed by pfst_wino_dy, the
 * UNFLIPPED forward filter sets packed in the data-gradient layout (K = Cout, rows = Cin), the forward sets' maxima, v_packed = 1);
 * pfst_wino_dx forms the R x R patches B P B^T and overlap-adds them at stride m into dx [N][Cin][H][W] as a gather with a fixed
 * summation order (no atomics).  partials / bnb_*: as pfst_wino_output's stats / bnb_* -- the BatchNorm-backward partials
 * [Cin][N * pfst_wino_dx_slots(H, W, dil, m)][2] of the layer that owns dx (both given or both NULL) */
int pfst_wino_dx_slots(int H, int W, int dil, int m);
int pfst_wino_dx(const float* P, float* dx, long long dx_bs, int N, int Cin, int H, int W, int dil, int accumulate, float* partials,
                 const float* bnb_x, long long bnb_x_bs, const float* bnb_coef, int bnb_relu, int m, pfst_stream_t stream);
int pfst_wino_wgrad(const float* V, const float* dM, float* dU, float* dw, int N, int Cin, int Cout, int T, int m,
                    int split, const float* v_amax, const float* dm_amax, int packed, pfst_stream_t stream);
/* split = 1: the transform-domain products with the fp32-faithful bf16x6 split on the bf16 matrix cores; split = 2: with the f16x3 split,
 * v_amax / dm_amax = the slot groups pfst_wino_input / pfst_wino_dy published the operands' absolute maxima to (NULL otherwise) */
/* the same GEMMs on the fp32-faithful bf16x6 path: plain [X][Cout][Cin] filter sets (normal / flipped) -> X split-packed sets of
 * 6*Cout*Cin bytes each -> pfst_wino_gemm_split */
int pfst_wino_filter_plain(const float* w, float* P_fprop, float* P_dgrad, int Cout, int Cin, int m, pfst_stream_t stream);
int pfst_wino_pack_weight_split(const float* plain_f, const float* plain_d, void* U6_fprop, void* U6_dgrad, int Cout, int Cin,
                                int m, pfst_stream_t stream);
int pfst_wino_gemm_split(const float* V, const void* U6, float* Mbuf, int N, int K, int M, int T, int m, pfst_stream_t stream);

/* ---- the same GEMMs with the fp32-faithful TWO-piece fp16 split (csrc/conv_f16x3.hip): three fp16 MFMAs per product instead of
 * six bf16 ones.  Every operand tensor is scaled by the power of two its absolute maximum implies; the maxima are device
 * scalars (fp32 slots) written by pfst_absmax or by the kernels that produce the operands -- never read back to the host.
 * Replaces the same reference calls as pfst_conv_igemm (F.conv2d / its data gradient inside mmcv ConvModule:
 * rsiseg/models/backbones/resnet.py:273-305, decode_heads/aspp_head.py:34-42,85-92).  Needs C % 32 == 0 and M > 64 (-3 otherwise). */
int pfst_absmax(const float* x, long long n, int planes, long long plane_stride, int slot_stride, float* slots, pfst_stream_t stream);
int pfst_conv_pack_weight_f16x2(const float* w, void* wk4_fprop, void* wk4_dgrad, int Cout, int Cin, int T, int sets,
                                const float* amax, pfst_stream_t stream);
/* Batched weight preparation of a whole network (two launches per model and step instead of 2-5 tiny ones per convolution; the
 * reference re-reads its weights inside every cuDNN call and has no such step).  A job table lives on the device; the host copy is
 * passed beside it and checked (pointers, shapes, block prefix) before the launch.
 *   pfst_weight_prep_batched:  m == 0: amax_f[0] (one slot group) <- max |src[Cout*Cin*T]|
 *                              m == 2/4: src = 3x3 filters; dst_f / dst_d (either may be NULL) <- the X = (m+2)^2 plain transform-domain
 *                              sets [X][Cout][Cin] of pfst_wino_filter_plain, amax_f / amax_d <- X consecutive slot groups with each set's maximum
 *   pfst_conv_pack_weight_f16x2_batched: src [sets][Cout][Cin][T] -> dst_f / dst_d two-piece fp16 images exactly as
 *                              pfst_conv_pack_weight_f16x2 writes them, scales from the `sets` consecutive slot groups at amax_f
 * The slot groups must be zeroed before the prep launch.  first_block: prefix sum of pfst_weight_job_blocks over the table. */
typedef struct pfst_weight_job {
  const float* src;
  void* dst_f;
  void* dst_d;
  float* amax_f;
  float* amax_d;
  int Cout, Cin, T, sets, m, first_block;
} pfst_weight_job_t;
int pfst_weight_job_blocks(const pfst_weight_job_t* job, int pack);     /* workgroups one job takes in the prep (0) / pack (1) launch */
int pfst_weight_prep_batched(const pfst_weight_job_t* jobs_host, const pfst_weight_job_t* jobs_dev, int njobs, pfst_stream_t stream);
int pfst_conv_pack_weight_f16x2_batched(const pfst_weight_job_t* jobs_host, const pfst_weight_job_t* jobs_dev, int njobs,
                                        pfst_stream_t stream);
int pfst_conv_igemm_f16x3(const float* in, long long in_bs, const void* wk4, const float* w_amax, const float* in_amax,
                          const float* bias, float* out, long long out_bs, int N, int C, int Hi, int Wi, int M, int Ho, int Wo,
                          int ksize, int stride, int dil, int pad, int mode, int accumulate, float* stats, const pfst_bnb_fuse_t* bnb,
                          const float* gate_dy, long long gate_dy_bs, const unsigned long long* gate_mask, int stats_minmax,
                          const float* bnl, pfst_stream_t stream);
/* bnl != NULL (forward 1x1 launches, M % 256 == 0, C <= 2048): `in` is the PRE-normalisation output of the conv -> BN -> ReLU layer feeding this
 * convolution (Bottleneck conv2 -> bn2 -> relu -> conv3, resnet.py:282-290) and bnl its coef [C][4] = (mean, invstd, sc, sh): elements are
 * normalised between their load and their split, the normalised tensor is never written; in_amax = the slot group
 * pfst_bn_finalize_partials published the predicted max |relu(bn(in))| to */
/* stats_minmax != 0 (with stats): stats has room for 4 * M * slots floats; behind the [M][slots][2] (sum, sum of squares) partials the
 * launch writes [M][slots][2] (minimum, maximum) partials of the output, from which pfst_bn_finalize_partials predicts max |relu(bn(out))| */
/* gate_dy != NULL (mode 1, accumulate 0, M % 128 == 0, Ho * Wo % 256 == 0): out = data gradient + (bit ? gate_dy : 0), gate_mask = the ReLU
 * bitmask pfst_bn_apply wrote for an [N][M][Ho * Wo] tensor -- the identity branch of a residual block (resnet.py:149-167, out = relu(bn3 +
 * identity)): dL/d(block input) = conv1's data gradient + dL/d(block output) gated by that ReLU, formed in conv1's epilogue instead of
 * being written by pfst_bn_backward (dres) and read back here */
/* The f16x3 GEMMs walk their tiles in chains of up to 8 per workgroup, the grid sized for the resident workgroup slots of the device
 * (2 per CU).  pfst_f16x3_set_slots overrides that number (0 = the device's): a test hook that makes small problems chain. */
int pfst_f16x3_set_slots(int slots);
int pfst_f16x3_chain_grid(long long total_tiles, int chainable);   /* the workgroup count such a launch uses */
/* Test hook: the two-piece split of n values (n % 8 == 0), scale from the slot group `amax`, as the GEMM loops issue it (8-value and
 * 4-value pinned instruction sequences) and as the prologues / packing kernels compute it; each output element = h | l << 16. */
int pfst_f16x3_split_probe(const float* x, long long n, const float* amax, unsigned* pieces_loop, unsigned* pieces_loop4,
                           unsigned* pieces_plain, pfst_stream_t stream);
int pfst_wino_gemm_f16x3(const float* V, const void* U4, const float* u_amax, const float* v_amax, float* Mbuf, int N, int K,
                         int M, int T, int m, int v_packed, pfst_stream_t stream);
int pfst_conv_wgrad_f16x3(const float* x, long long x_bs, const float* dy, long long dy_bs, float* dw, int N, int Cin, int Cout,
                          int HW, const float* x_amax, const float* dy_amax, const float* bnl, pfst_stream_t stream);
/* bnl != NULL: x is the PRE-normalisation tensor the forward launch read with its own bnl (pfst_conv_igemm_f16x3): rows normalised on load */
/* the same for the layers that kernel does not take -- stride-1 'same' 3x3 (pad == dil <= 8, W % 16 == 0) and 1x1 with <= 64 output channels
 * (the stems, layer1: resnet.py:593-624,169-209) -- on the K-quad kernel with both operands split as they are staged (csrc/conv_wgrad_q.hip) */
int pfst_conv_wgrad_f16x3_q(const float* x, long long x_bs, const float* dy, long long dy_bs, float* dw, int N, int Cin, int H, int W,
                            int Cout, int ksize, int dil, const float* x_amax, const float* dy_amax, pfst_stream_t stream);

/* ---- depthwise 3x3 convolution, stride 1, pad = dil (mmcv DepthwiseSeparableConvModule,
 * sep_aspp_head.py:17-26,63-77).  flip != 0 mirrors the taps (= data gradient). */
int pfst_dwconv3x3(const float* x, long long x_bs, const float* w, float* y, long long y_bs,
                   int N, int C, int H, int W, int dil, int flip, int accumulate, float* stats, int stats_minmax,
                   const float* bn_on_load_coef, pfst_stream_t stream);
/* stats_minmax != 0 (with stats): `stats` has room for twice the partials and also receives the per-channel (minimum, maximum) partials
 * behind the sums (as pfst_conv_igemm_f16x3's): the pointwise layer of the DepthwiseSeparableConvModule then normalises this output as it
 * loads it (pfst_conv_igemm_f16x3 bnl) from the predicted maximum */
/* bn_on_load_coef: NULL, or coef[C][4] = (mean, invstd, sc, sh) of the conv -> BN -> ReLU layer that feeds this depthwise layer: x is then that
 * layer's PRE-normalisation output, normalised + rectified while it is staged (forward only; the normalised tensor is never written) */
/* stats != NULL: per-channel partial (sum, sum of squares) of the outputs, stats[C][N * pfst_dwconv_stats_slots(H, W, dil)][2],
 * for pfst_bn_finalize_partials (as the `stats` argument of pfst_conv_igemm) */
int pfst_dwconv_stats_slots(int H, int W, int dil);
int pfst_dwconv3x3_wgrad(const float* x, long long x_bs, const float* dy, long long dy_bs, float* dw,
                         int N, int C, int H, int W, int dil, pfst_stream_t stream);
/* ns <= 3 depthwise branches that read the SAME input (the ASPP head's atrous branches, sep_aspp_head.py:63-77: dilations 12 / 24 / 36 on one
 * 2048-channel map), whole planes (H * W <= 16384, W % 4 == 0), dilations % 4 == 0, 16-byte aligned dense planes.
 *   fwd: y[i] = dwconv(x, w[i], dils[i]) (+ BatchNorm partials stats[i][C][N][2] or NULL) with every input plane staged once;
 *        plane_mean != NULL: also [N][C] means of x's planes = nn.AdaptiveAvgPool2d(1) of the image-pool branch (aspp_head.py:69-77),
 *        as pfst_global_avgpool forms them (fp64 sum);
 *   bwd: dw[i] += weight gradients, dx (+)= sum_i conv(dy[i], mirrored w[i]) [+ plane_mean_grad[n][c] / (H W), the pool's adjoint]:
 *        x read once, every dy[i] once, dx written once. */
int pfst_dwconv3x3_multi_ok(int H, int W, int ns, const int* dils);
int pfst_dwconv3x3_multi_fwd(const float* x, long long x_bs, int ns, const float* const* w, float* const* y, const long long* y_bs,
                             float* const* stats, int stats_minmax, const int* dils, float* plane_mean, int N, int C, int H, int W,
                             pfst_stream_t stream);
int pfst_dwconv3x3_multi_bwd(const float* x, long long x_bs, int ns, const float* const* w, const float* const* dy,
                             const long long* dy_bs, float* const* dw, const int* dils, const float* plane_mean_grad, float* dx,
                             long long dx_bs, int accumulate, const float* const* bn_pre, const pfst_bn_bwd_rec_t* const* bn_rec,
                             int N, int C, int H, int W, pfst_stream_t stream);
/* bn_pre / bn_rec != NULL (all branches or none): as in pfst_dwconv3x3_bwd, per branch (bn_pre[i] has dy[i]'s batch stride) */
/* both gradients of the depthwise convolution in one pass over dy and the forward input x (autograd of the same F.conv2d(groups = C)):
 * dx (+)= conv(dy, mirrored w), dw += sum dy * shifted x -- 3 N of HBM traffic instead of the two kernels' 4 N */
int pfst_dwconv3x3_bwd(const float* dy, long long dy_bs, const float* x, long long x_bs, const float* w, float* dx, long long dx_bs,
                       float* dw, int N, int C, int H, int W, int dil, int accumulate, const float* bn_on_load_coef,
                       const float* bn_pre, long long bn_pre_bs, const pfst_bn_bwd_rec_t* bn_rec, pfst_stream_t stream);
/* (bn_on_load_coef as in pfst_dwconv3x3: x holds the pre-normalisation tensor, its quads are normalised as they are loaded)
 * bn_rec != NULL: dy is the gradient of the BatchNorm + ReLU OUTPUT of this depthwise layer, bn_pre the layer's pre-normalisation tensor
 * (the depthwise convolution's own output): dL/dpre is formed while the rows are staged (pfst_bn_backward_sums ran before) */

/* ---- BatchNorm2d, training mode (nn.BatchNorm2d inside mmcv ConvModule; eps 1e-5, momentum .1) */
/* batch mean / 1/sqrt(biased var + eps) per channel; updates running stats (unbiased var) when
 * running_mean != NULL.  ws: >= 2*C doubles of scratch. */
int pfst_bn_stats(const float* x, long long x_bs, int N, int C, int HW, float* mean, float* invstd,
                  float* running_mean, float* running_var, float momentum, float eps, double* ws,
                  const float* gamma, const float* beta, float* coef, pfst_stream_t stream);
/* coef != NULL (needs gamma, beta): also writes coef[C][4] = (mean, invstd, sc = invstd*gamma, sh = beta - mean*sc), the per-channel
 * record the fused BatchNorm-backward sums of a data-gradient launch read (pfst_bnb_fuse_t) */
/* the same from the conv epilogue's partials[C][T][2] (count = N*H*W elements per channel) */
int pfst_bn_finalize_partials(const float* partials, int T, int C, double count, float* mean, float* invstd,
                              float* running_mean, float* running_var, float momentum, float eps,
                              const float* gamma, const float* beta, float* coef, const float* minmax, int relu, float* y_amax,
                              pfst_stream_t stream);
/* minmax != NULL (with gamma, beta, y_amax): the producer's [C][T][2] (minimum, maximum) partials (pfst_conv_igemm_f16x3 stats_minmax).  BatchNorm
 * [+ ReLU] is monotone per channel, so the extreme outputs are the images of the extreme inputs: the slot group y_amax receives
 * max |[relu](bn(x))| -- exactly what pfst_bn_apply(..., y_amax) would publish -- without the normalised tensor being written. */
/* y = [relu]( (x-mean)*invstd*gamma + beta [+ residual] ).  relu_mask != NULL (needs relu, HW % 256 == 0, 16-byte aligned planes):
 * also writes the ReLU gate as a bitmask of N*C*HW/64 words for pfst_bn_backward -- the backward of a residual layer then reads
 * 1 bit per element instead of the fp32 output y in both of its passes. */
int pfst_bn_apply(const float* x, long long x_bs, const float* residual, long long res_bs, float* y, long long y_bs,
                  const float* mean, const float* invstd, const float* gamma, const float* beta,
                  int N, int C, int HW, int relu, unsigned long long* relu_mask, float* y_amax, const float* post_scale,
                  const float* residual_coef, pfst_stream_t stream);
/* residual_coef: NULL, or coef [C][4] = (mean, invstd, sc, sh) of the downsample conv -> BN layer (no ReLU, resnet.py:298-303) whose
 * PRE-normalisation output `residual` then is: normalised as it is loaded, the normalised identity branch is never written */
/* y_amax: NULL, or the slot group (1024 floats, zeroed) that receives max |y|: the scale of an f16x3 GEMM reading y.
 * post_scale: NULL, or [N][C] factors y is multiplied by after the ReLU -- nn.Dropout2d's keep / (1 - p) mask of the layer feeding conv_seg
 * (decode_head.py:103-107,242-247) folded into this pass (no residual then) */
/* backward of the above: dz = dy * (y > 0 if relu); dres (+)= dz; dgamma += sum dz*xhat; dbeta += sum dz;
 * dx = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)).  ws: >= 2*C doubles.  The ReLU gate comes from relu_mask (as written by
 * pfst_bn_apply), else from the saved output y; if both are NULL and beta != NULL (layer without residual) it is recomputed from
 * x exactly as bn_apply did. */
int pfst_bn_backward(const float* dy, long long dy_bs, const float* y, long long y_bs, const float* x, long long x_bs,
                     const float* mean, const float* invstd, const float* gamma, const float* beta,
                     float* dx, long long dx_bs, float* dres, long long dres_bs, int dres_accumulate,
                     float* dgamma, float* dbeta, int N, int C, int HW, int relu, const unsigned long long* relu_mask,
                     double* ws, const float* bwd_partials, int bwd_slots, float* dx_amax, const float* post_scale, pfst_stream_t stream);
/* post_scale: the factors pfst_bn_apply folded into y: dy is the gradient of the SCALED output, dz = dy * post_scale[n][c] * gate (no dres, no
 * bwd_partials then) */
/* Two BatchNorm layers behind ONE gated gradient -- the last BN of a stage's first Bottleneck (a: bn3) and its downsample branch's BN (b),
 * out = relu(bn3(conv3(.)) + bn_d(conv_d(x))), resnet.py:298-307: both receive g = (relu_mask bit ? dy : 0).  One reduction pass over
 * (dy, xa, xb) and one apply pass writing dxa and dxb replace the two pfst_bn_backward calls (8 N instead of 10 N of traffic); the results
 * are those of pfst_bn_backward(relu = 1, relu_mask) per layer.  bwd_partials_a: layer a's sums from the launch that wrote dy (as in
 * pfst_bn_backward).  ws_a, ws_b: >= 2*C doubles each.  Needs HW % 256 == 0 and 16-byte aligned planes; PFST_ERR_UNSUPPORTED otherwise and in
 * deterministic mode (the caller then runs the layers one by one). */
int pfst_bn_backward_dual(const float* dy, long long dy_bs, const unsigned long long* relu_mask,
                          const float* xa, long long xa_bs, const float* mean_a, const float* invstd_a, const float* gamma_a,
                          float* dxa, long long dxa_bs, float* dgamma_a, float* dbeta_a, double* ws_a,
                          const float* bwd_partials_a, int bwd_slots_a, float* dxa_amax,
                          const float* xb, long long xb_bs, const float* mean_b, const float* invstd_b, const float* gamma_b,
                          float* dxb, long long dxb_bs, float* dgamma_b, float* dbeta_b, double* ws_b, float* dxb_amax,
                          int N, int C, int HW, pfst_stream_t stream);
/* The FIRST half of pfst_bn_backward alone, for a conv -> BN -> ReLU layer without residual whose convolution is depthwise: the two sums
 * (from bwd_partials, else by the reduction pass), dgamma += sum dz*xhat, dbeta += sum dz, and rec[C] for the consumer that applies the
 * second half while it loads dy and x (no dx is written here: 3 N of traffic less per layer).  ws: >= 2*C doubles. */
/* out (+)= (bit ? g : 0) with the ReLU bitmask pfst_bn_apply wrote (HW % 256 == 0): the gated identity-branch gradient of a residual block
 * written out by itself -- the product folds it into conv1's data-gradient epilogue (pfst_conv_igemm_f16x3 gate_dy); this is the fallback
 * when another reader needs the gradient first */
int pfst_relu_gate(const float* g, long long g_bs, const unsigned long long* relu_mask, float* out, long long out_bs, int N, int C, int HW,
                   int accumulate, pfst_stream_t stream);
int pfst_bn_backward_sums(const float* dy, long long dy_bs, const float* x, long long x_bs, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, float* dgamma, float* dbeta, int N, int C, int HW,
                          double* ws, const float* bwd_partials, int bwd_slots, pfst_bn_bwd_rec_t* rec, pfst_stream_t stream);
/* bwd_partials != NULL: (sum dz, sum dz*x) were already produced by the launch that wrote dy (pfst_bnb_fuse_t, [C][bwd_slots][2]); the
 * reduction pass over dy and x is skipped and only the partials are summed (fp64). */

/* ---- pooling / resize ---------------------------------------------------------------------- */
/* nn.MaxPool2d(3, 2, 1) (resnet.py:638); idx holds the winning tap 0..8 */
int pfst_maxpool3x3s2(const float* x, float* y, unsigned char* idx, int NC, int H, int W, int Ho, int Wo, const float* bn_on_load_coef, int C,
                      float* y_amax, pfst_stream_t stream);
/* bn_on_load_coef: NULL, or coef[C][4] = (mean, invstd, sc, sh) (pfst_bn_finalize_partials / pfst_bn_stats) of the conv -> BN -> ReLU layer
 * in front of the pool: x is then that layer's PRE-normalisation output (NC = N * C planes) and y = maxpool(relu(x * sc + sh)) -- the
 * normalised tensor is never written (its only consumer is the pool) */
int pfst_maxpool3x3s2_bwd(const float* dy, const unsigned char* idx, float* dx, int NC, int H, int W, int Ho, int Wo, pfst_stream_t stream);
/* F.interpolate(mode='bilinear', align_corners=False) (ops/wrappers.py:27) and its adjoint */
int pfst_resize_bilinear(const float* x, long long x_bs, float* y, long long y_bs, int N, int C, int Hi, int Wi, int Ho, int Wo, pfst_stream_t stream);
int pfst_resize_bilinear_bwd(const float* dy, long long dy_bs, float* dx, long long dx_bs, int N, int C, int Hi, int Wi, int Ho, int Wo, int accumulate, pfst_stream_t stream);
/* nn.AdaptiveAvgPool2d(1) (aspp_head.py:69-77): y[n][c] = mean_hw x */
int pfst_global_avgpool(const float* x, long long x_bs, float* y, int N, int C, int HW, pfst_stream_t stream);
/* dx[n][c][hw] (+)= dy[n][c] * scale */
int pfst_broadcast_hw(const float* v, float* y, long long y_bs, int N, int C, int HW, float scale, int accumulate, float* y_amax,
                      pfst_stream_t stream);
/* y_amax (both): NULL, or the slot group (1024 floats, zeroed) that receives max |y| of what the launch writes (f16x3 scale, csrc/amax.h) */
/* v[n][c] = sum_hw dy[n][c][hw]  (adjoint of the 1x1 -> HxW bilinear broadcast) */
int pfst_reduce_hw(const float* dy, long long dy_bs, float* v, int N, int C, int HW, pfst_stream_t stream);
/* ---- plane <-> pyramid of small grids (csrc/pyramid.hip): PSPHead's pooling pyramid (psp_head.py:9-50) both ways.
 * K <= PFST_PYR_MAX_SCALES grids of s_k x s_k cells, 1 <= s_k <= PFST_PYR_MAX_SCALE (`scales`, `chan_off`: HOST arrays of K ints; the grid
 * pointers: HOST arrays of K device pointers, grid k dense [N][C][s_k][s_k]).  S1 = sum_k s_k.  Tables (DEVICE, built by the host once per
 * (H, W, scales), pfst_amd.hip_ops.pyramid_operator): op_h [S1][H] / op_w [S1][W] the dense per-axis operator D, row off1[k] + i = cell
 * row / column i of scale k; span_* [S1][2] the [begin, end) of each row's non-zeros; tspan_h [K][H][2] / tspan_w [K][W][2] the
 * [begin, end) of the cells of scale k whose operator row is non-zero at that pixel row / column.  No atomics, fixed summation order. */
#define PFST_PYR_MAX_SCALES 6
#define PFST_PYR_MAX_SCALE 8
/* outs[k][n][c] = Dh_k . X . Dw_k^T.  shared != 0: X = x[n][chan_off[0] + c] for every scale, read once (AdaptiveAvgPool2d(s_k) of one tensor);
 * shared == 0: X = x[n][chan_off[k] + c] (the adjoint of the resize into the concat slices).  x: dense planes, batch stride x_bs. */
int pfst_pyramid_reduce(const float* x, long long x_bs, int N, int C, int H, int W, int K, const int* scales, const int* chan_off, int shared,
                        const float* op_h, const float* op_w, const int* span_h, const int* span_w, float* const* outs, pfst_stream_t stream);
/* sliced == 0: y[n][c] = (accumulate ? y : 0) + (add ? add[n][c] : 0) + sum_k Dh_k^T . G_k . Dw_k (the adjoint of the pooling, written once);
 * sliced != 0: y[n][chan_off[k] + c] = (accumulate ? y : 0) + Dh_k^T . G_k . Dw_k for every k (the bilinear resize of each grid into its slice
 * of the concat; add must be NULL).  y_amax: NULL, or the slot group that receives max |y| of what is written (not with accumulate). */
int pfst_pyramid_expand(const float* const* grids, int N, int C, int H, int W, int K, const int* scales, const int* chan_off, int sliced, float* y,
                        long long y_bs, const float* add, long long add_bs, int accumulate, const float* op_h, const float* op_w,
                        const int* tspan_h, const int* tspan_w, float* y_amax, pfst_stream_t stream);
/* y[n][0:CHW] = (accumulate ? y : 0) + x[n][0:CHW] between two dense-plane views (the identity slice of a concat buffer and its adjoint);
 * y_amax as above */
int pfst_copy_planes(const float* x, long long x_bs, float* y, long long y_bs, int N, long long CHW, int accumulate, float* y_amax,
                     pfst_stream_t stream);
/* ---- the top-down path of a feature pyramid (csrc/fpn.hip): UPerHead's merges and multi-level concat (uper_head.py:108-132).  Bilinear,
 * align_corners=False, any Hc x Wc -> Hf x Wf with Hf >= Hc, Wf >= Wc; dense planes with batch strides; no atomics, fixed summation order.
 * Every value is bit-identical to what pfst_resize_bilinear / pfst_resize_bilinear_bwd give for the same planes. */
#define PFST_FPN_MAX_LEVELS 3
/* out[n][c] = lat[n][c] + resize(coarse[n][c] -> Hf x Wf): the resize's value and ONE rounded fp32 add.  out is a buffer of its own (not lat, not
 * coarse).  y_amax: NULL, or the slot group that receives max |out|.  Adjoint: d_lat = d_out, d_coarse (+)= pfst_resize_bilinear_bwd(d_out). */
int pfst_topdown_merge(const float* lat, long long lat_bs, const float* coarse, long long coarse_bs, float* out, long long out_bs, int N, int C,
                       int Hc, int Wc, int Hf, int Wf, float* y_amax, pfst_stream_t stream);
/* y[n][chan_off[k] + c] = resize(srcs[k][n][c] -> Hf x Wf) for K <= PFST_FPN_MAX_LEVELS levels in one launch.  srcs: HOST array of K device
 * pointers; src_bs / src_h / src_w / chan_off: HOST arrays of K (batch stride, grid, first channel of the level's slice of y; the slices must
 * not overlap).  y_amax: NULL, or the slot group that receives max |y| over everything written. */
int pfst_fpn_resize_concat(const float* const* srcs, const long long* src_bs, const int* src_h, const int* src_w, const int* chan_off, int K,
                           float* y, long long y_bs, int N, int C, int Hf, int Wf, float* y_amax, pfst_stream_t stream);
/* its adjoint as a gather: d_srcs[k][n][c] = (accumulate[k] ? d_srcs[k] : 0) + resize^T(dy[n][chan_off[k] + c]) for every level in one launch */
int pfst_fpn_resize_concat_bwd(const float* dy, long long dy_bs, float* const* d_srcs, const long long* src_bs, const int* src_h, const int* src_w,
                               const int* chan_off, const int* accumulate, int K, int N, int C, int Hf, int Wf, pfst_stream_t stream);
/* the form a launch of the three takes for these operands (alignment, sizes), as the launchers decide it.  merge: 0 one pixel per thread, 1 four
 * pixels and 16-byte accesses, 2 the exact-1/2 walk; concat: 0 / 1 likewise; concat_bwd, per level: 0 the generic gather, 1 x2 on 2 x 2 blocks */
int pfst_topdown_merge_route(const float* lat, long long lat_bs, const float* coarse, long long coarse_bs, const float* out, long long out_bs,
                             int Hc, int Wc, int Hf, int Wf);
int pfst_fpn_resize_concat_route(const float* y, long long y_bs, int Hf, int Wf);
int pfst_fpn_resize_concat_bwd_route(const float* dy_plane, long long dy_bs, const float* d_src, long long src_bs, int Hc, int Wc, int Hf, int Wf);
/* ---- Semantic FPN (csrc/fpn.hip): the FPN neck's nearest top-down path (necks/fpn.py) and FPNHead's level sum
 * (decode_heads/fpn_head.py).  The conventions above hold: dense planes with batch strides, no atomics, one summation order.
 * out[n][c][y][x] = lat[n][c][y][x] + coarse[n][c][sy(y)][sx(x)] with torch's legacy 'nearest' rule for a given output size,
 * s(dst) = min((int)floorf(dst * scale), in - 1), scale = (float)in / (float)out in fp32: ONE rounded fp32 add, the bits of
 * lat + F.interpolate(coarse, size, mode='nearest').  out is a buffer of its own; Hf >= Hc, Wf >= Wc.  y_amax: NULL, or the slot group that
 * receives max |out|.  Adjoint: d_lat = d_out, d_coarse (+)= pfst_nearest_resize_bwd(d_out). */
int pfst_topdown_merge_nearest(const float* lat, long long lat_bs, const float* coarse, long long coarse_bs, float* out, long long out_bs, int N,
                               int C, int Hc, int Wc, int Hf, int Wf, float* y_amax, pfst_stream_t stream);
/* the adjoint of that resize as a gather: dx[s] = (accumulate ? dx[s] : 0) + the plain fp32 sum of dy over the pre-image of s -- a contiguous row
 * range times a contiguous column range (the rule is monotone), its ends found with the forward's own expression; rows ascending, columns
 * ascending within a row */
int pfst_nearest_resize_bwd(const float* dy, long long dy_bs, float* dx, long long dx_bs, int N, int C, int Hc, int Wc, int Hf, int Wf,
                            int accumulate, pfst_stream_t stream);
/* out = bilinear_x2(act(pre)) on Hc x Wc -> 2 Hc x 2 Wc, act(v) = max(fma(v, sc, sh), 0) with (sc, sh) = coef[c][2], coef[c][3] of a [C, 4] table
 * (mean, invstd, sc, sh) -- the record a deferred conv -> BN -> ReLU layer leaves; coef NULL: the values are final.  Bit-identical to pfst_bn_apply
 * followed by pfst_resize_bilinear.  y_amax: NULL, or the slot group that receives max |out|.  Adjoint: pfst_resize_bilinear_bwd. */
int pfst_upsample2x_norm(const float* pre, long long pre_bs, const float* coef, float* out, long long out_bs, int N, int C, int Hc, int Wc,
                         float* y_amax, pfst_stream_t stream);
/* out = act0(pre0) + bilinear_x2((act1(m1) + act2(m2)) + act3(m3)) [+ addend] on H0 x W0, the K <= PFST_FPN_MAX_LEVELS members on exactly
 * (H0 / 2, W0 / 2); summed in the order written, so bit-identical to pfst_bn_apply per operand, K - 1 fp32 adds on the half grid,
 * pfst_resize_bilinear, one add, and one more for the addend.  K = 0: out = act0(pre0) [+ addend], any H0 x W0.  members / member_bs /
 * member_coef: HOST arrays of K (device pointers, batch strides, tables or NULL); coef0 / addend may be NULL.  y_amax as above.  No adjoint kernel:
 * d_pre0's upstream is d_out, every member's is ONE pfst_resize_bilinear_bwd(d_out). */
int pfst_fpn_level_sum(const float* pre0, long long pre0_bs, const float* coef0, const float* const* members, const long long* member_bs,
                       const float* const* member_coef, int K, const float* addend, long long addend_bs, float* out, long long out_bs, int N, int C,
                       int H0, int W0, float* y_amax, pfst_stream_t stream);
/* the form a launch of the four takes.  merge_nearest: 0 one pixel per thread, 1 four pixels with 16-byte accesses, 2 the exact x2 form (a coarse
 * value feeds a 2 x 2 block); nearest_resize_bwd: 0 the generic gather, 1 x2 on 2 x 2 blocks; upsample2x_norm: 0 the pixel form, 1 the x2 walk;
 * fpn_level_sum: 0 the pixel form, 1 16-byte accesses (the x2 walk, or for K = 0 a flat pass) */
int pfst_topdown_merge_nearest_route(const float* lat, long long lat_bs, const float* coarse, long long coarse_bs, const float* out,
                                     long long out_bs, int Hc, int Wc, int Hf, int Wf);
int pfst_nearest_resize_bwd_route(const float* dy, long long dy_bs, const float* dx, long long dx_bs, int Hc, int Wc, int Hf, int Wf);
int pfst_upsample2x_norm_route(const float* pre, long long pre_bs, const float* out, long long out_bs, int Hc, int Wc);
int pfst_fpn_level_sum_route(const float* pre0, long long pre0_bs, const float* const* members, const long long* member_bs, int K,
                             const float* addend, long long addend_bs, const float* out, long long out_bs, int H0, int W0);
/* ---- HRNet's exchange unit (csrc/hrnet.hip): the sum that ends every HRModule (backbones/hrnet.py:199-213).  The
 * conventions above hold: bilinear, align_corners=False, dense planes with batch strides, no atomics, one summation order.
 * out[n][c] = max(((t_0 + t_1) + t_2) + t_3, 0) over B <= PFST_HR_MAX_BRANCHES operands in the order given, one rounded fp32 add each.  ops /
 * op_bs / op_coef / op_h / op_w: HOST arrays of B (device pointer, batch stride, [C, 4] table (mean, invstd, sc, sh) or NULL, grid).  An operand
 * on the output grid contributes fma(v, sc, sh) (no ReLU), or v itself under a NULL table; an operand on exactly (Hf / r, Wf / r), r in {2, 4, 8}
 * -- at most PFST_FPN_MAX_LEVELS of them -- contributes the bilinear interpolation of its normalised values.  Bit-identical to pfst_bn_apply
 * (relu = 0) per tabled operand, pfst_resize_bilinear per coarser one, the adds in that order and a ReLU.  out is a buffer of its own.  y_amax:
 * NULL, or the slot group that receives max |out|. */
#define PFST_HR_MAX_BRANCHES 4
int pfst_hr_fuse(const float* const* ops, const long long* op_bs, const float* const* op_coef, const int* op_h, const int* op_w, int B, float* out,
                 long long out_bs, int N, int C, int Hf, int Wf, float* y_amax, pfst_stream_t stream);
/* its adjoint in at most two launches: gy = (out > 0 ? d_out : 0), the upstream gradient of EVERY output-grid operand (gy may be d_out itself),
 * then d_coarse[k] = (accumulate[k] ? d_coarse[k] : 0) + resize^T(gy) for the K <= PFST_FPN_MAX_LEVELS coarser operands in one gather launch, each
 * bit-identical to pfst_resize_bilinear_bwd(gy).  d_coarse / coarse_bs / coarse_h / coarse_w / accumulate: HOST arrays of K (unread for K = 0).  The
 * tabled operands' BatchNorm backward is pfst_bn_backward from their pre-normalisation tensors. */
int pfst_hr_fuse_bwd(const float* d_out, long long d_out_bs, const float* out, long long out_bs, float* gy, long long gy_bs, float* const* d_coarse,
                     const long long* coarse_bs, const int* coarse_h, const int* coarse_w, const int* accumulate, int K, int N, int C, int Hf,
                     int Wf, pfst_stream_t stream);
/* the form a pfst_hr_fuse launch takes: 0 one pixel per thread, 1 four pixels with 16-byte accesses (Wf % 4 == 0; out and every output-grid operand
 * 16-byte aligned with a batch stride % 4 == 0) */
int pfst_hr_fuse_route(const float* const* ops, const long long* op_bs, const int* op_h, const int* op_w, int B, const float* out, long long out_bs,
                       int Hf, int Wf);
/* F.interpolate(mode='nearest') by an integer factor on [NC][h][w] maps and its adjoint (pfgst_loss.py:57-58) */
int pfst_upsample_nearest(const float* x, float* y, int NC, int h, int w, int factor, pfst_stream_t stream);
int pfst_upsample_nearest_bwd(const float* dy, float* dx, int NC, int h, int w, int factor, pfst_stream_t stream);
/* nn.Dropout2d (decode_head.py:103-107): y = x * mask[n][c] */
int pfst_channel_scale(const float* x, const float* mask, float* y, int N, int C, int HW, pfst_stream_t stream);
/* ---- test-time inference beyond the whole-image arg-max (rsiseg/models/segmentors/encoder_decoder.py): sliding windows, flips, averaging */
/* F.softmax(seg_logit, dim=1) (:311) with torch's arithmetic: y[n][c][p] = exp(x - max_c) / sum_c exp(x - max_c) */
int pfst_softmax_nchw(const float* x, long long x_bs, float* y, long long y_bs, int N, int C, int HW, pfst_stream_t stream);
/* slide_inference (:220-263): preds[:, :, y1:y1+Hc, x1:x1+Wc] += crop (F.pad + add, :246-248), count[:, y1:.., x1:..] += 1 (:250) */
int pfst_window_accumulate(const float* crop, float* preds, float* count, int N, int C, int Hc, int Wc, int H, int W, int y1, int x1,
                           pfst_stream_t stream);
int pfst_window_normalize(float* preds, const float* count, int N, int C, int HW, pfst_stream_t stream);      /* preds / count_mat (:256) */
/* seg_logit.argmax(dim=1) (:332, :368): first maximal class per pixel, the first NaN class if there is one (torch.argmax), uint8 */
int pfst_argmax_nchw(const float* x, long long x_bs, unsigned char* label_u8, int N, int C, int HW, pfst_stream_t stream);
/* output.flip(dims=(3,)) / (2,) (:316-325) on `planes` H x W maps, out of place */
int pfst_flip_planes(const float* x, float* y, int planes, int H, int W, int horizontal, int vertical, pfst_stream_t stream);
int pfst_div_scalar(float* x, long long n, float divisor, pfst_stream_t stream);                              /* seg_logit /= len(imgs) (:367) */
/* aug_test (:355-372), one view in one pass, bit-identical to the chain resize_bilinear (src Hs x Ws -> input grid Hm x Wm; skipped when
 * equal) -> resize_bilinear (-> ori_shape Ho x Wo; skipped when equal) -> softmax_nchw -> flip_planes -> acc = (accumulate ? acc : 0) + probs.
 * src: [N][C][Hs][Ws] with batch stride src_bs (the 1/4 logits, or slide mode's input-size map with Hs x Ws = Hm x Wm); acc: dense
 * [N][C][Ho][Wo].  C <= PFST_TTA_MAX_C (larger C: -1, the caller runs the chain). */
#define PFST_TTA_MAX_C 32
int pfst_tta_accumulate(const float* src, long long src_bs, int N, int C, int Hs, int Ws, int Hm, int Wm, int Ho, int Wo, int hflip, int vflip,
                        float* acc, int accumulate, pfst_stream_t stream);
/* seg_logit /= views, then seg_logit.argmax(dim=1) (:367-368) in one pass: labels equal to pfst_div_scalar + pfst_argmax_nchw's */
int pfst_tta_finalize(const float* acc, int N, int C, int HW, int views, unsigned char* label_u8, pfst_stream_t stream);

/* ---- whole-scene prediction (pfst_amd/scene.py): slide_inference (:220-263) over a uint8 scene resident on the device, the windows forwarded
 * in batches.  win_yx is a HOST array of B (y1, x1) pairs, B <= PFST_SCENE_MAX_WINDOWS: the offsets travel by value in the kernel arguments
 * (no copy, no synchronisation); every window of size h x w must lie inside the H x W scene. */
#define PFST_SCENE_MAX_WINDOWS 16
/* out[b][c][i][j] = (scene[y1_b + i][x1_b + j][to_rgb ? 2 - c : c] - mean[c]) / std[c], float32 [B][3][h][w]: mmcv.imnormalize
 * (pfst_amd.pipeline.normalize) of each window of the H x W x 3 uint8 scene (BGR as read), transposed to CHW, bit for bit */
int pfst_scene_windows(const unsigned char* scene_u8, int H, int W, const int* win_yx, int B, int h, int w, float mean0, float mean1, float mean2,
                       float std0, float std1, float std2, int to_rgb, float* out, pfst_stream_t stream);
/* sums[C][H][W] += the batch's window logits resized to h x w, window by window in index order: bit-identical to B x (pfst_resize_bilinear of
 * logits[b] ([C][hl][wl], batch stride logits_bs) to h x w, then pfst_window_accumulate at (y1_b, x1_b)).  Pixels that no window of the
 * batch covers are neither read nor written.  Any C >= 1. */
int pfst_scene_accumulate(const float* logits, long long logits_bs, int B, int C, int hl, int wl, const int* win_yx, int h, int w, float* sums,
                          int H, int W, pfst_stream_t stream);
/* sums -> label_u8 [H][W] (+ conf_u8 [H][W] = rint(p_max * 255), + probs [C][H][W]; either may be NULL): sums / count, softmax, first maximal
 * class -- bit-identical to pfst_window_normalize -> pfst_softmax_nchw -> pfst_argmax_nchw.  The cover count of (y, x) is
 * row_count[y] * col_count[x] (device int tables of H and W entries, all >= 1); there is no H x W count plane. */
int pfst_scene_finalize(const float* sums, int C, int H, int W, const int* row_count, const int* col_count, unsigned char* label_u8,
                        unsigned char* conf_u8, float* probs, pfst_stream_t stream);
/* BaseSegmentor.show_result (segmentors/base.py:278-285): out_rgb[H][W][3] = palette_rgb[label] (colours <= 256 rows; labels beyond: 0), or with
 * scene_bgr (H x W x 3 uint8, BGR) uint8(img * keep + colour * opacity) per channel in double arithmetic, truncated, img in RGB order;
 * keep = 1 - opacity formed in double by the caller.  Bit-identical to the NumPy expression for every opacity in [0, 1]. */
int pfst_paint_labels(const unsigned char* label_u8, int H, int W, const unsigned char* palette_rgb, int colours, const unsigned char* scene_bgr,
                      double keep, double opacity, unsigned char* out_rgb, pfst_stream_t stream);

/* ---- test-time augmentation on whole scenes (pfst_amd/scene.py predict_scene_tta): aug_test (:355-372) over slide_inference, the views of
 * MultiScaleFlipAug with img_scale=None (test_time_aug.py:98-126).  scene_tta.hip. */
/* out_u8 [Hr][Wr][3] = the bilinear resize of src_u8 [h][w][3] (pfst_amd.pipeline.resize_bilinear_u8 / pfst_cpu_resize_window_u8, bit for bit),
 * written mirrored horizontally / vertically when asked (RandomFlip after Resize).  y_index / x_index: DEVICE int tables [2][Hr] / [2][Wr], the
 * lower then the upper source index of every output row / column; y_frac / x_frac: device float tables [Hr] / [Wr], the weight of the upper
 * index -- pipeline._src_index's, so the geometry has one definition (indices are clamped into the source).  Equal sizes: an exact copy. */
int pfst_scene_resize_u8(const unsigned char* src_u8, int h, int w, const int* y_index, const float* y_frac, const int* x_index, const float* x_frac,
                         int Hr, int Wr, int hflip, int vflip, unsigned char* out_u8, pfst_stream_t stream);
/* one view in one pass: acc [C][H][W] = (accumulate ? acc : 0) + flip(softmax(resize(sums / count, (H, W)))), bit-identical to the chain
 * pfst_window_normalize -> pfst_resize_bilinear (skipped when Hr x Wr = H x W) -> pfst_softmax_nchw -> pfst_flip_planes -> pfst_axpy_f32.  sums:
 * the view's window sums [C][Hr][Wr]; its cover count at (y, x) is row_count[y] * col_count[x] (device int tables, all >= 1): neither a count
 * plane nor a normalised copy of the sums is written.  C <= PFST_TTA_MAX_C (larger C: -1, the caller runs the chain). */
int pfst_scene_tta_accumulate(const float* sums, int C, int Hr, int Wr, const int* row_count, const int* col_count, int hflip, int vflip, float* acc,
                              int H, int W, int accumulate, pfst_stream_t stream);
/* acc / views -> label_u8 [H][W], the first maximal class (+ conf_u8 = rint(p_max * 255), + probs [C][H][W] = acc / views; either may be NULL):
 * bit-identical to pfst_div_scalar -> pfst_argmax_nchw.  Any C <= 255; acc is left as it is. */
int pfst_scene_tta_finalize(const float* acc, int C, int H, int W, int views, unsigned char* label_u8, unsigned char* conf_u8, float* probs,
                            pfst_stream_t stream);

/* ---- fused bilinear-upsample + softmax cross-entropy + accuracy (decode_head.py:249-283,
 * cross_entropy_loss.py:45-65, accuracy.py:6-61).  logits are [N][C][h][w]; labels/weights [N][H][W].
 * acc[0] += sum_i w_i*cw[y_i]*nll_i (0 at ignore), acc[1] += #correct, acc[2] += #non-ignored, acc[3] += #labels that are neither
 * in [0, C) nor ignore_index (F.cross_entropy raises on those; pfst_ce_finalize reports the count so the caller can).  acc: 4 doubles.
 * lse[N][H][W] (log-sum-exp of the upsampled logits) is saved for the backward. */
int pfst_ce_upsample_fwd(const float* logits, int N, int C, int h, int w, const unsigned char* label, const float* pix_weight,
                         const float* class_weight, int H, int W, int ignore_index, float* lse, double* acc, pfst_stream_t stream);
/* dlogits[n][c][ly][lx] (+)= scale * sum_p bilin(p->l) * w_p*cw[y_p] * (softmax_c(p) - [c==y_p]) */
int pfst_ce_upsample_bwd(const float* logits, int N, int C, int h, int w, const unsigned char* label, const float* pix_weight,
                         const float* class_weight, int H, int W, int ignore_index, const float* lse, float scale,
                         float* dlogits, int accumulate, pfst_stream_t stream);

/* ---- pseudo labels (pfgst.py:259-268 + encoder_decoder.py:77-81): bilinear upsample of the teacher
 * logits, softmax (exp(z - max) / sum as torch computes it), then torch.max over the PROBABILITIES: the first class whose
 * rounded probability is maximal (not the arg-max of the logits: distinct logits may tie after rounding); prob >= threshold
 * counted into count[0].  conf_mask (0/1 per pixel) and max_prob (the softmax value itself) may be NULL. */
int pfst_pseudo_label(const float* logits, int N, int C, int h, int w, int H, int W, float threshold,
                      long long* label_i64, unsigned char* label_u8, unsigned long long* count, float* conf_mask, float* max_prob,
                      pfst_stream_t stream);

/* ---- offline pseudo-labels with class-wise entropy thresholds (core/hook/pseudo_labeling_hookv4.py:173-205, datasets/pipelines/loading.py:475-494;
 * DESIGN.md 8i).  logits [N][C][h][w] are resized bilinearly (align_corners=False) to H x W per pixel, in registers (H == h: identity);
 * p = exp(z - max) / sum.  C <= 255.
 *   mode 0 (the hook): pred = the first class whose rounded p is maximal, entropy = -sum p log p (a term with p == 0 is 0)
 *   mode 1 (the loader): pred = the first maximal logit, entropy = -sum p log(p + 1e-8)
 * Entropies are >= +0, never -0.  ent [N][H][W] float and pred [N][H][W] uint8 may each be NULL (not both). */
int pfst_entropy_upsample(const float* logits, int N, int C, int h, int w, int H, int W, int mode, float* ent, unsigned char* pred,
                          pfst_stream_t stream);
/* One level of an exact radix select over the mode-0 entropies per predicted class: ADDS, for every pixel, one count at
 * hist[pred][(key >> shift) & ((1 << bits) - 1)], key = the fp32 bit pattern of the entropy (unsigned order = value order).  With prefix
 * (unsigned 32-bit [C]; needs shift + bits < 32) only pixels with key >> (shift + bits) == prefix[pred] count.  hist: unsigned 64-bit
 * [C][1 << bits], never cleared here; integer counters, so the result does not depend on launch, image or stream order.  1 <= bits <= 16;
 * the counting is privatised in LDS where C << bits <= 12288 and goes through global atomics otherwise. */
int pfst_entropy_class_hist(const float* logits, int N, int C, int h, int w, int H, int W, int shift, int bits, const unsigned int* prefix,
                            unsigned long long* hist, pfst_stream_t stream);
/* label [N][H][W] uint8 = mode-1 pred where the mode-1 entropy < thr[pred] (float [C]), else 255; with annotation_space = 1 instead pred + 1
 * and 0 (files that LoadAnnotations(reduce_zero_label=True) reads back as pred / 255).  counts: unsigned 64-bit [C][2], ADDED to:
 * (pixels predicted c, pixels kept as c). */
int pfst_entropy_pseudo_label(const float* logits, int N, int C, int h, int w, int H, int W, const float* thr, int annotation_space,
                              unsigned char* label, unsigned long long* counts, pfst_stream_t stream);

/* ---- OHEMPixelSampler (core/seg/sampler/ohem_pixel_sampler.py): the 0/1 pixel-weight map of online hard example mining from
 * logits [N][C][h][w], resized bilinearly (align_corners=False) to H x W per pixel in registers, and label [N][H][W].  A pixel is valid where
 * its label is neither ignore_index nor outside [0, C).  The whole sequence (key pass, three histogram levels of an exact radix select whose
 * digits are chosen on the device, weight pass) is enqueued on `stream` from device pointers only; nothing is read on the host.
 *   has_thresh = 1: key = the softmax probability of the label, exp(z_y - max) / sum; s = the valid keys in ascending order,
 *                   k = min(batch_kept, n_valid - 1), threshold = max(s[k], thresh); weight = 1 where valid and key < threshold.
 *                   Where at least k + 1 keys are <= thresh the threshold is thresh and the select's passes return at once.
 *   has_thresh = 0: key = coef[y] * max(lse - z_y, 0), coef float [C] >= 0 (the sum over the head's CE terms of loss_weight * class_weight);
 *                   the k = min(batch_kept, n_valid) valid pixels of largest key get weight 1: every key above the cut value, and of the
 *                   pixels equal to it the first in raster order (n, y, x) until exactly k are kept.
 * weight [N][H][W] float, 16-byte aligned, holds the keys (-1 at pixels that are not valid) between the passes and the 0 / 1 map at the end.
 * info: 4 x 64-bit = (bit pattern of the fp32 threshold / cut value, n_valid, n_kept, k).  keys_out [N][H][W] (or NULL) receives a copy of the
 * key map, for tests and diagnosis.  workspace: pfst_ohem_workspace_bytes bytes, 8-byte aligned, any contents. */
int pfst_ohem_workspace_bytes(int N, int H, int W, long long* bytes);
int pfst_ohem_sample(const float* logits, int N, int C, int h, int w, const unsigned char* label, int H, int W, int ignore_index,
                     int has_thresh, float thresh, long long batch_kept, const float* coef, void* workspace, float* weight, long long* info,
                     float* keys_out, pfst_stream_t stream);

/* ---- evaluation: intersect_and_union (rsiseg/core/evaluation/metrics.py:26-86).  hist[3*C] (+)= per-class
 * #intersect, #pred, #label over pixels whose label != ignore_index (caller zeroes hist once per evaluation) */
int pfst_confusion_hist(const unsigned char* pred, const unsigned char* label, long long n, int C, int ignore_index,
                        unsigned long long* hist, pfst_stream_t stream);

/* ---- class mix (dacs_transforms.py:110-144, pfgst.py:281-300) ------------------------------- */
/* presence[v] = 1 if label value v occurs (torch.unique over the batch) */
int pfst_label_presence(const unsigned char* label, long long n, int* presence256, pfst_stream_t stream);
/* mask[n][p] = 1 if gt[n][p] is one of classes[n][0..K) (entries < 0 are padding) */
int pfst_class_mask(const unsigned char* gt, const int* classes, int K, unsigned char* mask, int N, long long HW, pfst_stream_t stream);
/* mixed = M*src + (1-M)*trg for image, label and pixel weight; the target weight is the scalar
 * q = conf_count[0] / (N*HW) (thre_type 'all') or, if trg_weight != NULL, the per-pixel map (thre_type 'part',
 * conf_mask of pfst_pseudo_label).  mixed_lbl_i64 may be NULL. */
int pfst_class_mix(const float* img, const float* trg_img, const unsigned char* gt, const unsigned char* pseudo,
                   const unsigned char* mask, const unsigned long long* conf_count, const float* trg_weight, float* mixed_img,
                   unsigned char* mixed_lbl, long long* mixed_lbl_i64, float* mixed_w, int N, int Cimg, long long HW, pfst_stream_t stream);

/* ---- DACS strong augmentation of the mixed image (dacs_transforms.py:44-107; kornia arithmetic restated,
 * parity unpinned).  params[n][8] = brightness, contrast, saturation, hue(rad), order[4] (0..3 = b,c,s,h) */
int pfst_color_jitter(float* img, const float* params, const float* mean3, const float* std3, int N, long long HW,
                      int denorm, pfst_stream_t stream);
/* separable gaussian blur, reflect border; taps_*[n][K*] per image; taps farther than `reach` from the centre are skipped */
int pfst_gaussian_blur(const float* x, float* tmp, float* y, const float* taps_y, int Ky, const float* taps_x, int Kx,
                       int N, int C, int H, int W, int reach, pfst_stream_t stream);

/* ---- PFGSTLoss (pfgst_loss.py:44-234), kernel K x K for ksize K in {3, 5, 7} ------------------------------------
 * Tap order (nn.Unfold(K, dilation dil, padding r*dil)): k = (dy+r)*ksize + (dx+r), r = ksize/2, neighbour offset (dy*dil, dx*dil),
 * dy, dx in [-r, r]; maps with taps are [N][ksize*ksize][H][W].  The mirror tap of k is ksize*ksize-1-k: pixel r is that tap of its
 * k-neighbour r+D_k.  A neighbour in the zero-padding band has label 0 (a real class) and similarity against a zero vector.
 * Every entry with a `ksize` argument refuses values outside {3, 5, 7}.
 *
 * Similarity map, 3x3 (the shipped configs: strip kernels for the cosine type on whole-row 256-pixel strips, generic kernels otherwise):
 * sim_type 0: sim[n][k][y][x] = cos(f[n][:,y,x], f[n][:,y+dy_k,x+dx_k]) (0 outside); norm[n][y][x] = |f|
 * sim_type 1: sim = exp(-|f(neighbour) - f(centre)|^2 / sigma^2), the zero padding counting as f = 0 (pfgst_loss.py:199-201) */
int pfst_sim_map(const float* feat, int N, int C, int H, int W, int dil, int sim_type, float sigma, float* sim, float* norm,
                 pfst_stream_t stream);
/* d feat (+)= adjoint of pfst_sim_map for upstream gradient gsim[n][9][H][W] */
int pfst_sim_map_bwd(const float* feat, const float* sim, const float* norm, const float* gsim, int N, int C, int H, int W, int dil,
                     int sim_type, float sigma, float* dfeat, int accumulate, float* coef_ws, pfst_stream_t stream);
/* coef_ws: 10*N*H*W floats of scratch (per-pixel stencil coefficients) for the strip kernel of the cosine path; NULL selects the
 * generic kernel */
/* Similarity map and adjoint, K x K, any map size: (16 + 2*r*dil)^2 halo tiles staged in LDS, so r*dil <= 37 */
int pfst_sim_map_k(const float* feat, int N, int C, int H, int W, int ksize, int dil, int sim_type, float sigma, float* sim, float* norm,
                   pfst_stream_t stream);
/* coef_ws (required, both sim types): (ksize*ksize + 1)*N*H*W floats of scratch (per-pixel stencil coefficients) */
int pfst_sim_map_bwd_k(const float* feat, const float* sim, const float* norm, const float* gsim, int N, int C, int H, int W, int ksize,
                       int dil, int sim_type, float sigma, float* dfeat, int accumulate, float* coef_ws, pfst_stream_t stream);
/* source statistics: sets (neighbour label == / != centre label, centre != 255) of src sims.
 * gt is full resolution [N][Hg][Wg] uint8, nearest-sampled to HxW.
 * loss_type 0 (mean_std): stats[0..5] = n_pos, sum_pos, sumsq_pos, n_neg, sum_neg, sumsq_neg
 * loss_type 1 / 2 (margin / margin2, pfgst_loss.py:116-131): stats[1] = sum relu(margin_pos - s)^e over positive pairs,
 *   stats[4] = sum relu(s - margin_neg)^e over negative pairs, e = loss_type */
int pfst_src_sim_stats(const float* sim, const unsigned char* gt, int N, int H, int W, int Hg, int Wg, int ksize, int dil, int loss_type,
                       float margin_pos, float margin_neg, double* stats, const void* select, pfst_stream_t stream);
/* loss_type 0: losses[0..3] = -w*mean_pos, w*mean_neg, w*std_pos, w*std_neg; 1 / 2: losses[0..1] = w_pos*mean hinge_pos,
 * w_neg*mean hinge_neg (losses[2..3] = 0); gsim = d(sum of the losses)/d sim */
int pfst_src_sim_grad(const float* sim, const unsigned char* gt, int N, int H, int W, int Hg, int Wg, int ksize, int dil, int loss_type,
                      float margin_pos, float margin_neg, const double* stats,
                      float w_pos, float w_neg, float w_pos_std, float w_neg_std, float* gsim, float* losses, const void* select, pfst_stream_t stream);
/* src_perc (pfgst_loss.py:98-102: only the int(n * src_perc) smallest positive / largest negative similarities enter the source
 * losses): pfst_src_sim_select finds, with an exact radix select and no sort, the threshold value of each set and the share of its
 * ties that lies inside the sorted prefix; pass the filled `select` buffer (pfst_src_sim_select_bytes() bytes, 8-byte aligned) to
 * pfst_src_sim_stats / pfst_src_sim_grad, or NULL for all pairs. */
int pfst_src_sim_select_bytes(void);
int pfst_src_sim_select(const float* sim, const unsigned char* gt, int N, int H, int W, int Hg, int Wg, int ksize, int dil, double src_perc,
                        void* select, pfst_stream_t stream);
/* prob[n][c][y][x] = softmax_c(logits[n][c][y*ds][x*ds]) (nearest down-scaling by ds) */
int pfst_softmax_down(const float* logits, int N, int C, int h, int w, int ds, float* prob, int H, int W, pfst_stream_t stream);
/* valid = (gt != 255) && all ksize*ksize dilated neighbours inside the map and un-mixed; all_in = the second condition alone;
 * count[0] = #valid */
int pfst_trg_valid_mask(const unsigned char* gt, const unsigned char* mix_mask, int N, int H, int W, int Hg, int Wg, int ksize, int dil,
                        unsigned char* valid, unsigned char* all_in, unsigned long long* count, pfst_stream_t stream);
/* top-k target losses, 0 <= top_k <= ksize*ksize - 1 (0: all pairs, the reference's top_k=None); acc[0] += sum loc_pos,
 * acc[1] += sum loc_neg over valid pixels; gP[n][k][y][x] = d(w_pos*mean loc_pos + w_neg*mean loc_neg)/d cross_prob (0 when
 * count <= 1).  Ranks: stable descending similarity, the lower tap index first on ties; the top-(top_k+1) and bottom-top_k sets
 * may overlap (2*top_k + 1 > ksize*ksize): a pair in both counts in both losses and both gradient terms.
 * g_sim != NULL: also d(losses)/d ema_sim [N][ksize*ksize][H][W] -- needed only when the similarity has trainable inputs (proj_net) */
int pfst_sim_topk_loss(const float* ema_sim, const float* prob, const unsigned char* valid, const unsigned long long* count,
                       int N, int C, int H, int W, int ksize, int dil, int top_k, float w_pos, float w_neg, float* gP, double* acc,
                       float* g_sim, pfst_stream_t stream);
/* d logits[n][c][y*ds][x*ds] += softmax-backward( sum_k gP[k] * prob_c(neighbour k) ); unfold_grad != 0 (detach_unfold=False)
 * adds the gradient through the unfolded factor: coefficient gP[k][r] + gP[ksize*ksize-1-k][r+D_k] */
int pfst_cross_prob_bwd(const float* prob, const float* gP, int N, int C, int H, int W, int ksize, int dil, int ds, int unfold_grad,
                        float* dlogits, int h, int w, pfst_stream_t stream);
/* out[0] = w_pos*acc[0]/((top_k+1)*count), out[1] = w_neg*acc[1]/(top_k*count); top_k = 0: both /(ksize*ksize*count)  (zeros when
 * count <= 1); top_k as for pfst_sim_topk_loss */
int pfst_sim_loss_finalize(const double* acc, const unsigned long long* count, int ksize, int top_k, float w_pos, float w_neg, float* out,
                           pfst_stream_t stream);
/* Pair statistics of a similarity map against a prediction and an annotation: the counters of the reference's PlotStatisticsHook
 * (rsiseg/core/hook/plot_statistics_hook.py), restated in DESIGN.md 8g.  sim: [N][ksize^2][H][W] as pfst_sim_map / pfst_sim_map_k write it;
 * pred [N][Hp][Wp] and gt [N][Hg][Wg] uint8 (gt 255 = ignore), nearest-sampled to H x W.  A centre pixel counts when all its ksize^2 taps lie
 * inside the map and its gt is not 255.  edges: bins + 1 ascending floats on the device, 1 <= bins <= 256.
 * counters (unsigned 64-bit, ADDED to, never cleared here), pfst_sim_pair_stats_counters(ksize, bins) of them, in this order:
 *   hist[4][bins + 2]   per case 0 (1a: pred same, gt same), 1 (1b: pred same, gt different), 2 (2b: both different), 3 (2a: pred different,
 *                       gt same) the similarities of (correctly predicted centre, non-centre tap with gt != 255): slot #{edges <= s} - 1,
 *                       s == edges[bins] in the last bin; slot bins: s < edges[0]; slot bins + 1: s > edges[bins] (or NaN)
 *   rank[ksize^2 - 1][2] per rank of a non-centre tap in its centre's order (descending similarity, stable, lower tap first on ties, as
 *                       pfst_sim_topk_loss): [0] taps with the centre's gt, [1] taps with another gt; taps with gt 255 keep their rank and
 *                       count nowhere
 *   n_centres, n_correct_centres */
int pfst_sim_pair_stats_counters(int ksize, int bins);
int pfst_sim_pair_stats(const float* sim, const unsigned char* pred, const unsigned char* gt, int N, int H, int W, int Hp, int Wp, int Hg, int Wg,
                        int ksize, int dil, const float* edges, int bins, unsigned long long* counters, pfst_stream_t stream);

/* ---- EMA teacher + AdamW + SGD on flat parameter arenas (pfgst.py:105-127, torch.optim.AdamW / SGD) ------ */
int pfst_ema_update(float* teacher, const float* student, long long n, float alpha, pfst_stream_t stream);
int pfst_adamw_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int step, float grad_scale, pfst_stream_t stream);
/* torch.optim.SGD, single-tensor form, maximize=False: d = g*grad_scale + weight_decay*p; with momentum != 0: buf = d when first_step, else
 * momentum*buf + (1-dampening)*d, then d = d + momentum*buf (nesterov) or buf; p -= lr*d.  Each of these sums with a scaled term is one
 * fused multiply-add, as in torch's add(alpha) kernels; momentum*buf rounds on its own.  buf is null iff momentum == 0.  Pointers that are
 * all 16-byte aligned (a ParamArena) take the float4 body, others the scalar loop. */
int pfst_sgd_step(float* p, const float* g, float* buf, long long n, float lr, float momentum, float dampening,
                  float weight_decay, int nesterov, int first_step, float grad_scale, pfst_stream_t stream);

/* ---- loss bookkeeping (base.py:177-222) ------------------------------------------------------- */
/* out[0] = loss_weight*acc[0]/numel ; out[1] = 100*(acc[1]+eps)/(acc[2]+eps) ; out[2] = acc[3] (count of invalid labels) */
int pfst_ce_finalize(const double* acc, double numel, float loss_weight, float* out, pfst_stream_t stream);

/* ---- fused bilinear upsample + softmax + Dice loss (losses/dice_loss.py behind decode_head.py:249-283) ----
 * p = softmax(up(logits)), t = one_hot(min(label, C-1)), valid = label != ignore_index (the LOSS's); per image n and class c
 *   I = sum valid*t_c*p_c,  P = sum p_c^e,  T = sum t_c  (P, T over every pixel);  num = 2I + smooth, den = P + T + smooth,
 *   loss = loss_weight/C * sum_{c != ignore_index} cw_c * mean_n (1 - num/den).
 * form: 0 = generic kernels (any H x W, C <= 255), 4 / 8 = inter-cell block kernels (H == form*h, W == form*w, C <= 8, lse 8-byte and
 * label 2-byte aligned).  Exactly one of lse_in (read: the CE term's) and lse_out[N][H][W] (written) is set.  Every workgroup STORES one row
 * of partials, no atomics: slab[N][blocks][C][2] = (I, P), counts[N][blocks][C+3] = (T per class, #correct, #valid, #bad labels), the last
 * three as pfst_ce_upsample_fwd counts them under head_ignore_index (bad: label >= C that is neither ignore index).
 * blocks: form 0: ceil(H*W/1024); form 4: ceil((w+1)/16)*ceil((h+1)/32); form 8: ceil((w+1)/16)*ceil((h+1)/16). */
int pfst_dice_upsample_fwd(const float* logits, int N, int C, int h, int w, const unsigned char* label, int H, int W,
                           int ignore_index, int head_ignore_index, float exponent, int form, const float* lse_in, float* lse_out,
                           double* slab, long long* counts, int blocks, pfst_stream_t stream);
/* adds the rows in a fixed order: sums[N*C*3 + 3] = (I, P, T) per (n, c), then (#correct, #valid, #bad);
 * coef[N][C][2] = (a, b) = (k*2/den, k*e*num/den^2), k = cw_c/(C*N), zeros for c == ignore_index; out[3] laid out as pfst_ce_finalize's */
int pfst_dice_finalize(const double* slab, const long long* counts, int N, int C, int blocks, const float* class_weight,
                       int ignore_index, double smooth, double exponent, double loss_weight, double* sums, float* coef, float* out,
                       pfst_stream_t stream);
/* dlogits (+)= scale * adjoint of the resize applied to p_c*(g_c - sum_k g_k p_k), g_c = -a*valid*t_c + b*p_c^(e-1); gather form, no
 * atomics.  work[N][H][W] is needed by the generic form at C > 8 only. */
int pfst_dice_upsample_bwd(const float* logits, int N, int C, int h, int w, const unsigned char* label, int H, int W,
                           int ignore_index, float exponent, int form, const float* lse, const float* coef, float scale,
                           float* work, float* dlogits, int accumulate, pfst_stream_t stream);

/* ---- fused bilinear upsample + per-(pixel, class) logistic losses: FocalLoss (losses/focal_loss.py:13-68) and CrossEntropyLoss(use_sigmoid)
 * (cross_entropy_loss.py:68-156) behind decode_head.py:249-283 ----
 * x = up(logits), t = [label == c], y = t ? -x : x, q = sigmoid(y), b = softplus(y), k = coef[c][t ? 0 : 1] (coef[C][2] = (k_pos, k_neg)):
 *   l = k q^gamma b, summed with pix_weight (NULL: 1) over the pixels with label != ignore_index and label < C; no softmax across classes.
 * form: 0 = generic kernels (any H x W, C <= 255), 4 / 8 = inter-cell block kernels (H == form*h, W == form*w, C <= 8, pix_weight 8-byte and
 * label 2-byte aligned).  Every workgroup STORES one row of partials, no atomics: slab[N][blocks][C] = the class's weighted loss sum,
 * counts[N][blocks][3] = (#correct, #valid, #bad labels) as pfst_ce_upsample_fwd counts them.  gamma >= 0 (NaN: -1).
 * blocks: form 0: ceil(H*W/1024); form 4: ceil((w+1)/16)*ceil((h+1)/32); form 8: ceil((w+1)/16)*ceil((h+1)/16). */
int pfst_sigloss_upsample_fwd(const float* logits, int N, int C, int h, int w, const unsigned char* label, const float* pix_weight,
                              int H, int W, int ignore_index, const float* coef, float gamma, int form, double* slab,
                              long long* counts, int blocks, pfst_stream_t stream);
/* adds the rows in a fixed order: sums[N*C + 3] = the loss sum per (n, c), then (#correct, #valid, #bad);
 * out[3] = (loss_weight / divisor * sum, acc_seg %, #bad) laid out as pfst_ce_finalize's */
int pfst_sigloss_finalize(const double* slab, const long long* counts, int N, int C, int blocks, double divisor, double loss_weight,
                          double* sums, float* out, pfst_stream_t stream);
/* dlogits (+)= scale * adjoint of the resize applied to pix_weight * valid * dl/dx, dl/dx = (t ? -1 : 1) k q^gamma (q + gamma (1 - q) b);
 * gather form, no atomics, no full-resolution buffer at any C */
int pfst_sigloss_upsample_bwd(const float* logits, int N, int C, int h, int w, const unsigned char* label, const float* pix_weight,
                              int H, int W, int ignore_index, const float* coef, float gamma, int form, float scale, float* dlogits,
                              int accumulate, pfst_stream_t stream);

/* ---- fused bilinear upsample + softmax + Lovasz-Softmax loss (losses/lovasz_loss.py behind decode_head.py:249-283), csrc/lovasz_loss.hip ----
 * The class set is `slot` (int [C] on the device: the class's slot 0 .. K-1, or -1) and `cls` (int [K]: the class of a slot).  Segments: one
 * per slot over the batch (per_image = 0: K segments of N*H*W elements) or one per (image, slot) (per_image = 1: N*K segments of H*W).
 * workspace: pfst_lovasz_workspace_bytes(segments, elements per segment) bytes, 16-byte aligned, any contents; it carries the (key, value)
 * ping-pong buffers, the digit histograms and the per-tile partials from pfst_lovasz_keys to pfst_lovasz_finalize.
 * counters: 3 + N*K 64-bit words = (#correct, #valid, #bad labels, foreground count per (image, slot)), zeroed by pfst_lovasz_keys. */
int pfst_lovasz_workspace_bytes(int segments, long long seg_stride, long long* bytes);
/* The sort on its own: a stable ascending LSD radix sort (8-bit digits, 4 passes) of 32-bit keys in `segments` independent segments; segment
 * s holds elements [s*seg_stride, s*seg_stride + len_s), len_s = seg_len[s] (device int [segments], clamped to [0, seg_stride]; NULL: every
 * segment is full).  vals_in NULL: the value of an element is its index in its segment (vals_out is then the permutation).  Equal keys keep
 * their input order; elements at and beyond len_s of the outputs are not written.  keys_out == keys_in (and vals) is allowed. */
int pfst_lovasz_sort(const unsigned int* keys_in, const unsigned int* vals_in, int segments, long long seg_stride, const int* seg_len,
                     void* workspace, unsigned int* keys_out, unsigned int* vals_out, pfst_stream_t stream);
/* key pass: acc_seg / bad-label counts, the log-sum-exp map (exactly one of lse_in / lse_out [N][H][W], as pfst_dice_upsample_fwd) and, per
 * slot and pixel, key = 0x3F800000 - bits(e), e = |fg - min(p_c, 1)| (0x3F800001 where label == ignore_index: behind every valid key) and
 * value = pixel index in the segment (n, y, x order) | foreground << 31, into the workspace.  form: as pfst_dice_upsample_fwd. */
int pfst_lovasz_keys(const float* logits, int N, int C, int h, int w, const unsigned char* label, int H, int W, int ignore_index,
                     int form, const int* slot, int K, int per_image, const float* lse_in, float* lse_out, void* workspace,
                     long long* counters, pfst_stream_t stream);
/* sorts the workspace's segments in place (descending error, equal errors by ascending pixel index) */
int pfst_lovasz_sort_keys(int N, int H, int W, int K, int per_image, void* workspace, pfst_stream_t stream);
/* over the sorted order: g_k = J_k - J_{k-1} (lovasz_grad), coef_map[N][K][H][W] = sign(fg - p) * slot_weight[slot] * g_k at valid pixels
 * (others are not written), and the per-tile fp64 partials of sum e_k g_k, in a fixed order (no atomics).  slot_weight: float [K] or NULL */
int pfst_lovasz_grad(int N, int H, int W, int K, int per_image, const long long* counters, const float* slot_weight, void* workspace,
                     float* coef_map, pfst_stream_t stream);
/* sums[segments] = sum e_k g_k per segment; the class mean over the kept slots (mode_present: those with foreground among the segment's valid
 * pixels), per image when per_image (reduction 0: mean over N, 1: sum); no kept slot: 0.  scale[N][K] = what the backward multiplies
 * coef_map with (0 for a skipped slot); out[3] = (loss_weight * loss, acc_seg %, #bad labels) laid out as pfst_ce_finalize's */
int pfst_lovasz_finalize(int N, int H, int W, int K, int per_image, int mode_present, int reduction, const long long* counters,
                         const float* slot_weight, double loss_weight, void* workspace, double* sums, float* scale, float* out,
                         pfst_stream_t stream);
/* dlogits (+)= grad_scale * adjoint of the resize applied to p_j (d_j - sum_c d_c p_c), d_c = -scale[n][slot] coef_map[n][slot][pixel]
 * (0 outside the class set), zero at pixels with label == ignore_index; gather form, no atomics.  work[N][H][W]: generic form at C > 8 only */
int pfst_lovasz_upsample_bwd(const float* logits, int N, int C, int h, int w, const unsigned char* label, int H, int W,
                             int ignore_index, int form, const int* slot, const int* cls, int K, const float* lse,
                             const float* coef_map, const float* scale, float grad_scale, float* work, float* dlogits,
                             int accumulate, pfst_stream_t stream);

/* ---- EntropyLoss on low-resolution logits (losses/entropy_loss.py:27-42), csrc/entropy_loss.hip ----
 * logits[N][C][HW] dense, p = softmax_c(logits) = exp(z - max) / sum, one pixel per thread, no resize.
 *   kind 0 (entropy, MinEnt):  loss =  weight / (N HW) * sum_px -sum_c p_c log2(p_c + 1e-30) / log2(C)
 *   kind 1 (max_square):       loss = -weight / (2 N C HW) * sum_px sum_c p_c^2
 * 2 <= C <= 255 (C = 1: log2(1) = 0, the reference's division by zero, PFST_ERR_ARG).  form: 0 = by C (C <= 8: the logits of a pixel in
 * registers, else a loop over the classes), 1 = the loop at any C (tests compare the two on one shape; same operations, same bits).
 * workspace: pfst_softmax_entropy_workspace_bytes bytes, 8-byte aligned, any contents: N * ceil(HW / 256) fp64 partials, one STORED per
 * workgroup; a single workgroup adds them in a fixed order and writes out[0].  No atomics: bit-identical run to run in every mode. */
int pfst_softmax_entropy_workspace_bytes(int N, long long HW, long long* bytes);
int pfst_softmax_entropy_fwd(const float* logits, int N, int C, long long HW, int kind, int form, double weight, double* workspace,
                             float* out, pfst_stream_t stream);
/* dlogits (+)= grad_scale * p_j (g_j - sum_c p_c g_c) with p formed again from the logits (nothing is kept from the forward pass) and
 * g_c = dloss/dp_c:  kind 0: -(log2(p_c + 1e-30) + p_c / ((p_c + 1e-30) ln 2)) / log2(C) * weight / (N HW);  kind 1: -p_c weight / (N C HW).
 * accumulate: 0 writes, 1 adds (the value that 0 writes, exactly).  dlogits[N][C][HW] dense; it may not overlap logits */
int pfst_softmax_entropy_bwd(const float* logits, int N, int C, long long HW, int kind, int form, double weight, float grad_scale,
                             float* dlogits, int accumulate, pfst_stream_t stream);

/* ---- adversarial baseline (ADVENT): the per-class entropy map, csrc/entropy_loss.hip (losses/adv_loss.py:47-50, 77-81, 96-97) ----
 * ent[n][c][px] = -p_c log2(p_c + 1e-30) / log2(C), p = softmax_c(logits) as above: C channels at the logits' own resolution, NOT summed
 * over the classes.  logits, ent, grad_ent, dlogits: [N][C][HW] dense; 2 <= C <= 255; form as pfst_softmax_entropy_fwd.  One pixel per
 * thread, the class walk of the EntropyLoss kernels (csrc/entropy_walk.h), nothing kept between forward and backward. */
int pfst_entropy_map(const float* logits, int N, int C, long long HW, int form, float* ent, pfst_stream_t stream);
/* dlogits (+)= p_j (G_j - sum_c p_c G_c), G_c = grad_ent[c] * -(log2(p_c + 1e-30) + p_c / ((p_c + 1e-30) ln 2)) / log2(C): through the
 * entropy term and the softmax.  accumulate: 0 writes every element, 1 adds (the value that 0 writes, exactly) */
int pfst_entropy_map_bwd(const float* logits, const float* grad_ent, int N, int C, long long HW, int form, float* dlogits, int accumulate,
                         pfst_stream_t stream);

/* ---- adversarial baseline: the discriminator's convolutions, csrc/adv_conv.hip (discriminators/fc_discriminator.py:8-19) ----
 * Conv2d(kernel 4, stride 2, padding 1, bias): x[N][Cin][Hi][Wi] -> y[N][Cout][Ho][Wo], Ho = Hi / 2, Wo = Wi / 2 (floor; Hi, Wi >= 2),
 * w[Cout][Cin][4][4] in torch's layout (nothing is packed), all tensors dense fp32; N <= 16383, Cout <= 65535.  Implicit GEMMs on the
 * fp32-input MFMA, except the forward pass with Cout = 1: a reduction per output pixel (csrc/adv_tail.hip).
 *   y = act(b + conv(x, w)),  act(v) = v > 0 ? v : slope * v when act = 1 (LeakyReLU fused into the epilogue), the identity when act = 0.
 *   bias may be NULL. */
int pfst_adv_conv_fwd(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int Hi, int Wi, int Cout, int act,
                      float slope, pfst_stream_t stream);
/* dx (+)= gate * conv_transpose(dy, w): four 2x2 sub-convolutions by the parity of the input row and column; every element of dx is written.
 * x_gate (or NULL): x itself when x is the LeakyReLU output of the layer below -- gate = x > 0 ? 1 : slope, what torch's in-place
 * LeakyReLU differentiates (slope > 0: x > 0 iff its pre-activation was) -- so that dx is the gradient of that layer's PRE-activation. */
int pfst_adv_conv_dgrad(const float* dy, const float* w, const float* x_gate, float* dx, int N, int Cin, int Hi, int Wi, int Cout, float slope,
                        int accumulate, pfst_stream_t stream);
/* dw[Cout][Cin][4][4] += sum_{n, pixels} dy x, db[Cout] += sum_{n, pixels} dy (db may be NULL).  Split over images and pixel chunks
 * (pfst_wgrad_split_k); fp32 atomics, or per-slice scratch and an ordered sum under pfst_set_deterministic(1). */
int pfst_adv_conv_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int Cin, int Hi, int Wi, int Cout, pfst_stream_t stream);
/* The tail, csrc/adv_tail.hip (fc_discriminator.py:18 AdaptiveAvgPool2d(1), adv_loss.py:58-63 l1_loss): y[N][HW] is the last layer's one-channel plane.
 *   d[n] = mean_i y[n][i] (fp64 sums in a fixed order),  loss[0] = weight * mean_n |d[n] - label|,
 *   gy[n][i] = grad_scale * weight * sign(d[n] - label) / (N HW)  (sign(0) = 0, as torch's).  One workgroup, no atomics.
 * d, loss, gy: each may be NULL (at least one is not). */
int pfst_adv_tail(const float* y, int N, int HW, float label, double weight, float grad_scale, float* d, float* loss, float* gy,
                  pfst_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
