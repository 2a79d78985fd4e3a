/*
 * rag_amd.h — C ABI of librag_amd.so: the MI355X (gfx950) kernels behind the
 * RAG stereo Matching-Net forward path.
 *
 * The reference (chzhang18/RAG) is pure PyTorch and offers no FFI; its "plugin
 * API" for this path is the nn.Module composition in src/models/rag_model.py.
 * Each entry point below replaces the ATen op sequence of one reference
 * construct (cited per function); rag_amd/modules.py mirrors the reference's
 * module names/signatures on top of these calls.
 *
 * Conventions:
 *  - plain pointers and sizes, no torch types; all tensors are device pointers
 *    owned by the caller (PyTorch allocates), contiguous N-C-D-H-W planes;
 *    "bstride" arguments are batch strides in ELEMENTS so that a call may read
 *    or write a channel slice of a wider buffer (this is how torch.cat and the
 *    running sum in Cell_3d are folded into the producing kernels);
 *  - every function returns 0 on success and a negative RAGMI_E* code on
 *    failure; no C++ exception crosses the ABI; ragmi_last_error() gives a
 *    thread-local message for the last failure on this thread;
 *  - stateless and re-entrant; kernels are enqueued on the hipStream_t passed
 *    as `stream` (void*), never synchronise, never allocate device memory;
 *  - dtype selects activation storage AND the arithmetic contract of the call (no environment variable changes either):
 *      RAGMI_F32    fp32 storage, fp32 arithmetic: the contractions run on the fp32-input MFMA forms, bitwise an fmaf chain
 *                   per output (one rounding per product, fp32 accumulate);
 *      RAGMI_F32X3  fp32 storage; accepted by the 3x3x3 convolution entry points only (ragmi_conv3d_k3_fwd(_ex),
 *                   ragmi_conv3d_k3_dual_fwd(_ex)).  On shapes for which ragmi_conv3d_k3_uses_x3() answers 1 every fp32
 *                   operand is scaled by a power of two and split into two FP16 halves, a * 2^s = hi + lo + r with hi = fp16(a 2^s),
 *                   lo = fp16(a 2^s - hi), |lo| <= 2^-11 |hi|, and a product a*b is accumulated in fp32 as hi_a*hi_b + hi_a*lo_b +
 *                   lo_a*hi_b on the fp16 matrix cores (16x the fp32 MFMA rate).  The scales are exact (powers of two) and chosen by
 *                   the library: per output channel for the weights (largest |w| of the channel -> [2^9, 2^10]), per workgroup
 *                   tile for the activations (largest |x| of the tile's halo planes -> at most 2^15, 2^10..2^11 when chosen; a plane
 *                   that would overflow makes the tile restart with a larger scale — fp16's range is never exceeded).  Dropped per
 *                   product: lo_a*lo_b and the roundings of the lo halves, each <= 2^-22 |a b|, plus — fp16 has no exponents below
 *                   2^-24 — an ABSOLUTE 2^-25 of the scaled operand, i.e. 2^-35 of the tile's largest |x| (2^-34 of the channel's
 *                   largest |w|).  Per output:
 *                        |y_x3 - y_exact| <= 2^-20 * sum_k |w_k x_k| + 2^-33 * (Xmax * sum_k |w_k| + Wmax * sum_k |x_k|)
 *                                            + fp32 accumulation error
 *                   with Xmax the largest |x| in the workgroup's tile and Wmax the largest |w| of the output channel.  On
 *                   activations of one magnitude class (anything a network produces) the second term vanishes and the error is
 *                   ~1e-7 * sum |w x| (measured 9e-8 on N(0,1) data with a common offset of 1000: the class of RAGMI_F32 itself, 1.1e-7);
 *                   it matters only when operands ~2^-25 smaller than their tile's largest carry the sum (measured 1e-3 * sum |w x|
 *                   on operands spread element by element over 2^-20..2^20).  The bound is relative to the sum of |products|, not to
 *                   |y|: cancelling sums lose that many ABSOLUTE digits, as in fp32.  Non-finite inputs give non-finite outputs (an
 *                   Inf may come out as NaN); so do operands above ~2^110 in magnitude, which no scale brings into fp16's range.  With ReLU a NaN
 *                   pre-activation is stored as 0 on every route (the epilogues apply fmaxf(u, 0.f)), unlike F.relu, which keeps the NaN.  Round 2 used bf16 halves (8 bits each, ~2^-17 per product): measured over weight
 *                   seeds at the headline size that left the EPE against the CPU reference between 1e-5 and 1.4e-3 px; the fp16
 *                   halves sit on the strict fp32 path's EPE for every seed (tests/test_hip_parity.py::
 *                   test_x3_margin_over_seeds_and_genotypes_at_headline_size).
 *                   Elsewhere (small volumes, a residual input, unsupported channel counts) the call is computed exactly as
 *                   RAGMI_F32.  tests/test_hip_parity.py::test_x3_error_bound_adversarial and tests/test_conv3d_k3_sweep.py (every route and form) enforce the bound.
 *      RAGMI_BF16   bf16 activation storage (BASELINE config 3), fp32 on-chip accumulation, BN and tails; the contraction may run
 *                   on the bf16 matrix cores with the (exact) bf16 activations and hi+lo split fp32 weights — an error of
 *                   <= 2^-16 per weight, far below the 2^-8 of the storage format (both halves are rounded to nearest, which leaves
 *                   <= 2^-18 |w|: the term tests/test_conv3d_k3_sweep.py holds the split-operand kernels to under this storage).
 *    Weights, scale/shift and the final disparity are fp32 in every case.
 */
#ifndef RAG_AMD_H
#define RAG_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAGMI_OK 0
#define RAGMI_EINVAL (-1)       /* bad argument (null pointer, non-positive size, ...) */
#define RAGMI_EUNSUPPORTED (-2) /* shape / dtype combination not built */
#define RAGMI_ELAUNCH (-3)      /* hipLaunch / runtime error */

#define RAGMI_F32 0
#define RAGMI_BF16 1 /* activations stored as bf16; fp32 on chip (LDS, MFMA, accumulate, BN); weights/BN stay fp32 */
#define RAGMI_F32X3 2 /* fp32 storage, scaled-fp16 split products (hi*hi + hi*lo + lo*hi) in the eligible 3x3x3 convolutions (see the dtype note above) */

#define RAGMI_MAX_GROUPS 16 /* output-channel groups of 4 per conv call */

/* Library version (major*10000 + minor*100 + patch) and last error text. */
int ragmi_version(void);
const char* ragmi_last_error(void);

/*
 * Cost-volume build.  Replaces the inline slice-copy loop of
 * src/models/rag_model.py:375-383 (dups :694-702, src/automl/mdenas_basicmodel.py:83-91):
 *   cost[b, c,   i, y, x] = L[b, c, y, x]      if x >= i else 0
 *   cost[b, C+c, i, y, x] = R[b, c, y, x - i]  if x >= i else 0,      i in [0, d)
 * L, R: [B, C, h, w]; cost: [B, 2C, d, h, w] (fully written, no memset needed).
 */
int ragmi_costvol_fwd(const void* left_fea, const void* right_fea, void* cost,
                      int B, int C, int d, int h, int w, int dtype, void* stream);

/*
 * Weight pre-pack for ragmi_conv3d_k3_fwd: reorders an nn.Conv3d weight
 * [Cout, Cin, 3, 3, 3] (src/automl/operations_3d.py:37), Cout <= 64, into the operand
 * fragments of the matrix-core kernels.  `packed` must hold
 * ragmi_conv3d_k3_packed_elems(Cout, Cin) floats: the per-lane broadcast fragments of
 * v_mfma_f32_4x4x1_16b_f32 (RAGMI_F32), then the bf16 hi / lo fragments (RAGMI_BF16),
 * then the fp16 hi / lo fragments of w * 2^k[co] and the per-output-channel
 * multipliers 2^-k[co] (RAGMI_F32X3).  One pack serves every dtype of the convolution
 * entry points (ragmi_conv3d_k3_pack_for fills only what one contract reads).
 */
int64_t ragmi_conv3d_k3_packed_elems(int Cout, int Cin);
int ragmi_conv3d_k3_pack(const void* weight, void* packed, int Cout, int Cin, int dtype, void* stream);

/*
 * Fused ConvBR_3d, 3x3x3 / stride 1 / pad 1 (src/automl/operations_3d.py:31-47),
 * plus the running sum and channel concat of Cell_3d (src/models/rag_model.py:160-176):
 *   v    = conv3d(x, W)[co]                      (fp32, bias-free)
 *   v    = v * scale[co] + shift[co]             (folded eval BatchNorm3d; NULL scale => skip)
 *   v    = max(v, 0)                  if relu
 *   v   += res[b, res_ch(co), ...]    if res != NULL   (res may alias y: accumulate in place)
 *   y[b, y_ch(co), z, y, x] = v
 * Output channel co belongs to group g = co/4; y_ch(co) = y_group_ch[g] + co%4 when
 * y_group_ch != NULL (host array of ceil(Cout/4) ints), else co; same for res_group_ch.
 * Sibling convolutions that read the same input are fused by concatenating their
 * weights along Cout and pointing each group at its own destination channels.
 * x: [B, Cin, D, H, W] with batch stride x_bstride; y/res likewise.
 */
int ragmi_conv3d_k3_fwd(const void* x, int64_t x_bstride,
                        const void* packed_weight, const void* scale, const void* shift, int relu,
                        void* y, int64_t y_bstride, const int32_t* y_group_ch,
                        const void* res, int64_t res_bstride, const int32_t* res_group_ch,
                        int B, int Cin, int Cout, int D, int H, int W,
                        int dtype, void* stream);

/*
 * Consumer 1x1x1 ConvBR_3d fused into the producing 3x3x3 kernel's epilogue (a "tail"):
 *   y_t[b, y_ch0 + j] = act(bn_t(sum_c W_t[j][c] * out[b, c]))       j < cout <= 4
 * where out is the (activated, summed) result of the 3x3x3 call it is attached to.  This is how the level-3
 * Cell_3d.pre_preprocess / preprocess convs (rag_model.py:125-126, 154-155) of the NEXT cells are computed by the
 * stem / cell that produces their input, instead of as separate HBM-bound passes.  weight: raw [cout][Cout_main].
 */
typedef struct {
  const void* weight;
  const void* scale;   /* folded BN of the tail, or NULL/NULL */
  const void* shift;
  int32_t relu;
  void* y;
  int64_t y_bstride;
  int32_t y_ch0;
  int32_t cout;
} ragmi_tail_t;
/* `relu` bit 0: ReLU after the BatchNorm.  `relu` bit 1 (value 2): a DOWN-SAMPLING tail — the 1x1x1 ConvBR_3d of a consumer cell that
 * works one level down (Cell_3d with downup_sample = -1: F.interpolate(x, half size, 'trilinear', align_corners=True) followed by
 * pre_preprocess / preprocess, rag_model.py:146-155), computed conv-first in the producer's epilogue: y is [B, *, D/2, H/2, W/2].
 * Up to two of them (4 output channels each) beside up to two full-resolution tails; only the z-marching split-operand form takes
 * them (ragmi_conv3d_k3_uses_x3 with RAGMI_F32X3 or RAGMI_BF16, <= 12 input channels) and only for even D, H, W whose x0.5 source
 * pairs are aligned (ragmi_down2_tail_supported: output o reads inputs (2o, 2o+1) on every axis; the last may clamp). */
int ragmi_down2_tail_supported(int D, int H, int W);

/* Channel-group-interleaved tensors ("G4"): [B][C/4][D][H][W][4] fp32 — the four channels of a group of a voxel are 16 contiguous
 * bytes — instead of channel planes [B][C][D][H][W].  A PRIVATE layout of the fused executor (rag_amd.MatchingNet._run_chain) for
 * the level-3 tensors its own kernels exchange (the 8-channel s0|s1 inputs of the dual cells, stem3d0's output): every module
 * boundary of the reference (rag_model.py:143-177, 325-366) keeps channel planes.  Why: on gfx950 the vector memory path costs per
 * INSTRUCTION; in G4 a halo voxel of a group is one 16-byte load and a fused tail one 16-byte store instead of four 4-byte ones into
 * four planes (profiles/r05_x3_stamps.md).  Flags (fp32 storage, or bf16 storage: four bf16 = one 8-byte access; RAGMI_EUNSUPPORTED where the kernel a call lands on does not
 * take them — ask ragmi_conv3d_k3_g4_caps first):
 *   `relu` argument of ragmi_conv3d_k3_fwd_ex / _dual_fwd_ex:  bit 1 (RAGMI_CONV_X_G4): x is G4 (x_bstride in floats, as ever);
 *   ragmi_tail_t.relu bit 2 (RAGMI_TAIL_G4): the tail's destination y is G4; y_ch0 (a multiple of 4) names the group y_ch0 / 4; the
 *                  tail must have exactly 4 output channels.  All full-resolution tails of a call agree; down-sampling tails are planes.
 *   `relu` argument of ragmi_costvol_stem_fwd: bit 2 (RAGMI_CONV_Y_G4): y (Cout a multiple of 4) is G4; its tails as above. */
#define RAGMI_CONV_RELU 1
#define RAGMI_CONV_X_G4 2
#define RAGMI_CONV_Y_G4 4
#define RAGMI_TAIL_G4 4
/* Mixed storage (round 5, BASELINE configs[2]): bf16 storage is kept for the full-resolution (level-3) tensors only — the deep levels and
 * the head are fp32 (tests/analysis_bf16_stage_epe.py: they carry most of the bf16 error and almost none of the bytes).  Two edges cross:
 *   ragmi_tail_t.relu bit 3 (RAGMI_TAIL_F32): the destination of this DOWN-SAMPLING tail is fp32 (y_bstride in floats) although the
 *                  call's storage is RAGMI_BF16 (ignored under fp32 storage; RAGMI_EINVAL on a full-resolution tail);
 *   dtype RAGMI_BF16 | RAGMI_OUT_F32 of ragmi_conv3d_k1_resample_fwd: x is bf16, y is fp32 (same arithmetic: fp32 on chip). */
#define RAGMI_TAIL_F32 8
/* ragmi_costvol_stem_conv3d_fwd only, tails0[0].relu bit 4 (RAGMI_TAIL_ROWS): this tail (4 output channels on stem3d0's 12) is NOT evaluated
 * from `weight` by the combine kernel but falls out of stem3d1's matrix product: the caller packed stem3d1's weight as a SIXTEEN-channel
 * convolution whose rows 12..15 hold the tail's weights at the centre tap (zero elsewhere) — rows the 12-channel product leaves idle.  Cout
 * stays 12; the tail's scale / shift / relu / y are used as ever, its products are split-operand ones like the convolution's (the
 * RAGMI_F32X3 bound) instead of an exact fp32 chain. */
#define RAGMI_TAIL_ROWS 16
#define RAGMI_OUT_F32 0x100
/* bit mask: 1 = this call accepts a G4 input, 2 = it can write G4 full-resolution tails (arguments as ragmi_conv3d_k3_uses_x3) */
int ragmi_conv3d_k3_g4_caps(int Cin, int Cout, int B, int D, int H, int W, int nset, int ntail, int ndown, int dtype);

/* Quarter store (round 6).  store_main bit 1 (RAGMI_STORE_QUARTER_ROWS, with bit 0) of ragmi_conv3d_k3_dual_fwd_ex: the ONLY reader of the
 * main output y is a x0.25 trilinear align_corners=True resample (F.interpolate to [D/4, H/4, W/4], Cell_3d's pre_preprocess input two
 * levels down, rag_model.py:146-155).  That resample reads two source indices per output and axis, both inside the aligned group
 * [4X, 4X + 3], so the launch writes only the planes and rows that are some output's source and leaves every other (plane, row) of y
 * UNWRITTEN; what it writes is bit for bit what the full store writes there.  A PRIVATE contract of the fused executor, like G4.
 * Taken only where ragmi_conv3d_k3_quarter_store_supported says so (RAGMI_EUNSUPPORTED otherwise): RAGMI_F32X3, a 12-channel level-3
 * dual launch with down-sampling tails and no full-resolution ones, D, H, W multiples of 4 with D, H <= 256, and a work list whose
 * items (half items included) all start on a multiple of 4 planes and span at most 32.  Arguments as ragmi_conv3d_k3_g4_caps. */
#define RAGMI_STORE_QUARTER_ROWS 2
int ragmi_conv3d_k3_quarter_store_supported(int Cin, int Cout, int B, int D, int H, int W, int nset, int ntail, int ndown, int dtype);
/* used[i] (n_in bytes) = 1 where source index i of an axis of n_in = 4 * n_out voxels is read by that resample (the set the launch above
 * writes, per axis: planes and rows); returns 0 when n_in is no multiple of 4, below 8, or a source pair leaves its aligned group. */
int ragmi_quarter_store_rows(int n_in, unsigned char* used);

/*
 * ragmi_conv3d_k3_fwd / ragmi_conv3d_k3_dual_fwd with up to two full-resolution tails (plus up to two down-sampling ones).  store_main = 0 skips writing the 3x3x3
 * result itself (only the tails consume it).  Tails need Cout in {4, 8, 12, 16} (all channels in one workgroup).
 */
int ragmi_conv3d_k3_fwd_ex(const void* x, int64_t x_bstride,
                           const void* packed_weight, const void* scale, const void* shift, int relu,
                           void* y, int64_t y_bstride, const int32_t* y_group_ch,
                           const void* res, int64_t res_bstride, const int32_t* res_group_ch,
                           int B, int Cin, int Cout, int D, int H, int W,
                           int store_main, int ntail, const ragmi_tail_t* tails, int dtype, void* stream);
int ragmi_conv3d_k3_dual_fwd_ex(const void* x, int64_t x_bstride,
                                int CinA, const void* packedA, const void* scaleA, const void* shiftA,
                                int CinB, const void* packedB, const void* scaleB, const void* shiftB,
                                int relu, void* y, int64_t y_bstride, const int32_t* y_group_ch,
                                const void* res, int64_t res_bstride, const int32_t* res_group_ch,
                                int B, int Cout, int D, int H, int W,
                                int store_main, int ntail, const ragmi_tail_t* tails, int dtype, void* stream);

/*
 * Same operation as ragmi_conv3d_k3_fwd for Cout <= 2 (last_3_3d: 12 -> 1, rag_model.py:269), computed with
 * v_fma and wave-uniform weights instead of MFMA (a 4-row MFMA tile would idle 3 rows at Cout = 1).
 * `weight` is the RAW nn.Conv3d weight [Cout, Cin, 3, 3, 3]; Cin must be a multiple of 4.
 * Writes y[b, y_ch0 + co]; res (optional) is read at res_ch0 + co.
 */
int ragmi_conv3d_k3_small_fwd(const void* x, int64_t x_bstride, const void* weight, const void* scale,
                              const void* shift, int relu, void* y, int64_t y_bstride, int y_ch0,
                              const void* res, int64_t res_bstride, int res_ch0,
                              int B, int Cin, int Cout, int D, int H, int W, int dtype, void* stream);

/* The same with the output stored in its own dtype: y_dtype == dtype, or RAGMI_F32 out of RAGMI_BF16 input — the head's `mat`
 * (rag_model.py:365), which the soft-argmin consumes at |cost| ~ 1e4, stays fp32 under bf16 activation storage.
 * res, when given, has the INPUT dtype. */
int ragmi_conv3d_k3_small_fwd_ex(const void* x, int64_t x_bstride, const void* weight, const void* scale,
                                 const void* shift, int relu, void* y, int64_t y_bstride, int y_ch0,
                                 const void* res, int64_t res_bstride, int res_ch0,
                                 int B, int Cin, int Cout, int D, int H, int W, int dtype, int y_dtype, void* stream);

/*
 * Two sibling ConvBR_3d groups fused into one launch (Cell_3d with two conv branches per new
 * state, rag_model.py:160-172):
 *   y[b, y_ch(co)] = act(bnA(convA(x[:, 0:CinA])))[co] + act(bnB(convB(x[:, CinA:CinA+CinB])))[co] (+ res)
 * x holds both inputs as consecutive channels (CinA a multiple of 4); packedA / packedB are
 * ragmi_conv3d_k3_pack outputs for [Cout, CinA, 3,3,3] and [Cout, CinB, 3,3,3].  Other arguments
 * as ragmi_conv3d_k3_fwd.  The running sum never touches HBM.
 */
int ragmi_conv3d_k3_dual_fwd(const void* x, int64_t x_bstride,
                             int CinA, const void* packedA, const void* scaleA, const void* shiftA,
                             int CinB, const void* packedB, const void* scaleB, const void* shiftB,
                             int relu, void* y, int64_t y_bstride, const int32_t* y_group_ch,
                             const void* res, int64_t res_bstride, const int32_t* res_group_ch,
                             int B, int Cout, int D, int H, int W, int dtype, void* stream);

/*
 * Introspection for profiling: which kernel instantiation(s) ragmi_conv3d_k3_fwd will launch
 * for this shape (nset = 1, or 2 for ragmi_conv3d_k3_dual_fwd).  Writes the x-tile log2 width and rows per lane, and the output groups per
 * workgroup (G) into launch_groups[0]; returns the number of launches (1) or a negative error
 * code.  Kernel name: conv3d_k3_kernel<G, log_tx, rows_per_lane, NSET> (NSET 1, or 2 for _dual).
 */
int ragmi_conv3d_k3_plan(int Cout, int B, int D, int H, int W, int nset, int32_t* log_tx,
                         int32_t* rows_per_lane, int32_t* launch_groups, int32_t max_launches);

/*
 * Fused ConvBR_3d, 1x1x1 (Cell_3d.pre_preprocess / preprocess, rag_model.py:125-126,
 * last_6_3d / last_12_3d :270-271): channel mix + folded BN + ReLU, HBM-bound.
 * weight: raw nn.Conv3d weight [Cout, Cin] (1x1x1 squeezed), row-major.
 * Writes y[b, y_ch0 + co, ...].
 *
 * Accuracy of the kernels of pointwise.hip, resample.hip, conv2d_strided.hip and of ragmi_cell2d_fwd's staging (enforced per
 * element against float64 by tests/test_pointwise_resample_sweep.py; mag = sum |w| * |operand|, A = the interpolation of |x| with
 * the same weights):
 *   trilinear interpolation               3 * 2^-23 * A                (three nested lerps: one product and one fma rounding each;
 *                                                                       indices and lambdas are ATen's fp32 rule, common.h)
 *   1x1x1 fmaf chain over n channels      (n + 1) * 2^-24 * mag
 *   resample + 1x1x1                      sum_ci |w| * 3 * 2^-23 * A_ci + (Cin + 1) * 2^-24 * sum_ci |w| * A_ci
 *   strided 3x3 (ragmi_conv2d_k3_strided) (9 Cin + 1) * 2^-24 * mag
 *   folded BatchNorm                      |scale| * arith + 2^-23 * (|scale * pre| + |shift|); ReLU leaves a bound unchanged
 *   bf16 storage                          + 2^-8 * |result| per stored tensor
 *   ragmi_add_fwd                         exact: the correctly rounded sum in the storage type
 *   ragmi_cell2d_fwd                      s0 / s1 within the resample + 1x1x1 + BatchNorm bound b_s; the 3x3 convolutions within
 *                                         conv(b_s, |w3|) + the RAGMI_F32X3 bound; then BatchNorm per set and the fp32 sum
 * The ReLU of all of them is fmaxf(u, 0.f): a NaN pre-activation (a NaN input, Inf - Inf, 0 * Inf) is stored as +0 behind a ReLU,
 * unlike F.relu, which keeps the NaN; without a ReLU a non-finite input gives non-finite outputs over exactly the outputs whose
 * taps read it (a zero weight does not shield them: 0 * Inf is NaN, as in ATen).
 *
 * Accuracy of the head's kernels — ragmi_conv3d_k3_small_fwd(_ex) on both of its kernels (ragmi_conv3d_k3_small_route),
 * ragmi_upconv3d_c1_fwd, ragmi_trilinear3d_act_k1_fwd / _xblend_fwd, ragmi_uptaps3d_fwd / _xblended_fwd — in the same vocabulary
 * (enforced per element against float64 by tests/test_head_kernel_sweep.py; conv(., |w|) = the 3x3x3 convolution with |w|, U = the x2
 * interpolation with the fp32 index rule):
 *   small 3x3x3 (VALU form and conv3d_c1)   (27 Cin + 1) * 2^-24 * mag                       (one fmaf chain, as the strided 3x3 line)
 *   ragmi_upconv3d_c1_fwd                   conv(3 * 2^-23 * A, |w|) + (27 Cin + 1) * 2^-24 * conv(A, |w|)
 *   ragmi_trilinear3d_act_k1_fwd            the resample + 1x1x1 line: b_P = (3 * 2^-23 + (C + 1) * 2^-24) * sum_c |w| * A_c
 *   ragmi_trilinear3d_act_k1_xblend_fwd     the same + 9 * 2^-24, of sum_dx shift_dx(U_x(sum_c |w| * A_c))    (the 9-term x chain)
 *   ragmi_uptaps3d_fwd                      25 * 2^-24 * M, M = sum_t shift_t(U(|P_t|))      (<= 9 roundings along x, 9 along y, 6 along z)
 *   ragmi_uptaps3d_xblended_fwd             16 * 2^-24 * sum_g shift_g(U_yz(|Q_g|))          (<= 9 along y, 6 along z, the epilogue)
 *   the tap pair from x                     sum_t shift_t(U(b_P)) + 25 * 2^-24 * sum_t shift_t(U(sum_c |w_t| * A_c))
 *   folded BatchNorm, ReLU, bf16 storage    the lines above, unchanged; the residual of the small form adds 2^-23 * (|act(u)| + |res|)
 * ragmi_trilinear3d_act_k1_fwd applies its ReLU before the mix: a NaN sample enters the mix as 0.  Non-finite inputs stay local as
 * described above in all of them: uptaps3d_kernel multiplies a window slot only where it belongs to the source pair (i0, i1) of the
 * row, column or plane, and the convolution's zero padding takes no part.
 */
int ragmi_conv3d_k1_fwd(const void* x, int64_t x_bstride,
                        const void* weight, const void* scale, const void* shift, int relu,
                        void* y, int64_t y_bstride, int y_ch0,
                        int B, int Cin, int Cout, int64_t DHW,
                        int dtype, void* stream);

/* Two 1x1x1 ConvBR_3d in a row as one launch: y = act2(bn2(W2 . act1(bn1(W1 . x)))), the intermediate (Cmid channels) in registers —
 * the head's last_12_3d followed by the channel mix of last_6_3d (rag_model.py:358-365, :270-271).  Results are those of two
 * ragmi_conv3d_k1_fwd calls, bit for bit.  Built for Cin <= 64 -> 24 -> 12 channels (ragmi_conv3d_k1_chain_supported). */
int ragmi_conv3d_k1_chain_supported(int Cin, int Cmid, int Cout);
int ragmi_conv3d_k1_chain_fwd(const void* x, int64_t x_bstride, const void* weight1, const void* scale1, const void* shift1, int relu1,
                              int Cmid, const void* weight2, const void* scale2, const void* shift2, int relu2,
                              void* y, int64_t y_bstride, int y_ch0, int B, int Cin, int Cout, int64_t DHW, int dtype, void* stream);

/* The same with the weight given TRANSPOSED in memory when w_transposed != 0 (weight[ci][co], i.e. [Cin][Cout] row-major): the
 * data gradient of a 1x1x1 conv is this conv with the forward weight read in place — no transposed copy per step. */
int ragmi_conv3d_k1_fwd_ex(const void* x, int64_t x_bstride, const void* weight, int w_transposed, const void* scale,
                           const void* shift, int relu, void* y, int64_t y_bstride, int y_ch0, int B, int Cin,
                           int Cout, int64_t DHW, int dtype, void* stream);

/*
 * Trilinear resample fused into the 1x1x1 ConvBR_3d that consumes it:
 *   y[b, y_ch0 + co] = act(bn(W . interpolate(x, [Do,Ho,Wo], 'trilinear', align_corners)))
 * (Cell_3d down/up-sampling + preprocess, rag_model.py:146-155; head last_6_3d(upsample_12(.)), :358-365).
 * x: [B, Cin, Di, Hi, Wi]; the interpolated tensor is never materialised.
 */
int ragmi_conv3d_k1_resample_fwd(const void* x, int64_t x_bstride, int Di, int Hi, int Wi,
                                 const void* weight, const void* scale, const void* shift, int relu,
                                 void* y, int64_t y_bstride, int y_ch0,
                                 int B, int Cin, int Cout, int Do, int Ho, int Wo, int align_corners,
                                 int dtype, void* stream);

/*
 * Two such resample + 1x1x1 ConvBR_3d calls that write into the same buffer at the same output size (a cell's
 * pre_preprocess and preprocess, each reading its own input at its own size) as ONE launch.
 */
typedef struct {
  const void* x;
  int64_t x_bstride;
  int32_t Di, Hi, Wi;
  const void* weight; /* [Cout][Cin] */
  const void* scale;
  const void* shift;
  int32_t relu;
  int32_t y_ch0;
  int32_t Cin, Cout;
} ragmi_k1r_t;
int ragmi_conv3d_k1_resample_pair_fwd(const ragmi_k1r_t* a, const ragmi_k1r_t* b, void* y, int64_t y_bstride,
                                      int B, int Do, int Ho, int Wo, int align_corners, int dtype, void* stream);
/* the same with up to three descriptors and ONE DESTINATION BUFFER PER DESCRIPTOR (ys[i], y_bstrides[i]; y_ch0 inside it), all at
 * the output size (Do, Ho, Wo): a cell's pre_preprocess + preprocess together with the NEXT cell's pre_preprocess when that one
 * resamples the same tensor to the same size (rag_model.py:146-155 of two consecutive cells: the level-6 tensor both level-12
 * cells 6 and 7 read) — the tensor is gathered by both in one launch instead of once per launch. */
int ragmi_conv3d_k1_resample_multi_fwd(const ragmi_k1r_t* const* specs, void* const* ys, const int64_t* y_bstrides, int n, int B,
                                       int Do, int Ho, int Wo, int align_corners, int dtype, void* stream);

/*
 * One launch per Cell_2d of the Feature Net (src/models/rag_model.py:143-177 with the 2-D operations of
 * src/automl/operations_2d.py; the cells built by rag_model.py:236-247), for cells in which every new state is the sum of one
 * 3x3 ConvBR_2d of s0 and one of s1 (the all-conv genotype):
 *     s0 = pre_preprocess(F.interpolate(prev_prev, (H, W), mode='bilinear', align_corners=True))      (1x1 ConvBR_2d)
 *     s1 = preprocess(F.interpolate(prev, (H, W), ...))                                                (1x1 ConvBR_2d)
 *     y[:, group g] = relu(bnA(convA(s0))) + relu(bnB(convB(s1)))          (the stacked sibling convs, as ragmi_conv3d_k3_dual_fwd)
 * s0 / s1 and the interpolated tensors are never written: the two 1x1 convs (resample first, then an fmaf chain over the input
 * channels in order, folded BatchNorm, ReLU — the arithmetic of ragmi_conv3d_k1_resample_fwd) run in the staging of the 3x3 launch.
 * An input already at (H, W) is read as is.  packedA / packedB: ragmi_conv3d_k3_pack(_ex) of the [Cout, C, 3, 3] weights
 * (planar2d) or of any [Cout, C, 3, 3, 3] weight (depth 1: only the middle slice acts).  dtype: RAGMI_F32X3 only (fp32 storage,
 * split products — the contract of ragmi_conv3d_k3_fwd on depth-1 volumes); C = 4 or 8 channels per set, Cin <= 48 per input,
 * W >= 16: ragmi_cell2d_supported answers 1 for what is built, and the host runs the separate launches otherwise.
 */
typedef struct {
  const void* x; /* [B, Cin, Hi, Wi] */
  int64_t x_bstride;
  int32_t Cin, Hi, Wi;
  const void* weight; /* [C][Cin] */
  const void* scale;  /* folded BatchNorm [C], or NULL */
  const void* shift;
  int32_t relu;
} ragmi_cell2d_in_t;
int ragmi_cell2d_supported(int C, int Cin0, int Cin1, int Cout, int H, int W, int dtype);
int ragmi_cell2d_fwd(const ragmi_cell2d_in_t* s0, const ragmi_cell2d_in_t* s1, int C, const void* packedA, const void* scaleA,
                     const void* shiftA, const void* packedB, const void* scaleB, const void* shiftB, int relu, void* y,
                     int64_t y_bstride, const int32_t* y_group_ch, int B, int Cout, int H, int W, int dtype, void* stream);

/*
 * Trilinear resample, F.interpolate(mode='trilinear') with ATen's source-index
 * rule for align_corners = 1 (rag_model.py:150-153, 357-358) or 0.
 * x: [B, C, Di, Hi, Wi] -> y: [B, C, Do, Ho, Wo] (contiguous).
 */
int ragmi_trilinear3d_fwd(const void* x, void* y, int B, int C,
                          int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                          int align_corners, int dtype, void* stream);

/* The same resample reading a channel slice (x_bstride elements between batch items) and writing y[b, y_ch0 + c] of a wider
 * buffer (y_bstride), with an optional ReLU after the interpolation.  It is the second half of an UPSAMPLING
 * `ConvBR_3d(1x1x1)(F.interpolate(x))` (rag_model.py:150-155, 358-365) run conv-first: the channel mix and the folded BatchNorm
 * are affine and the taps sum to one, so act(bn(conv(interp(x)))) == act(interp(bn(conv(x)))) and the mix runs on 1/8 of
 * the voxels. */
/* The Matching-Net head's last two steps in one kernel (rag_model.py:357-365: `upsample_6` = nn.Upsample(scale_factor=2,
 * mode='trilinear', align_corners=True), then last_3_3d = ConvBR_3d(C, 1, 3, 1, 1, bn=False, relu=False)):
 *   y[:, y_ch0] = act(scale * conv3x3x3_pad1(upsample2(x))[:, 0] + shift)   (scale/shift optional, one output channel)
 * x: [B, Cin, Di, Hi, Wi] (dtype, batch stride x_bstride), weight: the raw [1, Cin, 3, 3, 3] fp32 tensor, y: [B, *, 2Di, 2Hi, 2Wi]
 * (y_dtype: the input's, or RAGMI_F32 for a RAGMI_BF16 input).  The upsampled tensor is never materialised: every operand of the
 * convolution is interpolated in registers with the same fp32 source-index rule as ragmi_trilinear3d_fwd (nesting z, y, x instead
 * of ATen's x, y, z: reassociation only).  ragmi_upconv3d_c1_supported: Cin <= 64, every input axis >= 2; otherwise run
 * ragmi_trilinear3d_fwd + ragmi_conv3d_k3_small_fwd_ex. */
int ragmi_upconv3d_c1_supported(int Cin, int Di, int Hi, int Wi);
int ragmi_upconv3d_c1_fwd(const void* x, int64_t x_bstride, const void* weight, const void* scale, const void* shift, int relu, void* y,
                          int64_t y_bstride, int y_ch0, int B, int Cin, int Di, int Hi, int Wi, int dtype, int y_dtype, void* stream);

int ragmi_trilinear3d_act_fwd(const void* x, int64_t x_bstride, void* y, int64_t y_bstride, int y_ch0, int relu, int B, int C,
                              int Di, int Hi, int Wi, int Do, int Ho, int Wo, int align_corners, int dtype, void* stream);

/* The same head with the channel sum taken BEFORE the x2 upsample (rag_model.py:269, 357-365).  `upsample_6` is linear and acts per
 * channel and last_3_3d has one output channel, so
 *   last_3_3d(upsample2(y6))(v) = sum_t upsample2(P_t)(v + tap_t - 1),   P_t = sum_c w[c, t] * y6_c,   t = dz*9 + dy*3 + dx,
 * with the convolution's zero padding unchanged (positions outside the upsampled volume contribute zero).  Two launches:
 *
 * ragmi_trilinear3d_act_k1_fwd = ragmi_trilinear3d_act_fwd followed, in registers, by a bias-free 1x1x1 channel mix:
 *   y[b, y_ch0 + co] = sum_c weight[co, c] * act(interp(x)[b, c])     (c ascending, fp32 FMAs; the resampled channels are not stored)
 * weight: fp32 [Cout][C], or [C][Cout] with w_transposed != 0 — the head passes last_3_3d's raw [1, C, 3, 3, 3] weight as
 * [C][27].  The values entering the mix are bit-identical to what ragmi_trilinear3d_act_fwd stores.  fp32 only; supported: C <= 64,
 * Cout <= 32 and an up-sampling by two or more on every axis (scale <= 0.5).
 *
 * ragmi_uptaps3d_fwd: p = P [B, 27, Di, Hi, Wi] fp32 (batch stride p_bstride) ->
 *   y[:, y_ch0] = act(scale * sum_t upsample2(P_t)(v + tap_t - 1) + shift)   of [B, *, 2Di, 2Hi, 2Wi] fp32 (scale/shift optional),
 * upsample2 = trilinear, align_corners=True, with the fp32 source-index rule of ragmi_trilinear3d_fwd (nesting x, y, z).
 * supported: every input axis >= 2, even Wi, 27*Di*Hi*Wi < 2^31. */
int ragmi_trilinear3d_act_k1_supported(int C, int Cout, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int align_corners);
int ragmi_trilinear3d_act_k1_fwd(const void* x, int64_t x_bstride, const void* weight, int w_transposed, void* y, int64_t y_bstride,
                                 int y_ch0, int relu, int B, int C, int Cout, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                 int align_corners, int dtype, void* stream);
int ragmi_uptaps3d_supported(int Di, int Hi, int Wi);
int ragmi_uptaps3d_fwd(const void* p, int64_t p_bstride, const void* scale, const void* shift, int relu, void* y, int64_t y_bstride,
                       int y_ch0, int B, int Di, int Hi, int Wi, int dtype, void* stream);

/* The same two launches with the x blend of upsample_6 (rag_model.py:269, 357-365) moved into the first one.  The x-blended row of
 * a (dz, dy) tap pair depends on global coordinates only,
 *   Q[dz*3 + dy](z6, y6, gx) = sum over dx of upsample2_x(P[dz*9 + dy*3 + dx](z6, y6, .))(gx + dx - 1),   gx in [0, 2 Wo),
 * (zero where gx + dx - 1 leaves the row), so it is formed once per level-6 voxel instead of once per output tile and segment.
 *
 * ragmi_trilinear3d_act_k1_xblend_fwd: ragmi_trilinear3d_act_k1_fwd with weight = last_3_3d's raw [1, C, 3, 3, 3] tensor read as
 * [C][27]; the 27 P values of a voxel (the bits that launch stores) stay in registers and
 *   q[b, q_ch0 + g] = Q[g]   of [B, *, Do, Ho, 2 Wo] fp32 (batch stride q_bstride, 8-byte aligned rows)
 * leaves, two columns per level-6 voxel.  supported: ragmi_trilinear3d_act_k1_supported, Cout == 27 and Wo == 2 Wi.
 *
 * ragmi_uptaps3d_xblended_fwd: ragmi_uptaps3d_fwd from q = Q [B, 9, Di, Hi, 2 Wi] (16-byte aligned, q_bstride % 4 == 0) — the y and z
 * blends, the scale / shift / ReLU epilogue.  Same fmaf chains in the same order as ragmi_uptaps3d_fwd: the pair's output has the
 * bits of ragmi_trilinear3d_act_k1_fwd -> ragmi_uptaps3d_fwd.  supported: as ragmi_uptaps3d_supported. */
int ragmi_trilinear3d_act_k1_xblend_supported(int C, int Cout, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int align_corners);
int ragmi_trilinear3d_act_k1_xblend_fwd(const void* x, int64_t x_bstride, const void* weight, void* q, int64_t q_bstride, int q_ch0,
                                        int relu, int B, int C, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int align_corners,
                                        int dtype, void* stream);
int ragmi_uptaps3d_xblended_supported(int Di, int Hi, int Wi);
int ragmi_uptaps3d_xblended_fwd(const void* q, int64_t q_bstride, const void* scale, const void* shift, int relu, void* y,
                                int64_t y_bstride, int y_ch0, int B, int Di, int Hi, int Wi, int dtype, void* stream);

/*
 * Feature-Net stem: 2-D 3x3 / pad 1 / stride `stride` ConvBR (stem2d1 = ConvBR_2d(6, 12, 3,
 * stride=3, padding=1), rag_model.py:201).  x: [B, Cin, H, W] -> y: [B, Cout, (H-1)/stride+1, (W-1)/stride+1].
 * weight: raw nn.Conv2d weight [Cout, Cin, 3, 3].  The stride-1 2-D convs of the Feature Net run on the 3-D
 * kernels over a depth-1 volume (weights embedded in the middle z-slice).
 */
int ragmi_conv2d_k3_strided_fwd(const void* x, const void* weight, const void* scale, const void* shift, int relu,
                                void* y, int B, int Cin, int Cout, int H, int W, int stride, int dtype, void* stream);

/*
 * y[b, y_ch0 + c] = a[b, a_ch0 + c] + b[b, b_ch0 + c]   (sum of two Identity_3d branches,
 * rag_model.py:172 with operations_3d.py:84-90).
 */
int ragmi_add_fwd(const void* a, int64_t a_bstride, int a_ch0,
                  const void* b, int64_t b_bstride, int b_ch0,
                  void* y, int64_t y_bstride, int y_ch0,
                  int B, int C, int64_t DHW, int dtype, void* stream);

/*
 * Fused Disp.forward (rag_model.py:39-44): trilinear upsample of cost[B,1,d,h,w] to
 * [maxdisp, Ho, Wo] (align_corners=False) -> Softmin over the disparity axis ->
 * DisparityRegression (sum_d p_d * d).  The reference always uses Ho=3h, Wo=3w.
 * out: [B, Ho, Wo] fp32.  Nothing of size maxdisp*Ho*Wo is materialised.
 */
int ragmi_disp_softargmin_fwd(const void* cost, void* out, int B, int d, int h, int w,
                              int maxdisp, int Ho, int Wo, int dtype, void* stream);

/*
 * DisparityRegression.forward (rag_model.py:23-29): out[b,y,x] = sum_d prob[b,d,y,x] * d.
 * prob: [B, D, H, W] contiguous -> out [B, H, W] fp32.
 */
int ragmi_disparity_regression_fwd(const void* prob, void* out, int B, int D, int H, int W,
                                   int dtype, void* stream);

/*
 * The head with per-pixel statistics of its distribution, in the same pass (rag_model.py:18-44 computes the
 * distribution and keeps only its mean).  p_k, k = 0 .. maxdisp-1, is the Softmin over the trilinearly upsampled
 * cost (align_corners=False, to [maxdisp, Ho, Wo]) exactly as in ragmi_disp_softargmin_fwd.  Per output pixel:
 *   out      = sum_k p_k k                     the SAME BITS as ragmi_disp_softargmin_fwd on the same input
 *   variance = sum_k p_k (k - out)^2           px^2, accumulated about a pivot near the mode (not sum p k^2 - out^2)
 *   peak     = max_k p_k
 *   entropy  = -sum_k p_k ln p_k               nats; a term with p_k = 0 contributes 0
 * out: [B, Ho, Wo] fp32.  stats: [B, 3, Ho, Wo] fp32, planes (variance, peak, entropy).  cost: fp32 or bf16 storage.
 * One launch; arguments, refusals, status codes and the choice between the tiled and the generic kernel are those of
 * ragmi_disp_softargmin_fwd.  No allocation, synchronisation, memset, memcpy or atomics; bitwise reproducible.
 * Non-finite costs give unspecified statistics, never an access out of bounds.
 */
int ragmi_disp_softargmin_stats_fwd(const void* cost, void* out, void* stats, int B, int d, int h, int w,
                                    int maxdisp, int Ho, int Wo, int dtype, void* stream);

/*
 * DisparityRegression.forward (rag_model.py:18-29) with the same statistics of prob[B, D, H, W], taken as given (not
 * renormalised): out = the bits of ragmi_disparity_regression_fwd; stats [B, 3, H, W] by the definitions above with
 * p = prob, terms of p <= 0 contributing 0 to the entropy.  A one-hot prob has variance 0, peak 1, entropy 0 exactly.
 */
int ragmi_disparity_regression_stats_fwd(const void* prob, void* out, void* stats, int B, int D, int H, int W,
                                         int dtype, void* stream);

/*
 * The head with a mode-local disparity, in the same pass (rag_model.py:18-44 keeps only the mean; at a depth edge the
 * distribution has two wells and the mean lies on neither surface).  With p_k as above and an integer radius,
 * 0 <= radius <= maxdisp, in fine-disparity pixels, per output pixel:
 *   index = k*, the fine index of the smallest upsampled cost as the kernel's fp32 arithmetic produces it; the lowest
 *           index on exactly equal values.  In the tiled kernels k* = 3 am + 1 with am the first minimum over the coarse
 *           plane samples (fine sample 3 am + 1 sits on that plane), and k* = 0 when am = 0 (fine samples 0 and 1 are
 *           both plane 0: the source index is clamped).  Stored as an integer-valued fp32.
 *   W     = {k : |k - k*| <= radius, 0 <= k < maxdisp}          clipped at both ends, not renormalised to a full width
 *   mass  = sum_W p_k
 *   disp  = k* + sum_W p_k (k - k*) / mass                      the sum about k*, as the variance runs about its pivot
 * radius = 0 gives disp = k* exactly; radius = maxdisp gives disp = out and mass = 1 up to rounding.
 * out: [B, Ho, Wo] and stats: [B, 3, Ho, Wo] are the SAME BITS as ragmi_disp_softargmin_stats_fwd on the same input.
 * mode: [B, 3, Ho, Wo] fp32, planes (index, disp, mass).  One launch; arguments, refusals, status codes and the choice
 * between the tiled and the generic kernel are those of ragmi_disp_softargmin_stats_fwd; a null mode, radius < 0 and
 * radius > maxdisp are RAGMI_EINVAL before any launch.  radius is a kernel argument: no rebuild, no second code path.
 */
int ragmi_disp_softargmin_mode_fwd(const void* cost, void* out, void* stats, void* mode, int B, int d, int h, int w,
                                   int maxdisp, int Ho, int Wo, int radius, int dtype, void* stream);

/*
 * DisparityRegression.forward (rag_model.py:18-29) with the statistics and the mode-local disparity of prob[B, D, H, W],
 * taken as given: k* is the FIRST arg-max of prob, the sums run over prob itself, and a window without mass gives
 * disp = k*.  out and stats are the bits of ragmi_disparity_regression_stats_fwd; mode [B, 3, H, W] = (index, disp,
 * mass).  A one-hot prob gives (its index, its index, 1) exactly.  0 <= radius <= D, else RAGMI_EINVAL.
 */
int ragmi_disparity_regression_mode_fwd(const void* prob, void* out, void* stats, void* mode, int B, int D, int H, int W,
                                        int radius, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Cost volume + stem3d0 in one step, without materialising the cost volume (rag_model.py:375-383 followed by
 * ConvBR_3d(2C, Cout, 3, 1, 1), rag_model.py:234/341).  The left half of the cost volume does not depend on the disparity
 * plane and the right half depends on x - i only, so the 3-D convolution equals A[cls,tc][co,y,x] + B[cls,xr][co,y,x-i] with
 * A / B two-dimensional convolutions of the feature maps with pre-summed weights (classes: z border, distance to the x = i
 * diagonal, right border) — the same products, summed in another order.
 *   ragmi_costvol_stem_prepare: weight [Cout, 2C, 3,3,3] fp32 -> `variants` (ragmi_costvol_stem_weights_elems floats)
 *   ragmi_costvol_stem_fwd:     left/right [B,C,H,W] (dtype) -> y[B, Cout(+), D, H, W] = act(scale*(conv)+shift) (channels 0..Cout-1,
 *                               batch stride y_bstride), optional fused consumer 1x1x1 tails as in ragmi_conv3d_k3_fwd_ex;
 *                               `workspace`: ragmi_costvol_stem_workspace_elems floats.  C, Cout <= 16.
 *                               dtype RAGMI_F32: the A / B planes by fp32 FMAs (exact products).  RAGMI_F32X3 (fp32 storage) and
 *                               RAGMI_BF16 (bf16 features and outputs, fp32 planes): the planes as split-operand products on the
 *                               16-bit matrix cores under the bound documented for the 3x3x3 convolutions above, when C % 4 == 0,
 *                               C <= 12 and Cout % 4 == 0 (Cout in {4, 8, 12, 16}); any other C or Cout as RAGMI_F32's FMAs.
 *                               A non-finite feature makes non-finite exactly the outputs whose 3x3x3 window holds it in the
 *                               reference's cost volume (taps on the zero side of the x = i diagonal, or outside the volume, do
 *                               not carry it); every other output keeps the bound. */
int64_t ragmi_costvol_stem_weights_elems(int C, int Cout);
int ragmi_costvol_stem_prepare(const void* weight, void* variants, int C, int Cout, void* stream);
int64_t ragmi_costvol_stem_workspace_elems(int B, int C, int Cout, int D, int H, int W);
int ragmi_costvol_stem_fwd(const void* left, const void* right, const void* variants, const void* scale, const void* shift, int relu,
                           void* y, int64_t y_bstride, void* workspace, int B, int C, int Cout, int D, int H, int W,
                           int ntail, const ragmi_tail_t* tails, int dtype, void* stream);

/* stem3d0 AND stem3d1 (rag_model.py:234-235, 341-343: ConvBR_3d(2C, 12, 3, 1, 1) on the cost volume of rag_model.py:375-383, then
 * ConvBR_3d(12, Cout, 3, 1, 1)) with stem3d0's OUTPUT never written either: ragmi_costvol_stem_fwd's variant planes; its fused tails
 * (ntail0 consumer 1x1x1 convs of stem3d0's output — cell 0's pre_preprocess, rag_model.py:125,154 — by the combine kernel without its
 * main store; ragmi_costvol_stem_fwd itself takes y = NULL for that); then stem3d1's 3x3x3 convolution on the z-marching
 * split-operand kernel, whose halo staging evaluates act(scale0 * (A + B) + shift0) from the planes — the combine kernel's
 * arithmetic, bit for bit — instead of loading a tensor.  What it saves at the headline shape: a 164 MB write and its read-back
 * (stem3d0's combine kernel was bound by exactly that write).  RAGMI_F32X3 only, Cmid = 12 (stem3d0's output channels), C <= 12 a
 * multiple of 4; y / store_main / tails / y_group_ch as ragmi_conv3d_k3_fwd_ex (tails may be RAGMI_TAIL_G4); workspace as
 * ragmi_costvol_stem_workspace_elems(B, C, Cmid, D, H, W).  ragmi_costvol_stem_conv3d_supported: 1 when the stem3d1 launch of this shape
 * runs on that kernel. */
int ragmi_costvol_stem_conv3d_supported(int C, int Cmid, int Cout, int B, int D, int H, int W, int ntail, int dtype);
int ragmi_costvol_stem_conv3d_fwd(const void* left, const void* right, const void* variants, const void* scale0, const void* shift0, int relu0,
                                  void* workspace, int ntail0, const ragmi_tail_t* tails0,
                                  const void* packed_weight, const void* scale, const void* shift, int relu,
                                  void* y, int64_t y_bstride, const int32_t* y_group_ch, int store_main, int ntail, const ragmi_tail_t* tails,
                                  int B, int C, int Cmid, int Cout, int D, int H, int W, int dtype, void* stream);

/* 1 when ragmi_conv3d_k3_fwd(_ex) (nset = 1) / ragmi_conv3d_k3_dual_fwd(_ex) (nset = 2, Cin = both inputs) called with this
 * dtype (RAGMI_F32X3 or RAGMI_BF16) runs this shape on the 16-bit matrix cores (fp16 / bf16 operands), 0 when it runs on the fp32-MFMA kernel.  Three forms
 * (conv3d_x3.hip, conv2d_x3.hip), all without a residual input and with whole 4-channel groups in and out (Cin % 4 == 0, Cout % 4 == 0): the z-marching form for
 * D*H*W >= 2^18 voxels PER SAMPLE, W >= 32, D >= 8, <= 24 input channels; the deep-level form for 8 or 16 input channels per
 * set, no fused tails, D >= 2 and D*H*W >= 2^14 voxels per sample; the depth-1 form (RAGMI_F32X3 only: the Feature Net's 2-D
 * convolutions, rag_model.py:285-323) for D == 1, W >= 16, H >= 2, no fused tails and 4..16 input channels (4 or 8 per set of a
 * dual launch) — there the taps dz != 1 meet only zero padding and only the middle slice of the packed fragments is issued.
 * B never enters: the kernel (hence the rounding) a sample gets does not depend on how a batch is split over ranks.  Always 0 for RAGMI_F32. */
int ragmi_conv3d_k3_uses_x3(int Cin, int Cout, int B, int D, int H, int W, int nset, int has_res, int ntail, int dtype);
/* Which kernel the same call (with `ntail` full-resolution and `ndown` down-sampling tails of 4 channels) lands on: 0 the depth-1 form
 * (conv2d_x3_kernel), 1 the deep-level box form (conv3d_x3d_kernel), 2 the z-marching quad-ring form (conv3d_x3q_kernel), 3 the z-marching
 * form (conv3d_x3_kernel), 4 the fp32-MFMA kernel (conv3d_k3_kernel); RAGMI_EINVAL for arguments no entry point takes.  sched (4 ints, may
 * be NULL) receives the z-marching work list of routes 2 and 3 — planes per depth segment, segments per column, pairs per group cut into
 * half items, groups the list is dealt in — and zeros otherwise.  Host code only: no device is touched. */
int ragmi_conv3d_k3_route(int Cin, int Cout, int B, int D, int H, int W, int nset, int has_res, int ntail, int ndown, int dtype,
                          int32_t* sched);
/* The same for the 1x1x1 and resample launches (host code only, no device is touched; RAGMI_EINVAL / RAGMI_EUNSUPPORTED as the entry
 * points themselves).  ragmi_conv3d_k1_plan: the output-channel slab width *nco (24, 16, 12, 8 or 4; Cout runs in ceil(Cout / nco)
 * slabs) and whether a thread takes four voxels (*vec) in ragmi_conv3d_k1_fwd(_ex); x_align_ok / y_align_ok: the x and y pointers
 * are aligned to four elements.  ragmi_conv3d_k1_resample_plan: the slab width shared by the n = 1..3 descriptors of
 * ragmi_conv3d_k1_resample_fwd / _pair_fwd / _multi_fwd; in_sizes holds (Di, Hi, Wi) per descriptor.  ragmi_trilinear3d_route: 1 when
 * ragmi_trilinear3d_fwd / ragmi_trilinear3d_act_fwd stage their input through LDS (an up-sampling by two or more on every axis),
 * 0 for the generic gather; the two give the same bits. */
int ragmi_conv3d_k1_plan(int B, int Cin, int Cout, int64_t DHW, int64_t x_bstride, int64_t y_bstride, int x_align_ok, int y_align_ok,
                         int dtype, int32_t* nco, int32_t* vec);
int ragmi_conv3d_k1_resample_plan(int n, const int32_t* Cin, const int32_t* Cout, const int32_t* in_sizes, int B, int Do, int Ho, int Wo,
                                  int dtype, int32_t* nco);
int ragmi_trilinear3d_route(int Di, int Hi, int Wi, int Do, int Ho, int Wo, int C, int align_corners);
/* Which kernel ragmi_conv3d_k3_small_fwd_ex runs this call on, decided by the code the launch itself calls (host code only, no device
 * is touched; RAGMI_EINVAL / RAGMI_EUNSUPPORTED as the entry point itself): 0 the single-output-channel z-marching kernel
 * conv3d_c1_kernel (Cout == 1, no residual, Cin <= 64, W % 4 == 0, >= 2^18 voxels PER SAMPLE, batch strides that are multiples of
 * four elements and x / y pointers aligned to four elements: x_align_ok / y_align_ok), else 1 + cfg: conv3d_k3_kernel<.., VALU> on
 * tile configuration cfg of ragmi_conv3d_k3_plan's table (0: 32 x 8 x 4 voxels, 1: 16 x 8 x 4, 2: 8 x 8 x 4). */
int ragmi_conv3d_k3_small_route(int Cin, int Cout, int B, int D, int H, int W, int dtype, int y_dtype, int has_res, int64_t x_bstride,
                                int64_t y_bstride, int x_align_ok, int y_align_ok);

/* ragmi_conv3d_k3_pack with two options used by the training step: transpose != 0 packs the DATA-GRADIENT conv of a forward
 * weight (source [Cin][Cout][taps], taps flipped), Cout/Cin being those of the packed conv; planar2d != 0: the source is a 2-D
 * [.,.,3,3] weight living in the dz = 1 plane (Feature Net on depth-1 volumes). */
int ragmi_conv3d_k3_pack_ex(const void* weight, void* packed, int Cout, int Cin, int transpose, int planar2d, int dtype, void* stream);

/* ragmi_conv3d_k3_pack_ex for a weight that will be used under ONE known arithmetic contract (the training step packs ~150 weights
 * per step, each for the call that follows): for_dtype == RAGMI_F32 fills only the fp32-MFMA section of `packed` (same buffer size);
 * such a buffer must be passed to the convolution entry points with dtype RAGMI_F32 only — the sections it skips are POISONED (NaN
 * fragments and multipliers), so a call under another dtype returns NaN everywhere instead of reading uninitialised memory.  Any
 * other for_dtype fills every section, like ragmi_conv3d_k3_pack_ex. */
int ragmi_conv3d_k3_pack_for(const void* weight, void* packed, int Cout, int Cin, int transpose, int planar2d, int for_dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training step (BASELINE config 5; the reference runs autograd through the same modules, approaches/rag.py:155-219).
 * fp32 only.  Data-gradients of the convolutions are the forward kernels applied to the output gradient with the
 * weight transposed (and its taps flipped); the functions below are the pieces with no forward twin.
 * Buffers marked (+=) are accumulated into with atomics and must be zeroed by the caller.
 */

/* Train-mode BatchNorm3d statistics (operations_3d.py:44) of the raw conv output x[B,C,DHW]: batch mean / biased variance ->
 * mean[c], invstd[c], scale[c] = gamma*invstd, shift[c] = beta - mean*scale, and (running_mean != NULL) the momentum update of
 * running_mean / running_var (unbiased) / num_batches_tracked (int64, may be NULL) with nn.BatchNorm semantics.  Two-level
 * deterministic reduction of x - K and (x - K)^2 about the channel's pivot K = x[0,c,0] (mean = K + s/n, var = q/n - (s/n)^2: no
 * (mean/std)^2 cancellation); `workspace` holds ragmi_bn_workspace_elems(B, C, DHW) floats (no initialisation needed). */
int64_t ragmi_bn_workspace_elems(int B, int C, int64_t DHW);
int ragmi_bn_train_stats_fwd(const void* x, int64_t x_bstride, int B, int C, int64_t DHW, const void* gamma, const void* beta,
                             void* running_mean, void* running_var, void* num_batches_tracked, float momentum, float eps,
                             void* workspace, void* mean, void* invstd, void* scale, void* shift, void* stream);

/* the two launches of a train-mode BatchNorm + ReLU forward: statistics, then finalize (as ragmi_bn_train_stats_fwd) fused with the
 * affine + ReLU pass y[b, y_ch0+c] = act(x[b,c]*scale[c] + shift[c]) (+ res[b, res_ch0+c] when res != NULL: a cell's running sum of
 * branches, rag_model.py:163-172, without a separate add launch).  y must not overlap x: every workgroup of the second launch
 * reads the channel's pivot x[0,c,0] while others store y (res may be y's buffer only where the same element is read and written) */
int ragmi_bn_train_act_fwd(const void* x, int64_t x_bstride, int B, int C, int64_t DHW, const void* gamma, const void* beta,
                           void* running_mean, void* running_var, void* num_batches_tracked, float momentum, float eps, int relu,
                           void* workspace, void* mean, void* invstd, void* scale, void* shift, void* y, int64_t y_bstride, int y_ch0,
                           const void* res, int64_t res_bstride, int res_ch0, void* stream);

/* the two launches of its adjoint: the reduction of ragmi_bn_act_bwd_coeffs, then coefficients + dx = g*c1 + (x - mean)*c2 + c3 in
 * one pass (dgamma / dbeta may be NULL; accumulate != 0: +=) */
int ragmi_bn_act_bwd(const void* dy, int64_t dy_bstride, int dy_ch0, const void* x, int64_t x_bstride, const void* scale,
                     const void* shift, int relu, const void* mean, const void* invstd, int training, int B, int C, int64_t DHW,
                     void* workspace, void* dx, int64_t dx_bstride, void* dgamma, void* dbeta, int accumulate, void* stream);

/* y[b, y_ch0+c] = act(x[b,c] * scale[c] + shift[c]) (+ res[b, res_ch0+c]) — BN affine + ReLU (+ running sum) as one pass */
int ragmi_bn_act_fwd(const void* x, int64_t x_bstride, const void* scale, const void* shift, int relu,
                     const void* res, int64_t res_bstride, int res_ch0,
                     void* y, int64_t y_bstride, int y_ch0, int B, int C, int64_t DHW, void* stream);

/* ReLU + BatchNorm adjoint, reduction half: with g = dy * [x*scale+shift > 0] (x = the raw conv output) it reduces sum g and
 * sum g*(x - mean) per channel and writes dgamma[c], dbeta[c] and the coefficients of dx = g*c1 + (x - c0)*c2 + c3 with c0 = mean
 * (training != 0: batch statistics were used; 0: running statistics, c2 = c3 = 0).  The form is centred on the mean so that nothing
 * of the size of mean*c2 has to cancel in fp32.  Same workspace as ragmi_bn_train_stats_fwd. */
int ragmi_bn_act_bwd_coeffs(const void* dy, int64_t dy_bstride, int dy_ch0, const void* x, int64_t x_bstride,
                            const void* scale, const void* shift, int relu, const void* mean, const void* invstd, int training,
                            int B, int C, int64_t DHW, void* workspace, void* c0, void* c1, void* c2, void* c3, void* dgamma,
                            void* dbeta, int accumulate, void* stream);   /* dgamma / dbeta may be NULL; accumulate != 0: += */

/* dx[b,c] = g * c1[c] + (x - c0[c]) * c2[c] + c3[c]   (train-mode BN backward is linear in g and x per channel; eval BN: c2 = c3 = 0) */
int ragmi_bn_act_bwd_apply(const void* dy, int64_t dy_bstride, int dy_ch0, const void* x, int64_t x_bstride,
                           const void* scale, const void* shift, int relu, const void* c0, const void* c1, const void* c2,
                           const void* c3, void* dx, int64_t dx_bstride, int B, int C, int64_t DHW, void* stream);

/* dw[co][ci][tap] = sum_{b,v} g[b, g_ch0+co, v] * x[b, ci, v + tap]   — weight gradient of the 3x3x3 conv (MFMA; persistent
 * workgroups write partial sums to `workspace`, ragmi_conv3d_k3_wgrad_workspace_elems(...) floats, and a second kernel adds them:
 * deterministic, dw needs no initialisation) */
int64_t ragmi_conv3d_k3_wgrad_workspace_elems(int B, int Cin, int Cout, int D, int H, int W);
int ragmi_conv3d_k3_wgrad(const void* x, int64_t x_bstride, const void* g, int64_t g_bstride, int g_ch0, void* const* dw_list, int n_dw,
                          int accumulate, int planar2d, void* workspace, int B, int Cin, int Cout, int D, int H, int W, void* stream);
/* dw_list: n_dw (1..8) destination tensors, each [Cout/n_dw, Cin, 3,3,3] (planar2d: [.., 3,3], the dz = 1 plane) — stacked
 * sibling convolutions write every unit's gradient in place; accumulate != 0: dw += (gradient accumulation into .grad) */

/* dw[co][ci] (+=) sum_{b,v} g[b, g_ch0+co, v] * x[b, ci, v]   — weight gradient of the 1x1x1 conv */
int ragmi_conv3d_k1_wgrad(const void* x, int64_t x_bstride, const void* g, int64_t g_bstride, int g_ch0, void* dw,
                          int B, int Cin, int Cout, int64_t DHW, void* stream);

/* adjoint of ragmi_trilinear3d_fwd: dx[B,C,Di,Hi,Wi] gathers dy[B,C,Do,Ho,Wo] through the forward's taps (no atomics) */
int ragmi_trilinear3d_bwd(const void* dy, void* dx, int B, int C, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                          int align_corners, void* stream);

/* adjoint of ragmi_costvol_fwd: dleft/dright [B,C,h,w] from dcost [B,2C,d,h,w] */
int ragmi_costvol_bwd(const void* dcost, void* dleft, void* dright, int B, int C, int d, int h, int w, void* stream);

/* adjoint of ragmi_disp_softargmin_fwd: dcost[B,d,h,w] (+=) from dout[B,Ho,Wo] (recomputes the softmin statistics) */
int ragmi_disp_softargmin_bwd(const void* cost, const void* dout, void* dcost, int B, int d, int h, int w,
                              int maxdisp, int Ho, int Wo, void* stream);

/*
 * Adjoint of ragmi_disp_softargmin_stats_fwd (rag_model.py:18-44 under autograd, with the statistics as further outputs).
 * With v_k the fine cost of a pixel, p = softmin(v), mu = sum p_k k, var = sum p_k (k - mu)^2, H = -sum p_k ln p_k,
 * k* = argmax p (the first sample that holds the maximum), peak = p_k*, and the cotangents gmu = dout, (gV, gP, gH) = dstats:
 *   dL/dv_k = -p_k [ gmu (k - mu) + gV ((k - mu)^2 - var) - gH (ln p_k + H) - gP peak ] - [k = k*] gP peak
 * scattered through the trilinear taps into dcost.  The clamps of variance and entropy at 0 are treated as the identity.
 * cost, dcost: [B,d,h,w] fp32; dout: [B,Ho,Wo] fp32 or NULL; dstats: [B,3,Ho,Wo] fp32 (variance, peak, entropy) or NULL.  A NULL
 * cotangent is a zero one (the same bits); both NULL is RAGMI_EINVAL.  Same contract as ragmi_disp_softargmin_bwd: dcost is
 * pre-zeroed by the caller and added to with float atomics (one add per 16 x 16 fine tile, coarse cell and plane), Ho = 3h, Wo = 3w
 * and maxdisp <= 3072, else RAGMI_EUNSUPPORTED; sizes <= 0 or B > 65535 are RAGMI_EINVAL.  Every argument is checked before the
 * launch.  One launch; no allocation, synchronisation, memset or memcpy.  The softmin statistics are recomputed from cost.
 */
int ragmi_disp_softargmin_stats_bwd(const void* cost, const void* dout, const void* dstats, void* dcost, int B, int d, int h, int w,
                                    int maxdisp, int Ho, int Wo, void* stream);

/*
 * Uncertainty-aware regression loss over the head's own variance (Kendall & Gal's form; the reference trains the mean only,
 * approaches/rag.py:210-211).  mask = 0 < gt < maxdisp, s = stats[:,0] + var_floor, per masked pixel
 *   l = smooth_l1(est - gt) * rsqrt(s) + 0.5 ln s                      (smooth-L1 with beta = 1)
 * out[0] = sum l / N, out[1] = the masked smooth-L1 mean (out[0] of ragmi_stereo_metrics_fwd, for logging), out[2] = the mean of
 * sqrt(s) over the mask, out[3] = N.  An empty mask gives 0 / 0 (NaN) in out[0..2], as ragmi_stereo_metrics_fwd's out[0].
 * disp_est, disp_gt: [B,H,W] fp32; stats: [B,3,H,W] fp32 (plane 0 is read); acc: ragmi_uncertainty_loss_workspace_elems(B,H,W)
 * floats of scratch (nothing to zero); out: 4 floats.  var_floor > 0 (RAGMI_EINVAL otherwise).  Two launches; no atomics, no
 * memset, no synchronisation; bitwise reproducible (fixed-order two-level sum, the second level in double).
 */
int64_t ragmi_uncertainty_loss_workspace_elems(int B, int H, int W);
int ragmi_uncertainty_loss_fwd(const void* disp_est, const void* stats, const void* disp_gt, int B, int H, int W, float maxdisp,
                               float var_floor, void* acc, void* out, void* stream);

/* gradient of out[0], one launch: ddisp[B,H,W] = gout[0] [mask] clamp(est - gt, -1, 1) rsqrt(s) / out[3] and ALL THREE planes of
 * dstats[B,3,H,W]: plane 0 = gout[0] [mask] (0.5 / s - 0.5 smooth_l1 s^(-3/2)) / out[3], planes 1 and 2 = 0 (written here so that
 * no memset enters a captured step).  out: the forward's 4 floats; gout: 1 float on the device. */
int ragmi_uncertainty_loss_bwd(const void* disp_est, const void* stats, const void* disp_gt, const void* out, const void* gout,
                               void* ddisp, void* dstats, int B, int H, int W, float maxdisp, float var_floor, void* stream);

/* backward of ragmi_conv2d_k3_strided_fwd's convolution (Feature-Net stem, operations_2d.py ConvBR_2d stride 3):
 * dx[B,Cin,H,W] from g[B,Cout,Ho,Wo];  dw[Cout,Cin,3,3] (+=) */
int ragmi_conv2d_k3_strided_dgrad(const void* g, const void* weight, void* dx, int B, int Cin, int Cout, int H, int W, int stride,
                                  void* stream);
int ragmi_conv2d_k3_strided_wgrad(const void* x, const void* g, void* dw, int B, int Cin, int Cout, int H, int W, int stride,
                                  void* stream);

/* adjoint of ragmi_disparity_regression_fwd: dprob[B,D,H,W] = dout[B,H,W] * d */
int ragmi_disparity_regression_bwd(const void* dout, void* dprob, int B, int D, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Loss + evaluation metrics in one pass.  mask = 0 < gt < maxdisp (approaches/rag.py:210, 418).
 * out[0] = masked smooth-L1 loss over the batch (rag.py:211, 419); out[1..5] = EPE, D1, Thres1, Thres2, Thres3 of
 * utilstool/metrics.py:45-65, each the mean over the images that pass metrics.py:30's 10 % mask rule; out[6] = masked pixel
 * count; out[7] = images kept.  est, gt: [B,H,W] fp32; acc: B*8 floats of scratch; out: 8 floats. */
int ragmi_stereo_metrics_fwd(const void* disp_est, const void* disp_gt, int B, int H, int W, float maxdisp, void* acc, void* out,
                             void* stream);

/* The same three launches, and the epoch's meter (AverageMeterDict of utilstool/experiment.py:126-151, which the reference feeds
 * with six .item() floats per batch, rag.py:386-396, 457-466) updated in the finalize kernel: after storing out[0..7] its one
 * thread adds, in double, meter[k] += (double)out[k] for k < 6 (the stored floats, as the reference sums Python floats; a NaN
 * loss propagates), meter[6] += 1 (batches) and meter[7] += out[7] (images kept).  meter: 8 doubles on the device, zeroed by the
 * caller at the start of an epoch; no atomics, no memset, no extra launch.  out is bit for bit ragmi_stereo_metrics_fwd's. */
int ragmi_stereo_metrics_meter_fwd(const void* disp_est, const void* disp_gt, int B, int H, int W, float maxdisp, void* acc, void* out,
                                   void* meter, void* stream);

/* gradient of out[0] w.r.t. disp_est: ddisp = gout[0] * [mask] * clamp(est - gt, -1, 1) / out[6] */
int ragmi_masked_smooth_l1_bwd(const void* disp_est, const void* disp_gt, const void* out, const void* gout, void* ddisp,
                               int B, int H, int W, float maxdisp, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Sparsification curves of a per-pixel uncertainty and their areas (AUSE, AURG), per image, in one device pass without a sort
 * (no counterpart in the reference, which has no uncertainty).  disp, unc, gt: [B,H,W] fp32; larger unc = less certain.
 *   mask   0 < gt < maxdisp and disp, unc finite; N = masked pixels of the image
 *   e_q    rint(|double(disp) - double(gt)| 2^20), an integer (saturating at 2^32 - 1, i.e. 4096 px); every error sum is an integer sum
 *   bad    E > 3 && E / |gt| > 0.05 with E = |gt - disp| in fp32 (D1's flag of ragmi_stereo_metrics_fwd)
 *   cuts   j = 0..K-1: r_j = (j N) / K removed, n_j = N - r_j kept
 *   S_x[j] over the n_j pixels of smallest unc (total order on the values, -0 == +0); a group of c pixels of equal unc of which the cut
 *          keeps m contributes double(group sum) * double(m) / double(c), so no tie order enters:
 *          S_epe[j] = float((double(sum below) + share) 2^-20 / double(n_j)), S_d1[j] likewise over the bad counts
 *   O_epe[j] the same with e_q as the key;  O_d1[j] = max(0, Nbad - r_j) / n_j
 *   AUSE_x = mean_j(S_x[j] - O_x[j]),  AURG_x = mean_j(S_x[0] - S_x[j]), in double over the stored floats, j ascending
 * curves: [B,4,K] fp32 = S_epe, O_epe, S_d1, O_d1;  scalars: [B,6] fp32 = AUSE_epe, AURG_epe, AUSE_d1, AURG_d1, N, Nbad.  An image with
 * N = 0 gets NaN in its curves and its four areas (N = Nbad = 0 are stored) and is not added to the meter.
 * meter (may be NULL): double [4K + 7], 8-byte aligned, zeroed by the caller at the start of an epoch: a last one-workgroup launch adds
 * the counted images' 4K curve floats and 6 scalars in double, images in order, one thread per column, and their number to meter[4K + 6].
 * workspace: 16-byte aligned, ragmi_sparsification_workspace_elems(B,H,W,K) elements of 16 bytes =
 *   2 B (2048 + 3 K 128)      histogram bins {u32 count, u32 bad, u64 sum e_q} of the 11 / 7 / 7 / 7-bit radix levels, two keys
 *   + 2 B (4 * 32 * 3 + 1)    cut records of the four levels and {N, Nbad}
 * (0 for sizes the call refuses; independent of H and W; 2.5 MB at B = 8, K = 20); cleared on the stream by the call's first kernel.
 * Ten launches (eleven with a meter), kernels only (no memset / memcpy node); 64-bit integer atomics only, so bitwise reproducible;
 * no allocation, no host synchronisation.  RAGMI_EINVAL before any launch: a null disp / unc / gt / workspace / curves / scalars,
 * B, H, W <= 0 or B > 65535, K outside 1..32, H * W >= 2^31, maxdisp <= 0, a workspace not 16-byte or a meter not 8-byte aligned. */
int64_t ragmi_sparsification_workspace_elems(int B, int H, int W, int K);
int ragmi_sparsification_fwd(const void* disp, const void* unc, const void* gt, int B, int H, int W, float maxdisp, int K,
                             void* workspace, void* curves, void* scalars, void* meter, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Self-supervised loss of the continual-adaptation mode (src_self/approaches/rag.py:266-278, supervise=False):
 * re_and_sm_loss(disp, left, right) of src_self/models/loss.py:112-141 and its gradient with respect to disp.
 *   left_est[c] = m * bilinear(right[c], xs, ys), xs = ((2 (x - d)/(W-1) - 1 + 1) W - 1)/2, ys = ((2 y/(H-1) - 1 + 1) H - 1)/2
 *                 (warp, loss.py:6-37: align_corners=True normalisation, grid_sample's default align_corners=False, zero padding);
 *                 m = 1 where the same sample of an all-ones image is >= 0.9999, else 0 (no gradient through m);
 *   out[1] = SSIM_mean: clamp((1 - S)/2, 0, 1) over the non-overlapping 3x3 blocks of avg_pool2d(kernel_size=3) (loss.py:77-97;
 *            the H%3 / W%3 remainder takes no part), C1 = 1e-4, C2 = 9e-4, sigma = E[x^2] - mu^2;
 *   out[2] = L1_mean: mean |left - left_est| over B*C*H*W (loss.py:64-75);
 *   out[3] = smoothness: sum over x-edges |d(x) - d(x+1)| exp(-|mean_c(left(x) - left(x+1))|) + the same over y-edges, / (B*H*W)
 *            (loss.py:122-139);
 *   out[0] = 0.85 out[1] + 0.15 out[2] + 0.1 out[3].
 * left, right: [B,C,H,W], disp: [B,H,W], all fp32 (dtype must be RAGMI_F32), C in 1..4, H, W >= 3; out: 4 floats; workspace:
 * ragmi_selfsup_loss_workspace_elems(B,H,W) floats, 8-byte aligned, scratch.  unit_grad (may be NULL: no gradient work) receives
 * d out[0] / d disp, [B,H,W].  Two launches, no atomics (bitwise reproducible), no memset, no host synchronisation. */
int64_t ragmi_selfsup_loss_workspace_elems(int B, int H, int W);
int ragmi_selfsup_loss_fwd(const void* left, const void* right, const void* disp, int B, int C, int H, int W, int dtype,
                           void* workspace, void* out, void* unit_grad, void* stream);

/* backward of ragmi_selfsup_loss_fwd's out[0]: grad[i] = gout[0] * unit_grad[i], i < n (gout read on the device) */
int ragmi_selfsup_loss_bwd(const void* unit_grad, const void* gout, void* grad, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Occlusion-aware self-supervised step: the two-view batch, the left-right consistency check and the weighted loss.
 *
 * ragmi_lr_stack_fwd: out_left = [left ; mirror_x(right)], out_right = [right ; mirror_x(left)], both [2B,C,H,W] fp32 from left,
 * right [B,C,H,W] fp32 (mirror_x(v)[x] = v[W-1-x]).  Sample i < B is the ordinary pair, sample i + B the pair seen from the right
 * camera.  One launch that only moves data (a kernel, not a memcpy node); the outputs are the caller's and must not alias the
 * inputs.
 *
 * ragmi_lr_check_fwd: disp [B,H,W] fp32, disparities in their own view; the partner map of image b is
 * partner[(b + partner_shift) mod B], read mirrored along x when mirrored != 0 (element x is p[W-1-x]; never materialised).
 * Per pixel, d = disp[b,y,x], xr = x - d:
 *   in view     iff d is finite and 0 <= xr <= W-1;
 *   d'          = (1-f) p[x0] + f p[x1], x0 = floor(xr), x1 = min(x0+1, W-1), f = xr - x0, on the (mirrored) partner row;
 *   e           = |d - d'|;
 *   consistent  iff in view, e finite and e <= max(abs_tol, rel_tol |d|).
 * weight[b,y,x] = 1 if consistent, else occluded_weight (in [0, 1]); err[b,y,x] = e if in view and finite, else +inf (err may be
 * NULL); valid[b] = float(double(consistent pixels of image b) / double(H W)).  A non-finite d or tap stays in its own pixel and is
 * never used as an index.  For the stacked batch: disp = partner = the [2B,H,W] output, partner_shift = B, mirrored = 1.
 * workspace: ragmi_lr_check_workspace_elems(B,H,W) 4-byte elements, scratch.  Refused before any launch: a null pointer (but err),
 * B < 1, H < 1, W < 2, partner_shift outside [0, B), a tolerance that is negative or not finite, an occluded_weight outside [0, 1]
 * or not finite.  Two launches; integer counts per workgroup slot folded in a fixed order: no atomics, no memset, bitwise
 * reproducible, no host synchronisation. */
int ragmi_lr_stack_fwd(const void* left, const void* right, void* out_left, void* out_right, int B, int C, int H, int W, void* stream);
int64_t ragmi_lr_check_workspace_elems(int B, int H, int W);
int ragmi_lr_check_fwd(const void* disp, const void* partner, int B, int H, int W, int partner_shift, int mirrored, float abs_tol,
                       float rel_tol, float occluded_weight, void* workspace, void* weight, void* err, void* valid, void* stream);

/* ragmi_selfsup_loss_fwd with a per-pixel weight w = weight [B,H,W] fp32 (finite and non-negative: the caller's contract; constant,
 * no gradient flows to it) on the photometric terms; wb = avg_pool2d(w, 3), the mean of w over each 3x3 SSIM block:
 *   out[2] = L1   = sum_{b,c,y,x} w |left - left_est| / (C sum w);
 *   out[1] = SSIM = sum_{blocks,c} wb term / (C sum wb), term the clamped (1 - S)/2 of ragmi_selfsup_loss_fwd;
 *   out[3] = smoothness, unchanged and unweighted;   out[0] = 0.85 out[1] + 0.15 out[2] + 0.1 out[3].
 * A term whose weights sum to 0 is 0, and so is its gradient.  Other arguments and restrictions as ragmi_selfsup_loss_fwd;
 * workspace: ragmi_selfsup_loss_weighted_workspace_elems(B,H,W) floats, 8-byte aligned.  Four launches (a fixed-order pre-pass
 * leaves sum w and sum wb as two doubles on the device, the main kernel reads them): no atomics, no memset or memcpy, no host
 * synchronisation, bitwise reproducible.  _bwd: grad[i] = gout[0] * unit_grad[i] (ragmi_selfsup_loss_bwd's launch). */
int64_t ragmi_selfsup_loss_weighted_workspace_elems(int B, int H, int W);
int ragmi_selfsup_loss_weighted_fwd(const void* left, const void* right, const void* disp, const void* weight, int B, int C, int H,
                                    int W, int dtype, void* workspace, void* out, void* unit_grad, void* stream);
int ragmi_selfsup_loss_weighted_bwd(const void* unit_grad, const void* gout, void* grad, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Dense disparity: fill what a keep map (the left-right check's weight, or any mask) rejects, by background interpolation.
 *
 * ragmi_disp_fill_fwd: disp [B,H,W] fp32; keep [B,H,W], uint8 with non-zero = keep (keep_is_u8 != 0) or fp32 with == 1.0f = keep
 * (keep_is_u8 == 0; ragmi_lr_check_fwd's weight as it is).  A pixel is RELIABLE iff it is kept and its disparity is finite; a
 * value that is not reliable is never read as a value.
 *   Row pass, for a row with at least one reliable pixel; L / R = the nearest reliable pixel left / right of an unreliable x:
 *     both exist: out = (v[R] < v[L]) ? v[R] : v[L] (the farther surface; a tie or a signed zero takes the left value), code 1;
 *     one exists: out = that value, code 2;        a reliable pixel: out = its value, bit for bit, code 0.
 *   Column pass, for a row without a reliable pixel; U / D = the nearest rows above / below that have one, r = the row pass's result:
 *     both exist: out = (r[D,x] < r[U,x]) ? r[D,x] : r[U,x], code 3;     one exists: that one, code 4;
 *     neither (the image has no reliable pixel): out = fill_value, code 5.
 * out [B,H,W] fp32 (every value a copy of a reliable input or fill_value: finite), code [B,H,W] uint8, counts [B,6] int32 (pixels
 * per code), density [B] fp32 = float(double(counts[b,0]) / double(H W)).  workspace: ragmi_disp_fill_workspace_elems(B,H,W) 4-byte
 * elements (a flag per row, six counts per workgroup), scratch.  out must not alias disp or keep.  Any H, W >= 1.
 * Three launches (row pass, column pass, count finalize); integer counts per workgroup slot folded in a fixed order: no atomics, no
 * memset or memcpy, no host synchronisation, bitwise reproducible; every output and every workspace element read is written first.
 *
 * ragmi_disp_median_fwd: out[b,y,x] = the median (the (m*m+1)/2-th smallest) of the m x m values in[b, clamp(y+j,0,H-1),
 * clamp(x+i,0,W-1)], |i|, |j| <= m/2, m = 3 or 5; in, out [B,H,W] fp32, in != out; the result is a copy of one of them (finite
 * inputs: the caller's contract, ragmi_disp_fill_fwd's out satisfies it).  One launch.
 *
 * Refused before any launch, without touching a pointer: a null pointer, a size < 1, a fill_value that is not finite, m other than
 * 3 or 5, in == out, a workspace that is not 4-byte aligned, sizes whose grid or per-image pixel count would pass 2^31 - 1. */
int64_t ragmi_disp_fill_workspace_elems(int B, int H, int W);
int ragmi_disp_fill_fwd(const void* disp, const void* keep, int keep_is_u8, int B, int H, int W, float fill_value, void* workspace,
                        void* out, void* code, void* counts, void* density, void* stream);
int ragmi_disp_median_fwd(const void* in, void* out, int B, int H, int W, int m, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Speckle filter: segment a disparity map into connected regions of similar disparity and reject the small ones (the step between
 * the left-right check and ragmi_disp_fill_fwd; OpenCV's filterSpeckles).
 *
 * ragmi_speckle_fwd: disp [B,H,W] fp32; keep [B,H,W] by keep_kind: 0 = fp32 weight (== 1.0f keeps; ragmi_lr_check_fwd's weight as
 * it is), 1 = uint8 (non-zero keeps), 2 = none (every pixel is kept; keep may then be NULL).  max_size: integer >= 0; max_diff:
 * finite, >= 0.
 *   A pixel is RELIABLE iff it is kept and its disparity is finite (ragmi_disp_fill_fwd's own rule); a value that is not reliable is
 *   never read as a value.
 *   Two 4-neighbours p, q are JOINED iff both are reliable and fabsf(d_p - d_q) <= max_diff, evaluated in fp32 as one IEEE
 *   subtraction, one absolute value and one comparison, no other arithmetic; a difference that overflows to Inf does not join;
 *   diagonal neighbours never join.
 *   A SEGMENT is a connected component of that graph: similarity is per edge, so a ramp 5.0, 5.8, 6.6 with max_diff = 1 is one segment.
 * Outputs:
 *   label    [B,H,W] int32  the smallest y*W + x of the pixel's segment (a per-image index); -1 for an unreliable pixel
 *   size     [B,H,W] int32  the segment's pixel count; 0 for an unreliable pixel
 *   keep_out [B,H,W] uint8  1 iff reliable and size > max_size (a segment of at most max_size pixels is a speckle: OpenCV's rule;
 *                           with max_size = 0 keep_out is "reliable" and the call is a pure labelling)
 *   counts   [B,5]   int32  RAGMI_SPECKLE_COUNTS: reliable pixels, segments, removed pixels, removed segments, the largest segment's
 *                           size (0 if there is none)
 *   density  [B]     fp32   float(double(reliable - removed pixels) / double(H W))
 * workspace: ragmi_speckle_workspace_elems(B,H,W) 4-byte elements (three per pixel: parent, tile-local count, total; five counts
 * per workgroup of 1024 pixels; 0 for sizes that ragmi_speckle_fwd refuses), scratch.  The outputs must not alias the inputs.
 * Any H, W >= 1.
 * Five launches in a fixed sequence (tile labelling in LDS over RAGMI_SPECKLE_TILE_ROWS x RAGMI_SPECKLE_TILE_COLS tiles, lock-free
 * union at the tile seams, flatten and total, apply, count finalize; the seam launch is absent where the image is a single tile): no
 * loop over launches, no flag read by the host.  Integer atomics only (min, add: order-independent), no float atomics, no memset or
 * memcpy, no host synchronisation, graph-capturable, bitwise reproducible; every output element and every workspace element that is
 * read is written first by the call.
 *
 * Refused with status -1 before any launch, without touching a pointer: a null pointer (except keep with kind 2), a size < 1,
 * max_size < 0, a max_diff that is negative or not finite, an unknown keep_kind, a workspace that is not 4-byte aligned, sizes whose
 * grid or per-image pixel count would pass 2^31 - 1. */
#define RAGMI_SPECKLE_TILE_ROWS 16
#define RAGMI_SPECKLE_TILE_COLS 64
#define RAGMI_SPECKLE_COUNTS 5
int64_t ragmi_speckle_workspace_elems(int B, int H, int W);
int ragmi_speckle_fwd(const void* disp, const void* keep, int keep_kind, int B, int H, int W, int max_size, float max_diff,
                      void* workspace, void* label, void* size, void* keep_out, void* counts, void* density, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Depth head of the monocular-depth network (rag_depth/src/models/rag_model.py:51-64, 357-416) as ONE launch:
 *   u   = bilinear(y, (H, W), align_corners=True)                      (upsample_6)
 *   m   = conv3x3(u, w3[1, Cin, 3, 3]), zero padding 1, no bias         (last_3_3d: bn=False, relu=False)
 *   s   = sigmoid(conv3x3(m, w1[1, 1, 3, 3]) + b1[0]), zero padding 1   (DispHead.conv1 + sigmoid)
 *   out = max_depth * bilinear(s, x scale, align_corners=False)        (F.interpolate(scale_factor=scale); source index clamped)
 * y: [B, Cin, Hi, Wi] contiguous, out: [B, scale*H, scale*W]; w3, w1, b1 are device pointers (b1 is never read on the host).
 * fp32 only (dtype must be RAGMI_F32); Cin 1..16, Hi <= H, Wi <= W, scale 1..8 (ragmi_depth_head_supported returns 1 for a built
 * combination).  No allocation, no host synchronisation. */
int ragmi_depth_head_supported(int Cin, int Hi, int Wi, int H, int W, int scale, int dtype);
int ragmi_depth_head_fwd(const void* y, const void* w3, const void* w1, const void* b1, void* out, int B, int Cin, int Hi, int Wi,
                         int H, int W, int scale, float max_depth, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Depth loss + evaluation metrics in one pass (rag_depth/src/approaches/rag.py:440-489) over the n pixels of (est, gt) with
 * gt > 0, the whole batch together.  out10 = silog_loss (sqrt(mean d^2 - variance_focus mean(d)^2) * 10, d = log est - log gt,
 * utilstool/experiment.py:154-161), then compute_errors (approaches/rag.py:19-41): silog, abs_rel, log10, rms, sq_rel, log_rms,
 * d1, d2, d3.  No clamping: est == 0 or no masked pixel gives the reference's inf / NaN.  workspace:
 * ragmi_depth_metrics_workspace_elems(n) floats, 8-byte aligned, scratch.  fp32 only.  Two launches, no atomics (bitwise
 * reproducible), no memset, no host synchronisation. */
int ragmi_depth_metrics_workspace_elems(long long n);
int ragmi_depth_metrics_fwd(const void* est, const void* gt, long long n, float variance_focus, void* workspace, void* out10, int dtype,
                            void* stream);
/* The same two launches on the same kernels, for one batch of the unit search's loops (approaches/rag.py:401-427, 501-522).  Either
 * of the two further pointers may be null; both must be 8-byte aligned.
 *   saved3  (double[3]): {n, mean d, sqrt(mean d^2 - variance_focus mean(d)^2)}, what ragmi_silog_loss_fwd saves: with it
 *           ragmi_silog_loss_bwd is the backward of out10[0] (bit for bit the loss of ragmi_silog_loss_fwd).
 *   meter12 (double[12]): the epoch's meter.  The finalize kernel's one thread stores out10, then meter[k] += (double)out10[k] for
 *           k = 0..9 (the float it just stored), meter[10] += 1 (batches), meter[11] += n (masked pixels).  No atomics, no memset,
 *           no extra launch; a batch with no masked pixel adds NaN (the reference's numpy mean of an empty selection).
 * The caller zeroes meter12 at the start of an epoch. */
int ragmi_depth_metrics_meter_fwd(const void* est, const void* gt, long long n, float variance_focus, void* workspace, void* out10,
                                  void* saved3, void* meter12, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Backward of ragmi_depth_head_fwd (the depth training step, rag_depth/src/approaches/rag.py:182-246; the forward chain is
 * rag_model.py:51-64, 357-416): d_out [B, scale*H, scale*W] -> dy [B, Cin, Hi, Wi] (written), dw3 [Cin*9], dw1 [9], db1 [1]
 * (accumulate: bit 0 for dw3, bit 1 for dw1, bit 2 for db1; a clear bit writes the gradient, a set bit adds it to what the buffer
 * holds, e.g. a gradient bucket's view).  u, m, z and s are recomputed from y;
 * the forward saves nothing.  Same shapes and dtype as the forward (ragmi_depth_head_supported); all pointers non-NULL; workspace:
 * ragmi_depth_head_bwd_workspace_elems(B, Cin, H, W) floats, 8-byte aligned, scratch.  Two launches, no atomics (bitwise
 * reproducible), no memset, no host synchronisation. */
int64_t ragmi_depth_head_bwd_workspace_elems(int B, int Cin, int H, int W);
int ragmi_depth_head_bwd(const void* y, const void* w3, const void* w1, const void* b1, const void* d_out, void* dy, void* dw3,
                         void* dw1, void* db1, int accumulate, void* workspace, int B, int Cin, int Hi, int Wi, int H, int W, int scale,
                         float max_depth, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * silog_loss of the depth training step (rag_depth/src/utilstool/experiment.py:154-161, used at approaches/rag.py:237-239) over
 * the n pixels of (est, gt) with gt > 0, the whole batch together: d = log est - log gt,
 *   out[0] = 10 sqrt(mean d^2 - variance_focus mean(d)^2)      (float)
 *   saved  = {n, mean d, sqrt(mean d^2 - variance_focus mean(d)^2)}   (3 doubles, 8-byte aligned; input of the backward)
 * No masked pixel gives the reference's NaN loss.  workspace: ragmi_silog_loss_workspace_elems(n) floats, 8-byte aligned, scratch.
 * fp32 only (dtype must be RAGMI_F32; bf16 is refused with RAGMI_EUNSUPPORTED).  Two launches, no atomics (bitwise reproducible),
 * no memset, no host synchronisation. */
int ragmi_silog_loss_workspace_elems(long long n);
int ragmi_silog_loss_fwd(const void* est, const void* gt, long long n, float variance_focus, void* workspace, void* out, void* saved,
                         int dtype, void* stream);

/* gradient of out[0]: grad[i] = gout[0] * 10 (d_i - variance_focus mean d) / (n sqrt(.) est_i) where gt > 0, else 0; all zeros
 * when n = 0 (the loss is then NaN, but no NaN reaches a gradient).  gout is read on the device.  One launch. */
int ragmi_silog_loss_bwd(const void* est, const void* gt, long long n, float variance_focus, const void* saved, const void* gout,
                         void* grad, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * clip_grad_norm_(max_norm) + torch.optim.SGD(lr, momentum, weight_decay).step() over flat fp32 buffers of n elements
 * (approaches/rag.py:64-70, 215-216) as two launches: g *= min(1, max_norm/(||g||+1e-6)) (max_norm <= 0: no clipping);
 * d = g + weight_decay*p; buf = first_step ? d : momentum*buf + d; p -= lr*buf.  norm_out (may be NULL) receives ||g|| before
 * clipping; workspace: ragmi_sgd_workspace_bytes() bytes of device scratch. */
int64_t ragmi_sgd_workspace_bytes(void);
int ragmi_sgd_clip_step(void* param, void* grad, void* momentum_buf, int64_t n, float lr, float momentum, float weight_decay,
                        float max_norm, int first_step, void* workspace, void* norm_out, void* stream);

/* The same step over the elements with active[i] != 0 only (active: n bytes on the device): the step of a supernet whose forward
 * ran one sampled operation per edge (automl/mdenas_search.py:161-173).  torch.optim.SGD skips a parameter whose .grad is None -
 * no weight decay, no momentum, momentum buffer created at that parameter's own first update - so p, g and buf of an inactive
 * element are neither read nor written, and the norm and the clip coefficient are taken over the active elements only (all
 * inactive: norm 0, nothing moves).  Active elements: g *= coef; d = g + weight_decay*p; buf = momentum*buf + d; p -= lr*buf.
 * There is no first_step: momentum_buf must start at zero, and an element's first update then gives buf = d exactly.  With every
 * byte non-zero the result equals ragmi_sgd_clip_step(first_step = 0) bit for bit.  Two launches, fp64 partial sums in a fixed
 * order, no atomics, no memset.  RAGMI_EINVAL before any launch: a NULL param / grad / momentum_buf / active / workspace, n <= 0,
 * a negative lr / momentum / weight_decay. */
int ragmi_sgd_clip_step_masked(void* param, void* grad, void* momentum_buf, const void* active, int64_t n, float lr, float momentum,
                               float weight_decay, float max_norm, void* workspace, void* norm_out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Batch preparation on the device (the reference's loaders: src/dataloaders/data_io.py:6-13, stereo_dataset.py:35-38, 57-121;
 * src_self/dataloaders/sceneflow_driving_dataset.py:53-70), ONE launch per batch:
 *   left_u8, right_u8 [B,Hs,Ws,3] uint8 (HWC, as decoded)  ->  left, right [B,3,H,W] fp32
 *   gt [B,Hs,Ws] uint16 (RAGMI_GT_U16) or fp32 (RAGMI_GT_F32)  ->  gt_out [B,H,W] fp32 = (float)gt * gt_scale (1/256 for KITTI-style
 *   16-bit disparities: exact)
 * Output pixel (y, x) of sample b reads source pixel (y + origin[b,0], x + origin[b,1]) and is 0 where that falls outside the
 * source; origin: device int32 [B,2].  A training crop is origin = (y1, x1); the evaluation pad is origin = (-top_pad, 0) (the pad
 * is 0 AFTER normalisation, as the reference pads).  Image values are ToTensor + Normalize in fp32, bit for bit:
 * ((float)u / 255 - mean_c) / std_c with two IEEE divisions.  With stats_source (and stats_left, and stats_right when there is a
 * right view; each float64 [B,3,2] = (mean, std of column stds) per channel, as ragmi_color_stats writes) every byte first goes
 * through transfer_color's float64 sequence t = u/255; t -= tm; t /= ts/ss; t += sm; clip(t,0,1); trunc(t*255), and that level is
 * normalised.  ts == 0 gives an unspecified level (the reference divides by zero), never a fault.  right_u8/right and gt/gt_out
 * may be NULL in pairs.  RAGMI_EINVAL: null pointer, non-positive size, misaligned pointer; RAGMI_EUNSUPPORTED: gt_dtype.
 * No allocation, no host synchronisation, no host copy: the launch replays with new origins and new bytes. */
#define RAGMI_GT_F32 0
#define RAGMI_GT_U16 1
int ragmi_prep_batch(const void* left_u8, const void* right_u8, const void* gt, int gt_dtype, float gt_scale, const void* origin,
                     void* left, void* right, void* gt_out, int B, int Hs, int Ws, int H, int W, float mean0, float mean1, float mean2,
                     float std0, float std1, float std2, const void* stats_left, const void* stats_right, const void* stats_source,
                     void* stream);

/* Colour statistics of transfer_color for img_u8 [B,Hs,Ws,3] uint8: stats [B,3,2] float64 = per channel the mean of u/255 and the
 * population std over columns of the per-column population stds (numpy's x.std(0).std(0)).  The column sums of u and u^2 are
 * accumulated exactly in 64-bit integers; the rest is double, reduced in a fixed order.  workspace:
 * ragmi_color_stats_workspace_elems(B,Hs,Ws) 8-byte elements, 8-byte aligned, scratch.  Two launches, no atomics (bitwise
 * reproducible), no memset, no host synchronisation. */
int64_t ragmi_color_stats_workspace_elems(int B, int Hs, int Ws);
int ragmi_color_stats(const void* img_u8, int B, int Hs, int Ws, void* workspace, void* stats, void* stream);

/* transfer_color as an image: out_u8 [B,H,W,3] uint8 from target_u8 with statistics stats_target against stats_source (both
 * float64 [B,3,2]); the same per-byte sequence as ragmi_prep_batch's.  One launch. */
int ragmi_color_transfer(const void* target_u8, const void* stats_target, const void* stats_source, void* out_u8, int B, int H, int W,
                         void* stream);

/* Lanczos resize on the device, Pillow's arithmetic bit for bit: the Cityscapes branch of the reference's loaders
 * (src_self/dataloaders/stereo_dataset.py:56-69: left / right / disparity .resize((1024, 512), Image.ANTIALIAS), ANTIALIAS being
 * Lanczos, before the crop or pad; disparity / 256 / 2).  The taps come from the caller, per axis (y: Hs -> Hr, x: Ws -> Wr), as
 * Pillow's precompute_coeffs gives them in float64 (rag_amd.data.lanczos_taps), all on the device:
 *   bounds    int32 [m,2]        (first source index, tap count) per output index
 *   taps_i32  int32 [m,ksize]    8-bit path: the tap * 2^22 rounded half away from zero, 0 past the tap count
 *   taps_f64  float64 [m,ksize]  16-bit path: the tap, 0 past the tap count
 * with ksize = 2 * ceil(3 * max(n/m, 1)) + 1, and for n == m (an axis Pillow does not filter) the identity: bounds (i, 1), one tap
 * 2^22 / 1.0, ksize 1.  8-bit: clip8((2^21 + sum px * K) >> 22) in int32.  16-bit (I;16): a double from 0.0, acc += px * k in
 * ascending order with product and sum rounded separately, r = (int)(acc +- 0.5), the bytes clip8(r % 256) and clip8(r >> 8)
 * clipped separately.  The horizontal pass runs first and is stored as uint8 / uint16 before the vertical one.
 *
 * One workgroup resamples one 16x64 output tile from the window of source pixels it needs, staged in LDS; the window is sized on
 * the host from the sizes alone and every table entry is clamped to it, so a wrong table gives wrong pixels and never an access
 * out of bounds.  RAGMI_EUNSUPPORTED: a window that does not fit the 160 KiB of LDS (an extreme downscale); nothing is launched.
 * RAGMI_EINVAL: null / misaligned pointer, non-positive size, a ksize other than the formula's.  One launch each, no allocation,
 * no host synchronisation, no atomics, no memset or memcpy.
 *
 * ragmi_prep_batch_resized: ragmi_prep_batch with the resize in front, still ONE launch and without the resized image in memory
 * (stereo_dataset.py:56-69 then :73-122).  left_u8, right_u8 [B,Hs,Ws,3] uint8 and gt [B,Hs,Ws] uint16 (gt_dtype must be
 * RAGMI_GT_U16: the reference resizes PNGs only) are resized to Hr x Wr; origin (device int32 [B,2]) addresses the RESIZED image:
 * output pixel (y, x) is resized pixel (y + origin[b,0], x + origin[b,1]), 0 outside it (after normalisation); gt_out =
 * (float)resized * gt_scale (1/512 for the reference's / 256 / 2: exact).  No colour transfer.  ytaps_f64 / xtaps_f64 may be NULL
 * without a gt. */
int ragmi_prep_batch_resized(const void* left_u8, const void* right_u8, const void* gt, int gt_dtype, float gt_scale, const void* origin,
                             void* left, void* right, void* gt_out, int B, int Hs, int Ws, int Hr, int Wr, int H, int W, float mean0,
                             float mean1, float mean2, float std0, float std1, float std2, const void* ybounds, const void* ytaps_i32,
                             const void* ytaps_f64, int yksize, const void* xbounds, const void* xtaps_i32, const void* xtaps_f64,
                             int xksize, void* stream);
/* The resize alone (stereo_dataset.py:59-61), the same kernel and device functions: [B,Hs,Ws,3] uint8 -> [B,Hr,Wr,3] uint8 (mode
 * RGB) and [B,Hs,Ws] uint16 -> [B,Hr,Wr] uint16 (mode I;16). */
int ragmi_resize_lanczos_u8(const void* src_u8, void* dst_u8, int B, int Hs, int Ws, int Hr, int Wr, const void* ybounds,
                            const void* ytaps_i32, int yksize, const void* xbounds, const void* xtaps_i32, int xksize, void* stream);
int ragmi_resize_lanczos_u16(const void* src_u16, void* dst_u16, int B, int Hs, int Ws, int Hr, int Wr, const void* ybounds,
                             const void* ytaps_f64, int yksize, const void* xbounds, const void* xtaps_f64, int xksize, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Host-side guard for captured steps (no device work): counts the nodes of a captured hipGraph_t by kind.  A captured training
 * step must consist of kernel nodes only: on ROCm 7.2 memset / memcpy NODES of an instantiated graph were corrupted by memcpys
 * issued on the null stream between two replays, so rag_amd.train.GraphedTrainStep refuses a capture for which
 * n_memcpy + n_memset > 0.  `graph`: the hipGraph_t. */
int ragmi_graph_node_census(void* graph, int32_t* n_kernel, int32_t* n_memcpy, int32_t* n_memset, int32_t* n_other);

#ifdef __cplusplus
}
#endif
#endif /* RAG_AMD_H */
