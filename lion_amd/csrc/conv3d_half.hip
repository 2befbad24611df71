// conv3d_half.hip -- C3 at reduced precision, on purpose: the 3x3x3 / pad 1 Conv3d of PVConv's voxel branch with ONE fp16
// product per operand pair,
//   main += W_h * X_h      (v_mfma_f32_32x32x16_f16, fp32 accumulation inside the MFMA),   D = main
// i.e. conv3d_split.hip without the low pieces and without the corr accumulators: a third of its MFMAs, half of its LDS
// operand and weight bytes, half of its accumulator registers.  fp32 in HBM on both sides.
//
// What it computes: both operands carry the split kernel's exact power-of-two block scaling (one scale per weight tensor,
// a monotone scale per (workgroup tile, 16-channel chunk) with accumulator rescaling), so a hi piece is the operand rounded
// to an 11-bit significand (round to nearest even) whatever its magnitude -- operands more than 2^27 below their block's
// maximum go subnormal -- and the result is conv(rne11(W), rne11(act(X))) accumulated in fp32:
//   |y - conv64(rne11 W, rne11 X)| < 5e-6 max|y|  (the fp32-class bound of tests/test_conv_split_gpu.py),
//   |y - conv64(W, X)| <= 2^-10 sum |w||x|         (two roundings of 2^-11 each), elementwise.
// No clamp: |x| > 65504, 1e-30 and mixed ranges are representable; inf / nan stay out of the maximum and reach exactly the
// outputs whose window holds them.  Inference only (conv_ops.PRECISION = "half"); DESIGN.md 4.3.
//
// The kernel is the P = 1 instantiation of the split kernel (conv3d_split_kernel.h, which says where the one-piece form
// departs from the two-piece one) at r = 16 / 32: the same modes -- AdaGN+Swish prologue (PRO), GroupNorm tile sums
// (STATS), work queue + per-wave occupancy masks (occ), constant + delta (tconst), the consumer-aware levels -- and the
// same tile geometry, so the occupancy buffers and the statistics' tile count (lion_conv3d_split_stat_tiles) apply
// unchanged.  The weights are the hi pieces of the SPLIT pack ([Cin/16][27][piece][k-half][Cout][8], piece 0): the first
// half of every tap slice is fetched, there is no packer of its own.  r = 8 stays on the three-product kernel.
#include "conv3d_split_kernel.h"

extern "C" {

// Arguments exactly as lion_conv3d_k3_split_forward (include/lion_hip.h): wp from lion_conv3d_split_pack_weights (only its
// hi pieces and its scale are read), stats with lion_conv3d_split_stat_tiles(r, Cout) tiles, occ from
// lion_conv3d_tile_occupancy[_aware].
int lion_conv3d_k3_half_forward(const float *x, const uint16_t *wp, const float *bias, int B, int Cin, int Cout, int r,
                                const float *pro_a, const float *pro_b, const float *pro_bias, const float *tconst,
                                float *y, float *stats, int32_t *occ, lionStream_t stream) {
  const int e = split_tile_forward<1>(x, wp, bias, B, Cin, Cout, r, pro_a, pro_b, pro_bias, tconst, y, stats, occ,
                                      static_cast<hipStream_t>(stream));
  return e == LION_SPLIT_NO_TILE ? LION_EINVAL : e; // r = 8 stays on the three-product kernel
}

} // extern "C"
