// NOT BUILT, not part of the library: the merged "fold of conv1 + constant response of conv2" launch that was built, tested
// bit-identical to lion_groupnorm_fold + lion_conv3d_const_response, measured and NOT adopted
// (profiles/small_launches_ab.txt).  A workgroup of NB blocks of 256 threads folds its whole sample NB
// groups at a time with gn_fold_kernel's own lane mapping, then runs the response of NB border configurations.  In a 20-call
// graph at B = 32 it took 8.8 / 10.7 / 11.5 / 15.8 us (NB = 4) against 6.7 / 7.7 / 8.1 / 10.4 us for the two launches it
// replaces; NB = 2: 11.9 .. 17.8, NB = 1: 16.5 .. 19.8 -- about 1.3 us per round of groups (one L2 round trip, the double
// butterfly, a barrier), which a dependent launch (3 us here) does not cost.  To build it: paste the three parts into
// csrc/conv3d.hip (helpers above gn_fold_kernel, kernel below conv_tconst_kernel, entry among the extern "C" functions).

// ---- helpers (gn_fold_kernel rewritten on them compiles to the same ISA as today's) ----
// The two halves of a group's fold, shared by gn_fold_kernel and gn_fold_tconst_kernel (same lane-to-(channel, tile) mapping,
// same butterfly, same fixed-order loops: the same bits from either).  `t` is the thread's index in the 256-thread block that
// owns group g, `ws` that block's [4][2] combine buffer in LDS; `on` = the block has a group at all.
// (1) channel sums: valid in the lanes with ch < cpg && sub == 0.
struct GnSums { int ch, sub; double s1, s2; };
__device__ __forceinline__ GnSums gn_fold_channel_sums(const float *stats, int C, int T, int cpg, int b, int g, bool on, int t,
                                                       double (&ws)[4][2]) {
  int cp2 = 1;
  while (cp2 < cpg) cp2 <<= 1;
  const int LPC = 256 / cp2, ch = t / LPC, sub = t % LPC; // LPC in {4, ..., 256}, a power of two
  double s1 = 0.0, s2 = 0.0;
  if (on && ch < cpg) {
    const float2 *p = reinterpret_cast<const float2 *>(stats + (((size_t)b * C + g * cpg + ch) * T) * 2);
    for (int i = sub; i < T; i += LPC) { const float2 v = p[i]; s1 += (double)v.x; s2 += (double)v.y; }
  }
  for (int m = 1; m < LPC && m < 64; m <<= 1) { s1 += __shfl_xor(s1, m, 64); s2 += __shfl_xor(s2, m, 64); }
  if (LPC > 64) { // a channel spans several waves (C/G <= 2): combine through LDS
    if ((t & 63) == 0) *reinterpret_cast<double2 *>(ws[t >> 6]) = make_double2(s1, s2); // ws is 16-byte aligned (alignas at its definitions)
    __syncthreads();
    if (sub == 0) {
      s1 = 0.0; s2 = 0.0;
      for (int w = 0; w < LPC / 64; ++w) { s1 += ws[(t >> 6) + w][0]; s2 += ws[(t >> 6) + w][1]; }
    }
  }
  return {ch, sub, s1, s2};
}
// (2) group totals gs[0], gs[1] over cpg channels of `count` elements -> the folded scalars of channel c = cbase + t of sample b
// (parameters read here, in this order).  A caller that fetched the parameters ahead, or wants the results in registers,
// passes the addresses of its locals and zeros for b, ld_fg, C, cbase, t.
__device__ __forceinline__ void gn_fold_affine(const double *gs, float count, int cpg, float eps, const float *gamma,
                                               const float *beta, const float *fac, const float *gbias, float *A, float *Bs,
                                               int b, int ld_fg, int C, int cbase, int t) {
  const double n = (double)count * cpg;
  const double mean = gs[0] / n;
  double var = gs[1] / n - mean * mean;
  var = var > 0.0 ? var : 0.0;
  const float rstd = (float)(1.0 / sqrt(var + (double)eps));
  const int c = cbase + t;
  const float f = fac[(size_t)b * ld_fg + c], gb = gbias[(size_t)b * ld_fg + c];
  const float a0 = rstd * gamma[c];
  A[(size_t)b * C + c] = a0 * f;
  Bs[(size_t)b * C + c] = (beta[c] - (float)mean * a0) * f + gb;
}


// ---- kernel ----
// gn_fold_kernel (for every group of the sample) and conv_tconst_kernel in ONE launch and one memory round trip each: the
// fold of conv1 is a few hundred flops whose only reader on the spine of a PVConv is the constant response, which waited a
// whole launch for it and then started its weight walk behind the loads of A / Bs.  A workgroup is NB blocks of 256
// threads and owns sample b and NB border configurations.  It requests its first chunk of wsum rows (they depend on
// nothing computed), then folds the WHOLE sample itself -- NB groups at a time, each block exactly as a gn_fold_kernel
// workgroup does (gn_fold_channel_sums / gn_fold_affine: same lanes, same order, same bits) -- forms
// s[c] = pro_act(bias1[c], A, Bs) in LDS and runs conv_tconst_kernel's double accumulation over c = 0 .. Cin-1, one chunk of
// TC_CH rows ahead of the arithmetic.  The fold is recomputed ceil(27 / NB) times per sample (<= 64 KiB of tile sums from
// L2 each); workgroup 0 of a sample writes A / Bs (and chmean where asked).  No hand-over between workgroups.  C <= 256.
#ifndef LION_TC_CH // A/B builds (tools/build_variant.sh): rows of wsum per chunk, blocks per workgroup
#define LION_TC_CH 16
#endif
#ifndef LION_GN_TCONST_NB
#define LION_GN_TCONST_NB 4
#endif
constexpr int TC_CH = LION_TC_CH;
constexpr int GN_TCONST_NB = LION_GN_TCONST_NB; // blocks (= border configurations) per workgroup
template <int NB>
__global__ __launch_bounds__(256 * NB) void gn_fold_tconst_kernel(
    const float *__restrict__ stats, int C, int T, int G, float count, const float *__restrict__ gamma,
    const float *__restrict__ beta, const float *__restrict__ fac, const float *__restrict__ gbias, int ld_fg, float eps,
    const float *__restrict__ wsum, const float *__restrict__ bias2, const float *__restrict__ bias1, int Cout,
    float *__restrict__ A, float *__restrict__ Bs, float *__restrict__ chmean, float *__restrict__ tconst) {
  __shared__ double cs[256][2];
  __shared__ float sc[256];
  __shared__ alignas(16) double ws[NB][4][2];
  const int b = blockIdx.y, tid = threadIdx.x, t = tid & 255, blk = tid >> 8, cpg = C / G;
  const int cfg = blockIdx.x * NB + blk, cfgc = min(cfg, 26);
  const bool writer = blockIdx.x == 0;
  // (0) everything that depends on nothing computed: the first chunk of this thread's wsum column, the channel's parameters
  const float *wcfg = wsum + (size_t)cfgc * C * Cout;
  float cur[TC_CH], nxt[TC_CH];
  {
    const float *w = wcfg + min(t, Cout - 1);
#pragma unroll
    for (int u = 0; u < TC_CH; ++u) cur[u] = w[(size_t)min(u, C - 1) * Cout];
  }
  const int cc = min(tid, C - 1);
  const float p_f = fac[(size_t)b * ld_fg + cc], p_gb = gbias[(size_t)b * ld_fg + cc];
  const float p_gam = gamma[cc], p_bet = beta[cc], p_b1 = bias1 ? bias1[cc] : 0.f;
  // (1) channel sums of every group
  for (int g0 = 0; g0 < G; g0 += NB) {
    const int g = g0 + blk;
    const GnSums q = gn_fold_channel_sums(stats, C, T, cpg, b, g, g < G, t, ws[blk]);
    if (g < G && q.ch < cpg && q.sub == 0) {
      cs[g * cpg + q.ch][0] = q.s1;
      cs[g * cpg + q.ch][1] = q.s2;
      if (writer && chmean) chmean[(size_t)b * C + g * cpg + q.ch] = (float)(q.s1 / count);
    }
    __syncthreads(); // cs is complete after the last round; the combine buffer of gn_fold_channel_sums is free again
  }
  // (2) group totals in gn_fold_kernel's order, the folded scalars, the constant conv2 takes away from the points
  if (tid < C) {
    const int c0 = (tid / cpg) * cpg;
    double gt[2] = {0.0, 0.0};
    for (int c = 0; c < cpg; ++c) { gt[0] += cs[c0 + c][0]; gt[1] += cs[c0 + c][1]; }
    float a, bs;
    gn_fold_affine(gt, count, cpg, eps, &p_gam, &p_bet, &p_f, &p_gb, &a, &bs, 0, 0, 0, 0, 0);
    sc[tid] = pro_act(p_b1, a, bs);
    if (writer) { A[(size_t)b * C + tid] = a; Bs[(size_t)b * C + tid] = bs; }
  }
  __syncthreads();
  // (3) conv_tconst_kernel's sum, chunk i + 1 (or the next column's first) in flight under the arithmetic of chunk i
  for (int co = t; co < Cout; co += 256) {
    double acc = bias2 ? (double)bias2[co] : 0.0;
    for (int k0 = 0; k0 < C; k0 += TC_CH) {
      const bool last = k0 + TC_CH >= C;
      const float *w = wcfg + min(last ? co + 256 : co, Cout - 1);
      const int kn = last ? 0 : k0 + TC_CH;
#pragma unroll
      for (int u = 0; u < TC_CH; ++u) nxt[u] = w[(size_t)min(kn + u, C - 1) * Cout]; // clamped: issued on every path
#pragma unroll
      for (int u = 0; u < TC_CH; ++u)
        if (k0 + u < C) acc += (double)cur[u] * (double)sc[k0 + u];
#pragma unroll
      for (int u = 0; u < TC_CH; ++u) cur[u] = nxt[u];
    }
    if (cfg < 27) tconst[((size_t)b * 27 + cfg) * Cout + co] = (float)acc;
  }
}


// ---- entry point ----
// lion_groupnorm_fold (all groups of a sample) + lion_conv3d_const_response of the convolution that reads the folded layer,
// in one launch: the arguments of the first (chmean may be NULL here), then wsum f32[27][C][Cout], bias2 f32[Cout] or NULL,
// bias1 f32[C] or NULL of the second -> A, Bs f32[B,C] and tconst f32[B][27][Cout], all three the bits of the two calls.
// The limits of both: C / G <= 64 (LION_EINVAL, as lion_groupnorm_fold), C = Cin <= 256 (LION_EUNSUPPORTED).
int lion_groupnorm_fold_const_response(const float *stats, int B, int C, int T, int G, int voxels, const float *gamma,
                                       const float *beta, const float *fac, const float *gbias, int ld_fg, float eps,
                                       const float *wsum, const float *bias2, const float *bias1, int Cout, float *A,
                                       float *Bs, float *chmean, float *tconst, lionStream_t stream) {
  if (!stats || !gamma || !beta || !fac || !gbias || !A || !Bs || !wsum || !tconst) return LION_EINVAL;
  if (B <= 0 || C <= 0 || T <= 0 || G <= 0 || C % G != 0 || C / G > 64 || ld_fg < C || Cout <= 0) return LION_EINVAL;
  if (C > 256) return LION_EUNSUPPORTED;
  constexpr int NB = GN_TCONST_NB;
  return lion_launch<gn_fold_tconst_kernel<NB>>(dim3(lion_cdiv(27, NB), B), 256 * NB, 0, static_cast<hipStream_t>(stream), stats,
                                                C, T, G, (float)voxels, gamma, beta, fac, gbias, ld_fg, eps, wsum, bias2, bias1,
                                                Cout, A, Bs, chmean, tconst);
}

