// conv3d_split.hip -- C3 on the 16-bit matrix pipe at fp32 accuracy: the 3x3x3 / pad 1 Conv3d of PVConv's voxel
// branch (models/pvcnn2_ada.py:211-222) with every fp32 operand cut into two fp16 pieces.
//
// Why: conv3d.hip already runs at 0.86-0.89 of the fp32-input MFMA peak (157 TF), i.e. the fp32 pipe itself is the
// ceiling of shapes/s.  v_mfma_f32_32x32x16_f16 is 16x faster per FLOP, and
//   a = a_h + a_l / 2048,   a_h = fp16(a),  a_l = fp16((a - a_h) * 2048)       (22-23 significant bits)
//   main += W_h * X_h,   corr += W_h * X_l + W_l * X_h      (fp32 accumulation inside the MFMA)
//   D = main + corr / 2048                                   (the dropped W_l * X_l term is 2^-22 relative)
// costs 3 MFMAs of 32 cycles per K = 16 instead of 8 fp32 MFMAs of 64 cycles.  Measured error vs a float64
// convolution: 2.6e-7 rms of the output rms (the fp32 MFMA chain's own: 5e-7 -- it rounds the accumulator 8x more
// often).  tests/test_conv_split_gpu.py holds the dense forms at model shapes and the adversarial dynamic ranges (on the
// r = 16, CB = 2 tile) to the fp32 kernel's 5e-6 of max |y|; tests/test_conv3d_split_numerics_gpu.py holds every plan, form,
// Cin edge, the dynamic ranges on the r = 8 kernel and the CB = 1 tile, and the sparse / constant + delta forms at the three
// consumer-aware levels to the derived elementwise and per-tile bounds of tests/conv3d_split_ref.py.
//
// Range (fp16 has 5 exponent bits): both operands are block-scaled by exact powers of two.
//   weights: one scale per tensor, chosen at pack time so that max |w| * 2^ew lies in [2^13, 2^14);
//   activations: one scale per (workgroup tile, 16-channel chunk), kept MONOTONE along the K loop: the tile's
//   running maximum (after the fused AdaGN+Swish prologue) sets 2^E with max * 2^E in [2^13, 2^14); when a later
//   chunk raises the maximum the accumulators are multiplied by the (exact) power-of-two ratio first.  Every product
//   therefore carries >= 22 bits relative to the LARGEST operand the tile has seen -- block floating point with a
//   23-bit mantissa; there is no clamp: |x| > 65504, 1e-30 and mixed ranges are all representable; inf / nan are left
//   out of the maximum and propagate to exactly the outputs they reach, as in fp32 arithmetic.
//   The epilogue multiplies by 2^-(E + ew) (exact).
//
// Same contract and modes as conv3d.hip::conv3d_k3_kernel: AdaGN+Swish prologue (PRO), GroupNorm tile sums (STATS),
// persistent work queue + per-wave occupancy masks (occ), constant + delta decomposition (tconst).  K is walked in
// chunks of 16 input channels (Cin % 16 == 0; other layers stay on the fp32 kernel).  LDS operand planes
// [piece][k-half][HP halo positions][8 x fp16]: one ds_read_b128 per MFMA fragment, conflict free; the weight slice
// of a tap [piece][k-half][COT][8 x fp16] goes registers -> LDS in groups of 3 taps, double buffered (one barrier per
// group: 9 per chunk).
// History: tools/exp/split_*.hip (inner product 400 TF fp32-equivalent; whole layer 779 us vs 1973 us of the fp32
// kernel with statistics at B=32, 64->64, r=32).
#include "conv3d_split_kernel.h"

namespace {

// w f32[Cout][Cin][27] -> wp u16[Cin/16][27][piece][k-half][Cout][8]   (ci = chunk*16 + half*8 + j)
// pack: cuts w * 2^ew (split_ops.h: split_wmax_kernel left max |w| in the tail; split_tail_scale completes it).
__global__ void split_pack_kernel(const float *__restrict__ w, int Cout, int Cin, unsigned short *__restrict__ wp,
                                  unsigned *__restrict__ tail) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int ew = split_tail_scale(tail, i == 0);
  if (i >= Cout * Cin * 27) return;
  const int t = i % 27, c = (i / 27) % Cin, co = i / (27 * Cin), chunk = c / KS, g = (c % KS) / 8, j = c % 8;
  unsigned short hi, lo;
  cut(w[i] * pow2f(ew), hi, lo);
  const size_t base = ((size_t)chunk * 27 + t) * 4;
  wp[((base + 0 + g) * Cout + co) * 8 + j] = hi;
  wp[((base + 2 + g) * Cout + co) * 8 + j] = lo;
}

// ---- r = 8: the pipelined form -------------------------------------------------------------------------------------
// A sample has only 512 voxels, so B * Cout / 32 half-sample tiles (256 voxels x 32 channels) are all the work there is:
// ONE workgroup per CU at B = 32, Cout = 128, nothing else resident to hide its latencies behind.  The tile therefore
// pipelines itself:
//   * operand planes double buffered: the global loads of chunk q+1 are issued in front of the 27 taps of chunk q and
//     land in registers while the MFMAs run; they are activated, scaled, cut and written to the other plane buffer
//     behind the taps (one barrier for the chunk maximum);
//   * weight slices by LDS-DMA in groups of 9 taps (one kd plane: 18 KiB), ring of three groups, issued TWO groups
//     (108 MFMAs per wave) ahead; waited for with a counted s_waitcnt (memory operations retire in order; the counts
//     below are the operations this wave is known to have issued behind the awaited DMA -- at least DMA_MIN weight
//     instructions per group and the NLOAD operand loads -- so they can only be too strict, never too lax);
//   * fragments of tap t+1 are read from LDS in front of the MFMAs of tap t.
// Two facts measured in round 2 shape the workgroup (tools/exp/lds_b128_probe.hip, s_memtime): ONE wave reads LDS at
// 32 B/clk and issues a 32x32x16 MFMA every ~64 cycles, whatever else the CU does -- four waves x (32 channels x 64
// voxels: 6 fragment reads per 6 MFMAs) sit on both limits (taps: 331 cycles per tap round for 192 of MFMA).  So the
// default is EIGHT waves (two per SIMD) x one column block: 4 reads per 3 MFMAs and wave, 255 B/clk of LDS with the
// conflict-free row order below, 54 -> 48 us at 128 -> 128, B = 32.  (Only that form is built: the quad staging below
// static_asserts NW == 8, and the 4-wave geometry survives in the index arithmetic alone.)
// Voxel -> lane: a column block of 32 voxels is 8 w x 4 halo rows chosen so that a 32-lane group of a ds_read_b128
// touches every 16-byte slot of the 512-byte LDS window once: rows {h, h+2, h+4, h+6} at row stride 12 (8 waves), rows
// {h, h+4, h+1, h+5} at stride 10 (4 waves: conflict free in 16-lane groups at the 128 B/clk four waves can draw).
// Dense only (the sparse plan starts at r = 16), prologue and statistics as conv3d_split_kernel, no delta mode.
template <bool PRO, bool STATS, int NW>
__global__ __launch_bounds__(64 * NW, 1) void conv3d_split_pipe_kernel(const float *__restrict__ x, const u4 *__restrict__ wp,
                                                                  const float *__restrict__ wtail,
                                                                  const float *__restrict__ bias, float *__restrict__ y,
                                                                  int Cin, int Cout, const float *__restrict__ pro_a,
                                                                  const float *__restrict__ pro_b,
                                                                  float *__restrict__ stats) {
  // NW = 4 waves x 2 column blocks or NW = 8 waves x 1 (two waves per SIMD: see the comment above).  Halo row stride HW:
  // 10 for NW = 4 (block rows {h, h+4, h+1, h+5}), 12 for NW = 8 (block rows {h, h+2, h+4, h+6}: 24 / 48 / 72 = 24, 16, 8
  // mod 32 -- the four rows of a 32-lane group fall into four different quarters of the 512-byte LDS window)
  constexpr int r = 8, r3 = 512, TD = 4, TH = 8, TW = 8, VB = 8 / NW, COT = 32, TM = 64 * NW;
  static_assert(NW == 4 || NW == 8, "4 waves x 2 column blocks or 8 waves x 1");
  constexpr int HD = TD + 2, HH = TH + 2, HW = NW == 8 ? TW + 4 : TW + 2, HALO = HD * HH * HW; // 600 / 720
  constexpr int HP = (HALO + 63) / 64 * 64;                                 // 640 / 768
  constexpr int WPL = 4 * COT, TG = 9, NG = 27 / TG;                        // 128 u4 per tap slice; groups of 9 taps
  constexpr int DMA_PER_GROUP = TG * WPL / 64, DMA_MIN = DMA_PER_GROUP / NW; // 18 wave instructions over the waves
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u4 *sx = reinterpret_cast<u4 *>(smem);      // [2][piece][half][HP]
  u4 *sw = sx + 2 * 4 * HP;                   // [3][TG][piece][half][COT]
  float *sbias = reinterpret_cast<float *>(sw + 3 * TG * WPL);
  const int npro = PRO ? ((Cin + 63) & ~63) : 0;
  float *spa = sbias + COT, *spb = spa + npro;
  float *sred = spb + npro;                   // [NW][COT][2]
  __shared__ unsigned s_max[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 5, l32 = lane & 31;
  const int b = blockIdx.x, tile = blockIdx.y, co0 = blockIdx.z * COT, d0 = tile * TD;
  const float wscale_inv = wtail[2];
  if (PRO)
    for (int c = tid; c < Cin; c += TM) { spa[c] = pro_a[(size_t)b * Cin + c]; spb[c] = pro_b[(size_t)b * Cin + c]; }
  if (tid < COT) sbias[tid] = bias ? bias[co0 + tid] : 0.f;
  if (tid < 2) s_max[tid] = 0u;
  int E = 127;
  // @phase-init

  // Staging by aligned 16-byte row loads (round 3, as conv3d_split_kernel).  At r = 8 the tile spans the whole (h, w)
  // plane: its halo in h and w lies outside the grid -- always zero -- so only the 6 x 8 rows x 2 quads of real voxels
  // move at all (the planes' halo slots are zeroed once, below).  Thread t < 384 owns (k-half ig, 4 of its 8 channels,
  // row, quad): 4 dwordx4 loads, 16 values, 4 positions x 2 pieces x 8 bytes of LDS; threads 384 .. 511 issue the same
  // number of (out-of-range, zero) loads so that the counted vmcnt waits below stay uniform.
  static_assert(NW == 8, "the quad staging is laid out for 512 threads");
  constexpr int NLOAD = 4;
  const int st_ig = tid / 192, st_u = tid % 192, st_ch4 = st_u / 96, st_rq = st_u % 96;
  const int st_row = st_rq >> 1, st_quad = st_rq & 1, st_hd = st_row >> 3, st_gh = st_row & 7;
  const int st_gd = d0 - 1 + st_hd;
  const bool gok = tid < 384 && st_gd >= 0 && st_gd < r;
  const int goff = gok ? ((st_gd * r + st_gh) * r + st_quad * 4) * 4 + (st_ig * 8 + st_ch4 * 4) * r3 * 4 : 0x7fffff00;
  // byte offset of (position of voxel 0 of the quad, this thread's 8-byte channel half) inside a [piece][half] plane pair
  const int st_pos = (st_hd * HH + st_gh + 1) * HW + st_quad * 4 + 1;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(x + (size_t)b * Cin * r3), 0, Cin * r3 * 4, 0x00020000);
  // this lane's voxel in column block vbk = wave * VB + vb: d = vbk / 2, w = l % 8,
  // h = 2 (vbk % 2) + {0, 4, 1, 5}[l / 8] (NW = 4) or (vbk % 2) + {0, 2, 4, 6}[l / 8] (NW = 8)
  int xbase[VB], vox[VB];
#pragma unroll
  for (int vb = 0; vb < VB; ++vb) {
    const int vbk = wave * VB + vb;
    const int d = vbk >> 1, w = l32 & 7;
    const int h = NW == 8 ? (vbk & 1) + 2 * (l32 >> 3) : (vbk & 1) * 2 + ((l32 >> 4) & 1) + 4 * ((l32 >> 3) & 1);
    xbase[vb] = (d * HH + h) * HW + w;
    vox[vb] = ((d0 + d) * r + h) * r + w;
  }
  f32x16 acc[VB], cor[VB], cor2[VB]; // cor += W_h X_l, cor2 += W_l X_h: no two consecutive MFMAs share an accumulator
#pragma unroll
  for (int vb = 0; vb < VB; ++vb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[vb][i] = cor[vb][i] = cor2[vb][i] = 0.f;

  const int nchunks = Cin / KS, ngroups = nchunks * NG;
  typedef __attribute__((address_space(3))) unsigned char lds_byte;
  const uint32_t sw_lds = (uint32_t)(uintptr_t)(lds_byte *)reinterpret_cast<unsigned char *>(sw);
  auto weights_dma = [&](int sg) { // group sg (chunk sg / 3, taps 9 (sg % 3) ..) -> ring slot sg % 3
    const u4 *src = wp + (size_t)sg * TG * 4 * Cout + co0;
    const uint32_t dst0 = sw_lds + (uint32_t)((sg % 3) * TG * WPL * 16);
    for (int i = wave; i < DMA_PER_GROUP; i += NW) { // instruction i: tap i / 2, planes 2 (i % 2) + {0, 1}, 32 channels each
      const u4 *gp = src + (size_t)((i >> 1) * 4 + (i & 1) * 2 + g) * Cout + l32;
      const uint32_t dst = __builtin_amdgcn_readfirstlane(dst0 + (uint32_t)(i * 1024));
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(gp), "s"(dst) : "memory");
    }
  };
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 v[NLOAD];
  auto issue_loads = [&](int q) { // the operand loads of a chunk, unconditionally (outside the grid: offset past the end -> 0)
#pragma unroll
    for (int j = 0; j < NLOAD; ++j)
      v[j] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(xrs, goff, (q * KS + j) * r3 * 4, 0));
  };
  auto stage = [&](int q) { // registers -> activated, scaled, cut -> plane buffer q & 1 (contains the chunk-maximum barrier)
    unsigned mloc = 0u;
    if (PRO) {
      const int c0 = q * KS + st_ig * 8 + st_ch4 * 4;
      const float4 a4 = *reinterpret_cast<const float4 *>(spa + (tid < 384 ? c0 : 0));
      const float4 b4 = *reinterpret_cast<const float4 *>(spb + (tid < 384 ? c0 : 0));
      const float pa[4] = {a4.x, a4.y, a4.z, a4.w}, pb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int j = 0; j < NLOAD; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float act = pro_act(v[j][k], pa[j], pb[j]);
          v[j][k] = gok ? act : 0.f;
        }
    }
#pragma unroll
    for (int j = 0; j < NLOAD; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned a = __float_as_uint(v[j][k]) & 0x7fffffffu;
        mloc = (a > mloc && a <= 0x7f7fffffu) ? a : mloc;
      }
    mloc = wave_max_u32_lane63(mloc);
    if (lane == 63 && mloc) atomicMax(&s_max[q & 1], mloc);
    __syncthreads(); // the chunk's maximum is complete
    const unsigned mbits = s_max[q & 1];
    if (tid == 0) s_max[(q + 1) & 1] = 0u; // last read behind the previous chunk's maximum barrier
    if (mbits) {
      const int e = scale_exp(__uint_as_float(mbits));
      if (e < E) {
        if (E != 127) {
          const float f = pow2f(max(e - CONV_SPLIT_HEADROOM - E, -126));
#pragma unroll
          for (int vb = 0; vb < VB; ++vb)
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc[vb][i] *= f; cor[vb][i] *= f; cor2[vb][i] *= f; }
        }
        E = e - CONV_SPLIT_HEADROOM;
      }
    }
    const float xs = E == 127 ? 1.0f : pow2f(E);
    if (tid < 384) {
      uint2 *dst2 = reinterpret_cast<uint2 *>(sx + (q & 1) * 4 * HP);
#pragma unroll
      for (int k = 0; k < 4; ++k) { // voxel k of the quad: this thread's 4 channels = 8 bytes of the position's u4
        unsigned h0, l0, h1, l1;
        cut2(v[0][k] * xs, v[1][k] * xs, h0, l0);
        cut2(v[2][k] * xs, v[3][k] * xs, h1, l1);
        dst2[((0 + st_ig) * HP + st_pos + k) * 2 + st_ch4] = make_uint2(h0, h1);
        dst2[((2 + st_ig) * HP + st_pos + k) * 2 + st_ch4] = make_uint2(l0, l1);
      }
    }
  };

  // the halo slots (and the row-stride padding) of both plane buffers are never written again: zero everything once
  for (int e = tid; e < 2 * 4 * HP; e += TM) sx[e] = u4{0u, 0u, 0u, 0u};
  weights_dma(0);
  if (ngroups > 1) weights_dma(1);
  issue_loads(0);
  __syncthreads(); // prologue scalars, s_max = 0
  stage(0);
  // @phase 0
  for (int q = 0; q < nchunks; ++q) {
    const u4 *sxq = sx + (q & 1) * 4 * HP;
    const bool more = q + 1 < nchunks;
#pragma unroll
    for (int grp = 0; grp < NG; ++grp) {
      const int sg = q * NG + grp;
      // group sg's slices must have landed.  Issued behind them by this wave, in order: [grp 0] the DMA of group sg + 1;
      // [grp 1, 2] the DMA of group sg + 1 and this chunk's operand prefetch (when there is a next chunk)
      const bool dma_behind = sg + 1 < ngroups;
      if (grp == 0 || !more) { if (dma_behind) wait_vm<DMA_MIN>(); else wait_vm<0>(); }
      else { if (dma_behind) wait_vm<DMA_MIN + NLOAD>(); else wait_vm<NLOAD>(); }
      // @phase 1
      __syncthreads(); // slices of group sg and (grp 0) the planes of chunk q visible; ring slot of group sg - 1 free
      // @phase 5
      if (sg + 2 < ngroups) weights_dma(sg + 2);
      if (grp == 0 && more) issue_loads(q + 1);
      const u4 *swg = sw + (sg % 3) * TG * WPL;
      u4 wf[2][2], xf[2][VB][2];
      auto frags = [&](int t, int s_) {
        const int tap = grp * TG + t;
        const int toff = ((tap / 9) * HH + (tap / 3) % 3) * HW + tap % 3;
#pragma unroll
        for (int pc = 0; pc < 2; ++pc) {
          wf[s_][pc] = swg[t * WPL + (pc * 2 + g) * COT + l32];
#pragma unroll
          for (int vb = 0; vb < VB; ++vb) xf[s_][vb][pc] = sxq[(pc * 2 + g) * HP + xbase[vb] + toff];
        }
      };
      frags(0, 0);
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        if (t + 1 < TG) frags(t + 1, (t + 1) & 1);
        __builtin_amdgcn_sched_barrier(0); // keep the reads of tap t + 1 in front of the MFMAs of tap t (one wave per SIMD:
#pragma unroll                             // nothing else hides the LDS latency)
        for (int vb = 0; vb < VB; ++vb) {
          acc[vb] = mma(wf[t & 1][0], xf[t & 1][vb][0], acc[vb]);
          cor[vb] = mma(wf[t & 1][0], xf[t & 1][vb][1], cor[vb]);
          cor2[vb] = mma(wf[t & 1][1], xf[t & 1][vb][0], cor2[vb]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // @phase 6
    }
    if (more) stage(q + 1); // plane buffer (q + 1) & 1: last read by the taps of chunk q - 1, two barriers ago
    // @phase 4
  }

  float *yb = y + ((size_t)b * Cout + co0) * r3;
  const float us_x = E == 127 ? 1.0f : pow2f(-E), us_w = wscale_inv;
#pragma unroll
  for (int vb = 0; vb < VB; ++vb)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int co = (i & 3) + 8 * (i >> 2) + 4 * g;
      const float o = ((acc[vb][i] + (cor[vb][i] + cor2[vb][i]) * (1.f / 2048.f)) * us_x) * us_w + sbias[co];
      acc[vb][i] = o;
      yb[(size_t)co * r3 + vox[vb]] = o;
    }
  if (STATS) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float s1 = acc[0][i], s2 = acc[0][i] * acc[0][i];
#pragma unroll
      for (int vb = 1; vb < VB; ++vb) { s1 += acc[vb][i]; s2 += acc[vb][i] * acc[vb][i]; }
      s1 = row16_sum_rn(s1); s2 = row16_sum_rn(s2);
      s1 = row_pair_sum_odd_rows(s1); s2 = row_pair_sum_odd_rows(s2);
      if (l32 == 16) { // the row pair's sum lives in the odd rows
        const int co = (i & 3) + 8 * (i >> 2) + 4 * g;
        sred[(wave * COT + co) * 2] = s1;
        sred[(wave * COT + co) * 2 + 1] = s2;
      }
    }
    __syncthreads();
    if (tid < COT) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) { s1 += sred[(w * COT + tid) * 2]; s2 += sred[(w * COT + tid) * 2 + 1]; }
      float *o = stats + (((size_t)b * Cout + co0 + tid) * (r / TD) + tile) * 2;
      o[0] = s1;
      o[1] = s2;
    }
  }
  // @phase 7
  // @phase-flush
}

template <int NW>
static int launch_split_pipe(const float *x, const u4 *wp, const float *wtail, const float *bias, float *y, int B, int Cin,
                             int Cout, const float *pa, const float *pb, float *stats, hipStream_t st) {
  constexpr int HP = NW == 8 ? 768 : 640, COT = 32;
  const dim3 grid(B, 2, Cout / COT);
  const size_t LDS = (size_t)(2 * 4 * HP + 3 * 9 * 4 * COT) * 16 +
                     (size_t)(COT + (pa ? 2 * ((Cin + 63) & ~63) : 0) + NW * COT * 2) * 4;
  return lion_with_flags(pa != nullptr, stats != nullptr, [&](auto PRO, auto ST) {
    return lion_launch<conv3d_split_pipe_kernel<decltype(PRO)::value, decltype(ST)::value, NW>>(
        grid, 64 * NW, LDS, st, x, wp, wtail, bias, y, Cin, Cout, pa, pb, stats);
  });
}

} // namespace

extern "C" {

// number of uint16 in the packed weights: the pieces (split_piece_halfs) + an 8-halfword tail
// {max |w| bits, ew, 2^-ew, 0} (the tensor's power-of-two scale)
size_t lion_conv3d_split_packed_halfs(int Cout, int Cin) { return split_piece_halfs(Cout, Cin) + 8; }

int lion_conv3d_split_pack_weights(const float *w, int Cout, int Cin, uint16_t *wp, lionStream_t stream) {
  if (!w || !wp || Cout <= 0 || Cin <= 0) return LION_EINVAL;
  if (Cin % KS != 0 || (((uintptr_t)wp) & 15) != 0) return LION_EUNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned *tail = reinterpret_cast<unsigned *>(wp + split_piece_halfs(Cout, Cin));
  const int n = Cout * Cin * 27;
  if (hipMemsetAsync(tail, 0, 16, st) != hipSuccess) return LION_EINVAL;
  if (int e = lion_launch<split_wmax_kernel>(min(lion_cdiv(n, 2048), 128), 256, 0, st, w, n, tail)) return e;
  return lion_launch<split_pack_kernel>(lion_cdiv(n, 256), 256, 0, st, w, Cout, Cin, wp, tail);
}

// @phase-reader

int lion_conv3d_split_stat_tiles(int r, int Cout) {
  if (r != 8 && r != 16 && r != 32) return 0;
  // r = 8: the pipelined half-sample kernel (conv3d_split_pipe_kernel): 2 tiles of 256 voxels, 32 channels per workgroup
  // (history: 128-voxel tiles 144 us, whole-sample tiles x 32 channels on B * Cout/32 = 128 workgroups 104-108 us at
  // 128->128, B=32, against 114 us of the fp32 kernel); r = 16 / 32: the 256-voxel tiles of split_tile_forward
  return r == 8 ? 2 : conv_tile256_count(r);
}

// Arguments exactly as lion_conv3d_k3_fused_forward (include/lion_hip.h), wp from lion_conv3d_split_pack_weights;
// stats has lion_conv3d_split_stat_tiles(r, Cout) tiles; occ from lion_conv3d_tile_occupancy (same tile geometry:
// 4 waves x 2 column blocks of 32 voxels, the fp32 kernel's sparse plan).
int lion_conv3d_k3_split_forward(const float *x, const uint16_t *wp, const float *bias, int B, int Cin, int Cout,
                                 int r, const float *pro_a, const float *pro_b, const float *pro_bias,
                                 const float *tconst, float *y, float *stats, int32_t *occ, lionStream_t stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int e = split_tile_forward<2>(x, wp, bias, B, Cin, Cout, r, pro_a, pro_b, pro_bias, tconst, y, stats, occ, st);
  if (e != LION_SPLIT_NO_TILE) return e;
  // r = 8: the pipelined half-sample kernel, which has no work queue and no constant + delta form
  if (r != 8 || Cin % KS != 0 || (pro_a && Cin > 256) || Cout % 32 != 0 || occ || tconst) return LION_EUNSUPPORTED;
  return launch_split_pipe<8>(x, reinterpret_cast<const u4 *>(wp),
                              reinterpret_cast<const float *>(wp + split_piece_halfs(Cout, Cin)), bias, y, B, Cin, Cout,
                              pro_a, pro_b, stats, st);
}

} // extern "C"
