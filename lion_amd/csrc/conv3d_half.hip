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
// Same contract and modes as conv3d_split.hip::conv3d_split_kernel at r = 16 / 32 -- AdaGN+Swish prologue (PRO), GroupNorm
// tile sums (STATS), work queue + per-wave occupancy masks (occ), constant + delta (tconst), the consumer-aware levels --
// and the same tile geometry, so the occupancy buffers and the statistics' tile count (lion_conv3d_split_stat_tiles) apply
// unchanged.  The weights are the hi pieces of the SPLIT pack ([Cin/16][27][piece][k-half][Cout][8], piece 0): the first
// half of every tap slice is fetched, there is no packer of its own.  r = 8 stays on the three-product kernel.
//
// The body is a copy of conv3d_split_kernel's and not a shared header: that kernel sits at the 256-register limit and its
// register allocation, DMA placement and spill sites are pinned instruction by instruction (tests/test_isa_cpu.py); the
// reasons for the shape of every phase below (quad staging, per-chunk opaque addresses, builtin DMA, fragment double
// buffering, two-pass epilogue) are written down there and are not repeated here.
#include "split_ops.h"

namespace {

template <int N> struct IntC { static constexpr int value = N; };

// the hi pieces of a pair: the conversion of split_ops.h::cut2, bit for bit (v_cvt_pk_f16_f32, round to nearest even)
__device__ __forceinline__ unsigned hi2(float a, float b) {
  typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
  typedef float f2_t __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f2_t{a, b}, h2_t));
}

template <int TD, int TH, int TW, int CB, int VB, bool PRO, bool STATS, int OCC>
__global__ __launch_bounds__(256, OCC) void conv3d_half_kernel(const float *__restrict__ x, const u4 *__restrict__ wp,
                                                             const float *__restrict__ wtail,
                                                             const float *__restrict__ bias, float *__restrict__ y,
                                                             int Cin, int Cout, int r,
                                                             const float *__restrict__ pro_a,
                                                             const float *__restrict__ pro_b,
                                                             const float *__restrict__ pro_bias,
                                                             const float *__restrict__ tconst,
                                                             float *__restrict__ stats, int32_t *__restrict__ occ,
                                                             int B, int ntiles) {
  constexpr int TM = 256, COT = 32 * CB;
  static_assert(TD * TH * TW == 4 * VB * 32, "tile voxels = 4 waves x VB column blocks x 32");
  constexpr int HD = TD + 2, HH = TH + 2, HW = TW + 2, HALO = HD * HH * HW;
  constexpr int HP = (HALO + 63) / 64 * 64;   // plane stride: whole waves
  constexpr int WPL = 2 * COT;                // u4 per weight slice: the hi piece of one tap of one chunk, this channel tile
  constexpr int TG = 3;                       // taps per barrier
  static_assert(WPL <= TM && WPL % 64 == 0, "one u4 of a tap's weight slice per thread, whole waves");
  static_assert(27 % TG == 0, "whole groups per chunk");
  static_assert(27 * COT * 4 <= 2 * HP * 16, "the response table must fit the operand planes");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u4 *sx = reinterpret_cast<u4 *>(smem);      // [half][HP]
  u4 *sw = sx + 2 * HP;                       // [2][TG taps][half][COT]
  float *sbias = reinterpret_cast<float *>(sw + 2 * TG * WPL); // [COT]
  const int npro = PRO ? ((Cin + 63) & ~63) : 0;
  float *spa = sbias + COT, *spb = spa + npro, *spc = spb + npro; // prologue scalars / activated constant per channel
  float *sred = spc + npro;                   // [4][COT][2]
  float *sT = reinterpret_cast<float *>(sx);  // [27][COT] constant response (delta mode), loaded after the K loop
  __shared__ int s_work;
  __shared__ unsigned s_max[2];               // bits of the chunk's max |activation| (double buffered over chunks)
  __shared__ unsigned char s_rowok[256];      // aware level 2, delta launches: this staging thread's halo row has been written
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 5, l32 = lane & 31;
  const float wscale_inv = wtail[2]; // 2^-ew of the packed weights
  const bool queued = occ != nullptr;
  const int ncz = Cout / COT;
  const int n_tile_items = ntiles * B * ncz;
  const int aware_level = queued ? occ[2 * B * ntiles + 2] : 0;
  const bool aware = aware_level != 0;
  for (int iter = 0;; ++iter) {
  int b, tile, co0;
  if (queued) { // occ = [B*tiles wave masks][B*tiles list, occupied tiles first][queue counter, exit counter, aware level]
    __syncthreads();
    if (tid == 0) s_work = atomicAdd(occ + 2 * B * ntiles, 1);
    __syncthreads();
    const int work = s_work;
    if (work >= n_tile_items) break;
    const int item = work / ncz;
    b = item % B;
    tile = occ[B * ntiles + b * ntiles + item / B];
    co0 = (work % ncz) * COT;
  } else {
    if (iter) break;
    b = blockIdx.x;
    tile = blockIdx.y;
    co0 = blockIdx.z * COT;
  }
  const int ntw = r / TW, nth = r / TH;
  const int d0 = (tile / (ntw * nth)) * TD, h0 = ((tile / ntw) % nth) * TH, w0 = (tile % ntw) * TW;
  const int r3 = r * r * r;
  int n_act = 4 * VB * 32;
  int wmask = 0xf;
  if (queued) { // bit w of the tile's flag = wave w's 64-voxel block sees a point; bit 8 = has a reader
    const int fw = occ[b * ntiles + tile];
    wmask = fw & 0xf;
    n_act = wmask ? 4 * VB * 32 : 0;
    if (aware && fw == 0) {
      // an empty tile without a reader: nothing is stored, its GroupNorm sums follow in closed form (conv3d_split.hip)
      if (STATS && tid < COT) {
        const bool dl = PRO && pro_a != nullptr && tconst != nullptr;
        const int nd[3] = {d0 == 0 ? 1 : 0, TD - (d0 == 0 ? 1 : 0) - (d0 + TD == r ? 1 : 0), d0 + TD == r ? 1 : 0};
        const int nh[3] = {h0 == 0 ? 1 : 0, TH - (h0 == 0 ? 1 : 0) - (h0 + TH == r ? 1 : 0), h0 + TH == r ? 1 : 0};
        const int nw[3] = {w0 == 0 ? 1 : 0, TW - (w0 == 0 ? 1 : 0) - (w0 + TW == r ? 1 : 0), w0 + TW == r ? 1 : 0};
        float s1 = 0.f, s2 = 0.f;
        if (dl) {
#pragma unroll
          for (int cfg = 0; cfg < 27; ++cfg) {
            const float n = (float)(nd[cfg / 9] * nh[(cfg / 3) % 3] * nw[cfg % 3]);
            const float tv = tconst[((size_t)b * 27 + cfg) * Cout + co0 + tid];
            s1 += n * tv;
            s2 += n * (tv * tv);
          }
        } else {
          const float tv = bias ? bias[co0 + tid] : 0.f;
          s1 = (float)(TD * TH * TW) * tv;
          s2 = (float)(TD * TH * TW) * (tv * tv);
        }
        float *o = stats + (((size_t)b * Cout + co0 + tid) * ntiles + tile) * 2;
        o[0] = s1;
        o[1] = s2;
      }
      continue;
    }
  }
  n_act = __builtin_amdgcn_readfirstlane(n_act);
  const bool my_work = (wmask >> wave) & 1; // this wave runs the taps on all of its column blocks, or on none
  const bool pro_on = PRO && pro_a != nullptr;
  const bool delta = pro_on && tconst != nullptr;
  if (pro_on) {
    for (int c = tid; c < Cin; c += TM) {
      const float pa = pro_a[(size_t)b * Cin + c], pb = pro_b[(size_t)b * Cin + c];
      spa[c] = pa;
      spb[c] = pb;
      spc[c] = delta ? pro_act(pro_bias ? pro_bias[c] : 0.f, pa, pb) : 0.f;
    }
  }
  for (int c = tid; c < COT; c += TM) sbias[c] = bias ? bias[co0 + c] : 0.f;
  if (tid < 2) s_max[tid] = 0u;
  // aware level 2: the producer of x stored its occupied (margin-1) tiles only; the staged value is exactly zero in the
  // others, so their halo rows are not loaded (bit 9 of the flag words = occupied at margin 1)
  const bool rows_masked = delta && aware_level == 2;
  if (rows_masked) {
    constexpr int QR_ = (TW + 8) / 4, HH_ = TH + 2, HD_ = TD + 2;
    const int row = tid / QR_, hd = row / HH_, hh = row - hd * HH_;
    const int gd = d0 - 1 + hd, gh = h0 - 1 + hh;
    bool ok = tid < HD_ * HH_ * QR_ && gd >= 0 && gd < r && gh >= 0 && gh < r;
    if (ok) ok = (occ[b * ntiles + (gd / TD) * (r / TH) + gh / TH] >> 9) & 1;
    s_rowok[tid] = ok;
  }
  int E = 127; // exponent of the tile's activation scale 2^E; 127 = none yet (everything staged so far was zero)

  // quads outside the grid carry an offset beyond num_records, for which buffer loads return 0
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(x + (size_t)b * Cin * r3), 0, Cin * r3 * 4, 0x00020000);

  f32x16 acc[CB][VB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int vb = 0; vb < VB; ++vb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[cb][vb][i] = 0.f;

  const bool empty = n_act == 0;
  const int nchunks = empty ? 0 : Cin / KS;
  // this thread's u4 of a weight slice: element (k-half, co) of the tile <- piece 0 of the pack, [k-half][Cout] at co0 + co
  const int we_g = (tid / COT) * Cout + co0 + (tid % COT);
  const bool w_thread = tid < WPL;
  typedef __attribute__((address_space(3))) unsigned char lds_byte;
  const uint32_t sw_lds0 = (uint32_t)(uintptr_t)(lds_byte *)reinterpret_cast<unsigned char *>(sw);
  const uint32_t sw_lds = sw_lds0 + (uint32_t)wave * 1024u;
  const uint32_t sx_lds = (uint32_t)(uintptr_t)(lds_byte *)reinterpret_cast<unsigned char *>(sx);
  auto weights_dma = [&](int sg) { // group sg of the K walk (chunk sg / 9, taps (sg % 9) * TG ..) -> buffer sg & 1
    if (w_thread) {                // wave uniform: WPL is a multiple of 64
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        // the builtin, not inline asm: the compiler must count the DMA among the VM operations in flight
        const u4 *gp = wp + ((size_t)sg * TG + t) * 4 * Cout + we_g; // 4 Cout u4 per tap in HBM, of which the first 2 Cout
        typedef __attribute__((address_space(3))) void lds_void;
        typedef __attribute__((address_space(1))) const void glb_void;
        lds_void *dstp = (lds_void *)(uintptr_t)__builtin_amdgcn_readfirstlane(sw_lds + (uint32_t)(((sg & 1) * TG + t) * WPL * 16));
        __builtin_amdgcn_global_load_lds((glb_void *)gp, dstp, 16, 0, 0);
      }
    }
  };
  if (nchunks) { weights_dma(0); weights_dma(1); } // nchunks >= 1 -> at least 9 groups
  // One chunk of the K walk; WORK = false is the copy run by a wave whose block sees no point: it stages and takes part in
  // every barrier and in the weight DMA, but owns no MFMA.  Two separate loops, the branch outside them.
  auto chunk = [&](int q, auto work_c) {
    constexpr bool WORK = decltype(work_c)::value != 0;
    constexpr int NVB = WORK ? VB : 0;
    __syncthreads(); // the previous chunk's planes are no longer read (and the prologue scalars are visible)
    {
    // staging by aligned 16-byte row loads: thread rt owns one quad of a halo row for all 16 channels of the chunk
    constexpr int QR = (TW + 8) / 4, IPH = HD * HH * QR;
    static_assert(IPH <= TM, "one quad per thread");
    int rt = tid;
    asm volatile("" : "+v"(rt));
    const int row = rt / QR, qd = rt - row * QR;
    const int hd = row / HH, hh = row - hd * HH;
    const int gd = d0 - 1 + hd, gh = h0 - 1 + hh, gw0 = w0 - 4 + 4 * qd;
    const bool gok = rt < IPH && gd >= 0 && gd < r && gh >= 0 && gh < r && gw0 >= 0 && gw0 < r && (!rows_masked || s_rowok[rt]);
    const int goff = gok ? ((gd * r + gh) * r + gw0) * 4 : 0x7fffff00;
    const int p0 = row * HW + 4 * qd - 3; // halo position of the quad's first column (column k is used iff 0 <= hw0 + k < HW)
    const int hw0 = 4 * qd - 3;
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 v[2][8];
#pragma unroll
    for (int ig = 0; ig < 2; ++ig)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[ig][j] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(xrs, goff, (q * KS + ig * 8 + j) * r3 * 4, 0));
    unsigned mloc = 0u;
    if (pro_on) {
#pragma unroll
      for (int ig = 0; ig < 2; ++ig) {
        const int c0 = q * KS + ig * 8;
        const float4 a0 = *reinterpret_cast<const float4 *>(spa + c0), a1 = *reinterpret_cast<const float4 *>(spa + c0 + 4);
        const float4 b0 = *reinterpret_cast<const float4 *>(spb + c0), b1 = *reinterpret_cast<const float4 *>(spb + c0 + 4);
        const float4 c4 = *reinterpret_cast<const float4 *>(spc + c0), c5 = *reinterpret_cast<const float4 *>(spc + c0 + 4);
        const float pa8[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const float pb8[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
        const float pc8[8] = {c4.x, c4.y, c4.z, c4.w, c5.x, c5.y, c5.z, c5.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float act = pro_act(v[ig][j][k], pa8[j], pb8[j]) - pc8[j];
            v[ig][j][k] = gok ? act : 0.f;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool used = rt < IPH && hw0 + k >= 0 && hw0 + k < HW;
      unsigned mk = 0u;
#pragma unroll
      for (int ig = 0; ig < 2; ++ig)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const unsigned a = __float_as_uint(v[ig][j][k]) & 0x7fffffffu; // |t| as ordered bits; inf / nan do not set the scale
          mk = (a > mk && a <= 0x7f7fffffu) ? a : mk;
        }
      mloc = (used && mk > mloc) ? mk : mloc;
    }
    mloc = wave_max_u32_lane63(mloc);
    if (lane == 63 && mloc) atomicMax(&s_max[q & 1], mloc);
    __syncthreads(); // the chunk's maximum is complete
    const unsigned mbits = s_max[q & 1];
    if (tid == 0) s_max[(q + 1) & 1] = 0u; // its last readers passed the barrier at the top of this chunk
    if (mbits) {
      const int e = scale_exp(__uint_as_float(mbits));
      if (e < E) { // the tile's maximum grew: bring what has been accumulated onto the new (smaller) scale first
        if (WORK && E != 127) {
          const float f = pow2f(max(e - CONV_SPLIT_HEADROOM - E, -126));
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int vb = 0; vb < NVB; ++vb)
#pragma unroll
              for (int i = 0; i < 16; ++i) acc[cb][vb][i] *= f;
        }
        E = e - CONV_SPLIT_HEADROOM;
      }
    }
    const float xs = E == 127 ? 1.0f : pow2f(E);
#pragma unroll
    for (int ig = 0; ig < 2; ++ig)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        u4 ph;
#pragma unroll
        for (int m = 0; m < 4; ++m) ph[m] = hi2(v[ig][2 * m][k] * xs, v[ig][2 * m + 1][k] * xs);
        if (rt < IPH && hw0 + k >= 0 && hw0 + k < HW) sx[ig * HP + p0 + k] = ph;
      }
    }
    // The 27 taps.  Weight slices travel in groups of TG taps through two buffers (group k of chunk q = walk index
    // sg = 9 q + k, buffer sg & 1); barrier k sits in front of the LAST tap of group k.  Fragments are double buffered in
    // registers: the NVB + CB reads of tap t + 1 are spread over the CB NVB MFMA slots of tap t.
    {
      const int par = q & 1;
      typedef __attribute__((address_space(3))) const u4 lds_u4;
      uint32_t xq[NVB > 0 ? NVB : 1], wq2[2];
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const int g_ = ln >> 5, l32_ = ln & 31;
#pragma unroll
      for (int vb = 0; vb < NVB; ++vb) { // halo position of this lane's voxel in the wave's column block vb
        const int v = (wave * VB + vb) * 32 + l32_;
        const int d = v / (TH * TW), h = (v / TW) % TH, w = v % TW;
        xq[vb] = sx_lds + (uint32_t)((g_ * HP + (d * HH + h) * HW + w) * 16);
        asm volatile("" : "+v"(xq[vb]));
      }
      wq2[0] = sw_lds0 + (uint32_t)((par * TG * WPL + g_ * COT + l32_) * 16);
      wq2[1] = sw_lds0 + (uint32_t)(((par ^ 1) * TG * WPL + g_ * COT + l32_) * 16);
      asm volatile("" : "+v"(wq2[0]));
      asm volatile("" : "+v"(wq2[1]));
      constexpr int NX = NVB > 0 ? NVB : 1;
      u4 wf[2][CB], xf[2][NX];
      constexpr int NR = NVB + CB; // fragment reads per tap: X (NVB), then W (CB)
      auto frag = [&](int tap, int s_, int r_) {
        if (r_ < NVB) {
          const int toff = ((tap / 9) * HH + (tap / 3) % 3) * HW + tap % 3;
          xf[s_][r_] = *(lds_u4 *)(uintptr_t)(xq[r_] + (uint32_t)(toff * 16));
        } else {
          const int cb = r_ - NVB, k = tap / TG, t = tap % TG;
          wf[s_][cb] = *(lds_u4 *)(uintptr_t)(wq2[k & 1] + (uint32_t)((t * WPL + cb * 32) * 16));
        }
      };
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // group 9 q (requested two barriers ago / in the item prologue)
      __syncthreads(); // the chunk's operand planes and the first weight group are visible
      auto group_barrier = [&](int k) {
        const int sg = q * (27 / TG) + k;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // group sg + 1 has landed
        __syncthreads();
        if (sg + 2 < nchunks * (27 / TG)) weights_dma(sg + 2);
      };
      if constexpr (WORK) {
        __builtin_amdgcn_s_setprio(2); // while the wave owns MFMAs its issue wins against the co-resident staging VALU
#pragma unroll
        for (int r_ = 0; r_ < NR; ++r_) frag(0, 0, r_);
#pragma unroll
        for (int tap = 0; tap < 27; ++tap) {
          const int cur = tap & 1, nxt = cur ^ 1;
          if (tap % TG == TG - 1) group_barrier(tap / TG);
          constexpr int NM = CB * NX;                 // MFMA m of the tap: channel block m / NX, column block m % NX
          constexpr int PER = (NR + NM - 1) / NM;     // reads of tap + 1 in front of each MFMA slot
#pragma unroll
          for (int m = 0; m < NM; ++m) {
            if (tap + 1 < 27) {
#pragma unroll
              for (int r_ = m * PER; r_ < (m + 1) * PER && r_ < NR; ++r_) frag(tap + 1, nxt, r_);
            }
            const int cb = m / NX, vb = m % NX;
            acc[cb][vb] = mma(wf[cur][cb], xf[cur][vb], acc[cb][vb]);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        __builtin_amdgcn_s_setprio(0);
      } else {
#pragma unroll
        for (int k = 0; k < 27 / TG; ++k) group_barrier(k);
      }
    }
  };
  if (my_work) { for (int q = 0; q < nchunks; ++q) chunk(q, IntC<1>{}); }
  else { for (int q = 0; q < nchunks; ++q) chunk(q, IntC<0>{}); }

  if (delta) {
    __syncthreads(); // the last tap's LDS reads are done: the operand planes become the response table
    for (int e = tid; e < 27 * COT; e += TM) sT[e] = tconst[((size_t)b * 27 + e / COT) * Cout + co0 + e % COT];
    __syncthreads();
  } else if (empty) {
    __syncthreads(); // sbias was written by other threads and no barrier of the K loop ran
  }
  // epilogue: D = main * 2^-(E + ew) (+ bias | constant response), NCDHW store; two passes (values, then nothing but stores).
  // acc register i of lane l: channel row (i&3) + 8*(i>>2) + 4*(l>>5), voxel column l&31.
  float *yb = y + ((size_t)b * Cout + co0) * r3;
  const float us_x = E == 127 ? 1.0f : pow2f(-E), us_w = wscale_inv; // exact powers of two
  int gvv[VB];
#pragma unroll
  for (int vb = 0; vb < VB; ++vb) {
    const int v = (wave * VB + vb) * 32 + l32;
    const int d = v / (TH * TW), h = (v / TW) % TH, w = v % TW;
    const int gd = d0 + d, gh = h0 + h, gw = w0 + w;
    gvv[vb] = (gd * r + gh) * r + gw;
    const int cfg = (((gd == 0 ? 0 : gd == r - 1 ? 2 : 1) * 3 + (gh == 0 ? 0 : gh == r - 1 ? 2 : 1)) * 3 +
                     (gw == 0 ? 0 : gw == r - 1 ? 2 : 1));
    const float *addv = delta ? sT + cfg * COT : sbias;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = cb * 32 + (i & 3) + 8 * (i >> 2) + 4 * g;
        acc[cb][vb][i] = (acc[cb][vb][i] * us_x) * us_w + addv[co];
      }
  }
#pragma unroll
  for (int vb = 0; vb < VB; ++vb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = cb * 32 + (i & 3) + 8 * (i >> 2) + 4 * g;
        yb[(size_t)co * r3 + gvv[vb]] = acc[cb][vb][i];
      }
  if (STATS) { // per-tile channel sums, as csrc/conv3d.hip
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int vb = 0; vb < VB; ++vb) {
          const float o = acc[cb][vb][i];
          s1 += o;
          s2 += o * o;
        }
        s1 = row16_sum_rn(s1); s2 = row16_sum_rn(s2);
        s1 = row_pair_sum_odd_rows(s1); s2 = row_pair_sum_odd_rows(s2);
        if (l32 == 16) { // the row pair's sum lives in the odd rows
          const int co = cb * 32 + (i & 3) + 8 * (i >> 2) + 4 * g;
          sred[(wave * COT + co) * 2] = s1;
          sred[(wave * COT + co) * 2 + 1] = s2;
        }
      }
    __syncthreads();
    if (tid < COT) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) { s1 += sred[(w * COT + tid) * 2]; s2 += sred[(w * COT + tid) * 2 + 1]; }
      float *o = stats + (((size_t)b * Cout + co0 + tid) * ntiles + tile) * 2;
      o[0] = s1;
      o[1] = s2;
    }
  }
  } // work loop
  // the queue re-arms itself: the last workgroup to leave zeroes the queue and the exit counter
  if (queued && tid == 0) {
    int32_t *q = occ + 2 * B * ntiles;
    if (atomicAdd(q + 1, 1) == (int)gridDim.x - 1) { q[0] = 0; q[1] = 0; }
  }
}

template <int TD, int TH, int TW, int CB, int VB, int OCC>
static int launch_half_t(const float *x, const u4 *wp, const float *wtail, const float *bias, float *y, int B, int Cin,
                         int Cout, int r, const float *pa, const float *pb, const float *pbias, const float *tconst,
                         float *stats, int32_t *occ, hipStream_t st) {
  constexpr int COT = 32 * CB;
  constexpr int HALO = (TD + 2) * (TH + 2) * (TW + 2), HP = (HALO + 63) / 64 * 64;
  const int tiles = (r / TD) * (r / TH) * (r / TW);
  static int cu_count[LION_MAX_DEVICES] = {0};
  int dev = 0;
  if (int e = lion_current_device(&dev)) return e;
  if (!cu_count[dev]) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return LION_EINVAL;
    cu_count[dev] = prop.multiProcessorCount;
  }
  const long items = (long)B * tiles * (Cout / COT);
  const long resident = (long)OCC * cu_count[dev];
  const dim3 grid = occ ? dim3((unsigned)(items < resident ? items : resident)) : dim3(B, tiles, Cout / COT);
  const size_t LDS = (size_t)(2 * HP + 2 * 3 * 2 * COT) * 16 + // planes + two groups of 3 taps of hi weight slices
                     (size_t)(COT + (pa ? 3 * ((Cin + 63) & ~63) : 0) + 4 * COT * 2) * 4;
#define LION_HALF_GO(PRO_, ST_)                                                                              \
  {                                                                                                          \
    static LionLdsLimit cfg = {};                                                                            \
    if (int e = lion_dynamic_lds(&conv3d_half_kernel<TD, TH, TW, CB, VB, PRO_, ST_, OCC>, LDS, cfg)) return e;    \
    conv3d_half_kernel<TD, TH, TW, CB, VB, PRO_, ST_, OCC><<<grid, 256, LDS, st>>>(x, wp, wtail, bias, y, Cin, Cout, r, pa, pb, \
                                                                             pbias, tconst, stats, occ, B, tiles); \
  }
  if (pa && stats) LION_HALF_GO(true, true)
  else if (pa) LION_HALF_GO(true, false)
  else if (stats) LION_HALF_GO(false, true)
  else LION_HALF_GO(false, false)
#undef LION_HALF_GO
  LION_LAUNCH_CHECK();
  return 0;
}

} // namespace

extern "C" {

// Arguments exactly as lion_conv3d_k3_split_forward (include/lion_hip.h): wp from lion_conv3d_split_pack_weights (only its
// hi pieces and its scale are read), stats with lion_conv3d_split_stat_tiles(r, Cout) tiles, occ from
// lion_conv3d_tile_occupancy[_aware].
int lion_conv3d_k3_half_forward(const float *x, const uint16_t *wp, const float *bias, int B, int Cin, int Cout, int r,
                                const float *pro_a, const float *pro_b, const float *pro_bias, const float *tconst,
                                float *y, float *stats, int32_t *occ, lionStream_t stream) {
  if (!x || !wp || !y || B <= 0 || Cin <= 0 || Cout <= 0) return LION_EINVAL;
  if ((pro_a == nullptr) != (pro_b == nullptr)) return LION_EINVAL;
  if (tconst && !pro_a) return LION_EINVAL;
  if (occ && pro_a && !tconst) return LION_EINVAL;
  if ((r != 16 && r != 32) || Cin % KS != 0 || Cout % 32 != 0) return LION_EINVAL; // r = 8 stays on the three-product kernel
  if (pro_a && Cin > 256) return LION_EUNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const u4 *w4 = reinterpret_cast<const u4 *>(wp);
  const float *wtail = reinterpret_cast<const float *>(wp + (size_t)(Cin / KS) * 27 * 4 * Cout * 8);
  const int cb = Cout % 64 == 0 ? 2 : 1;
#define LION_HALF_TILE(R_, CB_, TD_, TH_, TW_, OCC_)                                                          \
  if (r == R_ && cb == CB_)                                                                                   \
    return launch_half_t<TD_, TH_, TW_, CB_, 2, OCC_>(x, w4, wtail, bias, y, B, Cin, Cout, r, pro_a, pro_b, pro_bias, tconst, \
                                                      stats, occ, st);
  LION_HALF_TILE(32, 2, 2, 4, 32, 2)
  LION_HALF_TILE(32, 1, 2, 4, 32, 2)
  LION_HALF_TILE(16, 2, 4, 4, 16, 2)
  LION_HALF_TILE(16, 1, 4, 4, 16, 2)
#undef LION_HALF_TILE
  return LION_EINVAL;
}

} // extern "C"
