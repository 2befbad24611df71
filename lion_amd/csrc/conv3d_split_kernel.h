// conv3d_split_kernel.h -- the tile kernel of the 3x3x3 voxel convolution on fp16 pieces (r = 16 / 32) and its launcher,
// one template for both precisions.  P = pieces per operand:
//   P = 2  csrc/conv3d_split.hip: hi and lo pieces, three products per operand pair, acc + cor / 2048 (fp32 accuracy);
//   P = 1  csrc/conv3d_half.hip:  the hi pieces only, one product, acc alone (the contract is written down there).
// Queue, aware levels, staging, prologue, block scale, weight ring, epilogue and statistics are the same text for both;
// P decides the LDS layout (2 P planes, 2 P COT u4 per weight slice), the cut, the fragments and MFMAs of a tap and the
// epilogue term.  Each translation unit instantiates its own P only.  tests/test_isa_cpu.py and
// tests/test_conv_half_isa_cpu.py pin the compiled code of either.
#pragma once
#include "conv3d_tiles.h"
#include "split_ops.h"

namespace {

// "// @phase N" comments mark the phase boundaries that tools/build_timing_lib.sh turns into s_memtime counters in an
// instrumented COPY of conv3d_split.hip with this header spliced in (0 item prologue, 1 waits at the chunk's two plane barriers, 2 load issue + wait + activate +
// max, 3 max barrier, 4 cut + LDS write, 5 wait for the next weight group + group barrier, 6 taps, 7 epilogue); the product build carries no instrumentation and no switches.

// Round-5 experiments on the sparse plan that were built, bit-exact, measured on one box inside the sampling step and NOT
// adopted live in tools/exp/conv3d_split_round5_experiments.hip (this kernel's file of then, with the switches LION_SPLIT_COMPACT /
// LION_SPLIT_FILL; build with tools/build_variant.sh NAME conv3d_split=tools/exp/conv3d_split_round5_experiments.hip:-D...):
//   * voxel compaction inside occupied tiles (active voxels packed into 32-column MFMA blocks, a one-block wave path):
//     sparse launches 8-11 % faster, dense ones 5-6 % slower (a third copy of the K walk costs the register allocation 40
//     bytes of scratch around the staging), step 6.84 -> 6.93 ms;
//   * a plane-fill kernel for empty tiles in front of the convolution: serialises 30-40 us per convolution, step 6.84 -> 7.05 ms
//     (as queue items inside this kernel it cost the dense layer 37 %).
// Evidence: profiles/r05a_conv_ab_variants_one_box.txt, r05a_conv_ab_r04_vs_fill_items_in_kernel.txt,
// r05b_conv_epilogue_phases.txt (where a launch's cycles go).  What was adopted instead is below: empty tiles nobody reads are
// not stored at all (aware levels), and the work queue re-arms itself.

template <int TD, int TH, int TW, int CB, int VB, bool PRO, bool STATS, int OCC, int P>
__global__ __launch_bounds__(256, OCC) void conv3d_split_kernel(const float *__restrict__ x, const u4 *__restrict__ wp,
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
  static_assert(P == 1 || P == 2, "pieces per operand: hi alone, or hi and lo");
  constexpr int HD = TD + 2, HH = TH + 2, HW = TW + 2, HALO = HD * HH * HW;
  constexpr int HP = (HALO + 63) / 64 * 64;   // plane stride: whole waves, so a staging wave never straddles two planes
  constexpr int WPL = 2 * P * COT;            // u4 per weight slice (one tap of one chunk, this channel tile; P = 1: its hi piece)
  constexpr int TG = 3;                       // taps per barrier: the weight slices of a (kd, kh) row of taps travel together
  static_assert(WPL <= TM && WPL % 64 == 0, "one u4 of a tap's weight slice per thread, whole waves");
  static_assert(27 % TG == 0, "whole groups per chunk");
  static_assert(27 * COT * 4 <= 2 * P * HP * 16, "the response table must fit the operand planes");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u4 *sx = reinterpret_cast<u4 *>(smem);      // [piece][half][HP]
  u4 *sw = sx + 2 * P * HP;                   // [2][TG taps][piece][half][COT]
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
  const float wscale_inv = wtail[2]; // 2^-ew of the packed weights (split_tail_scale)
  const bool queued = occ != nullptr;
  const int ncz = Cout / COT;
  const int n_tile_items = ntiles * B * ncz;
  // consumer-aware buffers (lion_conv3d_tile_occupancy_aware): empty tiles whose output nobody reads store nothing
  const int aware_level = queued ? occ[2 * B * ntiles + 2] : 0;
  const bool aware = aware_level != 0;
  // @phase-init
  for (int iter = 0;; ++iter) {
  int b, tile, co0;
  if (queued) { // see csrc/conv3d.hip: occ = [B*tiles wave masks][B*tiles list, occupied tiles first][queue counter]
    // (round 4: dealing the list round-robin to the resident workgroups instead -- no atomic, no dependent index load in
    // front of an item -- was measured and LOSES on every sparse launch: conv1 Gaussian clouds 395 -> 440 us, r = 16 flat
    // delta 171 -> 225 us, sampling step 6.82 -> 7.26 ms; dense 654 -> 648 us.  Items differ too much in cost -- wave
    // masks, empty tiles -- for a static deal; the queue's round trip is not what the in-step forms pay over the plain kernel.)
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
  // thread t owns voxel t of the tile ((d, h, w) order) for the bookkeeping of the sparse plan
  int n_act = 4 * VB * 32;
  int wmask = 0xf;
  if (queued) { // round-3 plan: bit w of the tile's flag = wave w's 64-voxel block sees a point; bit 8 = has a reader
    const int fw = occ[b * ntiles + tile];
    wmask = fw & 0xf;
    n_act = wmask ? 4 * VB * 32 : 0;
    if (aware && fw == 0) {
      // An empty tile WITHOUT A READER (conv_tile_occ_kernel (5)): no output is stored -- nobody stages or interpolates
      // from it -- only its GroupNorm sums are owed, in closed form: voxels per border configuration x the constant the
      // dense evaluation leaves there (bias, or the delta mode's constant response).  In the chain 73-80 % of the tiles of
      // an r = 32 launch are empty and most of them have no reader: 268 MB of constants per launch were written for nobody.
      if (STATS && tid < COT) {
        const bool dl = PRO && pro_a != nullptr && tconst != nullptr;
        const int nd[3] = {d0 == 0 ? 1 : 0, TD - (d0 == 0 ? 1 : 0) - (d0 + TD == r ? 1 : 0), d0 + TD == r ? 1 : 0};
        const int nh[3] = {h0 == 0 ? 1 : 0, TH - (h0 == 0 ? 1 : 0) - (h0 + TH == r ? 1 : 0), h0 + TH == r ? 1 : 0};
        const int nw[3] = {w0 == 0 ? 1 : 0, TW - (w0 == 0 ? 1 : 0) - (w0 + TW == r ? 1 : 0), w0 + TW == r ? 1 : 0};
        float s1 = 0.f, s2 = 0.f;
        if (dl) {
#pragma unroll
          for (int cfg = 0; cfg < 27; ++cfg) { // unrolled: constant indices keep the count arrays in registers
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
  const int my_nvb = ((wmask >> wave) & 1) ? VB : 0; // column blocks this wave runs the taps on: all of its own, or none
  const bool pro_on = PRO && pro_a != nullptr; // the PRO instantiation also serves launches without a prologue (see
  const bool delta = pro_on && tconst != nullptr; // launch_split_t: its register allocation is the better one)
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
  // Aware level 2 (lion_conv3d_tile_occupancy_aware): the producer of x stored its occupied (margin-1) tiles only.  Inside
  // its empty tiles x is bias1 exactly, so this launch's staged value -- the activation minus its constant -- is exactly
  // zero there: such halo rows are not loaded (their quads take the out-of-range offset, for which buffer loads return 0,
  // and the prologue writes 0 for them).  Bit 9 of this buffer's flag words = the tile is occupied at margin 1.
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

  // Everything derived from the thread index (the staging offsets, the fragment bases of the tap loop) is RECOMPUTED per
  // chunk from an opaque copy of it: computed once here it stays alive across the tap loop, where the allocator -- at the
  // 256-register limit -- spills exactly such long-lived values, and the reloads (scratch loads wait with vmcnt, memory
  // operations retire in order) then drain the operand loads they sit between.  Quads outside the grid carry an offset
  // beyond num_records, for which buffer loads return 0.
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(x + (size_t)b * Cin * r3), 0, Cin * r3 * 4, 0x00020000);

  f32x16 acc[CB][VB];
  [[maybe_unused]] f32x16 cor[CB][VB]; // the correction products: P = 2 only
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int vb = 0; vb < VB; ++vb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        acc[cb][vb][i] = 0.f;
        if constexpr (P == 2) cor[cb][vb][i] = 0.f;
      }

  const bool empty = n_act == 0;
  const int nchunks = empty ? 0 : Cin / KS;
  // this thread's u4 of a weight slice: element (pg, co) of the tile <- global [pg][Cout] at co0 + co
  const int we_g = (tid / COT) * Cout + co0 + (tid % COT);
  const bool w_thread = tid < WPL;
  // weight slices travel global -> LDS by LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave instruction lands at
  // M0 + lane * 16), one group of TG taps ahead of their use, into the buffer the group before last was read from.  No
  // registers and no VALU on the way: the register ring this replaces cost 12 VGPRs at the 256-register limit (87
  // spills), and the compiler was free to sink its loads next to their LDS writes (s_memtime phase counters: 29 % of a
  // wave's cycles went into waiting for them).  The DMA is issued right behind the group barrier and awaited (vmcnt 0)
  // in front of the next one.
  typedef __attribute__((address_space(3))) unsigned char lds_byte;
  const uint32_t sw_lds0 = (uint32_t)(uintptr_t)(lds_byte *)reinterpret_cast<unsigned char *>(sw);
  const uint32_t sw_lds = sw_lds0 + (uint32_t)wave * 1024u;
  const uint32_t sx_lds = (uint32_t)(uintptr_t)(lds_byte *)reinterpret_cast<unsigned char *>(sx);
  auto weights_dma = [&](int sg) { // group sg of the K walk (chunk sg / 9, taps (sg % 9) * TG ..) -> buffer sg & 1
    if (w_thread) {                // wave uniform: WPL is a multiple of 64
#pragma unroll
      for (int t = 0; t < TG; ++t) {
        // the BUILTIN, not inline asm: the compiler must know that three more VM operations are in flight.  With an asm
        // DMA its wait for the scratch reloads of the tap loop's addresses (issued in front of the barrier, waited for
        // at first use) was vmcnt(0), which -- memory operations retire in order -- also waited for the DMA: 27 of the
        // 30 DMA instructions of this kernel were drained before the first MFMA of their group, every group began with
        // the round trip of the NEXT group's slices (tools/dma_drain_check.py; found statically at the end of round 2,
        // NOT yet measured on the GPU).  With the builtin the same wait is vmcnt(3) and the DMA flies under the taps.
        const u4 *gp = wp + ((size_t)sg * TG + t) * 4 * Cout + we_g;
        typedef __attribute__((address_space(3))) void lds_void;
        typedef __attribute__((address_space(1))) const void glb_void;
        lds_void *dstp = (lds_void *)(uintptr_t)__builtin_amdgcn_readfirstlane(sw_lds + (uint32_t)(((sg & 1) * TG + t) * WPL * 16));
        __builtin_amdgcn_global_load_lds((glb_void *)gp, dstp, 16, 0, 0);
      }
    }
  };
  if (nchunks) { weights_dma(0); weights_dma(1); } // nchunks >= 1 -> at least 9 groups
  // @phase 0
  // One chunk of the K walk, for a wave that got NVB column blocks of the tile's active voxels.  NVB = 0 is the copy run by
  // a wave without a block: it stages and takes part in every barrier and in the weight DMA, but owns no MFMA and no
  // accumulator; NVB = 1 runs the taps on one column block (CB x 1 accumulator tiles, half the MFMAs).  The copies are
  // separate LOOPS (the branch on the block count sits outside them): with the branch inside the chunk -- per tap or around
  // the 27 taps -- the register allocator split the accumulators' live ranges around the working path and parked five of
  // the eight tuples in scratch across the staging of every chunk (684-792 bytes, 64->64 at 1070 us instead of 705).
  auto chunk = [&](int q, auto nvb_c) {
    constexpr int NVB = decltype(nvb_c)::value;
    constexpr bool WORK = NVB > 0;
    __syncthreads(); // the previous chunk's planes are no longer read (and the prologue scalars are visible)
    // @phase 1
    {
    // Staging by aligned 16-byte row loads: thread rt owns one QUAD of a halo row -- 4 consecutive w of row (hd, hh),
    // starting at w0 - 4 + 4 qd (the rows are read from w0 - 4 to w0 + TW + 3: 6 / 10 quads, of which the first and the
    // last contribute one column each) -- for all 16 channels of the chunk: 16 dwordx4 loads per thread instead of 48
    // dword gathers (per-lane dword gathers are bound by the texture-address path: ~13 k cycles per chunk).  r % 4 == 0 and
    // w0 % 4 == 0: a quad lies entirely inside or entirely outside the grid.
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
    // @phase 2
    __syncthreads(); // the chunk's maximum is complete
    // @phase 3
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
              for (int i = 0; i < 16; ++i) {
                acc[cb][vb][i] *= f;
                if constexpr (P == 2) cor[cb][vb][i] *= f;
              }
        }
        E = e - CONV_SPLIT_HEADROOM;
      }
    }
    const float xs = E == 127 ? 1.0f : pow2f(E);
#pragma unroll
    for (int ig = 0; ig < 2; ++ig)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if constexpr (P == 2) {
          u4 ph, pl;
#pragma unroll
          for (int m = 0; m < 4; ++m) { unsigned h2, l2; cut2(v[ig][2 * m][k] * xs, v[ig][2 * m + 1][k] * xs, h2, l2); ph[m] = h2; pl[m] = l2; }
          if (rt < IPH && hw0 + k >= 0 && hw0 + k < HW) {
            sx[(0 + ig) * HP + p0 + k] = ph;
            sx[(2 + ig) * HP + p0 + k] = pl;
          }
        } else {
          u4 ph;
#pragma unroll
          for (int m = 0; m < 4; ++m) ph[m] = hi2(v[ig][2 * m][k] * xs, v[ig][2 * m + 1][k] * xs);
          if (rt < IPH && hw0 + k >= 0 && hw0 + k < HW) sx[ig * HP + p0 + k] = ph;
        }
      }
    }
    // @phase 4
    // The 27 taps.  Weight slices travel in groups of TG taps through two buffers (group k of chunk q = walk index
    // sg = 9 q + k, buffer sg & 1).  Barrier k sits in front of the LAST tap of group k: by then every wave holds that
    // tap's fragments in registers, so buffer sg & 1 is free for the DMA of group sg + 2, and group sg + 1 (requested one
    // barrier earlier, awaited just before this one) is visible -- its first fragments are requested under the MFMAs of
    // this last tap.  Fragments are double buffered in registers: the reads of tap t + 1 are spread, one at a time,
    // between the MFMAs of tap t (a wave draws 1 KiB per 32 cycles from LDS at best; a burst of eight in front of a tap
    // takes 256 cycles to land), and ONE counted lgkmcnt wait in front of a tap finds them there.  Round 2 read just in
    // time -- five exposed LDS round trips per tap (`r6 wait M4 r wait M ...` in the ISA), as long as the MFMAs themselves.
    {
      const int par = q & 1;
      typedef __attribute__((address_space(3))) const u4 lds_u4;
      // opaque per-chunk base addresses: every fragment read = base + 16-bit immediate.  Left to itself the compiler
      // hoists 27 tap offsets x (VB + CB) addresses out of the chunk loop and spills them.
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
      u4 wf[2][CB][P], xf[2][NX][P];
      constexpr int NR = P * (NVB + CB); // fragment reads per tap
      // read r_ of a tap, in the order the tap's MFMAs need them: X_h (NVB), W_h (CB) -- the main sweep --, then X_l (NVB),
      // then W_l (CB); LDS returns in order, so the counted wait in front of the first MFMA covers only the first NVB + CB
      auto frag = [&](int tap, int s_, int r_) {
        const int pc = r_ >= NVB + CB, rr = pc ? r_ - (NVB + CB) : r_;
        if (rr < NVB) {
          const int vb = rr;
          const int toff = ((tap / 9) * HH + (tap / 3) % 3) * HW + tap % 3;
          xf[s_][vb][pc] = *(lds_u4 *)(uintptr_t)(xq[vb] + (uint32_t)((pc * 2 * HP + toff) * 16));
        } else {
          const int cb = rr - NVB, k = tap / TG, t = tap % TG;
          wf[s_][cb][pc] = *(lds_u4 *)(uintptr_t)(wq2[k & 1] + (uint32_t)((t * WPL + pc * 2 * COT + cb * 32) * 16));
        }
      };
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // group 9 q (requested two barriers ago / in the item prologue)
      __syncthreads(); // the chunk's operand planes and the first weight group are visible
      // @phase 1
      // a wave whose 64-voxel block sees no point (wave mask) takes part in the barriers and the weight DMA only: its own
      // copy of the walk, so that the working waves' 27 taps are straight-line code (one uniform branch per tap cost the
      // register allocator 350 bytes of scratch)
      auto group_barrier = [&](int k) {
        const int sg = q * (27 / TG) + k;
        // @phase 6
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // group sg + 1 has landed
        __syncthreads();
        // @phase 5
        if (sg + 2 < nchunks * (27 / TG)) weights_dma(sg + 2);
      };
      if constexpr (WORK) {
        // raised priority while the wave owns MFMAs: its issue wins the SIMD's arbitration against the co-resident
        // workgroup's staging VALU (64->64@32^3: 618-624 -> 603-614 us)
        __builtin_amdgcn_s_setprio(2);
#pragma unroll
        for (int r_ = 0; r_ < NR; ++r_) frag(0, 0, r_);
#pragma unroll
        for (int tap = 0; tap < 27; ++tap) {
          const int cur = tap & 1, nxt = cur ^ 1;
          if (tap % TG == TG - 1) group_barrier(tap / TG);
          if constexpr (P == 2) {
            // MFMA m of the tap: the CB VB main products, then the X_lo products, then the W_lo products (two MFMAs into one
            // accumulator are CB VB issues apart)
            auto mfma = [&](int m) {
              const int kind = m / (CB * NX), cb = (m / NX) % CB, vb = m % NX;
              if (kind == 0) acc[cb][vb] = mma(wf[cur][cb][0], xf[cur][vb][0], acc[cb][vb]);
              else if (kind == 1) cor[cb][vb] = mma(wf[cur][cb][0], xf[cur][vb][1], cor[cb][vb]);
              else cor[cb][vb] = mma(wf[cur][cb][1], xf[cur][vb][0], cor[cb][vb]);
            };
            constexpr int NM = 3 * CB * NX;
#pragma unroll
            for (int m = 0; m < NM; ++m) {
              // the reads of tap + 1: PER per MFMA slot from slot 1 on (1 at CB = 2: slots 1 .. 8 of 11; 2 at CB = 1), so that
              // the last of them has the rest of this tap to land
              constexpr int PER = (NR + NM - 2) / (NM - 1);
              if (m >= 1 && tap + 1 < 27) {
#pragma unroll
                for (int r_ = (m - 1) * PER; r_ < m * PER && r_ < NR; ++r_) frag(tap + 1, nxt, r_);
              }
              mfma(m);
              __builtin_amdgcn_sched_barrier(0);
            }
          } else {
            constexpr int NM = CB * NX;                 // MFMA m of the tap: channel block m / NX, column block m % NX
            constexpr int PER = (NR + NM - 1) / NM;     // reads of tap + 1 in front of each MFMA slot, from slot 0 on
#pragma unroll
            for (int m = 0; m < NM; ++m) {
              if (tap + 1 < 27) {
#pragma unroll
                for (int r_ = m * PER; r_ < (m + 1) * PER && r_ < NR; ++r_) frag(tap + 1, nxt, r_);
              }
              const int cb = m / NX, vb = m % NX;
              acc[cb][vb] = mma(wf[cur][cb][0], xf[cur][vb][0], acc[cb][vb]);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
        }
        __builtin_amdgcn_s_setprio(0);
      } else {
#pragma unroll
        for (int k = 0; k < 27 / TG; ++k) group_barrier(k);
      }
      // @phase 6
    }
  };
  if (my_nvb == VB) { for (int q = 0; q < nchunks; ++q) chunk(q, IntC<VB>{}); }
  else if (VB > 1 && my_nvb == 1) { for (int q = 0; q < nchunks; ++q) chunk(q, IntC<1>{}); }
  else { for (int q = 0; q < nchunks; ++q) chunk(q, IntC<0>{}); }

  if (delta) {
    __syncthreads(); // the last tap's LDS reads are done: the operand planes become the response table
    for (int e = tid; e < 27 * COT; e += TM) sT[e] = tconst[((size_t)b * 27 + e / COT) * Cout + co0 + e % COT];
    __syncthreads();
  } else if (empty) {
    __syncthreads(); // sbias was written by other threads and no barrier of the K loop ran
  }
  // epilogue: D = main + corr/2048, P = 1: D = main (+ bias | constant response), NCDHW store.  acc register i of lane l:
  // channel row (i&3) + 8*(i>>2) + 4*(l>>5), voxel column l&31.
  float *yb = y + ((size_t)b * Cout + co0) * r3;
  const float us_x = E == 127 ? 1.0f : pow2f(-E), us_w = wscale_inv; // exact powers of two
  // two passes: every output value first (the accumulators become the outputs), then NOTHING BUT stores.  In one loop
  // the compiler reloaded spilled values between the stores and waited for each reload with vmcnt(0|1) -- which also
  // waits for the stores issued before it: 18-23 store / wait / store sequences per epilogue (tools/store_wait_scan.py),
  // each a round trip to memory.
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
        if constexpr (P == 2) acc[cb][vb][i] = ((acc[cb][vb][i] + cor[cb][vb][i] * (1.f / 2048.f)) * us_x) * us_w + addv[co];
        else acc[cb][vb][i] = (acc[cb][vb][i] * us_x) * us_w + addv[co];
      }
  }
#pragma unroll
  for (int vb = 0; vb < VB; ++vb)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = cb * 32 + (i & 3) + 8 * (i >> 2) + 4 * g;
        const float o = acc[cb][vb][i];
        yb[(size_t)co * r3 + gvv[vb]] = o;
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
  // @phase 7
  } // work loop
  // the queue re-arms itself (see csrc/conv3d.hip): the last workgroup to leave zeroes the queue and the exit counter
  if (queued && tid == 0) {
    int32_t *q = occ + 2 * B * ntiles;
    if (atomicAdd(q + 1, 1) == (int)gridDim.x - 1) { q[0] = 0; q[1] = 0; }
  }
  // @phase-flush
}

template <int CB, int OCC, int P, int TD, int TH, int TW> // the spatial tile as conv_tile256_dispatch hands it over
static int launch_split_t(IntC<TD>, IntC<TH>, IntC<TW>, const float *x, const u4 *wp, const float *wtail, const float *bias,
                          float *y, int B, int Cin, int Cout, int r, const float *pa, const float *pb, const float *pbias,
                          const float *tconst, float *stats, int32_t *occ, hipStream_t st) {
  constexpr int COT = 32 * CB, VB = TD * TH * TW / 128;
  constexpr int HALO = (TD + 2) * (TH + 2) * (TW + 2), HP = (HALO + 63) / 64 * 64;
  const int tiles = conv_tile_count(r, VB);
  dim3 grid;
  if (int e = conv_grid(occ != nullptr, B, tiles, Cout / COT, OCC, &grid)) return e;
  // (PRO = false, STATS = true) of the 64-channel tile gets 556-568 bytes of scratch from the register allocator where
  // (true, true) gets 304-360: launches with statistics and without a prologue run on the PRO instantiation with the
  // prologue switched off at run time (pro_a == nullptr).  P = 2 only: that is the kernel it was measured on.
  const bool pro_inst = pa != nullptr || (P == 2 && stats != nullptr && CB == 2 && Cin <= 256);
  const size_t LDS = (size_t)(2 * P * HP + 2 * 3 * 2 * P * COT) * 16 + // planes + two groups of 3 taps of weight slices
                     (size_t)(COT + (pro_inst ? 3 * ((Cin + 63) & ~63) : 0) + 4 * COT * 2) * 4;
  return lion_with_flags(pro_inst, stats != nullptr, [&](auto PRO, auto ST) {
    return lion_launch<conv3d_split_kernel<TD, TH, TW, CB, VB, decltype(PRO)::value, decltype(ST)::value, OCC, P>>(
        grid, 256, LDS, st, x, wp, wtail, bias, y, Cin, Cout, r, pa, pb, pbias, tconst, stats, occ, B, tiles);
  });
}

// uint16 in the pieces of the packed weights, in front of their tail: (Cin/16) * 27 * [2 pieces][2 halves] * Cout * 8
static size_t split_piece_halfs(int Cout, int Cin) { return (size_t)(Cin / KS) * 27 * 4 * Cout * 8; }

// What lion_conv3d_k3_split_forward (P = 2) and lion_conv3d_k3_half_forward (P = 1) share: the argument validation and the
// tile table.  LION_SPLIT_NO_TILE: the tile kernel has no form for this (r, Cin, Cout) -- each entry point answers that
// with its own code (the split one first tries its r = 8 kernel).
constexpr int LION_SPLIT_NO_TILE = -1000;
template <int P>
static int split_tile_forward(const float *x, const uint16_t *wp, const float *bias, int B, int Cin, int Cout, int r,
                              const float *pro_a, const float *pro_b, const float *pro_bias, const float *tconst, float *y,
                              float *stats, int32_t *occ, hipStream_t st) {
  if (int e = conv_forward_args(x, wp, y, B, Cin, Cout, pro_a, pro_b, tconst, occ)) return e;
  if ((r != 16 && r != 32) || Cin % KS != 0 || Cout % 32 != 0) return LION_SPLIT_NO_TILE;
  if (pro_a && Cin > 256) return LION_EUNSUPPORTED;
  const u4 *w4 = reinterpret_cast<const u4 *>(wp);
  const float *wtail = reinterpret_cast<const float *>(wp + split_piece_halfs(Cout, Cin));
  // always the 256-voxel tile of the fp32 kernel's sparse plan, so that the occupancy lists of lion_conv3d_tile_occupancy
  // apply unchanged; 32 * CB channels, two workgroups per CU
  return conv_tile256_dispatch(r, [&](auto TD, auto TH, auto TW) {
    if constexpr (decltype(TW)::value == 8) return (int)LION_SPLIT_NO_TILE; // (refused above: no tile kernel at r = 8)
    else return lion_with_flags(Cout % 64 == 0, [&](auto WIDE) {
      return launch_split_t<decltype(WIDE)::value ? 2 : 1, 2, P>(TD, TH, TW, x, w4, wtail, bias, y, B, Cin, Cout, r, pro_a,
                                                                 pro_b, pro_bias, tconst, stats, occ, st);
    });
  });
}

} // namespace
