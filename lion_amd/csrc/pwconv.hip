// pwconv.hip -- G1: the 1x1 convolutions of SharedMLP (Conv1d / Conv2d with kernel 1,
// models/pvcnn2_ada.py:120-164) as an fp32-MFMA GEMM with the neighbouring AdaGN + Swish folded in.
//
//   y[b, co, l] = bias[co] + sum_ci W[co, ci] * act(x[b, ci, l]),   act(v) = swish(v * A[b,ci] + Bs[b,ci])  (PRO)
//
// The reference runs conv -> GroupNorm -> scale/shift -> sigmoid -> mul, five passes over an
// activation of up to 268 MB ([32,64,1024,32] in the first set-abstraction module); the GEMM itself is
// tiny (K <= 320).  These layers are bound by the bytes of the activations, so the kernel is organised
// around touching them once: the columns l (points, or (centre, neighbour) pairs) sit on the MFMA
// columns, which makes the B operand of v_mfma_f32_32x32x2_f32 a plain coalesced row read of x --
// lane (k-half, column) loads x[k][col] straight into the operand register, no LDS staging, no transpose --
// and every accumulator register a run of 32 consecutive columns of one output channel, i.e.
// 128-byte coalesced stores of the [B, Cout, L] layout.  The previous layer's AdaGN + Swish is
// applied to the operand in flight (PRO), this layer's GroupNorm sums leave with the epilogue
// (STATS: per (batch, channel, column tile) sum and sum of squares, folded by lion_groupnorm_fold).
// A wave owns VB x 32 columns x all Cout channels (CB = Cout / 32 row blocks) of a column tile; the weights (k-major
// packed copy [ceil2(Cin)][Cout]) are staged once per workgroup in LDS, and the workgroup walks several column tiles
// with the operand loads one group of k-steps ahead of the MFMAs (round 7, see "the schedule" in the kernel).
#include "common.h"
#include <algorithm>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// WLDS = false (short activations: L = 16 .. a few thousand columns): the weights are NOT staged in LDS -- every wave
// reads its A operands (128-byte rows of the k-major packed copy) straight from L2.  A staged 64-137 KiB slice per
// workgroup is repaid only by many column tiles; with a handful of tiles it is pure latency, and a workgroup that needs
// most of a CU's LDS cannot start beside the voxelize / devoxelize / convolution workgroups of the main stream (the
// point branch of a PVConv runs on a side stream, in their shadow).
// OUT (round 4): 0 = store y; 1 = GroupNorm sums only, y is NOT stored; 2 = y is not stored either: this layer's own
// AdaGN + Swish (out_a / out_b f32[B, CoutY]) is applied to the accumulators and the maximum over each block of 32
// consecutive columns -- the 32 neighbours of a set-abstraction centre, reference pvcnn2_ada.py:375-377 -- goes to
// ymax f32[B, CoutY, L / 32] (passed as y).  The last layer of a set-abstraction MLP is evaluated twice this way (sums,
// fold, then activated maximum) and its [B, 64, 1024, 32] = 268 MB output never exists: 134 MB read twice instead of
// 134 MB read + 268 MB written + 268 MB read.
// GRP (the first layer of a set-abstraction MLP, lion_pwconv_grouped_forward): the activation is not a tensor but the
// neighbourhood gather BallQuery.forward would have materialised -- column (m, u) of channel k is
// coords[b, k, idx[b, m, u]] - centers[b, k, m] for k < 3 (ONE IEEE subtraction, as grouping_fwd_kernel) and
// feat[b, k - 3, idx[b, m, u]] beyond.  A lane reads the (clamped) index of each of its columns once, before the k loop,
// and the operand loads become gathers from rows of N floats that stay in L2; the [B, 3 + C, M, U] tensor (147 MB at SA-0)
// is neither written nor read.  Same tiles, same k order, same epilogue: y and the sums are those of the two-kernel path,
// bit for bit.  The flag is a trailing parameter pack -- empty for the plain kernels, which keep their names, parameters
// and code (tools/isa_identical.py), PwGather (common.h) for the gathered form.  The pack is copied into a local `g` at
// the top of both kernels: here that leaves the plain instantiations' code as it was.  In pwconv_split.hip the same local
// changed their code (the LDS transposition of the epilogue was scheduled differently), so that kernel names the pack
// only inside its `if constexpr (GRP)` block.
__device__ __forceinline__ PwGather pw_gather() { return PwGather{}; }
__device__ __forceinline__ PwGather pw_gather(const PwGather &g) { return g; }
template <int CB, int VB, bool PRO, bool STATS, bool WLDS, int OUT = 0, typename... G>
__global__ __launch_bounds__(256, 2) void pwconv_kernel(const float *__restrict__ x, const float *__restrict__ wp,
                                                        const float *__restrict__ bias, float *__restrict__ y,
                                                        int Cin, int Cout, int CoutY, int L,
                                                        const float *__restrict__ pro_a,
                                                        const float *__restrict__ pro_b, float *__restrict__ stats,
                                                        const float *__restrict__ out_a = nullptr,
                                                        const float *__restrict__ out_b = nullptr, G... gather) {
  constexpr bool GRP = sizeof...(G) > 0; // pwconv_kernel<..., PwGather>: x is not read
  static_assert(!(GRP && (PRO || OUT)), "the gathered operand is a first layer: no prologue, stored output");
  [[maybe_unused]] const PwGather g = pw_gather(gather...);
  // Cout: channels of the packed weights (a multiple of 32, zero rows beyond CoutY); CoutY: channels of y / bias / stats
  constexpr int COUT = CB * 32; // output channels of this workgroup: [co0, co0 + COUT)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ksteps = (Cin + 1) >> 1;
  float *sw = smem;                       // [2 * ksteps][COUT] weight slice of this channel tile (WLDS)
  float *spa = sw + (WLDS ? 2 * ksteps * COUT : 0); // [Cin] prologue scale   (PRO)
  float *spb = spa + (PRO ? Cin : 0);     // [Cin] prologue shift   (PRO)
  float *sred = spb + (PRO ? Cin : 0);    // [4][COUT][2]           (STATS)
  float *sbias = sred + 4 * COUT * 2;     // [COUT] bias of this channel tile, zero beyond CoutY (read from global in the
                                          // epilogue, every load would sit in front of a store's vmcnt wait)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, co0 = blockIdx.y * COUT, cl = lane & 31, kh = lane >> 5;
  if (WLDS) {
    for (int e = tid; e < 2 * ksteps * COUT; e += 256) {
      const int k = e / COUT, c = e - k * COUT;
      sw[e] = wp[(size_t)k * Cout + co0 + c];
    }
  }
  if (PRO) {
    for (int c = tid; c < Cin; c += 256) { spa[c] = pro_a[(size_t)b * Cin + c]; spb[c] = pro_b[(size_t)b * Cin + c]; }
  }
  for (int c = tid; c < COUT; c += 256) sbias[c] = (bias && co0 + c < CoutY) ? bias[co0 + c] : 0.f;
  float *soa = sbias + COUT, *sob = soa + COUT; // [COUT] each: this layer's own AdaGN scalars (OUT == 2)
  if (OUT == 2) {
    for (int c = tid; c < COUT; c += 256) {
      const bool ok = co0 + c < CoutY;
      soa[c] = ok ? out_a[(size_t)b * CoutY + co0 + c] : 0.f;
      sob[c] = ok ? out_b[(size_t)b * CoutY + co0 + c] : 0.f;
    }
  }
  __syncthreads();
  // ---- the schedule (round 7): a walk over column tiles with the operand one group ahead -------------------------------
  // Until round 6 a wave owned ONE column tile: it requested the activation of 64 / VB k-steps (64 loads), waited once, ran
  // the prologue batch and 128 MFMAs, stored, and ended; the 8 waves of a CU started together and walked those phases in
  // step, so loads, MFMAs and stores added up instead of overlapping, and every tile paid a workgroup's start (weights into
  // LDS, the scalars, a barrier, the first load from a standing start).  Now
  //  * the workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of its (sample, channel tile): the staging is
  //    paid once, and the assignment is static -- no queue, no atomics, nothing read that another workgroup wrote;
  //  * the items (tile, group of GN = 32 / VB k-steps) form one stream and the operand loads of item i + 1, gathers
  //    included, are issued BEFORE the MFMA sweep of item i: `raw` (32 registers) is in flight while `bv` (32, the
  //    prologue's results) feeds the matrix pipe.  At the end of a tile item i + 1 is the first group of the NEXT tile, so
  //    the epilogue's stores and reductions run under loads in flight.  Weights that come from L2 are issued behind their
  //    own item's operand and ahead of that request where a group of them fits 16 registers (WPRE: CB <= 2); for CB = 4 / 8
  //    they are read inside the sweep as before, behind the request.
  // What the compiler's wait placement leaves: the paths with and without an epilogue meet at the loop head, so the wait
  // for `raw` there is vmcnt(0) and a wave drains its stores before the next tile's first MFMA (peeling the first tile would
  // lift that; not done).
  // Loads stay countable: the request of the next item is issued on every path, for the item after the last as well (tile
  // and k clamped to the last valid ones; nothing uses the result).  The arithmetic per column is what it was: ascending
  // k, the same prologue expression, bias add and reduction trees; the sums go to the TILE's slot of [B, CoutY, tiles, 2].
  constexpr int TILE = 4 * VB * 32; // columns of a workgroup's tile
  constexpr int GN = 32 / VB;       // k-steps of a group
  constexpr bool WPRE = !WLDS && CB * GN <= 16; // weights from L2 in registers: a group of them is issued ahead of the
                                                // next item's request (loads return in order: behind it they would wait for it)
  const int tiles = (L + TILE - 1) / TILE;
  const int lc0 = wave * VB * 32 + cl; // this lane's first column inside a tile
  f32x16 acc[CB][VB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int vb = 0; vb < VB; ++vb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[cb][vb][i] = 0.f;

  // Addresses: a uniform row pointer (scalar registers) + a 32-bit byte offset per lane (the launchers keep L and N below
  // PW_MAX_L, so (4 kh L + column) * 4 fits) -- one offset register per column block instead of a 64-bit pointer per load.
  const float *xb = x + (size_t)b * Cin * L;
  const unsigned khL4 = kh ? (unsigned)L * 4u : 0u; // byte offset of the k-half's row
  // GRP: index as a byte offset (gi4: of the tile being loaded, gin: of the tile after it, fetched a tile ahead) and centre
  // (rc0 / rc1: requested with the tile's first group; the centre rows a lane meets are row kh in k-step 0 and, for
  // kh = 0, row 2 in k-step 1) of every column of this lane; the clamped column keeps all three reads inside their tensors
  unsigned gi4[GRP ? VB : 1];
  int gin[GRP ? VB : 1];
  float rc0[GRP ? VB : 1], rc1[GRP ? VB : 1];
  const float *gcb = nullptr, *gfb = nullptr;
  int gfr = 0;
  unsigned khN4 = 0;
  float raw[GN][VB]; // the operand of the next item, in flight
  // clamped columns of tile t (a tile past the last reads the last one's)
  auto columns = [&](int t, int(&c)[VB]) {
    const int base = min(t, tiles - 1) * TILE + lc0;
#pragma unroll
    for (int vb = 0; vb < VB; ++vb) c[vb] = min(base + vb * 32, L - 1); // clamped load, select afterwards
  };
  [[maybe_unused]] auto request_idx = [&](int t) {
    int c[VB];
    columns(t, c);
    const int32_t *ib = g.idx + (size_t)b * L;
#pragma unroll
    for (int vb = 0; vb < VB; ++vb) gin[vb] = *(const int32_t *)((const char *)ib + (unsigned)c[vb] * 4u);
  };
  [[maybe_unused]] auto take_idx = [&]() {
#pragma unroll
    for (int vb = 0; vb < VB; ++vb) gi4[vb] = (unsigned)min(max(gin[vb], 0), g.N - 1) * 4u;
  };
  // issue the loads of item (t, s0): GN k-steps from s0 of tile t.  Lane (kh, column) wants row min(2 (s0 + u) + kh, Cin - 1):
  // the row of kh = 0, clamped, is the uniform base, and kh = 1 adds one row where that row exists.
  auto request = [&](int t, int s0) {
    int c[VB];
    columns(t, c);
    if constexpr (GRP) {
      if (s0 == 0) { // uniform
        const int M = L / g.U;
#pragma unroll
        for (int vb = 0; vb < VB; ++vb) {
          const int m = c[vb] / g.U;
          rc0[vb] = g.centers[((size_t)b * 3 + kh) * M + m];
          rc1[vb] = g.centers[((size_t)b * 3 + 2) * M + m];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < GN; ++u) {
      if constexpr (GRP) {
        if (u < 2) { // may meet rows 0..2, the coordinates: a pointer per lane
          const int kc = min(2 * (s0 + u) + kh, Cin - 1);
          const float *row = gfb + (size_t)min(max(kc - 3, 0), gfr) * g.N;
          row = kc < 3 ? gcb + (size_t)kc * g.N : row;
#pragma unroll
          for (int vb = 0; vb < VB; ++vb) raw[u][vb] = *(const float *)((const char *)row + gi4[vb]);
        } else { // k >= 4: feature rows only
          const int r0 = min(2 * (s0 + u) - 3, gfr);
          const char *ub = (const char *)(gfb + (size_t)r0 * g.N);
          const unsigned ho = r0 < gfr ? khN4 : 0u;
#pragma unroll
          for (int vb = 0; vb < VB; ++vb) raw[u][vb] = *(const float *)(ub + (gi4[vb] + ho));
        }
      } else {
        const int r0 = min(2 * (s0 + u), Cin - 1);
        const char *ub = (const char *)(xb + (size_t)r0 * L);
        const unsigned ho = r0 + 1 < Cin ? khL4 : 0u;
#pragma unroll
        for (int vb = 0; vb < VB; ++vb) raw[u][vb] = *(const float *)(ub + ((unsigned)c[vb] * 4u + ho));
      }
    }
  };

  int t = blockIdx.x, s0 = 0;
  if constexpr (GRP) {
    gcb = g.coords + (size_t)b * 3 * g.N;
    gfb = g.feat ? g.feat + (size_t)b * g.C * g.N : gcb; // no features: the (masked) rows past Cin read coordinates
    gfr = g.feat ? g.C - 1 : 0;
    khN4 = kh ? (unsigned)g.N * 4u : 0u;
    request_idx(t);
    take_idx();
  }
  request(t, 0);
  if constexpr (GRP) request_idx(t + gridDim.x);
  while (t < tiles) { // uniform
    const int col0 = t * TILE + wave * VB * 32;
    int col[VB];
    bool cok[VB];
#pragma unroll
    for (int vb = 0; vb < VB; ++vb) {
      col[vb] = col0 + vb * 32 + cl;
      cok[vb] = col[vb] < L;
    }
    // Round 4: the prologue of the WHOLE group first, the MFMAs afterwards.  Interleaved per operand (rounds 1-3) every
    // pair of MFMAs sat behind its own dependent chain -- LDS read of the scalars, fma, v_exp, v_rcp, mul, select (the
    // ISA: `ds_read x2, wait, v, wait, v v exp v rcp v v, MFMA MFMA` per (k-step, column block)) -- and the matrix pipe
    // ran at ~40 % of its rate inside a wave: SA-0 layer 2 took 108 us without storing a byte, 4x its MFMA time.  As one
    // batch the chains are independent and pipeline; the MFMA sweep that follows is back to back.
    float bv[GN][VB];
    [[maybe_unused]] float wv[WPRE ? GN : 1][WPRE ? CB : 1];
    if constexpr (WPRE) { // this item's weights: behind its operand, ahead of the next item's
#pragma unroll
      for (int u = 0; u < GN; ++u) {
        const char *wb = (const char *)(wp + (size_t)min(2 * (s0 + u), 2 * ksteps - 2) * Cout + co0); // rows exist to ceil2(Cin)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) wv[u][cb] = *(const float *)(wb + ((kh ? (unsigned)Cout : 0u) + cb * 32 + cl) * 4u);
      }
    }
#pragma unroll
    for (int u = 0; u < GN; ++u) {
      const int k = 2 * (s0 + u) + kh;
      const bool kok = k < Cin; // odd Cin: zero operand (the packed weights are zero there too)
#pragma unroll
      for (int vb = 0; vb < VB; ++vb) bv[u][vb] = raw[u][vb];
      if (PRO) {
        const int kc = min(k, Cin - 1);
        const float pa_ = spa[kc], pb_ = spb[kc];
#pragma unroll
        for (int vb = 0; vb < VB; ++vb) bv[u][vb] = swish_fast(bv[u][vb] * pa_ + pb_);
      }
      if constexpr (GRP) {
        if (u < 2) { // k < 3 only in the first group of a tile
#pragma unroll
          for (int vb = 0; vb < VB; ++vb) bv[u][vb] = k < 3 ? sub_rn(bv[u][vb], u == 0 ? rc0[vb] : rc1[vb]) : bv[u][vb];
        }
      }
#pragma unroll
      for (int vb = 0; vb < VB; ++vb) {
        bv[u][vb] = (kok && cok[vb]) ? bv[u][vb] : 0.f;
        asm volatile("" : "+v"(bv[u][vb])); // materialised HERE: left alone the compiler sinks each chain back in front of its MFMAs
      }
    }
    // the next item: this tile's next group, or the first group of the workgroup's next tile
    const bool last = s0 + GN >= ksteps;
    const int tn = last ? t + (int)gridDim.x : t, sn = last ? 0 : s0 + GN;
    if constexpr (GRP) {
      if (last) take_idx();
    }
    request(tn, sn);
    if constexpr (GRP) {
      if (last) request_idx(tn + (int)gridDim.x);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < GN; ++u) {
      if (s0 + u < ksteps) { // uniform
        const int k = 2 * (s0 + u) + kh;
        float av[CB];
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
          if constexpr (WPRE) av[cb] = wv[u][cb];
          else av[cb] = WLDS ? sw[k * COUT + cb * 32 + cl] : wp[(size_t)k * Cout + co0 + cb * 32 + cl]; // rows exist to ceil2(Cin)
        }
#pragma unroll
        for (int vb = 0; vb < VB; ++vb) {
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
            acc[cb][vb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cb], bv[u][vb], acc[cb][vb], 0, 0, 0);
        }
      }
    }
    if (last) { // uniform: the tile is complete
      // epilogue: + bias, [B, Cout, L] store.  acc register i of lane l: channel row (i&3) + 8*(i>>2) + 4*(l>>5),
      // column l&31 -> 32 consecutive columns per (register, half-wave).
      if (OUT == 2) {
        const int M = L >> 5; // centres: blocks of 32 columns (the launcher guarantees L % 32 == 0)
        float *ym = y + ((size_t)b * CoutY + co0) * M;
        unsigned mo[VB]; // byte offset of (row 4 kh, this column block's centre) from a row's uniform pointer
#pragma unroll
        for (int vb = 0; vb < VB; ++vb) mo[vb] = (unsigned)(4 * kh * M + ((col0 + vb * 32) >> 5)) * 4u;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int cu = cb * 32 + (i & 3) + 8 * (i >> 2), co = cu + 4 * kh;
            const bool rok = co0 + co < CoutY;
            const float bz = sbias[co], a2 = soa[co], b2 = sob[co];
            char *yr = (char *)(ym + (size_t)cu * M);
#pragma unroll
            for (int vb = 0; vb < VB; ++vb) {
              float v = swish_fast((acc[cb][vb][i] + bz) * a2 + b2); // == affine_swish_max on the stored y, bit for bit
              v = row16_max(v);                                       // max over the 32 columns of this half-wave:
              v = fmaxf(v, LION_DPP_F32_ROWS(v, 0x142, 0xa));         // rows 1 / 3 take lane 15 of rows 0 / 2
              const int m = (col0 + vb * 32) >> 5;
              if (cl == 16 && rok && m < M) *(float *)(yr + mo[vb]) = v;
            }
          }
      } else {
        float *yb = y + ((size_t)b * CoutY + co0) * L;
        unsigned so[VB]; // byte offset of (row 4 kh, this lane's column) from a row's uniform pointer
#pragma unroll
        for (int vb = 0; vb < VB; ++vb) so[vb] = khL4 * 4u + (unsigned)col[vb] * 4u;
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float bz = sbias[cb * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh];
#pragma unroll
            for (int vb = 0; vb < VB; ++vb) acc[cb][vb][i] = cok[vb] ? acc[cb][vb][i] + bz : 0.f;
          }
        if (OUT == 0) {
          // a tile wholly inside [0, L) x [0, CoutY) -- all but the last of a ragged L, all but a padded Cout's last channel
          // tile -- stores without a predicate: the general form costs a branch around every one of the 128 stores
          auto store = [&](auto WHOLE) {
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
#pragma unroll
              for (int i = 0; i < 16; ++i) {
                const int cu = cb * 32 + (i & 3) + 8 * (i >> 2);
                const bool rok = co0 + cu + 4 * kh < CoutY; // padded channel rows (CoutY % 32 != 0) are computed on zeros and dropped
                char *yr = (char *)(yb + (size_t)cu * L);
#pragma unroll
                for (int vb = 0; vb < VB; ++vb)
                  if (decltype(WHOLE)::value || (cok[vb] && rok)) *(float *)(yr + so[vb]) = acc[cb][vb][i];
              }
          };
          if ((t + 1) * TILE <= L && co0 + COUT <= CoutY) store(BoolC<true>{}); // uniform
          else store(BoolC<false>{});
        }
        if (STATS) {
#pragma unroll
          for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              float s1 = 0.f, s2 = 0.f;
#pragma unroll
              for (int vb = 0; vb < VB; ++vb) { s1 += acc[cb][vb][i]; s2 += acc[cb][vb][i] * acc[cb][vb][i]; }
              s1 = row16_sum_rn(s1); s2 = row16_sum_rn(s2);
              s1 = row_pair_sum_odd_rows(s1); s2 = row_pair_sum_odd_rows(s2);
              if (cl == 16) { // the row pair's sum lives in the odd rows
                const int co = cb * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh;
                sred[(wave * COUT + co) * 2] = s1;
                sred[(wave * COUT + co) * 2 + 1] = s2;
              }
            }
          __syncthreads();
          for (int c = tid; c < COUT && co0 + c < CoutY; c += 256) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { s1 += sred[(w * COUT + c) * 2]; s2 += sred[(w * COUT + c) * 2 + 1]; }
            float *o = stats + (((size_t)b * CoutY + co0 + c) * tiles + t) * 2; // the TILE's slot, not the workgroup's
            o[0] = s1;
            o[1] = s2;
          }
          if (tn < tiles) __syncthreads(); // sred is written again by the next tile
        }
      }
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int vb = 0; vb < VB; ++vb)
#pragma unroll
          for (int i = 0; i < 16; ++i) acc[cb][vb][i] = 0.f;
    }
    t = tn;
    s0 = sn;
  }
}


// ---- short activations (L <= PW_SMALL_L columns): latency, not bytes ------------------------------------------------
// The layers above with a few hundred columns (point branches of the r = 8 / 16 PVConvs, feature propagation, the
// last set-abstraction stages, the classifier, the attention projections) are GEMMs of a few MFLOP.  With the tiling
// of the large kernel they would run on 32 workgroups, each walking its k-steps behind one L2 round trip at a time
// (measured: 150 us at Cin = 256).  Here a workgroup owns 32 columns x 64 output channels and its four waves SPLIT K:
// a wave requests the operands of all its k-steps (<= 32 per round: 2 weight rows + 1 activation row of 128 bytes
// each) before the first MFMA -- one round trip -- and the four partial tiles are combined through LDS in a fixed
// order.  Same arithmetic (fmaf chains over k, then ((w0 + w1) + w2) + w3), prologue and GroupNorm sums as above.
constexpr int PW_SMALL_L = 4096;
template <bool PRO, bool STATS, typename... G>
__global__ __launch_bounds__(256) void pwconv_small_kernel(const float *__restrict__ x, const float *__restrict__ wp,
                                                           const float *__restrict__ bias, float *__restrict__ y,
                                                           int Cin, int Cout, int CoutY, int L,
                                                           const float *__restrict__ pro_a,
                                                           const float *__restrict__ pro_b, float *__restrict__ stats,
                                                           G... gather) {
  constexpr bool GRP = sizeof...(G) > 0; // as in pwconv_kernel
  static_assert(!(GRP && PRO), "the gathered operand is a first layer: no prologue");
  [[maybe_unused]] const PwGather g = pw_gather(gather...);
  __shared__ float part[4][2][1024];
  extern __shared__ __attribute__((aligned(16))) float smem[]; // [2][Cin] prologue scalars (PRO)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 31, kh = lane >> 5;
  const int b = blockIdx.z, co0 = blockIdx.y * 64, col = blockIdx.x * 32 + cl;
  const bool cok = col < L;
  const int colc = cok ? col : L - 1;
  const int ksteps = (Cin + 1) >> 1, per = (ksteps + 3) >> 2;
  const int s_lo = min(ksteps, wave * per), s_hi = min(ksteps, s_lo + per);
  float *spa = smem, *spb = smem + Cin;
  if (PRO) {
    for (int c = tid; c < Cin; c += 256) { spa[c] = pro_a[(size_t)b * Cin + c]; spb[c] = pro_b[(size_t)b * Cin + c]; }
    __syncthreads();
  }
  float brow[8]; // this thread's 8 output rows (tid / 32 + 8 j): fetched now, not in front of the stores
#pragma unroll
  for (int j = 0; j < 8; ++j) brow[j] = (bias && co0 + (tid >> 5) + 8 * j < CoutY) ? bias[co0 + (tid >> 5) + 8 * j] : 0.f;
  const float *xb = x + (size_t)b * Cin * L;
  int gi = 0; // GRP: as in pwconv_kernel -- index and centre of this lane's column, gathers in place of the row reads
  float gc0 = 0.f, gc1 = 0.f;
  const float *gcb = nullptr, *gfb = nullptr;
  int gfr = 0;
  if constexpr (GRP) {
    const int M = L / g.U, m = colc / g.U;
    gcb = g.coords + (size_t)b * 3 * g.N;
    gfb = g.feat ? g.feat + (size_t)b * g.C * g.N : gcb;
    gfr = g.feat ? g.C - 1 : 0;
    gc0 = g.centers[((size_t)b * 3 + kh) * M + m];
    gc1 = g.centers[((size_t)b * 3 + 2) * M + m];
    gi = min(max(g.idx[(size_t)b * L + colc], 0), g.N - 1);
  }
  f32x16 acc[2];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[cb][i] = 0.f;
  constexpr int UN = 32;
  for (int s0 = s_lo; s0 < s_hi; s0 += UN) {
    float av[UN][2], bv[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int k = min(2 * min(s0 + u, ksteps - 1) + kh, 2 * ksteps - 1); // packed rows exist up to ceil2(Cin)
      av[u][0] = wp[(size_t)k * Cout + co0 + cl];
      av[u][1] = wp[(size_t)k * Cout + co0 + 32 + cl];
      if constexpr (GRP) {
        const int kc = min(k, Cin - 1);
        const float *row = kc < 3 ? gcb + (size_t)kc * g.N : gfb + (size_t)min(max(kc - 3, 0), gfr) * g.N;
        bv[u] = row[gi];
      } else {
        bv[u] = xb[(size_t)min(k, Cin - 1) * L + colc];
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int k = 2 * (s0 + u) + kh;
      float v = bv[u];
      if (PRO) {
        const int kc = min(k, Cin - 1);
        const float t = v * spa[kc] + spb[kc];
        v = swish_fast(t); // as in pwconv_kernel
      }
      if constexpr (GRP) v = k < 3 ? sub_rn(v, k == 2 ? gc1 : gc0) : v; // rows 0 / 1 are this lane's row kh
      v = (s0 + u < s_hi && k < Cin && cok) ? v : 0.f;
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][0], v, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][1], v, acc[1], 0, 0, 0);
    }
  }
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) part[wave][cb][((i & 3) + 8 * (i >> 2) + 4 * kh) * 32 + cl] = acc[cb][i];
  __syncthreads();
  // thread -> (channel row = tid / 32 + 8 j, column = tid % 32): 8 channels per thread, coalesced 128-byte row stores
  const int c = tid & 31, colo = blockIdx.x * 32 + c;
  const bool ok = colo < L;
  float *yb = y + ((size_t)b * CoutY + co0) * L;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = (tid >> 5) + 8 * j, cb = row >> 5, e = (row & 31) * 32 + c;
    float o = ((part[0][cb][e] + part[1][cb][e]) + part[2][cb][e]) + part[3][cb][e];
    const bool rok = co0 + row < CoutY;
    o += brow[j];
    if (ok && rok) yb[(size_t)row * L + colo] = o;
    if (STATS) {
      float s1 = ok ? o : 0.f, s2 = s1 * s1;
      s1 = row16_sum_rn(s1); s2 = row16_sum_rn(s2);
      s1 = row_pair_sum_odd_rows(s1); s2 = row_pair_sum_odd_rows(s2);
      if (c == 16 && rok) { // the row pair's sum lives in the odd rows
        float *so = stats + (((size_t)b * CoutY + co0 + row) * gridDim.x + blockIdx.x) * 2;
        so[0] = s1;
        so[1] = s2;
      }
    }
  }
}

// pwconv_small_kernel without its dependent round trips (the library's kernel; the one above stays as the tests' twin,
// lion_internal_pwconv_small_plain).  Two things move, no arithmetic does:
//   * with a prologue the first round's operand loads are in flight BEFORE the scalars go through LDS and the barrier
//     (MR = false: the thread's one pair of scalars is requested first and waited for alone; MR = true: the staging loop's
//     wait covers the operands too) -- one round trip in front of the first MFMA instead of two;
//   * MR (a wave owns more than one round, Cin > 256): round i + 1 is requested before the MFMAs of round i, two register
//     buffers of UN = 16 k-steps (two of 32 do not fit 256 registers beside the accumulators); addresses clamped, loads on
//     every path.  MR = false is the single round of 32, and then the loop is gone.
// The k order of the MFMA chains, the masks, the combine, the bias add, the stores and the sums are pwconv_small_kernel's.
template <bool PRO, bool STATS, bool MR, typename... G>
__global__ __launch_bounds__(256) void pwconv_small_ahead_kernel(const float *__restrict__ x, const float *__restrict__ wp,
                                                                 const float *__restrict__ bias, float *__restrict__ y,
                                                                 int Cin, int Cout, int CoutY, int L,
                                                                 const float *__restrict__ pro_a,
                                                                 const float *__restrict__ pro_b, float *__restrict__ stats,
                                                                 G... gather) {
  constexpr bool GRP = sizeof...(G) > 0; // as in pwconv_kernel
  static_assert(!(GRP && PRO), "the gathered operand is a first layer: no prologue");
  [[maybe_unused]] const PwGather g = pw_gather(gather...);
  __shared__ float part[4][2][1024];
  extern __shared__ __attribute__((aligned(16))) float smem[]; // [2][Cin] prologue scalars (PRO)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 31, kh = lane >> 5;
  const int b = blockIdx.z, co0 = blockIdx.y * 64, col = blockIdx.x * 32 + cl;
  const bool cok = col < L;
  const int colc = cok ? col : L - 1;
  const int ksteps = (Cin + 1) >> 1, per = (ksteps + 3) >> 2;
  const int s_lo = min(ksteps, wave * per), s_hi = min(ksteps, s_lo + per);
  float *spa = smem, *spb = smem + Cin;
  [[maybe_unused]] float ra = 0.f, rb = 0.f;
  if (PRO && !MR) { // Cin <= 256: one pair per thread, requested in front of the operands and waited for alone
    ra = pro_a[(size_t)b * Cin + min(tid, Cin - 1)];
    rb = pro_b[(size_t)b * Cin + min(tid, Cin - 1)];
  }
  const float *xb = x + (size_t)b * Cin * L;
  int gi = 0; // GRP: as in pwconv_kernel -- index and centre of this lane's column, gathers in place of the row reads
  float gc0 = 0.f, gc1 = 0.f;
  const float *gcb = nullptr, *gfb = nullptr;
  int gfr = 0;
  if constexpr (GRP) {
    const int M = L / g.U, m = colc / g.U;
    gcb = g.coords + (size_t)b * 3 * g.N;
    gfb = g.feat ? g.feat + (size_t)b * g.C * g.N : gcb;
    gfr = g.feat ? g.C - 1 : 0;
    gc0 = g.centers[((size_t)b * 3 + kh) * M + m];
    gc1 = g.centers[((size_t)b * 3 + 2) * M + m];
    gi = min(max(g.idx[(size_t)b * L + colc], 0), g.N - 1);
  }
  constexpr int UN = MR ? 16 : 32;
  auto load = [&](int s0, float (&av)[UN][2], float (&bv)[UN]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int k = min(2 * min(s0 + u, ksteps - 1) + kh, 2 * ksteps - 1); // packed rows exist up to ceil2(Cin)
      av[u][0] = wp[(size_t)k * Cout + co0 + cl];
      av[u][1] = wp[(size_t)k * Cout + co0 + 32 + cl];
      if constexpr (GRP) {
        const int kc = min(k, Cin - 1);
        const float *row = kc < 3 ? gcb + (size_t)kc * g.N : gfb + (size_t)min(max(kc - 3, 0), gfr) * g.N;
        bv[u] = row[gi];
      } else {
        bv[u] = xb[(size_t)min(k, Cin - 1) * L + colc];
      }
    }
  };
  f32x16 acc[2];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[cb][i] = 0.f;
  auto mma = [&](int s0, const float (&av)[UN][2], const float (&bv)[UN]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int k = 2 * (s0 + u) + kh;
      float v = bv[u];
      if (PRO) {
        const int kc = min(k, Cin - 1);
        const float t = v * spa[kc] + spb[kc];
        v = swish_fast(t); // as in pwconv_kernel
      }
      if constexpr (GRP) v = k < 3 ? sub_rn(v, k == 2 ? gc1 : gc0) : v; // rows 0 / 1 are this lane's row kh
      v = (s0 + u < s_hi && k < Cin && cok) ? v : 0.f;
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][0], v, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][1], v, acc[1], 0, 0, 0);
    }
  };
  float av0[UN][2], bv0[UN];
  load(s_lo, av0, bv0); // in flight across the prologue's barrier
  float brow[8]; // this thread's 8 output rows (tid / 32 + 8 j): fetched now, not in front of the stores
#pragma unroll
  for (int j = 0; j < 8; ++j) brow[j] = (bias && co0 + (tid >> 5) + 8 * j < CoutY) ? bias[co0 + (tid >> 5) + 8 * j] : 0.f;
  if (PRO) {
    if (MR) {
      for (int c = tid; c < Cin; c += 256) { spa[c] = pro_a[(size_t)b * Cin + c]; spb[c] = pro_b[(size_t)b * Cin + c]; }
    } else if (tid < Cin) {
      spa[tid] = ra;
      spb[tid] = rb;
    }
    __syncthreads();
  }
  if constexpr (MR) {
    float av1[UN][2], bv1[UN];
    for (int s0 = s_lo; s0 < s_hi; s0 += 2 * UN) {
      load(s0 + UN, av1, bv1);
      mma(s0, av0, bv0);
      load(s0 + 2 * UN, av0, bv0);
      if (s0 + UN < s_hi) mma(s0 + UN, av1, bv1);
    }
  } else {
    if (s_lo < s_hi) mma(s_lo, av0, bv0);
  }
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int i = 0; i < 16; ++i) part[wave][cb][((i & 3) + 8 * (i >> 2) + 4 * kh) * 32 + cl] = acc[cb][i];
  __syncthreads();
  // thread -> (channel row = tid / 32 + 8 j, column = tid % 32): 8 channels per thread, coalesced 128-byte row stores
  const int c = tid & 31, colo = blockIdx.x * 32 + c;
  const bool ok = colo < L;
  float *yb = y + ((size_t)b * CoutY + co0) * L;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int row = (tid >> 5) + 8 * j, cb = row >> 5, e = (row & 31) * 32 + c;
    float o = ((part[0][cb][e] + part[1][cb][e]) + part[2][cb][e]) + part[3][cb][e];
    const bool rok = co0 + row < CoutY;
    o += brow[j];
    if (ok && rok) yb[(size_t)row * L + colo] = o;
    if (STATS) {
      float s1 = ok ? o : 0.f, s2 = s1 * s1;
      s1 = row16_sum_rn(s1); s2 = row16_sum_rn(s2);
      s1 = row_pair_sum_odd_rows(s1); s2 = row_pair_sum_odd_rows(s2);
      if (c == 16 && rok) { // the row pair's sum lives in the odd rows
        float *so = stats + (((size_t)b * CoutY + co0 + row) * gridDim.x + blockIdx.x) * 2;
        so[0] = s1;
        so[1] = s2;
      }
    }
  }
}

// nn.Linear on a [B, K] activation (time embedding MLP latent_points_ada.py:47-48, the AdaGN style projections
// adagn.py:45-60 batched by models/adagn.py::StylePlan): y[b][o] = act(bias[o] + sum_k x[b][k] W[o][k]).
// The batch (<= 32 rows per slab) sits on the MFMA columns, 32 output features on the rows, the four waves of a
// workgroup split K and combine through LDS in a fixed order.  W comes k-major from lion_pwconv_pack_weights
// (coalesced 128-byte operand rows); x is a few KiB and stays in L1.  Latency bound by construction: one launch.
__global__ __launch_bounds__(256) void linear_rows_kernel(const float *__restrict__ x, const float *__restrict__ wp,
                                                          const float *__restrict__ bias, int Bn, int K, int O,
                                                          int Opad, int act, float slope, float *__restrict__ y) {
  __shared__ float part[4][1024];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 31, kh = lane >> 5;
  const int o0 = blockIdx.x * 32, b0 = blockIdx.y * 32;
  const int ksteps = (K + 1) >> 1, per = (ksteps + 3) >> 2;
  const int s_lo = min(ksteps, wave * per), s_hi = min(ksteps, s_lo + per);
  const int brow = min(b0 + cl, Bn - 1);
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int s = s_lo; s < s_hi; ++s) {
    const int k = 2 * s + kh, kc = min(k, K - 1);
    const float a = wp[(size_t)k * Opad + o0 + cl];          // packed rows exist up to ceil2(K): zero beyond K
    const float v = (k < K && b0 + cl < Bn) ? x[(size_t)brow * K + kc] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, v, acc, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) part[wave][((i & 3) + 8 * (i >> 2) + 4 * kh) * 32 + cl] = acc[i];
  __syncthreads();
#pragma unroll
  for (int e = tid; e < 1024; e += 256) {
    const int o = o0 + (e >> 5), b = b0 + (e & 31);
    if (o < O && b < Bn) {
      float v = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
      if (bias) v += bias[o];
      if (act == 1) v = v > 0.f ? v : 0.f;
      else if (act == 2) v = v > 0.f ? v : v * slope;
      y[(size_t)b * O + o] = v;
    }
  }
}

// [Cout][Cin] (nn.Conv1d / Conv2d weight with kernel 1) -> [ceil2(Cin)][ceil64(Cout)], zero padded
__global__ void pwconv_pack_kernel(const float *__restrict__ w, int Cout, int Cout_pad, int Cin, int Cin_pad,
                                   float *__restrict__ wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Cin_pad * Cout_pad) return;
  const int co = i % Cout_pad, k = i / Cout_pad;
  wp[i] = (k < Cin && co < Cout) ? w[(size_t)co * Cin + k] : 0.f;
}

// Tile choice: a workgroup covers 4 waves x VB x 32 columns x CB x 32 output channels; CB x VB = 8
// accumulator tiles (128 VGPRs).  All output channels in one workgroup when Cout <= 256 (the activation
// is then read once); Cout = 32: 4 column blocks per wave.
struct PwPlan { int cb, vb; };
static int pw_pad(int Cout) { return (Cout + 31) / 32 * 32; }     // channel rows the tiles cover
static int pw_stride(int Cout) { return (Cout + 63) / 64 * 64; }  // row stride of the packed copy (zero columns beyond Cout)
static size_t pw_lds(int cb, int Cin, bool pro, bool wlds = true) {
  const int ksteps = (Cin + 1) / 2;
  return ((size_t)(wlds ? 2 * ksteps * cb * 32 : 0) + (pro ? 2 * Cin : 0) + 4 * cb * 32 * 2 + 3 * cb * 32) * 4;
}
constexpr size_t PW_LDS_MAX = 150 * 1024;
// Cout: any; the channel tile is the largest of 256 / 128 / 64 / 32 rows that divides ceil32(Cout) and whose weight slice
// (with the prologue scalars: the plan must not depend on the mode) fits LDS
static PwPlan pw_plan(int Cout, int Cin) {
  const int blocks = pw_pad(Cout) / 32;
  if (blocks <= 0 || Cin <= 0) return {0, 0};
  if (blocks % 8 == 0 && pw_lds(8, Cin, true) <= PW_LDS_MAX) return {8, 1};
  if (blocks % 4 == 0 && pw_lds(4, Cin, true) <= PW_LDS_MAX) return {4, 2};
  if (blocks % 2 == 0 && pw_lds(2, Cin, true) <= PW_LDS_MAX) return {2, 4};
  if (pw_lds(1, Cin, true) <= PW_LDS_MAX) return {1, 4};
  return {0, 0};
}

// The grid of pwconv_kernel: `tiles` column tiles of a (sample, channel tile) are walked by gx <= tiles workgroups (tile
// blockIdx.x + i gx each).  gx is capped so that the whole grid is about PW_WALK_WGS workgroups -- a few rounds of the two a CU
// holds, so that the staging of a workgroup is paid once for several tiles and the next tile's loads fly under the
// epilogue -- and then lowered to the smallest that keeps the longest walk as short: every workgroup gets cdiv(tiles, gx)
// tiles or one fewer.  Results do not depend on gx: the sums are stored per tile.
// PwSched: the test entry point's overrides (max_wg > 0: the cap itself; wlds 0 / 1: weights from L2 / through LDS
// whatever the grid).
constexpr int PW_WALK_WGS = 1024;
// pwconv_kernel addresses a lane's element as a uniform row pointer + a 32-bit byte offset of up to 5 rows: L (and the N of
// a gathered operand) stay below 2^27 columns -- 512 MiB per channel row.  Beyond: LION_EUNSUPPORTED, 0 statistics tiles.
constexpr int PW_MAX_L = 1 << 27;
struct PwSched { int max_wg = 0, wlds = -1; };
static int pw_grid_x(int tiles, int gy, int B, const PwSched &o) {
  const long cap = o.max_wg > 0 ? o.max_wg : std::max(1L, PW_WALK_WGS / ((long)gy * B));
  const int walk = lion_cdiv(tiles, (int)std::min<long>(tiles, cap));
  return lion_cdiv(tiles, walk);
}

// The one switch on the plan: cb -> f(IntC<CB>{}, IntC<VB>{}) for the four tiles pw_plan hands out.
template <typename F> static int pw_with_plan(const PwPlan &p, F f) {
  switch (p.cb) {
  case 1: return f(IntC<1>{}, IntC<4>{});
  case 2: return f(IntC<2>{}, IntC<4>{});
  case 4: return f(IntC<4>{}, IntC<2>{});
  case 8: return f(IntC<8>{}, IntC<1>{});
  default: return LION_EUNSUPPORTED; // pw_plan found no tile
  }
}

// What an entry point asks of a launcher.  The form is a compile-time tag, so that only the kernels a form can need exist:
//   PW_STORE   x is a tensor, y is stored (prologue and statistics as given);
//   PW_GATHER  the operand is `g` (x unused): no prologue, y is stored;
//   PW_MAX     the two passes of the "activated maximum without the layer's output" form: oa == nullptr -> OUT = 1, the
//              statistics and nothing else; oa set -> OUT = 2, the maximum into y (= ymax) and no statistics.
enum PwForm { PW_STORE, PW_GATHER, PW_MAX };
struct PwCall {
  const float *x, *wp, *bias;
  float *y, *stats;
  int B, Cin, Cout, L;
  hipStream_t st;
  const float *pa = nullptr, *pb = nullptr, *oa = nullptr, *ob = nullptr;
  PwGather g = {};
  PwSched o = {};
};
// form and the call's flags -> f(PRO, STATS, OUT, gather...), the template arguments after the tile and the trailing
// kernel argument: the kernels' static_asserts reject a combination that no form has
template <PwForm FORM, typename F> static int pw_with_form(const PwCall &c, F f) {
  if constexpr (FORM == PW_GATHER) {
    return lion_with_flags(c.stats != nullptr, [&](auto ST) { return f(BoolC<false>{}, ST, IntC<0>{}, c.g); });
  } else if constexpr (FORM == PW_MAX) {
    return lion_with_flags(c.pa != nullptr, c.oa != nullptr, [&](auto PRO, auto SECOND) {
      constexpr bool second = decltype(SECOND)::value;
      return f(PRO, BoolC<!second>{}, IntC<second ? 2 : 1>{});
    });
  } else {
    return lion_with_flags(c.pa != nullptr, c.stats != nullptr, [&](auto PRO, auto ST) { return f(PRO, ST, IntC<0>{}); });
  }
}

template <PwForm FORM, int CB, int VB> static int launch_pw(const PwCall &c, IntC<CB>, IntC<VB>) {
  const int gy = pw_pad(c.Cout) / (CB * 32), tiles = lion_cdiv(c.L, 4 * VB * 32);
  const dim3 grid(pw_grid_x(tiles, gy, c.B, c.o), gy, c.B);
  // weights through LDS only when a workgroup's column tile is one of many (the staging is then amortised by the L2); the
  // max form is for large activations only and refuses the others, whoever calls
  const bool many = (long)tiles * c.B >= 2048;
  if (FORM == PW_MAX && c.o.wlds < 0 && !many) return LION_EUNSUPPORTED;
  const bool wlds = c.o.wlds < 0 ? many : c.o.wlds != 0;
  const size_t lds = pw_lds(CB, c.Cin, c.pa != nullptr, wlds);
  return pw_with_form<FORM>(c, [&](auto PRO, auto ST, auto OUT, auto... gather) {
    return lion_with_flags(wlds, [&](auto WLDS) {
      return lion_launch<pwconv_kernel<CB, VB, decltype(PRO)::value, decltype(ST)::value, decltype(WLDS)::value,
                                       decltype(OUT)::value, decltype(gather)...>>(
          grid, 256, lds, c.st, c.x, c.wp, c.bias, c.y, c.Cin, pw_stride(c.Cout), c.Cout, c.L, c.pa, c.pb, c.stats, c.oa, c.ob,
          gather...);
    });
  });
}

// pwconv_small_kernel (L <= PW_SMALL_L; PW_STORE or PW_GATHER): one workgroup per 32 columns x 64 channels
// plain: pwconv_small_kernel itself (the tests' twin); otherwise pwconv_small_ahead_kernel, in its multi-round form where a
// wave owns more than 32 k-steps (Cin > 256)
template <PwForm FORM> static int launch_pw_small(const PwCall &c, bool plain = false) {
  const dim3 grid(lion_cdiv(c.L, 32), pw_stride(c.Cout) / 64, c.B);
  const size_t lds = c.pa ? (size_t)2 * c.Cin * 4 : 0;
  if (lds > 64 * 1024) return LION_EUNSUPPORTED;
  return pw_with_form<FORM>(c, [&](auto PRO, auto ST, auto, auto... gather) {
    if (plain)
      return lion_launch<pwconv_small_kernel<decltype(PRO)::value, decltype(ST)::value, decltype(gather)...>>(
          grid, 256, lds, c.st, c.x, c.wp, c.bias, c.y, c.Cin, pw_stride(c.Cout), c.Cout, c.L, c.pa, c.pb, c.stats, gather...);
    return lion_with_flags(c.Cin > 256, [&](auto MR) {
      return lion_launch<pwconv_small_ahead_kernel<decltype(PRO)::value, decltype(ST)::value, decltype(MR)::value,
                                                   decltype(gather)...>>(
          grid, 256, lds, c.st, c.x, c.wp, c.bias, c.y, c.Cin, pw_stride(c.Cout), c.Cout, c.L, c.pa, c.pb, c.stats, gather...);
    });
  });
}

} // namespace

extern "C" {

// The last layer of a set-abstraction MLP without its output (pvcnn2_ada.py:120-164 + :375-377: conv -> AdaGN -> Swish ->
// max over the 32 neighbours): call once with out_a == NULL (GroupNorm sums into stats, nothing else written), fold
// (lion_groupnorm_fold), call again with out_a / out_b f32[B,Cout] = this layer's AdaGN scalars and ymax f32[B,Cout,L/32].
// Same arguments otherwise as lion_pwconv_forward; L % 32 == 0, L > 4096, large grids only (LION_EUNSUPPORTED otherwise:
// the caller then stores y and runs lion_affine_swish_max).  Bit-identical to that three-kernel path.
int lion_pwconv_forward_max(const float *x, const float *wp, const float *bias, int B, int Cin, int Cout, int L,
                            const float *pro_a, const float *pro_b, const float *out_a, const float *out_b, float *stats,
                            float *ymax, lionStream_t stream) {
  if (!x || !wp || B <= 0 || Cin <= 0 || Cout <= 0 || L <= 0) return LION_EINVAL;
  if ((pro_a == nullptr) != (pro_b == nullptr) || (out_a == nullptr) != (out_b == nullptr)) return LION_EINVAL;
  if (out_a ? !ymax : !stats) return LION_EINVAL;
  if (L % 32 != 0 || L <= PW_SMALL_L || L >= PW_MAX_L) return LION_EUNSUPPORTED;
  const PwPlan p = pw_plan(Cout, Cin);
  if (!p.cb) return LION_EUNSUPPORTED;
  const PwCall c{x, wp, bias, ymax, stats, B, Cin, Cout, L, static_cast<hipStream_t>(stream), pro_a, pro_b, out_a, out_b};
  return pw_with_plan(p, [&](auto CB, auto VB) { return launch_pw<PW_MAX>(c, CB, VB); });
}

size_t lion_pwconv_packed_floats(int Cout, int Cin) { return (size_t)((Cin + 1) / 2 * 2) * pw_stride(Cout); }

int lion_pwconv_pack_weights(const float *w, int Cout, int Cin, float *wp, lionStream_t stream) {
  if (!w || !wp || Cout <= 0 || Cin <= 0) return LION_EINVAL;
  const int Cin_pad = (Cin + 1) / 2 * 2, Cout_pad = pw_stride(Cout);
  return lion_launch<pwconv_pack_kernel>(lion_cdiv(Cin_pad * Cout_pad, 256), 256, 0, static_cast<hipStream_t>(stream),
                                         w, Cout, Cout_pad, Cin, Cin_pad, wp);
}

// column tiles per batch element = rows of the stats tensor per channel (0: shape not supported)
int lion_pwconv_stat_tiles(int Cout, int Cin, int L) {
  if (L > 0 && L <= PW_SMALL_L && Cout > 0 && Cin > 0) return lion_cdiv(L, 32); // pwconv_small_kernel: 32-column tiles
  const PwPlan p = pw_plan(Cout, Cin);
  return (p.cb && L > 0 && L < PW_MAX_L) ? lion_cdiv(L, 4 * p.vb * 32) : 0;
}

// x f32[B,Cin,L], wp from lion_pwconv_pack_weights, bias f32[Cout] or NULL -> y f32[B,Cout,L];
// any Cout (channel tiles of 32..256, rows beyond Cout are zero weights and never stored), weight slice <= 150 KiB of LDS.  pro_a / pro_b f32[B,Cin] (both or neither):
// the input is swish(x*a+b).  stats f32[B,Cout,lion_pwconv_stat_tiles(Cout,Cin,L),2] or NULL.
// Built around the large activations (set-abstraction MLPs, L = M*U: one read + one write per layer); the short ones
// (L = 16 .. 256 points, classifier, attention projections) are latency bound whatever runs them and use it too.
int lion_pwconv_forward(const float *x, const float *wp, const float *bias, int B, int Cin, int Cout, int L,
                        const float *pro_a, const float *pro_b, float *y, float *stats, lionStream_t stream) {
  if (!x || !wp || !y || B <= 0 || Cin <= 0 || Cout <= 0 || L <= 0) return LION_EINVAL;
  if ((pro_a == nullptr) != (pro_b == nullptr)) return LION_EINVAL;
  const PwCall c{x, wp, bias, y, stats, B, Cin, Cout, L, static_cast<hipStream_t>(stream), pro_a, pro_b};
  if (L <= PW_SMALL_L) return launch_pw_small<PW_STORE>(c);
  const PwPlan p = pw_plan(Cout, Cin);
  if (!p.cb || L >= PW_MAX_L) return LION_EUNSUPPORTED;
  return pw_with_plan(p, [&](auto CB, auto VB) { return launch_pw<PW_STORE>(c, CB, VB); });
}

// lion_group_points_forward followed by lion_pwconv_forward (no prologue) without the [B, 3 + C, M, U] tensor between them:
// Cin = 3 + C, L = M * U, column (m, u) of channel k = coords[b,k,idx[b,m,u]] - centers[b,k,m] (k < 3) or
// feat[b,k-3,idx[b,m,u]]; idx is clamped to [0, N) as the grouping kernel clamps it.  wp, bias, y, stats as
// lion_pwconv_forward for (Cin, L); same kernels by the same rules, y and stats bit-identical to the two calls.
int lion_pwconv_grouped_forward(const float *coords, const float *centers, const float *feat, const int32_t *idx,
                                const float *wp, const float *bias, int B, int C, int N, int M, int U, int Cout, float *y,
                                float *stats, lionStream_t stream) {
  if (!coords || !centers || !idx || !wp || !y || B <= 0 || C < 0 || N <= 0 || M <= 0 || U <= 0 || Cout <= 0) return LION_EINVAL;
  if (C > 0 && !feat) return LION_EINVAL;
  if ((long)M * U >= (1L << 31) || (long)C * N >= (1L << 31)) return LION_EUNSUPPORTED;
  const int Cin = 3 + C, L = M * U;
  PwCall c{nullptr, wp, bias, y, stats, B, Cin, Cout, L, static_cast<hipStream_t>(stream)};
  c.g = PwGather{coords, centers, C > 0 ? feat : nullptr, idx, C, N, U};
  if (L <= PW_SMALL_L) return launch_pw_small<PW_GATHER>(c);
  const PwPlan p = pw_plan(Cout, Cin);
  if (!p.cb || L >= PW_MAX_L || N >= PW_MAX_L) return LION_EUNSUPPORTED;
  return pw_with_plan(p, [&](auto CB, auto VB) { return launch_pw<PW_GATHER>(c, CB, VB); });
}

// For tests only: pwconv_kernel itself at ANY L (the entry points above hand L <= 4096 to pwconv_small_kernel and refuse
// the max form on small grids), with at most max_wg workgroups per (sample, channel tile) (<= 0: the library's cap) and
// the weights through LDS (lds_weights 1), from L2 (0) or by the tiles * B >= 2048 rule (< 0): a few hundred columns then
// walk several tiles.  idx != NULL: the gathered operand of lion_pwconv_grouped_forward (x unused, Cin = 3 + C, feat NULL
// when Cin = 3, L = M * U); otherwise x as lion_pwconv_forward.  out_a != NULL: the second pass of
// lion_pwconv_forward_max (y = ymax); y == NULL: its first pass (sums only); otherwise y is stored.
int lion_internal_pwconv_walk(const float *x, const float *wp, const float *bias, int B, int Cin, int Cout, int L,
                              const float *pro_a, const float *pro_b, const float *out_a, const float *out_b,
                              const float *coords, const float *centers, const float *feat, const int32_t *idx, int N, int U,
                              float *y, float *stats, int max_wg, int lds_weights, lionStream_t stream) {
  if (!wp || B <= 0 || Cin <= 0 || Cout <= 0 || L <= 0) return LION_EINVAL;
  if ((pro_a == nullptr) != (pro_b == nullptr) || (out_a == nullptr) != (out_b == nullptr)) return LION_EINVAL;
  const bool grouped = idx != nullptr, maxform = out_a || !y;
  if (out_a ? !y : (!y && !stats)) return LION_EINVAL;
  if (grouped ? (!coords || !centers || N <= 0 || U <= 0 || L % U != 0 || Cin < 3 || (Cin > 3 && !feat) || pro_a || maxform) : !x)
    return LION_EINVAL;
  if ((maxform && L % 32 != 0) || L >= PW_MAX_L || (grouped && N >= PW_MAX_L)) return LION_EUNSUPPORTED;
  const PwPlan p = pw_plan(Cout, Cin);
  if (!p.cb) return LION_EUNSUPPORTED;
  const PwCall c{grouped ? nullptr : x, wp, bias, y, stats, B, Cin, Cout, L, static_cast<hipStream_t>(stream),
                 pro_a, pro_b, out_a, out_b, PwGather{coords, centers, Cin > 3 ? feat : nullptr, idx, Cin - 3, N, U},
                 PwSched{max_wg, lds_weights}};
  return pw_with_plan(p, [&](auto CB, auto VB) {
    if (grouped) return launch_pw<PW_GATHER>(c, CB, VB);
    if (maxform) return launch_pw<PW_MAX>(c, CB, VB);
    return launch_pw<PW_STORE>(c, CB, VB);
  });
}

// For tests only: pwconv_small_kernel itself (L <= 4096), which waits for the prologue scalars before it requests an operand
// and for each round's MFMAs before the next round's loads; lion_pwconv_forward / lion_pwconv_grouped_forward at such an L
// run pwconv_small_ahead_kernel and must equal it bit for bit.  Arguments of lion_pwconv_forward; idx != NULL: the gathered
// operand as in lion_internal_pwconv_walk (x unused, Cin = 3 + C, feat NULL when Cin = 3, L = M * U, no prologue).
int lion_internal_pwconv_small_plain(const float *x, const float *wp, const float *bias, int B, int Cin, int Cout, int L,
                                     const float *pro_a, const float *pro_b, const float *coords, const float *centers,
                                     const float *feat, const int32_t *idx, int N, int U, float *y, float *stats,
                                     lionStream_t stream) {
  if (!wp || !y || B <= 0 || Cin <= 0 || Cout <= 0 || L <= 0) return LION_EINVAL;
  if ((pro_a == nullptr) != (pro_b == nullptr)) return LION_EINVAL;
  const bool grouped = idx != nullptr;
  if (grouped ? (!coords || !centers || N <= 0 || U <= 0 || L % U != 0 || Cin < 3 || (Cin > 3 && !feat) || pro_a) : !x)
    return LION_EINVAL;
  if (L > PW_SMALL_L) return LION_EUNSUPPORTED;
  PwCall c{grouped ? nullptr : x, wp, bias, y, stats, B, Cin, Cout, L, static_cast<hipStream_t>(stream), pro_a, pro_b};
  if (!grouped) return launch_pw_small<PW_STORE>(c, true);
  c.g = PwGather{coords, centers, Cin > 3 ? feat : nullptr, idx, Cin - 3, N, U};
  return launch_pw_small<PW_GATHER>(c, true);
}

// y f32[B,O] = act(x f32[B,K] W^T + bias), wp = lion_pwconv_pack_weights(W f32[O,K]) (k-major, O padded to 32);
// act 0 none / 1 relu / 2 leaky-relu(slope).  nn.Linear of the time-embedding MLP and the batched AdaGN projections.
int lion_linear_forward(const float *x, const float *wp, const float *bias, int B, int K, int O, int act, float slope,
                        float *y, lionStream_t stream) {
  if (!x || !wp || !y || B <= 0 || K <= 0 || O <= 0 || act < 0 || act > 2) return LION_EINVAL;
  const int Opad = pw_stride(O);
  return lion_launch<linear_rows_kernel>(dim3(pw_pad(O) / 32, lion_cdiv(B, 32)), 256, 0,
                                         static_cast<hipStream_t>(stream), x, wp, bias, B, K, O, Opad, act, slope, y);
}

} // extern "C"
