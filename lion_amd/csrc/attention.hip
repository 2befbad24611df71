// attention.hip -- P5: the core of LinearAttention (models/pvcnn2_ada.py:43-71) between its two 1x1 convolutions:
//   q, k, v = split(to_qkv(x))                    [B, heads, 32, N] each  (channel order (qkv, head, d))
//   p = softmax over the N points of k, per row d
//   ctx[d][e] = sum_n p[d][n] v[e][n]             [32, 32] per (batch, head)
//   out[e][n] = sum_d ctx[d][e] q[d][n]           -> [B, heads * 32, N]
// The reference issues a rearrange copy, a softmax and two batched einsums (bmm) per call.  Here one workgroup per
// (batch, head) does all of it on the fp32 matrix cores: the row maxima / sums in two sweeps over the L2-resident k
// rows, ctx as a 32 x 32 x N GEMM whose operands go through LDS transposed (n-major, padded stride 33: conflict-free
// MFMA operand reads), out as a 32 x N x 32 GEMM whose B operand (q) is read straight from memory in 128-byte rows.
// Exact fp32 (fmaf chains), accurate expf: compared with a float64 evaluation at 1e-5 (tests).
#include "common.h"
#include <math.h>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int AD = 32;   // dim_head of every LinearAttention in the models
constexpr int AT = 64;   // points per staged tile

__global__ __launch_bounds__(256) void linattn_core_kernel(const float *__restrict__ qkv, int H, int N,
                                                           float *__restrict__ out) {
  __shared__ float pT[AT * 33], vT[AT * 33]; // [n][d] / [n][e], stride 33
  __shared__ float part[4][1024];
  __shared__ float rmax[AD], rinv[AD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 31, kh = lane >> 5;
  const int h = blockIdx.x, b = blockIdx.y;
  const size_t bs = (size_t)b * 3 * H * AD * N;
  const float *q = qkv + bs + (size_t)(0 * H + h) * AD * N;
  const float *k = qkv + bs + (size_t)(1 * H + h) * AD * N;
  const float *v = qkv + bs + (size_t)(2 * H + h) * AD * N;

  // ---- softmax statistics of the 32 rows of k: 8 lanes per row ----
  {
    const int d = tid >> 3, sub = tid & 7;
    const float *kr = k + (size_t)d * N;
    float m = -INFINITY;
    for (int n = sub; n < N; n += 8) { const float t = kr[n]; m = t > m ? t : m; }
    for (int s = 1; s < 8; s <<= 1) { const float o = __shfl_xor(m, s, 64); m = o > m ? o : m; }
    float sum = 0.f;
    for (int n = sub; n < N; n += 8) sum += expf(kr[n] - m);
    for (int s = 1; s < 8; s <<= 1) sum += __shfl_xor(sum, s, 64);
    if (sub == 0) { rmax[d] = m; rinv[d] = 1.0f / sum; }
  }
  __syncthreads();

  // ---- ctx[d][e] = sum_n p[d][n] v[e][n]: tiles of AT points through LDS, each wave 8 of the tile's 32 k-steps ----
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int tn = tid & 63, d0 = (tid >> 6) * 8; // staging: thread = (point of the tile, 8 rows)
  for (int n0 = 0; n0 < N; n0 += AT) {
    const int n = n0 + tn;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = d0 + j;
      float pv = 0.f, vv = 0.f;
      if (n < N) {
        pv = expf(k[(size_t)d * N + n] - rmax[d]) * rinv[d];
        vv = v[(size_t)d * N + n];
      }
      pT[tn * 33 + d] = pv;
      vT[tn * 33 + d] = vv;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int nn = 2 * (wave * 8 + u) + kh;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pT[nn * 33 + cl], vT[nn * 33 + cl], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  // acc register i of lane l: row d = (i&3) + 8*(i>>2) + 4*kh, column e = cl
#pragma unroll
  for (int i = 0; i < 16; ++i) part[wave][((i & 3) + 8 * (i >> 2) + 4 * kh) * 32 + cl] = acc[i];
  __syncthreads();
  float *ctx = pT; // [d][e], stride 33 (the tiles are done)
#pragma unroll
  for (int e = tid; e < 1024; e += 256)
    ctx[(e >> 5) * 33 + (e & 31)] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
  __syncthreads();

  // ---- out[e][n] = sum_d ctx[d][e] q[d][n]: rows e, 32-point column blocks round-robin over the waves ----
  float av[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) av[s] = ctx[(2 * s + kh) * 33 + cl]; // A[e = cl][d = 2s + kh]
  float *ob = out + ((size_t)b * H + h) * AD * N;
  for (int c0 = wave * 32; c0 < N; c0 += 128) {
    const int n = c0 + cl;
    const bool ok = n < N;
    const int nc = ok ? n : N - 1;
    float bv[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) bv[s] = q[(size_t)(2 * s + kh) * N + nc];
    f32x16 o;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) o = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], ok ? bv[s] : 0.f, o, 0, 0, 0);
    if (ok) {
#pragma unroll
      for (int i = 0; i < 16; ++i) ob[(size_t)((i & 3) + 8 * (i >> 2) + 4 * kh) * N + n] = o[i];
    }
  }
}

// The same core with every load ahead of its use (linattn_core_kernel above stays as the plain form: N % 4 != 0 or
// pointers off 16 bytes, and the twin the tests compare with).  The plain kernel sweeps k twice with one 4-byte load per
// step and consumes each value before the next is requested, reads k a third time and v tile by tile with nothing in
// flight during a tile's MFMAs, and loads each q column block only when its MFMAs are due.  Here
//   RES (the 32 x N block of k fits LDS: N <= 1024): k comes in ONCE, in 16-byte coalesced loads, up to 32 per lane in
//     flight, into rows of stride N + 4 (conflict-free 16-byte operand reads).  The row maxima, the row sums and p come
//     from LDS: the sum sweep leaves e = expf(k - max) in place of k -- the value the plain kernel evaluates a second
//     time for p = e * (1 / sum) -- and the ctx waves take their 16 points per row straight from that block;
//   streaming (larger N): k is read three times as before, the sweeps in batches of 8 loads per lane, the k tile staged
//     one tile ahead with v;
//   both: v tiles are requested one tile ahead in 16-byte loads and double buffered in LDS, one barrier per tile; the q
//     columns of block c + 1 are in flight under the MFMAs of block c.
// Every sum keeps its order: eight interleaved partials per row combined by the xor tree 1, 2, 4; wave w's ctx chain takes
// points 16w .. 16w + 15 of each tile, u = 0 .. 7; ((0 + 1) + 2) + 3; s = 0 .. 15 in the out phase.
constexpr int ASP = 4;            // padding of a resident k row, floats
constexpr int ATILE = AT * 33;    // floats of one staged tile

__host__ __device__ constexpr int linattn_region_a(bool res, int N) {
  return res ? (AD * (N + ASP) > AD * 33 ? AD * (N + ASP) : AD * 33) : 2 * ATILE;
}

// (one workgroup of four waves per CU -- the resident block fills LDS --: a wave may hold its 32 loads in registers)
template <bool RES>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void linattn_core_ahead_kernel(const float *__restrict__ qkv, int H, int N,
                                                                 float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *ra = lds;                              // RES: e[32][N + 4]; streaming: pT[2][64 * 33]; then ctx[32][33]
  float *vT = lds + linattn_region_a(RES, N);   // [2][64 * 33]; then part[4][1024]
  float *rmax = vT + 2 * ATILE, *rinv = rmax + AD;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), cl = lane & 31, kh = lane >> 5;
  const int h = blockIdx.x, b = blockIdx.y;
  const size_t bs = (size_t)b * 3 * H * AD * N;
  const float *q = qkv + bs + (size_t)(0 * H + h) * AD * N;
  const float *k = qkv + bs + (size_t)(1 * H + h) * AD * N;
  const float *v = qkv + bs + (size_t)(2 * H + h) * AD * N;
  const int ES = N + ASP, nq = N >> 2;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

  // staging of a tile: thread -> two (row, 4 points) pieces; addresses clamped, pieces beyond N zeroed when written
  float4 vn[2], kn[2];
  auto stage_load = [&](int n0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = tid + 256 * j, d = idx >> 4, n = min(n0 + 4 * (idx & 15), N - 4);
      vn[j] = *reinterpret_cast<const float4 *>(v + (size_t)d * N + n);
      if (!RES) kn[j] = *reinterpret_cast<const float4 *>(k + (size_t)d * N + n);
    }
  };
  stage_load(0);

  if (RES) { // k -> LDS once: wave w takes rows 8w .. 8w + 7, a lane 16-byte pieces lane, lane + 64, ...
    const float4 *k4 = reinterpret_cast<const float4 *>(k);
    auto rows_load = [&](int c, float4(&t)[8]) {
#pragma unroll
      for (int r = 0; r < 8; ++r) t[r] = k4[(size_t)(wave * 8 + r) * nq + c];
    };
    auto rows_store = [&](int c, const float4(&t)[8]) {
#pragma unroll
      for (int r = 0; r < 8; ++r) *reinterpret_cast<float4 *>(&ra[(wave * 8 + r) * ES + 4 * c]) = t[r];
    };
    int c0 = 0;
    for (; c0 + 256 <= nq; c0 += 256) { // 4 x 8 loads per lane before the first wait: all of k at N = 1024
      float4 t0[8], t1[8], t2[8], t3[8];
      rows_load(c0 + lane, t0);
      rows_load(c0 + 64 + lane, t1);
      rows_load(c0 + 128 + lane, t2);
      rows_load(c0 + 192 + lane, t3);
      rows_store(c0 + lane, t0);
      rows_store(c0 + 64 + lane, t1);
      rows_store(c0 + 128 + lane, t2);
      rows_store(c0 + 192 + lane, t3);
    }
    for (; c0 < nq; c0 += 64) { // a lane beyond the row repeats its last piece, in the row's padding or over itself
      float4 t0[8];
      const int c = min(c0 + lane, nq - 1);
      rows_load(c, t0);
      rows_store(c, t0);
    }
    __syncthreads();
  }

  // ---- softmax statistics of the 32 rows of k: 8 lanes per row, batches of 8 values per lane ----
  {
    const int d = tid >> 3, sub = tid & 7;
    const float *kg = k + (size_t)d * N;
    float *kl = ra + d * ES;
    float m = -INFINITY;
    for (int n = sub; n < N; n += 64) {
      float t[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { const int nn = min(n + 8 * j, N - 1); t[j] = RES ? kl[nn] : kg[nn]; }
#pragma unroll
      for (int j = 0; j < 8; ++j) m = t[j] > m ? t[j] : m; // a clamped repeat is another value of the same row
    }
    for (int s = 1; s < 8; s <<= 1) { const float o = __shfl_xor(m, s, 64); m = o > m ? o : m; }
    float sum = 0.f;
    for (int n = sub; n < N; n += 64) {
      float t[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { const int nn = min(n + 8 * j, N - 1); t[j] = RES ? kl[nn] : kg[nn]; }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int nn = n + 8 * j;
        const float ev = expf(t[j] - m);
        sum = nn < N ? sum + ev : sum;
        if (RES && nn < N) kl[nn] = ev;
      }
    }
    for (int s = 1; s < 8; s <<= 1) sum += __shfl_xor(sum, s, 64);
    if (sub == 0) { rmax[d] = m; rinv[d] = 1.0f / sum; }
  }
  __syncthreads();

  // ---- ctx[d][e] = sum_n p[d][n] v[e][n]: tiles of AT points, each wave 8 of the tile's 32 k-steps ----
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const float ri = rinv[cl];
  for (int n0 = 0, buf = 0; n0 < N; n0 += AT, buf ^= 1) {
    float *vb = vT + buf * ATILE, *pb = ra + buf * ATILE;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = tid + 256 * j, d = idx >> 4, c = 4 * (idx & 15);
      const bool ok = n0 + c < N;
      const float4 vv = ok ? vn[j] : zero4;
      vb[(c + 0) * 33 + d] = vv.x; vb[(c + 1) * 33 + d] = vv.y; vb[(c + 2) * 33 + d] = vv.z; vb[(c + 3) * 33 + d] = vv.w;
      if (!RES) {
        const float mx = rmax[d], rv = rinv[d];
        pb[(c + 0) * 33 + d] = ok ? expf(kn[j].x - mx) * rv : 0.f;
        pb[(c + 1) * 33 + d] = ok ? expf(kn[j].y - mx) * rv : 0.f;
        pb[(c + 2) * 33 + d] = ok ? expf(kn[j].z - mx) * rv : 0.f;
        pb[(c + 3) * 33 + d] = ok ? expf(kn[j].w - mx) * rv : 0.f;
      }
    }
    stage_load(n0 + AT); // the next tile travels under this tile's MFMAs (past the end: a clamped repeat, unused)
    __syncthreads(); // one per tile: the buffers written now were last read two tiles ago, before the previous barrier
    float pa[8]; // RES: p of points 16w + 2u + kh of the tile, row cl
    if (RES) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int n = n0 + 16 * wave + 4 * i;
        const float4 e4 = *reinterpret_cast<const float4 *>(&ra[cl * ES + min(n, N - 4)]);
        const bool ok = n < N;
        pa[2 * i + 0] = ok ? (kh ? e4.y : e4.x) * ri : 0.f;
        pa[2 * i + 1] = ok ? (kh ? e4.w : e4.z) * ri : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int nn = 2 * (wave * 8 + u) + kh;
      const float a = RES ? pa[u] : pb[nn * 33 + cl];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, vb[nn * 33 + cl], acc, 0, 0, 0);
    }
  }
  // the first q column block of this wave travels under the combine of the four chains
  float bv[16], bn[16];
  auto q_load = [&](int c0, float *dst) {
    const int nc = min(c0 + cl, N - 1);
#pragma unroll
    for (int s = 0; s < 16; ++s) dst[s] = q[(size_t)(2 * s + kh) * N + nc];
  };
  q_load(wave * 32, bv);
  __syncthreads(); // every wave is done with the tiles (and, RES, with e) before they become part and ctx
  float(*part)[1024] = reinterpret_cast<float(*)[1024]>(vT);
#pragma unroll
  for (int i = 0; i < 16; ++i) part[wave][((i & 3) + 8 * (i >> 2) + 4 * kh) * 32 + cl] = acc[i];
  __syncthreads();
  float *ctx = ra; // [d][e], stride 33
#pragma unroll
  for (int e = tid; e < 1024; e += 256)
    ctx[(e >> 5) * 33 + (e & 31)] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
  __syncthreads();

  // ---- out[e][n] = sum_d ctx[d][e] q[d][n]: rows e, 32-point column blocks round-robin over the waves ----
  float av[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) av[s] = ctx[(2 * s + kh) * 33 + cl]; // A[e = cl][d = 2s + kh]
  float *ob = out + ((size_t)b * H + h) * AD * N;
  auto q_block = [&](int c0, bool whole) {
    const int n = c0 + cl;
    const bool ok = whole || n < N;
    f32x16 o;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) o = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], ok ? bv[s] : 0.f, o, 0, 0, 0);
    if (ok) {
#pragma unroll
      for (int i = 0; i < 16; ++i) ob[(size_t)((i & 3) + 8 * (i >> 2) + 4 * kh) * N + n] = o[i];
    }
  };
  int c0 = wave * 32;
  for (; c0 + 32 <= N; c0 += 128) { // whole blocks: nothing in the loop depends on a lane, so every wait is counted exactly
    q_load(c0 + 128, bn);           // (past the end: clamped repeats, unused)
    q_block(c0, true);
#pragma unroll
    for (int s = 0; s < 16; ++s) bv[s] = bn[s];
  }
  if (c0 < N) q_block(c0, false); // the last, partly filled block
}

// Backward of the core (training; reference models/pvcnn2_ada.py:62-68 differentiated).  With p = softmax_n(k), g = the
// gradient of out:
//   gctx[d][e] = sum_n q[d][n] g[e][n]          gq[d][n] = sum_e ctx[d][e] g[e][n]        gv[e][n] = sum_d p[d][n] gctx[d][e]
//   gp[d][n]   = sum_e gctx[d][e] v[e][n]       gk[d][n] = p[d][n] (gp[d][n] - dot[d]),   dot[d] = sum_n p gp = sum_e gctx[d][e] ctx[d][e]
// (the softmax backward's row dot product needs no second sweep over the points: it is a 32 x 32 contraction).  One
// workgroup per (batch, head), as the forward: the row statistics of k, ctx and gctx as two 32 x 32 x N fp32-MFMA GEMMs
// over tiles staged through LDS, then per 32-point column block three 32 x 32 x 32 GEMMs (gq, gp, gv) whose B operands
// are read straight from memory in 128-byte rows.  Exact fp32 products (fmaf chains); compared with float64 autograd.
__global__ __launch_bounds__(256) void linattn_core_bwd_kernel(const float *__restrict__ qkv, const float *__restrict__ gout,
                                                               int H, int N, float *__restrict__ gqkv) {
  __shared__ float pT[AT * 33], vT[AT * 33], qT[AT * 33], gT[AT * 33]; // [n][row], stride 33
  __shared__ float part[4][1024];
  __shared__ float ctxs[AD * 33], gctxs[AD * 33];
  __shared__ float rmax[AD], rinv[AD], dots[AD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cl = lane & 31, kh = lane >> 5;
  const int h = blockIdx.x, b = blockIdx.y;
  const size_t bs = (size_t)b * 3 * H * AD * N;
  const float *q = qkv + bs + (size_t)(0 * H + h) * AD * N;
  const float *k = qkv + bs + (size_t)(1 * H + h) * AD * N;
  const float *v = qkv + bs + (size_t)(2 * H + h) * AD * N;
  const float *g = gout + ((size_t)b * H + h) * AD * N;
  float *gq = gqkv + bs + (size_t)(0 * H + h) * AD * N;
  float *gk = gqkv + bs + (size_t)(1 * H + h) * AD * N;
  float *gv = gqkv + bs + (size_t)(2 * H + h) * AD * N;

  { // softmax statistics of the 32 rows of k (as the forward)
    const int d = tid >> 3, sub = tid & 7;
    const float *kr = k + (size_t)d * N;
    float m = -INFINITY;
    for (int n = sub; n < N; n += 8) { const float t = kr[n]; m = t > m ? t : m; }
    for (int s = 1; s < 8; s <<= 1) { const float o = __shfl_xor(m, s, 64); m = o > m ? o : m; }
    float sum = 0.f;
    for (int n = sub; n < N; n += 8) sum += expf(kr[n] - m);
    for (int s = 1; s < 8; s <<= 1) sum += __shfl_xor(sum, s, 64);
    if (sub == 0) { rmax[d] = m; rinv[d] = 1.0f / sum; }
  }
  __syncthreads();

  // ctx[d][e] = sum_n p[d][n] v[e][n] and gctx[d][e] = sum_n q[d][n] g[e][n]
  f32x16 acc, gacc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = gacc[i] = 0.f;
  const int tn = tid & 63, d0 = (tid >> 6) * 8;
  for (int n0 = 0; n0 < N; n0 += AT) {
    const int n = n0 + tn;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = d0 + j;
      float pv = 0.f, vv = 0.f, qv = 0.f, gg = 0.f;
      if (n < N) {
        pv = expf(k[(size_t)d * N + n] - rmax[d]) * rinv[d];
        vv = v[(size_t)d * N + n];
        qv = q[(size_t)d * N + n];
        gg = g[(size_t)d * N + n];
      }
      pT[tn * 33 + d] = pv;
      vT[tn * 33 + d] = vv;
      qT[tn * 33 + d] = qv;
      gT[tn * 33 + d] = gg;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int nn = 2 * (wave * 8 + u) + kh;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pT[nn * 33 + cl], vT[nn * 33 + cl], acc, 0, 0, 0);
      gacc = __builtin_amdgcn_mfma_f32_32x32x2f32(qT[nn * 33 + cl], gT[nn * 33 + cl], gacc, 0, 0, 0);
    }
    __syncthreads();
  }
  // the four waves' partial sums in a fixed order, one matrix after the other through the same buffer
#pragma unroll
  for (int i = 0; i < 16; ++i) part[wave][((i & 3) + 8 * (i >> 2) + 4 * kh) * 32 + cl] = acc[i];
  __syncthreads();
  for (int e = tid; e < 1024; e += 256)
    ctxs[(e >> 5) * 33 + (e & 31)] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) part[wave][((i & 3) + 8 * (i >> 2) + 4 * kh) * 32 + cl] = gacc[i];
  __syncthreads();
  for (int e = tid; e < 1024; e += 256)
    gctxs[(e >> 5) * 33 + (e & 31)] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
  __syncthreads();
  if (tid < AD) { // dot[d] = sum_e gctx[d][e] ctx[d][e], ascending e
    float s = 0.f;
    for (int e = 0; e < AD; ++e) s += gctxs[tid * 33 + e] * ctxs[tid * 33 + e];
    dots[tid] = s;
  }
  __syncthreads();

  // per 32-point column block: gq = ctx g, gp = gctx v (rows d, k = e); gv = gctx^T p (rows e, k = d)
  float aq[16], ap[16], av[16];
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    aq[s] = ctxs[cl * 33 + 2 * s + kh];   // A[d = cl][e = 2s + kh]
    ap[s] = gctxs[cl * 33 + 2 * s + kh];
    av[s] = gctxs[(2 * s + kh) * 33 + cl]; // A[e = cl][d = 2s + kh]
  }
  for (int c0 = wave * 32; c0 < N; c0 += 128) {
    const int n = c0 + cl;
    const bool ok = n < N;
    const int nc = ok ? n : N - 1;
    float bg[16], bv[16], bp[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int r_ = 2 * s + kh;
      bg[s] = ok ? g[(size_t)r_ * N + nc] : 0.f;
      bv[s] = ok ? v[(size_t)r_ * N + nc] : 0.f;
      bp[s] = ok ? expf(k[(size_t)r_ * N + nc] - rmax[r_]) * rinv[r_] : 0.f;
    }
    f32x16 oq, op, ov;
#pragma unroll
    for (int i = 0; i < 16; ++i) oq[i] = op[i] = ov[i] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      oq = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[s], bg[s], oq, 0, 0, 0);
      op = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[s], bv[s], op, 0, 0, 0);
      ov = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bp[s], ov, 0, 0, 0);
    }
    if (ok) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = (i & 3) + 8 * (i >> 2) + 4 * kh;
        gq[(size_t)row * N + n] = oq[i];
        gv[(size_t)row * N + n] = ov[i];
        const float pr = expf(k[(size_t)row * N + n] - rmax[row]) * rinv[row];
        gk[(size_t)row * N + n] = pr * (op[i] - dots[row]);
      }
    }
  }
}

} // namespace

extern "C" {

// qkv f32[B, 3*H*32, N] (output of to_qkv, channel order (qkv, head, d)) -> out f32[B, H*32, N] (input of to_out).
int lion_linear_attention_core(const float *qkv, int B, int H, int D, int N, float *out, lionStream_t stream) {
  if (!qkv || !out || B <= 0 || H <= 0 || N <= 0) return LION_EINVAL;
  if (D != AD) return LION_EUNSUPPORTED;
  const bool aligned = ((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int path = lion_internal_linear_attention_path(N, aligned ? 1 : 0);
  const size_t lds = (size_t)(linattn_region_a(path == 1, N) + 2 * ATILE + 2 * AD) * sizeof(float);
  if (path == 1)
    return lion_launch<linattn_core_ahead_kernel<true>>(dim3(H, B), 256, lds, static_cast<hipStream_t>(stream), qkv, H, N, out);
  if (path == 2)
    return lion_launch<linattn_core_ahead_kernel<false>>(dim3(H, B), 256, lds, static_cast<hipStream_t>(stream), qkv, H, N, out);
  return lion_launch<linattn_core_kernel>(dim3(H, B), 256, 0, static_cast<hipStream_t>(stream), qkv, H, N, out);
}
// For tests only: which kernel lion_linear_attention_core takes at N points with (aligned != 0) or without 16-byte aligned
// qkv and out: 0 linattn_core_kernel (the plain form), 1 the resident form, 2 the streaming form.
int lion_internal_linear_attention_path(int N, int aligned) {
  if (N <= 0 || N % 4 != 0 || !aligned) return 0;
  return N <= 1024 ? 1 : 2; // 32 x (N + 4) floats of k beside the staged tiles: 145 KiB of the 160 at N = 1024
}
// For tests only: the same core through linattn_core_kernel whatever the shape.
int lion_internal_linear_attention_core_plain(const float *qkv, int B, int H, int D, int N, float *out, lionStream_t stream) {
  if (!qkv || !out || B <= 0 || H <= 0 || N <= 0) return LION_EINVAL;
  if (D != AD) return LION_EUNSUPPORTED;
  return lion_launch<linattn_core_kernel>(dim3(H, B), 256, 0, static_cast<hipStream_t>(stream), qkv, H, N, out);
}

// gradient of lion_linear_attention_core: qkv as the forward's, gout f32[B, H*32, N] -> gqkv f32[B, 3*H*32, N]
int lion_linear_attention_core_backward(const float *qkv, const float *gout, int B, int H, int D, int N, float *gqkv,
                                        lionStream_t stream) {
  if (!qkv || !gout || !gqkv || B <= 0 || H <= 0 || N <= 0) return LION_EINVAL;
  if (D != AD) return LION_EUNSUPPORTED;
  return lion_launch<linattn_core_bwd_kernel>(dim3(H, B), 256, 0, static_cast<hipStream_t>(stream), qkv, gout, H, N,
                                              gqkv);
}

} // extern "C"
