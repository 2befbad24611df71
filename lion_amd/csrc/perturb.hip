// perturb.hip -- the inputs of guided synthesis, made on the device from clouds resident in HBM:
// points on the surface of a cloud's voxelisation (lion_voxel_surface_points_keyed) and the uniform / outlier corruptions
// (lion_perturb_points_keyed).  Normal noise is lion_chain_diffuse_keyed with m = 1 and has no kernel here.
//
// Every draw is one Philox4x32-10 call under the sample's own key at counter (point index, reserved step word, stream_id), so a
// sample's output depends on neither the batch size nor its position (the contract of the keyed entry points of diffusion.hip).
// All arithmetic on coordinates is one IEEE rounding per written operation (common.h's *_rn helpers); everything that decides
// WHICH face or point is integer arithmetic.  No global atomics, no LDS atomics: the occupancy grid is built from byte flags
// (racing stores all write the same 1) and packed into bits by the thread that owns the word.
#include "common.h"

namespace {

constexpr int VS_BLOCK = 1024;                     // one workgroup per cloud: 16 waves
constexpr int VS_MAX_R = 32;
constexpr int VS_WORDS = VS_MAX_R * VS_MAX_R;   // the rows (x, y) of the largest grid, one 32-bit word each: 1024 = VS_BLOCK
static_assert(VS_WORDS <= VS_BLOCK, "every word has a thread of its own");
constexpr int PT_BLOCK = 256;
constexpr int PT_BOX_BLOCKS = 8;                   // outlier mode: every block folds the whole cloud's box, so at most this many

// (w >> 8) * 2^-24: a multiple of 2^-24 in [0, 1), exact
__device__ __forceinline__ float u24(uint32_t w) { return mul_rn((float)(w >> 8), 5.9604644775390625e-08f); }

__device__ __forceinline__ void point_words(uint64_t n, uint32_t step, uint32_t stream_id, const uint32_t *key, uint32_t w[4]) {
  philox4x32_10((uint32_t)n, (uint32_t)(n >> 32), step, stream_id, key[0], key[1], w);
}

// Per-axis min and max of the cloud p f32[N][3] (N >= 1), folded by the whole block and left in every thread.  min / max are
// exact and commute, so the order of the fold does not matter.  blockDim.x is a multiple of 64, red has a row per wave; the
// block is synchronised on return and red is free again.
__device__ __forceinline__ void cloud_box(const float *__restrict__ p, int N, float (*red)[6], float mn[3], float mx[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) mn[a] = mx[a] = p[a];
  for (size_t n = threadIdx.x; n < (size_t)N; n += blockDim.x) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = p[3 * n + a];
      mn[a] = fminf(mn[a], v);
      mx[a] = fmaxf(mx[a], v);
    }
  }
#pragma unroll
  for (int d = LION_WAVE / 2; d > 0; d >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], d, LION_WAVE));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], d, LION_WAVE));
    }
  }
  const int wave = threadIdx.x / LION_WAVE, waves = blockDim.x / LION_WAVE;
  if (threadIdx.x % LION_WAVE == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { red[wave][a] = mn[a]; red[wave][3 + a] = mx[a]; }
  }
  __syncthreads();
  for (int w = 0; w < waves; ++w) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], red[w][a]); mx[a] = fmaxf(mx[a], red[w][3 + a]); }
  }
  __syncthreads();
}

// ---- points on the surface of the voxelisation ---------------------------------------------------------------------------------
// One workgroup per cloud; the tables live in LDS (41 KB of the CU's 160).  A word is one row of the grid: word x*r + y holds
// the r voxels (x, y, 0 .. r-1) in its low bits, so ascending (word, bit) is ascending flat id x*r*r + y*r + z, the neighbours
// across -z / +z are the word shifted by one bit, and those across y and x the words 1 and r away: thread t makes all six
// exposure masks of word t from five words, without a loop over voxels.
//   buf   32 KB  first a byte flag per (word, bit), then -- the flags are dead once packed -- six exposure masks [f][word]
//   occ    4 KB  the rows' occupancy bits
//   pre    4 KB  per word its count of exposed faces, then the exclusive prefix sum of those counts
// Faces are numbered in ascending (voxel id, f): face j lies in the last word w with pre[w] <= j, there in the last voxel p
// with (faces of the word's voxels below p) <= j - pre[w], and is that voxel's exposed face of that rank.
__global__ void __launch_bounds__(VS_BLOCK) voxel_surface_kernel(const float *__restrict__ x, int N, int r,
                                                                 const uint32_t *__restrict__ keys, uint32_t stream_id, int K,
                                                                 float *__restrict__ out, int32_t *__restrict__ faces_out) {
  __shared__ uint4 buf4[VS_WORDS * 2];
  __shared__ uint32_t occ[VS_WORDS], pre[VS_WORDS];
  __shared__ float red[VS_BLOCK / LION_WAVE][6];
  __shared__ uint32_t wave_total[VS_BLOCK / LION_WAVE];
  uint32_t *buf = reinterpret_cast<uint32_t *>(buf4);
  uint8_t *flags = reinterpret_cast<uint8_t *>(buf4);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid % LION_WAVE, wave = tid / LION_WAVE;
  const float *p = x + (size_t)b * N * 3;
  const int W = r * r;

  // the box: a cube of half-side h around the middle of the points' bounding box
  float mn[3], mx[3], lo[3];
  cloud_box(p, N, red, mn, mx);
  float h = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) h = fmaxf(h, mul_rn(sub_rn(mx[a], mn[a]), 0.5f));
  if (h == 0.f) h = 1.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) lo[a] = sub_rn(mul_rn(add_rn(mn[a], mx[a]), 0.5f), h);
  const float side = mul_rn(2.f, h), s = div_rn(side, (float)r), inv = div_rn((float)r, side);

  // occupancy: a byte flag per voxel (racing stores write the same 1), then thread t packs the 32 flags of word t
  for (int i = tid; i < W * 2; i += VS_BLOCK) buf4[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  for (size_t n = tid; n < (size_t)N; n += VS_BLOCK) {
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int i = (int)floorf(mul_rn(sub_rn(p[3 * n + a], lo[a]), inv));
      c[a] = i < 0 ? 0 : (i > r - 1 ? r - 1 : i);
    }
    flags[(c[0] * r + c[1]) * 32 + c[2]] = 1;
  }
  __syncthreads();
  if (tid < W) {   // four flags (bytes of 0 / 1) -> four bits: the product moves byte k's bit 0 to bit 24 + k
    const uint4 f0 = buf4[2 * tid], f1 = buf4[2 * tid + 1];
    const uint32_t d[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
    uint32_t bits = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) bits |= ((d[q] * 0x01020408u) >> 24) << (4 * q);
    occ[tid] = bits;
  }
  __syncthreads();   // the flags are dead from here: buf becomes the exposure masks

  // exposed faces: f = 0..5 = -x, +x, -y, +y, -z, +z; the neighbour across f is empty or outside the grid
  if (tid < W) {
    const int vx = tid / r, vy = tid - vx * r;
    const uint32_t o = occ[tid];
    uint32_t e[6];
    e[0] = vx > 0 ? o & ~occ[tid - r] : o;
    e[1] = vx < r - 1 ? o & ~occ[tid + r] : o;
    e[2] = vy > 0 ? o & ~occ[tid - 1] : o;
    e[3] = vy < r - 1 ? o & ~occ[tid + 1] : o;
    e[4] = o & ~(o << 1);
    e[5] = o & ~(o >> 1);   // bit r of a row is never set: voxel r-1 sees the outside
    uint32_t cnt = 0;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      buf[f * VS_WORDS + tid] = e[f];
      cnt += __popc(e[f]);
    }
    pre[tid] = cnt;
  }
  __syncthreads();

  // exclusive prefix sum of the words' counts (thread t owns word t) and F, their total
  const uint32_t cnt = tid < W ? pre[tid] : 0u;
  const uint32_t incl = (uint32_t)wave_incl_scan((int)cnt, lane);
  if (lane == LION_WAVE - 1) wave_total[wave] = incl;
  __syncthreads();
  uint32_t before = 0, F = 0;
  for (int w = 0; w < VS_BLOCK / LION_WAVE; ++w) {
    if (w < wave) before += wave_total[w];
    F += wave_total[w];
  }
  if (tid < W) pre[tid] = before + incl - cnt;
  __syncthreads();
  if (tid == 0 && faces_out) faces_out[b] = (int32_t)F;

  const uint32_t *key = keys + 2 * (size_t)b;
  float *o3 = out + (size_t)b * K * 3;
  for (int k = tid; k < K; k += VS_BLOCK) {
    uint32_t w4[4];
    point_words((uint64_t)k, LION_VOXEL_STEP_WORD, stream_id, key, w4);
    const uint32_t j = (uint32_t)(((uint64_t)w4[0] * F) >> 32);
    const float fa = u24(w4[1]), fb = u24(w4[2]);
    int wl = 0, wh = W - 1;
    while (wl < wh) {
      const int mid = (wl + wh + 1) >> 1;
      if (pre[mid] <= j) wl = mid; else wh = mid - 1;
    }
    uint32_t e[6];
#pragma unroll
    for (int f = 0; f < 6; ++f) e[f] = buf[f * VS_WORDS + wl];
    uint32_t rem = j - pre[wl];
    int pl = 0, ph = 31;
    uint32_t below = 0;
    while (pl < ph) {
      const int mid = (pl + ph + 1) >> 1;
      const uint32_t lowbits = (1u << mid) - 1u;
      uint32_t cm = 0;
#pragma unroll
      for (int f = 0; f < 6; ++f) cm += __popc(e[f] & lowbits);
      if (cm <= rem) { pl = mid; below = cm; } else ph = mid - 1;
    }
    rem -= below;
    int face = 0;
#pragma unroll
    for (int f = 5; f >= 0; --f) {   // descending: the last assignment is the lowest f whose rank is rem
      uint32_t rank = 0;
#pragma unroll
      for (int g = 0; g < f; ++g) rank += (e[g] >> pl) & 1u;
      if (((e[f] >> pl) & 1u) && rank == rem) face = f;
    }
    const int vx = wl / r;
    const int c[3] = {vx, wl - vx * r, pl};
    const int axis = face >> 1, first = axis == 0 ? 1 : 0;   // the lower of the two tangential axes takes a, the other b
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float t = a == axis ? (float)(c[a] + (face & 1)) : add_rn((float)c[a], a == first ? fa : fb);
      o3[3 * (size_t)k + a] = add_rn(lo[a], mul_rn(t, s));
    }
  }
}

// ---- uniform noise and outliers ------------------------------------------------------------------------------------------------------
// grid (blocks, B), block-stride over the cloud's points.  MODE 0: out = x + p0*(2u - 1).  MODE 1: where w3 < thr the point
// becomes min + u*(max - min) per axis inside the cloud's own bounding box, else it is copied.
template <int MODE>
__global__ void __launch_bounds__(PT_BLOCK) perturb_kernel(const float *__restrict__ x, int N, float p0, uint32_t thr,
                                                           const uint32_t *__restrict__ keys, uint32_t stream_id,
                                                           float *__restrict__ out) {
  __shared__ float red[PT_BLOCK / LION_WAVE][6];
  const int b = blockIdx.y;
  const float *p = x + (size_t)b * N * 3;
  float *o3 = out + (size_t)b * N * 3;
  const uint32_t *key = keys + 2 * (size_t)b;
  float mn[3] = {0.f, 0.f, 0.f}, ext[3] = {0.f, 0.f, 0.f};
  if (MODE == 1) {
    float mx[3];
    cloud_box(p, N, red, mn, mx);
#pragma unroll
    for (int a = 0; a < 3; ++a) ext[a] = sub_rn(mx[a], mn[a]);
  }
  for (size_t n = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x; n < (size_t)N; n += (size_t)gridDim.x * PT_BLOCK) {
    uint32_t w4[4];
    point_words(n, LION_PERTURB_STEP_WORD, stream_id, key, w4);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = p[3 * n + a], u = u24(w4[a]);
      if (MODE == 0) o3[3 * n + a] = add_rn(v, mul_rn(p0, sub_rn(mul_rn(2.f, u), 1.f)));
      else o3[3 * n + a] = w4[3] < thr ? add_rn(mn[a], mul_rn(u, ext[a])) : v;
    }
  }
}

} // namespace

extern "C" {

size_t lion_voxel_surface_workspace_bytes(int B, int N, int r, int K) {
  (void)B; (void)N; (void)r; (void)K;
  return 0;   // every table of r <= 32 fits the workgroup's LDS
}

int lion_voxel_surface_points_keyed(const float *x, int B, int N, int r, const uint32_t *keys, uint32_t stream_id, int K,
                                    float *out, int32_t *faces_out, void *ws, size_t ws_bytes, lionStream_t stream) {
  if (!x || !keys || !out || B <= 0 || B > 65535 || N <= 0 || K <= 0 || r < 1 || r > VS_MAX_R) return LION_EINVAL;
  const size_t need = lion_voxel_surface_workspace_bytes(B, N, r, K);
  if (ws_bytes < need || (need && !ws)) return LION_EINVAL;
  return lion_launch<voxel_surface_kernel>((unsigned)B, VS_BLOCK, 0, static_cast<hipStream_t>(stream), x, N, r, keys,
                                           stream_id, K, out, faces_out);
}

int lion_perturb_points_keyed(int mode, const float *x, int B, int N, float p0, const uint32_t *keys, uint32_t stream_id,
                              float *out, lionStream_t stream) {
  if (!x || !keys || !out || B <= 0 || B > 65535 || N <= 0 || (mode != 0 && mode != 1)) return LION_EINVAL;
  if (!(p0 >= 0.f) || (mode == 1 && p0 > 1.f)) return LION_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned blocks = (unsigned)((N - 1) / PT_BLOCK + 1);
  if (mode == 0)
    return lion_launch<perturb_kernel<0>>(dim3(blocks, (unsigned)B), PT_BLOCK, 0, st, x, N, p0, 0u, keys, stream_id, out);
  const double t = (double)p0 * 4294967296.0;   // floor(p0 * 2^32), saturated
  const uint32_t thr = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
  return lion_launch<perturb_kernel<1>>(dim3(blocks < PT_BOX_BLOCKS ? blocks : PT_BOX_BLOCKS, (unsigned)B), PT_BLOCK, 0, st, x,
                                        N, p0, thr, keys, stream_id, out);
}

} // extern "C"
