// perturb.hip -- the inputs of guided synthesis, made on the device from clouds resident in HBM:
// points on the surface of a cloud's voxelisation (lion_voxel_surface_points_keyed) and the uniform / outlier corruptions
// (lion_perturb_points_keyed).  Normal noise is lion_chain_diffuse_keyed with m = 1 and has no kernel here.
// The occupancy grid of that voxelisation is also an object of its own: lion_voxel_occupancy writes it,
// lion_voxel_surface_points_grid_keyed draws the surface points of a given grid, lion_voxel_iou compares two grids.  The three
// surface / occupancy kernels are built from the same phases (vs_* below).
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
constexpr int IOU_BLOCK = 256;                     // one workgroup per pair of grids: at most 8 16-byte loads of each per thread
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
// The phases below are shared by voxel_surface_kernel (cloud -> points), voxel_occupancy_kernel (cloud -> grid: box, clear,
// mark, store) and voxel_surface_grid_kernel (grid -> points: load, pack, faces, draw); each is called by the whole block and
// leaves it synchronised where the next phase reads what it wrote.

// the cloud's own frame: the cube of half-side h around the middle of the points' bounding box
__device__ __forceinline__ void own_frame(const float mn[3], const float mx[3], float lo[3], float &side) {
  float h = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) h = fmaxf(h, mul_rn(sub_rn(mx[a], mn[a]), 0.5f));
  if (h == 0.f) h = 1.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) lo[a] = sub_rn(mul_rn(add_rn(mn[a], mx[a]), 0.5f), h);
  side = mul_rn(2.f, h);
}

// per byte of d: 1 where it is non-zero, else 0 (the low seven bits carry into bit 7, which the byte's own bit 7 joins)
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t d) {
  return ((((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u) >> 7;
}

__device__ __forceinline__ void vs_clear(uint4 *buf4, int W) {
  for (int i = threadIdx.x; i < W * 2; i += VS_BLOCK) buf4[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
}

// occupancy: a byte flag per voxel (racing stores write the same 1).  Returns this thread's count of points the clamp moved
// on at least one axis.  Not synchronised on return.  VETTED (the frame is the cloud's own, made by this kernel): the index
// is clamp((int)floorf(.), 0, r-1).  Otherwise the frame came from the device and is not vetted, so the index is clamped as a
// float, before the conversion: whatever lo and inv hold, it lies in 0 .. r-1 -- NaN and everything below 0 go to 0,
// everything above r-1 to r-1; for a finite product both forms give the same index.
template <bool VETTED>
__device__ __forceinline__ int vs_mark(const float *__restrict__ p, int N, int r, const float lo[3], float inv, uint8_t *flags) {
  const float top = (float)(r - 1);
  int moved = 0;
  for (size_t n = threadIdx.x; n < (size_t)N; n += VS_BLOCK) {
    int c[3];
    bool out = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (VETTED) {
        const int i = (int)floorf(mul_rn(sub_rn(p[3 * n + a], lo[a]), inv));
        c[a] = i < 0 ? 0 : (i > r - 1 ? r - 1 : i);
        out |= c[a] != i;
      } else {
        const float t = floorf(mul_rn(sub_rn(p[3 * n + a], lo[a]), inv));
        const bool in = t >= 0.f && t <= top;
        c[a] = in ? (int)t : (t > top ? r - 1 : 0);
        out |= !in;
      }
    }
    flags[(c[0] * r + c[1]) * 32 + c[2]] = 1;
    moved += out ? 1 : 0;
  }
  return moved;
}

// thread t packs the 32 flags (bytes of 0 / 1) of word t: four flags -> four bits, the product moves byte k's bit 0 to bit
// 24 + k.  The flags are dead on return: buf becomes the exposure masks.
__device__ __forceinline__ void vs_pack(const uint4 *buf4, uint32_t *occ, int W) {
  const int tid = threadIdx.x;
  if (tid < W) {
    const uint4 f0 = buf4[2 * tid], f1 = buf4[2 * tid + 1];
    const uint32_t d[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
    uint32_t bits = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) bits |= ((d[q] * 0x01020408u) >> 24) << (4 * q);
    occ[tid] = bits;
  }
  __syncthreads();
}

// exposed faces: f = 0..5 = -x, +x, -y, +y, -z, +z; the neighbour across f is empty or outside the grid.  Writes the six
// masks of every word into buf, the exclusive prefix sum of the words' face counts into pre, and returns F, their total.
__device__ __forceinline__ uint32_t vs_faces(const uint32_t *occ, uint32_t *buf, uint32_t *pre, uint32_t *wave_total, int r) {
  const int tid = threadIdx.x, lane = tid % LION_WAVE, wave = tid / LION_WAVE, W = r * r;
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
  return F;
}

// the K points of one sample: point k is the Philox draw at counter (k, LION_VOXEL_STEP_WORD, stream_id) under key.  Every
// index comes from the tables, none from the frame.  MAY_BE_EMPTY (a given grid; a cloud always has F >= 6): where F = 0 there
// is nothing to search and every point is the frame's centre.
template <bool MAY_BE_EMPTY>
__device__ __forceinline__ void vs_draw(const uint32_t *buf, const uint32_t *pre, uint32_t F, int r, const float lo[3], float s,
                                        float side, const uint32_t *__restrict__ key, uint32_t stream_id, int K,
                                        float *__restrict__ o3) {
  const int W = r * r;
  if (MAY_BE_EMPTY && F == 0) {
    for (int k = threadIdx.x; k < K; k += VS_BLOCK) {
#pragma unroll
      for (int a = 0; a < 3; ++a) o3[3 * (size_t)k + a] = add_rn(lo[a], mul_rn(side, 0.5f));
    }
    return;
  }
  for (int k = threadIdx.x; k < K; k += VS_BLOCK) {
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

__global__ void __launch_bounds__(VS_BLOCK) voxel_surface_kernel(const float *__restrict__ x, int N, int r,
                                                                 const uint32_t *__restrict__ keys, uint32_t stream_id, int K,
                                                                 float *__restrict__ out, int32_t *__restrict__ faces_out) {
  __shared__ uint4 buf4[VS_WORDS * 2];
  __shared__ uint32_t occ[VS_WORDS], pre[VS_WORDS];
  __shared__ float red[VS_BLOCK / LION_WAVE][6];
  __shared__ uint32_t wave_total[VS_BLOCK / LION_WAVE];
  uint32_t *buf = reinterpret_cast<uint32_t *>(buf4);
  const int b = blockIdx.x, W = r * r;
  const float *p = x + (size_t)b * N * 3;

  float mn[3], mx[3], lo[3], side;
  cloud_box(p, N, red, mn, mx);
  own_frame(mn, mx, lo, side);
  const float s = div_rn(side, (float)r), inv = div_rn((float)r, side);

  vs_clear(buf4, W);
  vs_mark<true>(p, N, r, lo, inv, reinterpret_cast<uint8_t *>(buf4));
  __syncthreads();
  vs_pack(buf4, occ, W);
  const uint32_t F = vs_faces(occ, buf, pre, wave_total, r);
  if (threadIdx.x == 0 && faces_out) faces_out[b] = (int32_t)F;
  vs_draw<false>(buf, pre, F, r, lo, s, side, keys + 2 * (size_t)b, stream_id, K, out + (size_t)b * K * 3);
}

// ---- the occupancy grid as an object: cloud -> grid, grid -> points, grid x grid -> IoU ---------------------------------------------
// The grid in HBM is u8[r][r][r] per sample, r bytes per row; the flag slots in LDS are 32 bytes per row.  Both kernels walk
// the flag slots a dword (four voxels z = 4q .. 4q+3 of row j >> 3) at a time; `dwords` (r % 4 == 0 and a 4-byte aligned
// grid: then every row and every sample starts on a dword) moves the grid by dwords too, else it moves by bytes.

// cloud -> grid: box (own frame only), clear, mark, store.  LDS: 32 KB of flags + the box fold's and the count's rows.
__global__ void __launch_bounds__(VS_BLOCK) voxel_occupancy_kernel(const float *__restrict__ x, int N, int r,
                                                                   const float *__restrict__ frame_in, int dwords,
                                                                   uint8_t *__restrict__ grid, float *__restrict__ frame_out,
                                                                   int32_t *__restrict__ clamped_out) {
  __shared__ uint4 buf4[VS_WORDS * 2];
  __shared__ float red[VS_BLOCK / LION_WAVE][6];
  __shared__ int moved_row[VS_BLOCK / LION_WAVE];
  const uint32_t *slots = reinterpret_cast<const uint32_t *>(buf4);
  const int b = blockIdx.x, tid = threadIdx.x, W = r * r;
  const float *p = x + (size_t)b * N * 3;

  float lo[3], side;
  if (frame_in) {
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = frame_in[4 * (size_t)b + a];
    side = frame_in[4 * (size_t)b + 3];
  } else {
    float mn[3], mx[3];
    cloud_box(p, N, red, mn, mx);
    own_frame(mn, mx, lo, side);
  }
  const float inv = div_rn((float)r, side);

  vs_clear(buf4, W);
  int moved = vs_mark<false>(p, N, r, lo, inv, reinterpret_cast<uint8_t *>(buf4));
#pragma unroll
  for (int d = LION_WAVE / 2; d > 0; d >>= 1) moved += __shfl_xor(moved, d, LION_WAVE);
  if (tid % LION_WAVE == 0) moved_row[tid / LION_WAVE] = moved;
  __syncthreads();

  uint8_t *g = grid + (size_t)b * W * r;
  for (int j = tid; j < W * 8; j += VS_BLOCK) {
    const int row = j >> 3, q = j & 7;
    if (4 * q >= r) continue;
    const uint32_t d = slots[j];
    if (dwords) {
      reinterpret_cast<uint32_t *>(g)[row * (r >> 2) + q] = d;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * q + k < r) g[row * r + 4 * q + k] = (uint8_t)((d >> (8 * k)) & 0xFFu);
    }
  }
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < VS_BLOCK / LION_WAVE; ++w) total += moved_row[w];
    if (clamped_out) clamped_out[b] = total;
    if (frame_out) {
#pragma unroll
      for (int a = 0; a < 3; ++a) frame_out[4 * (size_t)b + a] = lo[a];
      frame_out[4 * (size_t)b + 3] = side;
    }
  }
}

// grid -> points: the grid's bytes, normalised to 0 / 1, into the flag slots (the slots past z = r-1 are written 0: no clear
// pass), then pack, faces, draw as in voxel_surface_kernel.  LDS: its tables without the box fold's rows (40 KB).
__global__ void __launch_bounds__(VS_BLOCK) voxel_surface_grid_kernel(const uint8_t *__restrict__ grid,
                                                                      const float *__restrict__ frame, int r, int dwords,
                                                                      const uint32_t *__restrict__ keys, uint32_t stream_id,
                                                                      int K, float *__restrict__ out,
                                                                      int32_t *__restrict__ faces_out) {
  __shared__ uint4 buf4[VS_WORDS * 2];
  __shared__ uint32_t occ[VS_WORDS], pre[VS_WORDS];
  __shared__ uint32_t wave_total[VS_BLOCK / LION_WAVE];
  uint32_t *buf = reinterpret_cast<uint32_t *>(buf4);
  const int b = blockIdx.x, tid = threadIdx.x, W = r * r;
  const uint8_t *g = grid + (size_t)b * W * r;

  for (int j = tid; j < W * 8; j += VS_BLOCK) {
    const int row = j >> 3, q = j & 7;
    uint32_t d = 0;
    if (dwords) {
      if (4 * q < r) d = reinterpret_cast<const uint32_t *>(g)[row * (r >> 2) + q];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (4 * q + k < r) d |= (uint32_t)g[row * r + 4 * q + k] << (8 * k);
    }
    buf[j] = nonzero_bytes(d);
  }
  __syncthreads();
  vs_pack(buf4, occ, W);
  const uint32_t F = vs_faces(occ, buf, pre, wave_total, r);
  if (tid == 0 && faces_out) faces_out[b] = (int32_t)F;

  float lo[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) lo[a] = frame[4 * (size_t)b + a];
  const float side = frame[4 * (size_t)b + 3], s = div_rn(side, (float)r);
  vs_draw<true>(buf, pre, F, r, lo, s, side, keys + 2 * (size_t)b, stream_id, K, out + (size_t)b * K * 3);
}

// grid x grid -> |A and B|, |A or B| over n = r^3 voxels and their quotient.  16-byte loads where both samples' bytes can
// be read that way: n is a multiple of 16 only for r % 4 == 0 (r = 4k: n = 64 k^3) and a sample starts n bytes after the last,
// so the bytes before the first 16-byte boundary and after the last go one at a time; if the two grids sit differently
// against that boundary, all of them do.  Integer sums: shuffles inside a wave, a row per wave in LDS, thread 0 adds the rows.
__global__ void __launch_bounds__(IOU_BLOCK) voxel_iou_kernel(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int n,
                                                              int32_t *__restrict__ counts, float *__restrict__ iou) {
  __shared__ int rows[IOU_BLOCK / LION_WAVE][2];
  const int tid = threadIdx.x;
  const uint8_t *pa = a + (size_t)blockIdx.x * n, *pb = b + (size_t)blockIdx.x * n;
  const int ma = (int)(reinterpret_cast<uintptr_t>(pa) & 15u), mb = (int)(reinterpret_cast<uintptr_t>(pb) & 15u);
  int head = ma == mb ? (16 - ma) & 15 : n;
  if (head > n) head = n;
  const int vecs = (n - head) >> 4, tail = head + 16 * vecs;
  int inter = 0, uni = 0;
  for (int i = tid; i < head; i += IOU_BLOCK) {
    const int u = pa[i] != 0, v = pb[i] != 0;
    inter += u & v;
    uni += u | v;
  }
  const uint4 *va = reinterpret_cast<const uint4 *>(pa + head), *vb = reinterpret_cast<const uint4 *>(pb + head);
  for (int i = tid; i < vecs; i += IOU_BLOCK) {
    const uint4 u4 = va[i], v4 = vb[i];
    const uint32_t u[4] = {u4.x, u4.y, u4.z, u4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t nu = nonzero_bytes(u[q]), nv = nonzero_bytes(v[q]);
      inter += __popc(nu & nv);
      uni += __popc(nu | nv);
    }
  }
  for (int i = tail + tid; i < n; i += IOU_BLOCK) {
    const int u = pa[i] != 0, v = pb[i] != 0;
    inter += u & v;
    uni += u | v;
  }
#pragma unroll
  for (int d = LION_WAVE / 2; d > 0; d >>= 1) {
    inter += __shfl_xor(inter, d, LION_WAVE);
    uni += __shfl_xor(uni, d, LION_WAVE);
  }
  if (tid % LION_WAVE == 0) { rows[tid / LION_WAVE][0] = inter; rows[tid / LION_WAVE][1] = uni; }
  __syncthreads();
  if (tid == 0) {
    int si = 0, su = 0;
    for (int w = 0; w < IOU_BLOCK / LION_WAVE; ++w) { si += rows[w][0]; su += rows[w][1]; }
    counts[2 * (size_t)blockIdx.x] = si;
    counts[2 * (size_t)blockIdx.x + 1] = su;
    if (iou) iou[blockIdx.x] = su == 0 ? 1.f : div_rn((float)si, (float)su);
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

// r % 4 == 0 and a 4-byte aligned base: every row (r bytes) and every sample (r^3 bytes) of the grid starts on a dword
static int grid_moves_by_dwords(const void *grid, int r) { return r % 4 == 0 && (reinterpret_cast<uintptr_t>(grid) & 3u) == 0; }

int lion_voxel_occupancy(const float *x, int B, int N, int r, const float *frame_in, uint8_t *grid, float *frame_out,
                         int32_t *clamped_out, lionStream_t stream) {
  if (!x || !grid || B <= 0 || B > 65535 || N <= 0 || r < 1 || r > VS_MAX_R) return LION_EINVAL;
  return lion_launch<voxel_occupancy_kernel>((unsigned)B, VS_BLOCK, 0, static_cast<hipStream_t>(stream), x, N, r, frame_in,
                                             grid_moves_by_dwords(grid, r), grid, frame_out, clamped_out);
}

int lion_voxel_surface_points_grid_keyed(const uint8_t *grid, const float *frame, int B, int r, const uint32_t *keys,
                                         uint32_t stream_id, int K, float *out, int32_t *faces_out, lionStream_t stream) {
  if (!grid || !frame || !keys || !out || B <= 0 || B > 65535 || K <= 0 || r < 1 || r > VS_MAX_R) return LION_EINVAL;
  return lion_launch<voxel_surface_grid_kernel>((unsigned)B, VS_BLOCK, 0, static_cast<hipStream_t>(stream), grid, frame, r,
                                                grid_moves_by_dwords(grid, r), keys, stream_id, K, out, faces_out);
}

int lion_voxel_iou(const uint8_t *a, const uint8_t *b, int B, int r, int32_t *counts, float *iou, lionStream_t stream) {
  if (!a || !b || !counts || B <= 0 || B > 65535 || r < 1 || r > VS_MAX_R) return LION_EINVAL;
  return lion_launch<voxel_iou_kernel>((unsigned)B, IOU_BLOCK, 0, static_cast<hipStream_t>(stream), a, b, r * r * r, counts,
                                       iou);
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
