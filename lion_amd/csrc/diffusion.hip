// diffusion.hip -- D1: one fused elementwise kernel per denoiser update.
//
// Reference: utils/diffusion_pvd.py:451-467 (DDIM: ~6 ATen launches + a host->device noise copy
// per step) and :283-296 with get_q_posterior_mean :475-486 (DDPM ancestral step).
// The scalar coefficients are computed on the host exactly as the reference computes them
// (fp32 0-d tensor arithmetic); the kernel applies them in the reference's operation order with
// one rounding per operation, so the update is bit-exact versus the oracle for identical inputs.
// x is [B, 8192] or [B, 128] floats: launch-latency bound, hence a single launch, float4 lanes.
#include "common.h"

namespace {

__device__ __forceinline__ float ddim1(float x, float e, float z, float s, float c, float sigma) {
  // x = x_noisy*sqrt(a_next/a_t);  x += c*eps + sigma*randn
  return add_rn(mul_rn(x, s), add_rn(mul_rn(c, e), mul_rn(sigma, z)));
}

__global__ void ddim_kernel(const float *__restrict__ x, const float *__restrict__ eps,
                            const float *__restrict__ z, size_t numel, float s, float c,
                            float sigma, float *__restrict__ out) {
  const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 3 < numel) {
    const float4 xv = *reinterpret_cast<const float4 *>(x + i);
    const float4 ev = *reinterpret_cast<const float4 *>(eps + i);
    float4 zv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (z) zv = *reinterpret_cast<const float4 *>(z + i);
    *reinterpret_cast<float4 *>(out + i) =
        make_float4(ddim1(xv.x, ev.x, zv.x, s, c, sigma), ddim1(xv.y, ev.y, zv.y, s, c, sigma),
                    ddim1(xv.z, ev.z, zv.z, s, c, sigma), ddim1(xv.w, ev.w, zv.w, s, c, sigma));
  } else {
    for (size_t j = i; j < numel; ++j) out[j] = ddim1(x[j], eps[j], z ? z[j] : 0.f, s, c, sigma);
  }
}

__global__ void ddpm_kernel(const float *__restrict__ x, const float *__restrict__ eps,
                            const float *__restrict__ z, size_t numel, int t_is_zero, float k_outer,
                            float k_a, float k_b, float scale, float temp, float *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numel) return;
  if (t_is_zero) { // :479-480
    out[i] = mul_rn(k_outer, sub_rn(x[i], mul_rn(k_a, eps[i])));
  } else {         // :482-484, then :293-294
    const float mean = mul_rn(k_outer, sub_rn(x[i], div_rn(mul_rn(k_a, eps[i]), k_b)));
    out[i] = add_rn(mean, mul_rn(mul_rn(scale, z[i]), temp));
  }
}


// ---- whole-chain replay: device-resident step state + on-chip noise -----------------------------------------
// A sampling chain is 1000 replays of ONE captured graph [begin_step -> denoiser forward -> update_noise]; nothing
// a step needs may come from the host.  The schedule lives in a device table (8 floats per step:
// {t_model, a0..a5, -}); begin_step reads the step counter, broadcasts t to the denoiser's [B] timestep input,
// copies the step's coefficients to `cur` (cur[7] = the step index, as bits) and advances the counter.  The
// update kernel draws z ~ N(0,1) itself: Philox4x32-10 keyed by the chain's 64-bit seed, counter = (quad index,
// step, stream id) -- the seed is read from device memory so that a captured graph serves every chain --, four uniforms -> two Box-Muller pairs per float4 -- the reference draws the noise on the CPU
// and copies it to the device every step (diffusion_pvd.py:465-466).  Algorithmic bytes per step: x, eps in,
// x out (3*4*numel).
__device__ __forceinline__ float u01(uint32_t x) { // (0, 1]: x * 2^-32 + 2^-33, two roundings
  return add_rn(mul_rn((float)x, 2.3283064365386963e-10f), 1.1641532182693481e-10f);
}

__device__ __forceinline__ void normal4(uint64_t quad, uint32_t step, uint32_t stream_id, uint64_t seed, float z[4]) {
  uint32_t r[4];
  philox4x32_10((uint32_t)quad, (uint32_t)(quad >> 32), step, stream_id, (uint32_t)seed, (uint32_t)(seed >> 32), r);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float rad = sqrtf(mul_rn(-2.0f, logf(u01(r[2 * h]))));
    float sn, cs;
    sincospif(mul_rn(2.0f, u01(r[2 * h + 1])), &sn, &cs);
    z[2 * h] = mul_rn(rad, cs);
    z[2 * h + 1] = mul_rn(rad, sn);
  }
}

// ---- quad I/O: lane q of an update kernel owns elements i = 4q .. 4q+3 of every flat tensor ------------------------------
// `full`: the quad lies below numel and the pointer is 16-byte aligned -> one 16-byte access; else element by element, the
// elements at or past numel read as 0 and are not written.
__device__ __forceinline__ void load_quad(const float *p, size_t i, size_t numel, bool full, float v[4]) {
  if (full) {
    const float4 t = *reinterpret_cast<const float4 *>(p + i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    for (int j = 0; j < 4; ++j) v[j] = i + j < numel ? p[i + j] : 0.f;
  }
}

// ---- which quad a lane owns, and which Philox (counter, key) draws its noise ------------------------------------------------
// Unkeyed (one 64-bit key per chain): a 1-D grid over the flat tensor; lane q owns quad q, and q is also the counter's quad word.
// KEYED (one key per sample, keys = u32[2*B]): grid.y is the sample b, grid.x walks that sample's own `sample_quads` = n/4 quads
// (n % 4 == 0: no quad straddles two samples, every quad is full); the counter's quad word is j, the quad's index WITHIN the
// sample, under keys[b] -- what the unkeyed kernel draws for a one-sample tensor of n elements under that key, whatever B, b
// and the other keys are.  No division.  False: the lane owns nothing.  `key` is only pointed at, not read.
template <bool KEYED>
__device__ __forceinline__ bool own_quad(size_t numel, uint32_t sample_quads, const uint32_t *words, size_t &q, uint64_t &ctr,
                                         const uint32_t *&key) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (KEYED) {
    if (t >= sample_quads) return false;
    q = (size_t)blockIdx.y * sample_quads + t;
    key = words + 2 * (size_t)blockIdx.y;
  } else {
    if (t * 4 >= numel) return false;
    q = t;
    key = words;
  }
  ctr = t;
  return true;
}

// eps is flat like x, or (cm_points = N != 0) the denoiser's channel-major output [B][4][N] beside the point-major latent
// x [B][N][4]: quad q = (b, n) takes its four channels from four rows -- the permute(0, 2, 1).contiguous() copy of the model's
// output folded into this read.  numel = B*N*4 there: every quad is full.  KEYED: (b, n) = (grid.y, ctr), as own_quad left them.
template <bool KEYED>
__device__ __forceinline__ void load_eps_quad(const float *eps, size_t q, size_t ctr, size_t numel, bool full, int cm_points,
                                              float v[4]) {
  if (cm_points) {
    const size_t b = KEYED ? (size_t)blockIdx.y : q / (size_t)cm_points;
    const size_t n = KEYED ? ctr : q - b * (size_t)cm_points;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = eps[(b * 4 + j) * (size_t)cm_points + n];
  } else {
    load_quad(eps, q * 4, numel, full, v);
  }
}

__device__ __forceinline__ void store_quad(float *p, size_t i, size_t numel, bool full, const float v[4]) {
  if (full) {
    *reinterpret_cast<float4 *>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int j = 0; j < 4 && i + j < numel; ++j) p[i + j] = v[j];
  }
}

__global__ void begin_step_kernel(const float *__restrict__ table, int n_steps, int32_t *counter,
                                  float *__restrict__ t_out, int B, float *__restrict__ cur,
                                  const float *__restrict__ temb_table, int temb_width, float *__restrict__ temb_out) {
  __shared__ int step;
  if (threadIdx.x == 0) {
    int i = *counter;
    i = i < 0 ? 0 : (i >= n_steps ? n_steps - 1 : i);
    step = i;
  }
  __syncthreads();
  const int i = step;
  const float *row = table + (size_t)i * 8;
  for (int b = threadIdx.x; b < B; b += blockDim.x) t_out[b] = row[0];
  if (threadIdx.x < 7) cur[threadIdx.x] = row[threadIdx.x];
  if (threadIdx.x == 7) cur[7] = __int_as_float(i);
  if (threadIdx.x == 0) *counter = i + 1;
  if (temb_table)   // the step's row of the chain's time-embedding table (was an ATen index_select per step)
    for (int k = threadIdx.x; k < temb_width; k += blockDim.x) temb_out[k] = temb_table[(size_t)i * temb_width + k];
}

// MODE 0: DDIM  out = x*a0 + (a1*eps + a2*z)                     (a = {s, c, sigma})
// MODE 1: DDPM  a5 != 0 (t == 0): out = a0*(x - a1*eps);  else out = a0*(x - a1*eps/a2) + (a3*z)*a4
// one quad of it with a0..a5 = cur[1..6]: the arithmetic of every update_noise kernel
template <int MODE>
__device__ __forceinline__ void update_quad(const float xv[4], const float ev[4], const float z[4], float a0, float a1, float a2,
                                            float a3, float a4, float a5, float o[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (MODE == 0) {
      o[j] = ddim1(xv[j], ev[j], z[j], a0, a1, a2);
    } else if (a5 != 0.f) {
      o[j] = mul_rn(a0, sub_rn(xv[j], mul_rn(a1, ev[j])));
    } else {
      o[j] = add_rn(mul_rn(a0, sub_rn(xv[j], div_rn(mul_rn(a1, ev[j]), a2))), mul_rn(mul_rn(a3, z[j]), a4));
    }
  }
}

// `step` is the counter's step word: cur[7], the row's index, but in the per-sample-start form below.
template <int MODE, bool KEYED>
__device__ __forceinline__ void update_noise_body(const float *__restrict__ x, const float *__restrict__ eps, size_t numel,
                                                  uint32_t sample_quads, const float *__restrict__ cur,
                                                  const uint32_t *__restrict__ seed_words, uint32_t step, uint32_t stream_id,
                                                  float *__restrict__ out, float *__restrict__ z_out, int cm_points) {
  size_t q;
  uint64_t ctr;
  const uint32_t *key;
  if (!own_quad<KEYED>(numel, sample_quads, seed_words, q, ctr, key)) return;
  const size_t i = q * 4;
  const float a0 = cur[1], a1 = cur[2], a2 = cur[3], a3 = cur[4], a4 = cur[5], a5 = cur[6];
  const uint64_t seed = (uint64_t)key[0] | ((uint64_t)key[1] << 32);
  float z[4];
  normal4(ctr, step, stream_id, seed, z);
  float xv[4], ev[4], o[4];
  const bool full = i + 3 < numel;
  load_quad(x, i, numel, full, xv);
  load_eps_quad<KEYED>(eps, q, ctr, numel, full, cm_points, ev);
  update_quad<MODE>(xv, ev, z, a0, a1, a2, a3, a4, a5, o);
  store_quad(out, i, numel, full, o);
  if (z_out) store_quad(z_out, i, numel, full, z);
}

template <int MODE>
__global__ void update_noise_kernel(const float *__restrict__ x, const float *__restrict__ eps, size_t numel,
                                    const float *__restrict__ cur, const uint32_t *__restrict__ seed_words,
                                    uint32_t stream_id, float *__restrict__ out, float *__restrict__ z_out, int cm_points) {
  update_noise_body<MODE, false>(x, eps, numel, 0, cur, seed_words, (uint32_t)__float_as_int(cur[7]), stream_id, out, z_out,
                                 cm_points);
}

// the keyed form: grid (ceil(sample_quads / 256), B), keys u32[2*B]
template <int MODE>
__global__ void update_noise_keyed_kernel(const float *__restrict__ x, const float *__restrict__ eps, size_t numel,
                                          uint32_t sample_quads, const float *__restrict__ cur,
                                          const uint32_t *__restrict__ keys, uint32_t stream_id, float *__restrict__ out,
                                          float *__restrict__ z_out, int cm_points) {
  update_noise_body<MODE, true>(x, eps, numel, sample_quads, cur, keys, (uint32_t)__float_as_int(cur[7]), stream_id, out, z_out,
                                cm_points);
}

// a sample that an "_at" / "_from" kernel leaves alone: out = x bit for bit (nothing is stored where out IS x), z_out = 0;
// nothing is drawn and no key is read.  `full` as in load_quad: a keyed quad always lies below numel.
__device__ __forceinline__ void hold_quad(const float *x, size_t numel, uint32_t sample_quads, bool full, float *out,
                                          float *z_out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // own_quad<true>'s quad, without a key
  if (t >= sample_quads) return;
  const size_t i = ((size_t)blockIdx.y * sample_quads + t) * 4;
  if (out != x) {
    float v[4];
    load_quad(x, i, numel, full, v);
    store_quad(out, i, numel, full, v);
  }
  if (z_out) {
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    store_quad(z_out, i, numel, full, zero);
  }
}

// the keyed form with a first row per sample (first_row i32[B]): at row i = cur[7], sample b = blockIdx.y is held where
// i < first_row[b] and else takes the keyed update with the row's coefficients under step word i - first_row[b] -- its own row
// count.  One sample per grid.y: the branch is uniform per workgroup.  x and out are not __restrict__ here: they are compared.
template <int MODE>
__global__ void update_noise_keyed_from_kernel(const float *x, const float *__restrict__ eps, size_t numel,
                                               uint32_t sample_quads, const float *__restrict__ cur,
                                               const int32_t *__restrict__ first_row, const uint32_t *__restrict__ keys,
                                               uint32_t stream_id, float *out, float *z_out, int cm_points) {
  const int32_t local = __float_as_int(cur[7]) - first_row[blockIdx.y];
  if (local < 0) {
    hold_quad(x, numel, sample_quads, true, out, z_out);
    return;
  }
  update_noise_body<MODE, true>(x, eps, numel, sample_quads, cur, keys, (uint32_t)local, stream_id, out, z_out, cm_points);
}

// the per-sample-start form with a known region (RePaint's conditioning, Lugmayr et al. 2022, Algorithm 1 without its jumps):
// keep u8[B][sample_quads] marks the quads whose clean value known_x0 is given.  A sample below its first row is held as above,
// kept quads included.  Else a quad that is not kept takes the "_from" update (step word local, stream_id), and a kept one the
// forward draw of its clean value at the level the state has after this row, (m, s) = known_ms[row]: out = m*x0 + s*z' with
// diffuse_body's arithmetic, z' at counter (j, local, known_stream_id) -- or, where s == 0 (the last row), out = x0 bit for
// bit, nothing drawn, z_out = 0.  A kept quad reads neither x nor eps.  first_row NULL: every sample starts at row 0.
// The mask is per lane: a wave with both kinds runs the one draw below once and then each kind's loads and arithmetic.
// RESAMPLE (RePaint's resampling jumps, composed: DESIGN.md 4.6.11): row i may end with a forward move of the state,
// (mf, sf) = known_jump[row].  Where sf != 0 a quad that is not kept goes on from its update o to mf*o + sf*z'' with the same
// arithmetic, z'' at counter (j, local, resample_stream_id); z_out keeps the step's own z.  Kept quads are as above: known_ms
// already holds the level behind the jump.  sf is one value per row, so the branch is uniform.  Without RESAMPLE neither
// known_jump nor resample_stream_id is read.
template <int MODE, bool RESAMPLE>
__global__ void update_noise_keyed_known_kernel(const float *x, const float *__restrict__ eps, size_t numel,
                                                uint32_t sample_quads, const float *__restrict__ cur,
                                                const int32_t *__restrict__ first_row, const uint32_t *__restrict__ keys,
                                                uint32_t stream_id, const float *__restrict__ known_x0,
                                                const uint8_t *__restrict__ keep, const float *__restrict__ known_ms,
                                                uint32_t known_stream_id, const float *__restrict__ known_jump,
                                                uint32_t resample_stream_id, float *out, float *z_out, int cm_points) {
  const int32_t row = __float_as_int(cur[7]);
  const int32_t local = first_row ? row - first_row[blockIdx.y] : row;
  if (local < 0) {
    hold_quad(x, numel, sample_quads, true, out, z_out);
    return;
  }
  size_t q;
  uint64_t ctr;
  const uint32_t *key;
  if (!own_quad<true>(numel, sample_quads, keys, q, ctr, key)) return;
  const size_t i = q * 4;
  const bool kept = keep[q] != 0;
  const float m = known_ms[2 * (size_t)row], s = known_ms[2 * (size_t)row + 1];
  float z[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
  if (!kept || s != 0.f)
    normal4(ctr, (uint32_t)local, kept ? known_stream_id : stream_id, (uint64_t)key[0] | ((uint64_t)key[1] << 32), z);
  if (kept) {
    load_quad(known_x0, i, numel, true, o);
    if (s != 0.f) {
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = add_rn(mul_rn(m, o[j]), mul_rn(s, z[j]));
    }
  } else {
    float xv[4], ev[4];
    load_quad(x, i, numel, true, xv);
    load_eps_quad<true>(eps, q, ctr, numel, true, cm_points, ev);
    update_quad<MODE>(xv, ev, z, cur[1], cur[2], cur[3], cur[4], cur[5], cur[6], o);
    if constexpr (RESAMPLE) {
      const float mf = known_jump[2 * (size_t)row], sf = known_jump[2 * (size_t)row + 1];
      if (sf != 0.f) {
        float zr[4];
        normal4(ctr, (uint32_t)local, resample_stream_id, (uint64_t)key[0] | ((uint64_t)key[1] << 32), zr);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = add_rn(mul_rn(mf, o[j]), mul_rn(sf, zr[j]));
      }
    }
  }
  store_quad(out, i, numel, true, o);
  if (z_out) store_quad(z_out, i, numel, true, z);
}

// out[b][.] = z alone: sample b's draw at counter (j, step, stream_id) under keys[b] -- the start latent of a keyed chain
// (LION_START_STEP_WORD), the reparameterisation draws, the per-step noise of the eager loops
__global__ void normal_keyed_kernel(const uint32_t *__restrict__ keys, size_t numel, uint32_t sample_quads, uint32_t step,
                                    uint32_t stream_id, float *__restrict__ out) {
  size_t q;
  uint64_t ctr;
  const uint32_t *key;
  if (!own_quad<true>(numel, sample_quads, keys, q, ctr, key)) return;
  float z[4];
  normal4(ctr, step, stream_id, (uint64_t)key[0] | ((uint64_t)key[1] << 32), z);
  store_quad(out, q * 4, numel, true, z);
}

// ---- host side of the quad kernels ---------------------------------------------------------------------------------------
// every pointer is 16-byte aligned (torch allocations are 256-byte aligned); NULL counts as aligned
static bool aligned16(std::initializer_list<const void *> ptrs) {
  uintptr_t bits = 0;
  for (const void *p : ptrs) bits |= (uintptr_t)p;
  return (bits & 15) == 0;
}

// numel elements, one quad per lane, 256 lanes per block: LION_OK and the grid, or LION_EINVAL (no elements, or more blocks
// than a grid's x dimension holds)
static int quad_blocks(size_t numel, unsigned *blocks) {
  const size_t quads = (numel + 3) / 4, n = (quads + 255) / 256;
  if (numel == 0 || n > 0x7fffffffu) return LION_EINVAL;
  *blocks = (unsigned)n;
  return LION_OK;
}

// B samples of n elements, one key each: LION_OK, the grid (x over a sample's quads, y = sample) and n/4, or LION_EINVAL
// (B <= 0, n <= 0, n % 4 != 0 -- a quad would straddle two samples --, or more samples than a grid's y dimension holds)
static int keyed_grid(int B, int n, dim3 *grid, uint32_t *sample_quads) {
  if (B <= 0 || n <= 0 || n % 4 != 0 || B > 65535) return LION_EINVAL;
  *sample_quads = (uint32_t)(n / 4);
  *grid = dim3((*sample_quads + 255) / 256, (unsigned)B);
  return LION_OK;
}

// first_row: NULL for the plain keyed form, else the per-sample-start form on the same grid
static int update_noise_keyed_launch(int mode, hipStream_t st, const float *x, const float *eps, int B, int n, const float *cur,
                                     const int32_t *first_row, const uint32_t *keys, uint32_t stream_id, float *out,
                                     float *z_out, int cm_points) {
  dim3 grid;
  uint32_t sq;
  if (keyed_grid(B, n, &grid, &sq) != LION_OK) return LION_EINVAL;
  const size_t numel = (size_t)B * n;
  if (first_row)
    return mode == 0 ? lion_launch<update_noise_keyed_from_kernel<0>>(grid, 256, 0, st, x, eps, numel, sq, cur, first_row, keys,
                                                                      stream_id, out, z_out, cm_points)
                     : lion_launch<update_noise_keyed_from_kernel<1>>(grid, 256, 0, st, x, eps, numel, sq, cur, first_row, keys,
                                                                      stream_id, out, z_out, cm_points);
  return mode == 0 ? lion_launch<update_noise_keyed_kernel<0>>(grid, 256, 0, st, x, eps, numel, sq, cur, keys, stream_id, out,
                                                               z_out, cm_points)
                   : lion_launch<update_noise_keyed_kernel<1>>(grid, 256, 0, st, x, eps, numel, sq, cur, keys, stream_id, out,
                                                               z_out, cm_points);
}

// the known-region form on the same grid; first_row may be NULL here.  known_jump NULL: the form without resampling jumps
static int update_noise_known_launch(int mode, hipStream_t st, const float *x, const float *eps, int B, int n, const float *cur,
                                     const int32_t *first_row, const uint32_t *keys, uint32_t stream_id, const float *known_x0,
                                     const uint8_t *keep, const float *known_ms, uint32_t known_stream_id,
                                     const float *known_jump, uint32_t resample_stream_id, float *out, float *z_out,
                                     int cm_points) {
  dim3 grid;
  uint32_t sq;
  if (keyed_grid(B, n, &grid, &sq) != LION_OK) return LION_EINVAL;
  const size_t numel = (size_t)B * n;
#define LION_KNOWN_LAUNCH(MODE, RESAMPLE)                                                                                      \
  lion_launch<update_noise_keyed_known_kernel<MODE, RESAMPLE>>(grid, 256, 0, st, x, eps, numel, sq, cur, first_row, keys,      \
                                                               stream_id, known_x0, keep, known_ms, known_stream_id,           \
                                                               known_jump, resample_stream_id, out, z_out, cm_points)
  if (known_jump) return mode == 0 ? LION_KNOWN_LAUNCH(0, true) : LION_KNOWN_LAUNCH(1, true);
  return mode == 0 ? LION_KNOWN_LAUNCH(0, false) : LION_KNOWN_LAUNCH(1, false);
#undef LION_KNOWN_LAUNCH
}

static int update_noise_launch(int mode, hipStream_t st, const float *x, const float *eps, size_t numel,
                               const float *cur, const uint32_t *seed, uint32_t stream_id, float *out, float *z_out,
                               int cm_points) {
  unsigned blocks;
  if (quad_blocks(numel, &blocks) != LION_OK) return LION_EINVAL;
  return mode == 0 ? lion_launch<update_noise_kernel<0>>(blocks, 256, 0, st, x, eps, numel, cur, seed, stream_id, out, z_out,
                                                         cm_points)
                   : lion_launch<update_noise_kernel<1>>(blocks, 256, 0, st, x, eps, numel, cur, seed, stream_id, out, z_out,
                                                         cm_points);
}

// DPM-Solver++(2M) (Lu et al. 2022, Algorithm 2) in data-prediction form, one rounding per written operation:
//   x0 = a0*(x - a1*eps);   D = a5 == 0 ? a4*x0 : a4*x0 + a5*hist;   out = a2*x + a3*D;   hist_out = x0
// (a = {1/alpha_t, sigma_t, sigma_n/sigma_t, -alpha_n*expm1(-h), 1 + 1/(2r), -1/(2r)}).  hist is NOT read when a5 == 0 (first
// step, order 1, last step): it may then be NULL or hold anything.  The tensors are not __restrict__: out may alias x and
// hist_out may alias hist (a lane reads every quad it needs before its first store, no lane reads another's).
// NOISE (the stochastic form below): out gains + a6*z where a6 != 0; without it z_in, a6, the seed, step, stream_id and z_out
// are not looked at and nothing of that path is compiled in.
// KEYED: own_quad's per-sample counters and keys (seed_words = keys u32[2*B]; sample_quads = n/4, else unused).
template <bool NOISE, bool KEYED = false>
__device__ __forceinline__ void multistep_body(const float *x, const float *eps, const float *hist, const float *z_in,
                                               size_t numel, float a0, float a1, float a2, float a3, float a4, float a5,
                                               float a6, const uint32_t *__restrict__ seed_words, uint32_t step,
                                               uint32_t stream_id, float *out, float *hist_out, float *z_out, int cm_points,
                                               uint32_t sample_quads = 0) {
  size_t q;
  uint64_t ctr;
  const uint32_t *key;
  if (!own_quad<KEYED>(numel, sample_quads, seed_words, q, ctr, key)) return;
  const size_t i = q * 4;
  const bool second = a5 != 0.f, noisy = NOISE && a6 != 0.f;
  float xv[4], ev[4], hv[4] = {0.f, 0.f, 0.f, 0.f}, z[4] = {0.f, 0.f, 0.f, 0.f}, o[4], p[4];
  const bool full = i + 3 < numel;
  load_quad(x, i, numel, full, xv);
  if (second) load_quad(hist, i, numel, full, hv);
  load_eps_quad<KEYED>(eps, q, ctr, numel, full, cm_points, ev);
  if (noisy) {
    if (z_in) {
      load_quad(z_in, i, numel, full, z);
    } else {
      const uint64_t seed = (uint64_t)key[0] | ((uint64_t)key[1] << 32);
      normal4(ctr, step, stream_id, seed, z);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    p[j] = mul_rn(a0, sub_rn(xv[j], mul_rn(a1, ev[j])));
    float d = mul_rn(a4, p[j]);
    if (second) d = add_rn(d, mul_rn(a5, hv[j]));
    o[j] = add_rn(mul_rn(a2, xv[j]), mul_rn(a3, d));
    if (noisy) o[j] = add_rn(o[j], mul_rn(a6, z[j]));
  }
  store_quad(out, i, numel, full, o);
  store_quad(hist_out, i, numel, full, p);
  if (NOISE && z_out) store_quad(z_out, i, numel, full, z);
}

// The deterministic solver's step: no noise.  The coefficients come from cur[1..6] in device memory where `cur` is given (the
// captured step), else from the by-value copies (the eager loop).
__global__ void multistep_kernel(const float *x, const float *eps, const float *hist, size_t numel,
                                 const float *__restrict__ cur, float a0, float a1, float a2, float a3, float a4, float a5,
                                 float *out, float *hist_out, int cm_points) {
  if (cur) { a0 = cur[1]; a1 = cur[2]; a2 = cur[3]; a3 = cur[4]; a4 = cur[5]; a5 = cur[6]; }
  multistep_body<false>(x, eps, hist, nullptr, numel, a0, a1, a2, a3, a4, a5, 0.f, nullptr, 0, 0, out, hist_out, nullptr,
                        cm_points);
}

static int multistep_launch(hipStream_t st, const float *x, const float *eps, const float *hist, size_t numel, const float *cur,
                            const float a[6], float *out, float *hist_out, int cm_points) {
  unsigned blocks;
  if (quad_blocks(numel, &blocks) != LION_OK) return LION_EINVAL;
  return lion_launch<multistep_kernel>(blocks, 256, 0, st, x, eps, hist, numel, cur, a[0], a[1], a[2], a[3], a[4],
                                       a[5], out, hist_out, cm_points);
}

// SDE-DPM-Solver++(2M) (Lu et al. 2022, the SDE form of Algorithm 2): the multistep body's reads and its first three
// operations, then one Gaussian term, one rounding per written operation:
//   x0 = a0*(x - a1*eps);   D = a5 == 0 ? a4*x0 : a4*x0 + a5*hist;   hist_out = x0
//   out = a6 != 0 ? (a2*x + a3*D) + a6*z : a2*x + a3*D
// (a2 = (sigma_n/sigma_t)*exp(-h), a3 = -alpha_n*expm1(-2h), a6 = sigma_n*sqrt(-expm1(-2h))).  With `cur` (the captured step)
// a0..a5 are cur[1..6], the step word is cur[7] (the step's index, as begin_step leaves it) and a6 = table[8*step + 7]; else
// all come by value (the eager loop).  z = z_in where given, else normal4 at counter (quad, step word, stream_id) under the
// seed in device memory: update_noise_kernel's counters.  Nothing is drawn and neither z_in nor the seed is read when a6 == 0;
// z_out (may be NULL) then receives zeros, else the z that was used.  hist and aliasing as in the multistep body.
__global__ void multistep_noise_kernel(const float *x, const float *eps, const float *hist, const float *z_in, size_t numel,
                                       const float *__restrict__ cur, const float *__restrict__ table, float a0, float a1,
                                       float a2, float a3, float a4, float a5, float a6,
                                       const uint32_t *__restrict__ seed_words, uint32_t step, uint32_t stream_id, float *out,
                                       float *hist_out, float *z_out, int cm_points) {
  if (cur) {
    a0 = cur[1]; a1 = cur[2]; a2 = cur[3]; a3 = cur[4]; a4 = cur[5]; a5 = cur[6];
    step = (uint32_t)__float_as_int(cur[7]);
    a6 = table[(size_t)step * 8 + 7];
  }
  multistep_body<true>(x, eps, hist, z_in, numel, a0, a1, a2, a3, a4, a5, a6, seed_words, step, stream_id, out, hist_out, z_out,
                       cm_points);
}

static int multistep_noise_launch(hipStream_t st, const float *x, const float *eps, const float *hist, const float *z_in,
                                  size_t numel, const float *cur, const float *table, const float a[7], const uint32_t *seed,
                                  uint32_t step, uint32_t stream_id, float *out, float *hist_out, float *z_out, int cm_points) {
  unsigned blocks;
  if (quad_blocks(numel, &blocks) != LION_OK) return LION_EINVAL;
  return lion_launch<multistep_noise_kernel>(blocks, 256, 0, st, x, eps, hist, z_in, numel, cur, table, a[0], a[1],
                                             a[2], a[3], a[4], a[5], a[6], seed, step, stream_id, out, hist_out, z_out,
                                             cm_points);
}

// the captured step's form of it under per-sample keys (grid and keys: update_noise_keyed_kernel): coefficients, step word and
// a6 from `cur` and `table`, no z_in; where a6 == 0 no key is read
__global__ void multistep_noise_keyed_kernel(const float *x, const float *eps, const float *hist, size_t numel,
                                             uint32_t sample_quads, const float *__restrict__ cur,
                                             const float *__restrict__ table, const uint32_t *__restrict__ keys,
                                             uint32_t stream_id, float *out, float *hist_out, float *z_out, int cm_points) {
  const uint32_t step = (uint32_t)__float_as_int(cur[7]);
  multistep_body<true, true>(x, eps, hist, nullptr, numel, cur[1], cur[2], cur[3], cur[4], cur[5], cur[6],
                             table[(size_t)step * 8 + 7], keys, step, stream_id, out, hist_out, z_out, cm_points, sample_quads);
}

static int multistep_noise_keyed_launch(hipStream_t st, const float *x, const float *eps, const float *hist, int B, int n,
                                        const float *cur, const float *table, const uint32_t *keys, uint32_t stream_id,
                                        float *out, float *hist_out, float *z_out, int cm_points) {
  dim3 grid;
  uint32_t sq;
  if (keyed_grid(B, n, &grid, &sq) != LION_OK) return LION_EINVAL;
  return lion_launch<multistep_noise_keyed_kernel>(grid, 256, 0, st, x, eps, hist, (size_t)B * n, sq, cur, table, keys,
                                                   stream_id, out, hist_out, z_out, cm_points);
}

// Deterministic encoder (refined DDIM inversion, DiffusionDiscretized.run_ddim_forward): one row of a leg n -> t from low
// noise to high noise, one rounding per written operation:
//   out = a0*base + a1*eps;   if (a2 != 0) base_out = out
// (a0 = s = alpha_t/alpha_n, a1 = c = sigma_t - sigma_n*s, a2 = commit).  base is the state at the leg's low end, eps the
// model's output at the current iterate (the predictor row evaluates it at base itself, every corrector row at the previous
// row's out); the leg's last row commits its iterate as the next leg's base.  Coefficients from cur[1..3] where `cur` is given
// (the captured step), else by value (the eager loop).  base_out is neither read nor written when a2 == 0.
// The tensors are not __restrict__: out may alias the buffer the model read (the chain's x) or base, and
// base_out may alias base (a lane reads its quad of base and eps before it writes either output, no lane reads another's).
__global__ void encode_kernel(const float *base, const float *eps, size_t numel, const float *__restrict__ cur, float a0,
                              float a1, float a2, float *out, float *base_out, int cm_points) {
  const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t i = q * 4;
  if (i >= numel) return;
  if (cur) { a0 = cur[1]; a1 = cur[2]; a2 = cur[3]; }
  const bool commit = a2 != 0.f;
  float bv[4], ev[4], o[4];
  const bool full = i + 3 < numel;
  load_quad(base, i, numel, full, bv);
  load_eps_quad<false>(eps, q, q, numel, full, cm_points, ev);
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = add_rn(mul_rn(a0, bv[j]), mul_rn(a1, ev[j]));
  store_quad(out, i, numel, full, o);
  if (commit) store_quad(base_out, i, numel, full, o);
}

static int encode_launch(hipStream_t st, const float *base, const float *eps, size_t numel, const float *cur, float a0, float a1,
                         float a2, float *out, float *base_out, int cm_points) {
  unsigned blocks;
  if (quad_blocks(numel, &blocks) != LION_OK) return LION_EINVAL;
  return lion_launch<encode_kernel>(blocks, 256, 0, st, base, eps, numel, cur, a0, a1, a2, out, base_out, cm_points);
}

// Forward-process draw out = m*x0 + s*z (sample_q, utils/diffusion_pvd.py:105-113) with the chain's generator: quad q of the
// flat tensor takes Philox counter (q, LION_DIFFUSE_STEP_WORD, stream_id), whatever the pointers' alignment.  VEC: every pointer
// is 16-byte aligned, so that a quad below numel is `full`; without it every quad goes element by element.
// The tensors are not __restrict__: out may alias x0 (a lane reads its quad before it writes it, no lane reads another's).
// KEYED: own_quad's per-sample counters and keys.
template <bool VEC, bool KEYED>
__device__ __forceinline__ void diffuse_body(const float *x0, const float *z_in, size_t numel, uint32_t sample_quads, float m,
                                             float s, const uint32_t *__restrict__ seed_words, uint32_t stream_id, float *out,
                                             float *z_out) {
  size_t q;
  uint64_t ctr;
  const uint32_t *key;
  if (!own_quad<KEYED>(numel, sample_quads, seed_words, q, ctr, key)) return;
  const size_t i = q * 4;
  const bool full = VEC && i + 3 < numel;
  float xv[4], z[4], o[4];
  if (z_in) {
    load_quad(z_in, i, numel, full, z);
  } else {
    const uint64_t seed = (uint64_t)key[0] | ((uint64_t)key[1] << 32);
    normal4(ctr, LION_DIFFUSE_STEP_WORD, stream_id, seed, z);
  }
  load_quad(x0, i, numel, full, xv);
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = add_rn(mul_rn(m, xv[j]), mul_rn(s, z[j]));
  store_quad(out, i, numel, full, o);
  if (z_out) store_quad(z_out, i, numel, full, z);
}

template <bool VEC>
__global__ void diffuse_kernel(const float *x0, const float *z_in, size_t numel, float m, float s,
                               const uint32_t *__restrict__ seed_words, uint32_t stream_id, float *out, float *z_out) {
  diffuse_body<VEC, false>(x0, z_in, numel, 0, m, s, seed_words, stream_id, out, z_out);
}

template <bool VEC>
__global__ void diffuse_keyed_kernel(const float *x0, size_t numel, uint32_t sample_quads, float m, float s,
                                     const uint32_t *__restrict__ keys, uint32_t stream_id, float *out, float *z_out) {
  diffuse_body<VEC, true>(x0, nullptr, numel, sample_quads, m, s, keys, stream_id, out, z_out);
}

// the keyed draw with its scalars per sample (ms f32[B][2] = (m_b, s_b)); a sample with m_b == 1 and s_b == 0 is held
template <bool VEC>
__global__ void diffuse_keyed_at_kernel(const float *x0, size_t numel, uint32_t sample_quads, const float *__restrict__ ms,
                                        const uint32_t *__restrict__ keys, uint32_t stream_id, float *out, float *z_out) {
  const float m = ms[2 * (size_t)blockIdx.y], s = ms[2 * (size_t)blockIdx.y + 1];
  if (m == 1.f && s == 0.f) {
    hold_quad(x0, numel, sample_quads, VEC, out, z_out);
    return;
  }
  diffuse_body<VEC, true>(x0, nullptr, numel, sample_quads, m, s, keys, stream_id, out, z_out);
}

} // namespace

extern "C" {

int lion_ddim_update(const float *x, const float *eps, const float *z, size_t numel, float s,
                     float c, float sigma, float *out, lionStream_t stream) {
  unsigned blocks;
  if (!x || !eps || !out || quad_blocks(numel, &blocks) != LION_OK) return LION_EINVAL;
  if (!z && sigma != 0.f) return LION_EINVAL;
  if (!aligned16({x, eps, out, z})) return LION_EINVAL;
  return lion_launch<ddim_kernel>(blocks, 256, 0, static_cast<hipStream_t>(stream), x, eps, z,
                                  numel, s, c, sigma, out);
}

int lion_ddpm_update(const float *x, const float *eps, const float *z, size_t numel, int t_is_zero,
                     float k_outer, float k_a, float k_b, float scale, float temp, float *out,
                     lionStream_t stream) {
  if (!x || !eps || !out || numel == 0) return LION_EINVAL;
  if (!t_is_zero && !z) return LION_EINVAL;
  return lion_launch<ddpm_kernel>((unsigned)((numel + 255) / 256), 256, 0, static_cast<hipStream_t>(stream), x, eps, z,
                                  numel, t_is_zero, k_outer, k_a, k_b, scale, temp, out);
}

int lion_chain_begin_step(const float *table, int n_steps, int32_t *counter, float *t_out, int B, float *cur,
                          lionStream_t stream) {
  if (!table || !counter || !t_out || !cur || n_steps <= 0 || B <= 0) return LION_EINVAL;
  return lion_launch<begin_step_kernel>(1, 64, 0, static_cast<hipStream_t>(stream), table, n_steps, counter, t_out, B,
                                        cur, nullptr, 0, nullptr);
}

int lion_chain_begin_step_temb(const float *table, int n_steps, int32_t *counter, float *t_out, int B, float *cur,
                               const float *temb_table, int temb_width, float *temb_out, lionStream_t stream) {
  if (!table || !counter || !t_out || !cur || n_steps <= 0 || B <= 0) return LION_EINVAL;
  if (!temb_table || !temb_out || temb_width <= 0) return LION_EINVAL;
  return lion_launch<begin_step_kernel>(1, 64, 0, static_cast<hipStream_t>(stream), table, n_steps, counter, t_out, B,
                                        cur, temb_table, temb_width, temb_out);
}

int lion_chain_update_noise(int mode, const float *x, const float *eps, size_t numel, const float *cur,
                            const uint32_t *seed, uint32_t stream_id, float *out, float *z_out,
                            lionStream_t stream) {
  if (!x || !eps || !cur || !seed || !out || (mode != 0 && mode != 1)) return LION_EINVAL;
  if (!aligned16({x, eps, out, z_out})) return LION_EINVAL;
  return update_noise_launch(mode, static_cast<hipStream_t>(stream), x, eps, numel, cur, seed, stream_id, out, z_out, 0);
}

int lion_chain_update_noise_cm(int mode, const float *x, const float *eps_cm, int B, int N, const float *cur,
                               const uint32_t *seed, uint32_t stream_id, float *out, float *z_out, lionStream_t stream) {
  if (!x || !eps_cm || !cur || !seed || !out || B <= 0 || N <= 0 || (mode != 0 && mode != 1)) return LION_EINVAL;
  if (!aligned16({x, out, z_out})) return LION_EINVAL;
  return update_noise_launch(mode, static_cast<hipStream_t>(stream), x, eps_cm, (size_t)B * N * 4, cur, seed, stream_id, out,
                             z_out, N);
}

int lion_dpmpp_update(const float *x, const float *eps, const float *hist, size_t numel, float a0, float a1, float a2,
                      float a3, float a4, float a5, float *out, float *hist_out, lionStream_t stream) {
  if (!x || !eps || !out || !hist_out) return LION_EINVAL;
  if (!hist && a5 != 0.f) return LION_EINVAL;
  if (!aligned16({x, eps, hist, out, hist_out})) return LION_EINVAL;
  const float a[6] = {a0, a1, a2, a3, a4, a5};
  return multistep_launch(static_cast<hipStream_t>(stream), x, eps, hist, numel, nullptr, a, out, hist_out, 0);
}

int lion_chain_update_multistep(const float *x, const float *eps, const float *hist, size_t numel, const float *cur,
                                float *out, float *hist_out, lionStream_t stream) {
  if (!x || !eps || !hist || !cur || !out || !hist_out) return LION_EINVAL;
  if (!aligned16({x, eps, hist, out, hist_out})) return LION_EINVAL;
  const float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  return multistep_launch(static_cast<hipStream_t>(stream), x, eps, hist, numel, cur, a, out, hist_out, 0);
}

int lion_chain_update_multistep_cm(const float *x, const float *eps_cm, const float *hist, int B, int N, const float *cur,
                                   float *out, float *hist_out, lionStream_t stream) {
  if (!x || !eps_cm || !hist || !cur || !out || !hist_out || B <= 0 || N <= 0) return LION_EINVAL;
  if (!aligned16({x, hist, out, hist_out})) return LION_EINVAL;
  const float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  return multistep_launch(static_cast<hipStream_t>(stream), x, eps_cm, hist, (size_t)B * N * 4, cur, a, out, hist_out, N);
}

int lion_sde_dpmpp_update(const float *x, const float *eps, const float *hist, const float *z_in, size_t numel, float a0,
                          float a1, float a2, float a3, float a4, float a5, float a6, const uint32_t *seed, uint32_t step_word,
                          uint32_t stream_id, float *out, float *hist_out, float *z_out, lionStream_t stream) {
  if (!x || !eps || !out || !hist_out) return LION_EINVAL;
  if (!hist && a5 != 0.f) return LION_EINVAL;
  if (!z_in && !seed && a6 != 0.f) return LION_EINVAL;
  if (!aligned16({x, eps, hist, z_in, out, hist_out, z_out})) return LION_EINVAL;
  const float a[7] = {a0, a1, a2, a3, a4, a5, a6};
  return multistep_noise_launch(static_cast<hipStream_t>(stream), x, eps, hist, z_in, numel, nullptr, nullptr, a, seed,
                                step_word, stream_id, out, hist_out, z_out, 0);
}

int lion_chain_update_multistep_noise(const float *x, const float *eps, const float *hist, size_t numel, const float *cur,
                                      const float *table, const uint32_t *seed, uint32_t stream_id, float *out,
                                      float *hist_out, float *z_out, lionStream_t stream) {
  if (!x || !eps || !hist || !cur || !table || !seed || !out || !hist_out) return LION_EINVAL;
  if (!aligned16({x, eps, hist, out, hist_out, z_out})) return LION_EINVAL;
  const float a[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  return multistep_noise_launch(static_cast<hipStream_t>(stream), x, eps, hist, nullptr, numel, cur, table, a, seed, 0,
                                stream_id, out, hist_out, z_out, 0);
}

int lion_chain_update_multistep_noise_cm(const float *x, const float *eps_cm, const float *hist, int B, int N, const float *cur,
                                         const float *table, const uint32_t *seed, uint32_t stream_id, float *out,
                                         float *hist_out, float *z_out, lionStream_t stream) {
  if (!x || !eps_cm || !hist || !cur || !table || !seed || !out || !hist_out || B <= 0 || N <= 0) return LION_EINVAL;
  if (!aligned16({x, hist, out, hist_out, z_out})) return LION_EINVAL;
  const float a[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  return multistep_noise_launch(static_cast<hipStream_t>(stream), x, eps_cm, hist, nullptr, (size_t)B * N * 4, cur, table, a,
                                seed, 0, stream_id, out, hist_out, z_out, N);
}

int lion_ddim_encode_update(const float *base, const float *eps, size_t numel, float a0, float a1, float a2, float *out,
                            float *base_out, lionStream_t stream) {
  if (!base || !eps || !out) return LION_EINVAL;
  if (!base_out && a2 != 0.f) return LION_EINVAL;
  if (!aligned16({base, eps, out, base_out})) return LION_EINVAL;
  return encode_launch(static_cast<hipStream_t>(stream), base, eps, numel, nullptr, a0, a1, a2, out, base_out, 0);
}

int lion_chain_update_encode(const float *base, const float *eps, size_t numel, const float *cur, float *out, float *base_out,
                             lionStream_t stream) {
  if (!base || !eps || !cur || !out || !base_out) return LION_EINVAL;
  if (!aligned16({base, eps, out, base_out})) return LION_EINVAL;
  return encode_launch(static_cast<hipStream_t>(stream), base, eps, numel, cur, 0.f, 0.f, 0.f, out, base_out, 0);
}

int lion_chain_update_encode_cm(const float *base, const float *eps_cm, int B, int N, const float *cur, float *out,
                                float *base_out, lionStream_t stream) {
  if (!base || !eps_cm || !cur || !out || !base_out || B <= 0 || N <= 0) return LION_EINVAL;
  if (!aligned16({base, out, base_out})) return LION_EINVAL;
  return encode_launch(static_cast<hipStream_t>(stream), base, eps_cm, (size_t)B * N * 4, cur, 0.f, 0.f, 0.f, out, base_out, N);
}

int lion_chain_diffuse(const float *x0, const float *z_in, size_t numel, float m, float s, const uint32_t *seed,
                       uint32_t stream_id, float *out, float *z_out, lionStream_t stream) {
  unsigned blocks;
  if (!x0 || !out || (!z_in && !seed) || quad_blocks(numel, &blocks) != LION_OK) return LION_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return aligned16({x0, z_in, out, z_out})
             ? lion_launch<diffuse_kernel<true>>(blocks, 256, 0, st, x0, z_in, numel, m, s, seed, stream_id, out, z_out)
             : lion_launch<diffuse_kernel<false>>(blocks, 256, 0, st, x0, z_in, numel, m, s, seed, stream_id, out, z_out);
}

// ---- per-sample keys: keys u32[2*B] (lo, hi per sample), n elements per sample, n % 4 == 0 ---------------------------------
int lion_philox_normal_keyed(const uint32_t *keys, int B, int n, uint32_t step_word, uint32_t stream_id, float *out,
                             lionStream_t stream) {
  dim3 grid;
  uint32_t sq;
  if (!keys || !out || keyed_grid(B, n, &grid, &sq) != LION_OK) return LION_EINVAL;
  if (!aligned16({out})) return LION_EINVAL;
  return lion_launch<normal_keyed_kernel>(grid, 256, 0, static_cast<hipStream_t>(stream), keys, (size_t)B * n, sq, step_word,
                                          stream_id, out);
}

int lion_chain_update_noise_keyed(int mode, const float *x, const float *eps, int B, int n, const float *cur,
                                  const uint32_t *keys, uint32_t stream_id, float *out, float *z_out, lionStream_t stream) {
  if (!x || !eps || !cur || !keys || !out || (mode != 0 && mode != 1)) return LION_EINVAL;
  if (!aligned16({x, eps, out, z_out})) return LION_EINVAL;
  return update_noise_keyed_launch(mode, static_cast<hipStream_t>(stream), x, eps, B, n, cur, nullptr, keys, stream_id, out,
                                   z_out, 0);
}

int lion_chain_update_noise_cm_keyed(int mode, const float *x, const float *eps_cm, int B, int N, const float *cur,
                                     const uint32_t *keys, uint32_t stream_id, float *out, float *z_out, lionStream_t stream) {
  if (!x || !eps_cm || !cur || !keys || !out || N <= 0 || N > 0x1fffffff || (mode != 0 && mode != 1)) return LION_EINVAL;
  if (!aligned16({x, out, z_out})) return LION_EINVAL;
  return update_noise_keyed_launch(mode, static_cast<hipStream_t>(stream), x, eps_cm, B, N * 4, cur, nullptr, keys, stream_id,
                                   out, z_out, N);
}

// ---- per-sample start steps: a first row (or a forward draw's scalars) per sample, on the keyed kernels' grid ---------------
int lion_chain_update_noise_keyed_from(int mode, const float *x, const float *eps, int B, int n, const float *cur,
                                       const int32_t *first_row, const uint32_t *keys, uint32_t stream_id, float *out,
                                       float *z_out, lionStream_t stream) {
  if (!x || !eps || !cur || !first_row || !keys || !out || (mode != 0 && mode != 1)) return LION_EINVAL;
  if (!aligned16({x, eps, out, z_out})) return LION_EINVAL;
  return update_noise_keyed_launch(mode, static_cast<hipStream_t>(stream), x, eps, B, n, cur, first_row, keys, stream_id, out,
                                   z_out, 0);
}

int lion_chain_update_noise_cm_keyed_from(int mode, const float *x, const float *eps_cm, int B, int N, const float *cur,
                                          const int32_t *first_row, const uint32_t *keys, uint32_t stream_id, float *out,
                                          float *z_out, lionStream_t stream) {
  if (!x || !eps_cm || !cur || !first_row || !keys || !out || N <= 0 || N > 0x1fffffff || (mode != 0 && mode != 1))
    return LION_EINVAL;
  if (!aligned16({x, out, z_out})) return LION_EINVAL;
  return update_noise_keyed_launch(mode, static_cast<hipStream_t>(stream), x, eps_cm, B, N * 4, cur, first_row, keys, stream_id,
                                   out, z_out, N);
}

// ---- known region: a clean value and a mask byte per quad, beside the per-sample first rows -----------------------------------
int lion_chain_update_noise_keyed_known(int mode, const float *x, const float *eps, int B, int n, const float *cur,
                                        const int32_t *first_row, const uint32_t *keys, uint32_t stream_id,
                                        const float *known_x0, const uint8_t *keep, const float *known_ms,
                                        uint32_t known_stream_id, float *out, float *z_out, lionStream_t stream) {
  if (!x || !eps || !cur || !keys || !out || (mode != 0 && mode != 1)) return LION_EINVAL;
  if (!known_x0 || !keep || !known_ms || known_stream_id == stream_id) return LION_EINVAL;
  if (!aligned16({x, eps, known_x0, out, z_out})) return LION_EINVAL;
  return update_noise_known_launch(mode, static_cast<hipStream_t>(stream), x, eps, B, n, cur, first_row, keys, stream_id,
                                   known_x0, keep, known_ms, known_stream_id, nullptr, 0, out, z_out, 0);
}

int lion_chain_update_noise_cm_keyed_known(int mode, const float *x, const float *eps_cm, int B, int N, const float *cur,
                                           const int32_t *first_row, const uint32_t *keys, uint32_t stream_id,
                                           const float *known_x0, const uint8_t *keep, const float *known_ms,
                                           uint32_t known_stream_id, float *out, float *z_out, lionStream_t stream) {
  if (!x || !eps_cm || !cur || !keys || !out || N <= 0 || N > 0x1fffffff || (mode != 0 && mode != 1)) return LION_EINVAL;
  if (!known_x0 || !keep || !known_ms || known_stream_id == stream_id) return LION_EINVAL;
  if (!aligned16({x, known_x0, out, z_out})) return LION_EINVAL;
  return update_noise_known_launch(mode, static_cast<hipStream_t>(stream), x, eps_cm, B, N * 4, cur, first_row, keys, stream_id,
                                   known_x0, keep, known_ms, known_stream_id, nullptr, 0, out, z_out, N);
}

// ---- known region with resampling jumps: a forward move of the free quads at the end of the rows that known_jump marks --------
int lion_chain_update_noise_keyed_known_resample(int mode, const float *x, const float *eps, int B, int n, const float *cur,
                                                 const int32_t *first_row, const uint32_t *keys, uint32_t stream_id,
                                                 const float *known_x0, const uint8_t *keep, const float *known_ms,
                                                 uint32_t known_stream_id, const float *known_jump,
                                                 uint32_t resample_stream_id, float *out, float *z_out, lionStream_t stream) {
  if (!x || !eps || !cur || !keys || !out || (mode != 0 && mode != 1)) return LION_EINVAL;
  if (!known_x0 || !keep || !known_ms || known_stream_id == stream_id) return LION_EINVAL;
  if (!known_jump || resample_stream_id == stream_id || resample_stream_id == known_stream_id) return LION_EINVAL;
  if (!aligned16({x, eps, known_x0, out, z_out})) return LION_EINVAL;
  return update_noise_known_launch(mode, static_cast<hipStream_t>(stream), x, eps, B, n, cur, first_row, keys, stream_id,
                                   known_x0, keep, known_ms, known_stream_id, known_jump, resample_stream_id, out, z_out, 0);
}

int lion_chain_update_noise_cm_keyed_known_resample(int mode, const float *x, const float *eps_cm, int B, int N,
                                                    const float *cur, const int32_t *first_row, const uint32_t *keys,
                                                    uint32_t stream_id, const float *known_x0, const uint8_t *keep,
                                                    const float *known_ms, uint32_t known_stream_id, const float *known_jump,
                                                    uint32_t resample_stream_id, float *out, float *z_out,
                                                    lionStream_t stream) {
  if (!x || !eps_cm || !cur || !keys || !out || N <= 0 || N > 0x1fffffff || (mode != 0 && mode != 1)) return LION_EINVAL;
  if (!known_x0 || !keep || !known_ms || known_stream_id == stream_id) return LION_EINVAL;
  if (!known_jump || resample_stream_id == stream_id || resample_stream_id == known_stream_id) return LION_EINVAL;
  if (!aligned16({x, known_x0, out, z_out})) return LION_EINVAL;
  return update_noise_known_launch(mode, static_cast<hipStream_t>(stream), x, eps_cm, B, N * 4, cur, first_row, keys, stream_id,
                                   known_x0, keep, known_ms, known_stream_id, known_jump, resample_stream_id, out, z_out, N);
}

int lion_chain_update_multistep_noise_keyed(const float *x, const float *eps, const float *hist, int B, int n, const float *cur,
                                            const float *table, const uint32_t *keys, uint32_t stream_id, float *out,
                                            float *hist_out, float *z_out, lionStream_t stream) {
  if (!x || !eps || !hist || !cur || !table || !keys || !out || !hist_out) return LION_EINVAL;
  if (!aligned16({x, eps, hist, out, hist_out, z_out})) return LION_EINVAL;
  return multistep_noise_keyed_launch(static_cast<hipStream_t>(stream), x, eps, hist, B, n, cur, table, keys, stream_id, out,
                                      hist_out, z_out, 0);
}

int lion_chain_update_multistep_noise_cm_keyed(const float *x, const float *eps_cm, const float *hist, int B, int N,
                                               const float *cur, const float *table, const uint32_t *keys, uint32_t stream_id,
                                               float *out, float *hist_out, float *z_out, lionStream_t stream) {
  if (!x || !eps_cm || !hist || !cur || !table || !keys || !out || !hist_out || N <= 0 || N > 0x1fffffff) return LION_EINVAL;
  if (!aligned16({x, hist, out, hist_out, z_out})) return LION_EINVAL;
  return multistep_noise_keyed_launch(static_cast<hipStream_t>(stream), x, eps_cm, hist, B, N * 4, cur, table, keys, stream_id,
                                      out, hist_out, z_out, N);
}

int lion_chain_diffuse_keyed(const float *x0, int B, int n, float m, float s, const uint32_t *keys, uint32_t stream_id,
                             float *out, float *z_out, lionStream_t stream) {
  dim3 grid;
  uint32_t sq;
  if (!x0 || !keys || !out || keyed_grid(B, n, &grid, &sq) != LION_OK) return LION_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t numel = (size_t)B * n;
  return aligned16({x0, out, z_out})
             ? lion_launch<diffuse_keyed_kernel<true>>(grid, 256, 0, st, x0, numel, sq, m, s, keys, stream_id, out, z_out)
             : lion_launch<diffuse_keyed_kernel<false>>(grid, 256, 0, st, x0, numel, sq, m, s, keys, stream_id, out, z_out);
}

int lion_chain_diffuse_keyed_at(const float *x0, int B, int n, const float *ms, const uint32_t *keys, uint32_t stream_id,
                                float *out, float *z_out, lionStream_t stream) {
  dim3 grid;
  uint32_t sq;
  if (!x0 || !ms || !keys || !out || keyed_grid(B, n, &grid, &sq) != LION_OK) return LION_EINVAL;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t numel = (size_t)B * n;
  return aligned16({x0, out, z_out})
             ? lion_launch<diffuse_keyed_at_kernel<true>>(grid, 256, 0, st, x0, numel, sq, ms, keys, stream_id, out, z_out)
             : lion_launch<diffuse_keyed_at_kernel<false>>(grid, 256, 0, st, x0, numel, sq, ms, keys, stream_id, out, z_out);
}

} // extern "C"
