// ode.hip -- the probability-flow ODE solver of the continuous-time (VPSDE) samplers, on the device.
//
// Reference: utils/diffusion_continuous.py:90-255 (compute_ode_nll / sample_model_ode) integrate the PF-ODE with
// scipy.integrate.solve_ivp(method='RK45') through torchdiffeq's scipy wrapper: the whole batch is ONE system of B*D
// unknowns in float64, every evaluation copies the latent device -> host -> device.  Here the state of that solver --
// y, the seven stage derivatives K, the stage combinations, the RMS error norm and scipy's step-size controller
// (RK45._step_impl, rk.py; select_initial_step, common.py) -- lives in device memory, so that one evaluation is
//     lion_ode_stage -> denoiser forward -> lion_ode_drift
// with the stage index in device memory (a captured graph serves every stage), and one attempted step ends with
//     lion_ode_error_partials -> lion_ode_control
// after which the host reads the small control struct once.
//
// Arithmetic: float64 with one rounding per written operation (-ffp-contract=off), sums over stages in ascending stage
// order, exactly as the float64 restatement in the tests (numpy's BLAS dot may order or fuse differently: ulps).  The
// model sees the fp32 rounding of the float64 stage state, as torch.tensor(y).to(float32) does in the wrapper; its output
// becomes the drift in the fp32 scalar expressions of diffusion_continuous.py:205-226 / :599-622 and is widened exactly.
// The error norm is reduced deterministically (fixed per-block trees, then one block in block order): no float atomics,
// so eager runs and graph replays are bit-identical.
#include "common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxPartials = 1024;

// Dormand-Prince 5(4) as scipy's RK45 (rk.py): C, A (rows 1..5), B, E.
__constant__ double kC[7] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 0.0};
__constant__ double kA[6][5] = {
    {0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
__constant__ double kB[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
__constant__ double kE[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};

constexpr double SAFETY = 0.9, MIN_FACTOR = 0.2, MAX_FACTOR = 10.0, ERR_EXP = -1.0 / 5;

// logical stage row -> physical row of K: row 0 holds f (FSAL) and row 6 f_new; an accepted step swaps the two by
// flipping fslot instead of copying
__device__ __forceinline__ int krow(int logical, int fslot) {
  return logical == 0 ? fslot : (logical == 6 ? 6 - fslot : logical);
}

// rows of K an evaluation of stage s writes: 1..6 a step's stages, 7 = f0 at the start, 8 = the initial-step probe
__device__ __forceinline__ int stage_row(int s) { return s == 7 ? 0 : (s == 8 ? 1 : s); }

__global__ void stage_kernel(double *__restrict__ Y, const double *__restrict__ K, size_t n, lion_ode_ctrl *ctrl,
                             float *__restrict__ x32, float *__restrict__ t_model, int B) {
  const int s = ctrl->stage;
  const int ys = ctrl->yslot, fs = ctrl->fslot;
  const double t = ctrl->t, h = ctrl->h;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0) {
    double tm;
    if (s == 7) tm = ctrl->t;
    else if (s == 8) tm = t + ctrl->h0 * ctrl->direction;
    else if (s == 6) tm = t + h;                      // rk_step: fun(t + h, y_new)
    else tm = t + kC[s] * h;                           // fun(t + c * h, y + dy)
    float tf = (float)tm;                              // torch.tensor(t).to(float32)
    if (ctrl->sign < 0) tf = -tf;                      // torchdiffeq _ReverseFunc: base_func(-t, y)
    for (int b = threadIdx.x; b < B; b += blockDim.x) t_model[b] = tf;
    if (threadIdx.x == 0) ctrl->cur = s;
  }
  if (i >= n) return;
  const double y = Y[(size_t)ys * n + i];
  double v;
  if (s == 7) {
    v = y;
  } else if (s == 8) {                                 // select_initial_step: y1 = y0 + h0 * direction * f0
    v = y + (ctrl->h0 * ctrl->direction) * K[(size_t)fs * n + i];
  } else if (s == 6) {                                 // y_new = y + h * dot(K[:-1].T, B)
    double acc = K[(size_t)krow(0, fs) * n + i] * kB[0];
    for (int j = 1; j < 6; ++j) acc = acc + K[(size_t)krow(j, fs) * n + i] * kB[j];
    v = y + h * acc;
    Y[(size_t)(1 - ys) * n + i] = v;
  } else {                                             // dy = dot(K[:s].T, a[:s]) * h
    double acc = K[(size_t)krow(0, fs) * n + i] * kA[s][0];
    for (int j = 1; j < s; ++j) acc = acc + K[(size_t)krow(j, fs) * n + i] * kA[s][j];
    v = y + acc * h;
  }
  x32[i] = (float)v;
}

// VPSDE drift of sample_model_ode's ode_func in fp32: dx/dt = f(t)*x + 0.5*g2(t)*params/sqrt(var(t)),
// params = (1 - sigmoid(logit))*sqrt(var)*x + sigmoid(logit)*eps when mixing is on.
__global__ void drift_kernel(const float *__restrict__ eps, int cm_points, const float *__restrict__ x32, size_t n,
                             const float *__restrict__ t_model, float bs, float dbeta, float nbs, float hdb, float c2,
                             const float *__restrict__ mix_a, const float *__restrict__ mix_b, int mix_len,
                             double *__restrict__ K, lion_ode_ctrl *ctrl) {
  const int s = ctrl->cur;
  const int row = krow(stage_row(s), ctrl->fslot);
  const bool neg = ctrl->sign < 0;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctrl->nfe += 1;
    if (s >= 1 && s <= 5) ctrl->stage = s + 1;
  }
  if (i >= n) return;
  const float tm = t_model[0];
  const float g2 = add_rn(bs, mul_rn(dbeta, tm));                                     // g2(t)
  const float f = mul_rn(-0.5f, g2);                                                  // f(t) = -0.5 g2(t)
  const float var = sub_rn(1.0f, mul_rn(c2, expf(sub_rn(mul_rn(nbs, tm), mul_rn(mul_rn(hdb, tm), tm)))));
  const float sq = sqrt_rn(var);
  const float x = x32[i];
  float p;
  if (cm_points) {   // the local prior's channel-major [B][4][N] output for a point-major [B][N][4] latent
    const size_t q = i >> 2, b = q / (size_t)cm_points, pt = q - b * (size_t)cm_points;
    p = eps[(b * 4 + (i & 3)) * (size_t)cm_points + pt];
  } else {
    p = eps[i];
  }
  if (mix_a) {       // get_mixed_prediction (utils.py:1299-1305); mix_a = 1 - sigmoid(logit), mix_b = sigmoid(logit)
    const size_t d = i % (size_t)mix_len;
    p = add_rn(mul_rn(mix_a[d], mul_rn(sq, x)), mul_rn(mix_b[d], p));
  }
  float dx = add_rn(mul_rn(f, x), div_rn(mul_rn(mul_rn(0.5f, g2), p), sq));
  if (neg) dx = -dx;                                  // _ReverseFunc: mul * base_func(-t, y), mul = -1
  K[(size_t)row * n + i] = (double)dx;
}

__device__ __forceinline__ double block_sum(double v, double *sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + w];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__host__ __device__ inline int partial_blocks(size_t n) {
  const size_t b = (n + 4 * kThreads - 1) / (4 * kThreads);
  return (int)(b < 1 ? 1 : (b > kMaxPartials ? kMaxPartials : b));
}

// mode = ctrl->stage: 6 -> sum((dot(K.T, E) * h / scale)^2), scale = atol + max(|y|, |y_new|) * rtol;
// 7 -> sum((y0 / scale)^2), sum((f0 / scale)^2); 8 -> sum(((f1 - f0) / scale)^2), scale = atol + |y0| * rtol
__global__ void partials_kernel(const double *__restrict__ Y, const double *__restrict__ K, size_t n,
                                const lion_ode_ctrl *ctrl, double *__restrict__ partials) {
  __shared__ double sh[kThreads];
  const int mode = ctrl->stage, ys = ctrl->yslot, fs = ctrl->fslot;
  const double h = ctrl->h, rtol = ctrl->rtol, atol = ctrl->atol;
  double a0 = 0.0, a1 = 0.0;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double y = Y[(size_t)ys * n + i];
    if (mode == 6) {
      const double yn = Y[(size_t)(1 - ys) * n + i];
      double acc = K[(size_t)krow(0, fs) * n + i] * kE[0];
      for (int j = 1; j < 7; ++j) acc = acc + K[(size_t)krow(j, fs) * n + i] * kE[j];
      const double err = acc * h;
      const double ay = fabs(y), ayn = fabs(yn);
      const double q = err / (atol + (ay < ayn ? ayn : ay) * rtol);
      a0 = a0 + q * q;
    } else {
      const double sc = atol + fabs(y) * rtol;
      const double f0 = K[(size_t)fs * n + i];
      if (mode == 7) {
        const double q0 = y / sc, q1 = f0 / sc;
        a0 = a0 + q0 * q0;
        a1 = a1 + q1 * q1;
      } else {
        const double q = (K[(size_t)1 * n + i] - f0) / sc;
        a0 = a0 + q * q;
      }
    }
  }
  const double s0 = block_sum(a0, sh);
  const double s1 = block_sum(a1, sh);
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = s0;
    partials[2 * blockIdx.x + 1] = s1;
  }
}

__device__ void attempt(lion_ode_ctrl *c, double min_step) {   // the head of the while loop of _step_impl
  if (c->h_abs < min_step) { c->status = LION_ODE_TOO_SMALL_STEP; return; }
  double h = c->h_abs * c->direction;
  double t_new = c->t + h;
  if (c->direction * (t_new - c->t_bound) > 0) t_new = c->t_bound;
  h = t_new - c->t;
  c->h = h;
  c->t_new = t_new;
  c->h_abs = fabs(h);
  c->stage = 1;
}

__device__ double min_step_at(double t, double direction) {
  return 10 * fabs(nextafter(t, direction * INFINITY) - t);
}

__device__ void begin_step(lion_ode_ctrl *c) {              // OdeSolver.step -> RK45._step_impl, up to the loop
  if (c->t == c->t_bound) { c->status = LION_ODE_FINISHED; return; }
  c->step_rejected = 0;
  const double min_step = min_step_at(c->t, c->direction);
  if (c->h_abs < min_step) c->h_abs = min_step;             // max_step = inf: the other clamp never applies
  attempt(c, min_step);
}

__global__ void control_kernel(const double *__restrict__ partials, size_t n, lion_ode_ctrl *c) {
  __shared__ double sh[kThreads];
  const int P = partial_blocks(n);
  double a0 = 0.0, a1 = 0.0;
  for (int b = threadIdx.x; b < P; b += kThreads) {
    a0 = a0 + partials[2 * b];
    a1 = a1 + partials[2 * b + 1];
  }
  const double s0 = block_sum(a0, sh);
  const double s1 = block_sum(a1, sh);
  if (threadIdx.x != 0 || c->status != LION_ODE_RUNNING) return;
  const double rn = sqrt((double)n);                          // norm(x) = ||x|| / x.size ** 0.5
  const int mode = c->stage;
  const double interval = fabs(c->t_bound - c->t);
  if (mode == 7) {                                            // select_initial_step, first half
    if (interval == 0.0) { c->h_abs = 0.0; begin_step(c); return; }
    const double d0 = sqrt(s0) / rn, d1 = sqrt(s1) / rn;
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    if (interval < h0) h0 = interval;
    c->h0 = h0;
    c->d1 = d1;
    c->stage = 8;
  } else if (mode == 8) {                                     // second half: d2, h1, the first step size
    const double d1 = c->d1, h0 = c->h0;
    const double d2 = (sqrt(s0) / rn) / h0;
    double h1;
    if (d1 <= 1e-15 && d2 <= 1e-15) {
      h1 = h0 * 1e-3;
      if (h1 < 1e-6) h1 = 1e-6;
    } else {
      h1 = pow(0.01 / (d1 < d2 ? d2 : d1), 1.0 / (4 + 1));
    }
    double h = 100 * h0;
    if (h1 < h) h = h1;
    if (interval < h) h = interval;
    c->h_abs = h;
    begin_step(c);
  } else if (mode == 6) {                                     // the end of an attempt: accept or reject
    const double en = sqrt(s0) / rn;
    c->err_norm = en;
    if (en < 1) {
      double factor = en == 0 ? MAX_FACTOR : SAFETY * pow(en, ERR_EXP);
      if (factor > MAX_FACTOR) factor = MAX_FACTOR;
      if (c->step_rejected && factor > 1) factor = 1;
      c->h_abs = c->h_abs * factor;
      c->t = c->t_new;
      c->yslot = 1 - c->yslot;
      c->fslot = 6 - c->fslot;
      c->n_accepted += 1;
      c->accepted = 1;
      if (c->direction * (c->t - c->t_bound) >= 0) c->status = LION_ODE_FINISHED;
      else begin_step(c);
    } else {
      double factor = SAFETY * pow(en, ERR_EXP);
      if (factor < MIN_FACTOR) factor = MIN_FACTOR;
      c->h_abs = c->h_abs * factor;
      c->step_rejected = 1;
      c->n_rejected += 1;
      c->accepted = 0;
      attempt(c, min_step_at(c->t, c->direction));
    }
  }
}

} // namespace

extern "C" {

size_t lion_ode_partials_bytes(size_t n) { return n == 0 ? 0 : (size_t)partial_blocks(n) * 2 * sizeof(double); }

int lion_ode_stage(double *Y, const double *K, size_t n, lion_ode_ctrl *ctrl, float *x32, float *t_model, int B,
                   lionStream_t stream) {
  if (!Y || !K || !ctrl || !x32 || !t_model || n == 0 || B <= 0) return LION_EINVAL;
  const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
  return lion_launch<stage_kernel>(blocks, kThreads, 0, static_cast<hipStream_t>(stream), Y, K, n, ctrl, x32, t_model,
                                   B);
}

int lion_ode_drift(const float *eps, int cm_points, const float *x32, size_t n, const float *t_model, float beta_start,
                   float beta_delta, float neg_beta_start, float half_beta_delta, float one_minus_sigma2_0,
                   const float *mix_a, const float *mix_b, int mix_len, double *K, lion_ode_ctrl *ctrl,
                   lionStream_t stream) {
  if (!eps || !x32 || !t_model || !K || !ctrl || n == 0 || cm_points < 0) return LION_EINVAL;
  if (cm_points && n % ((size_t)cm_points * 4) != 0) return LION_EINVAL;
  if ((mix_a == nullptr) != (mix_b == nullptr) || (mix_a && (mix_len <= 0 || n % (size_t)mix_len != 0)))
    return LION_EINVAL;
  const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
  return lion_launch<drift_kernel>(blocks, kThreads, 0, static_cast<hipStream_t>(stream), eps, cm_points, x32, n,
                                   t_model, beta_start, beta_delta, neg_beta_start, half_beta_delta, one_minus_sigma2_0,
                                   mix_a, mix_b, mix_len, K, ctrl);
}

int lion_ode_error_partials(const double *Y, const double *K, size_t n, const lion_ode_ctrl *ctrl, double *partials,
                            lionStream_t stream) {
  if (!Y || !K || !ctrl || !partials || n == 0) return LION_EINVAL;
  return lion_launch<partials_kernel>(partial_blocks(n), kThreads, 0, static_cast<hipStream_t>(stream), Y, K, n, ctrl,
                                      partials);
}

int lion_ode_control(const double *partials, size_t n, lion_ode_ctrl *ctrl, lionStream_t stream) {
  if (!partials || !ctrl || n == 0) return LION_EINVAL;
  return lion_launch<control_kernel>(1, kThreads, 0, static_cast<hipStream_t>(stream), partials, n, ctrl);
}

} // extern "C"
