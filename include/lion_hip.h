/*
 * lion_hip.h -- C ABI of liblion_hip.so: the MI355X (gfx950) implementation of the
 * LION / PVCNN hot path.
 *
 * Every entry point replaces one function of the reference's pybind/ATen operator modules
 * (cited per function as file:line under /root/reference).  Conventions:
 *   - plain device pointers + sizes, no torch types; all tensors C-contiguous, fp32 / int32;
 *   - no allocation, no synchronisation, no global state that results depend on: safe under hipGraph
 *     capture and callable from any host thread, for any device of the process (the device is the
 *     calling thread's current one; the only state kept is a per-device note of which kernels already
 *     had their dynamic-LDS limit raised -- the first call of a kernel on a device makes one
 *     hipFuncSetAttribute call, so run one call outside a capture first);
 *     scratch memory is passed in (`ws`, size from the matching lion_*_workspace_bytes());
 *   - every launch goes to the caller's `stream` (the reference mixes the legacy default stream
 *     and the current stream; here it is always the caller's stream);
 *   - outputs are fully overwritten (callers may pass torch.empty buffers) unless a parameter
 *     is documented "pre-zeroed";
 *   - return 0 on success, a positive hipError_t if a launch failed, or a negative LION_E* code
 *     for a rejected argument.  Nothing ever calls exit() (the reference does: cuda_utils.cuh:28-37).
 */
#ifndef LION_HIP_H_
#define LION_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *lionStream_t; /* hipStream_t */

#define LION_OK 0
#define LION_EINVAL (-1)      /* bad shape / null pointer */
#define LION_EUNSUPPORTED (-2) /* shape outside what the kernels implement */
#define LION_EWORKSPACE (-3)  /* workspace too small */

/* Library / device info. */
int lion_abi_version(void);

/* ---- K1+K2: avg_voxelize_forward, voxelization/vox.cpp:17-43 (vox.cu:18-72) -------------
 * feat f32[B,C,N], coords i32[B,3,N] -> out f32[B,C,r^3], ind i32[B,N], cnt i32[B,r^3].
 * Deterministic: each voxel sums its points in ascending point index (bit-exact vs oracle). */
size_t lion_avg_voxelize_workspace_bytes(int B, int C, int N, int r);
int lion_avg_voxelize_forward(const float *feat, const int32_t *coords, int B, int C, int N,
                              int r, float *out, int32_t *ind, int32_t *cnt, void *ws,
                              size_t ws_bytes, lionStream_t stream);

/* ---- P1+K1+K2 fused: Voxelization.forward, models/pvcnn2_ada.py:173-188 -----------------
 * coords f32[B,3,N] (raw point coords) -> norm_coords f32[B,3,N] (voxel units, clamped) and
 * everything lion_avg_voxelize_forward returns.  feat may be NULL (C ignored): only
 * norm_coords / ind / cnt are produced (pvcnn2_ada.py:185-186).
 * The coordinate mean uses the fixed summation tree documented in oracle/lion_oracle.c. */
int lion_voxelize_points_forward(const float *feat, const float *coords, int B, int C, int N,
                                 int r, int normalize, float eps, float *out,
                                 float *norm_coords, int32_t *ind, int32_t *cnt, void *ws,
                                 size_t ws_bytes, lionStream_t stream);

/* ---- P1+K1 once, K2 many times: the index plan of a (cloud, resolution) pair ----------------
 * One forward of the denoiser voxelises 4 distinct (coordinates, r) pairs 14 times (PVConv.forward,
 * models/pvcnn2_ada.py:235-243: every PVConv of a stage re-derives the same voxel ids from the same
 * coordinates).  lion_voxel_index computes what depends on the coordinates only -- norm_coords, ind, cnt
 * exactly as lion_voxelize_points_forward, plus the points of every voxel in ascending point index
 * (an opaque plan of lion_voxel_plan_bytes bytes, 0 = shape outside the fast path: use the fused entry
 * point) -- and lion_voxel_scatter mean-pools feat f32[B,C,N] into out f32[B,C,r^3] from that plan:
 * same sums in the same order, bit-identical to lion_voxelize_points_forward (vox.cu:48-72). */
size_t lion_voxel_plan_bytes(int B, int N, int r);
int lion_voxel_index(const float *coords, int B, int N, int r, int normalize, float eps,
                     float *norm_coords, int32_t *ind, int32_t *cnt, void *plan, size_t plan_bytes,
                     lionStream_t stream);
int lion_voxel_scatter(const float *feat, const void *plan, size_t plan_bytes, int B, int C, int N,
                       int r, float *out, lionStream_t stream);
/* Round 5: the same scatter for a grid whose ONLY reader is the sparse convolution that pops occ_m1
 * (lion_conv3d_tile_occupancy[_aware], margin 1; r in {16, 32}) -- conv1 of a PVConv in the fused inference path
 * (pvcnn2_ada.py:206-222).  That convolution stages the halo of the tiles with a point within one voxel and nothing
 * else: z-rows of the grid outside every such halo are NOT written (left as allocated; their content is all zeros in the
 * full scatter and has no reader). */
int lion_voxel_scatter_read(const float *feat, const void *plan, size_t plan_bytes, int B, int C, int N, int r,
                            const int32_t *occ_m1, float *out, lionStream_t stream);
/* For tests only, pure host calls that launch nothing: the launch plans of the kernels above and of the devoxelize forward,
 * written into out, a HOST array of 8 ints.  stream is not used (every entry with a pointer parameter takes one).
 * lion_internal_voxelize_plan: kind 0 the fused kernel (lion_avg_voxelize_forward, lion_voxelize_points_forward, and with
 * C = 0 lion_voxel_index), 1 lion_voxel_scatter, 2 lion_voxel_scatter_read -> {slabs per cloud S, channel ranges CS, voxels
 * per slab SV, points per thread NP, plan words per slab, LDS arena words, LDS bytes, grid}; LION_OK, or LION_EUNSUPPORTED
 * for a shape the fast path (kind 0: the fallback runs) or the scatter launcher refuses.
 * lion_internal_devoxelize_path: the forward at (B, C, N, r) with (aligned != 0) or without a 16-byte aligned grid ->
 * {kind (0 ring, 1 slab, 2 gather), PX, XS, CI, ld (0 unless slab), channels per workgroup, LDS bytes, grid.x}. */
int lion_internal_voxelize_plan(int B, int C, int N, int r, int kind, int32_t *out, lionStream_t stream);
int lion_internal_devoxelize_path(int B, int C, int N, int r, int aligned, int32_t *out, lionStream_t stream);

/* ---- K3: avg_voxelize_backward, vox.cpp:54-79 (vox.cu:86-110) --------------------------
 * gy f32[B,C,r3], ind i32[B,N], cnt i32[B,r3] -> gx f32[B,C,N]. */
int lion_avg_voxelize_backward(const float *gy, const int32_t *ind, const int32_t *cnt, int B,
                               int C, int N, int r3, float *gx, lionStream_t stream);

/* ---- K4: trilinear_devoxelize_forward, interpolate/trilinear_devox.cpp:18-55 -------------
 * coords f32[B,3,N] (voxel units in [0,r-1]), feat f32[B,C,r^3] -> out f32[B,C,N];
 * training != 0 also writes inds i32[B,8,N], wgts f32[B,8,N] (else they may be NULL). */
int lion_trilinear_devoxelize_forward(const float *coords, const float *feat, int B, int C,
                                      int N, int r, int training, float *out, int32_t *inds,
                                      float *wgts, lionStream_t stream);

/* ---- K5: trilinear_devoxelize_backward, trilinear_devox.cpp:67-95 -------------------------
 * gy f32[B,C,N], inds i32[B,8,N], wgts f32[B,8,N] -> gx f32[B,C,r3] (fully written). */
int lion_trilinear_devoxelize_backward(const float *gy, const int32_t *inds, const float *wgts,
                                       int B, int C, int N, int r3, float *gx,
                                       lionStream_t stream);

/* ---- K6: ball_query, ball_query/ball_query.cpp:7-33 (ball_query.cu:19-50) ----------------
 * centers f32[B,3,M], points f32[B,3,N] -> idx i32[B,M,U]: the first U points (ascending
 * index) with d^2 < radius^2, padded with the first hit; all zero when there is none. */
int lion_ball_query(const float *centers, const float *points, int B, int M, int N,
                    float radius, int U, int32_t *idx, lionStream_t stream);

/* ---- K7/K8: grouping, grouping/grouping.cu:18-36 / :58-77 --------------------------------
 * feat f32[B,C,N], idx i32[B,M,U] -> out f32[B,C,M,U];  gy f32[B,C,M,U] -> gx f32[B,C,N]. */
int lion_grouping_forward(const float *feat, const int32_t *idx, int B, int C, int N, int M,
                          int U, float *out, lionStream_t stream);
/* BallQuery.forward (models/pvcnn2_ada.py:98-114) without the subtraction pass and the torch.cat of the grouped
 * activation: out f32[B, 3 + C, M, U], channels 0..2 = coords[b,:,idx[b,m,u]] - centers[b,:,m], 3.. = feat[b,:,idx]
 * (feat NULL with C = 0: coordinates only).  coords f32[B,3,N], centers f32[B,3,M], feat f32[B,C,N], idx i32[B,M,U]. */
int lion_group_points_forward(const float *coords, const float *centers, const float *feat, const int32_t *idx,
                              int B, int C, int N, int M, int U, float *out, lionStream_t stream);
int lion_grouping_backward(const float *gy, const int32_t *idx, int B, int C, int N, int M,
                           int U, float *gx, lionStream_t stream);

/* ---- K9: furthest_point_sampling, sampling/sampling.cpp:43-58 (sampling.cu:86-167) -------
 * coords f32[B,3,N] -> idx i32[B,M]; idx[.,0] = 0; ties resolved exactly as the reference's
 * 512-thread reduction does (lowest (k mod 512, k)). */
int lion_furthest_point_sampling(const float *coords, int B, int N, int M, int32_t *idx,
                                 lionStream_t stream);

/* ---- K10: gather_features, sampling/sampling.cu:17-31 / :52-66 --------------------------- */
int lion_gather_features_forward(const float *feat, const int32_t *idx, int B, int C, int N,
                                 int M, float *out, lionStream_t stream);
int lion_gather_features_backward(const float *gy, const int32_t *idx, int B, int C, int N,
                                  int M, float *gx, lionStream_t stream);

/* ---- K11+K12: three_nearest_neighbors_interpolate, interpolate/neighbor_interpolate.cu ----
 * points f32[B,3,N], centers f32[B,3,M], cfeat f32[B,C,M] ->
 * out f32[B,C,N], idx i32[B,3,N], wgt f32[B,3,N]   (:20-75 then :90-116);
 * backward gy f32[B,C,N] -> gx f32[B,C,M]           (:145-170). */
int lion_three_nn_interpolate_forward(const float *points, const float *centers,
                                      const float *cfeat, int B, int C, int N, int M,
                                      float *out, int32_t *idx, float *wgt,
                                      lionStream_t stream);
/* PointNetFPModule.forward (pvcnn2_ada.py:403-411) with its two torch.cat folded in: out f32[B][C1+C2+C3][N] = [interp(cfeat
 * f32[B][C1][M]) ; interp(temb[b*ld_t + c] taken as a [C2][M] constant row) ; skip f32[B][C3][N]] (C2 / C3 may be 0).  Same
 * three products and two sums per value as lion_three_nn_interpolate_forward on the materialised concatenation. */
int lion_three_nn_interpolate_cat_forward(const float *points, const float *centers, const float *cfeat, const float *temb,
                                          int ld_t, const float *skip, int B, int C1, int C2, int C3, int N, int M,
                                          float *out, int32_t *idx, float *wgt, lionStream_t stream);
int lion_three_nn_interpolate_backward(const float *gy, const int32_t *idx, const float *wgt,
                                       int B, int C, int N, int M, float *gx,
                                       lionStream_t stream);

/* ---- E1: chamfer_3D.forward / .backward, chamfer3D/chamfer_cuda.cpp:17-33 ----------------
 * xyz1 f32[B,N,3], xyz2 f32[B,M,3] (point-major) -> dist1 f32[B,N], idx1 i32[B,N],
 * dist2 f32[B,M], idx2 i32[B,M]; lowest index wins ties (chamfer3D.cu:36,126).
 * backward: gxyz1 f32[B,N,3], gxyz2 f32[B,M,3] fully written (chamfer3D.cu:155-185). */
int lion_chamfer_forward(const float *xyz1, const float *xyz2, int B, int N, int M,
                         float *dist1, float *dist2, int32_t *idx1, int32_t *idx2,
                         lionStream_t stream);
int lion_chamfer_backward(const float *xyz1, const float *xyz2, const float *gdist1,
                          const float *gdist2, const int32_t *idx1, const int32_t *idx2, int B,
                          int N, int M, float *gxyz1, float *gxyz2, lionStream_t stream);
/* Chamfer reconstruction loss (utils/model_helper.py:43-52: 'chamfer' = the mean over points of both directions, 'cd_sum' = their
 * sum) on top of lion_chamfer_forward's outputs, and its gradient without atomics (stands for chamfer3D.cu:155-185 under that loss).
 * loss_reduce: loss f32[B], loss[b] = s1 * sum_j dist1[b,j] + s2 * sum_k dist2[b,k]; fixed order: a lane adds dist[b, t], [t + 256],
 *   ... in fp32 (the longest chain has P = ceil(max(N,M) / 256) terms), the 256 lane sums of each direction are added in double by a
 *   fixed tree, loss[b] = (float)((double)s1 * S1 + (double)s2 * S2).
 * loss_backward: gloss f32[B] (device memory) = d(objective)/d(loss); gxyz1 f32[B,N,3] / gxyz2 f32[B,M,3] are fully written by plain
 *   stores (no pre-zeroing); either may be NULL and that direction is skipped (both NULL: LION_EINVAL).  Gather form, one rounding
 *   per written operation, c1 = 2 * (gloss[b] * s1), c2 = 2 * (gloss[b] * s2):
 *     gxyz1[b,j] = c1 * (x1[j] - x2[idx1[j]])                 -- the own term first
 *                  + c2 * (x1[j] - x2[k])  for every k with idx2[b,k] == j, added one by one in ascending k (a single fp32 chain)
 *     gxyz2[b,k] = c2 * (x2[k] - x1[idx2[k]])  + c1 * (x2[k] - x1[j])  for every j with idx1[b,j] == k, in ascending j
 *   -> the same bits on every run and on every rank; lion_chamfer_backward's float atomics add in arrival order. */
int lion_chamfer_loss_reduce(const float *dist1, const float *dist2, int B, int N, int M, float s1,
                             float s2, float *loss, lionStream_t stream);
int lion_chamfer_loss_backward(const float *xyz1, const float *xyz2, const int32_t *idx1,
                               const int32_t *idx2, const float *gloss, int B, int N, int M, float s1,
                               float s2, float *gxyz1, float *gxyz2, lionStream_t stream);

/* ---- E2: emd_ext.approxmatch_forward / matchcost_forward / matchcost_backward ------------
 * PyTorchEMD/cuda/emd.cpp:7-27 (emd_kernel.cu:24-156, :199-241, :285-353).
 * xyz1 f32[B,N,3], xyz2 f32[B,M,3] -> match f32[B,M,N]; cost f32[B]. */
size_t lion_emd_workspace_bytes(int B, int N, int M);
int lion_emd_approxmatch(const float *xyz1, const float *xyz2, int B, int N, int M,
                         float *match, void *ws, size_t ws_bytes, lionStream_t stream);
/* evaluation path (emd_nograd.py:19-44): approxmatch + matchcost without the [B,N,M] match matrix -> cost f32[B] */
int lion_emd_cost(const float *xyz1, const float *xyz2, int B, int N, int M, float *cost, void *ws,
                  size_t ws_bytes, lionStream_t stream);
int lion_emd_matchcost(const float *xyz1, const float *xyz2, const float *match, int B, int N,
                       int M, float *cost, void *ws, size_t ws_bytes, lionStream_t stream);
int lion_emd_matchcost_backward(const float *grad_cost, const float *xyz1, const float *xyz2,
                                const float *match, int B, int N, int M, float *grad1,
                                float *grad2, lionStream_t stream);
/* EMD reconstruction loss (utils/model_helper.py:82-96, 'emd' / 'chamfer_emd': earth_mover_distance = matchcost / N with the
 * match held constant in the gradient) without the [B,M,N] match matrix, forward and gradient.
 * loss_forward runs the auction of lion_emd_approxmatch operation for operation (the same expressions, quarters and merge
 *   order in every pass; pass 1 of a level rides on pass 3 of the level before it, whose distances it shares: 23 launches),
 *   so afterwards the first B * (2N + 2M) floats of the workspace hold the bits lion_emd_approxmatch leaves there on the same
 *   inputs.  Workspace layout of both, in floats:
 *     remainL[B,N] remainR[B,M] ratioL[B,N] ratioR[B,M] partial[B,ceil(N/256)] costrow[B,N]   (lion_emd_workspace_bytes)
 *   With E = __expf(level * |x1[k] - x2[l]|^2) and one rounding per written operation, per level (10 of them, in order):
 *     pass 3, row k:     w = (E * ratioL[k]) * ratioR[l];  crow += |..|^2 * w;  g += w * (x1[k] - x2[l])      (g: g1u != NULL)
 *       each sum runs over l ascending inside the four 256-element quarters of every 1024 tile, the four partial sums merged
 *       ((q0 + q1) + q2) + q3;  costrow[b,k] (+)= crow,  g1u[b,k,:] (+)= 2 * g: the first level stores, later levels add.
 *     pass 2, column l:  v += (E * ratioL[k]) * (x2[l] - x1[k]) over k, same quarters and merge, beside the auction's own sum;
 *       once ratioR[l] of the level is known  g2u[b,l,:] (+)= (2 * ratioR[l]) * v                              (g2u != NULL)
 *   loss[b] = (sum_k costrow[b,k]) / (float)N, the sum in lion_emd_cost's order.  loss f32[B], g1u f32[B,N,3], g2u f32[B,M,3]
 *   are fully written by plain stores (no pre-zeroing, no atomics); g1u and g2u may each be NULL and that gradient is compiled
 *   out (both NULL: the match-free cost on the literal auction).  g1u / g2u are d(N * loss)/d(xyz1) / d(xyz2).
 * loss_backward: one launch; gloss f32[B] (device memory) = d(objective)/d(loss);  c = gloss[b] / (float)N,
 *   gxyz1[b] = c * g1u[b], gxyz2[b] = c * g2u[b].  A direction is its pair (g1u, gxyz1) / (g2u, gxyz2): both NULL skips it,
 *   one NULL of a pair or both directions skipped is LION_EINVAL. */
int lion_emd_loss_forward(const float *xyz1, const float *xyz2, int B, int N, int M, float *loss,
                          float *g1u, float *g2u, void *ws, size_t ws_bytes, lionStream_t stream);
int lion_emd_loss_backward(const float *gloss, const float *g1u, const float *g2u, int B, int N, int M,
                           float *gxyz1, float *gxyz2, lionStream_t stream);

/* ---- D1: one denoiser update, utils/diffusion_pvd.py -------------------------------------
 * DDIM (:451-467): out = x*s + (c*eps + sigma*z).            z may be NULL when sigma == 0.
 * DDPM (:283-296 + get_q_posterior_mean :475-486):
 *   t>0 : out = k_outer*(x - k_a*eps/k_b) + scale*z*temp
 *   t==0: out = k_outer*(x - k_a*eps)
 * out may alias x. */
int lion_ddim_update(const float *x, const float *eps, const float *z, size_t numel, float s,
                     float c, float sigma, float *out, lionStream_t stream);
int lion_ddpm_update(const float *x, const float *eps, const float *z, size_t numel,
                     int t_is_zero, float k_outer, float k_a, float k_b, float scale,
                     float temp, float *out, lionStream_t stream);
/* The same updates for a chain that is replayed from ONE captured graph (whole-step capture, noise
 * on the device): the host supplies nothing per step.
 *   table f32[n_steps][8] = {t_model, a0..a5, -} per step, counter i32[1] (device), cur f32[8] (device).
 * lion_chain_begin_step: i = clamp(*counter); t_out[0..B) = table[i][0]; cur[0..7) = table[i][0..7),
 *   cur[7] = bits(i); *counter = i + 1.
 * lion_chain_update_noise: z ~ N(0,1) drawn in the kernel (Philox4x32-10, key = the 64-bit seed in device memory, counter = (element/4,
 *   cur step, stream_id); Box-Muller) replacing the reference's per-step CPU randn + H2D copy
 *   (diffusion_pvd.py:465-466);  mode 0 (DDIM): out = x*a0 + (a1*eps + a2*z);
 *   mode 1 (DDPM): a5 != 0: out = a0*(x - a1*eps), else out = a0*(x - a1*eps/a2) + (a3*z)*a4.
 *   z_out (may be NULL) receives the noise that was used (tests / trajectories).  out may alias x. */
int lion_chain_begin_step(const float *table, int n_steps, int32_t *counter, float *t_out, int B, float *cur,
                          lionStream_t stream);
int lion_chain_update_noise(int mode, const float *x, const float *eps, size_t numel, const float *cur,
                            const uint32_t *seed /* device u32[2]: lo, hi */, uint32_t stream_id, float *out,
                            float *z_out, lionStream_t stream);
/* Round 6 -- no ATen kernel inside a captured step.  lion_chain_begin_step_temb additionally copies row i of the chain's
 * time-embedding table temb_table f32[n_steps][temb_width] to temb_out (was an index_select per step).
 * lion_chain_update_noise_cm: x / out f32[B][N][4] (the point-major latent of the local prior, latent_dim 1), eps_cm the
 * denoiser's CHANNEL-major output f32[B][4][N] -- the permute(0, 2, 1).contiguous() of
 * models/latent_points_ada_localprior.py:84 folded into the update's read; same arithmetic, same Philox counters. */
int lion_chain_begin_step_temb(const float *table, int n_steps, int32_t *counter, float *t_out, int B, float *cur,
                               const float *temb_table, int temb_width, float *temb_out, lionStream_t stream);
int lion_chain_update_noise_cm(int mode, const float *x, const float *eps_cm, int B, int N, const float *cur,
                               const uint32_t *seed, uint32_t stream_id, float *out, float *z_out, lionStream_t stream);
/* DPM-Solver++(2M) (Lu, Zhou, Bao, Chen, Li, Zhu 2022, Algorithm 2), the second-order multistep solver of the probability-flow
 * ODE in data-prediction form: one step t -> n over numel floats, every written operation rounded once (no fma):
 *   x0  = a0*(x - a1*eps)                          a0 = 1/alpha_t, a1 = sigma_t: the model's data prediction
 *   D   = a5 == 0 ? a4*x0 : a4*x0 + a5*hist        a4 = 1 + 1/(2r), a5 = -1/(2r), hist = the previous step's x0
 *   out = a2*x + a3*D                              a2 = sigma_n/sigma_t, a3 = -alpha_n*expm1(-h)
 *   hist_out = x0
 * hist is NOT read when a5 == 0 (first step, order 1, last step).  out may alias x and hist_out may alias hist.  No noise.
 * lion_dpmpp_update takes the coefficients by value (hist may be NULL when a5 == 0); lion_chain_update_multistep reads
 * them from cur[1..6] in device memory, as lion_chain_begin_step leaves them -- the last launch of a captured step;
 * lion_chain_update_multistep_cm is that update on x / hist / out / hist_out f32[B][N][4] and the denoiser's channel-major
 * eps_cm f32[B][4][N], as lion_chain_update_noise_cm reads them.
 * LION_EINVAL before any launch: a NULL pointer (but hist, as said), numel == 0 / B <= 0 / N <= 0, or x, eps, hist, out or
 * hist_out not 16-byte aligned (eps_cm is read element by element and may have any alignment). */
int lion_dpmpp_update(const float *x, const float *eps, const float *hist, size_t numel, float a0, float a1, float a2,
                      float a3, float a4, float a5, float *out, float *hist_out, lionStream_t stream);
int lion_chain_update_multistep(const float *x, const float *eps, const float *hist, size_t numel, const float *cur,
                                float *out, float *hist_out, lionStream_t stream);
int lion_chain_update_multistep_cm(const float *x, const float *eps_cm, const float *hist, int B, int N, const float *cur,
                                   float *out, float *hist_out, lionStream_t stream);
/* SDE-DPM-Solver++(2M) (the same paper, the SDE form of Algorithm 2): the multistep update above with other exponents in a2 and
 * a3 and one Gaussian term.  Same reads, same first three operations, every written operation rounded once (no fma):
 *   x0  = a0*(x - a1*eps);   D = a5 == 0 ? a4*x0 : a4*x0 + a5*hist;   hist_out = x0
 *   out = (a2*x + a3*D) + a6*z        when a6 != 0
 *   out =  a2*x + a3*D                when a6 == 0: nothing is drawn, neither z_in nor seed is read
 *   a2 = (sigma_n/sigma_t)*exp(-h), a3 = -alpha_n*expm1(-2h), a6 = sigma_n*sqrt(-expm1(-2h))
 * z = z_in where z_in != NULL, else z ~ N(0,1) drawn in the kernel by the chain's generator, the device function of
 * lion_chain_update_noise, at counter = (element/4, step word, stream_id) under the 64-bit seed in device memory: for the same
 * seed, step index and stream_id it is the z of lion_chain_update_noise, bit for bit.  z_out (may be NULL) receives the z that
 * was used, zeros when a6 == 0.  hist is NOT read when a5 == 0; out may alias x and hist_out may alias hist.
 * lion_sde_dpmpp_update takes coefficients and step word by value (the eager loop; hist may be NULL when a5 == 0, z_in and
 * seed both NULL only when a6 == 0).  lion_chain_update_multistep_noise reads a0..a5 from cur[1..6] and the step index i from
 * cur[7] as lion_chain_begin_step leaves them (cur has no room for a6), and a6 from table[8*i + 7], the schedule table the
 * step was begun on: the last launch of a captured step.  lion_chain_update_multistep_noise_cm is that update on
 * x / hist / out / hist_out / z_out f32[B][N][4] and the denoiser's channel-major eps_cm f32[B][4][N].
 * LION_EINVAL before any launch: a NULL pointer (but hist, z_in, seed, z_out, as said), numel == 0 / B <= 0 / N <= 0, or x,
 * eps, hist, z_in, out, hist_out or z_out not 16-byte aligned (eps_cm may have any alignment). */
int lion_sde_dpmpp_update(const float *x, const float *eps, const float *hist, const float *z_in, size_t numel, float a0,
                          float a1, float a2, float a3, float a4, float a5, float a6,
                          const uint32_t *seed /* device u32[2]: lo, hi */, uint32_t step_word, uint32_t stream_id, float *out,
                          float *hist_out, float *z_out, lionStream_t stream);
int lion_chain_update_multistep_noise(const float *x, const float *eps, const float *hist, size_t numel, const float *cur,
                                      const float *table, const uint32_t *seed, uint32_t stream_id, float *out,
                                      float *hist_out, float *z_out, lionStream_t stream);
int lion_chain_update_multistep_noise_cm(const float *x, const float *eps_cm, const float *hist, int B, int N, const float *cur,
                                         const float *table, const uint32_t *seed, uint32_t stream_id, float *out,
                                         float *hist_out, float *z_out, lionStream_t stream);
/* Deterministic encoder: refined DDIM inversion, the inverse of the first-order solver step (DPM-Solver++ order 1 = DDIM with
 * kappa = 0).  The decoder step t -> n is x_n = s'*x_t + c'*eps(x_t, t); its exact inverse is the implicit equation
 * x_t = s*x_n + c*eps(x_t, t) with s = alpha_t/alpha_n, c = sigma_t - sigma_n*s, solved by fixed-point iteration from the
 * predictor eps(x_n, n).  One row of that iteration over numel floats, every written operation rounded once (no fma):
 *   out = a0*base + a1*eps                         a0 = s, a1 = c; base = x_n, eps = the model's output at the current iterate
 *   if (a2 != 0) base_out = out                    a2 = commit: the leg's last row hands its iterate on as the next base
 * base_out is neither read nor written when a2 == 0.  out may alias base or the buffer the model read, base_out may alias base.
 * lion_ddim_encode_update takes the coefficients by value (the eager loop; base_out may be NULL when a2 == 0);
 * lion_chain_update_encode reads them from cur[1..3] in device memory, as lion_chain_begin_step leaves them -- the last launch
 * of a captured step, base_out required; lion_chain_update_encode_cm is that update on base / out / base_out f32[B][N][4] and
 * the denoiser's channel-major eps_cm f32[B][4][N], as lion_chain_update_multistep_cm reads it.
 * LION_EINVAL before any launch: a NULL pointer (but base_out, as said), numel == 0 / B <= 0 / N <= 0, or base, eps, out or
 * base_out not 16-byte aligned (eps_cm is read element by element and may have any alignment). */
int lion_ddim_encode_update(const float *base, const float *eps, size_t numel, float a0, float a1, float a2, float *out,
                            float *base_out, lionStream_t stream);
int lion_chain_update_encode(const float *base, const float *eps, size_t numel, const float *cur, float *out, float *base_out,
                             lionStream_t stream);
int lion_chain_update_encode_cm(const float *base, const float *eps_cm, int B, int N, const float *cur, float *out,
                                float *base_out, lionStream_t stream);
/* The forward-process draw that starts a chain at an intermediate step (diffuse-denoise; sample_q of
 * utils/diffusion_pvd.py:105-113 with the scalars of iw_quantities_t :44-103):
 *   out = (m*x0) + (s*z)        two products and one sum, each rounded once (no fma)
 * over numel floats, any numel.  z = z_in where z_in != NULL (the given-noise path); else z ~ N(0,1) is drawn in the kernel
 * with the chain's generator (Philox4x32-10 keyed by the 64-bit seed in device memory, Box-Muller: the device function of
 * lion_chain_update_noise) at counter = (element/4, LION_DIFFUSE_STEP_WORD, stream_id).  A chain step's counter holds its
 * index into the schedule table there, 0 <= i < n_steps <= INT_MAX, so no step of any chain can have this word and a draw
 * never coincides with a step's noise under the same seed and stream_id.  The counter goes by element: a call on n elements
 * draws the prefix of a call on more.  z_out (may be NULL) receives the z that was used; out may alias x0.  Pointers that are
 * all 16-byte aligned take one 16-byte access per operand and lane, others and the last partial quad go element by element.
 * LION_EINVAL before any launch: x0 or out NULL, numel == 0, z_in and seed both NULL. */
#define LION_DIFFUSE_STEP_WORD 0xFFFFFFFFu
int lion_chain_diffuse(const float *x0, const float *z_in, size_t numel, float m, float s,
                       const uint32_t *seed /* device u32[2]: lo, hi; may be NULL with z_in */, uint32_t stream_id,
                       float *out, float *z_out, lionStream_t stream);
/* Per-sample keys: noise addressed by sample, not by batch position.  keys is device u32[2*B], the lo and hi word of sample b's
 * 64-bit Philox key at keys[2b], keys[2b+1]; n is the element count of ONE sample and must be a multiple of 4, so that no quad
 * straddles two samples.  The draw for elements 4j .. 4j+3 of sample b is the chain generator's (Philox4x32-10, Box-Muller: the
 * device function of lion_chain_update_noise) under keys[b] at counter = (j, step word, stream_id), j counted WITHIN the sample:
 * bit for bit what the single-seed entry points above draw for a one-sample tensor of n elements under seed = keys[b].  It
 * depends on neither B, nor b, nor the other keys.  (Grid: y = sample, x over the sample's quads; no division.)
 *   lion_philox_normal_keyed                   out f32[B][n] = z alone, at the given step word: a chain's start latent
 *                                              (LION_START_STEP_WORD), the per-step noise of an eager loop (the row's index)
 *   lion_chain_update_noise_keyed / _cm_keyed  lion_chain_update_noise / _cm (mode, `cur` contract, aliasing, z_out as there)
 *   lion_chain_update_multistep_noise_keyed / _cm_keyed   lion_chain_update_multistep_noise / _cm: the noise scale is
 *                                              table[8*i + 7]; where it is 0 nothing is drawn, no key is read, z_out gets zeros
 *   lion_chain_diffuse_keyed                   lion_chain_diffuse without z_in, at LION_DIFFUSE_STEP_WORD; any alignment
 * The _cm forms take x / out / z_out f32[B][N][4] and eps_cm f32[B][4][N]: n = 4*N there.
 * LION_START_STEP_WORD is the second reserved step word, beside LION_DIFFUSE_STEP_WORD: a chain step's word is its row index,
 * which is below the table's capacity (an int), so neither reserved word can collide with a step's, nor with each other.
 * LION_EINVAL before any launch: a NULL required pointer (z_out may be NULL), B <= 0 or B > 65535, n <= 0 / N <= 0, n % 4 != 0,
 * a mode outside {0, 1}, or (all but lion_chain_diffuse_keyed) a pointer other than eps_cm and keys not 16-byte aligned. */
#define LION_START_STEP_WORD 0xFFFFFFFEu
int lion_philox_normal_keyed(const uint32_t *keys /* device u32[2*B] */, int B, int n, uint32_t step_word, uint32_t stream_id,
                             float *out, lionStream_t stream);
int lion_chain_update_noise_keyed(int mode, const float *x, const float *eps, int B, int n, const float *cur,
                                  const uint32_t *keys, uint32_t stream_id, float *out, float *z_out, lionStream_t stream);
int lion_chain_update_noise_cm_keyed(int mode, const float *x, const float *eps_cm, int B, int N, const float *cur,
                                     const uint32_t *keys, uint32_t stream_id, float *out, float *z_out, lionStream_t stream);
int lion_chain_update_multistep_noise_keyed(const float *x, const float *eps, const float *hist, int B, int n, const float *cur,
                                            const float *table, const uint32_t *keys, uint32_t stream_id, float *out,
                                            float *hist_out, float *z_out, lionStream_t stream);
int lion_chain_update_multistep_noise_cm_keyed(const float *x, const float *eps_cm, const float *hist, int B, int N,
                                               const float *cur, const float *table, const uint32_t *keys, uint32_t stream_id,
                                               float *out, float *hist_out, float *z_out, lionStream_t stream);
int lion_chain_diffuse_keyed(const float *x0, int B, int n, float m, float s, const uint32_t *keys, uint32_t stream_id,
                             float *out, float *z_out, lionStream_t stream);
/* Per-sample start steps: the keyed DDIM / DDPM update and the keyed forward draw with one start per sample,
 * on the keyed kernels' grid (x over a sample's quads, y = sample: what a sample does is uniform per workgroup).
 *   lion_chain_update_noise_keyed_from / _cm_keyed_from
 *       first_row is device int32[B]; i is the row index in cur[7], as lion_chain_begin_step leaves it.  Where i < first_row[b]
 *       sample b is HELD: out[b] = x[b] bit for bit (nothing is stored where out == x), nothing is drawn, no key is read and
 *       z_out[b] = 0.  Otherwise sample b gets exactly the arithmetic and the draw of lion_chain_update_noise_keyed / _cm_keyed
 *       for that row's coefficients cur[1..6], with step word i - first_row[b]: the sample counts its own rows, so its noise is
 *       that of a chain which started at its first row.  out may alias x.
 *   lion_chain_diffuse_keyed_at
 *       ms is device f32[B][2] = (m_b, s_b): sample b is lion_chain_diffuse_keyed with (m_b, s_b), bit for bit.  A sample with
 *       m_b == 1 and s_b == 0 is copied bit for bit (not stored where out == x0), draws nothing, and its z_out is 0: "start 0".
 * LION_EINVAL before any launch: the rules of the keyed forms above (lion_chain_diffuse_keyed's for the draw), or a NULL
 * first_row / ms. */
int lion_chain_update_noise_keyed_from(int mode, const float *x, const float *eps, int B, int n, const float *cur,
                                       const int32_t *first_row /* device i32[B] */, const uint32_t *keys, uint32_t stream_id,
                                       float *out, float *z_out, lionStream_t stream);
int lion_chain_update_noise_cm_keyed_from(int mode, const float *x, const float *eps_cm, int B, int N, const float *cur,
                                          const int32_t *first_row, const uint32_t *keys, uint32_t stream_id, float *out,
                                          float *z_out, lionStream_t stream);
int lion_chain_diffuse_keyed_at(const float *x0, int B, int n, const float *ms /* device f32[B][2] */, const uint32_t *keys,
                                uint32_t stream_id, float *out, float *z_out, lionStream_t stream);
/* Known region: the per-sample-start update with part of the state given -- RePaint's known-region
 * conditioning (Lugmayr et al. 2022, Algorithm 1 without its resampling jumps), one byte per quad, in the kernel that ends the
 * keyed step.  Same grid as the forms above.
 *   known_x0         f32 laid out like x: the clean values
 *   keep             device u8[B][n/4] (cm: [B][N]), one byte per quad (cm: per point); non-zero = kept
 *   known_ms         device f32[rows][2], read at row i = cur[7] as (m, s): the forward process's scalars of the noise level the
 *                    state has AFTER row i; the last row of a chain holds (1, 0)
 *   first_row        as in the "_from" forms, or NULL: every sample starts at row 0
 * For the quad at position j of sample b, with local = i - first_row[b]:
 *   local < 0        the whole sample is held exactly as the "_from" forms hold it, kept quads included
 *   keep == 0        exactly the arithmetic, the draw (step word local, stream_id) and the z_out of the "_from" forms
 *   kept, s != 0     out = (m*x0) + (s*z'), two products and a sum, each rounded once (lion_chain_diffuse's arithmetic); z' is
 *                    the chain generator's draw under keys[b] at counter (j, local, known_stream_id); z_out receives z'; eps and
 *                    x are not read for this quad
 *   kept, s == 0     out = x0 bit for bit, nothing is drawn, z_out = 0
 * out may alias x; modes 0 and 1 as in the sibling entry points.
 * LION_EINVAL before any launch: the rules of the keyed forms above (known_x0 counts among the 16-byte aligned pointers), a
 * NULL known_x0, keep or known_ms, or known_stream_id == stream_id. */
int lion_chain_update_noise_keyed_known(int mode, const float *x, const float *eps, int B, int n, const float *cur,
                                        const int32_t *first_row /* device i32[B], or NULL */, const uint32_t *keys,
                                        uint32_t stream_id, const float *known_x0, const uint8_t *keep /* device u8[B][n/4] */,
                                        const float *known_ms /* device f32[rows][2] */, uint32_t known_stream_id, float *out,
                                        float *z_out, lionStream_t stream);
int lion_chain_update_noise_cm_keyed_known(int mode, const float *x, const float *eps_cm, int B, int N, const float *cur,
                                           const int32_t *first_row, const uint32_t *keys, uint32_t stream_id,
                                           const float *known_x0, const uint8_t *keep, const float *known_ms,
                                           uint32_t known_stream_id, float *out, float *z_out, lionStream_t stream);
/* Known region with resampling jumps: the "_known" pair with RePaint's jumps back up the chain (Lugmayr et
 * al. 2022, Algorithm 1, lines 9-10), the j one-step transitions of a jump composed into one draw.  Arguments of the "_known"
 * pair, and behind known_stream_id:
 *   known_jump          device f32[rows][2], read at row i = cur[7] as (mf, sf): the forward move that ends the row, from the
 *                       level the step leaves the state at to the level known_ms[i] names; (1, 0) where the row has none
 *   resample_stream_id  the Philox stream of the jumps' draws
 * A held sample and a kept quad are exactly those of the "_known" pair (known_ms[i] is the level BEHIND the jump).  A quad that
 * is not kept takes the "_known" update o and then, where sf != 0,
 *   out = (mf*o) + (sf*z''), two products and a sum, each rounded once (lion_chain_diffuse's arithmetic); z'' is the draw under
 *   keys[b] at counter (j, local, resample_stream_id); z_out still receives the step's own z.
 * A row with sf == 0 gives the bits of the "_known" entry point.
 * LION_EINVAL before any launch: everything the "_known" pair refuses, a NULL known_jump, or resample_stream_id equal to
 * stream_id or known_stream_id. */
int lion_chain_update_noise_keyed_known_resample(int mode, const float *x, const float *eps, int B, int n, const float *cur,
                                                 const int32_t *first_row, const uint32_t *keys, uint32_t stream_id,
                                                 const float *known_x0, const uint8_t *keep, const float *known_ms,
                                                 uint32_t known_stream_id, const float *known_jump /* device f32[rows][2] */,
                                                 uint32_t resample_stream_id, float *out, float *z_out, lionStream_t stream);
int lion_chain_update_noise_cm_keyed_known_resample(int mode, const float *x, const float *eps_cm, int B, int N,
                                                    const float *cur, const int32_t *first_row, const uint32_t *keys,
                                                    uint32_t stream_id, const float *known_x0, const uint8_t *keep,
                                                    const float *known_ms, uint32_t known_stream_id, const float *known_jump,
                                                    uint32_t resample_stream_id, float *out, float *z_out,
                                                    lionStream_t stream);
/* Inputs of guided synthesis (csrc/perturb.hip): perturbed copies of clouds x f32[B][N][3], every cloud on its
 * own and under its own key (keys as above).  One Philox4x32-10 call per output point at counter = (point index WITHIN the
 * sample, a reserved step word, stream_id), words w0..w3; a fraction is u(w) = (w >> 8) * 2^-24, exact.  LION_VOXEL_STEP_WORD
 * and LION_PERTURB_STEP_WORD are the third and fourth reserved step words: no chain step, start latent or forward draw
 * shares a counter with them.  Every written operation on a coordinate is rounded once (no fma); what selects a face or a
 * point is integer arithmetic; no atomics: the output is bit-reproducible and depends on neither B, nor b, nor the other keys.
 *
 * lion_voxel_surface_points_keyed: out f32[B][K][3] = K points on the surface of the cloud's voxelisation at resolution r.
 *   Box: mn, mx = the per-axis min and max of the points; c = (mn + mx)*0.5 per axis; h = the largest (mx - mn)*0.5 over the
 *   axes, 1 where that is 0; lo = c - h per axis; s = (2h)/r; inv = r/(2h).
 *   Occupancy: point p sets voxel i_axis = clamp((int)floorf((p - lo)*inv), 0, r-1), flat id x*r*r + y*r + z.
 *   Faces: face f = 0..5 = -x, +x, -y, +y, -z, +z of an occupied voxel is exposed when the neighbour across it is empty or
 *   outside the grid; the exposed faces are numbered in ascending (flat id, f), F of them (F >= 6); faces_out[b] = F.
 *   Point k: face (uint64(w0)*F) >> 32 of voxel (ix, iy, iz); the grid coordinate t is i on a - face and i + 1 on a + face
 *   along the face's axis, i + u(w1) and i + u(w2) along the other two in ascending axis order; out = lo + t*s per axis.
 *   One workgroup per cloud, every table in LDS: lion_voxel_surface_workspace_bytes is 0 for every shape and ws may be NULL
 *   (the parameters keep the call's shape should a finer grid ever spill).
 *   LION_EINVAL before any launch: x, keys or out NULL (faces_out may be NULL), B <= 0 or B > 65535, N <= 0, K <= 0, r < 1 or
 *   r > 32, ws_bytes below lion_voxel_surface_workspace_bytes or ws NULL where that is not 0.
 * lion_perturb_points_keyed: out f32[B][N][3]; out must not overlap x.
 *   mode 0 (uniform noise):  out = x + (p0*(2*u(w_axis) - 1)) per coordinate, axis = 0, 1, 2.
 *   mode 1 (outliers):       where w3 < floor(p0 * 2^32) (in double from the float p0, saturated at 2^32 - 1) the point becomes
 *                            mn + u(w_axis)*(mx - mn) per axis, mn / mx the cloud's own bounding box as above; else it is copied.
 *   LION_EINVAL before any launch: x, keys or out NULL, B <= 0 or B > 65535, N <= 0, a mode outside {0, 1}, p0 negative or
 *   NaN, p0 > 1 in mode 1.
 * Normal noise out = x + sigma*z is lion_chain_diffuse_keyed with m = 1, s = sigma, bit for bit. */
#define LION_VOXEL_STEP_WORD 0xFFFFFFFDu
#define LION_PERTURB_STEP_WORD 0xFFFFFFFCu
size_t lion_voxel_surface_workspace_bytes(int B, int N, int r, int K);
int lion_voxel_surface_points_keyed(const float *x, int B, int N, int r, const uint32_t *keys /* device u32[2*B] */,
                                    uint32_t stream_id, int K, float *out, int32_t *faces_out /* device i32[B], may be NULL */,
                                    void *ws, size_t ws_bytes, lionStream_t stream);
int lion_perturb_points_keyed(int mode, const float *x, int B, int N, float p0, const uint32_t *keys, uint32_t stream_id,
                              float *out, lionStream_t stream);
/* Voxel grids as inputs of guided synthesis and the voxel IoU (csrc/perturb.hip): the occupancy grid that
 * lion_voxel_surface_points_keyed builds and discards, as an object of its own.  The contract is the one above: one rounding
 * per written operation, integer arithmetic for everything that selects or counts, no atomics, one workgroup per cloud, no
 * workspace, no allocation, no host synchronisation (capturable); a sample's output depends on neither B nor b.
 *   Frame f32[4] = (lo_x, lo_y, lo_z, side): the cube a grid covers.  s = side/r, inv = r/side.  A cloud's OWN frame is the box
 *   above: lo = c - h per axis, side = 2h -- s and inv then are the very values lion_voxel_surface_points_keyed uses.
 *   Grid u8[B][r][r][r], flat id x*r*r + y*r + z; a non-zero byte is an occupied voxel (the memory of a torch.bool tensor;
 *   inputs may hold any non-zero byte, outputs hold 0 or 1).
 * lion_voxel_occupancy: grid = the voxels of cloud x f32[B][N][3] in a frame: point p sets voxel i_axis =
 *   clamp((int)floorf((p - lo)*inv), 0, r-1) -- ALWAYS clamped, in the cloud's own frame (frame_in NULL; there the grid is exactly
 *   the occupancy of lion_voxel_surface_points_keyed) or in a given one (frame_in f32[B][4] on the device).  frame_out f32[B][4]
 *   (may be NULL) receives the frame that was used; clamped_out i32[B] (may be NULL) the number of points whose index the clamp
 *   changed on at least one axis.  LION_EINVAL before any launch: x or grid NULL, B <= 0 or B > 65535, N <= 0, r < 1 or r > 32.
 * lion_voxel_surface_points_grid_keyed: out f32[B][K][3] = K points on the exposed faces of the grid, in frame f32[B][4]:
 *   faces, their numbering, point k's draw at counter (k, LION_VOXEL_STEP_WORD, stream_id) and out = lo + t*s exactly as in
 *   lion_voxel_surface_points_keyed, so the grid and frame lion_voxel_occupancy reports for a cloud reproduce that entry point's
 *   output to the bit.  faces_out[b] = F.  An empty grid has F = 0 and every one of its K points is the frame's centre,
 *   lo + side*0.5 per axis.  LION_EINVAL before any launch: grid, frame, keys or out NULL (faces_out may be NULL), B <= 0 or
 *   B > 65535, K <= 0, r < 1 or r > 32.
 * lion_voxel_iou: counts i32[B][2] = (|A and B|, |A or B|) over the r^3 voxels of grids a and b, iou f32[B] (may be NULL) =
 *   (float)inter / (float)union, correctly rounded, and 1 where the union is empty.  LION_EINVAL before any launch: a, b or
 *   counts NULL, B <= 0 or B > 65535, r < 1 or r > 32.
 * Frames live on the device and cannot be vetted by the host: whatever a frame holds (a zero, negative, NaN or infinite
 * side), every LDS and global index is clamped into range before it is used -- a bad frame gives a meaningless grid or
 * meaningless points, never an access out of range. */
int lion_voxel_occupancy(const float *x, int B, int N, int r, const float *frame_in /* device f32[B][4] or NULL = own frame */,
                         uint8_t *grid, float *frame_out /* may be NULL */, int32_t *clamped_out /* may be NULL */,
                         lionStream_t stream);
int lion_voxel_surface_points_grid_keyed(const uint8_t *grid, const float *frame, int B, int r, const uint32_t *keys,
                                         uint32_t stream_id, int K, float *out, int32_t *faces_out /* may be NULL */,
                                         lionStream_t stream);
int lion_voxel_iou(const uint8_t *a, const uint8_t *b, int B, int r, int32_t *counts /* i32[B][2] = inter, union */,
                   float *iou /* f32[B], may be NULL */, lionStream_t stream);
/* x f32[B][N][D] (point-major latent; 3 <= D <= 8) -> channel-major all f32[B][D][N], coords f32[B][3][N] (rows 0-2),
 * rest f32[B][D-3][N]; each output may be NULL: the view / permute / slice / contiguous head of
 * models/latent_points_ada_localprior.py:72-84 + models/latent_points_ada.py:118-121 in one launch. */
int lion_latent_unpack(const float *x, int B, int N, int D, float *all, float *coords, float *rest, lionStream_t stream);
/* out f32[B][Ca+Ct][N] = cat(a f32[B][Ca][N], t[b*ld_t + c] broadcast along N): torch.cat([features, temb], dim=1) of
 * models/latent_points_ada.py:139,147 (temb = the time embedding expanded over the points).  N % 4 == 0. */
int lion_concat_broadcast(const float *a, const float *t, int B, int Ca, int Ct, int N, int ld_t, float *out,
                          lionStream_t stream);

/* ---- C3: nn.Conv3d(kernel 3, stride 1, padding 1) of PVConv, models/pvcnn2_ada.py:211-222 --------
 * fp32-input MFMA implicit GEMM (exact fp32).  Weights are re-packed once per weight tensor:
 * w f32[Cout,Cin,3,3,3] -> wp f32[ceil4(Cin),27,Cout] (lion_conv3d_packed_floats floats).
 * x f32[B,Cin,r,r,r] with Cin % 4 == 0, r in {8,16,32}, Cout % 32 == 0 -> y f32[B,Cout,r,r,r];
 * bias f32[Cout] or NULL.  Other shapes: LION_EUNSUPPORTED (callers keep the library convolution). */
size_t lion_conv3d_packed_floats(int Cout, int Cin);
int lion_conv3d_pack_weights(const float *w, int Cout, int Cin, float *wp, lionStream_t stream);
int lion_conv3d_k3_forward(const float *x, const float *wp, const float *bias, int B, int Cin,
                           int Cout, int r, float *y, lionStream_t stream);
/* training: the data gradient is lion_conv3d_k3_forward(gy, pack(mirrored, channel-swapped w)); the weight gradient
 * gw f32[Cout,Cin,3,3,3] = sum_{b,v} gy * shifted x runs on the same MFMA instruction with the voxels on the k axis
 * (ws: lion_conv3d_wgrad_workspace_floats floats of partial sums, reduced in a fixed order). */
size_t lion_conv3d_wgrad_workspace_floats(int B, int Cin, int Cout, int r);
int lion_conv3d_k3_wgrad(const float *x, const float *gy, int B, int Cin, int Cout, int r, float *gw, float *ws,
                         size_t ws_floats, lionStream_t stream);
/* the same gradient on the 16-bit matrix pipe at fp32 accuracy (round 4): both operands cut into fp16 pairs in registers
 * (one power-of-two scale per tensor), v_mfma_f32_32x32x16_f16 with 16 voxels on K, fp32 accumulation; same arguments and
 * workspace as lion_conv3d_k3_wgrad; Cin % 8 == 0, x / gy 16-byte aligned (LION_EUNSUPPORTED otherwise). */
int lion_conv3d_k3_wgrad_split(const float *x, const float *gy, int B, int Cin, int Cout, int r, float *gw, float *ws,
                               size_t ws_floats, lionStream_t stream);
/* TRAINING, round 6: the same gradient when x is a freshly voxelised grid (the first Conv3d of a PVConv, models/pvcnn2_ada.py:211):
 * cnt i32[B, r^3] = the voxelisation's per-voxel point counts (16-byte aligned).  Tiles without a point within one voxel add nothing
 * and are neither loaded nor multiplied (a one-workgroup-per-sample kernel derives the tile map first).  Without counts the split
 * kernel still skips the arithmetic of a tile whose staged window turns out to be all zero.  Workspace:
 * lion_conv3d_wgrad_sparse_workspace_floats (the dense size + the tile map). */
size_t lion_conv3d_wgrad_sparse_workspace_floats(int B, int Cin, int Cout, int r);
int lion_conv3d_k3_wgrad_split_sparse(const float *x, const float *gy, const int32_t *cnt, int B, int Cin, int Cout, int r,
                                      float *gw, float *ws, size_t ws_floats, lionStream_t stream);

/* ---- P2+P3+P4 folded into C3 / K4 (inference): PVConv.forward voxel branch, pvcnn2_ada.py:211-226 ----
 * conv -> AdaGN -> Swish -> conv -> AdaGN -> SE3d -> devoxelize without a single stand-alone pass over
 * the grid: the conv epilogue emits per-tile channel sums (stats f32[B,Cout,T,2], T =
 * lion_conv3d_stat_tiles(r, Cout, B, sparse): the spatial tiling depends on the shape), lion_groupnorm_fold turns them into per-(batch, channel) scalars
 * A, Bs (GroupNorm(G) x adaptive affine fac/gbias, models/adagn.py:61-64; fac/gbias rows are ld_fg floats
 * apart, so the two halves of the [B,2C] style projection are consumed in place) and the channel mean,
 * the next conv applies swish(x*A+Bs) while staging its input (pro_a/pro_b f32[B,Cin]), and
 * lion_trilinear_devoxelize_affine_forward interpolates scale*feat+shift (second AdaGN x SE gate). */
int lion_conv3d_stat_tiles(int r, int Cout, int B, int sparse); /* sparse = 1: the call will be given an occ */
int lion_conv3d_k3_fused_forward(const float *x, const float *wp, const float *bias, int B, int Cin,
                                 int Cout, int r, const float *pro_a, const float *pro_b, const float *pro_bias,
                                 const float *tconst, float *y, float *stats, int32_t *occ, lionStream_t stream);
/* The first convolution of a PVConv reads the voxelised grid (>= 94 % zeros); spatial tiles whose whole halo is
 * empty produce exactly bias.  occ i32[lion_conv3d_occupancy_ints(r,Cout,B)] (per-tile flags: 1 = some voxel of
 * the tile's halo holds a point; a work list, occupied tiles first; a queue counter) is derived from the
 * voxelisation's cnt i32[B,r^3]; passing it to a fused forward (only without pro_a/pro_b) skips the K loop of
 * empty tiles and balances the occupied ones over all CUs through the queue -- bit-identical output.  The queue
 * re-arms itself when the launch's last workgroup leaves (round 5): one buffer serves any number of launches in
 * stream order (never two concurrently).
 * Layout: [B*tiles flags][B*tiles work list][queue counter, exit counter, mode, pad].  Flag bits 0-3 = wave w's
 * 64-voxel block of the tile has a point within the margin (0 = empty tile), bit 8 = the tile's output has a reader
 * (consumer-aware buffers), bit 9 (margin-2 words) = occupied at margin 1.  These are the only words the shipped
 * kernels read (round 5's active-voxel bit maps belonged to the rejected compaction experiment and are gone). */
size_t lion_conv3d_occupancy_ints(int r, int Cout, int B);
/* The second convolution sees swish(AdaGN(conv1)): a per-channel constant c = swish(A*bias1+Bs) wherever conv1 saw no
 * point, plus a sparse delta.  lion_conv3d_const_response turns c into tconst f32[B][27][Cout], the exact response of
 * the convolution to the constant field for each of the 27 border configurations (wsum f32[27][Cin][Cout] = weights
 * summed over the in-grid taps); with pro_bias (= bias1) and tconst the fused forward convolves only the delta, adds
 * tconst in the epilogue, and may take an occ built with margin 2 (within fp32 rounding of the dense evaluation). */
int lion_conv3d_const_response(const float *wsum, const float *bias2, const float *bias1, const float *pro_a,
                               const float *pro_b, int B, int Cin, int Cout, float *tconst, lionStream_t stream);
int lion_conv3d_tile_occupancy(const int32_t *cnt, int B, int r, int Cout, int32_t *occ_m1, int32_t *occ_m2,
                               lionStream_t stream); /* margin 1 / margin 2 lists; either may be NULL; r in {16, 32} */
/* Round 5: the same with consumer_aware != 0 for the pair of a PVConv (pvcnn2_ada.py:206-233: conv on the voxelised grid
 * -> delta conv -> trilinear devoxelisation).  Nobody reads the first conv's output outside the tiles the second one
 * stages (a point within 2 voxels, and their neighbours), nor the second one's outside the tiles around the points: a
 * split-kernel launch that pops such a buffer writes NO output for an empty tile without a reader (its GroupNorm sums
 * are still produced, in closed form).  The rest of y is left as allocated.  With consumer_aware == 0 (and through
 * lion_conv3d_tile_occupancy) every voxel of y is written, as before. */
int lion_conv3d_tile_occupancy_aware(const int32_t *cnt, int B, int r, int Cout, int32_t *occ_m1, int32_t *occ_m2,
                                     int consumer_aware, lionStream_t stream);
int lion_groupnorm_fold(const float *stats, int B, int C, int T, int G, int voxels, const float *gamma,
                        const float *beta, const float *fac, const float *gbias, int ld_fg, float eps,
                        float *A, float *Bs, float *chmean, lionStream_t stream);
/* ---- C3 on the 16-bit matrix pipe at fp32 accuracy (csrc/conv3d_split.hip) -----------------------------------
 * The same convolution and the same modes as lion_conv3d_k3_fused_forward with every fp32 operand cut into two fp16
 * pieces (a = a_h + a_l/2048; main += W_h X_h, corr += W_h X_l + W_l X_h in fp32 accumulators; 3 MFMAs of
 * v_mfma_f32_32x32x16_f16 per K = 16 instead of 8 fp32 MFMAs) and block-scaled by exact powers of two (one scale per
 * weight tensor, one monotone scale per workgroup tile for the activations): error vs float64 of the fp32 kernel's
 * class (2.6e-7 rms), no clamp, any fp32 range.  Cin % 16 == 0, Cout % 32 == 0, r in {8,16,32}; otherwise
 * LION_EUNSUPPORTED (callers keep the fp32 kernel).
 *   wp: lion_conv3d_split_packed_halfs(Cout, Cin) uint16 (16-byte aligned), filled by lion_conv3d_split_pack_weights
 *       (3 small launches: max |w|, scale, cut);
 *   stats f32[B,Cout,lion_conv3d_split_stat_tiles(r,Cout),2]; occ / tconst exactly as for the fp32 kernel's sparse
 *   plan (lion_conv3d_tile_occupancy, lion_conv3d_const_response). */
size_t lion_conv3d_split_packed_halfs(int Cout, int Cin);
int lion_conv3d_split_pack_weights(const float *w, int Cout, int Cin, uint16_t *wp, lionStream_t stream);
int lion_conv3d_split_stat_tiles(int r, int Cout);
int lion_conv3d_k3_split_forward(const float *x, const uint16_t *wp, const float *bias, int B, int Cin, int Cout,
                                 int r, const float *pro_a, const float *pro_b, const float *pro_bias,
                                 const float *tconst, float *y, float *stats, int32_t *occ, lionStream_t stream);
/* ---- C3 at reduced precision, on purpose (csrc/conv3d_half.hip) ----------------------------------------------
 * lion_conv3d_k3_split_forward with ONE fp16 product per operand pair (main += W_h X_h, no low pieces, no corr): a third
 * of the MFMAs -- the P = 1 instantiation of the split kernel (csrc/conv3d_split_kernel.h).  Same arguments, same modes (prologue, tile sums, occ / tconst, consumer-aware levels), same tile geometry
 * (stats has lion_conv3d_split_stat_tiles(r, Cout) tiles) and the SAME packed weights -- wp from
 * lion_conv3d_split_pack_weights, of which only the hi pieces and the scale are read.  With the block scaling a hi piece is
 * the operand rounded to an 11-bit significand, so the result is conv(rne11(W), rne11(act(X))) accumulated in fp32:
 * |y - conv64(W, X)| <= 2^-10 * conv64(|W|, |X|) elementwise; no clamp, inf / nan propagate.  Inference only.
 * r in {16, 32}, Cin % 16 == 0, Cout % 32 == 0; anything else (r = 8 included, which stays on the split kernel) is
 * LION_EINVAL and nothing is written. */
int lion_conv3d_k3_half_forward(const float *x, const uint16_t *wp, const float *bias, int B, int Cin, int Cout,
                                int r, const float *pro_a, const float *pro_b, const float *pro_bias,
                                const float *tconst, float *y, float *stats, int32_t *occ, lionStream_t stream);
/* ---- D2: global denoiser, models/score_sde/resnet.py:60-90, :195-218 -----------------------------------
 * The 1x1 convs of the [B, C, 1, 1] style-latent network as 32-row GEMMs on channel-major activations
 * f32[nb][C][32] (batch padded to 32 per slab), split over K into lion_skinny_splits workgroup rows that write raw
 * partial tiles; the consumer's operand load sums the partials and applies the producer's bias / ReLU (+ an added
 * tensor: ResBlockSEDrop's x + t), lion_skinny_finish applies the squeeze-excite tail or the last layer's bias.
 * wp = lion_skinny_pack_weights(w f32[Cout,Cin]) (lion_skinny_packed_floats floats, tile-major, 4 k-steps per
 * 16-byte lane load).  Cout % 32 == 0. */
size_t lion_skinny_packed_floats(int Cout, int Cin);
int lion_skinny_pack_weights(const float *w, int Cout, int Cin, float *wp, lionStream_t stream);
int lion_skinny_splits(int Cin, int Cout);
int lion_skinny_gemm(const float *pin, int ks_in, const float *bias_in, int act_in, const float *addT,
                     const float *wp, int nb, int Cin, int Cout, float *pout, lionStream_t stream);
int lion_skinny_finish(const float *A, int ks_a, const float *bias_a, const float *Bp, int ks_b, const float *resid,
                       int nb, int C, int mode, float *y, lionStream_t stream);
/* Round 6: the second squeeze-excite GEMM of a residual block WITH the block's tail (resnet.py:77-86) in its epilogue:
 * y = resid + relu(sum_q A[q] + bias_a) * sigmoid(W act_in(sum pin + bias_in)) == lion_skinny_gemm + lion_skinny_finish(mode 1)
 * bit for bit, one launch.  Needs lion_skinny_splits(Cin, Cout) == 1. */
int lion_skinny_gemm_se_finish(const float *pin, int ks_in, const float *bias_in, int act_in, const float *wp, int nb, int Cin,
                               int Cout, const float *A, int ks_a, const float *bias_a, const float *resid, float *y,
                               lionStream_t stream);
/* For tests only: the two entry points above through the plain kernel (operand loads behind the weight loads, two chunks
 * ahead), which the library itself runs only for ks_in > 8.  Same arguments; the public entry points -- every load of a
 * round requested before the first wait -- equal them bit for bit (tests/test_skinny_roundtrips_gpu.py). */
int lion_internal_skinny_gemm_plain(const float *pin, int ks_in, const float *bias_in, int act_in, const float *addT,
                                    const float *wp, int nb, int Cin, int Cout, float *pout, lionStream_t stream);
int lion_internal_skinny_gemm_se_finish_plain(const float *pin, int ks_in, const float *bias_in, int act_in, const float *wp,
                                              int nb, int Cin, int Cout, const float *A, int ks_a, const float *bias_a,
                                              const float *resid, float *y, lionStream_t stream);
/* activations of the global denoiser [B, C, 1, 1] <-> the channel-major [ceil(B/32)][C][32] form its layers work on
 * (models/score_sde/resnet.py:195-218 keeps [B, C, 1, 1]); a / b: two tensors per launch (either may be NULL), row strides
 * lda / ldb in floats (0 = one row broadcast over the batch: the time embedding of a chain step). */
int lion_to_channel_major(const float *a, int lda, int Ca, float *oa, const float *b, int ldb, int Cb, float *ob, int B,
                          lionStream_t stream);
int lion_from_channel_major(const float *x, int B, int C, float *y, lionStream_t stream);
/* SE3d (pvcnn2_ada.py:27-41) on the folded scalars: A, Bs f32[B,C] are multiplied in place by
 * sigmoid(W2 relu(W1 (A*chmean + Bs))), w1 f32[H,C], w2 f32[C,H] (C <= 1024, H <= 128). */
/* lion_groupnorm_fold + lion_se_gate in one launch (C <= 256, H <= 128): the second AdaGN of a PVConv with its SE3d gate
 * (models/pvcnn2_ada.py:27-41, :219-226). */
int lion_groupnorm_fold_se(const float *stats, int B, int C, int T, int G, int voxels, const float *gamma,
                           const float *beta, const float *fac, const float *gbias, int ld_fg, float eps, const float *w1,
                           const float *w2, int H, float *A, float *Bs, lionStream_t stream);
/* For tests only: the same through the plain kernel, which requests the operands of each of its four phases behind the
 * barrier of the phase before; lion_groupnorm_fold_se requests them all in front of the first wait (for H in {4, 8, 16, 32}
 * and a 16-byte aligned w2; otherwise it runs this kernel) and equals it bit for bit (tests/test_small_launches_gpu.py). */
int lion_internal_groupnorm_fold_se_plain(const float *stats, int B, int C, int T, int G, int voxels, const float *gamma,
                                          const float *beta, const float *fac, const float *gbias, int ld_fg, float eps,
                                          const float *w1, const float *w2, int H, float *A, float *Bs, lionStream_t stream);
int lion_se_gate(const float *chmean, const float *w1, const float *w2, int B, int C, int H, float *A,
                 float *Bs, lionStream_t stream);
int lion_trilinear_devoxelize_affine_forward(const float *coords, const float *feat, const float *scale,
                                             const float *shift, int B, int C, int N, int r, float *out,
                                             lionStream_t stream);
/* K4 in two steps (r = 32, N <= 2048; inference): everything the coordinates alone decide -- which 32-byte pieces of the
 * z-rows some point interpolates from (trilinear_devox.cu:36-66), their slots in the kernel's LDS ring, every point's 8
 * corner offsets -- is computed once per cloud (lion_trilinear_devoxelize_plan), and each feature tensor devoxelised at
 * those coordinates starts its first DMA one round trip after the kernel begins (PVConv: four devoxelisations per
 * (cloud, r = 32) and forward, pvcnn2_ada.py:235-243).  plan: lion_devoxelize_plan_bytes(B, N, r) bytes (0 = shape not
 * covered), 16-byte aligned; coords must be the tensor the plan was made from; scale / shift both or neither (the affine
 * form of lion_trilinear_devoxelize_affine_forward).  Bit-identical to the one-step entry points. */
size_t lion_devoxelize_plan_bytes(int B, int N, int r);
int lion_trilinear_devoxelize_plan(const float *coords, int B, int N, int r, void *plan, size_t plan_bytes,
                                   lionStream_t stream);
int lion_trilinear_devoxelize_planned_forward(const void *plan, size_t plan_bytes, const float *coords, const float *feat,
                                              const float *scale, const float *shift, int B, int C, int N, int r,
                                              float *out, lionStream_t stream);

/* ---- P2+P3(+P6) for 1-D / 2-D SharedMLP layers (inference), pvcnn2_ada.py:120-164, :375-377 --------
 * after the 1x1 convolution: row sums -> lion_groupnorm_fold (T = 1) -> y = swish(x*A+Bs), optionally
 * reduced with max over the U neighbours of each centre.  x is [rows = B*C, L] (L = N or M*U). */
int lion_row_stats(const float *x, int rows, int L, float *stats, lionStream_t stream);
/* G1 itself: the 1x1 Conv1d / Conv2d of SharedMLP (pvcnn2_ada.py:120) as an fp32-MFMA GEMM over
 * x f32[B,Cin,L] (L = N or M*U) with the previous layer's AdaGN+Swish applied to the operand in flight
 * (pro_a/pro_b f32[B,Cin] or both NULL) and this layer's GroupNorm sums in the epilogue
 * (stats f32[B,Cout,lion_pwconv_stat_tiles(Cout,Cin,L),2] or NULL; fold with lion_groupnorm_fold).
 * w f32[Cout,Cin] -> wp f32[ceil2(Cin),ceil64(Cout)] once per weight (lion_pwconv_packed_floats floats).
 * Any Cout (channel tiles of 32..256 output rows; rows beyond Cout carry zero weights and are never stored); the
 * weight slice of a tile must fit LDS (150 KiB), otherwise LION_EUNSUPPORTED. */
size_t lion_pwconv_packed_floats(int Cout, int Cin);
int lion_pwconv_pack_weights(const float *w, int Cout, int Cin, float *wp, lionStream_t stream);
int lion_pwconv_stat_tiles(int Cout, int Cin, int L);
int lion_pwconv_forward(const float *x, const float *wp, const float *bias, int B, int Cin, int Cout, int L,
                        const float *pro_a, const float *pro_b, float *y, float *stats, lionStream_t stream);
/* The LAST layer of a set-abstraction MLP without its output (pvcnn2_ada.py:120-164 + :375-377: conv -> AdaGN -> Swish
 * -> max over the U = 32 neighbours of a centre; x f32[B,Cin,M*32]): call once with out_a == NULL -- only the GroupNorm
 * sums are written (stats as lion_pwconv_forward) --, fold them (lion_groupnorm_fold), call again with out_a / out_b
 * f32[B,Cout] = this layer's AdaGN scalars and ymax f32[B,Cout,M]: max_u swish(y*a+b), bit-identical to
 * lion_pwconv_forward + lion_affine_swish_max, while y (268 MB in the first set-abstraction module) is never stored.
 * LION_EUNSUPPORTED outside the large-activation tiling (L % 32 != 0, L <= 4096, small grids). */
int lion_pwconv_forward_max(const float *x, const float *wp, const float *bias, int B, int Cin, int Cout, int L,
                            const float *pro_a, const float *pro_b, const float *out_a, const float *out_b,
                            float *stats, float *ymax, lionStream_t stream);
/* G1 on the 16-bit matrix pipe at fp32 accuracy (csrc/pwconv_split.hip): same contract as lion_pwconv_forward with both
 * operands cut into fp16 hi / lo pieces (power-of-two block scaling per tensor for w, per column and 16-channel chunk for
 * the activation, fp32 accumulation; error within that of the fp32 MFMA chain).  w f32[Cout,Cin] -> wp once per weight
 * (lion_pwconv_split_packed_halfs uint16, 16-byte aligned); stats f32[B,Cout,lion_pwconv_split_stat_tiles(Cout,Cin,L),2].
 * Any Cout, Cin, L with Cin * L < 2^29. */
size_t lion_pwconv_split_packed_halfs(int Cout, int Cin);
int lion_pwconv_split_pack_weights(const float *w, int Cout, int Cin, uint16_t *wp, lionStream_t stream);
/* TRAINING: the packed form of W^T (the matrix of the data gradient, autograd's mm(W^T, gy)) from W f32[Cout,Cin] as stored and
 * wp = lion_pwconv_split_pack_weights(W) (its tail carries the tensor's scale, which the transposition does not change):
 * wpt = lion_pwconv_split_packed_halfs(Cin, Cout) uint16.  One launch; no transposed copy, no second pass for max |w|. */
int lion_pwconv_split_pack_weights_t(const float *w, int Cout, int Cin, const uint16_t *wp, uint16_t *wpt, lionStream_t stream);
int lion_pwconv_split_stat_tiles(int Cout, int Cin, int L);
int lion_pwconv_split_forward(const float *x, const uint16_t *wp, const float *bias, int B, int Cin, int Cout, int L,
                              const float *pro_a, const float *pro_b, float *y, float *stats, lionStream_t stream);
/* The FIRST layer of a set-abstraction MLP straight from the ungrouped tensors: lion_group_points_forward followed by
 * lion_pwconv_forward / lion_pwconv_split_forward (no prologue) without the [B, 3 + C, M, U] tensor between them.
 * coords f32[B,3,N], centers f32[B,3,M], feat f32[B,C,N] (NULL with C = 0), idx i32[B,M,U] (clamped to [0, N) as the
 * grouping kernel clamps it); Cin = 3 + C, L = M * U.  The operand of column (m, u) and channel k is
 * coords[b,k,idx[b,m,u]] - centers[b,k,m] for k < 3 (one IEEE subtraction) and feat[b,k-3,idx[b,m,u]] beyond.  wp, bias,
 * y f32[B,Cout,M,U] and stats (sized by lion_pwconv_stat_tiles / lion_pwconv_split_stat_tiles for (Cout, Cin, L)) as in
 * the ungrouped call; same kernels, tiles and k order: y and stats are bit-identical to the two calls. */
int lion_pwconv_grouped_forward(const float *coords, const float *centers, const float *feat, const int32_t *idx,
                                const float *wp, const float *bias, int B, int C, int N, int M, int U, int Cout, float *y,
                                float *stats, lionStream_t stream);
int lion_pwconv_split_grouped_forward(const float *coords, const float *centers, const float *feat, const int32_t *idx,
                                      const uint16_t *wp, const float *bias, int B, int C, int N, int M, int U, int Cout,
                                      float *y, float *stats, lionStream_t stream);
/* For tests only: the fp32 kernel of lion_pwconv_forward / lion_pwconv_forward_max / lion_pwconv_grouped_forward at ANY L
 * (never the short-activation kernel), with at most max_wg workgroups per (sample, channel tile) walking the column tiles
 * (<= 0: the library's own cap) and the weights through LDS (lds_weights 1), from L2 (0) or by the library's rule (< 0).
 * idx != NULL: the gathered operand (x unused, Cin = 3 + C, feat NULL when Cin = 3, L = M * U); out_a != NULL: the second
 * pass of the max form (y = ymax f32[B,Cout,L/32]); y == NULL: its first pass (sums only); otherwise y is stored. */
int lion_internal_pwconv_walk(const float *x, const float *wp, const float *bias, int B, int Cin, int Cout, int L,
                              const float *pro_a, const float *pro_b, const float *out_a, const float *out_b,
                              const float *coords, const float *centers, const float *feat, const int32_t *idx, int N, int U,
                              float *y, float *stats, int max_wg, int lds_weights, lionStream_t stream);
/* For tests only: the short-activation kernel (L <= 4096) in its plain form -- prologue scalars waited for before the first
 * operand is requested, each round of 32 k-steps requested after the previous round's MFMAs.  The public entries at such an
 * L request the operands in front of the first wait and one round ahead, and equal this one bit for bit
 * (tests/test_small_launches_gpu.py).  Arguments of lion_pwconv_forward; idx != NULL: the gathered operand (x unused,
 * Cin = 3 + C, feat NULL when Cin = 3, L = M * U, no prologue). */
int lion_internal_pwconv_small_plain(const float *x, const float *wp, const float *bias, int B, int Cin, int Cout, int L,
                                     const float *pro_a, const float *pro_b, const float *coords, const float *centers,
                                     const float *feat, const int32_t *idx, int N, int U, float *y, float *stats,
                                     lionStream_t stream);
/* ---- P5: LinearAttention (models/pvcnn2_ada.py:43-71) between its two 1x1 convolutions ---------------------
 * qkv f32[B, 3*H*D, N] (to_qkv's output, channel order (qkv, head, d)) -> out f32[B, H*D, N] (to_out's input):
 * softmax over the N points of every k row, ctx = softmax(k) v^T (D x D), out = ctx^T q.  D = 32 (every
 * LinearAttention of the models); one workgroup per (batch, head), fp32 MFMA. */
int lion_linear_attention_core(const float *qkv, int B, int H, int D, int N, float *out, lionStream_t stream);
/* For tests only: the kernel lion_linear_attention_core takes at N points, with (aligned != 0) or without 16-byte aligned
 * qkv and out -- 0 the plain kernel (N % 4 != 0 or unaligned), 1 k resident in LDS (N <= 1024), 2 streaming -- and the
 * plain kernel at any shape, which the other two equal bit for bit (tests/test_attention_roundtrips_gpu.py). */
int lion_internal_linear_attention_path(int N, int aligned);
int lion_internal_linear_attention_core_plain(const float *qkv, int B, int H, int D, int N, float *out, lionStream_t stream);
/* its gradient (training): gout f32[B, H*D, N] -> gqkv f32[B, 3*H*D, N] (softmax backward included; the row dot product
 * sum_n p gp is the 32 x 32 contraction sum_e gctx[d][e] ctx[d][e]: no second sweep over the points). */
int lion_linear_attention_core_backward(const float *qkv, const float *gout, int B, int H, int D, int N, float *gqkv,
                                        lionStream_t stream);
/* nn.Linear on [B,K] (time-embedding MLP, batched AdaGN style projections): y[b][o] = act(bias[o] + sum_k x[b][k] W[o][k]),
 * wp = lion_pwconv_pack_weights(W f32[O,K]); act 0 none / 1 relu / 2 leaky-relu(slope).  One launch, fixed summation
 * order (4 K-quarters combined in order). */
int lion_linear_forward(const float *x, const float *wp, const float *bias, int B, int K, int O, int act, float slope,
                        float *y, lionStream_t stream);
int lion_affine_swish(const float *x, const float *A, const float *Bs, int rows, int L, float *y,
                      lionStream_t stream);
int lion_affine_swish_max(const float *x, const float *A, const float *Bs, int rows, int M, int U,
                          float *y, lionStream_t stream);
/* y = swish(x * A + Bs) + addend (rows x L, same layout): the point branch's last activation with PVConv's residual sum
 * (models/pvcnn2_ada.py:276-278) behind it. */
/* emb f32[B, D]: [sin, cos] of (t_b * scale) * row_i, i < half (D = 2 half, or 2 half + 1 with a zero column):
 * models/latent_points_ada.py get_timestep_embedding (reference latent_points_ada.py:101-115) in one launch. */
int lion_timestep_embedding(const float *t, const float *row, float scale, int B, int half, int D, float *emb,
                            lionStream_t stream);
int lion_affine_swish_add(const float *x, const float *A, const float *Bs, const float *addend, int rows, int L, float *y,
                          lionStream_t stream);

/* ---- backward scatters without float atomics (training; K5, K8, K12-grad) -------------------------------------------
 * gx f32[B,C,bins] = sum over the entries e with idx[b,e] = bin of (w ? w[b,e] : 1) * gy[b,c, e mod S]:
 *   grouping backward (grouping.cu:58-80):            idx [B, M*U], w NULL,       gy [B,C,M*U], S = E = M*U, bins = N
 *   3-NN interpolation backward (neighbor_interpolate.cu:145-170): idx / w [B, 3*N], gy [B,C,N], S = N, E = 3N, bins = M
 *   devoxelize backward (trilinear_devox.cu:119-162):  idx / w [B, 8*N], gy [B,C,N], S = N, E = 8N, bins = r^3
 * The inverse index is built once per sample, every channel is a gather-sum in ascending entry order: deterministic
 * (the reference's atomicAdd order is not), and not bound by the LDS float-atomic rate (csrc/scatter_csr.hip). */
size_t lion_scatter_csr_workspace_bytes(int B, int E, int bins);
int lion_scatter_csr(const float *gy, const int32_t *idx, const float *w, int B, int C, int S, int E, int bins, void *ws,
                     size_t ws_bytes, float *gx, lionStream_t stream);

/* ---- weight gradient of the 1x1 convolutions (training): gw[o][i] = sum_b sum_l gy[b][o][l] x[b][i][l] --------------
 * x f32[B,Cin,L], gy f32[B,Cout,L] (16-byte aligned), gw f32[Cout,Cin]; ws from lion_pwconv_wgrad_workspace_bytes.  What
 * autograd's mm([O, B L] x [B L, I]) of models/pvcnn2_ada.py's SharedMLP layers computes, without the transposing copies;
 * exact fp32 products on the MFMA pipe, slices summed in fixed order (csrc/pwconv_wgrad.hip).  gb f32[Cout] or NULL: the bias
 * gradient sum_b sum_l gy[b][o][l], taken from the same staged rows of gy (no second pass over it). */
size_t lion_pwconv_wgrad_workspace_bytes(int B, int Cin, int Cout, int L);
int lion_pwconv_wgrad(const float *x, const float *gy, int B, int Cin, int Cout, int L, void *ws, size_t ws_bytes,
                      float *gw, float *gb, lionStream_t stream);

/* ---- training forms of GroupNorm / AdaGN (+ Swish): models/adagn.py:45-65, models/pvcnn2_ada.py:78-84 --------------
 * Per row (b, c) of length L a GroupNorm followed by per-(batch, channel) scalars and an activation is
 * y = act(A x + Bs) (act: 0 identity, 1 swish).  Forward: lion_row_stats + lion_affine_act.  Backward:
 * lion_affine_act_bwd_stats -> S f32[rows, 2] = {sum da, sum da x} with da = gy act'(A x + Bs); the caller combines them
 * into Q, R f32[rows] (group means of the normalisation's gradient) and the parameter gradients;
 * lion_affine_act_bwd_apply writes dx = A da + Q + R x.  (csrc/norm_train.hip, lion_amd/train_ops.py) */
/* the [B, C] scalar algebra of both directions (double inside).  fac / bias f32[B, *] with row strides (views of the
 * [B, 2C] AdaGN projection) or NULL (plain GroupNorm); dfac / dbias f32[B, *] with row stride d_stride (the halves of one [B, 2C] buffer, or C) may be NULL; pw f32[B,C,3] = per-sample terms of the
 * GroupNorm weight / bias gradients (the caller sums them over the batch). */
int lion_gn_train_fold(const float *stats, const float *gw, const float *gb, const float *fac, int fac_stride,
                       const float *bias, int bias_stride, int B, int C, int G, int L, float eps, float *A, float *Bs,
                       float *mean, float *rstd, lionStream_t stream);
/* the same with the row sums taken on shifted values and carried in double (|mean| >> std rows keep their variance):
 * what lion_amd/train_ops.py uses.  The shift is the fp32 mean of the row's first min(L, 256) elements, so that no
 * single element -- an outlier in front -- decides it. */
int lion_row_stats64(const float *x, int rows, int L, double *stats, lionStream_t stream);
int lion_gn_train_fold64(const double *stats, const float *gw, const float *gb, const float *fac, int fac_stride,
                         const float *bias, int bias_stride, int B, int C, int G, int L, float eps, float *A,
                         float *Bs, float *mean, float *rstd, lionStream_t stream);
int lion_gn_train_bwd_fold(const float *S, const float *mean, const float *rstd, const float *gw, const float *gb,
                           const float *fac, int fac_stride, int B, int C, int G, int L, float *Q, float *R, float *dfac,
                           float *dbias, int d_stride, float *pw, const float *A, const double *xstats, const float *gate,
                           const float *qse, float *Aout, lionStream_t stream);
/* pw f32[B,C,3]: the per-sample terms of {d GroupNorm weight, d GroupNorm bias, sum over the row of dx}.  The third needs A (of the
 * forward fold) and xstats = the forward's lion_row_stats64 result (column 0 = row sums of x); both NULL: it is written as 0.
 * Summed over the batch it is the BIAS GRADIENT of the convolution that produced x (sum_l dx = A S1 + L Q + R sum_l x): Conv3d layers
 * in front of an AdaGN take it from here instead of a pass over dx (lion_amd/conv_ops.py).
 * gate / qse f32[B,C] (both or neither; with them A and Aout are required): an SE3d gate sits directly behind this AdaGN and the two
 * run as one op (lion_gn_se_gate_fwd / _bwd below) -- the upstream gradient was du = g gy + qse, S holds ITS row sums, and the apply
 * pass gets Aout = A g and Q = A qse + Q_gn: dx = Aout gy + Q + R x.
 * lion_gn_train_param_grads: dgw / dgb / dxs (or NULL) f32[C] = pw summed over the batch (ascending b). */
int lion_gn_train_param_grads(const float *pw, int B, int C, float *dgw, float *dgb, float *dxs, lionStream_t stream);
/* TRAINING, SE3d gate (reference models/pvcnn2_ada.py:27-41: x * sigmoid(W2 relu(W1 mean_voxels(x))), both Linear layers bias-free):
 * the [B, C] algebra between the row-sum pass (lion_row_stats) and the scaling pass (lion_affine_act with A = g, Bs = zero).
 * fwd: stats f32[B*C,2] (column 0 = row sums over the L voxels), w1 f32[Cr,C], w2 f32[C,Cr] -> mean f32[B,C], h f32[B,Cr] (after the
 * ReLU), g f32[B,C] (after the sigmoid), zero f32[B,C] (zeros).  bwd: S f32[B*C,2] (column 1 = sum_voxels gy*x, from
 * lion_affine_act_bwd_stats) -> dpre2 f32[B,C], dpre1 f32[B,Cr] (scratch outputs), Q f32[B,C] (per-voxel gradient through the mean,
 * for lion_affine_act_bwd_apply), dw1 f32[Cr,C], dw2 f32[C,Cr] (summed over the batch in ascending order).  C <= 1024, Cr <= 128. */
int lion_se_gate_fwd(const float *stats, const float *w1, const float *w2, int B, int C, int Cr, int L, float *mean, float *h,
                     float *g, float *zero, lionStream_t stream);
int lion_se_gate_bwd(const float *S, const float *g, const float *h, const float *mean, const float *w1, const float *w2, int B,
                     int C, int Cr, int L, float *dpre2, float *dpre1, float *Q, float *dw1, float *dw2, lionStream_t stream);
/* The tail of every PVConv's voxel branch is Conv3d -> AdaGN -> SE3d with NO activation between the last two (reference
 * pvcnn2_ada.py:211-226): both are affine per (sample, channel), so they run as ONE op -- u = A x + Bs is never written.
 * fwd: xstats f64[B*C,2] (lion_row_stats64 of x), A / Bs (lion_gn_train_fold64) -> mean f32[B,C] (channel means of u), h, g, and
 * A2 = g A, B2 = g Bs for one lion_affine_act pass (act 0) over x.  bwd: S f32[B*C,2] = {sum gy, sum gy x} (one
 * lion_affine_act_bwd_stats pass, act 0) -> Qse f32[B,C], Sp f32[B*C,2] (the row sums of du = g gy + Qse that
 * lion_gn_train_bwd_fold takes, with gate = g, qse = Qse), dpre2 / dpre1 (scratch), dw1, dw2; then one lion_affine_act_bwd_apply
 * pass with (Aout, Q, R).  3 passes over the grid forward and 5 backward instead of 6 and 10. */
/* ... and with the devoxelisation behind them (AdaGN -> SE3d -> trilinear_devoxelize, pvcnn2_ada.py:211-233: all linear): the gated
 * grid is never written either.  Forward: devoxelise x itself, apply (A2, B2) to the [B,C,N] result.  Backward, from the gradient g
 * f32[B,C,N] of that result: lion_rows_dot2 -> S f32[B*C,2] = {sum_p g ws, sum_p g v} (ws f32[B,N] = each point's 8 corner weights
 * summed, v = the devoxelised x saved by the forward) = the row sums {sum gy, sum gy x} of the scatter without a pass over the grid;
 * lion_gn_se_gate_bwd + lion_gn_train_bwd_fold as above; lion_trilinear_devoxelize_backward_affine writes
 * dx = A' scatter(g) + Q + R x in one pass (slab = Q + R x, corner contributions added in LDS; x 16-byte aligned, r3 * 4 <= 128 KiB,
 * r3 % 8 == 0).  Dense passes over the grid per PVConv tail: 1 forward (the row sums) and 2 backward -- were 6 + 10 as separate ops. */
int lion_rows_dot2(const float *g, const float *v, const float *ws, int B, int C, int N, float *S, lionStream_t stream);
int lion_trilinear_devoxelize_backward_affine(const float *gy, const int32_t *inds, const float *wgts, const float *x,
                                              const float *Ap, const float *Q, const float *R, int B, int C, int N, int r3,
                                              float *dx, lionStream_t stream);
int lion_gn_se_gate_fwd(const double *xstats, const float *A, const float *Bs, const float *w1, const float *w2, int B, int C, int Cr,
                        int L, float *mean, float *h, float *g, float *A2, float *B2, lionStream_t stream);
int lion_gn_se_gate_bwd(const float *S, const double *xstats, const float *A, const float *Bs, const float *g, const float *h,
                        const float *mean, const float *w1, const float *w2, int B, int C, int Cr, int L, float *Sp, float *dpre2,
                        float *dpre1, float *Qse, float *dw1, float *dw2, lionStream_t stream);
int lion_affine_act(const float *x, const float *A, const float *Bs, int rows, int L, int act, float *y,
                    lionStream_t stream);
int lion_affine_act_bwd_stats(const float *x, const float *gy, const float *A, const float *Bs, int rows, int L, int act,
                              float *S, lionStream_t stream);
int lion_affine_act_bwd_apply(const float *x, const float *gy, const float *A, const float *Bs, const float *Q,
                              const float *R, int rows, int L, int act, float *dx, lionStream_t stream);
/* TRAINING, round 6: the same three passes with nn.Dropout behind the activation (PVConv's voxel branch: Conv3d -> AdaGN -> Swish ->
 * Dropout, reference pvcnn2_ada.py:211-222; pvcnn2.py:170-186): y = act(A x + Bs) * m / keep, m ~ Bernoulli(keep) per element.
 * Element e is kept when word (e & 3) of Philox4x32-10(counter = {e >> 2, 'DROP', 0}, key = *seed) < keep * 2^32; seed: a 64-bit
 * word in DEVICE memory (drawn per call by the framework's generator, so that a replayed hipGraph draws a fresh mask); the two
 * backward passes regenerate the mask from the same seed (gy is masked and scaled on the fly) -- no mask tensor exists.
 * keep in (0, 1]. */
int lion_affine_act_dropout(const float *x, const float *A, const float *Bs, int rows, int L, int act, const uint64_t *seed,
                            float keep, float *y, lionStream_t stream);
int lion_affine_act_dropout_bwd_stats(const float *x, const float *gy, const float *A, const float *Bs, int rows, int L, int act,
                                      const uint64_t *seed, float keep, float *S, lionStream_t stream);
int lion_affine_act_dropout_bwd_apply(const float *x, const float *gy, const float *A, const float *Bs, const float *Q,
                                      const float *R, int rows, int L, int act, const uint64_t *seed, float keep, float *dx,
                                      lionStream_t stream);
/* Round 6 -- the same op with the set-abstraction pooling behind it (pvcnn2_ada.py:375-377): y f32[rows, M] = max over the U
 * neighbours of act(A x + Bs), x f32[rows, M, U] (U in {8, 16, 32, 64}).  The activated tensor is never written and its gradient
 * never materialised: backward = lion_affine_act_max_bwd_stats (S = {sum da, sum da x}, da = gy act'(.) at each group's FIRST
 * arg-max, 0 elsewhere) -> lion_gn_train_bwd_fold -> lion_affine_act_max_bwd_apply (dx = [arg-max] A da + Q + R x). */
int lion_affine_act_max(const float *x, const float *A, const float *Bs, int rows, int M, int U, int act, float *y,
                        lionStream_t stream);
int lion_affine_act_max_bwd_stats(const float *x, const float *gy, const float *A, const float *Bs, int rows, int M, int U,
                                  int act, float *S, lionStream_t stream);
int lion_affine_act_max_bwd_apply(const float *x, const float *gy, const float *A, const float *Bs, const float *Q,
                                  const float *R, int rows, int M, int U, int act, float *dx, lionStream_t stream);

/* ---- optimizer update (training): torch.optim.Adam with L2 weight decay (reference utils/utils.py:115-121; optimizer.step() of
 * trainers/hvae_trainer.py:150-154, train_2prior.py:405-410) over EVERY parameter tensor in one launch (csrc/optim.hip).
 * table u64[T,lion_adam_row()]: device addresses {param, grad, exp_avg, exp_avg_sq, step, ema} of T float32 tensors (step: that
 * parameter's f32 step count, incremented by the call, then used for the bias corrections; ema: 0, or the moving average of the
 * weights the reference's EMA wrapper keeps (utils/ema.py:60-75: ema = ema * ema_decay + (1 - ema_decay) * param after the update,
 * started from the updated parameter at the parameter's first step)); numel i32[T]; blockmap i32[blocks,2]: {tensor, chunk} per
 * workgroup, chunks of lion_adam_chunk() elements (all three in DEVICE memory, written by the caller once per gradient layout);
 * lr f32[1] (device).
 * Same arithmetic as torch.optim.Adam's single-tensor path (fp32 op for op, bias corrections in double). */
int lion_adam_chunk(void);
int lion_adam_row(void);
int lion_adam_step(const uint64_t *table, const int32_t *numel, const int32_t *blockmap, int blocks, int tensors, const float *lr,
                   float beta1, float beta2, float eps, float weight_decay, float ema_decay, lionStream_t stream);

/* ---- global gradient-norm clipping in front of the update (reference trainers/hvae_trainer.py:124-126, train_2prior.py:336-339:
 * torch.nn.utils.clip_grad_norm_(params, max_norm), error_if_nonfinite=False) over the SAME table / numel / blockmap, without
 * float atomics: the same gradients give the same bits on every rank.
 * lion_grad_sqnorm_partials: partials f32[blocks], one per blockmap row = the fp32 sum of squares of that chunk of the gradient
 *   (column 1 of the table row; nothing else is read, nothing else written).  Several tables (parameter groups) write into slices
 *   of one partials buffer.
 * lion_grad_clip_coef: ONE norm over partials[0..n), added in double in a fixed order; out2 f32[2] (device) = {norm, coef},
 *   norm = (float)sqrt(sum), coef = min(1, max_norm / (norm + 1e-6f)) in fp32 with a correctly rounded division (torch's
 *   `max_norm / (total_norm + 1e-6)` is reciprocal * max_norm: up to 1 ulp apart).  A NaN norm gives a NaN coefficient, an infinite
 *   norm 0, as torch's clamp(max=1.0) does.  max_norm > 0.
 * lion_adam_step_scaled: lion_adam_step with the gradient multiplied by grad_scale[0] (device; out2 + 1 above) in registers, one
 *   fp32 rounding, before the weight-decay term -- the gradient in memory is NOT rewritten, unlike clip_grad_norm_'s in-place
 *   multiply.  grad_scale NULL: lion_adam_step, bit for bit. */
int lion_grad_sqnorm_partials(const uint64_t *table, const int32_t *numel, const int32_t *blockmap, int blocks, float *partials,
                              lionStream_t stream);
int lion_grad_clip_coef(const float *partials, int n, float max_norm, float *out2, lionStream_t stream);
int lion_adam_step_scaled(const uint64_t *table, const int32_t *numel, const int32_t *blockmap, int blocks, int tensors,
                          const float *lr, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                          const float *grad_scale, lionStream_t stream);

/* ---- probability-flow ODE of the VPSDE: scipy's RK45 on the device (csrc/ode.hip) --------------------------------------
 * utils/diffusion_continuous.py:90-255 (compute_ode_nll / sample_model_ode) hand the PF-ODE of the whole batch -- ONE system
 * of n = B*D unknowns -- to scipy.integrate.solve_ivp(method='RK45') (rk.py RK45._step_impl, common.py select_initial_step)
 * through torchdiffeq's scipy wrapper.  Here its state stays on the device:
 *   Y f64[2][n]  (y and y_new; row ctrl->yslot is y), K f64[7][n] (stage derivatives; rows 0 / 6 swap roles via ctrl->fslot),
 *   x32 f32[n] (the model's input: fp32 of the stage state), t_model f32[B] (the model's time, sign-applied),
 *   partials f64[lion_ode_partials_bytes(n) / 8], ctrl (below; device memory, written by the host once per solve).
 * One evaluation: lion_ode_stage (stage ctrl->stage: 1..6 a step's stages, 7 = f0 at t0, 8 = the initial-step probe)
 *   -> the denoiser reads x32 / t_model -> lion_ode_drift writes row `stage` of K:
 *   dx/dt = f(t) x + 0.5 g2(t) params / sqrt(var(t)) in fp32 (diffusion_continuous.py:205-226, :599-622), negated when
 *   ctrl->sign < 0 (torchdiffeq misc.py:152-159, _ReverseFunc), widened to f64.  eps is the model output, [n] or, with
 *   cm_points = N != 0, the local prior's channel-major [B][4][N] for a point-major [B][N][4] latent.  mix_a / mix_b
 *   (f32[mix_len], n % mix_len == 0, both NULL without mixing): 1 - sigmoid(mixing_logit), sigmoid(mixing_logit).
 *   The schedule scalars are the fp32 roundings of beta_start, beta_end - beta_start, -beta_start,
 *   0.5 * (beta_end - beta_start) and 1 - sigma2_0, as torch applies them to a float32 t.
 * One attempted step ends with lion_ode_error_partials -> lion_ode_control: the RMS norm of the error estimate (or of the
 *   initial-step quantities d0, d1 / d2), reduced in a fixed order (no float atomics), and scipy's controller: accept /
 *   reject, SAFETY 0.9, factor in [0.2, 10], exponent -1/5, factor <= 1 after a rejection, the last step clipped to t_bound,
 *   TOO_SMALL_STEP below 10 x the spacing of doubles at t; the next attempt's h and t_new are prepared and stage = 1.
 *   The host reads ctrl once per attempted step. */
#define LION_ODE_RUNNING 0
#define LION_ODE_FINISHED 1
#define LION_ODE_TOO_SMALL_STEP (-1)
typedef struct lion_ode_ctrl {
  double t, h_abs, t_bound, direction, rtol, atol;
  double h, t_new, err_norm, h0, d1, sign;  /* attempt's step and end time; last norm; initial-step h0, d1; time sign */
  int32_t stage, cur, status, step_rejected; /* next stage; stage of the running evaluation; LION_ODE_*; this step */
  int32_t yslot, fslot, nfe, n_accepted;
  int32_t n_rejected, accepted, pad0, pad1;  /* accepted: the last attempt was */
} lion_ode_ctrl;
size_t lion_ode_partials_bytes(size_t n);
int lion_ode_stage(double *Y, const double *K, size_t n, lion_ode_ctrl *ctrl, float *x32, float *t_model, int B,
                   lionStream_t stream);
int lion_ode_drift(const float *eps, int cm_points, const float *x32, size_t n, const float *t_model, float beta_start,
                   float beta_delta, float neg_beta_start, float half_beta_delta, float one_minus_sigma2_0,
                   const float *mix_a, const float *mix_b, int mix_len, double *K, lion_ode_ctrl *ctrl,
                   lionStream_t stream);
int lion_ode_error_partials(const double *Y, const double *K, size_t n, const lion_ode_ctrl *ctrl, double *partials,
                            lionStream_t stream);
int lion_ode_control(const double *partials, size_t n, lion_ode_ctrl *ctrl, lionStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LION_HIP_H_ */
