// conv3d_tiles.h -- what the voxel Conv3d files share on the host (conv3d.hip, conv3d_split_kernel.h, conv3d_wgrad.hip, and
// voxelize.hip for its reader map): the spatial tile of a resolution, a forward entry's argument checks, the grid rule.
#pragma once
#include "common.h"

// The spatial tile at resolution r with vb 32-voxel column blocks per wave: 4 waves x vb x 32 voxels, the whole w axis
// (a wave's accumulator columns are runs of one row), 4 rows of it (8 at r = 8) and the depth that remains.
struct ConvTileDims { int td, th, tw; };
constexpr ConvTileDims conv_tile_dims(int r, int vb) { return {128 * vb / ((r == 8 ? 8 : 4) * r), r == 8 ? 8 : 4, r}; }
constexpr int conv_tile_count(int r, int vb) { return r * r * r / (128 * vb); }
// The 256-voxel tile (vb = 2): that of every sparse (work-queue) plan -- so the geometry of the occupancy flags and of
// lion_voxel_scatter_read's reader map --, of the split and half kernels and of both weight-gradient kernels and their skip map.
constexpr int CONV_TILE256_VB = 2;
constexpr ConvTileDims conv_tile256(int r) { return conv_tile_dims(r, CONV_TILE256_VB); }
constexpr int conv_tile256_count(int r) { return conv_tile_count(r, CONV_TILE256_VB); }
// Run-time (r, vb) -> f(IntC<TD>{}, IntC<TH>{}, IntC<TW>{}), as lion_with_flags does for booleans.  f is instantiated for all
// six tiles (three in the 256-voxel form): a caller whose kernel does not exist for one answers that with `if constexpr`.
template <int R, int VB, typename F> static inline int conv_tile_call(F &f) {
  constexpr ConvTileDims t = conv_tile_dims(R, VB);
  static_assert(t.td * t.th * t.tw == 128 * VB && t.tw == R && R % t.td == 0 && R % t.th == 0, "not an exact tile");
  return f(IntC<t.td>{}, IntC<t.th>{}, IntC<t.tw>{});
}
template <typename F> static inline int conv_tile256_dispatch(int r, F f) {
  if (r == 32) return conv_tile_call<32, CONV_TILE256_VB>(f);
  if (r == 16) return conv_tile_call<16, CONV_TILE256_VB>(f);
  if (r == 8) return conv_tile_call<8, CONV_TILE256_VB>(f);
  return LION_EUNSUPPORTED;
}
template <typename F> static inline int conv_tile_dispatch(int r, int vb, F f) {
  if (vb == CONV_TILE256_VB) return conv_tile256_dispatch(r, f);
  if (r == 32 && vb == 4) return conv_tile_call<32, 4>(f);
  if (r == 16 && vb == 4) return conv_tile_call<16, 4>(f);
  if (r == 8 && vb == 1) return conv_tile_call<8, 1>(f);
  return LION_EUNSUPPORTED;
}
// What every forward entry (fp32, split, half) refuses before it looks for a plan; wp: that entry's packed weights.
static inline int conv_forward_args(const float *x, const void *wp, const float *y, int B, int Cin, int Cout,
                                    const float *pro_a, const float *pro_b, const float *tconst, const int32_t *occ) {
  if (!x || !wp || !y || B <= 0 || Cin <= 0 || Cout <= 0) return LION_EINVAL;
  if ((pro_a == nullptr) != (pro_b == nullptr)) return LION_EINVAL;
  if (tconst && !pro_a) return LION_EINVAL;
  if (occ && pro_a && !tconst) return LION_EINVAL; // an activated input is sparse only as constant + delta
  return 0;
}
// Grid of a forward launch: (sample, tile, channel tile), or with a work queue min(items, `resident` per CU) persistent ones.
static inline int conv_grid(bool queued, int B, int tiles, int channel_tiles, int resident, dim3 *grid) {
  int n_cu = 0;
  if (int e = lion_cu_count(&n_cu)) return e;
  const long items = (long)B * tiles * channel_tiles, most = (long)resident * n_cu;
  *grid = queued ? dim3((unsigned)(items < most ? items : most)) : dim3(B, tiles, channel_tiles);
  return 0;
}
