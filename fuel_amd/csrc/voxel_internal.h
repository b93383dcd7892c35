// voxel_internal.h -- look-ups in the map's bit planes by voxel index or position, shared by the kernels that walk voxels
// (frontier_view.hip, path_cost.hip, goal_path.hip, kino_path.hip, traj_check.hip, map_cloud.hip, ...).  Included by
// fuelmi_internal.h below Geo.  Host and device: the host builds of kernel text under tests/golden compile this text too.
#ifndef FUELMI_VOXEL_INTERNAL_H_
#define FUELMI_VOXEL_INTERNAL_H_

#include <cmath>

__host__ __device__ __forceinline__ bool idx_in_map(const Geo& g, const int id[3]) {
  return !(id[0] < 0 || id[1] < 0 || id[2] < 0 || id[0] > g.nx - 1 || id[1] > g.ny - 1 || id[2] > g.nz - 1);
}
__host__ __device__ __forceinline__ void pos_to_idx(const Geo& g, const double p[3], int id[3]) {
  for (int k = 0; k < 3; ++k) id[k] = (int)floor((p[k] - g.org[k]) * g.res_inv);
}
__host__ __device__ __forceinline__ bool bit_at(const u64* pl, long a) { return (pl[a >> 6] >> (a & 63)) & 1ull; }
// the plane's bit at a position: getInflateOccupancy(pos) == 1 on the inflated plane, getOccupancy(pos) == UNKNOWN on
// the unknown one; a position outside the map reads -1 in both and passes
__host__ __device__ __forceinline__ bool plane_at_pos(const Geo& g, const u64* pl, const double p[3]) {
  int id[3];
  pos_to_idx(g, p, id);
  if (!idx_in_map(g, id)) return false;
  return bit_at(pl, (long)id[0] * g.nyz + (long)id[1] * g.nz + id[2]);
}
// 64 bits of the plane starting at (signed) bit index `bit`
__host__ __device__ __forceinline__ u64 plane_window(const u64* __restrict__ p, long bit) {
  long wi = bit >> 6;
  int sh = (int)(bit & 63);
  u64 lo = p[wi];
  if (sh == 0) return lo;
  u64 hi = p[wi + 1];
  return (lo >> sh) | (hi << (64 - sh));
}

#endif
