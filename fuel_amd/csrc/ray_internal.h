// ray_internal.h -- RayCaster::setInput / step (plan_env/src/raycast.cpp:228-321) as a voxel walk in registers, shared by
// the kernels that walk a voxel ray against the map (topo_path.hip lineVisib, info_gain.hip calcInformationGain).
// Included behind fuelmi_internal.h.  Host and device: the host builds of kernel text under tests/golden compile this
// text too.  f64, the reference's operations in the reference's order.
#ifndef FUELMI_RAY_INTERNAL_H_
#define FUELMI_RAY_INTERNAL_H_

#include <cmath>

// raycast.cpp:10-23: mod(value, 1) is fmod(fmod(value, 1) + 1, 1); fmod(v, 1) of a finite v is v - trunc(v), exactly
__host__ __device__ __forceinline__ double ray_intbound(double s, double ds) {
  if (ds < 0) s = -s, ds = -ds;
  const double a = s - trunc(s);
  const double t = a + 1.0;
  s = t - trunc(t);
  return (1 - s) / ds;
}

// The state of one walk.  setInput's return value is ignored by every caller we restate; an axis without a step has
// tMax = +inf and tDelta = NaN and is never chosen while another axis still steps.
struct RayWalk {
  int x, y, z, endx, endy, endz;
  int stx, sty, stz;
  double tmx, tmy, tmz, tdx, tdy, tdz;
};

// setInput(start, end), both in voxel units (:228-275)
__host__ __device__ __forceinline__ void ray_set_input(RayWalk& r, double sx, double sy, double sz, double ex, double ey,
                                                       double ez) {
  r.x = (int)floor(sx), r.y = (int)floor(sy), r.z = (int)floor(sz);
  r.endx = (int)floor(ex), r.endy = (int)floor(ey), r.endz = (int)floor(ez);
  const double dx = r.endx - r.x, dy = r.endy - r.y, dz = r.endz - r.z;
  r.stx = dx == 0 ? 0 : (dx < 0 ? -1 : 1), r.sty = dy == 0 ? 0 : (dy < 0 ? -1 : 1), r.stz = dz == 0 ? 0 : (dz < 0 ? -1 : 1);
  r.tmx = ray_intbound(sx, dx), r.tmy = ray_intbound(sy, dy), r.tmz = ray_intbound(sz, dz);
  r.tdx = (double)r.stx / dx, r.tdy = (double)r.sty / dy, r.tdz = (double)r.stz / dz;
}

__host__ __device__ __forceinline__ bool ray_at_end(const RayWalk& r) {
  return r.x == r.endx && r.y == r.endy && r.z == r.endz;
}

// the step of step() (:300-318)
__host__ __device__ __forceinline__ void ray_advance(RayWalk& r) {
  if (r.tmx < r.tmy) {
    if (r.tmx < r.tmz)
      r.x += r.stx, r.tmx += r.tdx;
    else
      r.z += r.stz, r.tmz += r.tdz;
  } else {
    if (r.tmy < r.tmz)
      r.y += r.sty, r.tmy += r.tdy;
    else
      r.z += r.stz, r.tmz += r.tdz;
  }
}

#endif
