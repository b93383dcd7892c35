// path_internal.h -- TopologyPRM's polyline helpers and the field's decision cut, shared by the kernels of guided
// replanning (topo_path.hip, collide_range.hip).  Included behind fuelmi_internal.h.  Host and device: the host builds of
// kernel text under tests/golden compile this text too.  f64, the reference's operations in the reference's order.
#ifndef FUELMI_PATH_INTERNAL_H_
#define FUELMI_PATH_INTERNAL_H_

#include <cmath>

__host__ __device__ __forceinline__ double path_norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// discretizePath's len_list (path_searching/src/topo_prm.cpp:428-434) of path [n][3], n >= 1: len[0 .. n - 1].
// len[n - 1] is pathLength(path) (:417-425) bit for bit: both add the same norms from the left, and a + b is b + a.
__host__ __device__ inline void path_prefix_lengths(const double* p, int n, double* len) {
  len[0] = 0.0;
  for (int i = 0; i < n - 1; ++i)
    len[i + 1] = path_norm3(p[3 * i + 3] - p[3 * i], p[3 * i + 4] - p[3 * i + 1], p[3 * i + 5] - p[3 * i + 2]) + len[i];
}

// point i of discretizePath(path, pt_num) (:436-458) over len = path_prefix_lengths: the FIRST segment whose +-1e-4 range
// holds cur_l, lambda as it comes (it may leave [0, 1]; a chosen segment of length zero divides by zero and the point is
// what IEEE gives).  false: no segment holds cur_l -- the reference indexes with -1 there; o is not written.
__host__ __device__ inline bool path_disc_point(const double* path, int n, const double* len, int pt_num, int i,
                                                double o[3]) {
  const double dl = len[n - 1] / double(pt_num - 1);
  const double cur_l = double(i) * dl;
  int idx = -1;
  for (int j = 0; j < n - 1; ++j)
    if (cur_l >= len[j] - 1e-4 && cur_l <= len[j + 1] + 1e-4) {
      idx = j;
      break;
    }
  if (idx < 0) return false;
  const double lambda = (cur_l - len[idx]) / (len[idx + 1] - len[idx]);
  for (int k = 0; k < 3; ++k) o[k] = (1 - lambda) * path[3 * idx + k] + lambda * path[3 * idx + 3 + k];
  return true;
}

// A decision on the distance field, taken on the device's f32 values.  The positive part of the reference's field is
// res * sqrt(k) for an integer k >= 0; the device holds the f32 product through an approximate square root, a few ulp
// from it (esdf.hip).  The host finds the largest k for which the reference's f64 comparison `res * sqrt(k) <= thresh`
// (strict: `< thresh`) holds and returns an f32 cut between the device's values for k and k + 1: on the device
// `dist <= cut` is the reference's comparison for both forms.  No k passes (strict with thresh = 0): -1, below every value.
inline float field_cut(double res, double thresh, bool strict) {
  auto pass = [&](long k) {
    const double d = res * std::sqrt((double)k);
    return strict ? d < thresh : d <= thresh;
  };
  long k = (long)std::floor((thresh / res) * (thresh / res));
  if (k < 0) k = 0;
  while (pass(k + 1)) ++k;
  while (k > 0 && !pass(k)) --k;
  if (!pass(k)) return -1.0f;
  return (float)((double)(float)res * std::sqrt((double)k + 0.5));
}

#endif
