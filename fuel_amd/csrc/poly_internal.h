// poly_internal.h -- PolynomialTraj's evaluation on the device (poly_traj/include/poly_traj/polynomial_traj.h:28-46,
// :82-90), shared by the kernels that read a piecewise quintic: waypoint_traj.hip, which builds one, and
// local_segment.hip, which reads it as the global trajectory.  f64, the reference's operations in the reference's order.
#ifndef FUELMI_POLY_INTERNAL_H_
#define FUELMI_POLY_INTERNAL_H_

// PolynomialTraj::evaluate(t, k) of S segments with the durations T [S] and the coefficients cf [S][3][6] (lowest power
// first): the lookup (idx clamped to the last segment, where the reference reads past its vector), then tv . c with
// tv[i] = i (i-1) .. (i-k+1) ts^(i-k), the powers as repeated products, summed from the lowest power
__device__ __forceinline__ void poly_eval(const double* cf, const double* T, int S, double t, int k, double out[3]) {
  int idx = 0;
  double ts = t;
  while (idx < S - 1 && T[idx] + 1e-4 < ts) {
    ts -= T[idx];
    ++idx;
  }
  const double* c = cf + 18 * idx;
  double o0 = 0.0, o1 = 0.0, o2 = 0.0, pw = 1.0;
  for (int i = k; i < 6; ++i) {
    int m = 1;
    for (int q = i; q > i - k; --q) m *= q;
    const double tv = (double)m * pw;
    pw = pw * ts;
    o0 += tv * c[i];
    o1 += tv * c[6 + i];
    o2 += tv * c[12 + i];
  }
  out[0] = o0, out[1] = o1, out[2] = o2;
}

#endif
