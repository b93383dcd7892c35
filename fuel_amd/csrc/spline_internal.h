// spline_internal.h -- NonUniformBspline's point evaluation on the device, shared by the kernels that evaluate a
// position spline (yaw_plan.hip, traj_check.hip).  f64, the reference's operations in the reference's order.
#ifndef FUELMI_SPLINE_INTERNAL_H_
#define FUELMI_SPLINE_INTERNAL_H_

// NonUniformBspline::evaluateDeBoorT (non_uniform_bspline.cpp:51-75) of a spline of degree P with n control points and
// the knots u[0 .. n + P]; ctrl(i, d) fetches control point i
template <int P, class F>
__device__ __forceinline__ void spline_deboor(const double* u, int n, double t, F ctrl, double out[3]) {
  const double lo = u[P], v = t + u[P], hi = u[n];
  double ub = lo < v ? v : lo;  // min(max(u_(p_), u), u_(m_ - p_))
  ub = hi < ub ? hi : ub;
  int k = P;
  while (k < n - 1 && u[k + 1] < ub) ++k;  // (k < n - 1 holds by the clamp; it keeps a bad spline inside its arrays)
  double d[P + 1][3];
#pragma unroll
  for (int i = 0; i <= P; ++i) ctrl(k - P + i, d[i]);
#pragma unroll
  for (int r = 1; r <= P; ++r)
#pragma unroll
    for (int i = P; i >= r; --i) {
      const double alpha = (ub - u[i + k - P]) / (u[i + 1 + k - r] - u[i + k - P]);
#pragma unroll
      for (int c = 0; c < 3; ++c) d[i][c] = (1 - alpha) * d[i - 1][c] + alpha * d[i][c];
    }
  out[0] = d[P][0], out[1] = d[P][1], out[2] = d[P][2];
}

// the position spline (degree p in 3..5, control points C [n][3]) at time t
__device__ __forceinline__ void spline_pos(const double* u, int p, int n, const double* C, double t, double out[3]) {
  auto ctrl = [C](int i, double d[3]) { d[0] = C[3 * i], d[1] = C[3 * i + 1], d[2] = C[3 * i + 2]; };
  if (p == 3)
    spline_deboor<3>(u, n, t, ctrl, out);
  else if (p == 4)
    spline_deboor<4>(u, n, t, ctrl, out);
  else
    spline_deboor<5>(u, n, t, ctrl, out);
}

#endif
