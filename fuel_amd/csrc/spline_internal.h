// spline_internal.h -- NonUniformBspline's evaluation on the device, shared by the kernels that read a batch of
// position splines (yaw_plan.hip, traj_check.hip, traj_sample.hip, traj_adjust.hip, collide_range.hip) or one spline a
// state (local_segment.hip): where a problem's spline lies, its knots, its evaluation, its derivative splines.  f64, the
// reference's operations in the reference's order.
#ifndef FUELMI_SPLINE_INTERNAL_H_
#define FUELMI_SPLINE_INTERNAL_H_

#include <cstddef>

// the position splines of a batch of problems, as the four kernels read them
struct SplineSrc {
  const int* n_ctrl;        // [n], or null: every problem has n_ctrl_all control points
  int n_ctrl_all;
  const double* pos;        // problem b: [n_ctrl][3] at pos + b * pos_stride
  size_t pos_stride;
  const double* knot;       // problem b: knot[b * knot_stride]
  size_t knot_stride;
  const double* knots;      // null: uniform knots of the span above.  Else problem b's whole knot vector u[0 .. n + p] at
  size_t knots_stride;      // knots + b * knots_stride, and the span is not read (k_traj_check, k_traj_sample, k_yaw_plan)
};

// problem b of a batch: its number of control points, its knot span, its control points [n][3].  Three reads, so that a
// kernel makes each where it needs it (the first two load, and only for a b below n_prob).
__device__ __forceinline__ int spline_n(const SplineSrc& s, int b) { return s.n_ctrl ? s.n_ctrl[b] : s.n_ctrl_all; }
__device__ __forceinline__ double spline_dt(const SplineSrc& s, int b) { return s.knot[(size_t)b * s.knot_stride]; }
__device__ __forceinline__ const double* spline_ctrl(const SplineSrc& s, int b) { return s.pos + (size_t)b * s.pos_stride; }

// what a kernel asks of a problem before it indexes anything by it.  (The host refuses the others before any launch
// wherever it sees them; the variables of a device batch it does not see.)
__device__ __forceinline__ bool spline_sane(double dt, int n, int p, int max_ctrl) {
  return dt > 0.0 && isfinite(dt) && n >= p + 1 && n <= max_ctrl;
}

// the span a kernel tests where whole knot vectors are given and none is read
__device__ __forceinline__ double spline_dt_or_one(const SplineSrc& s, int b) { return s.knots ? 1.0 : spline_dt(s, b); }

// doubles of one wave's knot block in LDS: n + p + 1 <= max_ctrl + 6 knots, kept a multiple of 16 bytes
__host__ __device__ inline int spline_knot_stride(int max_ctrl) { return (max_ctrl + 6 + 1) & ~1; }

// setUniformBspline's knots (non_uniform_bspline.cpp:25-31): u[0 .. n + p] of a spline of degree p with n control
// points and the span dt.  The knots behind u[p] are a running sum, not i * dt: every result is bit-equal to the
// reference's only in this order.
__device__ __forceinline__ void spline_uniform_knots(double* u, int p, int n, double dt) {
  for (int i = 0; i <= p; ++i) u[i] = (double)(i - p) * dt;
  double acc = u[p];
  for (int i = p + 1; i <= n + p; ++i) {
    acc = acc + dt;
    u[i] = acc;
  }
}

// problem b's knots into its wave's block u[0 .. n + p], by the 64 lanes of that wave; sane: spline_sane of the problem
// (false for a wave without one; the same in every lane).  Returns whether the wave may evaluate on u, the same answer in
// every lane.  No whole knot vectors: lane 0 accumulates the uniform ones, as above.  Else every lane copies its share
// and tests it -- finite, and above the knot in front of it (what the host asks of given knots wherever it sees them; a
// device batch's it does not see) -- and a ballot joins the lanes: one bad knot and the problem is a bad spline.  The
// caller's barrier stands between these writes and the first read.
__device__ __forceinline__ bool spline_stage_knots(const SplineSrc& s, int b, double* u, int p, int n, double dt, int lane,
                                                   bool sane) {
  if (!s.knots) {
    if (sane && lane == 0) spline_uniform_knots(u, p, n, dt);
    return sane;
  }
  if (!sane) return false;
  const double* kin = s.knots + (size_t)b * s.knots_stride;
  bool bad = false;
  for (int j = lane; j <= n + p; j += 64) {
    const double v = kin[j];
    u[j] = v;
    if (!isfinite(v) || (j > 0 && !(kin[j - 1] < v))) bad = true;
  }
  return __ballot(bad) == 0;
}

// the clamp and the knot search of evaluateDeBoor (non_uniform_bspline.cpp:52-57) for evaluateDeBoorT(t) of a spline of
// degree p with n control points and the knots u[0 .. n + p]: returns the span k, ub = the clamped parameter.  Every
// derivative spline of getDerivative (:97-106) finds the same ub and, counted in these knots, the same k: its knots are
// u without the first and the last, its degree and its number of points are one less, so its u_(p_) is u[p], its
// u_(m_ - p_) is u[n] and its search starts on u[p + 1].
__device__ __forceinline__ int spline_span(const double* u, int p, int n, double t, double& ub) {
  const double lo = u[p], v = t + u[p], hi = u[n];
  ub = lo < v ? v : lo;  // min(max(u_(p_), u), u_(m_ - p_))
  ub = hi < ub ? hi : ub;
  int k = p;
  while (k < n - 1 && u[k + 1] < ub) ++k;  // (k < n - 1 holds by the clamp; it keeps a bad spline inside its arrays)
  return k;
}

// the alpha recursion of evaluateDeBoor (:65-69) on the PD + 1 points d of span k, for a spline of degree PD or, k still
// counted in the parent's knots u, a derivative spline of degree PD: the shift of its knots and the shift of its k cancel
// in both indices.  The result is d[PD].
template <int PD, int DIM>
__device__ __forceinline__ void spline_alpha(const double* u, int k, double ub, double (*d)[DIM]) {
#pragma unroll
  for (int r = 1; r <= PD; ++r)
#pragma unroll
    for (int i = PD; i >= r; --i) {
      const double alpha = (ub - u[i + k - PD]) / (u[i + 1 + k - r] - u[i + k - PD]);
#pragma unroll
      for (int c = 0; c < DIM; ++c) d[i][c] = (1 - alpha) * d[i - 1][c] + alpha * d[i][c];
    }
}

// getDerivativeControlPoints (:77-86) on the points of span k, in place: q holds the PD + 1 points of a spline (or
// derivative spline) of degree PD that span k reads and receives the PD points its derivative reads there,
// Q[i] = double(PD) * (P[i+1] - P[i]) / (u_(i + PD + 1) - u_(i + 1)) in that spline's own knots -- in the parent's u
// the two are u[k + i + 1] and u[k - PD + i + 1] at every level
template <int PD, int DIM>
__device__ __forceinline__ void spline_derive(const double* u, int k, double (*q)[DIM]) {
#pragma unroll
  for (int i = 0; i < PD; ++i) {
    const double den = u[k + i + 1] - u[k - PD + i + 1];
#pragma unroll
    for (int c = 0; c < DIM; ++c) q[i][c] = (double)PD * (q[i + 1][c] - q[i][c]) / den;
  }
}

// NonUniformBspline::evaluateDeBoorT (non_uniform_bspline.cpp:51-75) of a spline of degree P with n control points and
// the knots u[0 .. n + P]; ctrl(i, d) fetches control point i
template <int P, class F>
__device__ __forceinline__ void spline_deboor(const double* u, int n, double t, F ctrl, double out[3]) {
  double ub;
  const int k = spline_span(u, P, n, t, ub);
  double d[P + 1][3];
#pragma unroll
  for (int i = 0; i <= P; ++i) ctrl(k - P + i, d[i]);
  spline_alpha<P, 3>(u, k, ub, d);
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

// the spline of degree PD on the points q of span k, then LEVELS derivatives of it: out[0 .. LEVELS].  A derivative of
// degree 0 is its one point: the knot search alone (evaluateDeBoor with p_ = 0).
template <int PD, int DIM, int LEVELS>
__device__ __forceinline__ void spline_levels(const double* u, int k, double ub, double (*q)[DIM], double (*out)[DIM]) {
  double w[PD + 1][DIM];
#pragma unroll
  for (int i = 0; i <= PD; ++i)
#pragma unroll
    for (int c = 0; c < DIM; ++c) w[i][c] = q[i][c];
  spline_alpha<PD, DIM>(u, k, ub, w);
#pragma unroll
  for (int c = 0; c < DIM; ++c) out[0][c] = w[PD][c];
  if constexpr (LEVELS > 0) {
    spline_derive<PD, DIM>(u, k, q);
    spline_levels<PD - 1, DIM, LEVELS - 1>(u, k, ub, q, out + 1);
  }
}

// evaluateDeBoorT(t) of a spline (degree P, n points C [n][DIM], knots u) and of its first LEVELS derivatives
template <int P, int DIM, int LEVELS>
__device__ __forceinline__ void spline_eval_levels(const double* u, int n, const double* C, double t, double (*out)[DIM]) {
  double ub;
  const int k = spline_span(u, P, n, t, ub);
  double q[P + 1][DIM];
#pragma unroll
  for (int i = 0; i <= P; ++i)
#pragma unroll
    for (int c = 0; c < DIM; ++c) q[i][c] = C[(size_t)DIM * (k - P + i) + c];
  spline_levels<P, DIM, LEVELS>(u, k, ub, q, out);
}

#endif
