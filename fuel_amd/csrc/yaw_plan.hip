// yaw_plan.hip -- the yaw trajectory of a position spline: FastPlannerManager::planYawExplore
// (plan_manage/src/planner_manager.cpp:774-865) and ::planYaw (:695-772) for a batch of problems (position control
// points, knot span, start yaw state, end yaw): the knots as setUniformBspline accumulates them, the look-ahead
// way-points (two evaluateDeBoorT and one atan2 each), calcNextYaw's unwrap chain, the initial control points, pt_dist_
// and the minimiser of the optimiser's objective.
//
// With SMOOTHNESS | START | END | WAYPOINTS, dimension 1, no bounds and pt_dist_ fixed, that objective is a sum of
// squares of linear forms of at most four neighbouring control points:
//     ld_smooth (J . q[i..i+3] / pt_dist)^2,  J = (-1, 3, -3, 1)                       i = 0 .. N-4
//     10 ld_start (P . q[0..2] - s0)^2 + ld_start (V . q[0..2] - s1)^2 + ld_start (A . q[0..2] - s2)^2
//     ld_end ((P . q[N-3..] - e)^2 + (V . q[N-3..])^2 [+ (A . q[N-3..])^2 with three end entries])
//     ld_waypt (P . q[i..i+2] - w_i)^2                                                 way-point indices i
//     P = (1, 4, 1) / 6,  V = (-1, 0, 1) / (2 dt),  A = (1, -2, 1) / dt^2
// so the minimiser solves H q = g with H = sum c a a^T symmetric positive definite of half-bandwidth 3 (the jerk rows
// leave quadratics free, the three start rows pin them).  One lane per row gathers its four diagonals and its right-hand
// side, lane 0 factors by Cholesky and substitutes: the reference's NLopt run iterates towards this point.
//
// One wave of YP_NT lanes per problem, one lane per way-point (looped past YP_NT), all f64, -ffp-contract=off.  The
// position knots are staged in LDS by the accumulated additions or copied and checked as given, the yaw spline's always by
// the additions; the unwrap chain and the factorisation are serial in lane 0
// (N <= 259).  A result does not depend on the problem's place in the batch.
// Behind the kernel, the entries that share its checks, argument fill, result layout and copy-out: fuelmi_map_plan_yaws
// and fuelmi_map_plan_yaws_knots (through a query slot, the position spline uniform or on given knots) and
// fuelmi_bspline_dev_plan_yaws (the splines a device batch's last solve left, on the knots its adjustment left if the
// batch says so, bspline_batch.h).
#include <cmath>
#include <cstring>
#include <vector>

#include "bspline_batch.h"

namespace {

constexpr int YP_NT = 64;
constexpr double YP_PI = 3.14159265358979323846;  // M_PI

// k_yaw_plan: one problem per wave; every pointer addresses memory the device can reach
struct YawArgs {
  fuelmi_yaw_cfg cfg;
  double ld_smooth, ld_start, ld_end, ld_waypt;
  int n_prob;
  SplineSrc src;
  const double* start_yaw;  // [n][3]
  const double* end_yaw;    // [n] (EXPLORE)
  int* status;
  int* seg_num;
  int* n_waypt;
  double* duration;
  double* dt_yaw;
  double* end_yaw_out;
  double* cost;
  double* yaw_ctrl;         // [n][max_seg + 3]
  double* waypts;           // [n][max_seg]
  double* yawdot_ctrl;      // [n][max_seg + 2] or null
  double* yawddot_ctrl;     // [n][max_seg + 1] or null
};

__host__ __device__ inline int yp_knots(int max_ctrl, int max_seg) {  // position knots n + p + 1 <= max_ctrl + 6; yaw knots N + p + 1
  return max_ctrl + 6 > max_seg + 9 ? max_ctrl + 6 : max_seg + 9;
}

// FastPlannerManager::calcNextYaw (:867-885)
__device__ __forceinline__ double yp_next_yaw(double last_yaw, double yaw) {
  double round_last = last_yaw;
  while (round_last < -YP_PI) round_last += 2 * YP_PI;
  while (round_last > YP_PI) round_last -= 2 * YP_PI;
  const double diff = yaw - round_last;
  if (fabs(diff) <= YP_PI) return last_yaw + diff;
  if (diff > YP_PI) return last_yaw + diff - 2 * YP_PI;
  if (diff < -YP_PI) return last_yaw + diff + 2 * YP_PI;
  return yaw;  // diff is not a number: the reference leaves yaw as it is
}

// its derivative (getDerivative :77-106) at time t: control points p (P[i+1] - P[i]) / (u[i+p+1] - u[i+1]), the knots
// without the first and the last, degree p - 1
__device__ __forceinline__ void yp_vel(const double* u, int p, int n, const double* C, double t, double out[3]) {
  auto ctrl = [C, u, p](int i, double d[3]) {
    const double den = u[i + p + 1] - u[i + 1];
    for (int c = 0; c < 3; ++c) d[c] = (double)p * (C[3 * (i + 1) + c] - C[3 * i + c]) / den;
  };
  if (p == 3)
    spline_deboor<2>(u + 1, n - 1, t, ctrl, out);
  else if (p == 4)
    spline_deboor<3>(u + 1, n - 1, t, ctrl, out);
  else
    spline_deboor<4>(u + 1, n - 1, t, ctrl, out);
}

__device__ __forceinline__ double yp_J(int k) { return k == 0 ? -1.0 : k == 1 ? 3.0 : k == 2 ? -3.0 : 1.0; }
__device__ __forceinline__ double yp_P(int k) { return k == 1 ? 4.0 / 6.0 : 1.0 / 6.0; }
__device__ __forceinline__ double yp_V(int k, double dt) { return (k == 0 ? -1.0 : k == 1 ? 0.0 : 1.0) / (2 * dt); }
__device__ __forceinline__ double yp_A(int k, double dt) { return (k == 1 ? -2.0 : 1.0) / (dt * dt); }

// everything a problem reports.  N = 0: no yaw spline (every array of the problem is written as 0)
__device__ void yp_write(const YawArgs& Y, int b, int tid, int status, double duration, int seg, double dt_yaw, int N,
                         const double* q, int nw, const double* wp, double e, double cost, const double* uy, int py) {
  const int maxs = Y.cfg.max_seg;
  if (tid == 0) {
    Y.status[b] = status;
    Y.duration[b] = duration;
    Y.seg_num[b] = seg;
    Y.dt_yaw[b] = dt_yaw;
    Y.n_waypt[b] = nw;
    Y.end_yaw_out[b] = e;
    Y.cost[b] = cost;
  }
  double* oc = Y.yaw_ctrl + (size_t)b * (maxs + 3);
  double* ow = Y.waypts + (size_t)b * maxs;
  for (int i = tid; i < maxs + 3; i += YP_NT) oc[i] = i < N ? q[i] : 0.0;
  for (int i = tid; i < maxs; i += YP_NT) ow[i] = i < nw ? wp[i] : 0.0;
  // getDerivativeControlPoints (:77-86) once and twice, on the knots of setUniformBspline(yaw, py, dt_yaw)
  if (Y.yawdot_ctrl) {
    double* o = Y.yawdot_ctrl + (size_t)b * (maxs + 2);
    for (int i = tid; i < maxs + 2; i += YP_NT)
      o[i] = i < N - 1 ? (double)py * (q[i + 1] - q[i]) / (uy[i + py + 1] - uy[i + 1]) : 0.0;
  }
  if (Y.yawddot_ctrl) {
    double* o = Y.yawddot_ctrl + (size_t)b * (maxs + 1);
    for (int i = tid; i < maxs + 1; i += YP_NT) {
      double v = 0.0;
      if (i < N - 2) {
        const double d0 = (double)py * (q[i + 1] - q[i]) / (uy[i + py + 1] - uy[i + 1]);
        const double d1 = (double)py * (q[i + 2] - q[i + 1]) / (uy[i + py + 2] - uy[i + 2]);
        v = (double)(py - 1) * (d1 - d0) / (uy[i + py + 1] - uy[i + 2]);
      }
      o[i] = v;
    }
  }
}

__global__ void __launch_bounds__(YP_NT) k_yaw_plan(YawArgs Y) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int maxs = Y.cfg.max_seg, maxn = maxs + 3, nu = yp_knots(Y.cfg.max_ctrl, maxs);
  double* u = reinterpret_cast<double*>(smem_raw);  // [nu]       position knots, later the yaw spline's
  double* wp = u + nu;                              // [maxs]     atan2 per way-point, then the unwrapped way-points
  double* band = wp + maxs;                         // [maxn][4]  H(r, r - d) at [r][d], then its Cholesky factor
  double* g = band + 4 * maxn;                      // [maxn]     right-hand side, then the minimiser
  double* q0 = g + maxn;                            // [maxn]     initial control points
  double* sh = q0 + maxn;                           // [8]
  int* ok = reinterpret_cast<int*>(sh + 8);         // [maxs]     the way-point's |pd| > 1e-6

  const bool follow = Y.cfg.mode == FUELMI_YAW_FOLLOW;
  const int p = Y.cfg.pos_degree;
  const int n = spline_n(Y.src, b);
  const double dt = spline_dt_or_one(Y.src, b);
  const double* C = spline_ctrl(Y.src, b);

  // 1. knots, duration = getTimeSum
  if (!spline_stage_knots(Y.src, b, u, p, n, dt, tid, spline_sane(dt, n, p, Y.cfg.max_ctrl))) {
    yp_write(Y, b, tid, FUELMI_YAW_DEGENERATE, 0.0, 0, 0.0, 0, nullptr, 0, nullptr, 0.0, 0.0, nullptr, 3);
    return;
  }
  __syncthreads();
  const double duration = u[n] - u[p];

  // 2. seg_num, dt_yaw, the way-points' range
  int seg = Y.cfg.seg_num;
  if (follow) {
    const double qd = ceil(duration / Y.cfg.dt_target);
    if (!(qd >= 1.0)) {
      yp_write(Y, b, tid, FUELMI_YAW_DEGENERATE, duration, 0, 0.0, 0, nullptr, 0, nullptr, 0.0, 0.0, nullptr, 3);
      return;
    }
    if (!(qd <= (double)maxs)) {
      seg = qd < 1073741824.0 ? (int)qd : 1073741824;
      yp_write(Y, b, tid, -1, duration, seg, duration / (double)seg, 0, nullptr, 0, nullptr, 0.0, 0.0, nullptr, 3);
      return;
    }
    seg = (int)qd;
  }
  const double dt_yaw = duration / (double)seg;
  const int N = seg + 3;
  int i0 = 0, nw = seg;
  if (!follow) {
    i0 = 1, nw = 0;
    if (Y.cfg.lookfwd) {
      double rq = Y.cfg.relax_time / dt_yaw;
      if (!(rq < (double)seg)) rq = (double)seg;
      const int relax_num = (int)rq;
      nw = seg - relax_num - 1;
      if (nw < 0) nw = 0;
    }
  }

  // 3. one lane per way-point: pd = pos(tf) - pos(tc), its norm, atan2
  for (int j = tid; j < nw; j += YP_NT) {
    const double tc = (double)(i0 + j) * dt_yaw;
    const double ts = tc + Y.cfg.forward_t;
    const double tf = ts < duration ? ts : duration;
    double pc[3], pf[3];
    spline_pos(u, p, n, C, tc, pc);
    spline_pos(u, p, n, C, tf, pf);
    const double x = pf[0] - pc[0], y = pf[1] - pc[1], z = pf[2] - pc[2];
    const bool far = sqrt(x * x + y * y + z * z) > 1e-6;
    ok[j] = far ? 1 : 0;
    wp[j] = far ? atan2(y, x) : 0.0;
  }
  __syncthreads();

  // 4. lane 0: the unwrap chain, the end yaw, the initial control points, pt_dist_
  if (tid == 0) {
    double s0 = Y.start_yaw[3 * b];
    const double s1 = Y.start_yaw[3 * b + 1], s2 = Y.start_yaw[3 * b + 2];
    if (!follow) {
      while (s0 < -YP_PI) s0 += 2 * YP_PI;
      while (s0 > YP_PI) s0 -= 2 * YP_PI;
    }
    double last_yaw = s0;
    for (int j = 0; j < nw; ++j) {
      // a stalled way-point repeats its predecessor; the first one has none (the reference reads waypts.back() of an
      // empty vector): it repeats last_yaw
      const double w = ok[j] ? yp_next_yaw(last_yaw, wp[j]) : last_yaw;
      wp[j] = w;
      last_yaw = w;
    }
    double e;
    if (follow) {
      double v[3];
      yp_vel(u, p, n, C, duration - Y.cfg.end_back, v);
      e = atan2(v[1], v[0]);
    } else {
      e = Y.end_yaw[b];
    }
    e = yp_next_yaw(last_yaw, e);
    for (int i = 0; i < N; ++i) q0[i] = 0.0;
    const double m02 = (1 / 3.0) * dt_yaw * dt_yaw, m12 = -(1 / 6.0) * dt_yaw * dt_yaw;
    q0[0] = 1.0 * s0 + (-dt_yaw) * s1 + m02 * s2;
    q0[1] = 1.0 * s0 + 0.0 * s1 + m12 * s2;
    q0[2] = 1.0 * s0 + dt_yaw * s1 + m02 * s2;
    q0[seg] = 1.0 * e + (-dt_yaw) * 0.0 + m02 * 0.0;
    q0[seg + 1] = 1.0 * e + 0.0 * 0.0 + m12 * 0.0;
    q0[seg + 2] = 1.0 * e + dt_yaw * 0.0 + m02 * 0.0;
    double pd = 0.0;
    for (int i = 0; i + 1 < N; ++i) pd += fabs(q0[i + 1] - q0[i]);
    pd /= (double)N;
    sh[0] = s0, sh[1] = e, sh[2] = pd;
    sh[3] = (pd == 0.0 || !isfinite(pd)) ? 1.0 : 0.0;
  }
  __syncthreads();
  const double s0 = sh[0], s1 = Y.start_yaw[3 * b + 1], s2 = Y.start_yaw[3 * b + 2];
  const double e = sh[1], pt_dist = sh[2];
  bool degenerate = sh[3] != 0.0;
  const bool end3 = follow;  // planYaw passes three end entries, planYawExplore two

  // 5. one lane per row of the normal equations
  if (!degenerate) {
    const double cs = Y.ld_smooth, cp = 10.0 * Y.ld_start, cv = Y.ld_start, ce = Y.ld_end, cw = Y.ld_waypt;
    for (int r = tid; r < N; r += YP_NT) {
      double h[4] = {0.0, 0.0, 0.0, 0.0}, gr = 0.0;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int c = r - d;
        if (c < 0) continue;
        double s = 0.0;
        for (int i = max(0, r - 3); i <= min(c, N - 4); ++i) s += (yp_J(r - i) / pt_dist) * (yp_J(c - i) / pt_dist);
        double hd = cs * s;
        if (r <= 2)
          hd += cp * (yp_P(r) * yp_P(c)) + cv * (yp_V(r, dt_yaw) * yp_V(c, dt_yaw)) +
                cv * (yp_A(r, dt_yaw) * yp_A(c, dt_yaw));
        if (c >= N - 3) {
          const int rr = r - (N - 3), cc = c - (N - 3);
          double t = yp_P(rr) * yp_P(cc) + yp_V(rr, dt_yaw) * yp_V(cc, dt_yaw);
          if (end3) t += yp_A(rr, dt_yaw) * yp_A(cc, dt_yaw);
          hd += ce * t;
        }
        double sw = 0.0;
        for (int i = max(i0, r - 2); i <= min(c, i0 + nw - 1); ++i) sw += yp_P(r - i) * yp_P(c - i);
        hd += cw * sw;
        h[d] = hd;
      }
      if (r <= 2) gr += cp * (s0 * yp_P(r)) + cv * (s1 * yp_V(r, dt_yaw)) + cv * (s2 * yp_A(r, dt_yaw));
      if (r >= N - 3) gr += ce * (e * yp_P(r - (N - 3)));
      double sw = 0.0;
      for (int i = max(i0, r - 2); i <= min(r, i0 + nw - 1); ++i) sw += wp[i - i0] * yp_P(r - i);
      gr += cw * sw;
#pragma unroll
      for (int d = 0; d < 4; ++d) band[4 * r + d] = h[d];
      g[r] = gr;
    }
    __syncthreads();

    // 6. lane 0: banded Cholesky (the loops of k_waypoint_traj), both substitutions, the objective at the result
    if (tid == 0) {
      constexpr int hb = 3;
      bool bad = false;
      for (int j = 0; j < N && !bad; ++j) {
        double s = band[4 * j];
        for (int d = 1; d <= hb && d <= j; ++d) s -= band[4 * j + d] * band[4 * j + d];
        if (!(s > 0.0) || !isfinite(s)) {
          bad = true;
          break;
        }
        const double ljj = sqrt(s);
        band[4 * j] = ljj;
        for (int i = j + 1; i <= j + hb && i < N; ++i) {
          double t = band[4 * i + (i - j)];
          for (int k = max(0, i - hb); k < j; ++k) t -= band[4 * i + (i - k)] * band[4 * j + (j - k)];
          band[4 * i + (i - j)] = t / ljj;
        }
      }
      double cost = 0.0;
      if (!bad) {
        for (int j = 0; j < N; ++j) {
          double s = g[j];
          for (int d = 1; d <= hb && d <= j; ++d) s -= band[4 * j + d] * g[j - d];
          g[j] = s / band[4 * j];
        }
        for (int j = N - 1; j >= 0; --j) {
          double s = g[j];
          for (int d = 1; d <= hb; ++d)
            if (j + d < N) s -= band[4 * (j + d) + d] * g[j + d];
          g[j] = s / band[4 * j];
        }
        // combineCost (bspline_optimizer.cpp:571-630) in the reference's order
        double fs = 0.0;
        for (int i = 0; i + 3 < N; ++i) {
          const double ji = (g[i + 3] - 3 * g[i + 2] + 3 * g[i + 1] - g[i]) / pt_dist;
          fs += ji * ji;
        }
        double f0 = 0.0, dq;
        dq = 1 / 6.0 * (g[0] + 4 * g[1] + g[2]) - s0;
        f0 += 10.0 * (dq * dq);
        dq = 1 / (2 * dt_yaw) * (g[2] - g[0]) - s1;
        f0 += dq * dq;
        dq = 1 / (dt_yaw * dt_yaw) * (g[0] - 2 * g[1] + g[2]) - s2;
        f0 += dq * dq;
        double fe = 0.0;
        const double q3 = g[N - 3], q2 = g[N - 2], q1 = g[N - 1];
        dq = 1 / 6.0 * (q1 + 4 * q2 + q3) - e;
        fe += dq * dq;
        dq = 1 / (2 * dt_yaw) * (q1 - q3) - 0.0;
        fe += dq * dq;
        if (end3) {
          dq = 1 / (dt_yaw * dt_yaw) * (q1 - 2 * q2 + q3) - 0.0;
          fe += dq * dq;
        }
        double fw = 0.0;
        for (int j = 0; j < nw; ++j) {
          const int i = i0 + j;
          dq = 1 / 6.0 * (g[i] + 4 * g[i + 1] + g[i + 2]) - wp[j];
          fw += dq * dq;
        }
        cost = 0.0;
        cost += Y.ld_smooth * fs;
        cost += Y.ld_start * f0;
        cost += Y.ld_end * fe;
        cost += Y.ld_waypt * fw;
        if (!isfinite(cost)) bad = true;
      }
      sh[4] = bad ? 1.0 : 0.0;
      sh[5] = bad ? 0.0 : cost;
    }
    __syncthreads();
    degenerate = sh[4] != 0.0;
  }
  const double cost = degenerate ? 0.0 : sh[5];

  // 7. the yaw spline's knots: setUniformBspline(yaw, 3, dt_yaw) in planYawExplore, (yaw, bspline_degree_, dt_yaw) in
  // planYaw; then everything is written side by side
  const int py = follow ? p : 3;
  if (tid == 0) spline_uniform_knots(u, py, N, dt_yaw);
  __syncthreads();
  yp_write(Y, b, tid, degenerate ? FUELMI_YAW_DEGENERATE : FUELMI_YAW_OK, duration, seg, dt_yaw, N, degenerate ? q0 : g,
           nw, wp, e, cost, u, py);
}

size_t yp_lds(int max_ctrl, int max_seg) {
  const size_t maxs = (size_t)max_seg, maxn = maxs + 3;
  return ((size_t)yp_knots(max_ctrl, max_seg) + maxs + 4 * maxn + maxn + maxn + 8) * sizeof(double) + maxs * sizeof(int);
}

bool fin_nonneg(double x) { return std::isfinite(x) && x >= 0.0; }

int yaw_cfg_check(const fuelmi_yaw_cfg* cfg) {
  ARGCHK(cfg);
  ARGCHK(cfg->mode == FUELMI_YAW_EXPLORE || cfg->mode == FUELMI_YAW_FOLLOW);
  ARGCHK(cfg->pos_degree >= 3 && cfg->pos_degree <= 5);
  ARGCHK(cfg->max_ctrl >= cfg->pos_degree + 1);
  ARGCHK(cfg->max_seg >= 1 && cfg->max_seg <= FUELMI_YAW_MAX_SEG);
  if (cfg->mode == FUELMI_YAW_EXPLORE) ARGCHK(cfg->seg_num >= 1 && cfg->seg_num <= cfg->max_seg);
  ARGCHK(fin_nonneg(cfg->forward_t) && fin_nonneg(cfg->relax_time) && fin_nonneg(cfg->dt_target) &&
         fin_nonneg(cfg->end_back));
  if (cfg->mode == FUELMI_YAW_FOLLOW) ARGCHK(cfg->dt_target > 0.0);
  if (cfg->max_ctrl > FUELMI_YAW_MAX_CTRL) {
    fuelmi_set_error("yaw plan: max_ctrl = %d exceeds %d", cfg->max_ctrl, FUELMI_YAW_MAX_CTRL);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

// the caller's host arrays of both entries (the first three null for a device batch: the host does not see its splines)
struct YawIO {
  const int* n_ctrl;
  const double *pos_ctrl, *knot_span, *start_yaw, *end_yaw;
  int *status, *seg_num, *n_waypt;
  double *duration, *dt_yaw, *yaw_ctrl, *waypts, *end_yaw_out, *cost, *yawdot_ctrl, *yawddot_ctrl;  // the last two or null
  const double* knots = nullptr;  // fuelmi_map_plan_yaws_knots: [n_prob][max_ctrl + pos_degree + 1] in place of knot_span
  bool knots_given = false;
};

int yaw_check(const fuelmi_bspline_cfg* w, const fuelmi_yaw_cfg* cfg, int n_prob, const YawIO& io) {
  {
    const int rc = yaw_cfg_check(cfg);
    if (rc) return rc;
  }
  ARGCHK(w);
  ARGCHK(std::isfinite(w->ld_smooth) && std::isfinite(w->ld_start) && std::isfinite(w->ld_end) &&
         std::isfinite(w->ld_waypt));
  ARGCHK(w->ld_smooth > 0.0 && w->ld_start > 0.0);
  ARGCHK(n_prob >= 0);
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(io.start_yaw);
  ARGCHK(io.end_yaw || cfg->mode == FUELMI_YAW_FOLLOW);
  for (int b = 0; b < n_prob; ++b) {
    for (int k = 0; k < 3; ++k) ARGCHK(std::fabs(io.start_yaw[3 * b + k]) <= 1e3);
    if (cfg->mode == FUELMI_YAW_EXPLORE) ARGCHK(std::fabs(io.end_yaw[b]) <= 1e3);
  }
  if (io.n_ctrl) {  // (a device batch: its variables are checked by the kernel)
    const int rc = spline_src_check(n_prob, cfg->pos_degree, cfg->max_ctrl, io.n_ctrl, io.pos_ctrl, io.knot_span, io.knots_given);
    if (rc) return rc;
    if (io.knots_given) {
      const int rck = spline_knots_check(n_prob, cfg->pos_degree, cfg->max_ctrl, io.n_ctrl, 0, io.knots);
      if (rck) return rck;
    }
  }
  ARGCHK(io.status && io.duration && io.seg_num && io.dt_yaw && io.yaw_ctrl && io.n_waypt && io.waypts &&
         io.end_yaw_out && io.cost);
  return FUELMI_OK;
}

// Y cleared, then its part that comes from the two configs
void yaw_args(const fuelmi_bspline_cfg* w, const fuelmi_yaw_cfg* cfg, int n_prob, YawArgs& Y) {
  memset(&Y, 0, sizeof(Y));
  Y.cfg = *cfg;
  Y.ld_smooth = w->ld_smooth, Y.ld_start = w->ld_start, Y.ld_end = w->ld_end, Y.ld_waypt = w->ld_waypt;
  Y.n_prob = n_prob;
}

// the result arrays, each declared once; the derivatives' control points only where the caller asks
void yaw_results(ResultBlock& R, YawArgs& Y, const YawIO& io) {
  const size_t n = (size_t)Y.n_prob, maxs = (size_t)Y.cfg.max_seg;
  R.add(Y.status, io.status, n);
  R.add(Y.seg_num, io.seg_num, n);
  R.add(Y.n_waypt, io.n_waypt, n);
  R.add(Y.duration, io.duration, n);
  R.add(Y.dt_yaw, io.dt_yaw, n);
  R.add(Y.end_yaw_out, io.end_yaw_out, n);
  R.add(Y.cost, io.cost, n);
  R.add(Y.yaw_ctrl, io.yaw_ctrl, n * (maxs + 3));
  R.add(Y.waypts, io.waypts, n * maxs);
  R.opt(Y.yawdot_ctrl, io.yawdot_ctrl, n * (maxs + 2));
  R.opt(Y.yawddot_ctrl, io.yawddot_ctrl, n * (maxs + 1));
}

// behind the results in the caller's arrays: FUELMI_ELIMIT when a problem's status is -1
int yaw_limit(const YawArgs& Y, const YawIO& io) {
  const int b = first_over_limit(io.status, Y.n_prob);
  if (b < 0) return FUELMI_OK;
  fuelmi_set_error("yaw plan: problem %d needs %d yaw segments, more than max_seg = %d", b, io.seg_num[b],
                   Y.cfg.max_seg);
  return FUELMI_ELIMIT;
}

int yaw_launch(hipStream_t st, const YawArgs& Y) {
  const size_t lds = yp_lds(Y.cfg.max_ctrl, Y.cfg.max_seg);  // < 64 KiB at the documented limits
  hipLaunchKernelGGL(k_yaw_plan, dim3(Y.n_prob), dim3(YP_NT), lds, st, Y);
  HIPCHK(hipGetLastError());
  return FUELMI_OK;
}

}  // namespace

extern "C" int fuelmi_yaw_plan(const fuelmi_yaw_cfg* cfg, int out3[3]) {
  ARGCHK(out3);
  {
    const int rc = yaw_cfg_check(cfg);
    if (rc) return rc;
  }
  out3[0] = YP_NT, out3[1] = (int)yp_lds(cfg->max_ctrl, cfg->max_seg), out3[2] = FUELMI_YAW_MAX_CTRL;
  return FUELMI_OK;
}

// the host route of both entries: staged in a query slot's pinned block, launched on the slot's stream, copied out of the
// pinned block; the position splines uniform (knot_span) or on given knots
static int yaw_host(fuelmi_map* m, const fuelmi_bspline_cfg* w, const fuelmi_yaw_cfg* cfg, int n_prob, const YawIO& io) {
  const int* n_ctrl = io.n_ctrl;
  const double *pos_ctrl = io.pos_ctrl, *knot_span = io.knot_span, *start_yaw = io.start_yaw, *end_yaw = io.end_yaw;
  {  // every argument on the host, before the map is touched
    ARGCHK(n_prob <= 0 || n_ctrl);
    const int rc = yaw_check(w, cfg, n_prob, io);
    if (rc) return rc;
  }
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  const size_t n = (size_t)n_prob, maxc = (size_t)cfg->max_ctrl;
  YawArgs Y;
  yaw_args(w, cfg, n_prob, Y);
  ResultBlock R(16);
  yaw_results(R, Y, io);
  ARGCHK(!R.overflow);
  const size_t ks = maxc + cfg->pos_degree + 1;
  int* p_nc;
  double *p_knot, *p_end, *p_pos, *p_start, *p_knots = nullptr;
  auto layout = [&](unsigned char* base) {  // the slot's pinned block: the inputs, then the results
    BlockLayout L(base, 16);
    p_nc = L.take<int>(n);
    p_knot = L.take<double>(n);
    if (io.knots_given) p_knots = L.take<double>(n * ks);
    p_end = L.take<double>(n);
    p_pos = L.take<double>(n * maxc * 3);
    p_start = L.take<double>(n * 3);
    R.place(L);
    return L.size();
  };
  QuerySlotGuard q;
  {
    const int rcq = q.acquire(m, layout(nullptr));
    if (rcq) return rcq;
  }
  layout(q.s->pin);
  memcpy(p_nc, n_ctrl, n * sizeof(int));
  if (knot_span)
    memcpy(p_knot, knot_span, n * sizeof(double));
  else
    memset(p_knot, 0, n * sizeof(double));
  if (end_yaw)
    memcpy(p_end, end_yaw, n * sizeof(double));
  else
    memset(p_end, 0, n * sizeof(double));
  memcpy(p_pos, pos_ctrl, n * maxc * 3 * sizeof(double));
  memcpy(p_start, start_yaw, n * 3 * sizeof(double));
  Y.src = {p_nc, 0, p_pos, maxc * 3, p_knot, 1};
  if (io.knots_given) {
    memcpy(p_knots, io.knots, n * ks * sizeof(double));
    Y.src.knots = p_knots, Y.src.knots_stride = ks;
  }
  Y.start_yaw = p_start, Y.end_yaw = p_end;
  {
    const int rc = yaw_launch(q.s->st, Y);
    if (rc) return rc;
  }
  HIPCHK(q.finish());
  R.scatter(R.base);
  return yaw_limit(Y, io);
}

extern "C" int fuelmi_map_plan_yaws(fuelmi_map* m, const fuelmi_bspline_cfg* w, const fuelmi_yaw_cfg* cfg, int n_prob,
                                    const int* n_ctrl, const double* pos_ctrl, const double* knot_span,
                                    const double* start_yaw, const double* end_yaw, int* status, double* duration,
                                    int* seg_num, double* dt_yaw, double* yaw_ctrl, int* n_waypt, double* waypts,
                                    double* end_yaw_out, double* cost, double* yawdot_ctrl, double* yawddot_ctrl) {
  const YawIO io = {n_ctrl, pos_ctrl, knot_span, start_yaw, end_yaw,     status, seg_num,     n_waypt,
                    duration, dt_yaw, yaw_ctrl,  waypts,    end_yaw_out, cost,   yawdot_ctrl, yawddot_ctrl};
  return yaw_host(m, w, cfg, n_prob, io);
}

// ... the position splines on whole knot vectors (fuelmi_map_adjust_trajs' knots_out as it stands) in place of the
// spans; the yaw spline that comes out is uniform, as the reference builds it
extern "C" int fuelmi_map_plan_yaws_knots(fuelmi_map* m, const fuelmi_bspline_cfg* w, const fuelmi_yaw_cfg* cfg, int n_prob,
                                          const int* n_ctrl, const double* pos_ctrl, const double* knots,
                                          const double* start_yaw, const double* end_yaw, int* status, double* duration,
                                          int* seg_num, double* dt_yaw, double* yaw_ctrl, int* n_waypt, double* waypts,
                                          double* end_yaw_out, double* cost, double* yawdot_ctrl, double* yawddot_ctrl) {
  const YawIO io = {n_ctrl,   pos_ctrl, nullptr,     start_yaw, end_yaw,     status,       seg_num, n_waypt, duration,
                    dt_yaw,   yaw_ctrl, waypts,      end_yaw_out, cost,      yawdot_ctrl,  yawddot_ctrl, knots, true};
  return yaw_host(m, w, cfg, n_prob, io);
}

// the batch route: the splines the batch's last solve left on the device; staged in yaw_dev on the map's stream, downloaded
extern "C" int fuelmi_bspline_dev_plan_yaws(fuelmi_bspline_dev* b, const fuelmi_yaw_cfg* cfg, const double* start_yaw,
                                            const double* end_yaw, int* status, double* duration, int* seg_num,
                                            double* dt_yaw, double* yaw_ctrl, int* n_waypt, double* waypts,
                                            double* end_yaw_out, double* cost, double* yawdot_ctrl,
                                            double* yawddot_ctrl) {
  ARGCHK(b && cfg);
  const BsplineArgs& A = b->a;
  ARGCHK(A.dim == 3 && b->opt_valid && b->opt_x);
  ARGCHK(cfg->pos_degree == A.cfg.bspline_degree);
  fuelmi_yaw_cfg yc = *cfg;
  yc.max_ctrl = A.N;  // (yaw_cfg_check's max_ctrl >= pos_degree + 1 is the batch's N >= degree + 1)
  const YawIO io = {nullptr,  nullptr, nullptr,  start_yaw, end_yaw,     status, seg_num,     n_waypt,
                    duration, dt_yaw,  yaw_ctrl, waypts,    end_yaw_out, cost,   yawdot_ctrl, yawddot_ctrl};
  {
    const int rc = yaw_check(&A.cfg, &yc, A.C, io);
    if (rc) return rc;
  }
  fuelmi_map* m = b->map;
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  const size_t C = (size_t)A.C;
  YawArgs Y;
  yaw_args(&A.cfg, &yc, A.C, Y);
  ResultBlock R(16);
  yaw_results(R, Y, io);
  ARGCHK(!R.overflow);
  double *d_start, *d_end;
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 16);
    d_start = L.take<double>(C * 3);
    d_end = L.take<double>(C);
    R.place(L);
    return L.size();
  };
  hipStream_t st = m->stream;
  {
    const int rc = b->yaw_dev.carve(st, layout);
    if (rc) return rc;
  }
  HIPCHK(hipMemcpyAsync(d_start, start_yaw, C * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  if (end_yaw)
    HIPCHK(hipMemcpyAsync(d_end, end_yaw, C * sizeof(double), hipMemcpyHostToDevice, st));
  else
    HIPCHK(hipMemsetAsync(d_end, 0, C * sizeof(double), st));
  Y.src = opt_spline_src_knots(b);
  Y.start_yaw = d_start, Y.end_yaw = d_end;
  {
    StageScope sc(m, FUELMI_K_BSPLINE);
    const int rc = yaw_launch(st, Y);
    if (rc) return rc;
  }
  {
    const int rc = result_fetch(R, st);
    if (rc) return rc;
  }
  return yaw_limit(Y, io);
}
