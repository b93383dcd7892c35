// traj_adjust.hip -- the half of the reference's NonUniformBspline (bspline/src/non_uniform_bspline.cpp) that moves the
// knots of a finished position spline and measures it, for a batch of problems (include/fuelmi.h has the contract):
//   checkRatio (:135-160), checkFeasibility (:443-487), lengthenTime (:162-176), the reallocateTime loop
//   (:346-441, planner_manager.cpp:222-230), getTimeSum, getLength (:271-281), getJerk (:283-298), getMeanAndMaxVel / Acc
//   (:300-344), the sampling half of reparamBspline (planner_manager.cpp:533-543) and selectBestTraj (:476-482).
// One 64-lane wave per problem, up to TA_MAX_WAVES problems per workgroup (as many as fit 64 KiB of LDS); the waves of a
// workgroup never meet.  Knots and control points live in LDS, one block per wave.  reallocateTime is serial: every lane
// makes the test of every i on the same LDS values, so the branch is uniform across the wave, and the lanes own the
// knots (knot j belongs to lane j % 64): each knot receives its additions one at a time, in the order of i.  The
// metric loops take windows of 64 samples: every lane accumulates the same t and keeps the one of its sample, the 64
// evaluations run side by side, then all lanes walk the window's samples in order by lane reads and make the same
// additions: the sums are the reference's, term by term.  All f64, -ffp-contract=off; min / max are the ternaries of
// std::min / std::max, so a value that is not a number takes the reference's way.
// Behind the kernels, the entries that share the checks, the layout and trajadj_run: fuelmi_map_adjust_trajs (splines
// from the host) and fuelmi_bspline_dev_adjust_trajs (the splines a device batch's last solve left, bspline_batch.h).
#include <cmath>
#include <cstring>
#include <vector>

#include "bspline_batch.h"

// the lanes of one wave meet: what every lane wrote to the wave's LDS block before is what every lane reads behind
__device__ __forceinline__ void ta_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

namespace {

constexpr int TA_WIN = 64;        // samples per window: one per lane
constexpr int TA_MAX_WAVES = 4;   // problems per workgroup at most
constexpr size_t TA_LDS_BUDGET = 64 * 1024;
constexpr int TA_MAX_STEPS = FUELMI_TRAJADJ_MAX_STEPS;

// k_traj_adjust: one problem per wave; every pointer addresses device memory
struct TrajAdjArgs {
  fuelmi_trajadj_cfg cfg;
  int n_prob;
  SplineSrc src;
  const double* knots_in;  // [n][max_ctrl + degree + 1] or null
  const double* ratio_in;  // [n] or null
  const int* group;        // [n] (SELECT)
  int* info;               // [n][FUELMI_TRAJADJ_NI]
  double* metrics;         // [n][FUELMI_TRAJADJ_NM]
  double* knots_out;       // [n][max_ctrl + degree + 1]
  double* samples;         // [n][max_samples][3] or null
  int* best;               // [n_group] (SELECT)
};

// doubles of one wave's LDS block: the knots, then the control points [max_ctrl][3]; a multiple of 16 bytes
__host__ __device__ inline int ta_wave_stride(int max_ctrl) { return spline_knot_stride(max_ctrl) + 3 * max_ctrl + (max_ctrl & 1); }
__host__ __device__ inline int ta_waves(int max_ctrl) {
  const int w = (int)(TA_LDS_BUDGET / ((size_t)ta_wave_stride(max_ctrl) * sizeof(double)));
  return w < 1 ? 1 : (w > TA_MAX_WAVES ? TA_MAX_WAVES : w);
}

__device__ __forceinline__ bool ta_any(bool x, int lane) {
  int v = x ? 1 : 0;
  for (int o = TA_WIN / 2; o > 0; o >>= 1) v |= __shfl(v, lane ^ o);
  return v != 0;
}
// std::max(a, b)
__device__ __forceinline__ double ta_max(double a, double b) { return a < b ? b : a; }
__device__ __forceinline__ double ta_wave_max(double v, int lane) {
  for (int o = TA_WIN / 2; o > 0; o >>= 1) v = ta_max(v, __shfl(v, lane ^ o));
  return v;
}

// vel of row i: p_ * (P.row(i + 1) - P.row(i)) / (u_(i + p_ + 1) - u_(i + 1))
__device__ __forceinline__ void ta_vel(const double* u, const double* P, int p, int i, double v[3]) {
  const double den = u[i + p + 1] - u[i + 1];
  for (int c = 0; c < 3; ++c) v[c] = (double)p * (P[3 * (i + 1) + c] - P[3 * i + c]) / den;
}
// acc of row i: p_ * (p_ - 1) * ((P.row(i + 2) - P.row(i + 1)) / (u_(i + p_ + 2) - u_(i + 2)) -
//                                (P.row(i + 1) - P.row(i)) / (u_(i + p_ + 1) - u_(i + 1))) / (u_(i + p_ + 1) - u_(i + 2))
__device__ __forceinline__ void ta_acc(const double* u, const double* P, int p, int i, double a[3]) {
  const double d1 = u[i + p + 2] - u[i + 2], d2 = u[i + p + 1] - u[i + 1], d3 = u[i + p + 1] - u[i + 2];
  const double s = (double)(p * (p - 1));
  for (int c = 0; c < 3; ++c)
    a[c] = s * ((P[3 * (i + 2) + c] - P[3 * (i + 1) + c]) / d1 - (P[3 * (i + 1) + c] - P[3 * i + c]) / d2) / d3;
}
__device__ __forceinline__ bool ta_over(const double v[3], double limit) {
  return fabs(v[0]) > limit + 1e-4 || fabs(v[1]) > limit + 1e-4 || fabs(v[2]) > limit + 1e-4;
}
__device__ __forceinline__ double ta_absmax(const double v[3]) {
  double m = -1.0;
  for (int c = 0; c < 3; ++c) m = ta_max(m, fabs(v[c]));
  return m;
}

// checkRatio (:135-160): the rows side by side, the maxima over lanes (std::max never takes a value that is not a
// number, so the order of the rows does not show)
__device__ double ta_check_ratio(const double* u, const double* P, int p, int n, int lane, const fuelmi_trajadj_cfg& c) {
  double max_vel = -1.0, max_acc = -1.0;
  for (int i = lane; i < n - 1; i += TA_WIN) {
    double v[3];
    ta_vel(u, P, p, i, v);
    max_vel = ta_max(max_vel, ta_absmax(v));
  }
  for (int i = lane; i < n - 2; i += TA_WIN) {
    double a[3];
    ta_acc(u, P, p, i, a);
    max_acc = ta_max(max_acc, ta_absmax(a));
  }
  max_vel = ta_wave_max(max_vel, lane), max_acc = ta_wave_max(max_acc, lane);
  return ta_max(max_vel / c.limit_vel, sqrt(fabs(max_acc) / c.limit_acc));
}

// checkFeasibility (:443-487)
__device__ bool ta_feasible(const double* u, const double* P, int p, int n, int lane, const fuelmi_trajadj_cfg& c) {
  bool bad = false;
  for (int i = lane; i < n - 1; i += TA_WIN) {
    double v[3];
    ta_vel(u, P, p, i, v);
    bad = bad || ta_over(v, c.limit_vel);
  }
  for (int i = lane; i < n - 2; i += TA_WIN) {
    double a[3];
    ta_acc(u, P, p, i, a);
    bad = bad || ta_over(a, c.limit_acc);
  }
  return !ta_any(bad, lane);
}

// this lane's first knot at or behind `from`
__device__ __forceinline__ int ta_first_own(int lane, int from) {
  return lane >= from ? lane : lane + ((from - lane + TA_WIN - 1) / TA_WIN) * TA_WIN;
}

// lengthenTime (:162-176)
__device__ void ta_lengthen(double* u, int p, int n, int lane, double ratio) {
  const int num1 = 2 * p - 1, num2 = (n + p) - 2 * p + 1, m = n + p;
  if (num1 >= num2) return;
  const double delta_t = (ratio - 1.0) * (u[num2] - u[num1]);
  const double t_inc = delta_t / (double)(num2 - num1);
  ta_wave_sync();
  for (int j = ta_first_own(lane, num1 + 1); j <= m; j += TA_WIN) u[j] = u[j] + (j <= num2 ? (double)(j - num1) * t_inc : delta_t);
  ta_wave_sync();
}

// reallocateTime (:346-441); every lane walks every i
__device__ bool ta_realloc(double* u, const double* P, int p, int n, int lane, const fuelmi_trajadj_cfg& c) {
  bool fea = true;
  const int m = n + p;
  for (int i = 0; i < n - 1; ++i) {
    double v[3];
    ta_vel(u, P, p, i, v);
    if (ta_over(v, c.limit_vel)) {
      fea = false;
      const double max_vel = ta_absmax(v);
      double ratio = max_vel / c.limit_vel + 1e-4;
      if (ratio > c.limit_ratio) ratio = c.limit_ratio;
      const double time_ori = u[i + p + 1] - u[i + 1];
      const double time_new = ratio * time_ori;
      const double delta_t = time_new - time_ori;
      const double t_inc = delta_t / (double)p;
      ta_wave_sync();
      for (int j = ta_first_own(lane, i + 2); j <= m; j += TA_WIN)
        u[j] = u[j] + (j <= i + p + 1 ? (double)(j - i - 1) * t_inc : delta_t);
      ta_wave_sync();
    }
  }
  for (int i = 0; i < n - 2; ++i) {
    double a[3];
    ta_acc(u, P, p, i, a);
    if (ta_over(a, c.limit_acc)) {
      fea = false;
      const double max_acc = ta_absmax(a);
      double ratio = sqrt(max_acc / c.limit_acc) + 1e-4;
      if (ratio > c.limit_ratio) ratio = c.limit_ratio;
      const double time_ori = u[i + p + 1] - u[i + 2];
      const double time_new = ratio * time_ori;
      const double delta_t = time_new - time_ori;
      const double t_inc = delta_t / (double)(p - 1);
      ta_wave_sync();
      if (i == 1 || i == 2) {
        for (int j = ta_first_own(lane, 2); j <= m; j += TA_WIN) u[j] = u[j] + (j <= 5 ? (double)(j - 1) * t_inc : 4.0 * t_inc);
      } else {
        for (int j = ta_first_own(lane, i + 3); j <= m; j += TA_WIN)
          u[j] = u[j] + (j <= i + p + 1 ? (double)(j - i - 2) * t_inc : delta_t);
      }
      ta_wave_sync();
    }
  }
  return fea;
}

// the number of t the loop `for (t = t0; t <= limit; t += step)` takes, counted to TA_MAX_STEPS + 1 at most
__device__ int ta_count(double t0, double step, double limit) {
  int cnt = 0;
  for (double t = t0; t <= limit && cnt <= TA_MAX_STEPS; t = t + step) ++cnt;
  return cnt;
}

// the clamp and the knot search of evaluateDeBoor (:52-57) for the ABSOLUTE parameter t
__device__ __forceinline__ int ta_span_abs(const double* u, int p, int n, double t, double& ub) {
  const double lo = u[p], hi = u[n];
  ub = lo < t ? t : lo;
  ub = hi < ub ? hi : ub;
  int k = p;
  while (k < n - 1 && u[k + 1] < ub) ++k;
  return k;
}

// the spline (L = 0) or its L-th derivative spline on span k at the clamped parameter ub
template <int P, int L>
__device__ __forceinline__ void ta_eval(const double* u, const double* C, int k, double ub, double out[3]) {
  double q[P + 1][3];
#pragma unroll
  for (int i = 0; i <= P; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) q[i][c] = C[3 * (k - P + i) + c];
  if constexpr (L >= 1) spline_derive<P, 3>(u, k, q);
  if constexpr (L >= 2) spline_derive<P - 1, 3>(u, k, q);
  spline_alpha<P - L, 3>(u, k, ub, q);
  out[0] = q[P - L][0], out[1] = q[P - L][1], out[2] = q[P - L][2];
}

// (x.norm() of the stand-in: s = 0, s += e * e per entry, sqrt)
__device__ __forceinline__ double ta_norm(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// this lane's t of the window that starts at t: every lane makes the window's 64 additions
__device__ __forceinline__ double ta_window_t(double& t, double step, int lane) {
  double mine = t;
  for (int j = 0; j < TA_WIN; ++j) {
    if (j == lane) mine = t;
    t = t + step;
  }
  return mine;
}

// getMeanAndMaxVel (L = 1) / Acc (L = 2) (:300-344) over cnt samples
template <int P, int L>
__device__ void ta_mean_max(const double* u, const double* C, int n, int lane, double step, int cnt, double& mean, double& mx) {
  mean = 0.0, mx = -1.0;
  double t = u[P];
  for (int base = 0; base < cnt; base += TA_WIN) {
    const double mine = ta_window_t(t, step, lane);
    double vn = 0.0;
    if (base + lane < cnt) {
      double ub, o[3];
      const int k = ta_span_abs(u, P, n, mine, ub);
      ta_eval<P, L>(u, C, k, ub, o);
      vn = ta_norm(o[0], o[1], o[2]);
    }
    const int w = cnt - base < TA_WIN ? cnt - base : TA_WIN;
    for (int j = 0; j < w; ++j) {
      const double v = __shfl(vn, j);
      mean = mean + v;
      if (v > mx) mx = v;
    }
  }
  mean = mean / (double)cnt;
}

// getLength (:271-281) over cnt steps
template <int P>
__device__ double ta_length(const double* u, const double* C, int n, int lane, double res, int cnt) {
  double length = 0.0, pl[3], ub;
  {
    const int k = spline_span(u, P, n, 0.0, ub);
    ta_eval<P, 0>(u, C, k, ub, pl);
  }
  double t = res;
  for (int base = 0; base < cnt; base += TA_WIN) {
    const double mine = ta_window_t(t, res, lane);
    double pn[3] = {0.0, 0.0, 0.0};
    if (base + lane < cnt) {
      const int k = spline_span(u, P, n, mine, ub);
      ta_eval<P, 0>(u, C, k, ub, pn);
    }
    double d[3];
    for (int c = 0; c < 3; ++c) {
      const double prev = __shfl(pn[c], lane > 0 ? lane - 1 : 0);
      d[c] = pn[c] - (lane > 0 ? prev : pl[c]);
    }
    const double nrm = ta_norm(d[0], d[1], d[2]);
    const int w = cnt - base < TA_WIN ? cnt - base : TA_WIN;
    for (int j = 0; j < w; ++j) length = length + __shfl(nrm, j);
    for (int c = 0; c < 3; ++c) pl[c] = __shfl(pn[c], TA_WIN - 1);
  }
  return length;
}

// getJerk (:283-298): row i of the third derivative spline from the rows i .. i + 3, the rows side by side
__device__ double ta_jerk(const double* u, const double* P, int p, int n, int lane) {
  double jerk = 0.0;
  const int rows = n - 3;
  for (int base = 0; base < rows; base += TA_WIN) {
    const int i = base + lane;
    double term[3] = {0.0, 0.0, 0.0};
    if (i < rows) {
      const double dtm = u[i + 4] - u[i + 3];
      for (int c = 0; c < 3; ++c) {
        double q1[3], q2[2];
        for (int k = 0; k < 3; ++k)
          q1[k] = (double)p * (P[3 * (i + k + 1) + c] - P[3 * (i + k) + c]) / (u[i + k + p + 1] - u[i + k + 1]);
        for (int k = 0; k < 2; ++k) q2[k] = (double)(p - 1) * (q1[k + 1] - q1[k]) / (u[i + k + p + 1] - u[i + k + 2]);
        const double q3 = (double)(p - 2) * (q2[1] - q2[0]) / (u[i + p + 1] - u[i + 3]);
        term[c] = dtm * q3 * q3;
      }
    }
    const int w = rows - base < TA_WIN ? rows - base : TA_WIN;
    for (int j = 0; j < w; ++j)
      for (int c = 0; c < 3; ++c) jerk = jerk + __shfl(term[c], j);
  }
  return jerk;
}

// the sampling of reparamBspline (planner_manager.cpp:541-543): cnt points, the rest of the stride 0
template <int P>
__device__ void ta_resample(const double* u, const double* C, int n, int lane, double dt, int cnt, int max_samples, double* out) {
  double t = 0.0;
  for (int base = 0; base < max_samples; base += TA_WIN) {
    const double mine = ta_window_t(t, dt, lane);
    double o[3] = {0.0, 0.0, 0.0};
    if (base + lane < cnt) {
      double ub;
      const int k = spline_span(u, P, n, mine, ub);
      ta_eval<P, 0>(u, C, k, ub, o);
    }
    if (base + lane < max_samples)
      for (int c = 0; c < 3; ++c) out[3 * (size_t)(base + lane) + c] = o[c];
  }
}

struct TaLoops {
  int cnt_len, cnt_vel, cnt_acc, cnt_smp;
  double length, mean_v, max_v, mean_a, max_a;
};

template <int P>
__device__ void ta_loops(const double* u, const double* C, int n, int lane, const fuelmi_trajadj_cfg& c, double dt_out, double* smp,
                         TaLoops& R) {
  R.length = ta_length<P>(u, C, n, lane, c.length_res, R.cnt_len);
  ta_mean_max<P, 1>(u, C, n, lane, c.stat_step, R.cnt_vel, R.mean_v, R.max_v);
  ta_mean_max<P, 2>(u, C, n, lane, c.stat_step, R.cnt_acc, R.mean_a, R.max_a);
  if (smp) ta_resample<P>(u, C, n, lane, dt_out, R.cnt_smp, c.max_samples, smp);
}

__global__ void __launch_bounds__(TA_WIN * TA_MAX_WAVES) k_traj_adjust(TrajAdjArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x & (TA_WIN - 1), wv = threadIdx.x >> 6;
  const int b = blockIdx.x * (blockDim.x >> 6) + wv;
  if (b >= A.n_prob) return;  // the waves of a workgroup never meet
  const fuelmi_trajadj_cfg& cfg = A.cfg;
  double* u = reinterpret_cast<double*>(smem_raw) + (size_t)wv * ta_wave_stride(cfg.max_ctrl);  // [n + p + 1]
  double* P = u + spline_knot_stride(cfg.max_ctrl);                                               // [n][3]
  const int p = cfg.degree, kstride = cfg.max_ctrl + p + 1;
  const int n = spline_n(A.src, b);
  const double dt = A.knots_in ? 1.0 : spline_dt(A.src, b);
  const bool sane = spline_sane(dt, n, p, cfg.max_ctrl);
  int* info = A.info + (size_t)b * FUELMI_TRAJADJ_NI;
  double* met = A.metrics + (size_t)b * FUELMI_TRAJADJ_NM;
  double* ko = A.knots_out + (size_t)b * kstride;
  double* smp = (cfg.ops & FUELMI_TRAJADJ_RESAMPLE) ? A.samples + (size_t)b * cfg.max_samples * 3 : nullptr;
  if (!sane) {  // BADSPLINE: nothing is indexed by the spline, every output 0
    if (lane < FUELMI_TRAJADJ_NI) info[lane] = lane == FUELMI_TRAJADJ_I_STATUS ? FUELMI_TRAJADJ_BADSPLINE : 0;
    if (lane < FUELMI_TRAJADJ_NM) met[lane] = 0.0;
    for (int j = lane; j < kstride; j += TA_WIN) ko[j] = 0.0;
    if (smp)
      for (int j = lane; j < 3 * cfg.max_samples; j += TA_WIN) smp[j] = 0.0;
    return;
  }
  const int m = n + p;  // the last knot

  // a. control points and knots into the wave's block
  {
    const double* src = spline_ctrl(A.src, b);
    for (int j = lane; j < 3 * n; j += TA_WIN) P[j] = src[j];
    if (A.knots_in) {
      const double* kin = A.knots_in + (size_t)b * kstride;
      for (int j = lane; j <= m; j += TA_WIN) u[j] = kin[j];
    } else if (lane == 0) {
      spline_uniform_knots(u, p, n, dt);
    }
  }
  ta_wave_sync();

  // b. on the input knots
  const double duration_in = u[n] - u[p];
  const double ratio = ta_check_ratio(u, P, p, n, lane, cfg);
  const bool feasible_in = ta_feasible(u, P, p, n, lane, cfg);

  // c. lengthenTime(min(cap, ratio))
  if (cfg.ops & FUELMI_TRAJADJ_LENGTHEN) {
    const double rin = A.ratio_in ? A.ratio_in[b] : ratio;
    ta_lengthen(u, p, n, lane, rin < cfg.lengthen_cap ? rin : cfg.lengthen_cap);
  }

  // d. the reallocation loop (planner_manager.cpp:222-230)
  int iters = 0;
  bool feasible = ta_feasible(u, P, p, n, lane, cfg);
  if (cfg.ops & FUELMI_TRAJADJ_REALLOC) {
    while (!feasible) {
      feasible = ta_realloc(u, P, p, n, lane, cfg);
      if (++iters >= cfg.realloc_iters) break;
    }
  }
  const bool feasible_out = ta_feasible(u, P, p, n, lane, cfg);

  // e. f. the final knots, the metrics, the samples
  for (int j = lane; j < kstride; j += TA_WIN) ko[j] = j <= m ? u[j] : 0.0;
  const double duration_out = u[n] - u[p];
  const double jerk = ta_jerk(u, P, p, n, lane);
  const double dt_out = duration_out / (double)(n - p);
  const double time_inc = duration_out - duration_in;
  TaLoops R;
  R.cnt_len = ta_count(cfg.length_res, cfg.length_res, duration_out + 1e-4);
  R.cnt_vel = ta_count(u[p], cfg.stat_step, u[n]);  // the derivative splines' getTimeSpan is [u[p], u[n]] too
  R.cnt_acc = R.cnt_vel;
  R.cnt_smp = smp ? ta_count(0.0, dt_out, duration_out + 1e-4) : 0;
  R.length = R.mean_v = R.max_v = R.mean_a = R.max_a = 0.0;
  const bool is_long = R.cnt_len > TA_MAX_STEPS || R.cnt_vel > TA_MAX_STEPS || R.cnt_smp > TA_MAX_STEPS || R.cnt_smp > cfg.max_samples;
  if (is_long) {
    R.cnt_len = R.cnt_vel = R.cnt_acc = R.cnt_smp = 0;
    if (smp)
      for (int j = lane; j < 3 * cfg.max_samples; j += TA_WIN) smp[j] = 0.0;
  } else if (p == 3) {
    ta_loops<3>(u, P, n, lane, cfg, dt_out, smp, R);
  } else if (p == 4) {
    ta_loops<4>(u, P, n, lane, cfg, dt_out, smp, R);
  } else {
    ta_loops<5>(u, P, n, lane, cfg, dt_out, smp, R);
  }
  if (lane == 0) {
    info[FUELMI_TRAJADJ_I_STATUS] = is_long ? FUELMI_TRAJADJ_LONG : FUELMI_TRAJADJ_OK;
    info[FUELMI_TRAJADJ_I_FEASIBLE_IN] = feasible_in ? 1 : 0;
    info[FUELMI_TRAJADJ_I_ITERS] = iters;
    info[FUELMI_TRAJADJ_I_FEASIBLE] = feasible ? 1 : 0;
    info[FUELMI_TRAJADJ_I_FEASIBLE_OUT] = feasible_out ? 1 : 0;
    info[FUELMI_TRAJADJ_I_NUM_VEL] = R.cnt_vel;
    info[FUELMI_TRAJADJ_I_NUM_ACC] = R.cnt_acc;
    info[FUELMI_TRAJADJ_I_N_SAMPLES] = R.cnt_smp;
    met[FUELMI_TRAJADJ_M_DURATION_IN] = duration_in;
    met[FUELMI_TRAJADJ_M_RATIO] = ratio;
    met[FUELMI_TRAJADJ_M_DURATION_OUT] = duration_out;
    met[FUELMI_TRAJADJ_M_LENGTH] = R.length;
    met[FUELMI_TRAJADJ_M_JERK] = jerk;
    met[FUELMI_TRAJADJ_M_MEAN_VEL] = R.mean_v;
    met[FUELMI_TRAJADJ_M_MAX_VEL] = R.max_v;
    met[FUELMI_TRAJADJ_M_MEAN_ACC] = R.mean_a;
    met[FUELMI_TRAJADJ_M_MAX_ACC] = R.max_a;
    met[FUELMI_TRAJADJ_M_DT_OUT] = dt_out;
    met[FUELMI_TRAJADJ_M_TIME_INC] = time_inc;
    met[FUELMI_TRAJADJ_NM - 1] = 0.0;
  }
}

// g. selectBestTraj: one wave per group; (jerk, index) has one smallest pair, so the order of the lanes does not show
__global__ void __launch_bounds__(TA_WIN) k_traj_select(TrajAdjArgs A) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int bi = -1;
  double bj = 0.0;
  for (int b = lane; b < A.n_prob; b += TA_WIN) {
    if (A.group[b] != g || A.info[(size_t)b * FUELMI_TRAJADJ_NI + FUELMI_TRAJADJ_I_STATUS] != FUELMI_TRAJADJ_OK) continue;
    const double j = A.metrics[(size_t)b * FUELMI_TRAJADJ_NM + FUELMI_TRAJADJ_M_JERK];
    if (j != j) continue;
    if (bi < 0 || j < bj) bi = b, bj = j;  // b only grows: a tie keeps the smaller index
  }
  for (int o = TA_WIN / 2; o > 0; o >>= 1) {
    const int oi = __shfl(bi, lane ^ o);
    const double oj = __shfl(bj, lane ^ o);
    if (oi >= 0 && (bi < 0 || oj < bj || (oj == bj && oi < bi))) bi = oi, bj = oj;
  }
  if (lane == 0) A.best[g] = bi;
}

size_t ta_lds(const fuelmi_trajadj_cfg& c) { return (size_t)ta_waves(c.max_ctrl) * ta_wave_stride(c.max_ctrl) * sizeof(double); }

int trajadj_cfg_check(const fuelmi_trajadj_cfg* cfg) {
  ARGCHK(cfg);
  const int all = FUELMI_TRAJADJ_LENGTHEN | FUELMI_TRAJADJ_REALLOC | FUELMI_TRAJADJ_RESAMPLE | FUELMI_TRAJADJ_SELECT;
  ARGCHK((cfg->ops & ~all) == 0);
  ARGCHK(cfg->degree >= 3 && cfg->degree <= 5);
  ARGCHK(cfg->max_ctrl >= cfg->degree + 1);
  ARGCHK(std::isfinite(cfg->limit_vel) && cfg->limit_vel > 0.0);
  ARGCHK(std::isfinite(cfg->limit_acc) && cfg->limit_acc > 0.0);
  ARGCHK(std::isfinite(cfg->limit_ratio) && cfg->limit_ratio > 1.0);
  ARGCHK(std::isfinite(cfg->lengthen_cap) && cfg->lengthen_cap >= 1.0);
  ARGCHK(cfg->realloc_iters >= 1 && cfg->realloc_iters <= 16);
  ARGCHK(std::isfinite(cfg->length_res) && cfg->length_res > 0.0);
  ARGCHK(std::isfinite(cfg->stat_step) && cfg->stat_step > 0.0);
  if (cfg->max_ctrl > FUELMI_TRAJADJ_MAX_CTRL) {
    fuelmi_set_error("trajectory adjustment: max_ctrl = %d exceeds %d", cfg->max_ctrl, FUELMI_TRAJADJ_MAX_CTRL);
    return FUELMI_ELIMIT;
  }
  if (cfg->ops & FUELMI_TRAJADJ_RESAMPLE) {
    ARGCHK(cfg->max_samples >= cfg->max_ctrl - cfg->degree + 2);
    if (cfg->max_samples > FUELMI_TRAJADJ_MAX_SAMPLES) {
      fuelmi_set_error("trajectory adjustment: max_samples = %d exceeds %d", cfg->max_samples, FUELMI_TRAJADJ_MAX_SAMPLES);
      return FUELMI_ELIMIT;
    }
  }
  if (cfg->ops & FUELMI_TRAJADJ_SELECT) {
    ARGCHK(cfg->n_group >= 1);
    if (cfg->n_group > FUELMI_TRAJADJ_MAX_PROB) {
      fuelmi_set_error("trajectory adjustment: n_group = %d exceeds %d", cfg->n_group, FUELMI_TRAJADJ_MAX_PROB);
      return FUELMI_ELIMIT;
    }
  }
  return FUELMI_OK;
}

// the caller's host arrays of both entries (the first three null for a device batch)
struct TrajAdjIO {
  const int* n_ctrl;
  const double *pos_ctrl, *knot_span;
  const double *knots_in, *ratio_in;
  const int* group;
  int* info;
  double *metrics, *knots_out, *samples;
  int* best;
};

// the scratch block (a BlockLayout over the map's or the batch's DevScratch): the inputs the host hands over, then the
// results.  base null: only the size.
size_t ta_layout(const fuelmi_trajadj_cfg& c, int n_prob, bool host_spline, const TrajAdjIO& io, TrajAdjArgs& A, unsigned char* base) {
  const size_t n = (size_t)n_prob, ks = (size_t)c.max_ctrl + c.degree + 1;
  BlockLayout L(base, 16);
  if (host_spline) spline_src_take(L, n, c.max_ctrl, A.src);
  A.knots_in = io.knots_in ? L.take<double>(n * ks) : nullptr;
  A.ratio_in = io.ratio_in ? L.take<double>(n) : nullptr;
  A.group = (c.ops & FUELMI_TRAJADJ_SELECT) ? L.take<int>(n) : nullptr;
  A.info = L.take<int>(n * FUELMI_TRAJADJ_NI);
  A.metrics = L.take<double>(n * FUELMI_TRAJADJ_NM);
  A.knots_out = L.take<double>(n * ks);
  A.samples = (c.ops & FUELMI_TRAJADJ_RESAMPLE) ? L.take<double>(n * c.max_samples * 3) : nullptr;
  A.best = (c.ops & FUELMI_TRAJADJ_SELECT) ? L.take<int>((size_t)c.n_group) : nullptr;
  return L.size();
}

// the host checks of both entries; n_all: the number of control points of every problem of a device batch
int trajadj_check(const fuelmi_trajadj_cfg* cfg, int n_prob, bool host_spline, int n_all, const TrajAdjIO& io) {
  {
    const int rc = trajadj_cfg_check(cfg);
    if (rc) return rc;
  }
  ARGCHK(n_prob >= 0);
  if (n_prob == 0) return FUELMI_OK;
  if (n_prob > FUELMI_TRAJADJ_MAX_PROB) {
    fuelmi_set_error("trajectory adjustment: n_prob = %d exceeds %d", n_prob, FUELMI_TRAJADJ_MAX_PROB);
    return FUELMI_ELIMIT;
  }
  const int p = cfg->degree;
  ARGCHK(io.info && io.metrics && io.knots_out);
  if (cfg->ops & FUELMI_TRAJADJ_RESAMPLE) ARGCHK(io.samples);
  if (cfg->ops & FUELMI_TRAJADJ_SELECT) ARGCHK(io.group && io.best);
  if (host_spline) {
    const int rc = spline_src_check(n_prob, p, cfg->max_ctrl, io.n_ctrl, io.pos_ctrl, io.knot_span, io.knots_in != nullptr);
    if (rc) return rc;
  }
  if (io.knots_in) {
    const int rc = spline_knots_check(n_prob, p, cfg->max_ctrl, host_spline ? io.n_ctrl : nullptr, n_all, io.knots_in);
    if (rc) return rc;
  }
  for (int b = 0; b < n_prob; ++b) {
    if (io.ratio_in) ARGCHK(std::isfinite(io.ratio_in[b]));
    if (cfg->ops & FUELMI_TRAJADJ_SELECT) ARGCHK(io.group[b] >= 0 && io.group[b] < cfg->n_group);
  }
  return FUELMI_OK;
}

size_t trajadj_bytes(const fuelmi_trajadj_cfg* cfg, int n_prob, bool host_spline, const TrajAdjIO& io) {
  TrajAdjArgs A;
  memset(&A, 0, sizeof(A));
  return ta_layout(*cfg, n_prob, host_spline, io, A, nullptr);
}

// uploads, the launches on stream st, the results into the caller's arrays and the wait.  A device batch presets A.src.
// keep: null, or where a device batch retains the final knots [n_prob][max_ctrl + degree + 1] (copied on the device).
int trajadj_run(hipStream_t st, const fuelmi_trajadj_cfg* cfg, int n_prob, bool host_spline, const TrajAdjIO& io, TrajAdjArgs& A,
                unsigned char* scratch, double* keep = nullptr) {
  const fuelmi_trajadj_cfg& c = *cfg;
  const size_t n = (size_t)n_prob, ks = (size_t)c.max_ctrl + c.degree + 1;
  A.cfg = c;
  A.n_prob = n_prob;
  ta_layout(c, n_prob, host_spline, io, A, scratch);
  auto up = [&](const void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
  };
  auto down = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
  };
  if (host_spline) {  // (knot_span may be null with knots_in: the kernel does not read the spans then)
    const int rc = spline_src_upload(st, A.src, n, c.max_ctrl, io.n_ctrl, io.pos_ctrl, io.knot_span);
    if (rc) return rc;
  }
  if (A.knots_in) HIPCHK(up(A.knots_in, io.knots_in, n * ks * sizeof(double)));
  if (A.ratio_in) HIPCHK(up(A.ratio_in, io.ratio_in, n * sizeof(double)));
  if (A.group) HIPCHK(up(A.group, io.group, n * sizeof(int)));
  const int waves = ta_waves(c.max_ctrl);
  hipLaunchKernelGGL(k_traj_adjust, dim3((n_prob + waves - 1) / waves), dim3(TA_WIN * waves), ta_lds(c), st, A);
  HIPCHK(hipGetLastError());
  if (A.best) {
    hipLaunchKernelGGL(k_traj_select, dim3(c.n_group), dim3(TA_WIN), 0, st, A);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(down(io.info, A.info, n * FUELMI_TRAJADJ_NI * sizeof(int)));
  HIPCHK(down(io.metrics, A.metrics, n * FUELMI_TRAJADJ_NM * sizeof(double)));
  HIPCHK(down(io.knots_out, A.knots_out, n * ks * sizeof(double)));
  if (keep) HIPCHK(hipMemcpyAsync(keep, A.knots_out, n * ks * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (A.samples) HIPCHK(down(io.samples, A.samples, n * c.max_samples * 3 * sizeof(double)));
  if (A.best) HIPCHK(down(io.best, A.best, (size_t)c.n_group * sizeof(int)));
  HIPCHK(stream_wait(st));
  return FUELMI_OK;
}

}  // namespace

extern "C" int fuelmi_traj_adjust_plan(const fuelmi_trajadj_cfg* cfg, int out3[3]) {
  ARGCHK(out3);
  {
    const int rc = trajadj_cfg_check(cfg);
    if (rc) return rc;
  }
  out3[0] = TA_WIN, out3[1] = (int)ta_lds(*cfg), out3[2] = FUELMI_TRAJADJ_MAX_CTRL;
  return FUELMI_OK;
}

extern "C" int fuelmi_map_adjust_trajs(fuelmi_map* m, const fuelmi_trajadj_cfg* cfg, int n_prob, const int* n_ctrl,
                                       const double* pos_ctrl, const double* knot_span, const double* knots_in,
                                       const double* ratio_in, const int* group, int* info, double* metrics,
                                       double* knots_out, double* samples, int* best) {
  const TrajAdjIO io = {n_ctrl, pos_ctrl, knot_span, knots_in, ratio_in, group, info, metrics, knots_out, samples, best};
  {  // every argument on the host, before the map is touched
    const int rc = trajadj_check(cfg, n_prob, true, 0, io);
    if (rc) return rc;
  }
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  {
    const int rc = m->trajadj_dev.reserve(st, trajadj_bytes(cfg, n_prob, true, io));
    if (rc) return rc;
  }
  TrajAdjArgs A;
  memset(&A, 0, sizeof(A));
  return trajadj_run(st, cfg, n_prob, true, io, A, m->trajadj_dev.base());
}

// the batch route: a device batch's optimised position splines adjusted, measured and ranked, read from the variables
// the last solve left on the device; only results travel
extern "C" int fuelmi_bspline_dev_adjust_trajs(fuelmi_bspline_dev* b, const fuelmi_trajadj_cfg* cfg, const double* knots_in,
                                               const double* ratio_in, const int* group, int* info, double* metrics,
                                               double* knots_out, double* samples, int* best) {
  ARGCHK(b && cfg);
  const BsplineArgs& A = b->a;
  ARGCHK(A.dim == 3 && b->opt_valid && b->opt_x);
  ARGCHK(cfg->degree == A.cfg.bspline_degree);
  fuelmi_trajadj_cfg sc = *cfg;
  sc.max_ctrl = A.N;
  const TrajAdjIO io = {nullptr, nullptr, nullptr, knots_in, ratio_in, group, info, metrics, knots_out, samples, best};
  {
    const int rc = trajadj_check(&sc, A.C, false, A.N, io);
    if (rc) return rc;
  }
  if (A.C == 0) return FUELMI_OK;
  fuelmi_map* m = b->map;
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  {
    const int rc = b->adj_dev.reserve(m->stream, trajadj_bytes(&sc, A.C, false, io));
    if (rc) return rc;
  }
  if (!b->adj_knots) {  // the knots this call leaves for check_trajs / sample_trajs / plan_yaws: once, freed with the batch
    void* d = nullptr;
    HIPCHK(hipMalloc(&d, (size_t)A.C * ((size_t)A.N + sc.degree + 1) * sizeof(double)));
    b->allocs.push_back(d);
    b->adj_knots = (double*)d;
  }
  b->adj_valid = false;
  TrajAdjArgs T;
  memset(&T, 0, sizeof(T));
  T.src = opt_spline_src(b);
  const int rc = trajadj_run(m->stream, &sc, A.C, false, io, T, b->adj_dev.base(), b->adj_knots);
  if (rc) {
    b->knot_source = FUELMI_KNOTS_UNIFORM;
    return rc;
  }
  b->adj_valid = true;
  return FUELMI_OK;
}

extern "C" int fuelmi_bspline_dev_set_knot_source(fuelmi_bspline_dev* b, int source) {
  ARGCHK(b);
  ARGCHK(source == FUELMI_KNOTS_UNIFORM || source == FUELMI_KNOTS_ADJUSTED);
  if (source == FUELMI_KNOTS_ADJUSTED && !(b->opt_valid && b->adj_valid && b->adj_knots)) {
    fuelmi_set_error("knot source: no fuelmi_bspline_dev_adjust_trajs has run since the batch's last solve");
    return FUELMI_EINVAL;
  }
  b->knot_source = source;
  return FUELMI_OK;
}

extern "C" int fuelmi_bspline_dev_knot_source(const fuelmi_bspline_dev* b) {
  return b ? b->knot_source : FUELMI_KNOTS_UNIFORM;
}
