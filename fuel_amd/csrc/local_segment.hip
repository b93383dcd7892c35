// local_segment.hip -- the head of FastPlannerManager::topoReplan's chain (plan_manage/src/planner_manager.cpp):
// paramLocalTraj (:605-617) and reparamLocalTraj (:619-634) for a batch of problems on a batch of trajectory states:
//   GlobalTrajData::getState             (plan_manage/include/plan_manage/plan_container.hpp:64-71) the polynomial global
//                                        trajectory stitched with the local spline and its two derivative splines
//   getTrajInfoInSphere   (:88-112)      the 0.2 s steps out to the radius or the trajectory's end -> seg_num, duration, dt
//   getTrajInfoInDuration (:74-85)       the points at the accumulated tp and the four boundary derivatives
//   parameterizeToBspline                k_bspline_fit (bspline.hip) behind the kernel, each problem its own point count
//
// k_local_segment: one 64-lane wave per problem, LS_WAVES problems per workgroup.  A wave keeps its state in LDS: the
// segment times, the coefficients, the local control points and their knots (setUniformBspline's accumulated additions,
// lane 0).  A step depends on its index alone -- its time is `min(. + 0.2, global_duration - start_t)` applied j times to
// 0, its point -- so the lanes take a window of 64 consecutive steps: each lane repeats the window's additions up to its
// own step, the 64 getState calls run side by side, one ballot of the loop's test (taken on step j's point for step
// j + 1) finds the last body that runs, and the distances up to it are added in step order.  The sample loop is the
// same scheme over `tp += dt`, one lane per point; the point count is the result of that accumulation.  The four
// boundary derivatives go on four lanes.
//
// All f64, -ffp-contract=off.  A result does not depend on the problem's place in the batch: the only workgroup-wide
// step is the barrier behind the staging.
// Behind the kernel, the two entries that share its checks and launch: fuelmi_map_local_segments (host arrays in and out)
// and fuelmi_bspline_dev_load_local_segments (points straight into a device batch's fit, bspline_batch.h).
#include <cmath>
#include <cstring>
#include <vector>

#include "bspline_batch.h"
#include "poly_internal.h"

namespace {

constexpr int LS_WIN = 64;    // steps / points per window: one per lane
constexpr int LS_WAVES = 2;   // problems per workgroup: 139.8 KiB of LDS at the largest strides
constexpr int LS_COUNT_CAP = FUELMI_WPTRAJ_MAX_SEG + 2;  // points: counting stops behind the window that passes it

// k_local_segment: one problem per wave; every pointer addresses device memory
struct LocalSegArgs {
  fuelmi_localseg_cfg cfg;
  int n_prob;
  int need_points;          // the loader: the batch's point count, any other is FUELMI_LOCALSEG_MISFIT; 0: none asked for
  // states
  const int* n_seg;         // [n_traj]
  const double* seg_times;  // [n_traj][max_seg]
  const double* coef;       // [n_traj][max_seg][3][6]
  const double* gdur;       // [n_traj]
  const int* n_local;       // [n_traj]
  const double* local_ctrl; // [n_traj][max_ctrl][3]
  const double *span, *lts, *lte, *tchg, *linc;  // [n_traj]
  // problems
  const int *traj_of, *mode;
  const double *start_t, *arg0, *arg1;
  // results, zeroed in front of the launch
  int *status, *n_steps, *seg_num, *n_points, *n_ctrl;
  int* fit_k;               // the fit's count: n_points of an OK problem, else 0
  double *segment_len, *duration, *dt;
  double* points;           // [n][max_points][3]
  double* derivs;           // [n][4][3]
};

// doubles of one wave's LDS block: times | coefficients | control points | knots
__host__ __device__ inline size_t ls_wave_doubles(const fuelmi_localseg_cfg& c) {
  return (size_t)c.max_seg * 19 + (size_t)c.max_ctrl * 3 + (size_t)spline_knot_stride(c.max_ctrl);
}

// a wave's GlobalTrajData
struct LsState {
  const double *T, *cf, *C, *u;  // LDS
  int S, nl, p;
  double gdur, lts, lte, tchg, linc;
};

// getState(t, k); false: the local branch of a state without a local trajectory
__device__ __forceinline__ bool ls_get_state(const LsState& s, double t, int k, double out[3]) {
  if (t >= -1e-3 && t <= s.lts) {
    poly_eval(s.cf, s.T, s.S, t - s.tchg + s.linc, k, out);
    return true;
  }
  if (t >= s.lte && t <= s.gdur + 1e-3) {
    poly_eval(s.cf, s.T, s.S, t - s.tchg, k, out);
    return true;
  }
  if (s.nl == 0) {
    out[0] = out[1] = out[2] = 0.0;
    return false;
  }
  double o[3][3];  // local_traj_[0 .. 2] at t - local_start_time_
  const double tl = t - s.lts;
  if (s.p == 3)
    spline_eval_levels<3, 3, 2>(s.u, s.nl, s.C, tl, o);
  else if (s.p == 4)
    spline_eval_levels<4, 3, 2>(s.u, s.nl, s.C, tl, o);
  else
    spline_eval_levels<5, 3, 2>(s.u, s.nl, s.C, tl, o);
  out[0] = o[k][0], out[1] = o[k][1], out[2] = o[k][2];
  return true;
}

// segment_time of a lane's step: `segment_time = min(segment_time + 0.2, lim)` applied lane + 1 times to base, one at a
// time; next = the value behind the window
__device__ __forceinline__ double ls_step_chain(double base, double lim, int lane, double& next) {
  double acc = base, v = base;
  for (int j = 0; j < LS_WIN; ++j) {
    const double a = acc + 0.2;
    acc = lim < a ? lim : a;  // std::min(a, lim)
    if (j == lane) v = acc;
  }
  next = acc;
  return v;
}

// tp of a lane's point: base plus `lane` additions of dt
__device__ __forceinline__ double ls_tp_chain(double base, double dt, int lane, double& next) {
  double acc = base, v = base;
  for (int j = 0; j < LS_WIN; ++j) {
    if (j == lane) v = acc;
    acc = acc + dt;
  }
  next = acc;
  return v;
}

__device__ __forceinline__ double ls_norm(const double a[3], const double b[3]) {
  const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
  return sqrt(x * x + y * y + z * z);
}

__global__ void __launch_bounds__(LS_WIN * LS_WAVES) k_local_segment(LocalSegArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x & (LS_WIN - 1), wv = threadIdx.x >> 6;
  const int b = blockIdx.x * LS_WAVES + wv;
  const int max_seg = A.cfg.max_seg, max_ctrl = A.cfg.max_ctrl, max_points = A.cfg.max_points;
  double* T = reinterpret_cast<double*>(smem_raw) + (size_t)wv * ls_wave_doubles(A.cfg);  // [max_seg]
  double* cf = T + max_seg;                // [max_seg][3][6]
  double* C = cf + (size_t)max_seg * 18;  // [max_ctrl][3]
  double* u = C + (size_t)max_ctrl * 3;   // [nl + p + 1]
  const bool live_prob = b < A.n_prob;
  LsState s;
  s.T = T, s.cf = cf, s.C = C, s.u = u;
  s.S = 0, s.nl = 0, s.p = A.cfg.degree;
  s.gdur = s.lts = s.lte = s.tchg = s.linc = 0.0;

  // 1. the state into LDS; every wave of the workgroup meets at the barrier, with or without a problem
  if (live_prob) {
    const int tr = A.traj_of[b];
    s.S = A.n_seg[tr], s.nl = A.n_local[tr];
    s.gdur = A.gdur[tr], s.lts = A.lts[tr], s.lte = A.lte[tr], s.tchg = A.tchg[tr], s.linc = A.linc[tr];
    const double* gT = A.seg_times + (size_t)tr * max_seg;
    const double* gc = A.coef + (size_t)tr * max_seg * 18;
    const double* gC = A.local_ctrl + (size_t)tr * max_ctrl * 3;
    for (int i = lane; i < s.S; i += LS_WIN) T[i] = gT[i];
    for (int i = lane; i < 18 * s.S; i += LS_WIN) cf[i] = gc[i];
    for (int i = lane; i < 3 * s.nl; i += LS_WIN) C[i] = gC[i];
    if (s.nl > 0 && lane == 0) spline_uniform_knots(u, s.p, s.nl, A.span[tr]);
  }
  __syncthreads();
  if (!live_prob) return;

  const bool sphere = A.mode[b] == FUELMI_LOCALSEG_SPHERE;
  const double start_t = A.start_t[b];
  bool no_local = false;
  int n_steps = 0, seg_num = 0;
  double segment_len = 0.0, duration = A.arg0[b], dt = A.arg1[b];

  // 2. getTrajInfoInSphere's loop, LS_WIN steps a window
  if (sphere) {
    const double radius = A.arg0[b], dist_pt = A.arg1[b];
    const double lim = s.gdur - start_t, stop = s.gdur - 1e-3;
    double segment_time = 0.0;
    double first[3];
    no_local = !ls_get_state(s, start_t, 0, first);
    bool run = !no_local && ls_norm(first, first) < radius && start_t + segment_time < stop;  // the test before step 1
    double prev[3] = {first[0], first[1], first[2]};
    double base = 0.0;
    while (run) {
      double next;
      const double sj = ls_step_chain(base, lim, lane, next);
      double cur[3];
      const bool ok = ls_get_state(s, start_t + sj, 0, cur);
      const bool pass = ok && ls_norm(cur, first) < radius && start_t + sj < stop;  // the test behind this lane's step
      const unsigned long long m_fail = ~__ballot(pass);
      const int nrun = m_fail ? __builtin_ctzll(m_fail) + 1 : LS_WIN;  // the step in front of a failed test still runs
      if (__ballot(!ok && lane < nrun) != 0ull) {
        no_local = true;
        break;
      }
      double pv[3];
      for (int c = 0; c < 3; ++c) {
        pv[c] = __shfl_up(cur[c], 1);
        if (lane == 0) pv[c] = prev[c];
      }
      const double d = ls_norm(cur, pv);
      for (int j = 0; j < nrun; ++j) segment_len = segment_len + __shfl(d, j);
      segment_time = __shfl(sj, nrun - 1);
      n_steps += nrun;
      if (m_fail) break;
      for (int c = 0; c < 3; ++c) prev[c] = __shfl(cur[c], LS_WIN - 1);
      base = next;
    }
    if (!no_local) {
      double q = floor(segment_len / dist_pt);
      if (!(q < (double)FUELMI_WPTRAJ_MAX_SEG)) q = (double)FUELMI_WPTRAJ_MAX_SEG;
      seg_num = (int)q;
      seg_num = seg_num < 6 ? 6 : seg_num;
      duration = segment_time;
      dt = duration / seg_num;
    }
  }

  // 3. getTrajInfoInDuration: the points, LS_WIN a window; row r is lane r % LS_WIN's
  int status = FUELMI_LOCALSEG_OK, n_points = 0;
  double* pts = A.points + (size_t)b * max_points * 3;
  if (no_local) {
    status = FUELMI_LOCALSEG_NO_LOCAL;
  } else if (!(isfinite(dt) && dt > 0.0)) {
    status = FUELMI_LOCALSEG_DEGENERATE;
  } else {
    const double lim = duration + 1e-4;
    double base = 0.0;
    for (;;) {
      double next;
      const double tp = ls_tp_chain(base, dt, lane, next);
      const unsigned long long m_dead = ~__ballot(tp <= lim);
      const int nlive = m_dead ? __builtin_ctzll(m_dead) : LS_WIN;
      bool ok = true;
      if (lane < nlive) {
        double q[3];
        ok = ls_get_state(s, start_t + tp, 0, q);
        if (ok && n_points + lane < max_points)
          for (int c = 0; c < 3; ++c) pts[3 * (size_t)(n_points + lane) + c] = q[c];
      }
      n_points += nlive;  // (with this window's rows: they are taken back below if one of them had no local spline)
      if (__ballot(!ok) != 0ull) {
        no_local = true;
        break;
      }
      if (nlive < LS_WIN || n_points > LS_COUNT_CAP) break;
      base = next;
    }
    // 4. the boundary derivatives on four lanes: k = 1 at both ends, then k = 2
    if (!no_local) {
      double q[3] = {0.0, 0.0, 0.0};
      bool ok = true;
      if (lane < 4) ok = ls_get_state(s, (lane & 1) ? start_t + duration : start_t, lane < 2 ? 1 : 2, q);
      no_local = __ballot(!ok) != 0ull;
      if (n_points < 2)
        status = FUELMI_LOCALSEG_DEGENERATE;
      else if (A.need_points && n_points != A.need_points)
        status = FUELMI_LOCALSEG_MISFIT;
      else if (n_points > max_points)
        status = -1;
      if (!no_local && status != FUELMI_LOCALSEG_DEGENERATE && lane < 4)
        for (int c = 0; c < 3; ++c) A.derivs[(size_t)b * 12 + 3 * lane + c] = q[c];
    }
    if (no_local) status = FUELMI_LOCALSEG_NO_LOCAL;
    if (status == FUELMI_LOCALSEG_NO_LOCAL || status == FUELMI_LOCALSEG_DEGENERATE) {  // no points: each lane its own rows
      const int rows = n_points < max_points ? n_points : max_points;
      for (int r = lane; r < rows; r += LS_WIN) pts[3 * (size_t)r] = pts[3 * (size_t)r + 1] = pts[3 * (size_t)r + 2] = 0.0;
      n_points = 0;
    }
  }
  if (lane == 0) {
    A.status[b] = status;
    if (status != FUELMI_LOCALSEG_NO_LOCAL) {  // (the outputs were zeroed in front of the launch)
      A.n_steps[b] = n_steps, A.seg_num[b] = seg_num, A.n_points[b] = n_points;
      A.segment_len[b] = segment_len, A.duration[b] = duration, A.dt[b] = dt;
      if (status == FUELMI_LOCALSEG_OK) A.n_ctrl[b] = n_points + s.p - 1, A.fit_k[b] = n_points;
    }
  }
}

size_t ls_lds(const fuelmi_localseg_cfg& c) { return (size_t)LS_WAVES * ls_wave_doubles(c) * sizeof(double); }

int localseg_cfg_check(const fuelmi_localseg_cfg* cfg) {
  ARGCHK(cfg);
  ARGCHK(cfg->degree >= 3 && cfg->degree <= 5);
  ARGCHK(cfg->max_seg >= 1 && cfg->max_ctrl >= cfg->degree + 1 && cfg->max_points >= 2);
  if (cfg->max_seg > FUELMI_WPTRAJ_MAX_WAY - 1 || cfg->max_ctrl > FUELMI_TRAJCHK_MAX_CTRL ||
      cfg->max_points > FUELMI_LOCALSEG_MAX_POINTS) {
    fuelmi_set_error("local segments: max_seg %d / max_ctrl %d / max_points %d exceed %d / %d / %d", cfg->max_seg,
                     cfg->max_ctrl, cfg->max_points, FUELMI_WPTRAJ_MAX_WAY - 1, FUELMI_TRAJCHK_MAX_CTRL,
                     FUELMI_LOCALSEG_MAX_POINTS);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

// the fit's dynamic LDS for K points (fit_lds of bspline.hip)
size_t ls_fit_lds(int K, int degree) {
  const int n = K + degree - 1;
  return (size_t)(16 + 5 * n + 3 * n + 3 * n + 3 * (K + 4) + n + degree + 1) * sizeof(double);
}

inline bool ls_fin(double v) { return std::isfinite(v) && std::fabs(v) < 1e7; }

// every argument both entries share, on the host, before anything is touched
int localseg_check(const fuelmi_localseg_cfg* cfg, int n_traj, const int* n_seg, const double* seg_times,
                   const double* coef, const double* global_duration, const int* n_local_ctrl, const double* local_ctrl,
                   const double* local_knot_span, const double* local_ts, const double* local_te,
                   const double* time_change, const double* last_time_inc, int n_prob, const int* traj_of, const int* mode,
                   const double* start_t, const double* arg0, const double* arg1) {
  ARGCHK(n_traj >= 1 && n_prob >= 1);
  ARGCHK(n_seg && seg_times && coef && global_duration && n_local_ctrl && local_ctrl && local_knot_span && local_ts &&
         local_te && time_change && last_time_inc);
  ARGCHK(traj_of && mode && start_t && arg0 && arg1);
  for (int i = 0; i < n_traj; ++i) {
    ARGCHK(n_seg[i] >= 1 && n_seg[i] <= cfg->max_seg);
    ARGCHK(n_local_ctrl[i] == 0 || (n_local_ctrl[i] >= cfg->degree + 1 && n_local_ctrl[i] <= cfg->max_ctrl));
    const double* T = seg_times + (size_t)i * cfg->max_seg;
    const double* c = coef + (size_t)i * cfg->max_seg * 18;
    for (int k = 0; k < n_seg[i]; ++k) ARGCHK(ls_fin(T[k]));
    for (int k = 0; k < 18 * n_seg[i]; ++k) ARGCHK(ls_fin(c[k]));
    if (n_local_ctrl[i] != 0) {
      const double* P = local_ctrl + (size_t)i * cfg->max_ctrl * 3;
      for (int k = 0; k < 3 * n_local_ctrl[i]; ++k) ARGCHK(ls_fin(P[k]));
      ARGCHK(ls_fin(local_knot_span[i]) && local_knot_span[i] > 0.0);
    }
    ARGCHK(ls_fin(global_duration[i]) && ls_fin(local_ts[i]) && ls_fin(local_te[i]) && ls_fin(time_change[i]) &&
           ls_fin(last_time_inc[i]));
    if (global_duration[i] > FUELMI_WPTRAJ_MAX_DURATION) {
      fuelmi_set_error("local segments: state %d lasts %g s, more than %g s", i, global_duration[i],
                       FUELMI_WPTRAJ_MAX_DURATION);
      return FUELMI_ELIMIT;
    }
  }
  for (int b = 0; b < n_prob; ++b) {
    ARGCHK(traj_of[b] >= 0 && traj_of[b] < n_traj);
    ARGCHK(mode[b] == FUELMI_LOCALSEG_SPHERE || mode[b] == FUELMI_LOCALSEG_DURATION);
    ARGCHK(ls_fin(start_t[b]) && ls_fin(arg0[b]) && ls_fin(arg1[b]));
    if (mode[b] == FUELMI_LOCALSEG_SPHERE) ARGCHK(arg0[b] > 0.0 && arg1[b] > 0.0);
  }
  return FUELMI_OK;
}

// the inputs of both entries in a block; the upload on stream st
struct LsIn {
  int *n_seg, *n_local, *traj_of, *mode;
  double *seg_times, *coef, *gdur, *local_ctrl, *span, *lts, *lte, *tchg, *linc, *start_t, *arg0, *arg1;
};
void ls_in_take(BlockLayout& L, const fuelmi_localseg_cfg& c, size_t nt, size_t np, LsIn& I) {
  I.n_seg = L.take<int>(nt), I.n_local = L.take<int>(nt);
  I.traj_of = L.take<int>(np), I.mode = L.take<int>(np);
  I.seg_times = L.take<double>(nt * c.max_seg), I.coef = L.take<double>(nt * c.max_seg * 18);
  I.local_ctrl = L.take<double>(nt * c.max_ctrl * 3);
  I.gdur = L.take<double>(nt), I.span = L.take<double>(nt), I.lts = L.take<double>(nt), I.lte = L.take<double>(nt);
  I.tchg = L.take<double>(nt), I.linc = L.take<double>(nt);
  I.start_t = L.take<double>(np), I.arg0 = L.take<double>(np), I.arg1 = L.take<double>(np);
}
#define LS_UP(dst, src, count) HIPCHK(hipMemcpyAsync(dst, src, (count) * sizeof(*(dst)), hipMemcpyHostToDevice, st))
int ls_in_upload(hipStream_t st, const fuelmi_localseg_cfg& c, size_t nt, size_t np, const LsIn& I, LocalSegArgs& A,
                 const int* n_seg, const double* seg_times, const double* coef, const double* global_duration,
                 const int* n_local_ctrl, const double* local_ctrl, const double* local_knot_span, const double* local_ts,
                 const double* local_te, const double* time_change, const double* last_time_inc, const int* traj_of,
                 const int* mode, const double* start_t, const double* arg0, const double* arg1) {
  LS_UP(I.n_seg, n_seg, nt);
  LS_UP(I.n_local, n_local_ctrl, nt);
  LS_UP(I.traj_of, traj_of, np);
  LS_UP(I.mode, mode, np);
  LS_UP(I.seg_times, seg_times, nt * c.max_seg);
  LS_UP(I.coef, coef, nt * c.max_seg * 18);
  LS_UP(I.local_ctrl, local_ctrl, nt * c.max_ctrl * 3);
  LS_UP(I.gdur, global_duration, nt);
  LS_UP(I.span, local_knot_span, nt);
  LS_UP(I.lts, local_ts, nt);
  LS_UP(I.lte, local_te, nt);
  LS_UP(I.tchg, time_change, nt);
  LS_UP(I.linc, last_time_inc, nt);
  LS_UP(I.start_t, start_t, np);
  LS_UP(I.arg0, arg0, np);
  LS_UP(I.arg1, arg1, np);
  A.n_seg = I.n_seg, A.n_local = I.n_local, A.traj_of = I.traj_of, A.mode = I.mode;
  A.seg_times = I.seg_times, A.coef = I.coef, A.local_ctrl = I.local_ctrl;
  A.gdur = I.gdur, A.span = I.span, A.lts = I.lts, A.lte = I.lte, A.tchg = I.tchg, A.linc = I.linc;
  A.start_t = I.start_t, A.arg0 = I.arg0, A.arg1 = I.arg1;
  return FUELMI_OK;
}
#undef LS_UP

int localseg_launch(hipStream_t st, const LocalSegArgs& A) {
  const size_t lds = ls_lds(A.cfg);
  if (lds > 64 * 1024)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_local_segment),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_local_segment, dim3((A.n_prob + LS_WAVES - 1) / LS_WAVES), dim3(LS_WIN * LS_WAVES), lds, st, A);
  HIPCHK(hipGetLastError());
  return FUELMI_OK;
}

// the scalar results of n problems, each declared once (a null destination: in the block, fetched by the caller itself)
void ls_scalars(ResultBlock& R, size_t n, LocalSegArgs& A, int* status, int* n_steps, int* seg_num, int* n_points,
                int* n_ctrl, double* segment_len, double* duration) {
  R.add(A.status, status, n);
  R.add(A.n_steps, n_steps, n);
  R.add(A.seg_num, seg_num, n);
  R.add(A.n_points, n_points, n);
  R.add(A.n_ctrl, n_ctrl, n);
  R.hold(A.fit_k, n);
  R.add(A.segment_len, segment_len, n);
  R.add(A.duration, duration, n);
}

}  // namespace

extern "C" int fuelmi_localseg_plan(const fuelmi_localseg_cfg* cfg, int out8[8]) {
  ARGCHK(out8);
  {
    const int rc = localseg_cfg_check(cfg);
    if (rc) return rc;
  }
  out8[0] = LS_WIN, out8[1] = (int)ls_lds(*cfg), out8[2] = LS_WAVES, out8[3] = FUELMI_WPTRAJ_MAX_WAY - 1;
  out8[4] = FUELMI_TRAJCHK_MAX_CTRL, out8[5] = FUELMI_LOCALSEG_MAX_POINTS, out8[6] = (LS_COUNT_CAP / LS_WIN + 1) * LS_WIN;
  out8[7] = (int)ls_fit_lds(cfg->max_points, cfg->degree);
  return FUELMI_OK;
}

extern "C" int fuelmi_map_local_segments(fuelmi_map* m, const fuelmi_localseg_cfg* cfg, int n_traj, const int* n_seg,
                                         const double* seg_times, const double* coef, const double* global_duration,
                                         const int* n_local_ctrl, const double* local_ctrl,
                                         const double* local_knot_span, const double* local_ts, const double* local_te,
                                         const double* time_change, const double* last_time_inc, int n_prob,
                                         const int* traj_of, const int* mode, const double* start_t, const double* arg0,
                                         const double* arg1, int* status, int* n_steps, double* segment_len, int* seg_num,
                                         double* duration, double* dt, int* n_points, double* points, double* derivs,
                                         int* n_ctrl, double* ctrl) {
  {  // every argument on the host, before the map is touched
    const int rc = localseg_cfg_check(cfg);
    if (rc) return rc;
  }
  ARGCHK(n_prob >= 0 && n_traj >= 0);
  if (n_prob == 0) return FUELMI_OK;
  {
    const int rc = localseg_check(cfg, n_traj, n_seg, seg_times, coef, global_duration, n_local_ctrl, local_ctrl,
                                  local_knot_span, local_ts, local_te, time_change, last_time_inc, n_prob, traj_of, mode,
                                  start_t, arg0, arg1);
    if (rc) return rc;
  }
  ARGCHK(status && n_steps && segment_len && seg_num && duration && dt && n_points && points && derivs && n_ctrl && ctrl);
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const size_t nt = (size_t)n_traj, n = (size_t)n_prob, mp = (size_t)cfg->max_points,
               rows = mp + (size_t)cfg->degree - 1;
  LocalSegArgs A;
  memset(&A, 0, sizeof(A));
  LsIn I;
  FitArgs F;  // each problem's own count; a problem without points (fit_k = 0) is left zero
  memset(&F, 0, sizeof(F));
  ResultBlock R(16);  // the fit reads dt, points, derivs and writes ctrl in the block
  ls_scalars(R, n, A, status, n_steps, seg_num, n_points, n_ctrl, segment_len, duration);
  R.add(A.dt, dt, n);
  R.add(A.points, points, n * mp * 3);
  R.add(A.derivs, derivs, n * 12);
  R.add(F.ctrl, ctrl, n * rows * 3);
  ARGCHK(!R.overflow);
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 16);
    ls_in_take(L, *cfg, nt, n, I);
    R.place(L);
    return L.size();
  };
  {
    const int rc = m->localseg_dev.carve(st, layout);
    if (rc) return rc;
  }
  {
    const int rc = ls_in_upload(st, *cfg, nt, n, I, A, n_seg, seg_times, coef, global_duration, n_local_ctrl, local_ctrl,
                                local_knot_span, local_ts, local_te, time_change, last_time_inc, traj_of, mode, start_t,
                                arg0, arg1);
    if (rc) return rc;
  }
  HIPCHK(hipMemsetAsync(R.base, 0, R.size(), st));
  A.cfg = *cfg;
  A.n_prob = n_prob;
  {
    const int rc = localseg_launch(st, A);
    if (rc) return rc;
  }
  F.C = n_prob, F.K = cfg->max_points, F.degree = cfg->degree;
  F.ts = A.dt, F.points = A.points, F.derivs = A.derivs;
  F.stride = (long)(rows * 3);
  F.Ks = A.fit_k, F.pt_stride = (long)mp;
  {
    const int rc = fit_launch(m, F, st);
    if (rc) return rc;
  }
  {
    const int rc = result_fetch(R, st);
    if (rc) return rc;
  }
  const int b = first_over_limit(status, n_prob);
  if (b < 0) return FUELMI_OK;
  fuelmi_set_error("local segments: problem %d has %d points, more than max_points = %d", b, n_points[b],
                   cfg->max_points);
  return FUELMI_ELIMIT;
}

// the batch route: one problem per candidate -> points, derivatives and knot spans (k_local_segment, written into the
// batch's staging) -> the fit (k_bspline_fit, bspline.hip), all on the map's stream.  A candidate whose problem is not OK
// or gives another point count than the batch's keeps its state.
extern "C" int fuelmi_bspline_dev_load_local_segments(
    fuelmi_bspline_dev* b, int max_seg, int max_ctrl, int n_traj, const int* n_seg, const double* seg_times,
    const double* coef, const double* global_duration, const int* n_local_ctrl, const double* local_ctrl,
    const double* local_knot_span, const double* local_ts, const double* local_te, const double* time_change,
    const double* last_time_inc, const int* traj_of, const int* mode, const double* start_t, const double* arg0,
    const double* arg1, int* status, double* duration) {
  ARGCHK(b && status);
  BsplineArgs& Ab = b->a;
  const int degree = Ab.cfg.bspline_degree;
  ARGCHK(Ab.dim == 3 && degree >= 3 && degree <= 5 && Ab.N - degree + 1 >= 2);
  fuelmi_localseg_cfg cfg;
  cfg.degree = degree, cfg.max_seg = max_seg, cfg.max_ctrl = max_ctrl, cfg.max_points = Ab.N - degree + 1;
  {
    const int rc = localseg_cfg_check(&cfg);
    if (rc) return rc;
  }
  {
    const int rc = localseg_check(&cfg, n_traj, n_seg, seg_times, coef, global_duration, n_local_ctrl, local_ctrl,
                                  local_knot_span, local_ts, local_te, time_change, last_time_inc, Ab.C, traj_of, mode,
                                  start_t, arg0, arg1);
    if (rc) return rc;
  }
  fuelmi_map* m = b->map;
  ARGCHK(m);
  opt_set_valid(b, false);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const size_t nt = (size_t)n_traj, C = (size_t)Ab.C, K = (size_t)cfg.max_points;
  LocalSegArgs A;
  memset(&A, 0, sizeof(A));
  LsIn I;
  ResultBlock R(16);  // only status and duration come back, in copies of their own
  ls_scalars(R, C, A, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  ARGCHK(!R.overflow);
  double* d_fit;  // ts | points | derivs: the layout fuelmi_bspline_dev_load_samples stages
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 16);
    d_fit = L.take<double>(C * (1 + K * 3 + 12));
    ls_in_take(L, cfg, nt, C, I);
    R.place(L);
    return L.size();
  };
  {
    const int rc = b->fit_in.carve(st, layout);
    if (rc) return rc;
  }
  {
    const int rc = ls_in_upload(st, cfg, nt, C, I, A, n_seg, seg_times, coef, global_duration, n_local_ctrl, local_ctrl,
                                local_knot_span, local_ts, local_te, time_change, last_time_inc, traj_of, mode, start_t,
                                arg0, arg1);
    if (rc) return rc;
  }
  HIPCHK(hipMemsetAsync(d_fit, 0, C * (1 + K * 3 + 12) * sizeof(double), st));
  HIPCHK(hipMemsetAsync(R.base, 0, R.size(), st));
  A.dt = d_fit;  // the fit's knot spans
  A.points = d_fit + C;
  A.derivs = d_fit + C + C * K * 3;
  A.cfg = cfg;
  A.n_prob = Ab.C;
  A.need_points = cfg.max_points;
  const FitArgs F = fit_args(b, A.dt, A.points, A.derivs, A.status);  // (a status that is not OK is not 0: skipped)
  {
    StageScope sc(m, FUELMI_K_BSPLINE);
    const int rcl = localseg_launch(st, A);
    if (rcl) return rcl;
    const int rcf = fit_launch(m, F);
    if (rcf) return rcf;
  }
  HIPCHK(hipMemcpyAsync(status, A.status, C * sizeof(int), hipMemcpyDeviceToHost, st));
  if (duration) HIPCHK(hipMemcpyAsync(duration, A.duration, C * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(stream_wait(st));
  return FUELMI_OK;
}
