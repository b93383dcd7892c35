// bspline_batch.h -- what bspline.hip shows the planner stages that have a fuelmi_bspline_dev_* entry: the device batch's
// state, the fit's argument record and three glue functions (all defined in bspline.hip, which shows nothing else); and
// the host half of a SplineSrc that the caller gives in host arrays.
#ifndef FUELMI_BSPLINE_BATCH_H_
#define FUELMI_BSPLINE_BATCH_H_

#include <cmath>

#include "fuelmi_internal.h"
#include "spline_internal.h"

struct BsplineArgs {
  fuelmi_bspline_cfg cfg;
  int cost_function, dim, N, C, end_n, n_waypt, nvar, order, n_guide;
  const double* x;
  const double* pt_dist;
  const double* knot_span;
  const double* time_lb;
  const double* start_state;
  const double* end_state;
  const double* guide_pts;
  const double* waypoints;
  const int* waypt_idx;
  const double* view_pt;
  const double* view_dir;
  const int* view_idx;
  double* cost;
  double* grad;
};

struct fuelmi_bspline_dev {
  fuelmi_map* map;  // cleared if the map is destroyed first (then only _destroy is legal)
  int device = 0;
  BsplineArgs a;
  std::vector<void*> allocs;
  size_t lds;       // evaluation scratch of one wave (the solves build on it)
  size_t lds_eval4; // ... plus the partial gradients / costs of the four-wave cost kernel
  double *opt_x = nullptr, *opt_cost = nullptr;  // fuelmi_bspline_dev_optimize outputs
  int* opt_evals = nullptr;
  // fuelmi_bspline_dev_eval_pinned: two pinned result slots (cost [C] | grad [C][nvar]) the cost kernel writes
  // directly, and the event behind each launch
  double* pin_out[2] = {nullptr, nullptr};
  hipEvent_t ev_out[2] = {nullptr, nullptr};
  bool opt_valid = false;    // opt_x holds the solve of what the batch holds now (a reload clears it)
  // the knots fuelmi_bspline_dev_adjust_trajs left for that solve: [C][N + degree + 1], allocated once (in allocs);
  // knot_source says whether check_trajs / sample_trajs / plan_yaws read them.  Only opt_set_valid changes opt_valid.
  double* adj_knots = nullptr;
  bool adj_valid = false;
  int knot_source = FUELMI_KNOTS_UNIFORM;
  // per-call scratch, reserved on the map's stream (every kernel that reads it runs there); no pointer into it
  // outlives the call that carved it
  DevScratch fit_in;   // fuelmi_bspline_dev_load_*: ts | points | derivs, then the loader's own arrays
  DevScratch yaw_dev;  // fuelmi_bspline_dev_plan_yaws: start | end | results
  DevScratch chk_dev;  // fuelmi_bspline_dev_check_trajs: t_now | results
  DevScratch smp_dev;  // fuelmi_bspline_dev_sample_trajs: yaw splines, times | results
  DevScratch adj_dev;  // fuelmi_bspline_dev_adjust_trajs: knots, ratios, groups | results
  DevScratch quad_dev; // fuelmi_bspline_dev_solve_quadratic: guide points | results
};

struct FitArgs {
  int C, K, degree;
  const double* ts;      // [C]
  const double* points;  // [C][K][3]
  const double* derivs;  // [C][4][3]  start vel, end vel, start acc, end acc
  double* ctrl;          // candidate c: ctrl + c * stride, (K + degree - 1) rows of 3
  long stride;
  // planner glue (all optional): what setBoundaryStates / optimize() derive from the fitted spline
  int write_dt;          // ctrl[c * stride + 3 n] = ts[c]   (trailing knot-span variable)
  double* knot_span;     // [C]
  double* pt_dist;       // [C]      optimize() :136-140
  double* start_state;   // [C][3][3]  getBoundaryStates(2, 0).start
  double* end_state;     // [C][3][3]  row 0 = getBoundaryStates(2, 0).end[0]
  const int* skip;       // [C] or null: a candidate with skip[c] != 0 is left as it is
  // a ragged batch (local_segment.hip): each candidate its own number of points, K the largest of them
  const int* Ks;         // [C] or null: candidate c fits Ks[c] <= K points (below 2: left as it is)
  long pt_stride;        // rows between two candidates' points; 0: the candidate's own count
};

// the fit of device samples into the batch's own state; its launch (st null: the map's stream); the position splines
// the last solve left on the device
FitArgs fit_args(const fuelmi_bspline_dev* b, double* ts, double* points, double* derivs, int* skip);
int fit_launch(fuelmi_map* m, const FitArgs& F, hipStream_t st = nullptr);
SplineSrc opt_spline_src(const fuelmi_bspline_dev* b);
// ... with the retained knots while the batch's knot source is FUELMI_KNOTS_ADJUSTED (the three calls that read them)
inline SplineSrc opt_spline_src_knots(const fuelmi_bspline_dev* b) {
  SplineSrc s = opt_spline_src(b);
  if (b->knot_source == FUELMI_KNOTS_ADJUSTED && b->adj_valid && b->adj_knots)
    s.knots = b->adj_knots, s.knots_stride = (size_t)b->a.N + b->a.cfg.bspline_degree + 1;
  return s;
}
// a reload (false) or a new solve (true): either way the retained knots belong to an earlier solve
inline void opt_set_valid(fuelmi_bspline_dev* b, bool valid) {
  b->opt_valid = valid;
  b->adj_valid = false;
  b->knot_source = FUELMI_KNOTS_UNIFORM;
}

// ---- a SplineSrc from the caller's host arrays n_ctrl [n], pos_ctrl [n][max_ctrl][3], knot_span [n] -----------------
// the arguments: every n_ctrl in degree + 1 .. max_ctrl, every knot span finite and positive (knots_given: the entry
// takes whole knot vectors, the spans are not read and may be null), every coordinate the spline reads below 1e7
inline int spline_src_check(int n_prob, int degree, int max_ctrl, const int* n_ctrl, const double* pos_ctrl,
                            const double* knot_span, bool knots_given = false) {
  ARGCHK(n_ctrl && pos_ctrl && (knot_span || knots_given));
  for (int b = 0; b < n_prob; ++b) {
    ARGCHK(n_ctrl[b] >= degree + 1 && n_ctrl[b] <= max_ctrl);
    if (!knots_given) ARGCHK(std::isfinite(knot_span[b]) && knot_span[b] > 0.0);
    const double* P = pos_ctrl + (size_t)b * max_ctrl * 3;
    for (int k = 0; k < 3 * n_ctrl[b]; ++k) ARGCHK(std::fabs(P[k]) < 1e7);
  }
  return FUELMI_OK;
}
// whole knot vectors knots [n][max_ctrl + degree + 1] given in place of spans (n_ctrl null: every problem has n_all
// control points): each problem's n_ctrl + degree + 1 knots finite and strictly increasing.  More than the reference
// asks, which asks nothing and divides by their differences.
inline int spline_knots_check(int n_prob, int degree, int max_ctrl, const int* n_ctrl, int n_all, const double* knots) {
  ARGCHK(knots);
  const size_t ks = (size_t)max_ctrl + degree + 1;
  for (int b = 0; b < n_prob; ++b) {
    const double* u = knots + (size_t)b * ks;
    const int m = (n_ctrl ? n_ctrl[b] : n_all) + degree;
    ARGCHK(std::isfinite(u[0]));
    for (int j = 1; j <= m; ++j) ARGCHK(std::isfinite(u[j]) && u[j - 1] < u[j]);
  }
  return FUELMI_OK;
}
// its three arrays in a block
inline void spline_src_take(BlockLayout& L, size_t n, int max_ctrl, SplineSrc& s) {
  s.n_ctrl = L.take<int>(n), s.n_ctrl_all = 0;
  s.knot = L.take<double>(n), s.knot_stride = 1;
  s.pos = L.take<double>(n * max_ctrl * 3), s.pos_stride = (size_t)max_ctrl * 3;
}
// ... filled from the caller's on stream st (knot_span null: zeros, for a kernel that does not read them)
inline int spline_src_upload(hipStream_t st, const SplineSrc& s, size_t n, int max_ctrl, const int* n_ctrl,
                             const double* pos_ctrl, const double* knot_span) {
  HIPCHK(hipMemcpyAsync(const_cast<int*>(s.n_ctrl), n_ctrl, n * sizeof(int), hipMemcpyHostToDevice, st));
  if (knot_span)
    HIPCHK(hipMemcpyAsync(const_cast<double*>(s.knot), knot_span, n * sizeof(double), hipMemcpyHostToDevice, st));
  else
    HIPCHK(hipMemsetAsync(const_cast<double*>(s.knot), 0, n * sizeof(double), st));
  HIPCHK(hipMemcpyAsync(const_cast<double*>(s.pos), pos_ctrl, n * max_ctrl * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  return FUELMI_OK;
}

#endif
