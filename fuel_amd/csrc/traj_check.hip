// traj_check.hip -- the safety check of a flown trajectory: FastPlannerManager::checkTrajCollision
// (plan_manage/src/planner_manager.cpp:96-118) for a batch of problems (position control points, knot span, t_now)
// against the map's inflated plane, without a host mirror.
//
// The reference's loop only looks sequential.  For sample k = 1, 2, ... the time t_now + fut_t_k (fut_t summed k times),
// the point p_k, its inflated occupancy and the radius r_k = |p_k - cur| depend on k alone.  The loop enters body k iff
// r_(k-1) < max_radius && t_now + fut_t_k < duration held for every sample up to k (r_0 = 0), so it ends before the FIRST
// k where that fails, and the answer is the first occupied k in front of that end with distance = r_(k-1).
//
// One 64-lane wave per problem, TC_WAVES problems per workgroup.  The lanes take a window of 64 consecutive samples:
// each lane repeats the window's additions of `step` up to its own sample (lane 63's value plus one addition is the next
// window's base), evaluates its point by the literal de Boor recursion, reads its bit and takes r_(k-1) from the lane
// below (lane 0: lane 63 of the previous window).  Three ballots and a count of trailing zeros pick the first event.
// Knots are staged in LDS (one block per wave), by the accumulated additions or copied and checked as given; control points are read from global memory
// through L2: a window touches p + 1 neighbouring points per lane, 24 B each, and neighbouring lanes share them, so
// staging up to 24 KiB per problem would cost more than it saves.  All f64, -ffp-contract=off.  A result does not depend
// on the problem's place in the batch: the only workgroup-wide step is the barrier behind the knots.
// Behind the kernel, the entries that share its checks, layout and trajchk_run: fuelmi_map_check_trajs and
// fuelmi_map_check_trajs_knots (splines from the host, uniform or on given knots) and fuelmi_bspline_dev_check_trajs (the
// splines a device batch's last solve left, on the knots its adjustment left if the batch says so, bspline_batch.h).
#include <cmath>
#include <cstring>
#include <vector>

#include "bspline_batch.h"

namespace {

constexpr int TC_WIN = 64;   // samples per window: one per lane
constexpr int TC_WAVES = 4;  // problems per workgroup
constexpr int TC_CAP = FUELMI_TRAJCHK_MAX_SAMPLES;

// k_traj_check: one problem per wave; every pointer addresses device memory
struct TrajChkArgs {
  fuelmi_trajchk_cfg cfg;
  int n_prob;
  SplineSrc src;
  const double* t_now;      // [n]
  const u64* infl;          // the map's inflated plane
  int* status;
  int* safe;
  int* n_samples;
  int* hit_index;
  int* end_reason;
  double* distance;
  double* hit_t;
  double* duration;
  double* hit_pos;          // [n][3]
};

// not finite, or |coordinate| >= 1e7: the reference's cast to int is undefined there
__device__ __forceinline__ bool tc_bad(const double q[3]) {
  return !(fabs(q[0]) < 1e7 && fabs(q[1]) < 1e7 && fabs(q[2]) < 1e7);
}

// SDFMap::getInflateOccupancy(Vector3d) == 1: posToIndex's floor, isInMap(Vector3i) (outside: -1, which passes), the
// inflated plane's bit.  The range test is made on the floor's f64 result -- the same answer as pos_to_idx + idx_in_map
// for every value an int holds, and no cast of one it does not hold (fine maps: 1e7 * resolution_inv may pass 2^31)
__device__ __forceinline__ bool tc_inflated(const Geo& g, const u64* infl, const double q[3]) {
  const double fx = floor((q[0] - g.org[0]) * g.res_inv), fy = floor((q[1] - g.org[1]) * g.res_inv),
               fz = floor((q[2] - g.org[2]) * g.res_inv);
  if (!(fx >= 0.0 && fy >= 0.0 && fz >= 0.0 && fx <= (double)(g.nx - 1) && fy <= (double)(g.ny - 1) &&
        fz <= (double)(g.nz - 1)))
    return false;
  const long a = (long)(int)fx * g.nyz + (long)(int)fy * g.nz + (int)fz;
  return bit_at(infl, a);
}

// everything a problem reports, by the one lane that knows it
__device__ void tc_write(const TrajChkArgs& T, int b, int status, int safe, double distance, int n_samples, int hit_index,
                         double hit_t, const double* hit_pos, int end_reason, double duration) {
  T.status[b] = status;
  T.safe[b] = safe;
  T.distance[b] = distance;
  T.n_samples[b] = n_samples;
  T.hit_index[b] = hit_index;
  T.hit_t[b] = hit_t;
  for (int c = 0; c < 3; ++c) T.hit_pos[3 * b + c] = hit_pos ? hit_pos[c] : 0.0;
  T.end_reason[b] = end_reason;
  T.duration[b] = duration;
}

__global__ void __launch_bounds__(TC_WIN * TC_WAVES) k_traj_check(Geo g, TrajChkArgs T) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x & (TC_WIN - 1), wv = threadIdx.x >> 6;
  const int b = blockIdx.x * TC_WAVES + wv;
  double* u = reinterpret_cast<double*>(smem_raw) + (size_t)wv * spline_knot_stride(T.cfg.max_ctrl);  // [n + p + 1]
  const int p = T.cfg.degree;
  const bool live = b < T.n_prob;
  int n = 0;
  double dt = 0.0;
  if (live) {
    n = spline_n(T.src, b);
    dt = spline_dt_or_one(T.src, b);
  }

  // 1. knots; every wave of the workgroup meets at the barrier, with or without a problem
  const bool sane = spline_stage_knots(T.src, b, u, p, n, dt, lane, live && spline_sane(dt, n, p, T.cfg.max_ctrl));
  __syncthreads();
  if (!live) return;
  if (!sane) {
    if (lane == 0)
      tc_write(T, b, FUELMI_TRAJCHK_NONFINITE, 0, 0.0, 0, 0, 0.0, nullptr, FUELMI_TRAJCHK_END_NONFINITE, 0.0);
    return;
  }
  const double* C = spline_ctrl(T.src, b);
  const double t_now = T.t_now[b], step = T.cfg.step, max_radius = T.cfg.max_radius;
  const double duration = u[n] - u[p];

  // 2. cur
  double cur[3];
  spline_pos(u, p, n, C, t_now, cur);
  if (tc_bad(cur)) {
    if (lane == 0)
      tc_write(T, b, FUELMI_TRAJCHK_NONFINITE, 0, 0.0, 0, 0, t_now, nullptr, FUELMI_TRAJCHK_END_NONFINITE, duration);
    return;
  }

  // 3. windows of TC_WIN samples; r_carry = r of the sample in front of the window, fut_base = fut_t of its first sample
  double r_carry = 0.0, fut_base = step;
  for (int kb = 1;; kb += TC_WIN) {
    double acc = fut_base, fut = fut_base;
    for (int j = 0; j < TC_WIN; ++j) {  // fut_t of sample kb + lane: the base plus `lane` additions, one at a time
      if (j == lane) fut = acc;
      acc = acc + step;
    }
    const int k = kb + lane;
    const double t = t_now + fut;
    double q[3];
    spline_pos(u, p, n, C, t, q);
    const bool bad = tc_bad(q);
    const double dx = q[0] - cur[0], dy = q[1] - cur[1], dz = q[2] - cur[2];
    const double r = sqrt(dx * dx + dy * dy + dz * dz);
    double r_prev = __shfl_up(r, 1);
    if (lane == 0) r_prev = r_carry;
    const bool end = !(r_prev < max_radius) || !(t < duration);  // the while condition fails in front of body k
    const bool over = k > TC_CAP;                                // body k would be one too many
    const bool hit = !bad && tc_inflated(g, T.infl, q);
    const unsigned long long m_end = __ballot(end), m_stop = __ballot(bad || over), m_hit = __ballot(hit);
    const unsigned long long m = m_end | m_stop | m_hit;
    if (m) {
      if (lane == __builtin_ctzll(m)) {  // the first sample with an event; on one sample: end, cap, bad point, hit
        if (end)
          tc_write(T, b, FUELMI_TRAJCHK_OK, 1, -1.0, k - 1, 0, 0.0, nullptr,
                   !(r_prev < max_radius) ? FUELMI_TRAJCHK_END_RADIUS : FUELMI_TRAJCHK_END_DURATION, duration);
        else if (over)
          tc_write(T, b, -1, 0, r_prev, TC_CAP, 0, 0.0, nullptr, FUELMI_TRAJCHK_END_CAP, duration);
        else if (bad)
          tc_write(T, b, FUELMI_TRAJCHK_NONFINITE, 0, 0.0, k, k, t, nullptr, FUELMI_TRAJCHK_END_NONFINITE, duration);
        else
          tc_write(T, b, FUELMI_TRAJCHK_OK, 0, r_prev, k, k, t, q, FUELMI_TRAJCHK_END_HIT, duration);
      }
      return;
    }
    r_carry = __shfl(r, TC_WIN - 1);
    fut_base = acc;
  }
}

size_t tc_lds(int max_ctrl) { return (size_t)TC_WAVES * spline_knot_stride(max_ctrl) * sizeof(double); }

int trajchk_cfg_check(const fuelmi_trajchk_cfg* cfg) {
  ARGCHK(cfg);
  ARGCHK(cfg->degree >= 3 && cfg->degree <= 5);
  ARGCHK(cfg->max_ctrl >= cfg->degree + 1);
  ARGCHK(std::isfinite(cfg->step) && cfg->step >= 1e-3);
  ARGCHK(std::isfinite(cfg->max_radius) && cfg->max_radius > 0.0);
  if (cfg->max_ctrl > FUELMI_TRAJCHK_MAX_CTRL) {
    fuelmi_set_error("trajectory check: max_ctrl = %d exceeds %d", cfg->max_ctrl, FUELMI_TRAJCHK_MAX_CTRL);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

// the caller's host arrays of both entries (the first three null for a device batch: the host does not see its splines)
struct TrajChkIO {
  const int* n_ctrl;
  const double *pos_ctrl, *knot_span, *t_now;
  int *status, *safe, *n_samples, *hit_index, *end_reason;
  double *distance, *hit_t, *hit_pos, *duration;
  const double* knots = nullptr;  // fuelmi_map_check_trajs_knots: [n_prob][max_ctrl + degree + 1] in place of knot_span
  bool knots_given = false;
};

int trajchk_check(const fuelmi_trajchk_cfg* cfg, int n_prob, const TrajChkIO& io) {
  {
    const int rc = trajchk_cfg_check(cfg);
    if (rc) return rc;
  }
  ARGCHK(n_prob >= 0);
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(io.t_now);
  for (int b = 0; b < n_prob; ++b) ARGCHK(std::isfinite(io.t_now[b]));
  if (io.n_ctrl) {  // (a device batch: its variables are checked by the kernel)
    const int rc = spline_src_check(n_prob, cfg->degree, cfg->max_ctrl, io.n_ctrl, io.pos_ctrl, io.knot_span, io.knots_given);
    if (rc) return rc;
    if (io.knots_given) {
      const int rck = spline_knots_check(n_prob, cfg->degree, cfg->max_ctrl, io.n_ctrl, 0, io.knots);
      if (rck) return rck;
    }
  }
  ARGCHK(io.status && io.safe && io.distance && io.n_samples && io.hit_index && io.hit_t && io.hit_pos && io.end_reason &&
         io.duration);
  return FUELMI_OK;
}

// the result arrays, each declared once
void trajchk_results(ResultBlock& R, TrajChkArgs& T, int n_prob, const TrajChkIO& io) {
  const size_t n = (size_t)n_prob;
  R.add(T.status, io.status, n);
  R.add(T.safe, io.safe, n);
  R.add(T.n_samples, io.n_samples, n);
  R.add(T.hit_index, io.hit_index, n);
  R.add(T.end_reason, io.end_reason, n);
  R.add(T.distance, io.distance, n);
  R.add(T.hit_t, io.hit_t, n);
  R.add(T.duration, io.duration, n);
  R.add(T.hit_pos, io.hit_pos, n * 3);
}

// both entries behind their uploads (T holds cfg, n_prob, src, t_now and the results R bound on the device), on the map's
// stream: launch, download, wait, the results into the caller's arrays (FUELMI_ELIMIT when a problem's status is -1)
int trajchk_run(fuelmi_map* m, TrajChkArgs& T, const ResultBlock& R, const TrajChkIO& io) {
  hipStream_t st = m->stream;
  const int n_prob = T.n_prob;
  T.infl = m->infl_bits.p;
  const size_t lds = tc_lds(T.cfg.max_ctrl);  // <= 32.2 KiB at FUELMI_TRAJCHK_MAX_CTRL
  hipLaunchKernelGGL(k_traj_check, dim3((n_prob + TC_WAVES - 1) / TC_WAVES), dim3(TC_WIN * TC_WAVES), lds, st, m->g, T);
  HIPCHK(hipGetLastError());
  {
    const int rc = result_fetch(R, st);
    if (rc) return rc;
  }
  const int b = first_over_limit(io.status, n_prob);
  if (b < 0) return FUELMI_OK;
  fuelmi_set_error("trajectory check: problem %d needs more than %d samples", b, FUELMI_TRAJCHK_MAX_SAMPLES);
  return FUELMI_ELIMIT;
}

}  // namespace

extern "C" int fuelmi_traj_check_plan(const fuelmi_trajchk_cfg* cfg, int out3[3]) {
  ARGCHK(out3);
  {
    const int rc = trajchk_cfg_check(cfg);
    if (rc) return rc;
  }
  out3[0] = TC_WIN, out3[1] = (int)tc_lds(cfg->max_ctrl), out3[2] = FUELMI_TRAJCHK_MAX_CTRL;
  return FUELMI_OK;
}

// the host route of both entries: io's splines uploaded, uniform (knot_span) or on given knots
static int trajchk_host(fuelmi_map* m, const fuelmi_trajchk_cfg* cfg, int n_prob, const TrajChkIO& io) {
  const int* n_ctrl = io.n_ctrl;
  const double *pos_ctrl = io.pos_ctrl, *knot_span = io.knot_span, *t_now = io.t_now;
  {  // every argument on the host, before the map is touched
    ARGCHK(n_prob <= 0 || n_ctrl);
    const int rc = trajchk_check(cfg, n_prob, io);
    if (rc) return rc;
  }
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const size_t n = (size_t)n_prob;
  TrajChkArgs T;
  memset(&T, 0, sizeof(T));
  ResultBlock R(16);
  trajchk_results(R, T, n_prob, io);
  ARGCHK(!R.overflow);
  const size_t ks = (size_t)cfg->max_ctrl + cfg->degree + 1;
  double *d_now, *d_knots = nullptr;
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 16);
    spline_src_take(L, n, cfg->max_ctrl, T.src);
    if (io.knots_given) d_knots = L.take<double>(n * ks);
    d_now = L.take<double>(n);
    R.place(L);
    return L.size();
  };
  {
    const int rc = m->trajchk_dev.carve(st, layout);
    if (rc) return rc;
  }
  {
    const int rc = spline_src_upload(st, T.src, n, cfg->max_ctrl, n_ctrl, pos_ctrl, knot_span);
    if (rc) return rc;
  }
  if (io.knots_given) {
    HIPCHK(hipMemcpyAsync(d_knots, io.knots, n * ks * sizeof(double), hipMemcpyHostToDevice, st));
    T.src.knots = d_knots, T.src.knots_stride = ks;
  }
  HIPCHK(hipMemcpyAsync(d_now, t_now, n * sizeof(double), hipMemcpyHostToDevice, st));
  T.cfg = *cfg;
  T.n_prob = n_prob;
  T.t_now = d_now;
  return trajchk_run(m, T, R, io);
}

extern "C" int fuelmi_map_check_trajs(fuelmi_map* m, const fuelmi_trajchk_cfg* cfg, int n_prob, const int* n_ctrl,
                                      const double* pos_ctrl, const double* knot_span, const double* t_now, int* status,
                                      int* safe, double* distance, int* n_samples, int* hit_index, double* hit_t,
                                      double* hit_pos, int* end_reason, double* duration) {
  const TrajChkIO io = {n_ctrl,    pos_ctrl,   knot_span, t_now, status,  safe,    n_samples,
                        hit_index, end_reason, distance,  hit_t, hit_pos, duration};
  return trajchk_host(m, cfg, n_prob, io);
}

// ... on whole knot vectors (fuelmi_map_adjust_trajs' knots_out as it stands) in place of the spans
extern "C" int fuelmi_map_check_trajs_knots(fuelmi_map* m, const fuelmi_trajchk_cfg* cfg, int n_prob, const int* n_ctrl,
                                            const double* pos_ctrl, const double* knots, const double* t_now, int* status,
                                            int* safe, double* distance, int* n_samples, int* hit_index, double* hit_t,
                                            double* hit_pos, int* end_reason, double* duration) {
  const TrajChkIO io = {n_ctrl,     pos_ctrl, nullptr, t_now,   status,   safe,  n_samples, hit_index,
                        end_reason, distance, hit_t,   hit_pos, duration, knots, true};
  return trajchk_host(m, cfg, n_prob, io);
}

// the safety check of a device batch's optimised position splines, read from the variables the last solve left on the
// device, against the batch's map; only the results travel
extern "C" int fuelmi_bspline_dev_check_trajs(fuelmi_bspline_dev* b, const fuelmi_trajchk_cfg* cfg, const double* t_now,
                                              int* status, int* safe, double* distance, int* n_samples, int* hit_index,
                                              double* hit_t, double* hit_pos, int* end_reason, double* duration) {
  ARGCHK(b && cfg);
  const BsplineArgs& A = b->a;
  ARGCHK(A.dim == 3 && b->opt_valid && b->opt_x);
  ARGCHK(cfg->degree == A.cfg.bspline_degree);
  fuelmi_trajchk_cfg tc = *cfg;
  tc.max_ctrl = A.N;
  const TrajChkIO io = {nullptr,   nullptr,    nullptr,  t_now, status,  safe,    n_samples,
                        hit_index, end_reason, distance, hit_t, hit_pos, duration};
  {
    const int rc = trajchk_check(&tc, A.C, io);
    if (rc) return rc;
  }
  fuelmi_map* m = b->map;
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  const size_t C = (size_t)A.C;
  TrajChkArgs T;
  memset(&T, 0, sizeof(T));
  ResultBlock R(16);
  trajchk_results(R, T, A.C, io);
  ARGCHK(!R.overflow);
  double* d_now;
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 16);
    d_now = L.take<double>(C);
    R.place(L);
    return L.size();
  };
  hipStream_t st = m->stream;
  {
    const int rc = b->chk_dev.carve(st, layout);
    if (rc) return rc;
  }
  HIPCHK(hipMemcpyAsync(d_now, t_now, C * sizeof(double), hipMemcpyHostToDevice, st));
  T.cfg = tc;
  T.n_prob = A.C;
  T.src = opt_spline_src_knots(b);
  T.t_now = d_now;
  return trajchk_run(m, T, R, io);
}
