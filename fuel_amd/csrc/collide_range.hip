// collide_range.hip -- the two links of FastPlannerManager::topoReplan's chain round the topological search
// (plan_manage/src/planner_manager.cpp), each for a batch on one map:
//   k_collide_range   findCollisionRange (:636-691): the initial local segment walked in 0.05 s ticks against the distance
//                     field -> colli_start / colli_end, t_s / t_e, start_pts / end_pts
//   k_guide_points    the head of optimizeTopoBspline (:553-577): seg_num, dt, the point count of reparamLocalTraj,
//                     pathToGuidePts and the degree's selection
//
// k_collide_range: one 64-lane wave per spline, CR_WAVES splines per workgroup (the packing of traj_check.hip).  A tick
// depends on its index alone -- its time is 0.05 added k times to t_m, its point, its verdict -- so the lanes take a window
// of 64 consecutive ticks: each lane repeats the window's additions up to its own tick (lane 63's value plus one addition
// is the next window's base), evaluates its point by the literal de Boor recursion and reads its voxel.  The events come
// from one ballot of the verdicts and the last_safe carried in from the window before; event k's row is the count of
// events in front of it.  `if (t_s < 0) t_s = tc - 0.05` is replayed over the window's start events in tick order (an
// unsafe tick 0 leaves -0.05, which the next start event overwrites).  start_pts / end_pts are a second short phase of
// the same launch: the same windows over the two accumulated loops of :670-690.  Knots are staged in LDS (one block per
// wave); control points are read from global memory through L2, as in traj_check.hip.
//
// The decision `getDistance(p) < clearance` is taken on k like the topological search's (path_internal.h field_cut): the
// host turns the clearance into the largest k the reference's STRICT f64 comparison accepts and hands the kernel an f32
// cut between the device's values for k and k + 1.
//
// k_guide_points: one wave per path.  Lane 0 builds discretizePath's prefix lengths in LDS in path order (their last
// entry is pathLength); every lane replays the integer and floating-point rules on the same values; then one lane per
// discretised point, in windows of 64.
//
// All f64, -ffp-contract=off.  A result does not depend on the problem's place in the batch.
#include <cmath>
#include <cstring>
#include <vector>

#include "bspline_batch.h"

namespace {

constexpr int CR_WIN = 64;   // ticks per window: one per lane
constexpr int CR_WAVES = 4;  // splines per workgroup
constexpr int CR_CAP = FUELMI_TRAJCHK_MAX_SAMPLES;  // ticks per spline, a multiple of CR_WIN
constexpr int GP_NT = 64;
constexpr int GP_PCAP = FUELMI_TOPO_MAX_PATH_POINTS;
constexpr int GP_CAP = FUELMI_GUIDE_MAX_PTS;

// k_collide_range: one spline per wave; every pointer addresses device memory
struct ColRangeArgs {
  fuelmi_colrange_cfg cfg;
  int n_prob;
  float cut;                // field_cut(res, clearance, strict)
  SplineSrc src;
  const float* dist;
  int *status, *n_ticks, *n_start_events, *n_end_events, *n_start_pts, *n_end_pts;
  double *t_s, *t_e;
  double *colli_start, *colli_end;  // [n][max_events][3]
  double *start_pts, *end_pts;      // [n][max_pts][3]
  double *first_start, *last_end;   // [n][3]
};

// k_guide_points: one path per workgroup
struct GuideArgs {
  int n_path, max_path_points, degree, max_guide;
  double ctrl_pt_dist;
  const double* paths;      // [n][max_path_points][3]
  const int* path_len;
  const double* duration;
  int *status, *seg_num, *n_pts, *n_ctrl, *n_guide;
  double* dt;
  double* guide_pts;        // [n][max_guide][3]
};

// a lane's value of an accumulated loop variable: `base` plus `lane` additions of `step`, one at a time; next = the
// value behind the window
__device__ __forceinline__ double cr_chain(double base, double step, int lane, double& next) {
  double acc = base, v = base;
  for (int j = 0; j < CR_WIN; ++j) {
    if (j == lane) v = acc;
    acc = acc + step;
  }
  next = acc;
  return v;
}

// evaluateDeBoor(tc): spline_pos is evaluateDeBoorT, which adds u[p] -- of a uniform spline double(0) * dt = 0.0, and
// tc + 0.0 is tc
__device__ __forceinline__ void cr_pos(const double* u, int p, int n, const double* C, double tc, double out[3]) {
  spline_pos(u, p, n, C, tc, out);
}

// evaluateCoarseEDT(q, -1.0) < clearance: getDistance(Vector3d) is posToIndex's floor and the voxel's value, -1 outside
// the map -- below every clearance >= 0.  The range test is made on the floor's f64 result (as in traj_check.hip: no
// cast of a value an int does not hold)
__device__ __forceinline__ bool cr_unsafe(const Geo& g, const float* __restrict__ dist, float cut, const double q[3]) {
  const double fx = floor((q[0] - g.org[0]) * g.res_inv), fy = floor((q[1] - g.org[1]) * g.res_inv),
               fz = floor((q[2] - g.org[2]) * g.res_inv);
  if (!(fx >= 0.0 && fy >= 0.0 && fz >= 0.0 && fx <= (double)(g.nx - 1) && fy <= (double)(g.ny - 1) &&
        fz <= (double)(g.nz - 1)))
    return true;
  return dist[(long)(int)fx * g.nyz + (long)(int)fy * g.nz + (int)fz] <= cut;
}

__device__ __forceinline__ int cr_prefix(unsigned long long live) {  // the lanes in front of the first one that is not live
  return ~live ? __builtin_ctzll(~live) : CR_WIN;
}

// for (tc = t0; tc <= lim; tc += step) out.push_back(evaluateDeBoor(tc)): the number of bodies (it stops counting behind
// CR_CAP), the first max_pts points written
__device__ int cr_points(const double* u, int p, int n, const double* C, double t0, double step, double lim, double* out,
                         int max_pts, int lane) {
  int count = 0;
  double base = t0;
  for (;;) {
    double next;
    const double tc = cr_chain(base, step, lane, next);
    const int nlive = cr_prefix(__ballot(tc <= lim));
    if (lane < nlive && count + lane < max_pts) {
      double q[3];
      cr_pos(u, p, n, C, tc, q);
      for (int c = 0; c < 3; ++c) out[3 * (size_t)(count + lane) + c] = q[c];
    }
    count += nlive;
    if (nlive < CR_WIN || count > CR_CAP) return count;
    base = next;
  }
}

__global__ void __launch_bounds__(CR_WIN * CR_WAVES) k_collide_range(Geo g, ColRangeArgs T) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x & (CR_WIN - 1), wv = threadIdx.x >> 6;
  const int b = blockIdx.x * CR_WAVES + wv;
  double* u = reinterpret_cast<double*>(smem_raw) + (size_t)wv * spline_knot_stride(T.cfg.max_ctrl);  // [n + p + 1]
  const int p = T.cfg.degree;
  const bool live_prob = b < T.n_prob;
  int n = 0;
  double dt = 0.0;
  if (live_prob) {
    n = spline_n(T.src, b);
    dt = spline_dt(T.src, b);
  }
  bool sane = live_prob && spline_sane(dt, n, p, T.cfg.max_ctrl);

  // 1. knots; every wave of the workgroup meets at the barrier, with or without a problem
  if (sane && lane == 0) spline_uniform_knots(u, p, n, dt);
  __syncthreads();
  if (!live_prob) return;
  const double* C = spline_ctrl(T.src, b);
  if (sane) {  // the last knot and every control point finite
    bool bad = !isfinite(u[n + p]);
    for (int i = lane; i < 3 * n; i += CR_WIN) bad = bad || !isfinite(C[i]);
    sane = __ballot(bad) == 0ull;
  }
  if (!sane) {  // (the other outputs were zeroed in front of the launch)
    if (lane == 0) T.status[b] = FUELMI_COLRANGE_NONFINITE;
    return;
  }
  const int max_ev = T.cfg.max_events, max_pts = T.cfg.max_pts;
  double* cs = T.colli_start + (size_t)b * max_ev * 3;
  double* ce = T.colli_end + (size_t)b * max_ev * 3;
  const double t_m = u[p], t_mp = u[n];  // getTimeSpan: u_(p_), u_(m_ - p_)

  // 2. the ticks, CR_WIN a window
  int n_ticks = 0, n_s = 0, n_e = 0;
  double t_s = -1.0, t_e = 0.0;
  double last_end[3] = {0.0, 0.0, 0.0};
  bool last_safe = true, over_ticks = false;
  double base = t_m;
  for (int kb = 0;; kb += CR_WIN) {
    double next;
    const double tc = cr_chain(base, 0.05, lane, next);
    const int nlive = cr_prefix(__ballot(tc <= t_mp + 1e-4));
    const bool live = lane < nlive;
    double q[3] = {0.0, 0.0, 0.0};
    bool unsafe = false;
    if (live) {
      cr_pos(u, p, n, C, tc, q);
      unsafe = cr_unsafe(g, T.dist, T.cut, q);
    }
    const unsigned long long m_live = nlive == CR_WIN ? ~0ull : (1ull << nlive) - 1ull;
    const unsigned long long m_unsafe = __ballot(live && unsafe);
    const unsigned long long m_safe = ~m_unsafe & m_live;
    const unsigned long long prev_safe = (m_safe << 1) | (last_safe ? 1ull : 0ull);  // last_safe as each tick meets it
    const unsigned long long m_start = prev_safe & m_unsafe, m_end = ~prev_safe & m_safe;
    const unsigned long long below = (1ull << lane) - 1ull;
    const double tb = tc - 0.05;  // recomputed from this tick's tc, not the tick before
    if ((m_start >> lane) & 1ull) {
      const int slot = n_s + __popcll(m_start & below);
      if (slot < max_ev) {
        double s[3];
        cr_pos(u, p, n, C, tb, s);
        for (int c = 0; c < 3; ++c) cs[3 * (size_t)slot + c] = s[c];
        if (slot == 0)
          for (int c = 0; c < 3; ++c) T.first_start[3 * (size_t)b + c] = s[c];
      }
    }
    if ((m_end >> lane) & 1ull) {
      const int slot = n_e + __popcll(m_end & below);
      if (slot < max_ev)
        for (int c = 0; c < 3; ++c) ce[3 * (size_t)slot + c] = q[c];
    }
    for (unsigned long long mm = m_start; t_s < 0.0 && mm; mm &= mm - 1ull) t_s = __shfl(tb, __builtin_ctzll(mm));
    if (m_end) {
      const int l = 63 - __builtin_clzll(m_end);
      t_e = __shfl(tc, l);
      for (int c = 0; c < 3; ++c) last_end[c] = __shfl(q[c], l);
    }
    n_s += __popcll(m_start), n_e += __popcll(m_end), n_ticks += nlive;
    if (nlive < CR_WIN) break;
    if (kb + CR_WIN >= CR_CAP) {  // tick CR_CAP would be one too many
      over_ticks = next <= t_mp + 1e-4;
      break;
    }
    last_safe = (m_safe >> (CR_WIN - 1)) & 1ull;
    base = next;
  }

  // 3. the status; start_pts and end_pts (:665-690)
  int status, n_sp = 0, n_ep = 0;
  if (over_ticks)
    status = -1;
  else if (n_s == 0)
    status = FUELMI_COLRANGE_NO_COLLISION;
  else if (n_s == 1 && n_e == 0)
    status = FUELMI_COLRANGE_ENDS_IN_OBSTACLE;
  else {
    status = FUELMI_COLRANGE_OK;
    int sn = (int)ceil((t_s - t_m) / dt);
    double step = (t_s - t_m) / sn;  // sn = 0: NaN (one point) or -inf (none)
    n_sp = cr_points(u, p, n, C, t_m, step, t_s + 1e-4, T.start_pts + (size_t)b * max_pts * 3, max_pts, lane);
    sn = (int)ceil((t_mp - t_e) / dt);
    step = (t_mp - t_e) / sn;
    if (step > 1e-4) {
      n_ep = cr_points(u, p, n, C, t_e, step, t_mp + 1e-4, T.end_pts + (size_t)b * max_pts * 3, max_pts, lane);
    } else {
      n_ep = 1;
      if (lane == 0) {
        double q[3];
        cr_pos(u, p, n, C, t_mp, q);
        for (int c = 0; c < 3; ++c) T.end_pts[((size_t)b * max_pts) * 3 + c] = q[c];
      }
    }
    if (n_s > max_ev || n_e > max_ev || n_sp > max_pts || n_ep > max_pts) status = -1;
  }
  if (lane == 0) {
    T.status[b] = status;
    T.n_ticks[b] = n_ticks, T.n_start_events[b] = n_s, T.n_end_events[b] = n_e;
    T.n_start_pts[b] = n_sp, T.n_end_pts[b] = n_ep;
    T.t_s[b] = t_s, T.t_e[b] = t_e;
    for (int c = 0; c < 3; ++c) T.last_end[3 * (size_t)b + c] = last_end[c];
  }
}

__global__ void __launch_bounds__(GP_NT) k_guide_points(GuideArgs G) {
  __shared__ double len[GP_PCAP];  // discretizePath's len_list
  const int lane = threadIdx.x, b = blockIdx.x;
  const int n = G.path_len[b];
  const double* path = G.paths + (size_t)b * G.max_path_points * 3;
  int status = FUELMI_TOPO_OK, seg_num = 0, n_pts = 0, n_ctrl = 0, n_guide = 0;
  double dt = 0.0;
  if (n < 2) {
    status = FUELMI_TOPO_UNDEFINED;  // discretizePath finds no segment
  } else {
    if (lane == 0) path_prefix_lengths(path, n, len);
    __syncthreads();  // (n is the workgroup's)
    const double q = len[n - 1] / G.ctrl_pt_dist;  // pathLength(guide_path) / pp_.ctrl_pt_dist
    if (!isfinite(q)) {
      status = FUELMI_TOPO_UNDEFINED;  // the cast to int
    } else if (!(q < (double)GP_CAP + 1.0)) {
      status = -1;
    } else {
      seg_num = (int)q;
      seg_num = seg_num < 6 ? 6 : seg_num;
      const double duration = G.duration[b];
      dt = duration / double(seg_num);
      bool over = false;
      for (double tp = 0.0; tp <= duration + 1e-4; tp += dt) {  // getTrajInfoInDuration's bodies
        if (n_pts == GP_CAP) {
          over = true;
          break;
        }
        ++n_pts;
      }
      if (over) {
        status = -1;
      } else {
        n_ctrl = n_pts + 2;  // parameterizeToBspline: K + 2 rows
        const int pt_num = G.degree == 4 ? 2 * n_ctrl - 7 : n_ctrl - 2;
        bool miss = pt_num < 2;
        double o[3];
        for (int i = lane; i < pt_num; i += GP_NT) miss = miss || !path_disc_point(path, n, len, pt_num, i, o);
        if (__ballot(miss) != 0ull) {
          status = FUELMI_TOPO_UNDEFINED;
        } else {
          n_guide = G.degree == 4 ? n_ctrl - 8 : n_ctrl - 6;
          if (n_guide < 0) n_guide = 0;
          double* out = G.guide_pts + (size_t)b * G.max_guide * 3;
          for (int i = lane; i < pt_num; i += GP_NT) {
            int gi;
            if (G.degree == 4) {  // i % 2 == 1 && i >= 5 && i <= size - 6
              if (!(i % 2 == 1 && i >= 5 && i <= pt_num - 6)) continue;
              gi = (i - 5) / 2;
            } else {              // tmp_pts.begin() + 2 .. tmp_pts.end() - 2
              if (!(i >= 2 && i < pt_num - 2)) continue;
              gi = i - 2;
            }
            if (gi >= G.max_guide) continue;
            path_disc_point(path, n, len, pt_num, i, o);
            for (int c = 0; c < 3; ++c) out[3 * (size_t)gi + c] = o[c];
          }
          if (n_guide > G.max_guide) status = -1;
        }
      }
    }
  }
  if (lane == 0) {
    G.status[b] = status;
    G.seg_num[b] = seg_num, G.n_pts[b] = n_pts, G.n_ctrl[b] = n_ctrl, G.n_guide[b] = n_guide;
    G.dt[b] = dt;
  }
}

size_t cr_lds(int max_ctrl) { return (size_t)CR_WAVES * spline_knot_stride(max_ctrl) * sizeof(double); }

int colrange_cfg_check(const fuelmi_colrange_cfg* cfg) {
  ARGCHK(cfg);
  ARGCHK(cfg->degree >= 3 && cfg->degree <= 5);
  ARGCHK(cfg->max_ctrl >= cfg->degree + 1);
  ARGCHK(std::isfinite(cfg->clearance) && cfg->clearance >= 0.0);
  ARGCHK(cfg->max_events >= 1 && cfg->max_pts >= 1);
  if (cfg->max_ctrl > FUELMI_TRAJCHK_MAX_CTRL || cfg->max_events > FUELMI_COLRANGE_MAX_EVENTS ||
      cfg->max_pts > FUELMI_TOPO_MAX_POINTS_IN) {
    fuelmi_set_error("collision ranges: max_ctrl %d / max_events %d / max_pts %d exceed %d / %d / %d", cfg->max_ctrl,
                     cfg->max_events, cfg->max_pts, FUELMI_TRAJCHK_MAX_CTRL, FUELMI_COLRANGE_MAX_EVENTS,
                     FUELMI_TOPO_MAX_POINTS_IN);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

}  // namespace

extern "C" int fuelmi_colrange_plan(const fuelmi_colrange_cfg* cfg, int out6[6]) {
  ARGCHK(out6);
  {
    const int rc = colrange_cfg_check(cfg);
    if (rc) return rc;
  }
  out6[0] = CR_WIN, out6[1] = (int)cr_lds(cfg->max_ctrl), out6[2] = CR_WAVES, out6[3] = CR_CAP;
  out6[4] = FUELMI_TRAJCHK_MAX_CTRL, out6[5] = FUELMI_TOPO_MAX_POINTS_IN;
  return FUELMI_OK;
}

extern "C" int fuelmi_map_collision_ranges(fuelmi_map* m, const fuelmi_colrange_cfg* cfg, int n_prob, const int* n_ctrl,
                                           const double* pos_ctrl, const double* knot_span, int* status, int* n_ticks,
                                           int* n_start_events, int* n_end_events, double* t_s, double* t_e,
                                           double* colli_start, double* colli_end, int* n_start_pts, double* start_pts,
                                           int* n_end_pts, double* end_pts, double* first_start, double* last_end) {
  {  // every argument on the host, before the map is touched
    const int rc = colrange_cfg_check(cfg);
    if (rc) return rc;
  }
  ARGCHK(n_prob >= 0);
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(n_ctrl && pos_ctrl && knot_span);
  ARGCHK(status && n_ticks && n_start_events && n_end_events && t_s && t_e && colli_start && colli_end && n_start_pts &&
         start_pts && n_end_pts && end_pts && first_start && last_end);
  for (int b = 0; b < n_prob; ++b) {
    ARGCHK(n_ctrl[b] >= cfg->degree + 1 && n_ctrl[b] <= cfg->max_ctrl);
    ARGCHK(!(knot_span[b] <= 0.0));  // (a span that is not finite is the kernel's FUELMI_COLRANGE_NONFINITE)
    const double* P = pos_ctrl + (size_t)b * cfg->max_ctrl * 3;
    for (int k = 0; k < 3 * n_ctrl[b]; ++k) ARGCHK(!std::isfinite(P[k]) || std::fabs(P[k]) < 1e7);
  }
  ARGCHK(m);
  ARGCHK(m->dist);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const size_t n = (size_t)n_prob, ev = (size_t)cfg->max_events, mp = (size_t)cfg->max_pts;
  ColRangeArgs T;
  memset(&T, 0, sizeof(T));
  ResultBlock R(16);
  R.add(T.status, status, n);
  R.add(T.n_ticks, n_ticks, n);
  R.add(T.n_start_events, n_start_events, n);
  R.add(T.n_end_events, n_end_events, n);
  R.add(T.n_start_pts, n_start_pts, n);
  R.add(T.n_end_pts, n_end_pts, n);
  R.add(T.t_s, t_s, n);
  R.add(T.t_e, t_e, n);
  R.add(T.colli_start, colli_start, n * ev * 3);
  R.add(T.colli_end, colli_end, n * ev * 3);
  R.add(T.start_pts, start_pts, n * mp * 3);
  R.add(T.end_pts, end_pts, n * mp * 3);
  R.add(T.first_start, first_start, n * 3);
  R.add(T.last_end, last_end, n * 3);
  ARGCHK(!R.overflow);
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 16);
    spline_src_take(L, n, cfg->max_ctrl, T.src);
    R.place(L);
    return L.size();
  };
  {
    const int rc = m->colrange_dev.carve(st, layout);
    if (rc) return rc;
  }
  {
    const int rc = spline_src_upload(st, T.src, n, cfg->max_ctrl, n_ctrl, pos_ctrl, knot_span);
    if (rc) return rc;
  }
  HIPCHK(hipMemsetAsync(R.base, 0, R.size(), st));
  T.cfg = *cfg;
  T.n_prob = n_prob;
  T.cut = field_cut(m->g.res, cfg->clearance, true);
  T.dist = m->dist;
  hipLaunchKernelGGL(k_collide_range, dim3((n_prob + CR_WAVES - 1) / CR_WAVES), dim3(CR_WIN * CR_WAVES),
                     cr_lds(cfg->max_ctrl), st, m->g, T);
  HIPCHK(hipGetLastError());
  {
    const int rc = result_fetch(R, st);
    if (rc) return rc;
  }
  const int b = first_over_limit(status, n_prob);
  if (b < 0) return FUELMI_OK;
  fuelmi_set_error("collision ranges: problem %d is over max_events = %d / max_pts = %d or %d ticks", b,
                   cfg->max_events, cfg->max_pts, CR_CAP);
  return FUELMI_ELIMIT;
}

extern "C" int fuelmi_map_guide_points(fuelmi_map* m, int n_path, int max_path_points, const double* paths,
                                       const int* path_len, const double* duration, double ctrl_pt_dist, int degree,
                                       int max_guide, int* status, int* seg_num, double* dt, int* n_pts, int* n_ctrl,
                                       int* n_guide, double* guide_pts) {
  ARGCHK(degree >= 3 && degree <= 5);
  ARGCHK(std::isfinite(ctrl_pt_dist) && ctrl_pt_dist > 0.0);
  ARGCHK(n_path >= 0 && max_path_points >= 1 && max_guide >= 1);
  if (max_path_points > FUELMI_TOPO_MAX_PATH_POINTS || max_guide > FUELMI_GUIDE_MAX_PTS) {
    fuelmi_set_error("guide points: max_path_points %d / max_guide %d exceed %d / %d", max_path_points, max_guide,
                     FUELMI_TOPO_MAX_PATH_POINTS, FUELMI_GUIDE_MAX_PTS);
    return FUELMI_ELIMIT;
  }
  if (n_path == 0) return FUELMI_OK;
  ARGCHK(paths && path_len && duration);
  ARGCHK(status && seg_num && dt && n_pts && n_ctrl && n_guide && guide_pts);
  for (int b = 0; b < n_path; ++b) {
    ARGCHK(path_len[b] >= 0 && path_len[b] <= max_path_points);
    ARGCHK(std::isfinite(duration[b]) && duration[b] > 0.0);
  }
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const size_t n = (size_t)n_path, mpp = (size_t)max_path_points;
  GuideArgs G;
  memset(&G, 0, sizeof(G));
  ResultBlock R(16);
  R.add(G.status, status, n);
  R.add(G.seg_num, seg_num, n);
  R.add(G.n_pts, n_pts, n);
  R.add(G.n_ctrl, n_ctrl, n);
  R.add(G.n_guide, n_guide, n);
  R.add(G.dt, dt, n);
  R.add(G.guide_pts, guide_pts, n * (size_t)max_guide * 3);
  ARGCHK(!R.overflow);
  double *d_paths, *d_dur;
  int* d_len;
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 16);
    d_paths = L.take<double>(n * mpp * 3);
    d_dur = L.take<double>(n);
    d_len = L.take<int>(n);
    R.place(L);
    return L.size();
  };
  {
    const int rc = m->colrange_dev.carve(st, layout);
    if (rc) return rc;
  }
  HIPCHK(hipMemcpyAsync(d_paths, paths, n * mpp * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_dur, duration, n * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_len, path_len, n * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(R.base, 0, R.size(), st));
  G.n_path = n_path, G.max_path_points = max_path_points, G.degree = degree, G.max_guide = max_guide;
  G.ctrl_pt_dist = ctrl_pt_dist;
  G.paths = d_paths, G.path_len = d_len, G.duration = d_dur;
  hipLaunchKernelGGL(k_guide_points, dim3(n_path), dim3(GP_NT), 0, st, G);
  HIPCHK(hipGetLastError());
  {
    const int rc = result_fetch(R, st);
    if (rc) return rc;
  }
  const int b = first_over_limit(status, n_path);
  if (b < 0) return FUELMI_OK;
  fuelmi_set_error("guide points: path %d is over max_guide = %d or %d points", b, max_guide, FUELMI_GUIDE_MAX_PTS);
  return FUELMI_ELIMIT;
}
