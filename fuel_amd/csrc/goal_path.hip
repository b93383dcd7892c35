// goal_path.hip -- the geometric path to the next viewpoint: FastExplorationManager::planExploreMotion's
// Astar::search + shortenPath + length branch (exploration_manager/src/fast_exploration_manager.cpp:234-276, 295-325)
// for a batch of (start, goal) problems.
//
// The raw paths come from the path engine (path_cost_enqueue with always_lattice: one lattice run for the whole batch,
// sources shared bitwise) and stay in its scratch; k_goal_shorten turns them into way-points, length, branch and next
// goal.  shortenPath's loop only looks sequential: short.back() changes when a point is pushed and at no other time,
// so for a fixed anchor a the test
//     push(i) = |path[i] - a| > shorten_dist  ||  !ray_clear<false>(a, path[i + 1])
// does not depend on the other candidates, and the loop pushes exactly the FIRST i behind the anchor for which it
// holds.  One 64-lane wave per problem: the lanes take GS_WIN consecutive candidates, each walks its own ray, a
// ballot picks the first push (the new anchor) or the window moves on with the anchor kept.  The tail rule, the
// mid-point, the running pathLength, the branch and the truncation mark are a few f64 operations every lane repeats;
// lane 0 stores.  Path points are read from global memory (L2): a raw path may hold thousands of points (24 B each,
// past the LDS of a workgroup at fine lattices) and a window reads each of its points twice, so staging saves nothing.
#include <cmath>
#include <vector>

#include "frontier_internal.h"

namespace {

constexpr int GS_WIN = 64;   // candidates per window: one per lane
constexpr int GS_WAVES = 4;  // problems per workgroup
constexpr int GOAL_RAW_OVER = -1, GOAL_BROKEN = -2;  // status of a raw path past max_path_points / without a chain

struct SArgs {
  int n;
  const int* kind;     // engine results: 1 lattice path, 2 no goal reachable, < 0 broken
  const int* plen;
  const double* path;  // [n][maxp][3]
  const double* p2;    // [n][3] the goals
  int maxp;
  const u64* infl;
  const u64* unk;
  double shorten_dist, end_eps, radius_close, radius_far;
  int maxw;
  int* status;
  int* n_way;
  int* raw_len;
  double* length;
  double* way;         // [n][maxw][3]
  double* next_goal;   // [n][3]
};

__device__ __forceinline__ double dist3(const double a[3], const double b[3]) {
  const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
  return sqrt(x * x + y * y + z * z);
}

__global__ void __launch_bounds__(GS_WIN * GS_WAVES) k_goal_shorten(Geo g, SArgs S) {
  const int lane = threadIdx.x & (GS_WIN - 1);
  const int b = blockIdx.x * GS_WAVES + (threadIdx.x >> 6);
  if (b >= S.n) return;
  const int kind = S.kind[b], n = S.plen[b];
  const double goal[3] = {S.p2[3 * b], S.p2[3 * b + 1], S.p2[3 * b + 2]};
  if (kind != 1 || n > S.maxp) {
    if (lane == 0) {
      S.status[b] = kind == 2 ? FUELMI_GOAL_NO_PATH : (kind == 1 ? GOAL_RAW_OVER : GOAL_BROKEN);
      S.raw_len[b] = kind == 1 ? n : 0;
      S.n_way[b] = 0;
      S.length[b] = 0.0;
      for (int k = 0; k < 3; ++k) S.next_goal[3 * b + k] = goal[k];
    }
    return;
  }
  const double* P = S.path + (size_t)b * S.maxp * 3;
  double* W = S.way + (size_t)b * S.maxw * 3;
  const double s0[3] = {P[0], P[1], P[2]};
  double a[3] = {s0[0], s0[1], s0[2]};  // short.back()
  int nw = 1;                           // short.size()
  double len = 0.0;                     // Astar::pathLength of short so far: the truncation loop's len2 as well
  int ntr = 0;                          // trunc.size() once len2 >= radius_far
  double tg[3] = {0.0, 0.0, 0.0};       // trunc.back()
  if (lane == 0)
    for (int k = 0; k < 3; ++k) W[k] = s0[k];
  auto push = [&](const double q[3]) {  // short.push_back(q)
    len += dist3(q, a);
    if (lane == 0 && nw < S.maxw)
      for (int k = 0; k < 3; ++k) W[3 * nw + k] = q[k];
    ++nw;
    for (int k = 0; k < 3; ++k) a[k] = q[k];
    if (!ntr && len >= S.radius_far) {
      ntr = nw;
      for (int k = 0; k < 3; ++k) tg[k] = q[k];
    }
  };
  // :303-318 -- candidates i = 1 .. n - 2, a window of GS_WIN behind the last push at a time
  for (int i0 = 1; i0 <= n - 2;) {
    const int i = i0 + lane;
    bool p = false;
    if (i <= n - 2) {
      const double q[3] = {P[3 * i], P[3 * i + 1], P[3 * i + 2]};
      p = dist3(q, a) > S.shorten_dist;
      if (!p) {
        const double e[3] = {P[3 * i + 3], P[3 * i + 4], P[3 * i + 5]};
        p = !ray_clear<false>(g, S.infl, S.unk, nullptr, nullptr, a, e);
      }
    }
    const unsigned long long m = __ballot(p);
    if (m) {
      const int f = i0 + __builtin_ctzll(m);
      const double q[3] = {P[3 * f], P[3 * f + 1], P[3 * f + 2]};
      push(q);
      i0 = f + 1;
    } else {
      i0 += GS_WIN;
    }
  }
  const double last[3] = {P[3 * (n - 1)], P[3 * (n - 1) + 1], P[3 * (n - 1) + 2]};
  if (dist3(last, a) > S.end_eps) push(last);  // :319
  if (nw == 2) {                               // :322-323
    const double s1[3] = {a[0], a[1], a[2]};
    const double mid[3] = {0.5 * (s0[0] + s1[0]), 0.5 * (s0[1] + s1[1]), 0.5 * (s0[2] + s1[2])};
    nw = 1, len = 0.0, ntr = 0;
    for (int k = 0; k < 3; ++k) a[k] = s0[k];
    push(mid);
    push(s1);
  }
  if (lane != 0) return;
  int status = FUELMI_GOAL_MID, cnt = nw;
  const double* ng = goal;
  if (len < S.radius_close) {
    status = FUELMI_GOAL_CLOSE;
  } else if (len > S.radius_far) {  // :251-263; ntr > 0: the last partial sum is len itself
    status = FUELMI_GOAL_FAR;
    cnt = ntr;
    ng = tg;
  }
  S.status[b] = status;
  S.raw_len[b] = n;
  S.n_way[b] = cnt;
  S.length[b] = len;
  for (int k = 0; k < 3; ++k) S.next_goal[3 * b + k] = ng[k];
}

bool pos_fin(double x) { return std::isfinite(x) && x > 0.0; }

}  // namespace

void goal_path_release(fuelmi_map* m) {
  for (hipEvent_t& e : m->goal_ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

extern "C" int fuelmi_map_goal_paths(fuelmi_map* m, const fuelmi_goal_cfg* cfg, int n_prob, const double* start_xyz,
                                     const double* goal_xyz, int* status, double* length, int* n_way, double* way_xyz,
                                     double* next_goal, int* raw_len, double* raw_xyz) {
  // every argument on the host, before the map is touched
  ARGCHK(cfg);
  ARGCHK(n_prob >= 0);
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(start_xyz && goal_xyz && status && length && n_way && way_xyz && next_goal);
  const fuelmi_path_cfg& pc = cfg->path;
  ARGCHK(pos_fin(pc.lattice_res) && pos_fin(pc.edge_step));
  ARGCHK(pos_fin(cfg->shorten_dist) && pos_fin(cfg->radius_close) && pos_fin(cfg->radius_far));
  ARGCHK(std::isfinite(cfg->end_eps) && cfg->end_eps >= 0.0);
  ARGCHK(pc.max_path_points >= 2 && cfg->max_way_points >= 1);
  for (long k = 0; k < 3L * n_prob; ++k) ARGCHK(std::fabs(start_xyz[k]) < 1e7 && std::fabs(goal_xyz[k]) < 1e7);
  ARGCHK(m);

  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  for (hipEvent_t& e : m->goal_ev)
    if (!e) HIPCHK(hipEventCreate(&e));
  const int maxp = pc.max_path_points, maxw = cfg->max_way_points;
  const size_t n = (size_t)n_prob;
  SArgs S;
  auto layout = [&](unsigned char* base) {  // the result block
    BlockLayout L(base, 256);
    S.status = L.take<int>(n);
    S.n_way = L.take<int>(n);
    S.raw_len = L.take<int>(n);
    S.length = L.take<double>(n);
    S.next_goal = L.take<double>(3 * n);
    S.way = L.take<double>(3 * n * maxw);
    return L.size();
  };
  int rc = m->goal_dev.reserve(st, layout(nullptr));
  if (rc != FUELMI_OK) return rc;
  for (int& v : m->path_stats) v = 0;
  HIPCHK(hipEventRecord(m->goal_ev[0], st));
  PathRun run;
  rc = path_cost_enqueue(m, &pc, n_prob, start_xyz, goal_xyz, maxp, run, true);
  if (rc != FUELMI_OK) return rc;
  HIPCHK(hipEventRecord(m->goal_ev[1], st));

  layout(m->goal_dev.base());
  S.n = n_prob;
  S.kind = run.kind;
  S.plen = run.plen;
  S.path = run.path;
  S.p2 = run.p2;
  S.maxp = maxp;
  S.infl = m->infl_bits.p;
  S.unk = m->unk_bits.p;
  S.shorten_dist = cfg->shorten_dist, S.end_eps = cfg->end_eps;
  S.radius_close = cfg->radius_close, S.radius_far = cfg->radius_far;
  S.maxw = maxw;
  hipLaunchKernelGGL(k_goal_shorten, dim3((n_prob + GS_WAVES - 1) / GS_WAVES), dim3(GS_WIN * GS_WAVES), 0, st, m->g, S);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(m->goal_ev[2], st));
  std::vector<int> rl(n);
  HIPCHK(hipMemcpyAsync(status, S.status, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(n_way, S.n_way, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(rl.data(), S.raw_len, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(length, S.length, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(next_goal, S.next_goal, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(way_xyz, S.way, sizeof(double) * 3 * n * maxw, hipMemcpyDeviceToHost, st));
  if (raw_xyz) HIPCHK(hipMemcpyAsync(raw_xyz, run.path, sizeof(double) * 3 * n * maxp, hipMemcpyDeviceToHost, st));
  HIPCHK(stream_wait(st));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, m->goal_ev[0], m->goal_ev[1]));
  m->goal_ms[0] = ms;
  HIPCHK(hipEventElapsedTime(&ms, m->goal_ev[1], m->goal_ev[2]));
  m->goal_ms[1] = ms;
  bool over_raw = false, over_way = false;
  for (int b = 0; b < n_prob; ++b) {
    if (raw_len) raw_len[b] = rl[b];
    if (status[b] == GOAL_BROKEN) {
      fuelmi_set_error("goal paths: problem %d found no predecessor chain back to its start", b);
      return FUELMI_EHIP;
    }
    if (status[b] == GOAL_RAW_OVER) over_raw = true;
    if (n_way[b] > maxw) over_way = true;
  }
  if (over_raw) {
    fuelmi_set_error("goal paths: a raw path has more than max_path_points = %d points (raw_len holds each count)", maxp);
    return FUELMI_ELIMIT;
  }
  if (over_way) {
    fuelmi_set_error("goal paths: a problem has more than max_way_points = %d way-points (n_way holds each count)", maxw);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

extern "C" int fuelmi_map_goal_path_times(const fuelmi_map* m, double ms2[2]) {
  ARGCHK(m && ms2);
  ms2[0] = m->goal_ms[0], ms2[1] = m->goal_ms[1];
  return FUELMI_OK;
}
