// kino_path.hip -- the kinodynamic search of the mid-range goal branch: KinodynamicAstar::search + getSamples
// (path_searching/src/kinodynamic_astar.cpp:15-263, 543-634) as FastPlannerManager::kinodynamicReplan calls them
// (plan_manage/src/planner_manager.cpp:124-164) for a batch of problems: static mode, init = true, after NO_PATH one
// retry with init = false inside the same launch.
//
// One workgroup of KN_NT lanes per problem.  A pop is a chain of dependent steps, so a single search is latency bound;
// what runs side by side is (a) the primitives of one expansion, one lane each: stateTransit, the box / closed /
// velocity / same-voxel tests, the check_num safety samples, g, estimateHeuristic (a quartic through a cubic: the
// costly part of an expansion) and f, and (b) the problems of the batch.  The reference's bookkeeping depends on the
// order of its double loop (a sibling of this expansion is compared by f, an older open node by g, both rewritten in
// place without repairing the heap; the pool may run out in the middle), so lane 0 REPLAYS the surviving lanes in loop
// order.  The replay needs no search of its own: every lane looked its voxel up in the hash BEFORE the expansion
// changed anything (nothing but new, open nodes can appear during it), and a lane without a node finds the first
// earlier surviving lane with the same voxel by scanning LDS -- that lane created the sibling it is compared with.
//
// The open set is libstdc++'s heap (std::priority_queue<PathNodePtr, vector, NodeComparator>): kn_push is push_heap's
// __push_heap, kn_pop is pop_heap's __adjust_heap (hole to a leaf along the preferred children, then __push_heap), the
// comparator reads the nodes' CURRENT f, which an in-place update may have changed behind the heap's back.
//
// Workspace per problem, in the map's kino_dev pool (a DevScratch, carved by a BlockLayout): allocate_num node records
// of 128 B, the heap (4 B a node), an open-addressing hash on the voxel triple (linear probing, >= 2 allocate_num slots
// of 4 B holding node numbers, -1 = empty; cleared by a memset on the stream per call and by the workgroup itself before
// the retry).
//
// All f64, -ffp-contract=off, no scratch (no dynamically indexed private arrays).  LDS: the lanes' results of one
// expansion (fuelmi_kino_plan reports the bytes).
// Behind the kernel, the two entries that share its lists, checks, workspace and launch: fuelmi_map_kino_paths (all to
// the host) and fuelmi_bspline_dev_load_kino (samples straight into a device batch's fit, bspline_batch.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "bspline_batch.h"

namespace {

constexpr int KN_NT = 256;
constexpr int KN_DEAD = -2, KN_NEW = -1;  // a lane's verdict: pruned / no node in its voxel yet / >= 0: that open node
constexpr int KN_OPEN = 1, KN_CLOSED = 2;
constexpr int KN_EXPAND = 0;              // lane 0's decision at the top of a pop; otherwise the search's status

// k_kino_path: one problem per workgroup; every pointer addresses device memory
struct KinoArgs {
  fuelmi_kino_cfg cfg;
  int n_prob;
  int n_init, n_reg;        // primitives of the two lists
  const double* prims;      // [n_init + n_reg][4]: input, tau (the init list's input is the problem's start_acc)
  int tolerance;            // ceil(1 / resolution)
  double inv_res;           // 1.0 / resolution
  double box_mind[3], box_maxd[3], map_size[3];
  const u64* infl;
  const u64* unk;
  const double* in;         // [n][5][3]: start, start_vel, start_acc, goal, goal_vel
  unsigned char* pool;      // [n][allocate_num] node records
  int* heap;                // [n][allocate_num]
  int* hash;                // [n][hash_cap], -1 = empty
  int hash_cap;             // a power of two >= 2 allocate_num
  int load_points;          // > 0: the batch route, a path must give exactly this many samples
  int* status;
  int* which;
  int* iter_num;
  int* use_node_num;
  int* n_nodes;
  int* shot;
  int* seg_num;
  int* n_samples;
  int* skip;                // [n] 0: ts / samples / derivs hold a path, 1: they do not (the fit leaves the candidate)
  double* t_shot;
  double* coef_shot;        // [n][3][4]
  double* T_sum;
  double* ts_out;
  double* samples;          // [n][max_samples][3]
  double* derivs;           // [n][4][3]
  double* node_state;       // [n][max_path_nodes][6] or null
  double* node_input;       // [n][max_path_nodes][3] or null
  double* node_duration;    // [n][max_path_nodes] or null
};

struct alignas(16) KNode {
  double st[6];
  double g, f;
  double in[3];
  double dur;
  int idx[3];
  int parent;
  int state;
  int pad[3];
};
static_assert(sizeof(KNode) == 128, "the node record the workspace figures are stated for");

struct KShared {
  double st[6][KN_NT];
  double g[KN_NT], f[KN_NT];
  int vx[KN_NT], vy[KN_NT], vz[KN_NT];
  int kind[KN_NT], first[KN_NT], made[KN_NT];
  double coef[12];
  double t_shot;
  int action, cur, init, hn, use, iter, shot;
};

// stateTransit (:657-668): phi * state0 + integral; phi is the identity with tau at (i, i + 3), so a row has two
// non-zero terms; pow(tau, 2) is tau * tau (the compiler's own folding)
__device__ __forceinline__ void kn_transit(const double s[6], const double u[3], double tau, double o[6]) {
  const double h = 0.5 * (tau * tau);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = (s[k] + tau * s[k + 3]) + h * u[k];
    o[k + 3] = s[k + 3] + tau * u[k];
  }
}

// cubic (:396-423): only its first root is used
__device__ double kn_cubic_front(double a, double b, double c, double d) {
  const double a2 = b / a, a1 = c / a, a0 = d / a;
  const double Q = (3 * a1 - a2 * a2) / 9;
  const double R = (9 * a1 * a2 - 27 * a0 - 2 * a2 * a2 * a2) / 54;
  const double D = Q * Q * Q + R * R;
  if (D > 0) {
    const double S = cbrt(R + sqrt(D));
    const double T = cbrt(R - sqrt(D));
    return -a2 / 3 + (S + T);
  } else if (D == 0) {
    const double S = cbrt(R);
    return -a2 / 3 + S + S;
  }
  const double theta = acos(R / sqrt(-Q * Q * Q));
  return 2 * sqrt(-Q) * cos(theta / 3) - a2 / 3;
}

// estimateHeuristic (:296-329): quartic(w_time, 0, c3, c2, c1) (:425-458), its roots and t_bar in push order
__device__ double kn_heuristic(const double x1[6], const double x2[6], double w_time, double max_vel, double& opt_t) {
  const double dp[3] = {x2[0] - x1[0], x2[1] - x1[1], x2[2] - x1[2]};
  const double* v0 = x1 + 3;
  const double* v1 = x2 + 3;
  const double c1 = -36 * (dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]);
  const double c2 = 24 * ((v0[0] + v1[0]) * dp[0] + (v0[1] + v1[1]) * dp[1] + (v0[2] + v1[2]) * dp[2]);
  const double c3 = -4 * ((v0[0] * v0[0] + v0[1] * v0[1] + v0[2] * v0[2]) + (v0[0] * v1[0] + v0[1] * v1[1] + v0[2] * v1[2]) +
                          (v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]));
  const double v_max = max_vel * 0.5;
  const double t_bar = fmax(fmax(fabs(x1[0] - x2[0]), fabs(x1[1] - x2[1])), fabs(x1[2] - x2[2])) / v_max;
  double cost = 100000000, t_d = t_bar;
  auto consider = [&](double t) {
    if (t < t_bar) return;
    const double c = -c1 / (3 * t * t * t) - c2 / (2 * t * t) - c3 / t + w_time * t;
    if (c < cost) {
      cost = c;
      t_d = t;
    }
  };
  {
    const double a = w_time, b = 0.0;
    const double a3 = b / a, a2 = c3 / a, a1 = c2 / a, a0 = c1 / a;
    const double y1 = kn_cubic_front(1, -a2, a1 * a3 - 4 * a0, 4 * a2 * a0 - a1 * a1 - a3 * a3 * a0);
    const double r = a3 * a3 / 4 - a2 + y1;
    if (!(r < 0)) {
      const double R = sqrt(r);
      double D, E;
      if (R != 0) {
        D = sqrt(0.75 * a3 * a3 - R * R - 2 * a2 + 0.25 * (4 * a3 * a2 - 8 * a1 - a3 * a3 * a3) / R);
        E = sqrt(0.75 * a3 * a3 - R * R - 2 * a2 - 0.25 * (4 * a3 * a2 - 8 * a1 - a3 * a3 * a3) / R);
      } else {
        D = sqrt(0.75 * a3 * a3 - 2 * a2 + 2 * sqrt(y1 * y1 - 4 * a0));
        E = sqrt(0.75 * a3 * a3 - 2 * a2 - 2 * sqrt(y1 * y1 - 4 * a0));
      }
      if (!isnan(D)) {
        consider(-a3 / 4 + R / 2 + D / 2);
        consider(-a3 / 4 + R / 2 - D / 2);
      }
      if (!isnan(E)) {
        consider(-a3 / 4 - R / 2 + E / 2);
        consider(-a3 / 4 - R / 2 - E / 2);
      }
    }
  }
  consider(t_bar);
  opt_t = t_d;
  const double tie_breaker = 1.0 + 1.0 / 10000;
  return 1.0 * (1 + tie_breaker) * cost;
}

__device__ __forceinline__ bool kn_in_box(const KinoArgs& K, const double p[3]) {
  for (int k = 0; k < 3; ++k)
    if (p[k] <= K.box_mind[k] || p[k] >= K.box_maxd[k]) return false;
  return true;
}
// KinodynamicAstar::posToIndex (:642-650): the search's own resolution on the map's origin
__device__ __forceinline__ void kn_idx(const Geo& g, const KinoArgs& K, const double p[3], int id[3]) {
  for (int k = 0; k < 3; ++k) id[k] = (int)floor((p[k] - g.org[k]) * K.inv_res);
}
__device__ __forceinline__ unsigned kn_hash(int x, int y, int z) {
  return (unsigned)x * 73856093u ^ (unsigned)y * 19349663u ^ (unsigned)z * 83492791u;
}
__device__ int kn_find(const KNode* pool, const int* hash, int cap, int x, int y, int z) {
  unsigned h = kn_hash(x, y, z) & (unsigned)(cap - 1);
  for (int probes = 0; probes < cap; ++probes) {
    const int n = hash[h];
    if (n < 0) return -1;
    const KNode& q = pool[n];
    if (q.idx[0] == x && q.idx[1] == y && q.idx[2] == z) return n;
    h = (h + 1) & (unsigned)(cap - 1);
  }
  return -1;
}
__device__ void kn_insert(int* hash, int cap, int x, int y, int z, int n) {
  unsigned h = kn_hash(x, y, z) & (unsigned)(cap - 1);
  while (hash[h] >= 0) h = (h + 1) & (unsigned)(cap - 1);  // the pool holds fewer nodes than half the slots
  hash[h] = n;
}

// std::__push_heap with NodeComparator (f1 > f2) on the nodes' current keys
__device__ void kn_sift_up(const KNode* pool, int* heap, int hole, int top, int value) {
  const double fv = pool[value].f;
  int parent = (hole - 1) / 2;
  while (hole > top && pool[heap[parent]].f > fv) {
    heap[hole] = heap[parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  heap[hole] = value;
}
__device__ void kn_push(const KNode* pool, int* heap, int& hn, int n) {
  heap[hn] = n;
  ++hn;
  kn_sift_up(pool, heap, hn - 1, 0, n);
}
// std::pop_heap + pop_back: __pop_heap moves the last element's value through __adjust_heap
__device__ void kn_pop(const KNode* pool, int* heap, int& hn) {
  if (hn > 1) {
    const int last = hn - 1;
    const int value = heap[last];
    heap[last] = heap[0];
    const int len = last;
    int hole = 0, child = 0;
    while (child < (len - 1) / 2) {
      child = 2 * (child + 1);
      if (pool[heap[child]].f > pool[heap[child - 1]].f) --child;
      heap[hole] = heap[child];
      hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
      child = 2 * (child + 1);
      heap[hole] = heap[child - 1];
      hole = child - 1;
    }
    kn_sift_up(pool, heap, hole, 0, value);
  }
  --hn;
}

// computeShotTraj (:331-394); coef[axis][power]
__device__ bool kn_shot(const Geo& g, const KinoArgs& K, const double s1[6], const double s2[6], double t_d, double* coef) {
  for (int k = 0; k < 3; ++k) {
    const double p0 = s1[k], dp = s2[k] - p0, v0 = s1[3 + k], v1 = s2[3 + k], dv = v1 - v0;
    const double a = 1.0 / 6.0 * (-12.0 / (t_d * t_d * t_d) * (dp - v0 * t_d) + 6 / (t_d * t_d) * dv);
    const double b = 0.5 * (6.0 / (t_d * t_d) * (dp - v0 * t_d) - 2 / t_d * dv);
    coef[4 * k + 0] = p0, coef[4 * k + 1] = v0, coef[4 * k + 2] = b, coef[4 * k + 3] = a;
  }
  const double t_delta = t_d / 10;
  int checks = 0;
  for (double time = t_delta; time <= t_d; time += t_delta) {
    if (++checks > 1000) return false;  // t_d = 0 or not finite: the reference does not return
    const double t2 = time * time, t3 = pow(time, 3.0);
    double c[3];
    for (int k = 0; k < 3; ++k) c[k] = ((coef[4 * k] * 1.0 + coef[4 * k + 1] * time) + coef[4 * k + 2] * t2) + coef[4 * k + 3] * t3;
    for (int k = 0; k < 3; ++k)
      if (c[k] < g.org[k] || c[k] >= K.map_size[k]) return false;  // (the reference compares with the SIZE)
    if (plane_at_pos(g, K.infl, c)) return false;
  }
  return true;
}

__device__ void kn_no_path(const KinoArgs& K, int b, int status, int which, int iter, int use) {
  K.status[b] = status, K.which[b] = which, K.iter_num[b] = iter, K.use_node_num[b] = use;
  K.n_nodes[b] = 0, K.shot[b] = 0, K.seg_num[b] = 0, K.n_samples[b] = 0, K.skip[b] = 1;
  K.t_shot[b] = 0.0, K.T_sum[b] = 0.0, K.ts_out[b] = 0.0;
  for (int i = 0; i < 12; ++i) K.coef_shot[(size_t)b * 12 + i] = 0.0, K.derivs[(size_t)b * 12 + i] = 0.0;
}

__global__ void __launch_bounds__(KN_NT) k_kino_path(Geo g, KinoArgs K) {
  __shared__ KShared S;
  const int tid = threadIdx.x, b = blockIdx.x;
  const fuelmi_kino_cfg& cfg = K.cfg;
  const int alloc = cfg.allocate_num, cap = K.hash_cap;
  KNode* pool = reinterpret_cast<KNode*>(K.pool) + (size_t)b * alloc;
  int* heap = K.heap + (size_t)b * alloc;
  int* hash = K.hash + (size_t)b * cap;
  const double* in = K.in + (size_t)b * 15;
  const double sp[3] = {in[0], in[1], in[2]}, sv[3] = {in[3], in[4], in[5]}, sa[3] = {in[6], in[7], in[8]};
  const double endst[6] = {in[9], in[10], in[11], in[12], in[13], in[14]};
  {  // kinodynamicReplan's refusal (planner_manager.cpp:131-134)
    const double x = sp[0] - endst[0], y = sp[1] - endst[1], z = sp[2] - endst[2];
    if (sqrt(x * x + y * y + z * z) < 1e-2) {
      if (tid == 0) kn_no_path(K, b, FUELMI_KINO_CLOSE_GOAL, 0, 0, 0);
      return;
    }
  }
  int eidx[3];
  kn_idx(g, K, endst, eidx);

  int status = FUELMI_KINO_NO_PATH, which = 0;
  for (int search = 0; search < 2; ++search) {
    which = search;
    if (search == 1) {  // reset(): the hash; node records are rewritten when they are taken from the pool
      __syncthreads();
      for (int i = tid; i < cap; i += KN_NT) hash[i] = -1;
      __syncthreads();
    }
    if (tid == 0) {
      KNode& n0 = pool[0];
      double t;
      for (int k = 0; k < 3; ++k) n0.st[k] = sp[k], n0.st[3 + k] = sv[k], n0.in[k] = 0.0;
      kn_idx(g, K, sp, n0.idx);
      n0.g = 0.0;
      n0.f = cfg.lambda_heu * kn_heuristic(n0.st, endst, cfg.w_time, cfg.max_vel, t);
      n0.dur = 0.0, n0.parent = -1, n0.state = KN_OPEN;
      heap[0] = 0;
      kn_insert(hash, cap, n0.idx[0], n0.idx[1], n0.idx[2], 0);
      S.hn = 1, S.use = 1, S.iter = 0, S.shot = 0;
      S.init = search == 0 ? 1 : 0;
    }
    for (;;) {
      __syncthreads();
      if (tid == 0) {
        int action = FUELMI_KINO_NO_PATH;  // "open set empty, no path!"
        if (S.hn > 0) {
          const int cur = heap[0];
          KNode& c = pool[cur];
          const double x = c.st[0] - sp[0], y = c.st[1] - sp[1], z = c.st[2] - sp[2];
          const bool reach_horizon = sqrt(x * x + y * y + z * z) >= cfg.horizon;
          const bool near_end = abs(c.idx[0] - eidx[0]) <= K.tolerance && abs(c.idx[1] - eidx[1]) <= K.tolerance &&
                                abs(c.idx[2] - eidx[2]) <= K.tolerance;
          S.cur = cur;
          if (near_end) {
            double t;
            double stc[6];
            for (int k = 0; k < 6; ++k) stc[k] = c.st[k];
            kn_heuristic(stc, endst, cfg.w_time, cfg.max_vel, t);
            if (kn_shot(g, K, stc, endst, t, S.coef)) S.shot = 1, S.t_shot = t;
          }
          if (reach_horizon) {
            action = S.shot ? FUELMI_KINO_REACH_END : FUELMI_KINO_REACH_HORIZON;
          } else if (near_end) {
            action = S.shot ? FUELMI_KINO_REACH_END : (c.parent >= 0 ? FUELMI_KINO_NEAR_END : FUELMI_KINO_NO_PATH);
          } else {
            int hn = S.hn;
            kn_pop(pool, heap, hn);
            S.hn = hn;
            c.state = KN_CLOSED;
            S.iter += 1;
            action = KN_EXPAND;
          }
        }
        S.action = action;
      }
      __syncthreads();
      if (S.action != KN_EXPAND) break;

      // ---- one primitive per lane
      const int cur = S.cur;
      const bool init = S.init != 0;
      const int nprim = init ? K.n_init : K.n_reg;
      const double* prims = K.prims + (init ? 0 : 4 * (size_t)K.n_init);
      double cst[6];
      for (int k = 0; k < 6; ++k) cst[k] = pool[cur].st[k];
      const double cg = pool[cur].g;
      const int cidx[3] = {pool[cur].idx[0], pool[cur].idx[1], pool[cur].idx[2]};
      int kind = KN_DEAD;
      if (tid < nprim) {
        const double tau = prims[4 * tid + 3];
        const double um[3] = {init ? sa[0] : prims[4 * tid], init ? sa[1] : prims[4 * tid + 1],
                              init ? sa[2] : prims[4 * tid + 2]};
        double pro[6];
        kn_transit(cst, um, tau, pro);
        bool ok = kn_in_box(K, pro);
        int pid[3] = {0, 0, 0}, node = -1;
        if (ok) {
          kn_idx(g, K, pro, pid);
          node = kn_find(pool, hash, cap, pid[0], pid[1], pid[2]);
          if (node >= 0 && pool[node].state == KN_CLOSED) ok = false;
        }
        if (ok && (fabs(pro[3]) > cfg.max_vel || fabs(pro[4]) > cfg.max_vel || fabs(pro[5]) > cfg.max_vel)) ok = false;
        if (ok && pid[0] == cidx[0] && pid[1] == cidx[1] && pid[2] == cidx[2]) ok = false;
        if (ok) {
          for (int k = 1; k <= cfg.check_num; ++k) {
            const double dt = tau * double(k) / double(cfg.check_num);
            double xt[6];
            kn_transit(cst, um, dt, xt);
            if (plane_at_pos(g, K.infl, xt) || !kn_in_box(K, xt) || (!cfg.optimistic && plane_at_pos(g, K.unk, xt))) {
              ok = false;
              break;
            }
          }
        }
        if (ok) {
          double t;
          const double gs = ((um[0] * um[0] + um[1] * um[1] + um[2] * um[2]) + cfg.w_time) * tau + cg;
          const double fs = gs + cfg.lambda_heu * kn_heuristic(pro, endst, cfg.w_time, cfg.max_vel, t);
          for (int k = 0; k < 6; ++k) S.st[k][tid] = pro[k];
          S.g[tid] = gs, S.f[tid] = fs;
          S.vx[tid] = pid[0], S.vy[tid] = pid[1], S.vz[tid] = pid[2];
          kind = node >= 0 ? node : KN_NEW;
        }
      }
      S.kind[tid] = kind;
      __syncthreads();
      if (kind == KN_NEW) {  // the first surviving lane of this expansion in the same, so far empty voxel
        int first = tid;
        const int x = S.vx[tid], y = S.vy[tid], z = S.vz[tid];
        for (int j = 0; j < tid; ++j)
          if (S.kind[j] == KN_NEW && S.vx[j] == x && S.vy[j] == y && S.vz[j] == z) {
            first = j;
            break;
          }
        S.first[tid] = first;
      }
      __syncthreads();

      // ---- the reference's double loop, replayed over the survivors
      if (tid == 0) {
        int use = S.use, hn = S.hn, action = KN_EXPAND;
        for (int p = 0; p < nprim; ++p) {
          const int kd = S.kind[p];
          if (kd == KN_DEAD) continue;
          const double tau = prims[4 * p + 3];
          const double u0 = init ? sa[0] : prims[4 * p], u1 = init ? sa[1] : prims[4 * p + 1],
                       u2 = init ? sa[2] : prims[4 * p + 2];
          int n;
          bool write;
          if (kd >= 0) {  // an older node in the open set: compared by g
            n = kd;
            write = S.g[p] < pool[n].g;
          } else if (S.first[p] != p) {  // a sibling created by this expansion: compared by f
            n = S.made[S.first[p]];
            write = S.f[p] < pool[n].f;
          } else {
            n = use;
            write = true;
          }
          if (write) {
            KNode& q = pool[n];
            for (int k = 0; k < 6; ++k) q.st[k] = S.st[k][p];
            q.f = S.f[p], q.g = S.g[p];
            q.in[0] = u0, q.in[1] = u1, q.in[2] = u2;
            q.dur = tau;
            q.parent = cur;
          }
          if (kd == KN_NEW && S.first[p] == p) {
            KNode& q = pool[n];
            q.idx[0] = S.vx[p], q.idx[1] = S.vy[p], q.idx[2] = S.vz[p];
            q.state = KN_OPEN;
            kn_push(pool, heap, hn, n);
            kn_insert(hash, cap, q.idx[0], q.idx[1], q.idx[2], n);
            S.made[p] = n;
            use += 1;
            if (use == alloc) {  // "run out of memory."
              action = FUELMI_KINO_NO_PATH;
              break;
            }
          }
        }
        S.use = use, S.hn = hn, S.init = 0;
        S.action = action;
      }
      __syncthreads();
      if (S.action != KN_EXPAND) break;
    }
    status = S.action;
    if (status != FUELMI_KINO_NO_PATH) break;
  }
  if (tid != 0) return;
  if (status == FUELMI_KINO_NO_PATH) {
    kn_no_path(K, b, status, which, S.iter, S.use);
    return;
  }

  // ---- retrievePath (:285-295)
  const int back = S.cur;
  int len = 1;
  for (int n = back; pool[n].parent >= 0; n = pool[n].parent) ++len;
  bool over = false;
  if (K.node_state || K.node_input || K.node_duration) {
    over = len > cfg.max_path_nodes;
    int i = len - 1;
    for (int n = back; n >= 0; n = pool[n].parent, --i) {
      if (i >= cfg.max_path_nodes) continue;
      const size_t at = (size_t)b * cfg.max_path_nodes + i;
      if (K.node_state)
        for (int k = 0; k < 6; ++k) K.node_state[at * 6 + k] = pool[n].st[k];
      if (K.node_input)
        for (int k = 0; k < 3; ++k) K.node_input[at * 3 + k] = pool[n].in[k];
      if (K.node_duration) K.node_duration[at] = pool[n].dur;
    }
  }

  // ---- getSamples (:543-634)
  const bool shot = S.shot != 0;
  const double t_shot = shot ? S.t_shot : 0.0;
  double T_sum = 0.0;
  if (shot) T_sum += t_shot;
  int node = back;
  while (pool[node].parent >= 0) {
    T_sum += pool[node].dur;
    node = pool[node].parent;
  }
  double t, end_vel[3], end_acc[3];
  if (shot) {
    t = t_shot;
    for (int k = 0; k < 3; ++k) {
      end_vel[k] = endst[3 + k];
      end_acc[k] = 2 * S.coef[4 * k + 2] + 6 * S.coef[4 * k + 3] * t_shot;
    }
  } else {
    t = pool[back].dur;
    for (int k = 0; k < 3; ++k) {
      end_vel[k] = pool[node].st[3 + k];  // the START node's velocity, as the reference has it
      end_acc[k] = pool[back].in[k];
    }
  }
  int seg = cfg.seg_num;
  if (seg <= 0) {
    double q = floor(T_sum / cfg.ts);
    if (!(q < (double)FUELMI_KINO_MAX_SEG)) q = (double)FUELMI_KINO_MAX_SEG;
    seg = max(cfg.min_seg, (int)q);
  }
  const double ts = T_sum / double(seg);
  int count = 0;
  for (double ti = T_sum; ti > -1e-5; ti -= ts)
    if (++count >= FUELMI_KINO_MAX_SEG + 2) break;
  const int maxs = K.load_points > 0 ? K.load_points : cfg.max_samples;
  double* smp = K.samples + (size_t)b * maxs * 3;
  bool sample_shot = shot;
  node = back;
  int i = 0;
  for (double ti = T_sum; ti > -1e-5 && i < count; ti -= ts, ++i) {
    double c[3];
    if (sample_shot) {
      const double t2 = t * t, t3 = pow(t, 3.0);
      for (int k = 0; k < 3; ++k)
        c[k] = ((S.coef[4 * k] * 1.0 + S.coef[4 * k + 1] * t) + S.coef[4 * k + 2] * t2) + S.coef[4 * k + 3] * t3;
      t -= ts;
      if (t < -1e-5) {
        sample_shot = false;
        if (pool[node].parent >= 0) t += pool[node].dur;
      }
    } else {
      const int par = pool[node].parent;
      if (par < 0) break;  // (the reference dereferences a null parent here; a one-node path never gets this far)
      double x0[6], xt[6];
      for (int k = 0; k < 6; ++k) x0[k] = pool[par].st[k];
      const double ut[3] = {pool[node].in[0], pool[node].in[1], pool[node].in[2]};
      kn_transit(x0, ut, t, xt);
      for (int k = 0; k < 3; ++k) c[k] = xt[k];
      t -= ts;
      if (t < -1e-5 && pool[par].parent >= 0) {
        node = par;
        t += pool[node].dur;
      }
    }
    const int at = count - 1 - i;  // reverse(point_set)
    if (at < maxs)
      for (int k = 0; k < 3; ++k) smp[3 * at + k] = c[k];
  }
  double* der = K.derivs + (size_t)b * 12;
  for (int k = 0; k < 3; ++k) {
    der[k] = sv[k];
    der[3 + k] = end_vel[k];
    der[6 + k] = pool[back].parent < 0 ? 2 * S.coef[4 * k + 2] : pool[node].in[k];
    der[9 + k] = end_acc[k];
  }
  over = over || (K.load_points > 0 ? count != K.load_points : count > cfg.max_samples);
  K.status[b] = over ? -1 : status;
  K.skip[b] = over ? 1 : 0;
  K.which[b] = which, K.iter_num[b] = S.iter, K.use_node_num[b] = S.use;
  K.n_nodes[b] = len, K.shot[b] = shot ? 1 : 0, K.seg_num[b] = seg, K.n_samples[b] = count;
  K.t_shot[b] = t_shot, K.T_sum[b] = T_sum, K.ts_out[b] = ts;
  for (int k = 0; k < 12; ++k) K.coef_shot[(size_t)b * 12 + k] = shot ? S.coef[k] : 0.0;
}

bool pos_fin(double x) { return std::isfinite(x) && x > 0.0; }

// the reference's accumulating loops (:107-122), literally
int kino_prims(const fuelmi_kino_cfg* cfg, std::vector<double>& prims, int& n_init, int& n_reg) {
  prims.clear();
  n_init = n_reg = 0;
  const double step_i = cfg->time_res_init * cfg->init_max_tau;
  for (double tau = step_i; tau <= cfg->init_max_tau + 1e-3; tau += step_i) {
    if (++n_init > FUELMI_KINO_MAX_PRIMS) break;
    prims.insert(prims.end(), {0.0, 0.0, 0.0, tau});
  }
  std::vector<double> acc, dur;
  const double step_a = cfg->max_acc * cfg->res;
  for (double a = -cfg->max_acc; a <= cfg->max_acc + 1e-3; a += step_a) {
    acc.push_back(a);
    if (acc.size() > FUELMI_KINO_MAX_PRIMS) break;
  }
  const double step_t = cfg->time_res * cfg->max_tau;
  for (double tau = step_t; tau <= cfg->max_tau; tau += step_t) {
    dur.push_back(tau);
    if (dur.size() > FUELMI_KINO_MAX_PRIMS) break;
  }
  const size_t nr = acc.size() * acc.size() * acc.size() * dur.size();
  if (n_init > FUELMI_KINO_MAX_PRIMS || nr > FUELMI_KINO_MAX_PRIMS) {
    fuelmi_set_error("kinodynamic search: an expansion has more than %d primitives (init list %d%s, regular list %zu)",
                     FUELMI_KINO_MAX_PRIMS, n_init, n_init > FUELMI_KINO_MAX_PRIMS ? "+" : "", nr);
    return FUELMI_ELIMIT;
  }
  for (double ax : acc)
    for (double ay : acc)
      for (double az : acc)
        for (double tau : dur) prims.insert(prims.end(), {ax, ay, az, tau});
  n_reg = (int)nr;
  return FUELMI_OK;
}

size_t kino_workspace(const fuelmi_kino_cfg* cfg, int* hash_cap) {
  int cap = 16;
  while (cap < 2 * cfg->allocate_num) cap <<= 1;
  if (hash_cap) *hash_cap = cap;
  return (size_t)cfg->allocate_num * (sizeof(KNode) + sizeof(int)) + (size_t)cap * sizeof(int);
}

int kino_check_cfg(const fuelmi_kino_cfg* cfg) {
  ARGCHK(cfg);
  ARGCHK(pos_fin(cfg->max_tau) && pos_fin(cfg->init_max_tau) && pos_fin(cfg->max_vel) && pos_fin(cfg->max_acc));
  ARGCHK(pos_fin(cfg->w_time) && pos_fin(cfg->horizon) && pos_fin(cfg->resolution) && pos_fin(cfg->lambda_heu));
  ARGCHK(pos_fin(cfg->res) && pos_fin(cfg->time_res) && pos_fin(cfg->time_res_init) && pos_fin(cfg->ts));
  ARGCHK(cfg->check_num >= 1 && cfg->allocate_num >= 2);
  ARGCHK(cfg->min_seg >= 1 && cfg->min_seg <= FUELMI_KINO_MAX_SEG);
  ARGCHK(cfg->seg_num >= 0 && cfg->seg_num <= FUELMI_KINO_MAX_SEG);
  ARGCHK(cfg->max_path_nodes >= 1 && cfg->max_samples >= 1);
  ARGCHK(2e7 / cfg->resolution < 2147483648.0);  // every voxel index of a checked coordinate fits an int
  if (cfg->allocate_num > FUELMI_KINO_MAX_ALLOC) {
    fuelmi_set_error("kinodynamic search: allocate_num = %d exceeds %d", cfg->allocate_num, FUELMI_KINO_MAX_ALLOC);
    return FUELMI_ELIMIT;
  }
  std::vector<double> prims;
  int ni, nr;
  return kino_prims(cfg, prims, ni, nr);
}

int kino_check(const fuelmi_kino_cfg* cfg, int n_prob, const double* start_xyz, const double* start_vel,
               const double* start_acc, const double* goal_xyz, const double* goal_vel) {
  {
    const int rc = kino_check_cfg(cfg);
    if (rc) return rc;
  }
  ARGCHK(n_prob >= 0);
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(start_xyz && start_vel && start_acc && goal_xyz && goal_vel);
  for (long k = 0; k < 3L * n_prob; ++k)
    ARGCHK(std::fabs(start_xyz[k]) < 1e7 && std::fabs(start_vel[k]) < 1e7 && std::fabs(start_acc[k]) < 1e7 &&
           std::fabs(goal_xyz[k]) < 1e7 && std::fabs(goal_vel[k]) < 1e7);
  const double total = (double)n_prob * (double)kino_workspace(cfg, nullptr);
  if (total > FUELMI_KINO_MAX_WORKSPACE) {
    fuelmi_set_error("kinodynamic search: %d problems x %zu bytes of workspace exceed %.0f bytes", n_prob,
                     kino_workspace(cfg, nullptr), FUELMI_KINO_MAX_WORKSPACE);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

// fills geometry / lists / workspace pointers of K from the map's kino_dev pool (reserved for io_bytes + the workspaces),
// uploads the inputs and the lists, clears the hashes; *io is the start of io_bytes of device memory for the caller's results
int kino_prepare(fuelmi_map* m, const fuelmi_kino_cfg* cfg, int n_prob, const double* start_xyz, const double* start_vel,
                 const double* start_acc, const double* goal_xyz, const double* goal_vel, size_t io_bytes, KinoArgs& K,
                 unsigned char** io) {
  std::vector<double> prims;
  int ni = 0, nr = 0;
  {
    const int rc = kino_prims(cfg, prims, ni, nr);
    if (rc) return rc;
  }
  hipStream_t st = m->stream;
  const size_t n = (size_t)n_prob, alloc = (size_t)cfg->allocate_num;
  int cap = 0;
  kino_workspace(cfg, &cap);
  double *d_in, *d_pr;
  memset(&K, 0, sizeof(K));
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 256);
    *io = L.take<unsigned char>(io_bytes);
    d_in = L.take<double>(n * 15);
    d_pr = L.take<double>(prims.size());
    K.pool = reinterpret_cast<unsigned char*>(L.take<KNode>(n * alloc));
    K.heap = L.take<int>(n * alloc);
    K.hash = L.take<int>(n * (size_t)cap);
    return L.size();
  };
  {
    const int rc = m->kino_dev.carve(st, layout);
    if (rc) return rc;
  }
  // staged in the map: the sources must outlive this function (the copies may run after it returns)
  std::vector<double>& hin = m->kino_host;
  hin.assign(n * 15 + prims.size(), 0.0);
  for (size_t b = 0; b < n; ++b)
    for (int k = 0; k < 3; ++k) {
      hin[15 * b + k] = start_xyz[3 * b + k], hin[15 * b + 3 + k] = start_vel[3 * b + k];
      hin[15 * b + 6 + k] = start_acc[3 * b + k], hin[15 * b + 9 + k] = goal_xyz[3 * b + k];
      hin[15 * b + 12 + k] = goal_vel[3 * b + k];
    }
  std::copy(prims.begin(), prims.end(), hin.begin() + (long)(n * 15));
  HIPCHK(hipMemcpyAsync(d_in, hin.data(), n * 15 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_pr, hin.data() + n * 15, prims.size() * sizeof(double), hipMemcpyHostToDevice, st));
  K.cfg = *cfg;
  K.n_prob = n_prob;
  K.n_init = ni, K.n_reg = nr;
  K.prims = d_pr;
  K.tolerance = (int)std::ceil(1 / cfg->resolution);
  K.inv_res = 1.0 / cfg->resolution;
  for (int k = 0; k < 3; ++k)
    K.box_mind[k] = m->cfg.box_min[k], K.box_maxd[k] = m->cfg.box_max[k], K.map_size[k] = m->cfg.map_size[k];
  K.infl = m->infl_bits.p;
  K.unk = m->unk_bits.p;
  K.in = d_in;
  K.hash_cap = cap;
  HIPCHK(hipMemsetAsync(K.hash, 0xFF, n * (size_t)cap * sizeof(int), st));
  return FUELMI_OK;
}

int kino_launch(fuelmi_map* m, const KinoArgs& K) {
  hipLaunchKernelGGL(k_kino_path, dim3(K.n_prob), dim3(KN_NT), 0, m->stream, m->g, K);
  HIPCHK(hipGetLastError());
  return FUELMI_OK;
}

}  // namespace

extern "C" int fuelmi_kino_plan(const fuelmi_kino_cfg* cfg, long long out8[8]) {
  ARGCHK(out8);
  {
    const int rc = kino_check_cfg(cfg);
    if (rc) return rc;
  }
  std::vector<double> prims;
  int ni = 0, nr = 0, cap = 0;
  kino_prims(cfg, prims, ni, nr);
  out8[0] = KN_NT, out8[1] = (long long)sizeof(KShared), out8[2] = (long long)kino_workspace(cfg, &cap);
  out8[3] = ni, out8[4] = nr, out8[5] = FUELMI_KINO_MAX_PRIMS, out8[6] = FUELMI_KINO_MAX_ALLOC, out8[7] = cap;
  return FUELMI_OK;
}

extern "C" int fuelmi_map_kino_paths(fuelmi_map* m, const fuelmi_kino_cfg* cfg, int n_prob, const double* start_xyz,
                                     const double* start_vel, const double* start_acc, const double* goal_xyz,
                                     const double* goal_vel, int* status, int* which, int* iter_num, int* use_node_num,
                                     int* n_nodes, double* node_state, double* node_input, double* node_duration,
                                     int* shot, double* t_shot, double* coef_shot, double* T_sum, double* ts_out,
                                     int* seg_num, int* n_samples, double* samples, double* derivs) {
  {  // every argument on the host, before the map is touched
    const int rc = kino_check(cfg, n_prob, start_xyz, start_vel, start_acc, goal_xyz, goal_vel);
    if (rc) return rc;
  }
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(status && which && iter_num && use_node_num && n_nodes && shot && t_shot && coef_shot && T_sum && ts_out &&
         seg_num && n_samples && samples && derivs);
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  const size_t n = (size_t)n_prob, maxs = (size_t)cfg->max_samples, maxn = (size_t)cfg->max_path_nodes;
  KinoArgs K;
  ResultBlock R(16);  // skip is the kernel's own; the path nodes only where the caller asks
  R.add(K.status, status, n);
  R.add(K.which, which, n);
  R.add(K.iter_num, iter_num, n);
  R.add(K.use_node_num, use_node_num, n);
  R.add(K.n_nodes, n_nodes, n);
  R.add(K.shot, shot, n);
  R.add(K.seg_num, seg_num, n);
  R.add(K.n_samples, n_samples, n);
  R.hold(K.skip, n);
  R.add(K.t_shot, t_shot, n);
  R.add(K.T_sum, T_sum, n);
  R.add(K.ts_out, ts_out, n);
  R.add(K.coef_shot, coef_shot, n * 12);
  R.add(K.derivs, derivs, n * 12);
  R.add(K.samples, samples, n * maxs * 3);
  R.opt(K.node_state, node_state, n * maxn * 6);
  R.opt(K.node_input, node_input, n * maxn * 3);
  R.opt(K.node_duration, node_duration, n * maxn);
  ARGCHK(!R.overflow);
  unsigned char* io = nullptr;
  {
    const int rc = kino_prepare(m, cfg, n_prob, start_xyz, start_vel, start_acc, goal_xyz, goal_vel, R.size(), K, &io);
    if (rc) return rc;
  }
  R.bind(io);
  {
    const int rc = kino_launch(m, K);
    if (rc) return rc;
  }
  {
    const int rc = result_fetch(R, m->stream);
    if (rc) return rc;
  }
  const int b = first_over_limit(status, n_prob);
  if (b < 0) return FUELMI_OK;
  fuelmi_set_error("kinodynamic search: problem %d has %d path nodes / %d samples, more than max_path_nodes = %d / "
                   "max_samples = %d", b, n_nodes[b], n_samples[b], cfg->max_path_nodes, cfg->max_samples);
  return FUELMI_ELIMIT;
}

// start / goal -> kinodynamic search -> getSamples (k_kino_path, written into the staging) -> the fit, all on the map's
// stream: the mid-range counterpart of fuelmi_bspline_dev_load_waypoints (waypoint_traj.hip)
extern "C" int fuelmi_bspline_dev_load_kino(fuelmi_bspline_dev* b, const fuelmi_kino_cfg* cfg, const double* start_xyz,
                                            const double* start_vel, const double* start_acc, const double* goal_xyz,
                                            const double* goal_vel, int* status, double* T_sum) {
  ARGCHK(b && cfg && status);
  BsplineArgs& A = b->a;
  const int degree = A.cfg.bspline_degree;
  ARGCHK(A.dim == 3 && degree >= 3 && degree <= 5 && A.N - degree >= 1);
  const int seg = A.N - degree, n_points = seg + 1;
  ARGCHK(cfg->seg_num == 0 || cfg->seg_num == seg);
  fuelmi_kino_cfg kc = *cfg;
  kc.seg_num = seg, kc.max_samples = n_points, kc.max_path_nodes = 1;
  {
    const int rc = kino_check(&kc, A.C, start_xyz, start_vel, start_acc, goal_xyz, goal_vel);
    if (rc) return rc;
  }
  fuelmi_map* m = b->map;
  ARGCHK(m);
  opt_set_valid(b, false);
  HIPCHK(hipSetDevice(m->device));
  const size_t C = (size_t)A.C, K = (size_t)n_points;
  hipStream_t st = m->stream;
  {
    const int rc = b->fit_in.reserve(st, C * (1 + K * 3 + 12) * sizeof(double));
    if (rc) return rc;
  }
  double* d_fit = static_cast<double*>(b->fit_in.p);  // ts | points | derivs
  KinoArgs W;
  auto layout = [&](unsigned char* base) {  // the results that do not go to the fit
    BlockLayout L(base, 16);
    W.status = L.take<int>(C);
    W.which = L.take<int>(C);
    W.iter_num = L.take<int>(C);
    W.use_node_num = L.take<int>(C);
    W.n_nodes = L.take<int>(C);
    W.shot = L.take<int>(C);
    W.seg_num = L.take<int>(C);
    W.n_samples = L.take<int>(C);
    W.skip = L.take<int>(C);
    W.t_shot = L.take<double>(C);
    W.T_sum = L.take<double>(C);
    W.coef_shot = L.take<double>(C * 12);
    return L.size();
  };
  unsigned char* io = nullptr;
  {
    const int rc = kino_prepare(m, &kc, A.C, start_xyz, start_vel, start_acc, goal_xyz, goal_vel, layout(nullptr), W, &io);
    if (rc) return rc;
  }
  layout(io);
  W.load_points = n_points;
  W.ts_out = d_fit;  // the fit's knot spans
  W.samples = d_fit + C;
  W.derivs = d_fit + C + C * K * 3;
  const FitArgs F = fit_args(b, W.ts_out, W.samples, W.derivs, W.skip);
  {
    const int rck = kino_launch(m, W);  // (outside the scope: the search is no spline stage)
    if (rck) return rck;
    StageScope sc(m, FUELMI_K_BSPLINE);
    const int rcf = fit_launch(m, F);
    if (rcf) return rcf;
  }
  HIPCHK(hipMemcpyAsync(status, W.status, C * sizeof(int), hipMemcpyDeviceToHost, st));
  if (T_sum) HIPCHK(hipMemcpyAsync(T_sum, W.T_sum, C * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(stream_wait(st));
  for (int c = 0; c < A.C; ++c)
    if (status[c] == -1) {
      fuelmi_set_error("kinodynamic search: candidate %d does not give %d samples", c, n_points);
      return FUELMI_ELIMIT;
    }
  return FUELMI_OK;
}
