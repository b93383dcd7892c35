// topo_path.hip -- the topological path search of guided replanning: TopologyPRM::findTopoPaths
// (path_searching/src/topo_prm.cpp:43-98) as FastPlannerManager::topoReplan calls it (plan_manage/src/planner_manager.cpp:431)
// for a batch of independent problems on one map: createGraph over a given sample stream, pruneGraph, searchPaths,
// shortcutPaths, pruneEquivalent, selectShortPaths.
//
// One workgroup of TP_NT lanes (one wave) per problem.  The time of the search goes into voxel ray walks (lineVisib:
// RayCaster::setInput / step, plan_env/src/raycast.cpp:228-321, against the distance field), and those are what runs side
// by side:
//   findVisibGuard   one lane per guard, TP_NT guards a step; the lanes' verdicts go through LDS and every lane reads them
//                    in list order, so "the first three visible guards" are the reference's
//   sameTopoPath     one lane per pair of path points
//   shortcutPath     the lanes test the next TP_NT points against short_path.back(); the first blocked one is committed
//                    (its lane does the gradient push), the points behind it are tested again from the new back
//   discretizeLine   one lane per point
//   pruneGraph       the fixed point of "drop every node past the first two with at most one neighbour", in rounds over
//                    all nodes instead of the reference's restart after every erase: the surviving nodes, their order and
//                    the order of their neighbours are the same (an erase keeps the order of what stays, and no node is
//                    twice in one neighbour list)
// The bookkeeping that depends on order (which guard a sample sees, needConnection's double loop, the depth-first search,
// the selection) is replayed by all lanes on the same values, or by lane 0 alone.  The graph, the raw / shortened paths and
// the discretised path live in the problem's workspace in the map's topo_dev pool; LDS holds the lanes' verdicts and the
// two length lists of sameTopoPath (fuelmi_topo_plan reports the bytes).
//
// Decisions on the field: the positive part of the reference's field is res * sqrt(k) for an integer k, the device's is
// the f32 product through an approximate square root, so `dist <= thresh` is taken on k: the host turns a threshold into
// the largest k the reference's f64 comparison accepts and hands the kernel an f32 cut between the device's values of k
// and k + 1 (topo_cut).  Only shortcutPath's gradient uses the f32 values as numbers.
//
// All f64, -ffp-contract=off, sums in the reference's order.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "fuelmi_internal.h"

namespace {

constexpr int TP_NT = 64;
constexpr int TP_PCAP = FUELMI_TOPO_MAX_PATH_POINTS;
constexpr int TP_DCAP = FUELMI_TOPO_MAX_DIS_POINTS;
constexpr int TP_NB = FUELMI_TOPO_MAX_NEIGHBORS;
constexpr int TP_RAWN = 100;  // searchPaths' path_list(100): a raw path of 100 nodes or more indexes past it
constexpr int TP_UNDEF = -2, TP_CAP = -3;  // a step's verdict besides its own >= 0 answers

// k_topo_path: one problem per workgroup; every pointer addresses device memory
struct TopoArgs {
  fuelmi_topo_cfg cfg;
  int n_prob;
  int max_start, max_end;  // strides of start_pts / end_pts
  int nc;                  // node records of one problem: max_sample_num + 2
  float cut_res, cut_zero, cut_clear;
  double off[3];           // TopologyPRM::offset_ = 0.5 - origin / resolution
  const float* dist;
  const double* in;        // [n][2][3]: start, end
  const double* spts;      // [n][max_start][3]
  const double* epts;      // [n][max_end][3]
  const int* n_spts;
  const int* n_epts;
  const double* samples;   // [n][max_sample_num][3]
  // workspace, [n] x the count given
  double* node_pos;        // [nc][3]
  unsigned char* node_type;  // [nc] GraphNode::Guard = 1, Connector = 2
  unsigned char* alive;    // [nc] 1, 2 = leaves in this round of pruneGraph, 0 = erased
  unsigned char* on_stack; // [nc] the depth-first search's `visited`
  unsigned short* nb;      // [nc][TP_NB] neighbours in push_back order
  int* nb_cnt;             // [nc]
  int* guards;             // [nc] the guards in list order
  int* dfs_node;           // [nc]
  int* dfs_it;             // [nc]
  unsigned short* raw_nodes;  // [max_raw_path][TP_RAWN]
  int* raw_len;            // [max_raw_path]
  int* kept;               // [max_raw_path2] raw paths the bucket filter keeps
  int* exist;              // [max(max_raw_path2, reserve_num)] pruneEquivalent's exist_paths_id
  int* avail;              // [max_raw_path2] selectShortPaths' shrinking `paths`
  double* shortp;          // [max_raw_path2][TP_PCAP][3] short_paths_
  int* short_len;          // [max_raw_path2]
  double* selp;            // [reserve_num][TP_PCAP][3]
  int* sel_len;            // [reserve_num]
  double* buf;             // [2][TP_PCAP][3] shortcutPath's short_path and last_path
  double* dis;             // [TP_DCAP][3]
  // results; all but status / counts / events may be null
  int* status;
  int* counts;             // [n][4] raw paths found, kept, filtered, selected
  int* events;             // [n][6]
  int* n_nodes;
  int* node_id;            // [n][max_nodes]
  int* node_kind;          // [n][max_nodes]
  double* node_xyz;        // [n][max_nodes][3]
  int* nb_off;             // [n][max_nodes + 1]
  int* nb_ids;             // [n][4 max_nodes]
  double* raw_paths;       // [n][max_raw_path2][max_path_points][3]
  int* raw_plen;           // [n][max_raw_path2]
  double* filt_paths;
  int* filt_plen;
  double* sel_paths;       // [n][reserve_num][max_path_points][3]
  int* sel_plen;           // [n][reserve_num]
  double* sel_length;      // [n][reserve_num]
};

struct TShared {
  double lenA[TP_PCAP], lenB[TP_PCAP];  // sameTopoPath's len_list of either path
  double tri[2][9];                     // needConnection's path1 / path2
  int flag[TP_NT];
  int code;
};

// one problem's slices of the workspace
struct TWork {
  double* node_pos;
  unsigned char *node_type, *alive, *on_stack;
  unsigned short* nb;
  int *nb_cnt, *guards, *dfs_node, *dfs_it;
  unsigned short* raw_nodes;
  int *raw_len, *kept, *exist, *avail;
  double* shortp;
  int* short_len;
  double* selp;
  int* sel_len;
  double *buf, *dis;
};

__device__ __forceinline__ bool tp_fin3(const double* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// SDFMap::getDistance(id) <= thresh, on k (see above): a voxel outside the map reads -1 and blocks
__device__ __forceinline__ bool tp_blocked(const Geo& g, const float* __restrict__ dist, int x, int y, int z, float cut) {
  if (x < 0 || y < 0 || z < 0 || x > g.nx - 1 || y > g.ny - 1 || z > g.nz - 1) return true;
  return dist[(long)x * g.nyz + (long)y * g.nz + z] <= cut;
}

// lineVisib (:252-270): the start voxel is tested, the end voxel is not; the walk itself (setInput / step) is
// ray_internal.h's
__device__ bool tp_visib(const Geo& g, const TopoArgs& T, const double* p1, const double* p2, float cut, double pc[3]) {
  RayWalk r;
  ray_set_input(r, p1[0] / g.res, p1[1] / g.res, p1[2] / g.res, p2[0] / g.res, p2[1] / g.res, p2[2] / g.res);
  // a walk that stays in the map takes fewer steps than this; one that leaves it is blocked there
  const int limit = g.nx + g.ny + g.nz + 8;
  int ix = 0, iy = 0, iz = 0;
  for (int n = 0; n < limit; ++n) {
    if (ray_at_end(r)) return true;
    ix = (int)((double)r.x + T.off[0]), iy = (int)((double)r.y + T.off[1]), iz = (int)((double)r.z + T.off[2]);
    if (tp_blocked(g, T.dist, ix, iy, iz, cut)) break;
    ray_advance(r);
  }
  pc[0] = (ix + 0.5) * g.res + g.org[0], pc[1] = (iy + 0.5) * g.res + g.org[1], pc[2] = (iz + 0.5) * g.res + g.org[2];
  return false;
}

__device__ __forceinline__ double tp_norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }
// pathLength (:417-425)
__device__ double tp_len(const double* p, int n) {
  double length = 0.0;
  for (int i = 0; i + 1 < n; ++i)
    length += tp_norm3(p[3 * i + 3] - p[3 * i], p[3 * i + 4] - p[3 * i + 1], p[3 * i + 5] - p[3 * i + 2]);
  return length;
}

// every lane's flag OR-ed (the flags of all lanes are read in lane order)
__device__ int tp_any(TShared& S, int v) {
  S.flag[threadIdx.x] = v;
  __syncthreads();
  int r = 0;
  for (int t = 0; t < TP_NT; ++t) r |= S.flag[t];
  __syncthreads();
  return r;
}

__device__ void tp_copy(double* dst, const double* src, int n) {
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * n; i += TP_NT) dst[i] = src[i];
  __syncthreads();
}

// point i of discretizePath(path, pt_num) (:427-461, path_internal.h); false: no segment found, or the point is not
// finite (a segment of length zero at the path's head divides 0 by 0)
__device__ bool tp_disc_point(const double* path, int n, const double* len, int pt_num, int i, double o[3]) {
  return path_disc_point(path, n, len, pt_num, i, o) && tp_fin3(o);
}

// sameTopoPath (:379-402): 1 / 0, or TP_UNDEF where the reference's behaviour is undefined
__device__ int tp_same_topo(const Geo& g, const TopoArgs& T, TShared& S, const double* A, int nA, const double* B, int nB,
                            float cut) {
  if (nA < 2 || nB < 2) return TP_UNDEF;  // discretizePath finds no segment
  if (nA > TP_PCAP || nB > TP_PCAP) return TP_CAP;
  __syncthreads();
  if (threadIdx.x == 0) {
    S.lenA[0] = 0.0, S.lenB[0] = 0.0;
    for (int i = 0; i < nA - 1; ++i)
      S.lenA[i + 1] = tp_norm3(A[3 * i + 3] - A[3 * i], A[3 * i + 4] - A[3 * i + 1], A[3 * i + 5] - A[3 * i + 2]) + S.lenA[i];
    for (int i = 0; i < nB - 1; ++i)
      S.lenB[i + 1] = tp_norm3(B[3 * i + 3] - B[3 * i], B[3 * i + 4] - B[3 * i + 1], B[3 * i + 5] - B[3 * i + 2]) + S.lenB[i];
  }
  __syncthreads();
  const double len1 = S.lenA[nA - 1], len2 = S.lenB[nB - 1];
  const double max_len = len1 < len2 ? len2 : len1;
  const double q = ceil(max_len / g.res);
  if (!(q < 1073741824.0)) return TP_CAP;
  const int pt_num = (int)q;
  if (pt_num < 2) return TP_UNDEF;
  int verdict = 0;  // 1: a pair is not visible, 2: a point is undefined
  for (int i = threadIdx.x; i < pt_num; i += TP_NT) {
    double a[3], b[3], pc[3];
    if (!tp_disc_point(A, nA, S.lenA, pt_num, i, a) || !tp_disc_point(B, nB, S.lenB, pt_num, i, b)) {
      verdict |= 2;
      continue;
    }
    if (!(verdict & 1) && !tp_visib(g, T, a, b, cut, pc)) verdict |= 1;
  }
  verdict = tp_any(S, verdict);
  if (verdict & 2) return TP_UNDEF;
  return (verdict & 1) ? 0 : 1;
}

// shortcutPath (:468-514) of src[n] -> dst, out_n; 0, TP_UNDEF or TP_CAP
__device__ int tp_shortcut(const Geo& g, const TopoArgs& T, TShared& S, const TWork& W, const double* src, int n, int iters,
                           double* dst, int& out_n, int& rollbacks) {
  const int tid = threadIdx.x;
  if (n > TP_PCAP) return TP_CAP;
  double* cur = W.buf;
  double* oth = W.buf + 3 * TP_PCAP;
  tp_copy(cur, src, n);
  int cn = n;
  for (int k = 0; k < iters; ++k) {
    // discretizePath(short_path) (:549-566) over discretizeLine (:533-547)
    int nd = 0;
    if (cn >= 2) {
      for (int i = 0; i < cn - 1; ++i) {
        const double p1[3] = {cur[3 * i], cur[3 * i + 1], cur[3 * i + 2]};
        const double dir[3] = {cur[3 * i + 3] - p1[0], cur[3 * i + 4] - p1[1], cur[3 * i + 5] - p1[2]};
        const double q = ceil(tp_norm3(dir[0], dir[1], dir[2]) / g.res);
        if (!(q < 1073741824.0)) return TP_CAP;
        const int seg_num = (int)q;
        if (seg_num <= 0) continue;
        // every segment but the last loses its end point to pop_back
        const int count = i != cn - 2 ? seg_num : seg_num + 1;
        if (nd + count > TP_DCAP) return TP_CAP;
        for (int j = tid; j < count; j += TP_NT)
          for (int c = 0; c < 3; ++c) W.dis[3 * (nd + j) + c] = p1[c] + dir[c] * double(j) / double(seg_num);
        nd += count;
      }
    }
    __syncthreads();
    if (nd < 2) {  // short_paths_[path_id] = dis_path
      tp_copy(dst, W.dis, nd);
      out_n = nd;
      return 0;
    }
    // visibility path shortening
    if (tid == 0)
      for (int c = 0; c < 3; ++c) oth[c] = W.dis[c];
    __syncthreads();
    int on = 1;
    int i = 1;
    while (i < nd) {
      const int j = i + tid;
      double pc[3] = {0.0, 0.0, 0.0};
      int blocked = 0;
      if (j < nd) blocked = tp_visib(g, T, oth + 3 * (on - 1), W.dis + 3 * j, T.cut_res, pc) ? 0 : 1;
      S.flag[tid] = blocked;
      __syncthreads();
      int f = -1;
      for (int t = 0; t < TP_NT; ++t)
        if (S.flag[t]) {
          f = t;
          break;
        }
      __syncthreads();
      if (f < 0) {
        i += TP_NT;
        continue;
      }
      if (on + 2 > TP_PCAP) return TP_CAP;  // this point and dis_path.back()
      if (tid == f) {
        double grad[3];
        dist_with_grad_dev(g, T.dist, pc, grad);  // SDFMap::getDistWithGrad: only the gradient is used
        const double gn = tp_norm3(grad[0], grad[1], grad[2]);
        if (gn > 1e-3) {
          for (int c = 0; c < 3; ++c) grad[c] /= gn;
          double dir[3];
          for (int c = 0; c < 3; ++c) dir[c] = W.dis[3 * j + c] - oth[3 * (on - 1) + c];
          const double dn = tp_norm3(dir[0], dir[1], dir[2]);
          for (int c = 0; c < 3; ++c) dir[c] /= dn;
          const double dot = grad[0] * dir[0] + grad[1] * dir[1] + grad[2] * dir[2];
          double push[3];
          for (int c = 0; c < 3; ++c) push[c] = grad[c] - dot * dir[c];
          const double pn = tp_norm3(push[0], push[1], push[2]);
          for (int c = 0; c < 3; ++c) push[c] /= pn;
          for (int c = 0; c < 3; ++c) pc[c] = pc[c] + g.res * push[c];
        }
        for (int c = 0; c < 3; ++c) oth[3 * on + c] = pc[c];
        S.code = tp_fin3(pc) ? 0 : 1;  // a push direction of length zero: the reference walks its next ray from NaN
      }
      __syncthreads();
      if (S.code) return TP_UNDEF;
      ++on;
      i += f + 1;
    }
    if (on + 1 > TP_PCAP) return TP_CAP;
    if (tid == 0)
      for (int c = 0; c < 3; ++c) oth[3 * on + c] = W.dis[3 * (nd - 1) + c];
    ++on;
    __syncthreads();
    // break if no shortcut
    const double len1 = tp_len(cur, cn), len2 = tp_len(oth, on);
    if (len2 > len1) {
      ++rollbacks;
      break;
    }
    double* t = cur;
    cur = oth, oth = t;
    cn = on;
  }
  tp_copy(dst, cur, cn);
  out_n = cn;
  return 0;
}

// pruneEquivalent (:301-337) over `count` paths of TP_PCAP points each: W.exist / the return value; < 0: TP_UNDEF, TP_CAP
__device__ int tp_prune_equivalent(const Geo& g, const TopoArgs& T, TShared& S, const TWork& W, const double* paths,
                                   const int* lens, int count) {
  if (count < 1) return 0;
  __syncthreads();
  if (threadIdx.x == 0) W.exist[0] = 0;
  __syncthreads();
  int ne = 1;
  for (int i = 1; i < count; ++i) {
    bool new_path = true;
    for (int j = 0; j < ne; ++j) {
      const int e = W.exist[j];
      const int same = tp_same_topo(g, T, S, paths + (size_t)i * TP_PCAP * 3, lens[i], paths + (size_t)e * TP_PCAP * 3, lens[e],
                                    T.cut_zero);
      if (same < 0) return same;
      if (same) {
        new_path = false;
        break;
      }
    }
    if (new_path) {
      if (threadIdx.x == 0) W.exist[ne] = i;
      ++ne;
      __syncthreads();
    }
  }
  return ne;
}

// a path set's rows out: lens in full, points up to max_path_points; true: a row was cut
__device__ bool tp_put_paths(const TopoArgs& T, double* out, int* out_len, int b, int cap, const double* paths, const int* lens,
                             const int* pick, int count) {
  const int mpp = T.cfg.max_path_points;
  bool over = false;
  for (int r = 0; r < count; ++r) {
    const int src = pick ? pick[r] : r;
    const int n = lens[src];
    over = over || n > mpp;
    if (out_len && threadIdx.x == 0) out_len[(size_t)b * cap + r] = n;
    if (out)
      for (int i = threadIdx.x; i < 3 * min(n, mpp); i += TP_NT)
        out[((size_t)b * cap + r) * mpp * 3 + i] = paths[(size_t)src * TP_PCAP * 3 + i];
  }
  if (out_len)
    for (int r = count + threadIdx.x; r < cap; r += TP_NT) out_len[(size_t)b * cap + r] = 0;
  return over;
}

__global__ void __launch_bounds__(TP_NT) k_topo_path(Geo g, TopoArgs T) {
  __shared__ TShared S;
  const int tid = threadIdx.x, b = blockIdx.x;
  const fuelmi_topo_cfg& cfg = T.cfg;
  const size_t nc = (size_t)T.nc, bz = (size_t)b;
  const int R1 = cfg.max_raw_path, R2 = cfg.max_raw_path2, RS = cfg.reserve_num;
  TWork W;
  W.node_pos = T.node_pos + bz * nc * 3;
  W.node_type = T.node_type + bz * nc, W.alive = T.alive + bz * nc, W.on_stack = T.on_stack + bz * nc;
  W.nb = T.nb + bz * nc * TP_NB;
  W.nb_cnt = T.nb_cnt + bz * nc, W.guards = T.guards + bz * nc, W.dfs_node = T.dfs_node + bz * nc, W.dfs_it = T.dfs_it + bz * nc;
  W.raw_nodes = T.raw_nodes + bz * R1 * TP_RAWN;
  W.raw_len = T.raw_len + bz * R1;
  W.kept = T.kept + bz * R2, W.exist = T.exist + bz * (R2 > RS ? R2 : RS), W.avail = T.avail + bz * R2;
  W.shortp = T.shortp + bz * R2 * TP_PCAP * 3;
  W.short_len = T.short_len + bz * R2;
  W.selp = T.selp + bz * RS * TP_PCAP * 3;
  W.sel_len = T.sel_len + bz * RS;
  W.buf = T.buf + bz * 2 * TP_PCAP * 3;
  W.dis = T.dis + bz * TP_DCAP * 3;

  int status = FUELMI_TOPO_OK;
  bool over = false;       // an output row was cut
  bool graph_out = false;  // the graph has been written
  int ev_reject = 0, ev_guard = 0, ev_conn = 0, ev_moved = 0, ev_three = 0, ev_roll = 0;
  int n_found = 0, n_kept = 0, n_filt = 0, n_sel = 0;
  int n_nodes = 2, n_guards = 2;
  int err = 0;

  const double* in = T.in + bz * 6;
  const double start[3] = {in[0], in[1], in[2]}, end[3] = {in[3], in[4], in[5]};

  // ---- createGraph (:100-188)
  const double diff[3] = {end[0] - start[0], end[1] - start[1], end[2] - start[2]};
  const double r0 = 0.5 * tp_norm3(diff[0], diff[1], diff[2]) + cfg.sample_inflate[0];
  const double r1 = cfg.sample_inflate[1], r2 = cfg.sample_inflate[2];
  const double tr[3] = {0.5 * (start[0] + end[0]), 0.5 * (start[1] + end[1]), 0.5 * (start[2] + end[2])};
  double xtf[3] = {end[0] - tr[0], end[1] - tr[1], end[2] - tr[2]};
  {
    const double n = tp_norm3(xtf[0], xtf[1], xtf[2]);
    for (int k = 0; k < 3; ++k) xtf[k] /= n;
  }
  // ytf = xtf.cross(downward(0, 0, -1)).normalized(), ztf = xtf.cross(ytf)
  double ytf[3] = {xtf[1] * -1.0 - xtf[2] * 0.0, xtf[2] * 0.0 - xtf[0] * -1.0, xtf[0] * 0.0 - xtf[1] * 0.0};
  {
    const double n = tp_norm3(ytf[0], ytf[1], ytf[2]);
    for (int k = 0; k < 3; ++k) ytf[k] /= n;
  }
  const double ztf[3] = {xtf[1] * ytf[2] - xtf[2] * ytf[1], xtf[2] * ytf[0] - xtf[0] * ytf[2], xtf[0] * ytf[1] - xtf[1] * ytf[0]};
  if (!tp_fin3(xtf) || !tp_fin3(ytf) || !tp_fin3(ztf)) err = TP_UNDEF;  // a vertical start -> end: every sample is NaN

  if (tid == 0) {
    for (int k = 0; k < 3; ++k) W.node_pos[k] = start[k], W.node_pos[3 + k] = end[k];
    for (int n = 0; n < 2; ++n) W.node_type[n] = 1, W.alive[n] = 1, W.nb_cnt[n] = 0, W.guards[n] = n;
  }
  const double* smp = T.samples + bz * (size_t)cfg.max_sample_num * 3;
  for (int s = 0; s < cfg.max_sample_num && !err; ++s) {
    __syncthreads();
    // getSample (:240-250)
    const double l0 = smp[3 * s] * r0, l1 = smp[3 * s + 1] * r1, l2 = smp[3 * s + 2] * r2;
    double pt[3];
    for (int k = 0; k < 3; ++k) pt[k] = ((xtf[k] * l0 + ytf[k] * l1) + ztf[k] * l2) + tr[k];
    {  // evaluateCoarseEDT(pt) <= clearance
      int id[3];
      pos_to_idx(g, pt, id);
      if (tp_blocked(g, T.dist, id[0], id[1], id[2], T.cut_clear)) {
        ++ev_reject;
        continue;
      }
    }
    // findVisibGuard (:190-208)
    int nvis = 0, v0 = -1, v1 = -1;
    for (int base = 0; base < n_guards && nvis < 3; base += TP_NT) {
      int vis = 0;
      if (base + tid < n_guards) {
        double pc[3];
        vis = tp_visib(g, T, pt, W.node_pos + 3 * W.guards[base + tid], T.cut_res, pc) ? 1 : 0;
      }
      S.flag[tid] = vis;
      __syncthreads();
      for (int t = 0; t < TP_NT && nvis < 3; ++t)
        if (S.flag[t]) {
          if (nvis == 0) v0 = W.guards[base + t];
          if (nvis == 1) v1 = W.guards[base + t];
          ++nvis;
        }
      __syncthreads();
    }
    if (nvis == 0) {
      __syncthreads();
      if (tid == 0) {
        for (int k = 0; k < 3; ++k) W.node_pos[3 * n_nodes + k] = pt[k];
        W.node_type[n_nodes] = 1, W.alive[n_nodes] = 1, W.nb_cnt[n_nodes] = 0;
        W.guards[n_guards] = n_nodes;
      }
      ++n_nodes, ++n_guards, ++ev_guard;
    } else if (nvis == 2) {
      // needConnection (:210-238)
      bool need = true;
      const int c0 = W.nb_cnt[v0], c1 = W.nb_cnt[v1];
      for (int i = 0; i < c0 && need && !err; ++i)
        for (int j = 0; j < c1; ++j) {
          const int c = W.nb[(size_t)v0 * TP_NB + i];
          if (c != W.nb[(size_t)v1 * TP_NB + j]) continue;
          __syncthreads();
          if (tid == 0)
            for (int k = 0; k < 3; ++k) {
              S.tri[0][k] = W.node_pos[3 * v0 + k], S.tri[0][3 + k] = pt[k], S.tri[0][6 + k] = W.node_pos[3 * v1 + k];
              S.tri[1][k] = W.node_pos[3 * v0 + k], S.tri[1][3 + k] = W.node_pos[3 * c + k], S.tri[1][6 + k] = W.node_pos[3 * v1 + k];
            }
          __syncthreads();
          const int same = tp_same_topo(g, T, S, S.tri[0], 3, S.tri[1], 3, T.cut_zero);
          if (same < 0) {
            err = same;
            break;
          }
          if (same) {
            if (tp_len(S.tri[0], 3) < tp_len(S.tri[1], 3)) {  // the shorter connection moves the connector
              __syncthreads();
              if (tid == 0)
                for (int k = 0; k < 3; ++k) W.node_pos[3 * c + k] = pt[k];
              ++ev_moved;
            }
            need = false;
            break;
          }
        }
      if (need && !err) {
        if (c0 >= TP_NB || c1 >= TP_NB) {
          err = TP_CAP;
        } else {
          __syncthreads();  // every lane has walked the two neighbour lists lane 0 is about to extend
          if (tid == 0) {
            for (int k = 0; k < 3; ++k) W.node_pos[3 * n_nodes + k] = pt[k];
            W.node_type[n_nodes] = 2, W.alive[n_nodes] = 1, W.nb_cnt[n_nodes] = 2;
            W.nb[(size_t)v0 * TP_NB + c0] = (unsigned short)n_nodes, W.nb_cnt[v0] = c0 + 1;
            W.nb[(size_t)v1 * TP_NB + c1] = (unsigned short)n_nodes, W.nb_cnt[v1] = c1 + 1;
            W.nb[(size_t)n_nodes * TP_NB] = (unsigned short)v0, W.nb[(size_t)n_nodes * TP_NB + 1] = (unsigned short)v1;
          }
          ++n_nodes, ++ev_conn;
        }
      }
    } else if (nvis == 3) {
      ++ev_three;
    }
  }

  int n_alive = 0;
  if (!err) {
    // ---- pruneGraph (:272-299), in rounds
    for (;;) {
      __syncthreads();
      int any = 0;
      for (int n = 2 + tid; n < n_nodes; n += TP_NT)
        if (W.alive[n] == 1 && W.nb_cnt[n] <= 1) W.alive[n] = 2, any = 1;
      if (!tp_any(S, any)) break;
      for (int n = tid; n < n_nodes; n += TP_NT) {
        if (W.alive[n] != 1) continue;
        const int c = W.nb_cnt[n];
        int kept = 0;
        for (int i = 0; i < c; ++i) {
          const unsigned short o = W.nb[(size_t)n * TP_NB + i];
          if (W.alive[o] == 2) continue;
          W.nb[(size_t)n * TP_NB + kept] = o;
          ++kept;
        }
        W.nb_cnt[n] = kept;
      }
      __syncthreads();
      for (int n = 2 + tid; n < n_nodes; n += TP_NT)
        if (W.alive[n] == 2) W.alive[n] = 0;
    }
    // the graph out, in list order
    if (tid == 0) {
      int at = 0, ids = 0;
      const int maxn = cfg.max_nodes;
      for (int n = 0; n < n_nodes; ++n) {
        if (!W.alive[n]) continue;
        if (at < maxn) {
          const size_t o = bz * maxn + at;
          if (T.node_id) T.node_id[o] = n;
          if (T.node_kind) T.node_kind[o] = W.node_type[n];
          if (T.node_xyz)
            for (int k = 0; k < 3; ++k) T.node_xyz[o * 3 + k] = W.node_pos[3 * n + k];
          // (a graph of n nodes has at most 4 n neighbour entries -- two a connector, each mirrored in a guard -- so the
          // ids run past their 4 max_nodes slots only in a problem that is over max_nodes as well; the offsets stop there)
          if (T.nb_off) T.nb_off[bz * (maxn + 1) + at] = min(ids, 4 * maxn);
          for (int i = 0; i < W.nb_cnt[n]; ++i, ++ids)
            if (T.nb_ids && ids < 4 * maxn) T.nb_ids[bz * 4 * maxn + ids] = W.nb[(size_t)n * TP_NB + i];
          if (T.nb_off) T.nb_off[bz * (maxn + 1) + at + 1] = min(ids, 4 * maxn);
        }
        ++at;
      }
      S.code = at;
    }
    __syncthreads();
    n_alive = S.code;
    __syncthreads();
    over = over || n_alive > cfg.max_nodes;
    graph_out = true;

    // ---- searchPaths / depthFirstSearch (:606-684)
    if (tid == 0) {
      for (int n = 0; n < n_nodes; ++n) W.on_stack[n] = 0;
      int nraw = 0, depth = 0, code = 0;
      bool stop = false;
      W.dfs_node[0] = 0, W.dfs_it[0] = -1, W.on_stack[0] = 1;
      while (depth >= 0 && !stop) {
        const int cur = W.dfs_node[depth];
        const int c = W.nb_cnt[cur];
        if (W.dfs_it[depth] < 0) {  // check reach goal
          for (int i = 0; i < c; ++i) {
            if (W.nb[(size_t)cur * TP_NB + i] != 1) continue;
            const int len = depth + 2;
            if (len >= TP_RAWN) {
              code = TP_UNDEF, stop = true;
              break;
            }
            for (int j = 0; j <= depth; ++j) W.raw_nodes[(size_t)nraw * TP_RAWN + j] = (unsigned short)W.dfs_node[j];
            W.raw_nodes[(size_t)nraw * TP_RAWN + depth + 1] = 1;
            W.raw_len[nraw] = len;
            ++nraw;
            if (nraw >= cfg.max_raw_path) stop = true;
            break;
          }
          if (stop) break;
          W.dfs_it[depth] = 0;
        }
        bool down = false;
        while (W.dfs_it[depth] < c) {
          const int nx = W.nb[(size_t)cur * TP_NB + W.dfs_it[depth]];
          W.dfs_it[depth] += 1;
          if (nx == 1 || W.on_stack[nx]) continue;
          ++depth;
          W.dfs_node[depth] = nx, W.dfs_it[depth] = -1, W.on_stack[nx] = 1;
          down = true;
          break;
        }
        if (!down) {
          W.on_stack[cur] = 0;
          --depth;
        }
      }
      // sort the path by node number, select paths with less nodes
      int nk = 0;
      if (!code) {
        int min_n = 100000, max_n = 1;
        for (int i = 0; i < nraw; ++i) {
          if (W.raw_len[i] > max_n) max_n = W.raw_len[i];
          if (W.raw_len[i] < min_n) min_n = W.raw_len[i];
        }
        bool reach_max = false;
        for (int i = min_n; i <= max_n && !reach_max; ++i)
          for (int j = 0; j < nraw; ++j) {
            if (W.raw_len[j] != i) continue;
            W.kept[nk] = j;
            ++nk;
            if (nk >= cfg.max_raw_path2) {
              reach_max = true;
              break;
            }
          }
      }
      S.flag[0] = code ? 0 : nraw, S.flag[1] = nk, S.code = code;
    }
    __syncthreads();
    n_found = S.flag[0], n_kept = S.flag[1], err = S.code;
    __syncthreads();
  }

  if (!err) {
    // ---- shortcutPaths (:516-531): raw path r -> buf (positions) -> short_paths_[r]
    double* rawp = W.buf + 3 * TP_PCAP;  // a raw path's positions: the second buffer is free until tp_shortcut copies it
    for (int r = 0; r < n_kept && !err; ++r) {
      const int src = W.kept[r], len = W.raw_len[src];
      __syncthreads();
      for (int i = tid; i < len; i += TP_NT)
        for (int k = 0; k < 3; ++k) rawp[3 * i + k] = W.node_pos[3 * W.raw_nodes[(size_t)src * TP_RAWN + i] + k];
      __syncthreads();
      over = over || len > cfg.max_path_points;
      if (T.raw_plen && tid == 0) T.raw_plen[bz * R2 + r] = len;
      if (T.raw_paths)
        for (int i = tid; i < 3 * min(len, cfg.max_path_points); i += TP_NT)
          T.raw_paths[(bz * R2 + r) * cfg.max_path_points * 3 + i] = rawp[i];
      int out_n = 0;
      err = tp_shortcut(g, T, S, W, rawp, len, 1, W.shortp + (size_t)r * TP_PCAP * 3, out_n, ev_roll);
      if (tid == 0) W.short_len[r] = out_n;
      __syncthreads();
    }
    if (T.raw_plen)
      for (int r = n_kept + tid; r < R2; r += TP_NT) T.raw_plen[bz * R2 + r] = 0;
  }
  if (!err) {
    // ---- pruneEquivalent(short_paths_)
    const int ne = tp_prune_equivalent(g, T, S, W, W.shortp, W.short_len, n_kept);
    if (ne < 0)
      err = ne;
    else
      n_filt = ne;
  }
  if (!err) {
    // ---- selectShortPaths (:339-377)
    __syncthreads();
    if (tid == 0)
      for (int i = 0; i < n_filt; ++i) W.avail[i] = W.exist[i];
    __syncthreads();
    int na = n_filt, ns = 0;
    double min_len = 0.0;
    const int nsp = T.n_spts[b], nep = T.n_epts[b];
    for (int i = 0; i < RS && na > 0 && !err; ++i) {
      int short_id = -1;  // shortestPath (:404-415)
      double best = 100000000;
      for (int a = 0; a < na; ++a) {
        const double len = tp_len(W.shortp + (size_t)W.avail[a] * TP_PCAP * 3, W.short_len[W.avail[a]]);
        if (len < best) short_id = a, best = len;
      }
      if (short_id < 0) {
        err = TP_UNDEF;  // paths[-1]
        break;
      }
      if (i == 0)
        min_len = best;
      else if (!(best / min_len < cfg.ratio_to_short))
        break;
      const int src = W.avail[short_id];
      const int len = W.short_len[src];
      if (nsp + len + nep > TP_PCAP) {
        err = TP_CAP;
        break;
      }
      // merge with start and end segment
      double* dst = W.selp + (size_t)ns * TP_PCAP * 3;
      __syncthreads();
      for (int k = tid; k < 3 * nsp; k += TP_NT) dst[k] = T.spts[bz * T.max_start * 3 + k];
      for (int k = tid; k < 3 * len; k += TP_NT) dst[3 * nsp + k] = W.shortp[(size_t)src * TP_PCAP * 3 + k];
      for (int k = tid; k < 3 * nep; k += TP_NT) dst[3 * (nsp + len) + k] = T.epts[bz * T.max_end * 3 + k];
      if (tid == 0) {
        W.sel_len[ns] = nsp + len + nep;
        for (int a = short_id; a + 1 < na; ++a) W.avail[a] = W.avail[a + 1];  // paths.erase
      }
      __syncthreads();
      --na, ++ns;
    }
    // the filtered set the caller gets back is what the selection left of it: it erases what it takes
    over = tp_put_paths(T, T.filt_paths, T.filt_plen, b, R2, W.shortp, W.short_len, W.avail, na) || over;
    for (int i = 0; i < ns && !err; ++i) {
      double* p = W.selp + (size_t)i * TP_PCAP * 3;
      int out_n = 0;
      err = tp_shortcut(g, T, S, W, p, W.sel_len[i], 5, p, out_n, ev_roll);
      __syncthreads();
      if (tid == 0) W.sel_len[i] = out_n;
      __syncthreads();
    }
    if (!err) {
      const int ne = tp_prune_equivalent(g, T, S, W, W.selp, W.sel_len, ns);
      if (ne < 0)
        err = ne;
      else
        n_sel = ne;
    }
  }
  if (!err) {
    over = tp_put_paths(T, T.sel_paths, T.sel_plen, b, RS, W.selp, W.sel_len, W.exist, n_sel) || over;
    if (T.sel_length)
      for (int r = tid; r < RS; r += TP_NT)
        T.sel_length[bz * RS + r] = r < n_sel ? tp_len(W.selp + (size_t)W.exist[r] * TP_PCAP * 3, W.sel_len[W.exist[r]]) : 0.0;
    status = n_sel == 0 ? FUELMI_TOPO_NO_PATH : FUELMI_TOPO_OK;
    if (over) status = -1;
  } else {
    // no path outputs: every length is zero.  TP_CAP: one of the kernel's own caps
    status = err == TP_UNDEF ? FUELMI_TOPO_UNDEFINED : -1;
    __syncthreads();
    for (int r = tid; r < R2; r += TP_NT) {
      if (T.raw_plen) T.raw_plen[bz * R2 + r] = 0;
      if (T.filt_plen) T.filt_plen[bz * R2 + r] = 0;
    }
    for (int r = tid; r < RS; r += TP_NT) {
      if (T.sel_plen) T.sel_plen[bz * RS + r] = 0;
      if (T.sel_length) T.sel_length[bz * RS + r] = 0.0;
    }
    n_kept = n_filt = n_sel = 0;
  }
  if (tid == 0) {
    T.status[b] = status;
    int* c = T.counts + bz * 4;
    c[0] = n_found, c[1] = n_kept, c[2] = n_filt, c[3] = n_sel;
    int* e = T.events + bz * 6;
    e[0] = ev_reject, e[1] = ev_guard, e[2] = ev_conn, e[3] = ev_moved, e[4] = ev_three, e[5] = ev_roll;
    if (T.n_nodes) T.n_nodes[b] = graph_out ? n_alive : 0;
  }
}

// the largest k for which the reference's f64 `res * sqrt(k) <= thresh` holds, as an f32 cut between the device's
// values for k and k + 1 (esdf.hip: f32 res times an approximate f32 square root, a few ulp from either)
float topo_cut(double res, double thresh) { return field_cut(res, thresh, false); }  // (path_internal.h)

// the workspace of n problems, carved from `base` (null: the sizing pass)
size_t topo_workspace(const fuelmi_topo_cfg* cfg, size_t n, unsigned char* base, TopoArgs* T) {
  TopoArgs dummy;
  TopoArgs& A = T ? *T : dummy;
  const size_t nc = (size_t)cfg->max_sample_num + 2, r1 = (size_t)cfg->max_raw_path, r2 = (size_t)cfg->max_raw_path2,
               rs = (size_t)cfg->reserve_num;
  BlockLayout L(base, 256);
  A.node_pos = L.take<double>(n * nc * 3);
  A.shortp = L.take<double>(n * r2 * TP_PCAP * 3);
  A.selp = L.take<double>(n * rs * TP_PCAP * 3);
  A.buf = L.take<double>(n * 2 * TP_PCAP * 3);
  A.dis = L.take<double>(n * TP_DCAP * 3);
  A.nb_cnt = L.take<int>(n * nc);
  A.guards = L.take<int>(n * nc);
  A.dfs_node = L.take<int>(n * nc);
  A.dfs_it = L.take<int>(n * nc);
  A.raw_len = L.take<int>(n * r1);
  A.kept = L.take<int>(n * r2);
  A.exist = L.take<int>(n * std::max(r2, rs));
  A.avail = L.take<int>(n * r2);
  A.short_len = L.take<int>(n * r2);
  A.sel_len = L.take<int>(n * rs);
  A.nb = L.take<unsigned short>(n * nc * TP_NB);
  A.raw_nodes = L.take<unsigned short>(n * r1 * TP_RAWN);
  A.node_type = L.take<unsigned char>(n * nc);
  A.alive = L.take<unsigned char>(n * nc);
  A.on_stack = L.take<unsigned char>(n * nc);
  return L.size();
}

bool fin(double x) { return std::isfinite(x); }

int topo_check_cfg(const fuelmi_topo_cfg* cfg) {
  ARGCHK(cfg);
  for (int k = 0; k < 3; ++k) ARGCHK(fin(cfg->sample_inflate[k]) && std::fabs(cfg->sample_inflate[k]) < 1e7);
  ARGCHK(fin(cfg->clearance) && cfg->clearance >= 0.0 && fin(cfg->ratio_to_short));
  ARGCHK(cfg->max_sample_num >= 0 && cfg->max_raw_path >= 1 && cfg->max_raw_path2 >= 1 && cfg->reserve_num >= 1);
  ARGCHK(cfg->max_path_points >= 1 && cfg->max_nodes >= 2);
  if (cfg->max_sample_num > FUELMI_TOPO_MAX_SAMPLES || cfg->max_raw_path > FUELMI_TOPO_MAX_RAW ||
      cfg->max_raw_path2 > FUELMI_TOPO_MAX_RAW || cfg->reserve_num > FUELMI_TOPO_MAX_RAW ||
      cfg->max_path_points > FUELMI_TOPO_MAX_PATH_POINTS || cfg->max_nodes > FUELMI_TOPO_MAX_SAMPLES + 2) {
    fuelmi_set_error("topological search: max_sample_num %d / max_raw_path %d / max_raw_path2 %d / reserve_num %d / "
                     "max_path_points %d / max_nodes %d exceed %d / %d / %d / %d / %d / %d", cfg->max_sample_num,
                     cfg->max_raw_path, cfg->max_raw_path2, cfg->reserve_num, cfg->max_path_points, cfg->max_nodes,
                     FUELMI_TOPO_MAX_SAMPLES, FUELMI_TOPO_MAX_RAW, FUELMI_TOPO_MAX_RAW, FUELMI_TOPO_MAX_RAW,
                     FUELMI_TOPO_MAX_PATH_POINTS, FUELMI_TOPO_MAX_SAMPLES + 2);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

}  // namespace

extern "C" int fuelmi_topo_plan(const fuelmi_topo_cfg* cfg, long long out[12]) {
  ARGCHK(out);
  {
    const int rc = topo_check_cfg(cfg);
    if (rc) return rc;
  }
  out[0] = TP_NT, out[1] = (long long)sizeof(TShared), out[2] = (long long)topo_workspace(cfg, 1, nullptr, nullptr);
  out[3] = TP_NT;  // the guard chunk
  out[4] = FUELMI_TOPO_MAX_SAMPLES, out[5] = FUELMI_TOPO_MAX_RAW, out[6] = FUELMI_TOPO_MAX_PATH_POINTS;
  out[7] = FUELMI_TOPO_MAX_DIS_POINTS, out[8] = FUELMI_TOPO_MAX_NEIGHBORS, out[9] = TP_RAWN;
  out[10] = FUELMI_TOPO_MAX_POINTS_IN, out[11] = (long long)FUELMI_TOPO_MAX_WORKSPACE;
  return FUELMI_OK;
}

extern "C" long long fuelmi_map_topo_pool_bytes(const fuelmi_map* m) { return m ? (long long)m->topo_dev.bytes : -1; }

extern "C" int fuelmi_map_topo_paths(fuelmi_map* m, const fuelmi_topo_cfg* cfg, int n_prob, const double* start_xyz,
                                     const double* end_xyz, int max_start, const int* n_start, const double* start_pts,
                                     int max_end, const int* n_end, const double* end_pts, const double* samples,
                                     int* status, int* counts, int* events, int* n_nodes, int* node_id, int* node_type,
                                     double* node_xyz, int* nb_off, int* nb_ids, double* raw_paths, int* raw_len,
                                     double* filt_paths, int* filt_len, double* sel_paths, int* sel_len,
                                     double* sel_length) {
  {  // every argument on the host, before the map is touched
    const int rc = topo_check_cfg(cfg);
    if (rc) return rc;
  }
  ARGCHK(n_prob >= 0 && max_start >= 0 && max_end >= 0);
  if (max_start > FUELMI_TOPO_MAX_POINTS_IN || max_end > FUELMI_TOPO_MAX_POINTS_IN) {
    fuelmi_set_error("topological search: max_start %d / max_end %d exceed %d", max_start, max_end, FUELMI_TOPO_MAX_POINTS_IN);
    return FUELMI_ELIMIT;
  }
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(start_xyz && end_xyz && status && counts && events);
  ARGCHK(cfg->max_sample_num == 0 || samples);
  ARGCHK((max_start == 0 || (n_start && start_pts)) && (max_end == 0 || (n_end && end_pts)));
  const size_t n = (size_t)n_prob, S = (size_t)cfg->max_sample_num, ms = (size_t)max_start, me = (size_t)max_end;
  for (size_t b = 0; b < n; ++b) {
    for (int k = 0; k < 3; ++k) {
      const double s = start_xyz[3 * b + k], e = end_xyz[3 * b + k];
      ARGCHK(fin(s) && fin(e) && std::fabs(s) < 1e7 && std::fabs(e) < 1e7);
    }
    const int ns = max_start ? n_start[b] : 0, ne = max_end ? n_end[b] : 0;
    ARGCHK(ns >= 0 && ns <= max_start && ne >= 0 && ne <= max_end);
    for (size_t k = 0; k < 3 * (size_t)ns; ++k) ARGCHK(fin(start_pts[b * ms * 3 + k]) && std::fabs(start_pts[b * ms * 3 + k]) < 1e7);
    for (size_t k = 0; k < 3 * (size_t)ne; ++k) ARGCHK(fin(end_pts[b * me * 3 + k]) && std::fabs(end_pts[b * me * 3 + k]) < 1e7);
    for (size_t k = 0; k < 3 * S; ++k) ARGCHK(samples[b * S * 3 + k] >= -1.0 && samples[b * S * 3 + k] < 1.0);
  }
  {
    const double total = (double)n * (double)topo_workspace(cfg, 1, nullptr, nullptr);
    if (total > FUELMI_TOPO_MAX_WORKSPACE) {
      fuelmi_set_error("topological search: %d problems x %zu bytes of workspace exceed %.0f bytes", n_prob,
                       topo_workspace(cfg, 1, nullptr, nullptr), FUELMI_TOPO_MAX_WORKSPACE);
      return FUELMI_ELIMIT;
    }
  }
  ARGCHK(m);  // what follows needs the map's resolution
  const double res = m->g.res;
  ARGCHK(1e8 / res < 2147483648.0);  // every voxel index of a sample or a pushed point fits an int
  ARGCHK(cfg->clearance / res < 1000.0);
  for (size_t b = 0; b < n; ++b) {
    double d2 = 0.0;
    for (int k = 0; k < 3; ++k) d2 += (end_xyz[3 * b + k] - start_xyz[3 * b + k]) * (end_xyz[3 * b + k] - start_xyz[3 * b + k]);
    ARGCHK(std::sqrt(d2) > res);
  }
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const size_t maxn = (size_t)cfg->max_nodes, mpp = (size_t)cfg->max_path_points, r2 = (size_t)cfg->max_raw_path2,
               rs = (size_t)cfg->reserve_num;
  TopoArgs T;
  memset(&T, 0, sizeof(T));
  ResultBlock R(256);  // everything behind events only where the caller asks
  R.add(T.status, status, n);
  R.add(T.counts, counts, n * 4);
  R.add(T.events, events, n * 6);
  R.opt(T.n_nodes, n_nodes, n);
  R.opt(T.node_id, node_id, n * maxn);
  R.opt(T.node_kind, node_type, n * maxn);
  R.opt(T.node_xyz, node_xyz, n * maxn * 3);
  R.opt(T.nb_off, nb_off, n * (maxn + 1));
  R.opt(T.nb_ids, nb_ids, n * 4 * maxn);
  R.opt(T.raw_paths, raw_paths, n * r2 * mpp * 3);
  R.opt(T.raw_plen, raw_len, n * r2);
  R.opt(T.filt_paths, filt_paths, n * r2 * mpp * 3);
  R.opt(T.filt_plen, filt_len, n * r2);
  R.opt(T.sel_paths, sel_paths, n * rs * mpp * 3);
  R.opt(T.sel_plen, sel_len, n * rs);
  R.opt(T.sel_length, sel_length, n * rs);
  ARGCHK(!R.overflow);
  // the block: results | inputs | workspace
  double *d_in, *d_sp, *d_ep, *d_smp;
  int *d_nsp, *d_nep;
  size_t in_at = 0, in_bytes = 0;
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 256);
    R.place(L);
    in_at = L.size();
    d_in = L.take<double>(n * 6);
    d_sp = L.take<double>(n * ms * 3 + 1);
    d_ep = L.take<double>(n * me * 3 + 1);
    d_smp = L.take<double>(n * S * 3 + 1);
    d_nsp = L.take<int>(n);
    d_nep = L.take<int>(n);
    in_bytes = L.size() - in_at;
    const size_t head = L.size();
    return head + topo_workspace(cfg, n, base ? base + head : nullptr, &T);
  };
  {
    const int rc = m->topo_dev.carve(st, layout);
    if (rc) return rc;
  }
  unsigned char* base = m->topo_dev.base();
  // the inputs, staged in the map: the source must outlive the copy
  std::vector<unsigned char>& hin = m->topo_host;
  hin.assign(in_bytes, 0);
  auto stage = [&](const void* dev) { return hin.data() + (static_cast<const unsigned char*>(dev) - (base + in_at)); };
  {
    double* hi = reinterpret_cast<double*>(stage(d_in));
    for (size_t b = 0; b < n; ++b)
      for (int k = 0; k < 3; ++k) hi[6 * b + k] = start_xyz[3 * b + k], hi[6 * b + 3 + k] = end_xyz[3 * b + k];
    int* hs = reinterpret_cast<int*>(stage(d_nsp));
    int* he = reinterpret_cast<int*>(stage(d_nep));
    double* hsp = reinterpret_cast<double*>(stage(d_sp));
    double* hep = reinterpret_cast<double*>(stage(d_ep));
    for (size_t b = 0; b < n; ++b) {
      hs[b] = max_start ? n_start[b] : 0, he[b] = max_end ? n_end[b] : 0;
      for (size_t k = 0; k < 3 * (size_t)hs[b]; ++k) hsp[b * ms * 3 + k] = start_pts[b * ms * 3 + k];
      for (size_t k = 0; k < 3 * (size_t)he[b]; ++k) hep[b * me * 3 + k] = end_pts[b * me * 3 + k];
    }
    if (S) memcpy(stage(d_smp), samples, n * S * 3 * sizeof(double));
  }
  HIPCHK(hipMemcpyAsync(base + in_at, hin.data(), in_bytes, hipMemcpyHostToDevice, st));
  T.cfg = *cfg;
  T.n_prob = n_prob, T.max_start = max_start, T.max_end = max_end, T.nc = cfg->max_sample_num + 2;
  T.cut_res = topo_cut(res, res), T.cut_zero = topo_cut(res, 0.0), T.cut_clear = topo_cut(res, cfg->clearance);
  for (int k = 0; k < 3; ++k) T.off[k] = 0.5 - m->g.org[k] / res;
  T.dist = m->dist;
  T.in = d_in, T.spts = d_sp, T.epts = d_ep, T.n_spts = d_nsp, T.n_epts = d_nep, T.samples = d_smp;
  hipLaunchKernelGGL(k_topo_path, dim3(n_prob), dim3(TP_NT), 0, st, m->g, T);
  HIPCHK(hipGetLastError());
  {
    const int rc = result_fetch(R, st);
    if (rc) return rc;
  }
  const int b = first_over_limit(status, n_prob);
  if (b < 0) return FUELMI_OK;
  fuelmi_set_error("topological search: problem %d is over max_nodes = %d / max_path_points = %d or one of the "
                   "kernel's caps (fuelmi_topo_plan)", b, cfg->max_nodes, cfg->max_path_points);
  return FUELMI_ELIMIT;
}
