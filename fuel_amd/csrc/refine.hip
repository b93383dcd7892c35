// refine.hip -- FastExplorationManager::refineLocalTour (exploration_manager/src/fast_exploration_manager.cpp:429-503)
// and its single-destination branch (:185-220) for a batch of problems.
//
// The edges' searchPath lengths come from the path engine (path_cost_enqueue, all problems' edges in one run, sources
// shared bitwise); k_refine then prices every edge with ViewNode::computeCost (graph_node.cpp:63-88) and runs
// GraphSearch::DijkstraSearch (graph_search.h) as the layer-by-layer min-plus pass it amounts to on a layered graph
// with costs >= 0.  One 256-lane workgroup per problem: per layer, wave w takes nodes v = w, w + 4, ...; its lanes
// take the predecessors u = lane, lane + 64, ... and reduce with the key (total, g(u), u) -- the first predecessor
// Dijkstra would pop among the cheapest.  g and the parents stay in LDS; one lane picks the goal and backtracks.
// The refined-tour polyline is one more engine run on the host's leg list.
#include <climits>
#include <cmath>
#include <vector>

#include "fuelmi_internal.h"

namespace {

constexpr int RF_LAYERS = FUELMI_REFINE_MAX_LAYERS, RF_NODES = FUELMI_REFINE_MAX_NODES;
static_assert(RF_NODES <= 256, "parents are stored as bytes");
constexpr double G_INIT = 1000000.0;      // BaseNode::g_value_ (graph_node.h:31)
constexpr double ARGMIN_INIT = 100000.0;  // min_cost of the single-destination branch (:199)

struct RArgs {
  const double* start;    // [B][7]
  const int* layer_ptr;   // [B + 1]
  const int* node_ptr;    // [layers + 1]
  const double* nodes;    // [N][4]
  const int* edge_off;    // [layers]: first edge of layer l's block, slot u * nv + v
  const double* length;   // [edges] searchPath lengths (path engine scratch)
  const int* kind;        // [edges]
  double vm, yd, w_dir;
  int last_argmin;
  int* choice;            // [layers]
  double* cost;           // [B]
  int* err;               // a predecessor chain the engine could not close
};

__device__ __forceinline__ double dnorm3(double a, double b, double c) { return sqrt(a * a + b * b + c * c); }

// ViewNode::computeCost with the length known, in FrontierFinder::hostCost's operation order (left-to-right sums);
// normalized() as real Eigen: a zero vector stays zero (acos(0) = pi / 2)
__device__ __forceinline__ double edge_cost(const RArgs& R, double len, const double* p1, const double* p2, double y1,
                                            double y2, bool dir_term, const double vd[3]) {
  double pos_cost = len / R.vm;
  if (dir_term) {
    double d[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double z = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (z > 0.0) {
      const double nz = sqrt(z);
      d[0] /= nz, d[1] /= nz, d[2] /= nz;
    }
    const double diff = acos(vd[0] * d[0] + vd[1] * d[1] + vd[2] * d[2]);
    pos_cost += R.w_dir * diff;
  }
  double diff = fabs(y2 - y1);
  const double other = 2 * M_PI - diff;
  diff = other < diff ? other : diff;  // std::min
  const double yaw_cost = diff / R.yd;
  return pos_cost < yaw_cost ? yaw_cost : pos_cost;  // std::max: a NaN pos_cost stays NaN
}

// key (total, g(u), u); u < 0: no candidate
__device__ __forceinline__ bool better(double t, double g, int u, double bt, double bg, int bu) {
  if (u < 0) return false;
  if (bu < 0) return true;
  return t < bt || (t == bt && (g < bg || (g == bg && u < bu)));
}

__global__ void __launch_bounds__(256) k_refine(RArgs R) {
  __shared__ double g_l[2][RF_NODES];
  __shared__ unsigned char par[RF_LAYERS][RF_NODES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l0 = R.layer_ptr[b], L = R.layer_ptr[b + 1] - l0;
  const double* S = R.start + 7 * (size_t)b;
  // only the start has a velocity (every other ViewNode: vel_ = 0, graph_node.cpp:21)
  const double sn = dnorm3(S[3], S[4], S[5]);
  const bool dir_term = sn > 1e-3;
  const double vd[3] = {S[3] / sn, S[4] / sn, S[5] / sn};
  if (tid == 0) g_l[0][0] = 0.0;
  __syncthreads();
  int nu = 1, nv = 1;
  for (int li = 0; li < L; ++li) {
    const int l = l0 + li;
    const int nb = R.node_ptr[l];
    nv = R.node_ptr[l + 1] - nb;
    if (li == L - 1 && !R.last_argmin) nv = 1;  // :459-462
    const double* gp = g_l[li & 1];
    double* gc = g_l[(li + 1) & 1];
    const int pb = li == 0 ? 0 : R.node_ptr[l - 1];
    const int eb = R.edge_off[l];
    for (int v = wave; v < nv; v += 4) {
      const double* V = R.nodes + 4 * (size_t)(nb + v);
      double bt = 0.0, bg = 0.0;
      int bu = -1;
      for (int u = lane; u < nu; u += 64) {
        const double* U = li == 0 ? S : R.nodes + 4 * (size_t)(pb + u);
        const double yu = li == 0 ? S[6] : U[3];
        const int e = eb + u * nv + v;
        if (R.kind[e] < 0) atomicOr(R.err, 1);
        const double gu = gp[u];
        const double t = gu + edge_cost(R, R.length[e], U, V, yu, V[3], li == 0 && dir_term, vd);
        if (t < G_INIT && better(t, gu, u, bt, bg, bu)) bt = t, bg = gu, bu = u;
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double ot = __shfl_xor(bt, off), og = __shfl_xor(bg, off);
        const int ou = __shfl_xor(bu, off);
        if (better(ot, og, ou, bt, bg, bu)) bt = ot, bg = og, bu = ou;
      }
      if (lane == 0) {
        gc[v] = bu >= 0 ? bt : G_INIT;
        par[li][v] = (unsigned char)(bu >= 0 ? bu : 0);
      }
    }
    __syncthreads();
    nu = nv;
  }
  if (tid != 0) return;
  const double* gl = g_l[L & 1];
  int goal = -1;
  if (R.last_argmin) {  // :199-208: the first strictly cheapest below 100000
    double best = ARGMIN_INIT;
    for (int v = 0; v < nv; ++v)
      if (gl[v] < best) best = gl[v], goal = v;
  } else if (gl[0] < G_INIT) {
    goal = 0;
  }
  if (goal < 0) {
    R.cost[b] = __builtin_huge_val();
    for (int li = 0; li < L; ++li) R.choice[l0 + li] = -1;
    return;
  }
  R.cost[b] = gl[goal];
  int v = goal;
  for (int li = L - 1; li >= 0; --li) {
    R.choice[l0 + li] = v;
    v = par[li][v];
  }
}

bool finite_below(double x, double lim) { return std::isfinite(x) && std::fabs(x) < lim; }

}  // namespace

extern "C" int fuelmi_map_refine_tours(fuelmi_map* m, const fuelmi_refine_cfg* cfg, int n_prob, const double* start,
                                       const int* layer_ptr, const int* node_ptr, const double* nodes, int* choice,
                                       double* cost, int* tour_len, double* tour_xyz) {
  // every argument and limit on the host, before the map is touched
  ARGCHK(cfg);
  ARGCHK(n_prob >= 0);
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(start && layer_ptr && node_ptr && nodes && choice && cost);
  const fuelmi_path_cfg& pc = cfg->path;
  ARGCHK(pc.lattice_res > 0.0 && pc.edge_step > 0.0 && std::isfinite(pc.lattice_res) && std::isfinite(pc.edge_step));
  ARGCHK(std::isfinite(pc.no_path_cost));
  ARGCHK(cfg->vm > 0.0 && cfg->yd > 0.0 && std::isfinite(cfg->vm) && std::isfinite(cfg->yd) && std::isfinite(cfg->w_dir));
  ARGCHK(std::isfinite(cfg->tour_lattice_res));
  const bool polyline = cfg->tour_lattice_res > 0.0 && tour_len;
  ARGCHK(!polyline || !tour_xyz || cfg->max_tour_points >= 1);
  ARGCHK(layer_ptr[0] == 0 && node_ptr[0] == 0);
  for (int b = 0; b < n_prob; ++b) {
    const int nl = layer_ptr[b + 1] - layer_ptr[b];
    if (nl < 1) {
      fuelmi_set_error("refine: problem %d has no layers", b);
      return FUELMI_EINVAL;
    }
    if (nl > FUELMI_REFINE_MAX_LAYERS) {
      fuelmi_set_error("refine: problem %d has %d layers, more than %d", b, nl, FUELMI_REFINE_MAX_LAYERS);
      return FUELMI_ELIMIT;
    }
  }
  const int n_layers = layer_ptr[n_prob];
  std::vector<int> edge_off(n_layers);
  long long edges = 0;
  for (int b = 0; b < n_prob; ++b) {
    int nu = 1;
    for (int l = layer_ptr[b]; l < layer_ptr[b + 1]; ++l) {
      int nv = node_ptr[l + 1] - node_ptr[l];
      if (nv < 1) {
        fuelmi_set_error("refine: layer %d of problem %d has no nodes", l - layer_ptr[b], b);
        return FUELMI_EINVAL;
      }
      if (nv > FUELMI_REFINE_MAX_NODES) {
        fuelmi_set_error("refine: layer %d of problem %d has %d nodes, more than %d", l - layer_ptr[b], b, nv,
                         FUELMI_REFINE_MAX_NODES);
        return FUELMI_ELIMIT;
      }
      if (l == layer_ptr[b + 1] - 1 && !(cfg->flags & FUELMI_REFINE_LAST_ARGMIN)) nv = 1;
      edge_off[l] = (int)std::min<long long>(edges, INT_MAX);
      edges += (long long)nu * nv;
      nu = nv;
    }
  }
  if (edges > INT_MAX) {
    fuelmi_set_error("refine: %lld edges in one call, more than %d", edges, INT_MAX);
    return FUELMI_ELIMIT;
  }
  const int n_nodes = node_ptr[n_layers];
  for (int b = 0; b < n_prob; ++b) {
    for (int k = 0; k < 3; ++k) ARGCHK(finite_below(start[7 * b + k], 1e7) && std::isfinite(start[7 * b + 3 + k]));
    ARGCHK(finite_below(start[7 * b + 6], 1e7));
  }
  for (long k = 0; k < 4L * n_nodes; ++k) ARGCHK(finite_below(nodes[k], 1e7));
  ARGCHK(m);

  // ---- the edge list: layer blocks in order, slot u * nv + v ----
  const int flags = cfg->flags;
  std::vector<double> p1(3 * (size_t)edges), p2(3 * (size_t)edges);
  for (int b = 0; b < n_prob; ++b) {
    const double* prev = start + 7 * (size_t)b;  // the previous layer's nodes (stride 4) or the start
    int nu = 1, stride = 7;
    for (int l = layer_ptr[b]; l < layer_ptr[b + 1]; ++l) {
      int nv = node_ptr[l + 1] - node_ptr[l];
      if (l == layer_ptr[b + 1] - 1 && !(flags & FUELMI_REFINE_LAST_ARGMIN)) nv = 1;
      const double* cur = nodes + 4 * (size_t)node_ptr[l];
      for (int u = 0; u < nu; ++u)
        for (int v = 0; v < nv; ++v) {
          const size_t e = (size_t)edge_off[l] + (size_t)u * nv + v;
          for (int k = 0; k < 3; ++k) p1[3 * e + k] = prev[(size_t)stride * u + k], p2[3 * e + k] = cur[4 * v + k];
        }
      prev = cur, stride = 4, nu = nv;
    }
  }

  HIPCHK(hipSetDevice(m->device));
  for (int& v : m->path_stats) v = 0;
  PathRun run;
  int rc = path_cost_enqueue(m, &pc, (int)edges, p1.data(), p2.data(), 0, run);
  if (rc != FUELMI_OK) return rc;

  // ---- problems to the device, k_refine, choices and costs back ----
  double *d_start, *d_nodes, *d_cost;
  int *d_lptr, *d_nptr, *d_eoff, *d_choice, *d_err;
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 256);
    d_start = L.take<double>(7 * (size_t)n_prob);
    d_lptr = L.take<int>(n_prob + 1);
    d_nptr = L.take<int>(n_layers + 1);
    d_nodes = L.take<double>(4 * (size_t)n_nodes);
    d_eoff = L.take<int>(n_layers);
    d_choice = L.take<int>(n_layers);
    d_cost = L.take<double>(n_prob);
    d_err = L.take<int>(1);
    return L.size();
  };
  hipStream_t st = m->stream;
  rc = m->refine_dev.reserve(st, layout(nullptr));
  if (rc != FUELMI_OK) return rc;
  layout(m->refine_dev.base());
  HIPCHK(hipMemcpyAsync(d_start, start, sizeof(double) * 7 * n_prob, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_lptr, layer_ptr, sizeof(int) * (n_prob + 1), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_nptr, node_ptr, sizeof(int) * (n_layers + 1), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_nodes, nodes, sizeof(double) * 4 * (size_t)n_nodes, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_eoff, edge_off.data(), sizeof(int) * n_layers, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(d_err, 0, sizeof(int), st));
  RArgs R;
  R.start = d_start;
  R.layer_ptr = d_lptr;
  R.node_ptr = d_nptr;
  R.nodes = d_nodes;
  R.edge_off = d_eoff;
  R.length = run.length;
  R.kind = run.kind;
  R.vm = cfg->vm, R.yd = cfg->yd, R.w_dir = cfg->w_dir;
  R.last_argmin = (flags & FUELMI_REFINE_LAST_ARGMIN) ? 1 : 0;
  R.choice = d_choice;
  R.cost = d_cost;
  R.err = d_err;
  hipLaunchKernelGGL(k_refine, dim3(n_prob), dim3(256), 0, st, R);
  HIPCHK(hipGetLastError());
  int err = 0;
  HIPCHK(hipMemcpyAsync(choice, d_choice, sizeof(int) * n_layers, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(cost, d_cost, sizeof(double) * n_prob, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&err, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(stream_wait(st));
  if (err) {
    fuelmi_set_error("refine: an edge search found no predecessor chain back to its start");
    return FUELMI_EHIP;
  }
  if (!polyline) return FUELMI_OK;

  // ---- the refined-tour polyline: every leg of every problem in one engine run at tour_lattice_res ----
  std::vector<double> a, c;
  std::vector<int> leg_first(n_prob + 1, 0);
  for (int b = 0; b < n_prob; ++b) {
    leg_first[b] = (int)(a.size() / 3);
    const double* from = start + 7 * (size_t)b;
    for (int l = layer_ptr[b]; l < layer_ptr[b + 1]; ++l) {
      if (choice[l] < 0) break;
      const double* to = nodes + 4 * (size_t)(node_ptr[l] + choice[l]);
      a.insert(a.end(), from, from + 3);
      c.insert(c.end(), to, to + 3);
      from = to;
    }
  }
  leg_first[n_prob] = (int)(a.size() / 3);
  const int legs = leg_first[n_prob];
  const int maxp = tour_xyz ? cfg->max_tour_points : 0;
  std::vector<double> leg_len(legs), leg_xyz((size_t)legs * maxp * 3);
  std::vector<int> leg_kind(legs), leg_plen(legs);
  if (legs > 0) {
    fuelmi_path_cfg tc = pc;
    tc.lattice_res = cfg->tour_lattice_res;
    tc.max_path_points = maxp;
    rc = path_cost_enqueue(m, &tc, legs, a.data(), c.data(), maxp, run);
    if (rc != FUELMI_OK) return rc;
    HIPCHK(hipMemcpyAsync(leg_len.data(), run.length, sizeof(double) * legs, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(leg_kind.data(), run.kind, sizeof(int) * legs, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(leg_plen.data(), run.plen, sizeof(int) * legs, hipMemcpyDeviceToHost, st));
    if (run.path)
      HIPCHK(hipMemcpyAsync(leg_xyz.data(), run.path, sizeof(double) * 3 * maxp * (size_t)legs, hipMemcpyDeviceToHost, st));
    HIPCHK(stream_wait(st));
  }
  bool over = false;
  for (int b = 0; b < n_prob; ++b) {
    double* out = tour_xyz ? tour_xyz + (size_t)b * maxp * 3 : nullptr;
    int cnt = 0;
    auto put = [&](const double* q) {
      if (out && cnt < maxp)
        for (int k = 0; k < 3; ++k) out[3 * cnt + k] = q[k];
      ++cnt;
    };
    put(start + 7 * (size_t)b);
    for (int e = leg_first[b]; e < leg_first[b + 1]; ++e) {
      if (leg_kind[e] < 0) {
        fuelmi_set_error("refine: a polyline leg found no predecessor chain back to its start");
        return FUELMI_EHIP;
      }
      if (leg_len[e] != 0.0) {  // :492-495: the whole path whenever searchPath's cost is non-zero
        for (int r = 0; r < leg_plen[e]; ++r) {
          if (r < maxp) put(leg_xyz.data() + ((size_t)e * maxp + r) * 3);
          else ++cnt;
        }
      } else {
        put(c.data() + 3 * (size_t)e);
      }
    }
    tour_len[b] = cnt;
    if (tour_xyz && cnt > maxp) over = true;
  }
  if (over) {
    fuelmi_set_error("refine: a polyline has more than max_tour_points = %d points (tour_len holds each count)", maxp);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}
