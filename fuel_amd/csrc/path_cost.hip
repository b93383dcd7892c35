// path_cost.hip -- ViewNode::searchPath (active_perception/src/graph_node.cpp:32-61) for a batch of point pairs:
// the tour cost matrix of FrontierFinder::updateFrontierCostMatrix / getFullCostMatrix / getPathForTour
// (frontier_finder.cpp:260-326, 508-592).
//
// Per pair (p1, p2):
//   1. the straight line: RayCaster::input(p1, p2) / nextId, unsafe at the first voxel that is inflated, UNKNOWN or
//      outside the index box (k_path_los, one lane per pair) -- bit for bit the reference's result;
//   2. when it is blocked, the SHORTEST path on the 26-connected lattice p1 + n * res (res = 0.4, graph_node.cpp:49)
//      under the edge-safety rule of Astar::search (path_searching/src/astar2.cpp:86-113), to the cheapest node of
//      the goal neighbourhood (posToIndex within +-1 of p2's, astar2.cpp:66-68) -- in place of the reference's
//      lambda_heu = 10000 best-first search with its wall-clock cap, so the result is well defined;
//   3. no goal reachable: cost no_path_cost, path {p1, p2} (graph_node.cpp:59-60).
//
// The lattice search runs once per distinct source p1 (pairs that share a p1 bitwise share it):
//   k_path_mask  one lane per lattice node: 27 bits -- bit 13: the node is in the domain (isInBox(pos), or the
//                start), bit j != 13: the edge from v - s_j to v is usable, s_j = (j/9-1, j/3%3-1, j%3-1) * res;
//   k_path_relax one workgroup per active tile of 8 x 8 x 4 nodes: the tile plus a one-node halo in LDS, relaxed
//                to a local fixed point of d(v) = min_u fl(d(u) + w(u, v)); improved face nodes put the neighbour
//                tiles on the next launch's work list.  Launches repeat until a list is empty (the host looks every
//                few launches); no grid-wide barrier.  Every value is an upper bound reached by a real path and a
//                launch leaves no edge of an empty list's tiles relaxable, so the end is the least fixed point --
//                the same bits as any exact shortest-path algorithm in f64;
//   k_path_goal  one lane per pair: the goal minimising fl(d(v) + |p2 - pos(v)|) (ties: smallest n), backtracked
//                through the first usable predecessor (dx, then dy, then dz from -1 to +1) with fl(d(u) + w) == d(v).
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "frontier_internal.h"

namespace {

constexpr int TX = 8, TY = 8, TZ = 4;  // lattice tile of one workgroup (256 nodes)
constexpr int HX = TX + 2, HY = TY + 2, HZ = TZ + 2;
constexpr int HALO = HX * HY * HZ;
constexpr unsigned DOMAIN_BIT = 1u << 13;
constexpr double DINF = __builtin_huge_val();
constexpr int PC_SEG = 64, PC_NCK = 128;  // k_path_goal's backtrack: checkpoint spacing, checkpoints per lane

struct PSrc {  // one source's lattice: nodes n = nlo + (i, j, k), 0 <= (i, j, k) < E
  double p1[3];
  int nlo[3], E[3], TT[3];  // TT: tiles per axis
  int tile_off;             // first tile of this source in the chunk
  long node_off;            // first node of this source in the chunk
};

struct PArgs {
  const u64* infl;
  const u64* unk;
  double box_mind[3], box_maxd[3];  // SDFMap::isInBox(Vector3d): strict (sdf_map.h:180-186)
  int bmin[3], bmax[3];             // SDFMap::isInBox(Vector3i): bmin <= id < bmax
  double res;                       // lattice resolution
  double inv_res;                   // Astar::inv_resolution_ = 1 / res (goal test)
  double edge_step;                 // sample spacing along an edge (astar2.cpp:105)
  double w[27];                     // |s_j|
  double dir[27][3];                // s_j / |s_j|
};

__device__ __forceinline__ bool in_box_d(const PArgs& A, const double p[3]) {
  for (int k = 0; k < 3; ++k)
    if (p[k] <= A.box_mind[k] || p[k] >= A.box_maxd[k]) return false;
  return true;
}
// getInflateOccupancy(pos) == 1 || getOccupancy(pos) == UNKNOWN
__device__ __forceinline__ bool blocked_at(const Geo& g, const PArgs& A, const double p[3]) {
  return plane_at_pos(g, A.infl, p) || plane_at_pos(g, A.unk, p);
}
__device__ __forceinline__ void node_pos(const PSrc& S, const int n[3], double res, double p[3]) {
  for (int k = 0; k < 3; ++k) p[k] = S.p1[k] + (double)n[k] * res;
}
__device__ __forceinline__ double norm3(double a, double b, double c) { return sqrt(a * a + b * b + c * c); }

__device__ __forceinline__ int find_src_node(const PSrc* S, int nsrc, long node) {
  int lo = 0, hi = nsrc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (S[mid].node_off <= node) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ int find_src_tile(const PSrc* S, int nsrc, int tile) {
  int lo = 0, hi = nsrc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (S[mid].tile_off <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- 1. straight line, one lane per pair ----------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_path_los(Geo g, PArgs A, int n, const double* __restrict__ p1,
                                                  const double* __restrict__ p2, double* length, int* kind, int* plen,
                                                  double* path, int maxp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double a[3] = {p1[3 * i], p1[3 * i + 1], p1[3 * i + 2]};
  const double b[3] = {p2[3 * i], p2[3 * i + 1], p2[3 * i + 2]};
  if (!ray_clear<true>(g, A.infl, A.unk, A.bmin, A.bmax, a, b)) {
    kind[i] = -1;  // the lattice search decides
    return;
  }
  kind[i] = 0;
  length[i] = norm3(a[0] - b[0], a[1] - b[1], a[2] - b[2]);
  plen[i] = 2;
  if (path && maxp >= 2) {
    double* o = path + (size_t)i * maxp * 3;
    for (int k = 0; k < 3; ++k) o[k] = a[k], o[3 + k] = b[k];
  }
}

// ---- 2a. node / edge masks, distances set to +inf (0 at the start, whose tile opens the first work list) --------
__global__ void __launch_bounds__(256) k_path_mask(Geo g, PArgs A, const PSrc* __restrict__ S, int nsrc, long nodes,
                                                   u32* mask, double* dist, u32* stamp, u32* list1, u32* cnt) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nodes) return;
  const int s = find_src_node(S, nsrc, t);
  const PSrc& P = S[s];
  const long loc = t - P.node_off;
  const int li = (int)(loc / ((long)P.E[1] * P.E[2])), rem = (int)(loc - (long)li * P.E[1] * P.E[2]);
  const int lj = rem / P.E[2], lk = rem - lj * P.E[2];
  const int n[3] = {P.nlo[0] + li, P.nlo[1] + lj, P.nlo[2] + lk};
  const bool start = n[0] == 0 && n[1] == 0 && n[2] == 0;
  double pv[3];
  node_pos(P, n, A.res, pv);
  u32 m = 0;
  if (start) {
    m = DOMAIN_BIT;
    dist[t] = 0.0;
    const int tile = P.tile_off + ((li / TX) * P.TT[1] + lj / TY) * P.TT[2] + lk / TZ;
    stamp[tile] = 1u;
    list1[atomicAdd(&cnt[1], 1u)] = (u32)tile;
  } else {
    dist[t] = DINF;
    if (in_box_d(A, pv)) {
      m = DOMAIN_BIT;
      if (!blocked_at(g, A, pv)) {
        for (int j = 0; j < 27; ++j) {
          if (j == 13) continue;
          const int sd[3] = {j / 9 - 1, (j / 3) % 3 - 1, j % 3 - 1};
          const int u[3] = {n[0] - sd[0], n[1] - sd[1], n[2] - sd[2]};
          bool ok = true;
          for (int k = 0; k < 3; ++k)
            if (u[k] < P.nlo[k] || u[k] >= P.nlo[k] + P.E[k]) ok = false;
          if (!ok) continue;
          double pu[3];
          node_pos(P, u, A.res, pu);
          if (!(u[0] == 0 && u[1] == 0 && u[2] == 0) && !in_box_d(A, pu)) continue;
          for (double l = A.edge_step; l < A.w[j]; l += A.edge_step) {
            const double c[3] = {pu[0] + l * A.dir[j][0], pu[1] + l * A.dir[j][1], pu[2] + l * A.dir[j][2]};
            if (blocked_at(g, A, c)) {
              ok = false;
              break;
            }
          }
          if (ok) m |= 1u << j;
        }
      }
    }
  }
  mask[t] = m;
}

// ---- 2b. tiled relaxation: launch t works through list (t & 1) of cnt[t] tiles and fills list ((t + 1) & 1) ------
__global__ void __launch_bounds__(256) k_path_relax(PArgs A, const PSrc* __restrict__ S, int nsrc,
                                                    const u32* __restrict__ mask, double* dist, u32* stamp, u32* lists,
                                                    int total_tiles, u32* cnt, int t) {
  __shared__ double d_l[HALO];
  __shared__ u32 faces;
  const int tid = threadIdx.x;
  const int lx = tid >> 5, ly = (tid >> 2) & 7, lz = tid & 3;
  const int me = ((lx + 1) * HY + (ly + 1)) * HZ + (lz + 1);
  const u32 todo = cnt[t];
  const u32* in = lists + (size_t)(t & 1) * total_tiles;
  u32* out = lists + (size_t)((t + 1) & 1) * total_tiles;
  for (u32 e = blockIdx.x; e < todo; e += gridDim.x) {
    const int tile = (int)in[e];
    const int s = find_src_tile(S, nsrc, tile);
    const PSrc& P = S[s];
    const int lt = tile - P.tile_off;
    const int tx = lt / (P.TT[1] * P.TT[2]), ty = (lt / P.TT[2]) % P.TT[1], tz = lt % P.TT[2];
    const int o[3] = {tx * TX, ty * TY, tz * TZ};
    double* D = dist + P.node_off;
    __syncthreads();  // the previous tile's LDS is no longer read
    if (tid == 0) faces = 0u;
    for (int h = tid; h < HALO; h += 256) {
      const int hx = h / (HY * HZ), hy = (h / HZ) % HY, hz = h % HZ;
      const int x = o[0] + hx - 1, y = o[1] + hy - 1, z = o[2] + hz - 1;
      double v = DINF;
      if (x >= 0 && y >= 0 && z >= 0 && x < P.E[0] && y < P.E[1] && z < P.E[2])
        v = __hip_atomic_load(D + ((long)x * P.E[1] + y) * P.E[2] + z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      d_l[h] = v;
    }
    const int x = o[0] + lx, y = o[1] + ly, z = o[2] + lz;
    const bool inside = x < P.E[0] && y < P.E[1] && z < P.E[2];
    const long adr = ((long)x * P.E[1] + y) * P.E[2] + z;
    u32 m = inside ? mask[P.node_off + adr] : 0u;
    m = (m & DOMAIN_BIT) ? (m & ~DOMAIN_BIT) : 0u;  // in-edges of a domain node
    __syncthreads();
    const double d0 = d_l[me];
    double cur = d0;
    while (true) {
      bool changed = false;
      for (u32 b = m; b; b &= b - 1) {
        const int j = __builtin_ctz(b);
        const int nb = me - ((j / 9 - 1) * HY * HZ + ((j / 3) % 3 - 1) * HZ + (j % 3 - 1));
        const double c = d_l[nb] + A.w[j];
        if (c < cur) {
          cur = c;
          changed = true;
        }
      }
      if (changed) d_l[me] = cur;
      if (!__syncthreads_or(changed)) break;
    }
    if (cur < d0) {
      __hip_atomic_store(D + adr, cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // neighbour tiles whose halo holds this node
      const int lim[3] = {min(TX, P.E[0] - o[0]) - 1, min(TY, P.E[1] - o[1]) - 1, min(TZ, P.E[2] - o[2]) - 1};
      const int lc[3] = {lx, ly, lz};
      u32 ax[3];
      for (int k = 0; k < 3; ++k) ax[k] = 2u | (lc[k] == 0 ? 1u : 0u) | (lc[k] == lim[k] ? 4u : 0u);
      u32 f = 0u;
      for (int j = 0; j < 27; ++j)
        if ((ax[0] >> (j / 9)) & (ax[1] >> ((j / 3) % 3)) & (ax[2] >> (j % 3)) & 1u) f |= 1u << j;
      atomicOr(&faces, f & ~DOMAIN_BIT);
    }
    __syncthreads();
    if (tid < 27 && ((faces >> tid) & 1u)) {
      const int nt[3] = {tx + tid / 9 - 1, ty + (tid / 3) % 3 - 1, tz + tid % 3 - 1};
      if (nt[0] >= 0 && nt[1] >= 0 && nt[2] >= 0 && nt[0] < P.TT[0] && nt[1] < P.TT[1] && nt[2] < P.TT[2]) {
        const int ng = P.tile_off + (nt[0] * P.TT[1] + nt[1]) * P.TT[2] + nt[2];
        if (atomicMax(&stamp[ng], (u32)(t + 1)) < (u32)(t + 1)) out[atomicAdd(&cnt[t + 1], 1u)] = (u32)ng;
      }
    }
  }
}

// ---- 2c. goal choice and backtrack, one lane per pair ------------------------------------------------------------
struct GArgs {
  const int* pair;  // [npairs] pair index
  const int* src;   // [npairs] source in the chunk
  int npairs;
  const double* p2;
  const u32* mask;
  const double* dist;
  double* length;
  int* kind;
  int* plen;
  double* path;
  int maxp;
  double org[3];      // map origin (Astar::origin_)
  double no_path_cost;
};

// first usable predecessor u of node (local) v with fl(d(u) + w) == d(v), in the reference's loop order
__device__ __forceinline__ long pred_of(const PArgs& A, const PSrc& P, const u32* M, const double* D, long v, int vi[3]) {
  const u32 m = M[v] & ~DOMAIN_BIT;
  const double dv = D[v];
  for (int j = 0; j < 27; ++j) {
    if (!((m >> j) & 1u)) continue;
    const int u[3] = {vi[0] - (j / 9 - 1), vi[1] - ((j / 3) % 3 - 1), vi[2] - (j % 3 - 1)};
    const long ua = ((long)u[0] * P.E[1] + u[1]) * P.E[2] + u[2];
    if (D[ua] + A.w[j] == dv) {
      vi[0] = u[0], vi[1] = u[1], vi[2] = u[2];
      return ua;
    }
  }
  return -1;  // unreachable at the fixed point
}

__global__ void __launch_bounds__(64) k_path_goal(PArgs A, const PSrc* __restrict__ S, GArgs G) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= G.npairs) return;
  const int i = G.pair[q];
  const PSrc& P = S[G.src[q]];
  const u32* M = G.mask + P.node_off;
  const double* D = G.dist + P.node_off;
  const double p2[3] = {G.p2[3 * i], G.p2[3 * i + 1], G.p2[3 * i + 2]};
  double* po = G.path ? G.path + (size_t)i * G.maxp * 3 : nullptr;
  // goal neighbourhood: posToIndex(pos(n)) within +-1 of posToIndex(p2) per axis (astar2.cpp:66-68, 231-233)
  int c[3], gi[3];
  unsigned ok[3];  // bit r: n = c - 4 + r qualifies
  for (int k = 0; k < 3; ++k) {
    gi[k] = (int)floor((p2[k] - G.org[k]) * A.inv_res);
    c[k] = (int)floor((p2[k] - P.p1[k]) / A.res + 0.5);
    ok[k] = 0u;
    for (int r = 0; r < 9; ++r) {
      const int n = c[k] - 4 + r;
      const int id = (int)floor((P.p1[k] + (double)n * A.res - G.org[k]) * A.inv_res);
      if (abs(id - gi[k]) <= 1 && n >= P.nlo[k] && n < P.nlo[k] + P.E[k]) ok[k] |= 1u << r;
    }
  }
  double best = DINF;
  long bv = -1;
  int bi[3] = {0, 0, 0};
  for (int r0 = 0; r0 < 9; ++r0) {
    if (!((ok[0] >> r0) & 1u)) continue;
    for (int r1 = 0; r1 < 9; ++r1) {
      if (!((ok[1] >> r1) & 1u)) continue;
      for (int r2 = 0; r2 < 9; ++r2) {
        if (!((ok[2] >> r2) & 1u)) continue;
        const int n[3] = {c[0] - 4 + r0, c[1] - 4 + r1, c[2] - 4 + r2};
        const int li[3] = {n[0] - P.nlo[0], n[1] - P.nlo[1], n[2] - P.nlo[2]};
        const long a = ((long)li[0] * P.E[1] + li[1]) * P.E[2] + li[2];
        if (!(M[a] & DOMAIN_BIT)) continue;
        const double d = D[a];
        if (!(d < DINF)) continue;
        double pv[3];
        node_pos(P, n, A.res, pv);
        const double f = d + norm3(p2[0] - pv[0], p2[1] - pv[1], p2[2] - pv[2]);
        if (f < best) {
          best = f;
          bv = a;
          bi[0] = li[0], bi[1] = li[1], bi[2] = li[2];
        }
      }
    }
  }
  if (bv < 0) {  // graph_node.cpp:59-60
    G.kind[i] = 2;
    G.length[i] = G.no_path_cost;
    G.plen[i] = 2;
    if (po && G.maxp >= 2)
      for (int k = 0; k < 3; ++k) po[k] = P.p1[k], po[3 + k] = p2[k];
    return;
  }
  const long s0 = ((long)(-P.nlo[0]) * P.E[1] - P.nlo[1]) * P.E[2] - P.nlo[2];  // the start node
  const long cap = (long)P.E[0] * P.E[1] * P.E[2];
  int H = 0;  // lattice edges from the start to the goal
  {
    long v = bv;
    int vi[3] = {bi[0], bi[1], bi[2]};
    while (v != s0 && v >= 0 && H <= cap) v = pred_of(A, P, M, D, v, vi), ++H;
    if (v != s0) H = -1;
  }
  if (H < 0) {  // (a broken fixed point; never seen -- reported rather than looped over)
    G.kind[i] = -2;
    return;
  }
  const int np = H + 2;
  G.plen[i] = np;
  // Points in path order: 0 = p1, r = 1..H the node H - r steps back from the goal, H + 1 = p2.  One more walk from
  // the goal leaves a checkpoint every PC_SEG nodes; each segment is then expanded from its checkpoint into a small
  // buffer and emitted forwards, so the sequential pathLength sum costs O(H) predecessor lookups.
  const bool write = po && np <= G.maxp;
  double prev[3] = {P.p1[0], P.p1[1], P.p1[2]};
  double len = 0.0;  // Astar::pathLength (astar2.cpp:186-192)
  if (write)
    for (int k = 0; k < 3; ++k) po[k] = P.p1[k];
  auto emit = [&](int r, const int vi[3]) {  // point r (1..H) at lattice node vi
    const int nn[3] = {vi[0] + P.nlo[0], vi[1] + P.nlo[1], vi[2] + P.nlo[2]};
    double q[3];
    node_pos(P, nn, A.res, q);
    len += norm3(q[0] - prev[0], q[1] - prev[1], q[2] - prev[2]);
    prev[0] = q[0], prev[1] = q[1], prev[2] = q[2];
    if (write)
      for (int k = 0; k < 3; ++k) po[3 * r + k] = q[k];
  };
  if (H > 0) {
    short ck[PC_NCK][3];  // node after c * PC_SEG steps back from the goal
    const int nck = (H + PC_SEG - 1) / PC_SEG;
    if (nck <= PC_NCK) {
      long v = bv;
      int vi[3] = {bi[0], bi[1], bi[2]};
      for (int t = 0; t < H; ++t) {
        if (t % PC_SEG == 0)
          for (int k = 0; k < 3; ++k) ck[t / PC_SEG][k] = (short)vi[k];
        v = pred_of(A, P, M, D, v, vi);
      }
      for (int c = nck - 1; c >= 0; --c) {  // segments from the start side on
        short seg[PC_SEG][3];
        int w[3] = {ck[c][0], ck[c][1], ck[c][2]};
        long a = ((long)w[0] * P.E[1] + w[1]) * P.E[2] + w[2];
        const int cnt = min(PC_SEG, H - c * PC_SEG);  // nodes t = c * PC_SEG .. + cnt - 1 steps back
        for (int q = 0; q < cnt; ++q) {
          for (int k = 0; k < 3; ++k) seg[q][k] = (short)w[k];
          if (q + 1 < cnt) a = pred_of(A, P, M, D, a, w);
        }
        for (int q = cnt - 1; q >= 0; --q) {
          const int vi2[3] = {seg[q][0], seg[q][1], seg[q][2]};
          emit(H - (c * PC_SEG + q), vi2);
        }
      }
    } else {  // (longer than PC_NCK * PC_SEG steps: each point by its own walk)
      for (int r = 1; r <= H; ++r) {
        long v = bv;
        int vi[3] = {bi[0], bi[1], bi[2]};
        for (int b = H; b > r; --b) v = pred_of(A, P, M, D, v, vi);
        emit(r, vi);
      }
    }
  }
  len += norm3(p2[0] - prev[0], p2[1] - prev[1], p2[2] - prev[2]);
  if (write)
    for (int k = 0; k < 3; ++k) po[3 * (H + 1) + k] = p2[k];
  G.length[i] = len;
  G.kind[i] = 1;
}

// one source's lattice extent along an axis: the n with box_mind < p1 + n * res < box_maxd (monotone in n)
void axis_range(double p1, double res, double lo, double hi, int& nlo, int& nhi) {
  auto pos = [&](long n) { return p1 + (double)n * res; };
  long a = (long)std::ceil((lo - p1) / res);
  while (pos(a - 1) > lo) --a;
  while (!(pos(a) > lo)) ++a;
  long b = (long)std::floor((hi - p1) / res);
  while (pos(b + 1) < hi) ++b;
  while (!(pos(b) < hi)) --b;
  nlo = (int)a, nhi = (int)b;
}

constexpr size_t CHUNK_NODE_BUDGET = (size_t)48 << 20;  // lattice nodes per chunk of sources (12 B each)
constexpr int POLL_EVERY = 8;

}  // namespace

// The searches of n pairs queued on the map's stream: source dedup, chunks, k_path_los / _mask / _relax / _goal.  The
// results stay in the map's path pool (path_dev, a DevScratch carved by a BlockLayout; valid until the next enqueue);
// fuelmi_map_path_stats' counters accumulate.  The caller has checked the arguments (finite, |coordinate| < 1e7) and
// n > 0.  always_lattice: k_path_los is skipped and every pair is searched on its source's lattice.

int path_cost_enqueue(fuelmi_map* m, const fuelmi_path_cfg* cfg, int n, const double* p1_xyz, const double* p2_xyz,
                      int maxp, PathRun& out, bool always_lattice) {
  HIPCHK(hipSetDevice(m->device));
  const Geo& g = m->g;

  PArgs A;
  A.infl = m->infl_bits.p;
  A.unk = m->unk_bits.p;
  for (int k = 0; k < 3; ++k) {
    A.box_mind[k] = m->cfg.box_min[k];
    A.box_maxd[k] = m->cfg.box_max[k];
    A.bmin[k] = m->info.box_min[k];
    A.bmax[k] = m->info.box_max[k];
  }
  A.res = cfg->lattice_res;
  A.inv_res = 1.0 / cfg->lattice_res;
  A.edge_step = cfg->edge_step;
  for (int j = 0; j < 27; ++j) {
    const double s[3] = {(j / 9 - 1) * A.res, ((j / 3) % 3 - 1) * A.res, (j % 3 - 1) * A.res};
    A.w[j] = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    for (int k = 0; k < 3; ++k) A.dir[j][k] = j == 13 ? 0.0 : s[k] / A.w[j];
  }

  // ---- every distinct p1 (bitwise) may become a source: its lattice, and from all of them the largest chunk ----
  std::map<std::array<u64, 3>, int> src_of;
  std::vector<int> src_idx(n);
  std::vector<PSrc> lat;
  for (int i = 0; i < n; ++i) {
    std::array<u64, 3> key;
    std::memcpy(key.data(), p1_xyz + 3 * i, 24);
    auto it = src_of.find(key);
    if (it != src_of.end()) {
      src_idx[i] = it->second;
      continue;
    }
    const int s = (int)lat.size();
    src_of.emplace(key, s);
    src_idx[i] = s;
    PSrc P;
    int lo[3], hi[3];
    bool touches = true;  // the in-box range reaches a neighbour of the start along every axis
    for (int k = 0; k < 3; ++k) {
      P.p1[k] = p1_xyz[3 * i + k];
      axis_range(P.p1[k], A.res, A.box_mind[k], A.box_maxd[k], lo[k], hi[k]);
      if (lo[k] > hi[k] || lo[k] > 1 || hi[k] < -1) touches = false;
    }
    for (int k = 0; k < 3; ++k) {
      if (!touches) lo[k] = hi[k] = 0;  // the start alone: nothing around it is in the box
      lo[k] = std::min(lo[k], 0);
      hi[k] = std::max(hi[k], 0);
      P.nlo[k] = lo[k];
      P.E[k] = hi[k] - lo[k] + 1;
    }
    P.TT[0] = (P.E[0] + TX - 1) / TX, P.TT[1] = (P.E[1] + TY - 1) / TY, P.TT[2] = (P.E[2] + TZ - 1) / TZ;
    P.tile_off = 0, P.node_off = 0;
    const double nodes = (double)P.E[0] * P.E[1] * P.E[2];
    if (nodes > (double)CHUNK_NODE_BUDGET || P.E[0] > 32767 || P.E[1] > 32767 || P.E[2] > 32767) {
      fuelmi_set_error("path costs: a lattice of %.0f nodes exceeds the limit of %zu", nodes, CHUNK_NODE_BUDGET);
      return FUELMI_ELIMIT;
    }
    lat.push_back(P);
  }
  // a chunk holds sources while their nodes fit the budget (or one source): it never needs more than these
  long all_nodes = 0, max_nodes = 0;
  size_t all_tiles = 0;
  for (const PSrc& P : lat) {
    const long nn = (long)P.E[0] * P.E[1] * P.E[2];
    all_nodes += nn;
    max_nodes = std::max(max_nodes, nn);
    all_tiles += (size_t)P.TT[0] * P.TT[1] * P.TT[2];
  }
  const size_t chunk_nodes = (size_t)std::min(all_nodes, (long)CHUNK_NODE_BUDGET);
  const size_t chunk_tiles = std::min(all_tiles, chunk_nodes);  // a tile holds at least one node
  // launches a chunk may take: the work lists settle after at most (tile segments of a shortest path) + 1 launches,
  // and a shortest path has fewer segments than its source has nodes -- a bound, not a guess
  const long cap_max = max_nodes + 2;
  double *d_p1, *d_p2, *d_len, *d_path, *d_dist;
  int *d_kind, *d_plen, *d_pair, *d_src;
  PSrc* d_lat;
  u32 *d_mask, *d_stamp, *d_lists, *d_cnt;
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 256);
    d_p1 = L.take<double>(3 * (size_t)n);
    d_p2 = L.take<double>(3 * (size_t)n);
    d_len = L.take<double>(n);
    d_kind = L.take<int>(n);
    d_plen = L.take<int>(n);
    d_pair = L.take<int>(n);
    d_src = L.take<int>(n);
    d_path = maxp > 0 ? L.take<double>((size_t)n * maxp * 3) : nullptr;
    d_lat = L.take<PSrc>(lat.size());
    d_mask = L.take<u32>(chunk_nodes);
    d_dist = L.take<double>(chunk_nodes);
    d_stamp = L.take<u32>(chunk_tiles);
    d_lists = L.take<u32>(2 * chunk_tiles);
    d_cnt = L.take<u32>(cap_max + 2);
    return L.size();
  };
  const int grow = m->path_dev.reserve(m->stream, layout(nullptr));  // one allocation per call at most
  if (grow != FUELMI_OK) return grow;
  layout(m->path_dev.base());

  hipStream_t st = m->stream;
  HIPCHK(hipMemcpyAsync(d_p1, p1_xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_p2, p2_xyz, sizeof(double) * 3 * n, hipMemcpyHostToDevice, st));
  std::vector<int> hk(n, -1);
  if (!always_lattice) {
    hipLaunchKernelGGL(k_path_los, dim3((n + 255) / 256), dim3(256), 0, st, g, A, n, d_p1, d_p2, d_len, d_kind, d_plen,
                       d_path, maxp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hk.data(), d_kind, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(stream_wait(st));
  }

  // the sources the straight line did not settle, in first-seen order, with their pairs
  std::vector<std::vector<int>> pairs_of(lat.size());
  std::vector<int> srcs;
  for (int i = 0; i < n; ++i) {
    if (hk[i] != -1) continue;
    if (pairs_of[src_idx[i]].empty()) srcs.push_back(src_idx[i]);
    pairs_of[src_idx[i]].push_back(i);
  }
  m->path_stats[2] += (int)srcs.size();

  // ---- chunks of sources: lattices that fit the node budget together ----
  std::vector<int> gp, gs;
  std::vector<PSrc> cl;
  for (size_t s0 = 0; s0 < srcs.size();) {
    size_t s1 = s0;
    long nodes = 0, cmax = 0;
    int tiles = 0;
    cl.clear();
    while (s1 < srcs.size()) {
      PSrc P = lat[srcs[s1]];
      const long nn = (long)P.E[0] * P.E[1] * P.E[2];
      if (s1 > s0 && (size_t)(nodes + nn) > CHUNK_NODE_BUDGET) break;
      P.node_off = nodes;
      P.tile_off = tiles;
      nodes += nn;
      tiles += P.TT[0] * P.TT[1] * P.TT[2];
      cmax = std::max(cmax, nn);
      cl.push_back(P);
      ++s1;
    }
    const int nsrc = (int)cl.size();
    const long cap = cmax + 2;
    gp.clear();
    gs.clear();
    for (int s = 0; s < nsrc; ++s)
      for (int i : pairs_of[srcs[s0 + s]]) gp.push_back(i), gs.push_back(s);
    HIPCHK(hipMemcpyAsync(d_lat, cl.data(), sizeof(PSrc) * nsrc, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_pair, gp.data(), sizeof(int) * gp.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_src, gs.data(), sizeof(int) * gs.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_stamp, 0, sizeof(u32) * tiles, st));
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(u32) * (cap + 2), st));
    hipLaunchKernelGGL(k_path_mask, dim3((unsigned)((nodes + 255) / 256)), dim3(256), 0, st, g, A, d_lat, nsrc, nodes,
                       d_mask, d_dist, d_stamp, d_lists + tiles, d_cnt);
    HIPCHK(hipGetLastError());
    const int grid = std::min(tiles, 2048);
    bool done = false;
    u32 last = 0;
    long t = 1;
    for (; t <= cap && !done; ++t) {
      hipLaunchKernelGGL(k_path_relax, dim3(grid), dim3(256), 0, st, A, d_lat, nsrc, d_mask, d_dist, d_stamp, d_lists,
                         tiles, d_cnt, (int)t);
      HIPCHK(hipGetLastError());
      if (t % POLL_EVERY == 0 || t == cap) {
        HIPCHK(hipMemcpyAsync(&last, d_cnt + t + 1, sizeof(u32), hipMemcpyDeviceToHost, st));
        HIPCHK(stream_wait(st));
        done = last == 0;
      }
    }
    if (!done) {
      fuelmi_set_error("path costs: the lattice relaxation did not settle within %ld launches", cap);
      return FUELMI_EHIP;
    }
    m->path_stats[0] += (int)(t - 1);
    m->path_stats[1] = std::max(m->path_stats[1], (int)(t - 1));
    m->path_stats[3] += 1;
    GArgs G;
    G.pair = d_pair;
    G.src = d_src;
    G.npairs = (int)gp.size();
    G.p2 = d_p2;
    G.mask = d_mask;
    G.dist = d_dist;
    G.length = d_len;
    G.kind = d_kind;
    G.plen = d_plen;
    G.path = d_path;
    G.maxp = maxp;
    for (int k = 0; k < 3; ++k) G.org[k] = g.org[k];
    G.no_path_cost = cfg->no_path_cost;
    hipLaunchKernelGGL(k_path_goal, dim3((G.npairs + 63) / 64), dim3(64), 0, st, A, d_lat, G);
    HIPCHK(hipGetLastError());
    s0 = s1;
  }
  out.length = d_len;
  out.kind = d_kind;
  out.plen = d_plen;
  out.path = d_path;
  out.p2 = d_p2;
  return FUELMI_OK;
}

extern "C" int fuelmi_map_path_costs(fuelmi_map* m, const fuelmi_path_cfg* cfg, int n, const double* p1_xyz,
                                     const double* p2_xyz, double* length, int* kind, int* path_len, double* path_xyz) {
  ARGCHK(m && cfg);
  ARGCHK(n >= 0);
  if (n == 0) return FUELMI_OK;
  ARGCHK(p1_xyz && p2_xyz && length && kind && path_len);
  ARGCHK(cfg->lattice_res > 0.0 && cfg->edge_step > 0.0 && std::isfinite(cfg->lattice_res) && std::isfinite(cfg->edge_step));
  ARGCHK(!path_xyz || cfg->max_path_points >= 0);
  for (long k = 0; k < 3L * n; ++k) ARGCHK(std::fabs(p1_xyz[k]) < 1e7 && std::fabs(p2_xyz[k]) < 1e7);
  HIPCHK(hipSetDevice(m->device));
  const int maxp = path_xyz ? cfg->max_path_points : 0;
  for (int& v : m->path_stats) v = 0;
  PathRun run;
  const int rc = path_cost_enqueue(m, cfg, n, p1_xyz, p2_xyz, maxp, run);
  if (rc != FUELMI_OK) return rc;
  hipStream_t st = m->stream;
  HIPCHK(hipMemcpyAsync(length, run.length, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(kind, run.kind, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(path_len, run.plen, sizeof(int) * n, hipMemcpyDeviceToHost, st));
  if (run.path) HIPCHK(hipMemcpyAsync(path_xyz, run.path, sizeof(double) * 3 * maxp * (size_t)n, hipMemcpyDeviceToHost, st));
  HIPCHK(stream_wait(st));
  bool over = false;
  for (int i = 0; i < n; ++i) {
    if (kind[i] < 0) {
      fuelmi_set_error("path costs: pair %d found no predecessor chain back to its start", i);
      return FUELMI_EHIP;
    }
    if (path_xyz && path_len[i] > maxp) over = true;
  }
  if (over) {
    fuelmi_set_error("path costs: a path has more than max_path_points = %d points (path_len holds each count)", maxp);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

extern "C" int fuelmi_map_path_stats(const fuelmi_map* m, int stats[4]) {
  ARGCHK(m && stats);
  for (int k = 0; k < 4; ++k) stats[k] = m->path_stats[k];
  return FUELMI_OK;
}
