// info_gain.hip -- HeadingPlanner's information gain and yaw search (active_perception/src/heading_planner.cpp), the
// hot part of FastPlannerManager::planYawActMap and localExplore (plan_manage/src/planner_manager_dev.cpp), each for a
// batch on one map:
//   k_info_gain   calcInformationGain (:236-322) / calcInfoGain (:324-391) for view groups: one camera position, up to
//                 FUELMI_GAIN_MAX_YAW yaws
//   k_yaw_path    Graph::dijkstraSearch (:52-100) on searchPathOfYaw's layered graph (:170-234) as a layered recurrence
//
// k_info_gain: one workgroup of IG_NT lanes per group.  A view's rotation, rotated plane normals and index box come from
// the host (gain_view_setup: libm, f64, the reference's order of operations), so every frustum decision is the
// reference's.  Phase 1, one lane per subsampled cell of the union of the group's index boxes, IG_NT cells a step: the
// cell's unknown bit, the exploration box, the far test and the four plane tests per yaw give the cell's member mask; a
// cell that is a candidate of some yaw walks its ray ONCE against occ_bits -- the CastFlags cache (:280-308) is a memo
// of a function of the cell alone -- and leaves mask | visible in LDS, under NON_UNIFORM its weight beside it.  Phase 2,
// one wave per yaw: lane l takes the cells whose subsampled ABSOLUTE y and z indices are l / 8 and l % 8 modulo 8, in
// x, y, z order, and the 64 partial sums meet in a butterfly.  The order of a view's sum therefore depends on the
// cells' own indices only -- not on the union box, the other yaws or the batch -- so a group of K yaws equals K groups of
// one yaw bit for bit, and UNIFORM gains are counts.
//
// k_yaw_path: one 64-lane workgroup (one wave) per problem, one lane per vertex of the current layer; the labels of the
// layer before are read from LDS in layer order, which is the order the FIFO pops them in.
//
// All f64, -ffp-contract=off.  A result does not depend on the problem's place in the batch.
#include <cmath>
#include <cstring>
#include <vector>

#include "fuelmi_internal.h"

namespace {

constexpr int IG_NT = 256;   // lanes of a gain workgroup
constexpr int IG_NW = IG_NT / 64;
constexpr int IG_CAP = FUELMI_GAIN_MAX_CELLS;  // cells of a group's union box, a multiple of 64
constexpr int IG_YAWS = FUELMI_GAIN_MAX_YAW;   // bit 31 of a cell's mask is its ray's verdict
constexpr int IG_CTRL = FUELMI_GAIN_MAX_CTRL;
constexpr int YP_NT = 64;
constexpr int YP_LAYERS = FUELMI_YAWPATH_MAX_LAYER;
constexpr unsigned IG_VISIBLE = 1u << 31;

struct GainView {
  double nrm[4][3];  // R_wc * n_top, n_bottom, n_left, n_right
  int lb[3], ub[3];  // calcFovAABB's index box cut to the map; ub < lb: no cell
};

struct GainGroup {
  double pos[3];
  int n_yaw;         // 0: nothing to do (an empty group, or one over the cell cap)
  int path;          // NON_UNIFORM: the group's control-point array
  int u0[3], ud[3];  // the union of the views' boxes in subsampled indices: first cell, cells per axis
  int cells;         // ud[0] * ud[1] * ud[2]
};

// k_info_gain: every pointer addresses device memory
struct GainArgs {
  fuelmi_gain_cfg cfg;
  int n_group;
  int lds_cells;           // cells the LDS block is laid out for, a multiple of 64
  double off[3];           // 0.5 - origin / resolution
  int bmin[3], bmax[3];    // SDFMap::isInBox(Vector3i)
  const u64 *unk, *occ;
  const GainGroup* groups;
  const GainView* views;   // [n_group][max_yaw]
  const int* n_ctrl;       // [n_path]
  const double* ctrl;      // [n_path][max_ctrl][3]
  double* gain;            // [n_group][max_yaw]
  int *n_cand, *n_visible; // [n_group][max_yaw]
  int* n_rays;             // [n_group]
};

// k_yaw_path: one problem per workgroup
struct YawPathArgs {
  int n_prob, max_layer, nv, h;
  double yaw_diff, max_yaw_rate, w;
  const int* n_layer;
  const double* yaws;      // [n][max_layer]
  const double* dt;
  const double* gains;     // [n][max_layer][nv]
  const int* over;         // [n]: a layer's group is over the cell cap
  int* status;
  double* path;            // [n][max_layer]
  int* path_vertex;        // [n][max_layer]
  double* g_value;         // [n][max_layer][nv]
};

__host__ __device__ __forceinline__ double ig_norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// :290-299: true when the ray from the cell to the camera meets an occupied voxel.  The start voxel is tested, the end
// voxel is not; a voxel outside the map is not occupied.  A walk that has not met its end voxel after one step per
// unit of |dx| + |dy| + |dz| never will (the reference walks on for ever): blocked.
__host__ __device__ inline bool ig_ray_blocked(const Geo& g, const u64* __restrict__ occ, const double off[3],
                                               const double p[3], const double pos[3]) {
  RayWalk r;
  ray_set_input(r, p[0] / g.res, p[1] / g.res, p[2] / g.res, pos[0] / g.res, pos[1] / g.res, pos[2] / g.res);
  const int limit = abs(r.endx - r.x) + abs(r.endy - r.y) + abs(r.endz - r.z) + 2;
  for (int n = 0; n < limit; ++n) {
    if (ray_at_end(r)) return false;
    int id[3] = {(int)((double)r.x + off[0]), (int)((double)r.y + off[1]), (int)((double)r.z + off[2])};
    if (idx_in_map(g, id) && bit_at(occ, (long)id[0] * g.nyz + (long)id[1] * g.nz + id[2])) return true;
    ray_advance(r);
  }
  return true;
}

// distToPathAndCurPos (:452-473) and the weight of :286: cp [n][3], len the polyline's prefix lengths from index 0
__host__ __device__ inline double ig_weight(const double* cp, const double* len, int n, const double p[3], double lambda1,
                                            double lambda2) {
  double min_squ = 1.7976931348623157e308;
  int idx = 0;
  for (int i = 0; i < n; ++i) {
    const double dx = cp[3 * i] - p[0], dy = cp[3 * i + 1] - p[1], dz = cp[3 * i + 2] - p[2];
    const double squ = dx * dx + dy * dy + dz * dz;
    if (squ < min_squ) min_squ = squ, idx = i;
  }
  const double d1 = sqrt(min_squ), d2 = len[idx];
  return exp(-lambda1 * d1 - lambda2 * d2);
}

// the dynamic LDS of k_info_gain for `cells` cells (a multiple of 64): weights, control points and their prefix lengths
// under NON_UNIFORM; the masks; the waves' ray counts
__host__ __device__ inline size_t ig_lds(int cells, bool weighted, int max_ctrl) {
  return (weighted ? ((size_t)cells + 4 * (size_t)max_ctrl) * sizeof(double) : 0) + (size_t)cells * sizeof(unsigned) + 16;
}

__global__ void __launch_bounds__(IG_NT) k_info_gain(Geo g, GainArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int b = blockIdx.x;
  const GainGroup G = A.groups[b];
  if (G.n_yaw <= 0 || G.cells <= 0 || G.cells > A.lds_cells) return;  // (the outputs were zeroed in front of the launch)
  const bool weighted = A.cfg.weight_type == FUELMI_GAIN_NON_UNIFORM;
  const int max_ctrl = A.cfg.max_ctrl;
  double* wgt = reinterpret_cast<double*>(smem_raw);                    // [lds_cells]
  double* cp = wgt + (weighted ? A.lds_cells : 0);                      // [max_ctrl][3]
  double* len = cp + (weighted ? 3 * max_ctrl : 0);                     // [max_ctrl]
  unsigned* mask = reinterpret_cast<unsigned*>(len + (weighted ? max_ctrl : 0));  // [lds_cells]
  int* rays = reinterpret_cast<int*>(mask + A.lds_cells);
  const GainView* views = A.views + (size_t)b * A.cfg.max_yaw;
  int nc = 0;

  // 0. the group's control points and their prefix lengths
  if (weighted) {
    nc = A.n_ctrl[G.path];
    const double* src = A.ctrl + (size_t)G.path * max_ctrl * 3;
    for (int i = tid; i < 3 * nc; i += IG_NT) cp[i] = src[i];
  }
  __syncthreads();
  if (weighted && tid == 0) {
    len[0] = 0.0;
    for (int i = 0; i + 1 < nc; ++i)
      len[i + 1] = len[i] + ig_norm3(cp[3 * i + 3] - cp[3 * i], cp[3 * i + 4] - cp[3 * i + 1], cp[3 * i + 5] - cp[3 * i + 2]);
  }
  __syncthreads();

  // 1. the cells, IG_NT a step: member mask, one ray, the weight
  const int f = A.cfg.factor;
  int n_walked = 0;
  for (int c0 = 0; c0 < G.cells; c0 += IG_NT) {
    const int c = c0 + tid;
    unsigned mem = 0u;
    if (c < G.cells) {
      const int iz = c % G.ud[2], t = c / G.ud[2], iy = t % G.ud[1], ix = t / G.ud[1];
      const int id[3] = {(G.u0[0] + ix) * f, (G.u0[1] + iy) * f, (G.u0[2] + iz) * f};
      double p[3] = {0.0, 0.0, 0.0};
      bool go = idx_in_map(g, id) && bit_at(A.unk, (long)id[0] * g.nyz + (long)id[1] * g.nz + id[2]);  // :275
      if (go && A.cfg.in_box)                                                                          // :276
        for (int k = 0; k < 3; ++k) go = go && id[k] >= A.bmin[k] && id[k] < A.bmax[k];
      if (go) {  // indexToPos, insideFoV (:475-487)
        for (int k = 0; k < 3; ++k) p[k] = (id[k] + 0.5) * g.res + g.org[k];
        const double dx = p[0] - G.pos[0], dy = p[1] - G.pos[1], dz = p[2] - G.pos[2];
        if (!(ig_norm3(dx, dy, dz) > A.cfg.far)) {
          for (int v = 0; v < G.n_yaw; ++v) {
            const GainView& V = views[v];
            bool in = true;
            for (int k = 0; k < 3; ++k) in = in && id[k] >= V.lb[k] && id[k] <= V.ub[k];
            for (int q = 0; in && q < 4; ++q)
              if (dx * V.nrm[q][0] + dy * V.nrm[q][1] + dz * V.nrm[q][2] < 0.1) in = false;
            if (in) mem |= 1u << v;
          }
        }
      }
      unsigned word = mem;
      double w = 0.0;
      if (mem) {
        if (!ig_ray_blocked(g, A.occ, A.off, p, G.pos)) {
          word |= IG_VISIBLE;
          if (weighted) w = ig_weight(cp, len, nc, p, A.cfg.lambda1, A.cfg.lambda2);
        }
      }
      mask[c] = word;
      if (weighted) wgt[c] = w;
    }
    n_walked += __popcll(__ballot(mem != 0u));  // (the wave's)
  }
  if (lane == 0) rays[wv] = n_walked;
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int k = 0; k < IG_NW; ++k) n += rays[k];
    A.n_rays[b] = n;
  }

  // 2. one wave per yaw; lane l owns the cells whose absolute subsampled (y, z) is (l / 8, l % 8) modulo 8
  const int iy0 = ((lane >> 3) - G.u0[1]) & 7, iz0 = ((lane & 7) - G.u0[2]) & 7;
  for (int v = wv; v < G.n_yaw; v += IG_NW) {
    int cand = 0, vis = 0;
    double sum = 0.0;
    for (int ix = 0; ix < G.ud[0]; ++ix)
      for (int iy = iy0; iy < G.ud[1]; iy += 8)
        for (int iz = iz0; iz < G.ud[2]; iz += 8) {
          const int c = (ix * G.ud[1] + iy) * G.ud[2] + iz;
          const unsigned word = mask[c];
          if (!((word >> v) & 1u)) continue;
          ++cand;
          if (word & IG_VISIBLE) {
            ++vis;
            if (weighted) sum = sum + wgt[c];
          }
        }
    for (int o = 32; o >= 1; o >>= 1) {
      cand += __shfl(cand, lane ^ o);
      vis += __shfl(vis, lane ^ o);
      const double other = __shfl(sum, lane ^ o);
      sum = sum + other;
    }
    if (lane == 0) {
      const size_t at = (size_t)b * A.cfg.max_yaw + v;
      A.n_cand[at] = cand, A.n_visible[at] = vis;
      A.gain[at] = weighted ? sum : (double)vis;
    }
  }
}

// Graph::penal (:42-49)
__host__ __device__ __forceinline__ double yp_penal(double diff, double dt, double max_yaw_rate) {
  const double yr = diff / dt;
  if (yr <= max_yaw_rate) return 0.0;
  return (yr - max_yaw_rate) * (yr - max_yaw_rate);  // pow(x, 2)
}

__global__ void __launch_bounds__(YP_NT) k_yaw_path(YawPathArgs Y) {
  __shared__ double s_g[2][32], s_yaw[2][32];
  __shared__ unsigned char s_par[YP_LAYERS][32];
  const int j = threadIdx.x, b = blockIdx.x;
  const int nl = Y.n_layer[b], nv = Y.nv, ml = Y.max_layer;
  if (Y.over[b]) {  // (the other outputs were zeroed in front of the launch)
    if (j == 0) Y.status[b] = -1;
    return;
  }
  const double* yaws = Y.yaws + (size_t)b * ml;
  const double dt = Y.dt[b];
  if (j == 0) s_g[0][0] = 0.0, s_yaw[0][0] = yaws[0];
  __syncthreads();
  int nprev = 1;
  for (int i = 1; i < nl; ++i) {  // (nl is the workgroup's)
    const bool last = i == nl - 1;
    const int ncur = last ? 1 : nv, pb = (i - 1) & 1, qb = i & 1;
    if (j < ncur) {
      const size_t at = ((size_t)b * ml + i) * nv + j;
      const double yb = last ? yaws[i] : yaws[i] + double(j - Y.h) * Y.yaw_diff;
      const double gain_b = last ? 0.0 : Y.gains[at];
      double gv = 0.0;
      int par = 0;
      for (int c = 0; c < nprev; ++c) {
        const double g_tmp = s_g[pb][c] - gain_b + Y.w * yp_penal(fabs(s_yaw[pb][c] - yb), dt, Y.max_yaw_rate);
        if (c == 0 || !(g_tmp > gv)) gv = g_tmp, par = c;
      }
      s_g[qb][j] = gv, s_yaw[qb][j] = yb;
      s_par[i][j] = (unsigned char)par;
      Y.g_value[at] = gv;
    }
    __syncthreads();
    nprev = ncur;
  }
  if (j == 0) {
    int v = 0;
    for (int i = nl - 1; i >= 1; --i) {
      Y.path_vertex[(size_t)b * ml + i] = v;
      Y.path[(size_t)b * ml + i] = i == nl - 1 ? yaws[i] : yaws[i] + double(v - Y.h) * Y.yaw_diff;
      v = s_par[i][v];
    }
    Y.path_vertex[(size_t)b * ml] = 0;
    Y.path[(size_t)b * ml] = yaws[0];
    Y.status[b] = 0;
  }
}

// One view on the host, libm and f64 in the reference's order: :240-255 and calcFovAABB (:401-418).  R_wb = Rz(yaw) and
// T_bc = T_cb^-1 = [[0, 0, 1], [-1, 0, 0], [0, 1, 0]] (:151-152) give R_wc = [[sin, 0, cos], [-cos, 0, sin], [0, 1, 0]]
// and t_wc = pt: every sum of the 4 x 4 product has one term that is not a zero.
void gain_view_setup(const fuelmi_gain_cfg& c, const Geo& g, const double bmind[3], const double bmaxd[3],
                     const double pt[3], double yaw, GainView& V) {
  const double sn = sin(yaw), cs = cos(yaw);
  const double R[3][3] = {{sn, 0.0, cs}, {-cs, 0.0, sn}, {0.0, 1.0, 0.0}};
  const double n[4][3] = {{0.0, sin(M_PI_2 - c.top_ang), cos(M_PI_2 - c.top_ang)},      // n_top_ (:122)
                          {0.0, -sin(M_PI_2 - c.top_ang), cos(M_PI_2 - c.top_ang)},     // n_bottom_
                          {sin(M_PI_2 - c.left_ang), 0.0, cos(M_PI_2 - c.left_ang)},    // n_left_ (:127)
                          {-sin(M_PI_2 - c.right_ang), 0.0, cos(M_PI_2 - c.right_ang)}};  // n_right_
  for (int q = 0; q < 4; ++q)
    for (int r = 0; r < 3; ++r) V.nrm[q][r] = R[r][0] * n[q][0] + R[r][1] * n[q][1] + R[r][2] * n[q][2];
  // :136-139: lefttop's x is the one tangent among the sines
  const double vert[4][3] = {{-c.far * tan(c.left_ang), -c.far * sin(c.top_ang), c.far},
                             {-c.far * sin(c.left_ang), c.far * sin(c.top_ang), c.far},
                             {c.far * sin(c.right_ang), -c.far * sin(c.top_ang), c.far},
                             {c.far * sin(c.right_ang), c.far * sin(c.top_ang), c.far}};
  double lbd[3], ubd[3];
  for (int r = 0; r < 3; ++r) lbd[r] = ubd[r] = pt[r];  // vertice[4] = t_wc lies in the box whatever the order
  for (int k = 0; k < 4; ++k)
    for (int r = 0; r < 3; ++r) {
      const double v = (R[r][0] * vert[k][0] + R[r][1] * vert[k][1] + R[r][2] * vert[k][2]) + pt[r];
      lbd[r] = std::min(lbd[r], v), ubd[r] = std::max(ubd[r], v);
    }
  const int nvx[3] = {g.nx, g.ny, g.nz};
  for (int r = 0; r < 3; ++r) {
    lbd[r] = std::max(lbd[r], bmind[r]), ubd[r] = std::min(ubd[r], bmaxd[r]);  // boundBox
    double lo = floor((lbd[r] - g.org[r]) * g.res_inv), hi = floor((ubd[r] - g.org[r]) * g.res_inv);  // posToIndex
    // cells outside the map are never unknown (:275): the box is cut to the map, in f64 before the cast
    lo = std::min(std::max(lo, 0.0), (double)nvx[r]), hi = std::min(std::max(hi, -1.0), (double)(nvx[r] - 1));
    V.lb[r] = (int)lo, V.ub[r] = (int)hi;
  }
}

// the union of the views' boxes in subsampled indices; false: more than IG_CAP cells
bool gain_group_box(const fuelmi_gain_cfg& c, const GainView* views, GainGroup& G) {
  int lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1};
  bool any = false;
  for (int v = 0; v < G.n_yaw; ++v) {
    int slo[3], shi[3];
    bool empty = false;
    for (int r = 0; r < 3; ++r) {
      slo[r] = (views[v].lb[r] + c.factor - 1) / c.factor;
      shi[r] = views[v].ub[r] < 0 ? -1 : views[v].ub[r] / c.factor;
      empty = empty || slo[r] > shi[r];
    }
    if (empty) continue;
    for (int r = 0; r < 3; ++r) {
      lo[r] = any ? std::min(lo[r], slo[r]) : slo[r];
      hi[r] = any ? std::max(hi[r], shi[r]) : shi[r];
    }
    any = true;
  }
  long cells = any ? 1 : 0;
  for (int r = 0; r < 3; ++r) {
    G.u0[r] = lo[r], G.ud[r] = any ? hi[r] - lo[r] + 1 : 0;
    cells *= G.ud[r];
  }
  if (cells > IG_CAP) {
    G.cells = 0;
    return false;
  }
  G.cells = (int)cells;
  return true;
}

bool fin3(const double* p) {
  return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::fabs(p[0]) < 1e7 &&
         std::fabs(p[1]) < 1e7 && std::fabs(p[2]) < 1e7;
}

int gain_cfg_check(const fuelmi_gain_cfg* c) {
  ARGCHK(c);
  ARGCHK(c->weight_type == FUELMI_GAIN_NON_UNIFORM || c->weight_type == FUELMI_GAIN_UNIFORM);
  ARGCHK(c->factor >= 1 && c->max_yaw >= 1);
  ARGCHK(std::isfinite(c->far) && c->far > 0.0 && c->far <= 1e3);
  ARGCHK(std::isfinite(c->top_ang) && std::isfinite(c->left_ang) && std::isfinite(c->right_ang));
  ARGCHK(std::isfinite(c->lambda1) && std::isfinite(c->lambda2));
  if (c->weight_type == FUELMI_GAIN_NON_UNIFORM) ARGCHK(c->max_ctrl >= 1);
  if (c->max_yaw > IG_YAWS || c->max_ctrl > IG_CTRL) {
    fuelmi_set_error("information gain: max_yaw %d / max_ctrl %d exceed %d / %d", c->max_yaw, c->max_ctrl, IG_YAWS, IG_CTRL);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

int ctrl_check(const fuelmi_gain_cfg& c, int n_path, const int* n_ctrl, const double* ctrl) {
  ARGCHK(n_path >= 1 && n_ctrl && ctrl);
  for (int p = 0; p < n_path; ++p) {
    ARGCHK(n_ctrl[p] >= 1 && n_ctrl[p] <= c.max_ctrl);
    for (int i = 0; i < n_ctrl[p]; ++i) ARGCHK(fin3(ctrl + ((size_t)p * c.max_ctrl + i) * 3));
  }
  return FUELMI_OK;
}

int yawpath_cfg_check(const fuelmi_yawpath_cfg* cfg, fuelmi_gain_cfg& gc) {
  ARGCHK(cfg);
  ARGCHK(cfg->half_vert_num >= 0 && cfg->max_layer >= 1);
  ARGCHK(std::isfinite(cfg->yaw_diff) && std::isfinite(cfg->max_yaw_rate) && std::isfinite(cfg->w));
  if (cfg->half_vert_num > (IG_YAWS - 1) / 2 || cfg->max_layer > YP_LAYERS) {
    fuelmi_set_error("yaw paths: half_vert_num %d / max_layer %d exceed %d / %d", cfg->half_vert_num, cfg->max_layer,
                     (IG_YAWS - 1) / 2, YP_LAYERS);
    return FUELMI_ELIMIT;
  }
  gc = cfg->gain;
  gc.max_yaw = 2 * cfg->half_vert_num + 1;
  return gain_cfg_check(&gc);
}

// what a yaw-path call adds to the gain launch (host pointers)
struct YawPathCall {
  const fuelmi_yawpath_cfg* cfg;
  int n_prob;
  const int* n_layer;
  const double *yaws, *dt, *gains_in;
  const int* over;  // [n_prob]
  int* status;
  double* path;
  int* path_vertex;
  double* g_value;
};

// The launches of both calls: the gain kernel over `groups` (skipped when the gains are given), then the search.  gain /
// n_cand / n_visible [n_group][max_yaw] and n_rays [n_group] are host arrays (n_cand / n_visible may be null).
int heading_run(fuelmi_map* m, const fuelmi_gain_cfg& gc, const std::vector<GainGroup>& groups,
                const std::vector<GainView>& views, int n_path, const int* n_ctrl, const double* ctrl, double* gain,
                int* n_cand, int* n_visible, int* n_rays, const YawPathCall* yp) {
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  const size_t ng = groups.size(), my = (size_t)gc.max_yaw, mc = (size_t)gc.max_ctrl;
  const bool weighted = gc.weight_type == FUELMI_GAIN_NON_UNIFORM;
  const bool walk = !(yp && yp->gains_in);
  const size_t np = weighted && walk ? (size_t)n_path : 0;
  const size_t n = yp ? (size_t)yp->n_prob : 0, ml = yp ? (size_t)yp->cfg->max_layer : 0;
  GainArgs A;
  memset(&A, 0, sizeof(A));
  YawPathArgs Y;
  memset(&Y, 0, sizeof(Y));
  GainGroup* d_groups;
  GainView* d_views;
  int *d_nctrl, *d_nlayer, *d_over;
  double *d_ctrl, *d_yaws, *d_dt;
  ResultBlock R(16);  // n_cand / n_visible are always in the block and copied where the caller asks; no search: n = 0
  R.add(A.gain, gain, ng * my);
  R.add(A.n_cand, n_cand, ng * my);
  R.add(A.n_visible, n_visible, ng * my);
  R.add(A.n_rays, n_rays, ng);
  R.add(Y.status, yp ? yp->status : nullptr, n);
  R.add(Y.path, yp ? yp->path : nullptr, n * ml);
  R.add(Y.path_vertex, yp ? yp->path_vertex : nullptr, n * ml);
  R.add(Y.g_value, yp ? yp->g_value : nullptr, n * ml * my);
  ARGCHK(!R.overflow);
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 16);
    d_groups = L.take<GainGroup>(ng);
    d_views = L.take<GainView>(ng * my);
    d_nctrl = L.take<int>(np);
    d_ctrl = L.take<double>(np * mc * 3);
    d_nlayer = L.take<int>(n);
    d_over = L.take<int>(n);
    d_yaws = L.take<double>(n * ml);
    d_dt = L.take<double>(n);
    R.place(L);
    return L.size();
  };
  {
    const int rc = m->heading_dev.carve(st, layout);
    if (rc) return rc;
  }
  HIPCHK(hipMemsetAsync(R.base, 0, R.size(), st));
  if (walk) {
    HIPCHK(hipMemcpyAsync(d_groups, groups.data(), ng * sizeof(GainGroup), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_views, views.data(), ng * my * sizeof(GainView), hipMemcpyHostToDevice, st));
    if (np) {
      HIPCHK(hipMemcpyAsync(d_nctrl, n_ctrl, np * sizeof(int), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(d_ctrl, ctrl, np * mc * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    }
    int cells = 0;
    for (const GainGroup& G : groups) cells = std::max(cells, G.n_yaw > 0 ? G.cells : 0);
    if (cells > 0) {
      A.cfg = gc;
      A.n_group = (int)ng;
      A.lds_cells = (cells + 63) & ~63;
      for (int k = 0; k < 3; ++k) {
        A.off[k] = 0.5 - m->g.org[k] / m->g.res;
        A.bmin[k] = m->info.box_min[k], A.bmax[k] = m->info.box_max[k];
      }
      A.unk = m->unk_bits.p, A.occ = m->occ_bits.p;
      A.groups = d_groups, A.views = d_views, A.n_ctrl = d_nctrl, A.ctrl = d_ctrl;
      const size_t lds = ig_lds(A.lds_cells, weighted, gc.max_ctrl);
      if (lds > 64 * 1024)  // (the attribute is the function's: always the kernel's ceiling)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_info_gain), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)ig_lds(IG_CAP, true, IG_CTRL)));
      hipLaunchKernelGGL(k_info_gain, dim3((unsigned)ng), dim3(IG_NT), lds, st, m->g, A);
      HIPCHK(hipGetLastError());
    }
  } else {
    HIPCHK(hipMemcpyAsync(A.gain, yp->gains_in, ng * my * sizeof(double), hipMemcpyHostToDevice, st));
  }
  if (yp) {
    HIPCHK(hipMemcpyAsync(d_nlayer, yp->n_layer, n * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_over, yp->over, n * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_yaws, yp->yaws, n * ml * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_dt, yp->dt, n * sizeof(double), hipMemcpyHostToDevice, st));
    Y.n_prob = yp->n_prob, Y.max_layer = yp->cfg->max_layer, Y.nv = gc.max_yaw, Y.h = yp->cfg->half_vert_num;
    Y.yaw_diff = yp->cfg->yaw_diff, Y.max_yaw_rate = yp->cfg->max_yaw_rate, Y.w = yp->cfg->w;
    Y.n_layer = d_nlayer, Y.yaws = d_yaws, Y.dt = d_dt, Y.gains = A.gain, Y.over = d_over;
    hipLaunchKernelGGL(k_yaw_path, dim3((unsigned)n), dim3(YP_NT), 0, st, Y);
    HIPCHK(hipGetLastError());
  }
  return result_fetch(R, st);
}

}  // namespace

extern "C" int fuelmi_yawpath_plan(const fuelmi_yawpath_cfg* cfg, int out10[10]) {
  ARGCHK(out10);
  fuelmi_gain_cfg gc;
  {
    const int rc = yawpath_cfg_check(cfg, gc);
    if (rc) return rc;
  }
  out10[0] = IG_NT, out10[1] = (int)ig_lds(IG_CAP, gc.weight_type == FUELMI_GAIN_NON_UNIFORM, gc.max_ctrl), out10[2] = 1;
  out10[3] = IG_CAP, out10[4] = IG_YAWS, out10[5] = IG_CTRL;
  out10[6] = YP_NT, out10[7] = (int)(4 * 32 * sizeof(double) + YP_LAYERS * 32), out10[8] = 1, out10[9] = YP_LAYERS;
  return FUELMI_OK;
}

extern "C" int fuelmi_map_info_gains(fuelmi_map* m, const fuelmi_gain_cfg* cfg, int n_group, const double* pos,
                                     const int* n_yaw, const double* yaws, int n_path, const int* n_ctrl,
                                     const double* ctrl, const int* path_of, int* status, double* gain, int* n_cand,
                                     int* n_visible, int* n_rays) {
  {  // every argument on the host, before the map is touched
    const int rc = gain_cfg_check(cfg);
    if (rc) return rc;
  }
  ARGCHK(n_group >= 0);
  if (n_group == 0) return FUELMI_OK;
  ARGCHK(pos && n_yaw && yaws && status && gain && n_cand && n_visible && n_rays);
  const bool weighted = cfg->weight_type == FUELMI_GAIN_NON_UNIFORM;
  if (weighted) {
    const int rc = ctrl_check(*cfg, n_path, n_ctrl, ctrl);
    if (rc) return rc;
    ARGCHK(path_of);
  }
  const size_t my = (size_t)cfg->max_yaw;
  for (int b = 0; b < n_group; ++b) {
    ARGCHK(n_yaw[b] >= 0 && n_yaw[b] <= cfg->max_yaw);
    ARGCHK(fin3(pos + 3 * (size_t)b));
    for (int v = 0; v < n_yaw[b]; ++v) ARGCHK(std::isfinite(yaws[b * my + v]) && std::fabs(yaws[b * my + v]) < 1e7);
    if (weighted) ARGCHK(path_of[b] >= 0 && path_of[b] < n_path);
  }
  ARGCHK(m);
  std::vector<GainGroup> groups((size_t)n_group);
  std::vector<GainView> views((size_t)n_group * my);
  memset(views.data(), 0, views.size() * sizeof(GainView));
  int over = -1;
  for (int b = 0; b < n_group; ++b) {
    GainGroup& G = groups[b];
    memset(&G, 0, sizeof(G));
    for (int k = 0; k < 3; ++k) G.pos[k] = pos[3 * (size_t)b + k];
    G.n_yaw = n_yaw[b], G.path = weighted ? path_of[b] : 0;
    for (int v = 0; v < G.n_yaw; ++v)
      gain_view_setup(*cfg, m->g, m->cfg.box_min, m->cfg.box_max, G.pos, yaws[b * my + v], views[b * my + v]);
    status[b] = 0;
    if (!gain_group_box(*cfg, views.data() + b * my, G)) {
      G.n_yaw = 0, status[b] = -1;
      if (over < 0) over = b;
    }
  }
  {
    const int rc = heading_run(m, *cfg, groups, views, n_path, n_ctrl, ctrl, gain, n_cand, n_visible, n_rays, nullptr);
    if (rc) return rc;
  }
  if (over >= 0) {
    fuelmi_set_error("information gain: group %d holds more than %d subsampled cells", over, IG_CAP);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

extern "C" int fuelmi_map_yaw_paths(fuelmi_map* m, const fuelmi_yawpath_cfg* cfg, int n_prob, const int* n_layer,
                                    const double* pts, const double* yaws, const double* dt, const int* n_ctrl,
                                    const double* ctrl, const double* gains_in, int* status, double* path,
                                    int* path_vertex, double* gains, double* g_value, int* n_rays) {
  fuelmi_gain_cfg gc;
  {
    const int rc = yawpath_cfg_check(cfg, gc);
    if (rc) return rc;
  }
  ARGCHK(n_prob >= 0);
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(n_layer && pts && yaws && dt && status && path && path_vertex && gains && g_value && n_rays);
  const bool weighted = gc.weight_type == FUELMI_GAIN_NON_UNIFORM && !gains_in;
  if (weighted) {
    const int rc = ctrl_check(gc, n_prob, n_ctrl, ctrl);
    if (rc) return rc;
  }
  const size_t ml = (size_t)cfg->max_layer, nv = (size_t)gc.max_yaw;
  const int h = cfg->half_vert_num;
  for (int b = 0; b < n_prob; ++b) {
    ARGCHK(n_layer[b] >= 1 && n_layer[b] <= cfg->max_layer);
    ARGCHK(std::isfinite(dt[b]) && dt[b] > 0.0);
    for (int i = 0; i < n_layer[b]; ++i) {
      ARGCHK(fin3(pts + (b * ml + i) * 3));
      ARGCHK(std::isfinite(yaws[b * ml + i]) && std::fabs(yaws[b * ml + i]) < 1e7);
      if (gains_in && i >= 1 && i < n_layer[b] - 1)
        for (size_t j = 0; j < nv; ++j) ARGCHK(std::isfinite(gains_in[(b * ml + i) * nv + j]));
    }
  }
  ARGCHK(m);
  const size_t ng = (size_t)n_prob * ml;
  std::vector<GainGroup> groups(ng);
  std::vector<GainView> views(gains_in ? 0 : ng * nv);
  std::vector<int> over((size_t)n_prob, 0);
  memset(groups.data(), 0, ng * sizeof(GainGroup));
  if (!gains_in) {
    memset(views.data(), 0, views.size() * sizeof(GainView));
    for (int b = 0; b < n_prob; ++b)
      for (int i = 1; i < n_layer[b] - 1; ++i) {  // the inner layers (:187-203)
        const size_t gi = b * ml + i;
        GainGroup& G = groups[gi];
        for (int k = 0; k < 3; ++k) G.pos[k] = pts[gi * 3 + k];
        G.n_yaw = (int)nv, G.path = weighted ? b : 0;
        for (int j = 0; j < (int)nv; ++j)
          gain_view_setup(gc, m->g, m->cfg.box_min, m->cfg.box_max, G.pos, yaws[gi] + double(j - h) * cfg->yaw_diff,
                          views[gi * nv + j]);
        if (!gain_group_box(gc, views.data() + gi * nv, G)) G.n_yaw = 0, over[b] = 1;
      }
    for (int b = 0; b < n_prob; ++b)
      if (over[b])  // no ray is walked for a problem that cannot finish
        for (size_t i = 0; i < ml; ++i) groups[b * ml + i].n_yaw = 0;
  }
  YawPathCall yp = {cfg, n_prob, n_layer, yaws, dt, gains_in, over.data(), status, path, path_vertex, g_value};
  {
    const int rc = heading_run(m, gc, groups, views, n_prob, n_ctrl, ctrl, gains, nullptr, nullptr, n_rays, &yp);
    if (rc) return rc;
  }
  const int b = first_over_limit(status, n_prob);
  if (b < 0) return FUELMI_OK;
  fuelmi_set_error("yaw paths: a layer of problem %d holds more than %d subsampled cells", b, IG_CAP);
  return FUELMI_ELIMIT;
}
