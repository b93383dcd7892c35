// quad_solve.hip -- the exact minimiser of the optimiser's quadratic phases: BsplineOptimizer::optimize()
// (bspline_opt/src/bspline_optimizer.cpp:110-253) for a cost mask within SMOOTHNESS | START | END | GUIDE | WAYPOINTS,
// for a ragged batch of problems (each its own number of control points), dimension 1 or 3.
//
// With the knot span fixed and pt_dist_ frozen from the initial control points (:136-140), every term of combineCost
// (:571-630) is a sum of c (a . q - b)^2 over at most four neighbouring control points, the same a for every axis:
//     ld_smooth (J . q[i..i+3] / pt_dist)^2,  J = (-1, 3, -3, 1)                       i = 0 .. N-4      (:263-266)
//     10 ld_start (P . q[0..2] - s0)^2 + ld_start (V . q[0..2] - s1)^2 + ld_start (A . q[0..2] - s2)^2   (:369-389)
//     ld_end ((P . q[N-3..] - e0)^2 [+ (V . q[N-3..] - e1)^2 [+ (A . q[N-3..] - e2)^2]])     end_n rows  (:407-430)
//     ld_guide (q[i] - guide[i - order])^2                                             i = order .. N-order-1  (:468-474)
//     ld_waypt (P . q[i..i+2] - w)^2                                                   way-point indices i     (:442-456)
//     P = (1, 4, 1) / 6,  V = (-1, 0, 1) / (2 dt),  A = (1, -2, 1) / dt^2
// so the minimiser solves H q = g, H = sum c a a^T symmetric of half-bandwidth 3, one right-hand side per axis.  One lane
// per row gathers its four diagonals and its right-hand sides (lanes loop past 64 rows), lane 0 factors the band once by
// Cholesky (the loops of k_yaw_plan), lanes 0 .. dim-1 substitute their axis side by side, and the objective at the result
// is summed in combineCost's order: per row across the axes, rows left to right.
//
// One wave of QS_NT lanes per problem, all f64, -ffp-contract=off, every scratch array in dynamic LDS.  A result does not
// depend on the problem's place in the batch.  Behind the kernel, the two entries that share its checks, argument fill and
// result layout: fuelmi_map_solve_quadratic (through a query slot) and fuelmi_bspline_dev_solve_quadratic (what a device
// batch holds, bspline_batch.h).
#include <cmath>
#include <cstring>
#include <vector>

#include "bspline_batch.h"

namespace {

constexpr int QS_NT = 64;
constexpr int QS_MASK = FUELMI_COST_SMOOTHNESS | FUELMI_COST_START | FUELMI_COST_END | FUELMI_COST_GUIDE | FUELMI_COST_WAYPOINTS;

// k_quad_solve: one problem per wave; every pointer addresses memory the device can reach
struct QuadArgs {
  int mask, dim, max_ctrl, end_n, max_waypt, bounds, order, n_prob;
  double ld_smooth, ld_start, ld_end, ld_guide, ld_waypt;
  double box_lo[3], box_hi[3];  // the map's box shrunk by 0.1 (:174-180)
  const int* n_ctrl;            // [n], or null: every problem has n_ctrl_all control points
  int n_ctrl_all;
  const double* ctrl;           // problem b: [n_ctrl][dim] at ctrl + b * ctrl_stride
  size_t ctrl_stride;
  const double* knot_span;      // [n]
  int vs;                       // doubles per row of the states, guide points and way-points (dim, or 3 in a device batch)
  const double* start_state;    // [n][3][vs]
  const double* end_state;      // [n][3][vs]
  const double* guide;          // problem b: [N - 2 order][vs] at guide + b * guide_stride
  size_t guide_stride;
  const int* n_waypt;           // [n], or null: every problem has n_waypt_all way-points
  int n_waypt_all;
  const double* waypts;         // [n][max_waypt][vs]
  const int* waypt_idx;         // [n][max_waypt]
  int* status;
  double* ctrl_out;             // [n][max_ctrl][dim]
  double* cost;
  double* pt_dist;
  // a device batch: where the next solve starts.  Written for FUELMI_QUAD_OK only
  double* x_next;               // problem b: [n_ctrl][dim] at x_next + b * x_next_stride, or null
  size_t x_next_stride;
  double* pt_dist_next;         // [n] or null: pt_dist_ of the solution
};

__host__ __device__ inline size_t qs_lds_doubles(int max_ctrl, int dim) {
  return (size_t)max_ctrl * (size_t)(4 + 1 + 3 * dim) + 16;
}

__device__ __forceinline__ double qs_J(int k) { return k == 0 ? -1.0 : k == 1 ? 3.0 : k == 2 ? -3.0 : 1.0; }
__device__ __forceinline__ double qs_P(int k) { return k == 1 ? 4.0 / 6.0 : 1.0 / 6.0; }
__device__ __forceinline__ double qs_V(int k, double dt) { return (k == 0 ? -1.0 : k == 1 ? 0.0 : 1.0) / (2 * dt); }
__device__ __forceinline__ double qs_A(int k, double dt) { return (k == 1 ? -2.0 : 1.0) / (dt * dt); }

// sum of |q[i+1] - q[i]| over N (:136-140): the norms side by side into t[], lane 0 adds them left to right.  Every
// lane of the wave calls it; the value comes back in *out (LDS)
__device__ void qs_pt_dist(const double* q, int N, int dim, int tid, double* t, double* out) {
  for (int i = tid; i + 1 < N; i += QS_NT) {
    double s = 0.0;
    for (int k = 0; k < dim; ++k) {
      const double d = q[dim * (i + 1) + k] - q[dim * i + k];
      s += d * d;
    }
    t[i] = sqrt(s);
  }
  __syncthreads();
  if (tid == 0) {
    double pd = 0.0;
    for (int i = 0; i + 1 < N; ++i) pd += t[i];
    *out = pd / (double)N;
  }
  __syncthreads();
}

// combineCost (:571-630) at the points q [N][dim]: the jerk and guide rows side by side into t[] (2 N doubles), then
// lane 0 adds every term in the reference's order.  Every lane of the wave calls it; the value comes back in *out (LDS)
__device__ void qs_cost(const QuadArgs& Q, int b, const double* q, int N, double dt, double pt_dist, int nw, int tid,
                        double* t, double* out) {
  const int dim = Q.dim, vs = Q.vs, order = Q.order;
  const double* gp = Q.guide + (size_t)b * Q.guide_stride;
  if (Q.mask & FUELMI_COST_SMOOTHNESS)
    for (int i = tid; i + 3 < N; i += QS_NT) {
      double s = 0.0;
      for (int k = 0; k < dim; ++k) {
        const double ji = (q[dim * (i + 3) + k] - 3 * q[dim * (i + 2) + k] + 3 * q[dim * (i + 1) + k] - q[dim * i + k]) / pt_dist;
        s += ji * ji;
      }
      t[i] = s;
    }
  if (Q.mask & FUELMI_COST_GUIDE)
    for (int i = order + tid; i < N - order; i += QS_NT) {
      double s = 0.0;
      for (int k = 0; k < dim; ++k) {
        const double d = q[dim * i + k] - gp[(size_t)(i - order) * vs + k];
        s += d * d;
      }
      t[N + i] = s;
    }
  __syncthreads();
  if (tid == 0) {
    double cost = 0.0, dq;
    if (Q.mask & FUELMI_COST_SMOOTHNESS) {
      double fs = 0.0;
      for (int i = 0; i + 3 < N; ++i) fs += t[i];
      cost += Q.ld_smooth * fs;
    }
    if (Q.mask & FUELMI_COST_START) {
      const double* S = Q.start_state + (size_t)b * 3 * vs;
      double f0 = 0.0, s;
      s = 0.0;
      for (int k = 0; k < dim; ++k) {
        dq = 1 / 6.0 * (q[k] + 4 * q[dim + k] + q[2 * dim + k]) - S[k];
        s += dq * dq;
      }
      f0 += 10.0 * s;
      s = 0.0;
      for (int k = 0; k < dim; ++k) {
        dq = 1 / (2 * dt) * (q[2 * dim + k] - q[k]) - S[vs + k];
        s += dq * dq;
      }
      f0 += s;
      s = 0.0;
      for (int k = 0; k < dim; ++k) {
        dq = 1 / (dt * dt) * (q[k] - 2 * q[dim + k] + q[2 * dim + k]) - S[2 * vs + k];
        s += dq * dq;
      }
      f0 += s;
      cost += Q.ld_start * f0;
    }
    if (Q.mask & FUELMI_COST_END) {
      const double* E = Q.end_state + (size_t)b * 3 * vs;
      const double *q3 = q + dim * (N - 3), *q2 = q + dim * (N - 2), *q1 = q + dim * (N - 1);
      double fe = 0.0, s;
      s = 0.0;
      for (int k = 0; k < dim; ++k) {
        dq = 1 / 6.0 * (q1[k] + 4 * q2[k] + q3[k]) - E[k];
        s += dq * dq;
      }
      fe += s;
      if (Q.end_n >= 2) {
        s = 0.0;
        for (int k = 0; k < dim; ++k) {
          dq = 1 / (2 * dt) * (q1[k] - q3[k]) - E[vs + k];
          s += dq * dq;
        }
        fe += s;
      }
      if (Q.end_n == 3) {
        s = 0.0;
        for (int k = 0; k < dim; ++k) {
          dq = 1 / (dt * dt) * (q1[k] - 2 * q2[k] + q3[k]) - E[2 * vs + k];
          s += dq * dq;
        }
        fe += s;
      }
      cost += Q.ld_end * fe;
    }
    if (Q.mask & FUELMI_COST_GUIDE) {
      double fg = 0.0;
      for (int i = order; i < N - order; ++i) fg += t[N + i];
      cost += Q.ld_guide * fg;
    }
    if (Q.mask & FUELMI_COST_WAYPOINTS) {
      const double* W = Q.waypts + (size_t)b * Q.max_waypt * vs;
      const int* I = Q.waypt_idx + (size_t)b * Q.max_waypt;
      double fw = 0.0;
      for (int j = 0; j < nw; ++j) {
        const int i = I[j];
        double s = 0.0;
        for (int k = 0; k < dim; ++k) {
          dq = 1 / 6.0 * (q[dim * i + k] + 4 * q[dim * (i + 1) + k] + q[dim * (i + 2) + k]) - W[(size_t)j * vs + k];
          s += dq * dq;
        }
        fw += s;
      }
      cost += Q.ld_waypt * fw;
    }
    *out = cost;
  }
  __syncthreads();
}

// q0 of optimize(): the input clamped into the shrunk box (:197-202)
__device__ __forceinline__ double qs_clamp(const QuadArgs& Q, double v, int k) {
  return fmax(fmin(v, Q.box_hi[k]), Q.box_lo[k]);
}

__global__ void __launch_bounds__(QS_NT) k_quad_solve(QuadArgs Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int dim = Q.dim, maxn = Q.max_ctrl, vs = Q.vs, order = Q.order;
  double* qin = reinterpret_cast<double*>(smem_raw);  // [maxn][dim]  the input control points
  double* band = qin + (size_t)dim * maxn;            // [maxn][4]    H(r, r - d) at [r][d], then its Cholesky factor; scratch
  double* g = band + 4 * (size_t)maxn;                // [maxn][dim]  right-hand sides, then the minimiser
  double* wc = g + (size_t)dim * maxn;                // [maxn]       way-points at index i
  double* ws = wc + maxn;                             // [maxn][dim]  their sum
  double* sh = ws + (size_t)dim * maxn;               // [16]

  const int N = Q.n_ctrl ? Q.n_ctrl[b] : Q.n_ctrl_all;
  const double dt = Q.knot_span[b];
  double* out = Q.ctrl_out + (size_t)b * maxn * dim;
  // (the host refuses these before any launch wherever it sees them; the variables of a device batch it does not see)
  if (N < 4 || N < order + 1 || N > maxn || !(dt > 0.0) || !isfinite(dt)) {
    for (int e = tid; e < maxn * dim; e += QS_NT) out[e] = 0.0;
    if (tid == 0) Q.status[b] = FUELMI_QUAD_DEGENERATE, Q.cost[b] = 0.0, Q.pt_dist[b] = 0.0;
    return;
  }
  const bool smooth = (Q.mask & FUELMI_COST_SMOOTHNESS) != 0;
  const int nw = (Q.mask & FUELMI_COST_WAYPOINTS) ? (Q.n_waypt ? Q.n_waypt[b] : Q.n_waypt_all) : 0;
  const double* Cin = Q.ctrl + (size_t)b * Q.ctrl_stride;

  // 1. the input; pt_dist_ from it, unclamped (:136-140); the way-points summed per index, in the order given
  for (int e = tid; e < dim * N; e += QS_NT) qin[e] = Cin[e];
  for (int i = tid; i < N; i += QS_NT) {
    wc[i] = 0.0;
    for (int k = 0; k < dim; ++k) ws[dim * i + k] = 0.0;
  }
  __syncthreads();
  qs_pt_dist(qin, N, dim, tid, band, &sh[0]);
  const double pt_dist = sh[0];
  if (tid == 0) {
    bool bad = smooth && (pt_dist == 0.0 || !isfinite(pt_dist));
    const double* W = Q.waypts + (size_t)b * Q.max_waypt * vs;
    const int* I = Q.waypt_idx + (size_t)b * Q.max_waypt;
    for (int j = 0; j < nw; ++j) {
      const int i = I[j];
      if (i < 0 || i > N - 3) {
        bad = true;
        break;
      }
      wc[i] += 1.0;
      for (int k = 0; k < dim; ++k) ws[dim * i + k] += W[(size_t)j * vs + k];
    }
    sh[1] = bad ? 1.0 : 0.0;
  }
  __syncthreads();
  bool degenerate = sh[1] != 0.0;

  if (!degenerate) {
    // 2. one lane per row of the normal equations
    const double cs = smooth ? Q.ld_smooth : 0.0;
    const bool has_s = (Q.mask & FUELMI_COST_START) != 0, has_e = (Q.mask & FUELMI_COST_END) != 0;
    const double cp = 10.0 * Q.ld_start, cv = Q.ld_start, ce = Q.ld_end, cg = Q.ld_guide, cw = Q.ld_waypt;
    const double* S = Q.start_state + (size_t)b * 3 * vs;
    const double* E = Q.end_state + (size_t)b * 3 * vs;
    const double* gp = Q.guide + (size_t)b * Q.guide_stride;
    for (int r = tid; r < N; r += QS_NT) {
      double h[4] = {0.0, 0.0, 0.0, 0.0}, gr[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int c = r - d;
        if (c < 0) continue;
        double hd = 0.0;
        if (smooth) {
          double s = 0.0;
          for (int i = max(0, r - 3); i <= min(c, N - 4); ++i) s += (qs_J(r - i) / pt_dist) * (qs_J(c - i) / pt_dist);
          hd += cs * s;
        }
        if (has_s && r <= 2)
          hd += cp * (qs_P(r) * qs_P(c)) + cv * (qs_V(r, dt) * qs_V(c, dt)) + cv * (qs_A(r, dt) * qs_A(c, dt));
        if (has_e && c >= N - 3) {
          const int rr = r - (N - 3), cc = c - (N - 3);
          double t = qs_P(rr) * qs_P(cc);
          if (Q.end_n >= 2) t += qs_V(rr, dt) * qs_V(cc, dt);
          if (Q.end_n == 3) t += qs_A(rr, dt) * qs_A(cc, dt);
          hd += ce * t;
        }
        if (nw > 0) {
          double sw = 0.0;
          for (int i = max(0, r - 2); i <= min(c, N - 3); ++i) sw += wc[i] * (qs_P(r - i) * qs_P(c - i));
          hd += cw * sw;
        }
        h[d] = hd;
      }
      const bool guided = (Q.mask & FUELMI_COST_GUIDE) && r >= order && r < N - order;
      if (guided) h[0] += cg;
      for (int k = 0; k < dim; ++k) {
        double v = 0.0;
        if (has_s && r <= 2) v += cp * (S[k] * qs_P(r)) + cv * (S[vs + k] * qs_V(r, dt)) + cv * (S[2 * vs + k] * qs_A(r, dt));
        if (has_e && r >= N - 3) {
          const int rr = r - (N - 3);
          double t = E[k] * qs_P(rr);
          if (Q.end_n >= 2) t += E[vs + k] * qs_V(rr, dt);
          if (Q.end_n == 3) t += E[2 * vs + k] * qs_A(rr, dt);
          v += ce * t;
        }
        if (guided) v += cg * gp[(size_t)(r - order) * vs + k];
        if (nw > 0) {
          double sw = 0.0;
          for (int i = max(0, r - 2); i <= min(r, N - 3); ++i) sw += ws[dim * i + k] * qs_P(r - i);
          v += cw * sw;
        }
        gr[k] = v;
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) band[4 * r + d] = h[d];
      for (int k = 0; k < dim; ++k) g[dim * r + k] = gr[k];
    }
    __syncthreads();

    // 3. lane 0: banded Cholesky (the loops of k_yaw_plan), once for every axis
    if (tid == 0) {
      constexpr int hb = 3;
      bool bad = false;
      for (int j = 0; j < N && !bad; ++j) {
        double s = band[4 * j];
        for (int d = 1; d <= hb && d <= j; ++d) s -= band[4 * j + d] * band[4 * j + d];
        if (!(s > 0.0) || !isfinite(s)) {
          bad = true;
          break;
        }
        const double ljj = sqrt(s);
        band[4 * j] = ljj;
        for (int i = j + 1; i <= j + hb && i < N; ++i) {
          double t = band[4 * i + (i - j)];
          for (int k = max(0, i - hb); k < j; ++k) t -= band[4 * i + (i - k)] * band[4 * j + (j - k)];
          band[4 * i + (i - j)] = t / ljj;
        }
      }
      sh[1] = bad ? 1.0 : 0.0;
    }
    __syncthreads();
    degenerate = sh[1] != 0.0;
  }

  if (!degenerate) {
    // 4. lanes 0 .. dim-1: both substitutions of their axis
    if (tid < dim) {
      constexpr int hb = 3;
      const int k = tid;
      for (int j = 0; j < N; ++j) {
        double s = g[dim * j + k];
        for (int d = 1; d <= hb && d <= j; ++d) s -= band[4 * j + d] * g[dim * (j - d) + k];
        g[dim * j + k] = s / band[4 * j];
      }
      for (int j = N - 1; j >= 0; --j) {
        double s = g[dim * j + k];
        for (int d = 1; d <= hb; ++d)
          if (j + d < N) s -= band[4 * (j + d) + d] * g[dim * (j + d) + k];
        g[dim * j + k] = s / band[4 * j];
      }
    }
    __syncthreads();
    // 5. the objective at the minimiser
    qs_cost(Q, b, g, N, dt, pt_dist, nw, tid, band, &sh[2]);
    if (!isfinite(sh[2])) degenerate = true;
  }

  // DEGENERATE: the input as it came, cost 0
  if (degenerate) {
    for (int e = tid; e < maxn * dim; e += QS_NT) out[e] = e < dim * N ? qin[e] : 0.0;
    if (tid == 0) Q.status[b] = FUELMI_QUAD_DEGENERATE, Q.cost[b] = 0.0, Q.pt_dist[b] = pt_dist;
    return;
  }

  // 6. the unconstrained minimiser is the constrained one only inside the bounds of :206-214, which refer to q0
  bool outside = false;
  if (Q.bounds && dim == 3)
    for (int e = tid; e < 3 * N; e += QS_NT) {
      const int k = e % 3;
      const double q0 = qs_clamp(Q, qin[e], k);
      const double lb = fmax(q0 - 10.0, Q.box_lo[k]), ub = fmin(q0 + 10.0, Q.box_hi[k]);
      if (!(lb <= g[e] && g[e] <= ub)) outside = true;
    }
  if (__ballot(outside) != 0) {
    for (int e = tid; e < 3 * N; e += QS_NT) g[e] = qs_clamp(Q, qin[e], e % 3);
    __syncthreads();
    qs_cost(Q, b, g, N, dt, pt_dist, nw, tid, band, &sh[2]);
    for (int e = tid; e < maxn * dim; e += QS_NT) out[e] = e < dim * N ? g[e] : 0.0;
    if (tid == 0) Q.status[b] = FUELMI_QUAD_BOUNDED, Q.cost[b] = sh[2], Q.pt_dist[b] = pt_dist;
    return;
  }

  // 7. FUELMI_QUAD_OK
  for (int e = tid; e < maxn * dim; e += QS_NT) out[e] = e < dim * N ? g[e] : 0.0;
  if (tid == 0) Q.status[b] = FUELMI_QUAD_OK, Q.cost[b] = sh[2], Q.pt_dist[b] = pt_dist;
  if (Q.x_next) {
    double* xn = Q.x_next + (size_t)b * Q.x_next_stride;
    for (int e = tid; e < dim * N; e += QS_NT) xn[e] = g[e];
  }
  if (Q.pt_dist_next) {
    qs_pt_dist(g, N, dim, tid, band, &sh[3]);
    if (tid == 0) Q.pt_dist_next[b] = sh[3];
  }
}

// The LDS of one problem: (4 + 1 + 3 dim) max_ctrl + 16 doubles -- 14 max_ctrl + 16 at dim 3.  The 160 KiB budget holds
// (163840 / 8 - 16) / 14 = 1462 control points; the cap is the power of two below, the yaw entry's 1024 (112 KiB + 128 B).
size_t qs_lds(int max_ctrl, int dim) { return qs_lds_doubles(max_ctrl, dim) * sizeof(double); }

bool fin_lt(double x, double lim) { return std::isfinite(x) && std::fabs(x) < lim; }

int quad_order(const fuelmi_bspline_cfg* w, int dim) { return dim == 1 ? 3 : w->bspline_degree; }  // optimize() :123-127

// what decides the launch: the config alone
int quad_shape_check(const fuelmi_quad_cfg* cfg) {
  ARGCHK(cfg);
  ARGCHK(cfg->cost_function != 0 && (cfg->cost_function & ~QS_MASK) == 0);
  ARGCHK(cfg->dim == 1 || cfg->dim == 3);
  ARGCHK(cfg->end_n >= 1 && cfg->end_n <= 3);
  ARGCHK(cfg->max_waypt >= 0);
  ARGCHK(cfg->max_ctrl >= 4);
  if (cfg->max_ctrl > FUELMI_QUAD_MAX_CTRL) {
    fuelmi_set_error("quadratic solve: max_ctrl = %d exceeds %d", cfg->max_ctrl, FUELMI_QUAD_MAX_CTRL);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

int quad_cfg_check(const fuelmi_bspline_cfg* w, const fuelmi_quad_cfg* cfg) {
  ARGCHK(w);
  {
    const int rc = quad_shape_check(cfg);
    if (rc) return rc;
  }
  ARGCHK(cfg->dim == 1 || (w->bspline_degree >= 3 && w->bspline_degree <= 5));
  ARGCHK(cfg->max_ctrl >= quad_order(w, cfg->dim) + 1);
  const int m = cfg->cost_function;
  ARGCHK(!(m & FUELMI_COST_SMOOTHNESS) || (std::isfinite(w->ld_smooth) && w->ld_smooth >= 0.0));
  ARGCHK(!(m & FUELMI_COST_START) || (std::isfinite(w->ld_start) && w->ld_start >= 0.0));
  ARGCHK(!(m & FUELMI_COST_END) || (std::isfinite(w->ld_end) && w->ld_end >= 0.0));
  ARGCHK(!(m & FUELMI_COST_GUIDE) || (std::isfinite(w->ld_guide) && w->ld_guide >= 0.0));
  ARGCHK(!(m & FUELMI_COST_WAYPOINTS) || (std::isfinite(w->ld_waypt) && w->ld_waypt >= 0.0));
  return FUELMI_OK;
}

int quad_max_guide(const fuelmi_bspline_cfg* w, const fuelmi_quad_cfg* cfg) {
  const int n = cfg->max_ctrl - 2 * quad_order(w, cfg->dim);
  return n > 0 ? n : 0;
}

// the caller's host arrays (the inputs null for a device batch: the host does not see what the batch holds)
struct QuadIO {
  const int* n_ctrl;
  const double *ctrl, *knot_span, *start_state, *end_state, *guide_pts;
  const int* n_waypt;
  const double* waypoints;
  const int* waypt_idx;
  int* status;
  double *ctrl_out, *cost, *pt_dist;
};

int quad_check(const fuelmi_bspline_cfg* w, const fuelmi_quad_cfg* cfg, int n_prob, const QuadIO& io) {
  {
    const int rc = quad_cfg_check(w, cfg);
    if (rc) return rc;
  }
  ARGCHK(n_prob >= 0);
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(io.status && io.ctrl_out && io.cost && io.pt_dist);
  if (!io.n_ctrl) return FUELMI_OK;  // (a device batch: its variables are checked by the kernel)
  const int m = cfg->cost_function, dim = cfg->dim, order = quad_order(w, dim), maxg = quad_max_guide(w, cfg);
  ARGCHK(io.ctrl && io.knot_span);
  ARGCHK(!(m & FUELMI_COST_START) || io.start_state);
  ARGCHK(!(m & FUELMI_COST_END) || io.end_state);
  ARGCHK(!(m & FUELMI_COST_GUIDE) || maxg == 0 || io.guide_pts);
  const bool wp = (m & FUELMI_COST_WAYPOINTS) && cfg->max_waypt > 0;
  ARGCHK(!wp || (io.n_waypt && io.waypoints && io.waypt_idx));
  for (int b = 0; b < n_prob; ++b) {
    const int N = io.n_ctrl[b];
    ARGCHK(N >= 4 && N >= order + 1 && N <= cfg->max_ctrl);
    ARGCHK(std::isfinite(io.knot_span[b]) && io.knot_span[b] > 0.0);
    const double* P = io.ctrl + (size_t)b * cfg->max_ctrl * dim;
    for (int k = 0; k < dim * N; ++k) ARGCHK(fin_lt(P[k], 1e7));
    if (m & FUELMI_COST_START)
      for (int k = 0; k < 3 * dim; ++k) ARGCHK(fin_lt(io.start_state[(size_t)b * 3 * dim + k], 1e7));
    if (m & FUELMI_COST_END)
      for (int k = 0; k < cfg->end_n * dim; ++k) ARGCHK(fin_lt(io.end_state[(size_t)b * 3 * dim + k], 1e7));
    if (m & FUELMI_COST_GUIDE)
      for (int k = 0; k < (N - 2 * order) * dim; ++k) ARGCHK(fin_lt(io.guide_pts[(size_t)b * maxg * dim + k], 1e7));
    if (wp) {
      const int nw = io.n_waypt[b];
      ARGCHK(nw >= 0 && nw <= cfg->max_waypt);
      for (int j = 0; j < nw; ++j) {
        const int i = io.waypt_idx[(size_t)b * cfg->max_waypt + j];
        ARGCHK(i >= 0 && i <= N - 3);
        for (int k = 0; k < dim; ++k) ARGCHK(fin_lt(io.waypoints[((size_t)b * cfg->max_waypt + j) * dim + k], 1e7));
      }
    }
  }
  return FUELMI_OK;
}

// Q cleared, then its part that comes from the two configs and the map
void quad_args(const fuelmi_map* m, const fuelmi_bspline_cfg* w, const fuelmi_quad_cfg* cfg, int n_prob, QuadArgs& Q) {
  memset(&Q, 0, sizeof(Q));
  Q.mask = cfg->cost_function, Q.dim = cfg->dim, Q.max_ctrl = cfg->max_ctrl, Q.end_n = cfg->end_n;
  Q.max_waypt = cfg->max_waypt, Q.bounds = cfg->bounds != 0, Q.order = quad_order(w, cfg->dim), Q.n_prob = n_prob;
  Q.ld_smooth = w->ld_smooth, Q.ld_start = w->ld_start, Q.ld_end = w->ld_end, Q.ld_guide = w->ld_guide;
  Q.ld_waypt = w->ld_waypt;
  for (int k = 0; k < 3; ++k) {  // getBox(bmin, bmax); bmin += 0.1; bmax -= 0.1  (:174-180)
    Q.box_lo[k] = m->cfg.box_min[k] + 0.1;
    Q.box_hi[k] = m->cfg.box_max[k] - 0.1;
  }
}

void quad_results(ResultBlock& R, QuadArgs& Q, const QuadIO& io) {
  const size_t n = (size_t)Q.n_prob;
  R.add(Q.status, io.status, n);
  R.add(Q.cost, io.cost, n);
  R.add(Q.pt_dist, io.pt_dist, n);
  R.add(Q.ctrl_out, io.ctrl_out, n * Q.max_ctrl * Q.dim);
}

int quad_launch(hipStream_t st, const QuadArgs& Q) {
  const size_t lds = qs_lds(Q.max_ctrl, Q.dim);
  if (lds > 64 * 1024)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_quad_solve), hipFuncAttributeMaxDynamicSharedMemorySize,
                               160 * 1024));
  hipLaunchKernelGGL(k_quad_solve, dim3(Q.n_prob), dim3(QS_NT), lds, st, Q);
  HIPCHK(hipGetLastError());
  return FUELMI_OK;
}

}  // namespace

extern "C" int fuelmi_quad_plan(const fuelmi_quad_cfg* cfg, int out3[3]) {
  ARGCHK(out3);
  {
    const int rc = quad_shape_check(cfg);
    if (rc) return rc;
  }
  out3[0] = QS_NT, out3[1] = (int)qs_lds(cfg->max_ctrl, cfg->dim), out3[2] = FUELMI_QUAD_MAX_CTRL;
  return FUELMI_OK;
}

// the host route: staged in a query slot's pinned block, launched on the slot's stream, copied out of the pinned block
extern "C" int fuelmi_map_solve_quadratic(fuelmi_map* m, const fuelmi_bspline_cfg* w, const fuelmi_quad_cfg* cfg, int n_prob,
                                          const int* n_ctrl, const double* ctrl, const double* knot_span,
                                          const double* start_state, const double* end_state, const double* guide_pts,
                                          const int* n_waypt, const double* waypoints, const int* waypt_idx, int* status,
                                          double* ctrl_out, double* cost, double* pt_dist) {
  const QuadIO io = {n_ctrl, ctrl,      knot_span, start_state, end_state, guide_pts, n_waypt,
                     waypoints, waypt_idx, status,    ctrl_out,    cost,      pt_dist};
  {  // every argument on the host, before the map is touched
    ARGCHK(n_prob <= 0 || n_ctrl);
    const int rc = quad_check(w, cfg, n_prob, io);
    if (rc) return rc;
  }
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  const size_t n = (size_t)n_prob, dim = (size_t)cfg->dim, maxc = (size_t)cfg->max_ctrl;
  const size_t maxg = (size_t)quad_max_guide(w, cfg), maxw = (size_t)cfg->max_waypt;
  QuadArgs Q;
  quad_args(m, w, cfg, n_prob, Q);
  ResultBlock R(16);
  quad_results(R, Q, io);
  ARGCHK(!R.overflow);
  int *p_nc, *p_nw, *p_idx;
  double *p_knot, *p_ctrl, *p_start, *p_end, *p_guide, *p_way;
  auto layout = [&](unsigned char* base) {  // the slot's pinned block: the inputs, then the results
    BlockLayout L(base, 16);
    p_nc = L.take<int>(n);
    p_nw = L.take<int>(n);
    p_idx = L.take<int>(n * maxw);
    p_knot = L.take<double>(n);
    p_ctrl = L.take<double>(n * maxc * dim);
    p_start = L.take<double>(n * 3 * dim);
    p_end = L.take<double>(n * 3 * dim);
    p_guide = L.take<double>(n * maxg * dim);
    p_way = L.take<double>(n * maxw * dim);
    R.place(L);
    return L.size();
  };
  QuerySlotGuard q;
  {
    const int rcq = q.acquire(m, layout(nullptr));
    if (rcq) return rcq;
  }
  layout(q.s->pin);
  auto put = [](void* dst, const void* src, size_t bytes) {  // an input the mask does not read may be null
    if (src)
      memcpy(dst, src, bytes);
    else
      memset(dst, 0, bytes);
  };
  const int mask = cfg->cost_function;
  memcpy(p_nc, n_ctrl, n * sizeof(int));
  memcpy(p_knot, knot_span, n * sizeof(double));
  memcpy(p_ctrl, ctrl, n * maxc * dim * sizeof(double));
  put(p_start, (mask & FUELMI_COST_START) ? start_state : nullptr, n * 3 * dim * sizeof(double));
  put(p_end, (mask & FUELMI_COST_END) ? end_state : nullptr, n * 3 * dim * sizeof(double));
  put(p_guide, (mask & FUELMI_COST_GUIDE) ? guide_pts : nullptr, n * maxg * dim * sizeof(double));
  const bool wp = (mask & FUELMI_COST_WAYPOINTS) && maxw > 0;
  put(p_nw, wp ? n_waypt : nullptr, n * sizeof(int));
  put(p_idx, wp ? waypt_idx : nullptr, n * maxw * sizeof(int));
  put(p_way, wp ? waypoints : nullptr, n * maxw * dim * sizeof(double));
  Q.n_ctrl = p_nc, Q.ctrl = p_ctrl, Q.ctrl_stride = maxc * dim, Q.knot_span = p_knot, Q.vs = (int)dim;
  Q.start_state = p_start, Q.end_state = p_end, Q.guide = p_guide, Q.guide_stride = maxg * dim;
  Q.n_waypt = p_nw, Q.waypts = p_way, Q.waypt_idx = p_idx;
  {
    const int rc = quad_launch(q.s->st, Q);
    if (rc) return rc;
  }
  HIPCHK(q.finish());
  R.scatter(R.base);
  return FUELMI_OK;
}

// the batch route: the variables, knot spans, states, guide points and way-points the batch holds on the device; staged in
// quad_dev on the map's stream, downloaded.  The solution of every FUELMI_QUAD_OK candidate becomes the batch's variables
// and its pt_dist_ the batch's, as optimize() sets both up for the phase that follows (:116, :136-140)
extern "C" int fuelmi_bspline_dev_solve_quadratic(fuelmi_bspline_dev* b, const fuelmi_quad_cfg* cfg, const double* guide_pts,
                                                  int* status, double* ctrl_out, double* cost, double* pt_dist) {
  ARGCHK(b && cfg);
  const BsplineArgs& A = b->a;
  fuelmi_map* m = b->map;
  ARGCHK(m);
  ARGCHK(!(A.cost_function & FUELMI_COST_MINTIME) && A.knot_span);
  fuelmi_quad_cfg qc = *cfg;  // (what describes the arrays is the batch's)
  qc.dim = A.dim, qc.max_ctrl = A.N, qc.max_waypt = A.n_waypt;
  if (qc.cost_function & FUELMI_COST_END) qc.end_n = A.end_n;
  const QuadIO io = {nullptr, nullptr, nullptr, nullptr, nullptr, guide_pts, nullptr, nullptr, nullptr, status, ctrl_out, cost, pt_dist};
  {
    const int rc = quad_check(&A.cfg, &qc, A.C, io);
    if (rc) return rc;
  }
  const int mask = qc.cost_function;
  const size_t C = (size_t)A.C, ng = A.n_guide > 0 ? (size_t)A.n_guide : 0;
  ARGCHK(!(mask & FUELMI_COST_START) || A.start_state);
  ARGCHK(!(mask & FUELMI_COST_END) || A.end_state);
  ARGCHK(!(mask & FUELMI_COST_GUIDE) || ng == 0 || guide_pts || A.guide_pts);
  ARGCHK(!(mask & FUELMI_COST_WAYPOINTS) || A.n_waypt == 0 || (A.waypoints && A.waypt_idx));
  if (guide_pts && (mask & FUELMI_COST_GUIDE))
    for (size_t k = 0; k < C * ng * 3; ++k) ARGCHK(fin_lt(guide_pts[k], 1e7));
  HIPCHK(hipSetDevice(m->device));
  QuadArgs Q;
  quad_args(m, &A.cfg, &qc, A.C, Q);
  ResultBlock R(16);
  quad_results(R, Q, io);
  ARGCHK(!R.overflow);
  const bool up_guide = guide_pts && (mask & FUELMI_COST_GUIDE) && ng > 0;
  double* d_guide;
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 16);
    d_guide = L.take<double>(up_guide ? C * ng * 3 : 0);
    R.place(L);
    return L.size();
  };
  hipStream_t st = m->stream;
  {
    const int rc = b->quad_dev.carve(st, layout);
    if (rc) return rc;
  }
  if (up_guide) HIPCHK(hipMemcpyAsync(d_guide, guide_pts, C * ng * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  Q.n_ctrl = nullptr, Q.n_ctrl_all = A.N, Q.ctrl = A.x, Q.ctrl_stride = (size_t)A.nvar, Q.knot_span = A.knot_span, Q.vs = 3;
  Q.start_state = A.start_state, Q.end_state = A.end_state;
  Q.guide = up_guide ? d_guide : A.guide_pts, Q.guide_stride = ng * 3;
  Q.n_waypt = nullptr, Q.n_waypt_all = A.n_waypt, Q.waypts = A.waypoints, Q.waypt_idx = A.waypt_idx;
  Q.x_next = const_cast<double*>(A.x), Q.x_next_stride = (size_t)A.nvar, Q.pt_dist_next = const_cast<double*>(A.pt_dist);
  opt_set_valid(b, false);  // opt_x no longer is the solve of what the batch holds
  {
    StageScope sc(m, FUELMI_K_BSPLINE);
    const int rc = quad_launch(st, Q);
    if (rc) return rc;
  }
  return result_fetch(R, st);
}
