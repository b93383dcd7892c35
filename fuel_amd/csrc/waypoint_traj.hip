// waypoint_traj.hip -- the min-jerk initial trajectory through way-points: the first half of
// FastPlannerManager::planExploreTraj (plan_manage/src/planner_manager.cpp:266-297) for a batch of problems
// (way-points, start velocity, start acceleration): segment times, PolynomialTraj::waypointsTraj
// (poly_traj/src/polynomial_traj.cpp:5-175) with end velocity = end acceleration = 0, getTotalTime, getLength,
// seg_num, the sample loop and the four boundary derivatives.
//
// waypointsTraj minimises d'^T R d' over the free boundary derivatives, R = C A^-T Q A^-1 C^T with 6S x 6S matrices.
// A and Q are block diagonal (one 6 x 6 block per segment), C^T only selects, and A_k^-1 is known in closed form, so
// M_k = A_k^-T Q_k A_k^-1 is an integer matrix scaled by powers of 1 / T_k (d_k = {p0, p1, v0, v1, a0, a1}):
//     T^5 M = [  720 -720  360T  360T   60T^2  -60T^2 ]      rows / columns 2, 4: velocity / acceleration at the
//             [ -720  720 -360T -360T  -60T^2   60T^2 ]      segment's start, 3, 5: at its end
//             [  360 -360  192T^2 168T^2 36T^3 -24T^3 ]
//             [  360 -360  168T^2 192T^2 24T^3 -36T^3 ]
//             [   60  -60   36T^3  24T^3  9T^4  -3T^4 ]
//             [  -60   60  -24T^3 -36T^3 -3T^4   9T^4 ]
// The free unknowns are the velocity and acceleration of the interior way-points w = 1 .. S-1 (unknowns 2 (w-1) and
// 2 (w-1) + 1, the reference's order).  Way-point w ends segment w-1 and starts segment w, so Rpp is symmetric of
// order 2S - 2 with half-bandwidth 3, and -Rfp^T d_f needs the two segments' way-points (and, next to the start, the
// start velocity / acceleration; the end ones are 0).  One lane per way-point gathers its two rows, lane 0 runs a
// banded Cholesky, lanes 0..2 substitute the three axes, one lane per segment writes p_k = A_k^-1 d_k.  Nothing of
// order S^2 is stored.
//
// The two sampling loops accumulate their time (eval_t += 0.01; ts += dt), and the number of samples is a result of
// that accumulation.  Every lane repeats the additions of a chunk of WT_NT samples and keeps the value of its own
// sample; the evaluations then run side by side.  getLength's norms are summed by a fixed tree per chunk, chunks left to
// right: the result does not depend on the batch.
//
// One workgroup of WT_NT lanes per problem, all f64, -ffp-contract=off.  LDS: times, band, right-hand sides,
// coefficients, one chunk of points, the reduction (fuelmi_wptraj_plan reports the bytes).
// Behind the kernel, the two entries that share its checks and launch: fuelmi_map_waypoint_trajs (through a query slot)
// and fuelmi_bspline_dev_load_waypoints (samples straight into a device batch's fit, bspline_batch.h).
#include <cmath>
#include <cstring>
#include <vector>

#include "bspline_batch.h"
#include "poly_internal.h"

namespace {

constexpr int WT_NT = 256;
constexpr int WT_LEN_CAP = 1 << 21;  // length samples: the host admits duration <= FUELMI_WPTRAJ_MAX_DURATION only

// k_waypoint_traj: one problem per workgroup; every pointer addresses memory the device can reach
struct WpTrajArgs {
  int n_prob;
  const int* n_way;    // [n]
  const double* way;   // [n][maxw][3]
  const double* vel;   // [n][3]
  const double* acc;   // [n][3]
  int maxw;
  double max_vel, ctrl_pt_dist;
  int min_seg, forced_seg, max_samples;
  int* status;
  double* duration;
  double* length;
  int* seg_num;
  double* dt;
  int* n_samples;
  double* samples;     // [n][max_samples][3]
  double* derivs;      // [n][4][3]
  double* seg_times;   // [n][maxw-1] or null
  double* coef;        // [n][maxw-1][3][6] or null
};

// a problem without a trajectory: every output of it is 0
__device__ void wt_zero(const WpTrajArgs& W, int b, int status, int tid) {
  if (tid == 0) {
    W.status[b] = status;
    W.duration[b] = 0.0;
    W.length[b] = 0.0;
    W.seg_num[b] = 0;
    W.dt[b] = 0.0;
    W.n_samples[b] = 0;
  }
  if (tid < 12) W.derivs[(size_t)b * 12 + tid] = 0.0;
  double* smp = W.samples + (size_t)b * W.max_samples * 3;
  for (int i = tid; i < 3 * W.max_samples; i += WT_NT) smp[i] = 0.0;
  const int rows = W.maxw - 1;
  if (W.seg_times)
    for (int i = tid; i < rows; i += WT_NT) W.seg_times[(size_t)b * rows + i] = 0.0;
  if (W.coef)
    for (int i = tid; i < 18 * rows; i += WT_NT) W.coef[(size_t)b * rows * 18 + i] = 0.0;
}

__global__ void __launch_bounds__(WT_NT) k_waypoint_traj(WpTrajArgs W) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int Smax = W.maxw > 2 ? W.maxw - 1 : 1, nn = 2 * Smax;
  double* T = reinterpret_cast<double*>(smem_raw);  // [Smax]
  double* band = T + Smax;                          // [nn][4]  Rpp(r, r - d) at [r][d]
  double* g = band + 4 * nn;                        // [nn][3]
  double* cf = g + 3 * nn;                          // [Smax][3][6]
  double* pbuf = cf + 18 * Smax;                    // [WT_NT + 1][3]: [0] the last point of the chunk before
  double* red = pbuf + 3 * (WT_NT + 1);             // [WT_NT]
  double* sh = red + WT_NT;                         // [2] duration, degenerate
  const int n = W.n_way[b], S = n - 1;
  if (n < 3) {
    wt_zero(W, b, FUELMI_WPTRAJ_FEW, tid);
    return;
  }
  const double* P = W.way + (size_t)b * W.maxw * 3;
  const double v0[3] = {W.vel[3 * b], W.vel[3 * b + 1], W.vel[3 * b + 2]};
  const double a0[3] = {W.acc[3 * b], W.acc[3 * b + 1], W.acc[3 * b + 2]};

  // 1. segment times (:276-278), getTotalTime
  for (int k = tid; k < S; k += WT_NT) {
    const double x = P[3 * k + 3] - P[3 * k], y = P[3 * k + 4] - P[3 * k + 1], z = P[3 * k + 5] - P[3 * k + 2];
    T[k] = sqrt(x * x + y * y + z * z) / (W.max_vel * 0.5);
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    bool bad = false;
    for (int k = 0; k < S; ++k) {
      s += T[k];
      bad = bad || T[k] == 0.0 || !isfinite(T[k]);
    }
    sh[0] = s;
    sh[1] = bad ? 1.0 : 0.0;
  }
  __syncthreads();
  const double dur = sh[0];
  if (sh[1] != 0.0) {
    wt_zero(W, b, FUELMI_WPTRAJ_DEGENERATE, tid);
    return;
  }

  // 2. Rpp and -Rfp^T d_f, two rows per interior way-point
  for (int w = tid + 1; w < S; w += WT_NT) {
    const double a1 = 1.0 / T[w - 1], a2 = a1 * a1, a3 = a2 * a1, a4 = a3 * a1;
    const double b1 = 1.0 / T[w], b2 = b1 * b1, b3 = b2 * b1, b4 = b3 * b1;
    const int r0 = 2 * (w - 1), r1 = r0 + 1;
    const bool first = w == 1;
    band[4 * r0 + 0] = 192.0 * a3 + 192.0 * b3;
    band[4 * r0 + 1] = first ? 0.0 : 24.0 * a2;   // v_w with a_{w-1}
    band[4 * r0 + 2] = first ? 0.0 : 168.0 * a3;  // v_w with v_{w-1}
    band[4 * r0 + 3] = 0.0;
    band[4 * r1 + 0] = 9.0 * a1 + 9.0 * b1;
    band[4 * r1 + 1] = -36.0 * a2 + 36.0 * b2;    // a_w with v_w
    band[4 * r1 + 2] = first ? 0.0 : -3.0 * a1;   // a_w with a_{w-1}
    band[4 * r1 + 3] = first ? 0.0 : -24.0 * a2;  // a_w with v_{w-1}
    for (int ax = 0; ax < 3; ++ax) {
      const double da = P[3 * (w - 1) + ax] - P[3 * w + ax], db = P[3 * w + ax] - P[3 * (w + 1) + ax];
      double sv = 360.0 * a4 * da + 360.0 * b4 * db;
      double sa = -60.0 * a3 * da + 60.0 * b3 * db;
      if (first) {
        sv = sv + (168.0 * a3 * v0[ax] + 24.0 * a2 * a0[ax]);
        sa = sa + (-24.0 * a2 * v0[ax] - 3.0 * a1 * a0[ax]);
      }
      g[3 * r0 + ax] = -sv;
      g[3 * r1 + ax] = -sa;
    }
  }
  __syncthreads();

  // 3. banded Cholesky (the loops of k_bspline_fit at half-bandwidth 3), the three axes on lanes 0..2
  const int n2 = 2 * S - 2;
  constexpr int hb = 3;
  if (tid == 0) {
    for (int j = 0; j < n2; ++j) {
      double s = band[4 * j];
      for (int d = 1; d <= hb && d <= j; ++d) s -= band[4 * j + d] * band[4 * j + d];
      const double ljj = sqrt(s);
      band[4 * j] = ljj;
      for (int i = j + 1; i <= j + hb && i < n2; ++i) {
        double t = band[4 * i + (i - j)];
        for (int k = max(0, i - hb); k < j; ++k) t -= band[4 * i + (i - k)] * band[4 * j + (j - k)];
        band[4 * i + (i - j)] = t / ljj;
      }
    }
  }
  __syncthreads();
  if (tid < 3) {
    for (int j = 0; j < n2; ++j) {
      double s = g[3 * j + tid];
      for (int d = 1; d <= hb && d <= j; ++d) s -= band[4 * j + d] * g[3 * (j - d) + tid];
      g[3 * j + tid] = s / band[4 * j];
    }
    for (int j = n2 - 1; j >= 0; --j) {
      double s = g[3 * j + tid];
      for (int d = 1; d <= hb; ++d)
        if (j + d < n2) s -= band[4 * (j + d) + d] * g[3 * (j + d) + tid];
      g[3 * j + tid] = s / band[4 * j];
    }
  }
  __syncthreads();

  // 4. p_k = A_k^-1 d_k, one segment per lane
  const int rows = W.maxw - 1;
  for (int k = tid; k < S; k += WT_NT) {
    const double Tk = T[k];
    const double i1 = 1.0 / Tk, i2 = i1 * i1, i3 = i2 * i1, i4 = i3 * i1, i5 = i4 * i1;
    for (int ax = 0; ax < 3; ++ax) {
      const double p0 = P[3 * k + ax], p1 = P[3 * k + 3 + ax];
      const double vs = k == 0 ? v0[ax] : g[3 * (2 * (k - 1)) + ax];
      const double as = k == 0 ? a0[ax] : g[3 * (2 * (k - 1) + 1) + ax];
      const double ve = k == S - 1 ? 0.0 : g[3 * (2 * k) + ax];
      const double ae = k == S - 1 ? 0.0 : g[3 * (2 * k + 1) + ax];
      const double d = p1 - p0;
      double* c = cf + 18 * k + 6 * ax;
      c[0] = p0;
      c[1] = vs;
      c[2] = 0.5 * as;
      c[3] = (10.0 * d) * i3 + (-6.0 * vs - 4.0 * ve) * i2 + (-1.5 * as + 0.5 * ae) * i1;
      c[4] = (-15.0 * d) * i4 + (8.0 * vs + 7.0 * ve) * i3 + (1.5 * as - ae) * i2;
      c[5] = (6.0 * d) * i5 + (-3.0 * vs - 3.0 * ve) * i4 + (-0.5 * as + 0.5 * ae) * i3;
      if (W.coef)
        for (int i = 0; i < 6; ++i) W.coef[((size_t)b * rows + k) * 18 + 6 * ax + i] = c[i];
    }
    if (W.seg_times) W.seg_times[(size_t)b * rows + k] = Tk;
  }
  __syncthreads();

  // 5. getLength: samples at the accumulated eval_t while eval_t < duration, norms of consecutive samples
  double len = 0.0;
  {
    double t = 0.0;
    int base = 0;
    for (;;) {
      double mine = 0.0;
      int cnt = 0;
      for (int j = 0; j < WT_NT; ++j) {
        if (!(t < dur)) break;
        if (j == tid) mine = t;
        t += 0.01;
        ++cnt;
      }
      if (cnt == 0) break;
      const bool have = tid < cnt;
      double p[3] = {0.0, 0.0, 0.0};
      if (have) {
        poly_eval(cf, T, S, mine, 0, p);
        for (int a = 0; a < 3; ++a) pbuf[3 * (tid + 1) + a] = p[a];
      }
      __syncthreads();
      double v = 0.0;
      if (have && base + tid >= 1) {
        const double x = p[0] - pbuf[3 * tid], y = p[1] - pbuf[3 * tid + 1], z = p[2] - pbuf[3 * tid + 2];
        v = sqrt(x * x + y * y + z * z);
      }
      red[tid] = v;
      __syncthreads();
      for (int s = WT_NT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
      }
      len += red[0];
      __syncthreads();
      if (tid < 3) pbuf[tid] = pbuf[3 * cnt + tid];
      __syncthreads();
      base += cnt;
      if (cnt < WT_NT || base >= WT_LEN_CAP) break;
    }
  }

  // 6. seg_num, dt (:285-288)
  int sn = W.forced_seg;
  if (sn <= 0) {
    double q = len / W.ctrl_pt_dist;
    if (!(q < (double)FUELMI_WPTRAJ_MAX_SEG)) q = (double)FUELMI_WPTRAJ_MAX_SEG;
    sn = max(W.min_seg, (int)q);
  }
  const double dt = dur / (double)sn;

  // 7. samples at the accumulated ts while ts <= duration + 1e-4 (:292-293)
  int count = 0;
  {
    const double bound = dur + 1e-4;
    double t = 0.0;
    double* smp = W.samples + (size_t)b * W.max_samples * 3;
    for (;;) {
      double mine = 0.0;
      int cnt = 0;
      for (int j = 0; j < WT_NT; ++j) {
        if (!(t <= bound) || count + cnt >= FUELMI_WPTRAJ_MAX_SEG + 2) break;
        if (j == tid) mine = t;
        t += dt;
        ++cnt;
      }
      if (tid < cnt && count + tid < W.max_samples) {
        double p[3];
        poly_eval(cf, T, S, mine, 0, p);
        for (int a = 0; a < 3; ++a) smp[3 * (count + tid) + a] = p[a];
      }
      count += cnt;
      if (cnt < WT_NT) break;
    }
  }

  // 8. boundary derivatives (:294-297) and the scalars
  if (tid < 4) {
    double p[3];
    poly_eval(cf, T, S, (tid & 1) ? dur : 0.0, tid < 2 ? 1 : 2, p);
    for (int a = 0; a < 3; ++a) W.derivs[(size_t)b * 12 + 3 * tid + a] = p[a];
  }
  if (tid == 0) {
    W.status[b] = count > W.max_samples ? -1 : FUELMI_WPTRAJ_OK;
    W.duration[b] = dur;
    W.length[b] = len;
    W.seg_num[b] = sn;
    W.dt[b] = dt;
    W.n_samples[b] = count;
  }
}

bool pos_fin(double x) { return std::isfinite(x) && x > 0.0; }

size_t wt_lds(int maxw) {
  const size_t Smax = maxw > 2 ? (size_t)maxw - 1 : 1;
  return (Smax + 4 * 2 * Smax + 3 * 2 * Smax + 18 * Smax + 3 * (WT_NT + 1) + WT_NT + 2) * sizeof(double);
}

int wptraj_check(const fuelmi_wptraj_cfg* cfg, int n_prob, const int* n_way, const double* way_xyz,
                 const double* vel_xyz, const double* acc_xyz) {
  ARGCHK(cfg);
  ARGCHK(pos_fin(cfg->max_vel) && pos_fin(cfg->ctrl_pt_dist));
  ARGCHK(cfg->min_seg >= 1 && cfg->min_seg <= FUELMI_WPTRAJ_MAX_SEG);
  ARGCHK(cfg->seg_num >= 0 && cfg->seg_num <= FUELMI_WPTRAJ_MAX_SEG);
  ARGCHK(cfg->max_way_points >= 1 && cfg->max_samples >= 1);
  if (cfg->max_way_points > FUELMI_WPTRAJ_MAX_WAY) {
    fuelmi_set_error("waypoint trajectories: max_way_points = %d exceeds %d", cfg->max_way_points, FUELMI_WPTRAJ_MAX_WAY);
    return FUELMI_ELIMIT;
  }
  ARGCHK(n_prob >= 0);
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(n_way && way_xyz && vel_xyz && acc_xyz);
  const int maxw = cfg->max_way_points;
  for (int b = 0; b < n_prob; ++b) {
    ARGCHK(n_way[b] >= 0 && n_way[b] <= maxw);
    const double* P = way_xyz + (size_t)b * maxw * 3;
    for (int k = 0; k < 3 * n_way[b]; ++k) ARGCHK(std::fabs(P[k]) < 1e7);
    for (int k = 0; k < 3; ++k) ARGCHK(std::fabs(vel_xyz[3 * b + k]) < 1e7 && std::fabs(acc_xyz[3 * b + k]) < 1e7);
    double dur = 0.0;  // the kernel's own sum: its sampling loops are as long as this allows
    for (int k = 0; k + 1 < n_way[b]; ++k) {
      const double x = P[3 * k + 3] - P[3 * k], y = P[3 * k + 4] - P[3 * k + 1], z = P[3 * k + 5] - P[3 * k + 2];
      dur += sqrt(x * x + y * y + z * z) / (cfg->max_vel * 0.5);
    }
    if (std::isfinite(dur) && dur > FUELMI_WPTRAJ_MAX_DURATION) {
      fuelmi_set_error("waypoint trajectories: problem %d lasts %g s, more than %g s", b, dur, FUELMI_WPTRAJ_MAX_DURATION);
      return FUELMI_ELIMIT;
    }
  }
  return FUELMI_OK;
}

int wptraj_launch(hipStream_t st, const WpTrajArgs& W) {
  const size_t lds = wt_lds(W.maxw);
  if (lds > 64 * 1024)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_waypoint_traj), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
  hipLaunchKernelGGL(k_waypoint_traj, dim3(W.n_prob), dim3(WT_NT), lds, st, W);
  HIPCHK(hipGetLastError());
  return FUELMI_OK;
}

}  // namespace

extern "C" int fuelmi_wptraj_plan(const fuelmi_wptraj_cfg* cfg, int out3[3]) {
  ARGCHK(cfg && out3);
  ARGCHK(cfg->max_way_points >= 1);
  if (cfg->max_way_points > FUELMI_WPTRAJ_MAX_WAY) {
    fuelmi_set_error("waypoint trajectories: max_way_points = %d exceeds %d", cfg->max_way_points, FUELMI_WPTRAJ_MAX_WAY);
    return FUELMI_ELIMIT;
  }
  out3[0] = WT_NT, out3[1] = (int)wt_lds(cfg->max_way_points), out3[2] = FUELMI_WPTRAJ_MAX_WAY;
  return FUELMI_OK;
}

extern "C" int fuelmi_map_waypoint_trajs(fuelmi_map* m, const fuelmi_wptraj_cfg* cfg, int n_prob, const int* n_way,
                                         const double* way_xyz, const double* vel_xyz, const double* acc_xyz,
                                         int* status, double* duration, double* length, int* seg_num, double* dt,
                                         int* n_samples, double* samples, double* derivs, double* seg_times,
                                         double* coef) {
  {  // every argument on the host, before the map is touched
    const int rc = wptraj_check(cfg, n_prob, n_way, way_xyz, vel_xyz, acc_xyz);
    if (rc) return rc;
  }
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(status && duration && length && seg_num && dt && n_samples && samples && derivs);
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  const size_t n = (size_t)n_prob, maxw = (size_t)cfg->max_way_points, maxs = (size_t)cfg->max_samples;
  const size_t rows = maxw - 1;
  WpTrajArgs W;
  memset(&W, 0, sizeof(W));
  int* p_nway;
  double *p_way, *p_vel, *p_acc;
  auto layout = [&](unsigned char* base) {  // the slot's pinned block: the inputs, then the results
    BlockLayout L(base, 16);
    p_nway = L.take<int>(n);
    p_way = L.take<double>(n * maxw * 3);
    p_vel = L.take<double>(n * 3);
    p_acc = L.take<double>(n * 3);
    W.status = L.take<int>(n);
    W.seg_num = L.take<int>(n);
    W.n_samples = L.take<int>(n);
    W.duration = L.take<double>(n);
    W.length = L.take<double>(n);
    W.dt = L.take<double>(n);
    W.samples = L.take<double>(n * maxs * 3);
    W.derivs = L.take<double>(n * 12);
    W.seg_times = seg_times ? L.take<double>(n * rows) : nullptr;
    W.coef = coef ? L.take<double>(n * rows * 18) : nullptr;
    return L.size();
  };
  QuerySlotGuard q;
  {
    const int rcq = q.acquire(m, layout(nullptr));
    if (rcq) return rcq;
  }
  layout(q.s->pin);
  W.n_prob = n_prob;
  W.maxw = cfg->max_way_points;
  W.max_vel = cfg->max_vel, W.ctrl_pt_dist = cfg->ctrl_pt_dist;
  W.min_seg = cfg->min_seg, W.forced_seg = cfg->seg_num, W.max_samples = cfg->max_samples;
  memcpy(p_nway, n_way, n * sizeof(int));
  memcpy(p_way, way_xyz, n * maxw * 3 * sizeof(double));
  memcpy(p_vel, vel_xyz, n * 3 * sizeof(double));
  memcpy(p_acc, acc_xyz, n * 3 * sizeof(double));
  W.n_way = p_nway, W.way = p_way, W.vel = p_vel, W.acc = p_acc;
  {
    const int rc = wptraj_launch(q.s->st, W);
    if (rc) return rc;
  }
  HIPCHK(q.finish());
  memcpy(status, W.status, n * sizeof(int));
  memcpy(seg_num, W.seg_num, n * sizeof(int));
  memcpy(n_samples, W.n_samples, n * sizeof(int));
  memcpy(duration, W.duration, n * sizeof(double));
  memcpy(length, W.length, n * sizeof(double));
  memcpy(dt, W.dt, n * sizeof(double));
  memcpy(samples, W.samples, n * maxs * 3 * sizeof(double));
  memcpy(derivs, W.derivs, n * 12 * sizeof(double));
  if (seg_times) memcpy(seg_times, W.seg_times, n * rows * sizeof(double));
  if (coef) memcpy(coef, W.coef, n * rows * 18 * sizeof(double));
  for (int b = 0; b < n_prob; ++b)
    if (status[b] == -1) {
      fuelmi_set_error("waypoint trajectories: problem %d has %d samples, more than max_samples = %d", b, n_samples[b],
                       cfg->max_samples);
      return FUELMI_ELIMIT;
    }
  return FUELMI_OK;
}

// the batch route: way-points -> min-jerk samples (k_waypoint_traj, written into the batch's staging) -> the fit
// (k_bspline_fit, bspline.hip), all on the map's stream
extern "C" int fuelmi_bspline_dev_load_waypoints(fuelmi_bspline_dev* b, const fuelmi_wptraj_cfg* cfg, const int* n_way,
                                                 const double* way_xyz, const double* vel_xyz, const double* acc_xyz,
                                                 int* status, double* duration) {
  ARGCHK(b && cfg && status);
  BsplineArgs& A = b->a;
  const int degree = A.cfg.bspline_degree;
  ARGCHK(A.dim == 3 && degree >= 3 && degree <= 5 && A.N - degree >= 1);
  const int seg = A.N - degree, n_points = seg + 1;
  ARGCHK(cfg->seg_num == 0 || cfg->seg_num == seg);
  fuelmi_wptraj_cfg wc = *cfg;
  wc.seg_num = seg, wc.max_samples = n_points;
  {
    const int rc = wptraj_check(&wc, A.C, n_way, way_xyz, vel_xyz, acc_xyz);
    if (rc) return rc;
  }
  fuelmi_map* m = b->map;
  ARGCHK(m);
  opt_set_valid(b, false);
  HIPCHK(hipSetDevice(m->device));
  const size_t C = (size_t)A.C, K = (size_t)n_points, maxw = (size_t)wc.max_way_points;
  WpTrajArgs W;
  memset(&W, 0, sizeof(W));
  double* d_fit;  // ts | points | derivs: the layout fuelmi_bspline_dev_load_samples stages
  int* d_nway;
  double *d_way, *d_vel, *d_acc;
  auto layout = [&](unsigned char* base) {
    BlockLayout L(base, 16);
    d_fit = L.take<double>(C * (1 + K * 3 + 12));
    d_nway = L.take<int>(C);
    d_way = L.take<double>(C * maxw * 3);
    d_vel = L.take<double>(C * 3);
    d_acc = L.take<double>(C * 3);
    W.status = L.take<int>(C);
    W.seg_num = L.take<int>(C);
    W.n_samples = L.take<int>(C);
    W.duration = L.take<double>(C);
    W.length = L.take<double>(C);
    return L.size();
  };
  hipStream_t st = m->stream;
  {
    const int rc = b->fit_in.reserve(st, layout(nullptr));
    if (rc) return rc;
  }
  layout(b->fit_in.base());
  W.n_prob = A.C;
  W.maxw = wc.max_way_points;
  W.max_vel = wc.max_vel, W.ctrl_pt_dist = wc.ctrl_pt_dist;
  W.min_seg = wc.min_seg, W.forced_seg = seg, W.max_samples = n_points;
  HIPCHK(hipMemcpyAsync(d_nway, n_way, C * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_way, way_xyz, C * maxw * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_vel, vel_xyz, C * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_acc, acc_xyz, C * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  W.n_way = d_nway, W.way = d_way, W.vel = d_vel, W.acc = d_acc;
  W.dt = d_fit;  // the fit's knot spans
  W.samples = d_fit + C;
  W.derivs = d_fit + C + C * K * 3;
  const FitArgs F = fit_args(b, W.dt, W.samples, W.derivs, W.status);
  {
    StageScope sc(m, FUELMI_K_BSPLINE);
    const int rcw = wptraj_launch(st, W);
    if (rcw) return rcw;
    const int rcf = fit_launch(m, F);
    if (rcf) return rcf;
  }
  HIPCHK(hipMemcpyAsync(status, W.status, C * sizeof(int), hipMemcpyDeviceToHost, st));
  if (duration) HIPCHK(hipMemcpyAsync(duration, W.duration, C * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(stream_wait(st));
  for (int c = 0; c < A.C; ++c)
    if (status[c] == -1) {
      fuelmi_set_error("waypoint trajectories: candidate %d does not give %d samples", c, n_points);
      return FUELMI_ELIMIT;
    }
  return FUELMI_OK;
}
