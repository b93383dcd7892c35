// traj_sample.hip -- what the reference does with a finished trajectory, for a batch of problems (position spline,
// uniform or on given knots, optional uniform yaw spline, a tape of sample times):
//   FUELMI_TRAJSMP_COMMAND  traj_server's cmdCallback (plan_manage/src/traj_server.cpp:257-343): position, velocity,
//                           acceleration, jerk, yaw and yaw rate at each tick, and the flight record (:328-339)
//   FUELMI_TRAJSMP_STATE    the FSM's replan start state (exploration_manager/src/fast_exploration_fsm.cpp:86-95)
// The derivative splines of getDerivative (non_uniform_bspline.cpp:77-106) are never stored: the clamp and the knot search
// of evaluateDeBoor give every derivative the same span (spline_internal.h), and the p + 1 position points of that span
// give the points each derivative reads there by getDerivativeControlPoints' own operations.
//
// One 64-lane wave per problem, TS_WAVES problems per workgroup.  The knots of both splines are staged in LDS (one block
// per wave): by lane 0's accumulated additions, or the position spline's copied and checked as given; control points are read from global memory through L2 (traj_check.hip
// says why).  The lanes take a window of 64 consecutive sample times, one each.  The flight record is a chain through
// the samples -- each is compared with the last one PUSHED -- so behind every window all lanes walk its 64 samples in
// order by lane reads, each lane making the same additions, and lane 0 stores the record at the end: the sums are the
// reference's, term by term.  All f64, -ffp-contract=off.  A result does not depend on the problem's place in the
// batch: the only workgroup-wide step is the barrier behind the knots.
// Behind the kernel, the entries that share its checks, layout and trajsmp_run: fuelmi_map_sample_trajs and
// fuelmi_map_sample_trajs_knots (splines from the host, the position spline uniform or on given knots) and
// fuelmi_bspline_dev_sample_trajs (the splines a device batch's last solve left, on the knots its adjustment left if the
// batch says so, bspline_batch.h).
#include <cmath>
#include <cstring>
#include <vector>

#include "bspline_batch.h"

namespace {

constexpr int TS_WIN = 64;   // samples per window: one per lane
constexpr int TS_WAVES = 3;  // problems per workgroup: two knot blocks each, 48.4 KiB at the largest strides

// k_traj_sample: one problem per wave; every pointer addresses device memory
struct TrajSmpArgs {
  fuelmi_trajsmp_cfg cfg;
  int n_prob;
  SplineSrc src;
  const int* n_yaw;         // [n] (0: that problem has no yaw spline), or null: none has
  const double* yaw;        // [n][max_yaw_ctrl]
  const double* yaw_dt;     // [n]
  const double* t_stop;     // [n] or null
  const int* n_t;           // [n]
  const double* t;          // [n][max_t]
  double* flight;           // [n][8] in and out, or null
  int* status;              // [n][max_t]
  double *o_pos, *o_vel, *o_acc, *o_jerk;  // [n][max_t][3]
  double *o_yaw, *o_yawdot, *o_yawddot;    // [n][max_t]
  double* duration;         // [n]
};

__host__ __device__ inline int ts_wave_stride(const fuelmi_trajsmp_cfg& c) {
  return spline_knot_stride(c.max_ctrl) + (c.max_yaw_ctrl > 0 ? spline_knot_stride(c.max_yaw_ctrl) : 0);
}

__global__ void __launch_bounds__(TS_WIN * TS_WAVES) k_traj_sample(TrajSmpArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x & (TS_WIN - 1), wv = threadIdx.x >> 6;
  const int b = blockIdx.x * TS_WAVES + wv;
  double* u = reinterpret_cast<double*>(smem_raw) + (size_t)wv * ts_wave_stride(A.cfg);  // [n + p + 1]
  double* uy = u + spline_knot_stride(A.cfg.max_ctrl);                                        // [ny + py + 1]
  const int p = A.cfg.degree, py = A.cfg.yaw_degree, max_t = A.cfg.max_t;
  const bool live = b < A.n_prob;
  int n = 0, ny = 0;
  double dt = 0.0, dty = 0.0;
  if (live) {
    n = spline_n(A.src, b);
    dt = spline_dt_or_one(A.src, b);
    if (A.n_yaw && A.cfg.max_yaw_ctrl > 0) ny = A.n_yaw[b];
    if (ny > 0) dty = A.yaw_dt[b];
  }
  const bool sane_in = live && spline_sane(dt, n, p, A.cfg.max_ctrl) &&
                       (ny <= 0 || (dty > 0.0 && isfinite(dty) && py >= 3 && py <= 5 && ny >= py + 1 && ny <= A.cfg.max_yaw_ctrl));

  // 1. knots (the yaw spline's are always uniform); every wave of the workgroup meets at the barrier, with or without
  // a problem
  const bool sane = spline_stage_knots(A.src, b, u, p, n, dt, lane, sane_in);
  if (sane && lane == 0 && ny > 0) spline_uniform_knots(uy, py, ny, dty);
  __syncthreads();
  if (!live) return;

  const bool command = A.cfg.mode == FUELMI_TRAJSMP_COMMAND;
  const int nt_given = A.n_t[b] < max_t ? A.n_t[b] : max_t;
  const int nt = sane ? nt_given : 0;  // a bad spline is never indexed: its samples are BADSPLINE and 0
  const double D = sane ? u[n] - u[p] : 0.0;
  double T = D;  // traj_duration_ as replanCallback leaves it (:171): min(t_stop, traj_duration_)
  if (A.t_stop) {
    const double ts = A.t_stop[b];
    T = D < ts ? D : ts;
  }
  const double* C = spline_ctrl(A.src, b);
  const double* Cy = ny > 0 ? A.yaw + (size_t)b * A.cfg.max_yaw_ctrl : nullptr;
  const bool record = command && A.flight && sane;
  double* F = A.flight ? A.flight + (size_t)b * 8 : nullptr;
  bool have = false;
  double lp[3] = {0.0, 0.0, 0.0}, last_t = 0.0, length = 0.0, energy = 0.0, n_cmd = 0.0;
  if (record) {
    have = F[0] != 0.0;
    lp[0] = F[1], lp[1] = F[2], lp[2] = F[3];
    last_t = F[4], length = F[5], energy = F[6], n_cmd = F[7];
  }

  // 2. windows of TS_WIN samples; the entries from n_t[b] to max_t are written as 0
  for (int kb = 0; kb < max_t; kb += TS_WIN) {
    const int k = kb + lane;
    int status = k < nt_given && !sane ? FUELMI_TRAJSMP_BADSPLINE : FUELMI_TRAJSMP_IN;
    double t = 0.0;
    double o[4][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};  // pos, vel, acc, jerk
    double y[3][1] = {{0.0}, {0.0}, {0.0}};                                                // yaw, yawdot, yawddot
    if (k < nt) {
      t = A.t[(size_t)b * max_t + k];
      double te = t;
      if (command) {  // cmdCallback :266, :274, :288 in that order
        if (t < T && t >= 0.0)
          status = FUELMI_TRAJSMP_IN;
        else if (t >= T)
          status = FUELMI_TRAJSMP_PAST, te = T;
        else
          status = FUELMI_TRAJSMP_INVALID;
      }
      if (status != FUELMI_TRAJSMP_INVALID) {
        if (p == 3)
          spline_eval_levels<3, 3, 3>(u, n, C, te, o);
        else if (p == 4)
          spline_eval_levels<4, 3, 3>(u, n, C, te, o);
        else
          spline_eval_levels<5, 3, 3>(u, n, C, te, o);
        if (ny > 0) {
          if (py == 3)
            spline_eval_levels<3, 1, 2>(uy, ny, Cy, te, y);
          else if (py == 4)
            spline_eval_levels<4, 1, 2>(uy, ny, Cy, te, y);
          else
            spline_eval_levels<5, 1, 2>(uy, ny, Cy, te, y);
        }
        if (status == FUELMI_TRAJSMP_PAST) {  // the final position and yaw, everything else 0 (:277-281)
          for (int l = 1; l < 4; ++l) o[l][0] = o[l][1] = o[l][2] = 0.0;
          y[1][0] = y[2][0] = 0.0;
        }
      }
    }
    if (k < max_t) {
      const size_t e = (size_t)b * max_t + k;
      A.status[e] = status;
      for (int c = 0; c < 3; ++c) {
        A.o_pos[3 * e + c] = o[0][c];
        A.o_vel[3 * e + c] = o[1][c];
        A.o_acc[3 * e + c] = o[2][c];
        A.o_jerk[3 * e + c] = o[3][c];
      }
      A.o_yaw[e] = y[0][0];
      A.o_yawdot[e] = y[1][0];
      A.o_yawddot[e] = y[2][0];
    }
    // 3. the flight record (:328-339) through this window's samples in order; every lane walks the same chain
    if (record && kb < nt) {
      const int cnt = nt - kb < TS_WIN ? nt - kb : TS_WIN;
      for (int j = 0; j < cnt; ++j) {
        const int sj = __shfl(status, j);
        const double tj = __shfl(t, j);
        const double px = __shfl(o[0][0], j), py_ = __shfl(o[0][1], j), pz = __shfl(o[0][2], j);
        const double jx = __shfl(o[3][0], j), jy = __shfl(o[3][1], j), jz = __shfl(o[3][2], j);
        if (sj != FUELMI_TRAJSMP_INVALID) {
          if (!have) {  // traj_cmd_ is empty: the first position
            have = true;
            lp[0] = px, lp[1] = py_, lp[2] = pz;
            n_cmd = 1.0;
          } else {
            const double dx = px - lp[0], dy = py_ - lp[1], dz = pz - lp[2];
            const double nrm = sqrt(dx * dx + dy * dy + dz * dz);
            if (nrm > 1e-6) {  // a new different commanded position
              lp[0] = px, lp[1] = py_, lp[2] = pz;
              length = length + nrm;                                         // calcPathLength (:49-56)
              energy = energy + (jx * jx + jy * jy + jz * jz) * (tj - last_t);  // :335-336
              n_cmd = n_cmd + 1.0;
            }
          }
        }
        last_t = tj;  // :339
      }
    }
  }
  if (lane == 0) {
    A.duration[b] = D;
    if (record) {
      F[0] = have ? 1.0 : 0.0;
      F[1] = lp[0], F[2] = lp[1], F[3] = lp[2];
      F[4] = last_t, F[5] = length, F[6] = energy, F[7] = n_cmd;
    }
  }
}

size_t ts_lds(const fuelmi_trajsmp_cfg& c) { return (size_t)TS_WAVES * ts_wave_stride(c) * sizeof(double); }

int trajsmp_cfg_check(const fuelmi_trajsmp_cfg* cfg) {
  ARGCHK(cfg);
  ARGCHK(cfg->mode == FUELMI_TRAJSMP_COMMAND || cfg->mode == FUELMI_TRAJSMP_STATE);
  ARGCHK(cfg->degree >= 3 && cfg->degree <= 5);
  ARGCHK(cfg->max_ctrl >= cfg->degree + 1);
  ARGCHK(cfg->max_yaw_ctrl >= 0);
  if (cfg->max_yaw_ctrl > 0) {
    ARGCHK(cfg->yaw_degree >= 3 && cfg->yaw_degree <= 5);
    ARGCHK(cfg->max_yaw_ctrl >= cfg->yaw_degree + 1);
  }
  ARGCHK(cfg->max_t >= 0);
  if (cfg->max_ctrl > FUELMI_TRAJSMP_MAX_CTRL || cfg->max_yaw_ctrl > FUELMI_TRAJSMP_MAX_CTRL) {
    fuelmi_set_error("trajectory sampling: max_ctrl = %d / max_yaw_ctrl = %d exceeds %d", cfg->max_ctrl,
                     cfg->max_yaw_ctrl, FUELMI_TRAJSMP_MAX_CTRL);
    return FUELMI_ELIMIT;
  }
  if (cfg->max_t > FUELMI_TRAJSMP_MAX_T) {
    fuelmi_set_error("trajectory sampling: max_t = %d exceeds %d", cfg->max_t, FUELMI_TRAJSMP_MAX_T);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

// the caller's host arrays of both entries (the first three null for a device batch)
struct TrajSmpIO {
  const int* n_ctrl;
  const double *pos_ctrl, *knot_span;
  const int* n_yaw_ctrl;
  const double *yaw_ctrl, *yaw_dt, *t_stop;
  const int* n_t;
  const double* t;
  int* status;
  double *pos, *vel, *acc, *jerk, *yaw, *yawdot, *yawddot, *duration, *flight;
  const double* knots = nullptr;  // fuelmi_map_sample_trajs_knots: [n_prob][max_ctrl + degree + 1] in place of knot_span
  bool knots_given = false;
};

// the scratch block (a BlockLayout over the map's or the batch's DevScratch): the inputs the host hands over, the
// flight record (in and out), then the results.  base null: only the size.
size_t ts_layout(const fuelmi_trajsmp_cfg& c, int n_prob, bool host_spline, const TrajSmpIO& io, TrajSmpArgs& A,
                 unsigned char* base) {
  const size_t n = (size_t)n_prob, s = n * (size_t)c.max_t;
  BlockLayout L(base, 16);
  if (host_spline) spline_src_take(L, n, c.max_ctrl, A.src);
  if (io.knots_given) A.src.knots_stride = (size_t)c.max_ctrl + c.degree + 1, A.src.knots = L.take<double>(n * A.src.knots_stride);
  const bool yaw = io.n_yaw_ctrl && c.max_yaw_ctrl > 0;
  A.n_yaw = yaw ? L.take<int>(n) : nullptr;
  A.yaw = yaw ? L.take<double>(n * c.max_yaw_ctrl) : nullptr;
  A.yaw_dt = yaw ? L.take<double>(n) : nullptr;
  A.t_stop = io.t_stop ? L.take<double>(n) : nullptr;
  A.n_t = L.take<int>(n);
  A.t = L.take<double>(s);
  A.flight = io.flight ? L.take<double>(n * 8) : nullptr;
  A.status = L.take<int>(s);
  A.o_pos = L.take<double>(3 * s), A.o_vel = L.take<double>(3 * s);
  A.o_acc = L.take<double>(3 * s), A.o_jerk = L.take<double>(3 * s);
  A.o_yaw = L.take<double>(s), A.o_yawdot = L.take<double>(s), A.o_yawddot = L.take<double>(s);
  A.duration = L.take<double>(n);
  return L.size();
}

// the host checks of both entries (*nothing: no problem or no sample, the call returns FUELMI_OK at once); the bytes of
// the scratch block; uploads, the launch on stream st, the results into the caller's arrays and the wait.  A device
// batch presets A's n_ctrl .. knot_stride.
int trajsmp_check(const fuelmi_trajsmp_cfg* cfg, int n_prob, bool host_spline, const TrajSmpIO& io, bool* nothing) {
  {
    const int rc = trajsmp_cfg_check(cfg);
    if (rc) return rc;
  }
  *nothing = true;
  ARGCHK(n_prob >= 0);
  if (n_prob == 0) return FUELMI_OK;
  if ((long long)n_prob * cfg->max_t > FUELMI_TRAJSMP_MAX_SAMPLES) {
    fuelmi_set_error("trajectory sampling: n_prob * max_t = %lld exceeds %d", (long long)n_prob * cfg->max_t,
                     FUELMI_TRAJSMP_MAX_SAMPLES);
    return FUELMI_ELIMIT;
  }
  ARGCHK(io.n_t);
  ARGCHK(io.t || cfg->max_t == 0);
  const int p = cfg->degree, py = cfg->yaw_degree;
  if (cfg->mode == FUELMI_TRAJSMP_STATE) ARGCHK(!io.t_stop && !io.flight);  // cmdCallback's alone
  if (host_spline) {
    const int rc = spline_src_check(n_prob, p, cfg->max_ctrl, io.n_ctrl, io.pos_ctrl, io.knot_span, io.knots_given);
    if (rc) return rc;
    if (io.knots_given) {
      const int rck = spline_knots_check(n_prob, p, cfg->max_ctrl, io.n_ctrl, 0, io.knots);
      if (rck) return rck;
    }
  }
  if (io.n_yaw_ctrl) {
    ARGCHK(cfg->max_yaw_ctrl > 0 && io.yaw_ctrl && io.yaw_dt);
    for (int b = 0; b < n_prob; ++b) {
      const int ny = io.n_yaw_ctrl[b];
      if (ny == 0) continue;  // this problem has no yaw spline
      ARGCHK(ny >= py + 1 && ny <= cfg->max_yaw_ctrl);
      ARGCHK(std::isfinite(io.yaw_dt[b]) && io.yaw_dt[b] > 0.0);
      const double* Y = io.yaw_ctrl + (size_t)b * cfg->max_yaw_ctrl;
      for (int k = 0; k < ny; ++k) ARGCHK(std::fabs(Y[k]) < 1e7);
    }
  }
  for (int b = 0; b < n_prob; ++b) {
    ARGCHK(io.n_t[b] >= 0 && io.n_t[b] <= cfg->max_t);
    const double* t = io.t + (size_t)b * cfg->max_t;
    for (int k = 0; k < io.n_t[b]; ++k) ARGCHK(std::isfinite(t[k]));
    if (io.t_stop) ARGCHK(std::isfinite(io.t_stop[b]));
    if (io.flight)
      for (int k = 0; k < 8; ++k) ARGCHK(std::isfinite(io.flight[(size_t)b * 8 + k]));
    if (io.n_t[b] > 0) *nothing = false;
  }
  if (*nothing) return FUELMI_OK;
  ARGCHK(io.status && io.pos && io.vel && io.acc && io.jerk && io.yaw && io.yawdot && io.yawddot && io.duration);
  return FUELMI_OK;
}

size_t trajsmp_bytes(const fuelmi_trajsmp_cfg* cfg, int n_prob, bool host_spline, const TrajSmpIO& io) {
  TrajSmpArgs A;
  memset(&A, 0, sizeof(A));
  return ts_layout(*cfg, n_prob, host_spline, io, A, nullptr);
}

int trajsmp_run(hipStream_t st, const fuelmi_trajsmp_cfg* cfg, int n_prob, bool host_spline, const TrajSmpIO& io,
                TrajSmpArgs& A, unsigned char* scratch) {
  const fuelmi_trajsmp_cfg& c = *cfg;
  const size_t n = (size_t)n_prob, s = n * (size_t)c.max_t;
  A.cfg = c;
  A.n_prob = n_prob;
  ts_layout(c, n_prob, host_spline, io, A, scratch);
  auto up = [&](const void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
  };
  auto down = [&](void* dst, const void* src, size_t bytes) {
    return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
  };
  if (host_spline) {
    const int rc = spline_src_upload(st, A.src, n, c.max_ctrl, io.n_ctrl, io.pos_ctrl, io.knot_span);
    if (rc) return rc;
  }
  if (io.knots_given) HIPCHK(up(A.src.knots, io.knots, n * A.src.knots_stride * sizeof(double)));
  if (A.n_yaw) {
    HIPCHK(up(A.n_yaw, io.n_yaw_ctrl, n * sizeof(int)));
    HIPCHK(up(A.yaw, io.yaw_ctrl, n * c.max_yaw_ctrl * sizeof(double)));
    HIPCHK(up(A.yaw_dt, io.yaw_dt, n * sizeof(double)));
  }
  if (A.t_stop) HIPCHK(up(A.t_stop, io.t_stop, n * sizeof(double)));
  HIPCHK(up(A.n_t, io.n_t, n * sizeof(int)));
  HIPCHK(up(A.t, io.t, s * sizeof(double)));
  if (A.flight) HIPCHK(up(A.flight, io.flight, n * 8 * sizeof(double)));
  hipLaunchKernelGGL(k_traj_sample, dim3((n_prob + TS_WAVES - 1) / TS_WAVES), dim3(TS_WIN * TS_WAVES), ts_lds(c), st, A);
  HIPCHK(hipGetLastError());
  HIPCHK(down(io.status, A.status, s * sizeof(int)));
  HIPCHK(down(io.pos, A.o_pos, 3 * s * sizeof(double)));
  HIPCHK(down(io.vel, A.o_vel, 3 * s * sizeof(double)));
  HIPCHK(down(io.acc, A.o_acc, 3 * s * sizeof(double)));
  HIPCHK(down(io.jerk, A.o_jerk, 3 * s * sizeof(double)));
  HIPCHK(down(io.yaw, A.o_yaw, s * sizeof(double)));
  HIPCHK(down(io.yawdot, A.o_yawdot, s * sizeof(double)));
  HIPCHK(down(io.yawddot, A.o_yawddot, s * sizeof(double)));
  HIPCHK(down(io.duration, A.duration, n * sizeof(double)));
  if (A.flight) HIPCHK(down(io.flight, A.flight, n * 8 * sizeof(double)));
  HIPCHK(stream_wait(st));
  return FUELMI_OK;
}

}  // namespace

extern "C" int fuelmi_traj_sample_plan(const fuelmi_trajsmp_cfg* cfg, int out3[3]) {
  ARGCHK(out3);
  {
    const int rc = trajsmp_cfg_check(cfg);
    if (rc) return rc;
  }
  out3[0] = TS_WIN, out3[1] = (int)ts_lds(*cfg), out3[2] = FUELMI_TRAJSMP_MAX_CTRL;
  return FUELMI_OK;
}

// the host route of both entries: io's splines uploaded, uniform (knot_span) or on given knots
static int trajsmp_host(fuelmi_map* m, const fuelmi_trajsmp_cfg* cfg, int n_prob, const TrajSmpIO& io) {
  bool nothing = true;
  {  // every argument on the host, before the map is touched
    const int rc = trajsmp_check(cfg, n_prob, true, io, &nothing);
    if (rc) return rc;
  }
  if (nothing) return FUELMI_OK;
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  {
    const int rc = m->trajsmp_dev.reserve(st, trajsmp_bytes(cfg, n_prob, true, io));
    if (rc) return rc;
  }
  TrajSmpArgs A;
  memset(&A, 0, sizeof(A));
  return trajsmp_run(st, cfg, n_prob, true, io, A, m->trajsmp_dev.base());
}

extern "C" int fuelmi_map_sample_trajs(fuelmi_map* m, const fuelmi_trajsmp_cfg* cfg, int n_prob, const int* n_ctrl,
                                       const double* pos_ctrl, const double* knot_span, const int* n_yaw_ctrl,
                                       const double* yaw_ctrl, const double* yaw_dt, const double* t_stop,
                                       const int* n_t, const double* t, int* status, double* pos, double* vel,
                                       double* acc, double* jerk, double* yaw, double* yawdot, double* yawddot,
                                       double* duration, double* flight) {
  const TrajSmpIO io = {n_ctrl, pos_ctrl, knot_span, n_yaw_ctrl, yaw_ctrl, yaw_dt, t_stop, n_t,     t,     status,
                        pos,    vel,      acc,       jerk,       yaw,      yawdot, yawddot, duration, flight};
  return trajsmp_host(m, cfg, n_prob, io);
}

// ... the position splines on whole knot vectors (fuelmi_map_adjust_trajs' knots_out as it stands) in place of the
// spans; the yaw splines stay uniform (the reference builds every one with setUniformBspline)
extern "C" int fuelmi_map_sample_trajs_knots(fuelmi_map* m, const fuelmi_trajsmp_cfg* cfg, int n_prob, const int* n_ctrl,
                                             const double* pos_ctrl, const double* knots, const int* n_yaw_ctrl,
                                             const double* yaw_ctrl, const double* yaw_dt, const double* t_stop,
                                             const int* n_t, const double* t, int* status, double* pos, double* vel,
                                             double* acc, double* jerk, double* yaw, double* yawdot, double* yawddot,
                                             double* duration, double* flight) {
  const TrajSmpIO io = {n_ctrl, pos_ctrl, nullptr, n_yaw_ctrl, yaw_ctrl, yaw_dt,  t_stop,   n_t,    t,     status, pos,
                        vel,    acc,      jerk,    yaw,        yawdot,   yawddot, duration, flight, knots, true};
  return trajsmp_host(m, cfg, n_prob, io);
}

// the batch route: a device batch's optimised position splines sampled as commands or replan states, read from
// the variables the last solve left on the device; the yaw splines and the times come from the host, only results travel
extern "C" int fuelmi_bspline_dev_sample_trajs(fuelmi_bspline_dev* b, const fuelmi_trajsmp_cfg* cfg, const int* n_yaw_ctrl,
                                               const double* yaw_ctrl, const double* yaw_dt, const double* t_stop,
                                               const int* n_t, const double* t, int* status, double* pos, double* vel,
                                               double* acc, double* jerk, double* yaw, double* yawdot, double* yawddot,
                                               double* duration, double* flight) {
  ARGCHK(b && cfg);
  const BsplineArgs& A = b->a;
  ARGCHK(A.dim == 3 && b->opt_valid && b->opt_x);
  ARGCHK(cfg->degree == A.cfg.bspline_degree);
  fuelmi_trajsmp_cfg sc = *cfg;
  sc.max_ctrl = A.N;
  const TrajSmpIO io = {nullptr, nullptr, nullptr, n_yaw_ctrl, yaw_ctrl, yaw_dt, t_stop, n_t,      t,     status,
                        pos,     vel,     acc,     jerk,       yaw,      yawdot, yawddot, duration, flight};
  bool nothing = true;
  {
    const int rc = trajsmp_check(&sc, A.C, false, io, &nothing);
    if (rc) return rc;
  }
  if (nothing) return FUELMI_OK;
  fuelmi_map* m = b->map;
  ARGCHK(m);
  HIPCHK(hipSetDevice(m->device));
  {
    const int rc = b->smp_dev.reserve(m->stream, trajsmp_bytes(&sc, A.C, false, io));
    if (rc) return rc;
  }
  TrajSmpArgs T;
  memset(&T, 0, sizeof(T));
  T.src = opt_spline_src_knots(b);
  return trajsmp_run(m->stream, &sc, A.C, false, io, T, b->smp_dev.base());
}
