// facade_trajsample.cpp -- drives BsplineOptimizer::evaluateCommand and ::replanState the way traj_server's cmdCallback
// (plan_manage/src/traj_server.cpp:257-343) and the exploration FSM's replan branch (fast_exploration_fsm.cpp:86-95) use a
// finished trajectory, runs the same loop through a literal host restatement of NonUniformBspline in the same process,
// and prints one JSON document that tests/test_traj_sample_gpu.py and scripts/traj_sample_timing.py read.
//   facade_trajsample <scenario.bin> [reps]
// scenario.bin: double map_size[3], box_min[3], box_max[3], resolution, ground_height; then any number of problems:
// double mode, degree, n_ctrl, knot span, yaw_degree, n_yaw (0: no yaw spline), yaw_dt, has_t_stop, t_stop, n_t; then
// n_ctrl x 3 control points, n_yaw yaw control points, n_t times.  COMMAND problems go through evaluateCommand in one
// call with a flight record from zeros; STATE problems through one replanState per time.  With reps > 0 every problem is
// also timed, median of reps runs each: the facade's device route and the host loop.
#include "facade_driver.h"

#include <bspline_opt/bspline_optimizer.h>

// NonUniformBspline on the host with the members evaluateDeBoor reads: setUniformBspline's knots (:25-31), evaluateDeBoorT
// (:51-75) and getDerivative (:77-106) as the class has them -- a derivative is a spline of its own
struct HostSpline {
  std::vector<std::vector<double>> c;  // control_points_ rows
  int p = 0;
  std::vector<double> u;
  HostSpline() {}
  HostSpline(const std::vector<std::vector<double>>& ctrl, int degree, double dt) : c(ctrl), p(degree) {
    const int m = (int)c.size() + p;
    u.assign(m + 1, 0.0);
    for (int i = 0; i <= m; ++i) u[i] = i <= p ? double(-p + i) * dt : u[i - 1] + dt;
  }
  double duration() const { return u[c.size()] - u[p]; }  // u_(m_ - p_) - u_(p_)
  std::vector<double> at(double t) const {
    const double ub = std::min(std::max(u[p], t + u[p]), u[c.size()]);
    int k = p;
    while (u[k + 1] < ub) ++k;
    std::vector<std::vector<double>> d;
    for (int i = 0; i <= p; ++i) d.push_back(c[k - p + i]);
    for (int r = 1; r <= p; ++r)
      for (int i = p; i >= r; --i) {
        const double alpha = (ub - u[i + k - p]) / (u[i + 1 + k - r] - u[i + k - p]);
        for (size_t a = 0; a < d[i].size(); ++a) d[i][a] = (1 - alpha) * d[i - 1][a] + alpha * d[i][a];
      }
    return d[p];
  }
  HostSpline derivative() const {
    HostSpline q;
    q.p = p - 1;
    for (size_t i = 0; i + 1 < c.size(); ++i) {
      std::vector<double> row(c[i].size());
      for (size_t a = 0; a < row.size(); ++a) row[a] = double(p) * (c[i + 1][a] - c[i][a]) / (u[i + p + 1] - u[i + 1]);
      q.c.push_back(row);
    }
    q.u.assign(u.begin() + 1, u.end() - 1);
    return q;
  }
};

struct Problem {
  int mode, degree, yaw_degree, has_stop;
  double dt, yaw_dt, t_stop;
  Eigen::MatrixXd ctrl, yaw;
  std::vector<double> t;
};

// per sample: status, pos, vel, acc, jerk, yaw, yawdot, yawddot (16 numbers after the status)
struct Result {
  std::vector<int> status;
  std::vector<double> v;  // [n_t][16]
  double flight[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

static void host_route(const Problem& P, Result& R) {
  std::vector<std::vector<double>> c, y;
  for (int i = 0; i < P.ctrl.rows(); ++i) c.push_back({P.ctrl(i, 0), P.ctrl(i, 1), P.ctrl(i, 2)});
  for (int i = 0; i < P.yaw.rows(); ++i) y.push_back({P.yaw(i, 0)});
  std::vector<HostSpline> traj(1, HostSpline(c, P.degree, P.dt)), ytraj;  // bsplineCallback :239-245
  for (int o = 0; o < 3; ++o) traj.push_back(traj.back().derivative());
  if (!y.empty()) {
    ytraj.push_back(HostSpline(y, P.yaw_degree, P.yaw_dt));
    for (int o = 0; o < 2; ++o) ytraj.push_back(ytraj.back().derivative());
  }
  double traj_duration = traj[0].duration();
  if (P.has_stop) traj_duration = std::min(P.t_stop, traj_duration);  // replanCallback :171
  const size_t n_t = P.t.size();
  R.status.assign(n_t, 0);
  R.v.assign(16 * n_t, 0.0);
  std::vector<std::vector<double>> traj_cmd;
  double energy = 0.0, last_time = 0.0;
  for (size_t k = 0; k < n_t; ++k) {
    const double t_cur = P.t[k];
    double* o = &R.v[16 * k];
    int status = FUELMI_TRAJSMP_IN;
    double te = t_cur;
    if (P.mode == FUELMI_TRAJSMP_COMMAND) {
      if (t_cur < traj_duration && t_cur >= 0.0)
        status = FUELMI_TRAJSMP_IN;
      else if (t_cur >= traj_duration)
        status = FUELMI_TRAJSMP_PAST, te = traj_duration;
      else
        status = FUELMI_TRAJSMP_INVALID;
    }
    R.status[k] = status;
    if (status != FUELMI_TRAJSMP_INVALID) {
      const int levels = status == FUELMI_TRAJSMP_PAST ? 1 : 4;
      for (int l = 0; l < levels; ++l) {
        const std::vector<double> q = traj[l].at(te);
        for (int a = 0; a < 3; ++a) o[3 * l + a] = q[a];
      }
      if (!ytraj.empty())
        for (int l = 0; l < (status == FUELMI_TRAJSMP_PAST ? 1 : 3); ++l) o[12 + l] = ytraj[l].at(te)[0];
    }
    if (P.mode != FUELMI_TRAJSMP_COMMAND) continue;
    if (status != FUELMI_TRAJSMP_INVALID) {  // :328-339
      const std::vector<double> pos = {o[0], o[1], o[2]};
      if (traj_cmd.empty()) {
        traj_cmd.push_back(pos);
      } else {
        const std::vector<double>& b = traj_cmd.back();
        const double dx = pos[0] - b[0], dy = pos[1] - b[1], dz = pos[2] - b[2];
        if (std::sqrt(dx * dx + dy * dy + dz * dz) > 1e-6) {
          traj_cmd.push_back(pos);
          energy += (o[9] * o[9] + o[10] * o[10] + o[11] * o[11]) * (t_cur - last_time);
        }
      }
    }
    last_time = t_cur;
  }
  if (P.mode != FUELMI_TRAJSMP_COMMAND) return;
  double len = 0.0;  // calcPathLength :49-56
  for (size_t i = 0; i + 1 < traj_cmd.size(); ++i) {
    const double dx = traj_cmd[i + 1][0] - traj_cmd[i][0], dy = traj_cmd[i + 1][1] - traj_cmd[i][1],
                 dz = traj_cmd[i + 1][2] - traj_cmd[i][2];
    len += std::sqrt(dx * dx + dy * dy + dz * dz);
  }
  R.flight[0] = traj_cmd.empty() ? 0.0 : 1.0;
  for (int a = 0; a < 3; ++a) R.flight[1 + a] = traj_cmd.empty() ? 0.0 : traj_cmd.back()[a];
  R.flight[4] = last_time, R.flight[5] = len, R.flight[6] = energy, R.flight[7] = (double)traj_cmd.size();
}

static bool device_route(BsplineOptimizer& opt, const Problem& P, Result& R) {
  const size_t n_t = P.t.size();
  R.status.assign(n_t, 0);
  R.v.assign(16 * n_t, 0.0);
  for (double& f : R.flight) f = 0.0;
  if (P.mode == FUELMI_TRAJSMP_COMMAND) {
    Eigen::MatrixXd pos, vel, acc, jerk, yaw;
    if (!opt.evaluateCommand(P.ctrl, P.degree, P.dt, P.yaw, P.yaw_degree, P.yaw_dt, P.t, P.has_stop ? &P.t_stop : nullptr,
                             R.status, pos, vel, acc, jerk, yaw, R.flight))
      return false;
    for (size_t k = 0; k < n_t; ++k)
      for (int a = 0; a < 3; ++a) {
        R.v[16 * k + a] = pos(k, a), R.v[16 * k + 3 + a] = vel(k, a), R.v[16 * k + 6 + a] = acc(k, a);
        R.v[16 * k + 9 + a] = jerk(k, a), R.v[16 * k + 12 + a] = yaw(k, a);
      }
    return true;
  }
  for (size_t k = 0; k < n_t; ++k) {
    Eigen::Vector3d pt, vel, acc, yaw;
    if (!opt.replanState(P.ctrl, P.degree, P.dt, P.yaw, P.yaw_degree, P.yaw_dt, P.t[k], pt, vel, acc, yaw)) return false;
    for (int a = 0; a < 3; ++a)
      R.v[16 * k + a] = pt(a), R.v[16 * k + 3 + a] = vel(a), R.v[16 * k + 6 + a] = acc(a), R.v[16 * k + 12 + a] = yaw(a);
  }
  return true;
}

static void print_result(const char* name, const Result& R, bool command) {
  std::printf("\"%s\": {\"status\": [", name);
  for (size_t k = 0; k < R.status.size(); ++k) std::printf("%s%d", k ? ", " : "", R.status[k]);
  std::printf("], \"values\": [");
  for (size_t k = 0; k < R.v.size(); ++k) std::printf("%s%.17g", k ? ", " : "", R.v[k]);
  std::printf("], \"flight\": [");
  for (int k = 0; k < (command ? 8 : 0); ++k) std::printf("%s%.17g", k ? ", " : "", R.flight[k]);
  std::printf("]}");
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  const int reps = argc > 2 ? atoi(argv[2]) : 0;
  double hdr[11];
  rd(in, hdr, 11);
  ros::NodeHandle nh;
  sdf_map_params(nh, hdr, hdr + 3, hdr + 6, hdr[9], hdr[10]);
  optimization_params(nh);
  const DriverMap dm = make_map(nh, true);  // sampling reads no plane and no mirror
  BsplineOptimizer opt;
  opt.setParam(nh);
  opt.setEnvironment(dm.edt);
  std::printf("{\"problems\": [");
  double head[10];
  for (int b = 0; fread(head, sizeof(double), 10, in) == 10; ++b) {
    Problem Q;
    Q.mode = (int)head[0], Q.degree = (int)head[1], Q.dt = head[3], Q.yaw_degree = (int)head[4], Q.yaw_dt = head[6];
    Q.has_stop = (int)head[7], Q.t_stop = head[8];
    const int n_ctrl = (int)head[2], n_yaw = (int)head[5], n_t = (int)head[9];
    if (n_ctrl < 1 || n_ctrl > 4096 || n_yaw < 0 || n_yaw > 4096 || n_t < 0 || n_t > (1 << 20)) return 2;
    std::vector<double> c(3 * (size_t)n_ctrl), y((size_t)n_yaw);
    Q.t.assign((size_t)n_t, 0.0);
    if (fread(c.data(), sizeof(double), c.size(), in) != c.size()) return 2;
    if (n_yaw && fread(y.data(), sizeof(double), y.size(), in) != y.size()) return 2;
    if (n_t && fread(Q.t.data(), sizeof(double), Q.t.size(), in) != Q.t.size()) return 2;
    Q.ctrl = Eigen::MatrixXd(n_ctrl, 3);
    for (int i = 0; i < n_ctrl; ++i)
      for (int k = 0; k < 3; ++k) Q.ctrl(i, k) = c[3 * i + k];
    Q.yaw = Eigen::MatrixXd(n_yaw, 1);
    for (int i = 0; i < n_yaw; ++i) Q.yaw(i, 0) = y[i];
    Result dev, host;
    const bool ok = n_t == 0 || device_route(opt, Q, dev);
    host_route(Q, host);
    const bool command = Q.mode == FUELMI_TRAJSMP_COMMAND;
    std::printf("%s\n{\"ok\": %d, ", b ? "," : "", ok ? 1 : 0);
    if (reps > 0) {
      const double us_dev = median_us(reps, [&] { device_route(opt, Q, dev); });
      const double us_host = median_us(reps, [&] { host_route(Q, host); });
      std::printf("\"n_t\": %d, \"device_us\": %.3f, \"host_us\": %.3f}", n_t, us_dev, us_host);
      continue;  // (a timing run prints no values)
    }
    print_result("device", dev, command);
    std::printf(", ");
    print_result("host", host, command);
    std::printf("}");
  }
  fclose(in);
  std::printf("\n]}\n");
  return 0;
}
