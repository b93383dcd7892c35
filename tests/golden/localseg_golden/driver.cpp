// The reference's GlobalTrajData (plan_manage/include/plan_manage/plan_container.hpp) over its real PolynomialTraj and
// NonUniformBspline, driven for tests/golden/make_localseg_golden.py.
//   driver <in.txt> <out.txt>
// in.txt, records, doubles as hexadecimal floats:
//   S degree n_seg global_duration n_local span local_ts local_te time_change last_time_inc <times> <coef> <ctrl>
//       the state of the problems that follow.  The members are public and are set as setGlobalTraj / setLocalTraj leave
//       them: the segments through addSegment, local_traj_ = {spline, getDerivative(), its getDerivative()}.
//   P mode start_t arg0 arg1
//       mode 0: getTrajInfoInSphere(start_t, radius = arg0, dist_pt = arg1); mode 1: getTrajInfoInDuration(start_t,
//       duration = arg0, dt = arg1)
// out.txt, one line a problem: n_points dt duration, the four derivatives, the points.  seg_num is a local of
// getTrajInfoInSphere and is not printed.  The time inside the two functions goes to stderr.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include <plan_manage/plan_container.hpp>

using namespace fast_planner;

static double num(std::ifstream& in) {
  std::string s;
  in >> s;
  return strtod(s.c_str(), nullptr);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream in(argv[1]);
  FILE* out = std::fopen(argv[2], "w");
  GlobalTrajData g;
  double secs = 0.0;
  std::string kind;
  while (in >> kind) {
    if (kind == "S") {
      int degree, n_seg, n_local;
      in >> degree >> n_seg;
      const double gd = num(in);
      in >> n_local;
      const double span = num(in), lts = num(in), lte = num(in), tchg = num(in), linc = num(in);
      std::vector<double> T(n_seg);
      for (double& t : T) t = num(in);
      PolynomialTraj traj;
      traj.reset();
      for (int s = 0; s < n_seg; ++s) {
        Polynomial::Vector6d c[3];
        for (auto& ax : c)
          for (int i = 0; i < 6; ++i) ax[i] = num(in);
        traj.addSegment(Polynomial(c[0], c[1], c[2], T[s]));
      }
      g = GlobalTrajData();
      g.global_traj_ = traj;
      g.global_duration_ = gd;
      g.local_start_time_ = lts, g.local_end_time_ = lte, g.time_change_ = tchg, g.last_time_inc_ = linc;
      if (n_local > 0) {
        Eigen::MatrixXd ctrl(n_local, 3);
        for (int i = 0; i < n_local; ++i)
          for (int d = 0; d < 3; ++d) ctrl(i, d) = num(in);
        g.local_traj_.resize(3);
        g.local_traj_[0] = NonUniformBspline(ctrl, degree, span);
        g.local_traj_[1] = g.local_traj_[0].getDerivative();
        g.local_traj_[2] = g.local_traj_[1].getDerivative();
      }
    } else {
      int mode;
      in >> mode;
      const double start_t = num(in), a0 = num(in), a1 = num(in);
      vector<Eigen::Vector3d> pts, der;
      double dt = a1, duration = a0;
      const auto t0 = std::chrono::steady_clock::now();
      if (mode == 0)
        g.getTrajInfoInSphere(start_t, a0, a1, pts, der, dt, duration);
      else
        g.getTrajInfoInDuration(start_t, a0, a1, pts, der);
      secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      std::fprintf(out, "%d %a %a", (int)pts.size(), dt, duration);
      for (const auto& q : der) std::fprintf(out, " %a %a %a", q(0), q(1), q(2));
      for (const auto& q : pts) std::fprintf(out, " %a %a %a", q(0), q(1), q(2));
      std::fprintf(out, "\n");
    }
  }
  std::fclose(out);
  std::fprintf(stderr, "getTrajInfo seconds %.9f\n", secs);
  return 0;
}
