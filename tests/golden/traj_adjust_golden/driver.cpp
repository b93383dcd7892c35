// Runs one scene of tests/traj_adjust_cases.py through the reference's own NonUniformBspline
// (bspline/src/non_uniform_bspline.cpp, compiled unmodified beside this file) and writes what it gives as hex floats.
// The calls are the ones the reference's callers make: setPhysicalLimits, checkRatio, checkFeasibility,
// lengthenTime(min(cap, ratio)) (planner_manager.cpp:205, :534-536), the reallocation loop (:222-230), getTimeSum,
// getLength, getJerk, getMeanAndMaxVel / Acc and the sampling loop of reparamBspline (:541-543).
// in:  p n has_knots ops has_ratio iters loops / dt ratio_in limit_vel limit_acc cap res / ctrl [n][3] / knots [n + p + 1]
// With a third argument (a number of repetitions) the whole sequence, from the constructor on, is also timed that often and
// the median in microseconds goes to stdout (scripts/traj_adjust_timing.py: the reference on one CPU core).
// out: feasible_in iters feasible feasible_out num_vel num_acc n_samples, then duration_in ratio duration_out length
//      jerk mean_vel max_vel mean_acc max_acc dt_out time_inc, then the knots, then the samples
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bspline/non_uniform_bspline.h"

using fast_planner::NonUniformBspline;

static double rd(FILE* f) {
  char tok[64];
  if (fscanf(f, "%63s", tok) != 1) exit(2);
  return strtod(tok, nullptr);
}

// the sample count getMeanAndMaxVel / Acc divide by (:307, :330): the class keeps it to itself
static int count_stat(NonUniformBspline d) {
  double tm, tmp;
  d.getTimeSpan(tm, tmp);
  int num = 0;
  for (double t = tm; t <= tmp; t += 0.01) ++num;
  return num;
}

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  int p, n, has_knots, ops, has_ratio, iters, loops;
  if (fscanf(f, "%d %d %d %d %d %d %d", &p, &n, &has_knots, &ops, &has_ratio, &iters, &loops) != 7) return 2;
  const double dt = rd(f), ratio_in = rd(f), limit_vel = rd(f), limit_acc = rd(f), cap = rd(f), res = rd(f);
  Eigen::MatrixXd ctrl(n, 3);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 3; ++j) ctrl(i, j) = rd(f);
  Eigen::VectorXd knot(has_knots ? n + p + 1 : 0);
  for (int i = 0; i < (int)knot.rows(); ++i) knot(i) = rd(f);
  fclose(f);
  double length = 0.0, mean_v = 0.0, max_v = 0.0, mean_a = 0.0, max_a = 0.0, duration_in = 0.0, ratio = 0.0, duration = 0.0,
         jerk = 0.0, dt_out = 0.0, time_inc = 0.0;
  int num_v = 0, num_a = 0, iter_num = 0;
  bool feasible_in = false, feasible = false, feasible_out = false;
  std::vector<Eigen::VectorXd> point_set;
  Eigen::VectorXd u;
  auto run = [&]() {
    NonUniformBspline pos(ctrl, p, has_knots ? 1.0 : dt);
    if (has_knots) pos.setKnot(knot);
    pos.setPhysicalLimits(limit_vel, limit_acc);
    duration_in = pos.getTimeSum();
    ratio = pos.checkRatio();
    feasible_in = pos.checkFeasibility(false);
    if (ops & 1) pos.lengthenTime(min(cap, has_ratio ? ratio_in : ratio));
    feasible = pos.checkFeasibility(false);
    iter_num = 0;
    if (ops & 2) {
      while (!feasible) {
        feasible = pos.reallocateTime();
        if (++iter_num >= iters) break;
      }
    }
    feasible_out = pos.checkFeasibility(false);
    duration = pos.getTimeSum();
    jerk = pos.getJerk();
    const int seg_num = pos.getControlPoint().rows() - p;
    dt_out = duration / double(seg_num);
    time_inc = duration - duration_in;
    point_set.clear();
    if (loops) {
      length = pos.getLength(res);
      pos.getMeanAndMaxVel(mean_v, max_v);
      pos.getMeanAndMaxAcc(mean_a, max_a);
      num_v = count_stat(pos.getDerivative());
      num_a = count_stat(pos.getDerivative().getDerivative());
      if (ops & 4)
        for (double time = 0.0; time <= duration + 1e-4; time += dt_out) point_set.push_back(pos.evaluateDeBoorT(time));
    }
    u = pos.getKnot();
  };
  run();
  if (argc == 4) {
    std::vector<double> us;
    for (int r = 0; r < atoi(argv[3]); ++r) {
      const auto a = std::chrono::steady_clock::now();
      run();
      us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count());
    }
    std::sort(us.begin(), us.end());
    if (!us.empty()) printf("%.3f\n", us[us.size() / 2]);
  }
  FILE* o = fopen(argv[2], "w");
  if (!o) return 2;
  fprintf(o, "%d %d %d %d %d %d %d", feasible_in ? 1 : 0, iter_num, feasible ? 1 : 0, feasible_out ? 1 : 0, num_v, num_a,
          (int)point_set.size());
  for (double v : {duration_in, ratio, duration, length, jerk, mean_v, max_v, mean_a, max_a, dt_out, time_inc}) fprintf(o, " %a", v);
  for (int i = 0; i < n + p + 1; ++i) fprintf(o, " %a", u(i));
  for (const auto& pt : point_set)
    for (int j = 0; j < 3; ++j) fprintf(o, " %a", pt(j));
  fprintf(o, "\n");
  fclose(o);
  return 0;
}
