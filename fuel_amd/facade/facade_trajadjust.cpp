// facade_trajadjust.cpp -- drives BsplineOptimizer::adjustTime, ::trajectoryMetrics and ::selectBestTraj the way
// FastPlannerManager uses NonUniformBspline's time adjustment (plan_manage/src/planner_manager.cpp:200-230, :476-482,
// :528-547), and prints one JSON document that tests/test_traj_adjust_gpu.py reads.
//   facade_trajadjust <scenario.bin>
// scenario.bin: double map_size[3], box_min[3], box_max[3], resolution, ground_height; the number of problems; then per
// problem: double degree, n_ctrl, ops, n_knots (0: uniform knots of the span), knot span, has_ratio, ratio_in, limit_vel,
// limit_acc, limit_ratio, lengthen_cap, realloc_iters, length_res, stat_step; then n_ctrl x 3 control points and n_knots
// knots.  A problem with ops == 0 goes through trajectoryMetrics, every other through adjustTime.  The last four
// problems (uniform, one degree) are ranked by selectBestTraj, and the first of them alone once more.  Every double is
// printed as a hex float in a string: the test compares bits.
#include "facade_driver.h"

#include <bspline_opt/bspline_optimizer.h>

static void print_hex(const char* name, const double* v, size_t n) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < n; ++i) std::printf("%s\"%a\"", i ? ", " : "", v[i]);
  std::printf("]");
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  double hdr[12];
  rd(in, hdr, 12);
  ros::NodeHandle nh;
  sdf_map_params(nh, hdr, hdr + 3, hdr + 6, hdr[9], hdr[10]);
  optimization_params(nh);
  const DriverMap dm = make_map(nh, true);  // the adjustment reads no plane and no mirror
  BsplineOptimizer opt;
  opt.setParam(nh);
  opt.setEnvironment(dm.edt);
  const int n_prob = (int)hdr[11];
  if (n_prob < 4 || n_prob > 4096) return 2;
  std::vector<Eigen::MatrixXd> tail;
  std::vector<double> tail_dt;
  int tail_degree = 3;
  std::printf("{\"problems\": [");
  for (int b = 0; b < n_prob; ++b) {
    double head[14];
    if (fread(head, sizeof(double), 14, in) != 14) return 2;
    const int degree = (int)head[0], n_ctrl = (int)head[1], ops = (int)head[2], n_knots = (int)head[3];
    if (n_ctrl < 1 || n_ctrl > 4096 || n_knots < 0 || n_knots > 8192) return 2;
    BsplineOptimizer::TrajAdjust cfg;
    cfg.limit_vel = head[7], cfg.limit_acc = head[8], cfg.limit_ratio = head[9], cfg.lengthen_cap = head[10];
    cfg.realloc_iters = (int)head[11], cfg.length_res = head[12], cfg.stat_step = head[13];
    std::vector<double> c(3 * (size_t)n_ctrl), u((size_t)n_knots);
    if (fread(c.data(), sizeof(double), c.size(), in) != c.size()) return 2;
    if (n_knots && fread(u.data(), sizeof(double), u.size(), in) != u.size()) return 2;
    Eigen::MatrixXd ctrl(n_ctrl, 3);
    for (int i = 0; i < n_ctrl; ++i)
      for (int k = 0; k < 3; ++k) ctrl(i, k) = c[3 * i + k];
    Eigen::VectorXd knots(n_knots);
    for (int i = 0; i < n_knots; ++i) knots(i) = u[i];
    BsplineOptimizer::TrajMetrics r;
    Eigen::MatrixXd samples(0, 3);
    bool ok;
    if (ops == 0) {
      ok = opt.trajectoryMetrics(ctrl, degree, head[4], knots, cfg, r);
      if (ok) {  // (the measured spline's own knots, for the document)
        Eigen::VectorXd again = knots;
        ok = opt.adjustTime(ctrl, degree, head[4], again, 0, nullptr, cfg, r, nullptr);
        knots = again;
      }
    } else {
      ok = opt.adjustTime(ctrl, degree, head[4], knots, ops, head[5] != 0.0 ? &head[6] : nullptr, cfg, r, &samples);
    }
    std::printf("%s\n{\"ok\": %d", b ? "," : "", ok ? 1 : 0);
    if (ok) {
      std::printf(", \"info\": [");
      for (int k = 0; k < FUELMI_TRAJADJ_NI; ++k) std::printf("%s%d", k ? ", " : "", r.info[k]);
      std::printf("], ");
      print_hex("metrics", r.metrics, FUELMI_TRAJADJ_NM - 1);
      std::vector<double> kv((size_t)knots.rows()), sv(3 * (size_t)samples.rows());
      for (int i = 0; i < (int)kv.size(); ++i) kv[i] = knots(i);
      for (int i = 0; i < (int)samples.rows(); ++i)
        for (int k = 0; k < 3; ++k) sv[3 * (size_t)i + k] = samples(i, k);
      std::printf(", ");
      print_hex("knots", kv.data(), kv.size());
      std::printf(", ");
      print_hex("samples", sv.data(), sv.size());
    }
    std::printf("}");
    if (b >= n_prob - 4) tail.push_back(ctrl), tail_dt.push_back(head[4]), tail_degree = degree;
  }
  fclose(in);
  BsplineOptimizer::TrajAdjust cfg;
  std::vector<BsplineOptimizer::TrajMetrics> all;
  const int best = opt.selectBestTraj(tail, tail_degree, tail_dt, cfg, &all);
  const int none = opt.selectBestTraj({tail[0]}, tail_degree, {tail_dt[0]}, cfg, nullptr);
  std::printf("\n], \"best\": %d, \"best_of_none\": %d}\n", best, none);
  return 0;
}
