// facade_quad.cpp -- drives the exact solve of the optimiser's quadratic phases through the facade, the way
// FastPlannerManager::optimizeTopoBspline runs its first phase (plan_manage/src/planner_manager.cpp:584-588: setGuidePath,
// optimize(ctrl_pts, dt, GUIDE_PHASE, 0, 1) per guide path) and planYawActMap its closing solve
// (planner_manager_dev.cpp:84-92: setWaypoints, optimize(yaw, dt_yaw, SMOOTHNESS | WAYPOINTS | START | END, 1, 1)), and
// prints one JSON document that tests/test_quad_solve_gpu.py reads:
//   "batch"      BsplineOptimizer::optimizeGuidePhase on ALL guide paths, each its own point count, in one device call
//   "exact"      optimize() per guide path with optimization/exact_quadratic set
//   "iterative"  optimize() per guide path as it is without the parameter (max_iteration_num1 = 2 evaluations)
//   "yaw"        the closing yaw solve with the parameter set, and its cost without
//   facade_quad <scenario.bin>
// scenario.bin, all f64: map_size[3], box_min[3], box_max[3]; the number of guide paths; per path N, dt, ctrl[N][3],
// start[3][3], end[3][3], guide[N-6][3]; then the yaw problem: N, dt, ctrl[N], start[3], end[2], the number of
// way-points, their indices, their values.
#include "facade_driver.h"

#include <bspline_opt/bspline_optimizer.h>

typedef std::vector<Eigen::Vector3d> Pts;

static std::vector<double> rd(FILE* in, size_t n) {
  std::vector<double> v(n);
  rd(in, v.data(), n);
  return v;
}
static Pts pts(const std::vector<double>& v) {
  Pts p;
  for (size_t i = 0; i + 2 < v.size(); i += 3) p.push_back(Eigen::Vector3d(v[i], v[i + 1], v[i + 2]));
  return p;
}
static void print_rows(const Eigen::MatrixXd& m) {
  std::printf("[");
  for (int i = 0; i < m.rows(); ++i) {
    std::printf("%s[", i ? ", " : "");
    for (int j = 0; j < m.cols(); ++j) std::printf("%s%.17g", j ? ", " : "", m(i, j));
    std::printf("]");
  }
  std::printf("]");
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  const std::vector<double> hdr = rd(in, 9);
  ros::NodeHandle nh;
  sdf_map_params(nh, hdr.data(), hdr.data() + 3, hdr.data() + 6);
  const EDTEnvironment::Ptr edt = make_map(nh, false).edt;
  optimization_params(nh);
  nh.num["optimization/max_iteration_num2"] = 2000;  // the iterative yaw solve (max_num_id 1) gets 2000 evaluations
  BsplineOptimizer iter, exact;
  iter.setParam(nh);
  iter.setEnvironment(edt);
  nh.num["optimization/exact_quadratic"] = 1;
  exact.setParam(nh);
  exact.setEnvironment(edt);

  const int n = (int)rd(in, 1)[0];
  std::vector<Eigen::MatrixXd> ctrl(n);
  std::vector<double> dts(n);
  std::vector<Pts> start(n), end(n), guide(n);
  for (int b = 0; b < n; ++b) {
    const int N = (int)rd(in, 1)[0];
    dts[b] = rd(in, 1)[0];
    const std::vector<double> c = rd(in, 3 * (size_t)N);
    ctrl[b].resize(N, 3);
    for (int i = 0; i < N; ++i)
      for (int k = 0; k < 3; ++k) ctrl[b](i, k) = c[3 * i + k];
    start[b] = pts(rd(in, 9)), end[b] = pts(rd(in, 9)), guide[b] = pts(rd(in, 3 * (size_t)std::max(N - 6, 0)));
  }
  // one call for every guide path
  std::vector<Eigen::MatrixXd> batch = ctrl;
  std::vector<int> status;
  std::vector<double> cost;
  if (!exact.optimizeGuidePhase(batch, dts, start, end, guide, status, cost)) return 3;
  std::printf("{\"batch\": [");
  for (int b = 0; b < n; ++b) {
    std::printf("%s\n{\"status\": %d, \"cost\": %.17g, \"ctrl\": ", b ? "," : "", status[b], cost[b]);
    print_rows(batch[b]);
    std::printf("}");
  }
  // the reference's loop: one optimize() per guide path, with and without the parameter
  for (int pass = 0; pass < 2; ++pass) {
    BsplineOptimizer& opt = pass ? iter : exact;
    std::printf("],\n\"%s\": [", pass ? "iterative" : "exact");
    for (int b = 0; b < n; ++b) {
      Eigen::MatrixXd c = ctrl[b];
      double dt = dts[b];
      opt.setBoundaryStates(start[b], end[b]);
      opt.setGuidePath(guide[b]);
      opt.optimize(c, dt, BsplineOptimizer::GUIDE_PHASE, 0, 1);
      std::printf("%s\n{\"exact_status\": %d, \"ctrl\": ", b ? "," : "", opt.exact_status_);
      print_rows(c);
      std::printf("}");
    }
  }
  // planYawActMap's closing solve: dimension 1, way-points on every control point but the boundary ones
  const int Ny = (int)rd(in, 1)[0];
  double dty = rd(in, 1)[0];
  const std::vector<double> qy = rd(in, Ny), sy = rd(in, 3), ey = rd(in, 2);
  const int nw = (int)rd(in, 1)[0];
  const std::vector<double> wi = rd(in, nw), wv = rd(in, nw);
  fclose(in);
  Pts waypts;
  std::vector<int> widx;
  for (int j = 0; j < nw; ++j) waypts.push_back(Eigen::Vector3d(wv[j], 0, 0)), widx.push_back((int)wi[j]);
  const int yaw_mask = BsplineOptimizer::SMOOTHNESS | BsplineOptimizer::WAYPOINTS | BsplineOptimizer::START | BsplineOptimizer::END;
  std::printf("],\n\"yaw\": {");
  for (int pass = 0; pass < 2; ++pass) {
    BsplineOptimizer& opt = pass ? iter : exact;
    Eigen::MatrixXd yaw(Ny, 1);
    for (int i = 0; i < Ny; ++i) yaw(i, 0) = qy[i];
    double dt = dty;
    opt.setBoundaryStates({Eigen::Vector3d(sy[0], 0, 0), Eigen::Vector3d(sy[1], 0, 0), Eigen::Vector3d(sy[2], 0, 0)},
                          {Eigen::Vector3d(ey[0], 0, 0), Eigen::Vector3d(ey[1], 0, 0)});
    opt.setWaypoints(waypts, widx);
    opt.optimize(yaw, dt, yaw_mask, 1, 1);
    std::printf("%s\"%s\": {\"exact_status\": %d, \"ctrl\": ", pass ? ", " : "", pass ? "iterative" : "exact", opt.exact_status_);
    print_rows(yaw);
    std::printf("}");
  }
  std::printf("}}\n");
  return 0;
}
