// facade_localseg.cpp -- drives BsplineOptimizer::paramLocalTraj and ::reparamLocalTraj the way FastPlannerManager's
// topoReplan and optimizeTopoBspline use their namesakes (plan_manage/src/planner_manager.cpp:391-474, :553-603) with
// every host mirror of the map switched off, and prints what tests/test_localseg_facade_gpu.py compares with the
// restatement and with the C-ABI; doubles as hexadecimal floats.
//   facade_localseg <scenario.bin>
// scenario.bin: double map_size[3], box_min[3], box_max[3], resolution, ground_height, the number of states; then per
// state: double degree, S, global_duration, n_local, local_knot_span, local_ts, local_te, time_change, last_time_inc,
// the number of problems; S segment times; S x 3 x 6 coefficients; n_local x 3 control points; then per problem: double
// mode, start_t, arg0, arg1.  A SPHERE problem is one paramLocalTraj; consecutive DURATION problems with one start_t and
// one duration are ONE reparamLocalTraj over their dt.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <plan_env/sdf_map.h>
#include <plan_env/edt_environment.h>
#include <active_perception/graph_node.h>
#include <active_perception/perception_utils.h>
#include <bspline_opt/bspline_optimizer.h>

namespace fast_planner {
// the package's own ViewNode in a FUEL workspace (graph_node.cpp); the facade library refers to it, nothing here calls it
double ViewNode::computeCost(const Eigen::Vector3d& p1, const Eigen::Vector3d& p2, const double&, const double&,
                             const Eigen::Vector3d&, const double&, std::vector<Eigen::Vector3d>& path) {
  path = {p1, p2};
  return (p2 - p1).norm();
}
double ViewNode::searchPath(const Eigen::Vector3d& p1, const Eigen::Vector3d& p2, std::vector<Eigen::Vector3d>& path) {
  path = {p1, p2};
  return (p2 - p1).norm();
}
PerceptionUtils::PerceptionUtils(ros::NodeHandle&) {}
}  // namespace fast_planner
using namespace fast_planner;

static void put(size_t s, size_t b, const BsplineOptimizer::LocalSegment& o) {
  std::printf("seg %zu %zu %d %d %d %a %a %a %d %zu %zu\n", s, b, o.status, o.n_steps, o.seg_num, o.segment_len, o.dt,
              o.duration, (int)o.ctrl_pts.rows(), o.points.size(), o.start_end_derivative.size());
  std::printf("ctrl %zu %zu", s, b);
  for (int i = 0; i < o.ctrl_pts.rows(); ++i) std::printf(" %a %a %a", o.ctrl_pts(i, 0), o.ctrl_pts(i, 1), o.ctrl_pts(i, 2));
  std::printf("\npoints %zu %zu", s, b);
  for (const auto& q : o.points) std::printf(" %a %a %a", q(0), q(1), q(2));
  std::printf("\nderivs %zu %zu", s, b);
  for (const auto& q : o.start_end_derivative) std::printf(" %a %a %a", q(0), q(1), q(2));
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  double hdr[12];
  if (fread(hdr, sizeof(double), 12, in) != 12) return 2;
  ros::NodeHandle nh;
  auto& P = nh.num;
  P["sdf_map/resolution"] = hdr[9];
  P["sdf_map/map_size_x"] = hdr[0], P["sdf_map/map_size_y"] = hdr[1], P["sdf_map/map_size_z"] = hdr[2];
  P["sdf_map/obstacles_inflation"] = 0.199, P["sdf_map/local_bound_inflate"] = 0.5, P["sdf_map/ground_height"] = hdr[10];
  P["sdf_map/default_dist"] = 0.0, P["sdf_map/optimistic"] = 0, P["sdf_map/signed_dist"] = 0;
  P["sdf_map/p_hit"] = 0.65, P["sdf_map/p_miss"] = 0.35, P["sdf_map/p_min"] = 0.12, P["sdf_map/p_max"] = 0.90;
  P["sdf_map/p_occ"] = 0.80, P["sdf_map/max_ray_length"] = 4.5, P["sdf_map/virtual_ceil_height"] = -10;
  const char* ax[3] = {"x", "y", "z"};
  for (int i = 0; i < 3; ++i) {
    P[std::string("sdf_map/box_min_") + ax[i]] = hdr[3 + i];
    P[std::string("sdf_map/box_max_") + ax[i]] = hdr[6 + i];
  }
  SDFMap::Ptr map(new SDFMap);
  map->initMap(nh);
  map->setHostMirror(false, false, false);  // the local segment reads no voxel and no mirror
  EDTEnvironment::Ptr edt(new EDTEnvironment);
  edt->setMap(map);
  P["optimization/ld_smooth"] = 20.0, P["optimization/ld_dist"] = 10.0, P["optimization/ld_feasi"] = 2.0;
  P["optimization/ld_start"] = 100.0, P["optimization/ld_end"] = 0.5, P["optimization/ld_guide"] = 1.5;
  P["optimization/ld_waypt"] = 0.3, P["optimization/ld_view"] = 0.0, P["optimization/ld_time"] = 1.0;
  P["optimization/dist0"] = 0.7, P["optimization/max_vel"] = 2.0, P["optimization/max_acc"] = 2.0;
  P["optimization/dlmin"] = 0.0, P["optimization/wnl"] = 1.0;
  P["optimization/max_iteration_num1"] = 2, P["optimization/max_iteration_num2"] = 100;
  P["optimization/max_iteration_num3"] = 100, P["optimization/max_iteration_num4"] = 100;
  const int n_state = (int)hdr[11];
  if (n_state < 1 || n_state > 4096) return 2;
  for (size_t s = 0; s < (size_t)n_state; ++s) {
    double sh[10];
    if (fread(sh, sizeof(double), 10, in) != 10) return 2;
    const int degree = (int)sh[0], S = (int)sh[1], nl = (int)sh[3], n_prob = (int)sh[9];
    if (S < 1 || S > 4096 || nl < 0 || nl > 4096 || n_prob < 0 || n_prob > 4096) return 2;
    BsplineOptimizer::GlobalTrajState st;
    st.global_duration = sh[2], st.local_knot_span = sh[4], st.local_start_time = sh[5], st.local_end_time = sh[6];
    st.time_change = sh[7], st.last_time_inc = sh[8];
    st.seg_times.resize(S);
    if (fread(st.seg_times.data(), sizeof(double), S, in) != (size_t)S) return 2;
    std::vector<double> lc(3 * (size_t)nl), pr(4 * (size_t)n_prob);
    st.coef.resize(18 * (size_t)S);
    if (fread(st.coef.data(), sizeof(double), st.coef.size(), in) != st.coef.size()) return 2;
    if (fread(lc.data(), sizeof(double), lc.size(), in) != lc.size()) return 2;
    if (fread(pr.data(), sizeof(double), pr.size(), in) != pr.size()) return 2;
    st.local_ctrl.resize(nl, 3);
    for (int i = 0; i < nl; ++i)
      for (int k = 0; k < 3; ++k) st.local_ctrl(i, k) = lc[3 * (size_t)i + k];
    P["manager/bspline_degree"] = degree;
    BsplineOptimizer opt;
    opt.setParam(nh);
    opt.setEnvironment(edt);
    for (int b = 0; b < n_prob;) {
      const double* q = &pr[4 * (size_t)b];
      if ((int)q[0] == FUELMI_LOCALSEG_SPHERE) {
        BsplineOptimizer::LocalSegment o;
        const bool ok = opt.paramLocalTraj(st, q[1], q[2], q[3], o);
        std::printf("call %zu %d 1 %d\n", s, b, ok ? 1 : 0);
        if (ok) put(s, b, o);
        ++b;
        continue;
      }
      int e = b;
      std::vector<double> dts;
      while (e < n_prob && (int)pr[4 * (size_t)e] == FUELMI_LOCALSEG_DURATION && pr[4 * (size_t)e + 1] == q[1] &&
             pr[4 * (size_t)e + 2] == q[2])
        dts.push_back(pr[4 * (size_t)e++ + 3]);
      std::vector<BsplineOptimizer::LocalSegment> all;
      const bool ok = opt.reparamLocalTraj(st, q[1], q[2], dts, all);
      std::printf("call %zu %d %d %d\n", s, b, e - b, ok ? 1 : 0);
      if (ok)
        for (int i = b; i < e; ++i) put(s, i, all[i - b]);
      b = e;
    }
  }
  fclose(in);
  return 0;
}
