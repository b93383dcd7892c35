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
#include "facade_driver.h"

#include <bspline_opt/bspline_optimizer.h>

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
  rd(in, hdr, 12);
  ros::NodeHandle nh;
  auto& P = nh.num;
  sdf_map_params(nh, hdr, hdr + 3, hdr + 6, hdr[9], hdr[10]);
  optimization_params(nh);
  const DriverMap dm = make_map(nh, true);  // the local segment reads no voxel and no mirror
  const EDTEnvironment::Ptr& edt = dm.edt;
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
