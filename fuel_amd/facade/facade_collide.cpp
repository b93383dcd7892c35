// facade_collide.cpp -- the collide branch of FastPlannerManager::topoReplan (plan_manage/src/planner_manager.cpp:416-453)
// through the facade's TopologyPRM with every host mirror of the map switched off: findCollisionRange on the local
// segment's control points, findTopoPaths between colli_start.front() and colli_end.back() with the start_pts / end_pts it
// produced, then guidePoints of every select path.  Prints what tests/test_collide_facade_gpu.py compares with the
// restatement and with the C-ABI on the same map and sample stream; doubles as hexadecimal floats.
//   facade_collide <scenario.bin>
// scenario.bin: double map_size[3], resolution, ground_height; sample_inflate[3], clearance, ratio_to_short,
// max_sample_num, max_raw_path, max_raw_path2, reserve_num, seed; ctrl_pt_dist; one occupancy log-odds grid (f64, the
// map's voxel count); then any number of problems: double degree, n_ctrl, dt, and n_ctrl control points.  Every problem is
// searched with the engine seeded anew.
#include "facade_driver.h"

#include <path_searching/topo_prm.h>

static void put_path(const char* tag, size_t b, const vector<Eigen::Vector3d>& p) {
  std::printf("%s %zu %zu", tag, b, p.size());
  for (const auto& q : p) std::printf(" %a %a %a", q(0), q(1), q(2));
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  double hdr[16];
  rd(in, hdr, 16);
  ros::NodeHandle nh;
  auto& P = nh.num;
  double box_lo[3], box_hi[3];
  whole_map_box(hdr, hdr[4], box_lo, box_hi);
  sdf_map_params(nh, hdr, box_lo, box_hi, hdr[3], hdr[4]);
  P["topo_prm/sample_inflate_x"] = hdr[5], P["topo_prm/sample_inflate_y"] = hdr[6], P["topo_prm/sample_inflate_z"] = hdr[7];
  P["topo_prm/clearance"] = hdr[8], P["topo_prm/ratio_to_short"] = hdr[9], P["topo_prm/max_sample_num"] = hdr[10];
  P["topo_prm/max_raw_path"] = hdr[11], P["topo_prm/max_raw_path2"] = hdr[12], P["topo_prm/reserve_num"] = hdr[13];
  P["topo_prm/seed"] = hdr[14];
  const double ctrl_pt_dist = hdr[15];
  const DriverMap dm = make_map(nh, true);  // nothing below reads or refreshes a mirror
  const EDTEnvironment::Ptr& edt = dm.edt;
  load_occupancy(*dm.map, in, LOAD_BOUND | LOAD_INFLATE_ABI | LOAD_ESDF);
  double rec[3];
  for (size_t b = 0; fread(rec, sizeof(double), 3, in) == 3; ++b) {
    const int degree = (int)rec[0], n = (int)rec[1];
    const double dt = rec[2];
    if (n < 1 || n > 4096) return 2;
    std::vector<double> c(3 * (size_t)n);
    if (fread(c.data(), sizeof(double), c.size(), in) != c.size()) return 2;
    Eigen::MatrixXd ctrl(n, 3);
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) ctrl(i, k) = c[3 * i + k];
    const double duration = double(n - degree) * dt;  // (what paramLocalTraj would have returned with the points)
    TopologyPRM topo;
    topo.setEnvironment(edt);
    topo.init(nh);
    vector<Eigen::Vector3d> colli_start, colli_end, start_pts, end_pts;
    const int status = topo.findCollisionRange(ctrl, dt, degree, colli_start, colli_end, start_pts, end_pts);
    std::printf("range %zu %d %.17g\n", b, status, topo.clearance_);
    put_path("colli_start", b, colli_start), put_path("colli_end", b, colli_end);
    put_path("start_pts", b, start_pts), put_path("end_pts", b, end_pts);
    if (status != FUELMI_COLRANGE_OK) continue;  // no collision, or "Init traj ends in obstacle, no replanning."
    list<GraphNode::Ptr> graph;
    vector<vector<Eigen::Vector3d>> raw, filt, sel;
    topo.findTopoPaths(colli_start.front(), colli_end.back(), start_pts, end_pts, graph, raw, filt, sel);
    std::printf("call %zu %d %d\n", b, topo.last_rc_, topo.last_status_);
    for (size_t i = 0; i < sel.size(); ++i) {
      put_path("sel", b, sel[i]);
      int seg_num = 0, n_ctrl = 0;
      double gdt = 0.0;
      vector<Eigen::Vector3d> guide;
      const int gs = topo.guidePoints(sel[i], duration, ctrl_pt_dist, degree, seg_num, gdt, n_ctrl, guide);
      std::printf("guide_info %zu %d %d %a %d %a\n", b, gs, seg_num, gdt, n_ctrl, duration);
      put_path("guide", b, guide);
    }
  }
  fclose(in);
  return 0;
}
