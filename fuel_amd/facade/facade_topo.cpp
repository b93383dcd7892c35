// facade_topo.cpp -- drives TopologyPRM the way FastPlannerManager::topoReplan does (plan_manage/src/planner_manager.cpp:431,
// 554, 568): findTopoPaths, then pathLength and pathToGuidePts of every select path.  Prints what
// tests/test_topo_facade_gpu.py compares with fuelmi_map_topo_paths on the same map and sample stream: the graph, the
// three path sets, the lengths and the guide points; doubles as hexadecimal floats.
//   facade_topo <scenario.bin>
// scenario.bin: double map_size[3]; sample_inflate[3], clearance, ratio_to_short, max_sample_num, max_raw_path,
// max_raw_path2, reserve_num, seed, guide points per path; one occupancy log-odds grid (f64, the map's voxel count); then
// any number of problems, double start[3], end[3] each.  Every problem is searched with the engine seeded anew.
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
  double hdr[15];
  rd(in, hdr, 15);
  ros::NodeHandle nh;
  auto& P = nh.num;
  double box_lo[3], box_hi[3];
  whole_map_box(hdr, -1.0, box_lo, box_hi);
  sdf_map_params(nh, hdr, box_lo, box_hi);
  P["topo_prm/sample_inflate_x"] = hdr[3], P["topo_prm/sample_inflate_y"] = hdr[4], P["topo_prm/sample_inflate_z"] = hdr[5];
  P["topo_prm/clearance"] = hdr[6], P["topo_prm/ratio_to_short"] = hdr[7], P["topo_prm/max_sample_num"] = hdr[8];
  P["topo_prm/max_raw_path"] = hdr[9], P["topo_prm/max_raw_path2"] = hdr[10], P["topo_prm/reserve_num"] = hdr[11];
  P["topo_prm/seed"] = hdr[12];
  const int guide_num = (int)hdr[13];  // (hdr[14]: spare)
  const DriverMap dm = make_map(nh, false);
  const EDTEnvironment::Ptr& edt = dm.edt;
  load_occupancy(*dm.map, in, LOAD_BOUND | LOAD_INFLATE_ABI | LOAD_ESDF);
  const std::vector<double> pr = read_records(in, 6);
  fclose(in);
  for (size_t b = 0; b < pr.size() / 6; ++b) {
    const double* q = pr.data() + 6 * b;
    TopologyPRM topo;
    topo.setEnvironment(edt);
    topo.init(nh);
    list<GraphNode::Ptr> graph;
    vector<vector<Eigen::Vector3d>> raw, filt, sel;
    topo.findTopoPaths(Eigen::Vector3d(q[0], q[1], q[2]), Eigen::Vector3d(q[3], q[4], q[5]), {}, {}, graph, raw, filt, sel);
    std::printf("call %zu %d %d %.17g\n", b, topo.last_rc_, topo.last_status_, topo.clearance_);
    for (const auto& g : graph) {
      std::printf("node %zu %d %d %a %a %a %zu", b, g->id_, (int)g->type_, g->pos_(0), g->pos_(1), g->pos_(2),
                  g->neighbors_.size());
      for (const auto& n : g->neighbors_) std::printf(" %d", n->id_);
      std::printf("\n");
    }
    for (const auto& p : raw) put_path("raw", b, p);
    for (const auto& p : filt) put_path("filt", b, p);
    for (auto& p : sel) {
      put_path("sel", b, p);
      std::printf("length %zu %a\n", b, topo.pathLength(p));
      vector<Eigen::Vector3d> pts;
      topo.pathToGuidePts(p, guide_num, pts);
      put_path("guide", b, pts);
    }
  }
  return 0;
}
