// facade_topo.cpp -- drives TopologyPRM the way FastPlannerManager::topoReplan does (plan_manage/src/planner_manager.cpp:431,
// 554, 568): findTopoPaths, then pathLength and pathToGuidePts of every select path.  Prints what
// tests/test_topo_facade_gpu.py compares with fuelmi_map_topo_paths on the same map and sample stream: the graph, the
// three path sets, the lengths and the guide points; doubles as hexadecimal floats.
//   facade_topo <scenario.bin>
// scenario.bin: double map_size[3]; sample_inflate[3], clearance, ratio_to_short, max_sample_num, max_raw_path,
// max_raw_path2, reserve_num, seed, guide points per path; one occupancy log-odds grid (f64, the map's voxel count); then
// any number of problems, double start[3], end[3] each.  Every problem is searched with the engine seeded anew.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <plan_env/sdf_map.h>
#include <plan_env/edt_environment.h>
#include <active_perception/graph_node.h>
#include <active_perception/perception_utils.h>
#include <path_searching/topo_prm.h>

namespace fast_planner {
// the facade library's open ends, defined by the packages of a FUEL workspace; unused here
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
  if (fread(hdr, sizeof(double), 15, in) != 15) return 2;
  ros::NodeHandle nh;
  auto& P = nh.num;
  P["sdf_map/resolution"] = 0.1;
  P["sdf_map/map_size_x"] = hdr[0], P["sdf_map/map_size_y"] = hdr[1], P["sdf_map/map_size_z"] = hdr[2];
  P["sdf_map/obstacles_inflation"] = 0.199, P["sdf_map/local_bound_inflate"] = 0.5, P["sdf_map/ground_height"] = -1.0;
  P["sdf_map/default_dist"] = 0.0, P["sdf_map/optimistic"] = 0, P["sdf_map/signed_dist"] = 0;
  P["sdf_map/p_hit"] = 0.65, P["sdf_map/p_miss"] = 0.35, P["sdf_map/p_min"] = 0.12, P["sdf_map/p_max"] = 0.90;
  P["sdf_map/p_occ"] = 0.80, P["sdf_map/max_ray_length"] = 4.5, P["sdf_map/virtual_ceil_height"] = -10;
  const char* ax[3] = {"x", "y", "z"};
  const double ground = -1.0;
  for (int i = 0; i < 3; ++i) {
    const double lo = i < 2 ? -hdr[i] / 2.0 : ground;
    P[std::string("sdf_map/box_min_") + ax[i]] = lo;
    P[std::string("sdf_map/box_max_") + ax[i]] = lo + hdr[i];
  }
  P["topo_prm/sample_inflate_x"] = hdr[3], P["topo_prm/sample_inflate_y"] = hdr[4], P["topo_prm/sample_inflate_z"] = hdr[5];
  P["topo_prm/clearance"] = hdr[6], P["topo_prm/ratio_to_short"] = hdr[7], P["topo_prm/max_sample_num"] = hdr[8];
  P["topo_prm/max_raw_path"] = hdr[9], P["topo_prm/max_raw_path2"] = hdr[10], P["topo_prm/reserve_num"] = hdr[11];
  P["topo_prm/seed"] = hdr[12];
  const int guide_num = (int)hdr[13];  // (hdr[14]: spare)
  SDFMap::Ptr map(new SDFMap);
  map->initMap(nh);
  EDTEnvironment::Ptr edt(new EDTEnvironment);
  edt->setMap(map);
  fuelmi_map* m = map->device();
  fuelmi_map_info info;
  fuelmi_map_get_info(m, &info);
  const int N = info.voxel_num[0] * info.voxel_num[1] * info.voxel_num[2];
  std::vector<double> occ(N);
  if (fread(occ.data(), sizeof(double), N, in) != (size_t)N) return 2;
  const int b0[3] = {0, 0, 0};
  const int b1[3] = {info.voxel_num[0] - 1, info.voxel_num[1] - 1, info.voxel_num[2] - 1};
  if (fuelmi_map_upload_occupancy(m, occ.data()) || fuelmi_map_set_local_bound(m, b0, b1)) return 3;
  if (fuelmi_map_inflate_local(m)) return 3;
  map->updateESDF3d();
  std::vector<double> pr;
  double rec[6];
  while (fread(rec, sizeof(double), 6, in) == 6) pr.insert(pr.end(), rec, rec + 6);
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
