// The reference's HeadingPlanner (active_perception/src/heading_planner.cpp with plan_env/src/raycast.cpp, both
// unmodified) on a dense-array map (plan_env/sdf_map.h beside this file).  Built with -fno-access-control: the driver
// calls the private calcInformationGain / initCastFlag and sets the parameters the constructor read from the node handle.
//   driver <in.txt> <state.bin> <out.txt>
// in.txt: nx ny nz, origin, resolution, the exploration box (min, max), then records
//   G weight in_box far lambda1 lambda2  pos  n_yaw yaws  n_ctrl ctrl
//       -> per yaw the gain; the UNIFORM gain (= the visible cells); the UNIFORM gain with every occupied voxel made free
//          (= the candidates: an occupied voxel is known either way)
//   P h yaw_diff max_yaw_rate w weight far lambda1 lambda2 given  L dt pts yaws  n_ctrl ctrl  [gains L x (2h + 1)]
//       -> the gains per vertex (calcInformationGain behind initCastFlag, as :188-199 call it, or the given ones), then
//          the reference's Graph built as :179-223 build it and searched: g_value_ per vertex, the path's ids and yaws;
//          without given gains also what searchPathOfYaw itself returned
// far_ is a constant of the constructor (4.5); for another far the driver rebuilds the four vertices with the
// constructor's own expressions (:136-139).  out.txt: one line per record, doubles as hexadecimal floats.  The time of
// searchPathOfYaw goes to stderr.
#include <chrono>
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include <active_perception/heading_planner.h>
#include <plan_env/raycast.h>
#include <plan_env/sdf_map.h>

using namespace fast_planner;

static void put(FILE* f, double v) { std::fprintf(f, " %a", v); }

static void set_far(HeadingPlanner& hp, double far) {
  if (far == 4.5) return;  // the constructor's own vertices
  const double top_ang = 0.56125, left_ang = 0.69222, right_ang = 0.68901;
  hp.far_ = far;
  hp.lefttop_ << -hp.far_ * tan(left_ang), -hp.far_ * sin(top_ang), hp.far_;
  hp.leftbottom_ << -hp.far_ * sin(left_ang), hp.far_ * sin(top_ang), hp.far_;
  hp.righttop_ << hp.far_ * sin(right_ang), -hp.far_ * sin(top_ang), hp.far_;
  hp.rightbottom_ << hp.far_ * sin(right_ang), hp.far_ * sin(top_ang), hp.far_;
}

static Eigen::MatrixXd read_ctrl(std::ifstream& in) {
  int n;
  in >> n;
  Eigen::MatrixXd c(n, 3);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) in >> c(i, k);
  return c;
}

static double gain_of(HeadingPlanner& hp, int in_box, const Eigen::Vector3d& pt, double yaw, const Eigen::MatrixXd& ctrl) {
  return in_box ? hp.calcInformationGain(pt, yaw, ctrl, 0) : hp.calcInfoGain(pt, yaw, 0);
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  std::ifstream in(argv[1]);
  auto map = std::make_shared<SDFMap>();
  in >> map->nv[0] >> map->nv[1] >> map->nv[2];
  for (int i = 0; i < 3; ++i) in >> map->origin[i];
  in >> map->res;
  map->res_inv = 1.0 / map->res;
  for (int i = 0; i < 3; ++i) in >> map->box_mind[i];
  for (int i = 0; i < 3; ++i) in >> map->box_maxd[i];
  {
    Eigen::Vector3i a, b;
    map->posToIndex(Eigen::Vector3d(map->box_mind[0], map->box_mind[1], map->box_mind[2]), a);
    map->posToIndex(Eigen::Vector3d(map->box_maxd[0], map->box_maxd[1], map->box_maxd[2]), b);
    for (int i = 0; i < 3; ++i) map->box_min[i] = a(i), map->box_max[i] = b(i);
  }
  const size_t N = (size_t)map->nv[0] * map->nv[1] * map->nv[2];
  map->state.resize(N);
  std::ifstream(argv[2], std::ios::binary).read(reinterpret_cast<char*>(map->state.data()), N);
  const std::vector<signed char> state = map->state;
  std::vector<signed char> freed = state;
  for (auto& s : freed)
    if (s == SDFMap::OCCUPIED) s = SDFMap::FREE;
  FILE* out = std::fopen(argv[3], "w");
  double seconds = 0.0;
  int timed = 0;
  std::string kind;
  while (in >> kind) {
    ros::NodeHandle nh;
    if (kind == "G") {
      int weight, in_box, n_yaw;
      double far, l1, l2;
      Eigen::Vector3d pt;
      in >> weight >> in_box >> far >> l1 >> l2 >> pt(0) >> pt(1) >> pt(2) >> n_yaw;
      std::vector<double> yaws(n_yaw);
      for (double& y : yaws) in >> y;
      const Eigen::MatrixXd ctrl = read_ctrl(in);
      nh.num["heading_planner/half_vert_num"] = 0;
      HeadingPlanner hp(nh);
      hp.setMap(map);
      set_far(hp, far);
      hp.lambda1_ = l1, hp.lambda2_ = l2;
      std::fprintf(out, "G %d", n_yaw);
      for (int pass = 0; pass < 3; ++pass) {  // the scene's weights; UNIFORM; UNIFORM without obstacles
        hp.weight_type_ = pass == 0 ? weight : 1;
        map->state = pass == 2 ? freed : state;
        if (in_box) hp.initCastFlag(pt);  // (:188: once per way-point, in front of its yaws)
        for (double y : yaws) put(out, gain_of(hp, in_box, pt, y, ctrl));
      }
      map->state = state;
      std::fprintf(out, "\n");
    } else {
      int h, weight, given, L;
      double yaw_diff, rate, w, far, l1, l2, dt;
      in >> h >> yaw_diff >> rate >> w >> weight >> far >> l1 >> l2 >> given >> L >> dt;
      std::vector<Eigen::Vector3d> pts(L);
      std::vector<double> yaws(L);
      for (auto& p : pts) in >> p(0) >> p(1) >> p(2);
      for (double& y : yaws) in >> y;
      const Eigen::MatrixXd ctrl = read_ctrl(in);
      const int nv = 2 * h + 1;
      std::vector<double> gains((size_t)L * nv, 0.0);
      if (given)
        for (double& g : gains) in >> g;
      nh.num["heading_planner/half_vert_num"] = h, nh.num["heading_planner/yaw_diff"] = yaw_diff;
      nh.num["heading_planner/max_yaw_rate"] = rate, nh.num["heading_planner/w"] = w;
      nh.num["heading_planner/weight_type"] = weight;
      nh.num["heading_planner/lambda1"] = l1, nh.num["heading_planner/lambda2"] = l2;
      HeadingPlanner hp(nh);
      hp.setMap(map);
      set_far(hp, far);
      for (int i = 1; !given && i < L - 1; ++i) {
        hp.initCastFlag(pts[i]);
        for (int j = 0; j < nv; ++j)
          gains[(size_t)i * nv + j] = hp.calcInformationGain(pts[i], yaws[i] + double(j - h) * yaw_diff, ctrl, 0);
      }
      // the graph as :179-223 build it
      Graph graph;
      graph.setParams(w, rate, dt);
      int gid = 0;
      std::vector<YawVertex::Ptr> layer, last_layer, all;
      for (int i = 0; i < L; ++i) {
        if (i == 0 || i == L - 1) {
          YawVertex::Ptr vert(new YawVertex(yaws[i], 0, gid++));
          graph.addVertex(vert), layer.push_back(vert), all.push_back(vert);
        } else {
          for (int j = 0; j < nv; ++j) {
            YawVertex::Ptr vert(new YawVertex(yaws[i] + double(j - h) * yaw_diff, gains[(size_t)i * nv + j], gid++));
            graph.addVertex(vert), layer.push_back(vert), all.push_back(vert);
          }
        }
        for (auto v1 : last_layer)
          for (auto v2 : layer) graph.addEdge(v1->id_, v2->id_);
        last_layer.clear();
        last_layer.swap(layer);
      }
      std::vector<YawVertex::Ptr> vert_path;
      graph.dijkstraSearch(0, gid - 1, vert_path);
      std::fprintf(out, "P %d %d", L, nv);
      for (double g : gains) put(out, g);
      std::fprintf(out, " %d", gid);
      for (auto& v : all) put(out, v->g_value_);  // (the start's is 0; every other vertex was labelled before the goal was popped)
      std::fprintf(out, " %d", (int)vert_path.size());
      for (auto& v : vert_path) std::fprintf(out, " %d", v->id_);
      for (auto& v : vert_path) put(out, v->yaw_);
      std::vector<double> path;
      if (!given) {
        const auto t0 = std::chrono::steady_clock::now();
        hp.searchPathOfYaw(pts, yaws, dt, ctrl, path);
        seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        ++timed;
      }
      std::fprintf(out, " %d", (int)path.size());
      for (double y : path) put(out, y);
      std::fprintf(out, "\n");
    }
  }
  std::fclose(out);
  std::fprintf(stderr, "searchPathOfYaw seconds %.6f problems %d\n", seconds, timed);
  return 0;
}
