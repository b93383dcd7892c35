// The reference's KinodynamicAstar driven as FastPlannerManager::kinodynamicReplan drives it (reset, search with
// init = true, after NO_PATH reset and search with init = false, getSamples), on a dense-array map.
//   driver <in.txt> <infl.bin> <unk.bin> <out.txt>
// in.txt: nx ny nz, origin, size, box min, box max, map resolution, the search/* parameters, ts, n, then per problem
// start, start_vel, start_acc, goal, goal_vel.  out.txt: one record per problem, doubles as hexadecimal floats.
#define private public
#include <path_searching/kinodynamic_astar.h>
#undef private
#include <plan_env/sdf_map.h>

#include <cstdio>
#include <fstream>

using namespace fast_planner;

static void put(FILE* f, double v) { std::fprintf(f, " %a", v); }

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  std::ifstream in(argv[1]);
  auto map = std::make_shared<SDFMap>();
  in >> map->nv[0] >> map->nv[1] >> map->nv[2];
  for (int i = 0; i < 3; ++i) in >> map->origin[i];
  for (int i = 0; i < 3; ++i) in >> map->size[i];
  for (int i = 0; i < 3; ++i) in >> map->box_mind[i];
  for (int i = 0; i < 3; ++i) in >> map->box_maxd[i];
  double res;
  in >> res;
  map->res_inv = 1.0 / res;
  const size_t N = (size_t)map->nv[0] * map->nv[1] * map->nv[2];
  map->infl.resize(N);
  map->unk.resize(N);
  std::ifstream(argv[2], std::ios::binary).read(reinterpret_cast<char*>(map->infl.data()), N);
  std::ifstream(argv[3], std::ios::binary).read(reinterpret_cast<char*>(map->unk.data()), N);
  ros::NodeHandle nh;
  const char* names[] = {"search/max_tau", "search/init_max_tau", "search/max_vel", "search/max_acc", "search/w_time",
                         "search/horizon", "search/resolution_astar", "search/lambda_heu", "search/allocate_num",
                         "search/check_num", "search/optimistic"};
  for (const char* k : names) in >> nh.num[k];
  nh.num["search/time_resolution"] = 0.8;
  double ts0;
  int n;
  in >> ts0 >> n;
  auto env = std::make_shared<EDTEnvironment>();
  env->sdf_map_ = map;
  KinodynamicAstar kino;
  kino.setParam(nh);
  kino.setEnvironment(env);
  kino.init();
  FILE* out = std::fopen(argv[4], "w");
  for (int b = 0; b < n; ++b) {
    Eigen::Vector3d p[5];
    for (auto& v : p)
      for (int i = 0; i < 3; ++i) in >> v[i];
    kino.reset();
    int which = 0;
    int status = kino.search(p[0], p[1], p[2], p[3], p[4], true);
    if (status == KinodynamicAstar::NO_PATH) {
      kino.reset();
      which = 1;
      status = kino.search(p[0], p[1], p[2], p[3], p[4], false);
    }
    std::fprintf(out, "%d %d %d %d", status, which, kino.iter_num_, kino.use_node_num_);
    if (status == KinodynamicAstar::NO_PATH) {
      std::fprintf(out, "\n");
      continue;
    }
    std::fprintf(out, " %d", (int)kino.path_nodes_.size());
    for (PathNodePtr q : kino.path_nodes_) {
      std::fprintf(out, " %d %d %d", q->index(0), q->index(1), q->index(2));
      for (int i = 0; i < 6; ++i) put(out, q->state(i));
      const bool first = q->parent == NULL;  // input and duration of the start node are never written
      for (int i = 0; i < 3; ++i) put(out, first ? 0.0 : q->input(i));
      put(out, first ? 0.0 : q->duration);
    }
    std::fprintf(out, " %d", kino.is_shot_succ_ ? 1 : 0);
    put(out, kino.is_shot_succ_ ? kino.t_shot_ : 0.0);
    for (int d = 0; d < 3; ++d)
      for (int j = 0; j < 4; ++j) put(out, kino.is_shot_succ_ ? kino.coef_shot_(d, j) : 0.0);
    double ts = ts0;
    std::vector<Eigen::Vector3d> pts, der;
    kino.getSamples(ts, pts, der);
    put(out, ts);
    std::fprintf(out, " %d", (int)pts.size());
    for (auto& v : pts)
      for (int i = 0; i < 3; ++i) put(out, v[i]);
    for (auto& v : der)
      for (int i = 0; i < 3; ++i) put(out, v[i]);
    std::fprintf(out, "\n");
  }
  std::fclose(out);
  return 0;
}
