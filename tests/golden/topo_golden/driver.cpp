// The reference's TopologyPRM driven as FastPlannerManager::topoReplan drives it (findTopoPaths), on a dense-array
// distance field, with eng_ seeded and max_sample_time huge: the sample loop runs max_sample_num times.
//   driver <in.txt> <field.bin> <out.txt>
// in.txt: nx ny nz, origin, resolution, sample_inflate x y z, clearance, ratio_to_short, max_sample_num, max_raw_path,
// max_raw_path2, reserve_num, the seed, n, then per problem start, end, n_start, start_pts, n_end, end_pts.
// out.txt: first the sample stream (the 3 max_sample_num numbers rand_pos_(eng_) returns after the seeding), then one
// record per problem; doubles as hexadecimal floats.  The time of the findTopoPaths calls goes to stderr.
#include <chrono>
#include <cstdio>
#include <fstream>
#include <list>
#include <memory>
#include <random>
#include <vector>
#define private public
#include <path_searching/topo_prm.h>
#undef private

using namespace fast_planner;

static void put(FILE* f, double v) { std::fprintf(f, " %a", v); }
static void put_paths(FILE* f, const vector<vector<Eigen::Vector3d>>& paths) {
  std::fprintf(f, " %d", (int)paths.size());
  for (const auto& p : paths) {
    std::fprintf(f, " %d", (int)p.size());
    for (const auto& q : p)
      for (int i = 0; i < 3; ++i) put(f, q(i));
  }
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  std::ifstream in(argv[1]);
  auto map = std::make_shared<SDFMap>();
  in >> map->nv[0] >> map->nv[1] >> map->nv[2];
  for (int i = 0; i < 3; ++i) in >> map->origin[i];
  in >> map->res;
  map->res_inv = 1.0 / map->res;
  const size_t N = (size_t)map->nv[0] * map->nv[1] * map->nv[2];
  map->dist.resize(N);
  std::ifstream(argv[2], std::ios::binary).read(reinterpret_cast<char*>(map->dist.data()), N * sizeof(double));
  ros::NodeHandle nh;
  const char* names[] = {"topo_prm/sample_inflate_x", "topo_prm/sample_inflate_y", "topo_prm/sample_inflate_z",
                         "topo_prm/clearance", "topo_prm/ratio_to_short", "topo_prm/max_sample_num",
                         "topo_prm/max_raw_path", "topo_prm/max_raw_path2", "topo_prm/reserve_num"};
  for (const char* k : names) in >> nh.num[k];
  nh.num["topo_prm/max_sample_time"] = 1e9;
  nh.num["topo_prm/short_cut_num"] = 1;
  nh.num["topo_prm/parallel_shortcut"] = 0;
  unsigned seed;
  int n;
  in >> seed >> n;
  auto env = std::make_shared<EDTEnvironment>();
  env->sdf_map_ = map;
  TopologyPRM topo;
  topo.setEnvironment(env);
  topo.init(nh);
  FILE* out = std::fopen(argv[3], "w");
  {
    std::default_random_engine eng(seed);
    const int count = 3 * (int)nh.num["topo_prm/max_sample_num"];
    std::fprintf(out, "%d", count);
    for (int i = 0; i < count; ++i) put(out, topo.rand_pos_(eng));
    std::fprintf(out, "\n");
  }
  double seconds = 0.0;
  for (int b = 0; b < n; ++b) {
    Eigen::Vector3d start, end;
    for (int i = 0; i < 3; ++i) in >> start(i);
    for (int i = 0; i < 3; ++i) in >> end(i);
    vector<Eigen::Vector3d> sp, ep;
    int k;
    in >> k;
    sp.resize(k);
    for (auto& v : sp)
      for (int i = 0; i < 3; ++i) in >> v(i);
    in >> k;
    ep.resize(k);
    for (auto& v : ep)
      for (int i = 0; i < 3; ++i) in >> v(i);
    topo.eng_ = std::default_random_engine(seed);
    list<GraphNode::Ptr> graph;
    vector<vector<Eigen::Vector3d>> raw, filt, sel;
    const auto t0 = std::chrono::steady_clock::now();
    topo.findTopoPaths(start, end, sp, ep, graph, raw, filt, sel);
    seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(out, "%d", (int)graph.size());
    for (const auto& g : graph) {
      std::fprintf(out, " %d %d", g->id_, (int)g->type_);
      for (int i = 0; i < 3; ++i) put(out, g->pos_(i));
      std::fprintf(out, " %d", (int)g->neighbors_.size());
      for (const auto& q : g->neighbors_) std::fprintf(out, " %d", q->id_);
    }
    put_paths(out, raw);
    put_paths(out, filt);
    put_paths(out, sel);
    for (auto& p : sel) put(out, topo.pathLength(p));
    std::fprintf(out, "\n");
  }
  std::fclose(out);
  std::fprintf(stderr, "findTopoPaths seconds %.6f problems %d\n", seconds, n);
  return 0;
}
