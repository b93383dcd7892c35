// The reference's FastPlannerManager::findCollisionRange (private: this file is compiled with -fno-access-control) and the
// head of optimizeTopoBspline, driven on a dense-array distance field for tests/golden/make_collide_golden.py.
//   driver <in.txt> <field.bin> <out.txt>
// in.txt: nx ny nz, origin, resolution, then records
//   R degree n_ctrl dt clearance <n_ctrl control points>          findCollisionRange on NonUniformBspline(ctrl, degree, dt)
//   G degree n_path duration ctrl_pt_dist <n_path path points>    planner_manager.cpp:553-577
// out.txt, one line a record, doubles as hexadecimal floats:
//   R: the calls of evaluateCoarseEDT (one a tick), then colli_start, colli_end, start_pts, end_pts, each a count and
//      its points
//   G: seg_num dt n_pts n_ctrl, then the guide points.  Lines 553-577 are no function of their own: pathLength and
//      pathToGuidePts are the real TopologyPRM's, n_pts is the size of the point set the real
//      GlobalTrajData::getTrajInfoInDuration returns for a local trajectory that covers the span, and the integer rules
//      between them are restated here line by line.
// EDTEnvironment::evaluateCoarseEDT, the one map query findCollisionRange makes, is defined here on the dense array (the
// reference's reads SDFMap::getDistance for time < 0); every other symbol of the classes planner_manager.cpp names is
// never called and is left unresolved by the link.  The time inside findCollisionRange goes to stderr.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include <plan_manage/planner_manager.h>

using namespace fast_planner;

static int g_nv[3];
static double g_origin[3], g_res_inv;
static std::vector<double> g_dist;
static long g_calls = 0;

namespace fast_planner {
double EDTEnvironment::evaluateCoarseEDT(Eigen::Vector3d& pos, double time) {
  ++g_calls;
  int id[3];
  for (int i = 0; i < 3; ++i) id[i] = floor((pos(i) - g_origin[i]) * g_res_inv);  // SDFMap::posToIndex
  for (int i = 0; i < 3; ++i)
    if (id[i] < 0 || id[i] > g_nv[i] - 1) return -1;                              // SDFMap::getDistance: !isInMap
  return g_dist[((size_t)id[0] * g_nv[1] + id[1]) * g_nv[2] + id[2]];
}
}  // namespace fast_planner

static void put_pts(FILE* f, const vector<Eigen::Vector3d>& p) {
  std::fprintf(f, " %d", (int)p.size());
  for (const auto& q : p) std::fprintf(f, " %a %a %a", q(0), q(1), q(2));
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  std::ifstream in(argv[1]);
  double res;
  in >> g_nv[0] >> g_nv[1] >> g_nv[2] >> g_origin[0] >> g_origin[1] >> g_origin[2] >> res;
  g_res_inv = 1.0 / res;
  const size_t N = (size_t)g_nv[0] * g_nv[1] * g_nv[2];
  g_dist.resize(N);
  std::ifstream(argv[2], std::ios::binary).read(reinterpret_cast<char*>(g_dist.data()), N * sizeof(double));
  FILE* out = std::fopen(argv[3], "w");
  double secs = 0.0;
  std::string kind;
  while (in >> kind) {
    int degree, n;
    double a, b;
    in >> degree >> n >> a >> b;
    Eigen::MatrixXd pts(n, 3);
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) {
        std::string tok;
        in >> tok;
        pts(i, k) = strtod(tok.c_str(), nullptr);
      }
    if (kind == "R") {
      FastPlannerManager* mgr = new FastPlannerManager;  // (never destroyed: its destructor talks)
      mgr->edt_environment_ = EDTEnvironment::Ptr(static_cast<EDTEnvironment*>(operator new(sizeof(EDTEnvironment))),
                                                   [](EDTEnvironment*) {});  // only evaluateCoarseEDT above is called on it
      mgr->topo_prm_.reset(new TopologyPRM);
      mgr->topo_prm_->clearance_ = b;
      mgr->plan_data_.initial_local_segment_ = NonUniformBspline(pts, degree, a);
      vector<Eigen::Vector3d> cs, ce, sp, ep;
      g_calls = 0;
      const auto t0 = std::chrono::steady_clock::now();
      mgr->findCollisionRange(cs, ce, sp, ep);
      secs += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      std::fprintf(out, "R %ld", g_calls);
      put_pts(out, cs), put_pts(out, ce), put_pts(out, sp), put_pts(out, ep);
      std::fprintf(out, "\n");
    } else {
      const double duration = a, ctrl_pt_dist = b;
      vector<Eigen::Vector3d> guide_path(n);
      for (int i = 0; i < n; ++i) guide_path[i] = Eigen::Vector3d(pts(i, 0), pts(i, 1), pts(i, 2));
      TopologyPRM topo;
      int seg_num = topo.pathLength(guide_path) / ctrl_pt_dist;  // :554
      seg_num = max(6, seg_num);                                  // :555
      double dt = duration / double(seg_num);                     // :556
      // reparamLocalTraj (:619-634): the point set of getTrajInfoInDuration; parameterizeToBspline returns K + 2 rows
      GlobalTrajData gd;
      Eigen::MatrixXd line(8, 3);
      for (int i = 0; i < 8; ++i) line(i, 0) = 0.1 * i, line(i, 1) = 0.0, line(i, 2) = 0.0;
      gd.global_duration_ = 0.0, gd.time_change_ = 0.0, gd.last_time_inc_ = 0.0;
      gd.setLocalTraj(NonUniformBspline(line, 3, 1.0), -1.0, 1e300, 0.0);  // every getState goes to the local trajectory
      vector<Eigen::Vector3d> point_set, derivs;
      gd.getTrajInfoInDuration(0.0, duration, dt, point_set, derivs);
      const int rows = (int)point_set.size() + 2;
      vector<Eigen::Vector3d> tmp_pts, guide_pts;
      if (degree == 3 || degree == 5) {                           // :567-577
        topo.pathToGuidePts(guide_path, rows - 2, tmp_pts);
        guide_pts.insert(guide_pts.end(), tmp_pts.begin() + 2, tmp_pts.end() - 2);
      } else if (degree == 4) {
        topo.pathToGuidePts(guide_path, 2 * rows - 7, tmp_pts);
        for (int i = 0; i < tmp_pts.size(); ++i)
          if (i % 2 == 1 && i >= 5 && i <= tmp_pts.size() - 6) guide_pts.push_back(tmp_pts[i]);
      }
      std::fprintf(out, "G %d %a %d %d", seg_num, dt, (int)point_set.size(), rows);
      put_pts(out, guide_pts);
      std::fprintf(out, "\n");
    }
  }
  std::fclose(out);
  std::fprintf(stderr, "findCollisionRange seconds %.6f\n", secs);
  return 0;
}
