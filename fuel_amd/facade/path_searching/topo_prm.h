// path_searching/topo_prm.h -- drop-in for the reference header of the same name
// (fuel_planner/path_searching/include/path_searching/topo_prm.h): the public names FastPlannerManager uses
// (plan_manage/src/planner_manager.cpp:77-79, 431, 554, 568, 648).  findTopoPaths runs on the device
// (fuelmi_map_topo_paths, one problem); the class draws the sample stream the kernel consumes from its own
// default_random_engine, seeded from random_device like the reference's, or from topo_prm/seed when that is >= 0.
// Dropped: topo_prm/max_sample_time (exactly max_sample_num samples are taken), short_cut_num (read and never used by the
// reference) and parallel_shortcut (threading only).  pathLength and pathToGuidePts are host loops.
// Added for the rest of topoReplan's chain, both on the device: findCollisionRange (the reference keeps it private in
// FastPlannerManager, :636-691, where it reads the host's distance buffer; here it takes the local segment's control
// points and needs no ESDF mirror) and guidePoints (the head of optimizeTopoBspline, :553-577).
#ifndef _TOPO_PRM_H
#define _TOPO_PRM_H

#include <plan_env/edt_environment.h>
#include <plan_env/sdf_map.h>

#include <cmath>
#include <random>

namespace fast_planner {
/* ---------- node of topo graph ---------- */
class GraphNode {
public:
  enum NODE_TYPE { Guard = 1, Connector = 2 };
  enum NODE_STATE { NEW = 1, CLOSE = 2, OPEN = 3 };

  GraphNode() {}
  GraphNode(Eigen::Vector3d pos, NODE_TYPE type, int id) : pos_(pos), type_(type), state_(NEW), id_(id) {}

  vector<shared_ptr<GraphNode>> neighbors_;
  Eigen::Vector3d pos_;
  NODE_TYPE type_;
  NODE_STATE state_;
  int id_;

  typedef shared_ptr<GraphNode> Ptr;
};

class TopologyPRM {
public:
  double clearance_;
  // of the last findTopoPaths: the call's return value, the problem's status (FUELMI_TOPO_*, -1: over a cap), the counts
  // (raw paths found, kept, filtered, selected) and the event counters of fuelmi_map_topo_paths
  int last_rc_ = 0, last_status_ = 0, last_counts_[4] = {0, 0, 0, 0}, last_events_[6] = {0, 0, 0, 0, 0, 0};

  TopologyPRM() {}
  ~TopologyPRM() {}

  void init(ros::NodeHandle& nh) {
    rand_pos_ = std::uniform_real_distribution<double>(-1.0, 1.0);
    nh.param("topo_prm/sample_inflate_x", cfg_.sample_inflate[0], -1.0);
    nh.param("topo_prm/sample_inflate_y", cfg_.sample_inflate[1], -1.0);
    nh.param("topo_prm/sample_inflate_z", cfg_.sample_inflate[2], -1.0);
    nh.param("topo_prm/clearance", clearance_, -1.0);
    nh.param("topo_prm/reserve_num", cfg_.reserve_num, -1);
    nh.param("topo_prm/ratio_to_short", cfg_.ratio_to_short, -1.0);
    nh.param("topo_prm/max_sample_num", cfg_.max_sample_num, -1);
    nh.param("topo_prm/max_raw_path", cfg_.max_raw_path, 1);
    nh.param("topo_prm/max_raw_path2", cfg_.max_raw_path2, -1);
    int seed = -1;
    nh.param("topo_prm/seed", seed, -1);
    eng_ = std::default_random_engine(seed >= 0 ? (unsigned)seed : rd_());
  }

  void setEnvironment(const EDTEnvironment::Ptr& env) { edt_environment_ = env; }

  // The four sets as the reference returns them (filtered_paths: what selectShortPaths left of it).  A call the library
  // refuses, or a problem whose status is UNDEFINED or -1, leaves them empty (last_rc_ / last_status_ say which).
  void findTopoPaths(Eigen::Vector3d start, Eigen::Vector3d end, vector<Eigen::Vector3d> start_pts,
                     vector<Eigen::Vector3d> end_pts, list<GraphNode::Ptr>& graph,
                     vector<vector<Eigen::Vector3d>>& raw_paths, vector<vector<Eigen::Vector3d>>& filtered_paths,
                     vector<vector<Eigen::Vector3d>>& select_paths) {
    graph.clear(), raw_paths.clear(), filtered_paths.clear(), select_paths.clear();
    fuelmi_topo_cfg c = cfg_;
    c.clearance = clearance_;
    c.max_nodes = c.max_sample_num + 2;
    c.max_path_points = FUELMI_TOPO_MAX_PATH_POINTS;
    const int S = c.max_sample_num > 0 ? c.max_sample_num : 0;
    vector<double> smp(3 * (size_t)S + 1);
    for (int i = 0; i < 3 * S; ++i) smp[i] = rand_pos_(eng_);
    const int ns = (int)start_pts.size(), ne = (int)end_pts.size();
    vector<double> sp(3 * (size_t)ns + 1), ep(3 * (size_t)ne + 1);
    for (int i = 0; i < ns; ++i)
      for (int k = 0; k < 3; ++k) sp[3 * i + k] = start_pts[i](k);
    for (int i = 0; i < ne; ++i)
      for (int k = 0; k < 3; ++k) ep[3 * i + k] = end_pts[i](k);
    const double s3[3] = {start(0), start(1), start(2)}, e3[3] = {end(0), end(1), end(2)};
    const size_t maxn = c.max_nodes > 0 ? c.max_nodes : 0, mpp = c.max_path_points, r2 = c.max_raw_path2 > 0 ? c.max_raw_path2 : 0,
                 rs = c.reserve_num > 0 ? c.reserve_num : 0;
    int n_nodes = 0;
    vector<int> node_id(maxn + 1), node_type(maxn + 1), nb_off(maxn + 2), nb_ids(4 * maxn + 1);
    vector<double> node_xyz(3 * maxn + 1), raw(r2 * mpp * 3 + 1), filt(r2 * mpp * 3 + 1), sel(rs * mpp * 3 + 1), sel_length(rs + 1);
    vector<int> raw_len(r2 + 1), filt_len(r2 + 1), sel_len(rs + 1);
    last_status_ = 0;
    last_rc_ = fuelmi_map_topo_paths(edt_environment_->sdf_map_->device(), &c, 1, s3, e3, ns, &ns, sp.data(), ne, &ne, ep.data(),
                                     smp.data(), &last_status_, last_counts_, last_events_, &n_nodes, node_id.data(),
                                     node_type.data(), node_xyz.data(), nb_off.data(), nb_ids.data(), raw.data(),
                                     raw_len.data(), filt.data(), filt_len.data(), sel.data(), sel_len.data(),
                                     sel_length.data());
    if (last_rc_ != FUELMI_OK) {
      ROS_ERROR("[Topo]: fuelmi_map_topo_paths: %s", fuelmi_last_error());
      return;
    }
    if (last_status_ != FUELMI_TOPO_OK && last_status_ != FUELMI_TOPO_NO_PATH) return;
    // the graph: nodes in list order, neighbours by id in push_back order
    vector<GraphNode::Ptr> by_id(maxn);
    for (int i = 0; i < n_nodes; ++i) {
      GraphNode::Ptr g(new GraphNode(Eigen::Vector3d(node_xyz[3 * i], node_xyz[3 * i + 1], node_xyz[3 * i + 2]),
                                     (GraphNode::NODE_TYPE)node_type[i], node_id[i]));
      by_id[node_id[i]] = g;
      graph.push_back(g);
    }
    int at = 0;
    for (auto& g : graph) {
      for (int k = nb_off[at]; k < nb_off[at + 1]; ++k) g->neighbors_.push_back(by_id[nb_ids[k]]);
      ++at;
    }
    auto take = [mpp](const vector<double>& pts, const vector<int>& lens, size_t rows, vector<vector<Eigen::Vector3d>>& out) {
      for (size_t r = 0; r < rows && lens[r] > 0; ++r) {
        vector<Eigen::Vector3d> p(lens[r]);
        for (int i = 0; i < lens[r]; ++i)
          p[i] = Eigen::Vector3d(pts[(r * mpp + i) * 3], pts[(r * mpp + i) * 3 + 1], pts[(r * mpp + i) * 3 + 2]);
        out.push_back(p);
      }
    };
    take(raw, raw_len, r2, raw_paths);
    take(filt, filt_len, r2, filtered_paths);
    take(sel, sel_len, rs, select_paths);
  }

  // FastPlannerManager::findCollisionRange for the uniform position spline (ctrl_pts [n][3], knot span dt) against the
  // device's distance field with clearance_ (fuelmi_map_collision_ranges, one problem).  Returns the problem's status:
  // FUELMI_COLRANGE_OK (the four vectors as the reference fills them), _NO_COLLISION (all empty), _ENDS_IN_OBSTACLE
  // (colli_start has its one point), _NONFINITE, -1 over a cap (the vectors hold what fitted), or, where the library
  // refuses the call, its negative return value (fuelmi_last_error() says why; the vectors are empty).
  int findCollisionRange(const Eigen::MatrixXd& ctrl_pts, double dt, int degree, vector<Eigen::Vector3d>& colli_start,
                         vector<Eigen::Vector3d>& colli_end, vector<Eigen::Vector3d>& start_pts,
                         vector<Eigen::Vector3d>& end_pts) {
    colli_start.clear(), colli_end.clear(), start_pts.clear(), end_pts.clear();
    const int n = (int)ctrl_pts.rows();
    fuelmi_colrange_cfg c;
    c.degree = degree, c.max_ctrl = n > degree + 1 ? n : degree + 1, c.max_events = 64, c.max_pts = FUELMI_TOPO_MAX_POINTS_IN;
    c.clearance = clearance_;
    vector<double> pos(3 * (size_t)c.max_ctrl);
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) pos[3 * i + k] = ctrl_pts(i, k);
    const size_t ev = c.max_events, mp = c.max_pts;
    vector<double> cs(3 * ev), ce(3 * ev), sp(3 * mp), ep(3 * mp);
    int status = 0, n_ticks = 0, n_se = 0, n_ee = 0, n_sp = 0, n_ep = 0;
    double t_s = 0.0, t_e = 0.0, first[3], last[3];
    const int rc = fuelmi_map_collision_ranges(edt_environment_->sdf_map_->device(), &c, 1, &n, pos.data(), &dt, &status,
                                               &n_ticks, &n_se, &n_ee, &t_s, &t_e, cs.data(), ce.data(), &n_sp, sp.data(),
                                               &n_ep, ep.data(), first, last);
    if (rc != FUELMI_OK && rc != FUELMI_ELIMIT) {
      ROS_ERROR("[Topo]: fuelmi_map_collision_ranges: %s", fuelmi_last_error());
      return rc;
    }
    auto take = [](const vector<double>& a, int count, size_t cap, vector<Eigen::Vector3d>& out) {
      for (size_t i = 0; i < (size_t)count && i < cap; ++i) out.push_back(Eigen::Vector3d(a[3 * i], a[3 * i + 1], a[3 * i + 2]));
    };
    take(cs, n_se, ev, colli_start), take(ce, n_ee, ev, colli_end), take(sp, n_sp, mp, start_pts), take(ep, n_ep, mp, end_pts);
    return status;
  }

  // Lines 553-577 of optimizeTopoBspline for one guide path (fuelmi_map_guide_points): seg_num, the knot span dt, the rows
  // n_ctrl of the control points reparamLocalTraj would return for `duration`, and the guide points of `degree` (3 and
  // 5: n_ctrl - 6 of them, 4: n_ctrl - 8).  Returns FUELMI_TOPO_OK, FUELMI_TOPO_UNDEFINED (guide_pts empty), -1 over a
  // cap, or the library's negative return value where it refuses the call.
  int guidePoints(const vector<Eigen::Vector3d>& path, double duration, double ctrl_pt_dist, int degree, int& seg_num,
                  double& dt, int& n_ctrl, vector<Eigen::Vector3d>& guide_pts) {
    guide_pts.clear();
    seg_num = 0, dt = 0.0, n_ctrl = 0;
    const int len = (int)path.size(), mpp = len > 0 ? len : 1, max_guide = 1024;
    vector<double> p(3 * (size_t)mpp), g(3 * (size_t)max_guide);
    for (int i = 0; i < len; ++i)
      for (int k = 0; k < 3; ++k) p[3 * i + k] = path[i](k);
    int status = 0, n_pts = 0, n_guide = 0;
    const int rc = fuelmi_map_guide_points(edt_environment_->sdf_map_->device(), 1, mpp, p.data(), &len, &duration, ctrl_pt_dist,
                                           degree, max_guide, &status, &seg_num, &dt, &n_pts, &n_ctrl, &n_guide, g.data());
    if (rc != FUELMI_OK && rc != FUELMI_ELIMIT) {
      ROS_ERROR("[Topo]: fuelmi_map_guide_points: %s", fuelmi_last_error());
      return rc;
    }
    for (int i = 0; i < n_guide && i < max_guide; ++i) guide_pts.push_back(Eigen::Vector3d(g[3 * i], g[3 * i + 1], g[3 * i + 2]));
    return status;
  }

  double pathLength(const vector<Eigen::Vector3d>& path) {
    double length = 0.0;
    for (size_t i = 0; i + 1 < path.size(); ++i) length += (path[i + 1] - path[i]).norm();
    return length;
  }

  // pt_num points at equal arc length along the path.  Where the reference's behaviour is undefined (pt_num < 2, a
  // path of fewer than two points, no segment found for a point) pts comes back empty.
  void pathToGuidePts(vector<Eigen::Vector3d>& path, const int& pt_num, vector<Eigen::Vector3d>& pts) {
    pts.clear();
    if (pt_num < 2 || path.size() < 2) return;
    vector<double> len_list(1, 0.0);
    for (size_t i = 0; i + 1 < path.size(); ++i) len_list.push_back((path[i + 1] - path[i]).norm() + len_list[i]);
    const double dl = len_list.back() / double(pt_num - 1);
    for (int i = 0; i < pt_num; ++i) {
      const double cur_l = double(i) * dl;
      int idx = -1;
      for (size_t j = 0; j + 1 < len_list.size(); ++j)
        if (cur_l >= len_list[j] - 1e-4 && cur_l <= len_list[j + 1] + 1e-4) {
          idx = (int)j;
          break;
        }
      if (idx < 0) {
        pts.clear();
        return;
      }
      const double lambda = (cur_l - len_list[idx]) / (len_list[idx + 1] - len_list[idx]);
      pts.push_back((1 - lambda) * path[idx] + lambda * path[idx + 1]);
    }
  }

private:
  EDTEnvironment::Ptr edt_environment_;
  std::random_device rd_;
  std::default_random_engine eng_;
  std::uniform_real_distribution<double> rand_pos_;
  fuelmi_topo_cfg cfg_ = {};
};

}  // namespace fast_planner

#endif
