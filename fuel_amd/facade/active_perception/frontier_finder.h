// active_perception/frontier_finder.h -- drop-in for the reference header of the same name
// (fuel_planner/active_perception/include/active_perception/frontier_finder.h:25-80).
//
// Behind the same records (Frontier, Viewpoint) and calls: searchFrontiers() runs scan, clustering,
// splitLargeFrontiers and the down-sampling on the device; computeFrontiersToVisit() samples and scores
// the viewpoints there; isFrontierCovered() checks coverage there.  The cost-matrix / tour group
// (updateFrontierCostMatrix, getFullCostMatrix, getPathForTour, setNextFrontier) keeps the reference's
// bookkeeping.  By default each path comes from the package's own ViewNode (A* through the map, one pair at a
// time); with the addition frontier/device_path_cost = true the path searches run batched on the device
// (fuelmi_map_path_costs: one call per updateFrontierCostMatrix, per getFullCostMatrix row 0, per
// getPathForTour first leg) and ViewNode::computeCost's velocity / yaw terms are host arithmetic with
// exploration/vm, exploration/yd, exploration/w_dir.
#ifndef _FRONTIER_FINDER_H_
#define _FRONTIER_FINDER_H_

#include <ros/ros.h>
#include <Eigen/Eigen>
#include <list>
#include <memory>
#include <utility>
#include <vector>

#include "fuelmi.h"

using Eigen::Vector3d;
using std::list;
using std::pair;
using std::shared_ptr;
using std::unique_ptr;
using std::vector;

namespace fast_planner {
class EDTEnvironment;
class PerceptionUtils;  // active_perception/perception_utils.h (the package's own class, not replaced)

// one sampled viewpoint of a frontier cluster: where to hover, where to look, how many of the cluster's
// down-sampled cells it sees
struct Viewpoint {
  Vector3d pos_;
  double yaw_;
  int visib_num_;
};

// a frontier cluster as the exploration planner consumes it
struct Frontier {
  int id_;
  Vector3d average_, box_min_, box_max_;  // mean and AABB of the cells (voxel centres)
  vector<Vector3d> cells_;                // voxel centres, ascending voxel address (reference: BFS order)
  vector<Vector3d> filtered_cells_;       // VoxelGrid centroids (needs frontier/cluster_size_xy + down_sample)
  vector<Viewpoint> viewpoints_;          // best coverage first (needs the candidate_* / perception_utils params)
  list<vector<Vector3d>> paths_;          // to every frontier of frontiers_, in list order (updateFrontierCostMatrix)
  list<double> costs_;
};

class FrontierFinder {
public:
  FrontierFinder(const shared_ptr<EDTEnvironment>& edt, ros::NodeHandle& node);
  ~FrontierFinder();

  // per plan cycle: find / update the clusters, then sample viewpoints for the new ones
  void searchFrontiers();
  void computeFrontiersToVisit();
  bool isFrontierCovered();

  // cluster queries
  void getFrontiers(vector<vector<Vector3d>>& clusters);
  void getDormantFrontiers(vector<vector<Vector3d>>& clusters);
  void getFrontierBoxes(vector<pair<Vector3d, Vector3d>>& boxes);

  // viewpoint queries: the best viewpoint of every active cluster that is not too close to cur_pos, and
  // the few best of selected clusters
  void getTopViewpointsInfo(const Vector3d& cur_pos, vector<Vector3d>& points, vector<double>& yaws,
                            vector<Vector3d>& averages);
  void getViewpointsInfo(const Vector3d& cur_pos, const vector<int>& ids, const int& view_num,
                         const double& max_decay, vector<vector<Vector3d>>& points,
                         vector<vector<double>>& yaws);
  void wrapYaw(double& yaw);

  // tour planning (TSP input): pairwise costs between the best viewpoints of the active clusters, kept
  // incrementally across searches; the full matrix with the current state in row 0; the stored paths
  // along a tour
  void updateFrontierCostMatrix();
  void getFullCostMatrix(const Vector3d& cur_pos, const Vector3d& cur_vel, const Vector3d cur_yaw,
                         Eigen::MatrixXd& mat);
  void getPathForTour(const Vector3d& pos, const vector<int>& frontier_ids, vector<Vector3d>& path);
  void setNextFrontier(const int& id);

  // addition: FastExplorationManager::refineLocalTour (fast_exploration_manager.cpp:429-503) on the device
  // (fuelmi_map_refine_tours): the first node of each layer of n_points / n_yaws (getViewpointsInfo's output) that the
  // cheapest route from the current state passes, and with refined_tour the polyline the reference draws (lattice
  // 0.2).  Needs exploration/vm, exploration/yd, exploration/w_dir; false (with a message) when they are unset, a
  // layer is empty or the last layer cannot be reached.
  bool refineLocalTour(const Vector3d& cur_pos, const Vector3d& cur_vel, const Vector3d& cur_yaw,
                       const vector<vector<Vector3d>>& n_points, const vector<vector<double>>& n_yaws,
                       vector<Vector3d>& refined_pts, vector<double>& refined_yaws,
                       vector<Vector3d>* refined_tour = nullptr);
  // the single-destination branch (:197-208): the index of the cheapest of points (first on ties)
  bool refineSingleDestination(const Vector3d& cur_pos, const Vector3d& cur_vel, const Vector3d& cur_yaw,
                               const vector<Vector3d>& points, const vector<double>& yaws, int& min_cost_id);

  // addition: the geometric path to the next viewpoint, FastExplorationManager::planExploreMotion's Astar::search +
  // shortenPath + length branch (fast_exploration_manager.cpp:234-276, 295-325) on the device (fuelmi_map_goal_paths,
  // lattice 0.2).  Returns the branch: GOAL_CLOSE / GOAL_FAR -- planExploreTraj on path_next_goal (the shortened
  // path, truncated at 5 m for GOAL_FAR); GOAL_MID -- kinodynamicReplan to next_goal (path_next_goal: the shortened
  // path); GOAL_NO_PATH -- the reference's `return FAIL` (path_next_goal empty, with a message); GOAL_ERROR -- the
  // device call failed.  next_goal: ed_->next_goal_.
  enum { GOAL_ERROR = -1, GOAL_CLOSE = 0, GOAL_MID = 1, GOAL_FAR = 2, GOAL_NO_PATH = 3 };
  int planPathToViewpoint(const Vector3d& cur_pos, const Vector3d& next_pos, vector<Vector3d>& path_next_goal,
                          Vector3d& next_goal);

  // addition: FastExplorationManager::findGlobalTour (fast_exploration_manager.cpp:327-420) without the file round
  // trip through LKH: updateFrontierCostMatrix, getFullCostMatrix, the reference's int(cost * 100), then the device
  // ATSP solver (fuelmi_tsp_solve, created on first use on the map's device with the FUELMI_TSP_DEFAULT_* settings).
  // indices: the frontiers in tour order (LKH id - 2 in the reference); with global_tour also getPathForTour's polyline.
  // false (with a message) when an entry cannot be converted to int or the solve fails.
  bool findGlobalTour(const Vector3d& cur_pos, const Vector3d& cur_vel, const Vector3d cur_yaw, vector<int>& indices,
                      vector<Vector3d>* global_tour = nullptr);
  // camera model for the callers (field-of-view drawing); the device samples viewpoints with its own copy
  // of the same perception_utils/* parameters
  shared_ptr<PerceptionUtils> percep_utils_;

  // additions: clusters found by the last searchFrontiers() and the list positions it removed
  const list<Frontier>& newFrontiers() const { return tmp_frontiers_; }
  const vector<int>& removedIds() const { return removed_ids_; }
  fuelmi_frontier* device() const { return dev_; }  // the C-ABI object behind the finder (like SDFMap::device())

private:
  void pull(int which, list<Frontier>& out, int from = 0);
  // frontier/device_path_cost: searchPath for n pairs in one device call; paths may be NULL (costs only)
  void devicePaths(const vector<Vector3d>& p1, const vector<Vector3d>& p2, vector<double>& length,
                   vector<vector<Vector3d>>* paths);
  // ViewNode::computeCost (graph_node.cpp:63-88) with the path length already known
  double hostCost(double length, const Vector3d& p1, const Vector3d& p2, double y1, double y2,
                  const Vector3d& v1) const;
  // one fuelmi_map_refine_tours problem; choice per layer
  bool deviceRefine(const Vector3d& cur_pos, const Vector3d& cur_vel, double cur_yaw,
                    const vector<vector<Vector3d>>& n_points, const vector<vector<double>>& n_yaws, int flags,
                    vector<int>& choice, vector<Vector3d>* tour);

  fuelmi_frontier* dev_;
  fuelmi_tsp* tsp_ = nullptr;  // findGlobalTour's solver (created on first use)
  shared_ptr<EDTEnvironment> edt_env_;
  int cluster_min_;
  double resolution_, min_candidate_dist_;
  bool have_viewpoints_;  // frontier/candidate_* and perception_utils/* were all given
  bool device_path_cost_ = false;  // frontier/device_path_cost (addition, default false)
  double vm_ = -1.0, yd_ = -1.0, w_dir_ = -1.0;  // exploration/vm, exploration/yd, exploration/w_dir (-1: unset)
  bool order_fallback_logged_ = false;  // the first address-order fallback of reference_order = 2 has been reported
  vector<int> removed_ids_;
  list<Frontier> frontiers_, dormant_frontiers_, tmp_frontiers_;
  // storage of the large cells_ vectors a pull() replaces, kept for the next one: a fresh 3.4 MB vector<Vector3d> is a
  // new mapping whose first touch faults 830 pages -- as long as decoding the cells into it
  vector<vector<Vector3d>> cells_spare_;
  list<Frontier>::iterator first_new_ftr_;  // first cluster appended by the last computeFrontiersToVisit()
  Frontier next_frontier_;
};
}  // namespace fast_planner
#endif
