// active_perception/heading_planner.h -- drop-in for the reference header of the same name
// (fuel_planner/active_perception/include/active_perception/heading_planner.h): the public names FastPlannerManager uses
// (plan_manage/src/planner_manager.cpp:84-85, planner_manager_dev.cpp:63, 210).  searchPathOfYaw and calcInfoGain run on
// the device (fuelmi_map_yaw_paths / fuelmi_map_info_gains, one problem) against the map's own unknown and occupied
// planes: no host mirror of the map is read.  The parameters are read from the node handle under the reference's names;
// the definitions are in libfuelmi_facade.so.
// Added: the batch forms searchPathsOfYaw (many trajectories in one call) and calcInfoGains (many poses, localExplore's
// loop of :205-217 in one call); far_ and the three half angles as members (constants of the reference's constructor);
// what the last call left (its return value, the statuses, the chosen vertices, the gains).
// Dropped: setFrontier / calcVisibFrontier / showVisibFrontier (the kd-tree variant the reference itself calls "not
// good"); the Graph and vertex classes, which only searchPathOfYaw used; task_id, which selected a RayCaster.
#ifndef _HEADING_PLANNER_H_
#define _HEADING_PLANNER_H_

#include <list>
#include <memory>
#include <mutex>
#include <queue>
#include <unordered_map>
#include <vector>

#include <ros/ros.h>

#include <Eigen/Eigen>

using std::list;
using std::queue;
using std::shared_ptr;
using std::unique_ptr;
using std::unordered_map;
using std::vector;

namespace fast_planner {
class SDFMap;

class HeadingPlanner {
public:
  enum WEIGHT_TYPE { NON_UNIFORM, UNIFORM };

  HeadingPlanner(ros::NodeHandle& nh);
  ~HeadingPlanner();

  void setMap(const shared_ptr<SDFMap>& map);
  // path: the yaw per way-point; empty when the library refuses the call or the problem is over a cap (last_rc_,
  // last_status_ say which)
  void searchPathOfYaw(const vector<Eigen::Vector3d>& pts, const vector<double>& yaws, const double& dt,
                       const Eigen::MatrixXd& ctrl_pts, vector<double>& path);
  double calcInfoGain(const Eigen::Vector3d& pt, const double& yaw, const int& task_id);

  // searchPathOfYaw for many trajectories in one call; returns the library's return value.  paths[i] is empty for a
  // problem over a cap.
  int searchPathsOfYaw(const vector<vector<Eigen::Vector3d>>& pts, const vector<vector<double>>& yaws,
                       const vector<double>& dts, const vector<Eigen::MatrixXd>& ctrl_pts, vector<vector<double>>& paths);
  // calcInfoGain for many poses in one call; returns the library's return value
  int calcInfoGains(const vector<Eigen::Vector3d>& pts, const vector<double>& yaws, vector<double>& gains);

  // params (heading_planner/*) and the constants of the reference's constructor
  double yaw_diff_, lambda1_, lambda2_;
  int half_vert_num_;
  double max_yaw_rate_, w_;
  int weight_type_;
  double far_, top_ang_, left_ang_, right_ang_;

  // of the last call
  int last_rc_ = 0;
  vector<int> last_status_;                  // per problem
  vector<vector<int>> last_path_vertex_;     // per problem, per layer: the chosen candidate
  vector<vector<double>> last_gains_;        // per problem: [layer][2 * half_vert_num_ + 1]
  vector<vector<double>> last_g_value_;

private:
  shared_ptr<SDFMap> sdf_map_;
};

}  // namespace fast_planner

#endif
