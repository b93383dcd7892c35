// active_perception/heading_planner.h -- the two members of HeadingPlanner FastPlannerManager::initPlanModules names, for
// tests/golden/make_collide_golden.py's driver (which never calls initPlanModules): declared, defined nowhere
#ifndef COLLIDE_GOLDEN_HEADING_PLANNER_H_
#define COLLIDE_GOLDEN_HEADING_PLANNER_H_
#include <memory>
#include <ros/ros.h>
#include <plan_env/sdf_map.h>
namespace fast_planner {
class HeadingPlanner {
public:
  HeadingPlanner(ros::NodeHandle& nh);
  ~HeadingPlanner();
  void setMap(const std::shared_ptr<SDFMap>& map);
};
}  // namespace fast_planner
#endif
