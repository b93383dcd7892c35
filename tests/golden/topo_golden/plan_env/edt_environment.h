// plan_env/edt_environment.h -- the two queries TopologyPRM makes, on the dense-array SDFMap of this directory, for
// tests/golden/make_topo_golden.py's driver (time < 0: no moving obstacles)
#ifndef TOPO_GOLDEN_EDT_ENVIRONMENT_H_
#define TOPO_GOLDEN_EDT_ENVIRONMENT_H_
#include <Eigen/Eigen>
#include <ros/ros.h>
#include <iostream>
#include <list>
#include <memory>
#include <vector>
#include <plan_env/sdf_map.h>
using namespace std;
namespace fast_planner {
class EDTEnvironment {
public:
  typedef shared_ptr<EDTEnvironment> Ptr;
  shared_ptr<SDFMap> sdf_map_;
  void evaluateEDTWithGrad(const Eigen::Vector3d& pos, double time, double& dist, Eigen::Vector3d& grad) {
    dist = sdf_map_->getDistWithGrad(pos, grad);
  }
  double evaluateCoarseEDT(Eigen::Vector3d& pos, double time) { return sdf_map_->getDistance(pos); }
};
}  // namespace fast_planner
#endif
