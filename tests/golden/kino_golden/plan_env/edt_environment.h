// plan_env/edt_environment.h -- the holder of the map pointer, for tests/golden/make_kino_golden.py's driver
#ifndef KINO_GOLDEN_EDT_ENVIRONMENT_H_
#define KINO_GOLDEN_EDT_ENVIRONMENT_H_
#include <Eigen/Eigen>
#include <iostream>
#include <memory>
#include <vector>
using std::cout;
using std::endl;
using std::shared_ptr;
using std::vector;
namespace fast_planner {
class SDFMap;
class EDTEnvironment {
public:
  typedef shared_ptr<EDTEnvironment> Ptr;
  shared_ptr<SDFMap> sdf_map_;
};
}  // namespace fast_planner
#endif
