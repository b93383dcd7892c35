// plan_env/sdf_map.h -- a dense-array stand-in for the SDFMap members HeadingPlanner uses, for
// tests/golden/make_heading_golden.py's driver: the state of every voxel (0 unknown, 1 free, 2 occupied) is an array the
// driver reads from a file, the exploration box two corners in metres.
#ifndef HEADING_GOLDEN_SDF_MAP_H_
#define HEADING_GOLDEN_SDF_MAP_H_
#include <Eigen/Eigen>
#include <algorithm>
#include <cmath>
#include <future>
#include <limits>
#include <utility>
#include <vector>
using namespace std;  // (the reference's sdf_map.h says so too, and heading_planner.cpp relies on it)
#ifndef ROS_ASSERT
#define ROS_ASSERT(c) do { if (!(c)) std::abort(); } while (0)
#endif
namespace fast_planner {
class SDFMap {
public:
  enum OCCUPANCY { UNKNOWN, FREE, OCCUPIED };
  int nv[3];
  double origin[3], res, res_inv;
  double box_mind[3], box_maxd[3];
  int box_min[3], box_max[3];
  std::vector<signed char> state;

  double getResolution() { return res; }
  void getRegion(Eigen::Vector3d& ori, Eigen::Vector3d& size) {
    for (int i = 0; i < 3; ++i) ori(i) = origin[i], size(i) = nv[i] * res;
  }
  void posToIndex(const Eigen::Vector3d& pos, Eigen::Vector3i& id) {
    for (int i = 0; i < 3; ++i) id(i) = floor((pos(i) - origin[i]) * res_inv);
  }
  void indexToPos(const Eigen::Vector3i& id, Eigen::Vector3d& pos) {
    for (int i = 0; i < 3; ++i) pos(i) = (id(i) + 0.5) * res + origin[i];
  }
  bool isInMap(const Eigen::Vector3i& id) {
    for (int i = 0; i < 3; ++i)
      if (id(i) < 0 || id(i) > nv[i] - 1) return false;
    return true;
  }
  bool isInBox(const Eigen::Vector3i& id) {
    for (int i = 0; i < 3; ++i)
      if (id[i] < box_min[i] || id[i] >= box_max[i]) return false;
    return true;
  }
  void boundBox(Eigen::Vector3d& low, Eigen::Vector3d& up) {
    for (int i = 0; i < 3; ++i) {
      low[i] = std::max(low[i], box_mind[i]);
      up[i] = std::min(up[i], box_maxd[i]);
    }
  }
  int getOccupancy(const Eigen::Vector3i& id) {
    if (!isInMap(id)) return -1;
    return state[((size_t)id(0) * nv[1] + id(1)) * nv[2] + id(2)];
  }
};
}  // namespace fast_planner
#endif
