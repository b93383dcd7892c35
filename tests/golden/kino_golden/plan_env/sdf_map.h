// plan_env/sdf_map.h -- a dense-array stand-in for what kinodynamic_astar.cpp reads of SDFMap (isInBox, getInflateOccupancy,
// getOccupancy, getRegion and the UNKNOWN enumerator), used only by tests/golden/make_kino_golden.py's driver.
#ifndef KINO_GOLDEN_SDF_MAP_H_
#define KINO_GOLDEN_SDF_MAP_H_
#include <Eigen/Eigen>
#include <cmath>
#include <vector>
namespace fast_planner {
class SDFMap {
public:
  enum OCCUPANCY { UNKNOWN, FREE, OCCUPIED };
  Eigen::Vector3d origin, size, box_mind, box_maxd;
  double res_inv = 10.0;
  int nv[3] = {0, 0, 0};
  std::vector<signed char> infl;     // occupancy_buffer_inflate_
  std::vector<unsigned char> unk;    // occupancy below clamp_min_log - 1e-3
  void getRegion(Eigen::Vector3d& ori, Eigen::Vector3d& sz) { ori = origin, sz = size; }
  bool isInBox(const Eigen::Vector3d& pos) {
    for (int i = 0; i < 3; ++i)
      if (pos[i] <= box_mind[i] || pos[i] >= box_maxd[i]) return false;
    return true;
  }
  long address(const Eigen::Vector3d& pos) {
    int id[3];
    for (int i = 0; i < 3; ++i) {
      id[i] = (int)std::floor((pos[i] - origin[i]) * res_inv);
      if (id[i] < 0 || id[i] > nv[i] - 1) return -1;
    }
    return ((long)id[0] * nv[1] + id[1]) * nv[2] + id[2];
  }
  int getInflateOccupancy(const Eigen::Vector3d& pos) {
    const long a = address(pos);
    return a < 0 ? -1 : (int)infl[a];
  }
  int getOccupancy(const Eigen::Vector3d& pos) {
    const long a = address(pos);
    return a < 0 ? -1 : (unk[a] ? (int)UNKNOWN : (int)FREE);
  }
};
}  // namespace fast_planner
#endif
