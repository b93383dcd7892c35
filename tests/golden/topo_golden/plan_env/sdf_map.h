// plan_env/sdf_map.h -- a dense-array stand-in for the SDFMap members TopologyPRM uses, for tests/golden/make_topo_golden.py's
// driver: the distance field is an array of doubles the driver reads from a file.
#ifndef TOPO_GOLDEN_SDF_MAP_H_
#define TOPO_GOLDEN_SDF_MAP_H_
#include <Eigen/Eigen>
#include <cmath>
#include <vector>
namespace fast_planner {
class SDFMap {
public:
  int nv[3];
  double origin[3], res, res_inv;
  std::vector<double> dist;

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
  bool isInMap(const Eigen::Vector3d& pos) {
    for (int i = 0; i < 3; ++i)
      if (pos(i) < origin[i] + 1e-4) return false;
    for (int i = 0; i < 3; ++i)
      if (pos(i) > origin[i] + nv[i] * res - 1e-4) return false;
    return true;
  }
  double getDistance(const Eigen::Vector3i& id) {
    if (!isInMap(id)) return -1;
    return dist[((size_t)id(0) * nv[1] + id(1)) * nv[2] + id(2)];
  }
  double getDistance(const Eigen::Vector3d& pos) {
    Eigen::Vector3i id;
    posToIndex(pos, id);
    return getDistance(id);
  }
  // trilinear interpolation of the eight voxels round pos; the gradient of the interpolant
  double getDistWithGrad(const Eigen::Vector3d& pos, Eigen::Vector3d& grad) {
    if (!isInMap(pos)) {
      grad.setZero();
      return 0;
    }
    Eigen::Vector3d pos_m = pos - 0.5 * res * Eigen::Vector3d(1, 1, 1);
    Eigen::Vector3i idx;
    posToIndex(pos_m, idx);
    Eigen::Vector3d idx_pos, diff;
    indexToPos(idx, idx_pos);
    diff = (pos - idx_pos) * res_inv;
    double v[2][2][2];
    for (int x = 0; x < 2; x++)
      for (int y = 0; y < 2; y++)
        for (int z = 0; z < 2; z++) v[x][y][z] = getDistance(Eigen::Vector3i(idx(0) + x, idx(1) + y, idx(2) + z));
    double v00 = (1 - diff[0]) * v[0][0][0] + diff[0] * v[1][0][0];
    double v01 = (1 - diff[0]) * v[0][0][1] + diff[0] * v[1][0][1];
    double v10 = (1 - diff[0]) * v[0][1][0] + diff[0] * v[1][1][0];
    double v11 = (1 - diff[0]) * v[0][1][1] + diff[0] * v[1][1][1];
    double v0 = (1 - diff[1]) * v00 + diff[1] * v10;
    double v1 = (1 - diff[1]) * v01 + diff[1] * v11;
    double d = (1 - diff[2]) * v0 + diff[2] * v1;
    grad[2] = (v1 - v0) * res_inv;
    grad[1] = ((1 - diff[2]) * (v10 - v00) + diff[2] * (v11 - v01)) * res_inv;
    grad[0] = (1 - diff[2]) * (1 - diff[1]) * (v[1][0][0] - v[0][0][0]);
    grad[0] += (1 - diff[2]) * diff[1] * (v[1][1][0] - v[0][1][0]);
    grad[0] += diff[2] * (1 - diff[1]) * (v[1][0][1] - v[0][0][1]);
    grad[0] += diff[2] * diff[1] * (v[1][1][1] - v[0][1][1]);
    grad[0] *= res_inv;
    return d;
  }
};
}  // namespace fast_planner
#endif
