// facade.cpp -- the reference's C++ class interfaces over the libfuelmi C-ABI (host side only;
// every computation is a HIP kernel behind include/fuelmi.h).  See INTEGRATION.md.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <deque>
#include <limits>

#include "plan_env/sdf_map.h"
#include "plan_env/edt_environment.h"
#include "active_perception/frontier_finder.h"
#include "active_perception/graph_node.h"
#include "active_perception/heading_planner.h"
#include "active_perception/perception_utils.h"
#include "bspline_opt/bspline_optimizer.h"

namespace fast_planner {

// the device of the map initMap set up last: the drop-in solveTSPLKH (libfuelmi_lkh.so) solves there
static std::atomic<int> g_last_map_device(-1);

static void warn(const char* what, int rc) {
  // error convention of the reference: void returns, log and continue
  if (rc != FUELMI_OK) std::fprintf(stderr, "[fuelmi] %s failed (%d): %s\n", what, rc, fuelmi_last_error());
}

// ------------------------------------------------------------------------------------------------
// SDFMap
// ------------------------------------------------------------------------------------------------
SDFMap::SDFMap() : ext_(new Ext{nullptr, true, true, true, 0}) {}
SDFMap::~SDFMap() {
  if (ext_->dev) fuelmi_map_destroy(ext_->dev);
  delete ext_;
}
// (never called: this library does not create either object -- see the data members in plan_env/sdf_map.h)
void SDFMap::MapROSDelete::operator()(MapROS*) const {}
void SDFMap::RayCasterDelete::operator()(RayCaster*) const {}

void SDFMap::initMap(ros::NodeHandle& nh) {
  // parameter names and defaults of the reference (plan_env/src/sdf_map.cpp:19-47,78-82)
  mp_.reset(new MapParam);
  md_.reset(new MapData);
  fuelmi_map_cfg c;
  double x_size, y_size, z_size;
  nh.param("sdf_map/resolution", c.resolution, -1.0);
  nh.param("sdf_map/map_size_x", x_size, -1.0);
  nh.param("sdf_map/map_size_y", y_size, -1.0);
  nh.param("sdf_map/map_size_z", z_size, -1.0);
  nh.param("sdf_map/obstacles_inflation", c.obstacles_inflation, -1.0);
  nh.param("sdf_map/local_bound_inflate", c.local_bound_inflate, 1.0);
  nh.param("sdf_map/local_map_margin", mp_->local_map_margin_, 1);
  nh.param("sdf_map/ground_height", c.ground_height, 1.0);
  nh.param("sdf_map/default_dist", c.default_dist, 5.0);
  bool optimistic, signed_dist;
  nh.param("sdf_map/optimistic", optimistic, true);
  nh.param("sdf_map/signed_dist", signed_dist, false);
  c.optimistic = optimistic;
  c.signed_dist = signed_dist;
  nh.param("sdf_map/p_hit", c.p_hit, 0.70);
  nh.param("sdf_map/p_miss", c.p_miss, 0.35);
  nh.param("sdf_map/p_min", c.p_min, 0.12);
  nh.param("sdf_map/p_max", c.p_max, 0.97);
  nh.param("sdf_map/p_occ", c.p_occ, 0.80);
  nh.param("sdf_map/max_ray_length", c.max_ray_length, -0.1);
  nh.param("sdf_map/virtual_ceil_height", c.virtual_ceil_height, -0.1);
  int device = 0;
  nh.param("sdf_map/hip_device", device, 0);  // addition: which GPU hosts this map
  c.device = device;
  ext_->hip_device = device;
  g_last_map_device.store(device);
  c.map_size[0] = x_size, c.map_size[1] = y_size, c.map_size[2] = z_size;
  const double org[3] = {-x_size / 2.0, -y_size / 2.0, c.ground_height};
  const char* axis[3] = {"x", "y", "z"};
  for (int i = 0; i < 3; ++i) {
    nh.param(std::string("sdf_map/box_min_") + axis[i], c.box_min[i], org[i]);
    nh.param(std::string("sdf_map/box_max_") + axis[i], c.box_max[i], org[i] + c.map_size[i]);
  }
  // process set-up (include/fuelmi.h): hardware queues for the streams of the map, its finder and the optimiser threads.
  // In time only if nothing in the node has initialised HIP yet -- fuelmi_hw_queues_state() tells; exporting
  // GPU_MAX_HW_QUEUES in the launch file is the way that does not depend on the order
  fuelmi_init(0);
  int rc = fuelmi_map_create(&c, &ext_->dev);
  warn("fuelmi_map_create", rc);
  if (rc != FUELMI_OK) return;
  fuelmi_map_info I;
  fuelmi_map_get_info(ext_->dev, &I);
  mp_->resolution_ = c.resolution;
  mp_->resolution_inv_ = I.resolution_inv;
  mp_->obstacles_inflation_ = c.obstacles_inflation;
  mp_->local_bound_inflate_ = std::max(c.resolution, c.local_bound_inflate);
  mp_->ground_height_ = c.ground_height;
  mp_->virtual_ceil_height_ = c.virtual_ceil_height;
  mp_->default_dist_ = c.default_dist;
  mp_->optimistic_ = optimistic;
  mp_->signed_dist_ = signed_dist;
  mp_->p_hit_ = c.p_hit, mp_->p_miss_ = c.p_miss, mp_->p_min_ = c.p_min, mp_->p_max_ = c.p_max, mp_->p_occ_ = c.p_occ;
  mp_->prob_hit_log_ = I.prob_hit_log, mp_->prob_miss_log_ = I.prob_miss_log;
  mp_->clamp_min_log_ = I.clamp_min_log, mp_->clamp_max_log_ = I.clamp_max_log;
  mp_->min_occupancy_log_ = I.min_occupancy_log;
  mp_->max_ray_length_ = c.max_ray_length;
  mp_->unknown_flag_ = 0.01;
  for (int i = 0; i < 3; ++i) {
    mp_->map_origin_(i) = I.origin[i];
    mp_->map_size_(i) = c.map_size[i];
    mp_->map_min_boundary_(i) = I.min_boundary[i];
    mp_->map_max_boundary_(i) = I.max_boundary[i];
    mp_->map_voxel_num_(i) = I.voxel_num[i];
    mp_->box_min_(i) = I.box_min[i];
    mp_->box_max_(i) = I.box_max[i];
    mp_->box_mind_(i) = c.box_min[i];
    mp_->box_maxd_(i) = c.box_max[i];
  }
  const size_t n = (size_t)getVoxelNum();
  md_->occupancy_buffer_.assign(n, mp_->clamp_min_log_ - mp_->unknown_flag_);
  md_->occupancy_buffer_inflate_.assign(n, 0);
  md_->distance_buffer_.assign(n, mp_->default_dist_);
  md_->reset_updated_box_ = true;
  for (int i = 0; i < 3; ++i) {
    md_->update_min_(i) = md_->update_max_(i) = 0.0;
    md_->local_bound_min_(i) = md_->local_bound_max_(i) = 0;
  }
  // the mirrors never move again: pin and map them once, every refresh is then one kernel storing the box
  // voxels straight into them (no staging copy, one synchronisation)
  warn("fuelmi_map_register_mirrors",
       fuelmi_map_register_mirrors(ext_->dev, md_->occupancy_buffer_.data(), md_->occupancy_buffer_inflate_.data(),
                                   md_->distance_buffer_.data()));
}

void SDFMap::setHostMirror(bool occupancy, bool inflate, bool distance) {
  ext_->mirror_occ = occupancy, ext_->mirror_infl = inflate, ext_->mirror_dist = distance;
}

void SDFMap::pullBounds() {
  int lo[3], hi[3];
  double a[3], b[3];
  fuelmi_map_get_local_bound(ext_->dev, lo, hi);
  fuelmi_map_get_updated_box(ext_->dev, a, b, 0);
  for (int i = 0; i < 3; ++i) {
    md_->local_bound_min_(i) = lo[i], md_->local_bound_max_(i) = hi[i];
    md_->update_min_(i) = a[i], md_->update_max_(i) = b[i];
  }
}

void SDFMap::syncMirrors(const Eigen::Vector3i& bmin, const Eigen::Vector3i& bmax, bool occ, bool infl, bool dist) {
  if (!(occ || infl || dist)) return;
  const int lo[3] = {bmin(0), bmin(1), bmin(2)}, hi[3] = {bmax(0), bmax(1), bmax(2)};
  warn("fuelmi_map_sync_host",
       fuelmi_map_sync_host(ext_->dev, lo, hi, occ ? md_->occupancy_buffer_.data() : nullptr,
                            infl ? md_->occupancy_buffer_inflate_.data() : nullptr,
                            dist ? md_->distance_buffer_.data() : nullptr));
}

void SDFMap::inputPointCloud(const pcl::PointCloud<pcl::PointXYZ>& points, const int& point_num,
                             const Eigen::Vector3d& camera_pos) {
  if (point_num == 0) return;
  const double cam[3] = {camera_pos(0), camera_pos(1), camera_pos(2)};
  warn("fuelmi_map_input_points",
       fuelmi_map_input_points(ext_->dev, &points.points[0].x, (int)sizeof(pcl::PointXYZ), point_num, cam));
  pullBounds();
  md_->reset_updated_box_ = false;
  // fused voxels lie in the index box of camera + end points, inside the inflated local bound
  syncMirrors(md_->local_bound_min_, md_->local_bound_max_, ext_->mirror_occ, false, false);
}

void SDFMap::clearAndInflateLocalMap() {
  warn("fuelmi_map_inflate_local", fuelmi_map_inflate_local(ext_->dev));
  // stamps spill up to inflate_step voxels outside the box; a stamp that leaves the map in z lands in the
  // neighbouring y row at the other end of z, one that leaves it in y in the neighbouring x slab (the
  // reference only tests the linear address, sdf_map.cpp:453-458): widen the refreshed box accordingly
  Eigen::Vector3i lo = md_->local_bound_min_, hi = md_->local_bound_max_;
  const int s = (int)std::ceil(mp_->obstacles_inflation_ / mp_->resolution_);
  for (int k = 0; k < 3; ++k) lo(k) -= s, hi(k) += s;
  for (int k = 2; k >= 1; --k)
    if (lo(k) < 0 || hi(k) > mp_->map_voxel_num_(k) - 1) {
      lo(k) = 0, hi(k) = mp_->map_voxel_num_(k) - 1;
      lo(k - 1) -= 1, hi(k - 1) += 1;
    }
  boundIndex(lo);
  boundIndex(hi);
  syncMirrors(lo, hi, false, ext_->mirror_infl, false);
  // the virtual ceiling (sdf_map.cpp:464-471) rewrites occupancy_buffer_ in one z row over the x,y extent of
  // the local bound: the callers' inline getOccupancy() must see it right away, as in the reference
  if (ext_->mirror_occ && mp_->virtual_ceil_height_ > -0.5) {
    const int ceil_id = (int)floor((mp_->virtual_ceil_height_ - mp_->map_origin_(2)) * mp_->resolution_inv_);
    if (ceil_id >= 0 && ceil_id < mp_->map_voxel_num_(2)) {
      Eigen::Vector3i clo = md_->local_bound_min_, chi = md_->local_bound_max_;
      clo(2) = chi(2) = ceil_id;
      syncMirrors(clo, chi, true, false, false);
    }
  }
}

void SDFMap::updateESDF3d() {
  warn("fuelmi_map_update_esdf", fuelmi_map_update_esdf(ext_->dev));
  syncMirrors(md_->local_bound_min_, md_->local_bound_max_, false, false, ext_->mirror_dist);
}

void SDFMap::resetBuffer() {
  warn("fuelmi_map_reset_buffer_all", fuelmi_map_reset_buffer_all(ext_->dev));
  pullBounds();
  syncMirrors(md_->local_bound_min_, md_->local_bound_max_, false, ext_->mirror_infl, ext_->mirror_dist);
}

void SDFMap::resetBuffer(const Eigen::Vector3d& min_pos, const Eigen::Vector3d& max_pos) {
  const double a[3] = {min_pos(0), min_pos(1), min_pos(2)}, b[3] = {max_pos(0), max_pos(1), max_pos(2)};
  warn("fuelmi_map_reset_buffer", fuelmi_map_reset_buffer(ext_->dev, a, b));
  Eigen::Vector3i lo, hi;
  posToIndex(min_pos, lo);
  posToIndex(max_pos, hi);
  boundIndex(lo);
  boundIndex(hi);
  syncMirrors(lo, hi, false, ext_->mirror_infl, ext_->mirror_dist);
}

static fuelmi_cloud_cfg cloud_cfg(int kind, const Eigen::Vector3i& lo, const Eigen::Vector3i& hi, double z_low, double z_high) {
  fuelmi_cloud_cfg c;
  c.kind = kind;
  for (int k = 0; k < 3; ++k) c.lo[k] = lo(k), c.hi[k] = hi(k);
  c.z_low = z_low, c.z_high = z_high;
  return c;
}

int SDFMap::extractCloud(int kind, const Eigen::Vector3i& lo, const Eigen::Vector3i& hi, double z_low, double z_high,
                         std::vector<float>& xyz) {
  const fuelmi_cloud_cfg c = cloud_cfg(kind, lo, hi, z_low, z_high);
  int cap = (int)std::min<size_t>(xyz.capacity() / 3, (size_t)1 << 30), n = 0;
  xyz.resize((size_t)cap * 3);
  int rc = fuelmi_map_extract_cloud(ext_->dev, &c, cap ? xyz.data() : nullptr, cap, &n);
  if (rc == FUELMI_ELIMIT || (rc == FUELMI_OK && n > cap)) {  // the full count is known: once more, with room
    cap = n;
    xyz.resize((size_t)cap * 3);
    rc = fuelmi_map_extract_cloud(ext_->dev, &c, xyz.data(), cap, &n);
  }
  warn("fuelmi_map_extract_cloud", rc);
  if (rc != FUELMI_OK) n = -1;
  xyz.resize((size_t)std::max(n, 0) * 3);
  return n;
}

int SDFMap::countVoxels(int kind, const Eigen::Vector3i& lo, const Eigen::Vector3i& hi) {
  const double nan = std::numeric_limits<double>::quiet_NaN();  // no bound
  const fuelmi_cloud_cfg c = cloud_cfg(kind, lo, hi, nan, nan);
  int n = 0;
  const int rc = fuelmi_map_extract_cloud(ext_->dev, &c, nullptr, 0, &n);
  warn("fuelmi_map_extract_cloud", rc);
  return rc == FUELMI_OK ? n : -1;
}

void SDFMap::setOccupied(const Eigen::Vector3d& pos, const int& occ) {
  if (!isInMap(pos)) return;
  const double p[3] = {pos(0), pos(1), pos(2)};
  const int rc = fuelmi_map_set_occupied(ext_->dev, p, 1, occ);
  warn("fuelmi_map_set_occupied", rc);
  if (rc != FUELMI_OK) return;  // the device refused the value (only 0 / 1 exist there): the mirror must not diverge
  Eigen::Vector3i id;
  posToIndex(pos, id);
  md_->occupancy_buffer_inflate_[toAddress(id)] = (char)occ;
}

// Trilinear distance + gradient (sdf_map.cpp:497-536).  The reference's callers ask point by point inside host
// loops (traj_visibility.cpp:85,114,146, topo_prm.cpp:490): with the distance mirror on, the answer comes from
// the host copy -- eight loads like the reference, the device's own arithmetic on the same f64 values, hence
// the same doubles -- instead of a GPU round trip per point.  Batches go to the device (getDistWithGradBatch).
double SDFMap::getDistWithGrad(const Eigen::Vector3d& pos, Eigen::Vector3d& grad) {
  if (ext_->mirror_dist) {
    if (!isInMap(pos)) {
      grad = Eigen::Vector3d(0, 0, 0);
      return 0;
    }
    Eigen::Vector3i idx;
    double diff[3];
    for (int k = 0; k < 3; ++k) {
      const double pm = pos(k) - 0.5 * mp_->resolution_ * 1.0;
      idx(k) = (int)floor((pm - mp_->map_origin_(k)) * mp_->resolution_inv_);
      const double centre = (idx(k) + 0.5) * mp_->resolution_ + mp_->map_origin_(k);
      diff[k] = (pos(k) - centre) * mp_->resolution_inv_;
    }
    double v[2][2][2];
    for (int x = 0; x < 2; ++x)
      for (int y = 0; y < 2; ++y)
        for (int z = 0; z < 2; ++z) v[x][y][z] = getDistance(Eigen::Vector3i(idx(0) + x, idx(1) + y, idx(2) + z));
    const double ri = mp_->resolution_inv_;
    const double v00 = (1 - diff[0]) * v[0][0][0] + diff[0] * v[1][0][0];
    const double v01 = (1 - diff[0]) * v[0][0][1] + diff[0] * v[1][0][1];
    const double v10 = (1 - diff[0]) * v[0][1][0] + diff[0] * v[1][1][0];
    const double v11 = (1 - diff[0]) * v[0][1][1] + diff[0] * v[1][1][1];
    const double v0 = (1 - diff[1]) * v00 + diff[1] * v10;
    const double v1 = (1 - diff[1]) * v01 + diff[1] * v11;
    const double dist = (1 - diff[2]) * v0 + diff[2] * v1;
    grad(2) = (v1 - v0) * ri;
    grad(1) = ((1 - diff[2]) * (v10 - v00) + diff[2] * (v11 - v01)) * ri;
    double g0 = (1 - diff[2]) * (1 - diff[1]) * (v[1][0][0] - v[0][0][0]);
    g0 += (1 - diff[2]) * diff[1] * (v[1][1][0] - v[0][1][0]);
    g0 += diff[2] * (1 - diff[1]) * (v[1][0][1] - v[0][0][1]);
    g0 += diff[2] * diff[1] * (v[1][1][1] - v[0][1][1]);
    grad(0) = g0 * ri;
    return dist;
  }
  const double p[3] = {pos(0), pos(1), pos(2)};
  double d = 0.0, g[3] = {0, 0, 0};
  warn("fuelmi_map_dist_grad", fuelmi_map_dist_grad(ext_->dev, p, 1, &d, g));
  for (int k = 0; k < 3; ++k) grad(k) = g[k];
  return d;
}
void SDFMap::getDistWithGradBatch(const double* pos_xyz, int n, double* dist, double* grad_xyz) {
  warn("fuelmi_map_dist_grad", fuelmi_map_dist_grad(ext_->dev, pos_xyz, n, dist, grad_xyz));
}

void SDFMap::getRegion(Eigen::Vector3d& ori, Eigen::Vector3d& size) { ori = mp_->map_origin_, size = mp_->map_size_; }
void SDFMap::getBox(Eigen::Vector3d& bmin, Eigen::Vector3d& bmax) { bmin = mp_->box_mind_, bmax = mp_->box_maxd_; }
void SDFMap::getUpdatedBox(Eigen::Vector3d& bmin, Eigen::Vector3d& bmax, bool reset) {
  double a[3], b[3];
  fuelmi_map_get_updated_box(ext_->dev, a, b, reset ? 1 : 0);
  for (int k = 0; k < 3; ++k) bmin(k) = a[k], bmax(k) = b[k];
  if (reset) md_->reset_updated_box_ = true;
}
double SDFMap::getResolution() { return mp_->resolution_; }
int SDFMap::getVoxelNum() { return mp_->map_voxel_num_(0) * mp_->map_voxel_num_(1) * mp_->map_voxel_num_(2); }

// ------------------------------------------------------------------------------------------------
// EDTEnvironment (plan_env/src/edt_environment.cpp:7-20,78-97)
// ------------------------------------------------------------------------------------------------
void EDTEnvironment::init() {}
void EDTEnvironment::setMap(shared_ptr<SDFMap>& map) {
  sdf_map_ = map;
  resolution_inv_ = 1 / sdf_map_->getResolution();
}
void EDTEnvironment::setObjPrediction(ObjPrediction prediction) { obj_prediction_ = prediction; }
void EDTEnvironment::setObjScale(ObjScale scale) { obj_scale_ = scale; }
void EDTEnvironment::evaluateEDTWithGrad(const Eigen::Vector3d& pos, double, double& dist, Eigen::Vector3d& grad) {
  dist = sdf_map_->getDistWithGrad(pos, grad);
}
double EDTEnvironment::evaluateCoarseEDT(Eigen::Vector3d& pos, double) { return sdf_map_->getDistance(pos); }

// ------------------------------------------------------------------------------------------------
// FrontierFinder (grid part)
// ------------------------------------------------------------------------------------------------
FrontierFinder::FrontierFinder(const shared_ptr<EDTEnvironment>& edt, ros::NodeHandle& nh) : dev_(nullptr), edt_env_(edt) {
  nh.param("frontier/cluster_min", cluster_min_, -1);
  percep_utils_.reset(new PerceptionUtils(nh));  // for the callers (:44); the device has its own copy of the parameters
  resolution_ = edt_env_->sdf_map_->getResolution();
  double cluster_size_xy = -1.0;
  int down_sample = -1;
  nh.param("frontier/cluster_size_xy", cluster_size_xy, -1.0);
  nh.param("frontier/down_sample", down_sample, -1);
  fuelmi_frontier_cfg c;
  c.cluster_min = cluster_min_;
  c.min_z = 0.4;  // literal in frontier_finder.cpp:151
  c.cluster_size_xy = cluster_size_xy;
  c.down_sample = down_sample;
  // searchFrontiers ends with splitLargeFrontiers (:120); without its two parameters the search stops
  // at the region-grown clusters
  c.split = (cluster_size_xy > 0.0 && down_sample > 0) ? 1 : 0;
  // addition: frontier/reference_order.  1 lists cells_ in the reference's BFS order and sums average_ / the
  // VoxelGrid centroids in that order (bit-identical means, filtered_cells_, viewpoints and visib_num_) at the price
  // of a level-by-level sweep per search.  2 (default here): order 1 for every search whose clusters hold at most
  // 26624 cells each -- every incremental search of an exploration run, +0.15 ... 0.6 ms as measured on the
  // streaming workload -- and the address order for giant ones (a fresh full-box search: the sweep would cost
  // 24 ms on the 400x400x100 map).  0 is the address order throughout: the fastest path, means equal to the last
  // bits of a double, visib_num_ within a few cells (tests/test_golden_pillar.py asserts the bound).
  int ref_order = 2;
  nh.param("frontier/reference_order", ref_order, 2);
  c.reference_order = ref_order;
  // addition: frontier/device_path_cost.  true: the cost-matrix group's path searches run batched on the device
  // (fuelmi_map_path_costs) and computeCost's remaining terms need the exploration manager's ViewNode parameters
  // (fast_exploration_manager.cpp:55-59); false (default): ViewNode as in the reference.  refineLocalTour needs the
  // same parameters
  nh.param("frontier/device_path_cost", device_path_cost_, false);
  nh.param("exploration/vm", vm_, -1.0);
  nh.param("exploration/yd", yd_, -1.0);
  nh.param("exploration/w_dir", w_dir_, -1.0);
  warn("fuelmi_frontier_create", fuelmi_frontier_create(edt_env_->sdf_map_->device(), &c, &dev_));
  // viewpoint sampling parameters (frontier_finder.cpp:32-43, perception_utils.cpp:7-11)
  fuelmi_viewpoint_cfg v;
  nh.param("frontier/candidate_rmin", v.candidate_rmin, -1.0);
  nh.param("frontier/candidate_rmax", v.candidate_rmax, -1.0);
  nh.param("frontier/candidate_rnum", v.candidate_rnum, -1);
  nh.param("frontier/candidate_dphi", v.candidate_dphi, -1.0);
  nh.param("frontier/min_candidate_clearance", v.min_candidate_clearance, -1.0);
  nh.param("frontier/min_visib_num", v.min_visib_num, -1);
  nh.param("frontier/min_candidate_dist", v.min_candidate_dist, -1.0);
  nh.param("frontier/min_view_finish_fraction", v.min_view_finish_fraction, -1.0);
  nh.param("perception_utils/top_angle", v.top_angle, -1.0);
  nh.param("perception_utils/left_angle", v.left_angle, -1.0);
  nh.param("perception_utils/right_angle", v.right_angle, -1.0);
  nh.param("perception_utils/max_dist", v.max_dist, -1.0);
  min_candidate_dist_ = v.min_candidate_dist;
  have_viewpoints_ = c.split && dev_ && v.candidate_rnum > 0 && v.candidate_dphi > 0.0 && v.max_dist > 0.0;
  if (have_viewpoints_) warn("fuelmi_frontier_set_viewpoint_cfg", fuelmi_frontier_set_viewpoint_cfg(dev_, &v));
}
FrontierFinder::~FrontierFinder() {
  if (tsp_) fuelmi_tsp_destroy(tsp_);
  if (dev_) fuelmi_frontier_destroy(dev_);
}

// host copies of the device list `which`, from position `from` on (from = 0 replaces `out`)
void FrontierFinder::pull(int which, list<Frontier>& out, int from) {
  if (from == 0) {
    for (Frontier& old : out)  // (large cell buffers stay mapped for the clusters about to be built)
      if (old.cells_.capacity() >= 4096 && cells_spare_.size() < 8) cells_spare_.emplace_back(std::move(old.cells_));
    out.clear();
  }
  const int n = fuelmi_frontier_count(dev_, which);
  static_assert(sizeof(Vector3d) == 3 * sizeof(double), "cells_ is written as packed doubles");
  for (int k = from; k < n; ++k) {
    out.emplace_back();
    Frontier& f = out.back();  // (built in place: a 140 k-cell cluster is 3.4 MB, a copy of it a third of a plan cycle)
    const int sz = fuelmi_frontier_cluster_size(dev_, which, k);
    if (sz >= 4096) {  // the smallest spare buffer that holds the cluster
      int pick = -1;
      for (int i = 0; i < (int)cells_spare_.size(); ++i)
        if ((int)cells_spare_[i].capacity() >= sz && (pick < 0 || cells_spare_[i].capacity() < cells_spare_[pick].capacity())) pick = i;
      if (pick >= 0) {
        f.cells_.swap(cells_spare_[pick]);
        cells_spare_.erase(cells_spare_.begin() + pick);
      }
    }
    f.cells_.resize(sz);
    // voxel centres straight into the vector's storage (the library decodes them from its pinned result block)
    if (sz > 0) warn("fuelmi_frontier_cluster_centres", fuelmi_frontier_cluster_centres(dev_, which, k, f.cells_[0].data()));
    double info[9];
    fuelmi_frontier_cluster_info(dev_, which, k, info);
    for (int i = 0; i < 3; ++i) f.average_(i) = info[i], f.box_min_(i) = info[3 + i], f.box_max_(i) = info[6 + i];
    const int nf = fuelmi_frontier_cluster_filtered_size(dev_, which, k);
    if (nf > 0) {
      std::vector<float> xyz(3 * (size_t)nf);
      fuelmi_frontier_cluster_filtered(dev_, which, k, xyz.data());
      f.filtered_cells_.resize(nf);
      for (int i = 0; i < nf; ++i) f.filtered_cells_[i] = Vector3d(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    }
    const int nvp = fuelmi_frontier_viewpoint_count(dev_, which, k);
    if (nvp > 0) {
      std::vector<double> py(4 * (size_t)nvp);
      std::vector<int> vis(nvp);
      fuelmi_frontier_viewpoints(dev_, which, k, py.data(), vis.data());
      f.viewpoints_.resize(nvp);
      for (int i = 0; i < nvp; ++i) {
        f.viewpoints_[i].pos_ = Vector3d(py[4 * i], py[4 * i + 1], py[4 * i + 2]);
        f.viewpoints_[i].yaw_ = py[4 * i + 3];
        f.viewpoints_[i].visib_num_ = vis[i];
      }
    }
    f.id_ = k;
  }
}

void FrontierFinder::searchFrontiers() {
  int n_new = 0;
  warn("fuelmi_frontier_search", fuelmi_frontier_search(dev_, &n_new));
  {
    // frontier/reference_order = 2 answers per search: say so the first time a search is delivered in the address
    // order instead of the reference's (a cluster too large for the in-LDS level sweep) -- never silently
    int os[4] = {0, 0, 0, 0};
    if (fuelmi_frontier_order_stats(dev_, os) == 0 && os[2] > 0 && !order_fallback_logged_) {
      order_fallback_logged_ = true;
      std::fprintf(stderr, "[fuelmi facade] FrontierFinder: search delivered in ascending-address cell order, not the "
                   "reference's BFS order: a cluster of %d cells exceeds the in-LDS level sweep (frontier/reference_order = 2; "
                   "set it to 1 to pay for the order on every search).  Further fallbacks are counted, not logged: "
                   "fuelmi_frontier_order_stats.\n", os[3]);
    }
  }
  pull(0, tmp_frontiers_);
  removed_ids_.resize(fuelmi_frontier_removed_count(dev_));
  if (!removed_ids_.empty()) fuelmi_frontier_removed_ids(dev_, removed_ids_.data());
  // clusters dropped as "changed" leave the persistent list; the survivors keep their records (and with
  // them costs_ / paths_).  removed_ids_ are positions in the list as it shrinks (:74-85).
  for (int id : removed_ids_) {
    if (id < 0 || id >= (int)frontiers_.size()) break;
    auto it = frontiers_.begin();
    std::advance(it, id);
    frontiers_.erase(it);
  }
  if ((int)frontiers_.size() != fuelmi_frontier_count(dev_, 1)) pull(1, frontiers_);  // lists out of step: start over
  first_new_ftr_ = frontiers_.end();
  pull(2, dormant_frontiers_);
}

void FrontierFinder::computeFrontiersToVisit() {
  const int before = (int)frontiers_.size();
  if (have_viewpoints_) {
    // reference (:392-423): sampleViewpoints per new cluster on the device; clusters with viewpoints
    // join frontiers_ (viewpoints sorted by coverage), the others dormant_frontiers_
    int na = 0, nd = 0;
    warn("fuelmi_frontier_compute_to_visit", fuelmi_frontier_compute_to_visit(dev_, &na, &nd));
    pull(1, frontiers_, before);
    pull(2, dormant_frontiers_);
  } else {
    // without the viewpoint parameters every new cluster becomes an active frontier
    warn("fuelmi_frontier_commit", fuelmi_frontier_commit(dev_, 0));
    frontiers_.insert(frontiers_.end(), tmp_frontiers_.begin(), tmp_frontiers_.end());
  }
  first_new_ftr_ = frontiers_.begin();
  std::advance(first_new_ftr_, std::min(before, (int)frontiers_.size()));
  int id = 0;
  for (auto& f : frontiers_) f.id_ = id++;  // :417-419
}

// ---- tour planning: the reference's bookkeeping (frontier_finder.cpp:258-324, 507-589) on the host lists;
// path costs come from the package's own ViewNode (A* through the map), or with frontier/device_path_cost from
// fuelmi_map_path_costs in one call per method
void FrontierFinder::devicePaths(const vector<Vector3d>& p1, const vector<Vector3d>& p2, vector<double>& length,
                                 vector<vector<Vector3d>>* paths) {
  const int n = (int)p1.size();
  length.assign(n, 0.0);
  if (paths) paths->assign(n, {});
  if (n == 0) return;
  vector<double> a(3 * (size_t)n), b(3 * (size_t)n), xyz;
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) a[3 * i + k] = p1[i](k), b[3 * i + k] = p2[i](k);
  vector<int> kind(n), plen(n);
  fuelmi_path_cfg c;
  c.lattice_res = 0.4;  // graph_node.cpp:49
  c.edge_step = 0.1;    // astar2.cpp:105
  c.no_path_cost = 1000.0;  // graph_node.cpp:60
  c.max_path_points = paths ? 256 : 0;
  fuelmi_map* m = edt_env_->sdf_map_->device();
  int rc = FUELMI_OK;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (paths) xyz.assign((size_t)n * c.max_path_points * 3, 0.0);
    rc = fuelmi_map_path_costs(m, &c, n, a.data(), b.data(), length.data(), kind.data(), plen.data(),
                               paths ? xyz.data() : nullptr);
    if (rc != FUELMI_ELIMIT || !paths) break;
    c.max_path_points = *std::max_element(plen.begin(), plen.end());  // every path_len is filled: grow once
  }
  warn("fuelmi_map_path_costs", rc);
  if (!paths || rc != FUELMI_OK) return;
  for (int i = 0; i < n; ++i) {
    auto& P = (*paths)[i];
    P.resize(plen[i]);
    const double* q = xyz.data() + (size_t)i * c.max_path_points * 3;
    for (int r = 0; r < plen[i]; ++r) P[r] = Vector3d(q[3 * r], q[3 * r + 1], q[3 * r + 2]);
  }
}

double FrontierFinder::hostCost(double length, const Vector3d& p1, const Vector3d& p2, double y1, double y2,
                                const Vector3d& v1) const {  // graph_node.cpp:63-88
  double pos_cost = length / vm_;
  if (v1.norm() > 1e-3) {
    Vector3d dir = (p2 - p1).normalized();
    Vector3d vdir = v1.normalized();
    double diff = acos(vdir.dot(dir));
    pos_cost += w_dir_ * diff;
  }
  double diff = fabs(y2 - y1);
  diff = std::min(diff, 2 * M_PI - diff);
  double yaw_cost = diff / yd_;
  return std::max(pos_cost, yaw_cost);
}

void FrontierFinder::updateFrontierCostMatrix() {
  if (!removed_ids_.empty()) {
    // every surviving old cluster forgets its entries towards the removed ones
    for (auto it = frontiers_.begin(); it != first_new_ftr_; ++it)
      for (int id : removed_ids_) {
        if (id < 0 || id >= (int)it->costs_.size()) break;
        auto c = it->costs_.begin();
        auto p = it->paths_.begin();
        std::advance(c, id);
        std::advance(p, id);
        it->costs_.erase(c);
        it->paths_.erase(p);
      }
    removed_ids_.clear();
  }
  // best viewpoint to best viewpoint, stored in both records (the way back is the same path reversed)
  auto link = [](Frontier& a, Frontier& b) {
    const Viewpoint& va = a.viewpoints_.front();
    const Viewpoint& vb = b.viewpoints_.front();
    vector<Vector3d> path;
    const double cost = ViewNode::computeCost(va.pos_, vb.pos_, va.yaw_, vb.yaw_, Vector3d(0, 0, 0), 0, path);
    a.costs_.push_back(cost);
    a.paths_.push_back(path);
    std::reverse(path.begin(), path.end());
    b.costs_.push_back(cost);
    b.paths_.push_back(path);
  };
  if (device_path_cost_) {
    // every link of the cycle in ONE call, in the order the loops below consume them.  An old x new link is searched
    // from the new viewpoint (its lattice anchored there; sources are few per cycle) and the old record stores the
    // reversed path; a new x new link from the first of the two, as the reference does
    vector<Vector3d> p1, p2;
    for (auto old = frontiers_.begin(); old != first_new_ftr_; ++old)
      for (auto fresh = first_new_ftr_; fresh != frontiers_.end(); ++fresh)
        p1.push_back(fresh->viewpoints_.front().pos_), p2.push_back(old->viewpoints_.front().pos_);
    for (auto a = first_new_ftr_; a != frontiers_.end(); ++a) {
      auto b = a;
      for (++b; b != frontiers_.end(); ++b)
        p1.push_back(a->viewpoints_.front().pos_), p2.push_back(b->viewpoints_.front().pos_);
    }
    vector<double> len;
    vector<vector<Vector3d>> paths;
    devicePaths(p1, p2, len, &paths);
    size_t k = 0;
    // a's record gets the path a -> b, b's the reverse; `from_b`: the device path runs b -> a
    auto store = [&](Frontier& a, Frontier& b, bool from_b) {
      const Viewpoint& va = a.viewpoints_.front();
      const Viewpoint& vb = b.viewpoints_.front();
      const double cost = hostCost(len[k], va.pos_, vb.pos_, va.yaw_, vb.yaw_, Vector3d(0, 0, 0));
      vector<Vector3d> path = paths[k++];
      if (from_b) std::reverse(path.begin(), path.end());
      a.costs_.push_back(cost);
      a.paths_.push_back(path);
      std::reverse(path.begin(), path.end());
      b.costs_.push_back(cost);
      b.paths_.push_back(path);
    };
    for (auto old = frontiers_.begin(); old != first_new_ftr_; ++old)
      for (auto fresh = first_new_ftr_; fresh != frontiers_.end(); ++fresh) store(*old, *fresh, true);
    for (auto a = first_new_ftr_; a != frontiers_.end(); ++a) {
      a->costs_.push_back(0);
      a->paths_.push_back({});
      auto b = a;
      for (++b; b != frontiers_.end(); ++b) store(*a, *b, false);
    }
    first_new_ftr_ = frontiers_.end();
    return;
  }
  for (auto old = frontiers_.begin(); old != first_new_ftr_; ++old)
    for (auto fresh = first_new_ftr_; fresh != frontiers_.end(); ++fresh) link(*old, *fresh);
  for (auto a = first_new_ftr_; a != frontiers_.end(); ++a) {
    a->costs_.push_back(0);  // itself
    a->paths_.push_back({});
    auto b = a;
    for (++b; b != frontiers_.end(); ++b) link(*a, *b);
  }
  first_new_ftr_ = frontiers_.end();  // everything is linked now
}

void FrontierFinder::getFullCostMatrix(const Vector3d& cur_pos, const Vector3d& cur_vel, const Vector3d cur_yaw,
                                       Eigen::MatrixXd& mat) {
  // asymmetric TSP (:561-588): row/column 0 = the current state, nothing leads back to it
  const int n = (int)frontiers_.size();
  mat.resize(n + 1, n + 1);
  int i = 1;
  for (auto& ftr : frontiers_) {
    int j = 1;
    for (double cs : ftr.costs_) mat(i, j++) = cs;
    ++i;
  }
  mat.leftCols<1>().setZero();
  if (device_path_cost_) {  // row 0 in one call
    vector<Vector3d> p1, p2;
    for (auto& ftr : frontiers_) p1.push_back(cur_pos), p2.push_back(ftr.viewpoints_.front().pos_);
    vector<double> len;
    devicePaths(p1, p2, len, nullptr);
    int j = 1;
    for (auto& ftr : frontiers_) {
      const Viewpoint& v = ftr.viewpoints_.front();
      mat(0, j) = hostCost(len[j - 1], cur_pos, v.pos_, cur_yaw[0], v.yaw_, cur_vel);
      ++j;
    }
    return;
  }
  int j = 1;
  for (auto& ftr : frontiers_) {
    const Viewpoint& v = ftr.viewpoints_.front();
    vector<Vector3d> path;
    mat(0, j++) = ViewNode::computeCost(cur_pos, v.pos_, cur_yaw[0], v.yaw_, cur_vel, cur_yaw[1], path);
  }
}

void FrontierFinder::getPathForTour(const Vector3d& pos, const vector<int>& frontier_ids, vector<Vector3d>& path) {
  if (frontier_ids.empty()) return;
  vector<list<Frontier>::iterator> at;
  for (auto it = frontiers_.begin(); it != frontiers_.end(); ++it) at.push_back(it);
  vector<Vector3d> segment;
  if (device_path_cost_) {  // the first leg in one call
    vector<double> len;
    vector<vector<Vector3d>> legs;
    devicePaths({pos}, {at[frontier_ids[0]]->viewpoints_.front().pos_}, len, &legs);
    segment = legs[0];
  } else {
    ViewNode::searchPath(pos, at[frontier_ids[0]]->viewpoints_.front().pos_, segment);
  }
  path.insert(path.end(), segment.begin(), segment.end());
  for (size_t k = 0; k + 1 < frontier_ids.size(); ++k) {  // stored path from tour stop k to stop k+1
    auto p = at[frontier_ids[k]]->paths_.begin();
    std::advance(p, frontier_ids[k + 1]);
    path.insert(path.end(), p->begin(), p->end());
  }
}

bool FrontierFinder::findGlobalTour(const Vector3d& cur_pos, const Vector3d& cur_vel, const Vector3d cur_yaw,
                                    vector<int>& indices, vector<Vector3d>* global_tour) {
  updateFrontierCostMatrix();
  Eigen::MatrixXd mat;
  getFullCostMatrix(cur_pos, cur_vel, cur_yaw, mat);
  const int d = (int)mat.rows();
  // int int_cost = cost_mat(i, j) * scale (:368-374), refused where that conversion is undefined
  vector<int32_t> c((size_t)d * d);
  for (int i = 0; i < d; ++i)
    for (int j = 0; j < d; ++j) {
      const double x = mat(i, j) * 100;
      if (!std::isfinite(x) || std::fabs(x) >= 2147483648.0) {
        std::fprintf(stderr, "[fuelmi facade] FrontierFinder::findGlobalTour: cost (%d, %d) = %g has no int value\n", i,
                     j, mat(i, j));
        return false;
      }
      c[(size_t)i * d + j] = (int32_t)x;
    }
  if (!tsp_) {
    const fuelmi_tsp_cfg cfg = {FUELMI_TSP_DEFAULT_RESTARTS, FUELMI_TSP_DEFAULT_KICKS, FUELMI_TSP_DEFAULT_EXACT_MAX, 0};
    const int rc = fuelmi_tsp_create(edt_env_->sdf_map_->hipDevice(), &cfg, &tsp_);
    warn("fuelmi_tsp_create", rc);
    if (rc != FUELMI_OK) return false;
  }
  const int dim_ptr[2] = {0, d};
  vector<int> order(d);
  int64_t cost = 0;
  int method = 0;
  const int rc = fuelmi_tsp_solve(tsp_, 1, dim_ptr, c.data(), order.data(), &cost, &method);
  warn("fuelmi_tsp_solve", rc);
  if (rc != FUELMI_OK) return false;
  indices.clear();
  for (int k = 1; k < d; ++k) indices.push_back(order[k] - 1);
  if (global_tour) {
    global_tour->clear();
    getPathForTour(cur_pos, indices, *global_tour);
  }
  return true;
}

bool FrontierFinder::deviceRefine(const Vector3d& cur_pos, const Vector3d& cur_vel, double cur_yaw,
                                  const vector<vector<Vector3d>>& n_points, const vector<vector<double>>& n_yaws,
                                  int flags, vector<int>& choice, vector<Vector3d>* tour) {
  if (!(vm_ > 0.0 && yd_ > 0.0 && w_dir_ >= 0.0)) {
    std::fprintf(stderr, "[fuelmi facade] FrontierFinder::refineLocalTour needs exploration/vm, exploration/yd and "
                 "exploration/w_dir (vm %g, yd %g, w_dir %g)\n", vm_, yd_, w_dir_);
    return false;
  }
  if (n_points.empty() || n_points.size() != n_yaws.size()) {
    std::fprintf(stderr, "[fuelmi facade] FrontierFinder::refineLocalTour: %zu layers of points, %zu of yaws\n",
                 n_points.size(), n_yaws.size());
    return false;
  }
  const int L = (int)n_points.size();
  double start[7] = {cur_pos(0), cur_pos(1), cur_pos(2), cur_vel(0), cur_vel(1), cur_vel(2), cur_yaw};
  int layer_ptr[2] = {0, L};
  vector<int> node_ptr(1, 0);
  vector<double> nodes;
  for (int i = 0; i < L; ++i) {
    if (n_points[i].size() != n_yaws[i].size()) {
      std::fprintf(stderr, "[fuelmi facade] FrontierFinder::refineLocalTour: layer %d has %zu points, %zu yaws\n", i,
                   n_points[i].size(), n_yaws[i].size());
      return false;
    }
    for (size_t j = 0; j < n_points[i].size(); ++j) {
      for (int k = 0; k < 3; ++k) nodes.push_back(n_points[i][j](k));
      nodes.push_back(n_yaws[i][j]);
    }
    node_ptr.push_back(node_ptr.back() + (int)n_points[i].size());
  }
  fuelmi_refine_cfg c;
  c.path.lattice_res = 0.4;     // graph_node.cpp:49
  c.path.edge_step = 0.1;       // astar2.cpp:105
  c.path.no_path_cost = 1000.0;  // graph_node.cpp:60
  c.path.max_path_points = 0;
  c.vm = vm_, c.yd = yd_, c.w_dir = w_dir_;
  c.tour_lattice_res = tour ? 0.2 : 0.0;  // fast_exploration_manager.cpp:491
  c.max_tour_points = 1024;
  c.flags = flags;
  choice.assign(L, -1);
  double cost = 0.0;
  int tlen = 0;
  vector<double> xyz;
  fuelmi_map* m = edt_env_->sdf_map_->device();
  int rc = FUELMI_OK;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (tour) xyz.assign((size_t)c.max_tour_points * 3, 0.0);
    rc = fuelmi_map_refine_tours(m, &c, 1, start, layer_ptr, node_ptr.data(), nodes.data(), choice.data(), &cost,
                                 tour ? &tlen : nullptr, tour ? xyz.data() : nullptr);
    if (rc != FUELMI_ELIMIT || !tour || tlen <= c.max_tour_points) break;
    c.max_tour_points = tlen;  // tour_len holds the full count: grow once
  }
  warn("fuelmi_map_refine_tours", rc);
  if (rc != FUELMI_OK) return false;
  if (tour) {
    tour->resize(tlen);
    for (int r = 0; r < tlen; ++r) (*tour)[r] = Vector3d(xyz[3 * r], xyz[3 * r + 1], xyz[3 * r + 2]);
  }
  if (choice[0] < 0) {
    std::fprintf(stderr, "[fuelmi facade] FrontierFinder::refineLocalTour: the last layer is not reachable\n");
    return false;
  }
  return true;
}

bool FrontierFinder::refineLocalTour(const Vector3d& cur_pos, const Vector3d& cur_vel, const Vector3d& cur_yaw,
                                     const vector<vector<Vector3d>>& n_points, const vector<vector<double>>& n_yaws,
                                     vector<Vector3d>& refined_pts, vector<double>& refined_yaws,
                                     vector<Vector3d>* refined_tour) {  // fast_exploration_manager.cpp:429-503
  vector<int> choice;
  if (!deviceRefine(cur_pos, cur_vel, cur_yaw(0), n_points, n_yaws, 0, choice, refined_tour)) return false;
  for (size_t i = 0; i < choice.size(); ++i) {
    refined_pts.push_back(n_points[i][choice[i]]);
    refined_yaws.push_back(n_yaws[i][choice[i]]);
  }
  return true;
}

bool FrontierFinder::refineSingleDestination(const Vector3d& cur_pos, const Vector3d& cur_vel, const Vector3d& cur_yaw,
                                             const vector<Vector3d>& points, const vector<double>& yaws,
                                             int& min_cost_id) {  // fast_exploration_manager.cpp:197-208
  vector<int> choice;
  min_cost_id = -1;
  if (!deviceRefine(cur_pos, cur_vel, cur_yaw(0), {points}, {yaws}, FUELMI_REFINE_LAST_ARGMIN, choice, nullptr))
    return false;
  min_cost_id = choice[0];
  return true;
}

int FrontierFinder::planPathToViewpoint(const Vector3d& cur_pos, const Vector3d& next_pos,
                                        vector<Vector3d>& path_next_goal, Vector3d& next_goal) {
  // fast_exploration_manager.cpp:234-276
  fuelmi_goal_cfg c;
  c.path.lattice_res = 0.2;  // astar/resolution_astar (algorithm.xml)
  c.path.edge_step = 0.1;    // astar2.cpp:105
  c.path.no_path_cost = 0.0;
  c.path.max_path_points = 2048;
  c.shorten_dist = 3.0;  // :301
  c.end_eps = 1e-3;      // :319
  c.radius_close = 1.5;  // :243
  c.radius_far = 5.0;    // :242
  c.max_way_points = 64;
  const double s[3] = {cur_pos(0), cur_pos(1), cur_pos(2)}, g[3] = {next_pos(0), next_pos(1), next_pos(2)};
  int status = -1, n_way = 0, raw_len = 0, rc = FUELMI_OK;
  double length = 0.0, ng[3] = {g[0], g[1], g[2]};
  vector<double> way;
  fuelmi_map* m = edt_env_->sdf_map_->device();
  for (int attempt = 0; attempt < 2; ++attempt) {
    way.assign((size_t)c.max_way_points * 3, 0.0);
    rc = fuelmi_map_goal_paths(m, &c, 1, s, g, &status, &length, &n_way, way.data(), ng, &raw_len, nullptr);
    if (rc != FUELMI_ELIMIT) break;
    c.path.max_path_points = std::max(c.path.max_path_points, raw_len);  // both hold the full counts: grow once
    c.max_way_points = std::max(c.max_way_points, n_way);
  }
  warn("fuelmi_map_goal_paths", rc);
  path_next_goal.clear();
  if (rc != FUELMI_OK) return GOAL_ERROR;
  next_goal = Vector3d(ng[0], ng[1], ng[2]);
  if (status == FUELMI_GOAL_NO_PATH) {
    std::fprintf(stderr, "[fuelmi facade] FrontierFinder::planPathToViewpoint: no path to the next viewpoint\n");
    return GOAL_NO_PATH;
  }
  for (int r = 0; r < n_way; ++r) path_next_goal.push_back(Vector3d(way[3 * r], way[3 * r + 1], way[3 * r + 2]));
  return status;
}

void FrontierFinder::setNextFrontier(const int& id) {  // declared by the reference, never defined there
  for (auto& ftr : frontiers_)
    if (ftr.id_ == id) next_frontier_ = ftr;
}

void FrontierFinder::getTopViewpointsInfo(const Vector3d& cur_pos, vector<Vector3d>& points, vector<double>& yaws,
                                          vector<Vector3d>& averages) {  // :425-450
  points.clear();
  yaws.clear();
  averages.clear();
  for (auto& frontier : frontiers_) {
    if (frontier.viewpoints_.empty()) continue;
    const Viewpoint* pick = &frontier.viewpoints_.front();  // all close: the best one
    for (auto& view : frontier.viewpoints_) {
      if ((view.pos_ - cur_pos).norm() < min_candidate_dist_) continue;
      pick = &view;
      break;
    }
    points.push_back(pick->pos_);
    yaws.push_back(pick->yaw_);
    averages.push_back(frontier.average_);
  }
}

void FrontierFinder::getViewpointsInfo(const Vector3d& cur_pos, const vector<int>& ids, const int& view_num,
                                       const double& max_decay, vector<vector<Vector3d>>& points,
                                       vector<vector<double>>& yaws) {  // :452-487
  points.clear();
  yaws.clear();
  for (auto id : ids) {
    for (auto& frontier : frontiers_) {
      if (frontier.id_ != id || frontier.viewpoints_.empty()) continue;
      vector<Vector3d> pts;
      vector<double> ys;
      const int visib_thresh = frontier.viewpoints_.front().visib_num_ * max_decay;
      for (auto& view : frontier.viewpoints_) {
        if ((int)pts.size() >= view_num || view.visib_num_ <= visib_thresh) break;
        if ((view.pos_ - cur_pos).norm() < min_candidate_dist_) continue;
        pts.push_back(view.pos_);
        ys.push_back(view.yaw_);
      }
      if (pts.empty()) {  // all viewpoints are very close: take them regardless of the distance
        for (auto& view : frontier.viewpoints_) {
          if ((int)pts.size() >= view_num || view.visib_num_ <= visib_thresh) break;
          pts.push_back(view.pos_);
          ys.push_back(view.yaw_);
        }
      }
      points.push_back(pts);
      yaws.push_back(ys);
    }
  }
}

bool FrontierFinder::isFrontierCovered() {  // :697-719
  int covered = 0;
  warn("fuelmi_frontier_is_covered", fuelmi_frontier_is_covered(dev_, &covered));
  return covered != 0;
}

void FrontierFinder::getFrontiers(vector<vector<Vector3d>>& clusters) {
  clusters.clear();
  for (auto& f : frontiers_) clusters.push_back(f.cells_);
}
void FrontierFinder::getDormantFrontiers(vector<vector<Vector3d>>& clusters) {
  clusters.clear();
  for (auto& f : dormant_frontiers_) clusters.push_back(f.cells_);
}
void FrontierFinder::getFrontierBoxes(vector<pair<Vector3d, Vector3d>>& boxes) {
  boxes.clear();
  for (auto& f : frontiers_) boxes.push_back(std::make_pair((f.box_max_ + f.box_min_) * 0.5, f.box_max_ - f.box_min_));
}
void FrontierFinder::wrapYaw(double& yaw) {
  while (yaw < -M_PI) yaw += 2 * M_PI;
  while (yaw > M_PI) yaw -= 2 * M_PI;
}

// ------------------------------------------------------------------------------------------------
// BsplineOptimizer
// ------------------------------------------------------------------------------------------------
const int BsplineOptimizer::SMOOTHNESS = FUELMI_COST_SMOOTHNESS;
const int BsplineOptimizer::DISTANCE = FUELMI_COST_DISTANCE;
const int BsplineOptimizer::FEASIBILITY = FUELMI_COST_FEASIBILITY;
const int BsplineOptimizer::START = FUELMI_COST_START;
const int BsplineOptimizer::END = FUELMI_COST_END;
const int BsplineOptimizer::GUIDE = FUELMI_COST_GUIDE;
const int BsplineOptimizer::WAYPOINTS = FUELMI_COST_WAYPOINTS;
const int BsplineOptimizer::VIEWCONS = FUELMI_COST_VIEWCONS;
const int BsplineOptimizer::MINTIME = FUELMI_COST_MINTIME;
const int BsplineOptimizer::GUIDE_PHASE =
    BsplineOptimizer::SMOOTHNESS | BsplineOptimizer::GUIDE | BsplineOptimizer::START | BsplineOptimizer::END;
const int BsplineOptimizer::NORMAL_PHASE = BsplineOptimizer::SMOOTHNESS | BsplineOptimizer::DISTANCE |
    BsplineOptimizer::FEASIBILITY | BsplineOptimizer::START | BsplineOptimizer::END;

void BsplineOptimizer::setParam(ros::NodeHandle& nh) {
  nh.param("optimization/ld_smooth", cfg_.ld_smooth, -1.0);
  nh.param("optimization/ld_dist", cfg_.ld_dist, -1.0);
  nh.param("optimization/ld_feasi", cfg_.ld_feasi, -1.0);
  nh.param("optimization/ld_start", cfg_.ld_start, -1.0);
  nh.param("optimization/ld_end", cfg_.ld_end, -1.0);
  nh.param("optimization/ld_guide", cfg_.ld_guide, -1.0);
  nh.param("optimization/ld_waypt", cfg_.ld_waypt, -1.0);
  nh.param("optimization/ld_view", cfg_.ld_view, -1.0);
  nh.param("optimization/ld_time", cfg_.ld_time, -1.0);
  nh.param("optimization/dist0", cfg_.dist0, -1.0);
  nh.param("optimization/max_vel", cfg_.max_vel, -1.0);
  nh.param("optimization/max_acc", cfg_.max_acc, -1.0);
  nh.param("optimization/dlmin", cfg_.dlmin, -1.0);
  nh.param("optimization/wnl", cfg_.wnl, -1.0);
  const char* nums[4] = {"optimization/max_iteration_num1", "optimization/max_iteration_num2",
                         "optimization/max_iteration_num3", "optimization/max_iteration_num4"};
  const char* times[4] = {"optimization/max_iteration_time1", "optimization/max_iteration_time2",
                          "optimization/max_iteration_time3", "optimization/max_iteration_time4"};
  for (int i = 0; i < 4; ++i) {
    nh.param(nums[i], max_iteration_num_[i], -1);
    nh.param(times[i], max_iteration_time_[i], -1.0);
  }
  nh.param("optimization/algorithm1", algorithm1_, -1);
  nh.param("optimization/algorithm2", algorithm2_, -1);
  nh.param("manager/bspline_degree", bspline_degree_, 3);
  cfg_.bspline_degree = bspline_degree_;
  nh.param("optimization/exact_quadratic", exact_quadratic_, false);
  time_lb_ = -1;
  static bool told = false;
  if (!told && (algorithm1_ >= 0 || algorithm2_ >= 0)) {
    told = true;
    std::fprintf(stderr,
                 "[fuelmi] BsplineOptimizer: optimization/algorithm1,2 (NLopt ids %d, %d) are not used -- every solve is "
                 "one device launch of a box-projected L-BFGS under max_iteration_num* and max_iteration_time*\n",
                 algorithm1_, algorithm2_);
  }
}

void BsplineOptimizer::setEnvironment(const shared_ptr<EDTEnvironment>& env) {
  edt_environment_ = env;
  dynamic_ = false;
}
void BsplineOptimizer::setCostFunction(const int& cost_code) { cost_function_ = cost_code; }
void BsplineOptimizer::setGuidePath(const vector<Eigen::Vector3d>& guide_pt) { guide_pts_ = guide_pt; }
void BsplineOptimizer::setWaypoints(const vector<Eigen::Vector3d>& waypts, const vector<int>& waypt_idx) {
  waypoints_ = waypts;
  waypt_idx_ = waypt_idx;
}
void BsplineOptimizer::setViewConstraint(const ViewConstraint& vc) { view_cons_ = vc; }
void BsplineOptimizer::enableDynamic(double time_start) {
  dynamic_ = true;  // moving obstacles are out of scope: the static ESDF is used regardless
  start_time_ = time_start;
}
void BsplineOptimizer::setBoundaryStates(const vector<Eigen::Vector3d>& start, const vector<Eigen::Vector3d>& end) {
  start_state_ = start;
  end_state_ = end;
}
void BsplineOptimizer::setTimeLowerBound(const double& lb) { time_lb_ = lb; }

namespace {
struct BatchStore {  // keeps the arrays a one-candidate fuelmi_bspline_batch points to
  std::vector<double> st, en, guide, wp, vpt, vdir;
  double tlb;
};
}  // namespace
// one-candidate batch from the optimiser's members (what combineCost reads, :518-691)
#define FUELMI_FILL_BATCH(b, S, XV)                                                                      \
  S.st.assign(9, 0.0), S.en.assign(9, 0.0), S.vpt.assign(3, 0.0), S.vdir.assign(3, 0.0);                 \
  for (size_t i = 0; i < start_state_.size() && i < 3; ++i)                                              \
    for (int k = 0; k < 3; ++k) S.st[3 * i + k] = start_state_[i](k);                                    \
  for (size_t i = 0; i < end_state_.size() && i < 3; ++i)                                                \
    for (int k = 0; k < 3; ++k) S.en[3 * i + k] = end_state_[i](k);                                      \
  for (auto& g : guide_pts_)                                                                             \
    for (int k = 0; k < 3; ++k) S.guide.push_back(g(k));                                                 \
  for (auto& w : waypoints_)                                                                             \
    for (int k = 0; k < 3; ++k) S.wp.push_back(w(k));                                                    \
  for (int k = 0; k < 3; ++k) S.vpt[k] = view_cons_.pt_(k), S.vdir[k] = view_cons_.dir_(k);              \
  S.tlb = time_lb_;                                                                                      \
  b.cost_function = cost_function_;                                                                      \
  b.dim = dim_;                                                                                          \
  b.point_num = point_num_;                                                                              \
  b.n_traj = 1;                                                                                          \
  b.x = (XV).data();                                                                                     \
  b.pt_dist = &pt_dist_;                                                                                 \
  b.knot_span = &knot_span_;                                                                             \
  b.time_lb = &S.tlb;                                                                                    \
  b.start_state = S.st.data();                                                                           \
  b.end_state = S.en.data();                                                                             \
  b.end_n = (int)std::max<size_t>(1, std::min<size_t>(3, end_state_.size()));                            \
  b.guide_pts = S.guide.empty() ? nullptr : S.guide.data();                                              \
  b.waypoints = S.wp.empty() ? nullptr : S.wp.data();                                                    \
  b.waypt_idx = waypt_idx_.empty() ? nullptr : waypt_idx_.data();                                        \
  b.n_waypt = (int)waypoints_.size();                                                                    \
  b.view_pt = S.vpt.data();                                                                              \
  b.view_dir = S.vdir.data();                                                                            \
  b.view_idx = &view_cons_.idx_;

void BsplineOptimizer::combineCost(const std::vector<double>& x, std::vector<double>& grad, double& cost) {
  auto t1 = std::chrono::steady_clock::now();
  fuelmi_bspline_batch b;
  BatchStore S;
  FUELMI_FILL_BATCH(b, S, x)
  grad.assign(variable_num_, 0.0);
  warn("fuelmi_bspline_cost_grad",
       fuelmi_bspline_cost_grad(edt_environment_->sdf_map_->device(), &cfg_, &b, &cost, grad.data()));
  comb_time += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
}

void BsplineOptimizer::optimize(Eigen::MatrixXd& points, double& dt, const int& cost_function,
                                const int& max_num_id, const int& max_time_id) {
  if (start_state_.empty()) {
    ROS_ERROR("Initial state undefined!");
    return;
  }
  control_points_ = points;
  knot_span_ = dt;
  max_num_id_ = max_num_id;
  max_time_id_ = max_time_id;
  setCostFunction(cost_function);
  dim_ = control_points_.cols();
  order_ = (dim_ == 1) ? 3 : bspline_degree_;
  point_num_ = control_points_.rows();
  optimize_time_ = cost_function_ & MINTIME;
  variable_num_ = optimize_time_ ? dim_ * point_num_ + 1 : dim_ * point_num_;
  if (variable_num_ <= 0) {
    ROS_ERROR("Empty varibale to optimization solver.");
    return;
  }
  pt_dist_ = 0.0;
  for (int i = 0; i < point_num_ - 1; ++i) {
    double s = 0.0;
    for (int j = 0; j < dim_; ++j) {
      const double e = control_points_(i + 1, j) - control_points_(i, j);
      s += e * e;
    }
    pt_dist_ += std::sqrt(s);
  }
  pt_dist_ /= double(point_num_);
  iter_num_ = 0;
  min_cost_ = std::numeric_limits<double>::max();
  comb_time = 0.0;
  optimize();
  points = control_points_;
  dt = knot_span_;
  start_state_.clear();
  time_lb_ = -1;
}

// Box-projected L-BFGS (memory 8, Armijo backtracking) under the reference's stopping criteria.
// Replaces nlopt::opt (bspline_optimizer.cpp:165-229); iterates are NOT NLopt's.
void BsplineOptimizer::optimize() {
  // The reference hands the variables to NLopt (:165-253).  Here the whole solve runs in one kernel
  // launch on the device (fuelmi_bspline_dev_optimize: start clamping, bounds, best-variable tracking,
  // evaluation cap and xtol_rel as the reference configures them; box-projected L-BFGS in place of
  // NLopt's LD_LBFGS / LD_TNEWTON).  max_iteration_time_ is the solver's wall-clock cap (set_maxtime, :170-172):
  // the device checks its clock between evaluations and returns the best variables seen when it runs out.
  exact_status_ = -1;
  if (exact_quadratic_ && solveExact()) return;
  const int n = variable_num_;
  std::vector<double> q(n);
  for (int i = 0; i < point_num_; ++i)
    for (int j = 0; j < dim_; ++j) q[dim_ * i + j] = control_points_(i, j);
  if (optimize_time_) q[n - 1] = knot_span_;
  auto t1 = std::chrono::steady_clock::now();
  fuelmi_bspline_batch b;
  BatchStore S;
  FUELMI_FILL_BATCH(b, S, q)
  // one call on a query slot of the map: no device allocation, own side stream -- the ten optimiser threads of
  // topoReplan (planner_manager.cpp:446-453) solve side by side
  best_variable_.assign(n, 0.0);
  double cost = 0.0;
  int evals = 0;
  const int rc = fuelmi_bspline_optimize(edt_environment_->sdf_map_->device(), &cfg_, &b, std::max(1, max_iteration_num_[max_num_id_]),
                                         max_iteration_time_[max_time_id_], best_variable_.data(), &cost, &evals);
  warn("fuelmi_bspline_optimize", rc);
  comb_time += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
  if (rc) return;
  iter_num_ = evals;
  min_cost_ = cost;
  for (int i = 0; i < point_num_; ++i)
    for (int j = 0; j < dim_; ++j) control_points_(i, j) = best_variable_[dim_ * i + j];
  if (optimize_time_) knot_span_ = best_variable_[n - 1];
}

// optimization/exact_quadratic: a mask whose every term is quadratic goes to fuelmi_map_solve_quadratic (one problem);
// anything but FUELMI_QUAD_OK leaves the problem to the iteration
bool BsplineOptimizer::solveExact() {
  const int quad = SMOOTHNESS | START | END | GUIDE | WAYPOINTS;
  if (cost_function_ == 0 || (cost_function_ & ~quad) || (dim_ != 1 && dim_ != 3)) return false;
  const int N = point_num_, dim = dim_, nw = (int)waypoints_.size();
  fuelmi_quad_cfg qc = {cost_function_, dim, N, (int)std::max<size_t>(1, std::min<size_t>(3, end_state_.size())), nw, dim == 3};
  std::vector<double> q((size_t)N * dim), st(3 * dim, 0.0), en(3 * dim, 0.0), guide, wp((size_t)nw * dim), out((size_t)N * dim);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < dim; ++j) q[dim * i + j] = control_points_(i, j);
  for (size_t i = 0; i < start_state_.size() && i < 3; ++i)
    for (int k = 0; k < dim; ++k) st[dim * i + k] = start_state_[i](k);
  for (size_t i = 0; i < end_state_.size() && i < 3; ++i)
    for (int k = 0; k < dim; ++k) en[dim * i + k] = end_state_[i](k);
  const int n_guide = std::max(N - 2 * order_, 0);
  if (cost_function_ & GUIDE) {
    if ((int)guide_pts_.size() < n_guide) return false;
    for (int i = 0; i < n_guide; ++i)
      for (int k = 0; k < dim; ++k) guide.push_back(guide_pts_[i](k));
  }
  for (int i = 0; i < nw; ++i)
    for (int k = 0; k < dim; ++k) wp[dim * i + k] = waypoints_[i](k);
  if ((cost_function_ & WAYPOINTS) && (int)waypt_idx_.size() < nw) return false;
  int status = -1;
  double cost = 0.0, ptd = 0.0;
  auto t1 = std::chrono::steady_clock::now();
  const int rc = fuelmi_map_solve_quadratic(edt_environment_->sdf_map_->device(), &cfg_, &qc, 1, &N, q.data(), &knot_span_,
                                            st.data(), en.data(), guide.empty() ? nullptr : guide.data(), &nw,
                                            wp.empty() ? nullptr : wp.data(), waypt_idx_.empty() ? nullptr : waypt_idx_.data(),
                                            &status, out.data(), &cost, &ptd);
  comb_time += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
  if (rc) return false;  // (an input the exact route refuses is the iteration's to judge)
  exact_status_ = status;
  if (status != FUELMI_QUAD_OK) return false;
  iter_num_ = 0;
  min_cost_ = cost;
  best_variable_ = out;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < dim; ++j) control_points_(i, j) = out[dim * i + j];
  return true;
}

bool BsplineOptimizer::optimizeGuidePhase(std::vector<Eigen::MatrixXd>& ctrl_pts, const std::vector<double>& dts,
                                          const std::vector<vector<Eigen::Vector3d>>& start,
                                          const std::vector<vector<Eigen::Vector3d>>& end,
                                          const std::vector<vector<Eigen::Vector3d>>& guide, std::vector<int>& status,
                                          std::vector<double>& cost) {
  const size_t n = ctrl_pts.size();
  if (dts.size() != n || start.size() != n || end.size() != n || guide.size() != n) return false;
  int maxc = 4, end_n = 3;
  for (size_t b = 0; b < n; ++b) {
    if (ctrl_pts[b].cols() != 3 || start[b].size() < 3 || end[b].empty()) return false;
    maxc = std::max(maxc, (int)ctrl_pts[b].rows());
    end_n = b ? end_n : (int)std::min<size_t>(3, end[b].size());
    if ((int)std::min<size_t>(3, end[b].size()) != end_n) return false;  // (one call shares the number of end rows)
    if ((int)guide[b].size() < (int)ctrl_pts[b].rows() - 2 * bspline_degree_) return false;
  }
  const size_t maxg = (size_t)std::max(maxc - 2 * bspline_degree_, 0);
  fuelmi_quad_cfg qc = {GUIDE_PHASE, 3, maxc, end_n, 0, 1};
  std::vector<int> nc(n), st_out(n);
  std::vector<double> q(n * maxc * 3, 0.0), st(n * 9, 0.0), en(n * 9, 0.0), g(n * maxg * 3 + 1, 0.0), out(n * maxc * 3), c(n), pd(n);
  for (size_t b = 0; b < n; ++b) {
    nc[b] = (int)ctrl_pts[b].rows();
    for (int i = 0; i < nc[b]; ++i)
      for (int k = 0; k < 3; ++k) q[(b * maxc + i) * 3 + k] = ctrl_pts[b](i, k);
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) {
        st[b * 9 + 3 * i + k] = start[b][i](k);
        if (i < end_n) en[b * 9 + 3 * i + k] = end[b][i](k);
      }
    for (int i = 0; i < nc[b] - 2 * bspline_degree_; ++i)
      for (int k = 0; k < 3; ++k) g[(b * maxg + i) * 3 + k] = guide[b][i](k);
  }
  if (n == 0) {
    status.clear(), cost.clear();
    return true;
  }
  const int rc = fuelmi_map_solve_quadratic(edt_environment_->sdf_map_->device(), &cfg_, &qc, (int)n, nc.data(), q.data(),
                                            dts.data(), st.data(), en.data(), g.data(), nullptr, nullptr, nullptr,
                                            st_out.data(), out.data(), c.data(), pd.data());
  if (rc) {
    warn("fuelmi_map_solve_quadratic", rc);
    return false;
  }
  for (size_t b = 0; b < n; ++b)
    if (st_out[b] == FUELMI_QUAD_OK)
      for (int i = 0; i < nc[b]; ++i)
        for (int k = 0; k < 3; ++k) ctrl_pts[b](i, k) = out[(b * maxc + i) * 3 + k];
  status = st_out, cost = c;
  return true;
}

int BsplineOptimizer::planThroughWaypoints(const vector<Eigen::Vector3d>& tour, const Eigen::Vector3d& cur_vel,
                                           const Eigen::Vector3d& cur_acc, double max_vel, double ctrl_pt_dist,
                                           int cost_mask, double time_lb, Eigen::MatrixXd& ctrl_pts, double& dt) {
  if (tour.empty()) {
    ROS_ERROR("Empty path to traj planner");
    return FUELMI_WPTRAJ_FEW;
  }
  fuelmi_map* m = edt_environment_->sdf_map_->device();
  const int n_way = (int)tour.size();
  std::vector<double> way(3 * (size_t)n_way);
  for (int i = 0; i < n_way; ++i)
    for (int k = 0; k < 3; ++k) way[3 * i + k] = tour[i](k);
  const double vel[3] = {cur_vel(0), cur_vel(1), cur_vel(2)}, acc[3] = {cur_acc(0), cur_acc(1), cur_acc(2)};
  // :270-297 -- the sample count is a result: a second call with room for it when the first guess was short
  fuelmi_wptraj_cfg wc = {max_vel, ctrl_pt_dist, 8, 0, n_way, 256};
  int status = 0, seg_num = 0, n_samples = 0;
  double duration = 0.0, length = 0.0, ts = 0.0, derivs[12];
  std::vector<double> samples;
  for (int pass = 0; pass < 2; ++pass) {
    samples.assign(3 * (size_t)wc.max_samples, 0.0);
    const int rc = fuelmi_map_waypoint_trajs(m, &wc, 1, &n_way, way.data(), vel, acc, &status, &duration, &length, &seg_num,
                                             &ts, &n_samples, samples.data(), derivs, nullptr, nullptr);
    if (rc == FUELMI_ELIMIT && status == -1 && pass == 0 && n_samples > wc.max_samples) {
      wc.max_samples = n_samples;
      continue;
    }
    if (rc) {
      warn("fuelmi_map_waypoint_trajs", rc);
      return rc;
    }
    break;
  }
  if (status != FUELMI_WPTRAJ_OK) return status;
  // :299-309
  const int rows = n_samples + bspline_degree_ - 1;
  std::vector<double> ctrl(3 * (size_t)rows), st(9), en(3);
  int rc = fuelmi_bspline_parameterize(m, 1, n_samples, bspline_degree_, &ts, samples.data(), derivs, ctrl.data());
  if (!rc) rc = fuelmi_bspline_boundary_states(m, 1, rows, bspline_degree_, &ts, ctrl.data(), 2, 0, st.data(), en.data());
  if (rc) {
    warn("planThroughWaypoints: spline fit", rc);
    return rc;
  }
  vector<Eigen::Vector3d> start, end;
  for (int i = 0; i < 3; ++i) start.push_back(Eigen::Vector3d(st[3 * i], st[3 * i + 1], st[3 * i + 2]));
  end.push_back(Eigen::Vector3d(en[0], en[1], en[2]));
  setBoundaryStates(start, end);
  if (time_lb > 0) setTimeLowerBound(time_lb);
  ctrl_pts = Eigen::MatrixXd(rows, 3);
  for (int i = 0; i < rows; ++i)
    for (int k = 0; k < 3; ++k) ctrl_pts(i, k) = ctrl[3 * i + k];
  dt = ts;
  init_ctrl_pts_ = ctrl_pts;
  init_knot_span_ = dt;
  optimize(ctrl_pts, dt, cost_mask, 1, 1);  // :312
  final_cost_ = min_cost_;
  return FUELMI_WPTRAJ_OK;
}

int BsplineOptimizer::planKinodynamic(const Eigen::Vector3d& start_pt, const Eigen::Vector3d& start_vel,
                                      const Eigen::Vector3d& start_acc, const Eigen::Vector3d& end_pt,
                                      const Eigen::Vector3d& end_vel, const fuelmi_kino_cfg& search, double max_vel,
                                      double ctrl_pt_dist, int cost_mask, double time_lb, Eigen::MatrixXd& ctrl_pts,
                                      double& dt) {
  fuelmi_map* m = edt_environment_->sdf_map_->device();
  const double sp[3] = {start_pt(0), start_pt(1), start_pt(2)}, sv[3] = {start_vel(0), start_vel(1), start_vel(2)};
  const double sa[3] = {start_acc(0), start_acc(1), start_acc(2)}, gp[3] = {end_pt(0), end_pt(1), end_pt(2)};
  const double gv[3] = {end_vel(0), end_vel(1), end_vel(2)};
  fuelmi_kino_cfg kc = search;
  kc.ts = ctrl_pt_dist / max_vel;  // :162
  kc.min_seg = 8, kc.seg_num = 0, kc.max_path_nodes = 1, kc.max_samples = 256;
  int status = 0, which = 0, iter = 0, use = 0, n_nodes = 0, shot = 0, seg_num = 0, n_samples = 0;
  double t_shot = 0.0, coef[12], T_sum = 0.0, ts = 0.0, derivs[12];
  std::vector<double> samples;
  // the sample count is a result: a second call with room for it when the first guess was short
  for (int pass = 0; pass < 2; ++pass) {
    samples.assign(3 * (size_t)kc.max_samples, 0.0);
    const int rc = fuelmi_map_kino_paths(m, &kc, 1, sp, sv, sa, gp, gv, &status, &which, &iter, &use, &n_nodes, nullptr,
                                         nullptr, nullptr, &shot, &t_shot, coef, &T_sum, &ts, &seg_num, &n_samples,
                                         samples.data(), derivs);
    if (rc == FUELMI_ELIMIT && status == -1 && pass == 0 && n_samples > kc.max_samples) {
      kc.max_samples = n_samples;
      continue;
    }
    if (rc) {
      warn("fuelmi_map_kino_paths", rc);
      return rc;
    }
    break;
  }
  kino_iter_num_ = iter, kino_use_node_num_ = use, kino_which_ = which;
  if (status == FUELMI_KINO_NO_PATH || status == FUELMI_KINO_CLOSE_GOAL) return status;
  // :171-184
  const int rows = n_samples + bspline_degree_ - 1;
  std::vector<double> ctrl(3 * (size_t)rows), st(9), en(3);
  int rc = fuelmi_bspline_parameterize(m, 1, n_samples, bspline_degree_, &ts, samples.data(), derivs, ctrl.data());
  if (!rc) rc = fuelmi_bspline_boundary_states(m, 1, rows, bspline_degree_, &ts, ctrl.data(), 2, 0, st.data(), en.data());
  if (rc) {
    warn("planKinodynamic: spline fit", rc);
    return rc;
  }
  vector<Eigen::Vector3d> start, end;
  for (int i = 0; i < 3; ++i) start.push_back(Eigen::Vector3d(st[3 * i], st[3 * i + 1], st[3 * i + 2]));
  end.push_back(Eigen::Vector3d(en[0], en[1], en[2]));
  setBoundaryStates(start, end);
  if (time_lb > 0) setTimeLowerBound(time_lb);
  ctrl_pts = Eigen::MatrixXd(rows, 3);
  for (int i = 0; i < rows; ++i)
    for (int k = 0; k < 3; ++k) ctrl_pts(i, k) = ctrl[3 * i + k];
  dt = ts;
  init_ctrl_pts_ = ctrl_pts;
  init_knot_span_ = dt;
  optimize(ctrl_pts, dt, cost_mask, 1, 1);
  final_cost_ = min_cost_;
  return status;
}

// one fuelmi_map_plan_yaws problem; the outputs are touched only when its status is FUELMI_YAW_OK
// a problem's whole knot vector for a _knots entry; false: not n_ctrl + degree + 1 of them
static bool knots_of(const Eigen::VectorXd& knots, int n_ctrl, int degree, std::vector<double>& u) {
  if ((int)knots.rows() != n_ctrl + degree + 1) return false;
  u.resize((size_t)knots.rows());
  for (int i = 0; i < (int)u.size(); ++i) u[i] = knots(i);
  return true;
}

// (knots null: the uniform spline of the span pos_dt; else the spline on those knots, pos_dt is not read)
static int plan_one_yaw(fuelmi_map* m, const fuelmi_bspline_cfg& w, const fuelmi_yaw_cfg& yc, const Eigen::MatrixXd& pos_ctrl,
                        double pos_dt, const Eigen::Vector3d& start_yaw, double end_yaw, Eigen::MatrixXd& yaw_ctrl,
                        double& dt_yaw, std::vector<double>* path_yaw, const Eigen::VectorXd* knots = nullptr) {
  const int n_ctrl = (int)pos_ctrl.rows();
  if (n_ctrl < 1 || pos_ctrl.cols() != 3) return FUELMI_EINVAL;
  std::vector<double> u;
  if (knots && !knots_of(*knots, n_ctrl, yc.pos_degree, u)) return FUELMI_EINVAL;
  std::vector<double> pos(3 * (size_t)n_ctrl);
  for (int i = 0; i < n_ctrl; ++i)
    for (int k = 0; k < 3; ++k) pos[3 * i + k] = pos_ctrl(i, k);
  const double start[3] = {start_yaw(0), start_yaw(1), start_yaw(2)};
  int status = 0, seg_num = 0, n_waypt = 0;
  double duration = 0.0, dt = 0.0, e = 0.0, cost = 0.0;
  std::vector<double> q((size_t)yc.max_seg + 3), wp((size_t)yc.max_seg);
  const int rc = knots ? fuelmi_map_plan_yaws_knots(m, &w, &yc, 1, &n_ctrl, pos.data(), u.data(), start, &end_yaw, &status,
                                                    &duration, &seg_num, &dt, q.data(), &n_waypt, wp.data(), &e, &cost,
                                                    nullptr, nullptr)
                       : fuelmi_map_plan_yaws(m, &w, &yc, 1, &n_ctrl, pos.data(), &pos_dt, start, &end_yaw, &status, &duration,
                                              &seg_num, &dt, q.data(), &n_waypt, wp.data(), &e, &cost, nullptr, nullptr);
  if (rc) {
    warn(knots ? "fuelmi_map_plan_yaws_knots" : "fuelmi_map_plan_yaws", rc);
    return rc;
  }
  if (status != FUELMI_YAW_OK) return status;
  yaw_ctrl = Eigen::MatrixXd(seg_num + 3, 1);
  for (int i = 0; i < seg_num + 3; ++i) yaw_ctrl(i, 0) = q[i];
  dt_yaw = dt;
  if (path_yaw) path_yaw->assign(wp.begin(), wp.begin() + n_waypt);
  return FUELMI_YAW_OK;
}

int BsplineOptimizer::planYawExplore(const Eigen::MatrixXd& pos_ctrl, int pos_degree, double pos_dt,
                                     const Eigen::Vector3d& start_yaw, double end_yaw, bool lookfwd, double relax_time,
                                     Eigen::MatrixXd& yaw_ctrl, double& dt_yaw) {
  fuelmi_yaw_cfg yc = {FUELMI_YAW_EXPLORE, pos_degree, (int)pos_ctrl.rows(), 12, 12, lookfwd ? 1 : 0, relax_time, 2.0, 0.3, 0.1};
  return plan_one_yaw(edt_environment_->sdf_map_->device(), cfg_, yc, pos_ctrl, pos_dt, start_yaw, end_yaw, yaw_ctrl, dt_yaw,
                      nullptr);
}

int BsplineOptimizer::planYaw(const Eigen::MatrixXd& pos_ctrl, int pos_degree, double pos_dt,
                              const Eigen::Vector3d& start_yaw, Eigen::MatrixXd& yaw_ctrl, double& dt_yaw,
                              std::vector<double>* path_yaw) {
  fuelmi_yaw_cfg yc = {FUELMI_YAW_FOLLOW, pos_degree, (int)pos_ctrl.rows(), FUELMI_YAW_MAX_SEG, 0, 1, 0.0, 2.0, 0.3, 0.1};
  return plan_one_yaw(edt_environment_->sdf_map_->device(), cfg_, yc, pos_ctrl, pos_dt, start_yaw, 0.0, yaw_ctrl, dt_yaw,
                      path_yaw);
}

int BsplineOptimizer::planYaw(const Eigen::MatrixXd& pos_ctrl, int pos_degree, const Eigen::VectorXd& knots,
                              const Eigen::Vector3d& start_yaw, Eigen::MatrixXd& yaw_ctrl, double& dt_yaw,
                              std::vector<double>* path_yaw) {
  fuelmi_yaw_cfg yc = {FUELMI_YAW_FOLLOW, pos_degree, (int)pos_ctrl.rows(), FUELMI_YAW_MAX_SEG, 0, 1, 0.0, 2.0, 0.3, 0.1};
  return plan_one_yaw(edt_environment_->sdf_map_->device(), cfg_, yc, pos_ctrl, 0.0, start_yaw, 0.0, yaw_ctrl, dt_yaw,
                      path_yaw, &knots);
}

// both checkTrajCollision (knots null: the uniform spline of the span dt)
static bool check_one_traj(fuelmi_map* m, const Eigen::MatrixXd& pos_ctrl, int degree, double dt, const Eigen::VectorXd* knots,
                           double t_now, double& distance) {
  const int n_ctrl = (int)pos_ctrl.rows();
  int rc = FUELMI_EINVAL, status = 0, safe = 0, n_samples = 0, hit_index = 0, end_reason = 0;
  double dist = 0.0, hit_t = 0.0, hit_pos[3], duration = 0.0;
  std::vector<double> u;
  if (n_ctrl >= 1 && pos_ctrl.cols() == 3 && (!knots || knots_of(*knots, n_ctrl, degree, u))) {
    std::vector<double> pos(3 * (size_t)n_ctrl);
    for (int i = 0; i < n_ctrl; ++i)
      for (int k = 0; k < 3; ++k) pos[3 * i + k] = pos_ctrl(i, k);
    const fuelmi_trajchk_cfg tc = {degree, n_ctrl, 0.02, 6.0};  // planner_manager.cpp:102, 104
    rc = knots ? fuelmi_map_check_trajs_knots(m, &tc, 1, &n_ctrl, pos.data(), u.data(), &t_now, &status, &safe, &dist,
                                              &n_samples, &hit_index, &hit_t, hit_pos, &end_reason, &duration)
               : fuelmi_map_check_trajs(m, &tc, 1, &n_ctrl, pos.data(), &dt, &t_now, &status, &safe, &dist, &n_samples,
                                        &hit_index, &hit_t, hit_pos, &end_reason, &duration);
  }
  if (rc && rc != FUELMI_ELIMIT) {
    warn(knots ? "fuelmi_map_check_trajs_knots" : "fuelmi_map_check_trajs", rc);
    dist = 0.0, safe = 0;
  }
  if (safe) return true;
  distance = dist;
  return false;
}

bool BsplineOptimizer::checkTrajCollision(const Eigen::MatrixXd& pos_ctrl, int degree, double dt, double t_now,
                                          double& distance) {
  return check_one_traj(edt_environment_->sdf_map_->device(), pos_ctrl, degree, dt, nullptr, t_now, distance);
}

bool BsplineOptimizer::checkTrajCollision(const Eigen::MatrixXd& pos_ctrl, int degree, const Eigen::VectorXd& knots,
                                          double t_now, double& distance) {
  return check_one_traj(edt_environment_->sdf_map_->device(), pos_ctrl, degree, 0.0, &knots, t_now, distance);
}

// one problem through fuelmi_map_sample_trajs (knots null) or fuelmi_map_sample_trajs_knots; out = status | pos | vel |
// acc | jerk | yaw | yawdot | yawddot
static int sample_one_traj(fuelmi_map* m, int mode, const Eigen::MatrixXd& pos_ctrl, int degree, double dt,
                           const Eigen::VectorXd* knots, const Eigen::MatrixXd& yaw_ctrl, int yaw_degree, double yaw_dt,
                           const std::vector<double>& t, const double* t_stop, std::vector<int>& status,
                           std::vector<double> out[7], double* flight8) {
  const int n_ctrl = (int)pos_ctrl.rows(), n_yaw = (int)yaw_ctrl.rows(), n_t = (int)t.size();
  if (n_ctrl < 1 || pos_ctrl.cols() != 3 || (n_yaw > 0 && yaw_ctrl.cols() < 1)) return FUELMI_EINVAL;
  std::vector<double> u;
  if (knots && !knots_of(*knots, n_ctrl, degree, u)) return FUELMI_EINVAL;
  std::vector<double> pos(3 * (size_t)n_ctrl), yawc((size_t)n_yaw);
  for (int i = 0; i < n_ctrl; ++i)
    for (int k = 0; k < 3; ++k) pos[3 * i + k] = pos_ctrl(i, k);
  for (int i = 0; i < n_yaw; ++i) yawc[i] = yaw_ctrl(i, 0);
  const fuelmi_trajsmp_cfg sc = {mode, degree, yaw_degree, n_ctrl, n_yaw, n_t};
  status.assign(n_t, 0);
  for (int k = 0; k < 7; ++k) out[k].assign((k < 4 ? 3 : 1) * (size_t)n_t, 0.0);
  double duration = 0.0;
  if (knots)
    return fuelmi_map_sample_trajs_knots(m, &sc, 1, &n_ctrl, pos.data(), u.data(), n_yaw > 0 ? &n_yaw : nullptr, yawc.data(),
                                         &yaw_dt, t_stop, &n_t, t.data(), status.data(), out[0].data(), out[1].data(),
                                         out[2].data(), out[3].data(), out[4].data(), out[5].data(), out[6].data(), &duration,
                                         flight8);
  return fuelmi_map_sample_trajs(m, &sc, 1, &n_ctrl, pos.data(), &dt, n_yaw > 0 ? &n_yaw : nullptr, yawc.data(), &yaw_dt,
                                 t_stop, &n_t, t.data(), status.data(), out[0].data(), out[1].data(), out[2].data(),
                                 out[3].data(), out[4].data(), out[5].data(), out[6].data(), &duration, flight8);
}

// both evaluateCommand (knots null: the uniform spline of the span dt)
static bool command_one_traj(fuelmi_map* m, const Eigen::MatrixXd& pos_ctrl, int degree, double dt, const Eigen::VectorXd* knots,
                             const Eigen::MatrixXd& yaw_ctrl, int yaw_degree, double yaw_dt, const std::vector<double>& t,
                             const double* t_stop, std::vector<int>& status, Eigen::MatrixXd& pos, Eigen::MatrixXd& vel,
                             Eigen::MatrixXd& acc, Eigen::MatrixXd& jerk, Eigen::MatrixXd& yaw, double* flight8) {
  std::vector<int> st;
  std::vector<double> out[7];
  const int rc = sample_one_traj(m, FUELMI_TRAJSMP_COMMAND, pos_ctrl, degree, dt, knots, yaw_ctrl, yaw_degree, yaw_dt, t, t_stop,
                                 st, out, flight8);
  if (rc) {
    warn(knots ? "fuelmi_map_sample_trajs_knots" : "fuelmi_map_sample_trajs", rc);
    return false;
  }
  const int n_t = (int)t.size();
  status = st;
  Eigen::MatrixXd* dst[4] = {&pos, &vel, &acc, &jerk};
  for (int q = 0; q < 4; ++q) {
    *dst[q] = Eigen::MatrixXd(n_t, 3);
    for (int i = 0; i < n_t; ++i)
      for (int k = 0; k < 3; ++k) (*dst[q])(i, k) = out[q][3 * (size_t)i + k];
  }
  yaw = Eigen::MatrixXd(n_t, 3);
  for (int i = 0; i < n_t; ++i)
    for (int k = 0; k < 3; ++k) yaw(i, k) = out[4 + k][i];
  return true;
}

bool BsplineOptimizer::evaluateCommand(const Eigen::MatrixXd& pos_ctrl, int degree, double dt, const Eigen::MatrixXd& yaw_ctrl,
                                       int yaw_degree, double yaw_dt, const std::vector<double>& t, const double* t_stop,
                                       std::vector<int>& status, Eigen::MatrixXd& pos, Eigen::MatrixXd& vel,
                                       Eigen::MatrixXd& acc, Eigen::MatrixXd& jerk, Eigen::MatrixXd& yaw, double* flight8) {
  return command_one_traj(edt_environment_->sdf_map_->device(), pos_ctrl, degree, dt, nullptr, yaw_ctrl, yaw_degree, yaw_dt, t,
                          t_stop, status, pos, vel, acc, jerk, yaw, flight8);
}

bool BsplineOptimizer::evaluateCommand(const Eigen::MatrixXd& pos_ctrl, int degree, const Eigen::VectorXd& knots,
                                       const Eigen::MatrixXd& yaw_ctrl, int yaw_degree, double yaw_dt,
                                       const std::vector<double>& t, const double* t_stop, std::vector<int>& status,
                                       Eigen::MatrixXd& pos, Eigen::MatrixXd& vel, Eigen::MatrixXd& acc, Eigen::MatrixXd& jerk,
                                       Eigen::MatrixXd& yaw, double* flight8) {
  return command_one_traj(edt_environment_->sdf_map_->device(), pos_ctrl, degree, 0.0, &knots, yaw_ctrl, yaw_degree, yaw_dt, t,
                          t_stop, status, pos, vel, acc, jerk, yaw, flight8);
}

// both replanState (knots null: the uniform spline of the span dt)
static bool state_one_traj(fuelmi_map* m, const Eigen::MatrixXd& pos_ctrl, int degree, double dt, const Eigen::VectorXd* knots,
                           const Eigen::MatrixXd& yaw_ctrl, int yaw_degree, double yaw_dt, double t_r, Eigen::Vector3d& start_pt,
                           Eigen::Vector3d& start_vel, Eigen::Vector3d& start_acc, Eigen::Vector3d& start_yaw) {
  std::vector<int> st;
  std::vector<double> out[7];
  const int rc = sample_one_traj(m, FUELMI_TRAJSMP_STATE, pos_ctrl, degree, dt, knots, yaw_ctrl, yaw_degree, yaw_dt,
                                 std::vector<double>(1, t_r), nullptr, st, out, nullptr);
  if (rc) {
    warn(knots ? "fuelmi_map_sample_trajs_knots" : "fuelmi_map_sample_trajs", rc);
    return false;
  }
  for (int k = 0; k < 3; ++k) start_pt(k) = out[0][k], start_vel(k) = out[1][k], start_acc(k) = out[2][k], start_yaw(k) = out[4 + k][0];
  return true;
}

bool BsplineOptimizer::replanState(const Eigen::MatrixXd& pos_ctrl, int degree, double dt, const Eigen::MatrixXd& yaw_ctrl,
                                   int yaw_degree, double yaw_dt, double t_r, Eigen::Vector3d& start_pt,
                                   Eigen::Vector3d& start_vel, Eigen::Vector3d& start_acc, Eigen::Vector3d& start_yaw) {
  return state_one_traj(edt_environment_->sdf_map_->device(), pos_ctrl, degree, dt, nullptr, yaw_ctrl, yaw_degree, yaw_dt, t_r,
                        start_pt, start_vel, start_acc, start_yaw);
}

bool BsplineOptimizer::replanState(const Eigen::MatrixXd& pos_ctrl, int degree, const Eigen::VectorXd& knots,
                                   const Eigen::MatrixXd& yaw_ctrl, int yaw_degree, double yaw_dt, double t_r,
                                   Eigen::Vector3d& start_pt, Eigen::Vector3d& start_vel, Eigen::Vector3d& start_acc,
                                   Eigen::Vector3d& start_yaw) {
  return state_one_traj(edt_environment_->sdf_map_->device(), pos_ctrl, degree, 0.0, &knots, yaw_ctrl, yaw_degree, yaw_dt, t_r,
                        start_pt, start_vel, start_acc, start_yaw);
}

static fuelmi_trajadj_cfg trajadj_cfg(const BsplineOptimizer::TrajAdjust& c, int ops, int degree, int max_ctrl, int n_group) {
  fuelmi_trajadj_cfg a;
  a.ops = ops, a.degree = degree, a.max_ctrl = max_ctrl, a.max_samples = max_ctrl - degree + 2;
  a.realloc_iters = c.realloc_iters, a.n_group = n_group;
  a.limit_vel = c.limit_vel, a.limit_acc = c.limit_acc, a.limit_ratio = c.limit_ratio, a.lengthen_cap = c.lengthen_cap;
  a.length_res = c.length_res, a.stat_step = c.stat_step;
  return a;
}

bool BsplineOptimizer::adjustTime(const Eigen::MatrixXd& pos_ctrl, int degree, double dt, Eigen::VectorXd& knots, int ops,
                                  const double* ratio_in, const TrajAdjust& cfg, TrajMetrics& out, Eigen::MatrixXd* samples) {
  const int n_ctrl = (int)pos_ctrl.rows(), nk = n_ctrl + degree + 1;
  const int mask = FUELMI_TRAJADJ_LENGTHEN | FUELMI_TRAJADJ_REALLOC | FUELMI_TRAJADJ_RESAMPLE;
  if (n_ctrl < 1 || pos_ctrl.cols() != 3 || (ops & ~mask) || (knots.rows() != 0 && knots.rows() != nk)) {
    warn("adjustTime (arguments)", FUELMI_EINVAL);
    return false;
  }
  if (!samples) ops &= ~FUELMI_TRAJADJ_RESAMPLE;
  std::vector<double> pos(3 * (size_t)n_ctrl), kin((size_t)knots.rows()), kout((size_t)nk, 0.0);
  for (int i = 0; i < n_ctrl; ++i)
    for (int k = 0; k < 3; ++k) pos[3 * i + k] = pos_ctrl(i, k);
  for (int i = 0; i < (int)kin.size(); ++i) kin[i] = knots(i);
  const fuelmi_trajadj_cfg ac = trajadj_cfg(cfg, ops, degree, n_ctrl, 0);
  std::vector<double> smp(3 * (size_t)std::max(ac.max_samples, 1), 0.0);
  TrajMetrics r;
  const int rc = fuelmi_map_adjust_trajs(edt_environment_->sdf_map_->device(), &ac, 1, &n_ctrl, pos.data(), &dt,
                                         kin.empty() ? nullptr : kin.data(), ratio_in, nullptr, r.info, r.metrics,
                                         kout.data(), (ops & FUELMI_TRAJADJ_RESAMPLE) ? smp.data() : nullptr, nullptr);
  if (rc) {
    warn("fuelmi_map_adjust_trajs", rc);
    return false;
  }
  out = r;
  knots = Eigen::VectorXd(nk);
  for (int i = 0; i < nk; ++i) knots(i) = kout[i];
  if (samples) {
    const int ns = r.info[FUELMI_TRAJADJ_I_N_SAMPLES];
    *samples = Eigen::MatrixXd(ns, 3);
    for (int i = 0; i < ns; ++i)
      for (int k = 0; k < 3; ++k) (*samples)(i, k) = smp[3 * (size_t)i + k];
  }
  return true;
}

bool BsplineOptimizer::trajectoryMetrics(const Eigen::MatrixXd& pos_ctrl, int degree, double dt, const Eigen::VectorXd& knots,
                                         const TrajAdjust& cfg, TrajMetrics& out) {
  Eigen::VectorXd u = knots;
  return adjustTime(pos_ctrl, degree, dt, u, 0, nullptr, cfg, out, nullptr);
}

int BsplineOptimizer::selectBestTraj(const std::vector<Eigen::MatrixXd>& pos_ctrl, int degree, const std::vector<double>& dt,
                                     const TrajAdjust& cfg, std::vector<TrajMetrics>* all) {
  const int n = (int)pos_ctrl.size();
  if (n == 0 || dt.size() != pos_ctrl.size()) return -1;
  int max_ctrl = degree + 1;
  for (const auto& c : pos_ctrl) {
    if (c.rows() < 1 || c.cols() != 3) return -1;
    max_ctrl = std::max(max_ctrl, (int)c.rows());
  }
  std::vector<int> n_ctrl(n), group(n, 0), info((size_t)n * FUELMI_TRAJADJ_NI);
  std::vector<double> pos((size_t)n * max_ctrl * 3, 0.0), met((size_t)n * FUELMI_TRAJADJ_NM);
  std::vector<double> kout((size_t)n * (max_ctrl + degree + 1));
  for (int b = 0; b < n; ++b) {
    n_ctrl[b] = (int)pos_ctrl[b].rows();
    for (int i = 0; i < n_ctrl[b]; ++i)
      for (int k = 0; k < 3; ++k) pos[((size_t)b * max_ctrl + i) * 3 + k] = pos_ctrl[b](i, k);
  }
  const fuelmi_trajadj_cfg ac = trajadj_cfg(cfg, FUELMI_TRAJADJ_SELECT, degree, max_ctrl, 1);
  int best = -1;
  const int rc = fuelmi_map_adjust_trajs(edt_environment_->sdf_map_->device(), &ac, n, n_ctrl.data(), pos.data(), dt.data(),
                                         nullptr, nullptr, group.data(), info.data(), met.data(), kout.data(), nullptr, &best);
  if (rc) {
    warn("fuelmi_map_adjust_trajs", rc);
    return -1;
  }
  if (all) {
    all->resize(n);
    for (int b = 0; b < n; ++b) {
      std::copy(info.begin() + (size_t)b * FUELMI_TRAJADJ_NI, info.begin() + (size_t)(b + 1) * FUELMI_TRAJADJ_NI, (*all)[b].info);
      std::copy(met.begin() + (size_t)b * FUELMI_TRAJADJ_NM, met.begin() + (size_t)(b + 1) * FUELMI_TRAJADJ_NM, (*all)[b].metrics);
    }
  }
  return best;
}

// n problems (mode, start_t, arg0, arg1) on one state in one fuelmi_map_local_segments call
static bool local_segments(fuelmi_map* m, int degree, const BsplineOptimizer::GlobalTrajState& st, int n, const int* mode,
                           const double* start_t, const double* arg0, const double* arg1,
                           std::vector<BsplineOptimizer::LocalSegment>& out) {
  const int S = (int)st.seg_times.size(), nl = (int)st.local_ctrl.rows();
  if (n < 1 || S < 1 || st.coef.size() != 18 * st.seg_times.size() || (nl > 0 && st.local_ctrl.cols() != 3)) return false;
  fuelmi_localseg_cfg cfg;
  cfg.degree = degree, cfg.max_seg = S, cfg.max_ctrl = std::max(nl, degree + 1), cfg.max_points = FUELMI_LOCALSEG_MAX_POINTS;
  const int mp = cfg.max_points, rows = mp + degree - 1;
  std::vector<double> local((size_t)cfg.max_ctrl * 3, 0.0);
  for (int i = 0; i < nl; ++i)
    for (int k = 0; k < 3; ++k) local[(size_t)i * 3 + k] = st.local_ctrl(i, k);
  std::vector<int> traj_of(n, 0), iv((size_t)n * 5);
  std::vector<double> dv((size_t)n * 3), points((size_t)n * mp * 3), derivs((size_t)n * 12), ctrl((size_t)n * rows * 3);
  int *status = iv.data(), *n_steps = status + n, *seg_num = n_steps + n, *n_points = seg_num + n, *n_ctrl = n_points + n;
  double *segment_len = dv.data(), *duration = segment_len + n, *dt = duration + n;
  const int rc = fuelmi_map_local_segments(m, &cfg, 1, &S, st.seg_times.data(), st.coef.data(), &st.global_duration, &nl,
                                           local.data(), &st.local_knot_span, &st.local_start_time, &st.local_end_time,
                                           &st.time_change, &st.last_time_inc, n, traj_of.data(), mode, start_t, arg0, arg1,
                                           status, n_steps, segment_len, seg_num, duration, dt, n_points, points.data(),
                                           derivs.data(), n_ctrl, ctrl.data());
  if (rc) {
    warn("fuelmi_map_local_segments", rc);
    return false;
  }
  out.assign(n, BsplineOptimizer::LocalSegment());
  for (int b = 0; b < n; ++b) {
    BsplineOptimizer::LocalSegment& o = out[b];
    o.status = status[b], o.n_steps = n_steps[b], o.seg_num = seg_num[b];
    o.segment_len = segment_len[b], o.dt = dt[b], o.duration = duration[b];
    o.ctrl_pts.resize(n_ctrl[b], 3);
    for (int i = 0; i < n_ctrl[b]; ++i)
      for (int k = 0; k < 3; ++k) o.ctrl_pts(i, k) = ctrl[((size_t)b * rows + i) * 3 + k];
    for (int i = 0; i < n_points[b]; ++i) {
      const double* q = &points[((size_t)b * mp + i) * 3];
      o.points.push_back(Eigen::Vector3d(q[0], q[1], q[2]));
    }
    if (status[b] == FUELMI_LOCALSEG_OK)
      for (int i = 0; i < 4; ++i) {
        const double* q = &derivs[(size_t)b * 12 + 3 * i];
        o.start_end_derivative.push_back(Eigen::Vector3d(q[0], q[1], q[2]));
      }
  }
  return true;
}

bool BsplineOptimizer::paramLocalTraj(const GlobalTrajState& state, double start_t, double radius, double dist_pt,
                                      LocalSegment& out) {
  const int mode = FUELMI_LOCALSEG_SPHERE;
  std::vector<LocalSegment> one;
  if (!local_segments(edt_environment_->sdf_map_->device(), bspline_degree_, state, 1, &mode, &start_t, &radius, &dist_pt, one))
    return false;
  out = one[0];
  return true;
}

bool BsplineOptimizer::reparamLocalTraj(const GlobalTrajState& state, double start_t, double duration,
                                        const std::vector<double>& dts, std::vector<LocalSegment>& out) {
  const int n = (int)dts.size();
  const std::vector<int> mode(n, FUELMI_LOCALSEG_DURATION);
  const std::vector<double> t0(n, start_t), dur(n, duration);
  std::vector<LocalSegment> all;
  if (!local_segments(edt_environment_->sdf_map_->device(), bspline_degree_, state, n, mode.data(), t0.data(), dur.data(),
                      dts.data(), all))
    return false;
  out.swap(all);
  return true;
}

vector<Eigen::Vector3d> BsplineOptimizer::matrixToVectors(const Eigen::MatrixXd& ctrl_pts) {
  vector<Eigen::Vector3d> out;
  for (int i = 0; i < ctrl_pts.rows(); ++i) {
    Eigen::Vector3d p(0, 0, 0);
    for (int j = 0; j < ctrl_pts.cols() && j < 3; ++j) p(j) = ctrl_pts(i, j);
    out.push_back(p);
  }
  return out;
}
Eigen::MatrixXd BsplineOptimizer::getControlPoints() { return control_points_; }
bool BsplineOptimizer::isQuadratic() {
  return cost_function_ == GUIDE_PHASE || cost_function_ == SMOOTHNESS || cost_function_ == (SMOOTHNESS | WAYPOINTS);
}

// ------------------------------------------------------------------------------------------------
// HeadingPlanner (active_perception/heading_planner.h): fuelmi_map_yaw_paths / fuelmi_map_info_gains
// ------------------------------------------------------------------------------------------------
HeadingPlanner::HeadingPlanner(ros::NodeHandle& nh) {
  nh.param("heading_planner/yaw_diff", yaw_diff_, -1.0);
  nh.param("heading_planner/lambda1", lambda1_, -1.0);
  nh.param("heading_planner/lambda2", lambda2_, -1.0);
  nh.param("heading_planner/half_vert_num", half_vert_num_, -1);
  nh.param("heading_planner/max_yaw_rate", max_yaw_rate_, -1.0);
  nh.param("heading_planner/w", w_, -1.0);
  nh.param("heading_planner/weight_type", weight_type_, -1);
  far_ = 4.5, top_ang_ = 0.56125, left_ang_ = 0.69222, right_ang_ = 0.68901;  // heading_planner.cpp:119-126
}
HeadingPlanner::~HeadingPlanner() {}
void HeadingPlanner::setMap(const shared_ptr<SDFMap>& map) { sdf_map_ = map; }

static fuelmi_gain_cfg heading_gain_cfg(const HeadingPlanner& hp, int weight_type, int in_box, int max_yaw, int max_ctrl) {
  fuelmi_gain_cfg g;
  g.weight_type = weight_type, g.in_box = in_box, g.factor = 4, g.max_yaw = max_yaw, g.max_ctrl = max_ctrl;
  g.far = hp.far_, g.top_ang = hp.top_ang_, g.left_ang = hp.left_ang_, g.right_ang = hp.right_ang_;
  g.lambda1 = hp.lambda1_, g.lambda2 = hp.lambda2_;
  return g;
}

int HeadingPlanner::searchPathsOfYaw(const vector<vector<Eigen::Vector3d>>& pts, const vector<vector<double>>& yaws,
                                     const vector<double>& dts, const vector<Eigen::MatrixXd>& ctrl_pts,
                                     vector<vector<double>>& paths) {
  const size_t n = yaws.size();
  paths.assign(n, vector<double>());
  last_status_.assign(n, 0), last_path_vertex_.assign(n, vector<int>()), last_gains_.assign(n, vector<double>());
  last_g_value_.assign(n, vector<double>());
  if (pts.size() != n || dts.size() != n || ctrl_pts.size() != n || half_vert_num_ < 0) return last_rc_ = FUELMI_EINVAL;
  size_t ml = 1, mc = 1;
  for (size_t b = 0; b < n; ++b) {
    if (pts[b].size() != yaws[b].size()) return last_rc_ = FUELMI_EINVAL;
    ml = std::max(ml, yaws[b].size()), mc = std::max(mc, (size_t)ctrl_pts[b].rows());
  }
  const size_t nv = 2 * (size_t)half_vert_num_ + 1;
  fuelmi_yawpath_cfg c;
  c.gain = heading_gain_cfg(*this, weight_type_, 1, (int)nv, (int)mc);
  c.half_vert_num = half_vert_num_, c.max_layer = (int)ml;
  c.yaw_diff = yaw_diff_, c.max_yaw_rate = max_yaw_rate_, c.w = w_;
  vector<int> n_layer(n), n_ctrl(n), status(n), pv(n * ml), n_rays(n * ml);
  vector<double> P(n * ml * 3), Y(n * ml), C(n * mc * 3), path(n * ml), gains(n * ml * nv), gv(n * ml * nv);
  for (size_t b = 0; b < n; ++b) {
    n_layer[b] = (int)yaws[b].size(), n_ctrl[b] = (int)ctrl_pts[b].rows();
    for (size_t i = 0; i < yaws[b].size(); ++i) {
      Y[b * ml + i] = yaws[b][i];
      for (int k = 0; k < 3; ++k) P[(b * ml + i) * 3 + k] = pts[b][i](k);
    }
    for (int i = 0; i < n_ctrl[b]; ++i)
      for (int k = 0; k < 3; ++k) C[(b * mc + i) * 3 + k] = ctrl_pts[b](i, k);
  }
  last_rc_ = fuelmi_map_yaw_paths(sdf_map_ ? sdf_map_->device() : nullptr, &c, (int)n, n_layer.data(), P.data(), Y.data(),
                                  dts.data(), n_ctrl.data(), C.data(), nullptr, status.data(), path.data(), pv.data(),
                                  gains.data(), gv.data(), n_rays.data());
  if (last_rc_ != FUELMI_OK && last_rc_ != FUELMI_ELIMIT) {
    ROS_ERROR("[Heading]: fuelmi_map_yaw_paths: %s", fuelmi_last_error());
    return last_rc_;
  }
  for (size_t b = 0; b < n; ++b) {
    last_status_[b] = status[b];
    if (status[b] != 0) continue;
    paths[b].assign(path.begin() + b * ml, path.begin() + b * ml + n_layer[b]);
    last_path_vertex_[b].assign(pv.begin() + b * ml, pv.begin() + b * ml + n_layer[b]);
    for (int i = 0; i < n_layer[b]; ++i) {
      last_gains_[b].insert(last_gains_[b].end(), gains.begin() + (b * ml + i) * nv, gains.begin() + (b * ml + i + 1) * nv);
      last_g_value_[b].insert(last_g_value_[b].end(), gv.begin() + (b * ml + i) * nv, gv.begin() + (b * ml + i + 1) * nv);
    }
  }
  return last_rc_;
}

void HeadingPlanner::searchPathOfYaw(const vector<Eigen::Vector3d>& pts, const vector<double>& yaws, const double& dt,
                                     const Eigen::MatrixXd& ctrl_pts, vector<double>& path) {
  vector<vector<double>> paths;
  searchPathsOfYaw({pts}, {yaws}, {dt}, {ctrl_pts}, paths);
  // (the reference appends to `path`)
  if (!paths.empty()) path.insert(path.end(), paths[0].begin(), paths[0].end());
}

int HeadingPlanner::calcInfoGains(const vector<Eigen::Vector3d>& pts, const vector<double>& yaws, vector<double>& gains) {
  const size_t n = pts.size();
  gains.assign(n, 0.0);
  if (yaws.size() != n) return last_rc_ = FUELMI_EINVAL;
  const fuelmi_gain_cfg c = heading_gain_cfg(*this, FUELMI_GAIN_UNIFORM, 0, 1, 1);  // calcInfoGain: no isInBox, counts
  vector<double> P(n * 3 + 1);
  vector<int> n_yaw(n + 1, 1), status(n + 1), n_cand(n + 1), n_vis(n + 1), n_rays(n + 1);
  for (size_t b = 0; b < n; ++b)
    for (int k = 0; k < 3; ++k) P[b * 3 + k] = pts[b](k);
  last_rc_ = fuelmi_map_info_gains(sdf_map_ ? sdf_map_->device() : nullptr, &c, (int)n, P.data(), n_yaw.data(), yaws.data(),
                                   0, nullptr, nullptr, nullptr, status.data(), gains.data(), n_cand.data(), n_vis.data(),
                                   n_rays.data());
  last_status_.assign(status.begin(), status.begin() + n);
  if (last_rc_ != FUELMI_OK && last_rc_ != FUELMI_ELIMIT) ROS_ERROR("[Heading]: fuelmi_map_info_gains: %s", fuelmi_last_error());
  return last_rc_;
}

double HeadingPlanner::calcInfoGain(const Eigen::Vector3d& pt, const double& yaw, const int&) {
  vector<double> gains;
  calcInfoGains({pt}, {yaw}, gains);
  return gains.empty() ? 0.0 : gains[0];
}

}  // namespace fast_planner

// for libfuelmi_lkh.so (a weak reference there): the device of the SDFMap initialised last, -1 if none
extern "C" int fuelmi_facade_last_map_device(void) { return fast_planner::g_last_map_device.load(); }
