// facade_render.cpp -- the simulated depth camera in front of the map, WITH EVERY MIRROR SWITCHED OFF: a renderer and two
// facade maps on one device; a cloud (a wavy wall and a floor around the origin), a handful of camera poses rendered in one
// fuelmi_render_depth call, then frame k fused twice:
//   map A  fuelmi_map_input_depth on the renderer's device pointer of the raw frame (no depth image crosses PCIe)
//   map B  fuelmi_map_input_depth on the host copy of the same frame
// both maps inflated, their occupancy and inflate planes refreshed and compared; for both models of the renderer.  Prints
// one JSON document with what the two routes fused and whether the maps are byte-equal.
#include "facade_driver.h"

#include <cstring>

// the whole map's planes, refreshed from the device on request only
static void planes(SDFMap& m, std::vector<double>& occ, std::vector<char>& infl) {
  const Eigen::Vector3i lo(0, 0, 0), hi = MapROS::param(m).map_voxel_num_ - Eigen::Vector3i(1, 1, 1);
  MapROS::refresh(m, lo, hi, true, true, false);
  occ = MapROS::data(m).occupancy_buffer_;
  infl = MapROS::data(m).occupancy_buffer_inflate_;
}

static SDFMap::Ptr make_map(const double size[3]) {
  ros::NodeHandle nh;
  double box_lo[3], box_hi[3];
  inset_box(size, box_lo, box_hi);
  sdf_map_params(nh, size, box_lo, box_hi);
  return make_map(nh, true).map;  // nothing below refreshes a mirror unless it says so
}

#define CHK(call)                                                             \
  do {                                                                        \
    if ((call) != FUELMI_OK) {                                                \
      std::fprintf(stderr, "%s failed: %s\n", #call, fuelmi_last_error());   \
      return 4;                                                               \
    }                                                                         \
  } while (0)

int main() {
  const double size[3] = {12.0, 10.0, 3.0};
  const int rows = 120, cols = 160, n_frames = 5;
  const double s = cols / 640.0;
  fuelmi_depth_cfg dc;
  dc.fx = 387.229248046875 * s, dc.fy = 387.229248046875 * s, dc.cx = 321.04638671875 * s, dc.cy = 243.44969177246094 * s;
  dc.depth_filter_maxdist = 5.0, dc.depth_filter_mindist = 0.2, dc.depth_filter_margin = 2;
  dc.k_depth_scaling_factor = 1000.0, dc.skip_pixel = 2;
  // the world: a wavy wall 2.5 to 3.5 m from the origin all around, and a floor, as a 5 cm cloud
  std::vector<float> cloud;
  for (int i = 0; i < 720; ++i)
    for (int j = 0; j < 40; ++j) {
      const double az = 2.0 * M_PI * i / 720.0, r = 3.0 + 0.5 * std::sin(5.0 * az), z = -0.8 + 0.05 * j;
      cloud.push_back((float)(r * std::cos(az))), cloud.push_back((float)(r * std::sin(az))), cloud.push_back((float)z);
    }
  for (int i = -60; i <= 60; ++i)
    for (int j = -60; j <= 60; ++j) cloud.push_back(0.05f * i), cloud.push_back(0.05f * j), cloud.push_back(-0.8f);
  const int n_points = (int)cloud.size() / 3;
  // the poses: the camera turns on the spot and drifts; x right, y down, z forward (yaw about world z)
  std::vector<double> T_cw, cam_pos, cam_q;
  for (int k = 0; k < n_frames; ++k) {
    const double yaw = 0.9 * k, p[3] = {0.15 * k - 0.3, 0.1 * std::sin(1.7 * k), 0.1};
    Eigen::Matrix4d c2w = Eigen::Matrix4d::Identity();
    const double R[3][3] = {{std::sin(yaw), 0.0, std::cos(yaw)}, {-std::cos(yaw), 0.0, std::sin(yaw)}, {0.0, -1.0, 0.0}};
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) c2w(a, b) = R[a][b];
      c2w(a, 3) = p[a];
    }
    const Eigen::Matrix4d Tcw = c2w.inverse();  // what the node computes per frame
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 4; ++b) T_cw.push_back(Tcw(a, b));
    for (int a = 0; a < 3; ++a) cam_pos.push_back(p[a]);
    // the quaternion (w, x, y, z) of R: Rz(yaw) * [x right, y down, z forward]
    const double tr = R[0][0] + R[1][1] + R[2][2];
    double q[4];
    if (tr > 0) {
      const double s4 = std::sqrt(tr + 1.0) * 2;
      q[0] = 0.25 * s4, q[1] = (R[2][1] - R[1][2]) / s4, q[2] = (R[0][2] - R[2][0]) / s4, q[3] = (R[1][0] - R[0][1]) / s4;
    } else {
      int i = 0;
      if (R[1][1] > R[i][i]) i = 1;
      if (R[2][2] > R[i][i]) i = 2;
      const int j = (i + 1) % 3, l = (i + 2) % 3;
      const double s4 = std::sqrt(1.0 + R[i][i] - R[j][j] - R[l][l]) * 2;
      q[0] = (R[l][j] - R[j][l]) / s4, q[1 + i] = 0.25 * s4, q[1 + j] = (R[j][i] + R[i][j]) / s4,
      q[1 + l] = (R[l][i] + R[i][l]) / s4;
    }
    for (int a = 0; a < 4; ++a) cam_q.push_back(q[a]);
  }
  std::printf("{\"frames\": %d, \"points\": %d, \"image\": [%d, %d]", n_frames, n_points, rows, cols);
  const char* names[2] = {"host_node", "cuda_node"};
  for (int model = 0; model < 2; ++model) {
    SDFMap::Ptr A = make_map(size), B = make_map(size);
    int mir[3];
    MapROS::mirrors(*A, mir);
    if (model == 0) std::printf(", \"mirrors\": [%d, %d, %d]", mir[0], mir[1], mir[2]);
    fuelmi_render_cfg rc;
    rc.device = A->hipDevice(), rc.rows = rows, rc.cols = cols;
    rc.fx = dc.fx, rc.fy = dc.fy, rc.cx = dc.cx, rc.cy = dc.cy;
    rc.model = model == 0 ? FUELMI_RENDER_HOST_NODE : FUELMI_RENDER_CUDA_NODE;
    rc.range = 5.0, rc.max_poses = n_frames;
    fuelmi_render* ren = nullptr;
    CHK(fuelmi_render_create(&rc, &ren));
    CHK(fuelmi_render_set_cloud(ren, cloud.data(), n_points));
    std::vector<unsigned short> raw((size_t)n_frames * rows * cols);
    std::vector<int> stats(4 * n_frames);
    CHK(fuelmi_render_depth(ren, n_frames, T_cw.data(), cam_pos.data(), dc.k_depth_scaling_factor, nullptr, raw.data(),
                            stats.data()));
    long pixels = 0;
    std::string fa = "[", fb = "[";
    for (int k = 0; k < n_frames; ++k) {
      pixels += stats[4 * k + 2];
      int na = -1, nb = -1;
      CHK(fuelmi_map_input_depth(A->device(), fuelmi_render_frame_raw(ren, k), rows, cols, &dc, &cam_pos[3 * k], &cam_q[4 * k], &na));
      CHK(fuelmi_map_input_depth(B->device(), raw.data() + (size_t)k * rows * cols, rows, cols, &dc, &cam_pos[3 * k],
                                 &cam_q[4 * k], &nb));
      MapROS::inflate(*A);
      MapROS::inflate(*B);
      fa += (k ? ", " : "") + std::to_string(na), fb += (k ? ", " : "") + std::to_string(nb);
    }
    CHK(fuelmi_render_destroy(ren));
    std::vector<double> oa, ob;
    std::vector<char> ia, ib;
    planes(*A, oa, ia);
    planes(*B, ob, ib);
    long occupied = 0;
    for (double v : oa) occupied += v > MapROS::param(*A).min_occupancy_log_;
    const bool occ_eq = oa.size() == ob.size() && !oa.empty() && memcmp(oa.data(), ob.data(), oa.size() * sizeof(double)) == 0;
    const bool inf_eq = ia.size() == ib.size() && !ia.empty() && memcmp(ia.data(), ib.data(), ia.size()) == 0;
    std::printf(",\n\"%s\": {\"pixels_with_return\": %ld, \"fused_device_pointer\": %s], \"fused_host_copy\": %s], "
                "\"occupancy_byte_equal\": %s, \"inflate_byte_equal\": %s, \"occupied_voxels\": %ld}",
                names[model], pixels, fa.c_str(), fb.c_str(), occ_eq ? "true" : "false", inf_eq ? "true" : "false", occupied);
  }
  std::printf("}\n");
  return 0;
}
