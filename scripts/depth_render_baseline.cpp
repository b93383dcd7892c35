// depth_render_baseline.cpp -- the CPU baseline of scripts/depth_render_timing.py: HOST_NODE's rules (include/fuelmi.h
// "Depth renderer") as one sequential loop over the cloud on one core, the way the simulator's default-built node renders a
// frame, including its `value < 1e-3` pixel update.  A point nearer than 1e-3 is skipped like on the device (deviation 1),
// so that the two routes can be compared byte for byte.  Built by the script with -ffp-contract=off.
#include <algorithm>
#include <cmath>

extern "C" int render_host_loop(int rows, int cols, double fx, double fy, double cx, double cy, double range,
                                const float* cloud, int n_points, const double* T_cw, const double* cam_pos, float* image) {
  std::fill(image, image + (long)rows * cols, 0.0f);
  int kept = 0;
  for (int i = 0; i < n_points; ++i) {
    const float* p = cloud + 3 * (long)i;
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
    const double x = p[0], y = p[1], z = p[2];
    const double dx = cam_pos[0] - x, dy = cam_pos[1] - y, dz = cam_pos[2] - z;
    if (std::sqrt((dx * dx + dy * dy) + dz * dz) > range) continue;
    const double pcx = ((T_cw[0] * x + T_cw[1] * y) + T_cw[2] * z) + T_cw[3];
    const double pcy = ((T_cw[4] * x + T_cw[5] * y) + T_cw[6] * z) + T_cw[7];
    const double pcz = ((T_cw[8] * x + T_cw[9] * y) + T_cw[10] * z) + T_cw[11];
    if (!(pcz > 0.0)) continue;
    const float px = (float)(pcx / pcz * fx + cx), py = (float)(pcy / pcz * fy + cy);
    if (!(px >= 0 && px < (float)cols && py >= 0 && py < (float)rows)) continue;
    const float dist = (float)pcz;
    if (dist < 1e-3f) continue;
    const int r = (int)(0.0573 * fx / dist + 0.5);
    const int x0 = std::max((int)(px - r), 0), x1 = std::min((int)(px + r), cols - 1);
    const int y0 = std::max((int)(py - r), 0), y1 = std::min((int)(py + r), rows - 1);
    ++kept;
    for (int u = x0; u <= x1; ++u)
      for (int v = y0; v <= y1; ++v) {
        float& value = image[(long)v * cols + u];
        value = value < 1e-3 ? dist : std::min(value, dist);
      }
  }
  return kept;
}
