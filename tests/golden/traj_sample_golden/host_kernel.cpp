// A host build of k_traj_sample's own text (fuel_amd/csrc/traj_sample.hip between "namespace {" and the host code, cut
// out by tests/golden/check_traj_sample_host_build.py into kernel.inc) on the lanes of tests/golden/host_lanes.h.  The
// knots, the control points, the times and every result array are heap blocks of their exact size.  Reads the launches
// check_traj_sample_host_build.py writes and prints per problem one line (the bits of the duration and of the eight
// record numbers) and one line per sample slot (the status, then the bits of the fifteen doubles).
//   host_kernel <in.txt>
#include "host_lanes.h"
#include "spline_internal.h"
#include "kernel.inc"
}  // namespace (kernel.inc leaves it open)

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  std::ifstream in(argv[1]);
  int n_launch;
  in >> n_launch;
  for (int l = 0; l < n_launch; ++l) {
    TrajSmpArgs A;
    memset(&A, 0, sizeof(A));
    fuelmi_trajsmp_cfg& c = A.cfg;
    int n, has_yaw, has_stop, has_flight, device_batch;
    in >> c.mode >> c.degree >> c.yaw_degree >> c.max_ctrl >> c.max_yaw_ctrl >> c.max_t >> n >> has_yaw >> has_stop >>
        has_flight >> device_batch;
    const size_t s = (size_t)n * c.max_t;
    // (1e300 / -7: a read past a problem's own points or times shows in the results)
    std::vector<int> nc(n), ny(n), nt(n), status(s, -77);
    std::vector<double> knot(n), pos((size_t)n * c.max_ctrl * 3, 1e300), ydt(n), yaw((size_t)n * c.max_yaw_ctrl, 1e300),
        stop(n), t(s, 1e300), flight((size_t)n * 8), dur(n, -7.0);
    std::vector<double> o3[4], o1[3];
    for (auto& v : o3) v.assign(3 * s, -7.0);
    for (auto& v : o1) v.assign(s, -7.0);
    for (int b = 0; b < n; ++b) {
      in >> nc[b];
      knot[b] = num(in);
      for (int k = 0; k < 3 * nc[b] && k < 3 * c.max_ctrl; ++k) pos[(size_t)b * c.max_ctrl * 3 + k] = num(in);
      in >> ny[b];
      ydt[b] = num(in);
      for (int k = 0; k < ny[b]; ++k) yaw[(size_t)b * c.max_yaw_ctrl + k] = num(in);
      stop[b] = num(in);
      for (int k = 0; k < 8; ++k) flight[(size_t)b * 8 + k] = num(in);
      in >> nt[b];
      for (int k = 0; k < nt[b]; ++k) t[(size_t)b * c.max_t + k] = num(in);
    }
    A.n_prob = n;
    if (device_batch)  // every problem has the stride's number of points, as in a batch
      A.src.n_ctrl = nullptr, A.src.n_ctrl_all = c.max_ctrl;
    else
      A.src.n_ctrl = nc.data();
    A.src.pos = pos.data(), A.src.pos_stride = (size_t)c.max_ctrl * 3, A.src.knot = knot.data(), A.src.knot_stride = 1;
    if (has_yaw) A.n_yaw = ny.data(), A.yaw = yaw.data(), A.yaw_dt = ydt.data();
    if (has_stop) A.t_stop = stop.data();
    A.n_t = nt.data(), A.t = t.data();
    if (has_flight) A.flight = flight.data();
    A.status = status.data(), A.o_pos = o3[0].data(), A.o_vel = o3[1].data(), A.o_acc = o3[2].data(), A.o_jerk = o3[3].data();
    A.o_yaw = o1[0].data(), A.o_yawdot = o1[1].data(), A.o_yawddot = o1[2].data(), A.duration = dur.data();
    if (const int rc = launch((n + TS_WAVES - 1) / TS_WAVES, TS_WIN * TS_WAVES, ts_lds(c), [&] { k_traj_sample(A); })) return rc;
    for (int b = 0; b < n; ++b) {
      std::printf("P %016llx", bits(dur[b]));
      for (int k = 0; k < 8; ++k) std::printf(" %016llx", bits(flight[(size_t)b * 8 + k]));
      std::printf("\n");
      for (int k = 0; k < c.max_t; ++k) {
        const size_t e = (size_t)b * c.max_t + k;
        std::printf("%d", status[e]);
        for (auto& v : o3)
          for (int a = 0; a < 3; ++a) std::printf(" %016llx", bits(v[3 * e + a]));
        for (auto& v : o1) std::printf(" %016llx", bits(v[e]));
        std::printf("\n");
      }
    }
  }
  return 0;
}
