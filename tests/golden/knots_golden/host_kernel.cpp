// A host build of the three kernels that take given knots -- k_traj_check, k_traj_sample and k_yaw_plan, each its own text
// cut out of its .hip by tests/golden/check_knots_host_build.py into kernel.inc -- on the lanes of
// tests/golden/host_lanes.h, run through SplineSrc's knot pointer.  The knots, the control points, the times, the plane and
// every result array are heap blocks of their exact size; a problem's knot row is NaN behind its own n + p + 1 knots, so
// a read past them fails the kernel's own check and shows.  Reads the launches check_knots_host_build.py writes and
// prints per problem: C (the safety check), S and one line per sample slot (sampling), Y twice (the yaw plan, EXPLORE and
// FOLLOW).
//   host_kernel <in.txt>
#include "host_lanes.h"
#include "spline_internal.h"
#include "kernel.inc"

static void row(const char* head, const std::vector<double>& v, size_t from, size_t count) {
  std::printf("%s", head);
  for (size_t k = 0; k < count; ++k) std::printf(" %016llx", bits(v[from + k]));
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  std::ifstream in(argv[1]);
  Geo g;
  memset(&g, 0, sizeof(g));
  in >> g.nx >> g.ny >> g.nz;
  for (double& o : g.org) o = num(in);
  g.res_inv = num(in);
  g.res = 1 / g.res_inv;
  g.nyz = g.ny * g.nz, g.N = g.nx * g.nyz, g.W = (g.N + 63) / 64;
  std::vector<u64> plane(g.W, 0);
  int n_set;
  in >> n_set;
  for (int i = 0; i < n_set; ++i) {
    long adr;
    in >> adr;
    plane[adr >> 6] |= 1ull << (adr & 63);
  }
  int n_launch;
  in >> n_launch;
  for (int l = 0; l < n_launch; ++l) {
    int p, maxc, n, max_t;
    in >> p >> maxc >> n >> max_t;
    const size_t ks = (size_t)maxc + p + 1, s = (size_t)n * max_t;
    std::vector<int> nc(n), nt(n);
    std::vector<double> knots(n * ks, std::nan("")), pos((size_t)n * maxc * 3, 1e300), now(n), t(s, 1e300), start(3 * (size_t)n),
        end(n);
    for (int b = 0; b < n; ++b) {
      in >> nc[b];
      for (int k = 0; k < nc[b] + p + 1; ++k) knots[b * ks + k] = num(in);
      for (int k = 0; k < 3 * nc[b]; ++k) pos[(size_t)b * maxc * 3 + k] = num(in);
      now[b] = num(in);
      in >> nt[b];
      for (int k = 0; k < nt[b]; ++k) t[(size_t)b * max_t + k] = num(in);
      for (int k = 0; k < 3; ++k) start[3 * b + k] = num(in);
      end[b] = num(in);
    }
    const SplineSrc src = {nc.data(), 0, pos.data(), (size_t)maxc * 3, nullptr, 0, knots.data(), ks};

    {  // the safety check
      TrajChkArgs T;
      memset(&T, 0, sizeof(T));
      T.cfg.degree = p, T.cfg.max_ctrl = maxc, T.cfg.step = num(in), T.cfg.max_radius = num(in);
      std::vector<int> iv[5];
      std::vector<double> dv[3], hp((size_t)n * 3, -7.0);
      for (auto& v : iv) v.assign(n, -77);
      for (auto& v : dv) v.assign(n, -7.0);
      T.n_prob = n, T.src = src, T.t_now = now.data(), T.infl = plane.data();
      T.status = iv[0].data(), T.safe = iv[1].data(), T.n_samples = iv[2].data(), T.hit_index = iv[3].data();
      T.end_reason = iv[4].data(), T.distance = dv[0].data(), T.hit_t = dv[1].data(), T.duration = dv[2].data();
      T.hit_pos = hp.data();
      if (const int rc = launch((n + TC_WAVES - 1) / TC_WAVES, TC_WIN * TC_WAVES, tc_lds(maxc), [&] { k_traj_check(g, T); }))
        return rc;
      for (int b = 0; b < n; ++b)
        std::printf("C %d %d %d %d %d %016llx %016llx %016llx %016llx %016llx %016llx\n", iv[0][b], iv[1][b], iv[2][b],
                    iv[3][b], iv[4][b], bits(dv[0][b]), bits(dv[1][b]), bits(dv[2][b]), bits(hp[3 * b]), bits(hp[3 * b + 1]),
                    bits(hp[3 * b + 2]));
    }
    {  // sampling: commands with a flight record, no yaw spline
      TrajSmpArgs A;
      memset(&A, 0, sizeof(A));
      fuelmi_trajsmp_cfg& c = A.cfg;
      c.mode = FUELMI_TRAJSMP_COMMAND, c.degree = p, c.yaw_degree = 3, c.max_ctrl = maxc, c.max_yaw_ctrl = 0, c.max_t = max_t;
      std::vector<int> status(s, -77);
      std::vector<double> flight((size_t)n * 8, 0.0), dur(n, -7.0), o3[4], o1[3];
      for (auto& v : o3) v.assign(3 * s, -7.0);
      for (auto& v : o1) v.assign(s, -7.0);
      A.n_prob = n, A.src = src, A.n_t = nt.data(), A.t = t.data(), A.flight = flight.data();
      A.status = status.data(), A.o_pos = o3[0].data(), A.o_vel = o3[1].data(), A.o_acc = o3[2].data(), A.o_jerk = o3[3].data();
      A.o_yaw = o1[0].data(), A.o_yawdot = o1[1].data(), A.o_yawddot = o1[2].data(), A.duration = dur.data();
      if (const int rc = launch((n + TS_WAVES - 1) / TS_WAVES, TS_WIN * TS_WAVES, ts_lds(c), [&] { k_traj_sample(A); })) return rc;
      for (int b = 0; b < n; ++b) {
        std::printf("S %016llx", bits(dur[b]));
        for (int k = 0; k < 8; ++k) std::printf(" %016llx", bits(flight[(size_t)b * 8 + k]));
        std::printf("\n");
        for (int k = 0; k < max_t; ++k) {
          const size_t e = (size_t)b * max_t + k;
          std::printf("%d", status[e]);
          for (auto& v : o3)
            for (int a = 0; a < 3; ++a) std::printf(" %016llx", bits(v[3 * e + a]));
          for (auto& v : o1) std::printf(" %016llx", bits(v[e]));
          std::printf("\n");
        }
      }
    }
    YawArgs Y0;  // the yaw plan: the launch's line holds the configuration both modes share
    memset(&Y0, 0, sizeof(Y0));
    {
      fuelmi_yaw_cfg& c = Y0.cfg;
      c.pos_degree = p, c.max_ctrl = maxc;
      in >> c.seg_num >> c.lookfwd >> c.max_seg;
      c.relax_time = num(in), c.forward_t = num(in), c.dt_target = num(in), c.end_back = num(in);
      Y0.ld_smooth = num(in), Y0.ld_start = num(in), Y0.ld_end = num(in), Y0.ld_waypt = num(in);
    }
    for (int mode : {FUELMI_YAW_EXPLORE, FUELMI_YAW_FOLLOW}) {
      YawArgs Y = Y0;
      Y.cfg.mode = mode;
      const size_t maxs = (size_t)Y.cfg.max_seg;
      std::vector<int> status(n, -77), seg(n, -77), nw(n, -77);
      std::vector<double> dur(n, -7.0), dty(n, -7.0), eo(n, -7.0), cost(n, -7.0), yc(n * (maxs + 3), -7.0), wp(n * maxs, -7.0);
      Y.n_prob = n, Y.src = src, Y.start_yaw = start.data(), Y.end_yaw = end.data();
      Y.status = status.data(), Y.seg_num = seg.data(), Y.n_waypt = nw.data(), Y.duration = dur.data(), Y.dt_yaw = dty.data();
      Y.end_yaw_out = eo.data(), Y.cost = cost.data(), Y.yaw_ctrl = yc.data(), Y.waypts = wp.data();
      if (const int rc = launch(n, YP_NT, yp_lds(maxc, Y.cfg.max_seg), [&] { k_yaw_plan(Y); })) return rc;
      for (int b = 0; b < n; ++b) {
        std::printf("Y %d %d %d %d %016llx %016llx %016llx %016llx\n", mode, status[b], seg[b], nw[b], bits(dur[b]), bits(dty[b]),
                    bits(eo[b]), bits(cost[b]));
        row("W", wp, b * maxs, maxs);
        row("Q", yc, b * (maxs + 3), maxs + 3);
      }
    }
  }
  return 0;
}
