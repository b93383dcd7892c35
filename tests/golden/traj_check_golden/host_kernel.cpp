// A host build of k_traj_check's own text (fuel_amd/csrc/traj_check.hip between "namespace {" and the host code, cut out
// by tests/golden/check_traj_check_host_build.py into kernel.inc) on the lanes of tests/golden/host_lanes.h.  The
// knots, the control points, the plane and the result arrays are heap blocks of their exact size.  Reads the problems
// check_traj_check_host_build.py writes and prints one line per problem: the five integers, then the bits of the six
// doubles.
//   host_kernel <in.txt>
#include "host_lanes.h"
#include "spline_internal.h"
#include "kernel.inc"
}  // namespace (kernel.inc leaves it open)

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  std::ifstream in(argv[1]);
  int n_maps;
  in >> n_maps;
  std::vector<Geo> geo(n_maps);
  std::vector<std::vector<u64>> plane(n_maps);
  for (int m = 0; m < n_maps; ++m) {
    Geo& g = geo[m];
    memset(&g, 0, sizeof(g));
    in >> g.nx >> g.ny >> g.nz;
    for (double& o : g.org) o = num(in);
    g.res_inv = num(in);
    g.res = 1 / g.res_inv;
    g.nyz = g.ny * g.nz, g.N = g.nx * g.nyz, g.W = (g.N + 63) / 64;
    plane[m].assign(g.W, 0);  // exactly the words that cover the map: the sanitizer sees a read past them
    int n_set;
    in >> n_set;
    for (int i = 0; i < n_set; ++i) {
      long adr;
      in >> adr;
      plane[m][adr >> 6] |= 1ull << (adr & 63);
    }
  }
  int n_launch;
  in >> n_launch;
  for (int l = 0; l < n_launch; ++l) {
    int map, n, maxc;
    TrajChkArgs T;
    memset(&T, 0, sizeof(T));
    in >> map >> n >> T.cfg.degree >> maxc;
    T.cfg.max_ctrl = maxc, T.cfg.step = num(in), T.cfg.max_radius = num(in);
    std::vector<int> nc(n);
    std::vector<double> knot(n), now(n), pos((size_t)n * maxc * 3, 1e300);  // (a read past a problem's own points shows)
    for (int b = 0; b < n; ++b) {
      in >> nc[b];
      knot[b] = num(in), now[b] = num(in);
      for (int k = 0; k < 3 * nc[b]; ++k) pos[(size_t)b * maxc * 3 + k] = num(in);
    }
    std::vector<int> iv[5];
    std::vector<double> dv[3], hp((size_t)n * 3, -7.0);
    for (auto& v : iv) v.assign(n, -77);
    for (auto& v : dv) v.assign(n, -7.0);
    T.n_prob = n, T.src = {nc.data(), 0, pos.data(), (size_t)maxc * 3, knot.data(), 1};
    T.t_now = now.data(), T.infl = plane[map].data();
    T.status = iv[0].data(), T.safe = iv[1].data(), T.n_samples = iv[2].data(), T.hit_index = iv[3].data();
    T.end_reason = iv[4].data(), T.distance = dv[0].data(), T.hit_t = dv[1].data(), T.duration = dv[2].data();
    T.hit_pos = hp.data();
    if (const int rc = launch((n + TC_WAVES - 1) / TC_WAVES, TC_WIN * TC_WAVES, tc_lds(maxc), [&] { k_traj_check(geo[map], T); }))
      return rc;
    for (int b = 0; b < n; ++b)
      std::printf("%d %d %d %d %d %016llx %016llx %016llx %016llx %016llx %016llx\n", iv[0][b], iv[1][b], iv[2][b], iv[3][b],
                  iv[4][b], bits(dv[0][b]), bits(dv[1][b]), bits(dv[2][b]), bits(hp[3 * b]), bits(hp[3 * b + 1]),
                  bits(hp[3 * b + 2]));
  }
  return 0;
}
