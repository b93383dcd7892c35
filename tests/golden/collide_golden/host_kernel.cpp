// A host build of k_collide_range's and k_guide_points' own text (fuel_amd/csrc/collide_range.hip between "namespace {"
// and the host code, cut out by tests/golden/check_collide_host_build.py into kernel.inc) on the lanes of
// tests/golden/host_lanes.h.  The knots, the control points, the field, the paths and the result arrays are heap blocks of
// their exact size.  Reads the launches check_collide_host_build.py writes and prints one line per problem: the integers,
// then the bits of the doubles.
//   host_kernel <in.txt>
// in.txt: the maps (nx ny nz, origin, res_inv, res, the file of the f32 field), then launches
//   R map n degree max_ctrl max_events max_pts clearance, then per problem n_ctrl dt <control points>
//   G n max_path_points degree max_guide ctrl_pt_dist, then per path len duration <points>
#include "host_lanes.h"
#include "spline_internal.h"
#include "kernel.inc"
}  // namespace (kernel.inc leaves it open)

static void put_rows(const std::vector<double>& a, size_t at, int count, int cap) {
  for (int i = 0; i < 3 * (count < cap ? count : cap); ++i) std::printf(" %016llx", bits(a[at + i]));
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  std::ifstream in(argv[1]);
  int n_maps;
  in >> n_maps;
  std::vector<Geo> geo(n_maps);
  std::vector<std::vector<float>> field(n_maps);
  for (int m = 0; m < n_maps; ++m) {
    Geo& g = geo[m];
    memset(&g, 0, sizeof(g));
    in >> g.nx >> g.ny >> g.nz;
    for (double& o : g.org) o = num(in);
    g.res_inv = num(in), g.res = num(in);
    g.nyz = g.ny * g.nz, g.N = g.nx * g.nyz, g.W = (g.N + 63) / 64;
    std::string path;
    in >> path;
    field[m].resize(g.N);  // exactly the map's voxels: the sanitizer sees a read past them
    std::ifstream(path, std::ios::binary).read(reinterpret_cast<char*>(field[m].data()), g.N * sizeof(float));
  }
  std::string kind;
  while (in >> kind) {
    if (kind == "R") {
      int map, n;
      ColRangeArgs T;
      memset(&T, 0, sizeof(T));
      in >> map >> n >> T.cfg.degree >> T.cfg.max_ctrl >> T.cfg.max_events >> T.cfg.max_pts;
      T.cfg.clearance = num(in);
      const int maxc = T.cfg.max_ctrl, ev = T.cfg.max_events, mp = T.cfg.max_pts;
      std::vector<int> nc(n);
      std::vector<double> knot(n), pos((size_t)n * maxc * 3, 1e300);  // (a read past a problem's own points shows)
      for (int b = 0; b < n; ++b) {
        in >> nc[b];
        knot[b] = num(in);
        for (int k = 0; k < 3 * nc[b]; ++k) pos[(size_t)b * maxc * 3 + k] = num(in);
      }
      std::vector<int> iv[6];
      for (auto& v : iv) v.assign(n, 0);
      std::vector<double> ts(n, 0.0), te(n, 0.0), cs((size_t)n * ev * 3, 0.0), ce((size_t)n * ev * 3, 0.0),
          sp((size_t)n * mp * 3, 0.0), ep((size_t)n * mp * 3, 0.0), fs((size_t)n * 3, 0.0), le((size_t)n * 3, 0.0);
      T.n_prob = n, T.src = {nc.data(), 0, pos.data(), (size_t)maxc * 3, knot.data(), 1};
      T.cut = field_cut(geo[map].res, T.cfg.clearance, true);
      T.dist = field[map].data();
      T.status = iv[0].data(), T.n_ticks = iv[1].data(), T.n_start_events = iv[2].data(), T.n_end_events = iv[3].data();
      T.n_start_pts = iv[4].data(), T.n_end_pts = iv[5].data();
      T.t_s = ts.data(), T.t_e = te.data(), T.colli_start = cs.data(), T.colli_end = ce.data();
      T.start_pts = sp.data(), T.end_pts = ep.data(), T.first_start = fs.data(), T.last_end = le.data();
      if (const int rc = launch((n + CR_WAVES - 1) / CR_WAVES, CR_WIN * CR_WAVES, cr_lds(maxc), [&] { k_collide_range(geo[map], T); }))
        return rc;
      for (int b = 0; b < n; ++b) {
        std::printf("%d %d %d %d %d %d %016llx %016llx", iv[0][b], iv[1][b], iv[2][b], iv[3][b], iv[4][b], iv[5][b], bits(ts[b]),
                    bits(te[b]));
        put_rows(fs, (size_t)b * 3, 1, 1), put_rows(le, (size_t)b * 3, 1, 1);
        put_rows(cs, (size_t)b * ev * 3, iv[2][b], ev), put_rows(ce, (size_t)b * ev * 3, iv[3][b], ev);
        put_rows(sp, (size_t)b * mp * 3, iv[4][b], mp), put_rows(ep, (size_t)b * mp * 3, iv[5][b], mp);
        std::printf("\n");
      }
    } else {
      GuideArgs G;
      memset(&G, 0, sizeof(G));
      int n;
      in >> n >> G.max_path_points >> G.degree >> G.max_guide;
      G.ctrl_pt_dist = num(in);
      G.n_path = n;
      const int mpp = G.max_path_points, mg = G.max_guide;
      std::vector<int> len(n);
      std::vector<double> dur(n), paths((size_t)n * mpp * 3, 1e300);
      for (int b = 0; b < n; ++b) {
        in >> len[b];
        dur[b] = num(in);
        for (int k = 0; k < 3 * len[b]; ++k) paths[(size_t)b * mpp * 3 + k] = num(in);
      }
      std::vector<int> iv[5];
      for (auto& v : iv) v.assign(n, 0);
      std::vector<double> dt(n, 0.0), gp((size_t)n * mg * 3, 0.0);
      G.paths = paths.data(), G.path_len = len.data(), G.duration = dur.data();
      G.status = iv[0].data(), G.seg_num = iv[1].data(), G.n_pts = iv[2].data(), G.n_ctrl = iv[3].data(), G.n_guide = iv[4].data();
      G.dt = dt.data(), G.guide_pts = gp.data();
      if (const int rc = launch(n, GP_NT, 0, [&] { k_guide_points(G); })) return rc;
      for (int b = 0; b < n; ++b) {
        std::printf("%d %d %d %d %d %016llx", iv[0][b], iv[1][b], iv[2][b], iv[3][b], iv[4][b], bits(dt[b]));
        put_rows(gp, (size_t)b * mg * 3, iv[4][b], mg);
        std::printf("\n");
      }
    }
  }
  return 0;
}
