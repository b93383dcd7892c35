// A host build of k_topo_path's own text and topo_cut (fuel_amd/csrc/topo_path.hip between "namespace {" and the
// workspace's sizing, cut out by tests/golden/check_topo_host_build.py into kernel.inc) on the lanes of
// tests/golden/host_lanes.h.  Reads the input file tests/golden/make_topo_golden.py writes for the reference's driver,
// the field as f32 and the sample stream as f64 (one stream that every problem takes, or one per problem), and prints
// every result; every array the kernel sees is a heap block of its exact size.
//   host_kernel <in.txt> <field.f32> <samples.f64> <max_path_points> <max_nodes>
#include "host_lanes.h"
#include "kernel.inc"

static std::vector<std::unique_ptr<unsigned char[]>> g_blocks;  // owned until the program ends
template <class T>
static T* block(size_t n) {
  g_blocks.emplace_back(new unsigned char[(n ? n : 1) * sizeof(T)]());
  return reinterpret_cast<T*>(g_blocks.back().get());
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  std::ifstream in(argv[1]);
  Geo g{};
  TopoArgs T{};
  in >> g.nx >> g.ny >> g.nz;
  g.nyz = g.ny * g.nz, g.N = g.nx * g.nyz, g.W = (g.N + 63) / 64;
  for (int i = 0; i < 3; ++i) in >> g.org[i];
  in >> g.res;
  g.res_inv = 1 / g.res;
  for (int i = 0; i < 3; ++i) g.minb[i] = g.org[i], g.maxb[i] = g.org[i] + (i == 0 ? g.nx : i == 1 ? g.ny : g.nz) * g.res;
  fuelmi_topo_cfg c{};
  double v[6];
  for (int i = 0; i < 3; ++i) in >> c.sample_inflate[i];
  in >> c.clearance >> c.ratio_to_short;
  for (int i = 0; i < 4; ++i) in >> v[i];
  c.max_sample_num = (int)v[0], c.max_raw_path = (int)v[1], c.max_raw_path2 = (int)v[2], c.reserve_num = (int)v[3];
  c.max_path_points = atoi(argv[4]), c.max_nodes = atoi(argv[5]);
  unsigned seed;
  int n;
  in >> seed >> n;
  float* dist = block<float>(g.N);
  std::ifstream(argv[2], std::ios::binary).read((char*)dist, (size_t)g.N * 4);
  const size_t S = c.max_sample_num, nn = n;
  double* smp = block<double>(nn * S * 3);
  {
    std::ifstream f(argv[3], std::ios::binary);
    f.read((char*)smp, nn * S * 3 * 8);
    const size_t got = (size_t)f.gcount();
    if (got != nn * S * 3 * 8 && got != S * 3 * 8) return 2;
    if (got == S * 3 * 8)
      for (size_t b = 1; b < nn; ++b) memcpy(smp + b * S * 3, smp, S * 3 * 8);
  }
  const int MS = FUELMI_TOPO_MAX_POINTS_IN, ME = FUELMI_TOPO_MAX_POINTS_IN;
  double *inp = block<double>(nn * 6), *sp = block<double>(nn * MS * 3), *ep = block<double>(nn * ME * 3);
  int *nsp = block<int>(nn), *nep = block<int>(nn);
  for (int b = 0; b < n; ++b) {
    for (int k = 0; k < 6; ++k) in >> inp[6 * b + k];
    in >> nsp[b];
    for (int k = 0; k < 3 * nsp[b]; ++k) in >> sp[(size_t)b * MS * 3 + k];
    in >> nep[b];
    for (int k = 0; k < 3 * nep[b]; ++k) in >> ep[(size_t)b * ME * 3 + k];
  }
  T.cfg = c, T.n_prob = n, T.max_start = MS, T.max_end = ME, T.nc = c.max_sample_num + 2;
  T.cut_res = topo_cut(g.res, g.res), T.cut_zero = topo_cut(g.res, 0.0), T.cut_clear = topo_cut(g.res, c.clearance);
  for (int k = 0; k < 3; ++k) T.off[k] = 0.5 - g.org[k] / g.res;
  T.dist = dist, T.in = inp, T.spts = sp, T.epts = ep, T.n_spts = nsp, T.n_epts = nep, T.samples = smp;
  const size_t nc = T.nc, r1 = c.max_raw_path, r2 = c.max_raw_path2, rs = c.reserve_num, PC = TP_PCAP;
  T.node_pos = block<double>(nn * nc * 3), T.node_type = block<unsigned char>(nn * nc), T.alive = block<unsigned char>(nn * nc);
  T.on_stack = block<unsigned char>(nn * nc), T.nb = block<unsigned short>(nn * nc * TP_NB), T.nb_cnt = block<int>(nn * nc);
  T.guards = block<int>(nn * nc), T.dfs_node = block<int>(nn * nc), T.dfs_it = block<int>(nn * nc);
  T.raw_nodes = block<unsigned short>(nn * r1 * TP_RAWN), T.raw_len = block<int>(nn * r1), T.kept = block<int>(nn * r2);
  T.exist = block<int>(nn * std::max(r2, rs)), T.avail = block<int>(nn * r2), T.shortp = block<double>(nn * r2 * PC * 3);
  T.short_len = block<int>(nn * r2), T.selp = block<double>(nn * rs * PC * 3), T.sel_len = block<int>(nn * rs);
  T.buf = block<double>(nn * 2 * PC * 3), T.dis = block<double>(nn * TP_DCAP * 3);
  const size_t maxn = c.max_nodes, mpp = c.max_path_points;
  T.status = block<int>(nn), T.counts = block<int>(nn * 4), T.events = block<int>(nn * 6), T.n_nodes = block<int>(nn);
  T.node_id = block<int>(nn * maxn), T.node_kind = block<int>(nn * maxn), T.node_xyz = block<double>(nn * maxn * 3);
  T.nb_off = block<int>(nn * (maxn + 1)), T.nb_ids = block<int>(nn * 4 * maxn);
  T.raw_paths = block<double>(nn * r2 * mpp * 3), T.raw_plen = block<int>(nn * r2);
  T.filt_paths = block<double>(nn * r2 * mpp * 3), T.filt_plen = block<int>(nn * r2);
  T.sel_paths = block<double>(nn * rs * mpp * 3), T.sel_plen = block<int>(nn * rs), T.sel_length = block<double>(nn * rs);
  const int rc = launch(n, TP_NT, 0, [&] { k_topo_path(g, T); });
  if (rc) return rc;
  for (size_t b = 0; b < nn; ++b) {
    std::printf("%d", T.status[b]);
    for (int k = 0; k < 4; ++k) std::printf(" %d", T.counts[4 * b + k]);
    for (int k = 0; k < 6; ++k) std::printf(" %d", T.events[6 * b + k]);
    const int live = std::min<int>(T.n_nodes[b], (int)maxn);
    std::printf(" %d", T.n_nodes[b]);
    for (int i = 0; i < live; ++i) {
      std::printf(" %d %d", T.node_id[b * maxn + i], T.node_kind[b * maxn + i]);
      for (int k = 0; k < 3; ++k) std::printf(" %016llx", bits(T.node_xyz[(b * maxn + i) * 3 + k]));
      const int o0 = T.nb_off[b * (maxn + 1) + i], o1 = T.nb_off[b * (maxn + 1) + i + 1];
      std::printf(" %d", o1 - o0);
      for (int o = o0; o < o1; ++o) std::printf(" %d", T.nb_ids[b * 4 * maxn + o]);
    }
    struct Set { double* p; int* len; size_t rows; };
    const Set sets[3] = {{T.raw_paths, T.raw_plen, r2}, {T.filt_paths, T.filt_plen, r2}, {T.sel_paths, T.sel_plen, rs}};
    for (const Set& s : sets) {
      int rows = 0;
      while (rows < (int)s.rows && s.len[b * s.rows + rows] > 0) ++rows;
      std::printf(" %d", rows);
      for (int r = 0; r < rows; ++r) {
        const int len = s.len[b * s.rows + r];
        std::printf(" %d", len);
        for (int k = 0; k < 3 * std::min<int>(len, (int)mpp); ++k) std::printf(" %016llx", bits(s.p[(b * s.rows + r) * mpp * 3 + k]));
      }
    }
    for (size_t r = 0; r < rs && T.sel_plen[b * rs + r] > 0; ++r) std::printf(" %016llx", bits(T.sel_length[b * rs + r]));
    std::printf("\n");
  }
  return 0;
}
