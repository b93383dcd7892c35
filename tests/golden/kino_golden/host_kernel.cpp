// A host build of k_kino_path's own text (fuel_amd/csrc/kino_path.hip between "namespace {" and the host code, cut out by
// tests/golden/check_kino_host_build.py into kernel.inc) on the lanes of tests/golden/host_lanes.h, with glibc's libm.
// Reads the input files tests/golden/make_kino_golden.py writes for the reference's driver and writes the same output
// format, so the two output files can be compared byte for byte.  With RAW=1 it prints every result instead; FORCE_SEG /
// MAX_SAMPLES / MAX_NODES / LOAD_POINTS set the corresponding fields; guard zones behind the output arrays catch a write
// past a cap.
//   host_kernel <in.txt> <infl.bin> <unk.bin> <out.txt>
#include "host_lanes.h"
#include "kernel.inc"

static void put(FILE* f, double v) { std::fprintf(f, " %a", v); }
int main(int argc, char** argv) {
  std::ifstream in(argv[1]);
  Geo g{};
  KinoArgs K{};
  in >> g.nx >> g.ny >> g.nz;
  g.nyz = g.ny * g.nz, g.N = g.nx * g.nyz, g.W = (g.N + 63) / 64;
  for (int i = 0; i < 3; ++i) in >> g.org[i];
  for (int i = 0; i < 3; ++i) in >> K.map_size[i];
  for (int i = 0; i < 3; ++i) in >> K.box_mind[i];
  for (int i = 0; i < 3; ++i) in >> K.box_maxd[i];
  in >> g.res;
  g.res_inv = 1 / g.res;
  std::vector<signed char> infl(g.N);
  std::vector<unsigned char> unk(g.N);
  std::ifstream(argv[2], std::ios::binary).read((char*)infl.data(), g.N);
  std::ifstream(argv[3], std::ios::binary).read((char*)unk.data(), g.N);
  std::vector<u64> pi(g.W + 2), pu(g.W + 2);
  for (long a = 0; a < g.N; ++a) {
    if (infl[a] == 1) pi[a >> 6] |= 1ull << (a & 63);
    if (unk[a]) pu[a >> 6] |= 1ull << (a & 63);
  }
  fuelmi_kino_cfg c{};
  double alloc, chk, opt;
  in >> c.max_tau >> c.init_max_tau >> c.max_vel >> c.max_acc >> c.w_time >> c.horizon >> c.resolution >> c.lambda_heu >> alloc >> chk >> opt;
  c.allocate_num = (int)alloc, c.check_num = (int)chk, c.optimistic = (int)opt;
  c.res = 0.5, c.time_res = 1.0, c.time_res_init = 1 / 20.0;
  int n;
  in >> c.ts >> n;
  c.min_seg = 8, c.seg_num = 0, c.max_path_nodes = 64, c.max_samples = 256;
  if (getenv("FORCE_SEG")) c.seg_num = atoi(getenv("FORCE_SEG"));
  if (getenv("MAX_SAMPLES")) c.max_samples = atoi(getenv("MAX_SAMPLES"));
  if (getenv("MAX_NODES")) c.max_path_nodes = atoi(getenv("MAX_NODES"));
  const int MS = c.max_samples, MN = c.max_path_nodes;
  std::vector<double> prims;
  int ni, nr;
  // the host loops of kino_prims
  {
    const double step_i = c.time_res_init * c.init_max_tau;
    ni = 0;
    for (double tau = step_i; tau <= c.init_max_tau + 1e-3; tau += step_i) { ++ni; prims.insert(prims.end(), {0.0, 0.0, 0.0, tau}); }
    std::vector<double> acc, dur;
    for (double a = -c.max_acc; a <= c.max_acc + 1e-3; a += c.max_acc * c.res) acc.push_back(a);
    for (double tau = c.time_res * c.max_tau; tau <= c.max_tau; tau += c.time_res * c.max_tau) dur.push_back(tau);
    for (double ax : acc) for (double ay : acc) for (double az : acc) for (double tau : dur) prims.insert(prims.end(), {ax, ay, az, tau});
    nr = (int)(acc.size() * acc.size() * acc.size() * dur.size());
  }
  int cap = 16;
  while (cap < 2 * c.allocate_num) cap <<= 1;
  std::vector<double> inp(15 * n);
  for (int b = 0; b < n; ++b) for (int k = 0; k < 15; ++k) in >> inp[15 * b + k];
  std::vector<unsigned char> pool((size_t)n * c.allocate_num * 128);
  std::vector<int> heap((size_t)n * c.allocate_num), hash((size_t)n * cap, -1);
  std::vector<int> iv(9 * n);
  std::vector<double> dv(3 * n), coef(12 * n), der(12 * n), smp((size_t)n * MS * 3 + 64, -7.0), ns((size_t)n * MN * 6 + 64, -7.0), nin((size_t)n * MN * 3 + 64, -7.0), nd((size_t)n * MN + 64, -7.0);
  K.cfg = c, K.n_prob = n, K.n_init = ni, K.n_reg = nr, K.prims = prims.data();
  K.tolerance = (int)std::ceil(1 / c.resolution), K.inv_res = 1.0 / c.resolution;
  K.infl = pi.data(), K.unk = pu.data(), K.in = inp.data(), K.pool = pool.data(), K.heap = heap.data(), K.hash = hash.data(), K.hash_cap = cap;
  K.status = &iv[0], K.which = &iv[n], K.iter_num = &iv[2 * n], K.use_node_num = &iv[3 * n], K.n_nodes = &iv[4 * n];
  K.shot = &iv[5 * n], K.seg_num = &iv[6 * n], K.n_samples = &iv[7 * n], K.skip = &iv[8 * n];
  K.t_shot = &dv[0], K.T_sum = &dv[n], K.ts_out = &dv[2 * n], K.coef_shot = coef.data(), K.derivs = der.data(), K.samples = smp.data();
  K.node_state = ns.data(), K.node_input = nin.data(), K.node_duration = nd.data();
  if (getenv("LOAD_POINTS")) K.load_points = atoi(getenv("LOAD_POINTS")), K.cfg.seg_num = K.load_points - 1;
  launch(n, KN_NT, 0, [&] { k_kino_path(g, K); });
  for (size_t i = 0; i < 64; ++i)  // guard zones behind the arrays
    if (smp[(size_t)n * MS * 3 + i] != -7.0 || ns[(size_t)n * MN * 6 + i] != -7.0 || nin[(size_t)n * MN * 3 + i] != -7.0 || nd[(size_t)n * MN + i] != -7.0) { std::printf("GUARD HIT\n"); return 9; }
  if (getenv("RAW")) {
    for (int b = 0; b < n; ++b) {
      std::printf("%d %d %d %d %d %d %d %d %d", K.status[b], K.which[b], K.iter_num[b], K.use_node_num[b], K.n_nodes[b], K.shot[b], K.seg_num[b], K.n_samples[b], K.skip[b]);
      std::printf(" %a %a %a", K.t_shot[b], K.T_sum[b], K.ts_out[b]);
      const int live = K.status[b] == 3 || K.status[b] == 5 ? 0 : (K.n_samples[b] < MS ? K.n_samples[b] : MS);
      const int stride = K.load_points > 0 ? K.load_points : MS;
      for (int k = 0; k < 3 * live; ++k) std::printf(" %a", smp[(size_t)b * stride * 3 + k]);
      for (int k = 0; k < 12; ++k) std::printf(" %a", der[12 * b + k]);
      std::printf("\n");
    }
    return 0;
  }
  FILE* out = std::fopen(argv[4], "w");
  for (int b = 0; b < n; ++b) {
    std::fprintf(out, "%d %d %d %d", K.status[b], K.which[b], K.iter_num[b], K.use_node_num[b]);
    if (K.status[b] == 3 || K.status[b] == 5) { std::fprintf(out, "\n"); continue; }
    const int len = K.n_nodes[b];
    std::fprintf(out, " %d", len);
    for (int i = 0; i < len; ++i) {
      const double* s = &ns[((size_t)b * 64 + i) * 6];
      for (int k = 0; k < 3; ++k) std::fprintf(out, " %d", (int)floor((s[k] - g.org[k]) * K.inv_res));
      for (int k = 0; k < 6; ++k) put(out, s[k]);
      for (int k = 0; k < 3; ++k) put(out, nin[((size_t)b * 64 + i) * 3 + k]);
      put(out, nd[(size_t)b * 64 + i]);
    }
    std::fprintf(out, " %d", K.shot[b]);
    put(out, K.t_shot[b]);
    for (int k = 0; k < 12; ++k) put(out, coef[12 * b + k]);
    put(out, K.ts_out[b]);
    std::fprintf(out, " %d", K.n_samples[b]);
    for (int k = 0; k < 3 * K.n_samples[b]; ++k) put(out, smp[(size_t)b * 256 * 3 + k]);
    for (int k = 0; k < 12; ++k) put(out, der[12 * b + k]);
    std::fprintf(out, "\n");
  }
  std::fclose(out);
  return 0;
}
