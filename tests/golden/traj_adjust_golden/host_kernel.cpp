// A host build of k_traj_adjust's and k_traj_select's own text (fuel_amd/csrc/traj_adjust.hip between "namespace {" and
// the host code, cut out by tests/golden/check_traj_adjust_host_build.py into kernel.inc) on the lanes of
// tests/golden/host_lanes.h; the wave's meeting point (ta_wave_sync) is the per-wave barrier.  The knots, the control
// points and every result array are heap blocks of their exact size.  Reads the launches
// check_traj_adjust_host_build.py writes and prints per problem four lines (info; the bits of metrics, knots_out and
// samples) and per launch the line of best.
//   host_kernel <in.txt>
#include "host_lanes.h"
static inline void ta_wave_sync() { wave_barrier(); }
#include "spline_internal.h"
#include "kernel.inc"
}  // namespace (kernel.inc leaves it open)

static void line(const std::vector<double>& v, size_t at, size_t n) {
  for (size_t k = 0; k < n; ++k) std::printf("%s%016llx", k ? " " : "", bits(v[at + k]));
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  std::ifstream in(argv[1]);
  int n_launch;
  in >> n_launch;
  for (int l = 0; l < n_launch; ++l) {
    TrajAdjArgs A;
    memset(&A, 0, sizeof(A));
    fuelmi_trajadj_cfg& c = A.cfg;
    int n, has_knots, has_ratio, device_batch;
    in >> c.ops >> c.degree >> c.max_ctrl >> c.max_samples >> c.realloc_iters >> c.n_group >> n >> has_knots >> has_ratio >>
        device_batch;
    c.limit_vel = num(in), c.limit_acc = num(in), c.limit_ratio = num(in), c.lengthen_cap = num(in);
    c.length_res = num(in), c.stat_step = num(in);
    const size_t ks = (size_t)c.max_ctrl + c.degree + 1, ms = (size_t)(c.max_samples > 0 ? c.max_samples : 0);
    // (1e300 / -7: a read past a problem's own points or knots shows in the results)
    std::vector<int> nc(n), group(n), info((size_t)n * FUELMI_TRAJADJ_NI, -77), best((size_t)(c.n_group > 0 ? c.n_group : 0), -77);
    std::vector<double> knot(n), pos((size_t)n * c.max_ctrl * 3, 1e300), kin((size_t)n * ks, 1e300), ratio(n),
        met((size_t)n * FUELMI_TRAJADJ_NM, -7.0), kout((size_t)n * ks, -7.0), smp((size_t)n * ms * 3, -7.0);
    for (int b = 0; b < n; ++b) {
      in >> nc[b] >> group[b];
      knot[b] = num(in), ratio[b] = num(in);
      for (int k = 0; k < 3 * nc[b]; ++k) pos[(size_t)b * c.max_ctrl * 3 + k] = num(in);
      if (has_knots)
        for (int k = 0; k < nc[b] + c.degree + 1; ++k) kin[(size_t)b * ks + k] = num(in);
    }
    A.n_prob = n;
    if (device_batch)  // every problem has the stride's number of points, as in a batch
      A.src.n_ctrl = nullptr, A.src.n_ctrl_all = c.max_ctrl;
    else
      A.src.n_ctrl = nc.data();
    A.src.pos = pos.data(), A.src.pos_stride = (size_t)c.max_ctrl * 3, A.src.knot = knot.data(), A.src.knot_stride = 1;
    if (has_knots) A.knots_in = kin.data();
    if (has_ratio) A.ratio_in = ratio.data();
    A.group = group.data(), A.info = info.data(), A.metrics = met.data(), A.knots_out = kout.data();
    A.samples = (c.ops & FUELMI_TRAJADJ_RESAMPLE) ? smp.data() : nullptr;
    A.best = (c.ops & FUELMI_TRAJADJ_SELECT) ? best.data() : nullptr;
    const int waves = ta_waves(c.max_ctrl);
    if (const int rc = launch((n + waves - 1) / waves, 64 * waves, ta_lds(c), [&] { k_traj_adjust(A); })) return rc;
    if (A.best) launch(c.n_group, 64, 0, [&] { k_traj_select(A); });
    for (int b = 0; b < n; ++b) {
      for (int k = 0; k < FUELMI_TRAJADJ_NI; ++k) std::printf("%s%d", k ? " " : "", info[(size_t)b * FUELMI_TRAJADJ_NI + k]);
      std::printf("\n");
      line(met, (size_t)b * FUELMI_TRAJADJ_NM, FUELMI_TRAJADJ_NM);
      line(kout, (size_t)b * ks, ks);
      line(smp, (size_t)b * ms * 3, A.samples ? ms * 3 : 0);
    }
    std::printf("B");
    for (int v : best) std::printf(" %d", A.best ? v : -77);
    std::printf("\n");
  }
  return 0;
}
