// A host build of k_quad_solve's own text (fuel_amd/csrc/quad_solve.hip between "namespace {" and the host code, cut out
// by tests/golden/check_quad_solve_host_build.py into kernel.inc) on the lanes of tests/golden/host_lanes.h.  Every array
// the kernel sees is a heap block of its exact size; what lies behind a problem's own rows is 1e300, so that a read past
// them shows in the result.  Reads the launches check_quad_solve_host_build.py writes and prints one line per problem:
// the status, the number of entries behind the problem's rows that are not 0, then the bits of cost, pt_dist and every
// control point.
//   host_kernel <in.txt>
#include "host_lanes.h"
#include "kernel.inc"
}  // namespace (kernel.inc leaves it open)

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  std::ifstream in(argv[1]);
  int n_launch;
  in >> n_launch;
  for (int l = 0; l < n_launch; ++l) {
    QuadArgs Q;
    memset(&Q, 0, sizeof(Q));
    int n;
    in >> Q.mask >> Q.dim >> Q.max_ctrl >> Q.end_n >> Q.max_waypt >> Q.bounds >> Q.order >> n;
    Q.ld_smooth = num(in), Q.ld_start = num(in), Q.ld_end = num(in), Q.ld_guide = num(in), Q.ld_waypt = num(in);
    for (double& v : Q.box_lo) v = num(in);
    for (double& v : Q.box_hi) v = num(in);
    const size_t dim = Q.dim, maxc = Q.max_ctrl, maxw = Q.max_waypt;
    const size_t maxg = Q.max_ctrl > 2 * Q.order ? Q.max_ctrl - 2 * Q.order : 0;
    std::vector<int> nc(n), nw(n), idx(n * maxw + 1, 1 << 30);
    std::vector<double> knot(n), ctrl(n * maxc * dim, 1e300), st(n * 3 * dim), en(n * 3 * dim);
    std::vector<double> guide(n * maxg * dim + 1, 1e300), way(n * maxw * dim + 1, 1e300);
    for (int b = 0; b < n; ++b) {
      in >> nc[b];
      knot[b] = num(in);
      in >> nw[b];
      for (size_t k = 0; k < dim * nc[b]; ++k) ctrl[b * maxc * dim + k] = num(in);
      for (size_t k = 0; k < 3 * dim; ++k) st[b * 3 * dim + k] = num(in);
      for (size_t k = 0; k < 3 * dim; ++k) en[b * 3 * dim + k] = num(in);
      const size_t ng = nc[b] > 2 * Q.order ? nc[b] - 2 * Q.order : 0;
      for (size_t k = 0; k < ng * dim; ++k) guide[b * maxg * dim + k] = num(in);
      for (int j = 0; j < nw[b]; ++j) in >> idx[b * maxw + j];
      for (size_t k = 0; k < nw[b] * dim; ++k) way[b * maxw * dim + k] = num(in);
    }
    std::vector<int> status(n, -77);
    std::vector<double> out(n * maxc * dim, -7.0), cost(n, -7.0), pd(n, -7.0);
    Q.n_prob = n, Q.n_ctrl = nc.data(), Q.ctrl = ctrl.data(), Q.ctrl_stride = maxc * dim, Q.knot_span = knot.data();
    Q.vs = Q.dim, Q.start_state = st.data(), Q.end_state = en.data(), Q.guide = guide.data(), Q.guide_stride = maxg * dim;
    Q.n_waypt = nw.data(), Q.waypts = way.data(), Q.waypt_idx = idx.data();
    Q.status = status.data(), Q.ctrl_out = out.data(), Q.cost = cost.data(), Q.pt_dist = pd.data();
    if (const int rc = launch(n, QS_NT, qs_lds(Q.max_ctrl, Q.dim), [&] { k_quad_solve(Q); })) return rc;
    for (int b = 0; b < n; ++b) {
      int tail = 0;
      for (size_t k = dim * nc[b]; k < maxc * dim; ++k) tail += out[b * maxc * dim + k] != 0.0;
      std::printf("%d %d %016llx %016llx", status[b], tail, bits(cost[b]), bits(pd[b]));
      for (size_t k = 0; k < dim * nc[b]; ++k) std::printf(" %016llx", bits(out[b * maxc * dim + k]));
      std::printf("\n");
    }
  }
  return 0;
}
