// A host build of k_local_segment's own text (fuel_amd/csrc/local_segment.hip between "namespace {" and the host code,
// cut out by tests/golden/check_localseg_host_build.py into kernel.inc) on the lanes of tests/golden/host_lanes.h.  The
// states, the problems and the result arrays are heap blocks of their exact size; what lies between a state's own rows
// and its stride is 1e300, so that a read past a state's own data shows in the results.  Reads the launches
// check_localseg_host_build.py writes and prints one line per problem: the integers, then the bits of the doubles.
//   host_kernel <in.txt>
// in.txt: launches
//   L n_traj n_prob degree max_seg max_ctrl max_points need_points
//     per state    n_seg global_duration n_local span local_ts local_te time_change last_time_inc <times> <coef> <ctrl>
//     per problem  state mode start_t arg0 arg1
#include "host_lanes.h"
#include "spline_internal.h"
#include "poly_internal.h"
#include "kernel.inc"
}  // namespace (kernel.inc leaves it open)

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  std::ifstream in(argv[1]);
  std::string kind;
  while (in >> kind) {
    LocalSegArgs A;
    memset(&A, 0, sizeof(A));
    int nt, n;
    in >> nt >> n >> A.cfg.degree >> A.cfg.max_seg >> A.cfg.max_ctrl >> A.cfg.max_points >> A.need_points;
    const int ms = A.cfg.max_seg, mc = A.cfg.max_ctrl, mp = A.cfg.max_points;
    std::vector<int> n_seg(nt), n_local(nt), traj_of(n), mode(n);
    std::vector<double> T((size_t)nt * ms, 1e300), cf((size_t)nt * ms * 18, 1e300), C((size_t)nt * mc * 3, 1e300), gd(nt),
        span(nt), lts(nt), lte(nt), tchg(nt), linc(nt), start_t(n), arg0(n), arg1(n);
    for (int i = 0; i < nt; ++i) {
      in >> n_seg[i];
      gd[i] = num(in);
      in >> n_local[i];
      span[i] = num(in), lts[i] = num(in), lte[i] = num(in), tchg[i] = num(in), linc[i] = num(in);
      for (int k = 0; k < n_seg[i]; ++k) T[(size_t)i * ms + k] = num(in);
      for (int k = 0; k < 18 * n_seg[i]; ++k) cf[(size_t)i * ms * 18 + k] = num(in);
      for (int k = 0; k < 3 * n_local[i]; ++k) C[(size_t)i * mc * 3 + k] = num(in);
    }
    for (int b = 0; b < n; ++b) {
      in >> traj_of[b] >> mode[b];
      start_t[b] = num(in), arg0[b] = num(in), arg1[b] = num(in);
    }
    std::vector<int> iv[6];
    for (auto& v : iv) v.assign(n, 0);
    std::vector<double> seg_len(n, 0.0), dur(n, 0.0), dt(n, 0.0), pts((size_t)n * mp * 3, 0.0), der((size_t)n * 12, 0.0);
    A.n_prob = n;
    A.n_seg = n_seg.data(), A.seg_times = T.data(), A.coef = cf.data(), A.gdur = gd.data(), A.n_local = n_local.data();
    A.local_ctrl = C.data(), A.span = span.data(), A.lts = lts.data(), A.lte = lte.data(), A.tchg = tchg.data();
    A.linc = linc.data(), A.traj_of = traj_of.data(), A.mode = mode.data(), A.start_t = start_t.data();
    A.arg0 = arg0.data(), A.arg1 = arg1.data();
    A.status = iv[0].data(), A.n_steps = iv[1].data(), A.seg_num = iv[2].data(), A.n_points = iv[3].data();
    A.n_ctrl = iv[4].data(), A.fit_k = iv[5].data();
    A.segment_len = seg_len.data(), A.duration = dur.data(), A.dt = dt.data(), A.points = pts.data(), A.derivs = der.data();
    if (const int rc = launch((n + LS_WAVES - 1) / LS_WAVES, LS_WIN * LS_WAVES, ls_lds(A.cfg), [&] { k_local_segment(A); }))
      return rc;
    for (int b = 0; b < n; ++b) {
      std::printf("%d %d %d %d %d %d %016llx %016llx %016llx", iv[0][b], iv[1][b], iv[2][b], iv[3][b], iv[4][b], iv[5][b],
                  bits(seg_len[b]), bits(dur[b]), bits(dt[b]));
      for (int k = 0; k < 12; ++k) std::printf(" %016llx", bits(der[(size_t)b * 12 + k]));
      for (int k = 0; k < 3 * mp; ++k) std::printf(" %016llx", bits(pts[(size_t)b * mp * 3 + k]));  // every row: zeros behind
      std::printf("\n");
    }
  }
  return 0;
}
