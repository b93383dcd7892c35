// A host build of k_traj_adjust's and k_traj_select's own text (fuel_amd/csrc/traj_adjust.hip between "namespace {" and
// the host code, cut out by tests/golden/check_traj_adjust_host_build.py into kernel.inc, with
// fuel_amd/csrc/spline_internal.h included as it is): a thread per lane, the wave's meeting point (ta_wave_sync) a
// per-wave std::barrier, __shfl an exchange through a per-wave block behind that barrier, the LDS block a heap block of
// exactly the launch's size between two guard zones.  Meant for -fsanitize=address,undefined: a read or write past the
// knots, the control points or a result array (each a heap block of its exact size) is reported by the sanitizer, one
// inside a guard zone by the check below.  Reads the launches check_traj_adjust_host_build.py writes and prints per
// problem four lines (info; the bits of metrics, knots_out and samples) and per launch the line of best.
//   host_kernel <in.txt>
#define __HIP_PLATFORM_AMD__ 1
#include "fuelmi_internal.h"
#include <barrier>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <thread>
#include <vector>
using namespace std;
#undef __launch_bounds__
#define __launch_bounds__(x)
struct Idx { int x; };
static thread_local Idx threadIdx_, blockIdx_, blockDim_;
#define threadIdx threadIdx_
#define blockIdx blockIdx_
#define blockDim blockDim_
struct WaveBlock {
  std::barrier<> bar{64};
  double d[64];
  int p[64];
};
static WaveBlock* g_waves;
static inline WaveBlock& my_wave() { return g_waves[threadIdx_.x >> 6]; }
static inline void ta_wave_sync() { my_wave().bar.arrive_and_wait(); }
static double host_shfl(double v, int src) {
  WaveBlock& w = my_wave();
  w.d[threadIdx_.x & 63] = v;
  w.bar.arrive_and_wait();
  const double r = w.d[src];
  w.bar.arrive_and_wait();
  return r;
}
static int host_shfl(int v, int src) {
  WaveBlock& w = my_wave();
  w.p[threadIdx_.x & 63] = v;
  w.bar.arrive_and_wait();
  const int r = w.p[src];
  w.bar.arrive_and_wait();
  return r;
}
#define __shfl host_shfl
void fuelmi_set_error(const char*, ...) {}
static unsigned char* g_lds;  // the launch's LDS block (kernel.inc: `unsigned char* smem_raw = g_lds;`)
#include "spline_internal.h"
#include "kernel.inc"
}  // namespace (kernel.inc leaves it open)

static unsigned long long bits(double v) {
  unsigned long long b;
  memcpy(&b, &v, 8);
  return b;
}
static double num(std::ifstream& in) {
  std::string s;
  in >> s;
  return strtod(s.c_str(), nullptr);
}
static void line(const std::vector<double>& v, size_t at, size_t n) {
  for (size_t k = 0; k < n; ++k) std::printf("%s%016llx", k ? " " : "", bits(v[at + k]));
  std::printf("\n");
}

template <class K>
static void launch(K kernel, const TrajAdjArgs& A, int blocks, int waves) {
  for (int blk = 0; blk < blocks; ++blk) {
    std::unique_ptr<WaveBlock[]> wb(new WaveBlock[waves]);
    g_waves = wb.get();
    std::vector<std::thread> th;
    for (int i = 0; i < 64 * waves; ++i)
      th.emplace_back([&, i, blk] {
        threadIdx_.x = i, blockIdx_.x = blk, blockDim_.x = 64 * waves;
        kernel(A);
      });
    for (auto& x : th) x.join();
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  std::ifstream in(argv[1]);
  int n_launch;
  in >> n_launch;
  constexpr size_t GUARD = 256;
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
    const size_t lds = ta_lds(c);
    const int waves = ta_waves(c.max_ctrl);
    std::unique_ptr<unsigned char[]> block(new unsigned char[lds + 2 * GUARD]);
    memset(block.get(), 0xA5, lds + 2 * GUARD);
    g_lds = block.get() + GUARD;
    launch(k_traj_adjust, A, (n + waves - 1) / waves, waves);
    for (size_t i = 0; i < GUARD; ++i)
      if (block[i] != 0xA5 || block[GUARD + lds + i] != 0xA5) {
        std::printf("GUARD HIT\n");
        return 9;
      }
    if (A.best) launch(k_traj_select, A, c.n_group, 1);
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
