// A host build of k_traj_check's own text (fuel_amd/csrc/traj_check.hip between "namespace {" and the host code, cut out
// by tests/golden/check_traj_check_host_build.py into kernel.inc, with fuel_amd/csrc/spline_internal.h included as it
// is): a thread per lane, std::barrier for __syncthreads, the wave operations (__ballot, __shfl, __shfl_up) as exchanges
// through a per-wave block behind a per-wave barrier, the LDS block a heap block of exactly the launch's size between two
// guard zones.  Meant for -fsanitize=address,undefined: a read or write past the knots, the control points, the plane
// or the result arrays (each a heap block of its exact size) is reported by the sanitizer, one inside a guard zone by
// the check below.  Reads the problems check_traj_check_host_build.py writes and prints one line per problem: the five
// integers, then the bits of the six doubles.
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
static thread_local Idx threadIdx_, blockIdx_;
#define threadIdx threadIdx_
#define blockIdx blockIdx_
static std::barrier<>* g_bar;
#define __syncthreads() g_bar->arrive_and_wait()
struct WaveBlock {
  std::barrier<> bar{64};
  double d[64];
  int p[64];
};
static WaveBlock* g_waves;
static inline WaveBlock& my_wave() { return g_waves[threadIdx_.x >> 6]; }
static unsigned long long host_ballot(bool p) {
  WaveBlock& w = my_wave();
  w.p[threadIdx_.x & 63] = p ? 1 : 0;
  w.bar.arrive_and_wait();
  unsigned long long m = 0;
  for (int i = 0; i < 64; ++i) m |= (unsigned long long)w.p[i] << i;
  w.bar.arrive_and_wait();
  return m;
}
static double host_shfl(double v, int src) {
  WaveBlock& w = my_wave();
  w.d[threadIdx_.x & 63] = v;
  w.bar.arrive_and_wait();
  const double r = w.d[src];
  w.bar.arrive_and_wait();
  return r;
}
static double host_shfl_up(double v, int delta) {
  WaveBlock& w = my_wave();
  const int lane = threadIdx_.x & 63;
  w.d[lane] = v;
  w.bar.arrive_and_wait();
  const double r = lane >= delta ? w.d[lane - delta] : v;
  w.bar.arrive_and_wait();
  return r;
}
#define __ballot host_ballot
#define __shfl host_shfl
#define __shfl_up host_shfl_up
static inline bool bit_at(const u64* pl, long a) { return (pl[a >> 6] >> (a & 63)) & 1ull; }
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
    std::string a, b, c, d;
    in >> g.nx >> g.ny >> g.nz >> a >> b >> c >> d;
    g.org[0] = strtod(a.c_str(), nullptr), g.org[1] = strtod(b.c_str(), nullptr), g.org[2] = strtod(c.c_str(), nullptr);
    g.res_inv = strtod(d.c_str(), nullptr);
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
  constexpr size_t GUARD = 256;
  for (int l = 0; l < n_launch; ++l) {
    int map, n, maxc;
    std::string s_step, s_rad;
    TrajChkArgs T;
    memset(&T, 0, sizeof(T));
    in >> map >> n >> T.cfg.degree >> maxc >> s_step >> s_rad;
    T.cfg.max_ctrl = maxc, T.cfg.step = strtod(s_step.c_str(), nullptr), T.cfg.max_radius = strtod(s_rad.c_str(), nullptr);
    std::vector<int> nc(n);
    std::vector<double> knot(n), now(n), pos((size_t)n * maxc * 3, 1e300);  // (a read past a problem's own points shows)
    for (int b = 0; b < n; ++b) {
      std::string s;
      in >> nc[b] >> s;
      knot[b] = strtod(s.c_str(), nullptr);
      in >> s;
      now[b] = strtod(s.c_str(), nullptr);
      for (int k = 0; k < 3 * nc[b]; ++k) {
        in >> s;
        pos[(size_t)b * maxc * 3 + k] = strtod(s.c_str(), nullptr);
      }
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
    const size_t lds = tc_lds(maxc);
    const int nt = TC_WIN * TC_WAVES;
    for (int blk = 0; blk < (n + TC_WAVES - 1) / TC_WAVES; ++blk) {
      std::unique_ptr<unsigned char[]> block(new unsigned char[lds + 2 * GUARD]);
      memset(block.get(), 0xA5, lds + 2 * GUARD);
      g_lds = block.get() + GUARD;
      std::barrier<> bar(nt);
      g_bar = &bar;
      std::unique_ptr<WaveBlock[]> waves(new WaveBlock[TC_WAVES]);
      g_waves = waves.get();
      std::vector<std::thread> th;
      for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t, blk] {
          threadIdx_.x = t;
          blockIdx_.x = blk;
          k_traj_check(geo[map], T);
          bar.arrive_and_drop();
        });
      for (auto& t : th) t.join();
      for (size_t i = 0; i < GUARD; ++i)
        if (block[i] != 0xA5 || block[GUARD + lds + i] != 0xA5) {
          std::printf("GUARD HIT\n");
          return 9;
        }
    }
    for (int b = 0; b < n; ++b)
      std::printf("%d %d %d %d %d %016llx %016llx %016llx %016llx %016llx %016llx\n", iv[0][b], iv[1][b], iv[2][b], iv[3][b],
                  iv[4][b], bits(dv[0][b]), bits(dv[1][b]), bits(dv[2][b]), bits(hp[3 * b]), bits(hp[3 * b + 1]),
                  bits(hp[3 * b + 2]));
  }
  return 0;
}
