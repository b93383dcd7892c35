// frontier_query.hip -- read-back of the frontier finder's results: cluster counts, cells, voxel centres,
// down-sampled cells and records of the new / committed / dormant / previous cluster lists, the removed ids and
// the flag plane.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <list>
#include <mutex>
#include <thread>
#include <vector>

#include "frontier_internal.h"

__global__ void k_expand_flag_bits(const u64* __restrict__ bits, long n, char* __restrict__ out) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (long)gridDim.x * blockDim.x) out[i] = (char)((bits[i >> 6] >> (i & 63)) & 1ull);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static const std::list<HCluster>* pick(const fuelmi_frontier* f, int which) {
  return which == 0 ? &f->tmp : (which == 1 ? &f->frontiers : (which == 2 ? &f->dormant : (which == 3 ? &f->prev : nullptr)));
}
static const HCluster* nth(const fuelmi_frontier* f, int which, int k) {
  const std::list<HCluster>* L = pick(f, which);
  if (!L || k < 0 || k >= (int)L->size()) return nullptr;
  auto it = L->begin();
  std::advance(it, k);
  return &*it;
}
extern "C" int fuelmi_frontier_count(const fuelmi_frontier* f, int which) {
  ARGCHK(f && pick(f, which));
  return (int)pick(f, which)->size();
}
extern "C" int fuelmi_frontier_cluster_size(const fuelmi_frontier* f, int which, int k) {
  ARGCHK(f);
  const HCluster* c = nth(f, which, k);
  ARGCHK(c);
  return (int)c->size();
}
extern "C" int fuelmi_frontier_cluster_cells(const fuelmi_frontier* f, int which, int k, int* adr) {
  ARGCHK(f && adr);
  const HCluster* c = nth(f, which, k);
  ARGCHK(c);
  if (c->lazy) {
    int rc = which == 3 ? frontier_prev_ready(f) : frontier_cells_ready(f);
    if (rc) return rc;
  }
  {
    const int rcf = frontier_fetch_cluster(f, c);
    if (rcf) return rcf;
  }
  c->copy_to(adr);
  return FUELMI_OK;
}
// A few helper threads for the host-side bulk steps of result delivery (decoding a large cluster's cells): created on
// first use, parked on a condition variable, shared by every finder of the process.  FUELMI_HOST_HELPERS=0 switches them
// off (everything then runs on the calling thread).
namespace {
struct HostHelpers {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv_go, cv_done;
  const std::function<void(size_t, size_t)>* job = nullptr;
  size_t n = 0, piece = 0;
  std::atomic<size_t> next{0};
  int gen = 0, running = 0;
  bool stop = false;
  void worker() {
    int seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_go.wait(lk, [&] { return stop || gen != seen; });
        if (stop) return;
        seen = gen;
      }
      take();
      {
        std::lock_guard<std::mutex> lk(mu);
        if (--running == 0) cv_done.notify_one();
      }
    }
  }
  void take() {
    for (;;) {
      const size_t i0 = next.fetch_add(piece);
      if (i0 >= n) return;
      (*job)(i0, std::min(n, i0 + piece));
    }
  }
  void run(size_t total, const std::function<void(size_t, size_t)>& f) {
    static const int want = getenv("FUELMI_HOST_HELPERS") ? atoi(getenv("FUELMI_HOST_HELPERS")) : 3;
    if (want <= 0) {
      f(0, total);
      return;
    }
    std::unique_lock<std::mutex> lk(mu);
    if (th.empty())
      for (int k = 0; k < want; ++k) th.emplace_back([this] { worker(); });
    job = &f, n = total, piece = std::max<size_t>(8192, (total + 4 * (th.size() + 1) - 1) / (4 * (th.size() + 1)));
    next = 0;
    running = (int)th.size();
    ++gen;
    lk.unlock();
    cv_go.notify_all();
    take();  // the caller works too
    lk.lock();
    cv_done.wait(lk, [&] { return running == 0; });
  }
  ~HostHelpers() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv_go.notify_all();
    for (auto& t : th) t.join();
  }
};
std::mutex g_helpers_once;
}  // namespace
static void host_parallel_for(size_t n, const std::function<void(size_t, size_t)>& f) {
  static HostHelpers* H = new HostHelpers;  // (leaked on purpose: joining threads from a static destructor at exit can hang)
  std::lock_guard<std::mutex> lk(g_helpers_once);  // one bulk step at a time
  H->run(n, f);
}

// Frontier::cells_ as the reference's callers hold them: the voxel CENTRES of cluster k, three doubles per cell (the
// layout of a vector<Eigen::Vector3d>), decoded by the library straight out of the pinned result block into the
// caller's storage -- no intermediate address list, and no division per cell: consecutive cells of a list mostly share
// a z-line (ascending addresses) or neighbour one (BFS order), so the line's base address is carried along.
extern "C" int fuelmi_frontier_cluster_centres(const fuelmi_frontier* f, int which, int k, double* xyz) {
  ARGCHK(f && xyz);
  const HCluster* c = nth(f, which, k);
  ARGCHK(c);
  if (c->lazy) {
    int rc = which == 3 ? frontier_prev_ready(f) : frontier_cells_ready(f);
    if (rc) return rc;
  }
  if (!f->map) {
    fuelmi_set_error("fuelmi_frontier_cluster_centres: the map of this finder has been destroyed");
    return FUELMI_EINVAL;
  }
  {
    const int rcf = frontier_fetch_cluster(f, c);
    if (rcf) return rcf;
  }
  const Geo& g = f->map->g;
  const size_t n = c->size();
  // (a cluster started by an NQ seed keeps the seed apart from its sorted list: materialise the merged order first)
  std::vector<int> merged;
  const int* adr = nullptr;
  if (c->lazy && c->lazy_seed < 0)
    adr = c->lazy;
  else if (!c->lazy)
    adr = c->cells.data();
  else {
    merged.resize(n);
    c->copy_to(merged.data());
    adr = merged.data();
  }
  const double res = g.res, ox = g.org[0], oy = g.org[1], oz = g.org[2];
  const unsigned nz = (unsigned)g.nz, nyz = (unsigned)g.nyz;
  auto decode = [&](size_t i0, size_t i1) {
    // address of z = 0 of the current z-line; the start value makes the first cell decode whatever its address is
    // (addresses are below 2^31; 0xFFFFFFFF made a - lb wrap to a + 1 < nz for cells of the column x = y = 0)
    unsigned lb = 0x80000000u;
    double cx = 0.0, cy = 0.0;
    for (size_t i = i0; i < i1; ++i) {
      const unsigned a = (unsigned)adr[i];
      unsigned z = a - lb;
      if (z >= nz) {  // another line
        const unsigned x = a / nyz, r = a - x * nyz, y = r / nz;
        z = r - y * nz;
        lb = a - z;
        cx = (x + 0.5) * res + ox, cy = (y + 0.5) * res + oy;
      }
      xyz[3 * i] = cx, xyz[3 * i + 1] = cy, xyz[3 * i + 2] = (z + 0.5) * res + oz;
    }
  };
  // a map-spanning cluster (140 k cells = 3.4 MB of doubles) is decoded by the caller and three helper threads of the
  // library: one host thread writing it was the longest single step of a full-box cycle through the facade
  if (n >= 32768)
    host_parallel_for(n, decode);
  else
    decode(0, n);
  return FUELMI_OK;
}
extern "C" int fuelmi_frontier_cluster_filtered_size(const fuelmi_frontier* f, int which, int k) {
  ARGCHK(f);
  const HCluster* c = nth(f, which, k);
  ARGCHK(c);
  return (int)(c->filtered.size() / 3);
}
extern "C" int fuelmi_frontier_cluster_filtered(const fuelmi_frontier* f, int which, int k, float* xyz) {
  ARGCHK(f && xyz);
  const HCluster* c = nth(f, which, k);
  ARGCHK(c);
  if (!c->filtered.empty()) memcpy(xyz, c->filtered.data(), c->filtered.size() * sizeof(float));
  return FUELMI_OK;
}
extern "C" int fuelmi_frontier_cluster_info(const fuelmi_frontier* f, int which, int k, double out9[9]) {
  ARGCHK(f && out9);
  const HCluster* c = nth(f, which, k);
  ARGCHK(c);
  for (int i = 0; i < 3; ++i) out9[i] = c->avg[i], out9[3 + i] = c->bmin[i], out9[6 + i] = c->bmax[i];
  return FUELMI_OK;
}
extern "C" int fuelmi_frontier_removed_count(const fuelmi_frontier* f) {
  ARGCHK(f);
  return (int)f->removed_ids.size();
}
extern "C" int fuelmi_frontier_removed_ids(const fuelmi_frontier* f, int* ids) {
  ARGCHK(f && ids);
  memcpy(ids, f->removed_ids.data(), f->removed_ids.size() * sizeof(int));
  return FUELMI_OK;
}
extern "C" int fuelmi_frontier_get_flags(fuelmi_frontier* f, char* flags) {
  ARGCHK(f && flags);
  FRONTIER_HAS_MAP(f);
  fuelmi_map* m = f->map;
  HIPCHK(hipSetDevice(m->device));
  long n = m->g.N;
  int rc = frontier_ensure_stage(f, (size_t)n);
  if (rc) return rc;
  {
    const int rcr = frontier_apply_reset(f);
    if (rcr) return rcr;
  }
  k_expand_flag_bits<<<fblocks(n, 256), 256, 0, f->stream>>>(f->flag.p, n, (char*)f->d_stage);
  FDBG("k_expand_flag_bits");
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(flags, f->d_stage, (size_t)n, hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  return FUELMI_OK;
}
