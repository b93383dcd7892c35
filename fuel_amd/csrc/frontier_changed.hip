// frontier_changed.hip -- the changed-cluster test of FrontierFinder::searchFrontiers (frontier_finder.cpp:62-93;
// haveOverlap / isFrontierChanged :353-372) and the device pool of the committed clusters' cells it reads.
//
// remove_changed_begin queues the test of every committed cluster whose box overlaps the updated box on the finder's
// stream, ahead of the search's chain: a cluster with a cell that is no longer a frontier cell loses its flags on the
// device, and the verdicts reach pinned host memory with the search result.  remove_changed_end applies them to the
// lists once the search has been collected (frontier.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <list>
#include <vector>

#include "frontier_internal.h"

__device__ __forceinline__ bool f1_cell(const Geo& g, const u64* __restrict__ occ, const u64* __restrict__ unk,
                                        long a) {
  auto bit = [&](const u64* p, long q) { return (p[q >> 6] >> (q & 63)) & 1ull; };
  if (bit(occ, a) || bit(unk, a)) return false;
  int x = (int)(a / g.nyz);
  int r = (int)(a - (long)x * g.nyz);
  int y = r / g.nz, z = r - y * g.nz;
  if (x > 0 && bit(unk, a - g.nyz)) return true;
  if (x < g.nx - 1 && bit(unk, a + g.nyz)) return true;
  if (y > 0 && bit(unk, a - g.nz)) return true;
  if (y < g.ny - 1 && bit(unk, a + g.nz)) return true;
  if (z > 0 && bit(unk, a - 1)) return true;
  if (z < g.nz - 1 && bit(unk, a + 1)) return true;
  return false;
}

// committed clusters' cells live in one device pool; candidate k of a changed-cluster test owns the
// global indices [start[k], start[k+1]).  The (pool offset, start) table is read straight from the pinned host
// copy and staged in LDS (no H2D copy node in front of the search), verdicts go straight back to pinned memory.
struct RmCand {
  u64 off;    // pool offset of the cluster's cells
  u32 start;  // first flat index
  u32 pad;
};
#define RM_LDS 1024  // candidates staged per block
__device__ __forceinline__ int rm_cluster_of(const u32* s_start, int ncand, u32 i) {
  int lo = 0, hi = ncand - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (s_start[mid] <= i)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}
// MODE 0: "did a cell stop being a frontier cell?" -> d_mark[k] = mark, h_changed[k] = 1
// MODE 1: clear the flags of the clusters marked by MODE 0
template <int MODE>
__global__ void __launch_bounds__(256)
k_rm_pool(Geo g, const u64* __restrict__ occ, const u64* __restrict__ unk, u64* flag, const u32* __restrict__ pool,
          const RmCand* __restrict__ cand, int ncand, u32 total, int* d_mark, int mark, int* h_changed) {
  __shared__ u32 s_start[RM_LDS];
  __shared__ u64 s_off[RM_LDS];
  const bool staged = ncand <= RM_LDS;  // else `cand` is a device copy and the look-ups go to memory
  if (staged) {
    for (int k = threadIdx.x; k < ncand; k += 256) {
      const RmCand c = cand[k];
      s_start[k] = c.start;
      s_off[k] = c.off;
    }
    __syncthreads();
  }
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int k;
  u32 a;
  if (staged) {
    k = rm_cluster_of(s_start, ncand, i);
    a = pool[s_off[k] + (i - s_start[k])];
  } else {
    int lo = 0, hi = ncand - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (cand[mid].start <= i)
        lo = mid;
      else
        hi = mid - 1;
    }
    k = lo;
    a = pool[cand[k].off + (i - cand[k].start)];
  }
  if (MODE == 0) {
    if (!f1_cell(g, occ, unk, a) && d_mark[k] != mark) {
      d_mark[k] = mark;
      h_changed[k] = 1;
    }
  } else {
    if (d_mark[k] == mark) atomicAnd(&flag[a >> 6], ~(1ull << (a & 63)));
  }
}
// Both modes in ONE launch of many workgroups (round 6; a streaming frame's changed-cluster test walks a 20 k-cell
// surface: too long for one workgroup, and two dependent launches stood at the head of the frame's critical loop):
// the marks leave with agent-scope stores, every workgroup counts itself in behind s_waitcnt vmcnt(0) and spins until
// the count reaches `target` (the host keeps the running total: nobody resets the counter), then clears the flags of
// the marked clusters, reading the marks past its L2.  The grid is capped at RM_BAR_BLOCKS workgroups of 256 lanes --
// far below what the chip holds at once, so every workgroup is resident (or becomes so as other kernels drain) while
// the others spin: no deadlock.  No fence anywhere.
#define RM_BAR_BLOCKS 512
__global__ void __launch_bounds__(256)
k_rm_pool_bar(Geo g, const u64* __restrict__ occ, const u64* __restrict__ unk, u64* flag, const u32* __restrict__ pool,
              const RmCand* __restrict__ cand, int ncand, u32 total, int* d_mark, int mark, int* h_changed, u32* bar, u32 target) {
  __shared__ u32 s_start[RM_LDS];
  __shared__ u64 s_off[RM_LDS];
  for (int k = threadIdx.x; k < ncand; k += 256) {  // (ncand <= RM_LDS: checked by the host)
    const RmCand c = cand[k];
    s_start[k] = c.start;
    s_off[k] = c.off;
  }
  __syncthreads();
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  int k = 0;
  u32 a = 0u;
  bool chg = false;
  if (i < total) {
    k = rm_cluster_of(s_start, ncand, i);
    a = pool[s_off[k] + (i - s_start[k])];
    chg = !f1_cell(g, occ, unk, a);
  }
  {  // one mark per wave and cluster (a wave's cells nearly always belong to one cluster: the verdict crosses PCIe)
    const unsigned long long bm = __ballot(chg);
    if (bm) {
      const int leader = __builtin_ctzll(bm);
      const int kl = __shfl(k, leader, 64);
      if (chg && ((int)(threadIdx.x & 63) == leader || k != kl)) {
        st_agent(reinterpret_cast<u32*>(d_mark) + k, (u32)mark);
        h_changed[k] = 1;
      }
    }
  }
  wait_vm_stores();
  __syncthreads();
  // arrival: ONE returning atomic per workgroup; the last arriver releases everybody through per-workgroup words 64 bytes
  // apart (pollers of one word serialise at the memory-side atomic unit and starve the arrivals: measured, 9 % of a frame)
  __shared__ u32 s_lastw;
  if (threadIdx.x == 0) s_lastw = atomicAdd(bar, 1u) + 1u == target ? 1u : 0u;
  __syncthreads();
  if (s_lastw) {
    for (u32 w = threadIdx.x; w < gridDim.x; w += 256) st_agent(bar + 16u * (w + 1u), (u32)mark);
  } else if (threadIdx.x == 0) {
    const u32* mine = bar + 16u * (blockIdx.x + 1u);
    const unsigned long long t0 = wall_clock64();
    for (u32 spins = 0; ld_agent(mine) != (u32)mark; ++spins) {
      if ((spins & 63u) == 63u && wall_clock64() - t0 > 5000000ull) {  // 50 ms: unreachable with a resident grid -- never
        h_changed[ncand] = -1;                                          // hang the device, and never finish silently:
        break;                                                          // _search_end reports the search as failed
      }
      __builtin_amdgcn_s_sleep(2);
    }
  }
  __syncthreads();
  if (i < total && ld_agent(reinterpret_cast<const u32*>(d_mark) + k) == (u32)mark) atomicAnd(&flag[a >> 6], ~(1ull << (a & 63)));
}
// both modes in ONE workgroup for the searches of an exploration (a few thousand pooled cells in the clusters the updated
// box touches: one launch instead of two dependent ones -- the first kernels of a streaming frame's critical path).
// The marks live in LDS; h_changed[k] is written as by MODE 0.
#define RM_ONE_T 1024
#define RM_ONE_CELLS (2 * RM_ONE_T)  // (round 6: was 16 per lane -- a streaming frame's 10-16 k-cell candidates kept ONE workgroup busy for 13-77 us,
                                     // profiles/r06_rm_pool_variants.txt; beyond two cells per lane k_rm_pool_bar takes the test)
__global__ void __launch_bounds__(RM_ONE_T)
k_rm_pool_one(Geo g, const u64* __restrict__ occ, const u64* __restrict__ unk, u64* flag, const u32* __restrict__ pool,
              const RmCand* __restrict__ cand, int ncand, u32 total, int* h_changed) {
  __shared__ u32 s_start[RM_LDS];
  __shared__ u64 s_off[RM_LDS];
  __shared__ u32 s_mark[RM_LDS];
  for (int k = threadIdx.x; k < ncand; k += RM_ONE_T) {
    const RmCand c = cand[k];
    s_start[k] = c.start;
    s_off[k] = c.off;
    s_mark[k] = 0u;
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i < total; i += RM_ONE_T) {
    const int k = rm_cluster_of(s_start, ncand, i);
    const u32 a = pool[s_off[k] + (i - s_start[k])];
    if (!f1_cell(g, occ, unk, a) && s_mark[k] == 0u) {
      s_mark[k] = 1u;
      h_changed[k] = 1;
    }
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i < total; i += RM_ONE_T) {
    const int k = rm_cluster_of(s_start, ncand, i);
    if (s_mark[k]) {
      const u32 a = pool[s_off[k] + (i - s_start[k])];
      atomicAnd(&flag[a >> 6], ~(1ull << (a & 63)));
    }
  }
}
__global__ void k_pool_put(u32* __restrict__ pool, const u32* __restrict__ cells, const PoolPut* __restrict__ table) {
  const PoolPut e = table[blockIdx.x];  // one workgroup per cluster (the table sits in pinned host memory)
  u32* dst = pool + e.dst;
  const u32* src = cells + e.src;
  for (u32 i = threadIdx.x; i < e.n; i += blockDim.x) dst[i] = src[i];
  if (e.seed >= 0 && threadIdx.x == 0) dst[e.n] = (u32)e.seed;  // order is irrelevant on the device
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static bool have_overlap(const double* min1, const double* max1, const double* min2, const double* max2) {
  // haveOverlap (:353-363)
  for (int i = 0; i < 3; ++i) {
    double bmin = std::max(min1[i], min2[i]);
    double bmax = std::min(max1[i], max2[i]);
    if (bmin > bmax + 1e-3) return false;
  }
  return true;
}

// ---- device pool of committed clusters' cells ---------------------------------------------------
static int pool_upload(fuelmi_frontier* f, HCluster& c) {  // from the host list (rebuilds)
  c.pool_off = f->pool_used;
  if (!c.cells.empty())
    HIPCHK(hipMemcpyAsync(f->pool + f->pool_used, c.cells.data(), c.cells.size() * sizeof(int), hipMemcpyHostToDevice,
                          f->stream));
  f->pool_used += c.cells.size();
  return FUELMI_OK;
}
static int pool_reserve(fuelmi_frontier* f, size_t need) {
  if (f->pool_used + need <= f->pool_cap) return FUELMI_OK;
  // compact (erased clusters leave holes) and grow: re-upload the live clusters from their host lists
  size_t live = need;
  {
    const int rcm = frontier_materialize_lists(f);
    if (rcm) return rcm;
  }
  for (std::list<HCluster>* L : {&f->frontiers, &f->dormant})
    for (HCluster& c : *L) {
      const int rcf = frontier_fetch_cluster(f, &c);  // (the pool is about to be rebuilt from the host lists)
      if (rcf) return rcf;
      live += c.cells.size();
    }
  HIPCHK(hipStreamSynchronize(f->stream));
  if (f->pool) ++f->n_pool_rebuilds;  // (the first allocation is not a rebuild)
  if (live > f->pool_cap / 2 || !f->pool) {
    size_t cap = std::max<size_t>(1u << 20, f->pool_cap);
    while (cap / 2 < live) cap *= 2;
    if (f->pool) HIPCHK(hipFree(f->pool));
    f->pool = nullptr;
    f->pool_cap = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&f->pool), cap * sizeof(u32)));
    f->pool_cap = cap;
  }
  f->pool_used = 0;
  for (std::list<HCluster>* L : {&f->frontiers, &f->dormant})
    for (HCluster& c : *L) {
      int rc = pool_upload(f, c);
      if (rc) return rc;
    }
  HIPCHK(hipStreamSynchronize(f->stream));  // the host lists may be freed by the caller afterwards
  return FUELMI_OK;
}
// commit this search's clusters to the pool: the ones whose cells still sit grouped on the device are
// copied there by ONE launch (a table of {destination, source, count, seed} per cluster)
int frontier_keep_clusters(fuelmi_frontier* f, std::list<HCluster>& clusters) {
  // The kept clusters stay "lazy" -- their cell lists still sit in the pinned result buffer, which the tail of
  // the search may not even have filled yet: the pool copy below is ordered behind that tail on the stream, and
  // the host lists are materialised by frontier_materialize_lists before the buffer is reused (next search) or
  // when somebody asks for them.  Waiting for the tail here cost ~25 us per streaming cycle.
  size_t need = 0, nlazy = 0;
  for (HCluster& c : clusters) need += c.size(), nlazy += c.lazy ? 1 : 0;
  f->pool_dirty = true;
  int rc = pool_reserve(f, need);
  if (rc) return rc;
  std::vector<PoolPut> table;
  table.reserve(nlazy);
  for (HCluster& c : clusters) {
    if (!c.lazy) {
      if ((rc = pool_upload(f, c))) return rc;
      continue;
    }
    // one workgroup per table entry: a large cluster (the growing surface of a streaming run reaches 20 k cells) is
    // cut into pieces of 2048 cells -- one workgroup walking it alone was 13 us of every frame's frontier stream
    const u32 src0 = (u32)(c.lazy - reinterpret_cast<const int*>(f->F.h_cells)), ncell = (u32)c.lazy_n;
    for (u32 at = 0; at < ncell || at == 0; at += 2048u) {
      PoolPut e;
      e.dst = f->pool_used + at;
      e.src = src0 + at;
      e.n = std::min(2048u, ncell - at);
      e.seed = at + 2048u >= ncell ? c.lazy_seed : -1;  // (the seed goes behind the last piece)
      e.pad = 0;
      table.push_back(e);
      if (ncell == 0) break;
    }
    c.pool_off = f->pool_used;
    f->pool_used += c.size();
    f->lazy_kept = true;
  }
  if (table.empty()) return FUELMI_OK;
  if (table.size() > f->h_put_cap) {
    if (f->h_put) HIPCHK(hipHostFree(f->h_put));
    f->h_put = nullptr;
    f->h_put_cap = 0;
    const size_t cap = table.size() + table.size() / 2 + 64;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&f->h_put), cap * sizeof(PoolPut), hipHostMallocDefault));
    f->h_put_cap = cap;
  }
  // (the table of the previous commit was consumed before the search in between was collected)
  memcpy(f->h_put, table.data(), table.size() * sizeof(PoolPut));
  k_pool_put<<<(unsigned)table.size(), 256, 0, f->stream>>>(f->pool, f->F.ms_val[f->last_fin],
                                                             reinterpret_cast<const PoolPut*>(f->h_put));
  HIPCHK(hipGetLastError());
  return FUELMI_OK;
}

// Drop the clusters that overlap the updated box and contain a cell that is no longer a frontier cell
// (searchFrontiers :62-93).  The test and the clearing of the flags run on the device ahead of the
// scan; the host learns the verdicts together with the search result (no round trip of its own) and
// updates frontiers_ / dormant_frontiers_ / removed_ids_ in _search_end.  The search region therefore
// includes the boxes of ALL candidates, not only of the ones that turn out to be dropped.
int remove_changed_begin(fuelmi_frontier* f, const double* umin, const double* umax) {
  fuelmi_map* m = f->map;
  f->pend_rm.clear();
  for (std::list<HCluster>* L : {&f->frontiers, &f->dormant}) {
    int pos = 0;
    for (auto it = L->begin(); it != L->end(); ++it, ++pos)
      if (have_overlap(it->bmin, it->bmax, umin, umax)) f->pend_rm.push_back({L, it, pos});
  }
  const size_t nc = f->pend_rm.size();
  if (nc == 0) return FUELMI_OK;
  std::vector<u64> off(nc);
  std::vector<u32> start(nc);
  u32 total = 0;
  for (size_t k = 0; k < nc; ++k) {
    const HCluster& c = *f->pend_rm[k].it;
    off[k] = c.pool_off;
    start[k] = total;
    total += (u32)c.size();
    for (int q = 0; q < 3; ++q) {  // if dropped, its cells lose their flags and may be re-grown from the scan box
      const int lo = (int)std::floor((c.bmin[q] - m->g.org[q]) * m->g.res_inv);
      const int hi = (int)std::floor((c.bmax[q] - m->g.org[q]) * m->g.res_inv);
      if (f->rm_lo[q] > f->rm_hi[q])
        f->rm_lo[q] = lo, f->rm_hi[q] = hi;
      else
        f->rm_lo[q] = std::min(f->rm_lo[q], lo), f->rm_hi[q] = std::max(f->rm_hi[q], hi);
    }
  }
  if (nc > f->h_changed_cap) {
    if (f->h_changed) HIPCHK(hipHostFree(f->h_changed));
    if (f->h_cand) HIPCHK(hipHostFree(f->h_cand));
    if (f->d_mark) HIPCHK(hipFree(f->d_mark));
    f->h_changed = nullptr;
    f->h_cand = nullptr;
    f->d_mark = nullptr;
    f->h_changed_cap = 0;
    const size_t cap = nc + nc / 2 + 64;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&f->h_changed), cap * sizeof(int), hipHostMallocDefault));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&f->h_cand), cap * sizeof(RmCand), hipHostMallocDefault));
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&f->d_mark), cap * sizeof(int)));
    HIPCHK(hipMemsetAsync(f->d_mark, 0, cap * sizeof(int), f->stream));
    // rm_mark is NOT restarted: the fresh d_mark is zero and marks are >= 1, while k_rm_pool_bar's release words in
    // rm_bar still hold the marks of earlier launches -- a repeated mark would let workgroups skip the barrier
    f->h_changed_cap = cap;
  }
  RmCand* hc = reinterpret_cast<RmCand*>(f->h_cand);
  for (size_t k = 0; k < nc; ++k) {
    hc[k].off = off[k], hc[k].start = start[k], hc[k].pad = 0u;
    f->h_changed[k] = 0;
  }
  f->h_changed[nc] = 0;  // (time-out word of k_rm_pool_bar's barrier: h_changed holds nc + nc / 2 + 64 entries)
  if (nc > RM_LDS) {  // too many candidates for the LDS table: the kernels search a device copy
    int rcs = frontier_ensure_stage(f, nc * sizeof(RmCand));
    if (rcs) return rcs;
    HIPCHK(hipMemcpyAsync(f->d_stage, hc, nc * sizeof(RmCand), hipMemcpyHostToDevice, f->stream));
    hc = reinterpret_cast<RmCand*>(f->d_stage);
  }
  f->rm_last_nc = (int)nc;
  f->rm_last_total = total;
  f->rm_last_mark = 0;
  if (nc <= RM_LDS && total <= RM_ONE_CELLS) {
    ++f->rm_paths[0];
    k_rm_pool_one<<<1, RM_ONE_T, 0, f->stream>>>(m->g, m->occ_bits.p, m->unk_bits.p, f->flag.p, f->pool, hc, (int)nc, total,
                                                 f->h_changed);
    FDBG("k_rm_pool_one");
    return FUELMI_OK;
  }
  const int mark = ++f->rm_mark;  // (marks of earlier searches never match -- rm_mark is never restarted: no clearing pass)
  f->rm_last_mark = mark;
  if (nc <= RM_LDS && fblocks((long)total, 256) <= RM_BAR_BLOCKS) {
    if (!f->rm_bar) {
      HIPCHK(hipMalloc(reinterpret_cast<void**>(&f->rm_bar), 64 * (RM_BAR_BLOCKS + 1)));
      HIPCHK(hipMemsetAsync(f->rm_bar, 0, 64 * (RM_BAR_BLOCKS + 1), f->stream));
      f->rm_bar_total = 0u;
    }
    const int nb = fblocks((long)total, 256);
    ++f->rm_paths[1];
    f->rm_bar_total += (u32)nb;
    k_rm_pool_bar<<<nb, 256, 0, f->stream>>>(m->g, m->occ_bits.p, m->unk_bits.p, f->flag.p, f->pool, hc, (int)nc, total, f->d_mark,
                                             mark, f->h_changed, f->rm_bar, f->rm_bar_total);
    FDBG("k_rm_pool_bar");
    return FUELMI_OK;
  }
  // (fblocks caps the grid at 65 536 workgroups: 16.7 M candidate cells, far beyond any map of this library)
  ++f->rm_paths[nc <= RM_LDS ? 2 : 3];
  k_rm_pool<0><<<fblocks((long)total, 256), 256, 0, f->stream>>>(m->g, m->occ_bits.p, m->unk_bits.p, f->flag.p, f->pool, hc,
                                                               (int)nc, total, f->d_mark, mark, f->h_changed);
  FDBG("k_rm_pool<0>");
  k_rm_pool<1><<<fblocks((long)total, 256), 256, 0, f->stream>>>(m->g, m->occ_bits.p, m->unk_bits.p, f->flag.p, f->pool, hc,
                                                               (int)nc, total, f->d_mark, mark, f->h_changed);
  FDBG("k_rm_pool<1>");
  return FUELMI_OK;
}
// after the stream has drained: apply the verdicts.  removed_ids_ semantics (:74-85): index in
// frontiers_ as the list shrinks; dormant clusters are dropped silently.
void remove_changed_end(fuelmi_frontier* f) {
  int erased_active = 0;
  if (!f->pend_rm.empty() && f->h_changed[f->pend_rm.size()] == -1) f->rm_failed = true;  // (k_rm_pool_bar's time-out)
  for (size_t k = 0; k < f->pend_rm.size(); ++k) {
    if (!f->h_changed[k]) continue;
    const fuelmi_frontier::PendingRm& p = f->pend_rm[k];
    if (p.list == &f->frontiers) {
      f->removed_ids.push_back(p.pos - erased_active);
      ++erased_active;
    }
    p.list->erase(p.it);
  }
  f->pend_rm.clear();
}
