// frontier.hip -- frontier detection + clustering (FrontierFinder::searchFrontiers /
// expandFrontier, active_perception/src/frontier_finder.cpp:54-164; predicates :862-877;
// computeFrontierInfo :374-390).
//
// The reference scans the search box in x,y,z order and region-grows (26-neighbourhood BFS) from
// every unflagged frontier cell.  The result of that SEQUENTIAL process is reproduced exactly by
// an order-independent formulation:
//   F1(c)   = FREE(c) and one of the 6 face neighbours is UNKNOWN            (:862-877)
//   Q0      = F1 & flag==0 & isInBox(idx) & centre.z >= min_z   cells the BFS may ADD (:146-151)
//   seeds   = F1 & flag==0 & inside the scanned index box       cells the scan may START from
//   NQ seed = seed & !Q0 (below min_z / on the box_max face): starts a cluster, is never added.
// BFS growth only walks Q0 cells, so clusters are unions of 26-connected components of Q0.
// A component C is claimed by the first (lowest address = scan order) of: its own cells inside
// the scan box, or the NQ seeds adjacent to it.  cluster(C) = that claimer; every NQ seed also
// forms a cluster with the components it claims.  Flags are set for every claimed cell and every
// NQ seed, kept or not (the reference's sticky flags of rejected small clusters, :136,154-163).
//
// Two device chains compute that: the tile chain (frontier_tile.hip), which labels spatial tiles in LDS and resolves
// the search on one record per tile-local component, and the legacy chain (frontier_legacy.hip), which works on the
// cells themselves and is the fallback when a capacity of the tile chain is exceeded.  The changed-cluster test and
// the device pool of committed cells are in frontier_changed.hip, the read-back C-ABI in frontier_query.hip.
// This file holds the finder's lifecycle (create / destroy / reset / commit), _search_begin (search region, tile menu,
// launch of a chain) and _search_end (collection of the result, re-tiled runs and fallback, assembly of the
// clusters), and the FUELMI_FR_TIMING / FUELMI_HOST_TIMING reports.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <vector>

#include "fuelmi_internal.h"
#include "frontier_internal.h"

__global__ void k_zero_words(u64* p, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0ull;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <typename T>
static int dmalloc(fuelmi_frontier* f, T** p, size_t n) {
  void* d = nullptr;
  HIPCHK(hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T)));
  f->allocs.push_back(d);
  *p = (T*)d;
  const char* fp = reinterpret_cast<const char*>(p), *f0 = reinterpret_cast<const char*>(&f->F);
  if (fp >= f0 && fp < f0 + sizeof(FArgs))  // a per-search buffer of F: the other plane's set gets a twin (frontier_twin_set)
    f->f_scratch.push_back({(size_t)(fp - f0), std::max<size_t>(n, 1) * sizeof(T)});
  return FUELMI_OK;
}
// priority of the finder's streams: the highest (a chain of short latency-bound kernels beside the wide ESDF passes;
// normal / lowest measured in rounds 3, 4 and 6: within the run-to-run spread or worse, profiles/r06_frontier_prio_threads_sweep2.txt)
static int frontier_stream_priority() {
  int lo_p = 0, hi_p = 0;
  if (hipDeviceGetStreamPriorityRange(&lo_p, &hi_p) != hipSuccess) return 0;
  return hi_p;
}
// the second set of per-search buffers (see fuelmi_frontier::F2): a twin of every device buffer F points to, its own
// per-search variables and its own pinned result block
static int frontier_twin_set(fuelmi_frontier* f) {
  FArgs& F = f->F;
  f->F2 = F;
  char* f2 = reinterpret_cast<char*>(&f->F2);
  const std::vector<fuelmi_frontier::ScratchRec> recs = f->f_scratch;  // (dmalloc below appends)
  for (const auto& r : recs) {
    void* d = nullptr;
    HIPCHK(hipMalloc(&d, r.bytes));
    f->allocs.push_back(d);
    memcpy(f2 + r.field_off, &d, sizeof(void*));
  }
  f->f_scratch = recs;
  FArgs& G2 = f->F2;
  G2.kept = G2.counts + 16;
  HIPCHK(hipMemsetAsync(G2.counts, 0, 16 * sizeof(u32), f->stream));
  HIPCHK(hipMemsetAsync(G2.fctr, 0, FR_NCTR * sizeof(u32), f->stream));
  FVar* d_var2 = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&d_var2), sizeof(FVar)));
  f->allocs.push_back(d_var2);
  G2.var = d_var2, G2.var_w = d_var2;
  HIPCHK(hipHostMalloc(&f->h_pin2, f->pin_bytes, hipHostMallocDefault));
  G2.h_counts = reinterpret_cast<u32*>(f->h_pin2);
  G2.h_rec = reinterpret_cast<KeptRec*>(G2.h_counts + 16);
  G2.h_part = reinterpret_cast<u32*>(G2.h_rec + G2.cap_kept);
  G2.h_cells = G2.h_part + ((size_t)G2.cap_q / SZ_CH + 2) * 10;
  memset(f->h_pin2, 0, 64);
  G2.flag = f->flag2.p;
  HIPCHK(fuelmi_stream_create(&f->stream2, frontier_stream_priority(), "FR"));
  HIPCHK(hipStreamSynchronize(f->stream));
  return FUELMI_OK;
}

int frontier_ensure_stage(fuelmi_frontier* f, size_t bytes) {
  if (bytes > f->d_stage_bytes) {
    if (f->d_stage) HIPCHK(hipFree(f->d_stage));
    f->d_stage = nullptr;
    f->d_stage_bytes = 0;
    size_t want = bytes + bytes / 4 + 4096;
    HIPCHK(hipMalloc(&f->d_stage, want));
    f->d_stage_bytes = want;
  }
  return FUELMI_OK;
}

// both streams of the finder (the current search's and the one the previous fresh search left its tail on)
hipError_t frontier_drain(const fuelmi_frontier* f) {
  const hipError_t e = stream_wait(f->stream);
  if (e != hipSuccess || !f->stream2) return e;
  return stream_wait(f->stream2);
}
static void frontier_orphan(void* p) {  // the map is going away under a live finder
  fuelmi_frontier* f = static_cast<fuelmi_frontier*>(p);
  if (f->stream) (void)hipStreamSynchronize(f->stream);
  if (f->stream2) (void)hipStreamSynchronize(f->stream2);
  f->scope.reset();
  f->map = nullptr;
}
extern "C" void fuelmi_frontier_destroy(fuelmi_frontier* f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  if (f->map) {
    (void)hipStreamSynchronize(f->map->stream);
    std::lock_guard<std::mutex> lk(f->map->dep_mu);
    auto& deps = f->map->dependents;
    for (size_t k = 0; k < deps.size(); ++k)
      if (deps[k].obj == f) {
        deps.erase(deps.begin() + (long)k);
        break;
      }
  }
  for (hipStream_t st : {f->stream, f->stream2})
    if (st) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
    }
  if (f->h_pin2) (void)hipHostFree(f->h_pin2);
  if (f->ev_dep) (void)hipEventDestroy(f->ev_dep);
  if (f->d_stage) (void)hipFree(f->d_stage);
  for (void* p : f->allocs) (void)hipFree(p);
  if (f->h_pin) (void)hipHostFree(f->h_pin);
  if (f->h_var) (void)hipHostFree(f->h_var);
  if (f->pool) (void)hipFree(f->pool);
  if (f->h_changed) (void)hipHostFree(f->h_changed);
  if (f->h_cand) (void)hipHostFree(f->h_cand);
  if (f->h_put) (void)hipHostFree(f->h_put);
  if (f->d_mark) (void)hipFree(f->d_mark);
  if (f->rm_bar) (void)hipFree(f->rm_bar);
  frontier_split_free(f);
  frontier_order_free(f);
  for (auto& row : f->graph_exec)
    for (hipGraphExec_t e : row)
      if (e) (void)hipGraphExecDestroy(e);
  if (f->ev_tail) (void)hipEventDestroy(f->ev_tail);
  if (f->ev_prev) (void)hipEventDestroy(f->ev_prev);
  if (f->ev_planes_read) {
    if (f->map) map_drop_plane_reader(f->map, f->ev_planes_read), map_drop_late_reader(f->map, f->ev_planes_read);
    (void)hipEventDestroy(f->ev_planes_read);
  }
  Plane* pl[] = {&f->flag, &f->flag2, &f->qb, &f->sb};
  for (Plane* p : pl)
    if (p->base) (void)hipFree(p->base);
  delete f;
}

extern "C" int fuelmi_frontier_create(fuelmi_map* m, const fuelmi_frontier_cfg* cfg, fuelmi_frontier** out) {
  ARGCHK(m && cfg && out);
  ARGCHK(cfg->reference_order >= 0 && cfg->reference_order <= 2);
  *out = nullptr;
  HIPCHK(hipSetDevice(m->device));
  fuelmi_frontier* f = new fuelmi_frontier;
  f->map = m;
  f->device = m->device;
  f->cfg = *cfg;
  const Geo& g = m->g;
  // first z index whose centre is NOT below min_z (reference: if (pos[2] < 0.4) continue;)
  f->iz_min = g.nz;
  for (int iz = 0; iz < g.nz; ++iz) {
    double pz = (iz + 0.5) * g.res + g.org[2];
    if (!(pz < cfg->min_z)) {
      f->iz_min = iz;
      break;
    }
  }
  int rc;
  if ((rc = plane_alloc(m, f->flag)) || (rc = plane_alloc(m, f->flag2)) || (rc = plane_alloc(m, f->qb)) ||
      (rc = plane_alloc(m, f->sb))) {
    fuelmi_frontier_destroy(f);
    return rc;
  }
  FArgs& F = f->F;
  memset(&F, 0, sizeof(F));
  size_t nwords = ((size_t)g.W + 255) / 256 * 256 + 256;
  F.cap_q = (u32)std::max<size_t>(1u << 20, (size_t)g.N / 8);
  F.cap_s = (u32)std::max<size_t>(1u << 18, (size_t)g.N / 32);
  F.cap_kept = 1u << 16;
  F.cluster_min = cfg->cluster_min;
  if ((rc = dmalloc(f, &F.pref, nwords)) || (rc = dmalloc(f, &F.blocksum, nwords / 256 + 1)) ||
      (rc = dmalloc(f, &F.blockscan, nwords / 256 + 1)) ||
      (rc = dmalloc(f, &F.counts, 16 + (size_t)F.cap_kept * 3)) ||  // counts, then the kept list
      (rc = dmalloc(f, &F.cell_adr, F.cap_q)) || (rc = dmalloc(f, &F.parent, F.cap_q)) ||
      (rc = dmalloc(f, &F.claim, F.cap_q)) || (rc = dmalloc(f, &F.cell_slot, F.cap_q)) ||
      (rc = dmalloc(f, &F.seed_adr, F.cap_s)) || (rc = dmalloc(f, &F.csize, (size_t)F.cap_q + F.cap_s)) ||
      (rc = dmalloc(f, &F.slot2rank, (size_t)F.cap_q + F.cap_s)) || (rc = dmalloc(f, &F.krec, F.cap_kept)) ||
      (rc = dmalloc(f, &F.ms_key[0], F.cap_q)) || (rc = dmalloc(f, &F.ms_key[1], F.cap_q)) ||
      (rc = dmalloc(f, &F.ms_val[0], F.cap_q)) || (rc = dmalloc(f, &F.ms_val[1], F.cap_q)) ||
      (rc = dmalloc(f, &F.ms_hist, (size_t)256 * (F.cap_q / MS_CH + 2))) ||
      (rc = dmalloc(f, &F.info_part, ((size_t)F.cap_q / SZ_CH + 2) * 10))) {
    fuelmi_frontier_destroy(f);
    return rc;
  }
  F.kept = F.counts + 16;
  HIPCHK(hipMemsetAsync(F.counts, 0, 16 * sizeof(u32), m->stream));  // ([8]: epoch of the last search resolved; no search has epoch 0)
  F.keys_from_slots = 1;
  if ((rc = dmalloc(f, &F.trec, FR_RCAP + 256)) || (rc = dmalloc(f, &F.tclaim, FR_RCAP + 256)) || (rc = dmalloc(f, &F.rcode, FR_RCAP + 256)) ||
      (rc = dmalloc(f, &F.rrow, (size_t)FR_RCAP * FR_TXS)) || (rc = dmalloc(f, &F.pairs, (size_t)FR_PCAP)) ||
      (rc = dmalloc(f, &F.fctr, FR_NCTR))) {
    fuelmi_frontier_destroy(f);
    return rc;
  }
  HIPCHK(hipMemsetAsync(F.fctr, 0, FR_NCTR * sizeof(u32), m->stream));
  F.dbg = nullptr;
  if (getenv("FUELMI_FR_TIMING")) {  // dev aid: phase time stamps of the fast chain (one row per tile + one for k_resolve)
    const size_t nrow = (size_t)(3 * ((g.nx + 4) / 4) * ((g.ny + 8) / 8) + 64);
    if ((rc = dmalloc(f, &F.dbg, nrow * FR_DBG_SLOTS))) {
      fuelmi_frontier_destroy(f);
      return rc;
    }
    HIPCHK(hipMemsetAsync(F.dbg, 0, nrow * FR_DBG_SLOTS * sizeof(unsigned long long), m->stream));
  }
  F.occ = m->occ_bits.p;
  F.unk = m->unk_bits.p;
  F.flag = f->flag.p;
  F.qb = f->qb.p;
  F.sb = f->sb.p;
  HIPCHK(hipStreamSynchronize(m->stream));
  {
    // the scan is a chain of short latency-bound kernels and is the critical path of a plan cycle:
    // give its stream the highest priority so the wide ESDF kernels of the map stream fill in around it
    HIPCHK(fuelmi_stream_create(&f->stream, frontier_stream_priority(), "FR"));
  }
  HIPCHK(hipEventCreateWithFlags(&f->ev_dep, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&f->ev_tail, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&f->ev_prev, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&f->ev_planes_read, hipEventDisableTiming));

  // ---- everything below is constant for the life of the object (the kernel chain is replayed
  // as a graph with these arguments baked in) ----
  // Q box: isInBox(idx) (min <= id < max) and z >= iz_min, inside the map
  const int nv[3] = {g.nx, g.ny, g.nz};
  for (int k = 0; k < 3; ++k) {
    F.qbox.lo[k] = std::max(m->info.box_min[k], 0);
    F.qbox.hi[k] = std::min(m->info.box_max[k] - 1, nv[k] - 1);
  }
  F.qbox.lo[2] = std::max(F.qbox.lo[2], f->iz_min);
  for (int k = 0; k < 3; ++k)
    if (F.qbox.lo[k] > F.qbox.hi[k]) {  // degenerate exploration box: nothing can be added
      F.qbox.lo[k] = 1;
      F.qbox.hi[k] = 0;
    }
  // per-search arguments: pinned host copy + device copy
  HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&f->h_var), sizeof(FVar), hipHostMallocDefault));
  memset(f->h_var, 0, sizeof(FVar));
  if ((rc = dmalloc(f, &f->d_var, 1))) {
    fuelmi_frontier_destroy(f);
    return rc;
  }
  F.var = f->d_var;
  F.var_w = f->d_var;
  // results land in one pinned host buffer [counts | cluster records | chunk records | cells]
  f->pin_bytes = 64 + (size_t)F.cap_kept * sizeof(KeptRec) + ((size_t)F.cap_q / SZ_CH + 2) * 40 + (size_t)F.cap_q * 4;
  HIPCHK(hipHostMalloc(&f->h_pin, f->pin_bytes, hipHostMallocDefault));
  F.h_counts = reinterpret_cast<u32*>(f->h_pin);
  F.h_rec = reinterpret_cast<KeptRec*>(F.h_counts + 16);
  F.h_part = reinterpret_cast<u32*>(F.h_rec + F.cap_kept);
  F.h_cells = F.h_part + ((size_t)F.cap_q / SZ_CH + 2) * 10;
  F.hcells_direct_max = FR_HCELLS_DIRECT;
  // CCL tile = TX x TY z-lines with u32 labels in LDS (<= 48 KiB so three workgroups share a CU)
  f->TY = 16;
  f->TX = std::max(1, std::min(8, (48 * 1024) / (f->TY * g.nz * 4)));
  const int qx = F.qbox.hi[0] - F.qbox.lo[0] + 1, qy = F.qbox.hi[1] - F.qbox.lo[1] + 1;
  f->ccl_tiles = 0;
  if (qx > 0 && qy > 0 && F.qbox.lo[2] <= F.qbox.hi[2]) {
    const int TX = f->TX, TY = f->TY;
    const int ntx = (qx + TX - 1) / TX, nty = (qy + TY - 1) / TY;
    f->ccl_tiles = ntx * nty;
    f->ccl_lds = ((size_t)TX * TY * g.nz + 2 * (size_t)TX * TY * ((g.nz + 31) / 32) + 2 * (size_t)TX) * sizeof(u32);
    if (f->ccl_lds > 160 * 1024) {
      fuelmi_set_error("frontier CCL tile of %d z-lines x %d voxels does not fit the LDS", TX * TY, g.nz);
      fuelmi_frontier_destroy(f);
      return FUELMI_ELIMIT;
    }
    if ((rc = frontier_legacy_attrs(f))) return rc;
    // fast path: sparse labels -- the tile is not bound by nz.  32 z-lines deep, 8 wide, 16 wide once that
    // still leaves >= 512 tiles (measured on 400^2 x 100 and 800^2 x 200 maps: fewer tile roots and face pairs
    // for k_tile_cross / k_resolve outweigh the longer tiles).
    // The tile of a search is picked from a menu by the size of its region; the launch grid of a menu entry is
    // that tile over the largest rectangle a search can cover (the Q box plus the box_max face of the scan box).
    const int mtx = 4, mty = 8;  // smallest tile of the menu
    f->fast_tiles = ((qx + 1 + mtx - 1) / mtx) * ((qy + 1 + mty - 1) / mty);
    F.pm_stride = (qx + 1 + mtx - 1) / mtx;
    if ((rc = dmalloc(f, &F.vlab, (size_t)g.N + 64)) || (rc = dmalloc(f, &F.tlab, (size_t)f->fast_tiles * FR_TCELL)) ||
        (rc = dmalloc(f, &F.t_base, (size_t)f->fast_tiles)) || (rc = dmalloc(f, &F.t_nroots, (size_t)f->fast_tiles)) ||
        (rc = dmalloc(f, &F.pm, (size_t)FR_KCAP * F.pm_stride))) {
      fuelmi_frontier_destroy(f);
      return rc;
    }
    const size_t seg_words = frontier_tile_lds(f, qx, qy);  // per-tile segment arrays of the menu
    if ((rc = dmalloc(f, &F.tq, seg_words + 64)) || (rc = dmalloc(f, &F.ts, seg_words + 64))) {
      fuelmi_frontier_destroy(f);
      return rc;
    }
  }
  if ((rc = frontier_tile_attrs(f))) return rc;
  // the fast path needs tiles, a cluster threshold that rules out one-seed clusters, and tile-local indices
  // that fit the 16-bit root numbers
  f->fast_ok = f->ccl_tiles > 0 && cfg->cluster_min >= 1 && frontier_tile_fits(f) && getenv("FUELMI_FRONTIER_LEGACY") == nullptr;
  if ((rc = frontier_twin_set(f))) {
    fuelmi_frontier_destroy(f);
    return rc;
  }
  {
    std::lock_guard<std::mutex> lk(m->dep_mu);
    m->dependents.push_back({f, &frontier_orphan});
  }
  *out = f;
  return FUELMI_OK;
}

// copy the cell lists of kept-but-still-lazy clusters out of the pinned result buffer (see frontier_keep_clusters)
int frontier_materialize_lists(fuelmi_frontier* f) {
  // (the name is round 2's: the lists are no longer copied out here -- see HCluster::dev_only)
  if (!f->lazy_kept) return FUELMI_OK;
  for (std::list<HCluster>* L : {&f->frontiers, &f->dormant})
    for (HCluster& c : *L)
      if (c.lazy) {
        c.dev_n = (u32)c.size();
        c.lazy = nullptr;
        c.lazy_n = 0;
        c.dev_only = true;
      }
  f->lazy_kept = false;
  return FUELMI_OK;
}
// the host list of a cluster that lives in the device pool only: fetched when somebody asks for it
int frontier_fetch_cluster(const fuelmi_frontier* f, const HCluster* cc) {
  HCluster* c = const_cast<HCluster*>(cc);
  if (!c->dev_only) return FUELMI_OK;
  HIPCHK(hipStreamSynchronize(f->stream));  // (the copy into the pool is queued on the finder's stream)
  std::vector<int> v(c->dev_n);
  if (c->dev_n) HIPCHK(hipMemcpy(v.data(), f->pool + c->pool_off, (size_t)c->dev_n * sizeof(int), hipMemcpyDeviceToHost));
  if (c->lazy_seed >= 0 && !v.empty()) {  // the NQ seed travels behind the sorted cells: back into address order
    const int seed = v.back();
    v.pop_back();
    v.insert(std::lower_bound(v.begin(), v.end(), seed), seed);
  }
  c->cells.swap(v);
  c->lazy_seed = -1;
  c->dev_only = false;
  return FUELMI_OK;
}

HostTiming g_ht;  // FUELMI_HOST_TIMING (frontier_internal.h)

// fuelmi_frontier_reset, executed: frontier_flag_ becomes all-zero by SWAPPING to the spare plane (zeroed on a side
// stream since it was retired) -- no kernel of the search clears flags on the way, no clearing pass in front of it.
// The plane just retired is zeroed behind everything queued on the finder's stream so far (the tail of the last
// search still sets flags in it).  The kernel chains are captured once per plane (F.flag is a kernel argument).
// second half of frontier_apply_reset: queue the zeroing of the retired plane on the side stream.  Off the critical
// path: _search_begin calls it AFTER it has launched the new chain (three API calls the chain's start does not wait for)
static int frontier_finish_reset(fuelmi_frontier* f) {
  if (!f->zero_deferred) return FUELMI_OK;
  f->zero_deferred = false;
  const int W = f->map->g.W;
  // The plane just retired belongs to the stream just retired (they swap together), so the zeroing goes onto that
  // stream itself -- in order behind the tail that still sets flags in the plane and in front of the search after
  // next that uses it again.  One launch instead of wait + launch + record on a side stream (10.7 -> ~4 us of host
  // time per search, profiles/r05_host_timing.txt), and one stream fewer per finder (hardware queues).
  k_zero_words<<<fblocks(W, 256, 1024), 256, 0, f->stream2>>>(f->flag2.p, W);
  HIPCHK(hipGetLastError());
  return FUELMI_OK;
}
int frontier_apply_reset(fuelmi_frontier* f, bool defer_zeroing) {
  if (!f->fresh_pending) return FUELMI_OK;
  f->fresh_pending = false;
  // (everything that still writes the retired plane / the shared cell pool is in front of this; with two buffer sets only
  // a commit since the last swap makes anybody wait for it)
  if (f->pool_dirty) HIPCHK(hipEventRecord(f->ev_tail, f->stream));
  {
    // the other plane's buffer set and stream: the retiring search's tail keeps running on its own stream.  (The cell
    // pool is the one device buffer both sets share: if it was written since the last swap -- a commit -- the new
    // stream waits for the old one.)
    std::swap(f->stream, f->stream2);
    std::swap(f->F, f->F2);
    if (f->pool_dirty) HIPCHK(hipStreamWaitEvent(f->stream, f->ev_tail, 0));
    f->pool_dirty = false;
  }
  std::swap(f->flag, f->flag2);
  f->flag_cur ^= 1;
  f->F.flag = f->flag.p;
  f->zero_deferred = true;
  return defer_zeroing ? FUELMI_OK : frontier_finish_reset(f);
}

// searchFrontiers, first half: drops changed clusters and enqueues the whole device pipeline on the
// frontier's own stream (asynchronous).  The caller may queue other work of the cycle (inflation,
// ESDF, B-spline evaluation on the map's stream) before collecting the result with _search_end.
extern "C" int fuelmi_frontier_search_begin(fuelmi_frontier* f) {
  ARGCHK(f);
  FRONTIER_HAS_MAP(f);
  FRONTIER_NOT_SEARCHING(f, "fuelmi_frontier_search_begin");
  fuelmi_map* m = f->map;
  HIPCHK(hipSetDevice(m->device));
  const Geo& g = m->g;
  FArgs& F = f->F;
  f->tmp.clear();
  g_ht.start();
  {
    const int rcm = frontier_materialize_lists(f);  // (the result buffer is about to be reused)
    if (rcm) return rcm;
  }
  {
    const int rcr = frontier_apply_reset(f, true);
    if (rcr) return rcr;
  }
  struct FinishReset {  // (on every exit path, behind whatever was launched)
    fuelmi_frontier* f;
    ~FinishReset() {
      (void)frontier_finish_reset(f);
      g_ht.lap(9);
    }
  } finish_reset{f};
  g_ht.lap(0);
  double umin[3], umax[3];
  fuelmi_map_get_updated_box(m, umin, umax, 1);

  // the scan reads only the occupancy state planes: it runs on its own stream, ordered after the
  // last kernel that rewrote them (fusion / upload), and overlaps the inflation / ESDF / B-spline
  // kernels the caller has queued on the map's stream for the same cycle
  // (once per record and search stream: a plan cycle on an unchanged map queues no wait packet in front of its chain)
  if (f->planes_waited[f->flag_cur] != m->planes_ver + 1) {
    HIPCHK(hipStreamWaitEvent(f->stream, m->ev_planes, 0));
    f->planes_waited[f->flag_cur] = m->planes_ver + 1;
  }
  f->scope.reset(new StageScope(m, FUELMI_K_FRONTIER, f->stream));
  f->removed_ids.clear();
  for (int q = 0; q < 3; ++q) f->rm_lo[q] = 1, f->rm_hi[q] = 0;
  g_ht.lap(1);
  // on EVERY exit path below (the changed-cluster test reads the occupancy planes too, and an empty search or an
  // error returns before the chain): whatever was queued, the planes are free behind it
  struct PlanesRead {
    fuelmi_frontier* f;
    bool done = false;
    ~PlanesRead() {
      if (done || !f->map) return;
      if (!f->mark_planes_read)
        map_add_late_reader(f->map, f->stream, f->ev_planes_read, &f->mark_planes_read);
      else if (hipEventRecord(f->ev_planes_read, f->stream) == hipSuccess)
        map_add_plane_reader(f->map, f->ev_planes_read);
    }
  } planes_read{f};
  int rc = remove_changed_begin(f, umin, umax);
  if (rc) return rc;
  g_ht.lap(2);

  // scan box (:95-106): updated box +- (1,1,0.5) clipped to the exploration box, as indices
  const int nv[3] = {g.nx, g.ny, g.nz};
  FVar hv;
  memset(&hv, 0, sizeof(hv));
  bool empty = false;
  for (int k = 0; k < 3; ++k) {
    double infl = (k == 2) ? 0.5 : 1.0;
    double smin = std::max(umin[k] - infl, m->cfg.box_min[k]);
    double smax = std::min(umax[k] + infl, m->cfg.box_max[k]);
    int lo = (int)std::floor((smin - g.org[k]) * g.res_inv);
    int hi = (int)std::floor((smax - g.org[k]) * g.res_inv);
    lo = std::max(lo, 0);
    hi = std::min(hi, nv[k] - 1);  // the reference would index out of the map here (UB)
    hv.sbox.lo[k] = lo;
    hv.sbox.hi[k] = hi;
    if (lo > hi) empty = true;
  }
  f->pending = true;
  f->fusion_at_begin = m->fusion_count;
  f->search_empty = empty;
  f->fast_launched = false;
  if (empty) return FUELMI_OK;

  // Region that can hold Q0 cells: the scan box, the boxes of the clusters just dropped (their flags were
  // cleared), or the whole exploration box when flags / occupancy changed behind the updated-box
  // bookkeeping (fresh finder, reset, uploadOccupancy, resetBuffer).  Everything a previous search
  // could reach is flagged, and every later change of the occupancy lies inside this search's updated
  // box, so nothing outside the region can be grown into.
  int rlo[3], rhi[3];
  const bool all = f->dirty_all || f->seen_epoch != m->occ_epoch;
  for (int k = 0; k < 3; ++k) {
    rlo[k] = hv.sbox.lo[k], rhi[k] = hv.sbox.hi[k];
    if (f->rm_lo[0] <= f->rm_hi[0]) rlo[k] = std::min(rlo[k], f->rm_lo[k]), rhi[k] = std::max(rhi[k], f->rm_hi[k]);
    if (all) rlo[k] = 0, rhi[k] = nv[k] - 1;
    hv.qreg.lo[k] = std::max(F.qbox.lo[k], rlo[k]);
    hv.qreg.hi[k] = std::min(F.qbox.hi[k], rhi[k]);
  }
  f->dirty_all = true;  // until this search has completed
  bool have_q = true;
  for (int k = 0; k < 3; ++k)
    if (hv.qreg.lo[k] > hv.qreg.hi[k]) have_q = false;
  if (!have_q)
    for (int k = 0; k < 3; ++k) hv.qreg.lo[k] = 1, hv.qreg.hi[k] = 0;
  hv.nty = hv.ntiles = 0;
  hv.nty_f = hv.ntiles_f = 0;
  hv.ftx = 4, hv.fty = 8;
  if (have_q) {
    const int qx = hv.qreg.hi[0] - hv.qreg.lo[0] + 1, qy = hv.qreg.hi[1] - hv.qreg.lo[1] + 1;
    hv.nty = (qy + f->TY - 1) / f->TY;
    hv.ntiles = ((qx + f->TX - 1) / f->TX) * hv.nty;  // <= f->ccl_tiles (tiles of the whole Q box)
  }
  {
    // tiles of the fast chain: over the x/y bounding rectangle of the Q region and the scan box (NQ seeds start
    // clusters from the box_max face, one voxel outside the Q box; seeds are flagged wherever they are).
    // Tile of this search: 32 z-lines deep and 16 or 8 wide while that leaves >= 512 tiles (measured on full
    // 400^2 x 100 / 800^2 x 200 boxes: fewer tile roots and face pairs outweigh the longer tiles); smaller
    // tiles for small regions (a streaming search covers ~100 x 100 lines: a handful of big tiles would run
    // one after the other on a handful of CUs)
    int p0[2], p1[2];
    for (int k = 0; k < 2; ++k) {
      p0[k] = hv.sbox.lo[k], p1[k] = hv.sbox.hi[k];
      if (have_q) p0[k] = std::min(p0[k], hv.qreg.lo[k]), p1[k] = std::max(p1[k], hv.qreg.hi[k]);
      // (never beyond what the launch grids and per-tile tables were sized for)
      p0[k] = std::max(p0[k], F.qbox.lo[k]);
      p1[k] = std::min(p1[k], F.qbox.hi[k] + 1);
    }
    const int qx = p1[0] - p0[0] + 1, qy = p1[1] - p0[1] + 1;
    int pick = 3;
    for (int k = 0; k < 4; ++k)
      if (menu_tiles(qx, qy, k) >= 512) {
        pick = k;
        break;
      }
    // (a finder whose tiles were too full lately starts on the smaller tile it ended on: the overflow costs a whole
    // chain run; forgotten after 64 searches)
    if (f->menu_min_ttl > 0) --f->menu_min_ttl, pick = std::max(pick, f->menu_min);
    f->fast_menu = pick;
    hv.px0 = p0[0], hv.py0 = p0[1], hv.px1 = p1[0], hv.py1 = p1[1];
    set_fast_tiles(hv, pick);
  }
  // words to process: the x-slabs of the region plus one slab either side (neighbour look-ups of the
  // claims / unions read the Q0 plane there: it must not hold bits of an earlier search)
  auto adr = [&](const int* id) { return (long)id[0] * g.nyz + (long)id[1] * g.nz + id[2]; };
  long a_lo = adr(hv.sbox.lo), a_hi = adr(hv.sbox.hi);
  if (have_q) {
    a_lo = std::min(a_lo, adr(hv.qreg.lo));
    a_hi = std::max(a_hi, adr(hv.qreg.hi));
  }
  a_lo = std::max(0L, a_lo - 2L * g.nyz);
  a_hi = std::min((long)g.N - 1, a_hi + 2L * g.nyz);
  hv.w0 = (int)((a_lo >> 6) & ~255L);
  const int w_hi = (int)(a_hi >> 6);
  hv.nblocks = (w_hi - hv.w0) / 256 + 1;
  hv.nwords = hv.nblocks * 256;
  const bool fast = f->fast_ok;
  hv.fresh = 0;  // (a reset has already swapped in an all-zero flag plane, frontier_apply_reset)
  if (F.dbg)  // FUELMI_FR_TIMING: stamps of this search only
    HIPCHK(hipMemsetAsync(F.dbg, 0, (size_t)(3 * (hv.ntiles_f + 1)) * FR_DBG_SLOTS * sizeof(unsigned long long), f->stream));
  hv.epoch = ++f->epoch;
  if (hv.epoch == 0u) hv.epoch = f->epoch = 1u;
  // pinned; read by the first kernel of the chain.  (The previous search's first kernel ran long ago -- its
  // result was collected -- and the tail that may still be running reads the device copy.)
  *f->h_var = hv;

  // the second radix pass is needed only beyond 256 kept clusters: guess from the previous search
  f->npass = f->last_nkept > 192 ? 2 : 1;

  // The fast chain's four kernels are launched DIRECTLY (rounds 2-3 replayed them as a hipGraph: cheaper for the host, but
  // the graph reaches the device ~10 us later, which is on the cycle's critical path since a fresh search runs beside the
  // previous one's tail -- same-box A/B in profiles/r04_tuning_ab_cycle.txt --, and only direct launches can mark the
  // point behind which the next depth frame may be fused).  The legacy chain is ~23 dependent launches whose arguments
  // never change (everything per-search sits behind F.var): it is replayed as a hipGraph.
  g_ht.lap(3);
  if (fast) {
    f->fast_launched = true;
    planes_read.done = true;
    return frontier_enqueue_fast(f);
  }
  return frontier_launch_legacy(f, f->npass);
}

// FUELMI_FR_TIMING: where the tile kernel and the resolve kernel spend their time (100 MHz ticks)
static void frontier_timing_report(fuelmi_frontier* f) {
  const FArgs& F = f->F;
  (void)hipStreamSynchronize(f->stream);
  const int nt = f->h_var->ntiles_f;
  std::vector<unsigned long long> d((size_t)(3 * (nt + 1)) * FR_DBG_SLOTS);
  (void)hipMemcpy(d.data(), F.dbg, d.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  unsigned long long t0 = ~0ull, t1 = 0;
  double phase[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int busiest = 0, nonempty = 0;
  for (int b = 0; b < nt; ++b) {
    const unsigned long long* r = &d[(size_t)b * FR_DBG_SLOTS];
    if (!r[0]) continue;
    t0 = std::min(t0, r[0]);
    for (int k = 1; k < 8; ++k)
      if (r[k]) t1 = std::max(t1, r[k]);
    if (r[8] > d[(size_t)busiest * FR_DBG_SLOTS + 8]) busiest = b;
    if (r[8]) ++nonempty;
  }
  {
    double st_av = 0, st_mx = 0, du_av = 0, du_mx = 0;
    int cnt = 0;
    for (int b = 0; b < nt; ++b) {
      const unsigned long long* r = &d[(size_t)b * FR_DBG_SLOTS];
      if (!r[0] || !r[6] || r[6] < r[0]) continue;
      const double st = (double)(r[0] - t0) / 100.0, du = (double)(r[6] - r[0]) / 100.0;
      st_av += st, st_mx = std::max(st_mx, st), du_av += du, du_mx = std::max(du_mx, du), ++cnt;
    }
    std::fprintf(stderr, "[fr-timing] ccl: %d tiles with cells: start avg %.1f max %.1f, duration avg %.1f max %.1f us\n", cnt,
                 st_av / std::max(cnt, 1), st_mx, du_av / std::max(cnt, 1), du_mx);
  }
  const unsigned long long* rb = &d[(size_t)busiest * FR_DBG_SLOTS];
  for (int k = 1; k < 8; ++k) phase[k] = rb[k] && rb[k - 1] ? (double)(rb[k] - rb[k - 1]) / 100.0 : 0.0;
  std::fprintf(stderr, "[fr-timing] tiles %d (non-empty %d) span %.1f us; busiest tile %d (%llu cells, start +%.1f us): "
               "bits %.1f labels %.1f unions %.1f roots %.1f records %.1f write %.1f us; %llu unions, %llu find steps, %llu links, %llu roots\n", nt, nonempty,
               (double)(t1 - t0) / 100.0, busiest, rb[8], (double)(rb[0] - t0) / 100.0, phase[1], phase[2], phase[3],
               phase[4], phase[5], phase[6], rb[9], rb[10], rb[11], rb[12]);
  for (int kern = 1; kern <= 2; ++kern) {  // k_tile_cross, k_tile_out: rows behind those of the tiles and of k_resolve
    const int np = kern == 1 ? 4 : 6;
    double mx[8] = {0}, av[8] = {0};
    unsigned long long c0 = ~0ull, c1 = 0;
    int cnt = 0;
    for (int b = 0; b < nt; ++b) {
      const unsigned long long* r = &d[(size_t)(kern * (nt + 1) + b) * FR_DBG_SLOTS];
      if (!r[0] || !r[np]) continue;
      c0 = std::min(c0, r[0]), c1 = std::max(c1, r[np]);
      for (int k = 1; k <= np; ++k) {
        const double ph = r[k] && r[k - 1] ? (double)(r[k] - r[k - 1]) / 100.0 : 0.0;
        mx[k] = std::max(mx[k], ph), av[k] += ph;
      }
      ++cnt;
    }
    double st_av = 0, st_mx = 0, du_av = 0, du_mx = 0;
    for (int b = 0; b < nt; ++b) {
      const unsigned long long* r = &d[(size_t)(kern * (nt + 1) + b) * FR_DBG_SLOTS];
      if (!r[0] || !r[np]) continue;
      const double st = (double)(r[0] - c0) / 100.0, du = (double)(r[np] - r[0]) / 100.0;
      st_av += st, st_mx = std::max(st_mx, st), du_av += du, du_mx = std::max(du_mx, du);
    }
    {
      unsigned long long e0 = ~0ull;
      double ea = 0, em = 0, la = 0, lm = 0;
      int n2 = 0;
      for (int b = 0; b < nt; ++b) {
        const unsigned long long v = d[(size_t)b * FR_DBG_SLOTS + 12 + kern];
        if (v) e0 = std::min(e0, v);
      }
      for (int b = 0; b < nt; ++b) {
        const unsigned long long v = d[(size_t)b * FR_DBG_SLOTS + 12 + kern];
        const unsigned long long* r = &d[(size_t)(kern * (nt + 1) + b) * FR_DBG_SLOTS];
        if (!v || !r[0] || r[0] < v) continue;
        const double e = (double)(v - e0) / 100.0, l = (double)(r[0] - v) / 100.0;
        ea += e, em = std::max(em, e), la += l, lm = std::max(lm, l), ++n2;
      }
      std::fprintf(stderr, "[fr-timing]   entry avg %.1f max %.1f us after the first workgroup; entry -> first stamp avg %.1f max %.1f us\n",
                   ea / std::max(n2, 1), em, la / std::max(n2, 1), lm);
    }
    std::fprintf(stderr, "[fr-timing] %s: span %.1f us over %d tiles; start avg %.1f max %.1f, duration avg %.1f max %.1f; phases avg/max:",
                 kern == 1 ? "cross (bits, build, list, append)" : "out (bits, cells, column, first, rows, flags)",
                 cnt ? (double)(c1 - c0) / 100.0 : 0.0, cnt, st_av / std::max(cnt, 1), st_mx, du_av / std::max(cnt, 1), du_mx);
    for (int k = 1; k <= np; ++k) std::fprintf(stderr, " %.1f/%.1f", av[k] / std::max(cnt, 1), mx[k]);
    std::fprintf(stderr, "\n");
  }
  const unsigned long long* rr = &d[(size_t)nt * FR_DBG_SLOTS];
  std::fprintf(stderr, "[fr-timing] resolve: init %.1f unions %.1f find %.1f reduce %.1f clusters %.1f seeds %.1f rank %.1f "
               "codes %.1f publish %.1f us; pairs %llu roots %llu cells %llu\n", (rr[1] - rr[0]) / 100.0,
               (rr[2] - rr[1]) / 100.0, (rr[3] - rr[2]) / 100.0, (rr[4] - rr[3]) / 100.0, (rr[5] - rr[4]) / 100.0, 0.0,
               (rr[6] - rr[5]) / 100.0, (rr[7] - rr[6]) / 100.0, (rr[8] - rr[7]) / 100.0, rr[9], rr[10], rr[11]);
}

// the fast chain publishes counts + cluster records from k_resolve and stamps them with the search's epoch; the two
// kernels behind it (flags, regrouping + copy-out of the cells) keep running -- whoever touches the cell lists waits for
// them (frontier_tail_sync).  Then: the late resolve, the re-tiled runs and the legacy fallback, as the result asks.
static int frontier_collect_fast(fuelmi_frontier* f) {
  fuelmi_map* m = f->map;
  FArgs& F = f->F;
  u32* counts = F.h_counts;
  volatile u32* stamp = counts + 15;
  const u32 want = f->h_var->epoch;
  // (poll, ~100 us of chain: a blocking wake-up costs a noticeable fraction of that; the time spent polling is the part
  // of _search_end that is the device's, not the host's)
  const auto w0 = std::chrono::steady_clock::now();
  const int rcw = stamp_wait<u32>(stamp, want, f->stream, "frontier search: the chain finished without publishing its result");
  f->wait_us_acc += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w0).count();
  if (rcw) return rcw;
  g_ht.lap(11);
  f->tail_pending = true;
  F.fast = 1;
  if (F.dbg) frontier_timing_report(f);
  if (counts[2] == 3u) {  // the search outgrew the launch that was to resolve it and no k_resolve was queued: do it now
    *stamp = 0u;
    const int rcl = frontier_enqueue_late_resolve(f);
    if (rcl) return rcl;
    const int rc = stamp_wait<u32>(stamp, want, f->stream, "frontier search: k_resolve finished without publishing its result");
    if (rc) return rc;
    ++f->n_late_resolve;
  }
  f->kr_skip_ok = counts[2] == 0u && counts[9] == 1u && 2u * counts[10] <= f->rcap_used;
  ++f->n_fast;
  if (counts[9] == 1u)
    ++f->n_in_launch;
  else if (f->fuse_tried && counts[2] == 0u)
    f->fuse_skip = 16;  // (too many tile roots for the launch's LDS: k_resolve did it)
  if (counts[2] == 2u && m->fusion_count != f->fusion_at_begin) {
    fuelmi_set_error("frontier search: the fast chain overflowed AFTER the map was fused again (a frame queued between "
                     "_search_begin and _search_end): the occupancy this search was about is gone -- call _search_end before the next fusion "
                     "on inputs this noisy");
    // the changed clusters' flags are already cleared on the device: take them off the lists too, and make the next
    // search look at the whole box again (the lists and the flag plane must not part ways on this path)
    remove_changed_end(f);
    f->dirty_all = true;
    return FUELMI_ELIMIT;
  }
  // A capacity of ONE TILE was exceeded (codes 11 cells, 12 components, 15 root pairs, 18 work-list entries -- a
  // full-height frontier wall along a y-line puts 32 x nz cells into one 8 x 32 tile): nothing was modified, and
  // the menu's next, smaller tile holds half as much per tile -- run the chain again on it before giving the search to
  // the legacy chain (round 6, with FR_TCELL = 2 048).
  while (counts[2] == 2u && f->fast_menu < 3 && (counts[6] == 11u || counts[6] == 12u || counts[6] == 15u || counts[6] == 18u)) {
    HIPCHK(frontier_tail_sync(f) == FUELMI_OK ? hipSuccess : hipErrorUnknown);
    ++f->fast_menu;
    FVar hv = *f->h_var;
    set_fast_tiles(hv, f->fast_menu);
    hv.epoch = ++f->epoch;
    if (hv.epoch == 0u) hv.epoch = f->epoch = 1u;
    *f->h_var = hv;
    f->kr_skip_ok = false;  // (k_resolve queued: no second round trip whatever the root count)
    if (getenv("FUELMI_FR_TIMING")) std::fprintf(stderr, "[fr-timing] capacity code %u: again with %d x %d tiles\n", counts[6], hv.ftx, hv.fty);
    const int rcr = frontier_enqueue_fast(f);
    if (rcr) return rcr;
    const int rcw = stamp_wait<u32>(stamp, hv.epoch, f->stream,
                                    "frontier search: the re-tiled chain finished without publishing its result");
    if (rcw) return rcw;
    f->tail_pending = true;
    ++f->n_retiled;
    f->menu_min = f->fast_menu, f->menu_min_ttl = 64;
  }
  if (counts[2] == 2u) {
    // a capacity of the fast path was exceeded (noise-like input): nothing was modified; run the legacy chain
    --f->n_fast;
    ++f->n_fallback;
    if (getenv("FUELMI_FR_TIMING")) std::fprintf(stderr, "[fr-timing] fallback to the legacy chain: capacity code %u\n", counts[6]);
    HIPCHK(frontier_tail_sync(f) == FUELMI_OK ? hipSuccess : hipErrorUnknown);
    F.fast = 0;
    f->npass = 1;
    int rcl = frontier_enqueue_chain(f, f->npass);
    if (rcl) return rcl;
    HIPCHK(hipStreamSynchronize(f->stream));
  }
  return FUELMI_OK;
}


// tmp_frontiers_ from the records of the search's nkept clusters (nq Q0 cells, n_out grouped cells)
static int frontier_assemble(fuelmi_frontier* f, u32 nq, u32 nkept, u32 n_out) {
  const Geo& g = f->map->g;
  FArgs& F = f->F;
  KeptRec* h_rec = F.h_rec;
  const u32* h_part = F.h_part;
  const u32* h_cells = F.h_cells;
  u32 ncl = nkept, ncells = n_out;
  std::vector<std::vector<float>> filtered;
  const bool split_mode = f->cfg.split != 0;
  // reference_order 1: always; 2 ("auto", the facade's default): whenever every cluster of the search holds at most
  // FR_REFORDER_AUTO cells (the level sweep then runs inside LDS) -- every incremental search of an exploration
  // run -- and the canonical order for the giant ones
  bool ref_order = f->cfg.reference_order == 1;
  if (f->cfg.reference_order == 2) {
    ref_order = true;
    for (u32 r = 0; r < nkept; ++r)
      if (h_rec[r].size > FR_REFORDER_AUTO) ref_order = false;
  }
  f->ref_now = ref_order;
  // never silent: which order this search delivers is part of its result -- fuelmi_frontier_order_stats
  f->order_last = ref_order ? 1 : 0;
  if (ref_order)
    ++f->n_order_ref;
  else if (f->cfg.reference_order == 2) {
    ++f->n_order_fallback;
    u32 big = 0;
    for (u32 r = 0; r < nkept; ++r) big = std::max(big, h_rec[r].size);
    f->order_fallback_cells = big;
  }
  int fin = nkept <= 256 ? 1 : 0;  // buffer pair holding the grouped cells of the search
  std::vector<u32> off2;
  u32 n_in = n_out;
  if (split_mode && !ref_order) HIPCHK(frontier_tail_sync(f) == FUELMI_OK ? hipSuccess : hipErrorUnknown);
  if (ref_order) {  // cells of every cluster in expandFrontier's order (an NQ seed first), into the other pair
    int rc = frontier_reference_order(f, nq, nkept, n_out, fin, &n_in, &off2, !split_mode);  // (queued behind the
    if (rc) return rc;                                                // search's tail; returns with the stream idle)
    f->tail_pending = false;
    fin = 1 - fin;
    ncells = n_in;
  }
  if (split_mode) {  // splitLargeFrontiers (:120) on the device; the pinned buffers then hold the pieces
    int rc = frontier_split_run(f, nq, nkept, n_in, fin, &ncl, &ncells, &filtered);
    if (rc) return rc;
    fin = ncl <= 256 ? 1 : 0;  // where the regrouping of the pieces ended
  }  // (reference order without the split: the ordered cells are in h_cells already)
  f->last_fin = fin;  // buffer holding the grouped cells the lazy clusters point into
  f->cells_fetch = F.fast && !ref_order && !split_mode && nq > F.hcells_direct_max;
  f->cells_fetch_n = ncells;
  // (the fast chain's records are complete; the legacy chain and the regrouping of the split pieces leave
  // per-chunk partial records to fold)
  const u32 nchunk = ((ref_order || F.fast) && !split_mode) ? 0u : (ncells + SZ_CH - 1) / SZ_CH;  // (records of the grouped
                                                                                       // array, not of the ordered one)
  for (u32 c = 0; c < nchunk; ++c) {  // fold the per-chunk records into the per-cluster totals
    const u32* rec = h_part + (size_t)c * 10;
    const u32 r = rec[0];
    if (r >= ncl) continue;
    for (int q = 0; q < 3; ++q) {
      h_rec[r].sum[q] += rec[1 + q];
      h_rec[r].box[q] = std::min(h_rec[r].box[q], rec[4 + q]);
      h_rec[r].box[3 + q] = std::max(h_rec[r].box[3 + q], rec[7 + q]);
    }
  }

  // host: bulk copies only (+ inserting an NQ seed where a seed started the cluster); records are
  // already in creation order (ascending claimer address = the reference's scan order)
  for (u32 r = 0; r < ncl; ++r) {
    const KeptRec& kr = h_rec[r];
    f->tmp.emplace_back();
    HCluster& c = f->tmp.back();
    const bool seed = !split_mode && kr.slot >= nq;
    const u32 cnt = kr.size - (seed ? 1u : 0u);
    c.lazy = reinterpret_cast<const int*>(h_cells) + kr.off;
    c.lazy_n = cnt;
    if (ref_order && !split_mode) {  // ordered list: the seed (if any) is already its first cell
      c.lazy = reinterpret_cast<const int*>(h_cells) + off2[r];
      c.lazy_n = kr.size;
    }
    unsigned long long sum[3] = {kr.sum[0], kr.sum[1], kr.sum[2]};
    u32 lo[3] = {kr.box[0], kr.box[1], kr.box[2]};
    u32 hi[3] = {kr.box[3], kr.box[4], kr.box[5]};
    if (split_mode) {
      // an NQ seed travels as the LAST cell of its piece (already in the sums): restore address order
      if (!ref_order && cnt > 1 && c.lazy[cnt - 1] < c.lazy[cnt - 2]) {
        c.lazy_seed = c.lazy[cnt - 1];
        c.lazy_n = cnt - 1;
      }
      c.filtered.swap(filtered[r]);
    }
    if (seed) {
      const int a = (int)kr.addr;
      if (!ref_order) c.lazy_seed = a;
      const u32 x = (u32)a / (u32)g.nyz, rr = (u32)a - x * (u32)g.nyz, y = rr / (u32)g.nz, z = rr - y * (u32)g.nz;
      const u32 id[3] = {x, y, z};
      for (int q = 0; q < 3; ++q) {
        sum[q] += id[q];
        lo[q] = cnt ? std::min(lo[q], id[q]) : id[q];
        hi[q] = cnt ? std::max(hi[q], id[q]) : id[q];
      }
    }
    // computeFrontierInfo (:374-390): mean of voxel centres = centre of the mean index
    const double nn = (double)c.size();
    for (int q = 0; q < 3; ++q) {
      c.avg[q] = ((double)sum[q] / nn + 0.5) * g.res + g.org[q];
      c.bmin[q] = ((int)lo[q] + 0.5) * g.res + g.org[q];
      c.bmax[q] = ((int)hi[q] + 0.5) * g.res + g.org[q];
    }
    if (ref_order) {
      // the reference's own evaluation: cell centres added one by one in list order, then divided; the box
      // from the same centres (identical to the index form above)
      double sm[3] = {0.0, 0.0, 0.0};
      u32 blo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, bhi[3] = {0u, 0u, 0u};
      const int* cl = c.lazy;
      const u32 ncell = c.lazy_n;
      for (u32 i = 0; i < ncell; ++i) {
        const u32 a = (u32)cl[i];
        const u32 x = a / (u32)g.nyz, rr = a - x * (u32)g.nyz, y = rr / (u32)g.nz, z = rr - y * (u32)g.nz;
        const u32 id[3] = {x, y, z};
        for (int q = 0; q < 3; ++q) {
          sm[q] += ((double)id[q] + 0.5) * g.res + g.org[q];
          blo[q] = std::min(blo[q], id[q]);
          bhi[q] = std::max(bhi[q], id[q]);
        }
      }
      for (int q = 0; q < 3; ++q) {
        c.avg[q] = sm[q] / (double)ncell;
        c.bmin[q] = ((int)blo[q] + 0.5) * g.res + g.org[q];
        c.bmax[q] = ((int)bhi[q] + 0.5) * g.res + g.org[q];
      }
    }
  }
  return FUELMI_OK;
}

// searchFrontiers, second half: waits for the pipeline and assembles tmp_frontiers_.
extern "C" int fuelmi_frontier_search_end(fuelmi_frontier* f, int* n_new) {
  ARGCHK(f && n_new);
  *n_new = 0;
  FRONTIER_HAS_MAP(f);
  if (!f->pending) {
    fuelmi_set_error("fuelmi_frontier_search_end without a matching _begin");
    return FUELMI_EINVAL;
  }
  f->pending = false;
  struct ScopeEnd {  // closes the profiling bracket on every exit path
    fuelmi_frontier* f;
    ~ScopeEnd() { f->scope.reset(); }
  } scope_end{f};
  fuelmi_map* m = f->map;
  HIPCHK(hipSetDevice(m->device));
  // (a plane mutator issued from here on comes behind this call's wait for the chain's result: the plane-reading
  // kernels are done by then -- nothing left for it to wait for)
  struct DropLate {
    fuelmi_frontier* f;
    ~DropLate() {
      if (f->map) map_drop_late_reader(f->map, f->ev_planes_read);
    }
  } drop_late{f};
  if (f->search_empty) {
    if (!f->pend_rm.empty()) {
      HIPCHK(hipStreamSynchronize(f->stream));
      remove_changed_end(f);
    }
    return FUELMI_OK;
  }
  FArgs& F = f->F;
  const u32* counts = F.h_counts;
  F.fast = 0;
  g_ht.start();
  if (g_ht.on) --g_ht.n;
  g_ht.lap(10);
  if (f->fast_launched) {
    const int rc = frontier_collect_fast(f);
    if (rc) return rc;
  } else {
    ++f->n_legacy;
    HIPCHK(stream_poll(f->stream));
  }
  remove_changed_end(f);
  if (f->rm_failed) {
    f->rm_failed = false;
    f->dirty_all = true;
    fuelmi_set_error("frontier search: the changed-cluster test's in-kernel barrier timed out (device oversubscribed for 50 ms?)");
    return FUELMI_EHIP;
  }
  if (counts[2] || counts[3] > F.cap_kept) {
    fuelmi_set_error("frontier capacity exceeded (cells %u/%u seeds %u/%u clusters %u/%u)", counts[0], F.cap_q,
                     counts[1], F.cap_s, counts[3], F.cap_kept);
    return FUELMI_ELIMIT;
  }
  const u32 nq = counts[0], nkept = counts[3], n_out = counts[5];
  f->last_nkept = (int)nkept;
  if (nkept > 256 && f->npass < 2) {
    const int rc = frontier_second_pass(f);
    if (rc) return rc;
  }
  if (nkept == 0) {
    f->dirty_all = false;
    f->seen_epoch = m->occ_epoch;
    return FUELMI_OK;
  }
  const int rc = frontier_assemble(f, nq, nkept, n_out);
  if (rc) return rc;
  *n_new = (int)f->tmp.size();
  f->dirty_all = false;
  f->seen_epoch = m->occ_epoch;
  g_ht.lap(12);
  return FUELMI_OK;
}


extern "C" int fuelmi_frontier_search(fuelmi_frontier* f, int* n_new) {
  ARGCHK(f && n_new);
  int rc = fuelmi_frontier_search_begin(f);
  if (rc) return rc;
  return fuelmi_frontier_search_end(f, n_new);
}

extern "C" int fuelmi_frontier_synchronize(fuelmi_frontier* f) {
  ARGCHK(f);
  FRONTIER_HAS_MAP(f);
  HIPCHK(hipSetDevice(f->device));
  f->tail_pending = false;
  HIPCHK(frontier_drain(f));
  return FUELMI_OK;
}
extern "C" int fuelmi_frontier_resolved_in_launch(const fuelmi_frontier* f) { return f ? f->n_in_launch : FUELMI_EINVAL; }
extern "C" int fuelmi_frontier_stats(const fuelmi_frontier* f, int out3[3]) {
  ARGCHK(f && out3);
  out3[0] = f->n_fast, out3[1] = f->n_legacy, out3[2] = f->n_fallback;
  return FUELMI_OK;
}
extern "C" int fuelmi_frontier_path_stats(const fuelmi_frontier* f, int out2[2]) {
  ARGCHK(f && out2);
  out2[0] = f->n_late_resolve, out2[1] = f->n_retiled;
  return FUELMI_OK;
}
extern "C" int fuelmi_frontier_changed_stats(const fuelmi_frontier* f, int out[9]) {
  ARGCHK(f && out);
  for (int k = 0; k < 4; ++k) out[k] = f->rm_paths[k];
  out[4] = f->rm_last_nc, out[5] = (int)f->rm_last_total, out[6] = f->rm_last_mark;
  out[7] = f->n_pool_rebuilds, out[8] = (int)f->pool_cap;
  return FUELMI_OK;
}
extern "C" int fuelmi_frontier_order_stats(const fuelmi_frontier* f, int out4[4]) {
  ARGCHK(f && out4);
  out4[0] = f->order_last, out4[1] = f->n_order_ref, out4[2] = f->n_order_fallback, out4[3] = (int)f->order_fallback_cells;
  return FUELMI_OK;
}

extern "C" int fuelmi_frontier_reset(fuelmi_frontier* f) {
  ARGCHK(f);
  FRONTIER_HAS_MAP(f);
  FRONTIER_NOT_SEARCHING(f, "fuelmi_frontier_reset");
  fuelmi_map* m = f->map;
  HIPCHK(hipSetDevice(m->device));
  f->frontiers.clear();
  f->dormant.clear();
  f->prev.clear();
  if (f->keep_prev && f->stream2 && !f->fresh_pending && !f->tmp.empty()) {
    // the new clusters of the last search stay readable as list 3 (see fuelmi_frontier::prev): their cells are in
    // the buffer set this reset retires.  Whatever still has to happen to them -- the search's tail, the copy of a
    // large grouped cell list to the pinned block -- is queued on the retiring stream now and waited for by whoever
    // reads list 3, not here
    f->prev.swap(f->tmp);
    if (f->cells_fetch) {
      f->cells_fetch = false;
      HIPCHK(hipMemcpyAsync(f->F.h_cells, f->F.ms_val[f->last_fin], (size_t)f->cells_fetch_n * sizeof(u32), hipMemcpyDeviceToHost,
                            f->stream));
    }
    HIPCHK(hipEventRecord(f->ev_prev, f->stream));
    f->prev_pending = true;
    f->tail_pending = false;
  }
  f->tmp.clear();
  f->removed_ids.clear();
  f->dirty_all = true;
  f->pool_used = 0;
  f->fresh_pending = true;  // executed by the next search (folded into its first kernel) or by whoever reads the flags
  return FUELMI_OK;
}

extern "C" int fuelmi_frontier_keep_previous(fuelmi_frontier* f, int on) {
  ARGCHK(f);
  f->keep_prev = on != 0;
  if (!on) f->prev.clear();
  return FUELMI_OK;
}

extern "C" int fuelmi_frontier_commit(fuelmi_frontier* f, int dormant) {
  ARGCHK(f);
  FRONTIER_HAS_MAP(f);
  FRONTIER_NOT_SEARCHING(f, "fuelmi_frontier_commit");
  auto& dst = dormant ? f->dormant : f->frontiers;
  HIPCHK(hipSetDevice(f->map->device));
  const int rc = frontier_keep_clusters(f, f->tmp);
  if (rc) return rc;
  dst.splice(dst.end(), f->tmp);
  return FUELMI_OK;
}

