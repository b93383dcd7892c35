// bench_drivers.hip -- measurement drivers of bench.py: the plan cycle and the streaming cycle issued from C++
// (map, frontier finder and B-spline batch together, through the public C-ABI), so that the host's time per cycle
// is the library's and not the Python caller's.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <vector>

#include "frontier_internal.h"

// ---- measurement driver (bench.py): the plan cycle issued from C++ ---------------------------------------
extern "C" int fuelmi_bench_cycles(fuelmi_map* m, fuelmi_frontier* f, fuelmi_bspline_dev* batch, const double ub_min[3],
                                   const double ub_max[3], int n, int serial, int* n_clusters, double* seconds) {
  ARGCHK(m && f && ub_min && ub_max && n >= 0 && n_clusters && seconds && f->map == m);
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  HIPCHK(frontier_drain(f));
  int rc = FUELMI_OK, ncl = 0;
  f->wait_us_acc = 0.0;
  using clk = std::chrono::steady_clock;
  // host time of every C-ABI call of the cycle (seven clock reads per cycle, ~0.2 us): fuelmi_bench_host_profile
  double hp[6] = {0, 0, 0, 0, 0, 0};
  auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
  const auto t0 = clk::now();
  for (int k = 0; k < n && rc == FUELMI_OK; ++k) {
    const auto a0 = clk::now();
    if ((rc = fuelmi_frontier_reset(f))) break;
    if ((rc = fuelmi_map_set_updated_box(m, ub_min, ub_max))) break;
    const auto a1 = clk::now();
    if (!serial && (rc = fuelmi_frontier_search_begin(f))) break;
    const auto a2 = clk::now();
    if ((rc = fuelmi_map_inflate_local(m))) break;
    const auto a3 = clk::now();
    if ((rc = fuelmi_map_update_esdf(m))) break;
    const auto a4 = clk::now();
    if (batch && (rc = fuelmi_bspline_dev_eval(batch))) break;
    const auto a5 = clk::now();
    if (serial) {
      HIPCHK(hipStreamSynchronize(m->stream));
      if ((rc = fuelmi_frontier_search_begin(f))) break;
    }
    if ((rc = fuelmi_frontier_search_end(f, &ncl))) break;
    const auto a6 = clk::now();
    hp[0] += us(a0, a1), hp[1] += us(a1, a2), hp[2] += us(a2, a3), hp[3] += us(a3, a4), hp[4] += us(a4, a5), hp[5] += us(a5, a6);
  }
  if (rc) return rc;
  HIPCHK(stream_wait(m->stream));
  HIPCHK(frontier_drain(f));
  f->tail_pending = false;
  *seconds = std::chrono::duration<double>(clk::now() - t0).count();
  *n_clusters = ncl;
  for (int q = 0; q < 6; ++q) m->bench_host_us[q] = n ? hp[q] / n : 0.0;
  m->bench_host_us[6] = f->wait_us_acc / std::max(n, 1);
  f->wait_us_acc = 0.0;
  g_ht.report();
  return FUELMI_OK;
}
extern "C" int fuelmi_bench_host_profile(const fuelmi_map* m, double out7[7]) {
  ARGCHK(m && out7);
  for (int q = 0; q < 7; ++q) out7[q] = m->bench_host_us[q];
  return FUELMI_OK;
}

// The same cycle with its results DELIVERED to the host containers the reference's callers read
// (fast_exploration_manager.cpp:99-114: the cluster cell lists of searchFrontiers; planner_manager.cpp:296-314: the
// cost and gradient of every candidate): after every search the cells of all new clusters are copied into
// cells_out (cluster after cluster, as many as fit), after every evaluation cost[C] / grad[C * nvar] are downloaded.
// seconds3: [0] elapsed wall time, [1] of it in the cell copies, [2] in the cost / gradient download.
extern "C" int fuelmi_bench_cycles_delivered(fuelmi_map* m, fuelmi_frontier* f, fuelmi_bspline_dev* batch,
                                             const double ub_min[3], const double ub_max[3], int n, int* cells_out,
                                             size_t cells_cap, double* cost, double* grad, int* n_clusters,
                                             double* seconds3) {
  ARGCHK(m && f && ub_min && ub_max && n >= 0 && n_clusters && seconds3 && cells_out && f->map == m);
  ARGCHK(!batch || (cost && grad));
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  HIPCHK(frontier_drain(f));
  int rc = FUELMI_OK, ncl = 0;
  double t_cells = 0.0, t_cg = 0.0;
  using clk = std::chrono::steady_clock;
  const bool kept = f->keep_prev;
  (void)fuelmi_frontier_keep_previous(f, 1);
  // Results are consumed one cycle behind the device: while cycle k runs, the host copies out what cycle k - 1 found
  // -- its cluster cells from the retired buffer set (list 3), its costs and gradients from the pinned slot the
  // B-spline kernel wrote them to.  Every cycle's results are delivered (the last one's after the loop); nothing
  // blocks on a copy engine.
  auto deliver = [&](int cyc, int ncl_of) -> int {
    const auto ta = clk::now();
    size_t at = 0;
    int r2 = FUELMI_OK;
    const int which = cyc < 0 ? 0 : 3;  // (the last cycle has not been retired: its clusters are still list 0)
    const int cnt = fuelmi_frontier_count(f, which);
    for (int c = 0; c < cnt && c < ncl_of && r2 == FUELMI_OK; ++c) {
      const int sz = fuelmi_frontier_cluster_size(f, which, c);
      if (sz < 0 || at + (size_t)sz > cells_cap) break;
      r2 = fuelmi_frontier_cluster_cells(f, which, c, cells_out + at);
      at += (size_t)sz;
    }
    const auto tb = clk::now();
    if (r2 == FUELMI_OK && batch) r2 = fuelmi_bspline_dev_collect(batch, (cyc < 0 ? n - 1 : cyc) & 1, cost, grad);
    const auto tc = clk::now();
    t_cells += std::chrono::duration<double>(tb - ta).count();
    t_cg += std::chrono::duration<double>(tc - tb).count();
    return r2;
  };
  const auto t0 = clk::now();
  int ncl_prev = 0;
  for (int k = 0; k < n && rc == FUELMI_OK; ++k) {
    if ((rc = fuelmi_frontier_reset(f))) break;  // (retires cycle k - 1's clusters to list 3)
    if ((rc = fuelmi_map_set_updated_box(m, ub_min, ub_max))) break;
    if ((rc = fuelmi_frontier_search_begin(f))) break;
    if ((rc = fuelmi_map_inflate_local(m))) break;
    if ((rc = fuelmi_map_update_esdf(m))) break;
    if (batch && (rc = fuelmi_bspline_dev_eval_pinned(batch, k & 1))) break;
    if (k > 0 && (rc = deliver(k - 1, ncl_prev))) break;
    if ((rc = fuelmi_frontier_search_end(f, &ncl))) break;
    ncl_prev = ncl;
  }
  if (rc == FUELMI_OK && n > 0) rc = deliver(-1, ncl_prev);
  (void)fuelmi_frontier_keep_previous(f, kept ? 1 : 0);
  if (rc) return rc;
  HIPCHK(stream_wait(m->stream));
  HIPCHK(frontier_drain(f));
  f->tail_pending = false;
  seconds3[0] = std::chrono::duration<double>(clk::now() - t0).count();
  seconds3[1] = t_cells;
  seconds3[2] = t_cg;
  *n_clusters = ncl;
  return FUELMI_OK;
}

// Measurement driver for the streaming cycle (one depth frame per cycle), issued from C++ like fuelmi_bench_cycles.
extern "C" int fuelmi_bench_stream(fuelmi_map* m, fuelmi_frontier* f, fuelmi_bspline_dev* batch, int n,
                                   const void* const* depth, int rows, int cols, const fuelmi_depth_cfg* cfg,
                                   const double* cam_pos3, const double* cam_q4, int serial, int* n_clusters,
                                   double* box_voxels, double* seconds) {
  ARGCHK(m && f && n >= 0 && depth && cfg && cam_pos3 && cam_q4 && n_clusters && seconds && f->map == m);
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  HIPCHK(frontier_drain(f));
  int rc = FUELMI_OK, ncl = 0;
  double vox = 0.0;
  const auto t0 = std::chrono::steady_clock::now();
  // Frame k + 1 is fused while the search of frame k is still running: the search reads the occupancy planes only in
  // its first kernels, the fusion waits for those ON THE DEVICE (map_wait_plane_readers), and the host's wait for the
  // fused frame's box (which the next search needs) falls beside the chain instead of in front of it.  Per frame: the
  // search bookkeeping (collect + commit the previous search, begin this one), the map chain (inflation, ESDF, B-spline
  // batch), the next fusion.  The frame is bound by the host's ~55 us of API calls plus the device's fusion ->
  // plane-reading kernels -> fusion chain (FUELMI_STREAM_TIMING=1: host time per call group, =2: also a device timeline
  // from events); issuing the map chain BEFORE the bookkeeping (measured in round 4) starts the map stream ~25 us
  // earlier and the search chain as much later: 1-2 % slower.  Same calls, same arguments, same results as the
  // frame-by-frame order (serial != 0 keeps that order for diagnostics).
  int npts = 0;
  if (n > 0)
    rc = fuelmi_map_input_depth(m, static_cast<const unsigned short*>(depth[0]), rows, cols, cfg, cam_pos3, cam_q4, &npts);
  auto map_chain = [&]() -> int {
    int r = FUELMI_OK;
    if (npts > 0) {
      int lo[3], hi[3];
      if ((r = fuelmi_map_get_local_bound(m, lo, hi))) return r;
      vox += (double)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
      if ((r = fuelmi_map_inflate_local(m))) return r;
      if ((r = fuelmi_map_update_esdf(m))) return r;
    }
    if (batch) r = fuelmi_bspline_dev_eval(batch);
    return r;
  };
  auto fuse_next = [&](int k, int* np) -> int {
    return fuelmi_map_input_depth(m, static_cast<const unsigned short*>(depth[k + 1]), rows, cols, cfg, cam_pos3 + 3 * (k + 1),
                                  cam_q4 + 4 * (k + 1), np);
  };
  if (serial) {
    for (int k = 0; k < n && rc == FUELMI_OK; ++k) {
      if ((rc = map_chain())) break;
      int npts_next = 0;
      HIPCHK(hipStreamSynchronize(m->stream));
      if ((rc = fuelmi_frontier_search_begin(f))) break;
      if ((rc = fuelmi_frontier_search_end(f, &ncl))) break;
      if ((rc = fuelmi_frontier_commit(f, 0))) break;
      if (k + 1 < n && (rc = fuse_next(k, &npts_next))) break;
      npts = npts_next;
    }
  } else {
    static const bool timing = getenv("FUELMI_STREAM_TIMING") != nullptr;  // host wall clock of every call of the loop
    double acc[5] = {0, 0, 0, 0, 0};
    auto tick = [&](int slot, std::chrono::steady_clock::time_point& t) {
      if (!timing) return;
      const auto now = std::chrono::steady_clock::now();
      acc[slot] += std::chrono::duration<double, std::micro>(now - t).count();
      t = now;
    };
    static const bool timeline = timing && atoi(getenv("FUELMI_STREAM_TIMING")) >= 2;  // + device timeline (events)
    std::vector<hipEvent_t> tl;  // per frame: chain start, planes read, resolved, tail done, fusion done, map chain done
    if (timeline) {
      tl.resize((size_t)n * 6);
      for (auto& e : tl) HIPCHK(hipEventCreate(&e));
    }
    // (Round 4 also tried a second host thread for the search bookkeeping, like the reference's separate map and
    // planning callbacks: launches from two threads serialise inside the HIP runtime and each gets slower -- 7.4 k
    // frames/s against 8.1 k.  One thread issues everything.)
    auto bookkeeping = [&](int k) -> int {
      int r = FUELMI_OK;
      if (k > 0) {
        if ((r = fuelmi_frontier_search_end(f, &ncl))) return r;
        if ((r = fuelmi_frontier_commit(f, 0))) return r;
      }
      return fuelmi_frontier_search_begin(f);
    };
    for (int k = 0; k < n && rc == FUELMI_OK; ++k) {
      auto t = std::chrono::steady_clock::now();
      if (timeline) {
        if (hipEventRecord(tl[(size_t)k * 6 + 4], m->stream) != hipSuccess) rc = FUELMI_EHIP;  // (the fusion of this frame is queued)
        f->tl_ev = &tl[(size_t)k * 6];
      }
      if (rc == FUELMI_OK) rc = bookkeeping(k);
      tick(3, t);
      if (rc == FUELMI_OK) rc = map_chain();
      if (timeline && rc == FUELMI_OK && hipEventRecord(tl[(size_t)k * 6 + 5], m->stream) != hipSuccess) rc = FUELMI_EHIP;
      tick(0, t);
      if (rc) break;
      int npts_next = 0;
      if (k + 1 < n && (rc = fuse_next(k, &npts_next))) break;
      tick(4, t);
      npts = npts_next;
    }
    if (timeline) {
      f->tl_ev = nullptr;
      HIPCHK(hipStreamSynchronize(m->stream));
      HIPCHK(frontier_drain(f));
      double off[6] = {0, 0, 0, 0, 0, 0}, period = 0;
      int cnt = 0;
      for (int k = 10; k + 1 < n; ++k) {
        float ms = 0.f;
        const hipEvent_t base = tl[(size_t)k * 6 + 4];  // fusion of frame k done
        bool okf = true;
        double o[6];
        for (int j = 0; j < 6 && okf; ++j) {
          okf = hipEventElapsedTime(&ms, base, tl[(size_t)k * 6 + j]) == hipSuccess;
          o[j] = ms * 1e3;
        }
        if (okf) okf = hipEventElapsedTime(&ms, base, tl[(size_t)(k + 1) * 6 + 4]) == hipSuccess;
        if (!okf) {
          (void)hipGetLastError();
          continue;
        }
        for (int j = 0; j < 6; ++j) off[j] += o[j];
        period += ms * 1e3;
        ++cnt;
      }
      if (cnt)
        std::fprintf(stderr, "[stream-timing] device timeline, us after the frame's fusion finished: map chain done %.1f; search "
                     "chain starts %.1f, planes read %.1f, resolved %.1f, tail done %.1f; next frame's fusion done %.1f (%d frames)\n",
                     off[5] / cnt, off[0] / cnt, off[1] / cnt, off[2] / cnt, off[3] / cnt, period / cnt, cnt);
      for (auto& e : tl) (void)hipEventDestroy(e);
    }
    if (timing && n > 0)
      std::fprintf(stderr, "[stream-timing] host us per frame: map chain %.1f, search bookkeeping (collect, commit, begin) %.1f, "
                   "input_depth (blocked on the device) %.1f\n", acc[0] / n, acc[3] / n, acc[4] / n);
    if (rc == FUELMI_OK && n > 0) {
      if ((rc = fuelmi_frontier_search_end(f, &ncl)) == FUELMI_OK) rc = fuelmi_frontier_commit(f, 0);
    }
  }
  if (rc) return rc;
  HIPCHK(stream_wait(m->stream));
  HIPCHK(frontier_drain(f));
  f->tail_pending = false;
  *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *n_clusters = ncl;
  if (box_voxels) *box_voxels = vox;
  return FUELMI_OK;
}
