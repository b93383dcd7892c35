// frontier_tile.hip -- FAST PATH of the clustering chain ("tile-root resolve")
//
// The legacy chain (frontier_legacy.hip) runs the cross-tile merge, the claims, the cluster sizes, the kept list and
// its ranking on the ~10^5 CELLS through device-scope atomics: five dependent kernels (k_union ..
// k_rank_kept, ~60 us) whose time is atomic latency.  Here a tile describes each of its local
// components by ONE record (k_tile_ccl: size, lowest claimer inside the scan box, index sums, index box,
// cells per x-row) and lists the component pairs that touch across tile faces (k_tile_cross); one
// workgroup then does all of the above on those few thousand records in its LDS (k_resolve).
//
// Round 3: no compaction anywhere, and no predicate pass in front.  The round-2 chain compacted the cells in address
// order first (predicate + in-block prefix, scan of the block sums, ordered compaction) and every later kernel found
// a cell's neighbours through rank look-ups in those tables (three dependent loads each); regrouping the cells by
// cluster took a histogram kernel and a scatter kernel.  Now four kernels:
//   k_tile_ccl  : a tile evaluates the frontier predicate for its own voxels straight from the occupancy planes,
//                 keeps the Q0 / seed bits of its 32-voxel segments in per-tile arrays (tq / ts), labels its cells run
//                 by run in LDS, writes one record per component and the component number of every cell BY VOXEL
//                 ADDRESS (vlab, one byte per voxel)
//   k_tile_cross: relations across tile faces + NQ seed claims, neighbours looked up in tq / vlab
//   k_resolve   : unions, clusters, ranks; additionally the (kept cluster x tile column) prefix matrix
//   k_tile_out  : flags + the grouped cell list: a cell's position = offset of its cluster + cells of the cluster
//                 in earlier tile columns (matrix) + in earlier x-rows / earlier tiles of its own column (per-row
//                 counts of the column's components) + earlier cells of its own row of the tile
// fuelmi_frontier_reset costs no kernel: the finder owns two flag planes and swaps to the zeroed one.
// Capacity limits (FR_* in frontier_internal.h) are those of pathological inputs (noise-like occupancy);
// when one is hit, or cluster_min < 1 (every NQ seed is then a cluster of its own), the search runs the
// legacy chain instead.  Results are identical (tests run both).
//
// Host side: frontier_enqueue_fast (the four launches of a search), the late resolve, the tile menu (kFastMenu) and
// the per-menu LDS sizes fuelmi_frontier_create reserves, declared in frontier_internal.h.
#include <algorithm>
#include <cstdlib>

#include "frontier_internal.h"

// ---- tiles ----------------------------------------------------------------------------------------
struct TileGeo {
  int tx, ty, x0, y0, nxl, nyl, TX, TY, nseg, items;
};
// What the tile kernels behind k_tile_ccl need before they can issue their bulk loads -- the per-search block, the
// chain's overflow verdict, the tile's component count and id base -- fetched by different lanes in ONE round trip and
// handed round through LDS.  (Read field by field from global memory, with an early return in between, this was
// five dependent round trips at the head of every workgroup.)
struct TilePro {
  FVar V;
  u32 ovf, nroots, gbase, pad;
};
__device__ __forceinline__ void stage_tile_pro(const FArgs& F, TilePro* sp) {
  constexpr int NV = (int)(sizeof(FVar) / 4);
  static_assert(sizeof(FVar) % 4 == 0 && NV + 3 <= 64, "FVar does not fit one wave's lanes");
  const int t = threadIdx.x;
  // (the address is selected, not the load: one load instruction, one wait)
  const u32* src = reinterpret_cast<const u32*>(F.var) + (t < NV ? t : 0);
  if (t == NV) src = F.counts + 2;
  if (t == NV + 1) src = F.t_nroots + blockIdx.x;
  if (t == NV + 2) src = F.t_base + blockIdx.x;
  if (t < NV + 3) reinterpret_cast<u32*>(sp)[t] = *src;
  __syncthreads();
}
__device__ __forceinline__ TileGeo tile_geo(const Geo& g, const FVar& V, int t) {
  TileGeo T;
  T.TX = V.ftx, T.TY = V.fty;
  T.tx = t / V.nty_f, T.ty = t - T.tx * V.nty_f;
  T.x0 = V.px0 + T.tx * T.TX, T.y0 = V.py0 + T.ty * T.TY;
  T.nxl = min(T.TX, V.px1 - T.x0 + 1), T.nyl = min(T.TY, V.py1 - T.y0 + 1);
  T.nseg = (g.nz + 31) >> 5;
  T.items = T.TX * T.TY * T.nseg;
  return T;
}
__device__ __forceinline__ long tile_line_adr(const Geo& g, const TileGeo& T, int line) {  // address of voxel z = 0
  const int lx = line / T.TY, ly = line - lx * T.TY;
  return (long)(T.x0 + lx) * g.nyz + (long)(T.y0 + ly) * g.nz;
}

#define FT_PER 8  // segments a lane of the tile kernels handles at most (tile segments / workgroup size)
#define FT_TRIP 2  // segments of a lane whose plane windows are fetched side by side (4 measured no faster than 2: the fetch
                   // is bound by the number of load instructions x cache lines they touch, not by their latency)
// ---- the predicate inside the tile kernel ----------------------------------------------------------------
// Q0 and NQ-seed bits of the 32 voxels from address a = (x, y, 32 c): knownfree && isNeighborUnknown
// (frontier_finder.cpp:862-877) && flag == 0, cut to the Q region / the scan box -- what k_pred / f1_word compute
// per 64-voxel word, per segment here.  The seven plane windows are independent loads.
struct SegPred {
  u32 q, s;
};
// 32 bits of a plane from (signed) bit index `bit`, through 32-bit loads: the planes are little-endian u64 words, so
// bit b of the plane is bit (b & 31) of the 32-bit word b >> 5 -- half the bytes of plane_window per window
// (both words of a window in ONE 8-byte load at 4-byte alignment -- the tile kernels are bound by how many load
// instructions and cache-line look-ups their scattered windows cost, and two 4-byte loads look the same line up twice;
// the word behind the last one of a plane lies in its zeroed margin)
struct __attribute__((packed, aligned(4))) W2 {
  u32 a, b;
};
struct __attribute__((packed, aligned(4))) W3 {
  u32 a, b, c;
};
__device__ __forceinline__ u32 plane_window32(const u64* __restrict__ p, long bit) {
  const u32* q = reinterpret_cast<const u32*>(p);
  const long wi = bit >> 5;
  const int sh = (int)(bit & 31);
  const W2 w = *reinterpret_cast<const W2*>(q + wi);
  return (u32)((((u64)w.b << 32) | (u64)w.a) >> sh);
}
__device__ __forceinline__ SegPred seg_predicate(const Geo& g, const FVar& V, const FArgs& F, int x, int y, int c) {
  const long a = (long)x * g.nyz + (long)y * g.nz + 32 * c;
  const int zn = min(32, g.nz - 32 * c);
  u64 W;  // the unknown plane at z = 32 c - 1 .. 32 c + 32 (bit 0 <-> z = 32 c - 1): three 32-bit words
  {
    const u32* q = reinterpret_cast<const u32*>(F.unk);
    const long wi = (a - 1) >> 5;
    const int sh = (int)((a - 1) & 31);
    const W3 w = *reinterpret_cast<const W3*>(q + wi);
    const u64 w01 = (u64)w.a | ((u64)w.b << 32);
    W = (w01 >> sh) | (((u64)w.c << 1) << (63 - sh));  // (no branch on sh: a load inside a branch is waited for inside it)
  }
  // Every window is fetched unconditionally and masked afterwards: the planes carry zeroed margins of more than a
  // slab on both sides, so the lines "before" y = 0 and "after" y = ny - 1 are addressable (they are the neighbouring
  // slab's lines, or margin), and seven independent loads cost one round trip where seven guarded ones cost seven.
  const u32 occw = plane_window32(F.occ, a);
  const u32 ym_raw = plane_window32(F.unk, a - g.nz), yp_raw = plane_window32(F.unk, a + g.nz);
  const u32 xm = plane_window32(F.unk, a - g.nyz), xp = plane_window32(F.unk, a + g.nyz);  // (zero margins beyond the map)
  const u32 fl_raw = plane_window32(F.flag, a);
  const u32 ym = y > 0 ? ym_raw : 0u, yp = y < g.ny - 1 ? yp_raw : 0u;
  const u32 fl = V.fresh ? 0u : fl_raw;
  u32 down = (u32)W, up = (u32)(W >> 2);
  const u32 self_unk = (u32)(W >> 1);
  if (c == 0) down &= ~1u;                                   // z = 0 has no lower neighbour
  if (g.nz - 32 * c <= 32) up &= ~(1u << (zn - 1));          // z = nz - 1 (this segment's last voxel) has no upper one
  const u32 valid = zn < 32 ? (1u << zn) - 1u : 0xFFFFFFFFu;
  const u32 f1 = ~occw & ~self_unk & (down | up | ym | yp | xm | xp) & valid & ~fl;
  auto zmask = [&](const Box3& b) -> u32 {
    if (x < b.lo[0] || x > b.hi[0] || y < b.lo[1] || y > b.hi[1]) return 0u;
    const int lo = max(32 * c, b.lo[2]) - 32 * c, hi = min(32 * c + 31, b.hi[2]) - 32 * c;
    if (lo > hi) return 0u;
    return ((hi - lo + 1 >= 32) ? 0xFFFFFFFFu : ((1u << (hi - lo + 1)) - 1u)) << lo;
  };
  const u32 mq = zmask(V.qreg), ms = zmask(V.sbox);
  SegPred r;
  r.q = f1 & mq;
  r.s = f1 & ms & ~mq;
  return r;
}

// The tile's segments: predicate, Q0 bits + exclusive prefix + CCL labels and the seed bits in the LDS (the caller
// copies both bit arrays into the per-tile arrays tq / ts -- what the later kernels and the neighbouring tiles read:
// coalesced, and no 64-bit plane that tiles ending in the middle of a word would have to share).  FT_TRIP segments per
// lane and trip.
template <int NT>
__device__ __forceinline__ u32 tile_load_pred(const Geo& g, const TileGeo& T, const FVar& V, const FArgs& F, u32* segb,
                                              u32* segpre, u32* s_wsum, u32* lab, u32* segs, unsigned short* cseg) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per = (T.items + NT - 1) / NT;  // <= FT_PER (checked on the host)
  const int it0 = threadIdx.x * per;
  u32 cnt = 0u;
  // (line, segment) of the lane's first item; the following ones by counting (a division by a run-time value is ~25
  // instructions, and this phase is bound by instruction issue)
  int c, lx, ly;
  {
    const int line = it0 / T.nseg;
    c = it0 - line * T.nseg;
    lx = line / T.TY;
    ly = line - lx * T.TY;
  }
#pragma nounroll
  for (int k0 = 0; k0 < per; k0 += FT_TRIP) {
    SegPred r[FT_TRIP];
#pragma unroll
    for (int h = 0; h < FT_TRIP; ++h) {
      r[h].q = r[h].s = 0u;
      const int it = it0 + k0 + h;
      if (k0 + h < per && it < T.items && lx < T.nxl && ly < T.nyl) r[h] = seg_predicate(g, V, F, T.x0 + lx, T.y0 + ly, c);
      if (++c == T.nseg) {
        c = 0;
        if (++ly == T.TY) ly = 0, ++lx;
      }
    }
#pragma unroll
    for (int h = 0; h < FT_TRIP; ++h) {
      const int it = it0 + k0 + h;
      if (k0 + h < per && it < T.items) {
        segb[it] = r[h].q, segs[it] = r[h].s;  // (to memory later: a store in front of a barrier is a round trip)
        cnt += (u32)__popc(r[h].q);
      }
    }
  }
  u32 v = cnt;
  for (int off = 1; off < 64; off <<= 1) {
    const u32 t = (u32)__shfl_up((int)v, off, 64);
    if (lane >= off) v += t;
  }
  if (lane == 63) s_wsum[wave] = v;
  __syncthreads();
  u32 woff = 0u, tot = 0u;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    if (k < wave) woff += s_wsum[k];
    tot += s_wsum[k];
  }
  u32 run = woff + v - cnt;
#pragma nounroll
  for (int k = 0; k < per; ++k) {
    if (it0 + k >= T.items) break;
    u32 rem = segb[it0 + k];  // (the lane re-reads what it just wrote)
    segpre[it0 + k] = run;
    if (tot <= FR_TCELL) {  // labels of the CCL: start of the cell's z-run inside its segment (runs are pre-joined)
      u32 l = run;
      while (rem) {
        const int s0 = __builtin_ctz(rem);
        const u32 inv = ~(rem >> s0);
        const int len = min(inv ? __builtin_ctz(inv) : 32, 32 - s0);
        rem &= ~((len >= 32 ? 0xFFFFFFFFu : ((1u << len) - 1u)) << s0);
        for (int q = 0; q < len; ++q) lab[l + (u32)q] = l, cseg[l + (u32)q] = (unsigned short)(it0 + k);  // (cell -> segment:
        l += (u32)len;                                                         // what a bisection of the prefix would find)
      }
    }
    run += (u32)__popc(segb[it0 + k]);
  }
  if (threadIdx.x == 0) segpre[T.items] = tot;
  __syncthreads();
  return tot;
}
// a tile's own bits from the arrays (k_tile_cross, k_tile_out): coalesced, no shifting
template <int NT, bool SCAN>
__device__ __forceinline__ u32 tile_load_arrays(const TileGeo& T, const FArgs& F, u32* segb, u32* segpre, u32* s_wsum,
                                                u32* segs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32* tq = F.tq + (size_t)blockIdx.x * T.items;
  const u32* ts = F.ts + (size_t)blockIdx.x * T.items;
  const int per = (T.items + NT - 1) / NT;
  const int it0 = threadIdx.x * per;
  u32 b[FT_PER], b2[FT_PER];
#pragma unroll
  for (int k = 0; k < FT_PER; ++k) {
    b[k] = b2[k] = 0u;
    if (k < per && it0 + k < T.items) b[k] = tq[it0 + k], b2[k] = ts[it0 + k];
  }
  u32 cnt = 0u;
#pragma unroll
  for (int k = 0; k < FT_PER; ++k)
    if (k < per && it0 + k < T.items) {
      segb[it0 + k] = b[k], segs[it0 + k] = b2[k];
      cnt += (u32)__popc(b[k]);
    }
  if (!SCAN) {
    __syncthreads();
    return 0u;
  }
  u32 v = cnt;
  for (int off = 1; off < 64; off <<= 1) {
    const u32 t = (u32)__shfl_up((int)v, off, 64);
    if (lane >= off) v += t;
  }
  if (lane == 63) s_wsum[wave] = v;
  __syncthreads();
  u32 woff = 0u, tot = 0u;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    if (k < wave) woff += s_wsum[k];
    tot += s_wsum[k];
  }
  u32 run = woff + v - cnt;
#pragma unroll
  for (int k = 0; k < FT_PER; ++k)
    if (k < per && it0 + k < T.items) {
      segpre[it0 + k] = run;
      run += (u32)__popc(b[k]);
    }
  if (threadIdx.x == 0) segpre[T.items] = tot;
  __syncthreads();
  return tot;
}
// first run of set bits of m (m != 0): start bit, length; removes it from m
__device__ __forceinline__ void pop_run32(u32& m, int& s, int& len) {
  s = __builtin_ctz(m);
  const u32 inv = ~(m >> s);
  len = inv ? __builtin_ctz(inv) : 32;
  len = min(len, 32 - s);
  m &= ~((len >= 32 ? 0xFFFFFFFFu : ((1u << len) - 1u)) << s);
}
__device__ __forceinline__ void pop_run64(u64& m, int& s, int& len) {
  s = __builtin_ctzll(m);
  const u64 inv = ~(m >> s);
  len = inv ? __builtin_ctzll(inv) : 64;
  len = min(len, 64 - s);
  m &= ~((len >= 64 ? ~0ull : ((1ull << len) - 1ull)) << s);
}

// Tile CCL.  Labels are SPARSE (one per Q0 cell of the tile, addressed through the tile-local prefix of the
// per-segment popcounts), so a tile costs the same LDS whatever nz is.  The unit of work is the z-RUN: the cells
// of a run share a label from the start, a run looks at each of the four lower z-lines through one 34-bit window
// and joins every run it finds there -- a wall costs one union per line, not one per cell.
template <int NT>
__global__ void __launch_bounds__(NT) k_tile_ccl(Geo g, FArgs F, const FVar V) {
  // the chain's first kernel: the per-search arguments arrive as a KERNEL ARGUMENT (the graph node's parameters are
  // rewritten before every launch: no memory read -- least of all one over PCIe -- stands in front of the tile's
  // loads); workgroup 0 leaves the device copy the later kernels read
  if (blockIdx.x == 0 && threadIdx.x == 0) *F.var_w = V;
  if ((int)blockIdx.x >= V.ntiles_f) return;
  const TileGeo T = tile_geo(g, V, blockIdx.x);
  const Box3 sbox = V.sbox;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int nz = g.nz, nseg = T.nseg, items = T.items, TY = T.TY;
  u32* lab = reinterpret_cast<u32*>(smem_raw);       // [FR_TCELL] union-find over the tile-local cell indices
  u32* segb = lab + FR_TCELL;                         // [items] Q0 bits of each 32-voxel segment
  u32* segpre = segb + items;                         // [items + 1]
  u32* acc = segpre + items + 1;                      // [FR_TROOT][8]: sy, sz, claim, ly, lz, hy, hz, -
  u32* rrow = acc + FR_TROOT * 8;                     // [FR_TROOT][FR_TXS] cells per x-row
  unsigned short* rootno = reinterpret_cast<unsigned short*>(rrow + FR_TROOT * FR_TXS);  // [FR_TCELL] at a root: its number
  unsigned char* rcell = reinterpret_cast<unsigned char*>(rootno + FR_TCELL);            // [FR_TCELL] component number per cell
  u32* segs = reinterpret_cast<u32*>(rcell + FR_TCELL);  // [items] NQ seed bits (on their way to the ts array)
  u32* plist = reinterpret_cast<u32*>(rootno);  // [FR_TPAIR] touching runs (cell << 16 | cell); shares the space of rootno + rcell, which are filled afterwards
  unsigned short* cseg = reinterpret_cast<unsigned short*>(acc);  // [FR_TCELL] segment of every cell, for the pair walk; shares the space of acc + rrow, which are initialised behind it
  static_assert((size_t)FR_TCELL * sizeof(unsigned short) <= (size_t)FR_TROOT * 8 * 4 + (size_t)FR_TROOT * FR_TXS * 4, "cell -> segment table does not fit");
  static_assert((size_t)FR_TPAIR * sizeof(u32) <= FR_TCELL * sizeof(unsigned short) + FR_TCELL, "pair list does not fit");
  __shared__ u32 s_wsum[NT / 64];
  __shared__ u32 s_nroots, s_base, s_flag;
  __shared__ u32 s_cnt[4];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x == 0) s_nroots = 0u, s_flag = 0u, s_cnt[0] = s_cnt[1] = s_cnt[2] = s_cnt[3] = 0u;
  FR_DBG_MARK(F, blockIdx.x, 0);
  const u32 total = tile_load_pred<NT>(g, T, V, F, segb, segpre, s_wsum, lab, segs, cseg);  // (uniform; predicate, prefix, labels)
  {  // the bit arrays of the tile, for the later kernels and the neighbours (in flight during the phases below)
    u32* tq = F.tq + (size_t)blockIdx.x * items;
    u32* ts = F.ts + (size_t)blockIdx.x * items;
    for (int it = threadIdx.x; it < items; it += NT) tq[it] = segb[it], ts[it] = segs[it];
  }
  FR_DBG_MARK(F, blockIdx.x, 1);
  if (total == 0u || total > FR_TCELL) {
    if (threadIdx.x == 0) {
      F.t_nroots[blockIdx.x] = 0u;
      F.t_base[blockIdx.x] = 0u;
      if (total > FR_TCELL) F.fctr[FCTR(9)] = 11u;  // (codes 11..17 name the capacity for FUELMI_FR_TIMING / debugging)
    }
    return;
  }
  FR_DBG_MARK(F, blockIdx.x, 2);
  // ---- components.  (1) One lane per CELL looks at the four lower z-lines around it through 3-bit windows of the LDS
  // bit arrays (walk_pairs below): every pair of touching runs (segment seams included) goes into an LDS list, a
  // cell's pairs collected in registers first (one list reservation per wave and trip).
  // (2) The list is then joined by HOOK + COMPRESS rounds (Shiloach-Vishkin style): both labels of a pair are read
  // side by side and the larger root takes the smaller with a non-returning atomicMin, then every cell walks to its
  // root; repeated until a round finds every pair joined.  Labels only ever decrease and parent < child always
  // holds, so there are no cycles; a hook that lost a race is simply repeated in the next round.
  // Why not a lock-free union-find inside the walk (rounds 2 and 3 tried it three ways): merging hundreds of runs
  // into one surface makes every lane retry against the same growing tree -- measured 7 us for one union per lane --
  // and the retry loops run under the divergence of the walk. ----
  __shared__ u32 s_np, s_chg, s_povf;
  if (threadIdx.x == 0) s_np = 0u, s_chg = 0u, s_povf = 0u;
  __syncthreads();
  auto walk_pairs = [&](auto&& fn) {  // fn(first cell of an own run, a cell of a touching run of a lower line / the seam)
    // One lane per CELL: its segment from the cell -> segment table, its bit inside the segment, then one 3-bit window
    // (z - 1, z, z + 1) per lower line.  A cell whose z-predecessor is a cell too (same run) shares that cell's
    // windows except for the voxel z + 1 of each lower line -- and that one only matters when it starts a new run
    // there (the line's voxel z is empty): a wall costs one look per cell and line, not one pair.
    for (u32 l = threadIdx.x; l < total; l += NT) {
      const int it = cseg[l];  // (written beside the labels: a bisection of the prefix here was 11 dependent LDS reads)
      const u32 bits = segb[it];
      u32 k = l - segpre[it], rem = bits;  // the k-th set bit
      while (k--) rem &= rem - 1u;
      const int zz = __builtin_ctz(rem);
      const int line = it / nseg, c = it - line * nseg, lx = line / TY, ly = line - lx * TY;
      const int z = 32 * c + zz;
      const bool seam = zz == 0 && c > 0 && (segb[it - 1] >> 31);
      const u32 own = seam ? l : lab[l];  // label node of the cell's run (its first cell inside the segment)
      // the cell's pairs are collected in registers (slot 0: the seam, slots 1 + 2 q, 2 + 2 q: lower line q) and handed
      // over together behind the loop, where the wave has reconverged: one list reservation per wave and trip instead
      // of one per (cell, line) among whatever lanes happened to sit in the same iteration
      u32 pk[9];
      u32 nv = 0u;
      pk[0] = (l << 16) | (l - 1u);
      if (seam) nv |= 1u;
      const bool has_prev = seam || (zz > 0 && ((bits >> (zz - 1)) & 1u));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        pk[1 + 2 * q] = pk[2 + 2 * q] = 0u;
        const int nlx = lx + (q < 3 ? -1 : 0), nly = ly + (q < 3 ? q - 1 : -1);
        if (nlx < 0 || nly < 0 || nly >= TY) continue;
        const int nline = nlx * TY + nly;
        const int zlo = z - 1;
        const int s0 = max(zlo, 0) >> 5;
        const u64 w = (u64)segb[nline * nseg + s0] | ((s0 + 1 < nseg) ? ((u64)segb[nline * nseg + s0 + 1] << 32) : 0ull);
        u32 pat = (zlo >= 0) ? (u32)((w >> (zlo - 32 * s0)) & 7ull) : (u32)((w << 1) & 6ull);
        if (z + 1 >= nz) pat &= 3u;
        if (has_prev) pat = (pat & 6u) == 4u ? 4u : 0u;
        if (!pat) continue;
        const int zn = zlo + __builtin_ctz(pat);
        const int nit = nline * nseg + (zn >> 5);
        const u32 ln = segpre[nit] + (u32)__popc(segb[nit] & ((1u << (zn & 31)) - 1u));
        pk[1 + 2 * q] = (own << 16) | ln;
        nv |= 1u << (1 + 2 * q);
        if (pat == 5u) {  // the next cell of that line sits at zlo + 2
          pk[2 + 2 * q] = (own << 16) | (ln + 1u);
          nv |= 1u << (2 + 2 * q);
        }
      }
      fn(pk, nv);
    }
  };
  walk_pairs([&](const u32 (&pk)[9], u32 nv) {
    // (all lanes of the trip arrive here together) positions by a ballot scan of the pair counts, one reservation
    const u32 cnt = (u32)__popc(nv);
    u32 excl = 0u, tot = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) {  // cnt <= 9
      const unsigned long long bal = __ballot((cnt >> b) & 1u);
      excl += (u32)__builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u)) << b;
      tot += (u32)__popcll(bal) << b;
    }
    if (tot == 0u) return;  // (uniform)
    const int leader = __builtin_ctzll(__ballot(1));
    u32 at = 0u;
    if (lane == leader) at = atomicAdd(&s_np, tot);
    at = (u32)__shfl((int)at, leader, 64) + excl;
#pragma unroll
    for (int k = 0; k < 9; ++k)
      if ((nv >> k) & 1u) {
        if (at < FR_TPAIR)
          plist[at] = pk[k];
        else
          s_povf = 1u;
        ++at;
      }
  });
  __syncthreads();
  {
    volatile u32* vl = lab;
    const u32 np = min(s_np, (u32)FR_TPAIR);
    for (;;) {
      bool any = false;
      for (u32 p = threadIdx.x; p < np; p += NT) {
        const u32 pr = plist[p];
        const u32 ru = vl[pr >> 16], rv = vl[pr & 0xFFFFu];  // (roots: the labels are flat at the start of a round)
        if (ru != rv) {
          atomicMin(&lab[max(ru, rv)], min(ru, rv));
          any = true;
        }
      }
      if (any) s_chg = 1u;
      __syncthreads();
      const bool again = s_chg != 0u;
      __syncthreads();
      if (!again) break;
      if (threadIdx.x == 0) s_chg = 0u;
      for (u32 i = threadIdx.x; i < total; i += NT) {
        u32 r = vl[i];
        for (;;) {
          const u32 rr = vl[r];
          if (rr == r) break;
          r = rr;
        }
        vl[i] = r;
      }
      __syncthreads();
    }
  }
  if (s_povf) {  // more touching pairs than the list holds (a tile of single-voxel runs): the plain union-find walk
    walk_pairs([&](const u32 (&pk)[9], u32 nv) {
#pragma unroll
      for (int k = 0; k < 9; ++k)
        if ((nv >> k) & 1u) lds_union_h(lab, pk[k] >> 16, pk[k] & 0xFFFFu);
    });
  }
  __syncthreads();
  // (the cell -> segment table is dead: its space becomes the accumulators of the record phase, two barriers ahead)
  for (int t = threadIdx.x; t < FR_TROOT * 8; t += NT) {
    const int k = t & 7;
    acc[t] = (k >= 2 && k <= 4) ? 0xFFFFFFFFu : 0u;  // claim / box minima start at +inf
  }
  for (int t = threadIdx.x; t < FR_TROOT * FR_TXS; t += NT) rrow[t] = 0u;
  FR_DBG_MARK(F, blockIdx.x, 3);
  // ---- roots: dense numbers ----
  for (u32 l = threadIdx.x; l < total; l += NT)
    if (lab[l] == l) {
      const u32 la = atomicAdd(&s_nroots, 1u);
      rootno[l] = (unsigned short)min(la, 0xFFFFu);
    }
  __syncthreads();
  const u32 nroots = s_nroots;
  if (nroots > FR_TROOT) {
    if (threadIdx.x == 0) {
      F.fctr[FCTR(9)] = 12u;
      F.t_nroots[blockIdx.x] = 0u;
      F.t_base[blockIdx.x] = 0u;
    }
    return;
  }
  // ---- ids of the components: one contiguous range per tile inside the XCD's part of the id space (the
  // returning atomic is issued here so that its latency hides behind the record loop) ----
  if (threadIdx.x == 0) {
    const u32 xcd = blockIdx.x & 7u;
    const u32 b = atomicAdd(&F.fctr[FCTR(xcd)], nroots);
    if (b + nroots > FR_RC8) {
      F.fctr[FCTR(9)] = 13u;
      s_flag = 1u;
    }
    s_base = xcd * FR_RC8 + b;
  }
  // ---- component number of every cell ----
  for (u32 l = threadIdx.x; l < total; l += NT) rcell[l] = (unsigned char)rootno[lds_find_h(lab, l)];
  __syncthreads();
  FR_DBG_MARK(F, blockIdx.x, 4);
  // ---- per-component records.  One lane per z-LINE adds up its runs in registers (a line's cells nearly always
  // belong to one component); a wave whose lanes all hold the same component reduces across the lanes first. ----
  for (int line0 = 0; line0 < T.TX * TY; line0 += NT) {  // (uniform trip count: the wave reduces below)
    const int line = line0 + threadIdx.x;
    const bool act = line < T.TX * TY;
    const int lx = line / TY, ly = line - lx * TY;
    const u32 x = (u32)(T.x0 + lx), y = (u32)(T.y0 + ly);
    const bool xy_in = (int)x >= sbox.lo[0] && (int)x <= sbox.hi[0] && (int)y >= sbox.lo[1] && (int)y <= sbox.hi[1];
    const long la = (long)x * g.nyz + (long)y * nz;
    u32 key = 0xFFFFFFFFu, n = 0u, sz = 0u, cl = 0xFFFFFFFFu, lz = 0xFFFFFFFFu, hz = 0u;
    auto flush = [&]() {  // direct LDS atomics (the slow path: a second component on the line)
      u32* r = acc + key * 8u;
      atomicAdd(&r[0], n * y), atomicAdd(&r[1], sz), atomicMin(&r[2], cl), atomicMin(&r[3], y), atomicMin(&r[4], lz);
      atomicMax(&r[5], y), atomicMax(&r[6], hz);
      atomicAdd(&rrow[key * FR_TXS + (u32)lx], n);
    };
    for (int c = 0; act && c < nseg; ++c) {
      const int it = line * nseg + c;
      u32 rem = segb[it];
      u32 l = segpre[it];
      while (rem) {
        int s, len;
        pop_run32(rem, s, len);
        const u32 k2 = (u32)rcell[l];
        if (k2 != key) {
          if (key != 0xFFFFFFFFu) flush();
          key = k2, n = 0u, sz = 0u, cl = 0xFFFFFFFFu, lz = 0xFFFFFFFFu, hz = 0u;
        }
        const u32 z0 = (u32)(32 * c + s), z1 = z0 + (u32)len - 1u;
        n += (u32)len;
        sz += (u32)len * z0 + (u32)(len * (len - 1) / 2);
        lz = min(lz, z0), hz = max(hz, z1);
        if (xy_in) {
          const int zc = max((int)z0, sbox.lo[2]);
          if (zc <= min((int)z1, sbox.hi[2])) cl = min(cl, (u32)(la + zc));
        }
        l += (u32)len;
      }
    }
    // the last (usually only) component of the line: wave-uniform -> one set of atomics per wave
    const bool have = key != 0xFFFFFFFFu;
    const u64 hm = __ballot(have);
    if (hm) {
      const u32 first = (u32)__shfl((int)key, __builtin_ctzll(hm), 64);
      const bool uni = __ballot(have && key != first) == 0ull;
      if (uni) {
        u32 sy = have ? n * y : 0u, s2 = have ? sz : 0u, c2 = have ? cl : 0xFFFFFFFFu;
        u32 ly2 = have ? y : 0xFFFFFFFFu, lz2 = have ? lz : 0xFFFFFFFFu, hy2 = have ? y : 0u, hz2 = have ? hz : 0u;
        sy = wave_add_u32(sy), s2 = wave_add_u32(s2), c2 = wave_min_u32(c2), ly2 = wave_min_u32(ly2);
        lz2 = wave_min_u32(lz2), hy2 = wave_max_u32(hy2), hz2 = wave_max_u32(hz2);
        if (lane == __builtin_ctzll(hm)) {
          u32* r = acc + first * 8u;
          atomicAdd(&r[0], sy), atomicAdd(&r[1], s2), atomicMin(&r[2], c2), atomicMin(&r[3], ly2), atomicMin(&r[4], lz2);
          atomicMax(&r[5], hy2), atomicMax(&r[6], hz2);
        }
        if (have) atomicAdd(&rrow[key * FR_TXS + (u32)lx], n);
      } else if (have)
        flush();
    }
  }
  __syncthreads();
  FR_DBG_MARK(F, blockIdx.x, 5);
  const u32 gbase = s_base;
  if (threadIdx.x == 0) {
    F.t_base[blockIdx.x] = gbase;
    F.t_nroots[blockIdx.x] = s_flag ? 0u : nroots;
  }
  if (s_flag) return;
  if (threadIdx.x < nroots) {
    const u32* r = acc + threadIdx.x * 8;
    const u32* rw = rrow + threadIdx.x * FR_TXS;
    TRec R;
    u32 size = 0u, sx = 0u, lox = 0xFFFFFFFFu, hix = 0u;
    unsigned short* grow = F.rrow + (size_t)(gbase + threadIdx.x) * FR_TXS;
    for (int lx = 0; lx < FR_TXS; ++lx) {
      const u32 cnt = lx < T.TX ? rw[lx] : 0u;
      grow[lx] = (unsigned short)cnt;  // (<= TY * nz <= 32 * 256 cells)
      if (cnt) {
        size += cnt, sx += cnt * (u32)(T.x0 + lx);
        lox = min(lox, (u32)(T.x0 + lx)), hix = max(hix, (u32)(T.x0 + lx));
      }
    }
    R.size = size, R.sx = sx, R.sy = r[0], R.sz = r[1];
    R.lo[0] = lox, R.lo[1] = r[3], R.lo[2] = r[4], R.hi[0] = hix, R.hi[1] = r[5], R.hi[2] = r[6];
    R.tx = (u32)T.tx, R.own = r[2];
    F.trec[gbase + threadIdx.x] = R;
    F.tclaim[gbase + threadIdx.x] = r[2];
  }
  // ---- component number of every cell, by tile-local index (k_tile_out) and by voxel address (k_tile_cross) ----
  {
    unsigned char* tl = F.tlab + (size_t)blockIdx.x * FR_TCELL;
    for (u32 l = threadIdx.x; l < total; l += NT) tl[l] = rcell[l];
  }
  for (int it = threadIdx.x; it < items; it += NT) {
    u32 rem = segb[it];
    if (!rem) continue;
    const int line = it / nseg, c = it - line * nseg;
    unsigned char* vl = F.vlab + tile_line_adr(g, T, line) + 32 * c;
    u32 l = segpre[it];
    while (rem) {
      const int b = __builtin_ctz(rem);
      rem &= rem - 1u;
      vl[b] = rcell[l++];
    }
  }
  FR_DBG_MARK(F, blockIdx.x, 6);
  if (F.dbg && threadIdx.x == 0) {
    F.dbg[(size_t)blockIdx.x * FR_DBG_SLOTS + 8] = total;
    F.dbg[(size_t)blockIdx.x * FR_DBG_SLOTS + 9] = s_cnt[0];
    F.dbg[(size_t)blockIdx.x * FR_DBG_SLOTS + 10] = s_cnt[1];
    F.dbg[(size_t)blockIdx.x * FR_DBG_SLOTS + 11] = s_cnt[2];
    F.dbg[(size_t)blockIdx.x * FR_DBG_SLOTS + 12] = nroots;
  }
}

// Joins across tile faces + seed claims, one launch after k_tile_ccl (every cell's component number is in vlab by
// now).  The runs of the tile's lower-face lines look across the face through the same 34-bit windows as inside
// the tile; the relation is recorded as a pair of TILE ROOTS, and a tile keeps one record per distinct pair (LDS
// set: a surface crossing a face gives the same pair from all of its cells) -- a few thousand records per search.
// The tile's NQ seeds claim the tile roots touching their 26-neighbourhood (atomicMin on tclaim).
#define XC_SET 256
#define XC_WCAP 6144  // entries of a tile's work list (beyond: processed on the spot)
template <int RS_T, bool IN_LAUNCH>
__device__ __forceinline__ bool resolve_body(const Geo& g, const FArgs& F, const FVar& V, unsigned char* smem_raw, const u32 rcap);

__device__ __forceinline__ void xc_insert(u32* s_set, u32* s_list, u32* s_n, u32* fctr, u32 key) {
  u32 h = (key * 2654435761u) >> 24;
  bool done = false;
  for (int probe = 0; probe < XC_SET && !done; ++probe) {
    const u32 old = atomicCAS(&s_set[h], 0xFFFFFFFFu, key);
    if (old == 0xFFFFFFFFu) {
      s_list[atomicAdd(s_n, 1u)] = key;
      done = true;
    } else if (old == key)
      done = true;
    h = (h + 1u) & (XC_SET - 1u);
  }
  if (!done) st_agent(&fctr[FCTR(9)], 15u);  // more than XC_SET distinct root pairs around one tile
}
// rcap != 0 (round 6): the workgroup that finishes LAST joins the tile roots itself (resolve_body, in the LDS its tile no
// longer needs) -- k_resolve's launch and kernel boundary leave the search's critical path.  What it reads of the
// other workgroups of this launch (pairs, claims, overflow codes) was written with agent-scope stores / memory-side
// atomics and is counted in behind s_waitcnt vmcnt(0): no release fence, no L2 write-back.  rcap = tile roots that fit
// the launch's LDS; searches with more leave the job to the kernel k_resolve behind (which returns at once otherwise).
template <int NT>
__global__ void __launch_bounds__(NT) k_tile_cross(Geo g, FArgs F, const u32 rcap) {
  FR_DBG_MARK(F, blockIdx.x, 13);  // (before the first load)
  __shared__ TilePro s_pro;
  stage_tile_pro(F, &s_pro);
  const FVar& V = s_pro.V;
  if ((int)blockIdx.x >= V.ntiles_f) return;
  // (no look at the chain's overflow word here: it shares a cache line with the counters k_tile_ccl just hit with
  // atomics, and thousands of waves waiting for that line cost more than the kernel.  After an overflow the
  // component numbers of some tile are stale: ids stay inside the padded tables, k_resolve discards everything.)
  const TileGeo T = tile_geo(g, V, blockIdx.x);
  const int nz = g.nz, nseg = T.nseg, TY = T.TY;
  const int lane = threadIdx.x & 63;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  u32* segq = reinterpret_cast<u32*>(smem_raw);  // [items] Q0 bits of the tile
  u32* segs = segq + T.items;                    // [items] NQ seed bits
  // work list: (own segment, neighbour line) combinations that have something to look up -- built from LDS only,
  // so that the global loads behind them (neighbour window, then component numbers) go out together.  An entry is
  // the item's number: face item fs * 4 + k, or seed item 0x80000000 | it * 9 + l.
  u32* wl = segs + T.items;                      // [XC_WCAP]
  __shared__ u32 s_set[XC_SET];   // distinct (root, root) pairs of this tile: open addressing
  __shared__ u32 s_list[XC_SET];  // ... in insertion order
  __shared__ u32 s_n, s_base, s_nw;
  __shared__ u32 s_tb[9];         // component-id base of the 3 x 3 tiles around this one
  const int dblk = V.ntiles_f + 1 + (int)blockIdx.x;
  FR_DBG_MARK(F, dblk, 0);
  u32 tb9;  // id base of one of the 3 x 3 tiles around this one (in flight beside the tile's arrays)
  {
    const int t9 = (int)threadIdx.x % 9, dtx = t9 / 3 - 1, dty = t9 % 3 - 1;
    const int ntx = T.tx + dtx, nty = T.ty + dty;
    const bool ok = ntx >= 0 && ntx < V.ntx_f && nty >= 0 && nty < V.nty_f;
    tb9 = F.t_base[ok ? ntx * V.nty_f + nty : (int)blockIdx.x];
    if (!ok) tb9 = 0u;
  }
  if (threadIdx.x < XC_SET) s_set[threadIdx.x] = 0xFFFFFFFFu;
  if (threadIdx.x == 0) s_n = 0u, s_nw = 0u;
  tile_load_arrays<NT, false>(T, F, segq, nullptr, nullptr, segs);
  if (threadIdx.x < 9) s_tb[threadIdx.x] = tb9;  // (read behind the barrier that ends the work-list phase)
  FR_DBG_MARK(F, dblk, 1);
  auto tile_of = [&](int x, int y) -> u32 {  // which of the 3 x 3 tiles holds column (x, y)
    const int dtx = x < T.x0 ? -1 : (x >= T.x0 + T.TX ? 1 : 0), dty = y < T.y0 ? -1 : (y >= T.y0 + TY ? 1 : 0);
    return (u32)((dtx + 1) * 3 + dty + 1);
  };
  // one item: the neighbour window w3 (bit j <-> z = 32 c - 1 + j of the neighbour line) against the own bits
  u32 k0 = 0xFFFFFFFFu, k1 = 0xFFFFFFFFu;  // up to two distinct pairs wait for the wave-level de-duplication
  auto do_item = [&](u32 bits, u32 own, int nb, u32 info, u64 w3) {
    const int c = (int)(info & 0xFFu);
    const u32 tb = s_tb[(info >> 8) & 0xFFu];
    w3 &= (1ull << 34) - 1ull;
    if (c == 0) w3 &= ~1ull;
    const int jend = nz - 32 * c + 1;  // bit position of z = nz
    if (jend < 34) w3 &= (1ull << jend) - 1ull;
    if (info >> 16) {
      // seeds: a component touching the segment's seeds is claimed by the lowest seed next to one of its cells
      while (w3) {
        int j, rl;
        pop_run64(w3, j, rl);
        const int b0 = max(j - 2, 0), b1 = min(j + rl - 1, 31);  // seeds at bits j - 2 .. j + rl - 1 touch the run
        if (b0 > b1) continue;
        const u32 m = bits & (((b1 - b0 + 1 >= 32) ? 0xFFFFFFFFu : ((1u << (b1 - b0 + 1)) - 1u)) << b0);
        if (!m) continue;
        const u32 r = tb + (u32)F.vlab[(long)nb + j];
        atomicMin(&F.tclaim[r], own + (u32)__builtin_ctz(m));
      }
      return;
    }
    u32 rem = bits;
    while (rem && w3) {
      int s, len;
      pop_run32(rem, s, len);
      u64 m = (w3 >> s) & ((1ull << (len + 2)) - 1ull);
      if (!m) continue;
      const u32 ga = s_tb[4] + (u32)F.vlab[(long)own + s];
      while (m) {
        int j, rl;
        pop_run64(m, j, rl);
        const u32 gb = tb + (u32)F.vlab[(long)nb + s + j];
        if (gb == ga) continue;
        const u32 key = (min(ga, gb) << 16) | max(ga, gb);
        if (key == k0 || key == k1) continue;
        if (k0 == 0xFFFFFFFFu)
          k0 = key;
        else if (k1 == 0xFFFFFFFFu)
          k1 = key;
        else
          xc_insert(s_set, s_list, &s_n, F.fctr, key);  // (a third distinct pair from one lane: rare)
      }
    }
  };
  auto flush_pairs = [&]() {  // (all lanes of the wave)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const u32 kq = q ? k1 : k0;
      const bool on = kq != 0xFFFFFFFFu;
      u64 todo = __ballot(on);
      while (todo) {  // one insertion per distinct pair of the wave
        const int leader = __builtin_ctzll(todo);
        const u32 key = (u32)__shfl((int)kq, leader, 64);
        todo &= ~__ballot(on && kq == key);
        if (lane == leader) xc_insert(s_set, s_list, &s_n, F.fctr, key);
      }
    }
    k0 = k1 = 0xFFFFFFFFu;
  };
  // what an entry stands for: own bits, address of the own segment, address of the neighbour window, info word
  auto decode = [&](u32 e, u32& bits, u32& own, int& nb, u32& info, int& xx, int& yy) {
    int it, c;
    if (e >> 31) {
      const int sj = (int)(e & 0x7FFFFFFFu), l = sj % 9;
      it = sj / 9;
      const int line = it / nseg, lx = line / TY, ly = line - lx * TY;
      c = it - line * nseg;
      xx = T.x0 + lx + l / 3 - 1, yy = T.y0 + ly + l % 3 - 1;
      bits = (xx >= V.px0 && xx <= V.px1 && yy >= V.py0 && yy <= V.py1) ? segs[it] : 0u;  // (no Q0 cells outside the tiles)
      own = (u32)((long)(T.x0 + lx) * g.nyz + (long)(T.y0 + ly) * nz + 32 * c);
      info = (u32)c | (tile_of(xx, yy) << 8) | (1u << 16);
    } else {
      const int k = (int)(e & 3u), fs = (int)(e >> 2), fl = fs / nseg;
      c = fs - fl * nseg;
      int lx = 0, ly = fl;
      if (fl >= TY) lx = 1 + ((fl - TY) >> 1), ly = ((fl - TY) & 1) ? TY - 1 : 0;
      xx = T.x0 + lx + (k < 3 ? -1 : 0), yy = T.y0 + ly + (k < 3 ? k - 1 : -1);
      bits = segq[(lx * TY + ly) * nseg + c];
      own = (u32)((long)(T.x0 + lx) * g.nyz + (long)(T.y0 + ly) * nz + 32 * c);
      info = (u32)c | (tile_of(xx, yy) << 8);
    }
    nb = (int)((long)xx * g.nyz + (long)yy * nz + 32 * c - 1);
  };
  // ---- tile faces: the whole x-row 0 and, in the other x-rows, the lines ly = 0 and ly = TY - 1; an item per
  // (face line, segment, lower z-line across the face) ----
  const int nfl = TY + 2 * (T.nxl - 1);
  const int fitems = nfl * nseg * 4;
  for (int fi = threadIdx.x; fi < fitems; fi += NT) {
    const int k = fi & 3, fs = fi >> 2, fl = fs / nseg, c = fs - fl * nseg;
    int lx = 0, ly = fl;
    if (fl >= TY) lx = 1 + ((fl - TY) >> 1), ly = ((fl - TY) & 1) ? TY - 1 : 0;
    if (!segq[(lx * TY + ly) * nseg + c]) continue;
    const int kdx = k < 3 ? -1 : 0, kdy = k < 3 ? k - 1 : -1;
    const int xx = T.x0 + lx + kdx, yy = T.y0 + ly + kdy;
    const bool cross = (kdx < 0 && lx == 0) || (kdy < 0 && ly == 0) || (kdy > 0 && ly == TY - 1);
    if (!(cross && ly < T.nyl && xx >= V.px0 && yy >= V.py0 && yy <= V.py1)) continue;
    const u32 slot = atomicAdd(&s_nw, 1u);
    if (slot < XC_WCAP)
      wl[slot] = (u32)fi;
    else
      st_agent(&F.fctr[FCTR(9)], 18u);  // work list full (a tile made of seeds): the legacy chain takes the search
  }
  // ---- NQ seeds of the tile (most tiles have none): nine items per seed segment, one per line around it (one
  // reservation for all nine) ----
  for (int it = threadIdx.x; it < T.items; it += NT) {
    if (!segs[it]) continue;
    const u32 slot0 = atomicAdd(&s_nw, 9u);
    for (int l = 0; l < 9; ++l) {
      const u32 e = 0x80000000u | (u32)(it * 9 + l);
      if (slot0 + (u32)l < XC_WCAP)
        wl[slot0 + (u32)l] = e;
      else
        st_agent(&F.fctr[FCTR(9)], 18u);
    }
  }
  __syncthreads();
  FR_DBG_MARK(F, dblk, 2);
  // ---- the list: two items per lane and trip, their windows fetched together ----
  const u32 nw = min(s_nw, (u32)XC_WCAP);
  for (u32 w0 = 0; w0 < nw; w0 += 2 * NT) {
    u32 b0 = 0u, b1 = 0u, o0 = 0u, o1 = 0u, i0 = 0u, i1 = 0u;
    int n0 = 0, n1 = 0, xa = 0, ya = 0, xb = 0, yb = 0;
    u64 wa = 0ull, wb = 0ull;
    const u32 ja = w0 + threadIdx.x, jb = ja + NT;
    if (ja < nw) decode(wl[ja], b0, o0, n0, i0, xa, ya);
    if (jb < nw) decode(wl[jb], b1, o1, n1, i1, xb, yb);
    // (both windows unconditionally -- an idle slot looks at column (0, 0), outside the rectangle or not -- so that
    // the six loads go out together)
    wa = q_window34(g, V, F, xa, ya, (int)(i0 & 0xFFu));
    wb = q_window34(g, V, F, xb, yb, (int)(i1 & 0xFFu));
    if (!b0) wa = 0ull;
    if (!b1) wb = 0ull;
#pragma nounroll
    for (int h = 0; h < 2; ++h) {  // (one copy of the item code)
      const u32 bb = h ? b1 : b0;
      const u64 ww = h ? wb : wa;
      if (bb && ww) do_item(bb, h ? o1 : o0, h ? n1 : n0, h ? i1 : i0, ww);
      flush_pairs();
    }
  }
  __syncthreads();
  FR_DBG_MARK(F, dblk, 3);
  const u32 n = s_n;
  if (n != 0u) {  // (uniform)
    const u32 xcd = blockIdx.x & 7u;
    if (threadIdx.x == 0) s_base = atomicAdd(&F.fctr[FCTR(16 + xcd)], n);
    __syncthreads();
    const u32 base = s_base;
    if (base + n > FR_PCAP / 8u) {
      if (threadIdx.x == 0) st_agent(&F.fctr[FCTR(9)], 14u);
    } else if (threadIdx.x < n)
      st_agent(&F.pairs[(size_t)xcd * (FR_PCAP / 8u) + base + threadIdx.x], s_list[threadIdx.x]);
  }
  FR_DBG_MARK(F, dblk, 4);
  if constexpr (NT == 512) {
    if (rcap == 0u) return;
    // ---- last one out joins the roots ----
    __shared__ u32 s_last;
    wait_vm_stores();  // (every wave: its pairs and codes have left)
    __syncthreads();
    // (the counter has a cache line of its own: on the line of the pair-list counters its 576 returning atomics stood in
    // front of every tile's list reservation -- the busiest tile's cross phase 13 -> 19 us)
    // two levels: the workgroups of an XCD (blockIdx & 7) count into that XCD's word, the last of each into the global one:
    // 72 + 8 returning atomics per line instead of 576 on one
    if (threadIdx.x == 0) {
      const u32 xcd = blockIdx.x & 7u, n_x = ((u32)V.ntiles_f + 7u - xcd) >> 3;  // workgroups b < ntiles_f with b & 7 == xcd
      u32 last = 0u;
      if (atomicAdd(&F.fctr[FR_DONE_CTR + FCTR(1 + xcd)], 1u) == n_x - 1u) {
        const u32 n_groups = min((u32)V.ntiles_f, 8u);
        last = atomicAdd(&F.fctr[FR_DONE_CTR], 1u) == n_groups - 1u ? 1u : 0u;
      }
      s_last = last;
    }
    __syncthreads();
    if (!s_last) return;
    const bool no_kr = (rcap >> 31) != 0u;  // no k_resolve is queued behind this launch (the host expected this search to fit)
    if (resolve_body<NT, true>(g, F, V, smem_raw, rcap & 0x7FFFFFFFu) || !no_kr) return;
    // more tile roots (or clusters) than this launch's LDS holds and nobody behind to do the job: tell the host (it queues k_resolve and
    // k_tile_out again and waits for the stamp a second time) and make the k_tile_out already queued return at once
    if (threadIdx.x == 0) {
      F.counts[2] = 3u;
      F.h_counts[2] = 3u;
      F.h_counts[6] = 20u;
      __hip_atomic_store(&F.h_counts[15], V.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// one wave-level reduction step of the per-component accumulators (sum / min / max over the lanes that share
// the leading key)
struct CAcc {
  u32 n, sx, sy, sz, cl, lx, ly, lz, hx, hy, hz;
};
__device__ __forceinline__ void cacc_reduce(CAcc& a) {
  a.n = wave_add_u32(a.n), a.sx = wave_add_u32(a.sx), a.sy = wave_add_u32(a.sy), a.sz = wave_add_u32(a.sz);
  a.cl = wave_min_u32(a.cl), a.lx = wave_min_u32(a.lx), a.ly = wave_min_u32(a.ly), a.lz = wave_min_u32(a.lz);
  a.hx = wave_max_u32(a.hx), a.hy = wave_max_u32(a.hy), a.hz = wave_max_u32(a.hz);
}

// Everything between "tile-local components" and "kept clusters in creation order", on the tile-root records,
// inside one workgroup: cross-tile union-find, sizes and claims per final component, clusters (a component
// claimed by one of its own cells is a cluster; components claimed by the same NQ seed form one with it), the
// kept list, its ranking by claimer address (= the reference's creation order), offsets of the grouped cell
// array, per-cluster index sums / boxes, the (cluster x tile column) prefix matrix k_tile_out places the cells
// with -- and the result records, written straight to pinned host memory.
#define RS_TK 1024  // lanes of the kernel k_resolve
#define RS_SH 512   // seed-claimed clusters (hash slots)
// bytes of LDS resolve_body needs for `rcap` tile roots
static inline size_t resolve_lds_bytes(size_t rcap) {
  return (4 * rcap + 6 * (size_t)FR_KCAP + 6 * (size_t)FR_KCAP + 3 * (size_t)RS_SH) * sizeof(u32) + 3 * (size_t)FR_KCAP * sizeof(unsigned long long);
}
// RS_T lanes of ONE workgroup; rcap = tile roots the LDS arrays hold (FR_RCAP in the kernel k_resolve; what the LDS of
// k_tile_cross holds when its last workgroup does the job).  IN_LAUNCH: pairs, claims and overflow codes were written
// by other workgroups of the SAME launch (agent-scope stores / memory-side atomics): they are read with agent-scope
// loads, past this XCD's L2 (the records are the previous kernel's and would be visible anyway; they take the same
// path).  Returns false when the search has more tile roots than rcap or (IN_LAUNCH) more (kept cluster x tile column)
// matrix entries than 2 rcap (nothing written: the kernel k_resolve, queued behind or by the host, does the work).
template <int RS_T, bool IN_LAUNCH>
__device__ __forceinline__ bool resolve_body(const Geo& g, const FArgs& F, const FVar& V, unsigned char* smem_raw, const u32 rcap) {
  auto ldw = [&](const u32* p) -> u32 { return IN_LAUNCH ? ld_agent(p) : *p; };
  u32* par = reinterpret_cast<u32*>(smem_raw);  // [rcap] union-find over the DENSE numbers of the tile roots
  u32* siz = par + rcap;                        // [rcap] cells of the final component (at its root); later the matrix
  u32* clm = siz + rcap;                        // [rcap] lowest claimer address (at its root); later the matrix
  u32* rko = clm + rcap;                        // [rcap] lowest OWN claimer (at its root), then: index into the kept list | FR_NOTKEPT | FR_UNCLAIMED
  u32* k_adr = rko + rcap;                      // [FR_KCAP] kept list: claimer address
  u32* k_slot = k_adr + FR_KCAP;                //   0: claimed by an own cell, 0xFFFFFFFF: by an NQ seed
  u32* k_size = k_slot + FR_KCAP;               //   cluster size (the seed counts)
  u32* k_nq = k_size + FR_KCAP;                 //   its Q0 cells
  u32* k_rank = k_nq + FR_KCAP;                 //   rank by claimer address
  u32* k_off = k_rank + FR_KCAP;                //   first position in the grouped cell array
  u32* kbox = k_off + FR_KCAP;                  // [FR_KCAP][6] index box per kept cluster (by kept index)
  u32* h_adr = kbox + FR_KCAP * 6;              // [RS_SH] seed hash: claimer address
  u32* h_sum = h_adr + RS_SH;                   //   cells of the components it claims
  u32* h_kept = h_sum + RS_SH;                  //   index into the kept list | FR_NOTKEPT
  unsigned long long* ksum = reinterpret_cast<unsigned long long*>(h_kept + RS_SH);  // [FR_KCAP][3] index sums
  u32* pmx = siz;                               // [nk][ntx] (2 rcap entries) once siz / clm are dead
  __shared__ u32 s_nk, s_ovf, s_nout, s_nq;
  __shared__ u32 s_fc[32];  // the chain's counters (one round trip for all of them)
  __shared__ u32 s_pre[9];  // dense number of the first tile root of every XCD range
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntx = V.ntx_f;
  if (threadIdx.x < 32) s_fc[threadIdx.x] = ldw(&F.fctr[FCTR(threadIdx.x)]);
  const int dblk = V.ntiles_f;  // time stamps of this kernel go behind those of the tiles
  FR_DBG_MARK(F, dblk, 0);
  __syncthreads();
  if (threadIdx.x == 0) {
    s_nk = 0u, s_ovf = s_fc[9], s_nout = 0u, s_nq = 0u;
    u32 run = 0u;
    for (int k = 0; k < 8; ++k) {
      s_pre[k] = run;
      run += min(s_fc[k], (u32)FR_RC8);
    }
    s_pre[8] = run;
  }
  __syncthreads();
  const bool dead = s_ovf != 0u;  // an earlier kernel hit a capacity limit: report, leave everything untouched
  const u32 R = s_pre[8];         // tile roots of this search
  if (!dead && R > rcap) return false;  // (uniform; IN_LAUNCH only: FR_RCAP holds every search that is not dead)
  // tile-root id (XCD range | index) <-> dense number
  auto dense_of = [&](u32 gidx) { return s_pre[gidx / FR_RC8] + (gidx & (FR_RC8 - 1u)); };
  auto gid_of = [&](u32 d) {
    u32 xc = 0u;
#pragma unroll
    for (int k = 1; k < 8; ++k) xc += d >= s_pre[k] ? 1u : 0u;
    return xc * FR_RC8 + (d - s_pre[xc]);
  };
  const u32 Rr = (R + RS_T - 1u) / RS_T * RS_T;
  // the pair lists, walked as one sequence; a lane's first three pairs are fetched beside the records
  u32 pp[9];
  pp[0] = 0u;
#pragma unroll
  for (int xc = 0; xc < 8; ++xc) pp[xc + 1] = pp[xc] + min(s_fc[16 + xc], FR_PCAP / 8u);
  auto pair_at = [&](u32 p) {
    u32 xc = 0u;
#pragma unroll
    for (int k = 1; k < 8; ++k) xc += p >= pp[k] ? 1u : 0u;
    return ldw(&F.pairs[(size_t)xc * (FR_PCAP / 8u) + (p - pp[xc])]);
  };
  u32 pk0 = 0u, pk1 = 0u, pk2 = 0u, pk3 = 0u;
  TRec T0, T1;  // records of tile roots d = threadIdx.x and d + RS_T (most searches have fewer than 2 RS_T roots: read once)
  T0.size = T1.size = 0u;
  auto load_rec = [&](u32 gi) -> TRec {
    TRec T;
    if (IN_LAUNCH)
      ld_agent_trec2(&F.trec[gi], &F.trec[gi], T, T);
    else
      T = F.trec[gi];
    return T;
  };
  if (!dead) {
    if (threadIdx.x < pp[8]) pk0 = pair_at(threadIdx.x);
    if (threadIdx.x + RS_T < pp[8]) pk1 = pair_at(threadIdx.x + RS_T);
    if (threadIdx.x + 2 * RS_T < pp[8]) pk2 = pair_at(threadIdx.x + 2 * RS_T);
    if (threadIdx.x + 3 * RS_T < pp[8]) pk3 = pair_at(threadIdx.x + 3 * RS_T);
    u32 nq_part = 0u;
    {  // the first two records of the lane side by side (one round trip)
      const u32 d0 = threadIdx.x, d1 = threadIdx.x + RS_T;
      const u32 g0 = gid_of(min(d0, R ? R - 1u : 0u)), g1 = gid_of(min(d1, R ? R - 1u : 0u));
      const u32 c0 = ldw(&F.tclaim[g0]), c1 = ldw(&F.tclaim[g1]);
      if (IN_LAUNCH)
        ld_agent_trec2(&F.trec[g0], &F.trec[g1], T0, T1);
      else
        T0 = F.trec[g0], T1 = F.trec[g1];
      if (d0 < R) par[d0] = d0, siz[d0] = T0.size, clm[d0] = c0, rko[d0] = T0.own, nq_part += T0.size;
      if (d1 < R) par[d1] = d1, siz[d1] = T1.size, clm[d1] = c1, rko[d1] = T1.own, nq_part += T1.size;
    }
    for (u32 d = threadIdx.x + 2 * RS_T; d < R; d += RS_T) {
      const u32 gi = gid_of(d);
      const TRec T = load_rec(gi);
      par[d] = d;
      siz[d] = T.size;
      clm[d] = ldw(&F.tclaim[gi]);
      rko[d] = T.own;
      nq_part += T.size;
    }
    nq_part = wave_add_u32(nq_part);
    if (lane == 0 && nq_part) atomicAdd(&s_nq, nq_part);
    for (u32 i = threadIdx.x; i < RS_SH; i += RS_T) h_adr[i] = NOCLAIM, h_sum[i] = 0u, h_kept[i] = FR_NOTKEPT;
    for (u32 i = threadIdx.x; i < FR_KCAP * 6; i += RS_T) kbox[i] = (i % 6u) < 3u ? 0xFFFFFFFFu : 0u;
    for (u32 i = threadIdx.x; i < FR_KCAP * 3; i += RS_T) ksum[i] = 0ull;
  }
  __syncthreads();
  FR_DBG_MARK(F, dblk, 1);
  if (!dead) {
    // ---- cross-tile unions (one list of distinct root pairs per XCD, walked as one sequence so that all
    // lanes are busy at once) ----
    if (threadIdx.x < pp[8]) lds_union_h(par, dense_of(pk0 >> 16), dense_of(pk0 & 0xFFFFu));
    if (threadIdx.x + RS_T < pp[8]) lds_union_h(par, dense_of(pk1 >> 16), dense_of(pk1 & 0xFFFFu));
    if (threadIdx.x + 2 * RS_T < pp[8]) lds_union_h(par, dense_of(pk2 >> 16), dense_of(pk2 & 0xFFFFu));
    if (threadIdx.x + 3 * RS_T < pp[8]) lds_union_h(par, dense_of(pk3 >> 16), dense_of(pk3 & 0xFFFFu));
    for (u32 p = threadIdx.x + 4 * RS_T; p < pp[8]; p += RS_T) {
      const u32 key = pair_at(p);
      lds_union_h(par, dense_of(key >> 16), dense_of(key & 0xFFFFu));
    }
  }
  __syncthreads();
  FR_DBG_MARK(F, dblk, 2);
  // ---- flatten; cells, lowest claimer and lowest own claimer of every final component (wave-reduced per
  // distinct root) ----
  if (!dead) {
    for (u32 d0 = 0; d0 < Rr; d0 += RS_T) {
      const u32 d = d0 + threadIdx.x;
      const u32 rt = d < R ? lds_find_h(par, d) : 0u;
      const bool mov = d < R && rt != d;
      const u32 sz = mov ? siz[d] : 0u, cl = mov ? clm[d] : NOCLAIM, ow = mov ? rko[d] : NOCLAIM;
      u64 todo = __ballot(mov);
      while (todo) {
        const int leader = __builtin_ctzll(todo);
        const u32 first = (u32)__shfl((int)rt, leader, 64);
        const bool mine = mov && rt == first;
        u32 s2 = mine ? sz : 0u, c2 = mine ? cl : NOCLAIM, o2 = mine ? ow : NOCLAIM;
        s2 = wave_add_u32(s2), c2 = wave_min_u32(c2), o2 = wave_min_u32(o2);
        if (lane == leader) {
          atomicAdd(&siz[first], s2);
          atomicMin(&clm[first], c2);
          atomicMin(&rko[first], o2);
        }
        todo &= ~__ballot(mine);
      }
    }
  }
  __syncthreads();
  FR_DBG_MARK(F, dblk, 3);
  if (!dead) {
    // (every find above ran before any sibling was re-parented by another thread's halving in a way that
    // matters: halving only ever installs ancestors; par[] is flat enough for the single look-ups below)
    // ---- clusters: own-claimed components straight to the kept list, seed-claimed ones through the hash.
    // A component is claimed by one of its own cells iff its lowest claimer IS its lowest own claimer (seeds and
    // Q0 cells are disjoint). ----
    for (u32 d = threadIdx.x; d < R; d += RS_T) {
      if (lds_find_h(par, d) != d) continue;
      const u32 cl = clm[d], ow = rko[d];
      if (cl == NOCLAIM) {
        rko[d] = FR_UNCLAIMED;
        continue;
      }
      if (cl == ow) {
        if ((int)siz[d] > F.cluster_min) {
          const u32 e = atomicAdd(&s_nk, 1u);
          if (e < FR_KCAP) {
            k_adr[e] = cl, k_slot[e] = 0u, k_size[e] = siz[d], k_nq[e] = siz[d];
            rko[d] = e;
          } else {
            s_ovf = 1u;
            rko[d] = FR_NOTKEPT;
          }
        } else
          rko[d] = FR_NOTKEPT;
      } else {
        u32 h = (cl * 2654435761u) >> 23;  // 9 bits
        bool done = false;
        for (int probe = 0; probe < RS_SH && !done; ++probe) {
          const u32 old = atomicCAS(&h_adr[h], NOCLAIM, cl);
          if (old == NOCLAIM || old == cl) {
            atomicAdd(&h_sum[h], siz[d]);
            rko[d] = 0x80000000u | h;  // resolved below
            done = true;
          }
          h = (h + 1u) & (RS_SH - 1u);
        }
        if (!done) {
          s_ovf = 1u;
          rko[d] = FR_NOTKEPT;
        }
      }
    }
  }
  __syncthreads();
  FR_DBG_MARK(F, dblk, 4);
  if (!dead && threadIdx.x < RS_SH && h_adr[threadIdx.x] != NOCLAIM) {
    const u32 cl = h_adr[threadIdx.x], sum = h_sum[threadIdx.x];
    if ((int)(sum + 1u) > F.cluster_min) {
      const u32 e = atomicAdd(&s_nk, 1u);
      if (e < FR_KCAP) {
        k_adr[e] = cl, k_slot[e] = 0xFFFFFFFFu, k_size[e] = sum + 1u, k_nq[e] = sum;
        h_kept[threadIdx.x] = e;
      } else
        s_ovf = 1u;
    }
  }
  __syncthreads();
  FR_DBG_MARK(F, dblk, 5);
  const u32 nk = min(s_nk, (u32)FR_KCAP);
  const u32 nq = s_nq;
  // (the matrix needs nk * ntx LDS words, 2 rcap of which fit.  In the launch, a search with more -- 43 clusters on a
  // full G400 box with its 48 tile columns -- is left to the kernel k_resolve like one with too many tile roots: only LDS
  // has been written so far, and nk comes from LDS behind a barrier (uniform).  k_resolve holds 2 FR_RCAP = FR_PMCAP
  // entries; beyond that -- hundreds of clusters on a huge map -- the legacy chain)
  if (IN_LAUNCH && !dead && s_ovf == 0u && (size_t)nk * (size_t)ntx > 2 * (size_t)rcap) return false;
  const bool bad =dead || s_ovf != 0u || (size_t)nk * (size_t)ntx > 2 * (size_t)rcap || ntx > F.pm_stride;
  if (!bad) {
    // ---- creation order = ascending claimer address; offsets of the grouped cell array ----
    if (threadIdx.x < nk) {
      const u32 ai = k_adr[threadIdx.x];
      u32 rank = 0u, off = 0u;
      for (u32 j = 0; j < nk; ++j)
        if (k_adr[j] < ai) {
          ++rank;
          off += k_nq[j];
        }
      k_rank[threadIdx.x] = rank;
      k_off[threadIdx.x] = off;
      atomicAdd(&s_nout, k_nq[threadIdx.x]);
    }
    // siz / clm are dead from here on: their space becomes the (rank, tile column) matrix
    for (u32 i = threadIdx.x; i < nk * (u32)ntx; i += RS_T) pmx[i] = 0u;
  }
  __syncthreads();
  FR_DBG_MARK(F, dblk, 6);
  if (!bad) {
    // ---- code of every tile root; index sums / boxes of the kept clusters; cells per (cluster, tile column) ----
    for (u32 d0 = 0; d0 < Rr; d0 += RS_T) {
      const u32 d = d0 + threadIdx.x;
      u32 e = FR_UNCLAIMED, gi = 0u;
      if (d < R) {
        gi = gid_of(d);
        e = rko[lds_find_h(par, d)];
        if (e != FR_UNCLAIMED && e != FR_NOTKEPT && (e & 0x80000000u)) e = h_kept[e & 0x7FFFFFFFu];
      }
      const bool kept = e < FR_KCAP;
      if (d < R) F.rcode[gi] = kept ? k_rank[e] : e;
      CAcc A;
      A.n = 0u, A.sx = A.sy = A.sz = 0u, A.cl = A.lx = A.ly = A.lz = 0xFFFFFFFFu, A.hx = A.hy = A.hz = 0u;
      if (kept) {
        const TRec T = d0 == 0u ? T0 : (d0 == (u32)RS_T ? T1 : load_rec(gi));
        A.sx = T.sx, A.sy = T.sy, A.sz = T.sz, A.lx = T.lo[0], A.ly = T.lo[1], A.lz = T.lo[2];
        A.hx = T.hi[0], A.hy = T.hi[1], A.hz = T.hi[2];
        atomicAdd(&pmx[k_rank[e] * (u32)ntx + T.tx], T.size);
      }
      // the cluster most of the wave's roots belong to (the giant surface) is reduced across the lanes; the few
      // roots of other clusters add themselves (distinct LDS words, no contention to speak of)
      const u64 km = __ballot(kept);
      if (km) {
        u32 first = (u32)__shfl((int)e, __builtin_ctzll(km), 64);
        {  // majority vote between the first two distinct clusters of the wave
          const u64 same = __ballot(kept && e == first);
          const u64 rest = km & ~same;
          if (rest) {
            const u32 second = (u32)__shfl((int)e, __builtin_ctzll(rest), 64);
            if (__popcll(__ballot(kept && e == second)) > __popcll(same)) first = second;
          }
        }
        const bool mine = kept && e == first;
        auto add = [&](u32 ke, const CAcc& B) {
          unsigned long long* qs = ksum + ke * 3u;
          u32* q = kbox + ke * 6u;
          atomicAdd(&qs[0], (unsigned long long)B.sx), atomicAdd(&qs[1], (unsigned long long)B.sy);
          atomicAdd(&qs[2], (unsigned long long)B.sz);
          atomicMin(&q[0], B.lx), atomicMin(&q[1], B.ly), atomicMin(&q[2], B.lz);
          atomicMax(&q[3], B.hx), atomicMax(&q[4], B.hy), atomicMax(&q[5], B.hz);
        };
        if (kept && !mine) add(e, A);
        CAcc B = A;
        if (!mine) B.sx = B.sy = B.sz = 0u, B.lx = B.ly = B.lz = 0xFFFFFFFFu, B.hx = B.hy = B.hz = 0u;
        cacc_reduce(B);
        if (lane == __builtin_ctzll(__ballot(mine))) add(first, B);
      }
    }
  }
  __syncthreads();
  FR_DBG_MARK(F, dblk, 7);
  if (!bad) {
    // ---- exclusive prefix of every matrix row along the tile columns (a wave per cluster), to memory ----
    for (u32 r = (u32)wave; r < nk; r += RS_T / 64) {
      u32 run = 0u;
      for (int c0 = 0; c0 < ntx; c0 += 64) {
        const int c = c0 + lane;
        const u32 v = c < ntx ? pmx[r * (u32)ntx + (u32)c] : 0u;
        u32 s = v;
        for (int off = 1; off < 64; off <<= 1) {
          const u32 t = (u32)__shfl_up((int)s, off, 64);
          if (lane >= off) s += t;
        }
        if (c < ntx) F.pm[(size_t)r * F.pm_stride + c] = run + s - v;
        run += (u32)__shfl((int)s, 63, 64);
      }
    }
  }
  if (F.dbg && threadIdx.x == 0) {
    F.dbg[(size_t)dblk * FR_DBG_SLOTS + 9] = pp[8];
    F.dbg[(size_t)dblk * FR_DBG_SLOTS + 10] = R;
    F.dbg[(size_t)dblk * FR_DBG_SLOTS + 11] = nq;
  }
  // ---- records: device copy for the kernels that follow, pinned host copy for _search_end ----
  if (!bad && threadIdx.x < nk) {
    const u32 e = threadIdx.x;
    KeptRec r;
    r.addr = k_adr[e], r.slot = k_slot[e], r.size = k_size[e], r.off = k_off[e];
    r.sum[0] = ksum[e * 3u], r.sum[1] = ksum[e * 3u + 1u], r.sum[2] = ksum[e * 3u + 2u];
    for (int k = 0; k < 6; ++k) r.box[k] = kbox[e * 6u + (u32)k];
    r.pad[0] = r.pad[1] = 0u;
    F.krec[k_rank[e]] = r;
    F.h_rec[k_rank[e]] = r;
  }
  if (threadIdx.x == 0) {
    const bool cap = !bad && nq > F.cap_q;  // more Q0 cells than the result arrays hold: an error, not a fallback
    F.counts[0] = min(nq, F.cap_q);
    F.counts[1] = 0u;
    F.counts[2] = bad ? 2u : (cap ? 1u : 0u);  // 2: capacity of the fast path exceeded -> the host runs the legacy chain
    F.counts[6] = dead ? s_fc[9] : (s_ovf ? 16u : (bad ? 17u : 0u));  // which one
    F.counts[3] = bad ? 0u : nk;
    F.counts[5] = bad ? 0u : s_nout;
  }
  if (threadIdx.x < 32) F.fctr[FCTR(threadIdx.x)] = 0u;  // the counters of the NEXT search (its first kernel adds to them at once)
  if (threadIdx.x >= 32 && threadIdx.x < 41) F.fctr[FR_DONE_CTR + FCTR(threadIdx.x - 32)] = 0u;
  if (threadIdx.x == 0) {
    F.counts[8] = V.epoch;              // "resolved" (the kernel k_resolve behind a k_tile_cross that did it returns at once)
    F.counts[9] = IN_LAUNCH ? 1u : 0u;  // ... by whom (fuelmi_frontier_resolved_in_launch)
    F.counts[10] = R;                   // ... and how many tile roots it had (the host's guess for the next search)
  }
  __syncthreads();
  if (threadIdx.x < 15) F.h_counts[threadIdx.x] = F.counts[threadIdx.x];
  // the barrier orders every thread's record stores before thread 0's system-scope release (cumulative): one
  // write-back instead of one per wave
  __syncthreads();
  FR_DBG_MARK(F, dblk, 8);
  if (threadIdx.x == 0) {
    __hip_atomic_store(&F.h_counts[15], V.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);  // "records are in"
  }
  return true;
}
__global__ void __launch_bounds__(RS_TK) k_resolve(Geo g, FArgs F) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ FVar s_v;
  __shared__ u32 s_done;
  {
    constexpr int NV = (int)(sizeof(FVar) / 4);
    const int t = threadIdx.x;
    const u32* src = reinterpret_cast<const u32*>(F.var) + (t < NV ? t : 0);
    if (t == NV) src = F.counts + 8;
    const u32 w = *src;  // (one load instruction for the block and the "resolved" word)
    if (t < NV) reinterpret_cast<u32*>(&s_v)[t] = w;
    if (t == NV) s_done = w;
    __syncthreads();
    if (s_done == s_v.epoch) return;  // the last workgroup of k_tile_cross has resolved this search
  }
  (void)resolve_body<RS_TK, false>(g, F, s_v, smem_raw, FR_RCAP);
}

// Flags (every claimed cell, every NQ seed) and the grouped result: the kept cells cluster by cluster in creation
// order, ascending address inside a cluster.  Address order is (x-row, y, z); a tile column's x-rows interleave the
// column's tiles, so the position of a cell is
//   offset of its cluster + cells of the cluster in the tile columns in front (k_resolve's matrix)
//   + cells of the cluster in the x-rows in front inside this column, over all of its tiles
//   + cells of the cluster in this x-row in the tiles in front (smaller y)        -- both from the per-row counts of
//                                                                                    the column's components
//   + cells of the cluster in front of it in this x-row of this tile (a wave walks the row in order).
// Clusters are told apart inside a tile by a REPRESENTATIVE component (the lowest-numbered component of the tile
// that belongs to the cluster).
template <int NT>
__global__ void __launch_bounds__(NT) k_tile_out(Geo g, FArgs F) {
  FR_DBG_MARK(F, blockIdx.x, 14);  // (before the first load)
  __shared__ TilePro s_pro;
  stage_tile_pro(F, &s_pro);
  const FVar& V = s_pro.V;
  if ((int)blockIdx.x >= V.ntiles_f) return;
  if (s_pro.ovf) return;  // overflow (k_resolve's verdict; not the counter line the atomics went to)
  const TileGeo T = tile_geo(g, V, blockIdx.x);
  const int nseg = T.nseg, items = T.items, TY = T.TY;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  u32* segb = reinterpret_cast<u32*>(smem_raw);  // [items] Q0 bits
  u32* segpre = segb + items;                    // [items + 1]
  u32* segs = segpre + items + 1;                // [items] seed bits
  u32* cadr = segs + items;                      // [FR_TCELL] address of the l-th cell
  u32* rowall = cadr + FR_TCELL;                 // [TX][FR_TROOT] cells of the representative's cluster in x-row lx, whole column
  u32* rowpos = rowall + T.TX * FR_TROOT;        // [TX][FR_TROOT] ... in the tiles in front; then the running output position
  u32* kmap = rowpos + T.TX * FR_TROOT;          // [FR_KCAP] cluster rank -> representative component of this tile (or 0xFFFFFFFF)
  u32* code = kmap + FR_KCAP;                    // [FR_TROOT] rcode of the tile's components
  unsigned short* ckey = reinterpret_cast<unsigned short*>(code + FR_TROOT);  // [FR_TCELL] per cell: representative | 0xFFFE claimed, not kept | 0xFFFF
  __shared__ u32 s_wsum[NT / 64];
  __shared__ u32 s_cn[64], s_cb[64], s_cp[65];  // a chunk of the column's tiles: components, id base, prefix
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dblk = 2 * V.ntiles_f + 2 + (int)blockIdx.x;
  FR_DBG_MARK(F, dblk, 0);
  const u32 nroots = s_pro.nroots, gbase = s_pro.gbase;
  // fetched ahead, beside the bit-planes: the codes of the tile's components, the component numbers of its cells
  // (eight consecutive cells per lane), the first 64 tiles of the column
  u32 my_code = F.rcode[gbase + (threadIdx.x < nroots ? threadIdx.x : 0u)];  // (unconditional, masked)
  if (threadIdx.x >= nroots) my_code = FR_UNCLAIMED;
  const u64 my_tl = reinterpret_cast<const u64*>(F.tlab + (size_t)blockIdx.x * FR_TCELL)[threadIdx.x & (FR_TCELL / 8 - 1)];
  u32 pre_cn, pre_cb;
  {  // (unconditional, masked: see stage_tile_pro)
    const bool ok = threadIdx.x < 64 && (int)threadIdx.x < V.nty_f;
    const int tt = ok ? T.tx * V.nty_f + (int)threadIdx.x : (int)blockIdx.x;
    pre_cn = F.t_nroots[tt], pre_cb = F.t_base[tt];
    if (!ok) pre_cn = 0u, pre_cb = 0u;
  }
  const u32 total = tile_load_arrays<NT, true>(T, F, segb, segpre, s_wsum, segs);  // (uniform)
  FR_DBG_MARK(F, dblk, 1);
  // ---- NQ seeds are flagged whatever happens to the components around them ----
  auto or_flags = [&](long a0, u32 bits) {  // bits of the 32 voxels from address a0
    if (!bits) return;
    const long w = a0 >> 6;
    const int sh = (int)(a0 & 63);
    atomicOr(reinterpret_cast<unsigned long long*>(&F.flag[w]), (unsigned long long)bits << sh);
    if (sh > 32) atomicOr(reinterpret_cast<unsigned long long*>(&F.flag[w + 1]), (unsigned long long)bits >> (64 - sh));
  };
  if (total == 0u || nroots == 0u) {
    for (int it = threadIdx.x; it < items; it += NT) {
      const u32 sb = segs[it];
      if (!sb) continue;
      const int line = it / nseg, c = it - line * nseg;
      or_flags(tile_line_adr(g, T, line) + 32 * c, sb);
    }
    return;
  }
  // ---- codes of the tile's components, representatives ----
  for (int k = threadIdx.x; k < FR_KCAP; k += NT) kmap[k] = 0xFFFFFFFFu;
  for (int k = threadIdx.x; k < T.TX * FR_TROOT; k += NT) rowall[k] = 0u, rowpos[k] = 0u;
  if (threadIdx.x < nroots) code[threadIdx.x] = my_code;
  __syncthreads();
  if (threadIdx.x < nroots && code[threadIdx.x] < FR_KCAP) atomicMin(&kmap[code[threadIdx.x]], threadIdx.x);
  // ---- cells: address, key ----
  if (threadIdx.x < FR_TCELL / 8) {  // (component number for now)
#pragma unroll
    for (int q = 0; q < 8; ++q) ckey[8 * threadIdx.x + q] = (unsigned short)((my_tl >> (8 * q)) & 0xFFull);
  }
  for (int it = threadIdx.x; it < items; it += NT) {
    u32 rem = segb[it];
    if (!rem) continue;
    const int line = it / nseg, c = it - line * nseg;
    const u32 a0 = (u32)(tile_line_adr(g, T, line) + 32 * c);
    u32 l = segpre[it];
    while (rem) {
      const int b = __builtin_ctz(rem);
      rem &= rem - 1u;
      cadr[l++] = a0 + (u32)b;
    }
  }
  __syncthreads();
  for (u32 l = threadIdx.x; l < total; l += NT) {
    const u32 cd = code[ckey[l]];
    ckey[l] = (unsigned short)(cd < FR_KCAP ? kmap[cd] : (cd == FR_UNCLAIMED ? 0xFFFFu : 0xFFFEu));
  }
  FR_DBG_MARK(F, dblk, 2);
  // ---- the column: per-row counts of every component of every tile of column tx, folded into the
  // representatives of this tile's clusters ----
  const int nty = V.nty_f;
  for (int t0 = 0; t0 < nty; t0 += 64) {
    const int nt = min(64, nty - t0);
    __syncthreads();
    if (threadIdx.x < 64) {
      u32 cn = pre_cn, cb = pre_cb;
      if (t0 > 0) {
        cn = cb = 0u;
        if ((int)threadIdx.x < nt) {
          const int tt = T.tx * nty + t0 + threadIdx.x;
          cn = F.t_nroots[tt], cb = F.t_base[tt];
        }
      }
      u32 s = cn;
      for (int off = 1; off < 64; off <<= 1) {
        const u32 t = (u32)__shfl_up((int)s, off, 64);
        if (lane >= off) s += t;
      }
      s_cn[threadIdx.x] = cn, s_cb[threadIdx.x] = cb, s_cp[threadIdx.x] = s - cn;
      if (threadIdx.x == 63) s_cp[64] = s;
    }
    __syncthreads();
    const u32 ncomp = s_cp[64];
    for (u32 j = threadIdx.x; j < ncomp; j += NT) {
      int lo = 0, hi = nt - 1;  // tile of the j-th component of the chunk
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s_cp[mid] <= j)
          lo = mid;
        else
          hi = mid - 1;
      }
      const u32 gi = s_cb[lo] + (j - s_cp[lo]);
      const u32 cd = F.rcode[gi];
      if (cd >= FR_KCAP) continue;
      const u32 rep = kmap[cd];
      if (rep == 0xFFFFFFFFu) continue;  // a cluster this tile has no cell of
      const uint4* rw = reinterpret_cast<const uint4*>(F.rrow + (size_t)gi * FR_TXS);
      const uint4 r0 = rw[0], r1 = rw[1];
      const u32 pk[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
      const bool front = t0 + lo < T.ty;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const u32 c0 = pk[q] & 0xFFFFu, c1 = pk[q] >> 16;
        if (c0 && 2 * q < T.TX) {
          atomicAdd(&rowall[(2 * q) * FR_TROOT + rep], c0);
          if (front) atomicAdd(&rowpos[(2 * q) * FR_TROOT + rep], c0);
        }
        if (c1 && 2 * q + 1 < T.TX) {
          atomicAdd(&rowall[(2 * q + 1) * FR_TROOT + rep], c1);
          if (front) atomicAdd(&rowpos[(2 * q + 1) * FR_TROOT + rep], c1);
        }
      }
    }
  }
  __syncthreads();
  FR_DBG_MARK(F, dblk, 3);
  // ---- first output position of every (x-row, representative) ----
  for (u32 j = threadIdx.x; j < nroots * (u32)T.TX; j += NT) {
    const u32 rep = j / (u32)T.TX, lx = j - rep * (u32)T.TX;
    const u32 cd = code[rep];
    if (cd >= FR_KCAP || kmap[cd] != rep) continue;
    u32 pos = F.krec[cd].off + F.pm[(size_t)cd * F.pm_stride + T.tx];
    for (u32 q = 0; q < lx; ++q) pos += rowall[q * FR_TROOT + rep];
    rowpos[lx * FR_TROOT + rep] += pos;
  }
  __syncthreads();
  FR_DBG_MARK(F, dblk, 4);
  // ---- the rows: a wave walks the cells of an x-row in address order, 64 at a time ----
  u32* key_out = F.ms_key[1];
  u32* val_out = F.ms_val[1];
  const bool direct = F.counts[0] <= F.hcells_direct_max;  // big lists are fetched on demand (0.5 MB over PCIe
                                                           // per search otherwise, whether anybody reads it or not)
  for (int lx = wave; lx < T.nxl; lx += NT / 64) {
    const u32 l0 = segpre[lx * TY * nseg], l1 = segpre[(lx + 1) * TY * nseg];
    for (u32 lb = l0; lb < l1; lb += 64u) {
      const u32 l = lb + (u32)lane;
      const u32 kk = l < l1 ? (u32)ckey[l] : 0xFFFFu;
      const bool active = kk < FR_TROOT;
      u32 pos = 0u;
      u64 todo = __ballot(active);
      while (todo) {
        const int leader = __builtin_ctzll(todo);
        const u32 dl = (u32)__shfl((int)kk, leader, 64);
        const u64 same = __ballot(active && kk == dl);
        volatile u32* rp = &rowpos[(u32)lx * FR_TROOT + dl];  // (other lanes' stores must be seen: no caching in registers)
        const u32 base = *rp;
        if (active && kk == dl) pos = base + (u32)__popcll(same & ((1ull << lane) - 1ull));
        if (lane == leader) *rp = base + (u32)__popcll(same);
        todo &= ~same;
      }
      if (active) {
        const u32 a = cadr[l];
        key_out[pos] = code[kk];
        val_out[pos] = a;
        if (direct) F.h_cells[pos] = a;  // posted write over PCIe
      }
    }
  }
  FR_DBG_MARK(F, dblk, 5);
  // ---- flags: claimed cells + seeds, one or two atomics per 32-voxel segment ----
  for (int it = threadIdx.x; it < items; it += NT) {
    u32 rem = segb[it];
    u32 fl = segs[it];
    u32 l = segpre[it];
    while (rem) {
      const int b = __builtin_ctz(rem);
      rem &= rem - 1u;
      if (ckey[l++] != 0xFFFFu) fl |= 1u << b;
    }
    if (!fl) continue;
    const int line = it / nseg, c = it - line * nseg;
    or_flags(tile_line_adr(g, T, line) + 32 * c, fl);
  }  FR_DBG_MARK(F, dblk, 6);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static const int kFastMenu[4][2] = {{16, 32}, {8, 32}, {8, 16}, {4, 8}};  // tiles of the fast chain (x-rows, z-lines)
// tiles of menu entry mk over a qx x qy rectangle of z-lines
int menu_tiles(int qx, int qy, int mk) {
  return ((qx + kFastMenu[mk][0] - 1) / kFastMenu[mk][0]) * ((qy + kFastMenu[mk][1] - 1) / kFastMenu[mk][1]);
}
// launch grid of the tile kernels: menu entry mk's tile over the largest rectangle a search can cover
static int fast_launch_tiles(const FArgs& F, int mk) {
  return menu_tiles(F.qbox.hi[0] - F.qbox.lo[0] + 2, F.qbox.hi[1] - F.qbox.lo[1] + 2, mk);
}
// the search's fast tiles: menu entry mk's tile over hv's rectangle px0..px1 x py0..py1
void set_fast_tiles(FVar& hv, int mk) {
  const int qx = hv.px1 - hv.px0 + 1, qy = hv.py1 - hv.py0 + 1;
  hv.ftx = kFastMenu[mk][0], hv.fty = kFastMenu[mk][1];
  hv.ntx_f = std::max(0, (qx + hv.ftx - 1) / hv.ftx);
  hv.nty_f = std::max(0, (qy + hv.fty - 1) / hv.fty);
  hv.ntiles_f = hv.ntx_f * hv.nty_f;
}

// the fast chain: four direct launches (512-lane tile workgroups: 256 lanes measured 4-11 % slower in round 3 and again
// in round 6, profiles/r06_frontier_threads_prio_sweep.txt); falls back to the legacy one through counts[2] == 2
int frontier_enqueue_fast(fuelmi_frontier* f) {
  const Geo& g = f->map->g;
  FArgs& F = f->F;
  const int mk = f->fast_menu;
  const int tiles = fast_launch_tiles(F, mk);
  if (f->tl_ev) HIPCHK(hipEventRecord(f->tl_ev[0], f->stream));
  k_tile_ccl<512><<<tiles, 512, f->tile_lds[mk], f->stream>>>(g, F, *f->h_var);
  FDBG("k_tile_ccl");
  g_ht.lap(4);
  // the tile CCL (and the changed-cluster test in front of it) is the last reader of the map's occupancy planes: a
  // fusion queued behind this point may start as soon as it is done
  if (f->mark_planes_read) {
    HIPCHK(hipEventRecord(f->ev_planes_read, f->stream));
    map_add_plane_reader(f->map, f->ev_planes_read);
  } else {
    // nobody has rewritten the planes beside a running search of this finder yet (a plan cycle on a given map does
    // not; a streaming pipeline does from its first frame on): no barrier packet between the chain's kernels -- a
    // mutator that does arrive records the event behind what is queued and switches the marking on (map_wait_plane_readers)
    map_add_late_reader(f->map, f->stream, f->ev_planes_read, &f->mark_planes_read);
  }
  if (f->tl_ev) HIPCHK(hipEventRecord(f->tl_ev[1], f->stream));
  g_ht.lap(5);
  // round 6: the last workgroup of k_tile_cross resolves searches of up to 1 024 tile roots (measured against k_resolve
  // as a launch of its own: profiles/r06_cross_resolve_fusion_ab.txt)
  {
    // (a finder whose last search had more tile roots than the launch's LDS holds -- the 800^2 x 200 map's full box: 2 465 --
    // does not try again for the next 16 searches: the attempt costs every workgroup a barrier and two atomics, -5 % there)
    bool fuse_now = f->h_var->ntiles_f > 0;  // (no tile, no last workgroup: k_resolve publishes the empty result)
    if (fuse_now && f->fuse_skip > 0) --f->fuse_skip, fuse_now = false;
    f->fuse_tried = fuse_now;
    const size_t lds_x = fuse_now ? std::max(f->cross_lds[mk], resolve_lds_bytes(1024)) : f->cross_lds[mk];
    const u32 rcap = fuse_now ? (u32)std::min<size_t>((lds_x - resolve_lds_bytes(0)) / 16, FR_RCAP) : 0u;
    // k_resolve is not even queued when this finder's last search was resolved in the launch with at most half the tile
    // roots the launch holds (a launch and a kernel boundary of the tail per search); a search that outgrows the guess
    // says so in its result (counts[2] == 3) and _search_end queues the two kernels then
    f->kr_queued = !(fuse_now && f->kr_skip_ok);
    k_tile_cross<512><<<tiles, 512, lds_x, f->stream>>>(g, F, rcap | (f->kr_queued ? 0u : 0x80000000u));
    f->rcap_used = rcap;
  }
  FDBG("k_tile_cross");
  g_ht.lap(6);
  if (f->kr_queued) k_resolve<<<1, RS_TK, f->resolve_lds, f->stream>>>(g, F);
  FDBG("k_resolve");
  g_ht.lap(7);
  if (f->tl_ev) HIPCHK(hipEventRecord(f->tl_ev[2], f->stream));
  k_tile_out<512><<<tiles, 512, f->out_lds[mk], f->stream>>>(g, F);
  FDBG("k_tile_out");
  g_ht.lap(8);
  if (f->tl_ev) HIPCHK(hipEventRecord(f->tl_ev[3], f->stream));
  HIPCHK(hipGetLastError());
  return FUELMI_OK;
}

// fuelmi_frontier_create's part of the fast chain.  Per menu entry: segments per tile and the dynamic LDS of the tile
// kernels (f->fast_items, tile_lds, cross_lds, out_lds) for a qx x qy Q box; returns the words of the per-tile
// segment arrays (tq / ts)
size_t frontier_tile_lds(fuelmi_frontier* f, int qx, int qy) {
  const Geo& g = f->map->g;
  size_t seg_words = 0;  // per-tile segment arrays: the largest (tiles x segments per tile) of the menu
  for (int k = 0; k < 4; ++k) {
    const int ftx = kFastMenu[k][0], fty = kFastMenu[k][1];
    const size_t items = (size_t)(ftx * fty) * ((g.nz + 31) / 32);
    seg_words = std::max(seg_words, (size_t)((qx + 1 + ftx - 1) / ftx) * ((qy + 1 + fty - 1) / fty) * items);
    f->fast_items[k] = items;
    // k_tile_ccl: labels, bits + prefix, records, per-row counts, root numbers, component per cell
    f->tile_lds[k] = (FR_TCELL + 3 * items + 1 + (size_t)FR_TROOT * 8 + (size_t)FR_TROOT * FR_TXS) * sizeof(u32) +
                     FR_TCELL * sizeof(unsigned short) + FR_TCELL;
    f->cross_lds[k] = (2 * items + (size_t)XC_WCAP) * sizeof(u32);
    // k_tile_out: bits + prefix + seed bits, cell addresses, the two row tables, cluster map, codes, keys
    f->out_lds[k] = (3 * items + 1 + FR_TCELL + 2 * (size_t)kFastMenu[k][0] * FR_TROOT + FR_KCAP + FR_TROOT) * sizeof(u32) +
                    FR_TCELL * sizeof(unsigned short);
    f->tile_lds[k] = (f->tile_lds[k] + 15) & ~(size_t)15;
    f->cross_lds[k] = (f->cross_lds[k] + 15) & ~(size_t)15;
    f->out_lds[k] = (f->out_lds[k] + 15) & ~(size_t)15;
  }
  return seg_words;
}
// ... the kernels' dynamic LDS ceilings (f->resolve_lds)
int frontier_tile_attrs(fuelmi_frontier* f) {
  const size_t lds_max = std::max(f->tile_lds[0], f->out_lds[0]);
  if (lds_max > 64 * 1024 && lds_max <= 150 * 1024) {
    // (the attribute belongs to the FUNCTION, not to this finder: always the kernels' ceiling, so that a second
    // finder with a shorter map cannot lower it under a taller finder's launches -- ADVICE r3)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tile_ccl<512>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tile_out<512>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
  }
  f->resolve_lds = resolve_lds_bytes(FR_RCAP);
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_resolve), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)f->resolve_lds));
  return FUELMI_OK;
}
// ... and whether the menu's largest tile fits the tile kernels
// (a thread of the tile kernels fetches at most FT_PER segments: z-lines of up to 256 voxels with the largest tile)
bool frontier_tile_fits(const fuelmi_frontier* f) {
  return std::max(f->tile_lds[0], f->out_lds[0]) <= 150 * 1024 && f->fast_items[0] <= (size_t)FT_PER * 512;
}

// the search outgrew the launch that was to resolve it and no k_resolve was queued (counts[2] == 3): the two kernels
// behind k_tile_cross, queued by _search_end
int frontier_enqueue_late_resolve(fuelmi_frontier* f) {
  const Geo& g = f->map->g;
  FArgs& F = f->F;
  const int mk = f->fast_menu;
  k_resolve<<<1, RS_TK, f->resolve_lds, f->stream>>>(g, F);
  k_tile_out<512><<<fast_launch_tiles(F, mk), 512, f->out_lds[mk], f->stream>>>(g, F);
  HIPCHK(hipGetLastError());
  return FUELMI_OK;
}
