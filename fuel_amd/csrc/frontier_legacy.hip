// frontier_legacy.hip -- the legacy clustering chain of the frontier search (round 1), on the CELLS: bit-plane
// predicate per 64-voxel word (funnel-shifted neighbour planes, wave prefix sums) -> ordered compaction -> lock-free
// union-find over the compact cells (neighbour lookup = bit test + popcount rank) -> atomicMin claims -> sizes ->
// flags -> ranking of the kept clusters, stable radix multisplit of their cells and the per-cluster records, copied
// out to pinned host memory.  About 23 dependent launches whose arguments never change (everything per-search sits
// behind F.var): replayed as a hipGraph.
//
// It is the no-limits fallback of the tile chain (frontier_tile.hip): searches with cluster_min < 1, finders whose
// tiles do not fit, FUELMI_FRONTIER_LEGACY, and searches that exceed a capacity of the tile chain.  frontier_regroup
// (multisplit + records + copy-out) also serves the split stage (frontier_split.hip).
#include <cstdlib>

#include "frontier_internal.h"

// ---- per-word masks ---------------------------------------------------------------------------
__device__ __forceinline__ void word_masks(const Geo& g, int w, const Box3& qb, const Box3& sb, u64& z0,
                                           u64& zl, u64& y0, u64& yl, u64& mq, u64& ms) {
  z0 = zl = y0 = yl = mq = ms = 0ull;
  long a0 = 64L * w;
  if (a0 >= g.N) return;
  int line = (int)(a0 / g.nz);
  int z = (int)(a0 - (long)line * g.nz);
  int x = line / g.ny;
  int y = line - x * g.ny;
  int bpos = 0;
  while (bpos < 64 && x < g.nx) {
    int len = min(g.nz - z, 64 - bpos);
    if (z == 0) z0 |= 1ull << bpos;
    if (z + len == g.nz) zl |= 1ull << (bpos + len - 1);
    u64 seg = bit_range(bpos, len);
    if (y == 0) y0 |= seg;
    if (y == g.ny - 1) yl |= seg;
    if (x >= qb.lo[0] && x <= qb.hi[0] && y >= qb.lo[1] && y <= qb.hi[1]) {
      int zlo = max(z, qb.lo[2]), zhi = min(z + len - 1, qb.hi[2]);
      if (zlo <= zhi) mq |= bit_range(bpos + (zlo - z), zhi - zlo + 1);
    }
    if (x >= sb.lo[0] && x <= sb.hi[0] && y >= sb.lo[1] && y <= sb.hi[1]) {
      int zlo = max(z, sb.lo[2]), zhi = min(z + len - 1, sb.hi[2]);
      if (zlo <= zhi) ms |= bit_range(bpos + (zlo - z), zhi - zlo + 1);
    }
    bpos += len;
    z = 0;
    if (++y == g.ny) {
      y = 0;
      ++x;
    }
  }
}

__device__ void scan_sums_tail(const FArgs& F) {
  // one block of 1024 threads: contiguous slices of the block sums per thread, then a Hillis-Steele scan
  // of the 1024 partials in LDS (a 256-thread version with a serial middle cost 18 us on an 800^2 x 200 map)
  __shared__ u64 part[1024];
  const int nblocks = F.var->nblocks;
  const int T = blockDim.x;
  const int per = (nblocks + T - 1) / T;
  const int b0 = threadIdx.x * per, b1 = min(nblocks, b0 + per);
  u64 s = 0;
  for (int b = b0; b < b1; ++b) s += F.blocksum[b];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < T; off <<= 1) {
    const u64 v = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0ull;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  if (threadIdx.x == T - 1) {
    const u64 run = part[T - 1];
    u32 nq = (u32)run, ns = (u32)(run >> 32);
    u32 ovf = 0;
    if (nq > F.cap_q) {
      nq = F.cap_q;
      ovf = 1;
    }
    if (ns > F.cap_s) {
      ns = F.cap_s;
      ovf = 1;
    }
    F.counts[0] = nq;
    F.counts[1] = ns;
    F.counts[2] = ovf;
    F.counts[3] = 0;
    F.counts[5] = 0;
  }
  u64 run = part[threadIdx.x] - s;  // exclusive prefix of this thread's slice
  for (int b = b0; b < b1; ++b) {
    u64 v = F.blocksum[b];
    F.blockscan[b] = run;
    run += v;
  }
}

// predicate planes + in-block packed prefix of their popcounts
__global__ void __launch_bounds__(256) k_pred(Geo g, FArgs F) {
  __shared__ u64 wsum[4];
  const FVar& V = *F.var;
  if ((int)blockIdx.x >= V.nblocks) return;
  const int rel = blockIdx.x * 256 + threadIdx.x;
  const int w = V.w0 + rel;
  u64 q = 0ull, s = 0ull;
  if (w < g.W) {
    u64 z0, zl, y0, yl, mq, ms;
    word_masks(g, w, V.qreg, V.sbox, z0, zl, y0, yl, mq, ms);
    if ((mq | ms) != 0ull) {
      u64 f1 = f1_word(g, F.occ, F.unk, w, z0, zl, y0, yl) & ~F.flag[w];
      q = f1 & mq;
      s = f1 & ms & ~mq;
    }
    F.qb[w] = q;
    F.sb[w] = s;
  }
  u64 packed = (u64)__popcll(q) | ((u64)__popcll(s) << 32);
  u64 v = packed;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    u64 t = __shfl_up(v, off, 64);
    if (lane >= off) v += t;
  }
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  u64 woff = 0;
  for (int k = 0; k < wave; ++k) woff += wsum[k];
  u64 excl = v - packed + woff;
  F.pref[rel] = excl;
  if (threadIdx.x == 255) F.blocksum[blockIdx.x] = excl + packed;
}
__global__ void __launch_bounds__(1024) k_scan_sums(FArgs F) { scan_sums_tail(F); }

// ordered compaction of Q0 cells and NQ seeds
__global__ void __launch_bounds__(256) k_compact(Geo g, FArgs F) {
  if ((int)blockIdx.x >= F.var->nblocks) return;
  const int rel = blockIdx.x * 256 + threadIdx.x;
  const int w = F.var->w0 + rel;
  if (w >= g.W) return;
  u64 q = F.qb[w], s = F.sb[w];
  if ((q | s) == 0ull) return;
  u64 pk = F.blockscan[rel >> 8] + F.pref[rel];
  u32 iq = (u32)pk, is = (u32)(pk >> 32);
  const u32 nq = F.counts[0];
  while (q) {
    int b = __builtin_ctzll(q);
    q &= q - 1;
    if (iq < F.cap_q) {
      F.cell_adr[iq] = (u32)(64L * w + b);
      F.parent[iq] = iq;
      F.claim[iq] = NOCLAIM;
      F.csize[iq] = 0;
    }
    ++iq;
  }
  while (s) {
    int b = __builtin_ctzll(s);
    s &= s - 1;
    if (is < F.cap_s) {
      F.seed_adr[is] = (u32)(64L * w + b);
      F.csize[nq + is] = 1;  // every NQ seed starts its own cluster
    }
    ++is;
  }
}

// find with path halving.  The shortcut is written with a (non-returning) device-scope atomicMin,
// NOT a plain store: plain stores stay dirty in this XCD's write-back L2 and their later line
// write-back would clobber links other XCDs made on neighbouring entries with memory-side atomics
// (observed as lost unions).  Every write to parent[] inside k_union is therefore an atomic; plain
// reads may be stale, but a stale parent is still an ancestor (parents only decrease).
__device__ __forceinline__ u32 uf_find(u32* parent, u32 i) {
  u32 p = parent[i];
  while (p != i) {
    u32 gp = parent[p];
    if (gp != p) (void)__hip_atomic_fetch_min(&parent[i], gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    i = p;
    p = gp;
  }
  return i;
}
__device__ __forceinline__ void uf_union(u32* parent, u32 a, u32 b) {
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) {
      u32 t = a;
      a = b;
      b = t;
    }
    u32 old = atomicMin(&parent[a], b);
    if (old == a) return;
    a = old;
  }
}

// ---- connected components, 26-connectivity -------------------------------------------------------
// Two levels.  (1) k_ccl_local: a workgroup owns a spatial tile of TX x TY z-lines, labels its Q0
// voxels in LDS (union-find with LDS atomics: ~40 ns per dependent step instead of ~1 us through
// memory-side atomics) and writes parent[cell] = compact index of the tile-local root, so every
// local component leaves the kernel flat.  (2) k_union: only neighbour relations that cross a tile
// face go through the global lock-free union-find.  (3) k_flatten.
#define LNONE 0xFFFFFFFFu
__device__ __forceinline__ u32 lds_find(volatile u32* lab, u32 i) {
  u32 p = lab[i];
  while (p != i) {
    i = p;
    p = lab[i];
  }
  return i;
}
__device__ __forceinline__ void lds_union(u32* lab, u32 a, u32 b) {
  while (true) {
    a = lds_find(lab, a);
    b = lds_find(lab, b);
    if (a == b) return;
    if (a < b) {
      u32 t = a;
      a = b;
      b = t;
    }
    u32 old = atomicMin(&lab[a], b);
    if (old == a) return;
    a = old;
  }
}

template <int NT>
__global__ void __launch_bounds__(NT) k_ccl_local(Geo g, FArgs F, int TX, int TY) {
  if ((int)blockIdx.x >= F.var->ntiles) return;
  const Box3& QR = F.var->qreg;
  const int nty = F.var->nty;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  u32* lab = reinterpret_cast<u32*>(smem_raw);  // [TX*TY lines][nz]
  const int tx = blockIdx.x / nty, ty = blockIdx.x - tx * nty;
  const int x0 = QR.lo[0] + tx * TX, y0 = QR.lo[1] + ty * TY;
  const int nxl = min(TX, QR.hi[0] - x0 + 1), nyl = min(TY, QR.hi[1] - y0 + 1);
  const int nz = g.nz, nseg = (nz + 31) >> 5;
  const int items = TX * TY * nseg;
  u32* segb = lab + TX * TY * nz;  // [TX*TY][nseg] Q0 bits of each 32-voxel segment
  u32* segrank = segb + items;     // compact index of the first Q0 voxel at/after the segment start
  u32* rowr = segrank + items;     // [2*TX] compact index range of each x-row of the tile
  if ((int)threadIdx.x < 2 * TX) {
    const int lx = threadIdx.x >> 1, hi = threadIdx.x & 1;
    u32 rk = 0u;
    if (lx < nxl) rk = min(rank_q(F, (long)(x0 + lx) * g.nyz + (long)(y0 + (hi ? nyl : 0)) * nz), F.cap_q);
    rowr[threadIdx.x] = rk;
  }
  // Everything below walks SET BITS only (frontier cells are ~1 % of the voxels); the only global
  // traffic is this prologue and the parent[] stores at the end.
  for (int it = threadIdx.x; it < items; it += NT) {
    const int line = it / nseg, c = it - line * nseg, lx = line / TY, ly = line - lx * TY;
    const int zn = min(32, nz - 32 * c);
    u32 bits = 0u, rk = 0u;
    if (lx < nxl && ly < nyl) {
      const long lb = (long)(x0 + lx) * g.nyz + (long)(y0 + ly) * nz + 32 * c;
      bits = (u32)plane_window(F.qb, lb);
      if (zn < 32) bits &= (1u << zn) - 1u;
      if (bits) rk = rank_q(F, lb);
    }
    segb[it] = bits;
    segrank[it] = rk;
    const u32 l0 = (u32)(line * nz + 32 * c);
    const u32 all = bits;
    while (bits) {  // 1: label = start of the cell's z-run inside the segment (runs are pre-joined)
      const int z = __builtin_ctz(bits);
      bits &= bits - 1;
      const u32 holes = ~all & ((1u << z) - 1u);
      lab[l0 + z] = l0 + (holes ? 32 - __builtin_clz(holes) : 0);
    }
  }
  __syncthreads();
  // 2 + 3 walk the tile's cells through their COMPACT indices so every lane gets one cell at a time
  // (a vertical frontier wall puts 20-30 cells into one 32-voxel segment; a per-segment loop would
  // leave one lane with all the dependent LDS work).  For a fixed x the TY lines of the tile are
  // contiguous in address, hence contiguous in compact index: TX ranges per tile.
  u32 total = 0u;
  for (int lx = 0; lx < nxl; ++lx) total += rowr[2 * lx + 1] - rowr[2 * lx];
  for (u32 t = threadIdx.x; t < total; t += NT) {
    {
      int lx = 0;
      u32 tt = t;
      for (; lx < nxl - 1; ++lx) {  // which x-row of the tile holds the t-th cell (<= TX steps)
        const u32 n = rowr[2 * lx + 1] - rowr[2 * lx];
        if (tt < n) break;
        tt -= n;
      }
      const u32 i = rowr[2 * lx] + tt;
      const long a_lo = (long)(x0 + lx) * g.nyz + (long)y0 * nz;
      const int rem = (int)(F.cell_adr[i] - (u32)a_lo);  // offset inside this x-row of the tile
      const int ly = rem / nz, z = rem - ly * nz;
      const int line = lx * TY + ly, c = z >> 5, zz = z & 31;
      const u32 v = (u32)(line * nz + z);
      // z-runs are pre-joined inside a segment; join across the segment seam ...
      if (zz == 0 && c > 0 && (segb[line * nseg + c - 1] >> 31)) lds_union(lab, v, v - 1);
      // ... and with the four lower z-lines of the tile: one 3-bit window (dz -1,0,+1) per line, one
      // union per run (only the pattern 101 holds two)
      for (int l = 0; l < 4; ++l) {
        const int nlx = lx + (l < 3 ? -1 : 0), nly = ly + (l < 3 ? l - 1 : -1);
        if (nlx < 0 || nly < 0 || nly >= TY) continue;
        const int nline = nlx * TY + nly;
        const int zlo = z - 1;
        const int s0 = max(zlo, 0) >> 5;
        const unsigned long long w = (unsigned long long)segb[nline * nseg + s0] |
            ((s0 + 1 < nseg) ? ((unsigned long long)segb[nline * nseg + s0 + 1] << 32) : 0ull);
        u32 pat = (zlo >= 0) ? (u32)((w >> (zlo - 32 * s0)) & 7ull) : (u32)((w << 1) & 6ull);
        if (z + 1 >= nz) pat &= 3u;
        if (!pat) continue;
        const u32 ln = (u32)(nline * nz + zlo + __builtin_ctz(pat));
        lds_union(lab, v, ln);
        if (pat == 5u) lds_union(lab, v, ln + 2);
      }
    }
  }
  __syncthreads();
  // 3: parent[cell] = compact index of its tile-local root
  for (u32 t = threadIdx.x; t < total; t += NT) {
    {
      int lx = 0;
      u32 tt = t;
      for (; lx < nxl - 1; ++lx) {
        const u32 n = rowr[2 * lx + 1] - rowr[2 * lx];
        if (tt < n) break;
        tt -= n;
      }
      const u32 i = rowr[2 * lx] + tt;
      const long a_lo = (long)(x0 + lx) * g.nyz + (long)y0 * nz;
      const int rem = (int)(F.cell_adr[i] - (u32)a_lo);
      const int ly = rem / nz, z = rem - ly * nz;
      const u32 v = (u32)((lx * TY + ly) * nz + z);
      const u32 r = lds_find(lab, v);
      u32 pr = i;
      if (r != v) {
        const int rline = (int)(r / (u32)nz), rz = (int)(r - (u32)rline * (u32)nz);
        const int rs = rline * nseg + (rz >> 5);
        pr = segrank[rs] + (u32)__popc(segb[rs] & ((1u << (rz & 31)) - 1u));
      }
      F.parent[i] = pr;
    }
  }
}

// global merge: neighbour relations crossing a tile face (lower-address side only).
// A wall crossing a tile face yields dozens of adjacent cell pairs that all join the same two
// tile-local components; since k_ccl_local left parent[] flat, the pair of tile roots identifies the
// union, and each wave issues one union per DISTINCT root pair (the dependent atomics of the
// lock-free union-find, and the same-address traffic on a huge component's roots, are what costs).
__global__ void __launch_bounds__(256) k_union(Geo g, FArgs F, int TX, int TY) {
  // Per 64 cells: (1) every lane looks up the tile roots behind its cross-face windows (independent
  // loads, all in flight together), (2) the wave removes duplicate root pairs and queues the distinct
  // ones in LDS, (3) the queue is spread over the lanes, one union each.  A union is a chain of
  // dependent ~1 us memory-side operations: what matters is that a wave runs them side by side, not
  // one face direction after the other.
  __shared__ u32 q_a[4][128], q_b[4][128];  // per wave: distinct root pairs of this round
  const u32 nq = F.counts[0];
  const u32 nq_r = (nq + 63u) & ~63u;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < nq_r; i += gridDim.x * blockDim.x) {
    const bool live = i < nq;
    // the four lower z-lines (dx,dy) = (-1,-1) (-1,0) (-1,1) (0,-1): one 3-bit window each (dz -1,0,+1);
    // a line inside this cell's tile was already handled in LDS
    const int ldx[4] = {-1, -1, -1, 0}, ldy[4] = {-1, 0, 1, -1};
    u32 pat[4] = {0u, 0u, 0u, 0u};
    long nb0[4] = {0, 0, 0, 0};
    u32 ri = 0u;
    if (live) {
      long a = F.cell_adr[i];
      int x = (int)(a / g.nyz);
      int r = (int)(a - (long)x * g.nyz);
      int y = r / g.nz, z = r - y * g.nz;
      const int lx = (x - F.var->qreg.lo[0]) % TX, ly = (y - F.var->qreg.lo[1]) % TY;
      const bool zlo = z > 0, zhi = z < g.nz - 1;
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        const int xx = x + ldx[l], yy = y + ldy[l];
        const bool cross = (ldx[l] < 0 && lx == 0) || (ldy[l] < 0 && ly == 0) || (ldy[l] > 0 && ly == TY - 1);
        const bool ok = cross && xx >= 0 && yy >= 0 && yy < g.ny;
        nb0[l] = a + (long)ldx[l] * g.nyz + (long)ldy[l] * g.nz - 1;
        u32 p = ok ? (u32)(plane_window(F.qb, nb0[l]) & 7ull) : 0u;
        if (!zlo) p &= ~1u;
        if (!zhi) p &= ~4u;
        pat[l] = p;
      }
      if (pat[0] | pat[1] | pat[2] | pat[3]) ri = F.parent[i];  // tile root (or already an ancestor of it)
    }
    if (!__ballot((pat[0] | pat[1] | pat[2] | pat[3]) != 0u)) continue;
    // z-adjacent neighbours of one line are joined by their own (0,0,-1) unions: one link per run; only
    // the pattern 101 holds two separate runs
    u32 rj[8];
    bool act[8];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      u32 j = F.cap_q;
      if (pat[l]) j = rank_q(F, nb0[l] + __builtin_ctz(pat[l]));
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const u32 jj = j + (u32)k;
        bool on = ((k == 0) ? (pat[l] != 0u) : (pat[l] == 5u)) && jj < F.cap_q;
        u32 v = 0u;
        if (on) v = F.parent[jj];
        rj[2 * l + k] = v;
        act[2 * l + k] = on;
      }
    }
    u32 nqueue = 0u;  // wave-uniform
#pragma unroll
    for (int s8 = 0; s8 < 8; ++s8) {
      const bool on = act[s8] && rj[s8] != ri;
      u64 todo = __ballot(on);
      bool lead = false;
      while (todo) {
        const int leader = __builtin_ctzll(todo);
        const u32 ki = (u32)__shfl((int)ri, leader, 64), kj = (u32)__shfl((int)rj[s8], leader, 64);
        const u64 same = __ballot(on && ri == ki && rj[s8] == kj) & todo;
        if (lane == leader) lead = true;
        todo &= ~same;
      }
      const u64 leads = __ballot(lead);
      if (lead) {
        const u32 slot = nqueue + (u32)__popcll(leads & ((1ull << lane) - 1ull));
        if (slot < 128u) {
          q_a[wv][slot] = ri;
          q_b[wv][slot] = rj[s8];
        } else {
          uf_union(F.parent, ri, rj[s8]);  // queue full (never seen): do it in place
        }
      }
      nqueue += (u32)__popcll(leads);
    }
    nqueue = min(nqueue, 128u);
    __builtin_amdgcn_wave_barrier();
    for (u32 t = lane; t < nqueue; t += 64u) uf_union(F.parent, q_a[wv][t], q_b[wv][t]);
    __builtin_amdgcn_wave_barrier();
  }
}

// root of a cell without writing (k_claim: k_union has finished, parents are final and chains short)
__device__ __forceinline__ u32 uf_root(const u32* parent, u32 i) {
  u32 p = parent[i];
  while (p != i) {
    i = p;
    p = parent[i];
  }
  return i;
}

__device__ __forceinline__ bool in_box(const Geo& g, const Box3& b, long a) {
  int x = (int)(a / g.nyz);
  int r = (int)(a - (long)x * g.nyz);
  int y = r / g.nz, z = r - y * g.nz;
  return x >= b.lo[0] && x <= b.hi[0] && y >= b.lo[1] && y <= b.hi[1] && z >= b.lo[2] && z <= b.hi[2];
}

// one atomicMin per distinct root per wave (a frontier surface is often ONE huge component:
// per-lane atomics on its root serialise)
__device__ __forceinline__ void wave_min_claim(u32* claim, bool active, u32 root, u32 a) {
  u64 todo = __ballot(active);
  const int lane = threadIdx.x & 63;
  while (todo) {
    int leader = __builtin_ctzll(todo);
    u32 k = __shfl(root, leader, 64);
    u64 same = __ballot(active && root == k) & todo;
    u32 v = ((same >> lane) & 1ull) ? a : 0xFFFFFFFFu;
    for (int off = 32; off > 0; off >>= 1) v = min(v, (u32)__shfl_xor((int)v, off, 64));
    if (lane == leader && claim[k] > v) atomicMin(&claim[k], v);
    todo &= ~same;
  }
}

// claims: own cells inside the scan box, then NQ seeds adjacent to a component
__global__ void __launch_bounds__(256) k_claim(Geo g, FArgs F) {
  const u32 nq = F.counts[0], ns = F.counts[1];
  const u32 ns_r = (ns + 63u) & ~63u;
  const Box3 sbox = F.var->sbox;
  // Own cells: cell_adr ascends with the compact index, so the lowest claimer of a component inside
  // a 1024-cell chunk is simply its first active cell.  One atomic per chunk for the chunk's leading
  // component (a frontier surface is mostly ONE component: per-wave atomics on its claim word were
  // thousands of same-address operations), wave-aggregated atomics for the other components.
  __shared__ u32 s_root[16], s_adr[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (u32 base = blockIdx.x * 1024u; base < nq; base += gridDim.x * 1024u) {
    bool act[4];
    u32 rt[4], ad[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const u32 i = base + (u32)k * 256u + threadIdx.x;
      act[k] = false;
      rt[k] = 0u;
      ad[k] = 0u;
      if (i < nq) {
        ad[k] = F.cell_adr[i];
        // flatten on the way: every cell ends with parent = root (k_sizes / the seed claims read it);
        // a plain store is safe here, nothing issues atomics on parent[] in this kernel
        const u32 root = uf_root(F.parent, i);
        F.parent[i] = root;
        if (in_box(g, sbox, ad[k])) {
          act[k] = true;
          rt[k] = root;
        }
      }
      const u64 m = __ballot(act[k]);
      if (lane == 0) s_root[k * 4 + wave] = NOCLAIM;
      if (m && lane == __builtin_ctzll(m)) {
        s_root[k * 4 + wave] = rt[k];
        s_adr[k * 4 + wave] = ad[k];
      }
    }
    __syncthreads();
    u32 key0 = NOCLAIM, adr0 = 0u;
    for (int e = 15; e >= 0; --e)
      if (s_root[e] != NOCLAIM) {
        key0 = s_root[e];
        adr0 = s_adr[e];
      }
    if (threadIdx.x == 0 && key0 != NOCLAIM) atomicMin(&F.claim[key0], adr0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool slow = act[k] && rt[k] != key0;
      if (__ballot(slow)) wave_min_claim(F.claim, slow, rt[k], ad[k]);
    }
    __syncthreads();
  }
  // NQ seeds: claim every component touching the seed's 26-neighbourhood.  The nine z-lines around
  // the seed are read as 3-bit windows first (independent loads); only lines that hold Q0 cells
  // take the dependent rank -> root -> claim chain, once per run (101 holds two runs).
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < ns_r; i += gridDim.x * blockDim.x) {
    const bool live = i < ns;
    const long a = live ? F.seed_adr[i] : 0;
    u32 pats = 0u;
    if (live) {
      const int x = (int)(a / g.nyz);
      const int rr = (int)(a - (long)x * g.nyz);
      const int y = rr / g.nz, z = rr - y * g.nz;
#pragma unroll
      for (int l = 0; l < 9; ++l) {
        const int dx = l / 3 - 1, dy = l % 3 - 1;
        const int xx = x + dx, yy = y + dy;
        if (xx < 0 || xx >= g.nx || yy < 0 || yy >= g.ny) continue;
        u32 p = (u32)(plane_window(F.qb, a + (long)dx * g.nyz + (long)dy * g.nz - 1) & 7ull);
        if (z == 0) p &= ~1u;
        if (z == g.nz - 1) p &= ~4u;
        pats |= p << (3 * l);
      }
    }
    u32 last = NOCLAIM;
    while (__ballot(pats != 0u)) {
      bool active = pats != 0u;
      u32 r = 0u, r2 = 0u;
      bool two = false;
      if (active) {
        const int l = __builtin_ctz(pats) / 3;
        const u32 p = (pats >> (3 * l)) & 7u;
        pats &= ~(7u << (3 * l));
        const int dx = l / 3 - 1, dy = l % 3 - 1;
        const u32 j = rank_q(F, a + (long)dx * g.nyz + (long)dy * g.nz - 1 + __builtin_ctz(p));
        active = j < F.cap_q;
        if (active) {
          r = uf_root(F.parent, j);
          if (p == 5u && j + 1 < F.cap_q) {
            r2 = uf_root(F.parent, j + 1);
            two = r2 != r;
          }
          if (r == last) active = false;  // this seed already claimed that component
          last = r;
        }
      }
      if (__ballot(active)) wave_min_claim(F.claim, active, r, (u32)a);
      if (__ballot(two)) wave_min_claim(F.claim, two, r2, (u32)a);
    }
  }
}

// one atomicAdd per distinct key per wave
__device__ __forceinline__ void wave_agg_add(u32* base, bool active, u32 key) {
  u64 todo = __ballot(active);
  const int lane = threadIdx.x & 63;
  while (todo) {
    int leader = __builtin_ctzll(todo);
    u32 k = __shfl(key, leader, 64);
    u64 same = __ballot(active && key == k) & todo;
    if (lane == leader) atomicAdd(&base[k], (u32)__popcll(same));
    todo &= ~same;
  }
}

// cluster sizes by slot: own claimer -> its compact index; NQ seed claimer -> nq + seed rank.
// A frontier surface is typically ONE huge cluster, so per-lane (even per-wave) atomics on its
// counter serialise: every 1024-cell chunk is reduced in the block for its leading slot (key0) and
// only cells of other slots take the wave-aggregated atomic path.
__global__ void __launch_bounds__(256) k_sizes(Geo g, FArgs F) {
  __shared__ u32 s_key0;
  __shared__ u32 s_part[4];
  const u32 nq = F.counts[0];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (u32 base = blockIdx.x * SZ_CH; base < nq; base += gridDim.x * SZ_CH) {
    u32 slots[SZ_CH / 256];
    bool act[SZ_CH / 256];
#pragma unroll
    for (int k = 0; k < SZ_CH / 256; ++k) {
      const u32 i = base + k * 256 + threadIdx.x;
      act[k] = false;
      slots[k] = 0;
      if (i < nq) {
        u32 cl = F.claim[F.parent[i]];
        if (cl != NOCLAIM) {
          act[k] = true;
          bool own = (F.qb[cl >> 6] >> (cl & 63)) & 1ull;
          slots[k] = own ? rank_q(F, cl) : nq + rank_s(F, cl);
          F.cell_slot[i] = (int)slots[k];
        } else
          F.cell_slot[i] = -1;
      }
    }
    if (wave == 0) {
      u64 m = __ballot(act[0]);
      u32 k0 = m ? (u32)__shfl((int)slots[0], __builtin_ctzll(m), 64) : NOCLAIM;
      if (lane == 0) s_key0 = k0;
    }
    __syncthreads();
    const u32 key0 = s_key0;
    u32 local = 0;
#pragma unroll
    for (int k = 0; k < SZ_CH / 256; ++k) {
      const bool fast = act[k] && slots[k] == key0;
      local += fast ? 1u : 0u;
      wave_agg_add(F.csize, act[k] && !fast, slots[k]);
    }
    for (int off = 32; off > 0; off >>= 1) local += __shfl_xor((int)local, off, 64);
    if (lane == 0) s_part[wave] = local;
    __syncthreads();
    if (threadIdx.x == 0 && key0 != NOCLAIM) atomicAdd(&F.csize[key0], s_part[0] + s_part[1] + s_part[2] + s_part[3]);
    __syncthreads();
  }
}

// flags (all claimed cells + all NQ seeds), kept-cluster list, per-cell kept slot
__global__ void __launch_bounds__(256) k_finalize(Geo g, FArgs F) {
  if ((int)blockIdx.x >= F.var->nblocks) return;
  const int rel = blockIdx.x * 256 + threadIdx.x;
  const int w = F.var->w0 + rel;
  if (w >= g.W) return;
  u64 q = F.qb[w], s = F.sb[w];
  if ((q | s) == 0ull) return;
  const u32 nq = F.counts[0];
  u64 pk = F.blockscan[rel >> 8] + F.pref[rel];
  u32 iq = (u32)pk, is = (u32)(pk >> 32);
  u64 newflag = s;
  u64 qq = q;
  while (qq) {
    int b = __builtin_ctzll(qq);
    qq &= qq - 1;
    if (iq < F.cap_q) {
      int slot = F.cell_slot[iq];
      if (slot >= 0) {
        newflag |= 1ull << b;
        u32 sz = F.csize[slot];
        if ((int)sz > F.cluster_min) {
          if ((u32)slot == iq) {  // this cell is the own claimer of a kept cluster
            u32 k = atomicAdd(&F.counts[3], 1u);
            if (k < F.cap_kept) {
              F.kept[3 * k] = (u32)(64L * w + b);
              F.kept[3 * k + 1] = (u32)slot;
              F.kept[3 * k + 2] = sz;
            }
          }
        } else
          F.cell_slot[iq] = -1;
      }
    }
    ++iq;
  }
  u64 ss = s;
  while (ss) {
    int b = __builtin_ctzll(ss);
    ss &= ss - 1;
    if (is < F.cap_s) {
      u32 slot = nq + is;
      u32 sz = F.csize[slot];
      if ((int)sz > F.cluster_min) {
        u32 k = atomicAdd(&F.counts[3], 1u);
        if (k < F.cap_kept) {
          F.kept[3 * k] = (u32)(64L * w + b);
          F.kept[3 * k + 1] = slot;
          F.kept[3 * k + 2] = sz;
        }
      }
    }
    ++is;
  }
  F.flag[w] |= newflag;
}

// ---- grouping of kept cells by cluster: stable radix multisplit ---------------------------------
// Every size (nq, nkept, n_out, digits, chunk counts) is read from device memory, so the whole tail
// is enqueued without a host round trip; grids are launched at their upper bound and surplus
// blocks exit at once.  counts[]: [0]=nq [1]=ns [2]=overflow [3]=nkept [4]=scratch [5]=n_out.

// rank the kept clusters by claimer address (= the reference's creation order) and lay out the
// grouped cell array: rank_i = #{j : addr_j < addr_i}, off_i = sum of their cell counts.
__global__ void __launch_bounds__(256) k_rank_kept(FArgs F) {
  const u32 nq = F.counts[0];
  const u32 nkept = min(F.counts[3], F.cap_kept);
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < nkept; i += gridDim.x * blockDim.x) {
    const u32 ai = F.kept[3 * i], si = F.kept[3 * i + 1], zi = F.kept[3 * i + 2];
    u32 rank = 0, off = 0;
    for (u32 j = 0; j < nkept; ++j) {
      const u32 aj = F.kept[3 * j];
      if (aj < ai) {
        ++rank;
        off += F.kept[3 * j + 2] - (F.kept[3 * j + 1] >= nq ? 1u : 0u);  // an NQ seed is not a Q0 cell
      }
    }
    F.slot2rank[si] = (int)rank;
    KeptRec& r = F.krec[rank];
    r.addr = ai, r.slot = si, r.size = zi, r.off = off;
    r.sum[0] = r.sum[1] = r.sum[2] = 0ull;
    for (int k = 0; k < 3; ++k) r.box[k] = 0xFFFFFFFFu, r.box[3 + k] = 0u;
    if (rank == nkept - 1) F.counts[5] = off + zi - (si >= nq ? 1u : 0u);
  }
}
struct MsPass {
  bool on;
  u32 n;
  int nb, ndig, shift;
  const u32 *key, *val;
  u32 *key_out, *val_out;
};
__device__ __forceinline__ MsPass ms_pass(const FArgs& F, int pass) {
  MsPass p;
  const u32 nkept = min(F.counts[3], F.cap_kept);
  p.on = nkept > 0 && (pass == 0 || nkept > 256);
  p.n = pass == 0 ? F.counts[0] : F.counts[5];
  p.nb = (int)((p.n + MS_CH - 1) / MS_CH);
  p.ndig = pass == 0 ? (int)min(nkept, 256u) : (int)((nkept - 1) >> 8) + 1;
  p.shift = 8 * pass;
  p.key = F.ms_key[pass], p.val = F.ms_val[pass];
  p.key_out = F.ms_key[1 - pass], p.val_out = F.ms_val[1 - pass];
  return p;
}
// (key, value) of input item i: pass 0 of the clustering chain derives them from the per-cell slot
// (what a separate k_ms_keys launch used to materialise); otherwise they are read from the buffers
__device__ __forceinline__ u32 ms_key_at(const FArgs& F, const MsPass& P, int pass, u32 i) {
  if (pass == 0 && F.keys_from_slots) {
    const int s = F.cell_slot[i];
    return s >= 0 ? (u32)F.slot2rank[s] : NOKEY;
  }
  return P.key[i];
}
__device__ __forceinline__ u32 ms_val_at(const FArgs& F, const MsPass& P, int pass, u32 i) {
  return (pass == 0 && F.keys_from_slots) ? F.cell_adr[i] : P.val[i];
}
// in-place exclusive scan of the ndig*nb histogram entries (one block)
__device__ void ms_scan_tail(const FArgs& F, const MsPass& P) {
  __shared__ u32 part[1024];
  u32* v = F.ms_hist;
  const int T = blockDim.x;
  const int cnt = P.ndig * P.nb;
  const int per = (cnt + T - 1) / T;
  const int b0 = threadIdx.x * per, b1 = min(cnt, b0 + per);
  u32 s = 0;
  for (int b = b0; b < b1; ++b) s += v[b];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < T; off <<= 1) {  // Hillis-Steele over the per-thread partials
    const u32 x = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
    __syncthreads();
    part[threadIdx.x] += x;
    __syncthreads();
  }
  u32 run = part[threadIdx.x] - s;
  for (int b = b0; b < b1; ++b) {
    u32 x = v[b];
    v[b] = run;
    run += x;
  }
}
// histogram of the current 8-bit digit per block, digit-major: hist[d * nb + block]
__global__ void __launch_bounds__(256) k_ms_hist(FArgs F, int pass) {
  __shared__ u32 h[256];
  const MsPass P = ms_pass(F, pass);
  if (!P.on) return;
  for (int chunk = blockIdx.x; chunk < P.nb; chunk += gridDim.x) {  // any grid size covers all chunks
    h[threadIdx.x] = 0;
    __syncthreads();
    const u32 base = (u32)chunk * MS_CH;
    for (int k = 0; k < MS_CH / 256; ++k) {
      u32 i = base + k * 256 + threadIdx.x;
      if (i < P.n) {
        u32 kk = ms_key_at(F, P, pass, i);
        if (kk != NOKEY) atomicAdd(&h[(kk >> P.shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < P.ndig) F.ms_hist[threadIdx.x * P.nb + chunk] = h[threadIdx.x];
    __syncthreads();
  }
}
__global__ void __launch_bounds__(1024) k_ms_scan(FArgs F, int pass) {
  const MsPass P = ms_pass(F, pass);
  if (P.on) ms_scan_tail(F, P);
}
// stable scatter: position = scanned[d][block] + (# earlier elements of this block with digit d)
__global__ void __launch_bounds__(256) k_ms_scatter(FArgs F, int pass) {
  __shared__ u32 running[256];
  __shared__ u32 wcnt[4][256];
  const MsPass P = ms_pass(F, pass);
  if (!P.on) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int chunk = blockIdx.x; chunk < P.nb; chunk += gridDim.x) {
  running[threadIdx.x] = (int)threadIdx.x < P.ndig ? F.ms_hist[threadIdx.x * P.nb + chunk] : 0u;
  const u32 base = (u32)chunk * MS_CH;
  for (int k = 0; k < MS_CH / 256; ++k) {
    for (int w = 0; w < 4; ++w) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    const u32 i = base + k * 256 + threadIdx.x;
    u32 kk = (i < P.n) ? ms_key_at(F, P, pass, i) : NOKEY;
    const bool active = kk != NOKEY;
    const u32 d = (kk >> P.shift) & 255u;
    u32 lane_rank = 0;
    u64 todo = __ballot(active);
    while (todo) {
      int leader = __builtin_ctzll(todo);
      u32 dl = __shfl(d, leader, 64);
      u64 same = __ballot(active && d == dl) & todo;
      if (active && d == dl) lane_rank = (u32)__popcll(same & ((1ull << lane) - 1ull));
      if (lane == leader) wcnt[wave][dl] = (u32)__popcll(same);
      todo &= ~same;
    }
    __syncthreads();
    if (active) {
      u32 pos = running[d] + lane_rank;
      for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
      P.key_out[pos] = kk;
      P.val_out[pos] = ms_val_at(F, P, pass, i);
    }
    __syncthreads();
    running[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
    __syncthreads();
  }
  }
}
// computeFrontierInfo (:374-390) accumulators per cluster: sum of voxel indices and index AABB.
// Input is grouped by cluster, so a 1024-cell chunk nearly always holds one key: reduce it in the
// block into a per-chunk record (folded on the host); cells of other keys (a chunk straddling a
// cluster boundary) are reduced per wave and added to the cluster record with atomics.
__device__ __forceinline__ void info_atomics(FArgs& F, u32 k, u32 sx, u32 sy, u32 sz, u32 nx_, u32 ny_, u32 nz_,
                                             u32 mx, u32 my, u32 mz) {
  KeptRec& r = F.krec[k];
  atomicAdd(&r.sum[0], (unsigned long long)sx);
  atomicAdd(&r.sum[1], (unsigned long long)sy);
  atomicAdd(&r.sum[2], (unsigned long long)sz);
  atomicMin(&r.box[0], nx_);
  atomicMin(&r.box[1], ny_);
  atomicMin(&r.box[2], nz_);
  atomicMax(&r.box[3], mx);
  atomicMax(&r.box[4], my);
  atomicMax(&r.box[5], mz);
}
// counts + cluster records -> pinned host memory (one block, after k_ms_info's atomics on the records)
__device__ void pack_tail(const FArgs& F) {
  const u32 nkept = min(F.counts[3], F.cap_kept);
  const u32 words = nkept * (u32)(sizeof(KeptRec) / 4);
  const u32* src = reinterpret_cast<const u32*>(F.krec);
  u32* dst = reinterpret_cast<u32*>(F.h_rec);
  for (u32 i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
  if (threadIdx.x < 16) F.h_counts[threadIdx.x] = F.counts[threadIdx.x];
}
__global__ void __launch_bounds__(256) k_ms_info(Geo g, FArgs F) {
  __shared__ u32 s_red[4][9];
  const u32 nkept = min(F.counts[3], F.cap_kept);
  if (nkept == 0) return;
  const int fin = nkept <= 256 ? 1 : 0;  // buffer holding the grouped output
  const u32* key = F.ms_key[fin];
  const u32* val = F.ms_val[fin];
  const u32 n = F.counts[5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (u32 base = blockIdx.x * SZ_CH; base < n; base += gridDim.x * SZ_CH) {
    const u32 key0 = key[base];
    u32 sx = 0, sy = 0, sz = 0, nx_ = 0xFFFFFFFFu, ny_ = 0xFFFFFFFFu, nz_ = 0xFFFFFFFFu, mx = 0, my = 0, mz = 0;
#pragma unroll
    for (int k = 0; k < SZ_CH / 256; ++k) {
      const u32 i = base + k * 256 + threadIdx.x;
      u32 kk = i < n ? key[i] : key0;
      // keys >= nkept can only appear when the radix-pass estimate was wrong and this buffer is not
      // the grouped one yet (the host then re-runs the grouping and this kernel): ignore them
      const bool in = i < n && kk < nkept;
      const u32 a = in ? val[i] : 0u;
      if (i < n) F.h_cells[i] = a;  // posted write over PCIe, 16 B.. 256 B per wave, coalesced
      const u32 x = a / (u32)g.nyz, r = a - x * (u32)g.nyz, y = r / (u32)g.nz, z = r - y * (u32)g.nz;
      if (in && kk == key0) {
        sx += x, sy += y, sz += z;
        nx_ = min(nx_, x), ny_ = min(ny_, y), nz_ = min(nz_, z);
        mx = max(mx, x), my = max(my, y), mz = max(mz, z);
      }
      u64 todo = __ballot(in && kk != key0);
      while (todo) {
        const int leader = __builtin_ctzll(todo);
        const u32 kl = (u32)__shfl((int)kk, leader, 64);
        const bool mine = in && kk == kl;
        const u64 same = __ballot(mine) & todo;
        u32 tx = mine ? x : 0, ty = mine ? y : 0, tz = mine ? z : 0;
        u32 ax = mine ? x : 0xFFFFFFFFu, ay = mine ? y : 0xFFFFFFFFu, az = mine ? z : 0xFFFFFFFFu;
        u32 bx = tx, by = ty, bz = tz;
        for (int off = 32; off > 0; off >>= 1) {
          tx += __shfl_xor((int)tx, off, 64);
          ty += __shfl_xor((int)ty, off, 64);
          tz += __shfl_xor((int)tz, off, 64);
          ax = min(ax, (u32)__shfl_xor((int)ax, off, 64));
          ay = min(ay, (u32)__shfl_xor((int)ay, off, 64));
          az = min(az, (u32)__shfl_xor((int)az, off, 64));
          bx = max(bx, (u32)__shfl_xor((int)bx, off, 64));
          by = max(by, (u32)__shfl_xor((int)by, off, 64));
          bz = max(bz, (u32)__shfl_xor((int)bz, off, 64));
        }
        if (lane == leader) info_atomics(F, kl, tx, ty, tz, ax, ay, az, bx, by, bz);
        todo &= ~same;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      sx += __shfl_xor((int)sx, off, 64);
      sy += __shfl_xor((int)sy, off, 64);
      sz += __shfl_xor((int)sz, off, 64);
      nx_ = min(nx_, (u32)__shfl_xor((int)nx_, off, 64));
      ny_ = min(ny_, (u32)__shfl_xor((int)ny_, off, 64));
      nz_ = min(nz_, (u32)__shfl_xor((int)nz_, off, 64));
      mx = max(mx, (u32)__shfl_xor((int)mx, off, 64));
      my = max(my, (u32)__shfl_xor((int)my, off, 64));
      mz = max(mz, (u32)__shfl_xor((int)mz, off, 64));
    }
    if (lane == 0) {
      u32* q = s_red[wave];
      q[0] = sx, q[1] = sy, q[2] = sz, q[3] = nx_, q[4] = ny_, q[5] = nz_, q[6] = mx, q[7] = my, q[8] = mz;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; ++w) {
        sx += s_red[w][0], sy += s_red[w][1], sz += s_red[w][2];
        nx_ = min(nx_, s_red[w][3]), ny_ = min(ny_, s_red[w][4]), nz_ = min(nz_, s_red[w][5]);
        mx = max(mx, s_red[w][6]), my = max(my, s_red[w][7]), mz = max(mz, s_red[w][8]);
      }
      u32* rec = F.h_part + (size_t)(base / SZ_CH) * 10;
      rec[0] = key0, rec[1] = sx, rec[2] = sy, rec[3] = sz;
      rec[4] = nx_, rec[5] = ny_, rec[6] = nz_, rec[7] = mx, rec[8] = my, rec[9] = mz;
    }
    __syncthreads();
  }
}
__global__ void __launch_bounds__(256) k_pack(FArgs F) { pack_tail(F); }

__global__ void k_load_var(const FVar* __restrict__ h, FVar* __restrict__ d) {
  const int n = (int)(sizeof(FVar) / 4);
  if ((int)threadIdx.x < n) reinterpret_cast<u32*>(d)[threadIdx.x] = reinterpret_cast<const u32*>(h)[threadIdx.x];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// passes p0 .. p1 - 1 of the radix multisplit on A (the kernels stride over however many 2048-cell chunks there are)
static void enqueue_ms_passes(fuelmi_frontier* f, const FArgs& A, int p0, int p1) {
  for (int p = p0; p < p1; ++p) {
    k_ms_hist<<<256, 256, 0, f->stream>>>(A, p);
    FDBG("k_ms_hist");
    k_ms_scan<<<1, 1024, 0, f->stream>>>(A, p);
    FDBG("k_ms_scan");
    k_ms_scatter<<<256, 256, 0, f->stream>>>(A, p);
    FDBG("k_ms_scatter");
  }
}

int frontier_regroup(fuelmi_frontier* f, const FArgs& F2, int npass) {
  const Geo& g = f->map->g;
  enqueue_ms_passes(f, F2, 0, npass);
  k_ms_info<<<256, 256, 0, f->stream>>>(g, F2);
  FDBG("k_ms_info");
  k_pack<<<1, 256, 0, f->stream>>>(F2);
  FDBG("k_pack");
  HIPCHK(hipGetLastError());
  return FUELMI_OK;
}

// the device pipeline of one search (all on f->stream; capturable)
int frontier_enqueue_chain(fuelmi_frontier* f, int npass) {
  const Geo& g = f->map->g;
  FArgs& F = f->F;
  const int nb_max = (g.W + 255) / 256 + 1;  // surplus blocks exit on F.var->nblocks
  const int cgrid = 2048;
  // (the CURRENT buffer set's copy: a reset swaps F and F2, each with a device FVar of its own -- ADVICE r4)
  k_load_var<<<1, 64, 0, f->stream>>>(f->h_var, F.var_w);
  FDBG("k_load_var");
  k_pred<<<nb_max, 256, 0, f->stream>>>(g, F);
  FDBG("k_pred");
  k_scan_sums<<<1, 1024, 0, f->stream>>>(F);
  FDBG("k_scan_sums");
  k_compact<<<nb_max, 256, 0, f->stream>>>(g, F);
  FDBG("k_compact");
  if (f->ccl_tiles > 0) {
    // 512 threads per tile: the busiest tiles (a wall of ~2000 cells) set the kernel's duration, and their
    // cells are independent chains of LDS unions (measured 29.5 -> 24.1 us on G400; 1024 loses occupancy)
    k_ccl_local<512><<<f->ccl_tiles, 512, f->ccl_lds, f->stream>>>(g, F, f->TX, f->TY);
    FDBG("k_ccl_local");
    k_union<<<cgrid, 256, 0, f->stream>>>(g, F, f->TX, f->TY);
    FDBG("k_union");
  }
  k_claim<<<cgrid, 256, 0, f->stream>>>(g, F);
  FDBG("k_claim");
  k_sizes<<<cgrid, 256, 0, f->stream>>>(g, F);
  FDBG("k_sizes");  // grid-stride over 1024-cell chunks
  k_finalize<<<nb_max, 256, 0, f->stream>>>(g, F);
  FDBG("k_finalize");
  // ---- grouping + cluster info, still without touching the host ----
  k_rank_kept<<<16, 256, 0, f->stream>>>(F);
  FDBG("k_rank_kept");
  return frontier_regroup(f, F, npass);
}

// more than 256 clusters but only one radix pass was enqueued: run the high-digit pass now, and wait for it
int frontier_second_pass(fuelmi_frontier* f) {
  const Geo& g = f->map->g;
  FArgs& F = f->F;
  enqueue_ms_passes(f, F, 1, 2);
  // cluster records must be re-initialised before the accumulators are refilled
  k_rank_kept<<<16, 256, 0, f->stream>>>(F);
  FDBG("k_rank_kept");
  k_ms_info<<<256, 256, 0, f->stream>>>(g, F);
  FDBG("k_ms_info");
  k_pack<<<1, 256, 0, f->stream>>>(F);
  FDBG("k_pack");
  HIPCHK(hipStreamSynchronize(f->stream));
  return FUELMI_OK;
}

// the chain as _search_begin queues it: replayed as a hipGraph, captured once per radix pass count and flag plane
// (FUELMI_DEBUG_SYNC: direct launches, synchronised and named one by one)
int frontier_launch_legacy(fuelmi_frontier* f, int npass) {
  static const bool no_graph = getenv("FUELMI_DEBUG_SYNC") != nullptr;
  if (no_graph) return frontier_enqueue_chain(f, npass);
  hipGraphExec_t& exec = f->graph_exec[npass - 1][f->flag_cur];
  if (!exec) {
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(f->stream, hipStreamCaptureModeThreadLocal));
    const int rc2 = frontier_enqueue_chain(f, npass);
    const hipError_t ec = hipStreamEndCapture(f->stream, &graph);
    if (rc2) return rc2;
    HIPCHK(ec);
    HIPCHK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    HIPCHK(hipGraphDestroy(graph));
  }
  HIPCHK(hipGraphLaunch(exec, f->stream));
  return FUELMI_OK;
}

// the dynamic LDS ceiling of k_ccl_local for the finder's CCL tile (f->ccl_lds, fuelmi_frontier_create)
int frontier_legacy_attrs(fuelmi_frontier* f) {
  if (f->ccl_lds > 64 * 1024) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ccl_local<512>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)f->ccl_lds));
  }
  return FUELMI_OK;
}
