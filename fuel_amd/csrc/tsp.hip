// tsp.hip -- batched ATSP solver for the global exploration tour (include/fuelmi.h "Global tour").
//
// The reference writes getFullCostMatrix as int(cost * 100) to a TSPLIB file and runs LKH-2 on it
// (exploration_manager/src/fast_exploration_manager.cpp:327-420).  Here a solver object owns a stream and a
// grow-only workspace and answers a batch of int32 matrices in one call:
//   k_tsp_transpose  the transposed matrix of every problem (the Or-opt insertion reads columns as rows)
//   k_tsp_exact      Held-Karp, one 1024-lane workgroup per problem with d - 1 <= exact_max (suffix DP over
//                    popcount layers, table in the workspace), then the forward construction of the
//                    lexicographically smallest optimal order by lane 0
//   k_tsp_ils        the iterated local search, one 512-lane workgroup per (problem, restart): nearest-neighbour
//                    start, best-improvement 2-opt + Or-opt, double-bridge kicks drawn from splitmix64
//   k_tsp_pick       the cheapest restart of every heuristic problem (smallest r on ties)
// Every rule (enumeration order, tie key, hash, acceptance) is the header's; tests/tsp_ref.py restates them.
#include "fuelmi_internal.h"

#include <algorithm>
#include <climits>
#include <cstring>

#define TSP_ILS_THREADS 512
#define TSP_EXACT_THREADS 1024
#define TSP_TABLE_CHUNK (64ull << 20)  // Held-Karp tables of one launch (eight 8 MiB tables at the cap)

struct TspProb {
  long long off;   // first matrix entry (row-major int32) in the concatenated matrices
  long long tbl;   // exact: first int64 of its Held-Karp table in the chunk; heuristic: first restart order (ints)
  int d;
  int oout;        // first entry of its order in the concatenated output
  int task0;       // heuristic: first (problem, restart) task
};

struct fuelmi_tsp {
  int device = 0;
  fuelmi_tsp_cfg cfg;
  hipStream_t stream = nullptr;
  void* dev = nullptr;  // device workspace (grow-only)
  size_t dev_bytes = 0;
  void* pin = nullptr;  // pinned staging of the matrices in and the results out (grow-only)
  size_t pin_bytes = 0;
};

// ---- device helpers -----------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 tsp_mix(u64 z) {  // splitmix64's finaliser (with its increment)
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// lexicographic minimum of (v, k) over the workgroup (8 waves of 64); every lane returns the result
__device__ __forceinline__ void blk_min(long long& v, int& k, long long* sv, int* sk) {
  for (int o = 32; o > 0; o >>= 1) {
    const long long ov = (long long)__shfl_xor((long)v, o, 64);
    const int ok = __shfl_xor(k, o, 64);
    if (ov < v || (ov == v && ok < k)) v = ov, k = ok;
  }
  const int w = threadIdx.x >> 6;
  __syncthreads();  // the previous reduction's readers are done with sv / sk
  if ((threadIdx.x & 63) == 0) sv[w] = v, sk[w] = k;
  __syncthreads();
  v = sv[0], k = sk[0];
  for (int i = 1; i < TSP_ILS_THREADS / 64; ++i)
    if (sv[i] < v || (sv[i] == v && sk[i] < k)) v = sv[i], k = sk[i];
}

// ---- transposed copies ----------------------------------------------------------------------------------------------
// (the heuristic problems ids[0 .. n_prob-1] only)
__global__ void k_tsp_transpose(const int* __restrict__ mat, int* __restrict__ matT, const TspProb* __restrict__ pr,
                                const int* __restrict__ ids, int n_prob) {
  for (int b = blockIdx.y; b < n_prob; b += gridDim.y) {
    const TspProb P = pr[ids[b]];
    const int d = P.d;
    const long long n = (long long)d * d;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
      const int i = (int)(t / d), j = (int)(t - (long long)i * d);
      matT[P.off + (long long)j * d + i] = mat[P.off + t];
    }
  }
}

// ---- Held-Karp --------------------------------------------------------------------------------------------------------
// g(S, j), S a set of the non-start nodes 1..n (bit j-1), j in S the node the tour stands at: the cheapest way to visit
// the rest and close at 0.  Table index S * n + (j - 1); layers by popcount, largest first.
__global__ void __launch_bounds__(TSP_EXACT_THREADS) k_tsp_exact(const int* __restrict__ mat, const TspProb* __restrict__ pr,
                                                                 const int* __restrict__ ids, long long* __restrict__ tbl,
                                                                 int* __restrict__ out_order, long long* __restrict__ out_cost) {
  const TspProb P = pr[ids[blockIdx.x]];
  const int d = P.d, n = d - 1;
  __shared__ int c[17 * 17];
  for (int t = threadIdx.x; t < d * d; t += blockDim.x) c[t] = mat[P.off + t];
  __syncthreads();
  if (n == 0) {
    if (threadIdx.x == 0) out_order[P.oout] = 0, out_cost[ids[blockIdx.x]] = 0;
    return;
  }
  long long* g = tbl + P.tbl;
  const u32 full = (1u << n) - 1;
  for (int p = n; p >= 1; --p) {
    for (u32 S = threadIdx.x; S <= full; S += blockDim.x) {
      if (__popc(S) != p) continue;
      for (int j = 0; j < n; ++j) {
        if (!(S >> j & 1)) continue;
        long long best;
        if (S == full) {
          best = c[(j + 1) * d];
        } else {
          best = LLONG_MAX;
          for (int k = 0; k < n; ++k) {
            if (S >> k & 1) continue;
            const long long v = (long long)c[(j + 1) * d + k + 1] + g[(size_t)(S | 1u << k) * n + k];
            best = v < best ? v : best;
          }
        }
        g[(size_t)S * n + j] = best;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  // forward construction: at every step the smallest j that keeps the optimum
  long long target = LLONG_MAX;
  for (int j = 0; j < n; ++j) {
    const long long v = (long long)c[j + 1] + g[(size_t)(1u << j) * n + j];
    target = v < target ? v : target;
  }
  out_cost[ids[blockIdx.x]] = target;
  out_order[P.oout] = 0;
  u32 S = 0;
  int last = 0;
  for (int step = 1; step <= n; ++step) {
    for (int j = 0; j < n; ++j) {
      if (S >> j & 1) continue;
      const long long gj = g[(size_t)(S | 1u << j) * n + j];
      if ((long long)c[last * d + j + 1] + gj == target) {
        S |= 1u << j;
        last = j + 1;
        target = gj;
        out_order[P.oout + step] = last;
        break;
      }
    }
  }
}

// ---- iterated local search -----------------------------------------------------------------------------------------
struct IlsLds {
  int ord[FUELMI_TSP_MAX_DIM];  // current tour
  int bst[FUELMI_TSP_MAX_DIM];  // the restart's best tour
  int tmp[FUELMI_TSP_MAX_DIM];  // rebuilds; visited flags of the nearest-neighbour start
  long long F[FUELMI_TSP_MAX_DIM + 1];  // F[k] = sum_{t<k} c[ord[t]][ord[t+1 mod d]]
  long long B[FUELMI_TSP_MAX_DIM];      // B[k] = sum_{t<k} c[ord[t+1]][ord[t]]
  long long sf[TSP_ILS_THREADS], sb[TSP_ILS_THREADS];
  long long rv[TSP_ILS_THREADS / 64];
  int rk[TSP_ILS_THREADS / 64];
};

// F and B of the current tour (the thread's chunk of at most 4 positions, then a Hillis-Steele scan of the chunk sums)
__device__ void ils_prefix(const int* __restrict__ c, int d, IlsLds& L) {
  const int tid = threadIdx.x;
  const int ch = (d + TSP_ILS_THREADS - 1) / TSP_ILS_THREADS;
  const int x0 = min(d, tid * ch), x1 = min(d, x0 + ch);
  long long ef[4], eb[4], sf = 0, sb = 0;
  for (int x = x0; x < x1; ++x) {
    const int a = L.ord[x], b = L.ord[x + 1 == d ? 0 : x + 1];
    ef[x - x0] = c[(size_t)a * d + b];
    eb[x - x0] = x + 1 < d ? (long long)c[(size_t)b * d + a] : 0;
    sf += ef[x - x0], sb += eb[x - x0];
  }
  L.sf[tid] = sf, L.sb[tid] = sb;
  __syncthreads();
  for (int o = 1; o < TSP_ILS_THREADS; o <<= 1) {
    const long long af = tid >= o ? L.sf[tid - o] : 0, ab = tid >= o ? L.sb[tid - o] : 0;
    __syncthreads();
    L.sf[tid] += af, L.sb[tid] += ab;
    __syncthreads();
  }
  long long rf = L.sf[tid] - sf, rb = L.sb[tid] - sb;
  if (tid == 0) L.F[0] = 0, L.B[0] = 0;
  for (int x = x0; x < x1; ++x) {
    rf += ef[x - x0], rb += eb[x - x0];
    L.F[x + 1] = rf;
    if (x + 1 < d) L.B[x + 1] = rb;
  }
  __syncthreads();
}

// best-improvement descent; returns the tour's cost
__device__ long long ils_descend(const int* __restrict__ c, const int* __restrict__ cT, int d, IlsLds& L) {
  const int tid = threadIdx.x;
  const int n2 = d - 2;                       // 2-opt rows: i = 1 .. d-2
  const u32 rows = (u32)n2 + 6u * (u32)(d - 1);  // then Or-opt rows (s, L, rev)
  const u32 total = rows * (u32)d;
  const float invd = 1.0f / (float)d;
  const int D1 = d * d * 6;                   // first Or-opt key
  for (;;) {
    ils_prefix(c, d, L);
    long long bd = 0;  // only strictly negative deltas are kept
    int bk = INT_MAX;
    for (u32 t = tid; t < total; t += TSP_ILS_THREADS) {
      u32 row = (u32)(((float)t + 0.5f) * invd);
      if (row * (u32)d > t) --row;
      else if ((row + 1) * (u32)d <= t) ++row;
      const int col = (int)(t - row * (u32)d);
      long long delta;
      int key;
      if ((int)row < n2) {  // 2-opt: reverse ord[i..j]
        const int i = (int)row + 1, j = col;
        if (j <= i) continue;
        const int a = L.ord[i - 1], b = L.ord[i], e = L.ord[j], f = L.ord[j + 1 == d ? 0 : j + 1];
        delta = (long long)c[(size_t)a * d + e] + c[(size_t)b * d + f] - (L.F[i] - L.F[i - 1]) - (L.F[j + 1] - L.F[j]) +
                (L.B[j] - L.B[i]) - (L.F[j] - L.F[i]);
        key = i * (d * 6) + j * 6;
      } else {  // Or-opt: move ord[s .. s+len-1] into gap g (after position g), forward or reversed
        const int r2 = (int)row - n2, rev = r2 & 1, q = r2 >> 1, len = q % 3 + 1, s = q / 3 + 1, g = col;
        const int e = s + len - 1;
        if (e > d - 1 || (rev && len == 1) || (g >= s - 1 && g <= e)) continue;
        const int first = L.ord[s], last = L.ord[e], p = L.ord[s - 1], nx = L.ord[e + 1 == d ? 0 : e + 1];
        const int u = L.ord[g], v = L.ord[g + 1 == d ? 0 : g + 1];
        const long long rem = (L.F[s] - L.F[s - 1]) + (L.F[e + 1] - L.F[e]) - c[(size_t)p * d + nx];
        const long long gap = L.F[g + 1] - L.F[g];
        if (!rev)
          delta = (long long)cT[(size_t)first * d + u] + c[(size_t)last * d + v] - gap - rem;
        else
          delta = (long long)cT[(size_t)last * d + u] + c[(size_t)first * d + v] - gap + (L.B[e] - L.B[s]) -
                  (L.F[e] - L.F[s]) - rem;
        key = D1 + s * (d * 6) + g * 6 + (len - 1) * 2 + rev;
      }
      if (delta < bd || (delta == bd && key < bk)) bd = delta, bk = key;
    }
    blk_min(bd, bk, L.rv, L.rk);
    if (bd >= 0) return L.F[d];
    if (bk < D1) {
      const int i = bk / (d * 6), j = (bk - i * d * 6) / 6;
      for (int x = tid; x < (j - i + 1) / 2; x += TSP_ILS_THREADS) {
        const int t0 = L.ord[i + x];
        L.ord[i + x] = L.ord[j - x];
        L.ord[j - x] = t0;
      }
    } else {
      const int r = bk - D1, s = r / (d * 6), g = (r - s * d * 6) / 6, k = r % 6, len = k / 2 + 1, rev = k & 1;
      const int gp = g < s ? g : g - len;  // the gap's position once the segment is out
      for (int q = tid; q < d; q += TSP_ILS_THREADS) {
        int src;
        if (q <= gp) src = q < s ? q : q + len;
        else if (q <= gp + len) src = s + (rev ? len - 1 - (q - gp - 1) : q - gp - 1);
        else src = q - len < s ? q - len : q;
        L.tmp[q] = L.ord[src];
      }
      __syncthreads();
      for (int q = tid; q < d; q += TSP_ILS_THREADS) L.ord[q] = L.tmp[q];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(TSP_ILS_THREADS) k_tsp_ils(const int* __restrict__ mat, const int* __restrict__ matT,
                                                             const TspProb* __restrict__ pr, const int2* __restrict__ tasks,
                                                             int kicks, u64 seed, long long* __restrict__ rcost,
                                                             int* __restrict__ rorder) {
  __shared__ IlsLds L;
  const int2 tk = tasks[blockIdx.x];
  const TspProb P = pr[tk.x];
  const int d = P.d, r = tk.y, tid = threadIdx.x;
  const int* c = mat + P.off;
  const int* cT = matT + P.off;
  // nearest neighbour from 0, ties to the smallest index
  for (int q = tid; q < d; q += TSP_ILS_THREADS) L.tmp[q] = q == 0;
  if (tid == 0) L.ord[0] = 0;
  __syncthreads();
  for (int step = 1; step < d; ++step) {
    const int last = L.ord[step - 1];
    long long bv = LLONG_MAX;
    int bj = INT_MAX;
    for (int j = tid; j < d; j += TSP_ILS_THREADS) {
      if (L.tmp[j]) continue;
      const long long v = c[(size_t)last * d + j];
      if (v < bv) bv = v, bj = j;
    }
    blk_min(bv, bj, L.rv, L.rk);
    if (tid == 0) L.ord[step] = bj, L.tmp[bj] = 1;
    __syncthreads();
  }
  long long best = ils_descend(c, cT, d, L);
  for (int q = tid; q < d; q += TSP_ILS_THREADS) L.bst[q] = L.ord[q];
  __syncthreads();
  const u64 m = (u64)(d - 1);
  for (int k = 0; k < kicks; ++k) {
    // double bridge A C B D at 1 <= p1 < p2 < p3 <= d-1 (every lane draws the same points)
    const u64 h = tsp_mix(seed ^ tsp_mix(((u64)(unsigned)r << 32) | (u64)(unsigned)k));
    int pt[3], got = 0;
    for (u64 t = 0; got < 3; ++t) {
      const int x = 1 + (int)(tsp_mix(h + t) % m);
      bool dup = false;
      for (int y = 0; y < got; ++y) dup |= pt[y] == x;
      if (!dup) pt[got++] = x;
    }
    const int p1 = min(pt[0], min(pt[1], pt[2])), p3 = max(pt[0], max(pt[1], pt[2]));
    const int p2 = pt[0] + pt[1] + pt[2] - p1 - p3;
    for (int q = tid; q < d; q += TSP_ILS_THREADS) {
      int src = q;
      if (q >= p1 && q < p3) src = q < p1 + (p3 - p2) ? p2 + (q - p1) : p1 + (q - p1 - (p3 - p2));
      L.ord[q] = L.bst[src];
    }
    __syncthreads();
    const long long cost = ils_descend(c, cT, d, L);
    if (cost < best) {  // keep; otherwise back to the best tour
      best = cost;
      for (int q = tid; q < d; q += TSP_ILS_THREADS) L.bst[q] = L.ord[q];
    }
    __syncthreads();
  }
  int* o = rorder + P.tbl + (long long)r * d;
  for (int q = tid; q < d; q += TSP_ILS_THREADS) o[q] = L.bst[q];
  if (tid == 0) rcost[blockIdx.x] = best;
}

__global__ void k_tsp_pick(const TspProb* __restrict__ pr, const int* __restrict__ ids, int restarts,
                           const long long* __restrict__ rcost, const int* __restrict__ rorder, int* __restrict__ out_order,
                           long long* __restrict__ out_cost) {
  const int b = ids[blockIdx.x];
  const TspProb P = pr[b];
  __shared__ int rbest;
  if (threadIdx.x == 0) {
    int rb = 0;
    for (int r = 1; r < restarts; ++r)
      if (rcost[P.task0 + r] < rcost[P.task0 + rb]) rb = r;
    rbest = rb;
    out_cost[b] = rcost[P.task0 + rb];
  }
  __syncthreads();
  const int* src = rorder + P.tbl + (long long)rbest * P.d;
  for (int q = threadIdx.x; q < P.d; q += blockDim.x) out_order[P.oout + q] = src[q];
}

// ---- host -----------------------------------------------------------------------------------------------------------
static int tsp_cfg_check(const fuelmi_tsp_cfg* c) {
  if (c->restarts < 1 || c->kicks < 0 || c->exact_max < 3 || c->exact_max > FUELMI_TSP_EXACT_CAP) {
    fuelmi_set_error("fuelmi_tsp: restarts %d (>= 1), kicks %d (>= 0), exact_max %d (3 .. %d)", c->restarts, c->kicks,
                     c->exact_max, FUELMI_TSP_EXACT_CAP);
    return FUELMI_EINVAL;
  }
  return FUELMI_OK;
}

extern "C" int fuelmi_tsp_create(int device, const fuelmi_tsp_cfg* cfg, fuelmi_tsp** out) {
  ARGCHK(cfg && out);
  const int rc = tsp_cfg_check(cfg);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    fuelmi_set_error("no HIP device available: libfuelmi has no CPU fallback");
    return FUELMI_ENODEV;
  }
  ARGCHK(device >= 0 && device < ndev);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    fuelmi_set_error("device %d is %s, not gfx950", device, prop.gcnArchName);
    return FUELMI_ENODEV;
  }
  HIPCHK(hipSetDevice(device));
  fuelmi_tsp* t = new fuelmi_tsp;
  t->device = device;
  t->cfg = *cfg;
  if (fuelmi_stream_create(&t->stream, INT_MIN, "TSP") != hipSuccess) {
    fuelmi_set_error("fuelmi_tsp_create: stream creation failed");
    delete t;
    return FUELMI_EHIP;
  }
  *out = t;
  return FUELMI_OK;
}

extern "C" void fuelmi_tsp_destroy(fuelmi_tsp* t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  if (t->stream) (void)hipStreamSynchronize(t->stream);
  if (t->dev) (void)hipFree(t->dev);
  if (t->pin) (void)hipHostFree(t->pin);
  if (t->stream) (void)hipStreamDestroy(t->stream);
  delete t;
}

static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" int fuelmi_tsp_solve(fuelmi_tsp* t, int n_prob, const int* dim_ptr, const int32_t* costs, int* order,
                                int64_t* tour_cost, int* method) {
  ARGCHK(t && n_prob >= 0);
  if (n_prob == 0) return FUELMI_OK;
  ARGCHK(dim_ptr && costs && order && tour_cost && method);
  ARGCHK(dim_ptr[0] == 0);
  const fuelmi_tsp_cfg& cf = t->cfg;
  // every check before anything is written
  long long entries = 0, nodes = 0, rorder_ints = 0;
  int n_heur = 0;
  for (int b = 0; b < n_prob; ++b) {
    const long long d = (long long)dim_ptr[b + 1] - dim_ptr[b];
    if (d < 1) {
      fuelmi_set_error("fuelmi_tsp_solve: problem %d has dimension %lld (>= 1)", b, d);
      return FUELMI_EINVAL;
    }
    if (d > FUELMI_TSP_MAX_DIM) {
      fuelmi_set_error("fuelmi_tsp_solve: problem %d has dimension %lld > FUELMI_TSP_MAX_DIM (%d)", b, d,
                       FUELMI_TSP_MAX_DIM);
      return FUELMI_ELIMIT;
    }
    entries += d * d, nodes += d;
    if (d - 1 > cf.exact_max) ++n_heur, rorder_ints += (long long)cf.restarts * d;
  }
  if (entries >= (1ll << 31)) {
    fuelmi_set_error("fuelmi_tsp_solve: %lld matrix entries in one call (< 2^31)", entries);
    return FUELMI_ELIMIT;
  }
  if ((long long)n_heur * cf.restarts >= (1ll << 31) || rorder_ints >= (1ll << 31)) {
    fuelmi_set_error("fuelmi_tsp_solve: %d heuristic problems x %d restarts in one call", n_heur, cf.restarts);
    return FUELMI_ELIMIT;
  }
  const long long ntask = (long long)n_heur * cf.restarts;
  // problems, task list, Held-Karp chunks (host)
  std::vector<TspProb> pr(n_prob);
  std::vector<int> exact_ids, heur_ids;
  std::vector<int2> tasks;
  tasks.reserve((size_t)ntask);
  long long off = 0, ro = 0;
  size_t tbl_max = 0;
  std::vector<std::pair<int, int>> chunks;  // [first, end) of exact_ids
  size_t chunk_bytes = 0;
  for (int b = 0; b < n_prob; ++b) {
    const int d = dim_ptr[b + 1] - dim_ptr[b];
    TspProb& P = pr[b];
    P.off = off, P.d = d, P.oout = dim_ptr[b], P.task0 = -1, P.tbl = 0;
    off += (long long)d * d;
    if (d - 1 <= cf.exact_max) {
      const size_t bytes = d > 1 ? ((size_t)1 << (d - 1)) * (size_t)(d - 1) * 8 : 0;
      if (exact_ids.empty() || chunk_bytes + bytes > TSP_TABLE_CHUNK) chunks.push_back({(int)exact_ids.size(), (int)exact_ids.size()}), chunk_bytes = 0;
      P.tbl = (long long)(chunk_bytes / 8);
      chunk_bytes += bytes;
      tbl_max = std::max(tbl_max, chunk_bytes);
      exact_ids.push_back(b);
      chunks.back().second = (int)exact_ids.size();
    } else {
      P.tbl = ro, P.task0 = (int)tasks.size();
      ro += (long long)cf.restarts * d;
      for (int r = 0; r < cf.restarts; ++r) tasks.push_back(make_int2(b, r));
      heur_ids.push_back(b);
    }
  }
  // workspace
  const size_t b_mat = al256((size_t)entries * 4), b_pr = al256(sizeof(TspProb) * n_prob),
               b_ids = al256(sizeof(int) * n_prob), b_tasks = al256(sizeof(int2) * (size_t)ntask + 8),
               b_rcost = al256(8 * (size_t)ntask + 8), b_rord = al256(4 * (size_t)rorder_ints + 4),
               b_oord = al256(4 * (size_t)nodes), b_ocost = al256(8 * (size_t)n_prob), b_tbl = al256(tbl_max + 8);
  const size_t need = 2 * b_mat + b_pr + b_ids + b_tasks + b_rcost + b_rord + b_oord + b_ocost + b_tbl;
  const size_t pin_in = b_mat + b_pr + b_ids + b_tasks, pin_out = b_oord + b_ocost;
  const size_t pin_need = std::max(pin_in, pin_out);
  HIPCHK(hipSetDevice(t->device));
  if (need > t->dev_bytes || pin_need > t->pin_bytes) {
    HIPCHK(hipStreamSynchronize(t->stream));
    if (need > t->dev_bytes) {
      if (t->dev) (void)hipFree(t->dev);
      t->dev = nullptr, t->dev_bytes = 0;
      if (hipMalloc(&t->dev, need) != hipSuccess) {
        (void)hipGetLastError();
        fuelmi_set_error("fuelmi_tsp_solve: device workspace of %zu bytes", need);
        return FUELMI_ENOMEM;
      }
      t->dev_bytes = need;
    }
    if (pin_need > t->pin_bytes) {
      if (t->pin) (void)hipHostFree(t->pin);
      t->pin = nullptr, t->pin_bytes = 0;
      if (hipHostMalloc(&t->pin, pin_need, 0) != hipSuccess) {
        (void)hipGetLastError();
        fuelmi_set_error("fuelmi_tsp_solve: pinned staging of %zu bytes", pin_need);
        return FUELMI_ENOMEM;
      }
      t->pin_bytes = pin_need;
    }
  }
  char* D = (char*)t->dev;
  int* d_mat = (int*)D;
  int* d_matT = (int*)(D + b_mat);
  TspProb* d_pr = (TspProb*)(D + 2 * b_mat);
  int* d_ids = (int*)(D + 2 * b_mat + b_pr);
  int2* d_tasks = (int2*)(D + 2 * b_mat + b_pr + b_ids);
  long long* d_rcost = (long long*)((char*)d_tasks + b_tasks);
  int* d_rord = (int*)((char*)d_rcost + b_rcost);
  int* d_oord = (int*)((char*)d_rord + b_rord);
  long long* d_ocost = (long long*)((char*)d_oord + b_oord);
  long long* d_tbl = (long long*)((char*)d_ocost + b_ocost);
  // inputs: one pinned block, one copy (ids: the exact problems first, then the heuristic ones)
  char* H = (char*)t->pin;
  memcpy(H, costs, (size_t)entries * 4);
  memcpy(H + b_mat, pr.data(), sizeof(TspProb) * n_prob);
  int* h_ids = (int*)(H + b_mat + b_pr);
  std::copy(exact_ids.begin(), exact_ids.end(), h_ids);
  std::copy(heur_ids.begin(), heur_ids.end(), h_ids + exact_ids.size());
  if (ntask) memcpy(H + b_mat + b_pr + b_ids, tasks.data(), sizeof(int2) * (size_t)ntask);
  HIPCHK(hipMemcpyAsync(d_mat, H, b_mat, hipMemcpyHostToDevice, t->stream));
  HIPCHK(hipMemcpyAsync(d_pr, H + b_mat, b_pr + b_ids + b_tasks, hipMemcpyHostToDevice, t->stream));
  for (auto& ch : chunks)
    hipLaunchKernelGGL(k_tsp_exact, dim3(ch.second - ch.first), dim3(TSP_EXACT_THREADS), 0, t->stream, d_mat, d_pr,
                       d_ids + ch.first, d_tbl, d_oord, d_ocost);
  if (n_heur) {
    int dmax = 0;
    for (int b : heur_ids) dmax = std::max(dmax, pr[b].d);
    const int gx = std::min(64, (int)(((long long)dmax * dmax + 1023) / 1024));
    hipLaunchKernelGGL(k_tsp_transpose, dim3(gx, std::min(n_heur, 65535)), dim3(256), 0, t->stream, d_mat, d_matT, d_pr,
                       d_ids + exact_ids.size(), n_heur);
    hipLaunchKernelGGL(k_tsp_ils, dim3((unsigned)ntask), dim3(TSP_ILS_THREADS), 0, t->stream, d_mat, d_matT, d_pr,
                       d_tasks, cf.kicks, (u64)cf.seed, d_rcost, d_rord);
    hipLaunchKernelGGL(k_tsp_pick, dim3(n_heur), dim3(256), 0, t->stream, d_pr, d_ids + exact_ids.size(), cf.restarts,
                       d_rcost, d_rord, d_oord, d_ocost);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(H, d_oord, b_oord + b_ocost, hipMemcpyDeviceToHost, t->stream));
  HIPCHK(stream_wait(t->stream));
  memcpy(order, H, sizeof(int) * (size_t)nodes);
  memcpy(tour_cost, H + b_oord, sizeof(int64_t) * n_prob);
  for (int b = 0; b < n_prob; ++b) method[b] = dim_ptr[b + 1] - dim_ptr[b] - 1 <= cf.exact_max ? 0 : 1;
  return FUELMI_OK;
}
