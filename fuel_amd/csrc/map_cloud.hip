// map_cloud.hip -- ordered extraction of map clouds and the known-volume count: the scans of MapROS::publishMapLocal,
// publishMapAll and publishUnknown (plan_env/src/map_ros.cpp:217-346) over the state planes the device holds, without
// a host mirror of the log-odds.
//
// A work item is one 64-bit chunk of one (x, y) line's z range of the box.  Items are numbered line-major, lines
// x-major, so the item number order is ascending voxel address: the order of the reference's three loops.  A line's
// bits start at bit (x * ny + y) * nz + z_lo of the linear plane, at any offset inside a word: a chunk is two word
// loads and a funnel shift (plane_window; the planes' zero margins make the second load safe), masked to the line's
// length and to the z-truncation, which depends on z alone and is built once per workgroup in LDS from the reference's
// f64 expression.
//
// Three launches, no waiting between workgroups of any kind:
//   k_cloud_count   popcount per item, workgroup reduction, one word per workgroup
//   k_cloud_scan    ONE workgroup of CL_SCAN lanes: exclusive scan of the workgroup counts in ceil(nwg / CL_SCAN)
//                   rounds with a running carry, in place; the total goes to a device word and a pinned word
//   k_cloud_write   recomputes the chunk, wave prefix of the popcounts + the waves in front + the workgroup's offset,
//                   then a per-lane loop over the set bits (ctz, clear lowest): a wave's lanes write one contiguous
//                   range of the output.  A workgroup whose offset is at or past `cap` leaves at once, a lane stops at it.
// Every loop has a bound known at launch.  -ffp-contract=off: the point expression rounds like the reference's.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "fuelmi_internal.h"

namespace {

constexpr int CL_WG = 256;     // items of a workgroup: one per lane
constexpr int CL_SCAN = 1024;  // lanes of the scan's one workgroup: workgroup counts per round
constexpr int CL_MAXCH = 4;    // chunks of a line: nz <= 255
static_assert(CL_WG == 64 * CL_MAXCH, "the z-mask is built by one wave per chunk");
constexpr size_t CL_HEAD = 256;  // bytes in front of the workgroup words: the total, on cache lines of its own

struct CloudArgs {
  const u64* plane;  // the kind's plane
  int invert;        // KNOWN: the complement of the unknown plane
  int lo[3];
  int ylen, zlen;
  int cpl;      // chunks per line
  int n_items;  // lines * cpl
  int nwg;
  double z_low, z_high;
  u32* wg;         // [nwg] counts, then exclusive offsets
  u32* total;      // device word
  u32* total_pin;  // pinned word
  float* out;      // [min(cap, voxels of the box)][3]
  u32 cap;
};

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ u32 cl_wave_incl(u32 v) {
  const int lane = threadIdx.x & 63;
  for (int d = 1; d < 64; d <<= 1) {
    const u32 t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// zm[c]: bit b set iff voxel z_lo + 64 c + b belongs to the line and passes map_ros.cpp's two `continue`s
// (:226-227, :276-277, :331-332): dropped iff pos_z > z_high or pos_z < z_low, pos_z = indexToPos (sdf_map.h:132-135).
// Wave c of the workgroup builds chunk c; ends with a barrier.
__device__ __forceinline__ void cl_zmask(const Geo& g, const CloudArgs& C, u64* zm) {
  const int c = threadIdx.x >> 6, zi = threadIdx.x;  // 64 c + lane
  bool keep = false;
  if (zi < C.zlen) {
    const double pz = (C.lo[2] + zi + 0.5) * g.res + g.org[2];
    keep = !(pz > C.z_high) && !(pz < C.z_low);
  }
  const u64 m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) zm[c] = m;
  __syncthreads();
}

// the selected bits of an item; x, y, z0: the voxel of its bit 0
__device__ __forceinline__ u64 cl_chunk(const Geo& g, const CloudArgs& C, const u64* zm, int item, int& x, int& y, int& z0) {
  const int line = item / C.cpl, c = item - line * C.cpl;
  const int xi = line / C.ylen;
  x = C.lo[0] + xi, y = C.lo[1] + (line - xi * C.ylen), z0 = C.lo[2] + 64 * c;
  u64 w = plane_window(C.plane, ((long)x * g.ny + y) * g.nz + z0);
  if (C.invert) w = ~w;
  return w & zm[c];
}

__global__ void __launch_bounds__(CL_WG) k_cloud_count(Geo g, CloudArgs C) {
  __shared__ u64 zm[CL_MAXCH];
  __shared__ u32 wsum[CL_WG / 64];
  cl_zmask(g, C, zm);
  const int item = blockIdx.x * CL_WG + threadIdx.x;
  u32 n = 0;
  if (item < C.n_items) {
    int x, y, z0;
    n = (u32)__popcll(cl_chunk(g, C, zm, item, x, y, z0));
  }
  const u32 inc = cl_wave_incl(n);
  if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 s = 0;
    for (int k = 0; k < CL_WG / 64; ++k) s += wsum[k];
    C.wg[blockIdx.x] = s;
  }
}

__global__ void __launch_bounds__(CL_SCAN) k_cloud_scan(CloudArgs C) {
  __shared__ u32 wtot[CL_SCAN / 64];
  const int wave = threadIdx.x >> 6;
  const int rounds = (C.nwg + CL_SCAN - 1) / CL_SCAN;
  u32 carry = 0;
  for (int r = 0; r < rounds; ++r) {
    const int j = r * CL_SCAN + threadIdx.x;
    const u32 v = j < C.nwg ? C.wg[j] : 0u;
    const u32 inc = cl_wave_incl(v);
    if ((threadIdx.x & 63) == 63) wtot[wave] = inc;
    __syncthreads();
    u32 before = 0, all = 0;
    for (int k = 0; k < CL_SCAN / 64; ++k) {
      const u32 t = wtot[k];
      if (k < wave) before += t;
      all += t;
    }
    if (j < C.nwg) C.wg[j] = carry + before + inc - v;
    carry += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *C.total = carry;
    *C.total_pin = carry;
  }
}

__global__ void __launch_bounds__(CL_WG) k_cloud_write(Geo g, CloudArgs C) {
  __shared__ u64 zm[CL_MAXCH];
  __shared__ u32 wsum[CL_WG / 64];
  const u32 off = C.wg[blockIdx.x];
  if (off >= C.cap) return;  // the whole workgroup: its offset is one word
  cl_zmask(g, C, zm);
  const int item = blockIdx.x * CL_WG + threadIdx.x;
  int x = 0, y = 0, z0 = 0;
  u64 w = 0ull;
  if (item < C.n_items) w = cl_chunk(g, C, zm, item, x, y, z0);
  const u32 n = (u32)__popcll(w);
  const u32 inc = cl_wave_incl(n);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) wsum[wave] = inc;
  __syncthreads();
  u32 at = off + inc - n;
  for (int k = 0; k < CL_WG / 64; ++k)
    if (k < wave) at += wsum[k];
  // pcl::PointXYZ is assigned from indexToPos's doubles (:228-230): the f64 expression, one rounding to float
  const float px = (float)((x + 0.5) * g.res + g.org[0]), py = (float)((y + 0.5) * g.res + g.org[1]);
  while (w && at < C.cap) {
    const int b = __builtin_ctzll(w);
    w &= w - 1ull;
    float* o = C.out + 3 * (size_t)at;
    o[0] = px;
    o[1] = py;
    o[2] = (float)((z0 + b + 0.5) * g.res + g.org[2]);
    ++at;
  }
}

// the geometry of a box: P = {items per line, lines, items per workgroup, workgroups, scan width, scan rounds, scratch
// bytes in front of the points, voxels of the box}.  Empty box (lo > hi on an axis): 1, everything 0.
int cl_plan(const int dims[3], const int lo[3], const int hi[3], int P[8]) {
  ARGCHK(dims && lo && hi && P);
  ARGCHK(dims[0] > 0 && dims[1] > 0 && dims[2] > 0 && dims[2] <= 255);
  ARGCHK((long)dims[0] * dims[1] * dims[2] < (1L << 31) - 64);
  for (int k = 0; k < 8; ++k) P[k] = 0;
  P[2] = CL_WG, P[4] = CL_SCAN;
  for (int k = 0; k < 3; ++k)
    if (lo[k] > hi[k]) return 1;
  for (int k = 0; k < 3; ++k) ARGCHK(lo[k] >= 0 && hi[k] < dims[k]);
  const long xlen = hi[0] - lo[0] + 1, ylen = hi[1] - lo[1] + 1, zlen = hi[2] - lo[2] + 1;
  const long cpl = (zlen + 63) / 64, lines = xlen * ylen, items = lines * cpl;
  const long nwg = (items + CL_WG - 1) / CL_WG;
  P[0] = (int)cpl, P[1] = (int)lines, P[3] = (int)nwg;
  P[5] = (int)((nwg + CL_SCAN - 1) / CL_SCAN);
  P[6] = (int)(CL_HEAD + (((size_t)nwg * sizeof(u32) + 255) & ~(size_t)255));
  P[7] = (int)(lines * zlen);
  return FUELMI_OK;
}

}  // namespace

void map_cloud_release(fuelmi_map* m) {
  if (m->cloud_pin) (void)hipHostFree(m->cloud_pin);
  m->cloud_pin = nullptr;
  for (hipEvent_t& e : m->cloud_ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

extern "C" int fuelmi_cloud_plan(const int dims[3], const int lo[3], const int hi[3], int out[8]) {
  const int rc = cl_plan(dims, lo, hi, out);
  return rc == 1 ? FUELMI_OK : rc;
}

extern "C" int fuelmi_map_cloud_times(const fuelmi_map* m, double ms3[3]) {
  ARGCHK(m && ms3);
  for (int k = 0; k < 3; ++k) ms3[k] = m->cloud_ms[k];
  return FUELMI_OK;
}

extern "C" int fuelmi_map_extract_cloud(fuelmi_map* m, const fuelmi_cloud_cfg* cfg, float* xyz, int cap, int* n_total) {
  // every argument on the host, before anything is launched
  ARGCHK(m && cfg && n_total);
  ARGCHK(cfg->kind >= FUELMI_CLOUD_OCCUPIED && cfg->kind <= FUELMI_CLOUD_INFLATED);
  ARGCHK(cap >= 0 && (xyz || cap == 0));
  const Geo& g = m->g;
  const int dims[3] = {g.nx, g.ny, g.nz};
  int P[8];
  {
    const int rc = cl_plan(dims, cfg->lo, cfg->hi, P);
    if (rc == 1) {  // the reference's loops do not run
      *n_total = 0;
      return FUELMI_OK;
    }
    if (rc) return rc;
  }
  HIPCHK(hipSetDevice(m->device));
  hipStream_t st = m->stream;
  if (!m->cloud_pin) {
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&m->cloud_pin), 64, hipHostMallocDefault));
    for (hipEvent_t& e : m->cloud_ev) HIPCHK(hipEventCreate(&e));
  }
  const size_t n_out = std::min((size_t)cap, (size_t)P[7]);
  {
    const int rc = m->cloud_dev.reserve(st, (size_t)P[6] + n_out * 3 * sizeof(float));
    if (rc) return rc;
  }
  unsigned char* base = m->cloud_dev.base();
  CloudArgs C;
  memset(&C, 0, sizeof(C));
  switch (cfg->kind) {
    case FUELMI_CLOUD_OCCUPIED: C.plane = m->occ_bits.p; break;
    case FUELMI_CLOUD_INFLATED: C.plane = m->infl_bits.p; break;
    default: C.plane = m->unk_bits.p; break;
  }
  C.invert = cfg->kind == FUELMI_CLOUD_KNOWN;
  for (int k = 0; k < 3; ++k) C.lo[k] = cfg->lo[k];
  C.ylen = cfg->hi[1] - cfg->lo[1] + 1, C.zlen = cfg->hi[2] - cfg->lo[2] + 1;
  C.cpl = P[0], C.n_items = P[0] * P[1], C.nwg = P[3];
  C.z_low = cfg->z_low, C.z_high = cfg->z_high;
  C.total = reinterpret_cast<u32*>(base);
  C.wg = reinterpret_cast<u32*>(base + CL_HEAD);
  C.total_pin = m->cloud_pin;
  C.out = reinterpret_cast<float*>(base + P[6]);
  C.cap = (u32)n_out;
  HIPCHK(hipEventRecord(m->cloud_ev[0], st));
  hipLaunchKernelGGL(k_cloud_count, dim3(C.nwg), dim3(CL_WG), 0, st, g, C);
  hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(CL_SCAN), 0, st, C);
  HIPCHK(hipEventRecord(m->cloud_ev[1], st));
  if (n_out) hipLaunchKernelGGL(k_cloud_write, dim3(C.nwg), dim3(CL_WG), 0, st, g, C);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(m->cloud_ev[2], st));
  HIPCHK(stream_wait(st));
  const size_t total = *m->cloud_pin, n_copy = std::min(total, n_out);
  if (n_copy) HIPCHK(hipMemcpyAsync(xyz, C.out, n_copy * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipEventRecord(m->cloud_ev[3], st));
  HIPCHK(hipStreamSynchronize(st));
  for (int k = 0; k < 3; ++k) {
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, m->cloud_ev[k], m->cloud_ev[k + 1]));
    m->cloud_ms[k] = ms;
  }
  *n_total = (int)total;
  if (xyz && total > (size_t)cap) {
    fuelmi_set_error("cloud extraction: %zu points, room for %d", total, cap);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}
