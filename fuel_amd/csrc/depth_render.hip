// depth_render.hip -- batched rendering of simulated depth frames from a world cloud (include/fuelmi.h "Depth renderer").
//
// The reference's simulated depth camera (uav_simulator/local_sensing) takes, per pixel, the minimum depth over the
// square windows that the cloud's points splat.  A renderer object owns a stream, the cloud, the frames of max_poses
// poses and a grow-only scratch, and answers a batch of poses in one call, all poses in one grid (pose = blockIdx.y):
//   k_render_project<MODEL>  one lane per (pose, point): the culls and the projection of the model, literally, then the
//                            window and the 32-bit key as a record.  A per-wave ballot and one returning atomic per wave
//                            reserve the slots; windows whose larger side reaches RENDER_WAVE_MIN go to a second list
//                            (the pose's slice of n_points records is filled from both ends, so nothing overflows)
//   k_render_splat           one unsigned atomic min of the key per pixel.  Small windows: one 16-lane segment each, the
//                            lanes running along x and wrapping to the next row; large windows: one wave each, the same
//                            way.  A plain read that already shows a key at least as small skips the atomic (keys only
//                            fall, so a stale read costs an atomic, never a pixel)
//   k_render_convert<MODEL>  key image -> f32 metres frame and u16 raw frame, the key image back to "empty", the count
//                            of pixels with a return
// The minimum makes the result independent of the schedule and of the cloud's order.  HOST_NODE's key is the bit pattern
// of the float depth (positive floats order as unsigned integers), CUDA_NODE's the millimetre value; empty = 0xFFFFFFFF.
// tests/depth_render_ref.py restates both models.
#include "fuelmi_internal.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <set>

#define RENDER_EMPTY 0xFFFFFFFFu
#define RENDER_PROJECT_THREADS 256
#define RENDER_SPLAT_THREADS 256
#define RENDER_SEG_LANES 16        // lanes of one small window
#define RENDER_WAVE_MIN 17         // a window whose larger side (clipped) reaches this is spread over a wave
#define RENDER_CONVERT_THREADS 256
#define RENDER_CONVERT_PER_THREAD 4
#define RENDER_SPLAT_MAX_WG 1024
#define RENDER_MAX_POSES 4096
#define RENDER_MAX_PIXELS (1ll << 24)         // of one frame
#define RENDER_MAX_FRAME_PIXELS (1ll << 28)   // of all max_poses frames
#define RENDER_MAX_POINTS (1ll << 27)
#define RENDER_MAX_RECORDS (1ll << 28)        // n_pose * n_points of one call

struct RenderPose {
  double R[9], t[3], pos[3];
  float Rf[9], tf[3];  // CUDA_NODE: rounded to float once
};
struct RenderRec {
  int x0, x1, y0, y1;
  u32 key;
};
struct RenderCam {
  int rows, cols;
  double fx, fy, cx, cy, range;
  float fxf, fyf, cxf, cyf;
};
enum { RC_SMALL = 0, RC_LARGE = 1, RC_UNDEF = 2, RC_PIXELS = 3, RC_N = 4 };  // counters of one pose
enum { ST_CULLED = 0, ST_UNDEF = 1, ST_SMALL = 2, ST_LARGE = 3 };

struct fuelmi_render {
  fuelmi_render_cfg cfg;
  RenderCam cam;
  hipStream_t stream = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool timed = false;
  float* cloud = nullptr;  // grow-only
  size_t cloud_cap = 0;    // points
  int n_points = 0;
  bool has_cloud = false;
  u32* keys = nullptr;  // [max_poses][rows * cols]
  float* metres = nullptr;
  unsigned short* raw = nullptr;
  bool keys_clean = false;  // every key is RENDER_EMPTY
  RenderPose* d_poses = nullptr;
  u32* d_cnt = nullptr;
  void* pin = nullptr;  // poses in, counters out
  DevScratch scratch;   // the records
};

static std::mutex g_render_mu;
static std::set<const fuelmi_render*> g_render_live;
static bool render_live(const fuelmi_render* r) {
  std::lock_guard<std::mutex> lk(g_render_mu);
  return r && g_render_live.count(r) != 0;
}
#define RENDER_LIVE(r)                                                                    \
  do {                                                                                    \
    if (!render_live(r)) {                                                                \
      fuelmi_set_error("fuelmi_render: not a live renderer (null, or used after destroy)"); \
      return FUELMI_EINVAL;                                                               \
    }                                                                                     \
  } while (0)

// ---- phase 1: cull, project, compact -------------------------------------------------------------------------------
__device__ __forceinline__ int render_window(int c0, int c1, int r0, int r1, u32 key, RenderRec& o) {
  o.x0 = c0, o.x1 = c1, o.y0 = r0, o.y1 = r1, o.key = key;
  return max(c1 - c0, r1 - r0) + 1 >= RENDER_WAVE_MIN ? ST_LARGE : ST_SMALL;
}

// depth_render_node.cpp:126-149
__device__ __forceinline__ int render_project_host(const float* __restrict__ p, const RenderPose& P, const RenderCam& cam,
                                                   RenderRec& o) {
  const float X = p[0], Y = p[1], Z = p[2];
  if (!(isfinite(X) && isfinite(Y) && isfinite(Z))) return ST_UNDEF;
  const double x = X, y = Y, z = Z;
  const double dx = P.pos[0] - x, dy = P.pos[1] - y, dz = P.pos[2] - z;
  if (sqrt((dx * dx + dy * dy) + dz * dz) > cam.range) return ST_CULLED;
  const double pcx = ((P.R[0] * x + P.R[1] * y) + P.R[2] * z) + P.t[0];
  const double pcy = ((P.R[3] * x + P.R[4] * y) + P.R[5] * z) + P.t[1];
  const double pcz = ((P.R[6] * x + P.R[7] * y) + P.R[8] * z) + P.t[2];
  if (pcz != pcz) return ST_UNDEF;
  if (pcz <= 0.0) return ST_CULLED;
  const float px = (float)(pcx / pcz * cam.fx + cam.cx);
  const float py = (float)(pcy / pcz * cam.fy + cam.cy);
  if (px != px || py != py) return ST_UNDEF;
  if (px < 0 || px >= (float)cam.cols || py < 0 || py >= (float)cam.rows) return ST_CULLED;
  const float dist = (float)pcz;
  if (dist < 1e-3f) return ST_UNDEF;
  const int r = (int)(0.0573 * cam.fx / (double)dist + 0.5);
  const float rf = (float)r;
  const float hx = px + rf, hy = py + rf;  // < 2^31 unless r rounds up to it: the window ends at the border then
  const int c0 = max((int)(px - rf), 0), c1 = hx >= 2147483648.0f ? cam.cols - 1 : min((int)hx, cam.cols - 1);
  const int r0 = max((int)(py - rf), 0), r1 = hy >= 2147483648.0f ? cam.rows - 1 : min((int)hy, cam.rows - 1);
  return render_window(c0, c1, r0, r1, __float_as_uint(dist), o);
}

// depth_render.cu:8-32
__device__ __forceinline__ int render_project_cuda(const float* __restrict__ p, const RenderPose& P, const RenderCam& cam,
                                                   RenderRec& o) {
  const float x = p[0], y = p[1], z = p[2];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return ST_UNDEF;
  const float tx = ((x * P.Rf[0] + y * P.Rf[1]) + z * P.Rf[2]) + P.tf[0];
  const float ty = ((x * P.Rf[3] + y * P.Rf[4]) + z * P.Rf[5]) + P.tf[1];
  const float tz = ((x * P.Rf[6] + y * P.Rf[7]) + z * P.Rf[8]) + P.tf[2];
  if (tz != tz) return ST_UNDEF;
  if (tz <= 0.0f) return ST_CULLED;
  const float qx = tx / tz * cam.fxf + cam.cxf, qy = ty / tz * cam.fyf + cam.cyf;
  const double ud = (double)qx + 0.5, vd = (double)qy + 0.5;
  if (!(ud > -2147483649.0 && ud < 2147483648.0 && vd > -2147483649.0 && vd < 2147483648.0)) return ST_UNDEF;
  const int u = (int)ud, v = (int)vd;
  if (u < 0 || u >= cam.cols || v < 0 || v >= cam.rows) return ST_CULLED;
  if (tz < 1e-3f) return ST_UNDEF;
  const float mf = tz * 1000.0f + 0.5f;
  if (!(mf < 2147483648.0f)) return ST_UNDEF;
  const int mm = (int)mf;
  const int r = (int)(0.0573 * (double)cam.fxf / (double)tz + (double)0.5f);
  const int c0 = max(u - r, 0), c1 = (int)min((long long)u + r, (long long)cam.cols - 1);
  const int r0 = max(v - r, 0), r1 = (int)min((long long)v + r, (long long)cam.rows - 1);
  return render_window(c0, c1, r0, r1, (u32)mm, o);
}

template <int MODEL>
__global__ void __launch_bounds__(RENDER_PROJECT_THREADS)
    k_render_project(const float* __restrict__ cloud, int n_points, const RenderPose* __restrict__ poses, RenderCam cam,
                     RenderRec* __restrict__ recs, u32* __restrict__ cnt) {
  const int pose = blockIdx.y;
  const RenderPose P = poses[pose];
  RenderRec* list = recs + (size_t)pose * n_points;
  u32* c = cnt + RC_N * pose;
  const int lane = threadIdx.x & 63;
  const u64 below = (1ull << lane) - 1ull;
  // the bound is the same for every lane of a wave: the ballots see whole waves
  for (long long base = (long long)blockIdx.x * blockDim.x; base < n_points; base += (long long)gridDim.x * blockDim.x) {
    const long long i = base + threadIdx.x;
    int st = ST_CULLED;
    RenderRec rec;
    if (i < n_points)
      st = MODEL == FUELMI_RENDER_HOST_NODE ? render_project_host(cloud + 3 * i, P, cam, rec)
                                            : render_project_cuda(cloud + 3 * i, P, cam, rec);
    const u64 ms = __ballot(st == ST_SMALL), ml = __ballot(st == ST_LARGE), mu = __ballot(st == ST_UNDEF);
    u32 bs = 0, bl = 0;
    if (lane == 0) {
      if (ms) bs = atomicAdd(&c[RC_SMALL], (u32)__popcll(ms));
      if (ml) bl = atomicAdd(&c[RC_LARGE], (u32)__popcll(ml));
      if (mu) atomicAdd(&c[RC_UNDEF], (u32)__popcll(mu));
    }
    bs = __shfl(bs, 0, 64), bl = __shfl(bl, 0, 64);
    if (st == ST_SMALL) list[bs + (u32)__popcll(ms & below)] = rec;                    // from the front
    if (st == ST_LARGE) list[(u32)n_points - 1u - (bl + (u32)__popcll(ml & below))] = rec;  // from the back
  }
}

// ---- phase 2: splat ----------------------------------------------------------------------------------------------------
// pixels t = first, first + step, ... of the window, row by row
__device__ __forceinline__ void render_splat_window(const RenderRec& r, u32* __restrict__ img, int cols, int first, int step) {
  const int w = r.x1 - r.x0 + 1, n = w * (r.y1 - r.y0 + 1);  // <= 2^24 pixels
  for (int t = first; t < n; t += step) {
    const int dy = t / w, dx = t - dy * w;
    u32* px = img + (size_t)(r.y0 + dy) * cols + (r.x0 + dx);
    if (*px > r.key) atomicMin(px, r.key);
  }
}

__global__ void __launch_bounds__(RENDER_SPLAT_THREADS)
    k_render_splat(const RenderRec* __restrict__ recs, int n_points, const u32* __restrict__ cnt, u32* __restrict__ keys,
                   int cols, int npix) {
  const int pose = blockIdx.y;
  const RenderRec* list = recs + (size_t)pose * n_points;
  u32* img = keys + (size_t)pose * npix;
  const u32 ns = cnt[RC_N * pose + RC_SMALL], nl = cnt[RC_N * pose + RC_LARGE];
  const u32 segs = RENDER_SPLAT_THREADS / RENDER_SEG_LANES, waves = RENDER_SPLAT_THREADS / 64;
  for (u32 i = blockIdx.x * segs + threadIdx.x / RENDER_SEG_LANES; i < ns; i += gridDim.x * segs)
    render_splat_window(list[i], img, cols, threadIdx.x % RENDER_SEG_LANES, RENDER_SEG_LANES);
  for (u32 i = blockIdx.x * waves + threadIdx.x / 64; i < nl; i += gridDim.x * waves)
    render_splat_window(list[(u32)n_points - 1u - i], img, cols, threadIdx.x & 63, 64);
}

// ---- phase 3: convert --------------------------------------------------------------------------------------------------
template <int MODEL>
__global__ void __launch_bounds__(RENDER_CONVERT_THREADS)
    k_render_convert(u32* __restrict__ keys, float* __restrict__ metres, unsigned short* __restrict__ raw,
                     u32* __restrict__ cnt, int npix, float kf) {
  const int pose = blockIdx.y;
  const size_t base = (size_t)pose * npix;
  int hits = 0;
  for (int j = 0; j < RENDER_CONVERT_PER_THREAD; ++j) {
    const long long p = ((long long)blockIdx.x * RENDER_CONVERT_PER_THREAD + j) * RENDER_CONVERT_THREADS + threadIdx.x;
    if (p >= npix) break;
    const u32 key = keys[base + p];
    float m;
    if (MODEL == FUELMI_RENDER_HOST_NODE) {
      m = key == RENDER_EMPTY ? 0.0f : __uint_as_float(key);
    } else {  // pcl_render_node.cpp:300-310 on the minimum over 999999
      const int mm = (int)min(key, 999999u);
      const float d = (float)mm / 1000.0f;
      m = d < 500.0f ? d : 0.0f;
    }
    if (key != RENDER_EMPTY) keys[base + p] = RENDER_EMPTY;
    metres[base + p] = m;
    // convertTo(CV_16UC1, k): saturate_u16(round_half_even(m * (float)k))
    const float v = rintf(m * kf);
    raw[base + p] = v >= 65535.0f ? (unsigned short)65535 : v > 0.0f ? (unsigned short)v : (unsigned short)0;
    hits += m != 0.0f;
  }
  for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);
  __shared__ int wsum[RENDER_CONVERT_THREADS / 64];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = hits;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < RENDER_CONVERT_THREADS / 64; ++w) tot += wsum[w];
    if (tot) atomicAdd(&cnt[RC_N * pose + RC_PIXELS], (u32)tot);
  }
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct RenderGeom {
  int project_wg, splat_wg, convert_wg;
};
static RenderGeom render_geom(long long npix, int n_points) {
  RenderGeom g;
  g.project_wg = (int)(((long long)n_points + RENDER_PROJECT_THREADS - 1) / RENDER_PROJECT_THREADS);
  g.splat_wg = (int)std::min<long long>(RENDER_SPLAT_MAX_WG, std::max<long long>(1, ((long long)n_points + 63) / 64));
  const long long per = (long long)RENDER_CONVERT_THREADS * RENDER_CONVERT_PER_THREAD;
  g.convert_wg = (int)((npix + per - 1) / per);
  return g;
}
static size_t render_scratch_bytes(int n_pose, int n_points) {
  BlockLayout lay(nullptr, 256);
  lay.take<RenderRec>((size_t)n_pose * (size_t)std::max(n_points, 1));
  return lay.size();
}

static int render_cfg_check(const fuelmi_render_cfg* c) {
  if (c->rows < 1 || c->cols < 1) {
    fuelmi_set_error("fuelmi_render: image of %d x %d (rows, cols >= 1)", c->rows, c->cols);
    return FUELMI_EINVAL;
  }
  if ((long long)c->rows * c->cols > RENDER_MAX_PIXELS) {
    fuelmi_set_error("fuelmi_render: image of %d x %d has more than 2^24 pixels", c->rows, c->cols);
    return FUELMI_ELIMIT;
  }
  if (!(std::isfinite(c->fx) && std::isfinite(c->fy) && c->fx > 0.0 && c->fy > 0.0)) {
    fuelmi_set_error("fuelmi_render: fx %g, fy %g (finite, > 0)", c->fx, c->fy);
    return FUELMI_EINVAL;
  }
  if (!(std::isfinite(c->cx) && std::isfinite(c->cy))) {
    fuelmi_set_error("fuelmi_render: cx %g, cy %g (finite)", c->cx, c->cy);
    return FUELMI_EINVAL;
  }
  if (57.3 * std::max(c->fx, c->fy) + 1.0 >= 2147483648.0) {
    fuelmi_set_error("fuelmi_render: fx %g, fy %g: the window radius of the closest point kept leaves int", c->fx, c->fy);
    return FUELMI_ELIMIT;
  }
  if (c->model != FUELMI_RENDER_HOST_NODE && c->model != FUELMI_RENDER_CUDA_NODE) {
    fuelmi_set_error("fuelmi_render: model %d (FUELMI_RENDER_HOST_NODE or FUELMI_RENDER_CUDA_NODE)", c->model);
    return FUELMI_EINVAL;
  }
  if (c->model == FUELMI_RENDER_HOST_NODE && !(c->range >= 0.0)) {
    fuelmi_set_error("fuelmi_render: range %g (>= 0, +inf switches the cull off)", c->range);
    return FUELMI_EINVAL;
  }
  if (c->max_poses < 1) {
    fuelmi_set_error("fuelmi_render: max_poses %d (>= 1)", c->max_poses);
    return FUELMI_EINVAL;
  }
  if (c->max_poses > RENDER_MAX_POSES || (long long)c->max_poses * c->rows * c->cols > RENDER_MAX_FRAME_PIXELS) {
    fuelmi_set_error("fuelmi_render: max_poses %d (<= %d, and at most 2^28 pixels in all frames)", c->max_poses,
                     RENDER_MAX_POSES);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}
static int render_points_check(long long n_points) {
  if (n_points < 0) {
    fuelmi_set_error("fuelmi_render: %lld points (>= 0)", n_points);
    return FUELMI_EINVAL;
  }
  if (n_points > RENDER_MAX_POINTS) {
    fuelmi_set_error("fuelmi_render: %lld points (<= 2^27)", n_points);
    return FUELMI_ELIMIT;
  }
  return FUELMI_OK;
}

extern "C" int fuelmi_render_plan(const fuelmi_render_cfg* cfg, int n_points, int out[8]) {
  ARGCHK(cfg && out);
  int rc = render_cfg_check(cfg);
  if (rc || (rc = render_points_check(n_points))) return rc;
  if ((long long)cfg->max_poses * n_points > RENDER_MAX_RECORDS) {
    fuelmi_set_error("fuelmi_render_plan: %d poses x %d points (<= 2^28 records)", cfg->max_poses, n_points);
    return FUELMI_ELIMIT;
  }
  const RenderGeom g = render_geom((long long)cfg->rows * cfg->cols, n_points);
  const size_t sb = render_scratch_bytes(cfg->max_poses, n_points);
  out[0] = RENDER_SEG_LANES;
  out[1] = RENDER_WAVE_MIN;
  out[2] = RENDER_PROJECT_THREADS;
  out[3] = g.project_wg;
  out[4] = g.splat_wg;
  out[5] = g.convert_wg;
  out[6] = (int)(sb & 0x7FFFFFFFu);
  out[7] = (int)(sb >> 31);
  return FUELMI_OK;
}

static void render_free(fuelmi_render* r) {
  (void)hipSetDevice(r->cfg.device);
  if (r->stream) (void)hipStreamSynchronize(r->stream);
  r->scratch.release();
  if (r->cloud) (void)hipFree(r->cloud);
  if (r->keys) (void)hipFree(r->keys);
  if (r->metres) (void)hipFree(r->metres);
  if (r->raw) (void)hipFree(r->raw);
  if (r->d_poses) (void)hipFree(r->d_poses);
  if (r->d_cnt) (void)hipFree(r->d_cnt);
  if (r->pin) (void)hipHostFree(r->pin);
  for (hipEvent_t e : r->ev)
    if (e) (void)hipEventDestroy(e);
  if (r->stream) (void)hipStreamDestroy(r->stream);
  delete r;
}

extern "C" int fuelmi_render_create(const fuelmi_render_cfg* cfg, fuelmi_render** out) {
  ARGCHK(cfg && out);
  const int rc = render_cfg_check(cfg);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    fuelmi_set_error("no HIP device available: libfuelmi has no CPU fallback");
    return FUELMI_ENODEV;
  }
  ARGCHK(cfg->device >= 0 && cfg->device < ndev);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    fuelmi_set_error("device %d is %s, not gfx950", cfg->device, prop.gcnArchName);
    return FUELMI_ENODEV;
  }
  HIPCHK(hipSetDevice(cfg->device));
  fuelmi_render* r = new fuelmi_render;
  r->cfg = *cfg;
  RenderCam& cam = r->cam;
  cam.rows = cfg->rows, cam.cols = cfg->cols;
  cam.fx = cfg->fx, cam.fy = cfg->fy, cam.cx = cfg->cx, cam.cy = cfg->cy, cam.range = cfg->range;
  cam.fxf = (float)cfg->fx, cam.fyf = (float)cfg->fy, cam.cxf = (float)cfg->cx, cam.cyf = (float)cfg->cy;
  const size_t frames = (size_t)cfg->max_poses * cfg->rows * cfg->cols;
  const size_t pin_bytes = (size_t)cfg->max_poses * (sizeof(RenderPose) + RC_N * sizeof(u32));
  bool ok = fuelmi_stream_create(&r->stream, INT_MIN, "RENDER") == hipSuccess;
  for (int i = 0; ok && i < 4; ++i) ok = hipEventCreate(&r->ev[i]) == hipSuccess;
  ok = ok && hipMalloc(&r->keys, frames * sizeof(u32)) == hipSuccess &&
       hipMalloc(&r->metres, frames * sizeof(float)) == hipSuccess &&
       hipMalloc(&r->raw, frames * sizeof(unsigned short)) == hipSuccess &&
       hipMalloc(&r->d_poses, (size_t)cfg->max_poses * sizeof(RenderPose)) == hipSuccess &&
       hipMalloc(&r->d_cnt, (size_t)cfg->max_poses * RC_N * sizeof(u32)) == hipSuccess &&
       hipHostMalloc(&r->pin, pin_bytes, 0) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    fuelmi_set_error("fuelmi_render_create: stream, events or the memory of %d frames of %d x %d", cfg->max_poses, cfg->rows,
                     cfg->cols);
    render_free(r);
    return FUELMI_ENOMEM;
  }
  {
    std::lock_guard<std::mutex> lk(g_render_mu);
    g_render_live.insert(r);
  }
  *out = r;
  return FUELMI_OK;
}

extern "C" int fuelmi_render_destroy(fuelmi_render* r) {
  {
    std::lock_guard<std::mutex> lk(g_render_mu);
    if (!r || g_render_live.erase(r) == 0) {
      fuelmi_set_error("fuelmi_render_destroy: not a live renderer (null, or destroyed before)");
      return FUELMI_EINVAL;
    }
  }
  render_free(r);
  return FUELMI_OK;
}

extern "C" int fuelmi_render_set_cloud(fuelmi_render* r, const float* xyz, int n_points) {
  RENDER_LIVE(r);
  const int rc = render_points_check(n_points);
  if (rc) return rc;
  ARGCHK(xyz || n_points == 0);
  HIPCHK(hipSetDevice(r->cfg.device));
  if ((size_t)n_points > r->cloud_cap) {
    HIPCHK(hipStreamSynchronize(r->stream));
    if (r->cloud) (void)hipFree(r->cloud);
    r->cloud = nullptr, r->cloud_cap = 0, r->has_cloud = false;
    if (hipMalloc(&r->cloud, (size_t)n_points * 3 * sizeof(float)) != hipSuccess) {
      (void)hipGetLastError();
      fuelmi_set_error("fuelmi_render_set_cloud: device memory of %d points", n_points);
      return FUELMI_ENOMEM;
    }
    r->cloud_cap = (size_t)n_points;
  }
  r->has_cloud = false;
  if (n_points) {
    HIPCHK(hipMemcpyAsync(r->cloud, xyz, (size_t)n_points * 3 * sizeof(float), hipMemcpyDefault, r->stream));
    HIPCHK(hipStreamSynchronize(r->stream));
  }
  r->n_points = n_points;
  r->has_cloud = true;
  return FUELMI_OK;
}

extern "C" int fuelmi_render_depth(fuelmi_render* r, int n_pose, const double* T_cw, const double* cam_pos,
                                   double k_depth_scaling_factor, float* metres, unsigned short* raw, int* stats) {
  RENDER_LIVE(r);
  ARGCHK(T_cw && cam_pos);
  if (n_pose < 1) {
    fuelmi_set_error("fuelmi_render_depth: %d poses (>= 1)", n_pose);
    return FUELMI_EINVAL;
  }
  if (n_pose > r->cfg.max_poses) {
    fuelmi_set_error("fuelmi_render_depth: %d poses, the renderer keeps %d", n_pose, r->cfg.max_poses);
    return FUELMI_ELIMIT;
  }
  if (!r->has_cloud) {
    fuelmi_set_error("fuelmi_render_depth: no cloud has been set");
    return FUELMI_EINVAL;
  }
  if (!(std::isfinite(k_depth_scaling_factor) && k_depth_scaling_factor > 0.0)) {
    fuelmi_set_error("fuelmi_render_depth: k_depth_scaling_factor %g (finite, > 0)", k_depth_scaling_factor);
    return FUELMI_EINVAL;
  }
  for (int i = 0; i < n_pose * 12; ++i) ARGCHK(std::isfinite(T_cw[i]));
  for (int i = 0; i < n_pose * 3; ++i) ARGCHK(std::isfinite(cam_pos[i]));
  const int n = r->n_points;
  if ((long long)n_pose * n > RENDER_MAX_RECORDS) {
    fuelmi_set_error("fuelmi_render_depth: %d poses x %d points (<= 2^28 records)", n_pose, n);
    return FUELMI_ELIMIT;
  }
  const int npix = r->cfg.rows * r->cfg.cols;
  const size_t fpix = (size_t)n_pose * npix;
  HIPCHK(hipSetDevice(r->cfg.device));
  const int rcs = r->scratch.reserve(r->stream, render_scratch_bytes(n_pose, n));
  if (rcs) return rcs;
  BlockLayout lay(r->scratch.base(), 256);
  RenderRec* recs = lay.take<RenderRec>((size_t)n_pose * (size_t)std::max(n, 1));
  RenderPose* hp = (RenderPose*)r->pin;
  u32* hc = (u32*)(hp + r->cfg.max_poses);
  for (int k = 0; k < n_pose; ++k) {
    const double* T = T_cw + 12 * k;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) hp[k].R[3 * i + j] = T[4 * i + j], hp[k].Rf[3 * i + j] = (float)T[4 * i + j];
      hp[k].t[i] = T[4 * i + 3], hp[k].tf[i] = (float)T[4 * i + 3];
      hp[k].pos[i] = cam_pos[3 * k + i];
    }
  }
  hipStream_t st = r->stream;
  r->timed = false;
  HIPCHK(hipMemcpyAsync(r->d_poses, hp, (size_t)n_pose * sizeof(RenderPose), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(r->d_cnt, 0, (size_t)n_pose * RC_N * sizeof(u32), st));
  if (!r->keys_clean) HIPCHK(hipMemsetAsync(r->keys, 0xFF, (size_t)r->cfg.max_poses * npix * sizeof(u32), st));
  r->keys_clean = false;  // until this call has converted what it splats
  const RenderGeom g = render_geom(npix, n);
  const bool host_node = r->cfg.model == FUELMI_RENDER_HOST_NODE;
  HIPCHK(hipEventRecord(r->ev[0], st));
  if (n > 0) {
    if (host_node)
      hipLaunchKernelGGL(k_render_project<FUELMI_RENDER_HOST_NODE>, dim3(g.project_wg, n_pose), dim3(RENDER_PROJECT_THREADS), 0,
                         st, r->cloud, n, r->d_poses, r->cam, recs, r->d_cnt);
    else
      hipLaunchKernelGGL(k_render_project<FUELMI_RENDER_CUDA_NODE>, dim3(g.project_wg, n_pose), dim3(RENDER_PROJECT_THREADS), 0,
                         st, r->cloud, n, r->d_poses, r->cam, recs, r->d_cnt);
  }
  HIPCHK(hipEventRecord(r->ev[1], st));
  if (n > 0)
    hipLaunchKernelGGL(k_render_splat, dim3(g.splat_wg, n_pose), dim3(RENDER_SPLAT_THREADS), 0, st, recs, n, r->d_cnt, r->keys,
                       r->cfg.cols, npix);
  HIPCHK(hipEventRecord(r->ev[2], st));
  const float kf = (float)k_depth_scaling_factor;
  if (host_node)
    hipLaunchKernelGGL(k_render_convert<FUELMI_RENDER_HOST_NODE>, dim3(g.convert_wg, n_pose), dim3(RENDER_CONVERT_THREADS), 0, st,
                       r->keys, r->metres, r->raw, r->d_cnt, npix, kf);
  else
    hipLaunchKernelGGL(k_render_convert<FUELMI_RENDER_CUDA_NODE>, dim3(g.convert_wg, n_pose), dim3(RENDER_CONVERT_THREADS), 0, st,
                       r->keys, r->metres, r->raw, r->d_cnt, npix, kf);
  HIPCHK(hipEventRecord(r->ev[3], st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(hc, r->d_cnt, (size_t)n_pose * RC_N * sizeof(u32), hipMemcpyDeviceToHost, st));
  if (metres) HIPCHK(hipMemcpyAsync(metres, r->metres, fpix * sizeof(float), hipMemcpyDeviceToHost, st));
  if (raw) HIPCHK(hipMemcpyAsync(raw, r->raw, fpix * sizeof(unsigned short), hipMemcpyDeviceToHost, st));
  HIPCHK(stream_wait(st));
  r->keys_clean = true;
  r->timed = true;
  if (stats)
    for (int k = 0; k < n_pose; ++k) {
      stats[4 * k + 0] = (int)(hc[RC_N * k + RC_SMALL] + hc[RC_N * k + RC_LARGE]);
      stats[4 * k + 1] = (int)hc[RC_N * k + RC_UNDEF];
      stats[4 * k + 2] = (int)hc[RC_N * k + RC_PIXELS];
      stats[4 * k + 3] = 0;
    }
  return FUELMI_OK;
}

extern "C" const unsigned short* fuelmi_render_frame_raw(const fuelmi_render* r, int k) {
  if (!render_live(r) || k < 0 || k >= r->cfg.max_poses) {
    fuelmi_set_error("fuelmi_render_frame_raw: not a live renderer, or frame %d outside its max_poses", k);
    return nullptr;
  }
  return r->raw + (size_t)k * r->cfg.rows * r->cfg.cols;
}
extern "C" const float* fuelmi_render_frame_metres(const fuelmi_render* r, int k) {
  if (!render_live(r) || k < 0 || k >= r->cfg.max_poses) {
    fuelmi_set_error("fuelmi_render_frame_metres: not a live renderer, or frame %d outside its max_poses", k);
    return nullptr;
  }
  return r->metres + (size_t)k * r->cfg.rows * r->cfg.cols;
}

extern "C" int fuelmi_render_times(const fuelmi_render* r, double ms3[3]) {
  RENDER_LIVE(r);
  ARGCHK(ms3);
  if (!r->timed) {
    fuelmi_set_error("fuelmi_render_times: no completed render to report");
    return FUELMI_EINVAL;
  }
  for (int i = 0; i < 3; ++i) {
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, r->ev[i], r->ev[i + 1]));
    ms3[i] = ms;
  }
  return FUELMI_OK;
}
