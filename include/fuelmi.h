/*
 * fuelmi.h -- C-ABI of libfuelmi.so: the MI355X (gfx950) implementation of FUEL's per-cycle
 * mapping-and-planning hot path.  Plain C types only (no torch / Eigen / ROS in any signature).
 *
 * The reference has no FFI layer: the path sits behind three C++ class APIs
 * (fast_planner::SDFMap / EDTEnvironment, FrontierFinder, BsplineOptimizer).  The C++ facade in
 * fuel_amd/facade/ re-declares those classes over this C-ABI.  Every entry
 * point below names the reference interface it replaces; paths are relative to
 * /root/reference/fuel_planner/.
 *
 * Conventions
 *   - every function returns 0 on success, a negative FUELMI_E* code on failure, and never
 *     throws or aborts; fuelmi_last_error() returns a thread-local message for the last failure.
 *   - voxel linear address: adr = x*ny*nz + y*nz + z  (plan_env/include/plan_env/sdf_map.h:145-147)
 *   - one HIP stream per map; mutators of one map must be called from one thread at a time
 *     (the reference runs them on the single ros::spin thread); different maps are independent.
 *     Host-staged queries (dist_grad, coarse_dist, query_state, sync_host) may run from other threads
 *     beside a mutator: they and the fusion entry points share the map's staging buffers under a per-map mutex.
 *     Ordering of a distance query (dist_grad, coarse_dist, the one-shot B-spline calls) against ESDF updates of the
 *     same map: it sees the field either before or after an update, never a mix -- a query issued while an update is
 *     queued or running waits for it on the device, an update queued behind launched query kernels waits for them,
 *     and a reader / writer lock keeps a query from slipping between the two (with signed_dist a reader can
 *     therefore never see the positive-only intermediate the negative pass merges into in place).
 *   - all work is done by HIP kernels; there is no CPU fallback.  If no gfx950 device is
 *     usable fuelmi_map_create fails with FUELMI_ENODEV.
 */
#ifndef FUELMI_H_
#define FUELMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FUELMI_OK 0
#define FUELMI_EINVAL (-1)  /* bad argument */
#define FUELMI_ENODEV (-2)  /* no usable HIP device */
#define FUELMI_EHIP (-3)    /* HIP runtime error (message in fuelmi_last_error) */
#define FUELMI_ENOMEM (-4)
#define FUELMI_ELIMIT (-5)  /* problem exceeds a documented limit */

/* Process-level set-up: hardware queues.  A map owns one HIP stream, a finder two, every busy query thread one; the HIP
 * runtime deals a process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default) and streams that share one
 * time-slice (INTEGRATION.md "streams and queues").  The runtime latches the variable at its first call, so the robust
 * way is to export GPU_MAX_HW_QUEUES where the process is launched.  fuelmi_init() is the explicit in-process
 * alternative (rounds 4-5 did this from a load-time constructor; that is now opt-in, FUELMI_SET_HW_QUEUES=1): called
 * BEFORE the process's first HIP call and before threads that touch the environment exist, it puts
 * GPU_MAX_HW_QUEUES=<hw_queues capped at 2, 2 if <= 0> into the environment unless a value is already there.  Idempotent; always
 * returns FUELMI_OK and reports through fuelmi_hw_queues_state() what happened -- including FUELMI_HWQ_LATE when the HIP
 * runtime was already up (it is detected through the runtime's open /dev/kfd handle; one line on stderr unless
 * FUELMI_QUIET is set): the streams then share the runtime's default of 4 queues.  fuelmi_map_create says so once on
 * stderr when neither the environment nor fuelmi_init() decided. */
#define FUELMI_HWQ_UNINIT 0 /* fuelmi_init() not called: the runtime sees the environment as it is */
#define FUELMI_HWQ_SET 1    /* set by fuelmi_init() before the HIP runtime initialised: in effect */
#define FUELMI_HWQ_ENV 2    /* the environment already held a value: kept */
#define FUELMI_HWQ_LATE 3   /* the HIP runtime was initialised first without the variable: its default (4) is in effect */
int fuelmi_init(int hw_queues);
/* the number of hardware queues the process's HIP runtime uses, as far as the library can know it: the environment's
 * value (4 if unset), or 4 in state FUELMI_HWQ_LATE */
int fuelmi_hw_queues(void);
int fuelmi_hw_queues_state(void);
const char* fuelmi_last_error(void);
const char* fuelmi_version(void);
/* number of visible HIP devices (0 if none / runtime unusable) */
int fuelmi_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Map: replaces fast_planner::SDFMap  (plan_env/include/plan_env/sdf_map.h:27-84)
 * ---------------------------------------------------------------------------------------- */

/* the ROS parameters SDFMap::initMap reads (plan_env/src/sdf_map.cpp:19-47,78-82) */
typedef struct {
  double resolution;          /* sdf_map/resolution */
  double map_size[3];         /* sdf_map/map_size_{x,y,z} */
  double ground_height;       /* sdf_map/ground_height */
  double obstacles_inflation; /* sdf_map/obstacles_inflation */
  double local_bound_inflate; /* sdf_map/local_bound_inflate */
  double default_dist;        /* sdf_map/default_dist */
  int optimistic;             /* sdf_map/optimistic */
  int signed_dist;            /* sdf_map/signed_dist */
  double p_hit, p_miss, p_min, p_max, p_occ;
  double max_ray_length;      /* sdf_map/max_ray_length */
  double virtual_ceil_height; /* sdf_map/virtual_ceil_height */
  double box_min[3], box_max[3]; /* sdf_map/box_{min,max}_{x,y,z} (exploration box) */
  int device;                 /* HIP device ordinal this map lives on */
} fuelmi_map_cfg;

/* derived constants, as initMap computes them (sdf_map.cpp:30-56,78-84) */
typedef struct {
  int voxel_num[3];
  double origin[3];
  double min_boundary[3], max_boundary[3];
  double resolution_inv;
  int box_min[3], box_max[3];           /* posToIndex of the exploration box */
  double prob_hit_log, prob_miss_log, clamp_min_log, clamp_max_log, min_occupancy_log;
  int inflate_step;                     /* ceil(obstacles_inflation / resolution) */
} fuelmi_map_info;

typedef struct fuelmi_map fuelmi_map;

/* SDFMap::initMap (sdf_map.cpp:12-93): allocates the device grid, all voxels unknown */
int fuelmi_map_create(const fuelmi_map_cfg* cfg, fuelmi_map** out);
void fuelmi_map_destroy(fuelmi_map* m);
int fuelmi_map_get_info(const fuelmi_map* m, fuelmi_map_info* info);

/* SDFMap::inputPointCloud (sdf_map.cpp:259-345).  xyz: n points, float x,y,z at the start of
 * each stride_bytes record (12 for packed, 16 for pcl::PointXYZ); host memory. */
int fuelmi_map_input_points(fuelmi_map* m, const float* xyz, int stride_bytes, int n,
                            const double camera_pos[3]);
/* The geometry the fusion kernels are compiled with (host only, no device needed): out[0] = lanes that share one ray
 * walk, out[1] = point slots per workgroup of the ray-walk kernel, out[2] = point slots per workgroup of the classify
 * kernel (whose end-point box places the miss cube of the ray workgroups inside it), out[3..5] = x, y, z extent in
 * voxels of the miss cube a ray workgroup collects in LDS, out[6..7] = 0.  For tests that aim at these edges. */
int fuelmi_map_insert_plan(int out[8]);
/* Depth-image front end of the fusion: MapROS::proessDepthImage (plan_env/src/map_ros.cpp:176-215) and
 * the part of MapROS::depthPoseCallback (:121-150) around it.  Parameters are the map_ros/... ROS
 * parameters of the same names (map_ros.cpp:22-30). */
typedef struct {
  double fx, fy, cx, cy;
  double depth_filter_maxdist, depth_filter_mindist;
  int depth_filter_margin;
  double k_depth_scaling_factor; /* raw 16-bit depth units per metre (1000 for millimetres) */
  int skip_pixel;
} fuelmi_depth_cfg;
/* depth: rows x cols row-major 16UC1 image; cam_q_wxyz: camera orientation quaternion (pose->orientation, w
 * first).  The image may lie in pageable host memory (a cv::Mat: staged through a pinned buffer, free again on
 * return), in pinned / registered host memory (fuelmi_host_register: read in place over PCIe) or in device memory
 * (read in place); in the last two cases the caller leaves it unchanged until its next call on this map.  Projects on the device and fuses the points without a host round
 * trip; a frame taken from outside the map is ignored like the reference does.  *n_points (may be
 * NULL) receives proj_points_cnt.  Follow with fuelmi_map_inflate_local (local_updated_ branch). */
int fuelmi_host_register(void* ptr, size_t bytes); /* hipHostRegister(mapped) of a frame ring; undo with _unregister
                                                     * BEFORE the memory is freed (a registration that outlives its
                                                     * memory makes later copies from that address range fail) */
int fuelmi_host_unregister(void* ptr);
/* plain device buffers for callers without a HIP runtime of their own (tests, bench.py) */
int fuelmi_device_alloc(int device, size_t bytes, void** out);
int fuelmi_device_upload(void* dst, const void* src, size_t bytes);
int fuelmi_device_free(void* ptr);
/* STREAM-triad over three device arrays of `bytes` each: the HBM bandwidth a plain kernel reaches on this device
 * (reported by bench.py beside the vendor peak the rooflines are quoted against). */
int fuelmi_hbm_triad(int device, size_t bytes, int reps, double* gb_per_s);
/* the same for the x pass's traffic mix: bytes_in of 16-bit values read, 2 * bytes_in of floats written; reports
 * 3 * bytes_in / time */
int fuelmi_hbm_expand(int device, size_t bytes_in, int reps, double* gb_per_s);
int fuelmi_map_input_depth(fuelmi_map* m, const unsigned short* depth, int rows, int cols,
                           const fuelmi_depth_cfg* cfg, const double cam_pos[3], const double cam_q_wxyz[4],
                           int* n_points);
/* projection only: the reference's point_cloud_[0..proj_points_cnt) as packed float xyz (host). */
int fuelmi_map_project_depth(fuelmi_map* m, const unsigned short* depth, int rows, int cols,
                             const fuelmi_depth_cfg* cfg, const double cam_pos[3], const double cam_q_wxyz[4],
                             float* xyz, int cap, int* n_points);
/* SDFMap::clearAndInflateLocalMap (sdf_map.cpp:434-471) over the current local bound */
int fuelmi_map_inflate_local(fuelmi_map* m);
/* SDFMap::updateESDF3d (sdf_map.cpp:152-241) over the current local bound */
int fuelmi_map_update_esdf(fuelmi_map* m);
/* Which kernel family runs the update (all are exact -- they differ in how far the outward scans of the y / x passes
 * look).  AUTO (default): chosen per update from the far-output statistic of the slabs the local
 * bound covers; PLAIN: the packed 16-bit z/y pass (falls back to PLAIN32 for boxes it does not cover: z extents above
 * 255 voxels, nz % 4 != 0); FAR: the far-field kernels (block / line minima); PLAIN32: the 32-bit plain z/y pass.
 * fuelmi_map_last_esdf_family returns the family the z/y pass of the last update actually ran (tests assert the
 * choice instead of a duration). */
enum { FUELMI_ESDF_AUTO = -1, FUELMI_ESDF_PLAIN = 0, FUELMI_ESDF_FAR = 1, FUELMI_ESDF_PLAIN32 = 2 };
int fuelmi_map_set_esdf_family(fuelmi_map* m, int family);
int fuelmi_map_last_esdf_family(const fuelmi_map* m);
/* The launches fuelmi_map_update_esdf issues for a box (host only, no device needed; the plan the update itself runs).
 * dims: grid voxels; lo / hi: the inclusive box; family: PLAIN / FAR / PLAIN32 (AUTO is resolved per update from the
 * statistic and refused here); flags: FUELMI_ESDF_PLAN_OPTIMISTIC | FUELMI_ESDF_PLAN_SIGNED.  The hand-over buffer of the
 * packed family is taken at the size a map of dims allocates.  out[0] = launches (2, or 4 with SIGNED), out[1] = the
 * family fuelmi_map_last_esdf_family then reports, then 10 ints per launch in order z/y+, x+, z/y-, x-: kernel
 * (FUELMI_ESDF_K_*), its three template arguments in declaration order (0 where it has fewer), grid, block, dynamic LDS
 * bytes, ZC, nzc, z0a.  FUELMI_ELIMIT, with the update's message, for a box the update refuses. */
enum {
  FUELMI_ESDF_K_ZY = 0,     /* k_esdf_zy<MODE>                  (z/y kernels first) */
  FUELMI_ESDF_K_ZY4 = 1,    /* k_esdf_zy4<MODE, FAR> */
  FUELMI_ESDF_K_ZY_PK2 = 2, /* k_esdf_zy_pk2<MODE, G, NW> */
  FUELMI_ESDF_K_X = 3,      /* k_esdf_x<S, OUT> */
  FUELMI_ESDF_K_X4 = 4,     /* k_esdf_x4<OUT, SEGS, FAR> */
  FUELMI_ESDF_K_X_PK2 = 5   /* k_esdf_x_pk2<OUT> */
};
enum { FUELMI_ESDF_PLAN_OPTIMISTIC = 1, FUELMI_ESDF_PLAN_SIGNED = 2, FUELMI_ESDF_PLAN_INTS = 42 };
int fuelmi_map_esdf_plan(const int dims[3], const int lo[3], const int hi[3], int family, int flags,
                         int out[FUELMI_ESDF_PLAN_INTS]);
/* which inflation kernels the last fuelmi_map_inflate_local ran: 0 the fused single launch, 1 the factored y/z + x pair
 * (chosen by the size of the box's address range; -1 before the first call).  For tests that must know which code ran. */
int fuelmi_map_last_inflate_kernel(const fuelmi_map* m);
/* Pins that choice (tests, A/B runs; both forms compute the same bits).  AUTO (default): by the step and the size of the
 * box's address range; FUSED: the single launch, which exists for an inflation step of 2 only -- FUELMI_EINVAL on a map
 * with another step; FACTORED: the y/z + x pair, any step.  The codes are fuelmi_map_last_inflate_kernel's. */
enum { FUELMI_INFLATE_AUTO = -1, FUELMI_INFLATE_FUSED = 0, FUELMI_INFLATE_FACTORED = 1 };
int fuelmi_map_set_inflate_kernel(fuelmi_map* m, int kernel);
/* The word ranges and launches fuelmi_map_inflate_local uses for a box (host only, no device needed; the plan the call
 * itself runs).  dims: grid voxels; step: the map's inflate_step (0..31); lo / hi: the inclusive box; kernel: a pin as
 * above.  out[0] = the kernel that runs (0 fused, 1 factored), out[1] = margin words either side of every bit-plane,
 * out[2] = W (words that cover the grid), out[3..4] = first / last output word, out[5..6] = first / last word of the
 * y/z-dilated plane the x pass reads, out[7..8] = first / last word of the box-masked source plane, out[9] = 1 if the
 * box is the whole map (no masking pass), out[10] = dynamic LDS bytes of the fused kernel, out[11] = its grid,
 * out[12..14] = grids of the masking pass (0 if none), the y/z pass and the x pass (a multiple of 8), out[15] = 0; grids
 * of the form that does not run are 0.  FUELMI_EINVAL for a box that leaves the grid or FUSED with a step other than 2,
 * FUELMI_ELIMIT for a grid or a step a map refuses. */
enum { FUELMI_INFLATE_PLAN_INTS = 16 };
int fuelmi_map_inflate_plan(const int dims[3], int step, const int lo[3], const int hi[3], int kernel,
                            int out[FUELMI_INFLATE_PLAN_INTS]);
/* SDFMap::resetBuffer() (sdf_map.cpp:95-99) and resetBuffer(min,max) (:101-114) */
int fuelmi_map_reset_buffer_all(fuelmi_map* m);
int fuelmi_map_reset_buffer(fuelmi_map* m, const double min_pos[3], const double max_pos[3]);
/* SDFMap::setOccupied (sdf_map.h:210-215) for n positions; occ must be 0 or 1 */
int fuelmi_map_set_occupied(fuelmi_map* m, const double* pos_xyz, int n, int occ);
/* md_->local_bound_min_/max_ (inclusive voxel indices).  The reference sets them inside
 * inputPointCloud / resetBuffer(); the setter lets a caller run "full-box" updates. */
int fuelmi_map_get_local_bound(const fuelmi_map* m, int bmin[3], int bmax[3]);
int fuelmi_map_set_local_bound(fuelmi_map* m, const int bmin[3], const int bmax[3]);
/* SDFMap::getUpdatedBox (sdf_map.cpp:491-495); setter for callers that fuse elsewhere */
int fuelmi_map_get_updated_box(fuelmi_map* m, double bmin[3], double bmax[3], int reset);
int fuelmi_map_set_updated_box(fuelmi_map* m, const double bmin[3], const double bmax[3]);

/* Bulk load of occupancy_buffer_ (log-odds, double[N], host) -- replaces nothing in the
 * reference (its buffers are host vectors); used to restore a map / build benchmarks. */
int fuelmi_map_upload_occupancy(fuelmi_map* m, const double* occ);

/* Host mirrors for the reference's inline getters (sdf_map.h:196-237 read host vectors
 * directly).  Each non-NULL pointer is a full-size host buffer laid out like the reference's
 * (occupancy_buffer_ double[N], occupancy_buffer_inflate_ char[N], distance_buffer_ double[N]);
 * exactly the voxels inside [bmin,bmax] (inclusive indices; NULL = whole map) are refreshed from
 * the device, with one stream synchronisation per call. */
int fuelmi_map_sync_host(fuelmi_map* m, const int bmin[3], const int bmax[3], double* occupancy,
                         char* inflate, double* distance);
/* Optional, once per mirror buffer: pins the caller's full-size buffers where they lie (any may be NULL)
 * and maps them into the device address space.  fuelmi_map_sync_host calls naming a registered buffer
 * then store the box voxels straight into it -- one kernel, box-limited PCIe traffic, one
 * synchronisation -- instead of staging them.  The buffers must outlive the registration
 * (fuelmi_map_unregister_mirrors / fuelmi_map_destroy end it). */
int fuelmi_map_register_mirrors(fuelmi_map* m, double* occupancy, char* inflate, double* distance);
int fuelmi_map_unregister_mirrors(fuelmi_map* m);

/* SDFMap::getDistWithGrad (sdf_map.cpp:497-536) == EDTEnvironment::evaluateEDTWithGrad
 * (plan_env/src/edt_environment.cpp:78-87) for n host positions; re-entrant w.r.t. queries */
int fuelmi_map_dist_grad(fuelmi_map* m, const double* pos_xyz, int n, double* dist, double* grad_xyz);
/* SDFMap::getDistance(pos) == EDTEnvironment::evaluateCoarseEDT(pos,-1) (edt_environment.cpp:89-97) */
int fuelmi_map_coarse_dist(fuelmi_map* m, const double* pos_xyz, int n, double* dist);
/* SDFMap::getOccupancy / getInflateOccupancy for n voxel indices (-1 outside the map) */
int fuelmi_map_query_state(fuelmi_map* m, const int* idx_xyz, int n, int* occupancy, int* inflate);

int fuelmi_map_synchronize(fuelmi_map* m);

/* ------------------------------------------------------------------------------------------
 * Frontier scan + clustering: replaces the grid part of active_perception::FrontierFinder
 * (active_perception/src/frontier_finder.cpp:54-164 searchFrontiers/expandFrontier,
 *  :353-390 haveOverlap/isFrontierChanged/computeFrontierInfo, :811-881 neighbour helpers)
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int cluster_min; /* frontier/cluster_min */
  double min_z;    /* the literal 0.4 at frontier_finder.cpp:151 */
  /* splitLargeFrontiers (frontier_finder.cpp:166-242) + computeFrontierInfo's down-sampling (:374-390,757-774) */
  double cluster_size_xy; /* frontier/cluster_size_xy (2.0) */
  int down_sample;        /* frontier/down_sample (3): VoxelGrid leaf = down_sample * resolution */
  int split;              /* 0: search stops before splitLargeFrontiers; 1: it runs, and every new cluster
                             carries its filtered_cells_ */
  int reference_order;    /* 0 (default): a cluster lists its cells in ascending voxel address and its mean is
                             evaluated order-free (exact integer sums) -- the fast path.  1: the reference's own
                             order -- cells in the BFS order of expandFrontier (frontier_finder.cpp:123-164,
                             neighbour order :848-860), average_ as its sequential f64 sum (:374-390), VoxelGrid
                             centroids accumulated in that order (:757-774) -- so that means, filtered_cells_,
                             split pieces and viewpoints reproduce the reference bit for bit; costs one BFS
                             level sweep per cluster on the device and host-side means (clusters of up to 26624
                             cells are swept inside LDS: +0.15 ... 0.6 ms per search as measured on the streaming
                             workload; larger ones through L2: 24 ms for the 140 k cells of a full 400x400x100
                             box).  2 ("auto"): the reference's order for every search whose clusters all hold at
                             most 26624 cells -- the incremental searches of an exploration run -- and the address
                             order for the giant ones */
} fuelmi_frontier_cfg;

typedef struct fuelmi_frontier fuelmi_frontier;

int fuelmi_frontier_create(fuelmi_map* m, const fuelmi_frontier_cfg* cfg, fuelmi_frontier** out);
void fuelmi_frontier_destroy(fuelmi_frontier* f);
/* forget all clusters and clear frontier_flag_ (== constructing a fresh FrontierFinder,
 * frontier_finder.cpp:23-27) */
int fuelmi_frontier_reset(fuelmi_frontier* f);
/* diagnostics: searches answered by the fast clustering chain [0], by the legacy chain [1], and searches that
 * started on the fast chain and fell back because an input exceeded one of its capacities [2] */
int fuelmi_frontier_stats(const fuelmi_frontier* f, int out3[3]);
/* of the searches the fast chain answered: how many were resolved (cross-tile unions, cluster records, the result the
 * caller polls for) by the last workgroup of the chain's second kernel itself rather than by a launch of their own --
 * searches of up to 1 024 tile-local components; for tests that must know which code ran */
int fuelmi_frontier_resolved_in_launch(const fuelmi_frontier* f);
/* of the searches the fast chain answered: [0] how many outgrew the launch that was to resolve them with no resolve
 * launch queued behind it (the library queued one after the chain had reported), [1] how many ran the chain again on
 * a smaller tile after a per-tile capacity overflow; for tests that must know which code ran */
int fuelmi_frontier_path_stats(const fuelmi_frontier* f, int out2[2]);
/* the changed-cluster test that runs in front of a search with committed clusters whose box overlaps the updated box
 * (searchFrontiers' removal of outdated clusters): [0..3] launches of each of its four paths -- one workgroup, one
 * launch with an in-kernel barrier, two launches on a candidate table staged in LDS, two launches on a table in device
 * memory --; of the last test: [4] its candidates, [5] their pooled cells, [6] its mark (0 for the one-workgroup path);
 * [7] rebuilds of the device pool of committed cells so far, [8] the pool's capacity in cells.  For tests that must know
 * which code ran */
int fuelmi_frontier_changed_stats(const fuelmi_frontier* f, int out[9]);
/* the cell order the searches delivered (cfg.reference_order is a request; mode 2 answers per search): [0] the last
 * search's order -- 0 ascending address, 1 the reference's BFS order --, [1] searches that delivered the reference's
 * order, [2] searches of a mode-2 finder that fell back to the address order because a cluster was too large for the
 * in-LDS level sweep, [3] cells of the largest cluster of the last such search.  A caller that needs the reference's
 * bits checks [0] after fuelmi_frontier_search_end (the facade logs the first fallback). */
int fuelmi_frontier_order_stats(const fuelmi_frontier* f, int out4[4]);
/* waits for everything queued on the finder's stream.  fuelmi_frontier_search_end returns as soon as the cluster
 * records have arrived; the regrouping of the cells and their copy to the host finish behind it (calls that read
 * cell lists wait by themselves) */
int fuelmi_frontier_synchronize(fuelmi_frontier* f);
/* Viewpoint sampling and coverage (frontier_finder.cpp:392-423,662-755,697-719; camera frustum
 * perception_utils.cpp:6-19,49-69,84-93).  Fields are the ROS parameters of the same names. */
typedef struct {
  double candidate_rmin, candidate_rmax; /* frontier/candidate_rmin, candidate_rmax */
  int candidate_rnum;                    /* frontier/candidate_rnum */
  double candidate_dphi;                 /* frontier/candidate_dphi */
  double min_candidate_clearance;        /* frontier/min_candidate_clearance */
  int min_visib_num;                     /* frontier/min_visib_num */
  double min_candidate_dist;             /* frontier/min_candidate_dist (used by the Top/ViewpointsInfo getters) */
  double min_view_finish_fraction;       /* frontier/min_view_finish_fraction */
  double top_angle, left_angle, right_angle, max_dist; /* perception_utils/... */
} fuelmi_viewpoint_cfg;
int fuelmi_frontier_set_viewpoint_cfg(fuelmi_frontier* f, const fuelmi_viewpoint_cfg* cfg);
/* computeFrontiersToVisit: samples viewpoints for every new cluster (needs cfg.split, i.e. filtered
 * cells, and the map's CURRENT inflated occupancy); clusters with at least one viewpoint are appended
 * to frontiers_ with their viewpoints sorted by coverage (best first), the others to
 * dormant_frontiers_.  The new-cluster list is left empty. */
int fuelmi_frontier_compute_to_visit(fuelmi_frontier* f, int* n_active_new, int* n_dormant_new);
int fuelmi_frontier_viewpoint_count(const fuelmi_frontier* f, int which, int k);
/* pos_yaw4: x, y, z, yaw per viewpoint; visib: Viewpoint::visib_num_ */
int fuelmi_frontier_viewpoints(const fuelmi_frontier* f, int which, int k, double* pos_yaw4, int* visib);
/* isFrontierCovered against the map's accumulated updated box (the box is not consumed) */
int fuelmi_frontier_is_covered(fuelmi_frontier* f, int* covered);
/* Frontier::filtered_cells_ of cluster k (VoxelGrid centroids, float xyz, ascending leaf index like PCL);
 * empty unless the cluster was found with cfg.split != 0 */
int fuelmi_frontier_cluster_filtered_size(const fuelmi_frontier* f, int which, int k);
int fuelmi_frontier_cluster_filtered(const fuelmi_frontier* f, int which, int k, float* xyz);
/* searchFrontiers up to (not including) splitLargeFrontiers: consumes the map's updated box
 * (getUpdatedBox(reset=true)), drops changed clusters, scans, clusters.  *n_new = number of new
 * clusters (tmp_frontiers_.size()). */
int fuelmi_frontier_search(fuelmi_frontier* f, int* n_new);
/* The same search split in two: _begin queues the test for changed clusters and the device pipeline on
 * the frontier's own HIP stream without waiting; _end waits, drops the changed clusters from
 * frontiers_ / dormant_frontiers_ (removed_ids_) and assembles the new ones.  Work queued on the map
 * between the two calls (inflation, ESDF, B-spline evaluation) overlaps the scan, which only reads the
 * occupancy state.  The next frame MAY be fused between _begin and _end (a streaming pipeline: fuelmi_bench_stream):
 * the search reads the occupancy planes only in its first kernels and the fusion waits for those on the device.
 * _commit, _reset, _compute_to_visit, _is_covered and a second _begin return FUELMI_EINVAL until _end has been called. */
int fuelmi_frontier_search_begin(fuelmi_frontier* f);
int fuelmi_frontier_search_end(fuelmi_frontier* f, int* n_new);
/* Pipelined delivery for callers that work in cycles (fresh search every cycle): with keep_previous on,
 * fuelmi_frontier_reset does not discard the new clusters of the search it retires -- they become list 3 and stay
 * readable (size / cells / centres / info) until the NEXT reset: their cell lists live in the buffer set the reset
 * retires, which nothing touches for a whole cycle.  Reading list 3 waits only for that search's own tail, so cycle
 * k - 1's cells are copied out while cycle k runs on the device. */
int fuelmi_frontier_keep_previous(fuelmi_frontier* f, int on);
/* move tmp_frontiers_ into frontiers_ (dormant=0) or dormant_frontiers_ (dormant=1) */
int fuelmi_frontier_commit(fuelmi_frontier* f, int dormant);
/* which: 0 tmp_frontiers_, 1 frontiers_, 2 dormant_frontiers_, 3 the new clusters of the search before the last reset
 * (fuelmi_frontier_keep_previous) */
int fuelmi_frontier_count(const fuelmi_frontier* f, int which);
int fuelmi_frontier_cluster_size(const fuelmi_frontier* f, int which, int k);
/* cells of cluster k as linear voxel addresses, ascending (the reference keeps BFS order;
 * the SET is identical) */
int fuelmi_frontier_cluster_cells(const fuelmi_frontier* f, int which, int k, int* adr);
/* the same cells as voxel CENTRES, xyz[3 * size] doubles (the storage of the reference's vector<Vector3d> cells_,
 * frontier_finder.h:27): indexToPos of every cell (sdf_map.h:137-140), same order as _cluster_cells.  Clusters of 32 768
 * cells and more are decoded by the calling thread and three helper threads of the library (created on first use, parked
 * on a condition variable between calls, shared by all finders of the process; FUELMI_HOST_HELPERS=0 keeps everything on
 * the caller) */
int fuelmi_frontier_cluster_centres(const fuelmi_frontier* f, int which, int k, double* xyz);
/* average_[3], box_min_[3], box_max_[3] (computeFrontierInfo) */
int fuelmi_frontier_cluster_info(const fuelmi_frontier* f, int which, int k, double out9[9]);
int fuelmi_frontier_removed_count(const fuelmi_frontier* f);
int fuelmi_frontier_removed_ids(const fuelmi_frontier* f, int* ids);
/* frontier_flag_ expanded to one byte per voxel (char[N], host) -- for tests/debug */
int fuelmi_frontier_get_flags(fuelmi_frontier* f, char* flags);

/* ------------------------------------------------------------------------------------------
 * Viewpoint path costs: ViewNode::searchPath (active_perception/src/graph_node.cpp:32-61) for a batch of
 * pairs, the entries of the tour cost matrix (frontier_finder.cpp:260-326, 508-592).  Per pair:
 *   kind 0: the straight line p1 -> p2 (RayCaster walk from p1's voxel, stopping before p2's) meets no voxel
 *           that is inflated, UNKNOWN or outside the index box: length = |p1 - p2|, path {p1, p2} -- bit for
 *           bit the reference;
 *   kind 1: the shortest path on the 26-connected lattice p1 + n * lattice_res under Astar::search's edge test
 *           (path_searching/src/astar2.cpp:86-113, samples every edge_step) to the goal node -- posToIndex at
 *           lattice_res within +-1 of p2's -- minimising d + |p2 - node|; path [p1, nodes..., p2], length its
 *           sequential sum of segment norms (Astar::pathLength).  Deterministic, without the reference's
 *           wall-clock cap (DESIGN.md section 10 lists the differences);
 *   kind 2: no goal reachable: length = no_path_cost, path {p1, p2}.
 * Reads the map's current inflated / unknown planes on the map's stream; same thread rule as the mutators.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  double lattice_res;  /* 0.4 (graph_node.cpp:49) */
  double edge_step;    /* 0.1 (astar2.cpp:105) */
  double no_path_cost; /* 1000 (graph_node.cpp:60) */
  int max_path_points; /* points per pair in path_xyz */
} fuelmi_path_cfg;
/* p1_xyz, p2_xyz: n points each (host).  length[n], kind[n], path_len[n] (points of each path, always the full
 * count).  path_xyz: n x max_path_points x 3 (host), may be NULL.  If a path has more than max_path_points points
 * the call fills length / kind / path_len (and the paths that fit) and returns FUELMI_ELIMIT. */
int fuelmi_map_path_costs(fuelmi_map* m, const fuelmi_path_cfg* cfg, int n, const double* p1_xyz,
                          const double* p2_xyz, double* length, int* kind, int* path_len, double* path_xyz);
/* what the last fuelmi_map_path_costs or fuelmi_map_refine_tours on this map did: [0] relaxation launches in all, [1]
 * the most of one chunk of sources, [2] lattice sources, [3] chunks.  After a refinement with a polyline: the sums
 * (the most: the larger) over its edge searches and its polyline legs. */
int fuelmi_map_path_stats(const fuelmi_map* m, int stats[4]);

/* ------------------------------------------------------------------------------------------
 * Local tour refinement: FastExplorationManager::refineLocalTour (exploration_manager/src/
 * fast_exploration_manager.cpp:429-503) and the single-destination choice (:185-220), for n_prob independent
 * problems in one call.  Problem b: node 0 = the start (pos, vel, yaw), then its layers in order (one per cluster
 * of the global tour, nodes = the top viewpoints, FrontierFinder::getViewpointsInfo).  Every node of layer i-1 links
 * to every node of layer i; the last layer keeps only its first node (:459-462) unless FUELMI_REFINE_LAST_ARGMIN.
 * Edge cost = ViewNode::computeCost (active_perception/src/graph_node.cpp:63-88) on the edge's searchPath length
 * (fuelmi_map_path_costs, cfg.path): max(length / vm + [|v| > 1e-3] w_dir acos(v^ . normalized(p2 - p1)),
 * min(|dy|, 2 pi - |dy|) / yd) with std::max's NaN rule (a NaN edge is never taken) and real Eigen's normalized()
 * (a zero-length edge adds w_dir pi / 2); only the start has a velocity.  Search = GraphSearch::DijkstraSearch
 * (graph_search.h) as a layer-by-layer min-plus pass: g(start) = 0, g = 1e6 elsewhere, a candidate is taken only
 * when strictly below; ties: smallest total, then smallest g(u), then smallest u.  Goal: the last layer's node 0, or
 * with FUELMI_REFINE_LAST_ARGMIN its first cheapest node below 100000 (:199-208).  An unreached goal is no error:
 * cost +inf, every choice -1.
 * Polyline (:486-497, when tour_lattice_res > 0 and tour_len is given): [start], then per chosen node the whole
 * path_costs path from the previous point at tour_lattice_res (shared joints appear twice, a no-path leg gives
 * {p1, p2}), or the node alone for a leg of length 0; an unreached problem: [start].
 * Limits, checked on the host before the map is touched: layers per problem <= FUELMI_REFINE_MAX_LAYERS, nodes per
 * layer <= FUELMI_REFINE_MAX_NODES, the edge count of the call < 2^31 (FUELMI_ELIMIT); a problem without layers or a
 * layer without nodes is FUELMI_EINVAL.  Same thread rule as the mutators.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_REFINE_LAST_ARGMIN 1 /* single-destination branch: keep the whole last layer, goal = its argmin */
#define FUELMI_REFINE_MAX_LAYERS 64
#define FUELMI_REFINE_MAX_NODES 256
typedef struct {
  fuelmi_path_cfg path;    /* edge searches: lattice_res 0.4, edge_step 0.1, no_path_cost 1000 (max_path_points unused) */
  double vm, yd, w_dir;    /* ViewNode::vm_, yd_, w_dir_ (exploration/vm, exploration/yd, exploration/w_dir) */
  double tour_lattice_res; /* 0.2 for the refined-tour polyline (:491); <= 0: no polyline */
  int max_tour_points;     /* per problem, for tour_xyz */
  int flags;               /* FUELMI_REFINE_* */
} fuelmi_refine_cfg;
/* start [n_prob][7] = pos xyz, vel xyz, yaw; problem b owns layers layer_ptr[b] .. layer_ptr[b+1]-1 (layer_ptr[0] =
 * 0), layer l owns nodes node_ptr[l] .. node_ptr[l+1]-1 (node_ptr[0] = 0) of nodes [N][4] = x y z yaw.  Out:
 * choice [n_layers] (index within its layer, -1 when unreached), cost [n_prob] (the goal's g, +inf when unreached);
 * tour_len [n_prob] (always the full count) and tour_xyz [n_prob][max_tour_points][3] may be NULL.  A polyline
 * longer than max_tour_points fills what fits and the call returns FUELMI_ELIMIT. */
int fuelmi_map_refine_tours(fuelmi_map* m, const fuelmi_refine_cfg* cfg, int n_prob, const double* start,
                            const int* layer_ptr, const int* node_ptr, const double* nodes, int* choice, double* cost,
                            int* tour_len, double* tour_xyz);

/* ------------------------------------------------------------------------------------------
 * Path to the next viewpoint: the geometric part of FastExplorationManager::planExploreMotion (exploration_manager/
 * src/fast_exploration_manager.cpp:234-276) with shortenPath (:295-325), for n_prob independent problems
 * (start, goal) in one call.  Per problem:
 *   1. raw path: Astar::search(start, goal) as the lattice search of fuelmi_map_path_costs' kind 1 at cfg.path
 *      (lattice_res 0.2, the manager's astar/resolution_astar) -- ALWAYS the lattice, no straight-line attempt:
 *      [start, nodes..., goal]; start = goal gives {start, goal}.  No goal node reachable: status
 *      FUELMI_GOAL_NO_PATH (the reference's `return FAIL`), n_way 0, raw_len 0, length 0, next_goal = goal.
 *   2. shortenPath, literally: short = [path[0]]; for i = 1 .. size-2: if |path[i] - short.back()| > shorten_dist push
 *      path[i], else walk RayCaster::input(short.back(), path[i+1]) / nextId and push path[i] at the first voxel that
 *      is inflated or UNKNOWN (no box test; voxels outside the map pass; the walk starts in short.back()'s voxel and
 *      stops before path[i+1]'s).  Then push path.back() iff |path.back() - short.back()| > end_eps; then, iff
 *      exactly two points are left, insert 0.5 * (short[0] + short[1]) between them.  ({p, p} comes out as {p}.)
 *   3. length = Astar::pathLength(short): segment norms sqrt(x x + y y + z z) summed left to right.
 *      length < radius_close: FUELMI_GOAL_CLOSE, way-points = short, next_goal = goal.
 *      length > radius_far:   FUELMI_GOAL_FAR: trunc = [short[0]], len2 = 0, for i = 1 while i < size and len2 <
 *                             radius_far: len2 += |short[i] - trunc.back()|, push short[i]; way-points = trunc,
 *                             next_goal = trunc.back().
 *      otherwise:             FUELMI_GOAL_MID (the reference's kinodynamicReplan branch): way-points = short,
 *                             next_goal = goal.
 * Every quantity is f64 + - * / sqrt in the order written: results do not depend on the batch.
 * Differences from the reference are those of the lattice search: the shortest lattice path in
 * place of A*'s, no wall-clock cap, no node pool.
 * Limits: all arguments are checked on the host before the map is touched (points finite with |coordinate| < 1e7;
 * lattice_res, edge_step, shorten_dist, radius_close, radius_far > 0 and finite, end_eps >= 0, max_path_points >= 2,
 * max_way_points >= 1: FUELMI_EINVAL).  A raw path of more than max_path_points points: raw_len holds the full count,
 * status -1, n_way 0; more way-points than max_way_points: n_way holds the full count, the first max_way_points are
 * written, status / length / next_goal are complete.  Either way every other problem is complete and the call
 * returns FUELMI_ELIMIT.  n_prob = 0 is FUELMI_OK.  Same thread rule as the mutators; fuelmi_map_path_stats
 * afterwards describes the lattice run.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_GOAL_CLOSE 0   /* length < radius_close: planExploreTraj on the way-points */
#define FUELMI_GOAL_MID 1     /* kinodynamicReplan to the goal */
#define FUELMI_GOAL_FAR 2     /* length > radius_far: planExploreTraj on the truncated way-points */
#define FUELMI_GOAL_NO_PATH 3 /* the search reached no goal node */
typedef struct {
  fuelmi_path_cfg path; /* lattice_res 0.2, edge_step 0.1; max_path_points = cap of a raw path (no_path_cost unused) */
  double shorten_dist;  /* 3.0 (:301) */
  double end_eps;       /* 1e-3 (:319) */
  double radius_close;  /* 1.5 (:243) */
  double radius_far;    /* 5.0 (:242) */
  int max_way_points;   /* per problem, for way_xyz */
} fuelmi_goal_cfg;
/* start_xyz, goal_xyz: n_prob points each (host).  Out, per problem: status (FUELMI_GOAL_*), length (of short,
 * before truncation), n_way and way_xyz [n_prob][max_way_points][3] (entries past n_way unspecified), next_goal
 * [n_prob][3]; raw_len [n_prob] and raw_xyz [n_prob][max_path_points][3], the raw path, may each be NULL. */
int fuelmi_map_goal_paths(fuelmi_map* m, const fuelmi_goal_cfg* cfg, int n_prob, const double* start_xyz,
                          const double* goal_xyz, int* status, double* length, int* n_way, double* way_xyz,
                          double* next_goal, int* raw_len, double* raw_xyz);
/* device milliseconds of the last fuelmi_map_goal_paths on this map, from events on the map's stream: [0] the lattice
 * run (with the host's looks at its work lists), [1] k_goal_shorten.  Zeros before the first call. */
int fuelmi_map_goal_path_times(const fuelmi_map* m, double ms2[2]);

/* ------------------------------------------------------------------------------------------
 * Global tour: the ATSP of FastExplorationManager::findGlobalTour (exploration_manager/src/
 * fast_exploration_manager.cpp:327-420), which the reference hands to LKH-2 as int(cost * 100) in a TSPLIB file,
 * for n_prob independent int32 matrices in one call.  Needs no map: the solver owns a stream and a workspace that
 * grows on demand (no allocation once warm).  Problem b has dimension d = dim_ptr[b+1] - dim_ptr[b] (dim_ptr[0] = 0)
 * and its matrix c at costs + sum of the earlier d^2 (row-major).  The answer order[0..d-1] has order[0] = 0 and
 * minimises the closed tour C = sum_k c[order[k]][order[k+1]] + c[order[d-1]][0], summed in int64 (with the
 * reference's column 0 of zeros: the cheapest open path from the current state, which is what LKH answers;
 * order[1..] - 1 are findGlobalTour's indices).  The method depends on d and the configuration only:
 *   exact (method 0), d - 1 <= exact_max: Held-Karp.  Suffix DP g(S, j) = the cheapest way to visit the rest of
 *     1..d-1 from j having visited S and close at 0; forward construction takes at every step the smallest j with
 *     c[last][j] + g(S u {j}, j) equal to the optimum: the LEXICOGRAPHICALLY SMALLEST optimal order.  d = 1: {0},
 *     cost 0; d = 2: {0, 1}, cost c01 + c10.  Table 2^(d-1) (d-1) int64 in the workspace (8 MiB at the cap).
 *   heuristic (method 1), larger d: a deterministic iterated local search, `restarts` independent restarts r
 *     (one workgroup each).  Restart r: the nearest-neighbour tour from 0 (ties: the smallest index); local search;
 *     then `kicks` times: double bridge of the best tour, local search, keep the result iff its cost is strictly
 *     below the restart's best (else back to the best).  Answer: the cheapest restart, the smallest r on ties.
 *   Local search = best improvement: every pass evaluates the whole neighbourhood of the current tour and applies
 *     the one move of the smallest key (delta, type, i, j, k) among those with delta < 0, until none is left.
 *     type 0, 2-opt: reverse order[i..j], 1 <= i < j <= d-1 (k = 0).  Its delta takes the reversed inner edges from
 *       prefix sums of the forward and backward edge costs along the tour.
 *     type 1, Or-opt: the segment order[i .. i+L-1] (L = 1, 2, 3; i >= 1, i+L-1 <= d-1) moves into the gap after
 *       position j (0 <= j <= d-1, the gap j = d-1 closes at 0; j outside [i-1, i+L-1]), forward (rev 0) or
 *       reversed (rev 1, L >= 2 only); k = 2 (L - 1) + rev.  Positions are those of the tour the pass starts from.
 *   Double bridge at 1 <= p1 < p2 < p3 <= d-1: A C B D with A = order[0..p1-1], B = [p1..p2-1], C = [p2..p3-1],
 *     D = [p3..d-1] (orientation kept).  Points: h = mix(seed ^ mix(r << 32 | k)) for kick k, then draws
 *     x_t = 1 + mix(h + t) % (d - 1) for t = 0, 1, ..., a value already drawn skipped, until three; sorted.
 *     mix = splitmix64's step (z += 0x9E3779B97F4A7C15, two xor-shift-multiplies, xor-shift), all mod 2^64.
 *     Seeds never depend on a problem's place in the batch: an answer is the same alone or batched, on any run.
 * Limits, checked on the host before anything is written or launched: d <= FUELMI_TSP_MAX_DIM and the call's
 * matrix entries < 2^31 (FUELMI_ELIMIT); d < 1, dim_ptr[0] != 0 are FUELMI_EINVAL.  fuelmi_tsp_create refuses
 * restarts < 1, kicks < 0 and exact_max outside [3, FUELMI_TSP_EXACT_CAP] with FUELMI_EINVAL (and *out untouched),
 * and returns FUELMI_ENODEV without a gfx950 device.  One thread per solver at a time.
 * Defaults (FUELMI_TSP_DEFAULT_*): measured on the headline G400 first-cycle matrix, DESIGN.md section 10.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_TSP_MAX_DIM 1024
#define FUELMI_TSP_EXACT_CAP 16
#define FUELMI_TSP_DEFAULT_RESTARTS 64
#define FUELMI_TSP_DEFAULT_KICKS 8
#define FUELMI_TSP_DEFAULT_EXACT_MAX 12
typedef struct {
  int restarts, kicks, exact_max;
  uint64_t seed;
} fuelmi_tsp_cfg;
typedef struct fuelmi_tsp fuelmi_tsp;
int fuelmi_tsp_create(int device, const fuelmi_tsp_cfg* cfg, fuelmi_tsp** out);
void fuelmi_tsp_destroy(fuelmi_tsp* t);
/* Out: order (concatenated, d each, at dim_ptr[b]), tour_cost[b] (int64), method[b] (0 exact, 1 heuristic);
 * synchronous. */
int fuelmi_tsp_solve(fuelmi_tsp* t, int n_prob, const int* dim_ptr, const int32_t* costs, int* order,
                     int64_t* tour_cost, int* method);

/* ------------------------------------------------------------------------------------------
 * B-spline cost + gradient: replaces BsplineOptimizer::combineCost and the calc*Cost terms
 * (bspline_opt/src/bspline_optimizer.cpp:255-516, 518-691), batched over C trajectories.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_COST_SMOOTHNESS (1 << 0)
#define FUELMI_COST_DISTANCE (1 << 1)
#define FUELMI_COST_FEASIBILITY (1 << 2)
#define FUELMI_COST_START (1 << 3)
#define FUELMI_COST_END (1 << 4)
#define FUELMI_COST_GUIDE (1 << 5)
#define FUELMI_COST_WAYPOINTS (1 << 6)
#define FUELMI_COST_VIEWCONS (1 << 7)
#define FUELMI_COST_MINTIME (1 << 8)

/* BsplineOptimizer::setParam (bspline_optimizer.cpp:25-53) */
typedef struct {
  double ld_smooth, ld_dist, ld_feasi, ld_start, ld_end, ld_guide, ld_waypt, ld_view, ld_time;
  double dist0, max_vel, max_acc, wnl, dlmin;
  int bspline_degree;
} fuelmi_bspline_cfg;

/* One batch of C independent combineCost evaluations, all with the same cost_function,
 * dimension and point count (host arrays, row-major, candidate-major):
 *   x          [C][nvar]   nvar = dim*N (+1 trailing knot span if MINTIME)     NLopt layout
 *   pt_dist    [C]         optimize()'s pt_dist_ from the INITIAL control points (:136-140)
 *   knot_span  [C]         used when MINTIME is clear
 *   time_lb    [C] or NULL (treated as -1)
 *   start_state[C][3][3]   pos, vel, acc (START)
 *   end_state  [C][3][3]   END; end_n = end_state_.size() in {1,2,3}
 *   guide_pts  [C][N-2*order][3]   (GUIDE)
 *   waypoints  [C][n_waypt][3], waypt_idx [C][n_waypt]   (WAYPOINTS)
 *   view_pt/view_dir [C][3], view_idx [C]                (VIEWCONS)
 * outputs: cost [C], grad [C][nvar]. */
typedef struct {
  int cost_function;
  int dim;
  int point_num;
  int n_traj;
  const double* x;
  const double* pt_dist;
  const double* knot_span;
  const double* time_lb;
  const double* start_state;
  const double* end_state;
  int end_n;
  const double* guide_pts;
  const double* waypoints;
  const int* waypt_idx;
  int n_waypt;
  const double* view_pt;
  const double* view_dir;
  const int* view_idx;
} fuelmi_bspline_batch;

int fuelmi_bspline_cost_grad(fuelmi_map* m, const fuelmi_bspline_cfg* cfg,
                             const fuelmi_bspline_batch* batch, double* cost, double* grad);

/* BsplineOptimizer::optimize() (bspline_optimizer.cpp:165-253) as ONE call for a batch given in host arrays -- what
 * the reference's callers do one trajectory at a time (plan_manage/src/planner_manager.cpp:296-314).  Like
 * fuelmi_bspline_cost_grad it runs on a query slot of the map (own side stream, inputs and results in the slot's pinned
 * block): no device allocation, re-entrant, concurrent callers do not queue behind each other or behind the map's
 * mutators.  Semantics of the solve: fuelmi_bspline_dev_optimize_timed.  x_out [C][nvar], cost_out [C], evals_out [C]
 * or NULL. */
int fuelmi_bspline_optimize(fuelmi_map* m, const fuelmi_bspline_cfg* cfg, const fuelmi_bspline_batch* batch,
                            int max_eval, double max_time_s, double* x_out, double* cost_out, int* evals_out);

/* Device-resident variant for benchmarking / optimiser loops: upload once, evaluate many times
 * without host copies.  Handles are owned by the map. */
typedef struct fuelmi_bspline_dev fuelmi_bspline_dev;
int fuelmi_bspline_dev_create(fuelmi_map* m, const fuelmi_bspline_cfg* cfg,
                              const fuelmi_bspline_batch* batch, fuelmi_bspline_dev** out);
int fuelmi_bspline_dev_eval(fuelmi_bspline_dev* b);             /* async on the map's stream */
int fuelmi_bspline_dev_download(fuelmi_bspline_dev* b, double* cost, double* grad);
/* the evaluation with its results delivered to one of two pinned host slots by the kernel itself (slot 0 / 1);
 * _collect waits for that launch only and copies cost [C] / grad [C][nvar] out */
int fuelmi_bspline_dev_eval_pinned(fuelmi_bspline_dev* b, int slot);
int fuelmi_bspline_dev_collect(fuelmi_bspline_dev* b, int slot, double* cost, double* grad);
/* BsplineOptimizer::optimize() (bspline_optimizer.cpp:165-253) for every candidate of the batch on the
 * device: start point and bounds as the reference sets them up (control points clamped into the
 * exploration box shrunk by 0.1, +-10 around the start, knot span in [0,5]), at most max_eval objective
 * evaluations (set_maxeval), xtol_rel 1e-5, the best variables seen are returned (best_variable_).  The
 * iteration itself is a box-projected L-BFGS instead of NLopt's (third party): final costs are
 * comparable, iterates are not.  x_out [C][nvar], cost_out [C], evals_out [C] or NULL; synchronous. */
int fuelmi_bspline_dev_optimize(fuelmi_bspline_dev* b, int max_eval, double* x_out, double* cost_out,
                                int* evals_out);
/* ... with the wall-clock cap of the reference's solver as well (opt.set_maxtime(max_iteration_time_[...]),
 * bspline_optimizer.cpp:170-172; 5 ms in exploration_manager/launch/algorithm.xml:190): a candidate's solve stops
 * at the first evaluation boundary past max_time_s seconds of device time and returns the best variables seen so far,
 * like costFunction keeps them (:693-707).  max_time_s <= 0: no cap. */
int fuelmi_bspline_dev_optimize_timed(fuelmi_bspline_dev* b, int max_eval, double max_time_s, double* x_out,
                                      double* cost_out, int* evals_out);
/* which solve kernel both optimise calls run for this batch (host only, no device needed): out3 = {npl, waves per
 * candidate, dynamic LDS bytes}.  npl 2 / 4: register state (nvar <= 128 / 256), 4 waves when n_traj <= 256, else 1;
 * npl 0: state in LDS (nvar > 256).  FUELMI_ELIMIT past the 160 KiB LDS budget, FUELMI_EINVAL for dim 2 (both
 * optimise calls refuse the batch the same way). */
int fuelmi_bspline_opt_plan(const fuelmi_bspline_batch* batch, int out3[3]);
void fuelmi_bspline_dev_destroy(fuelmi_bspline_dev* b);

/* Spline glue around the solve, batched (NonUniformBspline, bspline/src/non_uniform_bspline.cpp).
 *
 * fuelmi_bspline_parameterize = parameterizeToBspline (:178-265) for n_traj sample sets at once: the
 * least-squares control points of a uniform B-spline (degree 3..5, knot span ts) through n_points
 * samples whose start/end velocity and acceleration match `derivs` (the reference solves the
 * (K+4) x (K+degree-1) system with Eigen's ColPivHouseholderQR; results agree to ~1e-12).
 *   ts [C], points [C][K][3], derivs [C][4][3] (start vel, end vel, start acc, end acc)
 *   -> ctrl [C][K+degree-1][3].  ts <= 0 is rejected ("time step error", :181-184).
 * fuelmi_bspline_boundary_states = getBoundaryStates(ks, ke) (:107-122) of n_traj uniform B-splines
 * (setUniformBspline :15-32): position and the first ks / ke derivatives at t = 0 / t = duration.
 *   ctrl [C][n_ctrl][3] -> start [C][ks+1][3], end [C][ke+1][3].
 * Host arrays, synchronous. */
int fuelmi_bspline_parameterize(fuelmi_map* m, int n_traj, int n_points, int degree, const double* ts,
                                const double* points, const double* derivs, double* ctrl);
int fuelmi_bspline_boundary_states(fuelmi_map* m, int n_traj, int n_ctrl, int degree, const double* ts,
                                   const double* ctrl, int ks, int ke, double* start, double* end);
/* The planners' sequence "samples -> parameterizeToBspline -> getBoundaryStates(2, 0) ->
 * setBoundaryStates -> optimize" (plan_manage/src/planner_manager.cpp:161-184, 296-314) without leaving
 * the device: refills the batch `b` (dim 3, point_num = n_points + bspline_degree - 1) with the fitted
 * control points, knot span ts, pt_dist_, start state (pos, vel, acc) and end position; asynchronous on
 * the map's stream, the next _dev_eval / _dev_optimize uses them.  Rows 1..2 of end_state keep what
 * the batch was created with (the planners pass end_n = 1). */
/* Measurement driver: n full-box plan cycles issued back to back from C++ (no interpreter between the calls) --
 * per cycle fuelmi_frontier_reset, fuelmi_map_set_updated_box(ub_min, ub_max), fuelmi_frontier_search_begin,
 * fuelmi_map_inflate_local, fuelmi_map_update_esdf, fuelmi_bspline_dev_eval(batch) (batch may be NULL),
 * fuelmi_frontier_search_end; with `serial` != 0 the search runs after the map chain instead of beside it.
 * Both streams are drained before the clock starts and before it stops.  *n_clusters: clusters of the last
 * search; *seconds: elapsed wall time. */
/* The streaming counterpart: n cycles of fuelmi_map_input_depth(depth[k], pose k), fuelmi_frontier_search_begin,
 * (when the frame fused points) fuelmi_map_inflate_local + fuelmi_map_update_esdf, fuelmi_bspline_dev_eval,
 * fuelmi_frontier_search_end, fuelmi_frontier_commit.  depth[k]: any pointer fuelmi_map_input_depth takes;
 * cam_pos3 / cam_q4: n x 3 / n x 4 doubles; *box_voxels (may be NULL): sum of the local-bound volumes. */
int fuelmi_bench_stream(fuelmi_map* m, fuelmi_frontier* f, fuelmi_bspline_dev* batch, int n, const void* const* depth,
                        int rows, int cols, const fuelmi_depth_cfg* cfg, const double* cam_pos3, const double* cam_q4,
                        int serial, int* n_clusters, double* box_voxels, double* seconds);
int fuelmi_bench_cycles(fuelmi_map* m, fuelmi_frontier* f, fuelmi_bspline_dev* batch, const double ub_min[3],
                        const double ub_max[3], int n, int serial, int* n_clusters, double* seconds);
/* mean HOST microseconds per cycle the last fuelmi_bench_cycles run spent inside each C-ABI call: [0] _frontier_reset +
 * _set_updated_box, [1] _search_begin, [2] _inflate_local, [3] _update_esdf, [4] _bspline_dev_eval, [5] _search_end
 * (of which [6] polling for the device's result). */
int fuelmi_bench_host_profile(const fuelmi_map* m, double out7[7]);
/* fuelmi_bench_cycles with the results delivered to host memory every cycle, as the reference's callers receive
 * them (exploration_manager/src/fast_exploration_manager.cpp:99-114 reads the cell lists of searchFrontiers,
 * plan_manage/src/planner_manager.cpp:296-314 the optimiser's cost / gradient): cells of all new clusters into
 * cells_out (as many clusters as fit cells_cap), cost[C] and grad[C * nvar] of the batch.  seconds3: [0] elapsed,
 * [1] spent in the cell copies, [2] in the cost / gradient download. */
int fuelmi_bench_cycles_delivered(fuelmi_map* m, fuelmi_frontier* f, fuelmi_bspline_dev* batch, const double ub_min[3],
                                  const double ub_max[3], int n, int* cells_out, size_t cells_cap, double* cost,
                                  double* grad, int* n_clusters, double* seconds3);
int fuelmi_bspline_dev_load_samples(fuelmi_bspline_dev* b, int n_points, const double* ts, const double* points,
                                    const double* derivs);

/* ------------------------------------------------------------------------------------------
 * Min-jerk initial trajectory through way-points: the first half of FastPlannerManager::planExploreTraj
 * (plan_manage/src/planner_manager.cpp:266-297) for n_prob independent problems (way-points, start velocity, start
 * acceleration) in one call.  Per problem, with n_way points and S = n_way - 1 segments:
 *   1. times[k] = |p[k+1] - p[k]| / (max_vel * 0.5), the norm sqrt(x x + y y + z z) summed left to right; duration =
 *      the left-to-right sum of times (getTotalTime).
 *   2. PolynomialTraj::waypointsTraj (poly_traj/src/polynomial_traj.cpp:5-175) with end velocity = end acceleration
 *      = 0: the min-jerk quintic per segment and axis, coef[k][axis][i] the factor of t^i.  The 6S x 6S matrices are
 *      not formed: their blocks are known in closed form and the free derivatives solve a symmetric banded system
 *      (DESIGN.md section 10); coefficients agree with the dense inverses to those inverses' own rounding.
 *   3. length = getLength, literally: samples at the ACCUMULATED eval_t (eval_t = 0; while (eval_t < duration)
 *      { ...; eval_t += 0.01; }), norms of consecutive samples (summed by a fixed tree, not left to right).
 *      evaluate(t, k) looks its segment up as `while (times[idx] + 1e-4 < ts) ts -= times[idx++]`, idx clamped to the
 *      last segment (the reference reads past the end there).
 *   4. seg_num = max(min_seg, int(min(length / ctrl_pt_dist, FUELMI_WPTRAJ_MAX_SEG))) (the reference's int() is
 *      undefined past 2^31), or cfg.seg_num when that is > 0; dt = duration / seg_num.
 *   5. samples at the accumulated ts (for (ts = 0; ts <= duration + 1e-4; ts += dt)): n_samples of them, seg_num + 1
 *      whenever dt > 1e-4 (the loop stops at FUELMI_WPTRAJ_MAX_SEG + 2 samples at the latest); derivs = velocity at
 *      0 and at duration, then acceleration at 0 and at duration: fuelmi_bspline_parameterize's `derivs`.
 * Everything is f64 + - * / sqrt in a fixed order: a result does not depend on the problem's place in the batch.
 * Per-problem status:
 *   FUELMI_WPTRAJ_OK.
 *   FUELMI_WPTRAJ_FEW         n_way < 3 (for two points the reference writes outside its selection matrix; the
 *                             manager never passes two, shortenPath inserts a mid-point).
 *   FUELMI_WPTRAJ_DEGENERATE  a segment time that is 0 or not finite (a singular mapping matrix in the reference).
 *   -1                        more samples than max_samples.
 * FEW and DEGENERATE: n_samples 0 and every other output of the problem written as 0; the call is still FUELMI_OK.
 * -1: n_samples holds the full count, the first max_samples samples are written, everything else is complete, the
 * other problems are complete, and the call returns FUELMI_ELIMIT.
 * Checked on the host before anything is launched (FUELMI_EINVAL): way-points (the first n_way of a problem), vel_xyz
 * and acc_xyz finite with |coordinate| < 1e7; max_vel and ctrl_pt_dist finite and > 0; 1 <= min_seg and 0 <= seg_num
 * <= FUELMI_WPTRAJ_MAX_SEG; max_samples >= 1; 0 <= n_way[i] <= max_way_points.  FUELMI_ELIMIT, also before any launch:
 * max_way_points > FUELMI_WPTRAJ_MAX_WAY, or a problem whose duration exceeds FUELMI_WPTRAJ_MAX_DURATION seconds
 * (10^6 length samples).  n_prob = 0 is FUELMI_OK.
 * fuelmi_map_waypoint_trajs runs on a query slot of the map like fuelmi_bspline_parameterize: host arrays in, host
 * arrays out, synchronous, re-entrant.  way_xyz [n_prob][max_way_points][3] is fuelmi_map_goal_paths' way_xyz.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_WPTRAJ_OK 0
#define FUELMI_WPTRAJ_FEW 1
#define FUELMI_WPTRAJ_DEGENERATE 2
#define FUELMI_WPTRAJ_MAX_WAY 256         /* largest max_way_points */
#define FUELMI_WPTRAJ_MAX_SEG (1 << 20)   /* largest seg_num */
#define FUELMI_WPTRAJ_MAX_DURATION 1.0e4  /* seconds */
typedef struct {
  double max_vel;       /* pp_.max_vel_ */
  double ctrl_pt_dist;  /* pp_.ctrl_pt_dist */
  int min_seg;          /* 8 */
  int seg_num;          /* 0: the reference's rule; > 0: forced (every problem gets seg_num + 1 samples) */
  int max_way_points;   /* stride of way_xyz; same layout as fuelmi_map_goal_paths' output */
  int max_samples;      /* stride / cap of samples */
} fuelmi_wptraj_cfg;
/* Out, per problem: status, duration, length, seg_num, dt, n_samples, samples [n_prob][max_samples][3] (entries past
 * n_samples unspecified), derivs [n_prob][4][3]; seg_times [n_prob][max_way_points-1] and coef
 * [n_prob][max_way_points-1][3][6] may each be NULL (entries past n_way - 1 unspecified). */
int fuelmi_map_waypoint_trajs(fuelmi_map* m, const fuelmi_wptraj_cfg* cfg, int n_prob, const int* n_way,
                              const double* way_xyz, const double* vel_xyz, const double* acc_xyz, int* status,
                              double* duration, double* length, int* seg_num, double* dt, int* n_samples,
                              double* samples, double* derivs, double* seg_times, double* coef);
/* The device chain way-points -> fitted batch: refills the batch `b` exactly as fuelmi_bspline_dev_load_samples would
 * from the same problems' samples (ts = dt), but the samples never exist on the host: the kernel above writes
 * ts | points | derivs into the batch's staging and the spline fit follows on the map's stream.  One problem per
 * candidate (C = the batch's n_traj; n_way [C], way_xyz [C][max_way_points][3], vel_xyz, acc_xyz [C][3]).  seg_num is
 * forced to point_num - bspline_degree so that every candidate fits the batch: cfg->seg_num must be 0 or equal to
 * that; cfg->max_samples is ignored (it is seg_num + 1).  A candidate whose status is not FUELMI_WPTRAJ_OK keeps the
 * state it had in the batch.  status [C]; duration [C] or NULL.  Same host checks and return values as above.
 * Everything is queued on the map's stream without waiting, then status (and duration) are copied back and the call
 * waits for the map's stream once, behind the fit: when it returns the batch is loaded, and the next _dev_eval /
 * _dev_optimize uses it. */
int fuelmi_bspline_dev_load_waypoints(fuelmi_bspline_dev* b, const fuelmi_wptraj_cfg* cfg, const int* n_way,
                                      const double* way_xyz, const double* vel_xyz, const double* acc_xyz, int* status,
                                      double* duration);
/* what the kernel needs for cfg->max_way_points (host only, no device needed): out3 = {lanes per problem, dynamic LDS
 * bytes, largest max_way_points accepted}.  FUELMI_ELIMIT past FUELMI_WPTRAJ_MAX_WAY, like both calls above. */
int fuelmi_wptraj_plan(const fuelmi_wptraj_cfg* cfg, int out3[3]);

/* ------------------------------------------------------------------------------------------
 * Yaw trajectory of a position spline: FastPlannerManager::planYawExplore (plan_manage/src/planner_manager.cpp:774-865,
 * mode FUELMI_YAW_EXPLORE) and ::planYaw (:695-772, FUELMI_YAW_FOLLOW) for n_prob independent problems in one call.
 * The position spline is UNIFORM (control points + one knot span, setUniformBspline): the exploration path sets no
 * other.  Moving knots (lengthenTime, reallocateTime) is fuelmi_map_adjust_trajs, below; the moved knots go into
 * fuelmi_map_plan_yaws_knots (and, for a device batch, FUELMI_KNOTS_ADJUSTED; both below).  The yaw spline that comes
 * out is uniform either way: the reference builds every yaw spline with setUniformBspline, and given knots for yaw
 * splines are out of scope.
 * Per problem, EXPLORE, everything f64 in this order:
 *   1. knots as setUniformBspline builds them (non_uniform_bspline.cpp:25-31): u[i] = double(i - p) * dt for i <= p,
 *      then ACCUMULATED u[i] = u[i-1] + dt; duration = u[n_ctrl] - u[p] (a result of the additions, not a product).
 *   2. dt_yaw = duration / seg_num; start_yaw[0] wrapped into [-pi, pi] by the reference's two loops; last_yaw = it.
 *   3. initial control points q[0..2] = states2pts * start (rows (1, -dt, (1/3.0) dt dt), (1, 0, -(1/6.0) dt dt),
 *      (1, dt, (1/3.0) dt dt), products summed left to right), the rest 0.
 *   4. with lookfwd: relax_num = int(min(relax_time / dt_yaw, seg_num)); for i = 1 .. seg_num - relax_num - 1:
 *      tc = i dt_yaw, tf = min(duration, tc + forward_t), pd = evaluateDeBoorT(tf) - evaluateDeBoorT(tc) (the literal
 *      clamp, knot search and alpha recursion of :51-71); if sqrt(x x + y y + z z) > 1e-6: w = atan2(pd.y, pd.x)
 *      unwrapped by calcNextYaw(last_yaw, w) (:867-885), else w = the previous way-point.  THE FIRST WAY-POINT HAS NO
 *      PREDECESSOR (the reference reads waypts.back() of an empty vector there): it is defined as last_yaw, the
 *      wrapped start yaw.  last_yaw = w; the way-point's control-point index is i.
 *   5. e = end_yaw unwrapped against last_yaw; q[seg_num .. seg_num+2] = states2pts * (e, 0, 0); end_yaw_out = e.
 *   6. pt_dist = (sum |q[i+1] - q[i]|) / (seg_num + 3) (optimize(), bspline_optimizer.cpp:136-140).
 *   7. yaw_ctrl = THE MINIMISER of the reference's objective SMOOTHNESS | START | END | WAYPOINTS (order 3, dimension
 *      1, start state (s0, s1, s2), end state (e, 0)) (:255-282, 355-457, 571-630): a convex quadratic, solved exactly
 *      by a banded Cholesky factorisation (half-bandwidth 3).  The reference's NLopt run iterates towards this point
 *      for at most 2000 evaluations; its iterate is not reproduced, its cost is never below this one's except by
 *      rounding.  cost = the objective at yaw_ctrl.
 *   8. yawdot_ctrl / yawddot_ctrl = getDerivativeControlPoints (:77-86) once and twice on setUniformBspline(yaw, 3,
 *      dt_yaw)'s accumulated knots.
 * FOLLOW differs: seg_num = ceil(duration / dt_target); start_yaw[0] is not wrapped; way-points at i = 0 .. seg_num-1,
 * no relax; end = atan2(v.y, v.x) with v the DERIVATIVE spline (getDerivative) evaluated by its own evaluateDeBoorT at
 * duration - end_back, unwrapped against the last way-point; three end entries (e, 0, 0); the yaw spline (and so the
 * derivative control points) has degree pos_degree, as planYaw sets it.
 * Per-problem status:
 *   FUELMI_YAW_OK.
 *   FUELMI_YAW_DEGENERATE  pt_dist is 0 or not finite (the reference divides by it), or a Cholesky pivot is <= 0 or
 *                          not finite, or the cost is not finite: yaw_ctrl = the initial control points, cost = 0; the
 *                          way-points, end_yaw_out and the derivative control points (of the initial ones) are written.
 *                          Also (device batches only, the host route refuses it): a knot span that is not finite and > 0
 *                          -- then every output of the problem is 0.
 *   -1                     FOLLOW: seg_num exceeds cfg.max_seg; seg_num, duration and dt_yaw are reported, the arrays
 *                          are 0, the other problems are complete, and the call returns FUELMI_ELIMIT.
 * Entries of yaw_ctrl past seg_num + 3, of waypts past n_waypt (and of the derivative arrays) are written as 0.
 * Checked on the host before anything is launched (FUELMI_EINVAL): pointers; mode; pos_degree in 3..5; pos_degree + 1
 * <= n_ctrl[i] <= max_ctrl; knot spans finite and > 0; control points finite with |coordinate| < 1e7; yaw inputs finite
 * with |value| <= 1e3; the four weights finite, ld_start > 0 and ld_smooth > 0; forward_t, relax_time, dt_target,
 * end_back finite and >= 0 (dt_target > 0 in FOLLOW); 1 <= max_seg <= FUELMI_YAW_MAX_SEG; 1 <= seg_num <= max_seg in
 * EXPLORE.  max_ctrl > FUELMI_YAW_MAX_CTRL: FUELMI_ELIMIT.  n_prob = 0 is FUELMI_OK.
 * fuelmi_map_plan_yaws runs on a query slot of the map like fuelmi_map_waypoint_trajs: host arrays in and out,
 * synchronous, re-entrant, no device allocation once warm; a result does not depend on the problem's place in the batch.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_YAW_EXPLORE 0      /* FastPlannerManager::planYawExplore, planner_manager.cpp:774-865 */
#define FUELMI_YAW_FOLLOW  1      /* FastPlannerManager::planYaw,        planner_manager.cpp:695-772 */
#define FUELMI_YAW_OK 0
#define FUELMI_YAW_DEGENERATE 1
#define FUELMI_YAW_MAX_SEG  256   /* largest number of yaw segments */
#define FUELMI_YAW_MAX_CTRL 1024  /* largest max_ctrl (position control points per problem) */
typedef struct {
  int mode;            /* FUELMI_YAW_EXPLORE / _FOLLOW */
  int pos_degree;      /* degree of the position spline, 3..5 (pp_.bspline_degree_) */
  int max_ctrl;        /* stride of pos_ctrl */
  int max_seg;         /* stride of the outputs: yaw_ctrl [max_seg + 3], waypts [max_seg] */
  int seg_num;         /* EXPLORE: 12 */
  int lookfwd;         /* EXPLORE: way-points on / off */
  double relax_time;   /* EXPLORE: exploration/relax_time */
  double forward_t;    /* 2.0 */
  double dt_target;    /* FOLLOW: 0.3 */
  double end_back;     /* FOLLOW: 0.1 */
} fuelmi_yaw_cfg;
/* w: only ld_smooth, ld_start, ld_end, ld_waypt are read.  pos_ctrl [n_prob][max_ctrl][3], knot_span [n_prob],
 * start_yaw [n_prob][3] (yaw, rate, acceleration), end_yaw [n_prob] (EXPLORE only, may be NULL in FOLLOW).  Out, per
 * problem: status, duration, seg_num, dt_yaw, yaw_ctrl [n_prob][max_seg+3], n_waypt, waypts [n_prob][max_seg],
 * end_yaw_out, cost; yawdot_ctrl [n_prob][max_seg+2] and yawddot_ctrl [n_prob][max_seg+1] may each be NULL. */
int fuelmi_map_plan_yaws(fuelmi_map* m, const fuelmi_bspline_cfg* w, const fuelmi_yaw_cfg* cfg, int n_prob,
                         const int* n_ctrl, const double* pos_ctrl, const double* knot_span, const double* start_yaw,
                         const double* end_yaw, int* status, double* duration, int* seg_num, double* dt_yaw,
                         double* yaw_ctrl, int* n_waypt, double* waypts, double* end_yaw_out, double* cost,
                         double* yawdot_ctrl, double* yawddot_ctrl);
/* The same on whole knot vectors (setKnot) in place of the spans: knots [n_prob][max_ctrl + pos_degree + 1], the layout
 * of fuelmi_map_adjust_trajs' knots_out, so that call's output is this call's input as it stands.  Step 1 then takes
 * problem i's n_ctrl[i] + pos_degree + 1 knots as given; duration stays u[n_ctrl] - u[p], every evaluation stays
 * evaluateDeBoorT (t + u[p] and the clamp), FOLLOW's derivative points are divided by the given knots' differences.
 * Checked on the host before anything is launched (FUELMI_EINVAL), beside everything above but the spans: knots not
 * NULL, every knot finite, every knot above the one in front of it.  Strict increase is more than the reference asks
 * for: it asks for nothing and divides by knot differences. */
int fuelmi_map_plan_yaws_knots(fuelmi_map* m, const fuelmi_bspline_cfg* w, const fuelmi_yaw_cfg* cfg, int n_prob,
                               const int* n_ctrl, const double* pos_ctrl, const double* knots, const double* start_yaw,
                               const double* end_yaw, int* status, double* duration, int* seg_num, double* dt_yaw,
                               double* yaw_ctrl, int* n_waypt, double* waypts, double* end_yaw_out, double* cost,
                               double* yawdot_ctrl, double* yawddot_ctrl);
/* The device chain optimised batch -> yaw trajectories: one problem per candidate of `b` (dim 3), read from the
 * variables the batch's last fuelmi_bspline_dev_optimize[_timed] left in device memory: the control points are those
 * variables, the knot span is x[nvar-1] under MINTIME and the batch's knot span otherwise; the weights are the batch's;
 * cfg->pos_degree must be the batch's bspline_degree and cfg->max_ctrl is ignored (it is point_num).  Only the yaw
 * results are copied back; they equal, bit for bit, fuelmi_map_plan_yaws on the x_out that solve returned.
 * FUELMI_EINVAL when the batch is not dim 3 or has not been optimised since it was created or last (re)loaded by
 * fuelmi_bspline_dev_load_samples / _load_waypoints.  Runs on the map's stream and waits for it.
 * While the batch's knot source is FUELMI_KNOTS_ADJUSTED (fuelmi_bspline_dev_set_knot_source, below) the position
 * splines stand on the knots the batch's last fuelmi_bspline_dev_adjust_trajs left on the device, and the results equal,
 * bit for bit, fuelmi_map_plan_yaws_knots on that solve's x_out and that adjustment's knots_out.  The host never sees
 * those knots, so the kernel checks them (finite, strictly increasing): a candidate that fails -- one the adjustment
 * marked FUELMI_TRAJADJ_BADSPLINE, whose knots are 0 -- is FUELMI_YAW_DEGENERATE with every output 0. */
int fuelmi_bspline_dev_plan_yaws(fuelmi_bspline_dev* b, const fuelmi_yaw_cfg* cfg, const double* start_yaw,
                                 const double* end_yaw, int* status, double* duration, int* seg_num, double* dt_yaw,
                                 double* yaw_ctrl, int* n_waypt, double* waypts, double* end_yaw_out, double* cost,
                                 double* yawdot_ctrl, double* yawddot_ctrl);
/* what the kernel needs for cfg->max_ctrl and cfg->max_seg (host only, no device needed): out3 = {lanes per problem,
 * dynamic LDS bytes, largest max_ctrl accepted}.  cfg is checked like above. */
int fuelmi_yaw_plan(const fuelmi_yaw_cfg* cfg, int out3[3]);

/* ------------------------------------------------------------------------------------------
 * Exact solve of the optimiser's quadratic phases: BsplineOptimizer::optimize() (bspline_opt/src/bspline_optimizer.cpp:
 * 110-253) for a cost mask within SMOOTHNESS | START | END | GUIDE | WAYPOINTS, for n_prob independent problems in one
 * call, EACH WITH ITS OWN NUMBER OF CONTROL POINTS.  These are the reference's isQuadratic() masks (:738-747: GUIDE_PHASE,
 * SMOOTHNESS, SMOOTHNESS | WAYPOINTS) and the yaw objective SMOOTHNESS | WAYPOINTS | START | END.
 * Per problem, with N control points of dimension dim, the knot span dt fixed and everything f64 in this order:
 *   1. pt_dist = (sum |q[i+1] - q[i]|) / N from the input as given, not clamped (:136-140).
 *   2. with pt_dist frozen, every term of combineCost (:571-630) is c (a . q - b)^2 over at most four neighbouring
 *      control points, the same a for every axis:
 *        jerk rows (-1, 3, -3, 1) / pt_dist, i = 0 .. N-4, weight ld_smooth                               (:263-266)
 *        start rows: position (1, 4, 1)/6 with the literal weight 10, velocity (-1, 0, 1)/(2 dt), acceleration
 *        (1, -2, 1)/dt^2, weight ld_start                                                                  (:369-389)
 *        end rows: the first end_n of the same three on the last three control points, weight ld_end      (:407-430)
 *        guide rows: a unit row per guide point, i = order .. N-order-1, order = bspline_degree for dim 3 and 3 for
 *        dim 1 (:124-127), weight ld_guide; none when N <= 2 order                                        (:468-474)
 *        way-point rows (1, 4, 1)/6 at waypt_idx, weight ld_waypt; a repeated index is legal and adds up  (:442-456)
 *      ctrl_out = THE MINIMISER: H q = g with H = sum c a a^T symmetric of half-bandwidth 3, shared by the axes,
 *      factored once by a banded Cholesky, one substitution per axis.  cost = combineCost at ctrl_out, summed in the
 *      reference's order.
 *   3. bounds (dim 3 with cfg.bounds != 0): q0 = the input clamped into the map's box shrunk by 0.1 (:174-202), lb / ub =
 *      q0 -+ 10 cut to that box (:206-214).  The unconstrained minimiser is the reference's constrained one only if
 *      lb <= q <= ub holds in every coordinate; otherwise the status is FUELMI_QUAD_BOUNDED.  dim 1 has no bounds (:206).
 * THE REFERENCE'S ITERATE IS NOT REPRODUCED.  The reference runs GUIDE_PHASE with NLopt LD_TNEWTON, max_iteration_num1 = 2
 * and 0.1 ms (exploration_manager/launch/algorithm.xml:182-189): it keeps the better of two evaluations.  This call
 * returns the point that phase is defined to reach; its cost is never above the iteration's, except by rounding.
 * Per-problem status:
 *   FUELMI_QUAD_OK.
 *   FUELMI_QUAD_BOUNDED     ctrl_out = q0, cost = the objective at q0: the caller falls back to the iterative route
 *                           (fuelmi_bspline_optimize).
 *   FUELMI_QUAD_DEGENERATE  pt_dist is 0 or not finite while SMOOTHNESS is set, or a Cholesky pivot is <= 0 or not finite
 *                           (SMOOTHNESS alone, whose null space is the quadratics), or the cost is not finite: ctrl_out =
 *                           the input, cost = 0.  Also (device batches only, the host route refuses them): a knot span
 *                           that is not finite and > 0 -- then ctrl_out and pt_dist are 0 -- or a way-point index outside
 *                           [0, N-3].
 * Entries of ctrl_out past N are written as 0.  pt_dist is reported for every status.
 * Checked on the host before anything is launched (FUELMI_EINVAL): pointers the mask reads; a mask that is empty or has a
 * bit outside the five; dim 1 or 3; bspline_degree in 3..5 for dim 3; max(4, order + 1) <= n_ctrl[i] <= max_ctrl; end_n in
 * 1..3; 0 <= n_waypt[i] <= max_waypt, 0 <= waypt_idx <= N - 3; every input the mask reads finite with |value| < 1e7; knot
 * spans finite and > 0; the weights the mask reads finite and >= 0.  max_ctrl > FUELMI_QUAD_MAX_CTRL: FUELMI_ELIMIT (one
 * problem's LDS is 14 max_ctrl + 16 doubles at dim 3; the 160 KiB budget holds 1462 control points, the cap is the power
 * of two below, as for the yaw entry).  n_prob = 0 is FUELMI_OK.
 * fuelmi_map_solve_quadratic runs on a query slot of the map like fuelmi_map_plan_yaws: host arrays in and out,
 * synchronous, re-entrant, no device allocation once warm; a result does not depend on the problem's place in the batch.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_QUAD_OK 0
#define FUELMI_QUAD_BOUNDED 1
#define FUELMI_QUAD_DEGENERATE 2
#define FUELMI_QUAD_MAX_CTRL 1024  /* largest max_ctrl (control points per problem) */
typedef struct {
  int cost_function;   /* FUELMI_COST_* within SMOOTHNESS | START | END | GUIDE | WAYPOINTS */
  int dim;             /* 1 or 3 */
  int max_ctrl;        /* stride of ctrl / ctrl_out; guide_pts holds max(max_ctrl - 2 order, 0) rows per problem */
  int end_n;           /* end_state_.size(): 1..3 */
  int max_waypt;       /* stride of waypoints / waypt_idx */
  int bounds;          /* dim 3: != 0 checks the minimiser against optimize()'s bounds */
} fuelmi_quad_cfg;
/* w: ld_smooth, ld_start, ld_end, ld_guide, ld_waypt and bspline_degree are read.  ctrl [n_prob][max_ctrl][dim],
 * knot_span [n_prob], start_state / end_state [n_prob][3][dim] (position, velocity, acceleration), guide_pts
 * [n_prob][max(max_ctrl - 2 order, 0)][dim] (problem i reads its first n_ctrl[i] - 2 order rows), n_waypt [n_prob],
 * waypoints [n_prob][max_waypt][dim], waypt_idx [n_prob][max_waypt]; an array the mask does not read may be NULL.
 * Out, per problem: status, ctrl_out [n_prob][max_ctrl][dim], cost, pt_dist. */
int fuelmi_map_solve_quadratic(fuelmi_map* m, const fuelmi_bspline_cfg* w, const fuelmi_quad_cfg* cfg, int n_prob,
                               const int* n_ctrl, const double* ctrl, const double* knot_span, const double* start_state,
                               const double* end_state, const double* guide_pts, const int* n_waypt,
                               const double* waypoints, const int* waypt_idx, int* status, double* ctrl_out, double* cost,
                               double* pt_dist);
/* The same kernel on what a device batch holds (fuelmi_bspline_dev_create): one problem per candidate, its variables,
 * knot span, states, way-points and weights the batch's; only cfg->cost_function and cfg->bounds are read (dim, the point
 * count, end_n and the way-point count are the batch's).  guide_pts [C][point_num - 2 order][3]: the guide points of this
 * phase, or NULL for the batch's own (a NORMAL_PHASE batch holds none).  The batch must not optimise the knot span
 * (MINTIME): FUELMI_EINVAL.  The solution of every FUELMI_QUAD_OK candidate becomes the candidate's variables and its
 * pt_dist_ the candidate's, as optimize() sets both up for its next phase (:116, :136-140): the next
 * fuelmi_bspline_dev_optimize starts from it, and equals fuelmi_bspline_optimize on ctrl_out with that pt_dist_.  A
 * candidate of another status keeps its state.  The call clears the flag fuelmi_bspline_dev_plan_yaws / _check_trajs
 * test (the last solve's variables are no longer the batch's).  ctrl_out [C][point_num][dim].  Runs on the map's stream
 * and waits for it. */
int fuelmi_bspline_dev_solve_quadratic(fuelmi_bspline_dev* b, const fuelmi_quad_cfg* cfg, const double* guide_pts,
                                       int* status, double* ctrl_out, double* cost, double* pt_dist);
/* what the kernel needs for cfg->max_ctrl and cfg->dim (host only, no device needed): out3 = {lanes per problem, dynamic
 * LDS bytes, largest max_ctrl accepted}.  The mask, dim, end_n, max_waypt and max_ctrl are checked like above. */
int fuelmi_quad_plan(const fuelmi_quad_cfg* cfg, int out3[3]);

/* ------------------------------------------------------------------------------------------
 * Kinodynamic search for the mid-range goal branch: KinodynamicAstar::search + getSamples
 * (path_searching/src/kinodynamic_astar.cpp:15-263, 543-634) as FastPlannerManager::kinodynamicReplan calls them
 * (plan_manage/src/planner_manager.cpp:124-164) for n_prob independent problems (start position / velocity /
 * acceleration, goal position / velocity) in one call: static mode, first with init = true, then -- after NO_PATH --
 * reset() and one retry with init = false, inside the same launch.  One workgroup per problem.  Per problem:
 *   0. |start - goal| < 1e-2 (the norm sqrt(x x + y y + z z)): FUELMI_KINO_CLOSE_GOAL, nothing is searched.
 *   1. The open set is libstdc++'s binary heap of node pointers with the comparator f1 > f2 (push_heap's sift-up,
 *      pop_heap's hole-to-leaf walk followed by a sift-up), run on keys that may have gone stale: a node that is
 *      re-parented while it is open has its f and g changed IN PLACE and the heap is NOT repaired, exactly as the
 *      reference's std::priority_queue of pointers behaves.
 *   2. Per pop: the terminal tests on the heap's top (reach_horizon: |pos - start| >= horizon; near_end: every index
 *      difference to the goal's voxel <= tolerance = ceil(1 / resolution); on near_end estimateHeuristic and
 *      computeShotTraj with its accumulated `time += t_d / 10` checks), then the expansion.  The first expansion of the
 *      first search uses the `init` primitives (input = start acceleration, tau = k time_res_init init_max_tau summed
 *      up to init_max_tau + 1e-3), every other one the regular list (ax, ay, az each summed from -max_acc in steps of
 *      max_acc res up to max_acc + 1e-3, crossed with tau summed in steps of time_res max_tau up to max_tau).  Both
 *      lists are built on the host with the reference's accumulating loops.
 *   3. One lane per primitive: stateTransit, isInBox (strict on both sides), the search's own posToIndex (map origin,
 *      cfg.resolution), the closed test, the velocity limit, the same-voxel test, check_num safety samples (inflated,
 *      outside the box, unknown unless optimistic), g, estimateHeuristic (quartic / cubic literally, tie_breaker 1 +
 *      1e-4, the value (1 + tie_breaker) cost), f.  One lane then replays the survivors in the reference's loop order:
 *      a sibling landing in a voxel a sibling of this expansion created is compared by f (strict <), an older open node
 *      by g (strict <), a new voxel takes the next pool node and is pushed; use_node_num reaching allocate_num ends the
 *      search with NO_PATH in the middle of the expansion.
 *   4. retrievePath, then getSamples literally: T_sum summed from the shot and from the last node back to the first,
 *      seg_num = max(min_seg, floor(T_sum / ts)) (or cfg.seg_num when > 0), ts = T_sum / seg_num, the accumulated ti
 *      and t with their -1e-5 carries, the points in reversed order.  derivs = start velocity, end velocity, start
 *      acceleration, end acceleration (fuelmi_bspline_parameterize's order).  IN THE NO-SHOT BRANCH THE REFERENCE TAKES
 *      end_vel FROM THE START NODE (its `node` has walked back to the path's first node by then): reproduced.
 *      The shot's box test compares against the map SIZE (getRegion's second result), not the upper corner: reproduced.
 *      getKinoTraj is visualisation only and not part of this.
 * f64 throughout; + - * / sqrt in the reference's order with FMA contraction off, so g, the path's inputs, durations
 * and (without a shot) T_sum are bit-equal to the reference.  cbrt, acos, cos and pow(t, 3) come from the device's
 * libm, not glibc: h and f may differ from the reference's in the last bits.
 * A result does not depend on the problem's place in the batch.
 * Per-problem status: the reference's enum, FUELMI_KINO_CLOSE_GOAL, or -1 (over max_path_nodes / max_samples).
 * NO_PATH (both searches failed) and CLOSE_GOAL: n_nodes = n_samples = 0 and every other output of the problem 0,
 * except which / iter_num / use_node_num of the retry; the call is still FUELMI_OK.
 * -1: n_nodes / n_samples hold the full counts, the first max_path_nodes / max_samples entries are written, everything
 * else is complete, the other problems are complete, and the call returns FUELMI_ELIMIT.
 * Checked on the host before the map is touched (FUELMI_EINVAL): every input finite with |coordinate| < 1e7; every
 * double parameter finite and > 0; 2e7 / resolution < 2^31 (a voxel index of any admitted coordinate fits an int);
 * check_num >= 1; allocate_num >= 2; min_seg >= 1; seg_num >= 0; max_path_nodes >= 1;
 * max_samples >= 1.  FUELMI_ELIMIT, also before any launch: more than FUELMI_KINO_MAX_PRIMS primitives in the init list
 * or in the regular list; allocate_num > FUELMI_KINO_MAX_ALLOC; n_prob x workspace bytes > FUELMI_KINO_MAX_WORKSPACE.
 * n_prob = 0 is FUELMI_OK.
 * Workspace (one grow-only allocation on the map): per problem a node pool of allocate_num 128-byte records, the heap
 * array, and an open-addressing hash on the voxel triple with at least 2 allocate_num slots, cleared on the stream at
 * every call.  fuelmi_map_kino_paths runs on the map's stream: host arrays in, host arrays out, synchronous.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_KINO_REACH_HORIZON 1
#define FUELMI_KINO_REACH_END 2
#define FUELMI_KINO_NO_PATH 3
#define FUELMI_KINO_NEAR_END 4
#define FUELMI_KINO_CLOSE_GOAL 5
#define FUELMI_KINO_MAX_PRIMS 256                 /* primitives of one expansion */
#define FUELMI_KINO_MAX_ALLOC (1 << 22)           /* largest allocate_num */
#define FUELMI_KINO_MAX_SEG (1 << 20)             /* largest seg_num */
#define FUELMI_KINO_MAX_WORKSPACE 8589934592.0    /* bytes, n_prob x workspace of one problem */
typedef struct {
  double max_tau;         /* search/max_tau 0.8 */
  double init_max_tau;    /* search/init_max_tau 1.0 */
  double max_vel;         /* search/max_vel + search/vel_margin */
  double max_acc;         /* search/max_acc */
  double w_time;          /* search/w_time 10 */
  double horizon;         /* search/horizon 5 */
  double resolution;      /* search/resolution_astar */
  double lambda_heu;      /* search/lambda_heu 10 */
  double res;             /* 1 / 2.0: input step as a fraction of max_acc */
  double time_res;        /* 1 / 1.0 */
  double time_res_init;   /* 1 / 20.0 */
  double ts;              /* pp_.ctrl_pt_dist / pp_.max_vel_ */
  int allocate_num;       /* search/allocate_num 100000 */
  int check_num;          /* search/check_num 10 */
  int optimistic;         /* search/optimistic */
  int min_seg;            /* 8 */
  int seg_num;            /* 0: the reference's rule; > 0: forced */
  int max_path_nodes;     /* stride / cap of the node arrays */
  int max_samples;        /* stride / cap of samples */
} fuelmi_kino_cfg;
/* start_xyz, start_vel, start_acc, goal_xyz, goal_vel [n_prob][3].  Out, per problem: status; which (0: the first
 * search answered, 1: the retry); iter_num, use_node_num of the answering search; n_nodes; node_state
 * [n_prob][max_path_nodes][6], node_input [n_prob][max_path_nodes][3], node_duration [n_prob][max_path_nodes] (each may
 * be NULL; input and duration of the first node are written as 0, the reference leaves them unset); shot, t_shot,
 * coef_shot [n_prob][3][4] (axis, power); T_sum; ts_out (the adjusted knot span); seg_num; n_samples; samples
 * [n_prob][max_samples][3] (entries past n_samples unspecified); derivs [n_prob][4][3]. */
int fuelmi_map_kino_paths(fuelmi_map* m, const fuelmi_kino_cfg* cfg, int n_prob, const double* start_xyz,
                          const double* start_vel, const double* start_acc, const double* goal_xyz,
                          const double* goal_vel, int* status, int* which, int* iter_num, int* use_node_num,
                          int* n_nodes, double* node_state, double* node_input, double* node_duration, int* shot,
                          double* t_shot, double* coef_shot, double* T_sum, double* ts_out, int* seg_num,
                          int* n_samples, double* samples, double* derivs);
/* The device chain search -> fitted batch, the counterpart of fuelmi_bspline_dev_load_waypoints: one problem per
 * candidate of `b` (C = the batch's n_traj, inputs [C][3]), seg_num forced to point_num - bspline_degree (cfg->seg_num
 * must be 0 or that; cfg->max_samples and cfg->max_path_nodes are ignored), ts | points | derivs written into the
 * batch's staging by the kernel and the spline fit queued behind it on the map's stream.  A candidate whose status
 * yields no path (NO_PATH, CLOSE_GOAL, -1) keeps the state it had in the batch.  status [C]; T_sum [C] or NULL.  Same
 * host checks and return values as above; one host wait, for the statuses.  With profiling on, only the fit is counted
 * under FUELMI_K_BSPLINE; the search kernel belongs to no stage. */
int fuelmi_bspline_dev_load_kino(fuelmi_bspline_dev* b, const fuelmi_kino_cfg* cfg, const double* start_xyz,
                                 const double* start_vel, const double* start_acc, const double* goal_xyz,
                                 const double* goal_vel, int* status, double* T_sum);
/* what the kernel needs for cfg (host only, no device needed): out8 = {lanes per problem, LDS bytes, workspace bytes per
 * problem, primitives in the init list, primitives in the regular list, FUELMI_KINO_MAX_PRIMS, FUELMI_KINO_MAX_ALLOC,
 * hash slots per problem}.  cfg is checked like above. */
int fuelmi_kino_plan(const fuelmi_kino_cfg* cfg, long long out8[8]);

/* ------------------------------------------------------------------------------------------
 * Topological path search of guided replanning: TopologyPRM::findTopoPaths (path_searching/src/topo_prm.cpp:43-98),
 * the producer of the guide paths of FastPlannerManager::topoReplan (plan_manage/src/planner_manager.cpp:425-466), for
 * n_prob independent problems on one map in one call.  Per problem, everything f64 in the reference's order:
 *   1. createGraph (:100-188) over the problem's SAMPLE STREAM: samples [max_sample_num][3] are the raw numbers
 *      rand_pos_(eng_) would have returned, in [-1, 1); the kernel applies sample_r_, rotation_ and translation_
 *      (:113-128, :240-250).  There is no wall-clock cap (max_sample_time does not exist): exactly max_sample_num samples
 *      are taken, so a result never depends on the machine's speed.  A sample with evaluateCoarseEDT <= clearance is
 *      dropped; findVisibGuard walks the guards in list order up to the third visible one; no visible guard: a new
 *      guard; exactly two: needConnection (:210-238, with the move of an existing connector to the shorter position);
 *      one or three: nothing.
 *   2. pruneGraph (:272-299); searchPaths / depthFirstSearch (:606-684): neighbour order, the stop at max_raw_path, the
 *      bucket-by-node-count filter up to max_raw_path2.
 *   3. shortcutPaths (:516-531, one iteration a path), pruneEquivalent (:301-337), selectShortPaths (:339-377: reserve_num,
 *      ratio_to_short, the merge with start_pts / end_pts, five shortcut iterations, the second prune).
 * lineVisib (:252-270) is RayCaster::setInput / step (plan_env/src/raycast.cpp:228-321): the start voxel is tested, the
 * end voxel is not, the index is int(ray_pt + offset_), a voxel outside the map reads -1 and blocks the ray.
 * Decisions on the distance field (`dist <= thresh` for resolution, 0 and clearance) are the reference's: the positive
 * part of its field is res * sqrt(k) for an integer k, so each threshold becomes the largest k the f64 comparison
 * accepts, and the kernel compares the device's f32 field with a cut between its values for k and k + 1.  Only the
 * gradient push of shortcutPath uses the f32 values as numbers (trilinear getDistWithGrad).
 * Per-problem status: FUELMI_TOPO_OK; FUELMI_TOPO_NO_PATH (the select set is empty); FUELMI_TOPO_UNDEFINED where the
 * reference's behaviour is undefined (discretizePath(path, pt_num) with pt_num < 2 or without a segment for a point, a
 * raw path of 100 nodes or more, a point that is not finite: nothing is read out of bounds, no path outputs are written,
 * the other problems complete and the call stays FUELMI_OK); -1: over max_nodes / max_path_points (full counts and
 * lengths, truncated arrays) or over one of the kernel's own caps below (no path outputs), call status FUELMI_ELIMIT.
 * FUELMI_EINVAL before any launch: a coordinate that is not finite or >= 1e7 in magnitude, |end - start| <= resolution,
 * a sample outside [-1, 1), clearance < 0, counts < 1.  FUELMI_ELIMIT before any launch: a cfg field over its cap,
 * n_prob x workspace bytes > FUELMI_TOPO_MAX_WORKSPACE.  n_prob = 0 is FUELMI_OK.  A result does not depend on the
 * problem's place in the batch.  Runs on the map's stream: host arrays in, host arrays out, synchronous; the
 * workspace is one grow-only allocation on the map (fuelmi_map_topo_pool_bytes).
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_TOPO_OK 0
#define FUELMI_TOPO_NO_PATH 1
#define FUELMI_TOPO_UNDEFINED 2
#define FUELMI_TOPO_MAX_SAMPLES 8190              /* largest max_sample_num: a graph holds max_sample_num + 2 nodes */
#define FUELMI_TOPO_MAX_RAW 4096                  /* largest max_raw_path / max_raw_path2 / reserve_num */
#define FUELMI_TOPO_MAX_PATH_POINTS 256           /* points of a shortened or merged path; largest max_path_points */
#define FUELMI_TOPO_MAX_DIS_POINTS 4096           /* points of discretizePath(path) */
#define FUELMI_TOPO_MAX_NEIGHBORS 64              /* neighbours of one node */
#define FUELMI_TOPO_MAX_POINTS_IN 64              /* largest max_start / max_end */
#define FUELMI_TOPO_MAX_WORKSPACE 8589934592.0    /* bytes, n_prob x workspace of one problem */
typedef struct {
  double sample_inflate[3];  /* topo_prm/sample_inflate_x, _y, _z */
  double clearance;          /* topo_prm/clearance */
  double ratio_to_short;     /* topo_prm/ratio_to_short */
  int max_sample_num;        /* topo_prm/max_sample_num: the length of a problem's sample stream */
  int max_raw_path;          /* topo_prm/max_raw_path */
  int max_raw_path2;         /* topo_prm/max_raw_path2: also the rows of the raw / filtered path sets */
  int reserve_num;           /* topo_prm/reserve_num: also the rows of the select set */
  int max_path_points;       /* stride / cap of a path's points */
  int max_nodes;             /* stride / cap of the graph's nodes */
} fuelmi_topo_cfg;
/* In: start_xyz, end_xyz [n_prob][3]; start_pts [n_prob][max_start][3] with n_start [n_prob], end_pts likewise (the
 * pointers may be NULL when the stride is 0); samples [n_prob][max_sample_num][3].
 * Out (status, counts, events required, the others may be NULL): status [n_prob]; counts [n_prob][4]: raw paths found by
 * the depth-first search, kept by the bucket filter, left by the first pruneEquivalent, selected; events [n_prob][6]: samples rejected by
 * clearance, guards added, connectors added, connectors moved, samples that saw three guards, shortcut roll-backs;
 * the pruned graph in list order: n_nodes, node_id / node_type (GraphNode::Guard = 1, Connector = 2) [n_prob][max_nodes],
 * node_xyz [n_prob][max_nodes][3], nb_off [n_prob][max_nodes + 1] and nb_ids [n_prob][4 max_nodes] (node i's neighbours,
 * as ids in the reference's order, are nb_ids[nb_off[i] .. nb_off[i + 1]); a problem over max_nodes (status -1) holds
 * its first max_nodes nodes, and their neighbour ids only as far as the 4 max_nodes slots reach: nb_off never points
 * past them); the path sets raw_paths / filt_paths
 * [n_prob][max_raw_path2][max_path_points][3] with raw_len / filt_len [n_prob][max_raw_path2] (the filtered set is
 * what the caller of findTopoPaths gets back: selectShortPaths erases the paths it takes from it), sel_paths
 * [n_prob][reserve_num][max_path_points][3] with sel_len and sel_length (pathLength) [n_prob][reserve_num]. */
int fuelmi_map_topo_paths(fuelmi_map* m, const fuelmi_topo_cfg* cfg, int n_prob, const double* start_xyz,
                          const double* end_xyz, int max_start, const int* n_start, const double* start_pts, int max_end,
                          const int* n_end, const double* end_pts, const double* samples, int* status, int* counts,
                          int* events, int* n_nodes, int* node_id, int* node_type, double* node_xyz, int* nb_off,
                          int* nb_ids, double* raw_paths, int* raw_len, double* filt_paths, int* filt_len,
                          double* sel_paths, int* sel_len, double* sel_length);
/* the kernel's shape for cfg (host only, no device needed): out = {lanes per problem, LDS bytes, workspace bytes per
 * problem, the guard chunk (guards tested in one step of findVisibGuard), FUELMI_TOPO_MAX_SAMPLES, _MAX_RAW,
 * _MAX_PATH_POINTS, _MAX_DIS_POINTS, _MAX_NEIGHBORS, nodes of a raw path from which on the problem is UNDEFINED (100),
 * _MAX_POINTS_IN, _MAX_WORKSPACE}.  cfg is checked like above.  (The neighbour stride is 4 max_nodes, see above.) */
int fuelmi_topo_plan(const fuelmi_topo_cfg* cfg, long long out[12]);
/* bytes of the map's grow-only workspace of the topological search (0 before the first call) */
long long fuelmi_map_topo_pool_bytes(const fuelmi_map* m);

/* ------------------------------------------------------------------------------------------
 * Collision ranges of the initial local segment: FastPlannerManager::findCollisionRange
 * (plan_manage/src/planner_manager.cpp:636-691), the producer of colli_start.front(), colli_end.back(), start_pts and
 * end_pts that topoReplan (:418-432) hands to findTopoPaths, for n_prob UNIFORM position splines on one map in one call.
 * The reference's copy is private and reads the host's distance_buffer_; this one reads the device's field, no host
 * mirror is read or needed.  Per problem, everything f64 in this order:
 *   1. knots as setUniformBspline builds them (see fuelmi_map_check_trajs: accumulated); t_m = u[p], t_mp = u[m - p].
 *   2. tick k = 0, 1, ...: tc starts at t_m and is ACCUMULATED by += 0.05 (never k * 0.05), while tc <= t_mp + 1e-4;
 *      the point is evaluateDeBoor(tc) with its clamp; safe = !(getDistance(point) < clearance), where getDistance reads
 *      the voxel of floor((p - origin) * resolution_inv) and an index outside the map reads -1: UNSAFE for every accepted
 *      clearance.  The comparison is the reference's f64 `res * sqrt(k) < clearance`, STRICT, taken on the device's f32
 *      field through a host-computed cut (as the topological search takes its `<=`, above).
 *   3. events, last_safe = true at first: safe -> unsafe pushes evaluateDeBoor(tc - 0.05) to colli_start (the time is
 *      recomputed from this tick's tc) and `if (t_s < 0) t_s = tc - 0.05`, t_s = -1 at first -- an unsafe tick 0 leaves
 *      t_s = -0.05 < 0, so the NEXT start event overwrites it; unsafe -> safe pushes the point to colli_end, t_e = tc.
 *   4. status FUELMI_COLRANGE_NO_COLLISION without a start event; FUELMI_COLRANGE_ENDS_IN_OBSTACLE with one start event
 *      and no end event (topoReplan does not replan then); otherwise FUELMI_COLRANGE_OK and start_pts / end_pts as
 *      :665-690: sn = ceil((t_s - t_m) / dt), dt' = (t_s - t_m) / sn, points at tc = t_m, += dt' (accumulated) while
 *      tc <= t_s + 1e-4; the end side from t_e to t_mp likewise when its dt' > 1e-4, else the single point at t_mp.
 *      sn = 0 is what IEEE makes of it: 0 / 0 = NaN step, exactly one start point; negative / 0 = -inf, no start point;
 *      on the end side both fall to the single point.
 * Outputs per problem: status; n_ticks (loop bodies); n_start_events / n_end_events (the sizes of colli_start /
 * colli_end); t_s (-1 without a start event), t_e (0 without an end event); colli_start / colli_end [max_events][3];
 * start_pts / end_pts [max_pts][3] with n_start_pts / n_end_pts, in the layout fuelmi_map_topo_paths takes for
 * max_start = max_end = max_pts; first_start = colli_start.front() and last_end = colli_end.back() [3], the two points
 * topoReplan passes on (zeros where there is none).  Rows that are not written are zero.
 * Defined where the reference is not:
 *   FUELMI_COLRANGE_NONFINITE  a control point or the knot span is not finite (or the knots overflow): nothing is
 *               evaluated, every other output of the problem is zero, the other problems complete.
 *   -1          more than max_events start or end events, more than max_pts start or end points, or more than
 *               FUELMI_TRAJCHK_MAX_SAMPLES ticks: the counts are full (n_ticks stops at the cap, and a problem over the
 *               tick cap has no start_pts / end_pts), the arrays hold their first rows, the call returns FUELMI_ELIMIT.
 * FUELMI_EINVAL before any launch: pointers; degree outside 3..5; clearance < 0 or not finite; max_events or max_pts < 1;
 * n_ctrl[i] < degree + 1 or > max_ctrl; knot span <= 0; a finite coordinate with |coordinate| >= 1e7.  FUELMI_ELIMIT
 * before any launch: max_ctrl > FUELMI_TRAJCHK_MAX_CTRL, max_events > FUELMI_COLRANGE_MAX_EVENTS, max_pts >
 * FUELMI_TOPO_MAX_POINTS_IN.  n_prob = 0 is FUELMI_OK.  Runs on the map's stream behind whatever ESDF update was queued
 * before it: host arrays in and out, synchronous, one thread at a time per map; its scratch is one grow-only allocation
 * on the map.  One 64-lane wave per problem, 64 ticks a window; a result does not depend on the problem's place in the
 * batch.  The control points come from fuelmi_map_local_segments (below).  Out of scope: evaluateCoarseEDT with
 * time >= 0, moved knots as input, chaining the outputs on the device.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_COLRANGE_OK 0
#define FUELMI_COLRANGE_NO_COLLISION 1
#define FUELMI_COLRANGE_ENDS_IN_OBSTACLE 2
#define FUELMI_COLRANGE_NONFINITE 3
#define FUELMI_COLRANGE_MAX_EVENTS 4096       /* largest max_events */
typedef struct {
  int degree;          /* degree of the position spline, 3..5 (pp_.bspline_degree_) */
  int max_ctrl;        /* stride of pos_ctrl */
  int max_events;      /* stride / cap of colli_start and colli_end */
  int max_pts;         /* stride / cap of start_pts and end_pts */
  double clearance;    /* topo_prm/clearance (TopologyPRM::clearance_) */
} fuelmi_colrange_cfg;
/* pos_ctrl [n_prob][max_ctrl][3], n_ctrl / knot_span [n_prob].  Out, per problem, all required: see above. */
int fuelmi_map_collision_ranges(fuelmi_map* m, const fuelmi_colrange_cfg* cfg, int n_prob, const int* n_ctrl,
                                const double* pos_ctrl, const double* knot_span, int* status, int* n_ticks,
                                int* n_start_events, int* n_end_events, double* t_s, double* t_e, double* colli_start,
                                double* colli_end, int* n_start_pts, double* start_pts, int* n_end_pts, double* end_pts,
                                double* first_start, double* last_end);
/* the kernel's shape for cfg (host only, no device needed): out6 = {lanes per problem (= ticks per window), dynamic LDS
 * bytes of a workgroup, problems per workgroup, the tick cap, largest max_ctrl, largest max_pts}.  cfg is checked like
 * above. */
int fuelmi_colrange_plan(const fuelmi_colrange_cfg* cfg, int out6[6]);

/* ------------------------------------------------------------------------------------------
 * Guide points of a topological guide path: the head of FastPlannerManager::optimizeTopoBspline
 * (plan_manage/src/planner_manager.cpp:553-577) for n_path paths in one call -- sel_paths / sel_len of
 * fuelmi_map_topo_paths as they stand.  It hangs on the map for its stream and scratch and reads no voxel.  Per path,
 * everything f64 in this order:
 *   1. seg_num = max(6, int(pathLength(path) / ctrl_pt_dist)), the length summed left to right (topo_prm.cpp:417-425);
 *   2. dt = duration / double(seg_num);
 *   3. n_pts = the bodies of `for (tp = 0; tp <= duration + 1e-4; tp += dt)`, tp ACCUMULATED (getTrajInfoInDuration,
 *      plan_container.hpp:77): the points reparamLocalTraj samples;
 *   4. n_ctrl = n_pts + 2, the rows parameterizeToBspline returns;
 *   5. degree 3 or 5: discretizePath(path, n_ctrl - 2) without its first two and last two points, n_guide = n_ctrl - 6
 *      (for degree 5 this is the reference's count, NOT the N - 2 order = n_ctrl - 10 rows fuelmi_bspline_problem's guide
 *      layout holds, so a degree-5 result does not fit that layout as it stands); degree 4: discretizePath(path, 2 n_ctrl - 7), the odd i with 5 <= i <= size - 6,
 *      n_guide = n_ctrl - 8.  For degrees 3 and 4 the rows are what fuelmi_bspline_problem.guide_pts takes.
 *   discretizePath(path, pt_num) is topo_prm.cpp:427-461, literal: the FIRST segment whose +-1e-4 range holds the
 *   point's arc length; lambda may leave [0, 1]; a chosen segment of length zero gives the NaN or inf IEEE gives, and it
 *   is written out.
 * Outputs per path: status, seg_num, dt, n_pts, n_ctrl, n_guide, guide_pts [max_guide][3] (rows not written are zero).
 * Status: FUELMI_TOPO_OK; FUELMI_TOPO_UNDEFINED where the reference's behaviour is undefined -- path_len < 2, a length /
 * ctrl_pt_dist that is not finite (the cast to int), a discretised point without a segment (every point of
 * discretizePath counts, kept or not): n_guide = 0 and no guide point is written, what was computed before that stays
 * (seg_num .. n_ctrl; all zero for the first two causes), the other paths complete and the call stays FUELMI_OK;
 * -1: seg_num or n_pts over FUELMI_GUIDE_MAX_PTS (nothing further is computed) or n_guide > max_guide (full count, the
 * first max_guide rows), call status FUELMI_ELIMIT.  Path coordinates are NOT checked: every value is defined above.
 * FUELMI_EINVAL before any launch: pointers, degree outside 3..5, ctrl_pt_dist or a duration not finite or <= 0,
 * max_path_points < 1, path_len[i] outside 0 .. max_path_points, max_guide < 1.  FUELMI_ELIMIT before any launch:
 * max_path_points > FUELMI_TOPO_MAX_PATH_POINTS, max_guide > FUELMI_GUIDE_MAX_PTS.  n_path = 0 is FUELMI_OK.  One
 * 64-lane wave per path, one lane per discretised point; synchronous on the map's stream.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_GUIDE_MAX_PTS 65536            /* largest seg_num, n_pts and max_guide */
int fuelmi_map_guide_points(fuelmi_map* m, int n_path, int max_path_points, const double* paths, const int* path_len,
                            const double* duration, double ctrl_pt_dist, int degree, int max_guide, int* status,
                            int* seg_num, double* dt, int* n_pts, int* n_ctrl, int* n_guide, double* guide_pts);

/* ------------------------------------------------------------------------------------------
 * Local segments of the global trajectory: FastPlannerManager::paramLocalTraj / reparamLocalTraj
 * (plan_manage/src/planner_manager.cpp:605-634), the producers of the control points every call of the guided-replanning
 * chain above starts from, for n_prob problems on n_traj trajectory states in one call.  A state is what GlobalTrajData
 * (plan_manage/include/plan_manage/plan_container.hpp) holds: the polynomial global trajectory (n_seg segments,
 * seg_times / coef as fuelmi_map_waypoint_trajs returns them), global_duration, the uniform local spline (n_local_ctrl
 * control points of the call's degree with local_knot_span; 0: none yet, as setGlobalTraj leaves it with
 * local_ts = local_te = -1) and local_ts, local_te, time_change, last_time_inc.  A problem names its state (traj_of),
 * a mode, start_t and two arguments; several problems may name one state.  It hangs on the map for its stream and
 * scratch and reads no voxel.  Per problem, everything f64 `+ - * / sqrt floor` in this order:
 *   getState(t, k) (:64-71), the three branches literal, the comparisons inclusive:
 *     t >= -1e-3 && t <= local_ts:                      the polynomial at (t - time_change) + last_time_inc
 *     else t >= local_te && t <= global_duration + 1e-3: the polynomial at t - time_change
 *     else:                                             evaluateDeBoorT(t - local_ts) of the local spline's k-th
 *                                                       derivative spline (setUniformBspline's accumulated knots,
 *                                                       getDerivative, the clamp: see fuelmi_map_sample_trajs)
 *     The polynomial is PolynomialTraj::evaluate as fuelmi_map_waypoint_trajs has it: `times[idx] + 1e-4 < ts` walks the
 *     segments, idx clamped to the last one where the reference reads past its vector; powers as repeated products,
 *     summed from the lowest power.
 *   FUELMI_LOCALSEG_SPHERE (arg0 = radius, arg1 = dist_pt): getTrajInfoInSphere (:88-112), i.e. paramLocalTraj.
 *     first = getState(start_t, 0); while |cur - first| < radius && start_t + segment_time < global_duration - 1e-3:
 *     segment_time = min(segment_time + 0.2, global_duration - start_t) (the 0.2 ACCUMULATED), cur = getState(start_t +
 *     segment_time, 0), segment_len += |cur - prev| in step order; the norms are sqrt(x x + y y + z z).  n_steps = the
 *     bodies run.  seg_num = max(6, int(min(floor(segment_len / dist_pt), FUELMI_WPTRAJ_MAX_SEG))), duration =
 *     segment_time, dt = duration / seg_num; then as DURATION.
 *   FUELMI_LOCALSEG_DURATION (arg0 = duration, arg1 = dt): getTrajInfoInDuration (:74-85), i.e. reparamLocalTraj;
 *     n_steps = 0, segment_len = 0, seg_num = 0.  points = getState(start_t + tp, 0) for (tp = 0; tp <= duration + 1e-4;
 *     tp += dt), tp ACCUMULATED: n_points is the result of that accumulation, not seg_num + 1 (it stops counting at the
 *     first multiple of 64 above FUELMI_WPTRAJ_MAX_SEG + 2).  derivs [4][3] = getState(start_t, 1), getState(start_t +
 *     duration, 1), then the same two with k = 2: the layout fuelmi_bspline_parameterize takes.
 *   ctrl = parameterizeToBspline of the problem's n_points points with ts = dt, bit for bit what
 *     fuelmi_bspline_parameterize returns for them; n_ctrl = n_points + degree - 1.  Each problem has its own count.
 * Outputs per problem: status, n_steps, segment_len, seg_num, duration, dt, n_points, points [max_points][3], derivs,
 * n_ctrl, ctrl [max_points + degree - 1][3].  Rows that are not written are zero.
 * Status, defined where the reference is not:
 *   FUELMI_LOCALSEG_OK
 *   FUELMI_LOCALSEG_DEGENERATE  dt is not finite or <= 0 (SPHERE with start_t >= global_duration - 1e-3 has duration 0 and
 *               the reference loops forever on tp += 0), or fewer than 2 points; parameterizeToBspline rejects both.
 *               n_steps, segment_len, seg_num, duration and dt are as computed; n_points = 0, no points, derivs, ctrl.
 *   FUELMI_LOCALSEG_NO_LOCAL    a getState of the problem falls to the local branch of a state with n_local_ctrl = 0
 *               (the reference indexes an empty vector): every output of the problem is zero.
 *   -1          more than max_points points: n_points is the full count, the first max_points rows and derivs are
 *               written, n_ctrl = 0 and no ctrl; the call returns FUELMI_ELIMIT; the other problems complete.
 * FUELMI_EINVAL before any launch: pointers; degree outside 3..5; max_seg < 1, max_ctrl < degree + 1 or max_points < 2;
 * n_seg[i] outside 1..max_seg; n_local_ctrl[i] not 0 and outside degree + 1 .. max_ctrl; a local knot span <= 0 (where
 * there is a local spline); traj_of outside 0 .. n_traj - 1; an unknown mode; any value read that is not finite or with
 * |value| >= 1e7; SPHERE with radius or dist_pt not > 0.  FUELMI_ELIMIT before any launch: max_seg >
 * FUELMI_WPTRAJ_MAX_WAY - 1, max_ctrl > FUELMI_TRAJCHK_MAX_CTRL, max_points > FUELMI_LOCALSEG_MAX_POINTS, a
 * global_duration > FUELMI_WPTRAJ_MAX_DURATION (with start_t >= 0 that bounds the step loop at 50 001 bodies).
 * n_prob = 0 is FUELMI_OK.  Host arrays in and out, synchronous on the map's stream, one thread at a time per map; its
 * scratch is one grow-only allocation on the map.  One 64-lane wave per problem, 64 steps / points a window; a result
 * does not depend on the problem's place in the batch.  Out of scope: planGlobalTraj's way-point insertion and end ramps
 * (the polynomial is an input), setLocalTraj's bookkeeping (the four times are inputs), non-uniform local knots.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_LOCALSEG_SPHERE 0
#define FUELMI_LOCALSEG_DURATION 1
#define FUELMI_LOCALSEG_OK 0
#define FUELMI_LOCALSEG_DEGENERATE 1
#define FUELMI_LOCALSEG_NO_LOCAL 2
#define FUELMI_LOCALSEG_MAX_POINTS 1024       /* largest max_points (the fit's LDS) */
typedef struct {
  int degree;          /* 3..5: the local spline's and the fit's (pp_.bspline_degree_) */
  int max_seg;         /* stride of seg_times / coef, <= FUELMI_WPTRAJ_MAX_WAY - 1 */
  int max_ctrl;        /* stride of local_ctrl, <= FUELMI_TRAJCHK_MAX_CTRL */
  int max_points;      /* stride / cap of points; ctrl has max_points + degree - 1 rows */
} fuelmi_localseg_cfg;
/* states: n_seg / global_duration / n_local_ctrl / local_knot_span / local_ts / local_te / time_change / last_time_inc
 * [n_traj], seg_times [n_traj][max_seg], coef [n_traj][max_seg][3][6], local_ctrl [n_traj][max_ctrl][3].  problems:
 * traj_of / mode / start_t / arg0 / arg1 [n_prob].  Out, per problem, all required: see above. */
int fuelmi_map_local_segments(fuelmi_map* m, const fuelmi_localseg_cfg* cfg, int n_traj, const int* n_seg,
                              const double* seg_times, const double* coef, const double* global_duration,
                              const int* n_local_ctrl, const double* local_ctrl, const double* local_knot_span,
                              const double* local_ts, const double* local_te, const double* time_change,
                              const double* last_time_inc, int n_prob, const int* traj_of, const int* mode,
                              const double* start_t, const double* arg0, const double* arg1, int* status, int* n_steps,
                              double* segment_len, int* seg_num, double* duration, double* dt, int* n_points,
                              double* points, double* derivs, int* n_ctrl, double* ctrl);
/* the kernel's shape for cfg (host only, no device needed): out8 = {lanes per problem (= steps / points per window),
 * dynamic LDS bytes of a workgroup, problems per workgroup, largest max_seg, largest max_ctrl, largest max_points, the
 * point count at which counting stops at the latest, dynamic LDS bytes of the fit for max_points}.  cfg is checked like
 * above. */
int fuelmi_localseg_plan(const fuelmi_localseg_cfg* cfg, int out8[8]);
/* The batch route: one problem per candidate of a device batch (fuelmi_bspline_dev_create), the load_waypoints pattern.
 * The same kernel writes knot span | points | derivatives into the batch's staging and the fit follows on the map's
 * stream, so the batch afterwards holds what fuelmi_bspline_dev_load_samples would have been given: the call above
 * without its host round trip.  degree and the point count are the batch's (max_points = N - degree + 1); the states
 * and problems are as above, with n_prob = the batch's candidates.  status [C] as above, and
 *   FUELMI_LOCALSEG_MISFIT  the problem's n_points + degree - 1 is not the batch's point_num.
 * A candidate whose status is not FUELMI_LOCALSEG_OK keeps the state it had; the call stays FUELMI_OK.  duration [C]
 * may be null.  Checks as above.  Synchronous. */
#define FUELMI_LOCALSEG_MISFIT 3
int fuelmi_bspline_dev_load_local_segments(fuelmi_bspline_dev* b, int max_seg, int max_ctrl, int n_traj, const int* n_seg,
                                           const double* seg_times, const double* coef, const double* global_duration,
                                           const int* n_local_ctrl, const double* local_ctrl,
                                           const double* local_knot_span, const double* local_ts, const double* local_te,
                                           const double* time_change, const double* last_time_inc, const int* traj_of,
                                           const int* mode, const double* start_t, const double* arg0, const double* arg1,
                                           int* status, double* duration);

/* ------------------------------------------------------------------------------------------
 * Information gain of camera views and the yaw search of HeadingPlanner
 * (active_perception/src/heading_planner.cpp), the hot part of FastPlannerManager::planYawActMap
 * (plan_manage/src/planner_manager_dev.cpp:7-113) and of localExplore (:128-247), on the device's own unknown and
 * occupied bit planes: no host mirror is read or needed.
 *
 * fuelmi_map_info_gains: n_group view groups; a group is one camera position and n_yaw[g] <= max_yaw yaws.
 * calcInfoGain (:324-391) is a group of one yaw with in_box = 0 and UNIFORM; one layer of searchPathOfYaw (:187-203) is
 * a group of 2 * half_vert_num + 1 yaws with in_box = 1.  Per view, kept literally:
 *   1. The camera transform (:240-248): R_wb = Rz(yaw), T_wc = T_wb * T_bc with T_bc = T_cb^-1 (:151-152), so
 *      R_wc = [[sin, 0, cos], [-cos, 0, sin], [0, 1, 0]] and t_wc = pt.  The four plane normals (:121-128, built from
 *      sin / cos of pi/2 - the half angle) rotated by R_wc (:251-253).
 *   2. calcFovAABB (:401-418): the five vertices R_wc * v + t_wc of :136-139 -- lefttop's x is -far * TAN(left_ang), the
 *      other three are sines -- and t_wc; their bounding box; SDFMap::boundBox against the exploration box
 *      (sdf_map.h:189-194); posToIndex (floor) of both corners.
 *   3. The loops x, y, z over the index box (:268-270) with `x % factor == 0 && y % factor == 0 && z % factor == 0` on
 *      the INDEX (:272).
 *   4. `if (!sdf_map_->getOccupancy(pt_idx) == SDFMap::UNKNOWN) continue;` (:275).  As written `!` binds first:
 *      (!occ) == 0, which is true for every occ != 0 -- FREE, OCCUPIED and the -1 of an index outside the map.  So the
 *      line skips every KNOWN cell and every cell outside the map, and only unknown cells go on.
 *   5. in_box: isInBox(Vector3i) (sdf_map.h:171-178), box_min <= id < box_max (:276; calcInfoGain has no such line).
 *   6. insideFoV (:475-487) of indexToPos(id): |p - pt| > far is outside, then dot(p - pt, n) < 0.1 is outside per
 *      normal in the order top, bottom, left, right.  A cell that passes is a CANDIDATE (n_cand).
 *   7. The ray (:290-299): RayCaster::setInput(check_pt / resolution, pt / resolution), divisions by the resolution;
 *      every voxel step() hands out is read at int(ray + offset), offset = 0.5 - origin / resolution, the cast
 *      truncating toward zero; a voxel outside the map is not occupied; the start voxel is tested, the end voxel is
 *      not.  A candidate whose ray met no occupied voxel is VISIBLE (n_visible).
 *   8. UNIFORM: gain = n_visible.  NON_UNIFORM: gain = sum over the visible cells of exp(-lambda1 * d1 - lambda2 * d2),
 *      distToPathAndCurPos (:452-473): d1 the distance to the FIRST nearest control point (strict <), d2 the polyline
 *      length up to it summed from index 0.
 * Each view's rotation, rotated normals and index box are computed on the host inside the call, with libm and f64 in
 * the reference's order, so every frustum decision is the reference's; cells, rays, weights and sums run on the device.
 * The CastFlags cache (:280-308) is a memo -- a cell's ray depends on the position, not the yaw -- and is restated as
 * one: the rays of a group are walked once (n_rays [n_group]: the cells that are a candidate of at least one view)
 * and shared by its yaws.  A group of K yaws equals K groups of one yaw bit for bit.  The reference's races on that
 * array and its fixed 1 000 000 entries are not reproduced.  UNIFORM gains are exact counts; a NON_UNIFORM sum is
 * taken in an order fixed by the cells' own indices (not the reference's x, y, z order): the same bits on every run and
 * at every place in a batch, within tests/heading_ref.py parity_tolerance of the reference's sum.
 * Defined where the reference is not: a ray that has not met its end voxel after |dx| + |dy| + |dz| + 2 steps (the
 * reference would walk on for ever) counts as blocked.
 *   status -1   the group's subsampled union box holds more than FUELMI_GAIN_MAX_CELLS cells: its outputs are zero, the
 *               other groups complete, the call returns FUELMI_ELIMIT.
 * FUELMI_EINVAL before any launch: pointers; weight_type; factor < 1; far / angles / lambdas not finite, far <= 0 or
 * > 1e3; n_yaw[g] outside 0 .. max_yaw; a position or yaw that is not finite or a coordinate with |.| >= 1e7; under
 * NON_UNIFORM path_of[g] outside 0 .. n_path - 1, n_ctrl[p] outside 1 .. max_ctrl, a control point not finite.
 * FUELMI_ELIMIT before any launch: max_yaw > FUELMI_GAIN_MAX_YAW, max_ctrl > FUELMI_GAIN_MAX_CTRL.  n_group = 0 is
 * FUELMI_OK.  Runs on the map's stream behind the mutators queued before it: host arrays in and out, synchronous, one
 * thread at a time per map; its scratch is one grow-only allocation on the map.  One workgroup per group; a result
 * does not depend on the group's place in the batch.
 *
 * fuelmi_map_yaw_paths: n_prob problems of searchPathOfYaw (:170-234).  Layer 0 and layer n_layer - 1 hold the one
 * vertex (yaws[i], gain 0); an inner layer i holds the 2h + 1 vertices yaws[i] + double(j - h) * yaw_diff with the
 * gain of the view (pts[i], that yaw), in_box and weight type as cfg.gain says.  gains_in given: no ray is walked, the
 * search runs on those numbers (n_rays = 0).  Graph::dijkstraSearch (:52-100) is a FIFO label update on a layered
 * complete graph -- all of layer i is popped before any of layer i + 1 -- so it is this recurrence: g of the start is
 * 0; for a vertex b of layer i + 1 the predecessors c of layer i are taken in layer order, g_tmp = g_c - gain_b +
 * w * penal(|yaw_c - yaw_b|), penal(d) = 0 for yr = d / dt <= max_yaw_rate, else (yr - max_yaw_rate)^2 (:42-49); the
 * first predecessor sets g and the parent unconditionally, a later one replaces them unless g_tmp > g (:87-94: a tie
 * goes to the LATER predecessor).  Out per problem: status; path [max_layer] the yaws from start to goal; path_vertex
 * [max_layer] the index j per layer (0 for the first and last); gains and g_value [max_layer][2h + 1] (rows 0 and
 * n_layer - 1 use entry 0; what is not written is zero); n_rays [max_layer].
 * Defined where the reference is not: n_layer = 1: the path is the one yaw.  status -1: a layer's group is over
 * FUELMI_GAIN_MAX_CELLS; the problem's other outputs are zero, the others complete, FUELMI_ELIMIT.
 * FUELMI_EINVAL before any launch: as above, and n_layer[i] outside 1 .. max_layer, dt not finite or <= 0, yaw_diff /
 * max_yaw_rate / w or a gains_in entry not finite, half_vert_num < 0.  FUELMI_ELIMIT before any launch: 2h + 1 >
 * FUELMI_GAIN_MAX_YAW, max_layer > FUELMI_YAWPATH_MAX_LAYER, max_ctrl > FUELMI_GAIN_MAX_CTRL.  cfg.gain.max_yaw is
 * ignored (it is 2h + 1).  One wave per problem, one lane per candidate of the current layer.
 * Out of scope: the way-point sampling at the head of planYawActMap (fuelmi_map_plan_yaws' step 4 with other
 * constants) and its closing BsplineOptimizer::optimize; setFrontier / calcVisibFrontier / showVisibFrontier;
 * VisibilityUtil.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_GAIN_NON_UNIFORM 0  /* HeadingPlanner's enum (heading_planner.h) */
#define FUELMI_GAIN_UNIFORM 1
#define FUELMI_GAIN_MAX_YAW 31        /* largest max_yaw and 2 * half_vert_num + 1 */
#define FUELMI_GAIN_MAX_CELLS 12288   /* subsampled cells of a group's union box */
#define FUELMI_GAIN_MAX_CTRL 256      /* largest max_ctrl */
#define FUELMI_YAWPATH_MAX_LAYER 64   /* largest max_layer */
typedef struct {
  int weight_type;     /* FUELMI_GAIN_* (heading_planner/weight_type) */
  int in_box;          /* 1: calcInformationGain's isInBox test, 0: calcInfoGain */
  int factor;          /* the subsampling factor, 4 in the reference */
  int max_yaw;         /* stride of yaws / gain / n_cand / n_visible */
  int max_ctrl;        /* stride of ctrl */
  double far;          /* far_, 4.5 */
  double top_ang, left_ang, right_ang; /* 0.56125, 0.69222, 0.68901 */
  double lambda1, lambda2;             /* heading_planner/lambda1, lambda2 */
} fuelmi_gain_cfg;
typedef struct {
  fuelmi_gain_cfg gain;
  int half_vert_num;   /* heading_planner/half_vert_num */
  int max_layer;       /* stride of pts / yaws and of every per-layer output */
  double yaw_diff, max_yaw_rate, w; /* heading_planner/yaw_diff, max_yaw_rate, w */
} fuelmi_yawpath_cfg;
/* pos [n_group][3], n_yaw [n_group], yaws [n_group][max_yaw]; n_ctrl [n_path], ctrl [n_path][max_ctrl][3], path_of
 * [n_group] (all three may be null under UNIFORM).  Out: status / n_rays [n_group]; gain / n_cand / n_visible
 * [n_group][max_yaw], all required. */
int fuelmi_map_info_gains(fuelmi_map* m, const fuelmi_gain_cfg* cfg, int n_group, const double* pos, const int* n_yaw,
                          const double* yaws, int n_path, const int* n_ctrl, const double* ctrl, const int* path_of,
                          int* status, double* gain, int* n_cand, int* n_visible, int* n_rays);
/* n_layer / dt [n_prob], pts [n_prob][max_layer][3], yaws [n_prob][max_layer]; n_ctrl [n_prob], ctrl
 * [n_prob][max_ctrl][3] (problem i's own control points; may be null under UNIFORM or with gains_in); gains_in
 * [n_prob][max_layer][2h + 1] or null.  Out, all required: see above. */
int fuelmi_map_yaw_paths(fuelmi_map* m, const fuelmi_yawpath_cfg* cfg, int n_prob, const int* n_layer, const double* pts,
                         const double* yaws, const double* dt, const int* n_ctrl, const double* ctrl,
                         const double* gains_in, int* status, double* path, int* path_vertex, double* gains,
                         double* g_value, int* n_rays);
/* the kernels' shape for cfg (host only, no device needed): out10 = {lanes of a gain workgroup, its dynamic LDS bytes
 * for a group of FUELMI_GAIN_MAX_CELLS cells, groups per workgroup, FUELMI_GAIN_MAX_CELLS, FUELMI_GAIN_MAX_YAW,
 * FUELMI_GAIN_MAX_CTRL, lanes of a search problem, static LDS bytes of a search workgroup, search problems per
 * workgroup, FUELMI_YAWPATH_MAX_LAYER}.  cfg is checked like above. */
int fuelmi_yawpath_plan(const fuelmi_yawpath_cfg* cfg, int out10[10]);

/* ------------------------------------------------------------------------------------------
 * Safety check of planned trajectories: FastPlannerManager::checkTrajCollision
 * (plan_manage/src/planner_manager.cpp:96-118), which the exploration FSM's safetyCallback runs every 50 ms while a
 * trajectory is flown (exploration_manager/src/fast_exploration_fsm.cpp:335-345), for n_prob independent problems in
 * one call.  The position spline is UNIFORM (control points + one knot span, setUniformBspline); a time
 * reallocation is fuelmi_map_adjust_trajs, below, and the knots it moved go into fuelmi_map_check_trajs_knots (and,
 * for a device batch, FUELMI_KNOTS_ADJUSTED; both below).  Per problem, everything f64 in this order:
 *   1. knots as setUniformBspline builds them (non_uniform_bspline.cpp:25-31): u[i] = double(i - p) * dt for i <= p,
 *      then ACCUMULATED u[i] = u[i-1] + dt; duration = u[n_ctrl] - u[p].
 *   2. cur = evaluateDeBoorT(t_now) (the literal clamp, knot search and alpha recursion of :51-75).
 *   3. radius = 0, fut_t = step; while (radius < max_radius && t_now + fut_t < duration):
 *        p = evaluateDeBoorT(t_now + fut_t);
 *        if getInflateOccupancy(p) == 1: UNSAFE, distance = radius, stop;
 *        radius = sqrt(dx dx + dy dy + dz dz) of p - cur, summed left to right;  fut_t += step (ACCUMULATED, never
 *        k * step).
 *   4. getInflateOccupancy(Vector3d) (sdf_map.h:127-130, 163-169, 217-226): index floor((p - origin) * resolution_inv)
 *      per axis; an index outside the map gives -1, which PASSES; otherwise the voxel of the inflated plane as the last
 *      fuelmi_map_inflate_local (or upload) left it.  Neither the unknown nor the occupied plane is read.
 * Sample k = 1, 2, ... is the k-th loop body; r_k is the radius it computes, r_0 = 0.  Outputs per problem:
 *   status      FUELMI_TRAJCHK_OK, FUELMI_TRAJCHK_NONFINITE or -1 (below)
 *   safe        1: the loop ended without a hit (the reference returns true); 0 otherwise
 *   distance    unsafe: the reference's value r_(k-1) of the hit sample k; safe: -1 (the reference leaves the caller's
 *               variable untouched)
 *   n_samples   loop bodies entered
 *   hit_index   k of the hit, 0 without one;  hit_t = t_now + fut_t of that sample, hit_pos [3] its point (0 without)
 *   end_reason  FUELMI_TRAJCHK_END_HIT, _RADIUS (radius < max_radius failed; it is tested first), _DURATION
 *               (t_now + fut_t < duration failed), _CAP, _NONFINITE
 *   duration    of step 1
 * Defined where the reference is not:
 *   FUELMI_TRAJCHK_NONFINITE  an evaluated point (cur or a sample) is not finite or has |coordinate| >= 1e7 (the
 *               reference casts it to int: undefined): a failure on the safe side, safe = 0, distance = 0, end_reason
 *               _NONFINITE, hit_index / hit_t = the sample (0 / t_now for cur), hit_pos = 0, n_samples counts that
 *               sample.  Also (device batches only, the host route refuses it): a knot span that is not finite and
 *               > 0 -- then duration and n_samples are 0 as well.
 *   -1          more than FUELMI_TRAJCHK_MAX_SAMPLES loop bodies would be entered: the walk ends there, end_reason
 *               _CAP, safe = 0 (nothing was proven), distance = the radius reached, n_samples =
 *               FUELMI_TRAJCHK_MAX_SAMPLES; the other problems are complete and the call returns FUELMI_ELIMIT.
 * Checked on the host before anything is launched (FUELMI_EINVAL): pointers; degree in 3..5; degree + 1 <= n_ctrl[i]
 * <= max_ctrl; knot spans finite and > 0; control points finite with |coordinate| < 1e7; t_now finite; step finite and
 * >= 1e-3; max_radius finite and > 0.  max_ctrl > FUELMI_TRAJCHK_MAX_CTRL: FUELMI_ELIMIT.  n_prob = 0 is FUELMI_OK.
 * fuelmi_map_check_trajs runs on the map's stream, behind whatever inflation was queued before it (like
 * fuelmi_map_goal_paths): host arrays in and out, synchronous, one thread at a time per map (not a query-slot call);
 * its scratch is one grow-only allocation on the map.  No host mirror is read or needed.  One 64-lane wave per
 * problem; a result does not depend on the problem's place in the batch.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_TRAJCHK_OK 0
#define FUELMI_TRAJCHK_NONFINITE 1
#define FUELMI_TRAJCHK_END_HIT 0
#define FUELMI_TRAJCHK_END_RADIUS 1
#define FUELMI_TRAJCHK_END_DURATION 2
#define FUELMI_TRAJCHK_END_CAP 3
#define FUELMI_TRAJCHK_END_NONFINITE 4
#define FUELMI_TRAJCHK_MAX_CTRL 1024          /* largest max_ctrl (position control points per problem) */
#define FUELMI_TRAJCHK_MAX_SAMPLES 1048576    /* 2^20 loop bodies per problem */
typedef struct {
  int degree;          /* degree of the position spline, 3..5 (pp_.bspline_degree_) */
  int max_ctrl;        /* stride of pos_ctrl */
  double step;         /* 0.02 */
  double max_radius;   /* 6.0 */
} fuelmi_trajchk_cfg;
/* pos_ctrl [n_prob][max_ctrl][3], n_ctrl / knot_span / t_now [n_prob].  Out, per problem: status, safe, distance,
 * n_samples, hit_index, hit_t, hit_pos [n_prob][3], end_reason, duration. */
int fuelmi_map_check_trajs(fuelmi_map* m, const fuelmi_trajchk_cfg* cfg, int n_prob, const int* n_ctrl,
                           const double* pos_ctrl, const double* knot_span, const double* t_now, int* status, int* safe,
                           double* distance, int* n_samples, int* hit_index, double* hit_t, double* hit_pos,
                           int* end_reason, double* duration);
/* The same on whole knot vectors (setKnot, as local_data_.position_traj_ carries them behind a time adjustment) in place
 * of the spans: knots [n_prob][max_ctrl + degree + 1], the layout of fuelmi_map_adjust_trajs' knots_out, so that call's
 * output is this call's input as it stands.  Step 1 then takes problem i's n_ctrl[i] + degree + 1 knots as given;
 * duration stays u[n_ctrl] - u[p] and every evaluation stays evaluateDeBoorT (t + u[p] and the clamp).  Checked on the
 * host before anything is launched (FUELMI_EINVAL), beside everything above but the spans: knots not NULL, every knot
 * finite, every knot above the one in front of it.  Strict increase is more than the reference asks for: it asks for
 * nothing and divides by knot differences. */
int fuelmi_map_check_trajs_knots(fuelmi_map* m, const fuelmi_trajchk_cfg* cfg, int n_prob, const int* n_ctrl,
                                 const double* pos_ctrl, const double* knots, const double* t_now, int* status, int* safe,
                                 double* distance, int* n_samples, int* hit_index, double* hit_t, double* hit_pos,
                                 int* end_reason, double* duration);
/* The device chain optimised batch -> safety check: one problem per candidate of `b` (dim 3), read from the variables
 * the batch's last fuelmi_bspline_dev_optimize[_timed] left in device memory (control points = those variables, knot
 * span = x[nvar-1] under MINTIME and the batch's knot span otherwise) against the batch's map.  cfg->degree must be the
 * batch's bspline_degree and cfg->max_ctrl is ignored (it is point_num).  t_now [n_traj].  Only the results are copied
 * back; they equal, bit for bit, fuelmi_map_check_trajs on the x_out that solve returned.  FUELMI_EINVAL when the batch
 * is not dim 3 or has not been optimised since it was created or last (re)loaded (the flag fuelmi_bspline_dev_plan_yaws
 * uses).  Runs on the map's stream and waits for it.
 * While the batch's knot source is FUELMI_KNOTS_ADJUSTED (fuelmi_bspline_dev_set_knot_source, below) the splines stand on
 * the knots the batch's last fuelmi_bspline_dev_adjust_trajs left on the device, and the results equal, bit for bit,
 * fuelmi_map_check_trajs_knots on that solve's x_out and that adjustment's knots_out.  The host never sees those knots,
 * so the kernel checks them (finite, strictly increasing): a candidate that fails -- one the adjustment marked
 * FUELMI_TRAJADJ_BADSPLINE, whose knots are 0 -- is FUELMI_TRAJCHK_NONFINITE / _END_NONFINITE with duration and
 * n_samples 0, like a bad knot span. */
int fuelmi_bspline_dev_check_trajs(fuelmi_bspline_dev* b, const fuelmi_trajchk_cfg* cfg, const double* t_now, int* status,
                                   int* safe, double* distance, int* n_samples, int* hit_index, double* hit_t,
                                   double* hit_pos, int* end_reason, double* duration);
/* what the kernel needs for cfg->max_ctrl (host only, no device needed): out3 = {lanes per problem, dynamic LDS bytes of
 * a workgroup, largest max_ctrl accepted}.  cfg is checked like above. */
int fuelmi_traj_check_plan(const fuelmi_trajchk_cfg* cfg, int out3[3]);

/* ------------------------------------------------------------------------------------------
 * Sampling of flown trajectories: what the reference does with a finished trajectory, for n_prob independent problems
 * (a UNIFORM position spline, an optional UNIFORM 1-D yaw spline, n_t sample times) in one call.  Two modes:
 *   FUELMI_TRAJSMP_COMMAND  traj_server's cmdCallback (plan_manage/src/traj_server.cpp:257-343), which runs at 100 Hz:
 *                           position, velocity, acceleration, jerk, yaw, yaw rate, and the flight record (:328-339).
 *   FUELMI_TRAJSMP_STATE    the FSM's replan start state (exploration_manager/src/fast_exploration_fsm.cpp:86-95):
 *                           position, velocity, acceleration, yaw, yaw rate, yaw acceleration at t_r.
 * Both modes write all seven quantities (jerk is an addition to the second, yaw acceleration to the first).  Everything
 * f64, the reference's operations in the reference's order:
 *   1. knots as setUniformBspline builds them (bspline/src/non_uniform_bspline.cpp:25-31): u[i] = double(i - p) * dt
 *      for i <= p, then ACCUMULATED u[i] = u[i-1] + dt; duration D = u[n_ctrl] - u[p].  The yaw spline likewise from
 *      yaw_dt and its own degree (planYawExplore sets 3, planYaw the position degree).
 *   2. derivative splines as getDerivative builds them (:77-106), applied repeatedly (velocity, acceleration, jerk; yaw
 *      rate, yaw acceleration): control points Q[i] = double(p) * (P[i+1] - P[i]) / (u[i+p+1] - u[i+1]), knots the
 *      PARENT's u[1 .. m-1] (the accumulated values, not regenerated ones), degree p - 1.  A cubic's jerk spline has
 *      degree 0: evaluateDeBoor then is the knot search `while (u[k+1] < ub) ++k` from k = 0 and returns row k, with
 *      the strict < at a knot.
 *   3. every evaluation is the literal evaluateDeBoorT (:51-75): clamp to [u_(p_), u_(m_ - p_)], knot search, alpha
 *      recursion.
 *   COMMAND (:266-290): T = t_stop ? min(t_stop[b], D) : D (what replanCallback :166-172 leaves in traj_duration_).
 *      t < T && t >= 0: FUELMI_TRAJSMP_IN, everything at t.  Else t >= T: FUELMI_TRAJSMP_PAST, pos = S(T), yaw = Y(T),
 *      everything else 0.  Else FUELMI_TRAJSMP_INVALID.  The tests are made in this order, the reference's, so with a
 *      t_stop below 0 a time in [T, 0) is PAST.
 *   STATE: everything is evaluateDeBoorT(t) with its own clamp, for any finite t; the status is always IN.
 *   Flight record (COMMAND, optional, in and out): flight [n_prob][8] = have_last, last_pos[3], last_t, length, energy,
 *      n_cmd.  The samples are taken in order (:328-339, calcPathLength :49-56): have_last == 0: push pos (last_pos =
 *      pos, have_last = 1, n_cmd = 1).  Else if sqrt(dx dx + dy dy + dz dz) of pos - THE LAST PUSHED POSITION is
 *      > 1e-6: push, length += that norm, energy += (jx jx + jy jy + jz jz) * (t[k] - last_t), n_cmd += 1; the sums run
 *      left to right.  last_t = t[k] after every sample.  Carrying flight from call to call continues a flight across
 *      tapes and replans; a record of zeros starts one.
 * Defined where the reference is not:
 *   PAST     jerk = 0 (the reference leaves jer uninitialised; with a position that moved it enters the energy).
 *   INVALID  every output 0 (the reference prints "invalid time" and publishes uninitialised values); of the record only
 *            last_t is touched.
 *   no yaw spline (n_yaw_ctrl NULL, or n_yaw_ctrl[b] == 0): the three yaw outputs are 0.
 *   FUELMI_TRAJSMP_BADSPLINE (device batches only, the host route refuses it): a knot span that is not finite and > 0.
 *            The spline is never indexed: every sample of the problem has this status, every output is 0, duration 0,
 *            the record untouched.
 *   Entries from n_t[b] to max_t are written as 0 (status too).
 * Out of scope: loop correction (:292-300), the FOV markers and all publishing, and given knots for yaw splines
 * (Bspline.msg carries only yaw_dt).  Sampling a position spline on knots moved by a time reallocation (moving and
 * measuring them is fuelmi_map_adjust_trajs, below) is fuelmi_map_sample_trajs_knots, below.
 * Checked on the host before anything is launched (FUELMI_EINVAL): pointers; mode; degree in 3..5 and, with max_yaw_ctrl
 * > 0, yaw_degree in 3..5; degree + 1 <= n_ctrl[b] <= max_ctrl; n_yaw_ctrl[b] == 0 or yaw_degree + 1 <= n_yaw_ctrl[b] <=
 * max_yaw_ctrl; spans finite and > 0; control points finite with |value| < 1e7; 0 <= n_t[b] <= max_t; every t, t_stop and
 * flight value finite; t_stop or flight in STATE mode.  FUELMI_ELIMIT: max_ctrl or max_yaw_ctrl >
 * FUELMI_TRAJSMP_MAX_CTRL; max_t > FUELMI_TRAJSMP_MAX_T; n_prob * max_t > FUELMI_TRAJSMP_MAX_SAMPLES (the results of a
 * call, 124 bytes per sample, then stay below 260 MiB of device scratch).  n_prob = 0 or every n_t = 0 is FUELMI_OK:
 * nothing is launched and nothing is written.
 * fuelmi_map_sample_trajs takes host arrays in and out, is synchronous, runs on the map's stream, one thread at a time
 * per map (not a query-slot call); its scratch is one grow-only allocation on the map.  It reads no plane and no
 * mirror.  One 64-lane wave per problem, one sample per lane and window of 64; the record is walked in sample order by
 * every lane alike, so its sums are the reference's term by term.  A result does not depend on the problem's place in
 * the batch.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_TRAJSMP_COMMAND 0
#define FUELMI_TRAJSMP_STATE 1
#define FUELMI_TRAJSMP_IN 0
#define FUELMI_TRAJSMP_PAST 1
#define FUELMI_TRAJSMP_INVALID 2
#define FUELMI_TRAJSMP_BADSPLINE 3
#define FUELMI_TRAJSMP_MAX_CTRL 1024          /* largest max_ctrl and max_yaw_ctrl */
#define FUELMI_TRAJSMP_MAX_T 65536            /* largest max_t: sample times per problem and call */
#define FUELMI_TRAJSMP_MAX_SAMPLES 2097152    /* largest n_prob * max_t per call (2^21) */
typedef struct {
  int mode;            /* FUELMI_TRAJSMP_COMMAND or FUELMI_TRAJSMP_STATE */
  int degree;          /* degree of the position spline, 3..5 */
  int yaw_degree;      /* degree of the yaw spline, 3..5; not read with max_yaw_ctrl == 0 */
  int max_ctrl;        /* stride of pos_ctrl */
  int max_yaw_ctrl;    /* stride of yaw_ctrl; 0: no problem has a yaw spline */
  int max_t;           /* stride of t and of every per-sample output */
} fuelmi_trajsmp_cfg;
/* pos_ctrl [n_prob][max_ctrl][3], n_ctrl / knot_span [n_prob]; n_yaw_ctrl / yaw_dt [n_prob] and yaw_ctrl
 * [n_prob][max_yaw_ctrl], or n_yaw_ctrl NULL; t_stop [n_prob] or NULL; n_t [n_prob], t [n_prob][max_t].  Out, per
 * sample: status [n_prob][max_t]; pos, vel, acc, jerk [n_prob][max_t][3]; yaw, yawdot, yawddot [n_prob][max_t].  Per
 * problem: duration [n_prob]; flight [n_prob][8] in and out, or NULL. */
int fuelmi_map_sample_trajs(fuelmi_map* m, const fuelmi_trajsmp_cfg* cfg, int n_prob, const int* n_ctrl,
                            const double* pos_ctrl, const double* knot_span, const int* n_yaw_ctrl,
                            const double* yaw_ctrl, const double* yaw_dt, const double* t_stop, const int* n_t,
                            const double* t, int* status, double* pos, double* vel, double* acc, double* jerk,
                            double* yaw, double* yawdot, double* yawddot, double* duration, double* flight);
/* The same with the position splines on whole knot vectors in place of the spans -- what traj_server does with the knots
 * of Bspline.msg, pos_traj.setKnot(knots) (plan_manage/src/traj_server.cpp:230), before it samples commands: knots
 * [n_prob][max_ctrl + degree + 1], the layout of fuelmi_map_adjust_trajs' knots_out, so that call's output is this
 * call's input as it stands.  Step 1 then takes problem b's n_ctrl[b] + degree + 1 position knots as given; D stays
 * u[n_ctrl] - u[p], the derivative points of step 2 are divided by the given knots' differences, step 3 is unchanged (t +
 * u[p], the clamp, the strict < of the search).  The yaw splines stay uniform.  Checked on the host before anything is
 * launched (FUELMI_EINVAL), beside everything above but the position spans: knots not NULL, every knot finite, every
 * knot above the one in front of it.  Strict increase is more than the reference asks for: it asks for nothing and
 * divides by knot differences. */
int fuelmi_map_sample_trajs_knots(fuelmi_map* m, const fuelmi_trajsmp_cfg* cfg, int n_prob, const int* n_ctrl,
                                  const double* pos_ctrl, const double* knots, const int* n_yaw_ctrl,
                                  const double* yaw_ctrl, const double* yaw_dt, const double* t_stop, const int* n_t,
                                  const double* t, int* status, double* pos, double* vel, double* acc, double* jerk,
                                  double* yaw, double* yawdot, double* yawddot, double* duration, double* flight);
/* The device chain optimised batch -> commands / next start states: one problem per candidate of `b` (dim 3), the
 * position spline read from the variables the batch's last fuelmi_bspline_dev_optimize[_timed] left in device memory
 * (control points = those variables, knot span = x[nvar-1] under MINTIME and the batch's knot span otherwise).
 * cfg->degree must be the batch's bspline_degree and cfg->max_ctrl is ignored (it is point_num).  The yaw splines and
 * the times come from the host; only the results are copied back.  They equal, bit for bit, fuelmi_map_sample_trajs on
 * the x_out that solve returned.  FUELMI_EINVAL when the batch is not dim 3 or has not been optimised since it was
 * created or last (re)loaded (the preconditions of fuelmi_bspline_dev_check_trajs).  Runs on the map's stream and waits
 * for it.
 * While the batch's knot source is FUELMI_KNOTS_ADJUSTED (fuelmi_bspline_dev_set_knot_source, below) the position
 * splines stand on the knots the batch's last fuelmi_bspline_dev_adjust_trajs left on the device, and the results equal,
 * bit for bit, fuelmi_map_sample_trajs_knots on that solve's x_out and that adjustment's knots_out.  The host never sees
 * those knots, so the kernel checks them (finite, strictly increasing): a candidate that fails -- one the adjustment
 * marked FUELMI_TRAJADJ_BADSPLINE, whose knots are 0 -- is FUELMI_TRAJSMP_BADSPLINE on every sample. */
int fuelmi_bspline_dev_sample_trajs(fuelmi_bspline_dev* b, const fuelmi_trajsmp_cfg* cfg, const int* n_yaw_ctrl,
                                    const double* yaw_ctrl, const double* yaw_dt, const double* t_stop, const int* n_t,
                                    const double* t, int* status, double* pos, double* vel, double* acc, double* jerk,
                                    double* yaw, double* yawdot, double* yawddot, double* duration, double* flight);
/* what the kernel needs for cfg (host only, no device needed): out3 = {lanes per problem, dynamic LDS bytes of a
 * workgroup, largest max_ctrl accepted}.  cfg is checked like above. */
int fuelmi_traj_sample_plan(const fuelmi_trajsmp_cfg* cfg, int out3[3]);

/* ------------------------------------------------------------------------------------------
 * Time adjustment and metrics of B-spline trajectories: the half of the reference's NonUniformBspline
 * (bspline/src/non_uniform_bspline.cpp) that moves knots and measures a spline, for n_prob independent position splines
 * (degree 3..5, dimension 3) in one call.  Everything f64, the reference's operations in the reference's order; the
 * stages run in this order:
 *   a. Knots.  knots_in NULL: as setUniformBspline builds them (:25-31) from knot_span[b]: u[i] = double(i - p) * dt for
 *      i <= p, then ACCUMULATED u[i] = u[i-1] + dt.  Else the caller's n_ctrl[b] + p + 1 knots as given (setKnot), so a
 *      second call continues from the first call's knots_out.
 *   b. Always, on the input knots: DURATION_IN = u[n_ctrl] - u[p] (getTimeSum :267); RATIO = checkRatio() (:135-160,
 *      without the logging); FEASIBLE_IN = checkFeasibility() (:443-487; strict > against limit + 1e-4 per axis).
 *   c. FUELMI_TRAJADJ_LENGTHEN: lengthenTime(r) (:162-176), r = min(cfg.lengthen_cap, ratio_in ? ratio_in[b] : RATIO)
 *      (the cap is 1.01 in both reference callers).  num1 = 2p - 1 >= num2 = n_ctrl - p + 1: the knots stay untouched.
 *   d. FUELMI_TRAJADJ_REALLOC: the loop of plan_manage/src/planner_manager.cpp:222-230 on the current knots:
 *        feasible = checkFeasibility(); while (!feasible) { feasible = reallocateTime(); if (++iter >= realloc_iters) break; }
 *      reallocateTime is :346-441 literally: the velocity pass over i, then the acceleration pass; every infeasible i
 *      moves knots that the test of the next i reads; ratio = max / limit + 1e-4, resp. sqrt(max_acc / limit_acc) + 1e-4,
 *      capped at limit_ratio; t_inc = delta_t / double(p), resp. double(p - 1); the acceleration pass's branch for
 *      i == 1 || i == 2 (:416-424) moves u(2..5) and adds 4.0 * t_inc to every knot from 6 on.  Every knot receives its
 *      additions one at a time in the order of i.  ITERS and FEASIBLE are what the loop left; without REALLOC they are 0
 *      and checkFeasibility() of the current knots.  FEASIBLE_OUT = checkFeasibility() on the final knots (an addition).
 *   e. Metrics on the final knots, always: DURATION_OUT; LENGTH = getLength(length_res) (:271-281: the accumulated
 *      t += res while t <= dur + 1e-4, norms summed left to right); JERK = getJerk() (:283-298: three getDerivative, then
 *      jerk += (times(i+1) - times(i)) * c * c over rows, then axes); MEAN_VEL / MAX_VEL / NUM_VEL and MEAN_ACC /
 *      MAX_ACC / NUM_ACC = getMeanAndMaxVel / Acc (:300-344) with the step cfg.stat_step (0.01 in the reference): the
 *      accumulated t from u_(p_) while t <= u_(m_ - p_) of the derivative spline, evaluateDeBoor(t) with the ABSOLUTE
 *      parameter, and the sample counts the reference divides by.
 *   f. FUELMI_TRAJADJ_RESAMPLE: the sampling half of reparamBspline (planner_manager.cpp:533-543): seg_num = n_ctrl - p,
 *      DT_OUT = DURATION_OUT / double(seg_num), TIME_INC = DURATION_OUT - DURATION_IN (both always written), points
 *      evaluateDeBoorT(time) for the accumulated time += DT_OUT from 0 while time <= DURATION_OUT + 1e-4: N_SAMPLES and
 *      samples -- what fuelmi_bspline_parameterize / fuelmi_bspline_dev_load_samples take next, with DT_OUT as ts.
 *   g. FUELMI_TRAJADJ_SELECT (selectBestTraj, planner_manager.cpp:476-482): best[g] = the index of the smallest JERK
 *      among the problems with group[b] == g and status OK.  std::sort leaves ties open; here the smallest index wins.
 *      A JERK that is not a number is never chosen; -1: the group has no candidate.  On the device, after the metrics.
 * Defined where the reference is not: a status per problem.
 *   FUELMI_TRAJADJ_BADSPLINE (device batches only, the host route refuses it): a knot span that is not finite and > 0.
 *            Nothing is indexed: every other output of the problem is 0, knots_out and samples too.
 *   FUELMI_TRAJADJ_LONG      one of the loops of e and f would take more than FUELMI_TRAJADJ_MAX_STEPS steps (or the
 *            resampling more than max_samples): the adjusted knots, the durations, RATIO, the feasibility flags, ITERS,
 *            JERK, DT_OUT and TIME_INC are returned, LENGTH, the mean / max / num values, N_SAMPLES and samples are 0.
 *   Knots from n_ctrl[b] + p + 1 to the stride and samples from N_SAMPLES to max_samples are written as 0.  No loop on the
 *   device is unbounded.
 * Checked on the host before anything is launched (FUELMI_EINVAL): pointers; ops a mask of the four; degree in 3..5;
 * degree + 1 <= n_ctrl[b] <= max_ctrl; spans finite and > 0; control points finite with |value| < 1e7; knots_in finite
 * and strictly increasing; ratio_in finite; limit_vel, limit_acc finite and > 0; limit_ratio finite and > 1;
 * lengthen_cap finite and >= 1; realloc_iters in 1..16; length_res, stat_step finite and > 0; with SELECT n_group >= 1,
 * group and best given and every group[b] in 0..n_group-1; with RESAMPLE samples given and max_samples >=
 * max_ctrl - degree + 2.  FUELMI_ELIMIT: max_ctrl > FUELMI_TRAJADJ_MAX_CTRL, max_samples > FUELMI_TRAJADJ_MAX_SAMPLES,
 * n_prob or n_group > FUELMI_TRAJADJ_MAX_PROB.  n_prob == 0 is FUELMI_OK: nothing is launched, nothing is written.
 * The moved knots go on: knots_out is, as it stands, the `knots` of fuelmi_map_check_trajs_knots, _sample_trajs_knots
 * and _plan_yaws_knots (above), and a device batch keeps them for its own three calls (FUELMI_KNOTS_ADJUSTED, below).
 * Out of scope: given knots into fuelmi_map_collision_ranges, fuelmi_map_local_segments and the kinodynamic loader
 * (those take uniform splines), and given knots for yaw splines; a device-to-device hand-over of the resampled points to load_samples; yaw (1-D)
 * splines; the reference's ROS_INFO output; the commented-out VIEWCONS path of refineTraj.
 * fuelmi_map_adjust_trajs takes host arrays in and out, is synchronous, runs on the map's stream, one thread at a time
 * per map; its scratch is one grow-only allocation on the map.  It reads no plane and no mirror.  One 64-lane wave per
 * problem, knots and control points in LDS; the serial passes are walked by every lane alike, the lanes own the knots; the
 * sums are taken in sample order.  A result does not depend on the problem's place in the batch.
 * ---------------------------------------------------------------------------------------- */
#define FUELMI_TRAJADJ_LENGTHEN 1
#define FUELMI_TRAJADJ_REALLOC 2
#define FUELMI_TRAJADJ_RESAMPLE 4
#define FUELMI_TRAJADJ_SELECT 8
#define FUELMI_TRAJADJ_OK 0
#define FUELMI_TRAJADJ_BADSPLINE 1
#define FUELMI_TRAJADJ_LONG 2
#define FUELMI_TRAJADJ_MAX_CTRL 1024      /* largest max_ctrl */
#define FUELMI_TRAJADJ_MAX_SAMPLES 4096   /* largest max_samples */
#define FUELMI_TRAJADJ_MAX_PROB 65536     /* largest n_prob and n_group */
#define FUELMI_TRAJADJ_MAX_STEPS 65536    /* steps of one metric or resample loop */
/* info [n_prob][FUELMI_TRAJADJ_NI] */
#define FUELMI_TRAJADJ_NI 8
#define FUELMI_TRAJADJ_I_STATUS 0
#define FUELMI_TRAJADJ_I_FEASIBLE_IN 1
#define FUELMI_TRAJADJ_I_ITERS 2
#define FUELMI_TRAJADJ_I_FEASIBLE 3
#define FUELMI_TRAJADJ_I_FEASIBLE_OUT 4
#define FUELMI_TRAJADJ_I_NUM_VEL 5
#define FUELMI_TRAJADJ_I_NUM_ACC 6
#define FUELMI_TRAJADJ_I_N_SAMPLES 7
/* metrics [n_prob][FUELMI_TRAJADJ_NM]; the last entry is 0 */
#define FUELMI_TRAJADJ_NM 12
#define FUELMI_TRAJADJ_M_DURATION_IN 0
#define FUELMI_TRAJADJ_M_RATIO 1
#define FUELMI_TRAJADJ_M_DURATION_OUT 2
#define FUELMI_TRAJADJ_M_LENGTH 3
#define FUELMI_TRAJADJ_M_JERK 4
#define FUELMI_TRAJADJ_M_MEAN_VEL 5
#define FUELMI_TRAJADJ_M_MAX_VEL 6
#define FUELMI_TRAJADJ_M_MEAN_ACC 7
#define FUELMI_TRAJADJ_M_MAX_ACC 8
#define FUELMI_TRAJADJ_M_DT_OUT 9
#define FUELMI_TRAJADJ_M_TIME_INC 10
typedef struct {
  int ops;              /* FUELMI_TRAJADJ_LENGTHEN | _REALLOC | _RESAMPLE | _SELECT, or 0: measure only */
  int degree;           /* 3..5 */
  int max_ctrl;         /* stride of pos_ctrl; knots_in / knots_out have the stride max_ctrl + degree + 1 */
  int max_samples;      /* stride of samples (RESAMPLE) */
  int realloc_iters;    /* 1..16; the reference: 3 */
  int n_group;          /* groups of SELECT */
  double limit_vel, limit_acc, limit_ratio;  /* setPhysicalLimits; the reference's limit_ratio is 1.1 */
  double lengthen_cap;  /* the reference: 1.01 */
  double length_res;    /* getLength's res */
  double stat_step;     /* the step of getMeanAndMaxVel / Acc; the reference: 0.01 */
} fuelmi_trajadj_cfg;
/* In: n_ctrl [n_prob]; pos_ctrl [n_prob][max_ctrl][3]; knot_span [n_prob] (not read with knots_in) or knots_in
 * [n_prob][max_ctrl + degree + 1]; ratio_in [n_prob] or NULL; group [n_prob] (SELECT).  Out: info
 * [n_prob][FUELMI_TRAJADJ_NI]; metrics [n_prob][FUELMI_TRAJADJ_NM]; knots_out [n_prob][max_ctrl + degree + 1]; samples
 * [n_prob][max_samples][3] (RESAMPLE, else NULL); best [n_group] (SELECT, else NULL). */
int fuelmi_map_adjust_trajs(fuelmi_map* m, const fuelmi_trajadj_cfg* cfg, int n_prob, const int* n_ctrl,
                            const double* pos_ctrl, const double* knot_span, const double* knots_in,
                            const double* ratio_in, const int* group, int* info, double* metrics, double* knots_out,
                            double* samples, int* best);
/* The device chain optimised batch -> adjusted, measured and ranked candidates: one problem per candidate of `b` (dim
 * 3), the control points read from the variables the batch's last fuelmi_bspline_dev_optimize[_timed] left in device
 * memory, the knot span x[nvar-1] under MINTIME and the batch's knot span otherwise (knots_in, a host array, replaces
 * the span).  cfg->degree must be the batch's bspline_degree and cfg->max_ctrl is ignored (it is point_num).  Only the
 * results are copied back; they equal, bit for bit, fuelmi_map_adjust_trajs on the x_out that solve returned.
 * FUELMI_EINVAL when the batch is not dim 3 or has not been optimised since it was created or last (re)loaded (the
 * preconditions of fuelmi_bspline_dev_check_trajs).  Runs on the map's stream and waits for it.
 * The call also keeps every candidate's final knots [n_traj][point_num + degree + 1] in a buffer the batch owns
 * (allocated by the first call, freed with the batch): what FUELMI_KNOTS_ADJUSTED reads. */
int fuelmi_bspline_dev_adjust_trajs(fuelmi_bspline_dev* b, const fuelmi_trajadj_cfg* cfg, const double* knots_in,
                                    const double* ratio_in, const int* group, int* info, double* metrics,
                                    double* knots_out, double* samples, int* best);
/* Which knots fuelmi_bspline_dev_check_trajs, _sample_trajs and _plan_yaws put under the batch's position splines:
 *   FUELMI_KNOTS_UNIFORM   (the default) setUniformBspline's, from the knot span
 *   FUELMI_KNOTS_ADJUSTED  the knots the last fuelmi_bspline_dev_adjust_trajs kept: the device chain solve -> adjustment
 *                          -> safety check / commands / yaw, the knots never leaving the device
 * FUELMI_KNOTS_ADJUSTED is FUELMI_EINVAL unless an adjustment has run since the batch's last solve.  Whatever ends that
 * solve -- a reload (fuelmi_bspline_dev_load_*), fuelmi_bspline_dev_solve_quadratic's hand-over, the next
 * fuelmi_bspline_dev_optimize[_timed] -- drops the kept knots and puts the source back to FUELMI_KNOTS_UNIFORM.  No
 * other call reads the source (fuelmi_bspline_dev_adjust_trajs itself starts from the span or its knots_in).  Host only:
 * nothing is launched.  _knot_source of NULL is FUELMI_KNOTS_UNIFORM. */
#define FUELMI_KNOTS_UNIFORM 0
#define FUELMI_KNOTS_ADJUSTED 1
int fuelmi_bspline_dev_set_knot_source(fuelmi_bspline_dev* b, int source);
int fuelmi_bspline_dev_knot_source(const fuelmi_bspline_dev* b);
/* what the kernel needs for cfg (host only, no device needed): out3 = {lanes per problem, dynamic LDS bytes of a
 * workgroup, largest max_ctrl accepted}.  cfg is checked like above. */
int fuelmi_traj_adjust_plan(const fuelmi_trajadj_cfg* cfg, int out3[3]);

/* ------------------------------------------------------------------------------------------
 * Map clouds and the known-volume count: the scans of MapROS::publishMapLocal, publishMapAll and publishUnknown
 * (plan_env/src/map_ros.cpp:217-346) as an ordered stream compaction over the state planes the device holds.  No host
 * mirror is read or needed.
 *   Selection   the voxels of the inclusive box lo..hi whose bit is set in the kind's plane:
 *                 FUELMI_CLOUD_OCCUPIED  occ > min_occupancy_log             (publishMapAll :223, publishMapLocal :272)
 *                 FUELMI_CLOUD_UNKNOWN   occ < clamp_min_log - 1e-3          (publishUnknown :328)
 *                 FUELMI_CLOUD_KNOWN     the complement of UNKNOWN           (publishMapAll's second loop :249)
 *                 FUELMI_CLOUD_INFLATED  occupancy_buffer_inflate_ == 1      (the lines commented out at :284-298)
 *   Order       x outermost, then y, then z: ascending voxel address, the order of all three reference loops.
 *   Truncation  a selected voxel is dropped iff pos_z > z_high or pos_z < z_low, pos_z = (z + 0.5) * resolution +
 *               origin_z in f64 (indexToPos and the reference's two `continue`s).  Both comparisons are false for a NaN
 *               bound: NaN and +-inf mean "no bound".  With z_high < z_low nothing is kept.
 *   Points      (float)((i + 0.5) * resolution + origin_i) per axis: the f64 expression without contraction, one
 *               rounding to float, as pcl::PointXYZ is assigned.
 *   Count, cap  *n_total is always the full count.  n_total <= cap: all points are written, FUELMI_OK.  More: the first
 *               `cap` points in order are written, nothing beyond them, FUELMI_ELIMIT.  xyz == NULL with cap == 0 counts
 *               only and returns FUELMI_OK (publishMapAll's known_volumn: KNOWN, no bounds; the count is the pinned
 *               quantity -- the reference adds 0.1 * 0.1 * 0.1 `count` times, count * 0.001 differs in the last bits).
 *   Arguments   checked on the host before anything is launched.  lo > hi on any axis: an empty box, 0 points,
 *               FUELMI_OK (the reference's loops do not run).  Otherwise a box that leaves the map, an unknown kind,
 *               cap < 0, xyz == NULL with cap > 0: FUELMI_EINVAL, and neither xyz nor *n_total is written.  The caller
 *               applies boundIndex, as the reference does.
 * The one deviation: for KNOWN the reference tests occ > clamp_min_log - 1e-3 and the plane gives
 * !(occ < clamp_min_log - 1e-3).  They differ only for a log-odds value exactly on the threshold, or a NaN, which this
 * call counts as known.  Fusion produces neither; only fuelmi_map_upload_occupancy can.
 * A mutator-class call: it runs on the map's stream behind every fusion, upload, reset and inflation queued before it,
 * host arrays out, synchronous, one thread at a time per map.  Its scratch is one grow-only allocation on the map
 * (workgroup words + min(cap, voxels of the box) points); nothing is allocated after the first call of a given size.
 * ---------------------------------------------------------------------------------------- */
enum { FUELMI_CLOUD_OCCUPIED = 0, FUELMI_CLOUD_UNKNOWN = 1, FUELMI_CLOUD_KNOWN = 2, FUELMI_CLOUD_INFLATED = 3 };
typedef struct {
  int kind;
  int lo[3], hi[3];      /* inclusive voxel box */
  double z_low, z_high;  /* visualization_truncate_low_ / _height_ */
} fuelmi_cloud_cfg;
int fuelmi_map_extract_cloud(fuelmi_map* m, const fuelmi_cloud_cfg* cfg, float* xyz, int cap, int* n_total);
/* the geometry the kernels use for a box of a dims[3] map (host only, no device needed): out = {items per line (64-bit
 * chunks of the z extent), lines, items per workgroup, workgroups, the scan's width, the scan's rounds, scratch bytes
 * in front of the points, voxels of the box}.  An empty box gives 0 items, lines, workgroups, rounds and voxels; a box
 * that leaves the map, dims outside 1 .. (nz: 255), or 2^31 - 64 voxels and more are FUELMI_EINVAL. */
int fuelmi_cloud_plan(const int dims[3], const int lo[3], const int hi[3], int out[8]);
/* device milliseconds of the last fuelmi_map_extract_cloud: count + scan, write, copy to the caller */
int fuelmi_map_cloud_times(const fuelmi_map* m, double ms3[3]);

/* ------------------------------------------------------------------------------------------
 * Depth renderer: the simulated depth camera pcl_render_node (uav_simulator/local_sensing) for a batch of poses.  A
 * renderer is not tied to a map: it owns a stream, a copy of the world cloud, the frames of max_poses poses and a
 * grow-only scratch (the records of n_pose * n_points); nothing is allocated after the first call of a given size.
 * Per pixel both of the reference's nodes take the minimum depth over the square windows that the points splat; each
 * model restates its node's arithmetic literally, with the usual C++ conversions and without FMA contraction.
 *   FUELMI_RENDER_HOST_NODE  (src/depth_render_node.cpp:112-161, the node built by default).  Per point, in this order:
 *     pw = the point as double; dropped if sqrt(dx^2 + dy^2 + dz^2) > range (f64, summed left to right, d = cam_pos - pw);
 *     pc = R pw + t in f64, each row ((r0 x + r1 y) + r2 z) + t; dropped if pc.z <= 0;
 *     float px = pc.x / pc.z * fx + cx (f64, rounded once), py likewise; dropped if px < 0 || px >= cols || py < 0 ||
 *     py >= rows (compared as float); float dist = pc.z; int r = 0.0573 * fx / dist + 0.5 (f64, truncated);
 *     window x from max(int(px - r), 0) to min(int(px + r), cols - 1) (float arithmetic, truncated toward zero), y
 *     likewise with the same r; the pixel is the smallest dist, an empty pixel 0.0f.
 *   FUELMI_RENDER_CUDA_NODE  (src/depth_render.cu:2-43 and the conversion of src/pcl_render_node.cpp:300-310).  fx, fy,
 *     cx, cy, R, t rounded to float once; the transform in f32, each row ((x r0 + y r1) + z r2) + t; dropped if
 *     z <= 0.0f; int u = x / z * fx + cx + 0.5 (f32 up to the sum, + 0.5 in f64, truncated), v likewise; dropped if u
 *     or v is outside the image; int mm = z * 1000.0f + 0.5f (f32); int r = 0.0573 * fx / z + 0.5f (f64); window
 *     u +- r, v +- r clipped to the image; the pixel is the minimum of mm and 999999, published as
 *     float d = (float)mm / 1000.0f; d = d < 500.0f ? d : 0.  range is ignored.
 *   The raw frame is what MapROS::depthPoseCallback makes of the published image (plan_env/src/map_ros.cpp:132-133,
 *     convertTo(CV_16UC1, k)): saturate_u16(round_half_even(metres * (float)k)), OpenCV's rule for 32F -> 16U.
 * Deviations, each counted in stats[1]:
 *   1. a point that passed the culls with (float)dist < 1e-3f is dropped.  The reference's `value < 1e-3` test makes the
 *      result depend on the cloud's order for such a point, its window covers the whole image and its `int r` conversion
 *      is undefined for a tiny dist.  Without such a point the sequential update equals the order-free minimum with 0 as
 *      "empty": the result does not depend on the schedule or on the cloud's order.
 *   2. a point with a non-finite coordinate is dropped before the culls; so is a point whose camera depth or projection
 *      is NaN, or (CUDA_NODE) whose u, v or mm would leave int before the truncation.  The reference's conversions are
 *      undefined there; every such point is off the image or beyond 500 m.  HOST_NODE: where float(r) rounds px + r up
 *      to 2^31 the window ends at the border.
 *   3. an nvcc build contracts CUDA_NODE's f32 transform into FMAs; this restates the source text without contraction.
 *   4. the summation order of norm() and of the 3 x 3 product is the one stated above (Eigen's own is the stand-in's).
 * fuelmi_render_depth: T_cw [n_pose][12] are the first three rows of world->camera (the node's cam2world.inverse(),
 * computed by the caller), cam_pos [n_pose][3] is cam2world's translation.  Synchronous: when it returns all n_pose
 * frames are complete on the device (fuelmi_render_frame_raw / _metres: device pointers, valid until the next render,
 * set_cloud or destroy of this renderer; frame k of the last call) and copied to the host arrays that were given
 * (metres [n_pose][rows][cols] f32, raw likewise u16; either may be NULL).  A raw frame pointer can go straight into
 * fuelmi_map_input_depth of any map on the same device.  stats [n_pose][4] (may be NULL): points that passed the culls,
 * points dropped as undefined, pixels whose metres value is not 0, 0.
 * Refused before anything is launched: rows or cols < 1, fx or fy not finite or <= 0, cx or cy not finite, an unknown
 * model, range < 0 or NaN (HOST_NODE), max_poses < 1, n_points < 0, n_pose < 1, a non-finite T_cw or cam_pos entry, a
 * render before any set_cloud (an empty cloud is legal: all-zero frames), k_depth_scaling_factor not finite or <= 0, a
 * renderer that is null or was destroyed (FUELMI_EINVAL); rows * cols > 2^24, 57.3 * max(fx, fy) + 1 >= 2^31 (the
 * radius of the closest point kept), max_poses > 4096 or max_poses * rows * cols > 2^28, n_points > 2^27, n_pose >
 * max_poses, n_pose * n_points > 2^28 (FUELMI_ELIMIT).  fuelmi_render_create returns FUELMI_ENODEV without a gfx950
 * device, after the checks of cfg.  One thread per renderer at a time.
 * ---------------------------------------------------------------------------------------- */
enum { FUELMI_RENDER_HOST_NODE = 0, FUELMI_RENDER_CUDA_NODE = 1 };
typedef struct {
  int device, rows, cols;
  double fx, fy, cx, cy;
  int model;     /* which of the reference's two nodes is restated */
  double range;  /* HOST_NODE: the node's 5.0 m cull around the camera; +inf switches it off; ignored by CUDA_NODE */
  int max_poses; /* frames the renderer keeps on the device */
} fuelmi_render_cfg;
typedef struct fuelmi_render fuelmi_render;
int fuelmi_render_create(const fuelmi_render_cfg* cfg, fuelmi_render** out);
int fuelmi_render_destroy(fuelmi_render* r);
/* xyz: n_points * 3 floats in host or device memory; copied */
int fuelmi_render_set_cloud(fuelmi_render* r, const float* xyz, int n_points);
int fuelmi_render_depth(fuelmi_render* r, int n_pose, const double* T_cw, const double* cam_pos,
                        double k_depth_scaling_factor, float* metres, unsigned short* raw, int* stats);
/* NULL (with a message) for a renderer that is not live or k outside 0 .. max_poses - 1 */
const unsigned short* fuelmi_render_frame_raw(const fuelmi_render* r, int k);
const float* fuelmi_render_frame_metres(const fuelmi_render* r, int k);
/* the kernels' geometry for cfg and a cloud of n_points (host only, no device needed): out = {lanes of a small window's
 * segment, the size (larger side of the clipped window, pixels) from which a window is spread over a wave, points of a
 * projection workgroup, projection workgroups per pose, splat workgroups per pose, convert workgroups per pose, scratch
 * bytes of max_poses poses modulo 2^31, the same divided by 2^31}.  cfg and n_points are checked like above. */
int fuelmi_render_plan(const fuelmi_render_cfg* cfg, int n_points, int out[8]);
/* device milliseconds of the last fuelmi_render_depth: cull + project, splat, convert */
int fuelmi_render_times(const fuelmi_render* r, double ms3[3]);

/* ------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py): HIP events recorded on the map's own stream.
 * ---------------------------------------------------------------------------------------- */
enum {
  FUELMI_K_INFLATE = 0,
  FUELMI_K_ESDF_ZY = 1,
  FUELMI_K_ESDF_X = 2,
  FUELMI_K_FRONTIER = 3,
  FUELMI_K_BSPLINE = 4,
  FUELMI_K_INSERT = 5,
  FUELMI_K_COUNT = 6
};
int fuelmi_timer_begin(fuelmi_map* m);
int fuelmi_timer_end(fuelmi_map* m, float* elapsed_ms); /* synchronises the stream */
/* bracket every launch of the stages selected by stage_mask (bit k = FUELMI_K_*) with events */
int fuelmi_profile_enable(fuelmi_map* m, unsigned stage_mask);
/* synchronises, then returns launches and summed device milliseconds of a stage since enable */
int fuelmi_profile_get(fuelmi_map* m, int stage, int* launches, double* total_ms);
/* the same brackets one by one (up to cap values, milliseconds; *n = how many were written): lets the
 * caller take a median, a single disturbed launch otherwise dominates a short sample */
int fuelmi_profile_get_samples(fuelmi_map* m, int stage, double* ms, int cap, int* n);
/* begin / end of every bracket of a stage, milliseconds after the fuelmi_profile_enable call that armed the stage: the
 * device's timeline of a few cycles without a tracer on the host */
int fuelmi_profile_get_timeline(fuelmi_map* m, int stage, double* begin_ms, double* end_ms, int cap, int* n);

#ifdef __cplusplus
}
#endif
#endif /* FUELMI_H_ */
