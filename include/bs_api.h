/*
 * bs_api.h -- C ABI of the MI355X-native buildingSegment hot path
 * (kNN neighbourhood build -> PCA normal estimation -> region-growing plane
 * labelling).  Plain pointers and sizes only; no C++ or torch types.
 *
 * Reference interfaces this boundary replaces (all paths relative to
 * /root/reference/):
 *   tmc3/TMC3.cpp:213-218        the four call-site lines in main()
 *   tmc3/my_function.h:48-85     get_Normal_and_K_neighbor<K>()      -> bs_knn_normals*
 *   tmc3/my_function.h:89-123    class seg_plane (ctor, get_planes)  -> bs_region_grow*
 *   tmc3/my_function.cpp:180-258 seg_plane::get_planes / Broad       -> bs_region_grow*
 *   tmc3/my_function.h:25-30     struct plane                        -> bs_planes (CSR)
 *   tmc3/my_function.cpp:260-275 seg_plane::set_plane_color          -> bs_plane_colors
 *   tmc3/PCCPointSet.h:60,67,605 positions (int32 AoS) / planeIdx    -> xyz / plane_idx buffers
 *
 * Conventions
 *   - xyz is the reference's AoS layout: int32 [n][3] millimetres == &cloud[0].
 *   - neigh is row-major int32 [n][k], nearest first, ties (equal squared
 *     distance) broken by ascending point index, self included.
 *   - normals are f64 [n][3], unit length, oriented to +z.
 *   - plane_idx is int32 [n]: -1 = unlabelled, >=1 = plane id (orphans of
 *     failed seeds carry the id of the next committed plane, exactly as the
 *     reference leaves them).
 *   - every function returns BS_OK (0) or a negative bs_status; nothing aborts.
 *   - *_dev entry points take DEVICE pointers, enqueue on the context's
 *     stream and do not synchronise unless stated.
 *   - a bs_ctx is owned by one host thread at a time.
 */
#ifndef BS_API_H
#define BS_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BS_API_VERSION 5

typedef enum bs_status {
  BS_OK = 0,
  BS_ERR_INVALID = -1,     /* null pointer, n < k, k out of range, bad params */
  BS_ERR_RANGE = -2,       /* coordinates outside the exactly-representable domain */
  BS_ERR_NOMEM = -3,       /* host or device allocation failed */
  BS_ERR_HIP = -4,         /* HIP runtime error (see bs_last_error) */
  BS_ERR_NO_DEVICE = -5,   /* no usable gfx950 device */
  BS_ERR_INTERNAL = -6,    /* invariant violated (watchdog, overflow of a work list) */
  BS_ERR_UNCERTIFIED = -7  /* halo too thin: some queries could not be certified */
} bs_status;

/* Parameters.  Defaults are the reference's literals:
 *   k 15 (TMC3.cpp:215-216), radius 100 / max_nn 50 (my_function.h:63),
 *   th_thickness 300, th_point_count 400 (my_function.h:117-118),
 *   cos_th 0.88 (my_function.cpp:230). */
typedef struct bs_params {
  int32_t k;              /* neighbour-list length, 2..32 */
  int32_t max_nn;         /* hybrid search cap for normals, 3..64 */
  double radius;          /* hybrid search radius (mm), strict d^2 < radius^2 */
  int32_t th_thickness;   /* region grow: |distance to plane| <= th_thickness */
  int32_t th_point_count; /* keep a plane iff pointIdx.size() > th_point_count */
  double cos_th;          /* region grow: cur_normal . normal[id] >= cos_th */
  int32_t cell_size;      /* search-grid cell edge in mm, 0 = choose automatically */
  int32_t rg_mode;        /* 0 = auto, 1 = single-wave sequential, 2 = multi-plane speculative */
} bs_params;

/* CSR form of std::vector<plane> (my_function.h:25-30), in the reference's
 * commit order.  point_idx keeps the reference's list order and duplicates
 * (the seed can appear twice).  Arrays are owned by the library after a
 * successful call and released by bs_planes_free. */
typedef struct bs_planes {
  int32_t n_planes;
  int32_t* id;        /* [n_planes]   plane::id (1-based)            */
  double* normal;     /* [n_planes*3] plane::normal                  */
  int32_t* center;    /* [n_planes*3] plane::center                  */
  int64_t* offset;    /* [n_planes+1] CSR offsets into point_idx     */
  int32_t* point_idx; /* [offset[n_planes]] plane::pointIdx, in order */
} bs_planes;

/* Per-call stage timings (milliseconds of device time, HIP events on the
 * context's stream) of the last *_dev / host call. */
typedef struct bs_timings {
  double grid_ms;    /* cell keys + sort + cell table                */
  double knn_ms;     /* kNN + normals kernels (incl. fallback rings) */
  double grow_ms;    /* region growing                               */
  double total_ms;   /* first kernel to last kernel                  */
  int64_t largest_plane;  /* pointIdx.size() of the largest committed plane */
  int64_t n_seed_attempts;
  int64_t n_fallback_queries; /* queries that left the LDS-tile fast path */
  int64_t rg_rounds;      /* speculative rounds (rg_mode 2) */
  double grow_kernel_ms;  /* sum of the plane-growth kernel launches alone (HIP events around each launch) */
  int64_t grow_kernel_launches;
  double grow_setup_ms;   /* region growing, one-time part: records, static masks, reverse lists, first owner fixed point */
  int64_t validation_rejects; /* finished planes (or duplicated list entries) the post-round validation refused;
                                 refused planes are grown again, the result stays exact */
  int64_t forged_seed;        /* seed of the plane bs_selftest_forge_next corrupted, -1 if none */
  int64_t forged_refused;     /* 1 if the validation refused exactly that plane */
  int64_t audit_attempts;     /* bs_set_audit: plane attempts replayed against the final owners (-1: audit off) */
  int64_t audit_mismatches;   /* ... of which differ from what was committed (must be 0) */
  double audit_ms;            /* time of the replay + comparison (not part of grow_ms / total_ms) */
  /* -- API version 5 -- */
  int64_t tie_rows;           /* queries of the last kNN call whose k-list has an equal-d^2 pair inside it or at its
                                 boundary (k-th vs (k+1)-th neighbour): the only rows where the reference's kd-tree
                                 traversal order may differ from this library's canonical (d^2, index) order */
  /* why the post-round validation refused finished planes (every refused plane is grown again; the result stays
   * exact).  validate1: the plane was robbed after it finished / a list entry no longer carries its claim / a point
   * is listed twice; validate3: normal or centre not reproducible from the list. */
  int64_t rej_v1_robbed, rej_v1_tag, rej_v1_dup, rej_v3_state;
  /* finished planes that were merely INCONSISTENT with the settled owners (normal outcome of the speculation, not
   * a refusal): seed row no longer free / an accepted point was taken earlier / a logged assumption failed */
  int64_t incons_seed, incons_list, incons_log;
} bs_timings;

/* sizeof(bs_timings) of the library build: a host compiled against another header version must not call
 * bs_get_timings (the struct is written whole).  host/bs_legacy.hpp and the Python loader check it. */
int64_t bs_sizeof_timings(void);

typedef struct bs_ctx bs_ctx;

int bs_api_version(void);
const char* bs_strerror(int status);
void bs_params_default(bs_params* p);

/* Context: binds one HIP device; owns the stream and all scratch buffers. */
int bs_create(int device, bs_ctx** out);
void bs_destroy(bs_ctx* ctx);
const char* bs_last_error(const bs_ctx* ctx);
/* Use an existing hipStream_t (e.g. the caller's current stream); NULL
 * restores the context's own stream. */
int bs_set_stream(bs_ctx* ctx, void* hip_stream);
int bs_get_timings(const bs_ctx* ctx, bs_timings* out);

/* ---- host-buffer entry points (what the reference's call sites bind) ---- */

/* Replaces get_Normal_and_K_neighbor<K>() (my_function.h:48-85). */
int bs_knn_normals(bs_ctx* ctx, const int32_t* xyz, int64_t n, const bs_params* p,
                   int32_t* neigh /* [n][k] out */, double* normals /* [n][3] out */);

/* Replaces seg_plane::seg_plane + get_planes (my_function.h:98-104,
 * my_function.cpp:180-258). */
int bs_region_grow(bs_ctx* ctx, const int32_t* xyz, const double* normals,
                   const int32_t* neigh, int64_t n, const bs_params* p,
                   int32_t* plane_idx /* [n] out */, bs_planes* planes /* out, may be NULL */);

/* Whole path, device-resident between the stages (TMC3.cpp:213-217). */
int bs_segment(bs_ctx* ctx, const int32_t* xyz, int64_t n, const bs_params* p,
               int32_t* neigh /* may be NULL */, double* normals /* may be NULL */,
               int32_t* plane_idx, bs_planes* planes /* may be NULL */);

/* Halo (multi-GPU slab) form of bs_knn_normals: the first n_query points of a
 * local cloud are the queries, the rest is halo; gidx [n] gives every local
 * point's global index (ties are broken by it and neigh holds global
 * indices).  A k-list is certified iff its k-th distance < cert_radius (the
 * halo width); *n_uncertified counts the failures (results are still written). */
int bs_knn_normals_halo(bs_ctx* ctx, const int32_t* xyz, const int32_t* gidx, int64_t n, int64_t n_query,
                        const bs_params* p, int32_t* neigh /* [n_query][k] */, double* normals /* [n_query][3] */,
                        double cert_radius, int64_t* n_uncertified);

void bs_planes_free(bs_planes* planes);

/* Replaces seg_plane::set_plane_color (my_function.cpp:260-275): colours
 * [n][3] uint16 in the reference's internal G,B,R slot order, all zero, then
 * one colour per plane applied to every pointIdx entry.  plane_rgb is
 * [n_planes][3], the values the caller drew (the reference draws
 * 55 + rand() % 200 three times per plane). */
int bs_plane_colors(const bs_planes* planes, const int32_t* plane_rgb, int64_t n,
                    uint16_t* colors /* [n][3] out */);

/* ---- device-buffer entry points (the measured path) ---- */

/* kNN + normals for the queries [q_begin, q_end) of a device-resident cloud of
 * n points.  d_gidx (nullable) gives the global index of each local point
 * (used for tie-breaking and written into d_neigh); NULL = identity.
 * Outputs are indexed by (query - q_begin).  cert_radius > 0 certifies a
 * k-list only if its k-th distance is < cert_radius (halo mode);
 * *n_uncertified (host, nullable) receives the number of failures after a
 * stream sync. */
int bs_knn_normals_dev(bs_ctx* ctx, const int32_t* d_xyz, const int32_t* d_gidx, int64_t n,
                       int64_t q_begin, int64_t q_end, const bs_params* p,
                       int32_t* d_neigh, double* d_normals, double cert_radius,
                       int64_t* n_uncertified);

/* Region growing on device-resident inputs; d_plane_idx [n] out.  Plane
 * records stay on the device until bs_planes_fetch. Synchronises the stream
 * (the speculative scheduler is host-driven). */
int bs_region_grow_dev(bs_ctx* ctx, const int32_t* d_xyz, const double* d_normals,
                       const int32_t* d_neigh, int64_t n, const bs_params* p,
                       int32_t* d_plane_idx);

/* Fused device-resident pipeline: xyz in HBM -> plane_idx in HBM.
 * d_neigh / d_normals may be NULL (scratch owned by the context is used). */
int bs_segment_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, const bs_params* p,
                   int32_t* d_neigh, double* d_normals, int32_t* d_plane_idx);

/* Pre-/post-processing either side of the path, on the device (SURVEY.md 8f-2,3).
 *
 * bs_shift_to_origin_dev: the buildingSeg constructor's bounding-box shift
 * (TMC3.cpp:55-73): min over the cloud, then xyz -= min IN PLACE; min_out [3]
 * (host, nullable) receives the subtracted minimum.  Synchronises.
 * Contract: the extent max - min of every axis is below 2^31 (the difference is
 * formed in int32; the reference's is undefined beyond that).  The call does not
 * check it; api.shift_tiles_to_origin refuses such a cloud on the host.
 *
 * bs_plane_colors_dev: seg_plane::set_plane_color (my_function.cpp:260-275) for
 * the planes of the last region grow on this context: d_colors [n][3] uint16
 * (G,B,R slots) zeroed, then plane_rgb[p] (host, [n_planes][3]) scattered to
 * every pointIdx entry of plane p. */
int bs_shift_to_origin_dev(bs_ctx* ctx, int32_t* d_xyz, int64_t n, int32_t* min_out);

/* PLY ingest on the device (replaces the per-property loop of
 * ply::read, ply.cpp:431-501, for the positions): d_records is the binary
 * little-endian vertex body resident on the device (n records of `stride` bytes,
 * x/y/z at byte offsets off_x/off_y/off_z, all three float32 (is_f64 = 0) or
 * float64; d_records may have any alignment, e.g. the byte just past the header
 * of an uploaded file: fields are assembled from bytes).  d_xyz [n][3] receives
 * (int32) trunc(value * scale) (ply.cpp:436-465;
 * float promoted to double first).  shift_to_origin != 0 additionally applies the
 * buildingSeg constructor's bounding-box shift (TMC3.cpp:55-73) and reports the
 * subtracted minimum in min_out (host [3], nullable).  BS_ERR_RANGE if a product
 * does not fit int32 (undefined behaviour in the reference).  Synchronises. */
int bs_ingest_dev(bs_ctx* ctx, const void* d_records, int64_t n, int32_t stride, int32_t off_x, int32_t off_y,
                  int32_t off_z, int32_t is_f64, double scale, int32_t shift_to_origin, int32_t* d_xyz,
                  int32_t* min_out);
int bs_plane_colors_dev(bs_ctx* ctx, const int32_t* plane_rgb, int32_t n_planes, int64_t n, uint16_t* d_colors);

/* 2-D density / height raster: the reference's (currently commented-out) 2-D
 * branch, SURVEY.md 8f-4.  Replaces buildingSeg::groundTH (TMC3.cpp:183-199) and
 * buildingSeg::compute_gird_picture (TMC3.cpp:123-174) for a cloud that has
 * already been shifted to its bounding-box origin (bs_shift_to_origin_dev, i.e.
 * the buildingSeg constructor, TMC3.cpp:55-73).
 *
 *   extent[3]  = box.max - box.min of the unshifted cloud (= max of the shifted one)
 *   bin        = pixel edge in mm (reference: 100), bin_height = height-histogram
 *                bin in mm (reference: 1000)
 *   bs_grid_dims: width = extent[0]/bin + 2, height = extent[1]/bin + 2 (TMC3.cpp:75-76)
 *   image      = [height][width][3] f64, caller-allocated, pixel(x,y,c) at
 *                (y*width + x)*3 + c as in TMC3.cpp:119-121:
 *                  c=0 mean height of the splatted points, c=1 log(density+1) (+20
 *                  where non-zero), c=2 zero (the reference never writes it)
 *   ground_th  (host, nullable) receives groundTH()
 * Bit-identical to the reference's sequential f64 accumulation in channel 0 and in
 * the density sums; the logarithm is bs_det_log of include/bs_detmath.h (within
 * 1 ulp of the platform libm the reference calls).  BS_ERR_RANGE if a coordinate
 * lies outside [0, extent].  Synchronises. */
int bs_grid_dims(const int32_t* extent, int32_t bin, int32_t* width, int32_t* height);
int bs_grid_picture(bs_ctx* ctx, const int32_t* xyz, int64_t n, const int32_t* extent, int32_t bin,
                    int32_t bin_height, double* image, double* ground_th);
int bs_grid_picture_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, const int32_t* extent, int32_t bin,
                        int32_t bin_height, double* d_image, double* ground_th);

/* Self-test of the grower's plane-centre division (csrc/bs_centerdiv.h) ON THE
 * DEVICE: out[i] = (int32_t)((uint64_t)(int64_t)c[i] / n[i]), the expression of
 * my_function.cpp:249-250, for count host-side pairs (1 <= n[i] < 2^31).  The
 * device version rests on the hardware reciprocal seed, which no host test can
 * exercise; tests/test_gpu_parity.py checks millions of pairs through this. */
int bs_selftest_center_div(bs_ctx* ctx, const int32_t* c, const uint32_t* n, int32_t* out, int64_t count);

/* Self-test of the grower's post-round validation: the NEXT region grow on this context corrupts one
 * finished plane before validating it -- mode 1: a list entry duplicated (a point held twice), mode 2:
 * the reported normal off by one ulp -- the way the claim-protocol bugs found by fuzzing did.  The
 * validation must refuse the plane (bs_timings.forged_refused == 1, forged_seed names it); it is
 * then grown again and the final result is still exact. */
int bs_selftest_forge_next(bs_ctx* ctx, int mode);

/* Audit mode (off by default; also switched on by the environment variable BS_AUDIT=1).  After a
 * speculative region grow (rg_mode 0 / 2) every plane attempt that exists under the FINAL owners -- the
 * committed planes and the attempts the reference rolls back (my_function.cpp:199) -- is grown once more,
 * all of them concurrently, with the production step engine but WITHOUT speculation: a point is taken iff
 * its final owner is an earlier attempt, nothing is assumed, nothing can be stolen.  Every Broad() decision
 * of every plane is thereby re-made against the state the sequential reference has at that plane's time;
 * the replayed lists must equal the committed ones entry by entry, in order, with bit-equal normal and
 * centre, and an attempt that was not committed must end at or below the commit threshold.  Together with
 * the owner equations (BS_VERIFY=1) this certifies the result of the speculation by induction over the
 * seed index.  Costs about one extra pass of the longest plane; bs_timings.audit_* report it. */
int bs_set_audit(bs_ctx* ctx, int on);

/* Self-test of the speculative grower's recovery paths: LOWER the capacities a region grow derives from the
 * cloud size, so that the code that runs when one of them is exhausted (capped rounds, a round pool that runs
 * out, finished planes that find no pending room) is reached on clouds of 10^4-10^6 points instead of 10^8.
 * Sticky: holds for every following grow on the context (bs_region_grow[_dev], bs_segment[_dev],
 * bs_segment_batch[_dev]) until cleared with lim == NULL; read once per call.  The result of a grow is the same
 * bits whatever the limits; a round pool too small for the lowest attempt alone ends the call with BS_ERR_NOMEM.
 *   Capacities (0 = default): only ever lowered -- a value above what the library would choose is clamped to
 *   it -- and every buffer keeps its normal size, so no setting can cause an access out of bounds.
 *   Policies (< 0 = default): any non-negative value, with the meaning of the environment switches
 *   BS_RETRY_MAX_LIST / BS_RETRY_BIG_ROUND (which keep working, as do BS_MAX_WAVES and BS_FULL_REFRESH; a value
 *   set here wins over the environment).  The audit replay (bs_set_audit) always runs with the full capacities. */
typedef struct bs_grow_limits {
  int64_t max_waves;       /* plane attempts grown per round */
  int64_t pool_cap;        /* round pool (lists + stacks + logs of the round's attempts), int32 entries */
  int64_t max_pending;     /* finished planes kept while an earlier attempt is open */
  int64_t pstore_cap;      /* store of their lists and logs, int32 entries */
  int32_t retry_max_list;  /* a stolen plane is grown again inside the launch while its list is at most this long;
                              set, it holds in rounds of every size (as BS_RETRY_MAX_LIST does) */
  int32_t retry_big_round; /* rounds of at least this many attempts re-grow lists of any length (0: every round) */
  int32_t full_refresh;    /* != 0: rebuild every record's owner fields before every round (BS_FULL_REFRESH) */
  int32_t reserved;        /* 0 */
} bs_grow_limits;
int bs_selftest_grow_limits(bs_ctx* ctx, const bs_grow_limits* lim);

/* What the host loop of the last speculative region grow on this context saw (also filled when that call failed
 * with BS_ERR_NOMEM): which of the limits above were reached.  All zero after a sequential grow (rg_mode 1). */
typedef struct bs_grow_counters {
  int64_t rounds;
  int64_t rounds_capped;      /* rounds with more candidates than attempts per round: the rest waited */
  int64_t rounds_big;         /* rounds of >= 4096 attempts (dispatch order, compacted copy-back) */
  int64_t attempts_nomem;     /* attempts that ended because the round pool was exhausted */
  int64_t waves_cut;          /* times the LOWEST attempt of a round ran out of pool: attempts per round cut to 1/8 */
  int64_t max_waves_end;      /* attempts per round when the call ended */
  int64_t attempts_stolen;    /* attempts that lost a point and were left for the next round.  Counted in rounds
                                 below 4096 attempts only: a bigger round copies back just the finished and the
                                 exhausted attempts */
  int64_t dropped_pend_count; /* finished, consistent planes dropped (and grown again) for lack of a pending slot */
  int64_t dropped_pend_store; /* ... for lack of room in the pending store */
  int64_t dropped_other;      /* planes dropped as inconsistent with the settled owners or refused by the validation */
  int64_t full_refreshes;     /* rounds that began with a full rebuild of the records' owner fields */
  int64_t pool_cap;           /* the round pool's capacity in force, int32 entries */
} bs_grow_counters;
int bs_get_grow_counters(const bs_ctx* ctx, bs_grow_counters* out);

/* Self-test of the context's scratch memory (off by default; tests/test_gpu_scratch_guard.py).  Every stage cuts the
 * buffers of its context into sub-arrays by hand, and an allocation normally carries 12.5 % + 256 B of slack that hides a
 * write past the requested size.  While the guard is set, every FRESH allocation of one of this context's buffers
 *   - is requested + guard bytes long, guard = max(4096, requested / 8 + 256) -- never less than the normal slack;
 *   - counts as exactly `requested` bytes: a later request up to that size keeps the buffer and its contents, a larger
 *     one allocates afresh, as always;
 *   - BS_SCRATCH_CANARY: has its guard filled with the byte 0xC5, which bs_selftest_scratch_check reads back;
 *   - BS_SCRATCH_POISON: has its requested bytes filled with poison_byte (0..255), so that a stage that reads scratch
 *     nothing wrote reads that and not the zeros of a first allocation.  A buffer that is kept is never filled again.
 * The page-locked host buffer the grower's kernels write gets the canary only.  Accepted only while the context has
 * nothing allocated (right after bs_create), BS_ERR_INVALID otherwise; flags == 0 leaves the guard off.  Other contexts
 * are not affected. */
#define BS_SCRATCH_CANARY 1
#define BS_SCRATCH_POISON 2
int bs_selftest_scratch_guard(bs_ctx* ctx, int flags, int poison_byte);

/* One guarded buffer: `name` is the member of bs_ctx (csrc/bs_common.h) with its array index, e.g. "rf[9]". */
typedef struct bs_scratch_slot {
  char name[24];
  uint64_t address;   /* of the first requested byte (device memory; page-locked host memory where host != 0) */
  int64_t requested;  /* bytes the stage asked for */
  int64_t guard;      /* bytes behind them */
  int64_t first_bad;  /* offsets of the first and the last damaged guard byte from the end of the request ... */
  int64_t last_bad;   /* ... as of the last bs_selftest_scratch_check that listed this slot; -1 = clean / bs_..._list */
  int32_t host;
  int32_t reserved;
} bs_scratch_slot;

/* Synchronises the context's streams and reads every guard back. */
#define BS_SCRATCH_REPORT_MAX 8
typedef struct bs_scratch_report {
  int64_t n_guarded;        /* buffers allocated under the guard */
  int64_t bytes_requested;  /* their requested sizes, summed */
  int64_t n_damaged;        /* buffers whose guard no longer holds the canary */
  int64_t n_listed;         /* min(n_damaged, BS_SCRATCH_REPORT_MAX) */
  bs_scratch_slot damaged[BS_SCRATCH_REPORT_MAX];  /* the first of them, in the order of bs_ctx */
} bs_scratch_report;
int bs_selftest_scratch_check(bs_ctx* ctx, bs_scratch_report* report);

/* Every buffer of the context allocated under the guard, in the order of bs_ctx: up to `capacity` of them into slots
 * (nullable with capacity 0), their number into *n_slots.  With ctx == NULL nothing is listed and *n_slots receives the
 * number of buffer members a context has -- after checking, without a device, that the member table the names come from
 * lists every one of them (BS_ERR_INTERNAL if not; bs_create makes the same check). */
int bs_selftest_scratch_list(bs_ctx* ctx, bs_scratch_slot* slots, int64_t capacity, int64_t* n_slots);

/* Copy the plane records of the last region-grow on this context to the host. */
int bs_planes_fetch(bs_ctx* ctx, bs_planes* planes);

/* ---- batches of independent tiles in one pass ----
 *
 * n_tiles independent clouds segmented in one device pass.  xyz is their concatenation; tile t is the points
 * [tile_offset[t], tile_offset[t+1]) (host array, tile_offset[0] == 0, non-decreasing, every tile >= k points, fewer
 * than INT32_MAX - 64 points in all).  Every output equals what bs_segment returns for that tile alone, bit for bit:
 *   neigh rows hold TILE-LOCAL indices; plane_idx numbers planes from 1 in every tile;
 *   planes is the concatenation of the per-tile plane lists (ids from 1 per tile, point_idx tile-local);
 *   plane_offset [n_tiles+1] (host out) delimits each tile's planes inside it.
 * The search grid keys cells by (tile, cell), so tiles that overlap or touch in space never see each other; the
 * grower runs once over the concatenation (the sequential rule gives each tile its solo result) and
 * the outputs are renumbered on the device.  BS_ERR_INVALID names the offending tile; BS_ERR_RANGE: a coordinate
 * outside |c| < 2^23 mm (shift every tile to its own origin first: bs_shift_tiles_to_origin_dev).  neigh, normals,
 * planes and plane_offset are nullable; the _dev form's d_neigh / d_normals may be NULL (context scratch). */
int bs_segment_batch(bs_ctx* ctx, const int32_t* xyz, const int64_t* tile_offset, int32_t n_tiles, const bs_params* p,
                     int32_t* neigh, double* normals, int32_t* plane_idx, bs_planes* planes, int32_t* plane_offset);
int bs_segment_batch_dev(bs_ctx* ctx, const int32_t* d_xyz, const int64_t* tile_offset, int32_t n_tiles,
                         const bs_params* p, int32_t* d_neigh, double* d_normals, int32_t* d_plane_idx);
/* The plane records of the last bs_segment_batch[_dev] on this context, renumbered per tile (see above);
 * plane_offset [n_tiles+1] (host, nullable). */
int bs_batch_planes_fetch(bs_ctx* ctx, bs_planes* planes, int32_t* plane_offset);
/* bs_shift_to_origin_dev applied to every tile separately (TMC3.cpp:55-73 per tile): min_out [n_tiles][3] (host,
 * nullable) receives each tile's subtracted minimum.  Offsets as above (every tile >= 1 point).  Synchronises.
 * Contract as for bs_shift_to_origin_dev, per tile: the extent max - min of every axis of every tile is below 2^31 (not
 * checked here; api.shift_tiles_to_origin refuses it on the host). */
int bs_shift_tiles_to_origin_dev(bs_ctx* ctx, int32_t* d_xyz, const int64_t* tile_offset, int32_t n_tiles,
                                 int32_t* min_out);

/* ---- building blocks of the multi-GPU path (component-sharded stage 3) ----
 *
 * The reference's seed scan (my_function.cpp:184-217) is global, but information only travels along kNN edges
 * (Broad tests neigh[Idx][1..K-1], :224-233; a failed seed labels part of its own row, :238-239): connected
 * components of the kNN graph never interact, and the only shared state is cur_planeId, which advances once per
 * committed plane (:199-202), i.e.
 *     planeIdx[p] = 1 + #(committed seeds < owner[p]),   owner[p] = the seed attempt that left p labelled.
 * So stage 3 shards exactly: whole components per GPU (local cloud in ascending global index order), committed
 * seeds all-gathered, labels from the owners.  buildingsegment_amd/dist.py (torch.distributed) and
 * bs_segment_sharded (RCCL, below) are built from these calls.
 *
 * bs_cc_hook_dev: one hooking step of a distributed union-find.  d_parent [n_total] (device, in/out) is a parent
 *   array over GLOBAL point ids with parent[x] <= x (start: identity).  The call unites u = d_gidx[i] (NULL: i) with
 *   every d_rows[i][j] (global ids, [m][k]) and points every node it touched straight at its root.  *n_hooks (host)
 *   = unions performed.  Multi-GPU: every rank hooks its own rows, the parent arrays are all-reduced with MIN, and
 *   the step repeats until no rank hooked anything; then parent[x] = smallest global id of x's component.
 *   Synchronises.
 * bs_owner_fetch_dev: d_owner [n] (device) receives, in the caller's index order, the seed index of the attempt
 *   that left each point labelled after the last bs_region_grow[_dev] / bs_segment[_dev] on this context (-1:
 *   unlabelled).  rg_mode 0 / 2 only (the single-wave grower keeps no owners: BS_ERR_INVALID).
 * bs_labels_from_owner_dev: d_plane_idx[i] = d_owner[i] < 0 ? -1 : 1 + #(d_seeds[] < d_owner[i]); d_seeds is the
 *   ascending list of ALL committed seeds (global indices), d_owner holds global seed indices.
 * bs_remap_rows_dev: d_out[t] = position of d_rows[t] in the ascending array d_sorted_gidx [n] (global -> local
 *   index of a component-complete local cloud); *n_missing (host) != 0 if some index was not found.  Synchronises. */
int bs_cc_hook_dev(bs_ctx* ctx, const int32_t* d_rows, const int32_t* d_gidx, int64_t m, int32_t k, int32_t* d_parent,
                   int64_t n_total, int64_t* n_hooks);
int bs_owner_fetch_dev(bs_ctx* ctx, int32_t* d_owner);
/* bs_plane_seeds_dev: the seeds (= pointIdx[0], my_function.cpp:191) of the planes the last speculative grow on this
 *   context committed, ascending (= commit order); *n_planes (host) receives their number, at most cap of them are
 *   copied to d_seeds (device, nullable).  bs_stream_sync: wait for everything enqueued on the context's stream. */
int bs_plane_seeds_dev(bs_ctx* ctx, int32_t* d_seeds, int64_t cap, int32_t* n_planes);
int bs_stream_sync(bs_ctx* ctx);
int bs_labels_from_owner_dev(bs_ctx* ctx, const int32_t* d_owner, int64_t n, const int32_t* d_seeds, int32_t n_seeds,
                             int32_t* d_plane_idx);
int bs_remap_rows_dev(bs_ctx* ctx, const int32_t* d_rows, int64_t n_rows, int32_t k, const int32_t* d_sorted_gidx,
                      int64_t n, int32_t* d_out, int32_t* n_missing);

/* ---- multi-GPU entry point: ONE cloud sharded over the ranks of a communicator ----
 *
 * bs_segment_sharded is what the C++ host of TMC3.cpp:213-217 calls when it runs as one process per GPU: rank r
 * passes the points it holds (any split of the cloud: d_xyz [m][3], d_gidx [m] = their global indices, both on
 * its device) and receives planeIdx for the WHOLE cloud (d_plane_idx [n_total], device, identical on every rank).
 * Stages 1-2 run on Morton slabs with a halo exchange, stage 3 on whole connected components of the kNN graph
 * (see "building blocks" above); results equal the single-GPU / sequential ones bit for bit.
 *
 * The collectives are reached through bs_comm_ops: three operations on DEVICE buffers, enqueued on `stream`
 * (the context's stream; they may synchronise it).  bs_comm_rccl() fills the table for an RCCL communicator
 * (ncclComm_t; librccl.so.1 is resolved at run time) -- reductions by ncclAllReduce, gathers by ncclAllGather,
 * the split-size all-to-all by grouped ncclSend / ncclRecv over xGMI.  A host with another transport (MPI, a test
 * harness) supplies its own three functions.  Every function returns 0 or a non-zero error. */
typedef enum bs_comm_dtype { BS_I32 = 0, BS_I64 = 1 } bs_comm_dtype;
typedef enum bs_comm_op { BS_MIN = 0, BS_MAX = 1, BS_SUM = 2 } bs_comm_op;
typedef struct bs_comm_ops {
  void* handle; /* passed back as the first argument */
  int32_t rank, world;
  /* in-place all-reduce of count elements */
  int (*all_reduce)(void* handle, void* d_buf, int64_t count, int dtype, int op, void* stream);
  /* every rank contributes `bytes` bytes; d_recv receives world * bytes in rank order */
  int (*all_gather)(void* handle, const void* d_send, void* d_recv, int64_t bytes, void* stream);
  /* d_send holds the blocks for ranks 0..world-1 back to back (send_bytes[r] each, host array); d_recv receives the
   * blocks of ranks 0..world-1 back to back (recv_bytes[r] each, host array, already agreed on by the caller) */
  int (*all_to_all_v)(void* handle, const void* d_send, const int64_t* send_bytes, void* d_recv,
                      const int64_t* recv_bytes, void* stream);
} bs_comm_ops;

/* RCCL-backed table for an existing communicator (`nccl_comm` is an ncclComm_t created by the host for this
 * device).  BS_ERR_NO_DEVICE if librccl cannot be loaded. */
int bs_comm_rccl(void* nccl_comm, int32_t rank, int32_t world, bs_comm_ops* out);
/* Convenience for hosts without RCCL code of their own: rank 0 draws a 128-byte id and hands it to the other
 * ranks by any means; every rank then creates its communicator for the context's device. */
int bs_comm_rccl_unique_id(char id[128]);
int bs_comm_rccl_init(bs_ctx* ctx, const char id[128], int32_t rank, int32_t world, void** nccl_comm);
int bs_comm_rccl_destroy(void* nccl_comm);

/* In-process communicator: the `world` ranks are THREADS of one process (one host thread per GPU without a
 * launcher; several ranks sharing one GPU in the tests).  Fills out[0..world-1]; every rank's buffers must be
 * reachable from the others' devices (same device, or peer access enabled by the host).  Collectives are device
 * copies between the ranks' buffers behind a host barrier -- functional, not tuned: use bs_comm_rccl across GPUs.
 * Every wait of that barrier has a deadline: 120 s by default, or BS_COMM_LOCAL_TIMEOUT_S seconds (environment,
 * a number > 0, read by bs_comm_local_create).  When a rank does not arrive in time (it left bs_segment_sharded
 * with an error of its own, or its thread died) the communicator is broken for good: the collective in progress
 * and every later one return non-zero on every rank, so bs_segment_sharded returns BS_ERR_INTERNAL instead of
 * waiting for ever.  Destroy a broken communicator and create a new one.  The default is about fifty times the
 * longest pass measured with thread-ranks sharing one GPU; waits on a real multi-GPU node have not been measured. */
int bs_comm_local_create(int32_t world, bs_comm_ops* out /* [world] */);
void bs_comm_local_destroy(bs_comm_ops* ops /* one entry of the array; call for every rank */);

typedef struct bs_shard_info {
  int64_t n_own;        /* points of this rank's Morton slab */
  int64_t n_local;      /* slab + halo */
  int64_t n_grow;       /* points of the components this rank grew */
  int64_t components;   /* connected components of the kNN graph (whole cloud) */
  int64_t planes_total; /* committed planes (whole cloud) */
  int32_t cc_iterations, halo_retries;
  double halo_mm;
  double ms_partition, ms_halo, ms_knn, ms_components, ms_redistribute, ms_grow, ms_labels; /* host wall time */
} bs_shard_info;

/* halo: initial halo width in mm (0 = 2 * radius); doubled until every k-list is certified.  d_gidx may be NULL
 * only at world 1 (identity).  info is optional.
 * Errors reach every rank: a rank whose own share is unusable (m < 0, m > n_total, a missing d_xyz or d_gidx)
 * returns BS_ERR_INVALID and its peers BS_ERR_INTERNAL after the first all-reduce; shares that do not cover
 * 0..n_total-1 exactly once give BS_ERR_INVALID and a halo that cannot be certified within six doublings
 * BS_ERR_UNCERTIFIED on every rank.  The contexts and the communicator stay usable after these.  Every d_gidx value
 * must lie in 0..n_total-1: it is used as a subscript before the shares are checked. */
int bs_segment_sharded(bs_ctx* ctx, const bs_comm_ops* comm, const int32_t* d_xyz, const int32_t* d_gidx, int64_t m,
                       int64_t n_total, const bs_params* p, double halo, int32_t* d_plane_idx, bs_shard_info* info);
/* The planes THIS rank grew in the last bs_segment_sharded, with global ids (1-based rank of the seed among all
 * committed seeds) and global point indices, ascending id.  Released by bs_planes_free. */
int bs_sharded_planes_fetch(bs_ctx* ctx, bs_planes* planes);

/* ---- building footprints: the reference's extracted_contour (my_function.cpp:8-145) on the density raster ----
 *
 * image is the [height][width][3] f64 raster of bs_grid_picture; channel 1 (density) is read.
 *   1. quantise as save_image does (TMC3.cpp:100-108): q = (uint8)(255.0 * (1.0 * v / max1)), max1 = max(0, max v),
 *      q = 0 where max1 == 0 (and where v < 0 or NaN, which the raster never holds)
 *   2. binarise: foreground iff q > threshold (reference: 10)
 *   3. close: `iterations` dilations, then as many erosions, with OpenCV's kernel_size x kernel_size ellipse;
 *      pixels outside the image count as background for dilation and as foreground for erosion
 *      (reference: 5, 2; iterations = 0 skips the closing)
 *   4. findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE): the outer border of every 8-connected foreground component
 *      that is not inside a hole of another one, traced from the component's first pixel in raster order, in
 *      OpenCV's point order; contours in descending order of that first pixel
 *   5. contourArea and arcLength(closed) of every contour
 * d_mask (nullable, device [height][width]) receives the closed mask as 0 / 255.  The result arrays are host
 * memory owned by the library and released by bs_contours_free (which accepts a zeroed struct).
 * BS_ERR_INVALID: null pointer, width or height < 1, (width+2)*(height+2) >= 2^31, kernel_size even or outside
 * 1..15, iterations outside 0..16, threshold outside 0..255.  BS_ERR_RANGE: more border states than the tracer can
 * index (2^31).  BS_ERR_INTERNAL: a contour's list ranking did not converge within its bound.  Synchronises. */
typedef struct bs_contours {
  int32_t n_contours;
  int32_t width, height; /* raster the contours were taken from (the OBJ normalisation) */
  int64_t* offset;       /* [n_contours+1] into xy */
  int32_t* xy;           /* [offset[n_contours]][2]: x = column, y = row */
  double* area;          /* [n_contours] contourArea */
  double* perimeter;     /* [n_contours] arcLength(contour, true) */
} bs_contours;

/* Per-stage device time (HIP events) of the last bs_footprints[_dev] call and the sizes it worked on. */
typedef struct bs_footprint_info {
  double ms_mask, ms_close, ms_label, ms_trace, ms_total;
  int64_t fg_pixels;     /* foreground pixels after the closing */
  int64_t border_states; /* (pixel, back-direction) states the tracer ranked */
  int64_t components;    /* external foreground components (= n_contours) */
  int64_t jump_rounds;   /* pointer-jumping rounds of the list ranking */
} bs_footprint_info;

int bs_footprints_dev(bs_ctx* ctx, const double* d_image, int32_t width, int32_t height, int32_t threshold,
                      int32_t kernel_size, int32_t iterations, uint8_t* d_mask, bs_contours* out,
                      bs_footprint_info* info);
/* Host-memory variant: image and mask (nullable) are host pointers. */
int bs_footprints(bs_ctx* ctx, const double* image, int32_t width, int32_t height, int32_t threshold,
                  int32_t kernel_size, int32_t iterations, uint8_t* mask, bs_contours* out, bs_footprint_info* info);
void bs_contours_free(bs_contours* c);
/* The reference's OBJ (my_function.cpp:64-131): every contour extruded into a prism of quads between z = 0 and
 * z = 1, x = x / width, y = 1 - y / height (float).  Host only; BS_ERR_INVALID if the file cannot be written. */
int bs_contours_write_obj(const bs_contours* c, const char* path);

/* ---- batches of rasters and footprints: every output the reference's main produces for a block, per tile ----
 *
 * Tiles follow the batch conventions above: tile_offset [n_tiles+1] (host, int64) starts at 0 and rises strictly
 * (every tile >= 1 point).  Every per-tile output equals, bit for bit, what the solo call returns for that tile
 * alone; error texts name the offending tile.  Limits are the solo ones applied to the batch totals: fewer than
 * 2^29 points (BS_ERR_RANGE), fewer than 2^31 - 1 pixels (BS_ERR_RANGE), fewer than 2^31 padded pixels
 * (W+2)(H+2) (BS_ERR_INVALID), fewer than 2^31 border states (BS_ERR_RANGE).  A failed call leaves the context
 * usable.  A device pipeline runs bs_shift_tiles_to_origin_dev -> bs_tile_boxes_dev (extents = max - min of the
 * shifted tiles) -> bs_grid_dims_batch -> bs_grid_picture_batch_dev -> bs_footprints_batch_dev. */

/* Per-tile {min x,y,z, max x,y,z} of a device-resident concatenation (host out [n_tiles][6]); synchronises.
 * A device pipeline gets its raster extents from this without copying the cloud back. */
int bs_tile_boxes_dev(bs_ctx* ctx, const int32_t* d_xyz, const int64_t* tile_offset, int32_t n_tiles,
                      int32_t* box_out);

/* Host only, no context: width[t], height[t] as bs_grid_dims for extent[t] ([n_tiles][3]), and
 * pixel_offset[n_tiles+1] (int64) = exclusive prefix sum of width*height.  Tile t's image is the
 * [height[t]][width[t]][3] f64 block starting at pixel pixel_offset[t] of the batch image.  BS_ERR_INVALID if
 * n_tiles < 1, a pointer is NULL or any tile's extent / bin is invalid for bs_grid_dims. */
int bs_grid_dims_batch(const int32_t* extent, int32_t n_tiles, int32_t bin, int32_t* width, int32_t* height,
                       int64_t* pixel_offset);

/* bs_grid_picture_dev for every tile (each already shifted to its own origin, e.g. by
 * bs_shift_tiles_to_origin_dev), in one pass: per-tile ground threshold (ground_th: host [n_tiles], nullable),
 * images at pixel_offset.  BS_ERR_RANGE names the first tile with a point outside [0, extent[t]].  Synchronises. */
int bs_grid_picture_batch_dev(bs_ctx* ctx, const int32_t* d_xyz, const int64_t* tile_offset, int32_t n_tiles,
                              const int32_t* extent, int32_t bin, int32_t bin_height, double* d_image,
                              double* ground_th);
/* Host-memory variant: xyz and image are host pointers. */
int bs_grid_picture_batch(bs_ctx* ctx, const int32_t* xyz, const int64_t* tile_offset, int32_t n_tiles,
                          const int32_t* extent, int32_t bin, int32_t bin_height, double* image, double* ground_th);

/* bs_footprints_dev for every tile image of the batch layout above (width/height: host [n_tiles]).
 * out is the concatenation of the per-tile contour lists, tile-major, each tile in its solo order;
 * contour_offset [n_tiles+1] (host out) delimits them; out->width = out->height = 0.
 * d_mask (nullable): per-tile closed masks, [height[t]][width[t]] bytes at pixel_offset[t].
 * info (nullable): stage times of the whole pass and totals over all tiles (jump_rounds: of the one ranking).
 * Tile t as a bs_contours of its own is the view {n_contours = co[t+1] - co[t], width[t], height[t],
 * offset = out.offset + co[t], the same xy, area + co[t], perimeter + co[t]}: bs_contours_write_obj reads offset
 * as absolute positions into xy, so the view writes the same bytes as the solo result.  Release out (not the
 * views) with bs_contours_free.  Synchronises. */
int bs_footprints_batch_dev(bs_ctx* ctx, const double* d_image, const int32_t* width, const int32_t* height,
                            int32_t n_tiles, int32_t threshold, int32_t kernel_size, int32_t iterations,
                            uint8_t* d_mask, bs_contours* out, int32_t* contour_offset, bs_footprint_info* info);
/* Host-memory variant: image and mask (nullable) are host pointers. */
int bs_footprints_batch(bs_ctx* ctx, const double* image, const int32_t* width, const int32_t* height,
                        int32_t n_tiles, int32_t threshold, int32_t kernel_size, int32_t iterations, uint8_t* mask,
                        bs_contours* out, int32_t* contour_offset, bs_footprint_info* info);

/* ---- buildings: which points and which planes belong to which footprint ----
 *
 * Building map of a closed mask [height][width] (bytes, non-zero = foreground: what bs_footprints[_dev] writes to
 * its mask), padded with a one-pixel background frame as the tracer pads it:
 *   outer background = the 4-connected background region that contains the frame;
 *   filled           = every other pixel (the foreground and whatever a foreground component encloses);
 *   a building       = an 8-connected component of the filled set; its start pixel is its first pixel in raster
 *                      order; buildings are numbered from 0 in DESCENDING order of start pixel;
 *   map[y][x]        = the building of the pixel, -1 for outer background.
 * Building c is contour c of bs_footprints on the same mask: the same count, start_xy[c] = the contour's first point,
 * and every point of contour c lies on a pixel of building c.
 *
 * Points (cloud shifted to its origin, as for bs_grid_picture): building_idx[i] = map[y_i / bin][x_i / bin], the
 * base pixel of the point's splat (TMC3.cpp:134-135); a point is above ground iff !(z < ground_th) (TMC3.cpp:139,
 * ground_th as bs_grid_picture returns it).  With the map of the same cloud's own raster at threshold 10, every
 * above-ground point has a building >= 0.
 * Planes: for p = 1 .. n_planes, over the points with plane_idx == p (the labels, not the lists), entry p - 1 of
 *   votes_total = their number, votes_outside = those with building -1, plane_building = the building >= 0 that
 *   holds most of them (ties: the lower index; -1 if none holds any), votes_in = that building's count.
 * Everything is an exact integer and independent of the order of summation. */
typedef struct bs_buildings {
  int32_t n_buildings;
  int32_t width, height; /* raster of the map */
  /* filled by bs_building_map[_dev] */
  int32_t* start_xy;  /* [n_buildings][2] first pixel in raster order: x, y */
  int32_t* bbox;      /* [n_buildings][4] inclusive pixel box: x0, y0, x1, y1 */
  int64_t* pixels;    /* [n_buildings] filled pixels */
  int64_t* fg_pixels; /* [n_buildings] ... of which foreground in the mask */
  /* filled by bs_assign_buildings[_dev] (0 / INT32_MAX / INT32_MIN / 0 before) */
  int64_t* n_points;  /* [n_buildings] points whose base pixel lies in the building */
  int64_t* n_above;   /* [n_buildings] ... of which above ground */
  int32_t* z_min;     /* [n_buildings] over the above-ground points; INT32_MAX if there is none */
  int32_t* z_max;     /* [n_buildings] INT32_MIN if there is none */
  int64_t* z_sum;     /* [n_buildings] sum of z over the above-ground points */
  /* device time (HIP events on the context's stream) of the last calls that filled this struct */
  double ms_label_mask; /* labelling pass 1: foreground / background of the mask (tile, seam and flatten kernels) */
  double ms_label_fill; /* labelling pass 2: the filled set */
  double ms_number;     /* start-pixel flags + scan + read-back of the count */
  double ms_map;        /* map and pixel figures */
  double ms_assign;     /* bs_assign_buildings_dev: the assignment kernel */
} bs_buildings;

/* d_mask [height][width] bytes and d_map [height][width] int32 are device pointers; out's arrays are host memory
 * owned by the library (bs_buildings_free, which accepts a zeroed struct).  An empty mask gives 0 buildings and a
 * map of -1.  BS_ERR_INVALID: null pointer, width or height < 1, (width+2)*(height+2) >= 2^31.  Synchronises. */
int bs_building_map_dev(bs_ctx* ctx, const uint8_t* d_mask, int32_t width, int32_t height, int32_t* d_map,
                        bs_buildings* out);
/* Host-memory variant: mask and map are host pointers. */
int bs_building_map(bs_ctx* ctx, const uint8_t* mask, int32_t width, int32_t height, int32_t* map, bs_buildings* out);
void bs_buildings_free(bs_buildings* b);

/* d_building_idx [n] int32 (device) receives every point's building; the point figures of inout (the struct the map
 * call for d_map created: same width and height) are overwritten.  BS_ERR_INVALID: null pointer, n < 1, bin < 1, a
 * struct of another raster; BS_ERR_RANGE: 2^29 points or more, or a point with a negative x / y or whose pixel lies
 * outside the image (inout is then left as it was).  Synchronises. */
int bs_assign_buildings_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t bin, double ground_th,
                            const int32_t* d_map, int32_t width, int32_t height, int32_t* d_building_idx,
                            bs_buildings* inout);
/* Host-memory variant: xyz, map and building_idx are host pointers. */
int bs_assign_buildings(bs_ctx* ctx, const int32_t* xyz, int64_t n, int32_t bin, double ground_th, const int32_t* map,
                        int32_t width, int32_t height, int32_t* building_idx, bs_buildings* inout);

/* d_plane_idx / d_building_idx [n] are device pointers, the four result arrays host [n_planes] (entry p - 1 is plane
 * p; not touched when n_planes == 0).  Labels outside 1 .. n_planes (-1 = unlabelled) are ignored.
 * BS_ERR_INVALID: null pointer, n < 1, n_planes < 0, n_buildings < 0; BS_ERR_RANGE: 2^29 points or more, or a
 * building index outside [-1, n_buildings).  Synchronises. */
int bs_plane_buildings_dev(bs_ctx* ctx, const int32_t* d_plane_idx, const int32_t* d_building_idx, int64_t n,
                           int32_t n_planes, int32_t n_buildings, int32_t* plane_building, int64_t* votes_in,
                           int64_t* votes_total, int64_t* votes_outside);
/* Host-memory variant: plane_idx and building_idx are host pointers. */
int bs_plane_buildings(bs_ctx* ctx, const int32_t* plane_idx, const int32_t* building_idx, int64_t n, int32_t n_planes,
                       int32_t n_buildings, int32_t* plane_building, int64_t* votes_in, int64_t* votes_total,
                       int64_t* votes_outside);

/* LoD1 model in millimetres: every kept footprint extruded from the ground threshold to the mean height of its
 * above-ground points.  Host only.  c and b describe the same mask (c->n_contours == b->n_buildings).  Contour i is
 * KEPT iff area[i] > min_area && perimeter[i] > min_perimeter (the reference's filter, my_function.cpp:42, uses 500
 * and 100) && n_above[i] > 0.  origin [3] is the shift that was subtracted from the cloud (NULL: 0).  The file, every
 * number a decimal integer, every line ended by '\n':
 *   "# buildings: <kept> of <n_contours>"
 *   for every kept contour in order, for every point (x, y) of it in order, two lines
 *     "v X Y Z0" and "v X Y Z1"   X = x * bin + origin[0], Y = y * bin + origin[1],
 *                                 Z0 = (int64) ground_th + origin[2]            (truncated towards zero)
 *                                 Z1 = z_sum[i] / n_above[i] + origin[2]        (quotient truncated towards zero)
 *   for every kept contour in order, for k = 0 .. n - 1 (n = its points, vertices numbered from 1 in file order,
 *   base = the contour's first vertex, nx = (k + 1) % n), the reference's side quad (my_function.cpp:109-126)
 *     "f <base+2k> <base+2nx> <base+2nx+1> <base+2k+1>"
 *   for every kept contour with n >= 3 in order, the roof over its top vertices
 *     "f <base+1> <base+3> ... <base+2n-1>"
 * BS_ERR_INVALID: null pointer, bin < 1, counts that differ, or the file cannot be written. */
int bs_buildings_write_obj(const bs_contours* c, const bs_buildings* b, int32_t bin, const int32_t* origin,
                           double ground_th, double min_area, double min_perimeter, const char* path);

/* ---- roofs: which plane is the roof over every pixel of a building, and how high it is there ----
 *
 * Inputs: the cloud shifted to its origin (n < 2^29), bin and ground_th as for bs_assign_buildings, the building map
 * map[height][width] as bs_building_map writes it, the labels plane_idx[n] with n_planes, and three host tables per
 * plane (entry p - 1 is plane p): home int32, normal f64 [3], center int32 [3]; min_votes >= 1.
 *
 * 1. Home of a plane (bs_roof_homes).  home[p] = plane_building[p] if normal_z[p] >= min_normal_z (an f64 compare: NaN
 *    fails) && plane_building[p] >= 0 && 2 * votes_in[p] > votes_total[p]; otherwise -1.  A plane can be a roof only
 *    in the one building that holds the majority of its points.
 * 2. Vote.  Point i COUNTS iff !(z < ground_th) && 1 <= plane_idx[i] <= n_planes && home[plane_idx[i]] == map[pixel]
 *    >= 0, pixel = (x / bin, y / bin), the base pixel of bs_assign_buildings.  Per pixel the winner is the plane with
 *    the most counting points (ties: the lower id) if it has at least min_votes of them.
 *      roof[y][x]    = -1 where map is -1; the winner where there is one; 0 otherwise
 *      support[y][x] = the winner's count, else 0
 * 3. Fill, in synchronous rounds.  In round r every pixel with roof == 0 after round r - 1 looks at its 4-neighbours
 *    inside the image that have the same map value and roof > 0 after round r - 1; if there is one, it takes the
 *    smallest plane id among them.  Rounds run until one changes nothing; fill_rounds = the rounds that changed
 *    something.  A label moves one pixel per round (an in-place sweep gives another result).  The pixels of a
 *    building without a seed stay 0.
 * 4. Figures per plane.  A SUPPORTING point is a counting point whose plane_idx equals the final roof of its pixel.
 *      pixels (roof == p), seed_pixels (... and support > 0), the inclusive pixel bbox,
 *      n_support, z_min, z_max, z_sum over the supporting points;
 *    a plane without any: 0 for the counts, INT32_MAX / INT32_MIN for z_min / z_max and the bbox
 *    {INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN}.  Totals: seeded_pixels, filled_pixels, unroofed_pixels (roof == 0).
 * 5. Height H(p, X, Y) at integer millimetres X, Y, in f64 without contraction (n = normal[p], c = center[p]):
 *      t = nx * ((double)X - cx) + ny * ((double)Y - cy)      two rounded products, one sum
 *      z = (double)cz - t / nz
 *      if (!(z >= z_min[p])) z = z_min[p];
 *      if (z > z_max[p])     z = z_max[p];
 *      H = (int64) z
 *    The two comparisons in that order make NaN and +-inf harmless: nz <= 0 is not an error.
 *      height[y][x] = H(roof, x * bin + bin / 2, y * bin + bin / 2) (integer bin / 2) where roof > 0, INT32_MIN elsewhere.
 * Everything but the one division is an exact integer and independent of the order of summation. */
/* (no typedef: the host-memory entry point below has the struct's name, so the type is always `struct bs_roofs`) */
struct bs_roofs {
  int32_t n_planes;
  int32_t width, height;
  int32_t fill_rounds;     /* rounds of the fill that changed something */
  int64_t seeded_pixels;   /* pixels the vote gave a roof */
  int64_t filled_pixels;   /* pixels the fill gave a roof */
  int64_t unroofed_pixels; /* roof == 0: building pixels no seed reaches */
  /* per plane, entry p - 1 is plane p; host memory owned by the library */
  int64_t* pixels;      /* [n_planes] */
  int64_t* seed_pixels; /* [n_planes] */
  int32_t* bbox;        /* [n_planes][4] x0, y0, x1, y1 */
  int64_t* n_support;   /* [n_planes] */
  int32_t* z_min;       /* [n_planes] */
  int32_t* z_max;       /* [n_planes] */
  int64_t* z_sum;       /* [n_planes] */
  /* device time (HIP events on the context's stream) */
  double ms_vote;    /* keys, sort, run lengths, per-pixel arg-max, seeds */
  double ms_fill;    /* all rounds */
  double ms_figures; /* the point pass and the pixel pass */
  double ms_height;  /* the height pass (0 without d_height) */
};

/* Host only, no context.  normal [n_planes][3]; the other inputs and home_out are [n_planes].  BS_ERR_INVALID: a null
 * pointer with n_planes > 0, or n_planes < 0. */
int bs_roof_homes(const double* normal, const int32_t* plane_building, const int64_t* votes_in, const int64_t* votes_total,
                  int32_t n_planes, double min_normal_z, int32_t* home_out);

/* d_xyz, d_map, d_plane_idx, d_roof [height][width] int32, d_support [height][width] int32 (may be NULL) and d_height
 * [height][width] int32 (may be NULL) are device pointers; home, normal and center are host tables [n_planes] (not read
 * when n_planes == 0); out's arrays are host memory owned by the library (bs_roofs_free, which accepts a zeroed
 * struct).  n_planes == 0 is valid: roof is -1 or 0 and no per-plane array is touched.
 * BS_ERR_INVALID: null pointer, n < 1, bin < 1, width or height < 1 (or width * height >= 2^31), n_planes < 0,
 * min_votes < 1.  BS_ERR_RANGE: 2^29 points or more, or a point with a negative x / y or whose pixel lies outside the
 * image; d_roof, d_support and d_height are then left untouched.  A failed call leaves the context usable.
 * Synchronises. */
int bs_roofs_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t bin, double ground_th, const int32_t* d_map,
                 int32_t width, int32_t height, const int32_t* d_plane_idx, int32_t n_planes, const int32_t* home,
                 const double* normal, const int32_t* center, int32_t min_votes, int32_t* d_roof, int32_t* d_support,
                 int32_t* d_height, struct bs_roofs* out);
/* Host-memory variant: xyz, map, plane_idx, roof, support (may be NULL) and height (may be NULL) are host pointers. */
int bs_roofs(bs_ctx* ctx, const int32_t* xyz, int64_t n, int32_t bin, double ground_th, const int32_t* map,
             int32_t width, int32_t height, const int32_t* plane_idx, int32_t n_planes, const int32_t* home,
             const double* normal, const int32_t* center, int32_t min_votes, int32_t* roof, int32_t* support,
             int32_t* height_out, struct bs_roofs* out);
void bs_roofs_free(struct bs_roofs* r);

/* Roof surfaces in millimetres, one quad per run of pixels; the walls stay bs_buildings_write_obj's.  Host only: roof
 * and map are host arrays [height][width], r supplies z_min / z_max of the n_planes planes, normal and center are the
 * tables of bs_roofs.  origin [3] is the shift that was subtracted from the cloud (NULL: 0).  The file, every number a
 * decimal integer, every line ended by '\n':
 *   "# roof runs: <runs> over <planes with pixels > 0> planes"
 *   for y ascending, for every maximal run [x0, x1] of equal map >= 0 and equal roof >= 1 (x0 ascending), four lines
 *     "v X+origin[0] Y+origin[1] H(roof, X, Y)+origin[2]"
 *   for the corners (x0*bin, y*bin), ((x1+1)*bin, y*bin), ((x1+1)*bin, (y+1)*bin), (x0*bin, (y+1)*bin) in that order;
 *   after all vertices, for run r = 0 ..: "f 4r+1 4r+2 4r+3 4r+4".
 * BS_ERR_INVALID: null pointer, bin < 1, width or height < 1, a roof value above r->n_planes, or the file cannot be
 * written. */
int bs_roofs_write_obj(const int32_t* roof, const int32_t* map, int32_t width, int32_t height, const struct bs_roofs* r,
                       const double* normal, const int32_t* center, int32_t bin, const int32_t* origin, const char* path);

/* ---- plane fit: every plane's exact centroid, least-squares normal and residuals from the points that carry its label ----
 *
 * bs_segment reproduces the reference's plane record bit for bit, quirks included: its centre is a wrapping 32-bit sum
 * divided as unsigned (my_function.cpp:241-250) and its normal the mean of the per-point normals.  This stage recomputes
 * both from the labels, for everything that uses a plane as geometry (bs_roof_homes, bs_roofs, bs_roofs_write_obj).
 *
 * Inputs: xyz int32 [n][3] with 1 <= n < 2^29 and every |coordinate| < 2^23 (the domain of stages 1-2), plane_idx int32 [n],
 * n_planes >= 0.  A point belongs to plane p iff plane_idx == p and 1 <= p <= n_planes (by label, as in
 * bs_plane_buildings); every other label (-1, 0, n_planes + 1, ...) is ignored.
 *
 * Per plane (entry p - 1 is plane p):
 * 1. Sums.  n_points; S = sum of (x, y, z) in int64; the inclusive box bbox = {x0, y0, z0, x1, y1, z1}.  A plane without
 *    points gets INT32_MAX / INT32_MIN for the box.
 * 2. Centroid.  center[a] = S[a] / n_points in int64, C division (truncated towards zero); 0 when n_points == 0.
 * 3. Verdict.  D = the largest of hi[a] - center[a] and center[a] - lo[a] over the three axes.
 *      status = 1 if n_points < 3;
 *      status = 2 if 3 * n_points * D^2 >= 2^63 (evaluated exactly: D^2 >= ceil(2^63 / (3 * n_points)) in 64 bits).  This is
 *                 the condition under which every integer sum below fits in int64;
 *      status = 0 otherwise: fitted.
 * 4. Moments (status 0 only; zero otherwise).  With d_i = p_i - center:
 *      dev_sum[3] = sum of d                                   (= S - n_points * center, the remainder of the division)
 *      moment[6]  = sum of (dx*dx, dx*dy, dx*dz, dy*dy, dy*dz, dz*dz), all int64.
 * 5. Normal (status 0; otherwise (0, 0, 1)).  In f64 without contraction:
 *      dn = (double)n_points, e[a] = (double)dev_sum[a] / dn, C[ab] = (double)moment[ab] / dn - e[a] * e[b],
 *    then the smallest eigenvector of C by the solver of stage 2 (csrc/bs_normal.h: Eberly's FastEigen3x3 with
 *    bs_detmath.h), (0, 0, 1) if its norm is zero, flipped if z < 0: the tail of stage 2's normal, the same code.
 * 6. Residuals (status 0).  r_i = (int32)(int64)(nx * dx + (ny * dy + nz * dz)) in f64 without contraction, truncated.
 *    Per plane r_abs_max int32, r_abs_sum int64, r_sq_sum int64 (zero for the other planes).  The optional per-point
 *    output residual[i] is r_i for a point of a fitted plane and INT32_MIN for every other point.
 * Everything except the eigen-solve and the one dot product per point is an exact integer and independent of the order
 * of summation; the solve and the dot product are fixed sequences of IEEE operations, the same on the device and the host. */
struct bs_plane_fits {
  int32_t n_planes;
  /* per plane, entry p - 1 is plane p; host memory owned by the library */
  int32_t* status;    /* [n_planes] 0 fitted, 1 fewer than 3 points, 2 too large for the exact sums */
  int64_t* n_points;  /* [n_planes] */
  int32_t* center;    /* [n_planes][3] */
  double* normal;     /* [n_planes][3] */
  int32_t* bbox;      /* [n_planes][6] x0, y0, z0, x1, y1, z1 */
  int64_t* dev_sum;   /* [n_planes][3] */
  int64_t* moment;    /* [n_planes][6] xx, xy, xz, yy, yz, zz */
  int32_t* r_abs_max; /* [n_planes] */
  int64_t* r_abs_sum; /* [n_planes] */
  int64_t* r_sq_sum;  /* [n_planes] */
  /* device time (HIP events on the context's stream) */
  double ms_sums;      /* pass A over the points (count, S, box) and the per-plane centroid and verdict */
  double ms_moments;   /* pass B over the points (the six moments) */
  double ms_solve;     /* the per-plane covariance and eigen-solve */
  double ms_residuals; /* pass C over the points (residuals and their figures) */
};

/* d_xyz [n][3], d_plane_idx [n] and d_residual [n] int32 (may be NULL) are device pointers; out's arrays are host memory
 * owned by the library (bs_plane_fits_free, which accepts a zeroed struct); out is written whole on success (not freed
 * first).  n_planes == 0 is valid: no per-plane array is touched and every residual is INT32_MIN.
 * BS_ERR_INVALID: null pointer, n < 1, n_planes < 0.  BS_ERR_RANGE: n >= 2^29, or a coordinate of ANY point outside
 * |c| < 2^23; out and d_residual are then left untouched and the context stays usable.  Synchronises. */
int bs_plane_fit_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, const int32_t* d_plane_idx, int32_t n_planes,
                     int32_t* d_residual, struct bs_plane_fits* out);
/* Host-memory variant: xyz, plane_idx and residual (may be NULL) are host pointers. */
int bs_plane_fit(bs_ctx* ctx, const int32_t* xyz, int64_t n, const int32_t* plane_idx, int32_t n_planes, int32_t* residual,
                 struct bs_plane_fits* out);
void bs_plane_fits_free(struct bs_plane_fits* f);

/* Host only, no context: the bridge to bs_roof_homes / bs_roofs / bs_roofs_write_obj.  normal f64 [n_planes][3] and center
 * int32 [n_planes][3] are the tables of bs_segment's planes; row p - 1 of both is overwritten with the fit for every
 * plane with status 0, the other rows are left alone.  BS_ERR_INVALID: a null pointer (f, or a table / an array of f with
 * n_planes > 0), or n_planes < 0. */
int bs_plane_fit_apply(const struct bs_plane_fits* f, double* normal, int32_t* center);

/* ---- solids: a closed, oriented mesh per building (roof, walls, floor) from the roof image ----
 *
 * Inputs: map[height][width] (negative: outside, else a building in 0 .. n_buildings - 1) and roof[height][width] of
 * bs_roofs (<= 0: no roof plane, else 1 .. n_planes), the host tables normal / center / z_min / z_max per plane that
 * bs_roofs used and returned, bin, base_z, and a host table flat[n_buildings]: the top of a building's unroofed pixels.
 * Everything is an integer millimetre; the mesh is exact to the pixel.
 *
 * 1. Tops.  Pixel (x, y) of building c has four corner heights t[j][i] at the lattice corners (x + i, y + j):
 *      roof > 0:   max(base_z, H(roof, (x + i) * bin, (y + j) * bin)), H the height function of the roof stage (step 5
 *                  there: the same f64 sequence and clamps);
 *      otherwise:  max(base_z, flat[c]).
 *    top[y][x] = {t00, t10, t01, t11} (tij: i along x), {INT32_MIN x 4} where map < 0.
 * 2. Vertices.  A lattice corner (X, Y) and a building c with a pixel incident to it carry one vertex for every distinct
 *    value of {base_z} and the tops of c's incident pixels at that corner: int32 [4] {X * bin, Y * bin, Z, c}, ordered by
 *    ascending (Y, X, c, Z).  A corner carries at most 8.
 * 3. Faces.  For every pixel with map >= 0 in row-major order, vertices named (corner, height), counter-clockwise seen
 *    from above:
 *      top triangles (00, 10, 11) and (00, 11, 01) at the top heights;
 *      the floor quad (00, 01, 11, 10) at base_z;
 *      one wall per directed top edge s -> e, in the order 00->10 (neighbour y - 1), 10->11 (x + 1), 11->01 (y + 1),
 *      01->00 (x - 1).  a_s, a_e are the pixel's tops at s and e; b_s, b_e the neighbour's tops at the same corners if it
 *      lies inside the image and belongs to the same building, else both base_z.  The wall exists iff
 *      (a_s, a_e) != (b_s, b_e); between two pixels of one building only the one with the smaller row-major index emits
 *      it (on its x + 1 and y + 1 edges).  It is the polygon
 *        (e, a_e), (s, a_s), the vertices of (s, c) strictly between a_s and b_s walking from a_s, (s, b_s), (e, b_e),
 *        the vertices of (e, c) strictly between b_e and a_e walking from b_e
 *      with (s, b_s) left out when b_s == a_s and (e, b_e) when b_e == a_e: 3 to 8 vertices.  A wall with a_s - b_s and
 *      a_e - b_e of opposite signs is a CROSSING wall: it is emitted as this one polygon (a bow-tie in a vertical plane)
 *      and counted.
 *    face_offset int32 [n_faces + 1], face_index int32 [n_indices] (vertex numbers from 0), face_building int32 [n_faces],
 *    face_kind uint8 [n_faces]: 0 top, 1 floor, 2 wall.
 * 4. Figures per building: pixels, vertices, faces, wall_faces, crossing_walls, top_min / top_max over its tops
 *    (INT32_MAX / INT32_MIN without a pixel) and volume6 = the sum over its pixels of 2 t00 + 2 t11 + t10 + t01 - 6 base_z;
 *    the volume in mm^3 is volume6 * bin^2 / 6 (the fixed diagonal 00-11 makes it exact).  And their totals.
 * Every directed edge of the mesh occurs exactly as often as its reverse, per building: the mesh is closed and oriented.
 * It is not always manifold (diagonal contact and alternating heights put four faces on one vertical edge). */
/* (no typedef: the host-memory entry point below has the struct's name, so the type is always `struct bs_solids`) */
struct bs_solids {
  int32_t n_buildings;
  int32_t width, height;
  int32_t bin, base_z;
  int64_t n_pixels, n_vertices, n_faces, n_indices, n_wall_faces, n_crossing_walls, total_volume6; /* totals */
  /* per building; host memory owned by the library */
  int64_t* pixels;         /* [n_buildings] */
  int64_t* vertices;       /* [n_buildings] */
  int64_t* faces;          /* [n_buildings] */
  int64_t* wall_faces;     /* [n_buildings] */
  int64_t* crossing_walls; /* [n_buildings] */
  int32_t* top_min;        /* [n_buildings] */
  int32_t* top_max;        /* [n_buildings] */
  int64_t* volume6;        /* [n_buildings] */
  /* the mesh, host memory owned by the library: filled by the host-memory entry point only (NULL after the count) */
  int32_t* vertex;        /* [n_vertices][4] */
  int32_t* face_offset;   /* [n_faces + 1] */
  int32_t* face_index;    /* [n_indices] */
  int32_t* face_building; /* [n_faces] */
  uint8_t* face_kind;     /* [n_faces] */
  /* device time (HIP events on the context's stream) */
  double ms_tops;     /* the corner heights */
  double ms_vertices; /* vertices per corner */
  double ms_faces;    /* faces and indices per pixel */
  double ms_figures;  /* the per-building figures */
  double ms_scans;    /* the three exclusive sums */
  double ms_emit_vertices, ms_emit_faces; /* the two passes of the emit (host-memory entry point only) */
};

/* Tops, counts and figures.  d_map, d_roof and d_top ([height][width][4] int32, may be NULL) are device pointers; the
 * plane tables (not read when n_planes == 0) and flat (not read when n_buildings == 0) are host arrays.  The offsets
 * stay in the context for the emit below; out's per-building arrays are host memory owned by the library
 * (bs_solids_free, which accepts a zeroed struct).
 * BS_ERR_INVALID: null pointer, width or height < 1 (or (width + 1) * (height + 1) >= 2^31), n_buildings or n_planes < 0,
 * bin < 1.  BS_ERR_RANGE: a map value >= n_buildings, a roof value > n_planes, roof > 0 where map < 0, or 2^31 or more
 * vertices or indices; d_top is then left untouched.  A failed call leaves the context usable.  Synchronises. */
int bs_solids_count_dev(bs_ctx* ctx, const int32_t* d_map, const int32_t* d_roof, int32_t width, int32_t height,
                        int32_t n_buildings, int32_t n_planes, const double* normal, const int32_t* center,
                        const int32_t* z_min, const int32_t* z_max, int32_t bin, int32_t base_z, const int32_t* flat,
                        int32_t* d_top, struct bs_solids* out);
/* The mesh of the last successful count on this context into device buffers of exactly its sizes: d_vertex
 * [n_vertices][4], d_face_offset [n_faces + 1], d_face_index [n_indices], d_face_building and d_face_kind [n_faces] (a
 * pointer to an array of no element may be NULL).  May be called more than once; the map and roof of the count are not
 * read again.  BS_ERR_INVALID: null pointer, or no successful count (the last one on this context failed, or there was
 * none).  Synchronises. */
int bs_solids_emit_dev(bs_ctx* ctx, int32_t* d_vertex, int32_t* d_face_offset, int32_t* d_face_index,
                       int32_t* d_face_building, uint8_t* d_face_kind);
/* Host-memory twin: map, roof and top ([height][width][4], may be NULL) are host pointers; both steps, and the mesh
 * comes back in out's library-owned arrays. */
int bs_solids(bs_ctx* ctx, const int32_t* map, const int32_t* roof, int32_t width, int32_t height, int32_t n_buildings,
              int32_t n_planes, const double* normal, const int32_t* center, const int32_t* z_min, const int32_t* z_max,
              int32_t bin, int32_t base_z, const int32_t* flat, int32_t* top, struct bs_solids* out);
void bs_solids_free(struct bs_solids* s);

/* The mesh as an OBJ in millimetres.  Host only, no context: the five arrays are host memory.  origin [3] is the shift
 * that was subtracted from the cloud (NULL: 0).  The file, every number a decimal integer, every line ended by '\n':
 *   "# solids: <buildings with faces> buildings, <n_vertices> vertices, <n_faces> faces"
 *   for every vertex in order "v X+origin[0] Y+origin[1] Z+origin[2]"
 *   for every building c with faces, ascending: "o building_<c>", then its faces in face order (a stable counting sort
 *   by building), each "f i j k ..." with the vertices numbered from 1.
 * BS_ERR_INVALID: null pointer, a negative count, face_offset that does not start at 0 or decreases, a vertex number
 * outside [0, n_vertices), a building outside [0, n_buildings), or the file cannot be written. */
int bs_solids_write_obj(const int32_t* vertex, int64_t n_vertices, const int32_t* face_offset, const int32_t* face_index,
                        const int32_t* face_building, int64_t n_faces, int32_t n_buildings, const int32_t* origin,
                        const char* path);

/* ---- roof facets: the roof faces of every building and the edges between them (the roof topology graph) ----
 *
 * Inputs: map[height][width] (negative: outside, else a building in 0 .. n_buildings - 1), roof[height][width] of bs_roofs
 * (<= 0: no roof plane, else 1 .. n_planes) and top[height][width][4] = {t00, t10, t01, t11} as bs_solids_count_dev writes
 * it (tij at lattice corner (x + i, y + j)); top is read only where map >= 0.  The plane of a building pixel is
 * P = roof > 0 ? roof : 0; plane 0 is "unroofed".
 *
 * 1. Facets.  A facet is a 4-connected component of building pixels with equal (map, P).  Its start pixel is its first
 *    pixel in raster order.  Facets are numbered from 0 in ASCENDING order of start pixel (the buildings of
 *    bs_building_map are numbered in DESCENDING order of theirs: the contour order).  facet[y][x] is the facet of the
 *    pixel, -1 where map < 0.  Two pixels of equal (map, P) that touch only diagonally are different facets; adjacent
 *    pixels of different buildings are never joined, even under the same plane.
 * 2. Pixel edges.  For pixel A = (x, y) with map >= 0 look at B = (x + 1, y) (direction 0) and B = (x, y + 1)
 *    (direction 1).  The edge is a BORDER edge iff B is inside the image, map[B] == map[A] and facet[B] != facet[A]; it is
 *    numbered 2 * (y * width + x) + direction.  Any of the four sides of a pixel whose other side is outside the image,
 *    has map < 0 or belongs to another building is an OUTER edge of the pixel's facet.
 * 3. Heights of a border edge, all in int64.  The shared corners are s and e:
 *      direction 0: s = (x + 1, y), e = (x + 1, y + 1); a_s = A.t10, a_e = A.t11, b_s = B.t00, b_e = B.t01;
 *                   s_A = (A.t10 + A.t11) - (A.t00 + A.t01), s_B the same expression on B;
 *      direction 1: s = (x, y + 1), e = (x + 1, y + 1); a_s = A.t01, a_e = A.t11, b_s = B.t00, b_e = B.t10;
 *                   s_A = (A.t01 + A.t11) - (A.t00 + A.t10), s_B the same expression on B.
 *    bend = s_A - s_B: positive where the surface falls away across the edge (convex: a ridge), negative in a valley; it
 *    does not depend on which facet has the lower id.
 * 4. Edges.  An edge is an unordered pair of facets with at least one border edge between them; edges are listed in
 *    ascending (facet_lo, facet_hi).  Per edge: facet[2] = {lo, hi}, building, length (its border edges), n_dir0 (those of
 *    direction 0), n_step (those with (a_s, a_e) != (b_s, b_e): exactly the pixel edges where the solids put an inner
 *    wall), step_abs_sum = sum of |a_s - b_s| + |a_e - b_e|, step_abs_max = the largest single |a - b|, rise_sum = sum of
 *    (h_s - l_s) + (h_e - l_e) with h the side of facet_hi and l the side of facet_lo (signed), bend_sum = sum of bend,
 *    z_min / z_max over all a_s, a_e, b_s, b_e, and bbox[4] = {X0, Y0, X1, Y1}: the inclusive box of the lattice corners s
 *    and e of its border edges, in lattice units.
 * 5. Per facet: building, plane, start_xy[2], pixels, bbox[4] (inclusive pixel box {x0, y0, x1, y1}), inner_edges (border
 *    edges it takes part in), outer_edges, top_min / top_max over the four tops of its pixels, top_sum (all four tops of
 *    every pixel).
 * 6. Totals: n_facets, n_edges, n_pixels, n_border (= the sum of length).
 * Everything is an exact integer and independent of the order of summation. */
/* (no typedef: the host-memory entry point below has the struct's name, so the type is always `struct bs_roof_facets`) */
struct bs_roof_facets {
  int32_t width, height;
  int64_t n_facets, n_edges, n_pixels, n_border; /* totals */
  /* per facet; host memory owned by the library */
  int32_t* facet_building;    /* [n_facets] */
  int32_t* facet_plane;       /* [n_facets] */
  int32_t* facet_start_xy;    /* [n_facets][2] */
  int64_t* facet_pixels;      /* [n_facets] */
  int32_t* facet_bbox;        /* [n_facets][4] */
  int64_t* facet_inner_edges; /* [n_facets] */
  int64_t* facet_outer_edges; /* [n_facets] */
  int32_t* facet_top_min;     /* [n_facets] */
  int32_t* facet_top_max;     /* [n_facets] */
  int64_t* facet_top_sum;     /* [n_facets] */
  /* per edge; host memory owned by the library */
  int32_t* edge_facet;        /* [n_edges][2] */
  int32_t* edge_building;     /* [n_edges] */
  int64_t* edge_length;       /* [n_edges] */
  int64_t* edge_n_dir0;       /* [n_edges] */
  int64_t* edge_n_step;       /* [n_edges] */
  int64_t* edge_step_abs_sum; /* [n_edges] */
  int64_t* edge_step_abs_max; /* [n_edges] */
  int64_t* edge_rise_sum;     /* [n_edges] */
  int64_t* edge_bend_sum;     /* [n_edges] */
  int32_t* edge_z_min;        /* [n_edges] */
  int32_t* edge_z_max;        /* [n_edges] */
  int32_t* edge_bbox;         /* [n_edges][4] */
  /* device time (HIP events on the context's stream) */
  double ms_label;   /* tiles, seams, flatten */
  double ms_number;  /* roots scanned, the facet image */
  double ms_figures; /* the per-facet figures and the border flags */
  double ms_edges;   /* keys, sort, run heads, the per-edge figures */
};

/* d_map, d_roof, d_top ([height][width][4] int32) and d_facet ([height][width] int32, written) are device pointers; out's
 * arrays are host memory owned by the library (bs_roof_facets_free, which accepts a zeroed struct).  An image without a
 * building pixel is valid: 0 facets, 0 edges, facet -1 everywhere.
 * BS_ERR_INVALID: null pointer, width or height < 1, width * height >= 2^30 (the number of a pixel edge fits 31 bits),
 * n_buildings or n_planes < 0, or d_top not 16-byte aligned (every device allocation is).  BS_ERR_RANGE: a map value >= n_buildings, a roof value > n_planes, or roof > 0 where
 * map < 0 (the checks of bs_solids_count_dev).  On any error d_facet and out are left untouched, and the context stays
 * usable.  Synchronises. */
int bs_roof_facets_dev(bs_ctx* ctx, const int32_t* d_map, const int32_t* d_roof, const int32_t* d_top, int32_t width,
                       int32_t height, int32_t n_buildings, int32_t n_planes, int32_t* d_facet, struct bs_roof_facets* out);
/* Host-memory twin: map, roof, top and facet are host pointers. */
int bs_roof_facets(bs_ctx* ctx, const int32_t* map, const int32_t* roof, const int32_t* top, int32_t width, int32_t height,
                   int32_t n_buildings, int32_t n_planes, int32_t* facet, struct bs_roof_facets* out);
void bs_roof_facets_free(struct bs_roof_facets* f);

/* The kind of every edge into kind_out [n_edges].  Host only, no context.  In int64:
 *   3 STEP    if step_abs_sum > 2 * step_tol * length,
 *   1 RIDGE   else if bend_sum > bend_tol * length,
 *   2 VALLEY  else if bend_sum < -bend_tol * length,
 *   0 FLAT    otherwise.
 * step_tol is the mean height difference in millimetres along the border; bend_tol is in the units of bend: twice the
 * change of rise per pixel.  BS_ERR_INVALID: null pointer or a negative tolerance. */
int bs_roof_edge_kinds(const struct bs_roof_facets* f, int32_t step_tol, int32_t bend_tol, uint8_t* kind_out);

/* The border edges as an OBJ of line segments in millimetres.  Host only, no context: facet, map and top are host
 * images, kind [n_edges] the kinds above, origin [3] the shift that was subtracted from the cloud (NULL: 0).  The border
 * edges are found from facet and map and grouped by edge with a stable counting sort.  The file, every number a decimal
 * integer, every line ended by '\n':
 *   "# roof edges: <n_edges> edges, <n_border> segments"
 *   for every edge e ascending: "g edge_<e>_<flat|ridge|valley|step>", then for each of its border edges in ascending
 *   (y, x, direction) of pixel A three lines: "v X*bin+origin[0] Y*bin+origin[1] Z+origin[2]" for corner s and for corner
 *   e, with Z = max(a, b) at that corner, and "l i j" with the vertices numbered from 1 in file order.
 * BS_ERR_INVALID: null pointer (origin apart), bin < 1, width or height < 1, a kind above 3, a facet pair the struct
 * does not list, or the file cannot be written. */
int bs_roof_edges_write_obj(const int32_t* facet, const int32_t* map, const int32_t* top, int32_t width, int32_t height,
                            int32_t bin, const struct bs_roof_facets* f, const uint8_t* kind, const int32_t* origin,
                            const char* path);

/* ---- roof generalisation: small facets and facets across a FLAT edge merged into their neighbours ----
 *
 * A step between bs_roofs and bs_solids_count_dev: its output is a new roof image, and every later stage runs on it
 * unchanged.  Inputs are those of bs_solids_count_dev: map, roof, width, height, n_buildings, n_planes, the host tables
 * normal / center / z_min / z_max, bin, base_z and flat; and the parameters below.  The plane of a building pixel is
 * P = roof > 0 ? roof : 0.
 *
 * The state is an image R, R0 = roof.  An EVALUATION of R is:
 * 1. T = the tops of (map, R): step 1 of the solids, with the same H, the same clamps and the same flat.
 * 2. The facets and edges of (map, R, T) exactly as "roof facets" defines them: ids by ascending start pixel, pixels,
 *    plane, building, and per edge length, step_abs_sum and bend_sum.
 * 3. kind(e) by the rule of bs_roof_edge_kinds(step_tol, bend_tol).
 * 4. g OUTRANKS f iff pixels[g] > pixels[f], or they are equal and g < f.
 * 5. A neighbour g of f (an edge {f, g} exists) is a CANDIDATE of f iff plane[g] > 0, g outranks f, and
 *    pixels[f] < min_pixels or (merge_flat and kind == FLAT).  Its reason is FLAT when merge_flat and the edge is FLAT,
 *    else SMALL.
 * 6. target[f] is the candidate with the largest length; among equals the one that outranks the others.  A facet without
 *    a candidate STAYS; every other facet MOVES.
 * 7. end[f] = f if f stays, else end[target[f]].  Ranks rise strictly along a chain, so chains are finite and acyclic.
 *    The chain of f has as many links as there are moves from f to end[f]; longest_chain is the largest (0 without a mover).
 * 8. movers is the number of facets that move; movers_small / movers_flat split it by the reason of the target.
 * APPLYING an evaluation gives R': a pixel of a moving facet f gets plane[end[f]] (always > 0); every other pixel keeps its
 * value bit for bit, -1 and 0 included.
 *
 * The call runs evaluations r = 1, 2, ..., max_rounds + 1.  An evaluation with movers == 0 ends it (converged = 1);
 * evaluation max_rounds + 1 is never applied (converged = 0 if it has movers); every other evaluation is applied.  rounds is
 * the number of applied evaluations, so there are rounds + 1 evaluations and the last one is always of the final image.
 * max_rounds = 0 only reports.  Every moving chain joins one connected region of one plane, so the facet count falls by at
 * least movers in each applied round and the loop ends without the cap.
 *
 * Consequences.  Pixels of different buildings never merge (no edge between them).  Diagonal contact is no edge.  An
 * unroofed facet (plane 0) is never a target, but it can move and become roofed.  min_pixels <= 1 with merge_flat == 0
 * returns the input with rounds == 0.  A converged output run again with the same parameters returns itself with
 * rounds == 0.  Everything is an exact integer except the division inside H, which the roof stage pins. */
struct bs_roof_generalise_params {
  int64_t min_pixels; /* facets with fewer pixels look for a neighbour; 0 or 1: none */
  int32_t merge_flat; /* != 0: a facet also moves across a FLAT edge */
  int32_t step_tol;   /* of bs_roof_edge_kinds */
  int32_t bend_tol;   /* of bs_roof_edge_kinds */
  int32_t max_rounds; /* applied evaluations at most */
};

#define BS_GEN_FIG_CAP 1024   /* buildings 0 .. cap - 1: per-building figures reduced in LDS, global atomics from the cap on */
#define BS_GEN_PLANE_CAP 1024 /* planes 0 .. cap - 1 (0 = unroofed): pixel counts in LDS, global atomics from the cap on */

/* (no typedef: the host-memory entry point below has the struct's name, so the type is always `struct bs_roof_generalise`) */
struct bs_roof_generalise {
  int32_t width, height, n_buildings, n_planes;
  int32_t rounds, converged;
  /* "in": the first evaluation, "out": the last.  n_flat: FLAT edges; n_small: facets below min_pixels */
  int64_t n_facets_in, n_facets_out, n_edges_in, n_edges_out, n_flat_in, n_flat_out, n_small_in, n_small_out;
  int64_t pixels_changed; /* pixels whose output value differs from the input */
  int64_t pixels_roofed;  /* of those: P was 0 and is now > 0 */
  /* per evaluation [rounds + 1]; host memory owned by the library */
  int64_t* eval_facets;
  int64_t* eval_movers;
  int64_t* eval_movers_small;
  int64_t* eval_movers_flat;
  int64_t* eval_longest_chain;
  /* per plane [n_planes + 1], entry 0 = unroofed: building pixels with that P */
  int64_t* plane_pixels_in;
  int64_t* plane_pixels_out;
  /* per building [n_buildings].  dtop = |T_last - T_first| over the four corners of every pixel of the building, T_first
   * and T_last the tops of the first and the last evaluation: what min_pixels and the tolerances are chosen by */
  int64_t* building_facets_in;
  int64_t* building_facets_out;
  int64_t* building_pixels_changed;
  int64_t* building_sum_abs_dtop;
  int64_t* building_max_abs_dtop;
  /* device time (HIP events on the context's stream), summed over the evaluations */
  double ms_tops;    /* step 1 */
  double ms_facets;  /* step 2, the read-backs of its sizes included */
  double ms_decide;  /* steps 3 to 8 */
  double ms_apply;   /* the applied rounds */
  double ms_figures; /* the per-plane and per-building figures, once */
};

/* d_map, d_roof and d_roof_out ([height][width] int32, written; it may be d_roof) are device pointers, the tables and flat
 * host arrays as for bs_solids_count_dev; out's arrays are host memory owned by the library (bs_roof_generalise_free, which
 * accepts a zeroed struct).  The stage works in scratch of its own: it does not disturb what bs_solids_count_dev,
 * bs_roof_facets_dev or any *_count_dev left on the context for its *_emit_dev, and it keeps no state itself.
 * BS_ERR_INVALID: null pointer, width or height < 1, width * height >= 2^30 or (width + 1) * (height + 1) >= 2^31,
 * n_buildings or n_planes < 0, bin < 1, or a negative parameter.  BS_ERR_RANGE: a map value >= n_buildings, a roof value >
 * n_planes, or roof > 0 where map < 0.  On any error d_roof_out and out are left untouched and the context stays usable.
 * Synchronises. */
int bs_roof_generalise_dev(bs_ctx* ctx, const int32_t* d_map, const int32_t* d_roof, int32_t width, int32_t height,
                           int32_t n_buildings, int32_t n_planes, const double* normal, const int32_t* center,
                           const int32_t* z_min, const int32_t* z_max, int32_t bin, int32_t base_z, const int32_t* flat,
                           const struct bs_roof_generalise_params* params, int32_t* d_roof_out,
                           struct bs_roof_generalise* out);
/* Host-memory twin: map, roof and roof_out (may be roof) are host pointers. */
int bs_roof_generalise(bs_ctx* ctx, const int32_t* map, const int32_t* roof, int32_t width, int32_t height,
                       int32_t n_buildings, int32_t n_planes, const double* normal, const int32_t* center,
                       const int32_t* z_min, const int32_t* z_max, int32_t bin, int32_t base_z, const int32_t* flat,
                       const struct bs_roof_generalise_params* params, int32_t* roof_out, struct bs_roof_generalise* out);
void bs_roof_generalise_free(struct bs_roof_generalise* g);

/* ---- facet outlines: every label of a label image as polygon rings with holes ----
 *
 * Input: label[height][width] of int32, negative = outside, else 0 .. n_labels - 1; in the pipeline the facet image of
 * bs_roof_facets.  The definition holds for any label image; the identities marked (*) need every label to be one
 * 4-connected component, which the facet image guarantees.  Optionally top[height][width][4] = {t00, t10, t01, t11} as
 * bs_solids_count_dev writes it.
 *
 * Corners and directions.  Lattice corners are (X, Y) with 0 <= X <= width, 0 <= Y <= height.  delta[0] = (0, -1),
 * delta[1] = (1, 0), delta[2] = (0, 1), delta[3] = (-1, 0).  in(r, p): r is inside the image and label[r] == label[p].
 *
 * Half-edges.  Pixel p = (x, y) with label >= 0 has four sides, walked counter-clockwise seen from above (the order of the
 * solids' walls): side 0 (x, y) -> (x + 1, y), side 1 (x + 1, y) -> (x + 1, y + 1), side 2 (x + 1, y + 1) -> (x, y + 1),
 * side 3 (x, y + 1) -> (x, y).  Side k is a half-edge iff !in(p + delta[k], p); its number is h = 4 * (y * width + x) + k.
 * A half-edge has a pixel of its label on its left and none on its right.
 *
 * Successor.  For half-edge (p, k) let p' = p + delta[(k + 1) % 4] and q = p' + delta[k].
 *   If !in(p', p):      succ = (p, (k + 1) % 4)   (a left turn, it stays on the pixel);
 *   else if !in(q, p):  succ = (p', k)            (straight on);
 *   else                succ = (q, (k + 3) % 4)   (a right turn).
 * The first rule wins where two pixels of one label touch only diagonally, so a ring never crosses itself; it may visit
 * such a corner twice.  succ is a bijection on the half-edges, and its cycles are the rings.
 *
 * Vertices.  A half-edge g is a vertex iff its predecessor has another side number; locally, with a = p + delta[(k + 3) % 4]
 * and b = a + delta[k]: iff !in(a, p) || in(b, p).  The vertex is g's start corner.  With top its Z is the top of g's own
 * pixel at that corner (all pixels of one facet agree on it); without top there is no Z.
 *
 * Rings.  The start of a ring is its lowest half-edge number h0 (not always a vertex: the ring of a hole two pixels wide
 * starts in the middle of a straight run).  The vertex list of a ring holds its vertex half-edges in walk order from h0,
 * beginning with the first vertex at or after h0.  Rings are listed by ascending (label, h0).  Per ring: ring_label,
 * ring_start (h0), ring_length (its half-edges), ring_vertices, ring_area2 = the sum of Xs * Ye - Xe * Ys over its
 * half-edges s -> e in int64 (twice the signed area: positive for an outer ring, negative for a hole), ring_bbox[4] =
 * {X0, Y0, X1, Y1}, the inclusive box of its lattice corners, and ring_offset[n_rings + 1] into the vertex arrays.  Per
 * label: label_ring_offset[n_labels + 1]; the rings of a label are contiguous.  Totals: n_half, n_rings, n_vertices.
 * Vertex arrays: xy int32 [n_vertices][2] in lattice units, z int32 [n_vertices] only with top.
 * Everything is an exact integer and independent of the order of summation.
 *
 * Identities.  The sum of ring_length is n_half.  The sum of ring_area2 over a label is twice its pixels.  Every ring has
 * an even number of vertices, at least 4.  (*) The first ring of a label is its only ring with positive area.  (*) The
 * ring_start of that ring is 4 * (the label's first pixel in raster order).  (*) With the facet image, the sum of
 * ring_length over facet f is facet_inner_edges[f] + facet_outer_edges[f] of bs_roof_facets. */
struct bs_outlines {
  int32_t width, height;
  int32_t n_labels;
  int32_t has_z; /* the count had a top image */
  int64_t n_half, n_rings, n_vertices; /* totals */
  /* per ring; host memory owned by the library */
  int32_t* ring_label;    /* [n_rings] */
  int32_t* ring_start;    /* [n_rings] */
  int64_t* ring_length;   /* [n_rings] */
  int64_t* ring_vertices; /* [n_rings] */
  int64_t* ring_area2;    /* [n_rings] */
  int32_t* ring_bbox;     /* [n_rings][4] */
  int64_t* ring_offset;   /* [n_rings + 1] */
  /* per label */
  int64_t* label_ring_offset; /* [n_labels + 1] */
  /* the vertices, host memory owned by the library: filled by the host-memory entry point only (NULL after the count) */
  int32_t* xy; /* [n_vertices][2] */
  int32_t* z;  /* [n_vertices], NULL without top */
  /* device time (HIP events on the context's stream) */
  double ms_halfedges; /* side flags, their exclusive sum, numbers, successors, vertex flags */
  double ms_leaders;   /* the doubling rounds */
  double ms_rank;      /* the cut and the Wyllie rounds */
  double ms_rings;     /* slots, figures, sort, offsets, the place of every vertex */
  double ms_emit;      /* the emit (host-memory entry point only) */
};

/* Rings, figures and sizes.  d_label and d_top ([height][width][4] int32, may be NULL: no Z) are device pointers.  The
 * half-edges and the place of every vertex stay in the context for the emit below; out's arrays are host memory owned by
 * the library (bs_outlines_free, which accepts a zeroed struct).  An image without a labelled pixel is valid: 0 rings,
 * every offset 0.
 * BS_ERR_INVALID: null pointer, width or height < 1, width * height >= 2^29 (a half-edge number fits 31 bits; refused from
 * the arguments, before anything is read), n_labels < 0, or d_top not 16-byte aligned.  BS_ERR_RANGE: a label >= n_labels.
 * On any error out is left untouched, and the context stays usable.  Synchronises (three times: n_half, n_rings,
 * n_vertices; once without a labelled pixel). */
int bs_facet_outlines_count_dev(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width, int32_t height,
                                int32_t n_labels, struct bs_outlines* out);
/* The vertices of the last successful count on this context into device buffers of exactly its sizes: d_xy
 * [n_vertices][2], d_z [n_vertices] (NULL iff the count had no top; with no vertex both may be NULL).  May be called more
 * than once; the images of the count are not read again.  BS_ERR_INVALID: no successful count (the last one on this
 * context failed, or there was none), d_xy NULL, or d_z given or missing against the count.  Synchronises. */
int bs_facet_outlines_emit_dev(bs_ctx* ctx, int32_t* d_xy, int32_t* d_z);
/* Host-memory twin: label and top (may be NULL) are host pointers; both steps, and the vertices come back in out's
 * library-owned xy and z. */
int bs_facet_outlines(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height,
                      int32_t n_labels, struct bs_outlines* out);
void bs_outlines_free(struct bs_outlines* o);

/* The rings as an OBJ of closed polylines in millimetres.  Host only, no context: o with its xy (and z, or NULL) as the
 * host-memory entry point fills them; origin [3] is the shift that was subtracted from the cloud (NULL: 0).  The file,
 * every number a decimal integer, every line ended by '\n':
 *   "# facet outlines: <n_labels> labels, <n_rings> rings, <n_vertices> vertices"
 *   for every ring r in order: "g label_<l>_ring_<i>_<outer|hole>" with l its label, i = r - label_ring_offset[l] its
 *   number within the label, outer iff ring_area2 > 0; then its vertices "v X*bin+origin[0] Y*bin+origin[1] Z+origin[2]"
 *   (Z = 0 without z); then one closed polyline "l i1 ... in i1", the vertices numbered from 1 in file order.
 * BS_ERR_INVALID: null pointer (origin and z apart), bin < 1, a negative count, ring_offset that does not run from 0 to
 * n_vertices without decreasing, a ring_label outside [0, n_labels) or before its label's first ring, or the file cannot
 * be written. */
int bs_outlines_write_obj(const struct bs_outlines* o, int32_t bin, const int32_t* origin, const char* path);

/* ---- simplified outlines: the facet outlines cut into shared arcs, every arc simplified by an exact Douglas-Peucker ----
 *
 * Everything builds on "facet outlines" above: the label image, half-edges 4 * pixel + side, the successor rule, rings, h0
 * and the ring order (label, h0) are the same, and so are the ring count and label_ring_offset.  "Outside" below means
 * outside the image or a negative label; both count as the single label -1.
 *
 * Junctions.  The block of a lattice corner (X, Y) is the four pixels (X-1, Y-1), (X, Y-1), (X-1, Y), (X, Y).  A corner is
 * a junction iff its block holds three or more distinct labels, or is the saddle a b / b a with a != b.  At every other
 * corner that lies on a boundary exactly two labels meet along a simple curve, and the rings of both pass through it once,
 * in opposite directions.  (A ring passes exactly one junction only at a saddle: its right label can change only at a
 * junction and has to change back.)
 *
 * Nodes.  A half-edge is a node iff it is a vertex (the rule above) or its start corner is a junction; in the second case
 * it is a junction node.  A junction can lie in the middle of a straight run (a a / b c seen from a).  A node's position is
 * its start corner, its corner index Y * (width + 1) + X, its Z (with top) the top of its own pixel at that corner, its
 * right label the label across the half-edge, -1 for outside.
 *
 * Arcs.  A ring with junction nodes is cut at each of them: an arc runs from one junction node to the next in walk order,
 * both ends included.  A ring with exactly one junction node is one arc from that node round to itself.  A ring with no
 * junction node is one arc that starts and ends at its node with the lowest corner index (such a ring visits no corner
 * twice, so that node is unique).  The right label is constant along an arc.  An arc with right label B >= 0 is, corner for
 * corner in reverse, an arc of B's rings with the ring's own label on its right; every choice below is symmetric under
 * that reversal.
 *
 * Tolerance.  A rational tol2 = num / den in lattice units squared, 0 <= num < 2^31, 1 <= den < 2^31.  For a segment
 * S -> E and a node P, c = cross(E - S, P - S) is twice the triangle's area, in int64; |c| <= 2 * width * height < 2^30.
 * len2 = |E - S|^2.  P is farther than the tolerance iff c^2 * den > num * len2, evaluated exactly (the products reach 2^91:
 * 128 bits on the device).
 *
 * Douglas-Peucker on an arc.  The end nodes are kept.  A split of a segment S -> E: among the nodes strictly between the
 * ends take the one with the greatest c^2, ties to the lowest corner index; keep it and split both parts iff it is farther
 * than the tolerance, otherwise drop all nodes in between.  If the end corner differs from the start corner the arc is
 * split in this way, except that its FIRST split is made whatever the tolerance, provided its greatest c^2 is above 0.
 * (Without this a ring with exactly two junction nodes -- two open arcs -- would become those two nodes beyond a tolerance
 * of its width.  A rule per ring could not be symmetric under the reversal of a shared arc; this rule is per arc.  Its
 * price is one vertex on every arc that is not straight, however small its deviation.)  If the end corner equals the start
 * corner S (a ring without junctions or with one, or a lobe at a saddle): keep the node F with the greatest squared
 * distance from S, ties to the lowest corner index; each of the two parts S..F and F..S makes its first split whatever the
 * tolerance, provided its greatest c^2 is above 0; below that first split the tolerance decides as above.  So no ring
 * collapses to a line: every ring keeps at least 3 vertices, and one pixel keeps its four corners.  With num = 0 exactly the nodes are kept, and s_ring_area2
 * equals ring_area2.
 *
 * Result.  Per ring r of the plain outlines: s_ring_vertices, the kept nodes in walk order beginning with the first kept
 * node at or after h0; s_ring_area2, the shoelace sum over them in int64; s_ring_arcs; s_ring_offset[n_rings + 1].  Per
 * kept vertex: sxy[.][2]; sz (with top); s_right, the right label of the segment that starts there; s_flag, bit 0 junction
 * node, bit 1 the arc start of a ring without junctions.  Totals: n_nodes, n_junction_nodes, n_arcs, n_svertices; rounds,
 * the depth of the deepest split that kept a node (the device counts its synchronous rounds that kept something; the
 * choice of F is no round); max_arc_nodes, the largest node count of an arc with both ends included (a whole ring counts
 * its start twice).  ring_label, ring_area2 and label_ring_offset are copies of the plain outlines' for the writer.
 *
 * Promised: neighbouring facets share their simplified boundary exactly -- every segment with s_right = B >= 0 occurs
 * exactly once more, reversed, in a ring of B with the first ring's label as its s_right.  Every ring keeps at least 3
 * vertices.  The kept set at a larger tolerance is a subset of the kept set at a smaller one (where a segment splits does
 * not depend on the tolerance, only whether it does).  NOT promised: that two different arcs
 * never cross at a large tolerance; that is Douglas-Peucker's known limit: "clean outlines" below check and repair it. */
struct bs_simple_outlines {
  int32_t width, height;
  int32_t n_labels;
  int32_t has_z;            /* the count had a top image */
  int32_t tol_num, tol_den; /* the tolerance of the call */
  int64_t n_rings, n_nodes, n_junction_nodes, n_arcs, n_svertices, rounds, max_arc_nodes; /* totals */
  /* per ring; host memory owned by the library */
  int32_t* ring_label;      /* [n_rings], of the plain outlines */
  int64_t* ring_area2;      /* [n_rings], of the plain outlines */
  int64_t* s_ring_vertices; /* [n_rings] */
  int64_t* s_ring_area2;    /* [n_rings] */
  int64_t* s_ring_arcs;     /* [n_rings] */
  int64_t* s_ring_offset;   /* [n_rings + 1] */
  /* per label */
  int64_t* label_ring_offset; /* [n_labels + 1], of the plain outlines */
  /* the kept vertices, host memory owned by the library: filled by the host-memory entry point only (NULL after the count) */
  int32_t* sxy;     /* [n_svertices][2] */
  int32_t* sz;      /* [n_svertices], NULL without top */
  int32_t* s_right; /* [n_svertices] */
  uint8_t* s_flag;  /* [n_svertices] */
  /* device time (HIP events on the context's stream) */
  double ms_outlines; /* the plain count: the sum of its phases */
  double ms_nodes;    /* junction test, node flag, right label, corner index, Z */
  double ms_placing;  /* the cut and the Wyllie rounds with node counts, nodes per ring, their scan */
  double ms_arcs;     /* ring figures, rotation, scatter, arc ids, segments, the closed pass */
  double ms_rounds;   /* the rounds, the host's reads of the "kept something" words included */
  double ms_rings;    /* kept scan, places, area2 */
  double ms_emit;     /* the emit (host-memory entry point only) */
};

/* Counts, figures and sizes.  Runs bs_facet_outlines_count_dev on the same images first (its context state is replaced:
 * bs_facet_outlines_emit_dev afterwards emits the plain vertices of these images) and hands its result to *plain unless
 * plain is NULL (release it with bs_outlines_free).  The kept vertices stay in the context for the emit below.
 * BS_ERR_INVALID: as bs_facet_outlines_count_dev, or num outside [0, 2^31), or den outside [1, 2^31).  BS_ERR_RANGE: a label
 * >= n_labels.  On any error out and plain are left untouched, and the context stays usable.  Synchronises: the plain
 * count's three times, once for n_nodes, once every four rounds, once for the result. */
int bs_simple_outlines_count_dev(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width, int32_t height,
                                 int32_t n_labels, int64_t num, int64_t den, struct bs_simple_outlines* out,
                                 struct bs_outlines* plain);
/* The kept vertices of the last successful count on this context into device buffers of exactly its sizes: d_sxy
 * [n_svertices][2], d_sz [n_svertices] (NULL iff the count had no top), d_right [n_svertices], d_flag [n_svertices] bytes
 * (with no vertex all may be NULL).  May be called more than once.  BS_ERR_INVALID: no successful count, a missing buffer,
 * or d_sz given or missing against the count.  Synchronises. */
int bs_simple_outlines_emit_dev(bs_ctx* ctx, int32_t* d_sxy, int32_t* d_sz, int32_t* d_right, uint8_t* d_flag);
/* Host-memory twin: label and top (may be NULL) are host pointers; both steps, and the kept vertices come back in out's
 * library-owned sxy, sz, s_right and s_flag. */
int bs_simple_outlines(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height, int32_t n_labels,
                       int64_t num, int64_t den, struct bs_simple_outlines* out, struct bs_outlines* plain);
void bs_simple_outlines_free(struct bs_simple_outlines* o);

/* The simplified rings as an OBJ of closed polylines in millimetres, in the format of bs_outlines_write_obj.  Host only.
 *   "# simplified outlines: <n_labels> labels, <n_rings> rings, <n_svertices> vertices, tol2 <num>/<den>"
 *   for every ring r: "g label_<l>_ring_<i>_<outer|hole>" by the sign of the plain ring's area2, its kept vertices, and
 *   one closed polyline.
 * BS_ERR_INVALID: as bs_outlines_write_obj. */
int bs_simple_outlines_write_obj(const struct bs_simple_outlines* o, int32_t bin, const int32_t* origin, const char* path);

/* ---- clean outlines: the simplified outlines with every conflict between kept segments found and repaired ----
 *
 * Everything builds on "simplified outlines" above: nodes, arcs, the split choice, the rings and their order.
 *
 * Segments.  A segment is every pair of consecutive kept nodes of a ring (the last and the first included).  It carries the
 * ring's label on its left and s_right of its first node on its right.
 * Twins.  Two segments are twins iff their end corners are equal in reverse and their (left, right) labels are swapped.
 * Twins never conflict with each other.
 * Conflict.  Two segments that are not twins conflict iff their closed segments have a common point that is not an end
 * point of both: a proper crossing (cross), an end point of one in the open interior of the other (touch), or collinear
 * segments with more than a point in common (overlap; also between two segments that share an end corner and run the same
 * way).  All of it is evaluated with orientation tests in int64; the coordinates are lattice corners, so |cross| < 2^31.
 * Marked.  A segment is marked iff it conflicts with at least one other segment.
 * Repair round.  Every marked segment that has nodes strictly between its ends keeps its Douglas-Peucker choice -- the
 * greatest c^2, ties to the lowest corner index -- whatever the tolerance; the two halves are not simplified further and
 * keep no other node.  A marked segment without interior nodes stays as it is.  Rounds repeat until a round marks nothing.
 * Symmetry.  A twin is the same geometric segment: it conflicts with the same segments, is marked in the same round and
 * picks the same node, so neighbouring facets still share their boundary vertex for vertex.
 * Termination.  Interior nodes of an arc are vertices of a staircase, so a segment with interior nodes always has a greatest
 * c^2 > 0.  With every node kept (num = 0) no two segments conflict: junction nodes are arc ends and always kept, and runs
 * between adjacent nodes meet only in nodes.  Hence in every round with a conflict at least one marked segment has an
 * interior node, and the kept set grows.  Hence repair_rounds < n_nodes; more rounds than nodes is BS_ERR_INTERNAL.
 *
 * Result.  The per-ring and per-vertex arrays of the simplified outlines recomputed over the larger kept set.  s_flag gains
 * bit 2, kept by the repair, and bit 3, the segment that starts here is still marked (possible only when max_rounds stopped
 * the loop).  n_svertices_before: the vertex count of the plain simplification; n_marked_first: its marked segments, twins
 * counted each; n_marked_left: 0 unless stopped by max_rounds; n_forced: vertices added; repair_rounds.  Of the broad
 * phase (they depend on cell_log2, nothing else does): n_entries, the (cell, segment) entries of the first detection, and
 * max_cell_entries, the most entries of one cell in any detection.
 *
 * Sweeps (bs_set_outline_sweeps; off by default).  A chord can pass over a whole foreign ring -- an island, a hole -- without
 * meeting any of its segments.  No two segments conflict then, but which ring lies inside which has changed.
 * Lens.  A segment with kept ends a -> b whose ring has the nodes n_1 .. n_m strictly between them, m >= 1, has the lens
 * a, n_1, .., n_m, b, closed by the chord b -> a: a closed lattice polygon.  A segment without interior nodes has no lens.
 * Swept vertex.  A kept vertex position w, of any ring, is swept by a segment iff w does not lie on the lens's boundary
 * (the chord, its ends, the path's runs and nodes; a w on the chord is a touch, which the conflict test owns) and the
 * winding number of the lens around w is not zero.  The winding is the signed count of the lens's edges that a ray from w
 * crosses, with a half-open rule at the edges' ends and the sign of every crossing from an orientation test in int64.
 * Non-zero winding is the test, not odd parity.
 * Sweeping.  A segment is sweeping iff it sweeps at least one vertex.  A twin has the same lens reversed: it is sweeping in
 * the same detection and picks the same node.
 * Round.  In mode 2 a detection marks the conflicting and the sweeping segments over the same kept set; the repair round is
 * the one above, unchanged, and the loop ends when a detection marks nothing.  In mode 1 sweeps are detected and reported
 * and never marked: the vertices equal mode 0's.
 * Termination.  A sweeping segment has interior nodes, so the argument above holds: the kept set grows, repair_rounds <
 * n_nodes, and with every node kept no lens exists.
 * Not promised.  After the repair every chord is free of conflicts and its lens winds around no kept vertex.  Chords that
 * are homotopic to their paths in the plane punctured at the kept vertices would leave the rings isotopic to the original
 * ones, so that every hole lies in its outer ring and every label triangulates; zero winding is slightly weaker than that
 * homotopy, and nothing is promised.  The tests assert it on their cases.
 * Figures.  n_marked_first, n_marked_left and s_flag bit 3 keep their meaning: conflicts only.  s_flag gains bit 4: the
 * segment that starts here was sweeping in the last detection (0 in mode 0; after a repair to the end only mode 1 leaves
 * it).  repair_rounds, n_forced and bit 2 count every round and every vertex, whichever mark caused them. */
struct bs_outline_sweeps {
  int32_t mode;     /* of the count */
  int32_t wave_cap; /* BS_SWEEP_WAVE_CAP */
  int64_t n_lens_segments_first; /* segments with a lens at the first detection */
  int64_t n_sweeping_first;      /* sweeping segments at the first detection, twins counted each */
  int64_t n_sweeping_only_first; /* those of them that did not also conflict */
  int64_t n_swept_pairs_first;   /* (vertex position, segment) pairs with non-zero winding at the first detection */
  int64_t max_abs_winding;       /* over all detections */
  int64_t sweep_rounds;          /* repair rounds whose detection had a sweeping segment */
  int64_t n_sweeping_left;       /* sweeping segments of the last detection: 0 unless mode 1 or max_rounds stopped the loop */
  /* of the layout, at the first detection (they depend on the layout of the device pass, nothing else does) */
  int64_t n_items_first;         /* (run, lattice line) items */
  int64_t n_items_swapped_first; /* those of segments with |dx| < |dy|, whose rays run along X */
  int64_t n_candidates_first;    /* corners of all items' intervals */
  int64_t n_exact_first;         /* exact tests: candidates that are a kept vertex and no end of the segment */
  int64_t n_exact_wave_first;    /* those run by a wave: paths of more than wave_cap runs */
  int64_t n_rejected_first;      /* exact tests that found the boundary or winding 0 */
  double ms_sweep; /* device time of all sweep detections (HIP events); also inside the clean count's ms_detect */
};
#define BS_SWEEP_WAVE_CAP 64

/* The sweep mode of the context, as bs_set_audit a property of the context: every clean count on it follows, also the ones
 * that bs_outline_triangles*, bs_poly_solids* and bs_model_raster run.  0: off, the default -- every count behaves and
 * launches as without this paragraph; 1: report; 2: repair.  BS_ERR_INVALID for any other mode. */
int bs_set_outline_sweeps(bs_ctx* ctx, int32_t mode);
/* The figures of the last successful clean count on the context; all zero but mode and wave_cap after a count in mode 0 or
 * before any count. */
int bs_get_outline_sweeps(bs_ctx* ctx, struct bs_outline_sweeps* out);

struct bs_clean_outlines {
  int32_t width, height;
  int32_t n_labels;
  int32_t has_z;
  int32_t tol_num, tol_den;
  int32_t max_rounds, cell_log2; /* of the call; cell_log2 as used (the default resolved) */
  int64_t n_rings, n_nodes, n_junction_nodes, n_arcs, n_svertices, rounds, max_arc_nodes; /* as bs_simple_outlines */
  int64_t n_svertices_before, n_marked_first, n_marked_left, n_forced, repair_rounds, n_entries, max_cell_entries;
  /* per ring, per label and per kept vertex: as bs_simple_outlines, host memory owned by the library */
  int32_t* ring_label;
  int64_t* ring_area2;
  int64_t* s_ring_vertices;
  int64_t* s_ring_area2;
  int64_t* s_ring_arcs;
  int64_t* s_ring_offset;
  int64_t* label_ring_offset;
  int32_t* sxy;
  int32_t* sz;
  int32_t* s_right;
  uint8_t* s_flag;
  /* device time (HIP events on the context's stream) */
  double ms_simplify; /* the simplified count: the sum of its phases, the plain count included */
  double ms_detect;   /* all detections: segments, cells, scan, fill, sort, pair tests, sweeps, the host's reads included */
  double ms_repair;   /* all repair rounds */
  double ms_rings;    /* places, flags, area2 */
  double ms_emit;     /* the emit (host-memory entry point only) */
};

#define BS_CLEAN_DEFAULT_CELL_LOG2 4 /* cells of 16 x 16 corners: the fastest on urban_50m ("Clean outlines") */

/* Counts, figures and sizes.  Runs bs_simple_outlines_count_dev on the same images first (its context state and the plain
 * count's are replaced) and hands its results to *simple and *plain unless they are NULL.  max_rounds < 0: repair until
 * clean; 0: check only (the kept set equals the simplified outlines', bit 3 and n_marked_first report the conflicts);
 * > 0: a cap.  cell_log2: the broad-phase cell edge as a power of two in lattice units, 0 = the library's default, 1..30
 * valid, 30 puts everything into one cell; no result but n_entries and max_cell_entries depends on it.
 * Errors as bs_simple_outlines_count_dev; also BS_ERR_INVALID for cell_log2 outside 0..30, or where a detection would list more
 * than 2^31 - 1 (cell, segment) entries (take a larger cell_log2).  On any error the outputs are
 * left untouched.  Synchronises: the simplified count's times, then twice per detection (the entry count, with the sweep
 * pass's item count; the marked count, the sweep counts and the error word) -- one detection more than repair rounds -- and
 * once for the result.  With sweeps on, also BS_ERR_INVALID where a detection would list more than 2^31 - 1 items. */
int bs_clean_outlines_count_dev(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width, int32_t height,
                                int32_t n_labels, int64_t num, int64_t den, int32_t max_rounds, int32_t cell_log2,
                                struct bs_clean_outlines* out, struct bs_simple_outlines* simple, struct bs_outlines* plain);
/* The kept vertices of the last successful clean count on this context; buffers and errors as bs_simple_outlines_emit_dev. */
int bs_clean_outlines_emit_dev(bs_ctx* ctx, int32_t* d_sxy, int32_t* d_sz, int32_t* d_right, uint8_t* d_flag);
/* Host-memory twin: label and top (may be NULL) are host pointers; both steps. */
int bs_clean_outlines(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height, int32_t n_labels,
                      int64_t num, int64_t den, int32_t max_rounds, int32_t cell_log2, struct bs_clean_outlines* out,
                      struct bs_simple_outlines* simple, struct bs_outlines* plain);
void bs_clean_outlines_free(struct bs_clean_outlines* o);
/* The clean rings as an OBJ in the format of bs_simple_outlines_write_obj, with the first line
 *   "# clean outlines: <n_labels> labels, <n_rings> rings, <n_svertices> vertices, tol2 <num>/<den>, repair_rounds <r>,
 *    n_forced <f>" (one line).  Host only. */
int bs_clean_outlines_write_obj(const struct bs_clean_outlines* o, int32_t bin, const int32_t* origin, const char* path);

/* ---- outline triangles: every label's clean rings, holes included, as triangles over the clean vertices ----
 *
 * Input.  The result of bs_clean_outlines_count_dev with max_rounds = -1 on the same images and tolerance: the rings in the
 * order (label, h0), s_ring_offset and sxy as that stage leaves them, ring_area2 the plain outlines'.  A ring is outer iff its
 * plain ring_area2 > 0, else a hole.  A label may have several outer rings (a general label image); a facet image has exactly
 * one per label.  A vertex is an index into the clean vertex arrays; an occurrence is one visit of a vertex by a cyclic list.
 * A ring's label lies on the left of every segment, holes included.  No vertex is created: neighbouring labels that share a
 * segment vertex for vertex share it as a mesh edge.
 * Exact predicates.  orient(a, b, c) = (b - a) x (c - a) in int64 is the only arithmetic; the coordinates are lattice corners.
 * Cone.  At an occurrence v with predecessor p and successor n in its list a direction d lies in the cone
 *   if orient(p, v, n) > 0: iff (n - v) x d > 0 and d x (p - v) > 0;
 *   otherwise: iff not ((p - v) x d >= 0 and d x (n - v) >= 0).
 * Blocks.  A segment s-e blocks M-V iff the two cross properly, or an end of s-e that is at neither M's nor V's position lies
 * on the closed M-V, or M or V lies on s-e without being at one of its ends.
 * Bridges, per label.  The cyclic lists start as the label's outer rings in ring order.  The holes are taken in ascending
 * order of (x, y, vertex) of their leftmost vertex M (a ring that visits that position twice takes the lower vertex).
 * Candidates are all occurrences of all the label's lists whose position differs from M's.  An occurrence of vertex V is
 * valid iff M - V is in the cone at that occurrence, V - M is in the cone at M taken in its own ring, no segment of any ring
 * of the label blocks M-V (the holes not yet merged and M's own hole included), and no earlier bridge of the label blocks
 * M-V.  The bridge goes to the valid occurrence with the least (|V - M|^2, V); two occurrences of one vertex have disjoint
 * cones, so at most one of them is valid.  The list becomes ... V, M, (the hole from M round), M', V', ...: two occurrences
 * more.  A hole without a valid occurrence gives the label the status BS_TRI_NO_BRIDGE and no triangles: such a hole lies
 * outside its outer ring, which the clean outlines do not notice when a chord sweeps over a whole ring without touching it
 * -- unless the context repairs sweeps (bs_set_outline_sweeps, mode 2; "clean outlines", paragraph "Sweeps").  This count
 * runs the clean count itself and follows the context's mode ("Outline triangles", "Sweeps").
 * Ears, scanned as earcut scans, per list in the order of the outer rings.  stop = cursor = the outer ring's first
 * occurrence.  While more than 3 occurrences remain: b = cursor, a its predecessor, c its successor; b is an ear iff
 * orient(a, b, c) > 0 and no other occurrence q of the current list whose position differs from those of a, b and c has
 * orient(a, b, q) >= 0, orient(b, c, q) >= 0 and orient(c, a, q) >= 0.  An ear emits (a, b, c) as vertices, unlinks b and
 * sets cursor = stop = succ(c); otherwise cursor = succ(cursor), and if the cursor comes back to stop the label gets the
 * status BS_TRI_STALLED and no triangles.  The last three occurrences are emitted as (pred, cursor, succ).
 *
 * Result.  tri [n_triangles][3]: indices into the clean vertex arrays.  tri_offset [n_labels + 1] is known before anything
 * is clipped: a label has V + 2 H - 2 O triangles (V kept vertices, H holes, O outer rings), within a label the triangles
 * follow the outer rings in order, each in clip order; the slots of a label whose status is not BS_TRI_OK are all -1.
 * label_status; label_area2, the sum of orient over the label's triangles (0 unless OK); label_tests, the ear tests made
 * (every evaluation of "b is an ear").  bridge [n_rings][2] = (M, V), or (-1, -1) for outer rings and the holes of failed
 * labels.  Totals: n_triangles (all slots), n_failed_labels (NO_BRIDGE or STALLED), n_bridges, n_tests,
 * max_label_occurrences (the most V + 2 H of one label), and the labels that took each kernel path.
 * Promised for every OK label: every triangle has orient > 0; label_area2 equals the sum of s_ring_area2 over the label's
 * rings; every ring segment (i, next i) is a directed triangle edge exactly once; every other directed triangle edge occurs
 * exactly once and so does its reverse.  Hence the triangles tile the polygon. */
#define BS_TRI_OK 0
#define BS_TRI_NO_BRIDGE 1
#define BS_TRI_STALLED 2
#define BS_TRI_EMPTY 3 /* a label without a ring */
#define BS_TRI_WAVE_CAP 64  /* up to this many occurrences (V + 2 H) a label is one wave's work item */
#define BS_TRI_LDS_CAP 1024 /* up to this many a workgroup's, with its lists in LDS; beyond, in a global workspace */

struct bs_outline_triangles {
  int32_t n_labels;
  int32_t wave_cap, lds_cap; /* BS_TRI_WAVE_CAP, BS_TRI_LDS_CAP of the library */
  int32_t reserved;
  int64_t n_rings, n_svertices; /* of the clean outlines */
  int64_t n_triangles, n_failed_labels, n_bridges, n_tests, max_label_occurrences;
  int64_t n_labels_wave, n_labels_lds, n_labels_global; /* labels by kernel path (labels without a ring take none) */
  /* host memory owned by the library */
  int64_t* tri_offset;   /* [n_labels + 1] */
  int32_t* label_status; /* [n_labels] */
  int64_t* label_area2;  /* [n_labels] */
  int64_t* label_tests;  /* [n_labels] */
  int32_t* bridge;       /* [n_rings][2] */
  int32_t* tri;          /* [n_triangles][3]: host-memory entry point only, else NULL */
  /* device time (HIP events on the context's stream) */
  double ms_clean;    /* the clean count: the sum of its phases */
  double ms_prologue; /* uploads, the leftmost vertex of every hole */
  double ms_wave, ms_lds, ms_global; /* the three kernels */
  double ms_emit;     /* the emit (host-memory entry point only) */
};

/* Counts, triangulates and sizes.  Runs bs_clean_outlines_count_dev with max_rounds = -1 on the same images first (its
 * context state and that of the stages below it are replaced) and hands its results to *clean, *simple and *plain unless
 * they are NULL.  The triangles stay in the context for the emit below.  Errors as bs_clean_outlines_count_dev; also
 * BS_ERR_INVALID for n_svertices >= 2^31 or a label of 2^29 occurrences or more, BS_ERR_INTERNAL where an index read from
 * memory left its range.  On any error the outputs are left untouched.  Synchronises: the clean count's times, then once
 * for the result. */
int bs_outline_triangles_count_dev(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width, int32_t height,
                                   int32_t n_labels, int64_t num, int64_t den, int32_t cell_log2,
                                   struct bs_outline_triangles* out, struct bs_clean_outlines* clean,
                                   struct bs_simple_outlines* simple, struct bs_outlines* plain);
/* The triangles of the last successful count on this context into a device buffer d_tri [n_triangles][3] (may be NULL with
 * no triangle).  May be called more than once.  BS_ERR_INVALID: no successful count, or a missing buffer.  Synchronises. */
int bs_outline_triangles_emit_dev(bs_ctx* ctx, int32_t* d_tri);
/* Host-memory twin: label and top (may be NULL) are host pointers; both steps; the triangles come back in out's
 * library-owned tri, and *clean (unless NULL) carries the clean vertices as bs_clean_outlines returns them. */
int bs_outline_triangles(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height, int32_t n_labels,
                         int64_t num, int64_t den, int32_t cell_log2, struct bs_outline_triangles* out,
                         struct bs_clean_outlines* clean, struct bs_simple_outlines* simple, struct bs_outlines* plain);
void bs_outline_triangles_free(struct bs_outline_triangles* o);
/* The mesh as an OBJ in millimetres.  Host only: tri->tri and clean->sxy (and sz, else Z = 0) must be present.
 *   "# outline triangles: <n_labels> labels, <n_svertices> vertices, <n_triangles> triangles, <n_failed_labels> failed
 *    labels, <n_bridges> bridges" (one line)
 *   every clean vertex as "v X*bin+origin[0] Y*bin+origin[1] Z+origin[2]"
 *   for every label l with status BS_TRI_OK: "g label_<l>" and its triangles as "f i j k" (indices from 1).
 * Every number is a decimal integer, every line ends with \n.  origin may be NULL (zeros).  BS_ERR_INVALID: a null pointer,
 * bin < 1, counts or offsets that do not fit each other, a vertex index outside the vertices, or a file that cannot be
 * written. */
int bs_outline_triangles_write_obj(const struct bs_outline_triangles* tri, const struct bs_clean_outlines* clean, int32_t bin,
                                   const int32_t* origin, const char* path);

/* ---- polygon solids: a closed mesh per building (roof, floor, walls) over the clean vertices and the outline triangles ----
 *
 * The LoD2-style counterpart of "solids": the face count follows the simplified polygons, not the pixels.  Step 3 of "solids"
 * is followed so closely that the wall polygon is the same formula.  No vertex position is invented; every figure is an exact
 * integer.
 *
 * Input.  The state of a successful bs_outline_triangles_count_dev with a top image (d_top == NULL is BS_ERR_INVALID): the
 * clean vertices i with position sxy[i], height sz[i], s_right[i] and next(i) within their ring, the rings' labels, tri,
 * tri_offset and label_status.  And: a device table label_building[n_labels] (int32), each entry in 0 .. n_buildings - 1;
 * n_buildings; bin >= 1; base_z.  Nothing is assumed about sz against base_z: walls in both directions work.
 *
 * Open buildings.  A building is OPEN iff one of its labels has status BS_TRI_NO_BRIDGE or BS_TRI_STALLED.  An open building
 * contributes no vertex and no face and is counted.  BS_TRI_EMPTY labels contribute nothing and open nothing.
 *
 * Vertices.  Every clean vertex i of a label of a building c that is not open names two mesh vertices: (c, X, Y, sz[i]) and
 * (c, X, Y, base_z).  The mesh has one vertex per distinct quadruple: int32 [4] {X * bin, Y * bin, Z, c}, ordered by ascending
 * (c, Y, X, Z).  In this order bs_solids_write_obj writes the mesh unchanged, and the vertices of one (c, corner) -- a column
 * -- are consecutive by height.
 *
 * Faces.  Take the labels l in ascending order whose building c is not open and whose status is BS_TRI_OK.  For each label:
 *   1. roof, kind 0: every triangle (a, b, d) of l, in tri order, at the vertices (c, position, sz);
 *   2. floor, kind 1: the same triangles as (d, b, a) at base_z;
 *   3. walls, kind 2: every clean vertex s of l's rings in ascending order, with e = next(s), a_s = sz[s], a_e = sz[e] and
 *      R = s_right[s].
 *      If R >= 0 and label_building[R] == c, the segment has a twin t in a ring of R: the same two corners reversed and
 *      s_right[t] == l, which "simplified outlines" promise.  Then b_e = sz[t] and b_s = sz[next(t)], and only the smaller
 *      of the two labels emits the wall.  Otherwise b_s = b_e = base_z.
 *      The wall exists iff (a_s, a_e) != (b_s, b_e).  It is the polygon
 *        (e, a_e), (s, a_s), the vertices of (c, s) strictly between a_s and b_s walking from a_s, (s, b_s), (e, b_e), the
 *        vertices of (c, e) strictly between b_e and a_e walking from b_e
 *      with (s, b_s) left out when b_s == a_s and (e, b_e) when b_e == a_e: at least 3 vertices.
 *      A wall is CROSSING iff (a_s - b_s) * (a_e - b_e) < 0; it is emitted as that one polygon (a bow-tie in a vertical
 *      plane) and counted.
 * face_offset int32 [n_faces + 1], face_index int32 [n_indices] (vertex numbers from 0), face_building int32 [n_faces],
 * face_kind uint8 [n_faces], exactly as in struct bs_solids.  No new OBJ writer is needed: the five mesh arrays have the layout
 * that bs_solids_write_obj reads.
 *
 * Figures per building: status (0 closed, 1 open); labels (all labels the table maps to it); vertices; faces; roof_faces;
 * wall_faces; crossing_walls; max_wall_vertices; z_min / z_max over the sz of its clean vertices (INT32_MAX / INT32_MIN without
 * one); area2, the sum of orient over its roof triangles; volume6, the sum over its roof triangles of
 * orient(a, b, d) * (sz[a] + sz[b] + sz[d] - 3 * base_z) in int64.  The volume in mm^3 is volume6 * bin^2 / 6.  All but status
 * and labels are 0 (z_min / z_max: the values without a vertex) for an open building.  And the totals of these figures,
 * n_indices and n_open_buildings.
 *
 * Errors.  BS_ERR_RANGE: a clean vertex (of any label) with |sz - base_z| >= 2^24 (which keeps volume6 inside int64), a
 * label_building value outside its range, or 2^31 or more vertices or indices.  BS_ERR_INTERNAL: a twin that is missing or has
 * the wrong labels.  On any error the outputs are untouched and the context stays usable.
 *
 * Promised.  Per closed building every directed edge of the mesh occurs exactly as often as its reverse.  The sum over the fan
 * triangles of all its faces of det[(X, Y, Z)] in lattice units (X, Y not multiplied by bin) equals volume6.  NOT promised:
 * that the mesh is manifold or free of self-intersection -- crossing walls are bow-ties, and a chord may sweep over a foreign
 * building's ring ("Polygon solids"). */
#define BS_POLY_FIG_CAP 1024 /* buildings below this number have their figures reduced in LDS, the rest by global atomics */

struct bs_poly_solids {
  int32_t n_buildings, n_labels;
  int32_t bin, base_z;
  int32_t fig_cap; /* BS_POLY_FIG_CAP of the library */
  int32_t reserved;
  int64_t n_open_buildings, n_vertices, n_faces, n_indices, n_roof_faces, n_wall_faces, n_crossing_walls;
  int64_t max_wall_vertices_all, total_area2, total_volume6; /* totals (max_wall_vertices_all: the maximum) */
  /* per building; host memory owned by the library */
  int32_t* status;            /* [n_buildings] */
  int64_t* labels;            /* [n_buildings] */
  int64_t* vertices;          /* [n_buildings] */
  int64_t* faces;             /* [n_buildings] */
  int64_t* roof_faces;        /* [n_buildings] */
  int64_t* wall_faces;        /* [n_buildings] */
  int64_t* crossing_walls;    /* [n_buildings] */
  int64_t* max_wall_vertices; /* [n_buildings] */
  int32_t* z_min;             /* [n_buildings] */
  int32_t* z_max;             /* [n_buildings] */
  int64_t* area2;             /* [n_buildings] */
  int64_t* volume6;           /* [n_buildings] */
  /* the mesh, host memory owned by the library: filled by the host-memory entry point only (NULL after the count) */
  int32_t* vertex;        /* [n_vertices][4] */
  int32_t* face_offset;   /* [n_faces + 1] */
  int32_t* face_index;    /* [n_indices] */
  int32_t* face_building; /* [n_faces] */
  uint8_t* face_kind;     /* [n_faces] */
  /* device time (HIP events on the context's stream) */
  double ms_triangles; /* the triangle count: the sum of its phases, the clean count included */
  double ms_twins;     /* uploads, keys, the sort of the segments, the pairing */
  double ms_vertices;  /* the two sorts of the entries, head flags, their sum, the numbers */
  double ms_count;     /* walls, triangles, the two sums */
  double ms_emit_vertices, ms_emit_faces; /* the passes of the emit (host-memory entry point only) */
};

/* Counts, figures and sizes.  Runs bs_outline_triangles_count_dev on the same images first (its context state and that of the
 * stages below it are replaced) and hands its results to *tri, *clean, *simple and *plain unless they are NULL.
 * d_label_building is a device pointer (read once, not kept).  The twins, the vertex numbers and the offsets stay in the
 * context for the emit below; out's per-building arrays are host memory owned by the library (bs_poly_solids_free, which
 * accepts a zeroed struct).  An image without a labelled pixel is valid: an empty mesh.
 * BS_ERR_INVALID: a null pointer (d_top included; d_label_building may be NULL with n_labels == 0), n_buildings < 0, bin < 1,
 * or what bs_outline_triangles_count_dev refuses.  BS_ERR_RANGE and BS_ERR_INTERNAL as above.  On any error the outputs are
 * left untouched.  Synchronises: the triangle count's times, once for the table, once for the result. */
int bs_poly_solids_count_dev(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width, int32_t height,
                             int32_t n_labels, int64_t num, int64_t den, int32_t cell_log2, const int32_t* d_label_building,
                             int32_t n_buildings, int32_t bin, int32_t base_z, struct bs_poly_solids* out,
                             struct bs_outline_triangles* tri, struct bs_clean_outlines* clean,
                             struct bs_simple_outlines* simple, struct bs_outlines* plain);
/* The mesh of the last successful count on this context into device buffers of exactly its sizes: d_vertex [n_vertices][4]
 * (16-byte aligned), d_face_offset [n_faces + 1], d_face_index [n_indices], d_face_building and d_face_kind [n_faces] (a
 * pointer to an array of no element may be NULL; an empty mesh writes face_offset[0] alone).  May be called more than once.
 * The emit reads the clean vertices and the triangles of the count: a later count of the clean outlines or of a stage built on
 * them on this context ends its validity.  BS_ERR_INVALID: null pointer, or no successful count.  Synchronises. */
int bs_poly_solids_emit_dev(bs_ctx* ctx, int32_t* d_vertex, int32_t* d_face_offset, int32_t* d_face_index,
                            int32_t* d_face_building, uint8_t* d_face_kind);
/* Host-memory twin: label, top and label_building are host pointers; both steps; the mesh comes back in out's library-owned
 * arrays, *tri and *clean (unless NULL) as bs_outline_triangles returns them. */
int bs_poly_solids(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height, int32_t n_labels,
                   int64_t num, int64_t den, int32_t cell_log2, const int32_t* label_building, int32_t n_buildings, int32_t bin,
                   int32_t base_z, struct bs_poly_solids* out, struct bs_outline_triangles* tri, struct bs_clean_outlines* clean,
                   struct bs_simple_outlines* simple, struct bs_outlines* plain);
void bs_poly_solids_free(struct bs_poly_solids* s);

/* ---- model raster: the outline triangles back on the pixel lattice, and the model's error against the images ----
 *
 * The inverse of the chain facets -> outlines -> simplified -> clean -> triangles.  Per pixel: the label the model puts there,
 * how many triangles cover it, and the model's height at the pixel centre.  Per label: exact fidelity figures against the label
 * image and top.  Everything is an exact integer.  It reports overlaps and swept holes and repairs nothing itself: the
 * repair is the sweep mode of the clean outlines (bs_set_outline_sweeps), which the host-memory entry point follows.
 *
 * Input.  The state of a successful bs_outline_triangles_count_dev on the context, counted with a top image
 * (bs_poly_solids_count_dev runs that count, so its state serves as well): the clean vertices sxy, sz; tri, tri_offset,
 * label_status.  A label image d_label [height][width] and d_top [height][width][4] of the size of the count -- normally the
 * images of the count; the stage does not require it.  n_labels is the count's.  L(p) is label[p] if it lies in
 * 0 .. n_labels - 1, else -1.
 *
 * Coverage, in doubled lattice units.  The centre of pixel (x, y) is P = (2 x + 1, 2 y + 1).  A triangle slot t with vertices
 * a, b, c (not -1) has the doubled positions A, B, C and the weights w_a = orient(P, B, C), w_b = orient(P, C, A),
 * w_c = orient(P, A, B) in int64.  Each weight belongs to an edge u -> v: B -> C, C -> A, A -> B.  t covers the pixel iff every
 * weight is > 0, or is == 0 and its edge has v.y > u.y.  A centre never lies on a vertex or on an axis-parallel edge (its
 * coordinates are odd, theirs even), and the shared edge of two triangles runs in opposite directions in the two, so exactly
 * one of them owns a centre on it.  cover[p] is the number of slots covering p; win[p] the lowest covering slot, -1 if none;
 * M(p) the label of win[p] by tri_offset, -1 if none.
 *
 * Height.  For win[p] = t: D = w_a + w_b + w_c (> 0), N = w_a sz[a] + w_b sz[b] + w_c sz[c], and
 * mz2[p] = floor((4 N + D) / (2 D)): the model height at the centre times two, rounded half up; INT32_MIN where win[p] < 0.
 * The pixel-exact surface at the centre lies on the diagonal 00-11 of both top triangles; its doubled height is t00 + t11
 * (top[p][0] + top[p][3]).  Where L(p) >= 0 and M(p) >= 0: e2[p] = mz2[p] - (t00 + t11).  top is read nowhere else.  With
 * (width + 1)(height + 1) < 2^31 and |sz| < 2^24, 4 N + D stays below 2^61.
 *
 * Figures per label l, all int64: pixels = #{L = l}; model_pixels = #{M = l}; kept = #{L = l and M = l};
 * multi = #{M = l and cover > 1}; and over the pixels with M = l and L >= 0: err_pixels, sum_abs_e2, max_abs_e2,
 * sq_lo = sum of (e2^2 mod 2^32) and sq_hi = sum of (e2^2 div 2^32) -- both are order-free and cannot overflow; the sum of
 * squares is sq_hi * 2^32 + sq_lo.
 * Totals: the sums of the per-label figures (max_abs_e2_all: the maximum); n_uncovered = #{L >= 0, M < 0};
 * n_spill = #{L < 0, M >= 0}; n_moved = #{L >= 0, M >= 0, L != M}; n_multi = #{cover > 1}; sum_cover.  And of the
 * implementation ("Model raster"): n_rows and n_items, its row and pixel work items; n_empty_spans, the rows
 * without a candidate pixel; max_span, the longest span.
 *
 * Promised.  sum pixels = sum kept + n_moved + n_uncovered.  sum model_pixels = sum kept + n_moved + n_spill.  If every label
 * is BS_TRI_OK or BS_TRI_EMPTY and the tolerance is 0: M = L on every pixel and cover = [L >= 0].
 *
 * Errors.  BS_ERR_INVALID: no valid triangle state, that state's count had no top image, a null d_label or d_top or out, or a
 * size that differs from the count's.  BS_ERR_RANGE: a vertex of a triangle with |sz| >= 2^24, or |t00 + t11| >= 2^25 on a
 * pixel where e2 is formed.  On any error the outputs are untouched and the context stays usable. */
#define BS_MRASTER_FIG_CAP 512 /* labels below this number have their figures reduced in LDS, the rest by global atomics */
#define BS_MRASTER_CHUNK 256   /* the pixel items of one workgroup */
#define BS_MRASTER_FIG_GRID 2048 /* workgroups of 256 of the pass over the pixels: beyond 524 288 pixels a thread takes several */

struct bs_model_raster {
  int32_t width, height, n_labels;
  int32_t fig_cap, chunk; /* BS_MRASTER_FIG_CAP, BS_MRASTER_CHUNK of the library */
  int32_t reserved;
  int64_t n_triangles; /* all slots of the triangle state */
  int64_t total_pixels, total_model_pixels, total_kept, total_err_pixels, total_sum_abs_e2, max_abs_e2_all, total_sq_lo,
      total_sq_hi;
  int64_t n_uncovered, n_spill, n_moved, n_multi, sum_cover;
  int64_t n_rows, n_items, n_empty_spans, max_span;
  /* per label; host memory owned by the library */
  int64_t* pixels;       /* [n_labels] */
  int64_t* model_pixels; /* [n_labels] */
  int64_t* kept;         /* [n_labels] */
  int64_t* multi;        /* [n_labels] */
  int64_t* err_pixels;   /* [n_labels] */
  int64_t* sum_abs_e2;   /* [n_labels] */
  int64_t* max_abs_e2;   /* [n_labels] */
  int64_t* sq_lo;        /* [n_labels] */
  int64_t* sq_hi;        /* [n_labels] */
  /* device time (HIP events on the context's stream) */
  double ms_rows;    /* clearing the images, the rows of every slot, their sum, the host's read of n_rows */
  double ms_spans;   /* the span of every row, their sum, the host's read of n_items */
  double ms_pixels;  /* the pixel items: weights, win and cover */
  double ms_figures; /* the pass over the pixels: M, mz2, the figures; the host's read of the result; the copies into the
                        caller's images */
};

/* Rasterises the triangles of the last successful bs_outline_triangles_count_dev (or bs_poly_solids_count_dev) on this context
 * where they lie and changes none of that state: bs_outline_triangles_emit_dev and bs_poly_solids_emit_dev stay valid.
 * d_model, d_cover, d_mz2: device images int32 [height][width] for M, cover and mz2; each may be NULL.  The figures are
 * always computed; out's per-label arrays are host memory owned by the library (bs_model_raster_free, which accepts a zeroed
 * struct).  Synchronises: once for n_rows, once for n_items, once for the result, once for the copies. */
int bs_model_raster_dev(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width, int32_t height,
                        int32_t* d_model, int32_t* d_cover, int32_t* d_mz2, struct bs_model_raster* out);
/* Host-memory twin: label, top and the three images (each may be NULL) are host pointers.  Runs bs_outline_triangles on the
 * images, then the raster; hands the results of the stages before to *tri, *clean, *simple and *plain unless they are NULL, as
 * bs_outline_triangles returns them.  Errors of both. */
int bs_model_raster(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height, int32_t n_labels,
                    int64_t num, int64_t den, int32_t cell_log2, int32_t* model, int32_t* cover, int32_t* mz2,
                    struct bs_model_raster* out, struct bs_outline_triangles* tri, struct bs_clean_outlines* clean,
                    struct bs_simple_outlines* simple, struct bs_outlines* plain);
void bs_model_raster_free(struct bs_model_raster* r);

/* ---- point residuals: every point of the cloud against the polygon model ----
 *
 * The first check of the chain against its input: how far the model of the outline triangles lies from the points it was built
 * from.  Per point: the label of the triangle over it, how many triangles cover it, and twice its height above the model.  Per
 * label: the residual figures by which tolerance_mm, min_pixels and merge_flat are chosen.  Everything is an exact integer.
 *
 * Input.  The state of a successful bs_outline_triangles_count_dev or bs_poly_solids_count_dev with a top image, on the
 * context: the clean vertices sxy, sz; tri, tri_offset, label_status; its width, height and n_labels.  bin >= 1.  A cloud
 * d_xyz [n][3] int32 in millimetres, shifted to its origin as for bs_assign_buildings_dev; every point's base pixel
 * (x / bin, y / bin) lies inside the image.  Optionally d_plane_idx [n] together with a host table label_plane [n_labels] (in
 * the pipeline: facet_plane of the roof facets): both or neither.  clip2 >= 0 (int32): the inlier bound in doubled millimetres.
 *
 * Coverage, in doubled millimetres.  Point i stands for the centre of its millimetre cell: P = (2 x + 1, 2 y + 1).  Vertex v
 * stands at Q = (2 bin sxy[v].x, 2 bin sxy[v].y).  The weights w_a, w_b, w_c, the ownership rule for a weight of 0 (v.y > u.y),
 * cover, win (the lowest covering slot) and M (its label by tri_offset) are word for word those of "model raster", with P and
 * Q in place of its centre and corners.  P is odd and Q even, so P never lies on a vertex or on an axis-parallel edge; it can
 * lie on a slanted edge, and there the rule decides.  At bin == 1 the definition is the model raster's own.
 *
 * Residual.  For win = t: D, N and mz2 = floor((4 N + D) / (2 D)) as in "model raster"; r2[i] = 2 z_i - mz2, and INT32_MIN
 * where win < 0.  With width * bin and height * bin <= 2^24, |sz| < 2^24 and |z| < 2^24, D stays below 2^52, but 4 N + D does
 * not fit 64 bits.  The value is the mathematical one: the library forms it relative to the lowest of the three sz, in 64 bits
 * where the bit lengths of D and of the largest height difference prove per point that this fits, and in 128 bits elsewhere
 * (n_height_wide counts those points).
 *
 * Figures per label l, all int64, over the points with M = l: points; multi (cover > 1); above (r2 > clip2) and below
 * (r2 < -clip2); over the inliers (neither): in_points, sum_r2 (signed: the bias), sum_abs_r2, max_abs_r2, sq_lo and sq_hi
 * (the sum of r2^2 split as in "model raster"); with the plane table plane_points = #{plane_idx[i] == label_plane[l]} and
 * plane_in, those of them that are inliers (both 0 without the table).  Totals: the sums of these (max_abs_r2_all: the
 * maximum; n_multi: the sum of multi); n_uncovered = #{win < 0}.  And of the implementation ("Point residuals"):
 * n_rows and n_items, the row items and the entries of the per-pixel lists; max_list, the longest list; n_empty_pixel, the
 * points whose pixel has an empty list; n_height_wide.
 *
 * Promised.  n = sum points + n_uncovered.  points = in_points + above + below for every label.  At tolerance 0 with every
 * label BS_TRI_OK or BS_TRI_EMPTY: M_i = L(base pixel of i) for every point.  At bin == 1 with the points (x, y, .) of all
 * pixels in raster order: M, cover and mz2 (2 z - r2) equal the three images of bs_model_raster_dev on the same state.
 *
 * Errors.  BS_ERR_INVALID: no valid triangle state, or a state counted without top; a null cloud or out, n < 1, bin < 1,
 * clip2 < 0; only one of d_plane_idx / label_plane.  BS_ERR_RANGE: 2^29 points or more; a point with a negative x or y, or
 * whose pixel lies outside the image; |z| >= 2^24; an extent width * bin or height * bin above 2^24; |sz| >= 2^24 on a vertex
 * of a triangle; 2^31 or more list entries.  On any error the outputs are untouched and the context stays usable: the cloud
 * and the state are checked in passes of their own before the pass that writes. */
#define BS_PRESID_FIG_CAP 256 /* labels below this number have their figures reduced in LDS (16 KiB), the rest by global atomics */
#define BS_PRESID_CHUNK 256   /* the list entries of one workgroup while the lists are built */
#define BS_PRESID_GRID 2048   /* workgroups of 256 of the pass over the points: beyond 524 288 points a thread takes several */

struct bs_point_residuals {
  int32_t width, height, n_labels, bin, clip2;
  int32_t fig_cap, chunk, grid; /* BS_PRESID_FIG_CAP, BS_PRESID_CHUNK, BS_PRESID_GRID of the library */
  int64_t n_points, n_triangles; /* n; all slots of the triangle state */
  int64_t total_points, total_above, total_below, total_in_points, total_sum_r2, total_sum_abs_r2, max_abs_r2_all, total_sq_lo,
      total_sq_hi, total_plane_points, total_plane_in;
  int64_t n_uncovered, n_multi;
  int64_t n_rows, n_items, max_list, n_empty_pixel, n_height_wide;
  /* per label; host memory owned by the library */
  int64_t* points;       /* [n_labels] */
  int64_t* multi;        /* [n_labels] */
  int64_t* above;        /* [n_labels] */
  int64_t* below;        /* [n_labels] */
  int64_t* in_points;    /* [n_labels] */
  int64_t* sum_r2;       /* [n_labels] */
  int64_t* sum_abs_r2;   /* [n_labels] */
  int64_t* max_abs_r2;   /* [n_labels] */
  int64_t* sq_lo;        /* [n_labels] */
  int64_t* sq_hi;        /* [n_labels] */
  int64_t* plane_points; /* [n_labels] */
  int64_t* plane_in;     /* [n_labels] */
  /* device time (HIP events on the context's stream) */
  double ms_rows;   /* clearing, the check of the cloud, the rows of every slot, their sum, the host's read of n_rows */
  double ms_spans;  /* the span of every row item, their sum, the host's read of n_items */
  double ms_lists;  /* the count per pixel, its sum, the fill through the cursors */
  double ms_points; /* the pass over the points: the outputs and the figures; the host's read of the result */
};

/* Measures the cloud against the triangles of the last successful bs_outline_triangles_count_dev (or bs_poly_solids_count_dev)
 * on this context where they lie and changes none of that state: bs_outline_triangles_emit_dev and bs_poly_solids_emit_dev
 * stay valid.  d_label_out, d_r2, d_cover: device arrays int32 [n] for M, r2 and cover; each may be NULL.  d_plane_idx is a
 * device pointer, label_plane a host pointer.  The figures are always computed; out's per-label arrays are host memory owned
 * by the library (bs_point_residuals_free, which accepts a zeroed struct).  Synchronises: once for n_rows, once for n_items,
 * once for the checks, once for the result. */
int bs_point_residuals_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t bin, const int32_t* d_plane_idx,
                           const int32_t* label_plane, int32_t clip2, int32_t* d_label_out, int32_t* d_r2, int32_t* d_cover,
                           struct bs_point_residuals* out);
/* Host-memory twin: label, top, the cloud, plane_idx and the three outputs (each may be NULL) are host pointers.  Runs
 * bs_outline_triangles on the images, then the stage; hands the results of the stages before to *tri, *clean, *simple and
 * *plain unless they are NULL, as bs_outline_triangles returns them.  Errors of both. */
int bs_point_residuals(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height, int32_t n_labels,
                       int64_t num, int64_t den, int32_t cell_log2, const int32_t* xyz, int64_t n, int32_t bin,
                       const int32_t* plane_idx, const int32_t* label_plane, int32_t clip2, int32_t* label_out, int32_t* r2,
                       int32_t* cover, struct bs_point_residuals* out, struct bs_outline_triangles* tri,
                       struct bs_clean_outlines* clean, struct bs_simple_outlines* simple, struct bs_outlines* plain);
void bs_point_residuals_free(struct bs_point_residuals* r);

/* ---- terrain: the ground height of every building from the points around it ----
 *
 * ground_th is the lower edge of the height bin that holds the median z of the whole tile: it separates the points above
 * ground for the raster and was never a floor height.  The ground next to a building is in the points that fall just outside
 * its footprint; this stage reads it there.  Everything is an exact integer and independent of the order of summation.
 *
 * Input.  The cloud d_xyz [n][3] int32 in millimetres shifted to its origin, 1 <= n < 2^29, every |coordinate| < 2^23; bin >= 1;
 * map [height][width] as bs_building_map writes it (any negative value is outside, -1) with n_buildings >= 0;
 * ring in 1 .. BS_TERRAIN_MAX_RING; a quantile q_num / q_den with 0 <= q_num <= q_den, 1 <= q_den < 2^31; min_ground >= 1;
 * fallback_z.
 *
 * 1. Ring, in exactly `ring` synchronous rounds over the image alone.  owner_0 = map, and dist = 0 where map >= 0.  In round
 * r every pixel with owner_{r-1} == -1 looks at its 4-neighbours inside the image that have owner_{r-1} >= 0; if there is one,
 * the pixel takes the smallest owner among them and dist = r.  A label moves one pixel per round, and only through outside
 * pixels: a pocket behind another building is reached around the corner or not at all.  rounds_used = the rounds that labelled
 * something.  owner [height][width] int32 is -1 where never reached; dist [height][width] uint8 is 0 on buildings and on
 * unreached pixels, which owner tells apart.  A RING pixel has map == -1 and owner >= 0.
 *
 * 2. Low.  For every ring pixel, low = the minimum z over ALL points whose base pixel (x / bin, y / bin) it is -- no ground
 * threshold, no label test: the lowest return of a pixel beside a wall is the ground or close to it, whatever lies above.
 * low = INT32_MAX where no point lies, and on every pixel that is no ring pixel.
 *
 * 3. Per building c.  G_c = the multiset of low over c's ring pixels with low != INT32_MAX.  ring_pixels; ground_pixels =
 * |G_c|; ring_points (the points on its ring pixels); ground_min, ground_max (INT32_MAX / INT32_MIN for an empty G_c);
 * ground_sum.  If ground_pixels >= min_ground: ground = the element of rank floor((ground_pixels - 1) * q_num / q_den) of
 * G_c in ascending order (64-bit arithmetic) and status = 0.  Otherwise ground = fallback_z and status = 1.  A quantile, not
 * the minimum: one return from a pit or a multipath echo metres below the terrain must not set the floor.
 * Totals: n_ring_pixels, n_ground_pixels, n_ring_points, n_fallback (the sums), rounds_used.
 *
 * Promised.  ground_min <= ground <= ground_max where status == 0.  The rounds compute the L1 Voronoi diagram of the buildings
 * cut at `ring`: a ring pixel's dist is its L1 distance to the nearest building pixel, and its owner the lowest index among
 * the buildings at that distance ("Terrain", has the argument).  n_buildings == 0 is valid: nothing is reached and
 * no per-building array is touched.
 *
 * Errors.  BS_ERR_INVALID: a null cloud, map or out, n < 1, bin < 1, width or height < 1, width * height >= 2^31,
 * n_buildings < 0, ring outside 1 .. 255, q outside the ranges above, min_ground < 1.  BS_ERR_RANGE: 2^29 points or more; a
 * point with a negative x / y or whose pixel lies outside the image; a coordinate at or beyond 2^23; a map value
 * >= n_buildings.  On any of these the outputs and the struct are untouched and the context stays usable: everything is
 * computed in scratch of the context and copied once the ranges are known.  (BS_ERR_INTERNAL -- a sorted key that is not its
 * building's -- leaves the struct untouched and the images, which do not depend on the pick, written.) */
#define BS_TERRAIN_MAX_RING 255
#define BS_TERRAIN_FIG_CAP 1024 /* buildings below this number have their figures reduced in LDS, the rest by global atomics */
#define BS_TERRAIN_GRID 2048    /* workgroups of 256 of the pass over the points: beyond 524 288 points a thread takes several */

struct bs_terrain {
  int32_t width, height, n_buildings, bin, ring, q_num, q_den, min_ground, fallback_z;
  int32_t fig_cap, grid; /* BS_TERRAIN_FIG_CAP, BS_TERRAIN_GRID of the library */
  int32_t rounds_used, n_fallback, reserved;
  int64_t n_points, n_ring_pixels, n_ground_pixels, n_ring_points;
  /* per building; host memory owned by the library */
  int64_t* ring_pixels;   /* [n_buildings] */
  int64_t* ground_pixels; /* [n_buildings] */
  int64_t* ring_points;   /* [n_buildings] */
  int64_t* ground_sum;    /* [n_buildings] */
  int32_t* ground_min;    /* [n_buildings] */
  int32_t* ground_max;    /* [n_buildings] */
  int32_t* ground;        /* [n_buildings] */
  int32_t* status;        /* [n_buildings] 0: the quantile; 1: fallback_z */
  /* device time (HIP events on the context's stream) */
  double ms_ring;   /* clearing, the check of the map, the first frontier, the rounds */
  double ms_points; /* the pass over the points: the check of the cloud, ring_points, low */
  double ms_pixels; /* the pass over the pixels: the keys and the figures; the host's read of the range flags */
  double ms_pick;   /* the sort of the keys, the sum of ground_pixels, the pick, the copies into the caller's images, the
                       host's read of the result */
};

/* d_xyz and d_map are device pointers.  d_owner [height][width] int32, d_dist [height][width] uint8 and d_low
 * [height][width] int32 are device images; each may be NULL.  The figures are always computed; out's per-building arrays are
 * host memory owned by the library (bs_terrain_free, which accepts a zeroed struct).  All `ring` rounds are launched without a
 * host round trip.  Synchronises: once for the range flags, once for the result. */
int bs_terrain_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t bin, const int32_t* d_map, int32_t width,
                   int32_t height, int32_t n_buildings, int32_t ring, int32_t q_num, int32_t q_den, int32_t min_ground,
                   int32_t fallback_z, int32_t* d_owner, uint8_t* d_dist, int32_t* d_low, struct bs_terrain* out);
/* Host-memory twin: xyz, map and the three images (each may be NULL) are host pointers. */
int bs_terrain(bs_ctx* ctx, const int32_t* xyz, int64_t n, int32_t bin, const int32_t* map, int32_t width, int32_t height,
               int32_t n_buildings, int32_t ring, int32_t q_num, int32_t q_den, int32_t min_ground, int32_t fallback_z,
               int32_t* owner, uint8_t* dist, int32_t* low, struct bs_terrain* out);
void bs_terrain_free(struct bs_terrain* t);

/* ---- per-building bases: solids that stand on the terrain ----
 *
 * A switch of the context, as bs_set_outline_sweeps.  base [n_buildings] is a host table (in the pipeline: ground of
 * struct bs_terrain); the context keeps a copy.  NULL or n_buildings == 0 switches it off, which is the default.
 * While it is set, bs_solids_count_dev and its emit, bs_roof_generalise_dev, bs_poly_solids_count_dev and its emit, and their
 * host-memory twins use base[c] wherever their definition says base_z for a pixel, vertex, wall, floor or figure of building
 * c: the max(base_z, .) of the tops, the vertex sets of the corners and columns, the floor, the outer walls, volume6, and the
 * 2^24 range check of the polygon solids (a clean vertex is measured against the base of its label's building, open or not).
 * The definitions are per building already, so every building's mesh stays closed and oriented, and building c of a run under
 * the switch is building c of a scalar run with base_z = base[c].  The scalar base_z of a call is still validated and
 * reported in its struct.  A call of these stages whose n_buildings differs from the table's is BS_ERR_INVALID.  Switched
 * off, every byte these stages write is what they write without this paragraph.
 * Setting or clearing the table ends the validity of the last bs_solids_count_dev and bs_poly_solids_count_dev on the context:
 * an emit follows the table of its count.  BS_ERR_INVALID: n_buildings < 0, or a null table with n_buildings > 0. */
int bs_set_building_bases(bs_ctx* ctx, const int32_t* base, int32_t n_buildings);
/* *n_buildings = the length of the table (0: off); its first min(capacity, length) entries into base, which may be NULL
 * with capacity == 0.  BS_ERR_INVALID: a null n_buildings, a negative capacity, or a null base with capacity > 0. */
int bs_get_building_bases(bs_ctx* ctx, int32_t* base, int32_t capacity, int32_t* n_buildings);

/* ---- ground: a terrain raster of the tile by a progressive morphological filter ----
 *
 * ground_th is one scalar for the whole tile; on a slope it lies below the uphill ground and above the downhill roofs.  This
 * stage computes a ground surface per pixel (a digital terrain model, DTM) from the cloud alone; bs_set_ground_model below lets
 * the raster, the point assignment and the roofs read their threshold from it.  Everything is an exact integer.
 *
 * Input.  The cloud xyz [n][3] int32 in millimetres shifted to its origin, 1 <= n < 2^29, every |coordinate| < 2^23;
 * extent[3] as for bs_grid_picture; struct bs_ground_params: cell > 0 (mm); n_steps K in 1 .. BS_GROUND_MAX_STEPS; radius[k]
 * (k < K) in pixels, strictly increasing, each in 1 .. BS_GROUND_MAX_RADIUS; a slope s_num / s_den with s_num >= 0 and
 * s_den > 0; dh0, dh_max, tol, min_height >= 0 (mm).  The lattice is bs_grid_dims(extent, cell) = (width, height); the pixel
 * of a point is (x / cell, y / cell), no splat.  EMPTY = INT32_MAX.
 *
 * 1. low [height][width] int32: the lowest z of all points of the pixel, EMPTY without a point.
 * 2. S_0 = low; step [height][width] uint8 = 255 where low is EMPTY and 0 elsewhere; r_0 = 0.
 * 3. For k = 1 .. K, with r = radius[k - 1]:  E = erode(S_{k-1}, r): per pixel the minimum over the (2r+1)^2 square around
 *    it clipped to the image, IGNORING EMPTY (EMPTY if all are);  O_k = dilate(E, r): the maximum over the same square,
 *    ignoring EMPTY;  threshold[k - 1] = t_k = min(dh_max, dh0 + floor(s_num * (r_k - r_{k-1}) * cell / s_den)), exact;
 *    every pixel with step == 0, S_{k-1} != EMPTY and S_{k-1} - O_k > t_k (strictly) gets step = k -- the first step that
 *    flags a pixel stays -- and step_pixels[k - 1] counts them;  S_k = O_k.
 * 4. dtm [height][width] int32 = low where step == 0, else S_K.  It stays EMPTY where no point lies within reach.
 * 5. Per point: hag [n] int32 = z - dtm[pixel];  class [n] uint8 = 0 (ground) iff step[pixel] == 0 and hag <= tol,
 *    else 2 (object) iff hag >= min_height, else 1.
 *
 * Figures, all exact.  n_ground_pixels (step == 0), n_object_pixels (step in 1 .. K), n_empty_pixels (low EMPTY),
 * n_filled_pixels (low EMPTY, dtm not); n_ground_points, n_low_points, n_object_points (classes 0, 1, 2); dtm_min, dtm_max
 * over the pixels with a dtm (INT32_MAX / INT32_MIN when there is none); hag_min, hag_max over all points; sum_hag_ground
 * over the points of class 0.
 *
 * Promised.  dtm <= low wherever low != EMPTY (an opening never rises above its input, and a pixel that no step flagged
 * keeps low), so hag >= 0; a pixel EMPTY in low has step 255 and counts neither as ground nor as object.
 *
 * Errors.  BS_ERR_INVALID: a null cloud, extent, params or out, n < 1, cell < 1, a bad extent, K or a radius outside the
 * ranges above, radii not strictly increasing, s_num < 0, s_den < 1, a negative dh0, dh_max, tol or min_height.
 * BS_ERR_RANGE: 2^29 points or more; width * height >= 2^31 - 1; a point with a negative x / y or whose pixel lies outside
 * the lattice; a coordinate at or beyond 2^23.  On any of these the outputs and the struct are untouched and the context
 * stays usable: everything before the host's first wait works in scratch of the context. */
#define BS_GROUND_MAX_STEPS 16
#define BS_GROUND_MAX_RADIUS 255
#define BS_GROUND_GRID 2048  /* workgroups of 256 of the two passes over the points: beyond 524 288 points a thread takes several */
#define BS_GROUND_ROW_LDS 2048 /* entries of a row segment in LDS in the x passes: 2048 - 2 r outputs and r of apron each side */

struct bs_ground_params {
  int32_t cell, n_steps;
  int32_t radius[BS_GROUND_MAX_STEPS];
  int32_t s_num, s_den, dh0, dh_max, tol, min_height;
};

struct bs_ground {
  int32_t width, height, cell, n_steps;
  int32_t radius[BS_GROUND_MAX_STEPS], threshold[BS_GROUND_MAX_STEPS];
  int32_t grid, row_lds; /* BS_GROUND_GRID, BS_GROUND_ROW_LDS of the library */
  int32_t dtm_min, dtm_max, hag_min, hag_max;
  int64_t n_points;
  int64_t step_pixels[BS_GROUND_MAX_STEPS];
  int64_t n_ground_pixels, n_object_pixels, n_empty_pixels, n_filled_pixels;
  int64_t n_ground_points, n_low_points, n_object_points, sum_hag_ground;
  /* device time (HIP events on the context's stream) */
  double ms_low;    /* clearing, the check of the cloud, low */
  double ms_open;   /* the K steps and the pass over the pixels (dtm and its figures); the host's read of the range flags */
  double ms_points; /* the pass over the points, the copies into the caller's images, the host's read of the figures */
  double ms_step[BS_GROUND_MAX_STEPS]; /* each step of ms_open */
};

/* d_xyz is a device pointer.  d_low, d_dtm ([height][width] int32), d_step ([height][width] uint8), d_hag ([n] int32) and
 * d_class ([n] uint8) are device buffers; each may be NULL.  The figures are always computed.  All K steps are launched
 * without a host round trip.  Synchronises: once for the range flags, once for the result. */
int bs_ground_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, const int32_t* extent, const struct bs_ground_params* params,
                  int32_t* d_low, int32_t* d_dtm, uint8_t* d_step, int32_t* d_hag, uint8_t* d_class, struct bs_ground* out);
/* Host-memory twin: xyz and the five outputs (each may be NULL) are host pointers. */
int bs_ground(bs_ctx* ctx, const int32_t* xyz, int64_t n, const int32_t* extent, const struct bs_ground_params* params,
              int32_t* low, int32_t* dtm, uint8_t* step, int32_t* hag, uint8_t* cls, struct bs_ground* out);
/* Zeroes the struct (it owns no memory); accepts a zeroed struct and NULL. */
void bs_ground_free(struct bs_ground* g);

/* ---- ground model: the 2-D branch relative to a terrain raster ----
 *
 * A switch of the context, as bs_set_building_bases.  dtm [height][width] int32 is a host table over a lattice of `cell`
 * millimetres (in the pipeline: dtm of bs_ground), INT32_MAX where it holds nothing; the context keeps a device copy.  A NULL
 * table switches it off, which is the default.  While it is set, bs_grid_picture*, bs_assign_buildings* and bs_roofs* decide
 * "below ground" per point: wherever their definition says z < ground_th they test
 *     z < dtm[y / cell][x / cell] + min_height          (64-bit)
 * and a point with a negative x or y, whose model pixel lies outside the table, or whose model pixel is INT32_MAX falls back
 * to z < ground_th.  ground_th is still computed, taken and returned as before.  bs_grid_picture_batch* with more than one
 * tile refuse with BS_ERR_INVALID while it is set (one table cannot serve two tiles); the solo forms and a batch of one work.
 * Switched off, every byte these stages write is what they write without this paragraph.
 * BS_ERR_INVALID: width, height or cell < 1, width * height >= 2^31 - 1, min_height < 0. */
int bs_set_ground_model(bs_ctx* ctx, const int32_t* dtm, int32_t width, int32_t height, int32_t cell, int32_t min_height);
/* The same from a device table (copied on the context's stream; the call waits for the copy). */
int bs_set_ground_model_dev(bs_ctx* ctx, const int32_t* d_dtm, int32_t width, int32_t height, int32_t cell,
                            int32_t min_height);
/* The four numbers of the model (all 0 while it is off) and its first min(capacity, width * height) entries into dtm, which
 * may be NULL with capacity == 0.  BS_ERR_INVALID: a null number, a negative capacity, or a null dtm with capacity > 0. */
int bs_get_ground_model(bs_ctx* ctx, int32_t* dtm, int64_t capacity, int32_t* width, int32_t* height, int32_t* cell,
                        int32_t* min_height);

/* ---- plane quality: which planes of the segmentation are planes ----
 *
 * Host only, no context.  The grower cuts slabs of th_thickness out of anything dense, a tree crown included; the fit tells
 * them apart.  ok [n_planes] uint8, entry p - 1 is plane p:
 *     ok = status == 0 && n_points >= min_points && r_sq_sum <= (int64) max_rms * max_rms * n_points
 * that is, the rms residual of the least-squares plane is at most max_rms millimetres.  Integers only.  Only n_planes, status,
 * n_points and r_sq_sum of f are read.
 * BS_ERR_INVALID: f NULL, n_planes < 0, a NULL array or ok with n_planes > 0, min_points < 0, max_rms outside 0 .. 32767. */
int bs_plane_quality(const struct bs_plane_fits* f, int64_t min_points, int32_t max_rms, uint8_t* ok);

/* ---- roof evidence: the share of the points above ground that lie on a good plane, per pixel ----
 *
 * bs_footprints makes a building of every connected blob of pixels that a point above ground touches; a tree is such a blob.
 * This stage says per pixel whether what stands there looks like a roof, and bs_set_footprint_screen below lets the footprints
 * take it into account.  The cloud is shifted to its origin; the lattice is bs_grid_dims(extent, bin) = (width, height).
 * All exact integers:
 *   - a point COUNTS iff it is not below ground by the rule of the raster: !(z < ground_th), or, while bs_set_ground_model is
 *     set, the per-point rule of that paragraph;
 *   - the pixel of a point is (x / bin, y / bin), the base pixel of its splat, as in bs_assign_buildings;
 *   - above[pix] = the counting points of the pixel; planar[pix] = those of them with 1 <= plane_idx <= n_planes and
 *     plane_ok[plane_idx - 1] != 0 (plane_ok NULL: every plane counts).  Every other label is unlabelled, as in
 *     bs_plane_buildings;
 *   - A[pix], P[pix] = the sums of above and planar over the square [x - r, x + r] x [y - r, y + r] clipped to the image;
 *   - keep[pix] = A >= min_points && (int64) P * den >= (int64) num * A.
 * With r >= 1 the window covers the far pixels of a point's bilinear splat.  With r = 0 a pixel that only a neighbour's splat
 * touches has A = 0 and is rejected: r = 0 under the screen eats the east and south rim of every footprint.
 * 0 <= r <= BS_EVIDENCE_RMAX, min_points >= 1, den >= 1, 0 <= num <= den.
 * Outputs: keep uint8 [height][width] (0 / 1); above, planar, win_above (A), win_planar (P) int32 [height][width], each may
 * be NULL.  plane_ok [n_planes] is a host table in both forms.
 * BS_ERR_INVALID: a null pointer (keep and out included), n < 1, bin < 1, n_planes < 0, a bad extent or parameter.
 * BS_ERR_RANGE: n >= 2^29, width * height >= 2^31 - 1, or a point with a negative x or y or whose pixel lies outside the
 * lattice.  On an error no output and nothing of `out` is written. */
#define BS_EVIDENCE_RMAX 15
#define BS_EVIDENCE_TILE 32  /* a workgroup of the window kernel writes TILE x TILE pixels */
#define BS_EVIDENCE_GRID 256 /* workgroups of the window kernel: beyond 256 tiles a workgroup takes several */
struct bs_roof_evidence {
  int32_t width, height;
  int32_t r, min_points, num, den; /* of the call */
  int32_t grid, tile;              /* BS_GROUND_GRID (the pass over the points), BS_EVIDENCE_TILE of the library */
  int32_t max_window;              /* the largest A */
  int32_t pad_;
  int64_t n_points;        /* n */
  int64_t n_counted;       /* points that count: the sum of above */
  int64_t n_planar;        /* of them on a plane that counts: the sum of planar */
  int64_t n_pixels;        /* pixels with above > 0 */
  int64_t pixels_kept;     /* keep == 1 */
  int64_t pixels_rejected; /* A >= min_points, share too low */
  int64_t pixels_thin;     /* 0 < A < min_points */
  /* device time (HIP events on the context's stream) */
  double ms_counts; /* the pass over the points (with the clearing of its image) */
  double ms_window; /* window sums, keep, images and figures */
};
/* d_xyz [n][3], d_plane_idx [n] int32 and the images are device pointers. */
int bs_roof_evidence_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, const int32_t* d_plane_idx, int32_t n_planes,
                         const uint8_t* plane_ok, const int32_t* extent, int32_t bin, double ground_th, int32_t r,
                         int32_t min_points, int32_t num, int32_t den, uint8_t* d_keep, int32_t* d_above, int32_t* d_planar,
                         int32_t* d_win_above, int32_t* d_win_planar, struct bs_roof_evidence* out);
/* The same from and into host memory. */
int bs_roof_evidence(bs_ctx* ctx, const int32_t* xyz, int64_t n, const int32_t* plane_idx, int32_t n_planes,
                     const uint8_t* plane_ok, const int32_t* extent, int32_t bin, double ground_th, int32_t r,
                     int32_t min_points, int32_t num, int32_t den, uint8_t* keep, int32_t* above, int32_t* planar,
                     int32_t* win_above, int32_t* win_planar, struct bs_roof_evidence* out);

/* ---- footprint screen: footprints of the pixels that pass a test ----
 *
 * A switch of the context, as bs_set_ground_model.  keep [height][width] uint8 (in the pipeline: keep of bs_roof_evidence over
 * the raster's lattice); a NULL image switches it off, which is the default.  While it is set, step 2 of bs_footprints[_dev]
 * reads "foreground iff q > threshold AND keep[pixel] != 0"; the quantisation, the closing, the labelling, the tracing and
 * the mask output are unchanged.  A call whose width / height differ from the screen's returns BS_ERR_INVALID, and so does
 * bs_footprints_batch* with more than one tile (one image cannot serve two tiles); a batch of one works.  Switched off,
 * every byte the footprints write is what they write without this paragraph.
 * BS_ERR_INVALID: width or height < 1, width * height >= 2^31 - 1. */
int bs_set_footprint_screen(bs_ctx* ctx, const uint8_t* keep, int32_t width, int32_t height);
/* The same from a device image, which is NOT copied: the context keeps d_keep and every later footprints call reads whatever it
 * holds then.  It must stay allocated until the switch is cleared or set again. */
int bs_set_footprint_screen_dev(bs_ctx* ctx, const uint8_t* d_keep, int32_t width, int32_t height);
/* width and height of the screen (0 while it is off) and its first min(capacity, width * height) bytes into keep, which may
 * be NULL with capacity == 0.  BS_ERR_INVALID: a null number, a negative capacity, or a null keep with capacity > 0. */
int bs_get_footprint_screen(bs_ctx* ctx, uint8_t* keep, int64_t capacity, int32_t* width, int32_t* height);

/* ---- oriented boxes: the convex hull and the minimum-area enclosing rectangle of every label ----
 *
 * Input: a label image as for the facet outlines: label[height][width] of int32, negative = outside, else 0 .. n_labels - 1
 * (the building map of bs_building_map is one, the facet image of bs_roof_facets another).  C(l) is the set of lattice
 * corners of all pixels of label l; orient(a, b, c) = (bx - ax)(cy - ay) - (by - ay)(cx - ax) in int64.
 *
 * Hull.  H(l) is the list of the strict vertices of the convex hull of C(l): orient(prev, v, next) > 0 at every vertex, no
 * collinear vertex.  The order is the outlines' own (positive shoelace sum in (X, Y)); the list begins at the vertex with the
 * lowest corner index Y * (width + 1) + X, which is always a hull vertex.  hull_area2 is the shoelace sum in int64.  Every
 * hull vertex is the corner of a pixel that lies inside the hull, so every interior angle is at least 90 degrees and
 * n_hull >= 4 for every label with a pixel; the lowest row of corners holds a whole pixel side, so the hull has a
 * horizontal edge.
 *
 * Box.  For hull edge i let s = H[i], e = H[(i + 1) % n_hull], d = e - s, len2 = |d|^2, and over all p of H
 *   a(p) = (p - s) . d            with minimum a_min <= 0 and maximum a_max >= len2,
 *   c(p) = orient(s, e, p) >= 0   with maximum c_max > 0,
 *   area_num_i = (a_max - a_min) * c_max:
 * the rectangle with a side on edge i has the area area_num_i / len2_i.  best_edge is the edge of least area, compared
 * exactly as area_num_i * len2_j < area_num_j * len2_i (128 bits), the lowest i on a tie.  A minimum-area enclosing rectangle
 * always has a side on a hull edge, so this is the minimum-area rectangle.
 *
 * Bound.  A label whose box of lattice corners is wider or higher than BS_HULL_MAX_SIDE has the status BS_HULL_TOO_LARGE:
 * its box and pixels2 are reported, its n_hull and every other figure are 0.  Below the bound |a|, a_max - a_min and c_max
 * are under 2^29, area_num under 2^58 and the compared products under 2^87.  A label without a pixel has BS_HULL_EMPTY and
 * nothing but zeros.
 *
 * Per label: status, box[4] = {X0, Y0, X1, Y1} (inclusive, of its corners), pixels2 (twice its pixels), n_hull,
 * hull_offset[n_labels + 1] into hull_xy, hull_area2, best_edge, dir[2] = the d of the best edge (not reduced), len2,
 * a_min, a_max, c_max, area_num.  Totals: n_hull_vertices, n_ok, n_empty, n_too_large.  Vertices: hull_xy
 * [n_hull_vertices][2].  Everything above is an exact integer and independent of how the device pass is laid out.
 *
 * Identities.  hull_area2 >= pixels2.  2 * area_num >= hull_area2 * len2.  area_num <= (X1 - X0) * (Y1 - Y0) * len2 (the
 * horizontal edge).  A full w x h rectangle of one label: n_hull == 4, best_edge == 0, area_num == w * h * len2.  Moving a
 * label inside the image changes only box, hull_xy and the start corner.
 *
 * Layout figures (they depend on the device pass, DESIGN.md "Oriented boxes", and on nothing else): n_candidates, the
 * convex vertices of the outer rings of the labels within the bound; rounds, the QuickHull rounds that still had a live
 * candidate; max_live, the most live candidates at the start of a round. */
#define BS_HULL_MAX_SIDE 16383
#define BS_HULL_ROUND_BATCH 4   /* rounds between two reads of the live count */
#define BS_HULL_ROUND_CAP 16384 /* more rounds than this: BS_ERR_INTERNAL (a hull within the bound cannot need them) */
enum { BS_HULL_OK = 0, BS_HULL_EMPTY = 1, BS_HULL_TOO_LARGE = 2 };
struct bs_label_hulls {
  int32_t width, height;
  int32_t n_labels;
  int32_t reserved;
  int64_t n_hull_vertices, n_ok, n_empty, n_too_large; /* totals */
  int64_t n_candidates, rounds, max_live;              /* layout figures */
  /* per label; host memory owned by the library */
  int32_t* status;      /* [n_labels] */
  int32_t* box;         /* [n_labels][4] */
  int64_t* pixels2;     /* [n_labels] */
  int64_t* n_hull;      /* [n_labels] */
  int64_t* hull_offset; /* [n_labels + 1] */
  int64_t* hull_area2;  /* [n_labels] */
  int32_t* best_edge;   /* [n_labels] */
  int32_t* dir;         /* [n_labels][2] */
  int64_t* len2;        /* [n_labels] */
  int64_t* a_min;       /* [n_labels] */
  int64_t* a_max;       /* [n_labels] */
  int64_t* c_max;       /* [n_labels] */
  int64_t* area_num;    /* [n_labels] */
  /* the hull vertices, host memory owned by the library: filled by the host-memory entry point only (NULL after the count) */
  int32_t* hull_xy; /* [n_hull_vertices][2] */
  /* device time (HIP events on the context's stream) */
  double ms_outlines;   /* the plain outline count underneath */
  double ms_candidates; /* boxes and status per label, the candidates, the seeds */
  double ms_rounds;     /* the first assignment and the QuickHull rounds */
  double ms_order;      /* the sort into walk order, the strict vertices, the offsets */
  double ms_boxes;      /* every edge's rectangle and the best per label */
  double ms_emit;       /* the emit (host-memory entry point only) */
};

/* Hulls, boxes and sizes.  d_label is a device pointer.  Runs bs_facet_outlines_count_dev (without top) on the image first:
 * its context state is replaced, as by the simplified count.  The hull vertices stay in the context for the emit below; out's
 * arrays are host memory owned by the library (bs_label_hulls_free, which accepts a zeroed struct).  An image without a
 * labelled pixel is valid: every label BS_HULL_EMPTY.
 * The errors are exactly those of bs_facet_outlines_count_dev (BS_ERR_INVALID, BS_ERR_RANGE).  On any error out is left
 * untouched, and the context stays usable.  Synchronises: the three times of the outline count, once for the candidate
 * count, once every BS_HULL_ROUND_BATCH rounds, once for the results (once in all without a labelled pixel). */
int bs_label_hulls_count_dev(bs_ctx* ctx, const int32_t* d_label, int32_t width, int32_t height, int32_t n_labels,
                             struct bs_label_hulls* out);
/* The hull vertices of the last successful count on this context into a device buffer of exactly its size: d_hull_xy
 * [n_hull_vertices][2] (may be NULL without a vertex).  May be called more than once.  BS_ERR_INVALID: no successful count
 * (the last one on this context failed, or there was none), or d_hull_xy NULL.  Synchronises. */
int bs_label_hulls_emit_dev(bs_ctx* ctx, int32_t* d_hull_xy);
/* Host-memory twin: label is a host pointer; both steps, and the vertices come back in out's library-owned hull_xy. */
int bs_label_hulls(bs_ctx* ctx, const int32_t* label, int32_t width, int32_t height, int32_t n_labels,
                   struct bs_label_hulls* out);
void bs_label_hulls_free(struct bs_label_hulls* h);

/* The four corners of the rectangle of one label.  Host only, integers.  With s the start of the best edge (hull_xy), d = dir
 * and n = (-dy, dx):  K0 = s + (a_min d) / len2, K1 = s + (a_max d) / len2, K2 = K1 + (c_max n) / len2, K3 = K0 + (c_max n) /
 * len2.  Each coordinate is round(numerator * bin / len2) + origin, the numerator over len2 including s * len2; the division
 * is done once in 128 bits and rounds half away from zero.  origin [2] (NULL: 0).
 * BS_ERR_INVALID: null pointer (origin apart), bin < 1, no hull_xy, a label outside [0, n_labels) or not BS_HULL_OK. */
int bs_hull_box_corners(const struct bs_label_hulls* h, int32_t label, int32_t bin, const int32_t* origin, int64_t out[4][2]);
/* Hulls and rectangles as an OBJ of closed polylines in millimetres.  Host only, no context; origin [3] as for
 * bs_outlines_write_obj (NULL: 0), every Z is origin[2].  The file, every number a decimal integer, every line ended by '\n':
 *   "# oriented boxes: <n_labels> labels, <n_ok> ok, <n_empty> empty, <n_too_large> too large, <n_hull_vertices> hull vertices"
 *   for every BS_HULL_OK label l in order: "g label_<l>_hull", its hull vertices "v X*bin+origin[0] Y*bin+origin[1] origin[2]",
 *   one closed polyline "l i1 ... in i1"; then "g label_<l>_box", the four corners of bs_hull_box_corners as vertices and one
 *   closed polyline.  Vertices are numbered from 1 in file order.
 * BS_ERR_INVALID: as bs_hull_box_corners, hull_offset that does not fit n_hull, or the file cannot be written. */
int bs_hull_boxes_write_obj(const struct bs_label_hulls* h, int32_t bin, const int32_t* origin, const char* path);

#ifdef __cplusplus
}
#endif
#endif /* BS_API_H */
