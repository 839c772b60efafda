/*
 * se3icp.h — C-ABI of the MI355X-native SE(3)-ICP engine (libse3icp.so).
 *
 * Drop-in boundary for the reference's engine class
 *   class IterativeSE3Registration   include/iterative_SE3_registration.hpp:27-99
 * (kenahm/se3-icp).  Plain pointers and sizes only; no C++/torch types.
 *
 * Two surfaces:
 *   1. The object surface mirrors the reference class member for member
 *      (constructor, setSourceCloud/setTargetCloud, public config fields,
 *      run_icp / run_se3_icp / run_se3_icp_with_cf / run_se3_pure, and the
 *      result fields current_estimated_T_, num_iterations_,
 *      num_pure_se3_iterations_).  A binding for the reference would map each
 *      call 1:1.
 *   2. The batch surface registers many independent scan pairs in lockstep on
 *      one GPU (the loop the reference's benchmark drivers run serially,
 *      examples/benchmark_kitti.cpp:120-197), from host or device (HBM) buffers.
 *
 * Errors: functions return 0 on success and a negative se3icp_status otherwise;
 * se3icp_status_string() describes a code.  Point arrays are AoS xyz float64
 * (n*3 doubles), the layout of open3d::geometry::PointCloud::points_.
 * Matrices are 4x4 row-major float64.
 */
#ifndef SE3ICP_H
#define SE3ICP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SE3ICP_ABI_VERSION 4

typedef enum se3icp_status {
    SE3ICP_OK = 0,
    SE3ICP_ERR_INVALID_ARG = -1,
    SE3ICP_ERR_INVALID_METHOD = -2,   /* name not in the reference's whitelist */
    SE3ICP_ERR_EMPTY_CLOUD = -3,
    SE3ICP_ERR_K_TOO_LARGE = -4,      /* unused since ABI 3: number_of_nn_for_LRF is unbounded, as
                                         the reference's (ISR.hpp:80, ISR.cpp:253); k beyond what
                                         HBM holds fails with SE3ICP_ERR_OUT_OF_MEMORY */
    SE3ICP_ERR_NO_DEVICE = -5,        /* no HIP device / kernels not loadable: never a CPU fallback */
    SE3ICP_ERR_HIP = -6,              /* HIP runtime error */
    SE3ICP_ERR_NONFINITE = -7,        /* NaN/Inf in the resulting pose */
    SE3ICP_ERR_OUT_OF_MEMORY = -8,
    SE3ICP_ERR_INTERNAL = -9          /* a kernel left a result unset or out of range (se3icp_nn: an index
                                         outside the data cloud); the outputs are not to be used */
} se3icp_status;

/* Registration methods.  Names match examples/run_registration_method.cpp:19-24
 * ("pt2pt","pt2pl","gicp","se3_pt2pt","se3_pt2pl","se3_gicp") plus the two run
 * methods the CLI does not expose (run_se3_icp_with_cf, run_se3_pure). */
typedef enum se3icp_method {
    SE3ICP_PT2PT = 0,            /* run_icp("pt2pt")       ISR.cpp:473-552 */
    SE3ICP_PT2PL = 1,            /* run_icp("pt2pl")                        */
    SE3ICP_GICP = 2,             /* run_icp("gicp")                         */
    SE3ICP_SE3_PT2PT = 3,        /* run_se3_icp("pt2pt")   ISR.cpp:555-739 */
    SE3ICP_SE3_PT2PL = 4,        /* run_se3_icp("pt2pl")                    */
    SE3ICP_SE3_GICP = 5,         /* run_se3_icp("gicp")                     */
    SE3ICP_SE3_GICP_WITH_CF = 6, /* run_se3_icp_with_cf()  ISR.cpp:742-959 */
    SE3ICP_SE3_PURE_PT2PT = 7,   /* run_se3_pure("pt2pt")  ISR.cpp:962-1127 */
    SE3ICP_SE3_PURE_PT2PL = 8,
    SE3ICP_SE3_PURE_GICP = 9,
    SE3ICP_NUM_METHODS = 10
} se3icp_method;

/* Public config fields of IterativeSE3Registration (ISR.hpp:80-95); defaults are
 * the constructor's (ISR.cpp:334-348). */
typedef struct se3icp_params {
    int32_t max_num_iterations;     /* 150   max_num_iterations_       */
    int32_t max_num_se3_iterations; /* 20    max_num_se3_iterations_   */
    int32_t number_of_nn_for_LRF;   /* 30    number_of_nn_for_LRF_     */
    int32_t _reserved;
    double mse;                     /* 1e-5  mse_                      */
    double mse_switch_error;        /* 1e-3  mse_switch_error_         */
    double estimated_overlap;       /* 1.0   estimated_overlap_        */
    double alpha_rot;               /* 3.0   alpha_rot                 */
    double beta_transl;             /* 1.0   beta_transl               */
    double scale_preprocessing;     /* 3.0   scale_preprocessing       */
} se3icp_params;

/* Result of one registration (the reference's result members, ISR.hpp:85-98). */
typedef struct se3icp_result {
    double T[16];                     /* current_estimated_T_ (row-major)       */
    int32_t num_iterations;           /* num_iterations_                        */
    int32_t num_pure_se3_iterations;  /* num_pure_se3_iterations_ (-1 for run_icp, as the ctor) */
    int32_t status;                   /* se3icp_status of this pair             */
    int32_t num_rechecked;            /* NN queries re-resolved in f64 (diagnostic) */
    double scaling_factor;            /* 3 / max radius (1 for run_icp)         */
    double time_setup_ms;             /* normalization + TOLDI + normals (batch, GPU timeline) */
    double time_loop_ms;              /* ICP loop (batch, GPU timeline)                        */
    double time_se3_correspondence_search_ms; /* time_se3_correspondence_search_ */
    double time_before_pure_icp_ms;   /* time_before_pure_icp_: the whole run_se3_icp_with_cf
                                         (ISR.cpp:754, 957-958), GPU timeline; 0 for the other
                                         methods (the reference never sets it there).
                                         The times above are BATCH-WIDE: a batch of n_pairs > 1
                                         registers its pairs in lockstep, and every pair gets
                                         the batch's setup / loop / NN / total time, not a
                                         per-pair share (the reference times one registration;
                                         a batched caller divides by the batch size for a mean).
                                         After a sweep they are GROUP-WIDE: the shared setup plus
                                         the group's own expansion and 12-D trees, and the group's
                                         loop / NN times (parameter sweeps, below). */
} se3icp_result;

/* ------------------------------------------------------------- misc */
int se3icp_abi_version(void);
const char* se3icp_status_string(int status);
/* "se3_pt2pl" -> SE3ICP_SE3_PT2PL ...; also "se3_gicp_with_cf", "se3_pure_pt2pt" ...
 * Returns SE3ICP_ERR_INVALID_METHOD for any other string. */
int se3icp_method_from_name(const char* name);
const char* se3icp_method_name(int method);
void se3icp_default_params(se3icp_params* p);
/* Number of visible HIP devices (0 if none). */
int se3icp_device_count(void);

/* ------------------------------------------------------------- object surface
 * Mirrors IterativeSE3Registration (ISR.hpp:27-99). One object = one pair,
 * single use, like the reference (its run_* normalize member clouds in place). */
typedef struct se3icp_registration se3icp_registration;

se3icp_registration* se3icp_registration_new(void);           /* IterativeSE3Registration()   ISR.cpp:334 */
void se3icp_registration_free(se3icp_registration* r);
/* setSourceCloud(const PointCloud&) ISR.cpp:358-366 — APPENDS like the reference */
int se3icp_set_source_cloud(se3icp_registration* r, const double* xyz, int64_t n);
/* setTargetCloud(const PointCloud&) ISR.cpp:372-376 — appends */
int se3icp_set_target_cloud(se3icp_registration* r, const double* xyz, int64_t n);
/* the public config fields */
se3icp_params* se3icp_params_of(se3icp_registration* r);
/* run_icp(variant)  ISR.cpp:473 ;  variant in {"pt2pt","pt2pl","gicp"} */
int se3icp_run_icp(se3icp_registration* r, const char* variant);
/* run_se3_icp(variant)  ISR.cpp:555 */
int se3icp_run_se3_icp(se3icp_registration* r, const char* variant);
/* run_se3_icp_with_cf()  ISR.cpp:742 */
int se3icp_run_se3_icp_with_cf(se3icp_registration* r);
/* run_se3_pure(variant)  ISR.cpp:962 */
int se3icp_run_se3_pure(se3icp_registration* r, const char* variant);
/* result members */
int se3icp_get_result(const se3icp_registration* r, se3icp_result* out);

/* ------------------------------------------------------------- batch surface
 * Register n_pairs independent (source, target) pairs with one method and one
 * parameter set, on device `device` (HIP ordinal).  Host buffers.
 * Every entry taking `device` accepts `ordinal | slot << 8` (slot 0..15): slot s > 0 is a
 * further engine on the same GPU with its own stream and buffers, so independent batches
 * may be registered from several host threads at once (one engine serialises its calls). */
int se3icp_register_batch(int device, int32_t n_pairs, const double* const* src_xyz, const int64_t* n_src,
                          const double* const* tgt_xyz, const int64_t* n_tgt, int method,
                          const se3icp_params* params, se3icp_result* results);

/* Same, with all clouds already resident in HBM: d_src_xyz / d_tgt_xyz are
 * device pointers to the concatenation of every pair's AoS xyz; the host arrays
 * src_off/tgt_off (n_pairs+1 entries) give each pair's point range.
 * `hip_stream` is a hipStream_t (NULL = the engine's own stream); every kernel of the batch
 * runs on it, so work queued on `hip_stream` before the call is ordered before them. */
int se3icp_register_batch_device(int device, int32_t n_pairs, const double* d_src_xyz, const int64_t* src_off,
                                 const double* d_tgt_xyz, const int64_t* tgt_off, int method,
                                 const se3icp_params* params, se3icp_result* results, void* hip_stream);

/* ------------------------------------------------------------- parameter sweeps
 * The outer loop of the reference's benchmark drivers: the whole dataset registered once
 * per value of a parameter grid (makeHybridLGrid(), examples/benchmark_kitti.cpp:354-393).
 *
 * Register every pair under every parameter set of `variants` with ONE setup.
 * results[v * n_pairs + p]: pair p under variants[v], bitwise what
 * se3icp_register_batch(..., &variants[v], ...) returns for pair p
 * (T, num_iterations, num_pure_se3_iterations, status, scaling_factor;
 * not the times, not num_rechecked).
 * All variants share `method`, number_of_nn_for_LRF and scale_preprocessing
 * (else SE3ICP_ERR_INVALID_ARG): those shape the shared setup.  Every other
 * field may differ per variant.  The vanilla methods (pt2pt, pt2pl, gicp) have no frames:
 * their sweep shares ingest, 3-D trees and normals and varies the loop parameters only.
 * max_group: variants registered in lockstep at once (0 = engine's choice: up to 8, while
 * a group stays within 2^26 points, device memory and the 2^30 points of a batch).
 * Arguments are checked before the device is looked up (SE3ICP_ERR_INVALID_ARG for
 * n_variants <= 0, variants == NULL, max_group < 0; SE3ICP_ERR_INVALID_METHOD;
 * SE3ICP_ERR_EMPTY_CLOUD); without a device SE3ICP_ERR_NO_DEVICE, never a CPU fallback.
 * Returns as se3icp_register_batch: OK, or SE3ICP_ERR_NONFINITE when some result is
 * non-finite, each result's `status` set.
 * Times of a result: time_setup_ms is the shared setup plus its group's expansion and 12-D
 * trees; time_loop_ms and time_se3_correspondence_search_ms are its group's (GROUP-WIDE,
 * as a batch's are batch-wide); time_before_pure_icp_ms as for a batch, from those two.
 * se3icp_last_kernel_times(_n) after a sweep: the setup entries (lrf_*, setup_ms) are the one
 * shared setup's, the loop entries are summed over the groups.
 * se3icp_set_trace before a sweep: trace.pair indexes the result array, v * n_pairs + p; the
 * group that holds it runs without look-ahead; the trace disarms after the call. */
int se3icp_register_sweep(int device, int32_t n_pairs, const double* const* src_xyz, const int64_t* n_src,
                          const double* const* tgt_xyz, const int64_t* n_tgt, int method, int32_t n_variants,
                          const se3icp_params* variants, int32_t max_group, se3icp_result* results);
/* Same, with the clouds resident in HBM (see se3icp_register_batch_device). */
int se3icp_register_sweep_device(int device, int32_t n_pairs, const double* d_src_xyz, const int64_t* src_off,
                                 const double* d_tgt_xyz, const int64_t* tgt_off, int method, int32_t n_variants,
                                 const se3icp_params* variants, int32_t max_group, se3icp_result* results,
                                 void* hip_stream);

/* ------------------------------------------------------------- cloud graphs
 * What the reference's drivers actually hand over: a set of scans and the pairs to register
 * among them (examples/benchmark_kitti.cpp:101-131 registers scan i+1 onto scan i, so every
 * interior scan is the target of one pair and the source of the next); likewise scans
 * localised against one map, or the loop-closure edges of a pose graph.
 *
 * n_clouds distinct clouds; pair p registers clouds[src_cloud[p]] onto clouds[tgt_cloud[p]].
 * results[p] is bitwise what se3icp_register_batch returns for that pair (T, both iteration
 * counts, status, scaling_factor; not the times, not num_rechecked).
 * A self edge (src == tgt), a repeated edge, a cloud no edge uses (never read, may be empty)
 * and any edge order are valid.
 * sharing: 0 engine's choice (= 3); 1 upload / ingest / centroid / radius once per cloud;
 * 2 also one neighbour selection (exact kNN, TOLDI frames, normals: the bulk of the setup) per
 * (cloud, normalization) class -- the uses of a cloud whose pairs give it the same scale
 * (run_se3_*: scale_preprocessing / max(r_src, r_tgt)); for pt2pt / pt2pl / gicp, which keep
 * raw coordinates, one per cloud; 3 reserved for neighbour-set adoption between the classes
 * of one cloud, which is not built: it behaves as 2.  Every level returns the same bits.
 * The saving is upload and setup compute, NOT memory: the loop's state lives at a use's own
 * slots, so each of the 2 * n_pairs uses is materialised (normalized copy and 3-D kd-tree of
 * its own), and the distinct clouds' raw coordinates are held beside them.  Planning the
 * classes needs the clouds' centroids and radii on the host: one synchronisation more than a
 * batch.
 * Arguments are checked before the device is looked up: SE3ICP_ERR_INVALID_ARG for
 * n_clouds <= 0, n_pairs <= 0, NULL arrays, an index outside [0, n_clouds), sharing outside
 * 0..3; SE3ICP_ERR_INVALID_METHOD; SE3ICP_ERR_EMPTY_CLOUD for an empty cloud some edge uses;
 * without a device SE3ICP_ERR_NO_DEVICE, never a CPU fallback.
 * se3icp_set_trace before the call: trace.pair is the edge index.  se3icp_set_lrf_exact
 * applies to every class.  se3icp_last_kernel_times(_n): the setup entries (lrf_*) are the
 * classes' one selection each; setup_ms spans upload to the loop's start. */
int se3icp_register_graph(int device, int32_t n_clouds, const double* const* xyz, const int64_t* n_pts,
                          int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud, int method,
                          const se3icp_params* params, int32_t sharing, se3icp_result* results);
/* Same, with the clouds resident in HBM: d_xyz is the concatenation of every cloud's AoS xyz,
 * off (n_clouds + 1 host entries) each cloud's point range (see se3icp_register_batch_device
 * for hip_stream). */
int se3icp_register_graph_device(int device, int32_t n_clouds, const double* d_xyz, const int64_t* off,
                                 int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud, int method,
                                 const se3icp_params* params, int32_t sharing, se3icp_result* results,
                                 void* hip_stream);
/* The same plus a report per edge (registration reports, below); the per-point buffers of
 * opts are laid out per edge at the prefix sum of the edges' n_src, as for a batch. */
struct se3icp_report_options;
struct se3icp_report;
int se3icp_register_graph_report(int device, int32_t n_clouds, const double* const* xyz, const int64_t* n_pts,
                                 int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud, int method,
                                 const se3icp_params* params, int32_t sharing, se3icp_result* results,
                                 const struct se3icp_report_options* opts, struct se3icp_report* reports);
int se3icp_register_graph_report_device(int device, int32_t n_clouds, const double* d_xyz, const int64_t* off,
                                        int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud,
                                        int method, const se3icp_params* params, int32_t sharing,
                                        se3icp_result* results, void* hip_stream,
                                        const struct se3icp_report_options* opts, struct se3icp_report* reports);
/* Counters of the last graph call on `device`: out[SE3ICP_GRAPH_STATS_N], n >= that (else
 * SE3ICP_ERR_INVALID_ARG) = {distinct clouds some edge uses, uses (2 * n_pairs), classes,
 * classes that ran a full neighbour selection, queries adopted, queries rejected by order,
 * queries rejected by gap, queries without a list (the last four: adoption, always 0),
 * bytes uploaded}.  A class whose selection started from a sibling's neighbour distances
 * (se3icp_set_lrf_seeding, below) ran a full, self-certifying selection and counts as one: it
 * adopted nothing. */
#define SE3ICP_GRAPH_STATS_N 9
int se3icp_last_graph_stats(int device, int64_t* out, int n);

/* The device batch entries (se3icp_register_batch_device, _report_device) cannot be told that
 * two of their 2 * n_pairs cloud slots hold the same scan -- a chain of scans expanded into
 * pairs holds every interior scan twice -- so they look.  Slots of equal point count are
 * hashed on the device over their raw xyz bytes (64 bits, keyed with the count); slots of equal
 * (count, hash) are compared byte for byte on the device against the first of them, and only
 * a confirmed slot shares: never a hash match alone, a pointer or a batch position (-0.0 is
 * not +0.0 here, and a NaN is itself).  With a confirmed duplicate the neighbour selection
 * runs once per (cloud, normalization) class as in se3icp_register_graph at sharing 2, on the
 * slots as they lie (nothing is uploaded or moved); without one the call is the plain batch
 * plus the hash pass, and without two slots of one point count nothing is hashed at all.
 * results[p] is bitwise what the plain batch returns.  A call that looks waits twice for the
 * device during the setup (the hashes, with the normalization parameters the classes are
 * planned from; the compare flags, only when some hash agreed) where the plain batch waits
 * not at all (run_se3_*) or once.
 * level: 0 the highest level that is built (= 2, the default of every engine), 1 off (the
 * plain batch), 2 one selection per class.  Anything else is SE3ICP_ERR_INVALID_ARG, checked
 * before the device is looked up.  The setting is the engine's (device | slot << 8) and holds
 * until it is set again.  Neighbour-set adoption between the classes of one cloud is not
 * built here either; what a cloud's later classes do take from its first is a starting bound
 * for their own selection (se3icp_set_lrf_seeding, below).  The host-pointer entries and the sweeps do not look: a caller with host
 * buffers has se3icp_register_graph, which also uploads every cloud once.
 * se3icp_last_graph_stats after a device batch at level 0 or 2: {distinct clouds, slots,
 * classes, classes that selected, 0, 0, 0, 0, 0}. */
int se3icp_set_batch_sharing(int device, int level);

/* Seeding.  Where a cloud has several classes (se3icp_register_graph at sharing >= 2, a device
 * batch that found a shared cloud) under the run_se3_* normalization, they differ in the pair's
 * scale only: every squared distance of a later class is (s_b / s_a)^2 times the first class's
 * up to rounding.  The cloud's first selecting class stores each point's Kw-th neighbour
 * distance and a later class starts its selection from the bound that gives instead of from
 * infinity.  The later class still runs a full selection in its own arithmetic, and that
 * selection certifies itself (its closing bound must come out at or below the seeded one, else
 * its queries go to the exact kernel): no neighbour set is taken over, a wrong seed costs time
 * and never a result, and results are bitwise the unseeded ones.  So a seeded class counts in
 * `classes that ran a full neighbour selection` of se3icp_last_graph_stats, whose nine values
 * keep their meaning and whose four adoption counters stay 0.
 * mode: 0 seeded (the default of every engine), 1 off, 2 every seed halved before use (a
 * diagnostic: the certificate fails and the exact kernel takes the queries), 3 every seed
 * multiplied by 4 (a diagnostic: loose seeds).  Anything else is SE3ICP_ERR_INVALID_ARG, checked
 * before the device is looked up.  The setting is the engine's (device | slot << 8).  The
 * host-pointer batch entries, the sweeps and the se3icp_set_lrf_exact modes do not seed. */
int se3icp_set_lrf_seeding(int device, int mode);
/* Of the last registration call on `device`: out[SE3ICP_SEED_STATS_N], n >= that (else
 * SE3ICP_ERR_INVALID_ARG) = {classes seeded, queries of wavefronts that started from a seed,
 * queries of wavefronts of seeded classes that ran without one (a neighbour's seed absent: the
 * first class handed that point to the exact kernel; a cloud's last, partial, wavefront),
 * queries handed to the exact kernel after a failed certificate}. */
#define SE3ICP_SEED_STATS_N 4
int se3icp_last_seed_stats(int device, int64_t* out, int n);

/* Taking.  With one kd-tree order per cloud (se3icp_set_tree_sharing, below) a local tree slot
 * names the same point in every class of a cloud.  A seeded class whose selecting slot has its
 * source's tree order, the same cloud and pose, and the same Kw = min(k, n) then takes the
 * source's Kw neighbours of every point as a stored list instead of searching: it recomputes
 * their exact keys under its own scale, puts them in its own order and certifies, from a lower
 * bound the source stored of the distance of everything outside the list, that no other point
 * can be as near as the list's farthest.  A wavefront that cannot certify all of its queries is
 * redone as a seeded one, so a list costs time when it fails and never a result: results are
 * bitwise the same in every mode.  A taking class counts as a class that ran a full selection
 * in se3icp_last_graph_stats (whose adoption counters stay 0, reserved) and its taken queries
 * count as seeded in se3icp_last_seed_stats.  Nothing takes with seeding modes 1-3, without tree
 * sharing, across poses, under se3icp_set_lrf_exact, in the host-pointer batch entries or the
 * sweeps.
 * mode: 0 take (the default of every engine), 1 off, 2 every stored bound halved (a diagnostic:
 * every wavefront is redone).  Anything else is SE3ICP_ERR_INVALID_ARG, checked before the
 * device is looked up.  The setting is the engine's (device | slot << 8). */
int se3icp_set_lrf_taking(int device, int mode);
/* Of the last registration call on `device`: out[SE3ICP_TAKE_STATS_N], n >= that (else
 * SE3ICP_ERR_INVALID_ARG) = {classes taking, queries that took their list, queries of redone
 * wavefronts, queries whose stored list failed the order check or the certificate}.  A query the
 * source handed to the exact kernel has no list: its wavefront is redone and nothing failed. */
#define SE3ICP_TAKE_STATS_N 4
int se3icp_last_take_stats(int device, int64_t* out, int n);

/* One kd-tree order per cloud.  The trees are implicit and balanced, their node ranges come
 * from the point count alone and every search prunes on boxes computed from the points that
 * are in a node, so any order with correct boxes is a valid tree and no result depends on it.
 * Where several slots hold one confirmed cloud (se3icp_register_graph at sharing >= 2, a device
 * batch that found a shared cloud) only the cloud's first slot builds its 3-D and 12-D trees;
 * the later slots, of whatever class, take its finished order and compute their own
 * tree-ordered vectors and boxes from their own coordinates.  Results are bitwise the same.
 * mode: 0 adopt (the default of every engine), 1 off: every slot builds its own trees.
 * Anything else is SE3ICP_ERR_INVALID_ARG, checked before the device is looked up.  The setting
 * is the engine's (device | slot << 8) and does not depend on se3icp_set_lrf_seeding.  The
 * host-pointer batch entries, the sweeps, batch sharing level 1 and graph sharing level 1 adopt
 * nothing. */
int se3icp_set_tree_sharing(int device, int mode);
/* Of the last registration call on `device`: out[SE3ICP_TREE_STATS_N], n >= that (else
 * SE3ICP_ERR_INVALID_ARG) = {3-D trees built, 3-D trees adopted, 12-D trees built, 12-D trees
 * adopted}. */
#define SE3ICP_TREE_STATS_N 4
int se3icp_last_tree_stats(int device, int64_t* out, int n);

/* ------------------------------------------------------------- registration reports
 * What says whether a pose is any good, evaluated at the FINAL pose as Open3D's
 * RegistrationResult and GetInformationMatrixFromPointClouds are.  For every source point i
 * (all of them, no trimming) j(i) is the exact f64 nearest target point of T p_i (lowest
 * index on exact ties) and d_i = |T p_i - x_j|, searched in the engine's frame and reported
 * in the caller's units.  Point i is an inlier iff d_i <= max_correspondence_distance
 * (compared squared, in f64, in the engine's frame); a distance <= 0 or +inf makes every
 * point an inlier, NaN is SE3ICP_ERR_INVALID_ARG.
 * The *_report entries return the same se3icp_result as their plain entries, bit for bit
 * (T, both iteration counts, status, scaling_factor): the report runs after the loop and
 * never writes the loop's state.  time_loop_ms does not include it. */
typedef enum se3icp_stop_reason {
    SE3ICP_STOP_CONVERGED = 0,           /* the method's MSE criterion held (also: a max_num_iterations the
                                            SE(3) phase had already passed by) */
    SE3ICP_STOP_MAX_ITERATIONS = 1,      /* num_iterations reached max_num_iterations */
    SE3ICP_STOP_MAX_SE3_ITERATIONS = 2,  /* run_se3_pure: max_num_se3_iterations reached */
    SE3ICP_STOP_RUNAWAY = 3              /* the engine's 100,000-iteration guard */
} se3icp_stop_reason;

typedef struct se3icp_report_options {
    double max_correspondence_distance;  /* caller's units; <= 0 or +inf: every point is an inlier */
    int32_t* corr_idx;                   /* optional [sum n_src]: j(i), pair p at the prefix sum of n_src */
    double* corr_dist;                   /* optional [sum n_src]: d_i, same layout */
    int32_t outputs_on_device;           /* the two buffers are device pointers */
    int32_t _reserved;
} se3icp_report_options;

typedef struct se3icp_report {
    double fitness;            /* n_inliers / n_src */
    double inlier_rmse;        /* sqrt(sum d_i^2 / n_inliers) over the inliers; 0 without one */
    double information[36];    /* row-major sum G^T G over the inliers, G = [-[x]x  I] of the target point x
                                  (caller's coordinates; rotation first); zeros without an inlier */
    double final_mse;          /* the loop's last MSE and its last change (normalized units, */
    double final_mse_change;   /* see scaling_factor) */
    int64_t n_inliers;
    int32_t switched;          /* the run switched from SE(3) to R3 correspondences */
    int32_t stop_reason;       /* se3icp_stop_reason; when a cap and the criterion hold in the same
                                  iteration the cap is reported (the order of the reference's tests) */
} se3icp_report;

int se3icp_report_version(void);  /* 1 */

/* se3icp_register_batch(_device) plus a report per pair.  opts and reports must not be NULL. */
int se3icp_register_batch_report(int device, int32_t n_pairs, const double* const* src_xyz, const int64_t* n_src,
                                 const double* const* tgt_xyz, const int64_t* n_tgt, int method,
                                 const se3icp_params* params, se3icp_result* results,
                                 const se3icp_report_options* opts, se3icp_report* reports);
int se3icp_register_batch_report_device(int device, int32_t n_pairs, const double* d_src_xyz, const int64_t* src_off,
                                        const double* d_tgt_xyz, const int64_t* tgt_off, int method,
                                        const se3icp_params* params, se3icp_result* results, void* hip_stream,
                                        const se3icp_report_options* opts, se3icp_report* reports);
/* se3icp_register_sweep(_device) plus reports[v * n_pairs + p].  The per-point buffers of
 * opts must be NULL (SE3ICP_ERR_INVALID_ARG otherwise). */
int se3icp_register_sweep_report(int device, int32_t n_pairs, const double* const* src_xyz, const int64_t* n_src,
                                 const double* const* tgt_xyz, const int64_t* n_tgt, int method, int32_t n_variants,
                                 const se3icp_params* variants, int32_t max_group, se3icp_result* results,
                                 const se3icp_report_options* opts, se3icp_report* reports);
int se3icp_register_sweep_report_device(int device, int32_t n_pairs, const double* d_src_xyz, const int64_t* src_off,
                                        const double* d_tgt_xyz, const int64_t* tgt_off, int method,
                                        int32_t n_variants, const se3icp_params* variants, int32_t max_group,
                                        se3icp_result* results, void* hip_stream,
                                        const se3icp_report_options* opts, se3icp_report* reports);
/* Object surface: ask for a report before a run_*, read it after.  The per-point buffers of
 * opts (host pointers, n_src entries) must stay valid until the run returns; opts == NULL
 * withdraws the request.  se3icp_get_report: SE3ICP_ERR_INVALID_ARG when none was requested
 * or no run has produced one. */
int se3icp_request_report(se3icp_registration* r, const se3icp_report_options* opts);
int se3icp_get_report(const se3icp_registration* r, se3icp_report* out);

/* ------------------------------------------------------------- initial poses
 * What Open3D's RegistrationICP(source, target, d, init) and PCL's align(out, guess) take: a
 * pose to start from -- the odometry prior of a chain, the chained odometry of a loop-closure
 * edge, the last pose of a scan against a map.  A pose is a row-major 4x4 f64 matrix, source
 * frame -> target frame, bottom row (0, 0, 0, 1).  The arithmetic is Open3D's Transform and is
 * pinned (csrc/pose.hpp), every step one IEEE f64 operation, no FMA, no division:
 *   apply_pose(M, p)  q[e]    = ((M[4e]*p0 + M[4e+1]*p1) + M[4e+2]*p2) + M[4e+3]*1.0     e = 0..2
 *   compose(A, B)     C[i][j] = ((A[i][0]*B[0][j] + A[i][1]*B[1][j]) + A[i][2]*B[2][j]) + A[i][3]*B[3][j]
 *                     for rows 0..2, row 3 exactly (0, 0, 0, 1)
 *
 * se3icp_register_graph_init(_device): se3icp_register_graph(_report)(_device) with one pose per
 * edge.  With T_init[p] = T0, results[p] is BITWISE what the plain entry returns for the pair
 * (X', target), X' = apply_pose(T0, X) for every point of the source, except T, which is
 * compose(T_plain, T0); both iteration counts, status and scaling_factor are the plain run's on
 * X', and so is a report, per-point outputs included.  X' is never written out: the engine folds
 * the pose into the one read it makes of the raw cloud, and with host buffers every raw cloud is
 * uploaded once however many poses it is used under (se3icp_last_graph_stats: `clouds` and
 * `bytes uploaded` count the distinct RAW clouds).
 * A T0 that is bitwise the identity (zeros +0.0) means "no pose": that edge's source is the raw
 * cloud itself (X, not apply_pose(I, X), which would turn -0.0 into +0.0) and shares its classes,
 * seeds and tree orders with the cloud's other uses.  T_init == NULL is the plain entry, launch
 * for launch.  Equal pose bits on one cloud are one posed copy; kd-tree orders are adopted
 * between the slots of one (cloud, pose) only.
 * se3_gicp_with_cf, A STATED DEPARTURE: the lounge confidences are depths in the camera frame, a
 * sensor quantity, and come from the RAW z of the source.  The equality with the plain entry on
 * X' holds for a T0 that leaves z bitwise unchanged (third row exactly (0, 0, 1, 0)); for any
 * other T0 the call is the plain run on X' with the source's confidences taken from X.
 * opts and reports: both NULL (no report) or both given; exactly one NULL is
 * SE3ICP_ERR_INVALID_ARG.  Checked with the other arguments, before the device is looked up:
 * SE3ICP_ERR_INVALID_ARG for a non-finite entry of a pose or a bottom row that is not bitwise
 * (0, 0, 0, 1).  The 3x3 block is not checked: a block that is not orthonormal is applied as given,
 * as Open3D does, and only keeps that copy out of the seeding below.
 * se3icp_set_trace before a posed call records the plain run on X'. */
int se3icp_init_version(void);  /* 1 */
int se3icp_register_graph_init(int device, int32_t n_clouds, const double* const* xyz, const int64_t* n_pts,
                               int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud,
                               const double* T_init /* n_pairs * 16, or NULL */, int method,
                               const se3icp_params* params, int32_t sharing, se3icp_result* results,
                               const se3icp_report_options* opts, se3icp_report* reports);
int se3icp_register_graph_init_device(int device, int32_t n_clouds, const double* d_xyz, const int64_t* off,
                                      int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud,
                                      const double* T_init /* host, n_pairs * 16, or NULL */, int method,
                                      const se3icp_params* params, int32_t sharing, se3icp_result* results,
                                      void* hip_stream, const se3icp_report_options* opts, se3icp_report* reports);
/* Object surface: every later run_* of the object starts from T and returns the posed result
 * (current_estimated_T_ is the composed pose; a requested report follows).  T == NULL clears. */
int se3icp_set_initial_transform(se3icp_registration* r, const double* T);
/* A posed copy of a cloud is the cloud moved rigidly, so under the run_se3_* normalization its
 * neighbour distances are the raw cloud's up to rounding: the first selecting class of a raw
 * cloud, under whatever pose, seeds the later classes of all its copies whose pose is rigid
 * (max |R^T R - I| <= 2^-30), exactly as se3icp_set_lrf_seeding describes for the classes of one
 * cloud -- self-certifying, bitwise the unseeded results; its modes 1-3 act on these seeds too.
 * mode: 0 seeded across poses (the default of every engine), 1 within one (cloud, pose) only.
 * Anything else is SE3ICP_ERR_INVALID_ARG, checked before the device is looked up. */
int se3icp_set_pose_seeding(int device, int mode);
/* Of the last graph call on `device`: out[SE3ICP_INIT_STATS_N], n >= that (else
 * SE3ICP_ERR_INVALID_ARG) = {edges with a pose, posed copies ingested, classes seeded from a class
 * of another pose of their cloud}. */
#define SE3ICP_INIT_STATS_N 3
int se3icp_last_init_stats(int device, int64_t* out, int n);
/* out[i] = apply_pose(T, xyz[i]) for n points on the host (no device needed); out may be xyz.
 * SE3ICP_ERR_INVALID_ARG for a pose that is not valid (above), a NULL array with n > 0, n < 0. */
int se3icp_transform_points(const double* T, const double* xyz, int64_t n, double* out);
/* One pose per cloud applied to clouds resident in HBM, every cloud in one launch (T: host,
 * n_clouds * 16; d_xyz / off as se3icp_register_graph_device; d_out laid out as d_xyz): what puts
 * registered scans into one frame.  d_out == d_xyz is allowed; any other overlap of the two
 * ranges is SE3ICP_ERR_INVALID_ARG, as are an invalid pose, a NULL array, n_clouds <= 0 or over
 * 65,535 and a decreasing off -- all before the device is looked up.  Kernels run on hip_stream
 * (NULL = the engine's own stream); the call waits once, at its end. */
int se3icp_transform_device(int device, int32_t n_clouds, const double* d_xyz, const int64_t* off, const double* T,
                            double* d_out, void* hip_stream);

/* Single pair convenience (host buffers). */
int se3icp_register(int device, const double* src_xyz, int64_t n_src, const double* tgt_xyz, int64_t n_tgt,
                    int method, const se3icp_params* params, se3icp_result* result);

/* ------------------------------------------------------------- stage surface
 * One entry point per reference member/free function on the hot path, operating
 * on host buffers.  They let a caller (and the parity tests) check each stage in
 * isolation.  All run on device `device`. */

/* computeAllTOLDISE3FramesOMP (ISR.cpp:318-331 -> 241-316): frames [n*16] row-major 4x4. */
int se3icp_toldi_frames(int device, const double* xyz, int64_t n, int k, double* frames);
/* KDTreeFlann::SearchKNN of every point against its own cloud: idx [n*k], sorted by (d2, idx). */
int se3icp_knn_self(int device, const double* xyz, int64_t n, int k, int32_t* idx);
/* PointCloud::EstimateNormals(KNN k) (ISR.cpp:643, :43): normals [n*3]. */
int se3icp_estimate_normals(int device, const double* xyz, int64_t n, int k, double* normals);
/* update_correspondences_raw_flann_SE3 (ISR.cpp:444-470) / update_correspondences_kd_tree_XYZ
 * (ISR.cpp:402-416): exact 1-NN of nq queries among nd points in `dim` (12 or 3)
 * dimensions (AoS rows), tie -> lowest index.  idx [nq]; d2 [nq] (may be NULL). */
int se3icp_nn(int device, const double* query, int64_t nq, const double* data, int64_t nd, int dim,
              int32_t* idx, double* d2, int32_t* num_rechecked);

/* The loop's correspondence stage over a GIVEN pose sequence (diagnostic): the
 * setup of se3icp_nn (host-filled vectors, kd-trees, a neutral setup table with `alpha`), then
 * step k = 1 .. n_steps is iteration k of a one-pair run whose pose is poses[k - 1] (row-major
 * 4x4, bottom row bitwise (0, 0, 0, 1)): the loop's own k_nn_prep settles what the NN
 * certificates allow, its search (with the inline f64 recheck) resolves the rest, and matches and
 * certificates carry over to the next step.  From step restart_at on (0: never) the phase counts
 * as started at restart_at, which voids every earlier certificate.
 * dim 3: a query is the point poses[k] * query[i].  dim 12: a query row is [alpha x, alpha y,
 * alpha z, t] in the packing of the frames ([R00 R10 R20 R01 R11 R21 R02 R12 R22 t0 t1 t2]) with
 * (x y z) orthonormal, moved as a frame; data rows are plain 12-vectors.  The certificates assume
 * the orthonormality and `alpha`; the entry does not check either.
 * Outputs, all in query order and any of them NULL: per step and query [n_steps * nq] the match
 * `idx`, the stored distance `dist` and the certificate words after the step (cert_iter -1: none;
 * cert_d1 / cert_l2: the bounds D1 / L2; cert_j: the certified match); per step [n_steps] the
 * queries k_nn_prep did not settle (`searched`), how many of those went to the
 * one-query-per-wave list (`single`) and the queries re-resolved in f64 (`rechecked`).
 * SE3ICP_ERR_INVALID_ARG for a NULL query / data / poses, dim not 3 or 12, n_steps <= 0, a
 * non-finite alpha or pose entry, a wrong bottom row, restart_at outside [0, n_steps];
 * SE3ICP_ERR_EMPTY_CLOUD for nq or nd <= 0 -- all before the device is looked up. */
int se3icp_nn_sequence_version(void);  /* 1 */
int se3icp_nn_sequence(int device, const double* query, int64_t nq, const double* data, int64_t nd, int dim,
                       double alpha, int32_t n_steps, const double* poses, int32_t restart_at, int32_t* idx,
                       float* dist, float* cert_d1, float* cert_l2, int32_t* cert_iter, int32_t* cert_j,
                       int32_t* searched, int32_t* single, int32_t* rechecked);

/* ------------------------------------------------------------- data generators
 * The synthetic registration problems of examples/benchmark_synthetic.cpp:91-160
 * (add_noise_to_point_cloud B_SYN:13-56, RandomDownSample, T_c applied to the target),
 * generated on device `device` for n_cases cases at once: source_c = a random subset of
 * k = (int)(ratio * n) points of `base` plus N(0, noise_var I) noise, target_c = an
 * independent random subset of T_c * base plus noise.  base: host [n*3]; T: host
 * [n_cases*16] row-major.  src_out / tgt_out: [n_cases*k*3] AoS, device pointers when
 * outputs_on_device (ready for se3icp_register_batch_device with offsets c*k), host
 * pointers otherwise.  Returns k (>= 0) or a negative se3icp_status.  Counter-based
 * random streams (Philox4x32-10 keyed by `seed`, no host draws: any batch size in one pass):
 * same distributions as the reference's mt19937 draws, not the same samples (for those:
 * se3icp_synthetic_reference_device below). */
int64_t se3icp_synthetic_pairs(int device, const double* base, int64_t n, int32_t n_cases, const double* T,
                               double ratio, double noise_var, uint64_t seed, double* src_out, double* tgt_out,
                               int outputs_on_device);

/* The reference's own synthetic problems, number for number (host; no device needed):
 * examples/benchmark_synthetic.cpp:91-160 with its random streams -- Open3D's engine
 * (Seed(1), std::mt19937) for RandomDownSample, std::mt19937 gen(1) with
 * uniform_real_distribution for T (t in [-t_range, t_range]^3, rot_3d angles in
 * [-r_range, r_range]; "moderate" setup: 10, pi/2), one static std::mt19937{1} +
 * normal_distribution for the N(0, noise_var I) noise.  cloud: the full cloud in its file
 * order (stanford_bunny.ply x 50), n points.  src_out / tgt_out: [n_cases * k * 3]
 * (k = (int)(ratio * n), every case's noisy source copy and target), T_out [n_cases * 16]
 * row-major; any output may be NULL.  Returns k or a negative se3icp_status.
 * flags: SE3ICP_GEN_ARGS_LTR evaluates rot_3d's three angle draws left to right (a
 * clang-built reference) instead of GCC's right to left. */
#define SE3ICP_GEN_ARGS_LTR 1
int64_t se3icp_synthetic_reference(const double* cloud, int64_t n, int32_t n_cases, double ratio, double noise_var,
                                   double t_range, double r_range, int32_t flags, double* src_out, double* tgt_out,
                                   double* T_out);
/* The same problems, number for number, written by the GPU for a whole batch: the host
 * draws the reference's streams (as se3icp_synthetic_reference) and the device gathers,
 * transforms (Transform's arithmetic, no FMA) and adds the noise, so src_out / tgt_out equal
 * se3icp_synthetic_reference's bit for bit.  src_out / tgt_out: device pointers when
 * outputs_on_device (ready for se3icp_register_batch_device with offsets c*k), host
 * pointers otherwise; T_out: host [n_cases * 16] (may be NULL).  Returns k or a negative
 * se3icp_status. */
int64_t se3icp_synthetic_reference_device(int device, const double* cloud, int64_t n, int32_t n_cases, double ratio,
                                          double noise_var, double t_range, double r_range, int32_t flags,
                                          double* src_out, double* tgt_out, double* T_out, int outputs_on_device);
/* PointCloud::RandomDownSample(ratio) right after utility::random::Seed(seed) (Open3D 0.19):
 * the kept points in file order into out [k * 3] (may be NULL); returns k. */
int64_t se3icp_random_downsample(const double* xyz, int64_t n, double ratio, uint32_t seed, double* out);

/* ------------------------------------------------------------- voxel-grid downsample
 * What turns a raw scan into the cloud the reference's drivers register (their inputs are
 * already downsampled; VoxelDownSample(0.0042) is the bunny drivers' commented alternative,
 * examples/registration_example.cpp:17-18): Open3D PointCloud::VoxelDownSample for xyz, on the
 * GPU, batched, from HBM into HBM.  All f64:
 *   min_bound = min(p) - 0.5 * voxel_size                       per cloud and axis
 *   cell(p)   = floor((p - min_bound) / voxel_size)             one subtraction, one division
 *   output    = sum / (double)count, sum the sequential f64 sum of the cell's points in
 *               input-index order (Open3D's AccumulatedPoint::AddPoint order, from +0.0)
 * so a restatement that does the same IEEE operations gives the same bits.  Output order: Open3D's
 * is its unordered_map's, i.e. unspecified; here it is FIRST OCCURRENCE -- voxels ascending by
 * the lowest input index they contain -- whatever the batch around the cloud, the engine slot or
 * the layout of the hash table that groups the points.
 * Errors, the arguments checked before the device is looked up: SE3ICP_ERR_INVALID_ARG for
 * n_clouds <= 0, a NULL array, a voxel_size <= 0 or not finite; SE3ICP_ERR_EMPTY_CLOUD for a
 * cloud of 0 points; without a device SE3ICP_ERR_NO_DEVICE, never a CPU fallback.  Found on the
 * device and returned at the call's end (no output is then to be used): SE3ICP_ERR_NONFINITE for
 * a NaN or infinite coordinate; SE3ICP_ERR_INVALID_ARG for Open3D's "voxel_size is too small"
 * (voxel_size * INT_MAX < the largest extent of [min_bound, max(p) + 0.5 * voxel_size]) and,
 * A DEPARTURE FROM OPEN3D, for a grid whose three per-axis cell indices do not pack into one
 * 63-bit key (bit lengths of the largest index per axis summing to more than 63: Open3D hashes
 * an int triple and has no such bound); SE3ICP_ERR_INTERNAL if the grouping table ran full
 * (it holds twice the points; every probe sequence is bounded by it).  More than 65,535 clouds
 * or 2^30 points in one call: SE3ICP_ERR_INVALID_ARG. */
int se3icp_voxel_version(void);  /* 1 */
/* d_xyz: the device concatenation of every cloud's AoS xyz, off (n_clouds + 1 host entries)
 * each cloud's point range, voxel_size (n_clouds host entries) each cloud's own.  d_out: device,
 * room for off[n_clouds] - off[0] points; the clouds' outputs are written compacted and
 * contiguous and out_off (n_clouds + 1 host entries, out_off[0] = 0) is filled, so (d_out, out_off)
 * go straight into se3icp_register_batch_device / se3icp_register_graph_device.  d_count
 * (points per output voxel) and d_first (its lowest input index, relative to the cloud): optional
 * device outputs laid out as d_out's points, either may be NULL.  Kernels run on hip_stream
 * (NULL = the engine's own stream); the call waits once, at its end, to read the counts. */
int se3icp_voxel_downsample_device(int device, int32_t n_clouds, const double* d_xyz, const int64_t* off,
                                   const double* voxel_size, double* d_out, int64_t* out_off, int32_t* d_count,
                                   int32_t* d_first, void* hip_stream);
/* One host cloud: out [n * 3], count [n], first [n] host arrays with room for n entries (any may
 * be NULL; all NULL returns the size only).  Returns the number of output points or a negative
 * se3icp_status. */
int64_t se3icp_voxel_downsample(int device, const double* xyz, int64_t n, double voxel_size, double* out,
                                int32_t* count, int32_t* first);

/* ------------------------------------------------------------- diagnostics
 * Not part of the reference boundary: per-kernel GPU times (HIP events) of the
 * last batch on `device`, used by bench.py for the roofline figures.
 * (recheck_ms: ~0 since ABI 3's inline recheck -- the f64 re-resolution runs inside
 * the NN grids and is part of nn_se3_ms / nn_r3_ms.)
 * out[24] = {nn_se3_ms, nn_r3_ms, recheck_ms, trim_ms, reduce_ms, setup_ms,
 *            nn_se3_launches, nn_r3_launches, se3_dist_evals, se3_box_tests,
 *            r3_dist_evals, r3_box_tests,   (evals/tests counted per lane)
 *            lrf_ms, lrf_queries, lrf_leaves, lrf_merges, lrf_box_tests,
 *            lrf_candidates,   (kNN/TOLDI/normals kernel)
 *            nn_prep_ms, se3_queries, se3_searched, r3_queries, r3_searched,
 *            (NN certificates: queries of all iterations / those searched)
 *            lrf_fallback}  (setup queries handed to the exact one-per-wave kNN kernel) */
int se3icp_set_profiling(int device, int on);
int se3icp_last_kernel_times(int device, double* out);
/* The same record extended (ABI 4): out[SE3ICP_KERNEL_TIMES_N], n >= SE3ICP_KERNEL_TIMES_N
 * (else SE3ICP_ERR_INVALID_ARG): the 24 values above, then se3_useful_evals, r3_useful_evals --
 * the occupied (query, target) distance evaluations of the NN searches (the *_dist_evals
 * count 64-lane evaluation slots, idle lanes of partly filled sweeps included). */
#define SE3ICP_KERNEL_TIMES_N 26
int se3icp_last_kernel_times_n(int device, double* out, int n);

/* Per-iteration correspondence record of ONE pair of the next batch registered on
 * `device` (diagnostic; the parity tests compare it with the reference's loop
 * iteration by iteration).  Each row it (0-based) holds what iteration it+1 built:
 *   corr_idx / corr_dist  the pre-trim correspondence of every source point: target
 *                         index and the float distance of the pcl::Correspondence
 *                         (ISR.cpp:444-470 SE(3) phase, 402-416 R3 phase);
 *   trim_key              the trimmed rejector's cut (ISR.cpp:669-671): source point i
 *                         is kept iff (float bits of corr_dist[i]) << 32 | i <= trim_key;
 *                         UINT64_MAX when nothing is trimmed (overlap 1);
 *   T, mse                current_estimated_T_ after the iteration (normalized frame,
 *                         row-major) and the MSE it computed (ISR.cpp:684-711);
 *   phase                 1 = SE(3) correspondences, 2 = R3.
 * Any array may be NULL.  The record is armed by se3icp_set_trace (pointers are kept
 * until that batch returns, then the trace disarms itself; NULL disarms) and makes the
 * batch wait for every iteration (slower; never used by bench.py). */
typedef struct se3icp_trace {
    int32_t pair;            /* pair index within the next batch */
    int32_t max_iters;       /* rows of the arrays below */
    int32_t* corr_idx;       /* [max_iters * n_src] */
    float* corr_dist;        /* [max_iters * n_src] */
    uint64_t* trim_key;      /* [max_iters] */
    double* T;               /* [max_iters * 16] */
    double* mse;             /* [max_iters] */
    int32_t* phase;          /* [max_iters] */
    int32_t iters_recorded;  /* out: rows written */
    int32_t _reserved;
} se3icp_trace;
int se3icp_set_trace(int device, se3icp_trace* trace);

/* The setup's per-point arrays of ONE pair of the next registration call on `device`
 * (diagnostic, of the kind of se3icp_trace; the tests hold them to long-double references and
 * compare them bitwise between the entries and the sharing modes).  What is recorded is what
 * the loop is about to consume: the arrays of cloud slots 2 * pair (source) and 2 * pair + 1
 * (target) as they stand when the setup is complete and before the first iteration is queued,
 * whichever entry, sharing mode or kernel produced them.
 *   xyz      [n * 3] AoS, in the loop's frame: normalized ((p + (-norm_center)) * norm_scale)
 *            for the run_se3_* methods, the input for run_icp;
 *   rows     [n * 12] the weighted SE(3) element of every point,
 *            (alpha R00 R10 R20 R01 R11 R21 R02 R12 R22, beta t0 t1 t2): the columns of the
 *            TOLDI frame, then its translation.  Only for methods with frames (run_se3_*);
 *   normals  [n * 3] AoS; only where the method estimates normals for that side;
 *   conf     [n] lounge confidences; only for se3_gicp_with_cf.
 * `written` says which arrays were filled (SE3ICP_SETUP_* bits): an array the method does not
 * produce, or that is NULL, is left alone.  The scalars are the cloud's device-side setup
 * record.  Any array may be NULL; `cap` is the number of points the side's arrays have room
 * for: a cloud with more fails the call with SE3ICP_ERR_INVALID_ARG before its loop.
 * Armed by se3icp_set_setup_record as a trace is: one-shot, for the next registration call on
 * that engine (device | slot << 8); the pointers are kept until that call returns; NULL
 * disarms; a pair outside the call's results is SE3ICP_ERR_INVALID_ARG from that call.  After a
 * sweep `pair` indexes the result array (v * n_pairs + p) and the record shows variant v's
 * rows; after a graph call it is the edge index (a posed edge's source is the posed cloud).
 * Armed, the call waits once more for the device; unarmed, a call queues exactly what it
 * queues without this entry.  Never used by bench.py. */
#define SE3ICP_SETUP_XYZ 1
#define SE3ICP_SETUP_ROWS 2
#define SE3ICP_SETUP_NORMALS 4
#define SE3ICP_SETUP_CONF 8
typedef struct se3icp_setup_side {
    double* xyz;            /* [cap * 3] */
    double* rows;           /* [cap * 12] */
    double* normals;        /* [cap * 3] */
    double* conf;           /* [cap] */
    int64_t cap;            /* points the arrays have room for */
    int64_t n;              /* out: points of the cloud */
    double norm_center[3];  /* out: the cloud's setup scalars */
    double norm_scale;
    double f32_center[3];
    double alpha;
    double beta;
    int32_t written;        /* out: SE3ICP_SETUP_* bits of the arrays filled */
    int32_t _reserved;
} se3icp_setup_side;
typedef struct se3icp_setup_record {
    int32_t pair;           /* result index within the next call */
    int32_t recorded;       /* out: 1 once the record was taken */
    se3icp_setup_side src, tgt;
} se3icp_setup_record;
int se3icp_setup_record_version(void);  /* 1 */
int se3icp_set_setup_record(int device, se3icp_setup_record* rec);

/* The kd-trees of ONE pair as the next call that builds trees on `device` leaves them for its
 * searches (diagnostic, of the kind of se3icp_setup_record; the tests check the order, the
 * tree-ordered vectors and every node box exactly).  Recorded are the 3-D and the 12-D tree of
 * cloud slots 2 * pair (src) and 2 * pair + 1 (tgt), read back from the buffers the searches
 * read, whichever kernels, adoption or sweep expansion filled them; a registration call takes
 * the record where it takes the setup record (behind the 12-D build, before the first
 * iteration), se3icp_nn / se3icp_nn_sequence behind their build (pair 0: src the queries, tgt
 * the data; only the tree of `dim` exists).  One documented layout whatever the device's:
 *   perm    [n] tree position -> point;  pos [n] point -> tree position;
 *   vec     [n * D] the f32 input vectors in point order (3-D: the points minus f32_center);
 *   tvec    [n * D] the f32 vectors in tree order;
 *   tvec64  [n * 3] the f64 vectors in tree order: the points (3-D), the translation entries
 *           9..11 of the rows (12-D);
 *   tpt64   [n * 4] 3-D only: the (x, y, z, 0) records of the f64 points in tree order;
 *   lo, hi  [nnodes * D] the node boxes in heap order (node i of level l: 2^l - 1 + i).
 * `written` (SE3ICP_TREE_* bits) says which arrays the build produces for that tree and that
 * were asked for; an array the build does not produce is left alone: a loop source's 12-D tree
 * below depth 0 is its order and its f64 translation entries only, a 12-D target's has no f64
 * vectors.  `exists` is 0 for a tree the call did not build (the 12-D trees of run_icp, the
 * other dimension of se3icp_nn); its other outputs are then 0.  role: SE3ICP_TREE_BUILT, or the
 * cloud slot whose finished order the slot adopted in the last build that touched it (a sweep's
 * replicas show their base cloud's).  G: the levels the build splits with one grid over all
 * clouds; H: how many of those, the first ones, took the multi-pass sequence (the others one
 * workgroup per node); the levels below G are split by one workgroup per level-G node.
 * Any array may be NULL; `cap` (points) and `node_cap` (nodes) say what the arrays have room
 * for: a tree with more, for an array that is asked for, fails the call with
 * SE3ICP_ERR_INVALID_ARG before its loop.  One-shot, for the next such call on that engine
 * (device | slot << 8); the pointers are kept until that call returns; NULL disarms; a pair
 * outside the call's results is SE3ICP_ERR_INVALID_ARG from that call.  The arguments are
 * checked before the device is looked up.  May be armed together with a setup record.  Armed,
 * the call waits for the device before its loop; unarmed, a call queues exactly what it queues
 * without this entry.  Never used by bench.py. */
#define SE3ICP_TREE_PERM 1
#define SE3ICP_TREE_POS 2
#define SE3ICP_TREE_VEC 4
#define SE3ICP_TREE_TVEC 8
#define SE3ICP_TREE_TVEC64 16
#define SE3ICP_TREE_TPT64 32
#define SE3ICP_TREE_BOXES 64
#define SE3ICP_TREE_BUILT (-1)
typedef struct se3icp_tree_side {
    int32_t* perm;          /* [cap] */
    int32_t* pos;           /* [cap] */
    float* vec;             /* [cap * D] */
    float* tvec;            /* [cap * D] */
    double* tvec64;         /* [cap * 3] */
    double* tpt64;          /* [cap * 4] (3-D) */
    float* lo;              /* [node_cap * D] */
    float* hi;              /* [node_cap * D] */
    int64_t cap;            /* points the arrays have room for */
    int64_t node_cap;       /* nodes lo / hi have room for */
    int64_t n;              /* out: points of the cloud */
    int32_t exists;         /* out: 1 if the call built this tree */
    int32_t D;              /* out: 3 or 12 */
    int32_t L;              /* out: depth (leaves at level L) */
    int32_t nnodes;         /* out: 2^(L+1) - 1 nodes */
    int32_t G;              /* out: global levels of the build */
    int32_t H;              /* out: multi-pass levels among them */
    int32_t role;           /* out: SE3ICP_TREE_BUILT or the donor's cloud slot */
    int32_t written;        /* out: SE3ICP_TREE_* bits of the arrays filled */
} se3icp_tree_side;
typedef struct se3icp_tree_record {
    int32_t pair;           /* result index within the next call */
    int32_t recorded;       /* out: 1 once the record was taken */
    se3icp_tree_side src3, tgt3, src12, tgt12;
} se3icp_tree_record;
int se3icp_tree_record_version(void);  /* 1 */
int se3icp_set_tree_record(int device, se3icp_tree_record* rec);

/* Diagnostic: which kernels compute the setup's kNN / TOLDI / normals on `device`:
 *   0 = the default: eight queries per wavefront (k_lrf8), the exact one-query-per-wavefront
 *       kernel for the queries it hands over, the global-buffer kernel for k > 128;
 *   1 = the exact one-query-per-wavefront kernel for every point (k <= 128);
 *   2 = the global-buffer kernel (any k) for every point.
 * All give bitwise-identical results; the tests check that. */
int se3icp_set_lrf_exact(int device, int exact_only);

/* Diagnostic: HIP events around the SE(3) NN grids of timed (non-profiled) batches, on by
 * default; they fill time_se3_correspondence_search_ms.  Each marker leaves the GPU idle a
 * few microseconds, so bench.py turns them off for its timed steps (the field is then 0). */
int se3icp_set_nn_events(int device, int on);

#ifdef __cplusplus
}
#endif
#endif /* SE3ICP_H */
