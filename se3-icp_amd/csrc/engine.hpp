// engine.hpp — host driver of the MI355X SE(3)-ICP engine.
//
// One Engine per HIP device.  register_batch() runs every pair of a batch in
// lockstep: each iteration launches one grid per stage covering all active pairs
// (pairs in the SE(3) phase and pairs already switched to the R3 phase share the
// iteration); the f64 solve and the reference's switch / convergence logic
// (ISR.cpp:654-732) run on the device at the end of the iteration (pairmath.hpp), and
// the host queues the next iteration before the previous one has finished.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <stdint.h>
#include <vector>

#include "graph.hpp"
#include "pairmath.hpp"
#include "pose.hpp"
#include "se3icp.h"
#include "view.hpp"
#include "voxel.hpp"

namespace se3icp {

// k_voxel.hip: queue the voxel-grid downsample of a call's clouds (voxel.hpp)
void launch_voxel(const VoxelArgs& a, int max_chunks, int64_t n_points, int64_t n_slots, hipStream_t s);

// A device buffer (Engine::ensure) and a pinned host mirror.  Each names the engine's list it
// belongs to when it is declared: the destructor and the sweep's memory count walk those
// lists, so a new member cannot be left out of them.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    explicit DevBuf(std::vector<DevBuf*>& owner) { owner.push_back(this); }
};
struct PinnedMem {
    void* mem = nullptr;
    size_t cap = 0;  // elements
};
template <class T>
struct Pinned : PinnedMem {
    explicit Pinned(std::vector<PinnedMem*>& owner) { owner.push_back(this); }
    operator T*() const { return static_cast<T*>(mem); }
    // room for `count` elements (at least 16); growing frees first, the contents are not kept
    int reserve(size_t count) {
        if (cap >= count && mem) return 0;
        if (mem) (void)hipHostFree(mem);
        mem = nullptr;
        cap = 0;
        const size_t want = count > 16 ? count : 16;
        if (hipHostMalloc(&mem, want * sizeof(T), hipHostMallocDefault) != hipSuccess) return SE3ICP_ERR_OUT_OF_MEMORY;
        cap = want;
        return 0;
    }
};

// Per-kernel GPU time of the last register_batch (HIP events, ms), for bench.py.
struct KernelTimes {
    double nn_se3_ms = 0, nn_r3_ms = 0, recheck_ms = 0, trim_ms = 0, reduce_ms = 0;
    double setup_ms = 0;
    int64_t nn_se3_launches = 0, nn_r3_launches = 0;
    // work actually done by the NN kernels (device counters): lane-distance evaluations
    // in leaf sweeps and lane-box tests in the traversal
    double se3_dist_evals = 0, se3_box_tests = 0, r3_dist_evals = 0, r3_box_tests = 0;
    double se3_useful_evals = 0, r3_useful_evals = 0;  // occupied (query, target) evaluations
    // fused kNN/TOLDI/normals kernel of the setup: time, queries, leaves scanned, sorts
    double lrf_ms = 0, lrf_queries = 0, lrf_leaves = 0, lrf_merges = 0, lrf_box_tests = 0, lrf_candidates = 0;
    double lrf_fallback = 0;  // queries k_lrf8 handed to the exact kernel
    // NN certificates (k_nn_prep): its time, and per phase the queries of all iterations
    // and those that had to be searched
    double nn_prep_ms = 0, se3_queries = 0, se3_searched = 0, r3_queries = 0, r3_searched = 0;
};

// What a method asks of the setup and the loop (plan_method, engine.cpp).
struct MethodPlan {
    Kind kind;
    int est;
    bool se3;                            // an SE(3) method: frames, 12-D trees, normalized pairs
    int k_lrf, k_nrm_s, k_nrm_t, kmax;   // TOLDI k, normals k of sources / targets, the largest
};

class Engine {
  public:
    explicit Engine(int device);
    ~Engine();
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;

    int device() const { return dev_; }
    std::mutex& mutex() { return mu_; }
    void set_profiling(bool on) { profile_ = on; }
    void set_trace(se3icp_trace* t) { trace_ = t; }
    void set_setup_record(se3icp_setup_record* r) { setup_rec_ = r; }
    void set_tree_record(se3icp_tree_record* r) { tree_rec_ = r; }
    void set_lrf_exact(int mode) { lrf_exact_only_ = mode; }
    void set_nn_events(bool on) { nn_events_ = on; }
    void set_batch_sharing(int level) { batch_sharing_ = level; }
    void set_lrf_seeding(int mode) { lrf_seeding_ = mode; }
    void set_tree_sharing(int mode) { tree_sharing_ = mode; }
    void set_lrf_taking(int mode) { lrf_taking_ = mode; }
    const KernelTimes& kernel_times() const { return ktimes_; }

    int register_batch(int npairs, const double* const* src, const int64_t* ns, const double* const* tgt,
                       const int64_t* nt, bool on_device, int method, const se3icp_params& prm,
                       se3icp_result* out, hipStream_t user_stream, const se3icp_report_options* ropts = nullptr,
                       se3icp_report* reports = nullptr);
    // Every pair under every parameter set of `variants`, results[v * npairs + p], with one
    // shared setup (sweep.hpp); the caller has validated the arguments (capi.cpp).
    int register_sweep(int npairs, const double* const* src, const int64_t* ns, const double* const* tgt,
                       const int64_t* nt, bool on_device, int method, int nvariants, const se3icp_params* variants,
                       int max_group, se3icp_result* out, hipStream_t user_stream,
                       const se3icp_report_options* ropts = nullptr, se3icp_report* reports = nullptr);

    // Edge p registers clouds[src[p]] onto clouds[tgt[p]]; every distinct cloud is uploaded and
    // ingested once and every (cloud, normalization) class selects its neighbours once
    // (graph.hpp); results[p] is bitwise register_batch's for that pair.  The caller has
    // validated the arguments.
    // T_init (validated by the caller; may be null): one row-major 4x4 initial pose per edge, source
    // frame -> target frame.  results[p] is then bitwise the plain call's for (apply_pose(T0, source),
    // target) except T, which is compose(T_plain, T0).  The call is planned over variants
    // (graph.hpp): a posed variant is ingested from its raw cloud through the pose and is a cloud
    // of its own to everything behind the ingest.
    int register_graph(int nclouds, const double* const* xyz, const int64_t* npts, int npairs, const int32_t* src,
                       const int32_t* tgt, bool on_device, int method, const se3icp_params& prm, int sharing,
                       se3icp_result* out, hipStream_t user_stream, const se3icp_report_options* ropts = nullptr,
                       se3icp_report* reports = nullptr, const double* T_init = nullptr);
    // [IS_COUNT] of the last register_graph (se3icp_last_init_stats)
    const int64_t* init_stats() const { return init_stats_; }
    void set_pose_seeding(int mode) { pose_seeding_ = mode; }
    // One pose per cloud applied to clouds resident in HBM, all in one launch (k_pose.hip); T on
    // the host; d_out may be d_xyz.  The caller has validated the arguments.  One wait, at the end.
    int transform_device(int nclouds, const double* d_xyz, const int64_t* off, const double* T, double* d_out,
                         hipStream_t user_stream);
    // [GS_COUNT] of the last register_graph, or of the last device batch that looked for shared
    // clouds (setup_pairs_shared)
    const int64_t* graph_stats() const { return graph_stats_; }
    // [4] of the last registration call (se3icp_last_seed_stats): classes seeded, queries of
    // waves that started from a seed, that ran without one, that were handed over after a
    // failed certificate
    const int64_t* seed_stats() const { return seed_stats_; }
    // [TS_COUNT] of the last registration call (se3icp_last_take_stats): classes taking, queries
    // that took their source's list, queries of redone waves, queries that failed the order check
    // or the certificate
    const int64_t* take_stats() const { return take_stats_; }
    // [4] of the last registration call (se3icp_last_tree_stats): 3-D trees built / adopted,
    // 12-D trees built / adopted
    const int64_t* tree_stats() const { return tree_stats_; }

    // stage entry points (host buffers)
    int knn_self(const double* xyz, int64_t n, int k, int32_t* idx);
    int toldi_frames(const double* xyz, int64_t n, int k, double* frames);
    int estimate_normals(const double* xyz, int64_t n, int k, double* normals);
    int nn(const double* query, int64_t nq, const double* data, int64_t nd, int dim, int32_t* idx, double* d2,
           int32_t* num_rechecked);
    // the loop's k_nn_prep and search over a given pose sequence (se3icp_nn_sequence); the caller
    // has validated the arguments.  Any output may be null.
    struct NNSequenceOut {
        int32_t* idx;
        float* dist;
        float *cert_d1, *cert_l2;
        int32_t *cert_iter, *cert_j;
        int32_t *searched, *single, *rechecked;
    };
    int nn_sequence(const double* query, int64_t nq, const double* data, int64_t nd, int dim, double alpha,
                    int n_steps, const double* poses, int restart_at, const NNSequenceOut& out);

    // Voxel-grid downsample of nclouds clouds resident in HBM (cloud c: points off[c] .. off[c+1]
    // of d_xyz, voxel size vs[c]) into d_out, compacted and contiguous; out_off [nclouds + 1] on
    // the host.  d_count / d_first: optional device outputs per output voxel.  One wait, at the
    // end.  The caller has validated the sizes (voxel_check_sizes).
    int voxel_downsample(int nclouds, const double* d_xyz, const int64_t* off, const double* vs, double* d_out,
                         int64_t* out_off, int32_t* d_count, int32_t* d_first, hipStream_t user_stream);
    // The same for one host cloud: out / count / first are host arrays (any may be null); *n_out.
    int voxel_downsample_host(const double* xyz, int64_t n, double vs, double* out, int32_t* count, int32_t* first,
                              int64_t* n_out);

  private:
    struct CloudReq {
        const double* in = nullptr;  // AoS input
        int64_t n = 0;
        CloudSetup st{};
    };
    struct TreeBufs {
        DevBuf perm, pos, vec, vec64, vec64a, blo, bhi, lo, hi, scr, vecT;  // (vecT: 12-D input columns)
        int L = 0;  // depth of the trees in these buffers
        explicit TreeBufs(std::vector<DevBuf*>& o)
            : perm(o), pos(o), vec(o), vec64(o), vec64a(o), blo(o), bhi(o), lo(o), hi(o), scr(o), vecT(o) {}
    };
    int init();
    // the front of knn_self (neither), toldi_frames and estimate_normals: checks, one cloud's setup
    int setup_single(const double* xyz, const void* out, int64_t n, int k, bool frames, bool normals);
    template <class T>
    T* ensure(DevBuf& b, size_t count);
    int alloc_points(int64_t ntot, int kmax, bool knn_list = false);
    int nn_setup(const double* query, int64_t nq, const double* data, int64_t nd, int dim, double alpha);
    // build the D-dimensional kd-trees of every cloud over `vec` ([D][ld] f32).  role (null:
    // every cloud builds) says per cloud kTreeBuilds, kTreeAbsent or the cloud whose finished
    // order it adopts (tree.hpp); tab is the table's home on the host and the device until the
    // call's last synchronisation.
    struct TreeTab {
        Pinned<int32_t> host;  // role [nclouds], then the builders' and the adopters' ids (pinned: an async copy)
        DevBuf dev;
        TreeTab(std::vector<PinnedMem*>& p, std::vector<DevBuf*>& o) : host(p), dev(o) {}
    };
    int build_tree(int D, const float* vec, hipStream_t s, const double* vec64 = nullptr,
                   const std::vector<int32_t>* role = nullptr, TreeTab* tab = nullptr);
    // A registration call (register_batch, each group of register_sweep, register_graph) is
    // open_call, the entry's own setup of its clouds, and run_pairs.
    //
    // open_call: the engine check, the armed trace (taken, and so disarmed, even when the call
    // is then rejected) validated against the call's `nslots` result slots, the device, the
    // stream, the kernel times' reset and the begin event.  The entry's own argument checks
    // surround the trace's: `args` is the status of those before it, `rest` (evaluated by the
    // entry only when `args` is 0) of those after it.
    // The armed setup record (se3icp_set_setup_record) and tree record (se3icp_set_tree_record)
    // ride beside the trace: taken and validated with it, in that order; sr_pair / tk_pair the
    // recorded pair's index among the pairs run_pairs is given (the trace carries its own).
    struct Call {
        hipStream_t s = nullptr;
        se3icp_trace* tr = nullptr;
        se3icp_setup_record* sr = nullptr;
        se3icp_tree_record* tk = nullptr;
        int sr_pair = -1, tk_pair = -1;
    };
    int open_call(int args, int64_t nslots, int rest, hipStream_t user_stream, Call* c);
    // The Call of a sweep group of g variants from v0 over P pairs: the records of `c` whose pair
    // (result index v * P + p) lies in the group, remapped to the group's pairs.  The trace is
    // remapped in a copy, *gtr; the caller writes its iters_recorded back.
    static Call group_call(const Call& c, int v0, int g, int P, se3icp_trace* gtr);
    // The clouds back to back in the SoA columns: offsets, chunk list, inputs (uploaded, or
    // pointed at when on_device) and the cloud, setup, chunk and input tables on the device.
    int upload_clouds(const std::vector<CloudReq>& clouds, bool on_device, hipStream_t s);
    // every cloud's centroid from k_ingest's chunk sums on the host: chunks in order, then / n
    int host_centroids(hipStream_t s, std::vector<double>* cen);
    // upload_clouds -> ingest -> normalize -> 3-D kd-trees -> kNN -> frames for a list of
    // clouds.  pairs: clouds (2p, 2p+1) are source and target of pair p (otherwise every cloud
    // stands alone); normalize (pairs only): they are normalized together with the
    // reference's preprocessing, the centers and scale[p] staying on the device.
    int setup_clouds(const std::vector<CloudReq>& clouds, bool on_device, bool pairs, bool normalize, double scale_pre,
                     hipStream_t s);
    // The front of setup_clouds and setup_pairs_shared behind upload_clouds: k_ingest, then the
    // normalization parameters -- normalize: centers, radius and scales on the device, no host
    // wait; otherwise the centroids on the host (one wait) and the setup table's copy.  The
    // caller queues launch_normalize behind it.
    int queue_norm_params(bool pairs, bool normalize, double scale_pre, hipStream_t s);
    // kNN / frames / normals of the clouds set up so far (step 4 of setup_clouds).  sel: the
    // plan of a selection that seeds or takes (select_by_class); null: a plain selection.
    int setup_knn(hipStream_t s, const SelectPlan* sel = nullptr);
    // setup_clouds for the 2P resident cloud slots of a device batch that may hold one cloud
    // several times (graph.hpp): the slots are ingested, normalized and given their 3-D trees
    // in place exactly as setup_clouds does, hashed on the way, and compared where the hashes
    // agree; with a confirmed duplicate the neighbour selection runs once per class
    // (select_by_class), otherwise as setup_knn; with tree sharing the later slots of a confirmed
    // cloud adopt its first slot's 3-D tree order (and, in run_pairs, its 12-D one).  Two host waits where setup_clouds has none
    // (run_se3_*) or one (vanilla): the hashes, with the normalization parameters the class
    // plan needs; the compare flags, only when some hash agreed.
    int setup_pairs_shared(const std::vector<CloudReq>& clouds, const MethodPlan& mp, double scale_pre, hipStream_t s);
    // The neighbour selection of planned uses that are laid out, normalized and have their 3-D
    // trees: the first use of every class selects for it (setup_knn over a table in which the
    // other uses ask for nothing), k_graph_share hands its rows and normals to the others, and
    // `batch`, the uses' own setup table, is the device's and the host's from there on.
    int select_by_class(const GraphPlan& plan, const std::vector<CloudSetup>& batch, const MethodPlan& mp,
                        hipStream_t s);
    int setup_chunks(int npairs, hipStream_t s);
    // run_pairs: everything behind the clouds' setup, for npairs pairs laid out src 0, tgt 0,
    // src 1, ...: the 12-D kd-trees over the weighted SE(3) elements (SE(3) methods),
    // prepare_pairs (the work table of k_reduce and the per-pair buffers), setup_chunks, the
    // loop's cleared buffers, the setup-done event and run_loop (loop state, the loop, the
    // results and, with `ropts` and `reports`, the report of every pair).  Pair q takes its
    // parameters from vprm[q / pairs_per_variant] (a plain batch: one variant of npairs pairs;
    // a sweep group: the group's variants, pair q a replica of base pair
    // q % pairs_per_variant).  sweep: the setup time is the shared setup's (call begin -> shared
    // done) plus the group's (group begin -> setup done) instead of call begin -> setup done.
    int run_pairs(const MethodPlan& mp, int npairs, const int64_t* ns, const int64_t* nt,
                  const se3icp_params* vprm, int pairs_per_variant, bool sweep, const Call& c, se3icp_result* out,
                  const se3icp_report_options* ropts, se3icp_report* reports);
    int prepare_pairs(int npairs, const int64_t* ns, const int64_t* nt, hipStream_t s);
    // rq (may be null): the registration report of every pair, evaluated after the loop
    struct ReportReq {
        const se3icp_report_options* opts;  // (validated by the caller)
        se3icp_report* out;                 // [npairs]
    };
    int run_loop(int npairs, const int64_t* ns, int kind, int est, const se3icp_params* vprm, int pairs_per_variant,
                 bool sweep, se3icp_trace* tr, se3icp_result* out, hipStream_t s, const ReportReq* rq = nullptr);
    // queue the report stage behind the loop (k_report.hip): an R3 search at the final poses,
    // the per-pair sums into h_rep_, the per-point outputs into the caller's buffers
    int queue_report(int npairs, const int64_t* ns, const ReportReq& rq, hipStream_t s);
    int read_lrf_stats();
    int sync_stream(hipStream_t s);
    View view() const;

    int dev_;
    bool ok_ = false;
    bool profile_ = false;
    std::mutex mu_;
    hipStream_t stream_ = nullptr;
    KernelTimes ktimes_;

    // geometry of the current batch
    int nclouds_ = 0, npairs_ = 0;
    int64_t ntot_ = 0;
    int ld_ = 0, kmax_ = 1, nwork_ = 0, tree_L_ = 0;
    int chunk_level_ = 0, nchunks_ = 0;  // loop NN work chunks (View::chunk_level)
    bool knn_list_ = false;
    bool nn_trace_ = false;              // SE3ICP_NN_TRACE=1: per-iteration NN work on stderr
    // se3icp_set_lrf_exact: 0 k_lrf8 + hand-overs (default), 1 the exact one-query-per-wavefront
    // k_lrf for every point, 2 the global-buffer k_knn_big for every point (all bitwise equal)
    int lrf_exact_only_ = 0;
    // se3icp_set_nn_events(0): no HIP event bracket around the SE(3) NN search outside
    // profiled batches (each marker leaves the GPU idle a few us;
    // time_se3_correspondence_search_ms is then 0)
    bool nn_events_ = true;
    // se3icp_set_batch_sharing: 0 the highest level built (= 2), 1 off, 2 one selection per class
    int batch_sharing_ = 0;
    // se3icp_set_lrf_seeding: 0 a cloud's later classes start their selection from its first
    // class's neighbour distances (default), 1 off, 2 / 3 diagnostics: every seed halved / times 4
    int lrf_seeding_ = 0;
    // se3icp_set_tree_sharing: 0 the later slots of a confirmed cloud adopt its first slot's tree
    // order (default), 1 off
    int tree_sharing_ = 0;
    se3icp_trace* trace_ = nullptr;      // armed per-iteration record of one pair (se3icp_set_trace)
    int record_trace(se3icp_trace* tr, int it, int& phase_of_it, hipStream_t s);
    se3icp_setup_record* setup_rec_ = nullptr;  // armed setup record of one pair (se3icp_set_setup_record)
    int record_setup(se3icp_setup_record* rec, int pair, hipStream_t s);
    // The armed tree record of one pair (se3icp_set_tree_record) and, per dimension (0: 3-D,
    // 1: 12-D) and cloud slot, what the call's last build that touched the slot was: host
    // bookkeeping of build_tree, cleared by open_call and nn_setup.
    struct TreeLog {
        int32_t role = -2, L = 0, G = 0, H = 0;  // (-2: kTreeAbsent, no build of this call touched it)
    };
    se3icp_tree_record* tree_rec_ = nullptr;
    std::vector<TreeLog> tree_log_[2];
    int record_trees(se3icp_tree_record* rec, int pair, hipStream_t s);
    double trace_prev_[kStatCols] = {};
    std::vector<CloudDev> h_clouds_;
    std::vector<CloudSetup> h_setup_;
    std::vector<BlockWork> h_work_;
    std::vector<int32_t> h_wb_, h_wn_;
    std::vector<ChunkWork> h_chunks_;
    std::vector<const double*> h_inptr_;

    // device buffers and pinned host mirrors: each is named here and nowhere else (bufs_ and
    // pins_, declared first, collect them as they are constructed)
    std::vector<DevBuf*> bufs_;
    std::vector<PinnedMem*> pins_;
    DevBuf d_clouds_{bufs_}, d_setup_{bufs_}, d_pairs_{bufs_}, d_cloud_of_{bufs_}, d_inptr_{bufs_}, d_in_{bufs_},
        d_xyz64_{bufs_}, d_xyz32_{bufs_}, d_fr64_{bufs_}, d_fr32_{bufs_}, d_nrm64_{bufs_}, d_tgeo_{bufs_},
        d_conf64_{bufs_}, d_knn_{bufs_}, d_corr_idx_{bufs_}, d_corr_dist_{bufs_}, d_flag_count_{bufs_},
        d_gcost_{bufs_}, d_cls_{bufs_}, d_trim_key_{bufs_}, d_red_partial_{bufs_}, d_red_out_{bufs_}, d_work_{bufs_},
        d_wb_{bufs_}, d_wn_{bufs_}, d_chunks_{bufs_}, d_partial_{bufs_}, d_centers_{bufs_}, d_rechecked_{bufs_},
        d_keys0_{bufs_}, d_vals1_{bufs_}, d_sort_tmp_{bufs_}, d_stats_{bufs_}, d_qlist_{bufs_}, d_qcount_{bufs_},
        d_hist_{bufs_}, d_cert_{bufs_}, d_sqlist_{bufs_}, d_state_{bufs_}, d_trim_cand_{bufs_}, d_trim_ctr_{bufs_},
        d_scales_{bufs_}, d_trim_hist_{bufs_},
        d_lrf_fb_{bufs_}, d_lrf_fbn_{bufs_},  // k_lrf8 -> exact k_lrf hand-over list and its count
        d_big_d_{bufs_}, d_big_i_{bufs_},     // k_knn_big candidate buffers (neighbourhoods over kSmallK)
        d_raw_{bufs_}, d_sweep_w_{bufs_},     // register_sweep: unweighted SE(3) rows of the shared setup, a group's weights
        // the report's sums and per-point staging
        d_rep_partial_{bufs_}, d_rep_out_{bufs_}, d_rep_off_{bufs_}, d_rep_idx_{bufs_}, d_rep_dist_{bufs_};
    TreeBufs t3_{bufs_}, t12_{bufs_};
    // nn_setup: the host SoA staging of the NN stage entries and their pair record
    std::vector<double> nn_m64_;
    std::vector<float> nn_m32_;
    std::vector<int32_t> nn_cof_;
    PairDev nn_pair_{};
    // register_graph: the distinct clouds' raw columns and confidences (swapped with xyz64 /
    // conf64 between the call's two layouts), the segment and chunk tables of the k_graph kernels
    DevBuf g_raw_xyz_{bufs_}, g_raw_conf_{bufs_}, g_seg_{bufs_}, g_chunks_{bufs_};
    // setup_pairs_shared: the slots' hashes, the compare table and its flags, their host copies
    // and the device's setup table on the host
    DevBuf d_share_hash_{bufs_}, d_share_pairs_{bufs_}, d_share_same_{bufs_};
    Pinned<uint64_t> h_share_hash_{pins_};
    Pinned<int32_t> h_share_same_{pins_};
    Pinned<CloudSetup> h_share_setup_{pins_};
    std::vector<SharePair> share_pairs_;
    // select_by_class: the call's selection plan (graph.hpp), handed to setup_knn and never read as
    // state; kept because queued copies read its arrays until the call's last synchronisation
    SelectPlan sel_;
    int64_t graph_stats_[9] = {};
    // the seeds, and where each use stores / reads them, on the device
    DevBuf d_seed_{bufs_}, d_seed_ref_{bufs_};
    int64_t seed_stats_[4] = {};
    // se3icp_set_lrf_taking: 0 a seeded class with its source's tree order takes the source's
    // neighbour lists (default), 1 off, 2 a diagnostic: every stored bound halved, every wave redone
    int lrf_taking_ = 0;
    // the lists, the uses' take flags and the redo mask on the device (the bounds Lb follow the seeds)
    DevBuf d_take_lists_{bufs_}, d_take_flag_{bufs_}, d_take_mask_{bufs_};
    int64_t take_stats_[TS_COUNT] = {};
    // graph_plan_trees of the call: per slot -1 or the slot whose tree order it adopts.  Set by
    // setup_pairs_shared and register_graph, read by run_pairs for the 12-D trees, cleared by
    // open_call (a call that shares nothing has no donors).  The tables of the call's builds:
    // the 3-D trees queued before and behind the compare flags, the 12-D trees.
    std::vector<int32_t> tree_donor_;
    TreeTab tree_tab_a_{pins_, bufs_}, tree_tab_b_{pins_, bufs_}, tree_tab_12_{pins_, bufs_};
    int64_t tree_stats_[4] = {};
    // register_graph with initial poses: the pose of every slot of layout A (-1: none) and the
    // poses' table, on the host until the call's last synchronisation and on the device; per
    // variant its raw cloud and whether its pose is rigid (select_by_class: graph_plan_seeds_posed;
    // empty in a call without a posed edge); se3icp_set_pose_seeding (0 across variants, 1 off)
    std::vector<int32_t> pose_of_, pose_raw_, pose_rigid_;
    std::vector<double> pose_tab_;
    DevBuf d_pose_of_{bufs_}, d_pose_tab_{bufs_};
    int pose_seeding_ = 0;
    int64_t init_stats_[3] = {};
    // transform_device: the clouds' ranges and poses (pinned: async copies), their device copies
    Pinned<PoseCloud> h_tf_clouds_{pins_};
    Pinned<double> h_tf_poses_{pins_};
    DevBuf d_tf_clouds_{bufs_}, d_tf_poses_{bufs_};
    // voxel_downsample: the tables of VoxelArgs, the host's cloud table and what the call reads
    // back (out_off, then the clouds' status, the error flag); voxel_downsample_host's staging
    DevBuf v_clouds_{bufs_}, v_grids_{bufs_}, v_minmax_{bufs_}, v_sums_{bufs_}, v_table_{bufs_},
        v_vid_{bufs_}, v_members_{bufs_}, v_recs_{bufs_}, v_big_{bufs_}, v_flags_{bufs_},
        v_out_off_{bufs_}, v_in_{bufs_}, v_out_{bufs_}, v_oc_{bufs_}, v_of_{bufs_};
    Pinned<VoxelCloud> h_vclouds_{pins_};
    Pinned<long long> h_vout_{pins_};
    Pinned<int32_t> h_vflags_{pins_};
    Pinned<PairDev> h_pairs_{pins_};
    Pinned<double> h_red_{pins_}, h_partial_{pins_};
    Pinned<int32_t> h_rechecked_{pins_};
    Pinned<double> h_hist_{pins_};  // one pose-history row (npairs x 12)
    Pinned<double> h_rep_{pins_};   // the report's sums (npairs x kRepVals)
    std::vector<int64_t> h_rep_off_;  // first per-point output entry of each pair
    Pinned<PairState> h_state_{pins_};  // loop state of every pair (read back after the loop)
    // [kLoopRing][npairs] each pair's phase in the next iteration, written by k_reduce_final
    // into coherent host memory (h_phase_ host view, d_phase_ device view)
    int32_t* h_phase_ = nullptr;
    int32_t* d_phase_ = nullptr;
    size_t h_phase_cap_ = 0;
    Pinned<unsigned long long> h_lrf_stats_{pins_};   // k_lrf work counters (read at the next sync)
    Pinned<unsigned long long> h_loop_stats_{pins_};  // loop NN work counters (pinned: an async copy, not a staged one)
    bool lrf_stats_pending_ = false;
    // k_lrf time; a sweep's shared setup done / group begin; setup_pairs_shared's hashes and
    // compare flags on the host; call begin / setup done / loop done (GPU-timeline phase times);
    // sync_stream
    enum Ev : int { EV_LRF_BEGIN, EV_LRF_END, EV_SHARED_DONE, EV_GROUP_BEGIN, EV_SHARE_HASH, EV_SHARE_FLAGS,
                    EV_CALL_BEGIN, EV_SETUP_DONE, EV_LOOP_DONE, EV_SYNC, EV_COUNT };
    hipEvent_t ev_[EV_COUNT];
    // loop iterations in flight: kernel-time events and launched NN phases per ring slot
    static constexpr int kLoopRing = 4, kLoopEv = 7;
    hipEvent_t loop_ev_[kLoopRing * kLoopEv];
    int loop_flags_[kLoopRing] = {};
    bool loop_detail_[kLoopRing] = {};
};

// process-wide engine per device (lazily created)
Engine* engine_for(int device);

}  // namespace se3icp
