// engine.cpp — host driver (see engine.hpp).
#include "engine.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>

#include "graph.hpp"
#include "pose.hpp"
#include "report.hpp"
#include "sweep.hpp"
#include "tree.hpp"

namespace se3icp {

namespace {

#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                     \
            std::fprintf(stderr, "se3icp: HIP error %s at %s:%d (%s)\n", hipGetErrorString(e_), __FILE__, \
                         __LINE__, #x);                                                             \
            return SE3ICP_ERR_HIP;                                                                  \
        }                                                                                           \
    } while (0)
#define SYNC_STREAM(st)                   \
    do {                                  \
        const int rc_ = sync_stream(st);  \
        if (rc_) return rc_;              \
    } while (0)

// Kind (KIND_ICP / SE3 / CF / PURE): pairmath.hpp

struct MethodInfo {
    Kind kind;
    int est;
};

bool decode_method(int method, MethodInfo* mi) {
    switch (method) {
        case SE3ICP_PT2PT: *mi = {KIND_ICP, EST_PT2PT}; return true;
        case SE3ICP_PT2PL: *mi = {KIND_ICP, EST_PT2PL}; return true;
        case SE3ICP_GICP: *mi = {KIND_ICP, EST_GICP}; return true;
        case SE3ICP_SE3_PT2PT: *mi = {KIND_SE3, EST_PT2PT}; return true;
        case SE3ICP_SE3_PT2PL: *mi = {KIND_SE3, EST_PT2PL}; return true;
        case SE3ICP_SE3_GICP: *mi = {KIND_SE3, EST_GICP}; return true;
        case SE3ICP_SE3_GICP_WITH_CF: *mi = {KIND_CF, EST_GICP}; return true;
        case SE3ICP_SE3_PURE_PT2PT: *mi = {KIND_PURE, EST_PT2PT}; return true;
        case SE3ICP_SE3_PURE_PT2PL: *mi = {KIND_PURE, EST_PT2PL}; return true;
        case SE3ICP_SE3_PURE_GICP: *mi = {KIND_PURE, EST_GICP}; return true;
        default: return false;
    }
}

// The plan of `method` with number_of_nn_for_LRF = k_lrf; SE3ICP_ERR_INVALID_METHOD, or
// SE3ICP_ERR_INVALID_ARG for an SE(3) method without neighbours for its frames.
int plan_method(int method, int k_lrf, MethodPlan* mp) {
    MethodInfo mi;
    if (!decode_method(method, &mi)) return SE3ICP_ERR_INVALID_METHOD;
    *mp = MethodPlan{mi.kind, mi.est, mi.kind != KIND_ICP, 0, 0, 0, 1};
    mp->k_lrf = mp->se3 ? k_lrf : 0;
    if (mp->se3 && k_lrf <= 0) return SE3ICP_ERR_INVALID_ARG;
    if (mi.est == EST_PT2PL) mp->k_nrm_t = 30;                    // target_.EstimateNormals() default KNN(30)
    if (mi.est == EST_GICP) mp->k_nrm_s = mp->k_nrm_t = 20;       // InitializePointCloudForGeneralizedICP KNN(20)
    mp->kmax = std::max({mp->k_lrf, mp->k_nrm_s, mp->k_nrm_t, 1});
    return 0;
}

// The setup table entry of a pair's source (side 0) or target (side 1).  cf_now: a cf target's
// 12-D search rows are formed by this setup (a sweep forms them per variant instead).
CloudSetup cloud_setup(const MethodPlan& mp, int side, double alpha, double beta, bool cf_now) {
    CloudSetup st{};
    st.k_lrf = mp.k_lrf;
    st.k_nrm = side == 0 ? mp.k_nrm_s : mp.k_nrm_t;
    st.k_knn = std::max(st.k_lrf, st.k_nrm);
    st.want_cov = mp.est == EST_GICP;
    st.want_conf = mp.kind == KIND_CF;
    st.is_target = side;
    st.cf_target = cf_now && mp.kind == KIND_CF && side == 1;
    st.alpha = alpha;
    st.beta = beta;
    st.norm_scale = 1.0;
    return st;
}

// The plan of a batch's or a sweep's method and the check of its pairs' clouds, in the order
// the entries report them: the method, the clouds (SE3ICP_ERR_EMPTY_CLOUD, then
// SE3ICP_ERR_INVALID_ARG for a null cloud, pair by pair), the frames' k.
int plan_pairs(int method, int k_lrf, int npairs, const double* const* src, const int64_t* ns,
               const double* const* tgt, const int64_t* nt, MethodPlan* mp) {
    const int rc = plan_method(method, k_lrf, mp);
    if (rc == SE3ICP_ERR_INVALID_METHOD) return rc;
    for (int p = 0; p < npairs; ++p) {
        if (ns[p] <= 0 || nt[p] <= 0) return SE3ICP_ERR_EMPTY_CLOUD;
        if (!src[p] || !tgt[p]) return SE3ICP_ERR_INVALID_ARG;
    }
    return rc;
}

// The clouds some edge of a graph uses, in cloud order: slot[c] is cloud c's place in `used`
// (-1: unused).  SE3ICP_ERR_INVALID_ARG for an edge outside the set or a used cloud that is
// null, SE3ICP_ERR_EMPTY_CLOUD for an empty one.
int graph_used_clouds(int C, const double* const* xyz, const int64_t* npts, int P, const int32_t* esrc,
                      const int32_t* etgt, std::vector<int32_t>* slot, std::vector<int32_t>* used) {
    slot->assign(C, -1);
    for (int p = 0; p < P; ++p) {
        if (esrc[p] < 0 || esrc[p] >= C || etgt[p] < 0 || etgt[p] >= C) return SE3ICP_ERR_INVALID_ARG;
        (*slot)[esrc[p]] = (*slot)[etgt[p]] = 0;
    }
    for (int c = 0; c < C; ++c)
        if ((*slot)[c] == 0) {
            if (npts[c] <= 0) return SE3ICP_ERR_EMPTY_CLOUD;
            if (!xyz[c]) return SE3ICP_ERR_INVALID_ARG;
            (*slot)[c] = (int32_t)used->size();
            used->push_back(c);
        }
    return 0;
}

// Wait for an event by polling: the loop's host side has nothing else to do, and a
// blocking wait adds the thread's wake-up latency to every step.
hipError_t spin_wait(hipEvent_t e) {
    for (;;) {
        const hipError_t r = hipEventQuery(e);
        if (r != hipErrorNotReady) return r;
    }
}

// Wait until every pair's phase of the next iteration is in the coherent host slot
// (cleared to -1 before the iteration was queued; written by the next k_nn_prep, or by
// k_reduce_final without look-ahead): the loop needs no per-iteration end event, whose
// marker leaves the GPU idle ~5 us.  The stream is queried only after 20 ms without the slot
// (a stream that completed or failed with it unwritten is reported, not waited on):
// hipStreamQuery itself puts a marker into the stream, which held the GPU idle ~6 us per
// iteration when it was called every 1,024 polls (round 3).
hipError_t spin_phases(const volatile int32_t* slot, int n, hipStream_t s) {
    auto next = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
    for (unsigned spins = 0;; ++spins) {
        int left = 0;
        for (int p = 0; p < n; ++p) left += slot[p] < 0;
        if (left == 0) return hipSuccess;
        if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() >= next) {
            const hipError_t r = hipStreamQuery(s);
            if (r == hipSuccess) {
                left = 0;
                for (int p = 0; p < n; ++p) left += slot[p] < 0;
                return left == 0 ? hipSuccess : hipErrorUnknown;
            }
            if (r != hipErrorNotReady) return r;
            next = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
        }
    }
}

// An armed record against the call's `nslots` result slots (open_call): false if it names no slot
// or a negative capacity; otherwise it is reset and *pair (the trace carries its own) is its slot.
bool arm_record(se3icp_trace* tr, int64_t nslots) {
    if (tr->pair < 0 || (int64_t)tr->pair >= nslots || tr->max_iters < 0) return false;
    tr->iters_recorded = 0;
    return true;
}
bool arm_record(se3icp_setup_record* sr, int64_t nslots, int* pair) {
    if (sr->pair < 0 || (int64_t)sr->pair >= nslots || sr->src.cap < 0 || sr->tgt.cap < 0) return false;
    *pair = sr->pair;
    sr->recorded = 0;
    sr->src.n = sr->tgt.n = 0;
    sr->src.written = sr->tgt.written = 0;
    return true;
}
bool arm_record(se3icp_tree_record* tk, int64_t nslots, int* pair) {
    if (tk->pair < 0 || (int64_t)tk->pair >= nslots) return false;
    for (const se3icp_tree_side* t : {&tk->src3, &tk->tgt3, &tk->src12, &tk->tgt12})
        if (t->cap < 0 || t->node_cap < 0) return false;
    *pair = tk->pair;
    tk->recorded = 0;
    return true;
}

static_assert(GS_COUNT == 9, "Engine::graph_stats_");
constexpr size_t kShareMaxSlots = 65535;  // k_share_hash takes one grid row per slot
constexpr int kStatSlots = 64;  // work counters: [64][kStatCols] u64 (spread against atomic contention)

}  // namespace

Engine::Engine(int device) : dev_(device) {
    for (auto& e : ev_) e = nullptr;
    for (auto& e : loop_ev_) e = nullptr;
    ok_ = init() == 0;
}

int Engine::init() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || dev_ < 0 || dev_ >= n) return SE3ICP_ERR_NO_DEVICE;
    HIPCHK(hipSetDevice(dev_));
    HIPCHK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    for (auto& e : ev_) HIPCHK(hipEventCreate(&e));
    for (auto& e : loop_ev_) HIPCHK(hipEventCreate(&e));
    if (const char* e = std::getenv("SE3ICP_NN_TRACE")) nn_trace_ = std::atoi(e) != 0;
    return 0;
}

Engine::~Engine() {
    if (!ok_) return;
    (void)hipSetDevice(dev_);
    for (DevBuf* b : bufs_)
        if (b->p) (void)hipFree(b->p);
    for (PinnedMem* m : pins_)
        if (m->mem) (void)hipHostFree(m->mem);
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : loop_ev_)
        if (e) (void)hipEventDestroy(e);
    if (h_phase_) (void)hipHostFree(h_phase_);
    if (stream_) (void)hipStreamDestroy(stream_);
}

template <class T>
T* Engine::ensure(DevBuf& b, size_t count) {
    const size_t want = std::max<size_t>(count, 1) * sizeof(T);
    if (b.bytes >= want) return static_cast<T*>(b.p);
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
    const size_t alloc = want + want / 4;
    if (hipMalloc(&b.p, alloc) != hipSuccess) {
        b.p = nullptr;
        return nullptr;
    }
    b.bytes = alloc;
    return static_cast<T*>(b.p);
}

int Engine::alloc_points(int64_t ntot, int kmax, bool knn_list) {
    if (ntot >= (int64_t)1 << 30) return SE3ICP_ERR_INVALID_ARG;
    ntot_ = ntot;
    ld_ = (int)((std::max<int64_t>(ntot, 1) + 63) / 64 * 64);
    kmax_ = std::max(kmax, 1);
    knn_list_ = knn_list;
    const size_t L = (size_t)ld_;
    bool ok = ensure<int32_t>(d_cloud_of_, L) && ensure<double>(d_in_, 3 * L) && ensure<double>(d_xyz64_, 3 * L) &&
              ensure<float>(d_xyz32_, 3 * L) && ensure<double>(d_fr64_, 12 * L) && ensure<float>(d_fr32_, 12 * L) &&
              ensure<double>(d_nrm64_, 3 * L) && ensure<double>(d_conf64_, L) && ensure<double>(d_tgeo_, 8 * L) &&
              (!knn_list || ensure<int32_t>(d_knn_, L * kmax_)) && ensure<int32_t>(d_corr_idx_, L) && ensure<float>(d_corr_dist_, L) &&
              ensure<int32_t>(d_flag_count_, 4) &&
              ensure<uint32_t>(d_keys0_, L) &&
              ensure<int32_t>(d_vals1_, L) && ensure<unsigned long long>(d_stats_, kStatCols * kStatSlots) &&
              ensure<NNCert>(d_cert_, L) &&
              ensure<int32_t>(d_sqlist_, L);
    for (TreeBufs* t : {&t3_, &t12_})
        ok = ok && ensure<int32_t>(t->perm, L) && ensure<int32_t>(t->pos, L);
    ok = ok && ensure<float>(t3_.vec, 3 * L) && ensure<float>(t12_.vec, 12 * L);
    return ok ? 0 : SE3ICP_ERR_OUT_OF_MEMORY;
}

View Engine::view() const {
    View v{};
    v.ld = ld_;
    v.npts = (int32_t)ntot_;
    v.nclouds = nclouds_;
    v.npairs = npairs_;
    v.kmax = kmax_;
    v.clouds = (CloudDev*)d_clouds_.p;
    v.setup = (CloudSetup*)d_setup_.p;
    v.pairs = (PairDev*)d_pairs_.p;
    v.cloud_of = (int32_t*)d_cloud_of_.p;
    v.in_ptr = (const double* const*)d_inptr_.p;
    v.xyz64 = (double*)d_xyz64_.p;
    v.xyz32 = (float*)d_xyz32_.p;
    v.fr64 = (double*)d_fr64_.p;
    v.fr32 = (float*)d_fr32_.p;
    v.nrm64 = (double*)d_nrm64_.p;
    v.conf64 = (double*)d_conf64_.p;
    v.tgeo = (double*)d_tgeo_.p;
    v.knn = knn_list_ ? (int32_t*)d_knn_.p : nullptr;
    v.corr_idx = (int32_t*)d_corr_idx_.p;
    v.corr_dist = (float*)d_corr_dist_.p;
    v.stats = (unsigned long long*)d_stats_.p;
    v.flag_count = (int32_t*)d_flag_count_.p;
    v.gcost = (uint32_t*)d_gcost_.p;
    v.cls = (int32_t*)d_cls_.p;
    v.trim_key = (uint64_t*)d_trim_key_.p;
    v.trim_cand = (unsigned long long*)d_trim_cand_.p;
    v.trim_ctr = (unsigned*)d_trim_ctr_.p;
    v.trim_hist = (unsigned*)d_trim_hist_.p;
    v.red_partial = (double*)d_red_partial_.p;
    v.red_out = (double*)d_red_out_.p;
    v.work = (const BlockWork*)d_work_.p;
    v.nwork = nwork_;
    v.pair_rechecked = (int32_t*)d_rechecked_.p;
    auto ref = [&](const TreeBufs& t) {
        TreeRef r{};
        r.L = t.L;
        r.GL = tree_L_;
        r.nnodes = 2 << t.L;
        r.perm = (const int32_t*)t.perm.p;
        r.pos = (const int32_t*)t.pos.p;
        r.tvec = (const float*)t.vec.p;
        r.tvec64 = (const double*)t.vec64.p;
        r.tpt64 = (const double4*)t.vec64a.p;
        r.lo = (const float*)t.lo.p;
        r.hi = (const float*)t.hi.p;
        return r;
    };
    v.t3 = ref(t3_);
    v.t12 = ref(t12_);
    v.chunk_level = chunk_level_;
    v.nchunks = nchunks_;
    v.qlist = (int32_t*)d_qlist_.p;
    v.qcount = (int32_t*)d_qcount_.p;
    v.sq_list = (int32_t*)d_sqlist_.p;
    v.hist = (const double*)d_hist_.p;
    v.cert = (NNCert*)d_cert_.p;
    return v;
}

// ----------------------------------------------------------------------------- kd-trees
int Engine::build_tree(int D, const float* vec, hipStream_t s, const double* vec64, const std::vector<int32_t>* role,
                       TreeTab* tab) {
    TreeBufs& tb = (D == 12) ? t12_ : t3_;
    tb.L = tree_L_;
    const int nnodes = 2 << tb.L;
    const size_t nb = (size_t)nclouds_ * nnodes * D;
    if (!ensure<uint32_t>(tb.blo, nb) || !ensure<uint32_t>(tb.bhi, nb) || !ensure<float>(tb.lo, nb) ||
        !ensure<float>(tb.hi, nb) || !ensure<float>(tb.scr, (size_t)D * ld_) ||
        (D == 12 && !ensure<float>(tb.vecT, (size_t)12 * ld_)) ||
        (vec64 && !ensure<double>(tb.vec64, (size_t)3 * ld_)) ||
        (vec64 && D == 3 && !ensure<double4>(tb.vec64a, (size_t)ld_)))
        return SE3ICP_ERR_OUT_OF_MEMORY;
    std::vector<int32_t> host_n(nclouds_);
    int max_n = 0;
    for (int c = 0; c < nclouds_; ++c) max_n = std::max(max_n, host_n[c] = h_clouds_[c].n);
    const size_t need = tree_build_temp_bytes((int)ntot_, nclouds_, max_n, tb.L);
    if (!ensure<char>(d_sort_tmp_, std::max<size_t>(need, 256))) return SE3ICP_ERR_OUT_OF_MEMORY;
    TreeView t{};
    t.host_n = host_n.data();
    t.D = D;
    t.L = tb.L;
    t.nnodes = nnodes;
    t.nclouds = nclouds_;
    t.npts = (int32_t)ntot_;
    t.ld = ld_;
    t.clouds = (const CloudDev*)d_clouds_.p;
    t.cloud_of = (const int32_t*)d_cloud_of_.p;
    t.vec = vec;
    t.vecT = (D == 12) ? (float*)tb.vecT.p : const_cast<float*>(vec);  // (3-D: the input is columns)
    t.perm = (int32_t*)tb.perm.p;
    t.pos = (int32_t*)tb.pos.p;
    t.tvec = (float*)tb.vec.p;
    t.vec64 = vec64;
    t.tvec64 = vec64 ? (double*)tb.vec64.p : nullptr;
    t.tpt64 = (vec64 && D == 3) ? (double4*)tb.vec64a.p : nullptr;
    t.vec64_sources_only = D == 12;  // the loop reads f64 12-D vectors of source clouds (even ids) only
    t.blo = (uint32_t*)tb.blo.p;
    t.bhi = (uint32_t*)tb.bhi.p;
    t.scr = (float*)tb.scr.p;
    t.lo = (float*)tb.lo.p;
    t.hi = (float*)tb.hi.p;
    // builders and adopters: with every cloud a builder the launches are those of a build
    // without a table
    int nbuild = nclouds_, nadopt = 0;
    if (role && tab) {
        nbuild = 0;
        for (int c = 0; c < nclouds_; ++c) {
            nbuild += (*role)[c] == kTreeBuilds;
            nadopt += (*role)[c] >= 0;
        }
    }
    if (nbuild != nclouds_) {
        const size_t words = (size_t)nclouds_ + nbuild + nadopt;
        if (tab->host.reserve(words) || !ensure<int32_t>(tab->dev, words)) return SE3ICP_ERR_OUT_OF_MEMORY;
        int32_t* h = tab->host;
        size_t at = (size_t)nclouds_;
        for (int c = 0; c < nclouds_; ++c) h[c] = (*role)[c];
        for (int c = 0; c < nclouds_; ++c)
            if ((*role)[c] == kTreeBuilds) h[at++] = c;
        for (int c = 0; c < nclouds_; ++c)
            if ((*role)[c] >= 0) h[at++] = c;
        HIPCHK(hipMemcpyAsync(tab->dev.p, h, sizeof(int32_t) * words, hipMemcpyHostToDevice, s));
        t.role = (const int32_t*)tab->dev.p;
        t.list = t.role + nclouds_;
        t.nbuild = nbuild;
        t.nadopt = nadopt;
    }
    tree_stats_[D == 12 ? 2 : 0] += nbuild;
    tree_stats_[D == 12 ? 3 : 1] += nadopt;
    int levels[2] = {0, 0};  // G and H as build_trees launched them
    if (build_trees(t, d_sort_tmp_.p, d_sort_tmp_.bytes, (uint32_t*)d_keys0_.p, (int32_t*)d_vals1_.p, s, levels) != 0)
        return SE3ICP_ERR_HIP;
    {
        // what this build is for every slot it touches (se3icp_set_tree_record)
        std::vector<TreeLog>& log = tree_log_[D == 12];
        if ((int)log.size() != nclouds_) log.assign(nclouds_, TreeLog{});
        const int G = levels[0], H = levels[1];
        auto role_of = [&](int c) { return nbuild != nclouds_ ? (*role)[c] : kTreeBuilds; };
        for (int c = 0; c < nclouds_; ++c)
            if (role_of(c) == kTreeBuilds) log[c] = TreeLog{kTreeBuilds, tb.L, G, H};
        for (int c = 0; c < nclouds_; ++c)  // an adopter's order took its donor's path
            if (role_of(c) >= 0) log[c] = TreeLog{role_of(c), tb.L, G, log[role_of(c)].H};
    }
    return 0;
}

// ----------------------------------------------------------------------------- setup
int Engine::upload_clouds(const std::vector<CloudReq>& clouds, bool on_device, hipStream_t s) {
    nclouds_ = (int)clouds.size();
    h_clouds_.assign(nclouds_, CloudDev{});
    h_setup_.resize(nclouds_);
    h_chunks_.clear();
    h_inptr_.assign(nclouds_, nullptr);
    int64_t off = 0;
    int max_n = 1;
    for (int c = 0; c < nclouds_; ++c) {
        h_clouds_[c].off = (int32_t)off;
        h_clouds_[c].n = (int32_t)clouds[c].n;
        h_setup_[c] = clouds[c].st;
        max_n = std::max<int>(max_n, (int)clouds[c].n);
        for (int64_t p0 = 0; p0 < clouds[c].n; p0 += kChunk) h_chunks_.push_back(ChunkWork{c, (int32_t)p0});
        off += clouds[c].n;
    }
    tree_L_ = tree_depth_for(max_n);
    // inputs
    double* d_in = (double*)d_in_.p;
    for (int c = 0; c < nclouds_; ++c) {
        if (on_device) {
            h_inptr_[c] = clouds[c].in;
        } else {
            double* dst = d_in + 3 * (size_t)h_clouds_[c].off;
            HIPCHK(hipMemcpyAsync(dst, clouds[c].in, sizeof(double) * 3 * clouds[c].n, hipMemcpyHostToDevice, s));
            h_inptr_[c] = dst;
        }
    }
    const int nch = (int)h_chunks_.size();
    if (!ensure<CloudDev>(d_clouds_, nclouds_) || !ensure<CloudSetup>(d_setup_, nclouds_) ||
        !ensure<ChunkWork>(d_chunks_, nch) || !ensure<const double*>(d_inptr_, nclouds_) ||
        !ensure<double>(d_partial_, (size_t)nch * 9) || !ensure<double>(d_centers_, 3 * (size_t)nclouds_))
        return SE3ICP_ERR_OUT_OF_MEMORY;
    if (h_partial_.reserve((size_t)nch * 9 + 8)) return SE3ICP_ERR_OUT_OF_MEMORY;
    HIPCHK(hipMemcpyAsync(d_clouds_.p, h_clouds_.data(), sizeof(CloudDev) * nclouds_, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_setup_.p, h_setup_.data(), sizeof(CloudSetup) * nclouds_, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_chunks_.p, h_chunks_.data(), sizeof(ChunkWork) * nch, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_inptr_.p, h_inptr_.data(), sizeof(double*) * nclouds_, hipMemcpyHostToDevice, s));
    return 0;
}

// (the summation order is part of the result: it is the centroid every f32 copy is taken around)
int Engine::host_centroids(hipStream_t s, std::vector<double>* cen) {
    const int nch = (int)h_chunks_.size();
    HIPCHK(hipMemcpyAsync(h_partial_, d_partial_.p, sizeof(double) * 9 * nch, hipMemcpyDeviceToHost, s));
    SYNC_STREAM(s);
    std::vector<double> sum(3 * (size_t)nclouds_, 0.0);
    for (int k = 0; k < nch; ++k)
        for (int a = 0; a < 3; ++a) sum[3 * (size_t)h_chunks_[k].cloud + a] += h_partial_[9 * (size_t)k + a];
    cen->assign(3 * (size_t)nclouds_, 0.0);
    for (int c = 0; c < nclouds_; ++c)
        for (int a = 0; a < 3; ++a)
            (*cen)[3 * (size_t)c + a] = h_clouds_[c].n > 0 ? sum[3 * (size_t)c + a] / (double)h_clouds_[c].n : 0.0;
    return 0;
}

// (see engine.hpp)
int Engine::queue_norm_params(bool pairs, bool normalize, double scale_pre, hipStream_t s) {
    const int nch = (int)h_chunks_.size();
    const View v = view();
    // 1) ingest: SoA copy + sums + bbox
    launch_ingest(v, (const ChunkWork*)d_chunks_.p, nch, (double*)d_partial_.p, s);
    HIPCHK(hipGetLastError());
    if (normalize) {
        // 2) normalization parameters (ISR.cpp:568-574) on the device: no host round trip;
        // the centers (d_centers_) and scales (d_scales_) stay there for the loop and the
        // final de-normalization
        if (!ensure<double>(d_scales_, std::max(1, nclouds_ / 2))) return SE3ICP_ERR_OUT_OF_MEMORY;
        launch_pair_centers(v, (const ChunkWork*)d_chunks_.p, nch, (const double*)d_partial_.p, (double*)d_centers_.p,
                            s);
        launch_radius(v, (const ChunkWork*)d_chunks_.p, nch, (const double*)d_centers_.p, (double*)d_partial_.p, s);
        launch_pair_scales(v, (const ChunkWork*)d_chunks_.p, nch, (const double*)d_partial_.p,
                           (const double*)d_centers_.p, scale_pre, (double*)d_scales_.p, s);
        HIPCHK(hipGetLastError());
        for (int c = 0; c < nclouds_; ++c)  // (the device holds the normalization fields)
            for (int a = 0; a < 3; ++a) h_setup_[c].f32_center[a] = 0.0;
        return 0;
    }
    std::vector<double> cen;
    const int rc = host_centroids(s, &cen);
    if (rc) return rc;
    for (int c = 0; c < nclouds_; ++c) {
        // raw coordinates; f32 copies centered on the target (pairs) / own centroid (single clouds)
        const int cc = pairs ? (c | 1) : c;
        for (int a = 0; a < 3; ++a) {
            h_setup_[c].norm_center[a] = 0.0;
            h_setup_[c].f32_center[a] = cen[3 * cc + a];
        }
        h_setup_[c].norm_scale = 1.0;
    }
    HIPCHK(hipMemcpyAsync(d_setup_.p, h_setup_.data(), sizeof(CloudSetup) * nclouds_, hipMemcpyHostToDevice, s));
    return 0;
}

int Engine::setup_clouds(const std::vector<CloudReq>& clouds, bool on_device, bool pairs, bool normalize,
                         double scale_pre, hipStream_t s) {
    int rc = upload_clouds(clouds, on_device, s);
    if (rc) return rc;
    rc = queue_norm_params(pairs, normalize, scale_pre, s);
    if (rc) return rc;
    const int nch = (int)h_chunks_.size();
    View v = view();

    // 3) normalize in place + f32 copy
    launch_normalize(v, (const ChunkWork*)d_chunks_.p, nch, (double*)d_partial_.p, s);
    HIPCHK(hipGetLastError());

    // 4) 3-D kd-trees of every cloud (kNN for TOLDI / normals, and the R3 NN of the loop)
    rc = build_tree(3, (const float*)d_xyz32_.p, s, (const double*)d_xyz64_.p);
    if (rc) return rc;
    rc = setup_knn(s);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return 0;
}

// kNN / TOLDI frames / normals of the clouds that were normalized and given their 3-D trees
// (step 4 of setup_clouds; Engine::register_graph runs it over its classes).
int Engine::setup_knn(hipStream_t s, const SelectPlan* sel) {
    const View v = view();
    bool any_knn = false;
    for (int c = 0; c < nclouds_; ++c) any_knn |= h_setup_[c].k_knn > 0;
    if (any_knn) {
        HIPCHK(hipMemsetAsync(d_stats_.p, 0, sizeof(unsigned long long) * kStatCols * kStatSlots, s));
        HIPCHK(hipEventRecord(ev_[EV_LRF_BEGIN], s));
        // neighbourhoods over kSmallK (Kw = min(k, n)) go to k_knn_big, the rest to the LDS
        // kernels; the global-buffer kernel's candidate buffers are sized to the largest
        int kw_big = 0, n_big = 0;
        for (int c = 0; c < nclouds_; ++c) {
            const int kw = std::min<int>(h_setup_[c].k_knn, h_clouds_[c].n);
            if (kw > kSmallK || lrf_exact_only_ == 2) {
                kw_big = std::max(kw_big, kw);
                n_big += h_clouds_[c].n;
            }
        }
        int big_cap = 0, big_blocks = 0;
        if (n_big > 0) {
            big_cap = knn_big_cap(kw_big);
            big_blocks = knn_big_blocks(big_cap, n_big);
            if (!ensure<double>(d_big_d_, (size_t)big_blocks * big_cap) || !ensure<int32_t>(d_big_i_, (size_t)big_blocks * big_cap))
                return SE3ICP_ERR_OUT_OF_MEMORY;
        }
        auto big = [&](const int32_t* qlist, const int32_t* qcount, int k_min) {
            if (n_big > 0)
                launch_knn_big(v, knn_list_ ? 1 : 0, k_min, qlist, qcount, big_blocks, (double*)d_big_d_.p,
                               (int32_t*)d_big_i_.p, big_cap, s);
        };
        if (lrf_exact_only_ == 2) {
            big(nullptr, nullptr, 0);  // (diagnostic: every query through the global-buffer kernel)
        } else if (knn_list_ || lrf_exact_only_ == 1) {
            launch_lrf(v, knn_list_ ? 1 : 0, s);  // the sorted lists (se3icp_knn_self) need the exact kernel
            big(nullptr, nullptr, kSmallK);
        } else {
            // eight queries per wavefront; the few it cannot resolve from f32 keys (and every
            // query of a cloud whose k it cannot hold) go to the exact kernels.  Three wave tables
            // (graph.hpp, select_wave_tables): sources, take, redo in stream order.
            const bool seeding = sel && sel->seeds, taking = seeding && sel->takes;
            const int nt = nclouds_ + 1;
            const WaveTables wt = select_wave_tables(nclouds_, h_clouds_.data(), h_setup_.data(), sel);
            const int nw = wt.nw, nw_sd = wt.nw_sd, nw_tk = wt.nw_tk;
            if (!ensure<int32_t>(d_lrf_fb_, (size_t)8 * ((size_t)nw + nw_sd + nw_tk) + 64) ||
                !ensure<int32_t>(d_lrf_fbn_, 2 + 3 * (size_t)nt))
                return SE3ICP_ERR_OUT_OF_MEMORY;
            int32_t* d_wb = (int32_t*)d_lrf_fbn_.p + 2;
            int32_t* fb = (int32_t*)d_lrf_fb_.p;
            int32_t* fbn = (int32_t*)d_lrf_fbn_.p;
            HIPCHK(hipMemsetAsync(fbn, 0, 2 * sizeof(int32_t), s));
            HIPCHK(hipMemcpyAsync(d_wb, wt.wb.data(), sizeof(int32_t) * 3 * nt, hipMemcpyHostToDevice, s));
            if (seeding) {
                // (with taking the bounds Lb follow the seeds: one fill marks both absent)
                const size_t nseed = (size_t)sel->seed_floats * (taking ? 2 : 1);
                if (!ensure<float>(d_seed_, nseed) || !ensure<SeedRef>(d_seed_ref_, nclouds_))
                    return SE3ICP_ERR_OUT_OF_MEMORY;
                HIPCHK(hipMemsetAsync(d_seed_.p, 0xff, sizeof(float) * nseed, s));  // all ones: absent
                HIPCHK(hipMemcpyAsync(d_seed_ref_.p, sel->seed_ref.data(), sizeof(SeedRef) * nclouds_, hipMemcpyHostToDevice, s));
                const SeedRef* sref = (const SeedRef*)d_seed_ref_.p;
                float* sbuf = (float*)d_seed_.p;
                TakeArgs tk{nullptr, nullptr, nullptr, 0, 0, 0};
                if (taking && nw_tk > 0) {
                    if (!ensure<uint32_t>(d_take_lists_, (size_t)sel->seed_floats * (size_t)sel->take_stride) ||
                        !ensure<int32_t>(d_take_flag_, nclouds_) || !ensure<unsigned char>(d_take_mask_, (size_t)nw_tk + 64))
                        return SE3ICP_ERR_OUT_OF_MEMORY;
                    HIPCHK(hipMemcpyAsync(d_take_flag_.p, sel->take_flag.data(), sizeof(int32_t) * nclouds_, hipMemcpyHostToDevice, s));
                    HIPCHK(hipMemsetAsync(d_take_mask_.p, 0, (size_t)nw_tk + 64, s));
                    tk = TakeArgs{(const int32_t*)d_take_flag_.p, (uint32_t*)d_take_lists_.p, nullptr, sel->take_stride,
                                  (int32_t)sel->seed_floats, sel->take_mode};
                }
                launch_lrf8(v, d_wb, 0, nw, fb, fbn, s, sref, sbuf, false, sel->seed_mode, &tk);
                launch_lrf8(v, d_wb + nt, 0, nw_sd, fb, fbn, s, sref, sbuf, true, sel->seed_mode);
                if (tk.flag != nullptr) {
                    tk.mask = (unsigned char*)d_take_mask_.p;
                    launch_lrf8(v, d_wb + 2 * nt, 0, nw_tk, fb, fbn, s, sref, sbuf, true, sel->seed_mode, &tk, true);
                    launch_lrf8(v, d_wb + 2 * nt, 0, nw_tk, fb, fbn, s, sref, sbuf, true, sel->seed_mode, &tk);
                }
            } else {
                launch_lrf8(v, d_wb, 0, nw, fb, fbn, s);
            }
            launch_lrf_list(v, fb, fbn, s);
            big(fb, fbn, kSmallK);
        }
        HIPCHK(hipEventRecord(ev_[EV_LRF_END], s));
        HIPCHK(hipGetLastError());
        // work counters: copied now, read at the next synchronisation (read_lrf_stats)
        if (h_lrf_stats_.reserve((size_t)kStatCols * kStatSlots)) return SE3ICP_ERR_OUT_OF_MEMORY;
        HIPCHK(hipMemcpyAsync(h_lrf_stats_, d_stats_.p, sizeof(unsigned long long) * kStatCols * kStatSlots,
                              hipMemcpyDeviceToHost, s));
        lrf_stats_pending_ = true;
    }
    return 0;
}

// k_lrf time and work counters of the last setup (after the stream has passed them)
int Engine::read_lrf_stats() {
    if (!lrf_stats_pending_) return 0;
    lrf_stats_pending_ = false;
    double sum[kStatCols] = {};
    for (int i = 0; i < kStatSlots; ++i)
        for (int k = 0; k < kStatCols; ++k) sum[k] += (double)h_lrf_stats_[kStatCols * i + k];
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev_[EV_LRF_BEGIN], ev_[EV_LRF_END]));
    ktimes_.lrf_ms = ms;
    ktimes_.lrf_queries = sum[0];
    ktimes_.lrf_leaves = sum[1];
    ktimes_.lrf_merges = sum[2];
    ktimes_.lrf_box_tests = sum[3];
    ktimes_.lrf_candidates = sum[4];
    ktimes_.lrf_fallback = sum[6];
    for (int k = 0; k < 3; ++k) {  // k_lrf8's launch of seeded clouds (integers, summed as such)
        unsigned long long q = 0;
        for (int i = 0; i < kStatSlots; ++i) q += h_lrf_stats_[kStatCols * i + kSeedStatCol + k];
        seed_stats_[1 + k] = (int64_t)q;
    }
    {  // ... and of taking clouds (kTakeStatCol: taken; redone | failed << 32)
        unsigned long long t = 0, r = 0, f = 0;
        for (int i = 0; i < kStatSlots; ++i) {
            t += h_lrf_stats_[kStatCols * i + kTakeStatCol];
            r += h_lrf_stats_[kStatCols * i + kTakeStatCol + 1] & 0xffffffffull;
            f += h_lrf_stats_[kStatCols * i + kTakeStatCol + 1] >> 32;
        }
        take_stats_[TS_TAKEN] = (int64_t)t;
        take_stats_[TS_REDONE] = (int64_t)r;
        take_stats_[TS_FAILED] = (int64_t)f;
    }
#ifdef SE3ICP_PROF
    tree_prof_report();
    std::fprintf(stderr, "[prof] k_lrf cycles/query: knn|scan %.0f sort|tighten %.0f sums|final+sums %.0f finish %.0f "
                 "(queries %.0f, wave cycles summed over the kernel's waves)\n",
                 sum[8] / sum[0], sum[9] / sum[0], sum[10] / sum[0], sum[11] / sum[0], sum[0]);
    std::fprintf(stderr, "[prof] k_lrf8 per query: tightenings %.3f (overflow %.3f, final %.3f), leaf scans %.3f\n",
                 sum[2] / sum[0], sum[3] / sum[0], sum[7] / sum[0], sum[1] / sum[0]);
    {
        unsigned long long f = 0;  // (16-bit fields, summed as integers)
        for (int i = 0; i < kStatSlots; ++i) f += h_lrf_stats_[kStatCols * i + 5];
        std::fprintf(stderr, "[prof] k_lrf8 hand-overs: waves with the leaf table full %llu, no room %llu, > 128 at the end %llu; "
                     "queries with f32-equal f64-distinct ranks %llu\n",
                     f & 0xffff, (f >> 16) & 0xffff, (f >> 32) & 0xffff, f >> 48);
    }
#endif
    return 0;
}

// Wait for everything queued on `s` (polling, see spin_wait).
int Engine::sync_stream(hipStream_t s) {
    HIPCHK(hipEventRecord(ev_[EV_SYNC], s));
    HIPCHK(spin_wait(ev_[EV_SYNC]));
    return read_lrf_stats();
}

// loop NN work chunks: nodes of level tree_L_ - 4 of every source tree (<= kChunkQ
// positions each), their query lists, the pose history and void NN certificates
int Engine::setup_chunks(int npairs, hipStream_t s) {
    chunk_level_ = std::max(0, tree_L_ - 4);
    nchunks_ = npairs << chunk_level_;
    if (!ensure<int32_t>(d_qlist_, (size_t)nchunks_ * kChunkQ) || !ensure<int32_t>(d_qcount_, (size_t)nchunks_ * (kChunkQ / 64)) ||
        !ensure<double>(d_hist_, (size_t)kHist * npairs * 12) || !ensure<uint32_t>(d_gcost_, (size_t)nchunks_ * 16) ||
        !ensure<int32_t>(d_cls_, nn_cls_words(nchunks_)))
        return SE3ICP_ERR_OUT_OF_MEMORY;
    if (h_hist_.reserve((size_t)npairs * 12)) return SE3ICP_ERR_OUT_OF_MEMORY;
    HIPCHK(hipMemsetAsync(d_cert_.p, 0xff, sizeof(NNCert) * ld_, s));  // iteration -1: no certificate
    HIPCHK(hipMemsetAsync(d_gcost_.p, 0, sizeof(uint32_t) * nchunks_ * 16, s));
    HIPCHK(hipMemsetAsync(d_cls_.p, 0, sizeof(int32_t) * 2 * 8 * 16, s));
    return 0;
}

// ----------------------------------------------------------------------------- batch registration
// The opening of a registration call (see engine.hpp).
int Engine::open_call(int args, int64_t nslots, int rest, hipStream_t user_stream, Call* c) {
    if (!ok_) return SE3ICP_ERR_NO_DEVICE;
    c->tr = std::exchange(trace_, nullptr);  // one-shot: the records cover this call only, rejected or not
    c->sr = std::exchange(setup_rec_, nullptr);
    c->tk = std::exchange(tree_rec_, nullptr);
    for (std::vector<TreeLog>& log : tree_log_) log.clear();
    pose_raw_.clear();  // (a call without a posed edge plans its seeds over clouds)
    pose_rigid_.clear();
    if (args) return args;
    if (c->tr && !arm_record(c->tr, nslots)) return SE3ICP_ERR_INVALID_ARG;
    if (c->sr && !arm_record(c->sr, nslots, &c->sr_pair)) return SE3ICP_ERR_INVALID_ARG;
    if (c->tk && !arm_record(c->tk, nslots, &c->tk_pair)) return SE3ICP_ERR_INVALID_ARG;
    if (rest) return rest;
    HIPCHK(hipSetDevice(dev_));
    c->s = user_stream ? user_stream : stream_;
    ktimes_ = KernelTimes{};
    for (int64_t& x : seed_stats_) x = 0;
    for (int64_t& x : take_stats_) x = 0;
    for (int64_t& x : tree_stats_) x = 0;
    tree_donor_.clear();
    // phase times on the GPU timeline (the host does not wait for the setup): call begin,
    // setup done, loop done
    HIPCHK(hipEventRecord(ev_[EV_CALL_BEGIN], c->s));
    return 0;
}

// Everything behind the clouds' setup (see engine.hpp).
int Engine::run_pairs(const MethodPlan& mp, int npairs, const int64_t* ns, const int64_t* nt,
                      const se3icp_params* vprm, int pairs_per_variant, bool sweep, const Call& c, se3icp_result* out,
                      const se3icp_report_options* ropts, se3icp_report* reports) {
    hipStream_t s = c.s;
    int rc = 0;
    // 12-D kd-trees over the alpha/beta-weighted SE(3) elements (f64 source elements in tree order)
    // (the later slots of a confirmed cloud adopt its first slot's order: graph_plan_trees)
    const bool adopt12 = (int)tree_donor_.size() == nclouds_;
    if (mp.se3)
        rc = build_tree(12, (const float*)d_fr32_.p, s, (const double*)d_fr64_.p, adopt12 ? &tree_donor_ : nullptr,
                        &tree_tab_12_);
    if (rc) return rc;
    rc = prepare_pairs(npairs, ns, nt, s);
    if (rc) return rc;
    rc = setup_chunks(npairs, s);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(d_corr_idx_.p, 0xff, sizeof(int32_t) * ld_, s));  // no previous match yet
    HIPCHK(hipMemsetAsync(d_stats_.p, 0, sizeof(unsigned long long) * kStatCols * kStatSlots, s));
    for (double& t : trace_prev_) t = 0;
    HIPCHK(hipEventRecord(ev_[EV_SETUP_DONE], s));
    // The armed setup record, taken here: every entry's setup is complete (the kNN / frame /
    // normal kernels, k_graph_share's copies, k_sweep_expand's weighted rows) and nothing of the
    // loop is queued.  What ran between the end of the setup and this point -- the 12-D trees,
    // prepare_pairs, setup_chunks, the two clears above -- reads xyz64 / fr64 and writes the
    // trees' own buffers, the work tables, cert, gcost, cls, corr_idx and stats: none of them
    // writes xyz64, fr64, nrm64, conf64 or the setup table, and the loop only reads them, so
    // these are the arrays the loop consumes.  Unarmed, nothing is queued here.
    if (c.sr && (rc = record_setup(c.sr, c.sr_pair, s))) return rc;
    // The armed tree record, at the same point: both trees of the pair's slots are complete
    // (the 3-D ones of the setup, a sweep's replicas, the 12-D ones above) and the loop only
    // reads them.
    if (c.tk && (rc = record_trees(c.tk, c.tk_pair, s))) return rc;
    const ReportReq rq{ropts, reports};
    return run_loop(npairs, ns, mp.kind, mp.est, vprm, pairs_per_variant, sweep, c.tr, out, s,
                    (ropts && reports) ? &rq : nullptr);
}

// The Call of a sweep group (engine.hpp).
Engine::Call Engine::group_call(const Call& c, int v0, int g, int P, se3icp_trace* gtr) {
    auto local = [&](int pair) { return (pair >= v0 * P && pair < (v0 + g) * P) ? pair - v0 * P : -1; };
    Call gc;
    gc.s = c.s;
    if (c.tr && local(c.tr->pair) >= 0) {
        *gtr = *c.tr;
        gtr->pair = local(c.tr->pair);
        gc.tr = gtr;
    }
    if (c.sr && (gc.sr_pair = local(c.sr_pair)) >= 0) gc.sr = c.sr;
    if (c.tk && (gc.tk_pair = local(c.tk_pair)) >= 0) gc.tk = c.tk;
    return gc;
}

int Engine::register_batch(int npairs, const double* const* src, const int64_t* ns, const double* const* tgt,
                           const int64_t* nt, bool on_device, int method, const se3icp_params& prm,
                           se3icp_result* out, hipStream_t user_stream, const se3icp_report_options* ropts,
                           se3icp_report* reports) {
    const int args = (npairs <= 0 || !src || !tgt || !ns || !nt || !out) ? SE3ICP_ERR_INVALID_ARG : 0;
    MethodPlan mp{};
    const int rest = args ? 0 : plan_pairs(method, prm.number_of_nn_for_LRF, npairs, src, ns, tgt, nt, &mp);
    Call call;
    int rc = open_call(args, npairs, rest, user_stream, &call);
    if (rc) return rc;

    npairs_ = npairs;
    int64_t ntot = 0;
    for (int p = 0; p < npairs; ++p) ntot += ns[p] + nt[p];
    rc = alloc_points(ntot, mp.kmax);
    if (rc) return rc;
    // ---- setup (ISR.cpp:568-648)
    std::vector<CloudReq> clouds(2 * npairs);
    for (int p = 0; p < npairs; ++p)
        for (int side = 0; side < 2; ++side)
            clouds[2 * p + side] = CloudReq{side == 0 ? src[p] : tgt[p], side == 0 ? ns[p] : nt[p],
                                            cloud_setup(mp, side, prm.alpha_rot, prm.beta_transl, true)};
    // resident clouds: slots that hold the same cloud share its setup (setup_pairs_shared).
    // Slots of one point count are the only candidates; without two of them nothing is hashed.
    bool look = false;
    if (on_device && batch_sharing_ != 1) {
        std::vector<int64_t> n(clouds.size());
        for (size_t u = 0; u < clouds.size(); ++u) n[u] = clouds[u].n;
        look = clouds.size() <= kShareMaxSlots && share_any_equal_n((int32_t)n.size(), n.data());
        for (int64_t& g : graph_stats_) g = 0;
        graph_stats_[GS_CLOUDS] = graph_stats_[GS_USES] = graph_stats_[GS_CLASSES] = (int64_t)clouds.size();
        for (const CloudReq& c : clouds) graph_stats_[GS_FULL] += c.st.k_knn > 0;
    }
    rc = look ? setup_pairs_shared(clouds, mp, prm.scale_preprocessing, call.s)
              : setup_clouds(clouds, on_device, true, mp.se3, prm.scale_preprocessing, call.s);
    if (rc) return rc;
    return run_pairs(mp, npairs, ns, nt, &prm, npairs, false, call, out, ropts, reports);
}

// ----------------------------------------------------------------------------- shared slots of a device batch
// setup_clouds(clouds, on_device, pairs, normalize) for slots that may hold one cloud several
// times (engine.hpp), through the same queue_norm_params: a call without a confirmed duplicate is
// that path plus k_share_hash.  With tree sharing off the host waits for the hashes while the
// device normalizes and builds the 3-D trees; with it (the default) the trees are queued in two
// parts around the compare flags, see below.
int Engine::setup_pairs_shared(const std::vector<CloudReq>& clouds, const MethodPlan& mp, double scale_pre,
                               hipStream_t s) {
    const int U = (int)clouds.size();
    const bool se3 = mp.se3;
    int rc = upload_clouds(clouds, true, s);
    if (rc) return rc;
    const int nch = (int)h_chunks_.size();
    if (!ensure<uint64_t>(d_share_hash_, U) || !ensure<SharePair>(d_share_pairs_, U) ||
        !ensure<int32_t>(d_share_same_, U) || h_share_hash_.reserve(U) || h_share_same_.reserve(U) ||
        h_share_setup_.reserve(U))
        return SE3ICP_ERR_OUT_OF_MEMORY;
    View v = view();
    HIPCHK(hipMemsetAsync(d_share_hash_.p, 0, sizeof(uint64_t) * U, s));
    launch_share_hash(v, (unsigned long long*)d_share_hash_.p, s);
    HIPCHK(hipMemcpyAsync(h_share_hash_, d_share_hash_.p, sizeof(uint64_t) * U, hipMemcpyDeviceToHost, s));
    // (the host-centroid wait of a vanilla method brings the hashes with it)
    rc = queue_norm_params(true, se3, scale_pre, s);
    if (rc) return rc;
    if (se3) {
        // (its table comes back with the hashes: a class is the bits the device normalizes a slot with)
        HIPCHK(hipMemcpyAsync(h_share_setup_, d_setup_.p, sizeof(CloudSetup) * U, hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(ev_[EV_SHARE_HASH], s));
    }
    launch_normalize(v, (const ChunkWork*)d_chunks_.p, nch, (double*)d_partial_.p, s);
    HIPCHK(hipGetLastError());
    // The 3-D trees.  With tree sharing the later slots of a confirmed cloud adopt its first
    // slot's order, and which slots those are is known only behind the compare flags: the slots
    // that are no candidates build behind k_share_compare, so the device works through both
    // host waits (the normalization is still queued behind the first), and the candidates
    // follow the flags.  Without it every slot builds here, ahead of the first wait.
    const bool adopt = tree_sharing_ != 1;
    if (!adopt) {
        rc = build_tree(3, (const float*)d_xyz32_.p, s, (const double*)d_xyz64_.p);
        if (rc) return rc;
    }
    if (se3) HIPCHK(spin_wait(ev_[EV_SHARE_HASH]));

    // ---- candidates by (n, hash), confirmed byte for byte
    std::vector<int64_t> n(U);
    for (int u = 0; u < U; ++u) n[u] = clouds[u].n;
    std::vector<int32_t> first, cloud;
    const int ncand = share_candidates(U, n.data(), h_share_hash_, &first);
    int nc = U;
    if (ncand > 0) {
        share_pairs_.clear();
        for (int u = 0; u < U; ++u)
            if (first[u] != u) share_pairs_.push_back(SharePair{u, first[u]});
        HIPCHK(hipMemcpyAsync(d_share_pairs_.p, share_pairs_.data(), sizeof(SharePair) * ncand, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(d_share_same_.p, 1, sizeof(int32_t) * U, s));
        launch_share_compare(v, (const SharePair*)d_share_pairs_.p, ncand, (int32_t*)d_share_same_.p, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_share_same_, d_share_same_.p, sizeof(int32_t) * U, hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(ev_[EV_SHARE_FLAGS], s));
        std::vector<int32_t> role(U);
        if (adopt) {
            for (int u = 0; u < U; ++u) role[u] = first[u] == u ? kTreeBuilds : kTreeAbsent;
            rc = build_tree(3, (const float*)d_xyz32_.p, s, (const double*)d_xyz64_.p, &role, &tree_tab_a_);
            if (rc) return rc;
        }
        HIPCHK(spin_wait(ev_[EV_SHARE_FLAGS]));
        nc = share_clouds(U, first.data(), h_share_same_, &cloud);
        if (adopt) {
            // a confirmed slot adopts; a hash-equal slot the compare rejected builds
            std::vector<int32_t> donor;
            const int nad = graph_plan_trees(U, cloud.data(), n.data(), true, &donor);
            for (int u = 0; u < U; ++u) role[u] = first[u] == u ? kTreeAbsent : donor[u];
            rc = build_tree(3, (const float*)d_xyz32_.p, s, (const double*)d_xyz64_.p, &role, &tree_tab_b_);
            if (rc) return rc;
            if (nad > 0) tree_donor_ = donor;
        }
    } else if (adopt) {
        rc = build_tree(3, (const float*)d_xyz32_.p, s, (const double*)d_xyz64_.p);
        if (rc) return rc;
    }
    if (nc == U) return setup_knn(s);  // every slot a cloud of its own: the batch's path

    // ---- classes: a cloud under the bits the device normalizes the slot with
    const CloudSetup* dev_table = se3 ? (const CloudSetup*)h_share_setup_ : h_setup_.data();
    const std::vector<CloudSetup> table(dev_table, dev_table + U);
    std::vector<GraphUse> use(U);
    for (int u = 0; u < U; ++u) {
        const CloudSetup& st = table[u];
        use[u].cloud = cloud[u];
        use[u].k_nrm = st.k_nrm;
        use[u].norm_scale = st.norm_scale;
        for (int a = 0; a < 3; ++a) {
            use[u].norm_center[a] = st.norm_center[a];
            use[u].f32_center[a] = st.f32_center[a];
        }
    }
    GraphPlan plan;
    graph_plan_uses(U, use.data(), se3, true, &plan);
    graph_stats_[GS_CLOUDS] = nc;
    graph_stats_[GS_CLASSES] = (int64_t)plan.classes.size();
    return select_by_class(plan, table, mp, s);
}

// The neighbour selection of planned uses (engine.hpp): plan it (graph.hpp), copy the tables,
// select, then restore the batch's table and hand the homes' results to the other uses.
int Engine::select_by_class(const GraphPlan& plan, const std::vector<CloudSetup>& batch, const MethodPlan& mp,
                            hipStream_t s) {
    const int U = (int)batch.size();
    sel_ = graph_plan_selection(plan, h_clouds_.data(), batch.data(), mp.k_lrf,
                                SelectSwitches{lrf_seeding_, lrf_taking_, lrf_exact_only_, knn_list_, pose_seeding_},
                                tree_donor_, pose_raw_, pose_rigid_);
    graph_stats_[GS_FULL] = sel_.full;
    if (sel_.seeds) {
        seed_stats_[0] = sel_.seeded;
        init_stats_[IS_CROSS_SEEDED] = sel_.cross;
    }
    if (sel_.takes) take_stats_[TS_CLASSES] = sel_.taking;
    const int nchS = (int)sel_.chunks.size();
    if (!ensure<ChunkWork>(g_chunks_, nchS) || !ensure<GraphSeg>(g_seg_, U)) return SE3ICP_ERR_OUT_OF_MEMORY;
    h_setup_ = sel_.run;
    HIPCHK(hipMemcpyAsync(d_setup_.p, sel_.run.data(), sizeof(CloudSetup) * U, hipMemcpyHostToDevice, s));
    const int rc = setup_knn(s, &sel_);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    // the batch's own table from here on (the copies below read cf_target of the use itself)
    h_setup_ = sel_.batch;
    HIPCHK(hipMemcpyAsync(d_setup_.p, sel_.batch.data(), sizeof(CloudSetup) * U, hipMemcpyHostToDevice, s));
    if (nchS > 0) {
        HIPCHK(hipMemcpyAsync(g_chunks_.p, sel_.chunks.data(), sizeof(ChunkWork) * nchS, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(g_seg_.p, sel_.seg.data(), sizeof(GraphSeg) * U, hipMemcpyHostToDevice, s));
        launch_graph_share(view(), (const ChunkWork*)g_chunks_.p, nchS, (const GraphSeg*)g_seg_.p, s);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// Work table of k_reduce and the per-pair buffers of a batch (see engine.hpp).
int Engine::prepare_pairs(int npairs, const int64_t* ns, const int64_t* nt, hipStream_t s) {
    // work table of k_reduce: one entry per kRedQ queries of every pair
    int64_t soff = 0;
    h_work_.clear();
    h_wb_.assign(npairs, 0);
    h_wn_.assign(npairs, 0);
    for (int p = 0; p < npairs; ++p) {
        h_wb_[p] = (int32_t)h_work_.size();
        // (clouds are laid out src 0, tgt 0, src 1, ... as setup_clouds places them)
        for (int64_t q0 = 0; q0 < ns[p]; q0 += kRedQ)
            h_work_.push_back(BlockWork{p, (int32_t)q0, (int32_t)std::min<int64_t>(q0 + kRedQ, ns[p]), (int32_t)soff,
                                        (int32_t)(soff + ns[p]), {0, 0, 0}});
        soff += ns[p] + nt[p];
        h_wn_[p] = (int32_t)h_work_.size() - h_wb_[p];
    }
    nwork_ = (int)h_work_.size();
    if (!ensure<PairDev>(d_pairs_, npairs) || !ensure<BlockWork>(d_work_, nwork_) || !ensure<int32_t>(d_wb_, npairs) ||
        !ensure<int32_t>(d_wn_, npairs) || !ensure<uint64_t>(d_trim_key_, 2 * (size_t)npairs) ||
        !ensure<unsigned long long>(d_trim_cand_, (size_t)npairs * kTrimList) || !ensure<unsigned>(d_trim_ctr_, 4 * (size_t)npairs) ||
        !ensure<unsigned>(d_trim_hist_, 4096 * (size_t)npairs) ||
        !ensure<double>(d_red_partial_, (size_t)nwork_ * kRedVals) || !ensure<double>(d_red_out_, (size_t)npairs * kRedVals) ||
        !ensure<int32_t>(d_rechecked_, npairs))
        return SE3ICP_ERR_OUT_OF_MEMORY;
    if (h_pairs_.reserve(npairs) || h_red_.reserve((size_t)npairs * kRedVals) || h_rechecked_.reserve(npairs))
        return SE3ICP_ERR_OUT_OF_MEMORY;
    HIPCHK(hipMemcpyAsync(d_work_.p, h_work_.data(), sizeof(BlockWork) * nwork_, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_wb_.p, h_wb_.data(), sizeof(int32_t) * npairs, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_wn_.p, h_wn_.data(), sizeof(int32_t) * npairs, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_rechecked_.p, 0, sizeof(int32_t) * npairs, s));
    return 0;
}

// Loop state, loop and results of the pairs of the batch that was set up (see engine.hpp).
int Engine::run_loop(int npairs, const int64_t* ns, int kind, int est, const se3icp_params* vprm,
                     int pairs_per_variant, bool sweep, se3icp_trace* tr, se3icp_result* out, hipStream_t s,
                     const ReportReq* rq) {
    const MethodInfo mi{(Kind)kind, est};
    const bool se3 = mi.kind != KIND_ICP;
    int rc = 0;

    // ---- per-pair loop state (ISR.cpp:629-651); iteration 1 is opened here, every later
    // one by k_reduce_final on the device (pairmath.hpp), so the host only queues work
    if (!ensure<PairState>(d_state_, npairs) || h_state_.reserve(npairs))
        return SE3ICP_ERR_OUT_OF_MEMORY;
    if (h_phase_cap_ < (size_t)npairs * kLoopRing) {  // coherent host memory the device writes directly
        if (h_phase_) (void)hipHostFree(h_phase_);
        h_phase_ = nullptr;
        h_phase_cap_ = 0;
        const size_t want = std::max<size_t>((size_t)npairs * kLoopRing, 64);
        if (hipHostMalloc((void**)&h_phase_, want * sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent) !=
                hipSuccess ||
            hipHostGetDevicePointer((void**)&d_phase_, h_phase_, 0) != hipSuccess)
            return SE3ICP_ERR_OUT_OF_MEMORY;
        h_phase_cap_ = want;
    }
    // what the host's queueing decisions read of the parameters, over all variants: SE(3)
    // grids are queued up to the largest max_num_se3_iterations (without bound if any variant
    // has none, "< 1"); they only decide which grids are queued, a pair's own limits are in
    // its PairState
    int se3_limit = 0;
    for (int k = 0; k * pairs_per_variant < npairs; ++k) {
        const int m = vprm[k].max_num_se3_iterations;
        se3_limit = (m < 1 || se3_limit < 0) ? -1 : std::max(se3_limit, m);
    }
    int n_se3 = 0, n_r3 = 0;
    bool any_trim = false;
    for (int p = 0; p < npairs; ++p) {
        const se3icp_params& prm = vprm[p / pairs_per_variant];
        const float ratio = std::min(1.0f, std::max(0.0f, (float)prm.estimated_overlap));  // PCL setOverlapRatio(float)
        PairState& S = h_state_[p];
        std::memset(&S, 0, sizeof(S));
        S.T = M4::eye();
        S.mse_prev = S.mse_cur = S.rel = 1e7;
        S.sf = 1.0;  // run_se3_*: the device's scale, written by k_pair_norms
        S.mse = prm.mse;
        S.mse_switch = prm.mse_switch_error;
        S.kind = mi.kind;
        S.max_iter = prm.max_num_iterations;
        S.max_se3 = prm.max_num_se3_iterations;
        S.phase = PHASE_IDLE;
        S.phase_start = 1;
        const unsigned nv = (unsigned)std::floor(ratio * (float)ns[p]);
        const bool trim = (int64_t)nv < ns[p];
        S.K = trim ? (double)nv : (double)ns[p];
        PairDev& P = h_pairs_[p];
        std::memset(&P, 0, sizeof(P));
        P.src = 2 * p;
        P.tgt = 2 * p + 1;
        P.est = mi.est;
        P.cf = mi.kind == KIND_CF;
        P.trim = trim;
        P.nkeep = (int)nv;
        for (int a = 0; a < 3; ++a) P.f32_center[a] = h_setup_[2 * p].f32_center[a];
        pair_open_iteration(S, P);
        std::memcpy(h_hist_ + 12 * (size_t)p, P.T, sizeof(P.T));
        n_se3 += P.phase == PHASE_SE3;
        n_r3 += P.phase == PHASE_R3;
        any_trim |= trim;
    }
    HIPCHK(hipMemcpyAsync(d_pairs_.p, h_pairs_, sizeof(PairDev) * npairs, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_state_.p, h_state_, sizeof(PairState) * npairs, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync((double*)d_hist_.p + (size_t)(1 % kHist) * npairs * 12, h_hist_, sizeof(double) * 12 * npairs,
                          hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_flag_count_.p, 0, 3 * sizeof(int32_t), s));
    // norm bounds of the target search vectors (f32 error certificate) from the root
    // boxes, and the normalization scales into the loop state
    launch_pair_norms(view(), 2 << t3_.L, se3 ? 2 << t12_.L : 0, se3 ? (const double*)d_scales_.p : nullptr,
                      (double*)((char*)d_state_.p + offsetof(PairState, sf)), (int)(sizeof(PairState) / sizeof(double)),
                      s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync((uint64_t*)d_trim_key_.p + npairs, 0, sizeof(uint64_t) * npairs, s));  // no trim window yet
    HIPCHK(hipMemsetAsync(d_trim_ctr_.p, 0, sizeof(unsigned) * 4 * npairs, s));
    launch_geo_rows(view(), s);  // (after the setup's normals and confidences)
    HIPCHK(hipMemsetAsync(d_trim_hist_.p, 0, sizeof(unsigned) * 4096 * npairs, s));
    View v = view();
    double nn_ms = 0;
    // Iteration `it` is queued while iteration it-1 still runs; the host then waits for
    // it-1 and reads how many pairs iteration it has (counted by it-1's k_reduce_final).
    // Zero means iteration `it` is empty and the loop is over.  NN grids of a phase are
    // queued while any pair may be in it: SE(3) until a finished iteration shows none
    // left, R3 from iteration 2 on (a pair may switch after any iteration).
    // SE3ICP_NN_TRACE waits for every iteration (per-iteration work counters).
    const int lag = (nn_trace_ || tr) ? 0 : 1;
    int trace_phase = tr ? h_pairs_[tr->pair].phase : 0;  // phase of the iteration being recorded
    auto enqueue = [&](int it) -> int {
        hipEvent_t* ev = &loop_ev_[(it % kLoopRing) * kLoopEv];
        // the ring slot k_reduce_final of this iteration fills (its last reader, iteration
        // it - kLoopRing, is finished): unwritten until then (spin_phases)
        for (int p = 0; p < npairs; ++p) h_phase_[(size_t)(it % kLoopRing) * npairs + p] = -1;
        // SE(3) phase: iterations 1..max_num_se3_iterations at most (ISR.cpp:718-723, 1118)
        const bool do_se3 =
            n_se3 > 0 && (se3_limit < 1 || it <= se3_limit);
        const bool do_r3 = n_r3 > 0 || (mi.kind != KIND_ICP && mi.kind != KIND_PURE && it >= 2);
        // HIP events around the NN grids always (bench.py's roofline); around every other
        // stage only when profiling (each marker costs the stream a few microseconds)
        const bool detail = profile_ || nn_trace_;
        // (timed steps: the SE(3) NN bracket only when that grid is queued, plus the
        // iteration's end marker; profiled steps: every stage)
        const bool t_se3 = detail || (do_se3 && nn_events_);
        if (detail) HIPCHK(hipEventRecord(ev[0], s));
        // the phases of iteration it (opened by it-1's k_reduce_final) reach the host through
        // this k_nn_prep (ring slot it-1); without look-ahead, k_reduce_final writes them
        launch_nn_prep(v, (lag == 1 && it >= 2) ? d_phase_ + (size_t)((it - 1) % kLoopRing) * npairs : nullptr, s);
        // One search grid per phase (single-query waves and groups together, k_nn.hip): no
        // second stream and no cross-stream events.  ev[1] / ev[2] bracket the SE(3) search.
        if (t_se3) HIPCHK(hipEventRecord(ev[1], s));
        if (do_se3) launch_nn(v, 12, s);
        if (t_se3) HIPCHK(hipEventRecord(ev[2], s));
        if (do_r3) launch_nn(v, 3, s);
        if (detail) HIPCHK(hipEventRecord(ev[3], s));
        // (no recheck stage: the NN grids re-resolve their uncertified queries inline; the
        // ev[3] -> ev[4] bracket stays empty and time_recheck reads ~0)
        if (detail) HIPCHK(hipEventRecord(ev[4], s));
        if (any_trim) launch_trim(v, s);
        if (detail) HIPCHK(hipEventRecord(ev[5], s));
        launch_reduce(v, (const int32_t*)d_wb_.p, (const int32_t*)d_wn_.p, (PairState*)d_state_.p, (double*)d_hist_.p,
                      lag == 0 ? d_phase_ + (size_t)(it % kLoopRing) * npairs : nullptr, s);
        HIPCHK(hipGetLastError());
        if (detail) HIPCHK(hipEventRecord(ev[6], s));
        loop_detail_[it % kLoopRing] = detail;
        loop_flags_[it % kLoopRing] = (do_se3 ? 1 : 0) | (do_r3 ? 2 : 0) | (t_se3 ? 4 : 0);
        return 0;
    };
    // wait for iteration `it`, add its kernel times; returns the pairs of iteration it+1
    // (last: the loop's final, empty, iteration -- no k_nn_prep follows to publish its slot)
    auto finish = [&](int it, bool last) -> int {
        hipEvent_t* ev = &loop_ev_[(it % kLoopRing) * kLoopEv];
        // (the phase slot of iteration it is written by the next iteration's k_nn_prep, queued
        // already, or with lag 0 by this iteration's k_reduce_final -- after its end event)
        if (loop_detail_[it % kLoopRing]) HIPCHK(spin_wait(ev[6]));
        if (last && lag == 1) {
            if (!loop_detail_[it % kLoopRing]) {
                HIPCHK(hipEventRecord(ev_[EV_SYNC], s));
                HIPCHK(spin_wait(ev_[EV_SYNC]));
            }
        } else {
            HIPCHK(spin_phases(h_phase_ + (size_t)(it % kLoopRing) * npairs, npairs, s));
        }
        float ms[6] = {};
        if (loop_detail_[it % kLoopRing]) {
            for (int k = 0; k < 6; ++k) HIPCHK(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
        } else if (loop_flags_[it % kLoopRing] & 4) {
            HIPCHK(hipEventElapsedTime(&ms[1], ev[1], ev[2]));
        }
        ktimes_.nn_prep_ms += ms[0];
        ktimes_.nn_se3_ms += ms[1];
        ktimes_.nn_r3_ms += ms[2];
        ktimes_.recheck_ms += ms[3];
        ktimes_.trim_ms += ms[4];
        ktimes_.reduce_ms += ms[5];
        nn_ms += ms[0] + ms[1] + ms[2] + ms[3];
        const int flags = loop_flags_[it % kLoopRing];
        if (flags & 1) ktimes_.nn_se3_launches++;
        if (flags & 2) ktimes_.nn_r3_launches++;
        if (nn_trace_) {  // per-iteration NN work (diagnostics): diffs of the device counters
            unsigned long long stats[kStatCols * kStatSlots];
            HIPCHK(hipMemcpy(stats, d_stats_.p, sizeof(stats), hipMemcpyDeviceToHost));
            double sum[kStatCols] = {};
            for (int i = 0; i < kStatSlots; ++i)
                for (int k = 0; k < kStatCols; ++k) sum[k] += (double)stats[kStatCols * i + k];
            std::fprintf(stderr,
                         "[nn] iter %d: se3 %.0f/%.0f searched, evals %.3g boxes %.3g | r3 %.0f/%.0f, evals %.3g "
                         "boxes %.3g | prep %.3f nn12 %.3f nn3 %.3f recheck %.3f ms\n",
                         it, sum[5] - trace_prev_[5], sum[4] - trace_prev_[4], sum[0] - trace_prev_[0],
                         sum[1] - trace_prev_[1], sum[7] - trace_prev_[7], sum[6] - trace_prev_[6],
                         sum[2] - trace_prev_[2], sum[3] - trace_prev_[3], ms[0], ms[1], ms[2], ms[3]);
#ifdef SE3ICP_PROF
            {
                // this iteration's SE(3) group waves: count and summed duration (column 11:
                // (1 << 44) + dt per wave, 100 MHz clock), shader cycles in leaf visits (12),
                // in their target loads (14) and in the whole wave (13)
                double d[kStatCols];
                for (int k = 0; k < kStatCols; ++k) d[k] = sum[k] - trace_prev_[k];
                const double nw = std::floor(d[11] / 17592186044416.0), dt = d[11] - nw * 17592186044416.0;
                std::fprintf(stderr, "[nn] iter %d: %.0f SE(3) group waves, mean %.1f us, summed %.1f ms (100 MHz clock)\n",
                             it, nw, nw > 0 ? dt / nw / 100.0 : 0.0, dt / 1e5);
                std::fprintf(stderr, "[nn] iter %d: k_nn_prep span %.1f us\n", it, nn_prep_span());
                nn_wave_report(it);
                std::fprintf(stderr, "[nn] iter %d: wave cycles in leaf visits %.1f %% (target loads %.1f %%), "
                             "%.0f cycles per leaf visit, %.0f per box-test step\n", it, 100.0 * d[12] / std::max(1.0, d[13]),
                             100.0 * d[14] / std::max(1.0, d[13]), d[12] / std::max(1.0, d[9]),
                             (d[13] - d[12]) / std::max(1.0, d[1] / 128.0));
            }
#endif
            for (int k = 0; k < kStatCols; ++k) trace_prev_[k] = sum[k];
#ifdef SE3ICP_PROF
            std::fprintf(stderr, "[nn] iter %d: longest SE(3) group wave %.1f us (%llu box-test steps, %llu leaf visits, "
                         "%llu queries)\n", it, (double)(stats[10] >> 40) / 100.0, (stats[10] >> 20) & 0xfffffull,
                         (stats[10] >> 6) & 0x3fffull, stats[10] & 63ull);
            HIPCHK(hipMemset((unsigned long long*)d_stats_.p + 10, 0, sizeof(unsigned long long)));
#endif
        }
        if (last && lag == 1) return 0;
        const volatile int32_t* ph = h_phase_ + (size_t)(it % kLoopRing) * npairs;
        n_se3 = n_r3 = 0;
        for (int p = 0; p < npairs; ++p) {
            const int32_t f = ph[p];
            n_se3 += f == PHASE_SE3;
            n_r3 += f == PHASE_R3;
        }
        return n_se3 + n_r3;
    };
    static_assert(kLoopRing >= 2, "one iteration in flight while the previous one is read");
    int it = 1;
    if (enqueue(it)) return SE3ICP_ERR_HIP;
    for (;;) {
        if (lag == 0) {
            const int left = finish(it, false);
            if (tr) {
                rc = record_trace(tr, it, trace_phase, s);
                if (rc) return rc;
            }
            if (left == 0) break;
            ++it;
            if (enqueue(it)) return SE3ICP_ERR_HIP;
            continue;
        }
        ++it;
        if (enqueue(it)) return SE3ICP_ERR_HIP;  // phase flags as of iteration it-2
        if (finish(it - 1, false) == 0) {        // iteration `it` is empty
            (void)finish(it, true);
            break;
        }
    }
    HIPCHK(hipEventRecord(ev_[EV_LOOP_DONE], s));
    HIPCHK(hipMemcpyAsync(h_state_, d_state_.p, sizeof(PairState) * npairs, hipMemcpyDeviceToHost, s));
    // the device's GetCenter results, for the de-normalization (h_partial_ holds >= 9 * nclouds);
    // replicas of a sweep group share their base clouds' centers
    const int nbase = 2 * pairs_per_variant;
    if (se3) HIPCHK(hipMemcpyAsync(h_partial_, d_centers_.p, sizeof(double) * 3 * nbase, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_rechecked_, d_rechecked_.p, sizeof(int32_t) * npairs, hipMemcpyDeviceToHost, s));
    {
        if (h_loop_stats_.reserve((size_t)kStatCols * kStatSlots)) return SE3ICP_ERR_OUT_OF_MEMORY;
        const unsigned long long* stats = h_loop_stats_;
        HIPCHK(hipMemcpyAsync(h_loop_stats_, d_stats_.p, sizeof(unsigned long long) * kStatCols * kStatSlots,
                              hipMemcpyDeviceToHost, s));
        // the report stage, behind the loop's end event and every copy of the loop's results:
        // what it adds to the counters and rewrites of PairDev is read by nobody
        if (rq) {
            rc = queue_report(npairs, ns, *rq, s);
            if (rc) return rc;
        }
        SYNC_STREAM(s);
        double sum[kStatCols] = {};
        for (int i = 0; i < kStatSlots; ++i)
            for (int k = 0; k < kStatCols; ++k) sum[k] += (double)stats[kStatCols * i + k];
        ktimes_.se3_dist_evals += sum[0];
        ktimes_.se3_box_tests += sum[1];
        ktimes_.r3_dist_evals += sum[2];
        ktimes_.r3_box_tests += sum[3];
        ktimes_.se3_queries += sum[4];
        ktimes_.se3_searched += sum[5];
        ktimes_.r3_queries += sum[6];
        ktimes_.r3_searched += sum[7];
        ktimes_.se3_useful_evals += sum[kStatUseSe3];
        ktimes_.r3_useful_evals += sum[kStatUseR3];
#ifdef SE3ICP_PROF
        {
            const double nw = std::max(1.0, std::floor(sum[11] / 17592186044416.0));
            const double mean = std::fmod(sum[11], 17592186044416.0) / nw;  // 100 MHz ticks
            const double sq = (double)stats[kStatCols + 10] / nw;
            nn_prof_report();
            trim_prof_report();
            std::fprintf(stderr, "[prof] nn12: leaf visits %.0f; %.0f group waves, %.1f us each on average (sd %.1f, "
                         "longest %.1f us; 100 MHz clock)\n",
                         sum[9], nw, mean / 100.0, std::sqrt(std::max(0.0, sq - mean * mean)) / 100.0,
                         (double)(stats[10] >> 40) / 100.0);
            std::fprintf(stderr, "[prof] nn12 longest wave: %llu box-test steps, %llu leaf visits, %llu queries\n",
                         (stats[10] >> 20) & 0xfffffull, (stats[10] >> 6) & 0x3fffull, stats[10] & 63ull);
        }
#endif
    }
    float setup_ms = 0, loop_ms = 0;
    if (sweep) {
        float shared_ms = 0, group_ms = 0;
        HIPCHK(hipEventElapsedTime(&shared_ms, ev_[EV_CALL_BEGIN], ev_[EV_SHARED_DONE]));
        HIPCHK(hipEventElapsedTime(&group_ms, ev_[EV_GROUP_BEGIN], ev_[EV_SETUP_DONE]));
        setup_ms = shared_ms + group_ms;
        ktimes_.setup_ms = shared_ms;
    } else {
        HIPCHK(hipEventElapsedTime(&setup_ms, ev_[EV_CALL_BEGIN], ev_[EV_SETUP_DONE]));
        ktimes_.setup_ms = setup_ms;
    }
    HIPCHK(hipEventElapsedTime(&loop_ms, ev_[EV_SETUP_DONE], ev_[EV_LOOP_DONE]));

    int worst = 0;
    for (int p = 0; p < npairs; ++p) {
        const PairState& S = h_state_[p];
        M4 T = S.T;
        const int bp = p % pairs_per_variant;  // (a replica takes its base pair's centers)
        if (rq) {
            se3icp_report& Q = rq->out[p];
            std::memset(&Q, 0, sizeof(Q));
            const double origin[3] = {0.0, 0.0, 0.0};
            report_expand(h_rep_ + (size_t)kRepVals * p, S.sf, h_pairs_[p].f32_center,
                          se3 ? &h_partial_[3 * (2 * bp + 1)] : origin, ns[p], &Q);
            Q.final_mse = S.mse_cur;
            Q.final_mse_change = S.rel;
            Q.switched = S.sw;
            Q.stop_reason = report_stop_reason(S);
        }
        if (se3) {  // ISR.cpp:735-738 de-normalization
            const double* cs = &h_partial_[3 * (2 * bp)];
            const double* ct = &h_partial_[3 * (2 * bp + 1)];
            for (int r = 0; r < 3; ++r) {
                const double Rc = T.m[r][0] * cs[0] + T.m[r][1] * cs[1] + T.m[r][2] * cs[2];
                T.m[r][3] = (1.0 / S.sf) * T.m[r][3] - Rc + ct[r];
            }
        }
        se3icp_result& R = out[p];
        std::memset(&R, 0, sizeof(R));
        bool finite = true;
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                R.T[i * 4 + j] = T.m[i][j];
                finite &= std::isfinite(T.m[i][j]);
            }
        R.num_iterations = S.iter;
        R.num_pure_se3_iterations = se3 ? S.pure : -1;
        R.status = finite ? SE3ICP_OK : SE3ICP_ERR_NONFINITE;
        R.num_rechecked = h_rechecked_[p];
        R.scaling_factor = S.sf;
        R.time_setup_ms = setup_ms;
        R.time_loop_ms = loop_ms;
        R.time_se3_correspondence_search_ms = nn_ms;
        R.time_before_pure_icp_ms = mi.kind == KIND_CF ? (double)setup_ms + (double)loop_ms : 0.0;
        if (R.status != SE3ICP_OK) worst = R.status;
    }
    return worst;
}

// The report stage of the batch the loop just ran (report.hpp, k_report.hip), queued on the
// call's stream; run_loop's synchronisation follows.  Everything the loop's results are read
// from has been copied by then; the stage rewrites PairDev (phase, pose, iteration) and runs
// the loop's own R3 search once more, for every pair at once, at the final poses.
int Engine::queue_report(int npairs, const int64_t* ns, const ReportReq& rq, hipStream_t s) {
    const se3icp_report_options& o = *rq.opts;
    if (!ensure<double>(d_rep_partial_, (size_t)nwork_ * kRepVals) || !ensure<double>(d_rep_out_, (size_t)npairs * kRepVals) ||
        h_rep_.reserve((size_t)npairs * kRepVals))
        return SE3ICP_ERR_OUT_OF_MEMORY;
    ReportArgs a{};
    a.state = (const PairState*)d_state_.p;
    a.hist = (double*)d_hist_.p;
    a.max_d = o.max_correspondence_distance;
    a.all_inliers = report_all_inliers(o.max_correspondence_distance) ? 1 : 0;
    a.partial = (double*)d_rep_partial_.p;
    a.out = (double*)d_rep_out_.p;
    a.pair_wb = (const int32_t*)d_wb_.p;
    a.pair_wn = (const int32_t*)d_wn_.p;
    int64_t total = 0;
    if (o.corr_idx || o.corr_dist) {  // compact per pair: pair p at the prefix sum of n_src
        h_rep_off_.resize(npairs);
        for (int p = 0; p < npairs; ++p) {
            h_rep_off_[p] = total;
            total += ns[p];
        }
        if (!ensure<int64_t>(d_rep_off_, npairs)) return SE3ICP_ERR_OUT_OF_MEMORY;
        HIPCHK(hipMemcpyAsync(d_rep_off_.p, h_rep_off_.data(), sizeof(int64_t) * npairs, hipMemcpyHostToDevice, s));
        a.out_off = (const int64_t*)d_rep_off_.p;
        if (o.outputs_on_device) {
            a.out_idx = o.corr_idx;
            a.out_dist = o.corr_dist;
        } else {
            if ((o.corr_idx && !ensure<int32_t>(d_rep_idx_, (size_t)total)) ||
                (o.corr_dist && !ensure<double>(d_rep_dist_, (size_t)total)))
                return SE3ICP_ERR_OUT_OF_MEMORY;
            a.out_idx = o.corr_idx ? (int32_t*)d_rep_idx_.p : nullptr;
            a.out_dist = o.corr_dist ? (double*)d_rep_dist_.p : nullptr;
        }
    }
    // what k_reduce_final clears for the next k_nn_prep (the single-query lists' counts and
    // the searches' cost-class counts): the loop's last k_reduce_final did, cleared here too
    HIPCHK(hipMemsetAsync(d_flag_count_.p, 0, 3 * sizeof(int32_t), s));
    HIPCHK(hipMemsetAsync(d_cls_.p, 0, sizeof(int32_t) * 2 * 8 * 16, s));
    const View v = view();
    launch_report_open(v, a, s);
    launch_nn_prep(v, nullptr, s);
    launch_nn(v, 3, s);
    launch_report(v, a, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_rep_, d_rep_out_.p, sizeof(double) * kRepVals * npairs, hipMemcpyDeviceToHost, s));
    if (!o.outputs_on_device) {
        if (o.corr_idx)
            HIPCHK(hipMemcpyAsync(o.corr_idx, d_rep_idx_.p, sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, s));
        if (o.corr_dist)
            HIPCHK(hipMemcpyAsync(o.corr_dist, d_rep_dist_.p, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, s));
    }
    return 0;
}

// ----------------------------------------------------------------------------- parameter sweep
// One shared setup over the base clouds with alpha = beta = 1 (the stored rows are the raw
// frame and the raw normalized point: 1.0 * x is exact), then the variants in groups: each
// group is a batch of g * P virtual pairs -- the base slots are its first variant, replicas
// 1 .. g-1 follow at point offset v * N -- expanded and weighted by k_sweep_expand, given
// its 12-D trees and run through the loop.  A pair registers bitwise the same in any batch,
// so every result equals that of register_batch with its variant.
int Engine::register_sweep(int P, const double* const* src, const int64_t* ns, const double* const* tgt,
                           const int64_t* nt, bool on_device, int method, int nvariants,
                           const se3icp_params* variants, int max_group, se3icp_result* out, hipStream_t user_stream,
                           const se3icp_report_options* ropts, se3icp_report* reports) {
    const int args = (P <= 0 || !src || !tgt || !ns || !nt || !out || nvariants <= 0 || !variants || max_group < 0)
                         ? SE3ICP_ERR_INVALID_ARG : 0;
    MethodPlan mp{};
    int rest = args ? 0 : plan_pairs(method, variants[0].number_of_nn_for_LRF, P, src, ns, tgt, nt, &mp);
    for (int k = 1; !args && !rest && k < nvariants; ++k)  // what shapes the shared setup is common to all variants
        if (variants[k].number_of_nn_for_LRF != variants[0].number_of_nn_for_LRF ||
            variants[k].scale_preprocessing != variants[0].scale_preprocessing)
            rest = SE3ICP_ERR_INVALID_ARG;
    Call call;
    int rc = open_call(args, (int64_t)nvariants * P, rest, user_stream, &call);
    if (rc) return rc;
    hipStream_t s = call.s;
    const bool se3 = mp.se3;
    const se3icp_params& prm0 = variants[0];

    int64_t N = 0;
    int max_n = 1;
    for (int p = 0; p < P; ++p) {
        N += ns[p] + nt[p];
        max_n = (int)std::max<int64_t>(max_n, std::max(ns[p], nt[p]));
    }
    const int nbase = 2 * P;
    // group size: what the caller allows, the point limit of a batch and the memory hold
    // (free memory plus the buffers this engine would reuse)
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    int64_t held = 0;
    for (const DevBuf* b : bufs_) held += (int64_t)b->bytes;
    const int G = sweep_group_size(nvariants, max_group, N, nbase, kSweepBytesPerPoint, kSweepBytesPerCloud,
                                   (int64_t)free_b + held);
    const int ngroups = sweep_num_groups(nvariants, G);

    // buffers of the largest group, before the shared setup fills them (ensure() does not
    // keep a buffer's contents when it grows)
    rc = alloc_points((int64_t)G * N, mp.kmax);
    if (rc) return rc;
    const int nnodes3 = 2 << tree_depth_for(max_n);
    const size_t nbox = (size_t)G * nbase * nnodes3 * 3;
    if (!ensure<CloudDev>(d_clouds_, (size_t)G * nbase) || !ensure<CloudSetup>(d_setup_, (size_t)G * nbase) ||
        !ensure<float>(t3_.lo, nbox) || !ensure<float>(t3_.hi, nbox) || !ensure<double>(d_scales_, (size_t)G * P) ||
        !ensure<SweepWeight>(d_sweep_w_, G) || (se3 && !ensure<double>(d_raw_, 12 * (size_t)N)))
        return SE3ICP_ERR_OUT_OF_MEMORY;

    // ---- shared setup (ISR.cpp:568-648) of the base clouds
    npairs_ = P;
    ntot_ = N;  // (ld_ stays the group's: the SoA columns keep one stride through the sweep)
    // (alpha = beta = 1: the rows are weighted, and a cf target's f32 rows formed, per variant)
    std::vector<CloudReq> clouds(nbase);
    for (int p = 0; p < P; ++p)
        for (int side = 0; side < 2; ++side)
            clouds[2 * p + side] = CloudReq{side == 0 ? src[p] : tgt[p], side == 0 ? ns[p] : nt[p],
                                            cloud_setup(mp, side, 1.0, 1.0, false)};
    rc = setup_clouds(clouds, on_device, true, se3, prm0.scale_preprocessing, s);
    if (rc) return rc;
    if (se3)
        HIPCHK(hipMemcpyAsync(d_raw_.p, d_fr64_.p, sizeof(double) * 12 * (size_t)N, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipEventRecord(ev_[EV_SHARED_DONE], s));
    const std::vector<CloudDev> base_clouds = h_clouds_;
    const std::vector<CloudSetup> base_setup = h_setup_;

    std::vector<int64_t> vns((size_t)G * P), vnt((size_t)G * P);
    for (int q = 0; q < G * P; ++q) {
        vns[q] = ns[q % P];
        vnt[q] = nt[q % P];
    }
    std::vector<std::vector<SweepWeight>> weights(ngroups);  // (alive until the copies have run)
    int worst = 0;
    for (int gi = 0; gi < ngroups; ++gi) {
        int v0 = 0, g = 0;
        sweep_group(nvariants, G, gi, &v0, &g);
        HIPCHK(hipEventRecord(ev_[EV_GROUP_BEGIN], s));
        // ---- the group's batch: g * P virtual pairs over g * 2P virtual clouds
        nclouds_ = g * nbase;
        npairs_ = g * P;
        ntot_ = (int64_t)g * N;
        h_clouds_.resize(nclouds_);
        h_setup_.resize(nclouds_);
        std::vector<SweepWeight>& w = weights[gi];
        w.resize(g);
        for (int k = 0; k < g; ++k) {
            w[k] = SweepWeight{variants[v0 + k].alpha_rot, variants[v0 + k].beta_transl};
            for (int c = 0; c < nbase; ++c) {
                h_clouds_[k * nbase + c] = CloudDev{(int32_t)(base_clouds[c].off + (int64_t)k * N), base_clouds[c].n};
                CloudSetup st = base_setup[c];
                st.alpha = w[k].alpha;
                st.beta = w[k].beta;
                st.cf_target = (mp.kind == KIND_CF && st.is_target) ? 1 : 0;
                h_setup_[k * nbase + c] = st;  // (host mirror; the device's is written by k_sweep_expand)
            }
        }
        HIPCHK(hipMemcpyAsync(d_sweep_w_.p, w.data(), sizeof(SweepWeight) * g, hipMemcpyHostToDevice, s));
        SweepArgs a{};
        a.g = g;
        a.n = (int32_t)N;
        a.nclouds = nbase;
        a.nnodes3 = nnodes3;
        a.frames = se3 ? 1 : 0;
        a.cf = mp.kind == KIND_CF ? 1 : 0;
        a.raw = (const double*)d_raw_.p;
        a.w = (const SweepWeight*)d_sweep_w_.p;
        a.scales = se3 ? (double*)d_scales_.p : nullptr;
        a.tpt64 = (double4*)t3_.vec64a.p;
        a.perm3 = (int32_t*)t3_.perm.p;
        a.pos3 = (int32_t*)t3_.pos.p;
        a.tvec3 = (float*)t3_.vec.p;
        a.tvec64_3 = (double*)t3_.vec64.p;
        a.lo3 = (float*)t3_.lo.p;
        a.hi3 = (float*)t3_.hi.p;
        launch_sweep_expand(view(), a, s);
        HIPCHK(hipGetLastError());
        // the armed records whose pair is in this group; the tree record's replicas: their 3-D
        // trees are copies of their base clouds'
        se3icp_trace gtr{};
        const Call gcall = group_call(call, v0, g, P, &gtr);
        if (gcall.tk) {
            tree_log_[0].resize(nclouds_);
            for (int c = nbase; c < nclouds_; ++c) tree_log_[0][c] = tree_log_[0][c % nbase];
        }
        rc = run_pairs(mp, g * P, vns.data(), vnt.data(), variants + v0, P, true, gcall, out + (size_t)v0 * P,
                       ropts, reports ? reports + (size_t)v0 * P : nullptr);
        if (gcall.tr) call.tr->iters_recorded = gtr.iters_recorded;
        if (rc && rc != SE3ICP_ERR_NONFINITE) return rc;
        if (rc) worst = rc;
    }
    // (ktimes_: the setup entries are the shared setup's, read at the first group's
    // synchronisation; the loop entries were summed over the groups)
    return worst;
}

// ----------------------------------------------------------------------------- cloud graphs
// P edges over C distinct clouds (graph.hpp).  Two layouts follow one another in the same
// buffers, both with the column stride of the larger (the 2P uses):
//   A  the distinct clouds some edge uses: one upload, k_ingest, centroid, radius each; the
//      centroids and radii go to the host (ONE extra synchronisation against a plain batch,
//      whose normalization parameters never leave the device), which plans the classes;
//   B  the 2P uses, as a batch lays them out: k_graph_normalize from A's raw columns and a 3-D
//      tree for every use; kNN / frames / normals only for the first use of every class (the
//      other uses ask for no neighbours, which the kernels skip); k_graph_share copies those
//      to the class's other uses; then run_pairs, as a batch.
// A's raw columns are kept by swapping their buffer out for B's (memory is not saved: every
// use is materialised, the loop's state lives at a use's slots).  A cloud sets up bitwise the
// same at any position of any batch, so every result equals register_batch's for the expanded
// pair list.
int Engine::register_graph(int C, const double* const* xyz, const int64_t* npts, int P, const int32_t* esrc,
                           const int32_t* etgt, bool on_device, int method, const se3icp_params& prm, int sharing,
                           se3icp_result* out, hipStream_t user_stream, const se3icp_report_options* ropts,
                           se3icp_report* reports, const double* T_init) {
    // ---- layouts A (used clouds, in cloud order) and B (uses)
    const int args = (C <= 0 || P <= 0 || !xyz || !npts || !esrc || !etgt || !out) ? SE3ICP_ERR_INVALID_ARG : 0;
    MethodPlan mp{};
    std::vector<int32_t> slotA, cloudA;
    int rest = args ? 0 : plan_method(method, prm.number_of_nn_for_LRF, &mp);
    // Initial poses: the call is planned over VARIANTS (graph.hpp) instead of clouds.  C, xyz, npts,
    // esrc and etgt are rebound to the variants' -- numbered by first use -- and layout A becomes
    // "every used variant once"; everything below reads them as it reads clouds.  Without a posed
    // edge (T_init null, or every pose bitwise the identity) nothing is rebound: the plain call.
    VariantPlan vplan;
    std::vector<const double*> vxyz;
    std::vector<int64_t> vnpts;
    const int rawC = C;
    const double* const* rawxyz = xyz;
    const int64_t* rawnpts = npts;
    if (!args && !rest && T_init) {
        std::vector<int32_t> slotR, cloudR;  // (the clouds' own checks, before anything is rebound)
        rest = graph_used_clouds(C, xyz, npts, P, esrc, etgt, &slotR, &cloudR);
        if (!rest) graph_plan_variants(P, esrc, etgt, T_init, &vplan);
    }
    const bool posed = vplan.posed_edges > 0;
    if (posed) {
        C = (int)vplan.cloud.size();
        vxyz.resize(C);
        vnpts.resize(C);
        for (int v = 0; v < C; ++v) {
            vxyz[v] = rawxyz[vplan.cloud[v]];
            vnpts[v] = rawnpts[vplan.cloud[v]];
        }
        xyz = vxyz.data();
        npts = vnpts.data();
        esrc = vplan.edge_src.data();
        etgt = vplan.edge_tgt.data();
    }
    if (!args && !rest) rest = graph_used_clouds(C, xyz, npts, P, esrc, etgt, &slotA, &cloudA);
    Call call;
    int rc = open_call(args, P, rest, user_stream, &call);
    if (rc) return rc;
    for (int64_t& g : init_stats_) g = 0;
    hipStream_t s = call.s;
    const bool se3 = mp.se3;
    if (sharing == 0) sharing = 3;
    // (level 3, neighbour-set adoption between the classes of a cloud, is not built: as 2)
    for (int64_t& g : graph_stats_) g = 0;
    const int CA = (int)cloudA.size();
    std::vector<int64_t> ns(P), nt(P);
    int64_t NA = 0, NU = 0;
    int nchU = 0;
    for (int a = 0; a < CA; ++a) NA += npts[cloudA[a]];
    for (int p = 0; p < P; ++p) {
        ns[p] = npts[esrc[p]];
        nt[p] = npts[etgt[p]];
        NU += ns[p] + nt[p];
        nchU += (int)((ns[p] + kChunk - 1) / kChunk + (nt[p] + kChunk - 1) / kChunk);
    }

    // buffers of the larger layout first (NA <= NU points, and as many chunks at most)
    rc = alloc_points(NU, mp.kmax);
    if (rc) return rc;
    const size_t L = (size_t)ld_;
    if (!ensure<CloudDev>(d_clouds_, 2 * (size_t)P) || !ensure<CloudSetup>(d_setup_, 2 * (size_t)P) ||
        !ensure<ChunkWork>(d_chunks_, nchU) || !ensure<const double*>(d_inptr_, CA) ||
        !ensure<double>(d_partial_, (size_t)nchU * 9) || !ensure<double>(d_centers_, 6 * (size_t)P) ||
        !ensure<double>(d_scales_, P) || !ensure<GraphSeg>(g_seg_, 2 * (size_t)P))
        return SE3ICP_ERR_OUT_OF_MEMORY;
    if (h_partial_.reserve((size_t)nchU * 9 + 6 * (size_t)P + 8)) return SE3ICP_ERR_OUT_OF_MEMORY;

    // ---- A: every used cloud once
    npairs_ = 0;
    ntot_ = NA;
    std::vector<CloudReq> reqA(CA);
    for (int a = 0; a < CA; ++a) {
        reqA[a] = CloudReq{xyz[cloudA[a]], npts[cloudA[a]], CloudSetup{}};
        reqA[a].st.want_conf = mp.kind == KIND_CF;
        reqA[a].st.alpha = reqA[a].st.beta = reqA[a].st.norm_scale = 1.0;
        if (!on_device) graph_stats_[GS_BYTES_UPLOADED] += (int64_t)sizeof(double) * 3 * reqA[a].n;
    }
    int rawCA = CA;  // the distinct raw clouds among A's slots
    if (posed) {
        // every raw cloud is uploaded once, however many variants it has: the variants' inputs point
        // at their cloud's one copy (d_in_ has room for NU >= the raw clouds' points)
        std::vector<const double*> d_raw(rawC, nullptr);
        int64_t up = 0;
        rawCA = 0;
        graph_stats_[GS_BYTES_UPLOADED] = 0;
        for (int a = 0; a < CA; ++a) {
            const int c = vplan.cloud[cloudA[a]];
            if (!d_raw[c]) {
                ++rawCA;
                if (on_device) {
                    d_raw[c] = rawxyz[c];
                } else {
                    double* dst = (double*)d_in_.p + 3 * (size_t)up;
                    HIPCHK(hipMemcpyAsync(dst, rawxyz[c], sizeof(double) * 3 * rawnpts[c], hipMemcpyHostToDevice, s));
                    d_raw[c] = dst;
                    up += rawnpts[c];
                    graph_stats_[GS_BYTES_UPLOADED] += (int64_t)sizeof(double) * 3 * rawnpts[c];
                }
            }
            reqA[a].in = d_raw[c];
        }
    }
    rc = upload_clouds(reqA, on_device || posed, s);
    if (rc) return rc;
    const std::vector<CloudDev> clA = h_clouds_;
    const int nchA = (int)h_chunks_.size();
    View v = view();
    if (posed) {
        // the posed ingest: A's slot a is its raw cloud read through the pose of its variant
        pose_of_.assign(CA, -1);
        pose_tab_.clear();
        pose_raw_.assign(C, 0);
        pose_rigid_.assign(C, 1);
        for (int a = 0; a < CA; ++a) {
            const int vv = cloudA[a];
            pose_raw_[vv] = vplan.cloud[vv];
            if (vplan.pose_edge[vv] < 0) continue;
            const double* M = T_init + 16 * (size_t)vplan.pose_edge[vv];
            pose_of_[a] = (int32_t)(pose_tab_.size() / 16);
            pose_tab_.insert(pose_tab_.end(), M, M + 16);
            pose_rigid_[vv] = pose_is_rigid(M) ? 1 : 0;
        }
        if (!ensure<int32_t>(d_pose_of_, CA) || !ensure<double>(d_pose_tab_, pose_tab_.size()))
            return SE3ICP_ERR_OUT_OF_MEMORY;
        HIPCHK(hipMemcpyAsync(d_pose_of_.p, pose_of_.data(), sizeof(int32_t) * CA, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_pose_tab_.p, pose_tab_.data(), sizeof(double) * pose_tab_.size(), hipMemcpyHostToDevice, s));
        launch_ingest_posed(v, (const ChunkWork*)d_chunks_.p, nchA, (double*)d_partial_.p, (const int32_t*)d_pose_of_.p,
                            (const double*)d_pose_tab_.p, s);
        init_stats_[IS_EDGES] = vplan.posed_edges;
        init_stats_[IS_VARIANTS] = vplan.posed_variants;
    } else {
        launch_ingest(v, (const ChunkWork*)d_chunks_.p, nchA, (double*)d_partial_.p, s);
    }
    HIPCHK(hipGetLastError());
    std::vector<double> cenC(3 * (size_t)C, 0.0), radC(C, 0.0);  // by the call's cloud index
    if (se3) {
        // GetCenter and the radius as a batch forms them (k_pair_centers folds a cloud's chunks by
        // chunk index modulo 64, then a butterfly: the same sum at any position while a cloud's
        // chunks are contiguous and in order; the radius is a maximum)
        launch_pair_centers(v, (const ChunkWork*)d_chunks_.p, nchA, (const double*)d_partial_.p, (double*)d_centers_.p, s);
        launch_radius(v, (const ChunkWork*)d_chunks_.p, nchA, (const double*)d_centers_.p, (double*)d_partial_.p, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_partial_, d_centers_.p, sizeof(double) * 3 * CA, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(h_partial_ + 3 * (size_t)CA, d_partial_.p, sizeof(double) * nchA, hipMemcpyDeviceToHost, s));
        SYNC_STREAM(s);
        for (int a = 0; a < CA; ++a)
            for (int x = 0; x < 3; ++x) cenC[3 * (size_t)cloudA[a] + x] = h_partial_[3 * (size_t)a + x];
        for (int a = 0; a < CA; ++a) radC[cloudA[a]] = -1.0;
        for (int k = 0; k < nchA; ++k) {
            double& r = radC[cloudA[h_chunks_[k].cloud]];
            r = std::fmax(r, h_partial_[3 * (size_t)CA + k]);
        }
    } else {
        // run_icp: the centroid as setup_clouds forms it on the host
        std::vector<double> cenA;
        rc = host_centroids(s, &cenA);
        if (rc) return rc;
        for (int a = 0; a < CA; ++a)
            for (int x = 0; x < 3; ++x) cenC[3 * (size_t)cloudA[a] + x] = cenA[3 * (size_t)a + x];
    }

    // ---- classes
    GraphPlan plan;
    graph_plan(P, esrc, etgt, se3, prm.scale_preprocessing, cenC.data(), radC.data(), mp.k_nrm_s, mp.k_nrm_t,
               sharing >= 2, &plan);
    const int K = (int)plan.classes.size();
    graph_stats_[GS_CLOUDS] = rawCA;
    graph_stats_[GS_USES] = 2 * (int64_t)P;
    graph_stats_[GS_CLASSES] = K;

    // ---- B: the uses.  A's raw columns and confidences are kept aside; every use is normalized
    // from them and given its 3-D tree, the first use of a class ("home") runs the class's
    // neighbour selection, frames and normals, and the other uses copy them.
    auto regrow = [&](DevBuf& kept, DevBuf& cur, size_t bytes) {
        std::swap(kept, cur);
        return ensure<char>(cur, bytes) != nullptr;
    };
    if (!regrow(g_raw_xyz_, d_xyz64_, sizeof(double) * 3 * L) || !regrow(g_raw_conf_, d_conf64_, sizeof(double) * L))
        return SE3ICP_ERR_OUT_OF_MEMORY;
    nclouds_ = 2 * P;
    npairs_ = P;
    ntot_ = NU;
    std::vector<CloudDev> clU(2 * (size_t)P);
    std::vector<CloudSetup> stU(2 * (size_t)P);  // a batch's table
    std::vector<ChunkWork> chU;
    std::vector<GraphSeg> segU(2 * (size_t)P);
    std::vector<double> cenU(6 * (size_t)P), scaleU(P, 1.0);
    int max_n = 1;
    {
        int64_t off = 0;
        for (int u = 0; u < 2 * P; ++u) {
            const int side = u & 1;
            const GraphClass& gc = plan.classes[plan.use_class[u]];
            const int64_t n = npts[gc.cloud];
            clU[u] = CloudDev{(int32_t)off, (int32_t)n};
            CloudSetup& st = stU[u] = cloud_setup(mp, side, prm.alpha_rot, prm.beta_transl, true);
            for (int x = 0; x < 3; ++x) {
                st.norm_center[x] = gc.norm_center[x];
                st.f32_center[x] = gc.f32_center[x];
                cenU[3 * (size_t)u + x] = gc.norm_center[x];
            }
            st.norm_scale = gc.norm_scale;
            if (side == 0) scaleU[u >> 1] = gc.norm_scale;
            segU[u] = GraphSeg{clA[slotA[gc.cloud]].off, slotA[gc.cloud], 0, 0};
            for (int64_t p0 = 0; p0 < n; p0 += kChunk) chU.push_back(ChunkWork{u, (int32_t)p0});
            max_n = std::max<int>(max_n, (int)n);
            off += n;
        }
    }
    tree_L_ = tree_depth_for(max_n);
    h_clouds_ = clU;
    h_setup_ = stU;
    const int nchU2 = (int)chU.size();
    HIPCHK(hipMemcpyAsync(d_clouds_.p, clU.data(), sizeof(CloudDev) * 2 * P, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_setup_.p, stU.data(), sizeof(CloudSetup) * 2 * P, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_chunks_.p, chU.data(), sizeof(ChunkWork) * nchU2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(g_seg_.p, segU.data(), sizeof(GraphSeg) * 2 * P, hipMemcpyHostToDevice, s));
    if (se3) {
        HIPCHK(hipMemcpyAsync(d_centers_.p, cenU.data(), sizeof(double) * 6 * P, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_scales_.p, scaleU.data(), sizeof(double) * P, hipMemcpyHostToDevice, s));
    }
    launch_graph_normalize(view(), (const ChunkWork*)d_chunks_.p, nchU2, (const GraphSeg*)g_seg_.p,
                           (const double*)g_raw_xyz_.p, (const double*)g_raw_conf_.p, s);
    HIPCHK(hipGetLastError());
    // the later uses of a cloud adopt its first use's tree order (graph_plan_trees)
    {
        std::vector<int32_t> ucloud(2 * (size_t)P), donor;
        std::vector<int64_t> un(2 * (size_t)P);
        for (int u = 0; u < 2 * P; ++u) {
            ucloud[u] = plan.classes[plan.use_class[u]].cloud;
            un[u] = clU[u].n;
        }
        const int nad = graph_plan_trees(2 * P, ucloud.data(), un.data(), sharing >= 2 && tree_sharing_ != 1, &donor);
        if (nad > 0) tree_donor_ = donor;
        rc = build_tree(3, (const float*)d_xyz32_.p, s, (const double*)d_xyz64_.p, nad > 0 ? &tree_donor_ : nullptr,
                        &tree_tab_a_);
    }
    if (rc) return rc;
    rc = select_by_class(plan, stU, mp, s);
    if (rc) return rc;
    rc = run_pairs(mp, P, ns.data(), nt.data(), &prm, P, false, call, out, ropts, reports);
    if (posed && (rc == 0 || rc == SE3ICP_ERR_NONFINITE)) {
        // the pose of the raw source: the de-normalized result on the posed source, then the pose
        for (int p = 0; p < P; ++p) {
            const int vv = vplan.edge_src[p];
            if (vplan.pose_edge[vv] < 0) continue;
            double Tc[16];
            compose(out[p].T, T_init + 16 * (size_t)vplan.pose_edge[vv], Tc);
            std::memcpy(out[p].T, Tc, sizeof(Tc));
        }
    }
    return rc;
}

// Row it-1 of the armed trace after iteration `it` completed (the stream is idle: the
// trace runs the loop without look-ahead).  phase_of_it: the pair's phase in iteration
// it, updated to its phase in iteration it+1.
int Engine::record_trace(se3icp_trace* tr, int it, int& phase_of_it, hipStream_t s) {
    const int p = tr->pair;
    PairState S;
    HIPCHK(hipMemcpyAsync(&S, (const PairState*)d_state_.p + p, sizeof(S), hipMemcpyDeviceToHost, s));
    uint64_t cut = UINT64_MAX;
    if (h_pairs_[p].trim) HIPCHK(hipMemcpyAsync(&cut, (const uint64_t*)d_trim_key_.p + p, sizeof(cut), hipMemcpyDeviceToHost, s));
    const int phase = phase_of_it;
    const int r = it - 1;
    const bool active = phase != PHASE_IDLE && r < tr->max_iters;
    const CloudDev& cs = h_clouds_[2 * p];
    if (active) {
        if (tr->corr_idx)
            HIPCHK(hipMemcpyAsync(tr->corr_idx + (size_t)r * cs.n, (const int32_t*)d_corr_idx_.p + cs.off,
                                  sizeof(int32_t) * cs.n, hipMemcpyDeviceToHost, s));
        if (tr->corr_dist)
            HIPCHK(hipMemcpyAsync(tr->corr_dist + (size_t)r * cs.n, (const float*)d_corr_dist_.p + cs.off,
                                  sizeof(float) * cs.n, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    if (active) {
        // a pair that took part in iteration it has iter >= it (one that finished at j keeps j)
        if (S.iter < it) return SE3ICP_ERR_HIP;
        if (tr->trim_key) tr->trim_key[r] = cut;
        if (tr->T)
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) tr->T[(size_t)r * 16 + 4 * i + j] = S.T.m[i][j];
        if (tr->mse) tr->mse[r] = S.mse_cur;
        if (tr->phase) tr->phase[r] = phase;
        tr->iters_recorded = it;
    }
    phase_of_it = S.done ? PHASE_IDLE : S.phase;
    return 0;
}

// The armed setup record of pair `pair` (cloud slots 2 * pair, 2 * pair + 1 of the layout
// run_pairs was given): the device's setup table first, which says what the setup produced for
// each side, then the arrays.  Called with the setup queued and no loop work behind it.
int Engine::record_setup(se3icp_setup_record* rec, int pair, hipStream_t s) {
    if (pair < 0 || 2 * pair + 1 >= nclouds_) return SE3ICP_ERR_INVALID_ARG;
    CloudSetup st[2];
    HIPCHK(hipMemcpyAsync(st, (const CloudSetup*)d_setup_.p + 2 * pair, sizeof(st), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const size_t ld = (size_t)ld_;
    std::vector<double> col;
    for (int side = 0; side < 2; ++side) {
        se3icp_setup_side& o = side == 0 ? rec->src : rec->tgt;
        const CloudDev& cd = h_clouds_[2 * pair + side];
        const CloudSetup& cs = st[side];
        const size_t n = (size_t)cd.n, off = (size_t)cd.off;
        o.n = cd.n;
        if ((int64_t)cd.n > o.cap && (o.xyz || o.rows || o.normals || o.conf)) return SE3ICP_ERR_INVALID_ARG;
        for (int a = 0; a < 3; ++a) {
            o.norm_center[a] = cs.norm_center[a];
            o.f32_center[a] = cs.f32_center[a];
        }
        o.norm_scale = cs.norm_scale;
        o.alpha = cs.alpha;
        o.beta = cs.beta;
        // the SoA columns [3][ld] of the points and the normals into AoS
        auto columns = [&](const DevBuf& b, double* out) -> int {
            col.resize(3 * n);
            for (int a = 0; a < 3; ++a)
                HIPCHK(hipMemcpyAsync(col.data() + a * n, (const double*)b.p + a * ld + off, sizeof(double) * n,
                                      hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (size_t i = 0; i < n; ++i)
                for (int a = 0; a < 3; ++a) out[3 * i + a] = col[a * n + i];
            return 0;
        };
        int32_t written = 0;
        if (o.xyz) {
            const int rc = columns(d_xyz64_, o.xyz);
            if (rc) return rc;
            written |= SE3ICP_SETUP_XYZ;
        }
        if (o.rows && cs.k_lrf > 0) {
            HIPCHK(hipMemcpyAsync(o.rows, (const double*)d_fr64_.p + 12 * off, sizeof(double) * 12 * n,
                                  hipMemcpyDeviceToHost, s));
            written |= SE3ICP_SETUP_ROWS;
        }
        if (o.normals && cs.k_nrm > 0) {
            const int rc = columns(d_nrm64_, o.normals);
            if (rc) return rc;
            written |= SE3ICP_SETUP_NORMALS;
        }
        if (o.conf && cs.want_conf) {
            HIPCHK(hipMemcpyAsync(o.conf, (const double*)d_conf64_.p + off, sizeof(double) * n, hipMemcpyDeviceToHost, s));
            written |= SE3ICP_SETUP_CONF;
        }
        HIPCHK(hipStreamSynchronize(s));
        o.written = written;
    }
    rec->recorded = 1;
    return 0;
}

// The armed tree record of pair `pair` (cloud slots 2 * pair, 2 * pair + 1 of the current
// layout): per slot and dimension the scalars of the last build that touched the slot
// (tree_log_), then the arrays the searches read, from the device's layouts (tree.hpp: 3-D
// columns [3][ld], 12-D rows [ld][12], boxes [nclouds][2^(L+1)][D]) into [n][D].  `written`
// follows the kernels: a loop source's 12-D tree below depth 0 is order only (k_tree_local's
// order_only; at depth 0 k_tree_finish and k_tree_leafbox write every cloud alike), the f64
// 12-D vectors are the sources'.  Called with the builds queued and no loop work behind them.
int Engine::record_trees(se3icp_tree_record* rec, int pair, hipStream_t s) {
    if (pair < 0 || 2 * pair + 1 >= nclouds_) return SE3ICP_ERR_INVALID_ARG;
    HIPCHK(hipStreamSynchronize(s));
    const size_t ld = (size_t)ld_;
    std::vector<float> f32;
    std::vector<double> f64;
    for (int k = 0; k < 4; ++k) {
        const int side = k & 1, D = k < 2 ? 3 : 12;
        se3icp_tree_side& o = *(k == 0 ? &rec->src3 : k == 1 ? &rec->tgt3 : k == 2 ? &rec->src12 : &rec->tgt12);
        const int c = 2 * pair + side;
        const std::vector<TreeLog>& log = tree_log_[D == 12];
        o.n = 0;
        o.exists = o.D = o.L = o.nnodes = o.G = o.H = o.role = o.written = 0;
        if ((int)log.size() != nclouds_ || log[c].role == kTreeAbsent) continue;
        const TreeLog& lg = log[c];
        const TreeBufs& tb = D == 12 ? t12_ : t3_;
        const CloudDev& cd = h_clouds_[c];
        const size_t n = (size_t)cd.n, off = (size_t)cd.off;
        const size_t slots = (size_t)2 << lg.L, nodes = slots - 1;
        o.n = cd.n;
        o.exists = 1;
        o.D = D;
        o.L = lg.L;
        o.nnodes = (int32_t)nodes;
        o.G = lg.G;
        o.H = lg.H;
        o.role = lg.role;
        const bool order_only = D == 12 && side == 0 && lg.L > 0;
        const bool has64 = D == 3 || side == 0;
        if ((int64_t)cd.n > o.cap && (o.perm || o.pos || o.vec || o.tvec || o.tvec64 || o.tpt64)) return SE3ICP_ERR_INVALID_ARG;
        if ((int64_t)nodes > o.node_cap && (o.lo || o.hi)) return SE3ICP_ERR_INVALID_ARG;
        int32_t written = 0;
        auto get = [&](void* dst, const void* src, size_t bytes) -> int {
            HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
            return 0;
        };
        // [D][ld] f32 columns or [ld][12] rows of the cloud's n slots from `base` into out [n][D]
        auto vectors = [&](const void* base, float* out) -> int {
            if (D == 12) return get(out, (const float*)base + 12 * off, sizeof(float) * 12 * n);
            f32.resize(3 * n);
            for (int a = 0; a < 3; ++a)
                if (int rc = get(f32.data() + a * n, (const float*)base + a * ld + off, sizeof(float) * n)) return rc;
            for (size_t i = 0; i < n; ++i)
                for (int a = 0; a < 3; ++a) out[3 * i + a] = f32[a * n + i];
            return 0;
        };
        int rc = 0;
        if (o.perm) {
            if ((rc = get(o.perm, (const int32_t*)tb.perm.p + off, sizeof(int32_t) * n))) return rc;
            written |= SE3ICP_TREE_PERM;
        }
        if (o.pos && !order_only) {
            if ((rc = get(o.pos, (const int32_t*)tb.pos.p + off, sizeof(int32_t) * n))) return rc;
            written |= SE3ICP_TREE_POS;
        }
        if (o.vec) {
            if ((rc = vectors(D == 12 ? d_fr32_.p : d_xyz32_.p, o.vec))) return rc;
            written |= SE3ICP_TREE_VEC;
        }
        if (o.tvec && !order_only) {
            if ((rc = vectors(tb.vec.p, o.tvec))) return rc;
            written |= SE3ICP_TREE_TVEC;
        }
        if (o.tvec64 && has64 && tb.vec64.p) {
            f64.resize(3 * n);
            for (int a = 0; a < 3; ++a)
                if ((rc = get(f64.data() + a * n, (const double*)tb.vec64.p + a * ld + off, sizeof(double) * n))) return rc;
            for (size_t i = 0; i < n; ++i)
                for (int a = 0; a < 3; ++a) o.tvec64[3 * i + a] = f64[a * n + i];
            written |= SE3ICP_TREE_TVEC64;
        }
        if (o.tpt64 && D == 3 && tb.vec64a.p) {
            if ((rc = get(o.tpt64, (const double4*)tb.vec64a.p + off, sizeof(double4) * n))) return rc;
            written |= SE3ICP_TREE_TPT64;
        }
        if ((o.lo || o.hi) && !order_only) {
            const size_t at = (size_t)c * slots * D;
            if (o.lo && (rc = get(o.lo, (const float*)tb.lo.p + at, sizeof(float) * nodes * D))) return rc;
            if (o.hi && (rc = get(o.hi, (const float*)tb.hi.p + at, sizeof(float) * nodes * D))) return rc;
            if (o.lo && o.hi) written |= SE3ICP_TREE_BOXES;
        }
        o.written = written;
    }
    rec->recorded = 1;
    return 0;
}

// ----------------------------------------------------------------------------- stage entry points
// The front of knn_self, toldi_frames and estimate_normals: the argument checks, then the setup of
// one cloud that stands alone with k neighbours, frames (k_lrf) or normals (k_nrm) of them.
int Engine::setup_single(const double* xyz, const void* out, int64_t n, int k, bool frames, bool normals) {
    if (!ok_) return SE3ICP_ERR_NO_DEVICE;
    if (!xyz || !out || n <= 0) return n <= 0 ? SE3ICP_ERR_EMPTY_CLOUD : SE3ICP_ERR_INVALID_ARG;
    if (k <= 0) return SE3ICP_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(dev_));
    npairs_ = 0;
    const int rc = alloc_points(n, k, !frames && !normals);  // (the sorted lists: knn_self)
    if (rc) return rc;
    std::vector<CloudReq> cl(1);
    cl[0].in = xyz;
    cl[0].n = n;
    cl[0].st.k_knn = k;
    cl[0].st.k_lrf = frames ? k : 0;
    cl[0].st.k_nrm = normals ? k : 0;
    cl[0].st.alpha = cl[0].st.beta = frames ? 1.0 : 0.0;
    cl[0].st.norm_scale = 1.0;
    return setup_clouds(cl, false, false, false, 1.0, stream_);
}

int Engine::knn_self(const double* xyz, int64_t n, int k, int32_t* idx) {
    const int rc = setup_single(xyz, idx, n, k, false, false);
    if (rc) return rc;
    HIPCHK(hipMemcpy2DAsync(idx, sizeof(int32_t) * k, d_knn_.p, sizeof(int32_t) * kmax_, sizeof(int32_t) * k, n,
                            hipMemcpyDeviceToHost, stream_));
    SYNC_STREAM(stream_);
    return 0;
}

int Engine::toldi_frames(const double* xyz, int64_t n, int k, double* frames) {
    const int rc = setup_single(xyz, frames, n, k, true, false);
    if (rc) return rc;
    std::vector<double> fr(12 * (size_t)ld_);
    HIPCHK(hipMemcpyAsync(fr.data(), d_fr64_.p, sizeof(double) * 12 * ld_, hipMemcpyDeviceToHost, stream_));
    SYNC_STREAM(stream_);
    for (int64_t i = 0; i < n; ++i) {
        double* F = frames + 16 * i;
        // packing [R00 R10 R20 R01 R11 R21 R02 R12 R22 t0 t1 t2] -> row-major 4x4
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) F[r * 4 + c] = fr[(size_t)i * 12 + c * 3 + r];
            F[r * 4 + 3] = fr[(size_t)i * 12 + 9 + r];
        }
        F[12] = F[13] = F[14] = 0.0;
        F[15] = 1.0;
    }
    return 0;
}

int Engine::estimate_normals(const double* xyz, int64_t n, int k, double* normals) {
    const int rc = setup_single(xyz, normals, n, k, false, true);
    if (rc) return rc;
    std::vector<double> nr(3 * (size_t)ld_);
    HIPCHK(hipMemcpyAsync(nr.data(), d_nrm64_.p, sizeof(double) * 3 * ld_, hipMemcpyDeviceToHost, stream_));
    SYNC_STREAM(stream_);
    for (int64_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) normals[3 * i + a] = nr[(size_t)a * ld_ + i];
    return 0;
}

// The setup of the NN stage entries (nn, nn_sequence): the vectors in the source / target slots
// of a one-pair batch, host-filled SoA, the kd-trees, the chunks, a neutral setup table with
// `alpha`, and the pair record of iteration 1 with the identity pose -- everything up to the
// launches.  The arguments are valid.
int Engine::nn_setup(const double* query, int64_t nq, const double* data, int64_t nd, int dim, double alpha) {
    HIPCHK(hipSetDevice(dev_));
    hipStream_t s = stream_;
    npairs_ = 1;
    nclouds_ = 2;
    const int64_t ntot = nq + nd;
    int rc = alloc_points(ntot, 1);
    if (rc) return rc;
    if (!ensure<PairDev>(d_pairs_, 1) || !ensure<CloudDev>(d_clouds_, 2) || !ensure<CloudSetup>(d_setup_, 2) ||
        !ensure<int32_t>(d_rechecked_, 1))
        return SE3ICP_ERR_OUT_OF_MEMORY;
    // k_nn_prep reads the source cloud's alpha for every position: a neutral table of this
    // call's own (an engine whose first call this is has none)
    h_setup_.assign(2, CloudSetup{});
    for (CloudSetup& st : h_setup_) st.alpha = st.beta = st.norm_scale = 1.0;
    h_setup_[0].alpha = alpha;
    h_setup_[1].is_target = 1;
    HIPCHK(hipMemcpyAsync(d_setup_.p, h_setup_.data(), sizeof(CloudSetup) * 2, hipMemcpyHostToDevice, s));
    h_clouds_.assign(2, CloudDev{});
    h_clouds_[0].off = 0;
    h_clouds_[0].n = (int32_t)nq;
    h_clouds_[1].off = (int32_t)nq;
    h_clouds_[1].n = (int32_t)nd;
    tree_L_ = tree_depth_for((int)std::max(nq, nd));
    // SoA f64 masters + f32 copies, filled on the host (diagnostic entry point)
    const size_t L = ld_;
    // (members: the copies below are asynchronous and outlive this function)
    std::vector<int32_t>& cof = nn_cof_;
    cof.assign(L, 0);
    for (int64_t i = nq; i < ntot; ++i) cof[i] = 1;
    double cen[3] = {0, 0, 0};
    if (dim == 3) {
        for (int64_t j = 0; j < nd; ++j)
            for (int a = 0; a < 3; ++a) cen[a] += data[3 * j + a];
        for (int a = 0; a < 3; ++a) cen[a] /= (double)nd;
    }
    std::vector<double>& m64 = nn_m64_;
    std::vector<float>& m32 = nn_m32_;
    m64.assign((size_t)dim * L, 0.0);
    m32.assign((size_t)dim * L, 0.f);
    double nb = 0;
    for (int64_t i = 0; i < ntot; ++i) {
        const double* row = i < nq ? query + dim * i : data + dim * (i - nq);
        double n2 = 0;
        for (int r = 0; r < dim; ++r) {  // (12-D vectors as rows, 3-D points as columns: tree_in_ix)
            const size_t at = dim == 12 ? (size_t)i * 12 + r : (size_t)r * L + i;
            m64[at] = row[r];
            const double c = dim == 3 ? row[r] - cen[r] : row[r];
            m32[at] = (float)c;
            n2 += c * c;
        }
        if (i >= nq) nb = std::max(nb, std::sqrt(n2));
    }
    double* dst64 = dim == 12 ? (double*)d_fr64_.p : (double*)d_xyz64_.p;
    float* dst32 = dim == 12 ? (float*)d_fr32_.p : (float*)d_xyz32_.p;
    HIPCHK(hipMemcpyAsync(dst64, m64.data(), sizeof(double) * m64.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dst32, m32.data(), sizeof(float) * m32.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_cloud_of_.p, cof.data(), sizeof(int32_t) * L, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_clouds_.p, h_clouds_.data(), sizeof(CloudDev) * 2, hipMemcpyHostToDevice, s));
    for (std::vector<TreeLog>& log : tree_log_) log.clear();
    se3icp_tree_record* tk = tree_rec_;  // one-shot, as a registration call's
    tree_rec_ = nullptr;
    if (tk && tk->pair != 0) return SE3ICP_ERR_INVALID_ARG;
    if (tk) tk->recorded = 0;
    rc = build_tree(dim, dst32, s, dst64);
    if (rc) return rc;
    if (tk) {
        rc = record_trees(tk, 0, s);
        if (rc) return rc;
    }
    rc = setup_chunks(1, s);
    if (rc) return rc;
    PairDev& P = nn_pair_;
    std::memset(&P, 0, sizeof(P));
    P.T[0] = P.T[5] = P.T[10] = 1.0;
    P.src = 0;
    P.tgt = 1;
    P.phase = dim == 12 ? PHASE_SE3 : PHASE_R3;
    P.iter = 1;
    P.phase_start = 1;
    P.tgt_norm12 = (float)(nb * (1 + 1e-6));
    P.tgt_norm3 = (float)(nb * (1 + 1e-6));
    for (int a = 0; a < 3; ++a) P.f32_center[a] = cen[a];
    HIPCHK(hipMemcpyAsync(d_pairs_.p, &P, sizeof(P), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_flag_count_.p, 0, 3 * sizeof(int32_t), s));
    HIPCHK(hipMemsetAsync(d_rechecked_.p, 0, sizeof(int32_t), s));
    HIPCHK(hipMemsetAsync(d_corr_idx_.p, 0xff, sizeof(int32_t) * L, s));
    return 0;
}

// Exact 1-NN of arbitrary query vectors among data vectors (3 or 12 dims): the vectors
// are placed in the source/target slots of a one-pair batch with the identity pose, the
// kd-trees are built over them, and the loop's NN kernels (with their inline f64 recheck) run once.
int Engine::nn(const double* query, int64_t nq, const double* data, int64_t nd, int dim, int32_t* idx, double* d2,
               int32_t* num_rechecked) {
    if (!ok_) return SE3ICP_ERR_NO_DEVICE;
    if (!query || !data || !idx || (dim != 3 && dim != 12)) return SE3ICP_ERR_INVALID_ARG;
    if (nq <= 0 || nd <= 0) return SE3ICP_ERR_EMPTY_CLOUD;
    // (alpha only weighs certificates of earlier searches, and a one-search run has none)
    int rc = nn_setup(query, nq, data, nd, dim, 1.0);
    if (rc) return rc;
    hipStream_t s = stream_;
    View v = view();
    launch_nn_prep(v, nullptr, s);
    launch_nn(v, dim, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(idx, d_corr_idx_.p, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, s));
    int32_t rech = 0;
    HIPCHK(hipMemcpyAsync(&rech, d_rechecked_.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SYNC_STREAM(s);
    if (num_rechecked) *num_rechecked = rech;
    // every query was searched: an index left unset (-1) or outside the data cloud is a
    // defect of the build or the search, reported instead of used as a row of `data`
    for (int64_t i = 0; i < nq; ++i)
        if (idx[i] < 0 || idx[i] >= nd) return SE3ICP_ERR_INTERNAL;
    if (d2) {
        for (int64_t i = 0; i < nq; ++i) {
            const double* a = query + dim * i;
            const double* b = data + (size_t)dim * idx[i];
            double r = 0;
            if (dim == 12) {
                for (int d = 0; d < 12; d += 4) {
                    const double d0 = a[d] - b[d], d1 = a[d + 1] - b[d + 1], dd2 = a[d + 2] - b[d + 2], d3 = a[d + 3] - b[d + 3];
                    r += d0 * d0 + d1 * d1 + dd2 * dd2 + d3 * d3;
                }
            } else {
                const double d0 = a[0] - b[0], d1 = a[1] - b[1], dd2 = a[2] - b[2];
                r = (d0 * d0 + d1 * d1) + dd2 * dd2;
            }
            d2[i] = r;
        }
    }
    return 0;
}

// The loop's k_nn_prep and search of a one-pair run whose poses are given: step k is
// iteration k.  Before it the host writes, stream-ordered, what pair_open_iteration and
// k_reduce_final leave for an iteration's k_nn_prep -- the pair record (pose, iteration, phase
// start), the pose's ring row, and the cleared single-query counts and cost-class counts --
// and launches the loop's own two kernels; corr_idx and the certificates carry over.  After
// the step the correspondences and the certificate records are read back (a wait per step: a
// diagnostic entry), the records mapped from source tree slots to query order.
int Engine::nn_sequence(const double* query, int64_t nq, const double* data, int64_t nd, int dim, double alpha,
                        int n_steps, const double* poses, int restart_at, const NNSequenceOut& out) {
    if (!ok_) return SE3ICP_ERR_NO_DEVICE;
    int rc = nn_setup(query, nq, data, nd, dim, alpha);
    if (rc) return rc;
    hipStream_t s = stream_;
    constexpr size_t kStats = (size_t)kStatCols * kStatSlots;
    HIPCHK(hipMemsetAsync(d_stats_.p, 0, sizeof(unsigned long long) * kStats, s));
    const TreeBufs& tb = dim == 12 ? t12_ : t3_;
    std::vector<int32_t> perm(nq), ci(nq);
    std::vector<float> cd(nq);
    std::vector<NNCert> cert(nq);
    std::vector<unsigned long long> st(kStats);
    HIPCHK(hipMemcpyAsync(perm.data(), tb.perm.p, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, s));  // (source cloud: slot 0 on)
    const View v = view();
    unsigned long long searched_before = 0;
    PairDev& P = nn_pair_;
    for (int k = 1; k <= n_steps; ++k) {
        std::memcpy(P.T, poses + 16 * (size_t)(k - 1), sizeof(P.T));
        P.iter = k;
        P.phase_start = (restart_at > 0 && k >= restart_at) ? restart_at : 1;
        HIPCHK(hipMemcpyAsync(d_pairs_.p, &P, sizeof(P), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync((double*)d_hist_.p + (size_t)(k % kHist) * 12, P.T, sizeof(P.T), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemsetAsync(d_flag_count_.p, 0, 3 * sizeof(int32_t), s));
        HIPCHK(hipMemsetAsync(d_cls_.p, 0, sizeof(int32_t) * 2 * 8 * 16, s));
        HIPCHK(hipMemsetAsync(d_rechecked_.p, 0, sizeof(int32_t), s));
        launch_nn_prep(v, nullptr, s);
        launch_nn(v, dim, s);
        HIPCHK(hipGetLastError());
        int32_t fc[3] = {0, 0, 0}, rech = 0;
        HIPCHK(hipMemcpyAsync(ci.data(), d_corr_idx_.p, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(cd.data(), d_corr_dist_.p, sizeof(float) * nq, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(cert.data(), d_cert_.p, sizeof(NNCert) * nq, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(fc, d_flag_count_.p, sizeof(fc), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&rech, d_rechecked_.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(st.data(), d_stats_.p, sizeof(unsigned long long) * kStats, hipMemcpyDeviceToHost, s));
        SYNC_STREAM(s);
        // k_nn_prep's work counter of the phase: queries it left to the search, summed over the slots
        unsigned long long searched = 0;
        for (int r = 0; r < kStatSlots; ++r) searched += st[(size_t)kStatCols * r + (dim == 12 ? 5 : 7)];
        const size_t row = (size_t)(k - 1) * nq;
        for (int64_t i = 0; i < nq; ++i)
            if (ci[i] < 0 || ci[i] >= nd) return SE3ICP_ERR_INTERNAL;
        for (int64_t x = 0; x < nq; ++x)
            if (perm[x] < 0 || perm[x] >= nq) return SE3ICP_ERR_INTERNAL;
        if (out.idx) std::memcpy(out.idx + row, ci.data(), sizeof(int32_t) * nq);
        if (out.dist) std::memcpy(out.dist + row, cd.data(), sizeof(float) * nq);
        for (int64_t x = 0; x < nq; ++x) {
            const size_t at = row + perm[x];
            if (out.cert_d1) out.cert_d1[at] = cert[x].d1;
            if (out.cert_l2) out.cert_l2[at] = cert[x].l2;
            if (out.cert_iter) out.cert_iter[at] = cert[x].iter;
            if (out.cert_j) out.cert_j[at] = cert[x].j;
        }
        if (out.searched) out.searched[k - 1] = (int32_t)(searched - searched_before);
        if (out.single) out.single[k - 1] = fc[dim == 12 ? 1 : 2];
        if (out.rechecked) out.rechecked[k - 1] = rech;
        searched_before = searched;
    }
    return 0;
}

// ----------------------------------------------------------------------------- engine registry
// ----------------------------------------------------------------------------- voxel-grid downsample
int Engine::voxel_downsample(int nclouds, const double* d_xyz, const int64_t* off, const double* vs, double* d_out,
                             int64_t* out_off, int32_t* d_count, int32_t* d_first, hipStream_t user_stream) {
    if (!ok_) return SE3ICP_ERR_NO_DEVICE;
    if (!d_xyz || !d_out || !out_off) return SE3ICP_ERR_INVALID_ARG;
    if (nclouds > 65535) return SE3ICP_ERR_INVALID_ARG;  // one grid row per cloud
    HIPCHK(hipSetDevice(dev_));
    hipStream_t s = user_stream ? user_stream : stream_;
    if (h_vclouds_.reserve(nclouds)) return SE3ICP_ERR_OUT_OF_MEMORY;
    int64_t N = 0, slots = 0, chunks = 0;
    int max_chunks = 1;
    for (int c = 0; c < nclouds; ++c) {
        const int64_t n = off[c + 1] - off[c];
        if (N + n >= (int64_t)1 << 30) return SE3ICP_ERR_INVALID_ARG;  // as a batch's points
        VoxelCloud& cl = h_vclouds_[c];
        cl.off = off[c];
        cl.pt0 = N;
        cl.tab = slots;
        cl.slots = voxel_table_slots(n);
        cl.chunk0 = chunks;
        cl.voxel_size = vs[c];
        cl.n = (int32_t)n;
        cl.nchunks = (int32_t)((n + kVoxChunkPoints - 1) / kVoxChunkPoints);
        N += n;
        slots += cl.slots;
        chunks += cl.nchunks;
        max_chunks = std::max(max_chunks, (int)cl.nchunks);
    }
    const int64_t big_cap = N / (kVoxLane + 1) + 1;
    const size_t nflags = 2 * (size_t)nclouds + 2;  // status, n_out, error, n_big
    VoxelArgs a{};
    a.n_clouds = nclouds;
    a.big_cap = (int32_t)big_cap;
    a.xyz = d_xyz;
    a.clouds = ensure<VoxelCloud>(v_clouds_, nclouds);
    a.grids = ensure<VoxelGrid>(v_grids_, nclouds);
    a.minmax = ensure<double>(v_minmax_, 6 * (size_t)chunks);
    a.chunk_sums = ensure<int32_t>(v_sums_, 2 * (size_t)chunks);
    a.table = ensure<VoxelSlot>(v_table_, (size_t)slots);
    a.vid = ensure<int32_t>(v_vid_, (size_t)N);
    a.members = ensure<int32_t>(v_members_, (size_t)N);
    a.recs = ensure<VoxelRec>(v_recs_, (size_t)N);
    a.big = ensure<int32_t>(v_big_, (size_t)big_cap);
    int32_t* flags = ensure<int32_t>(v_flags_, nflags);
    a.out_off = ensure<long long>(v_out_off_, (size_t)nclouds + 1);
    if (!a.clouds || !a.grids || !a.minmax || !a.chunk_sums || !a.table || !a.vid ||
        !a.members || !a.recs || !a.big || !flags || !a.out_off || h_vout_.reserve((size_t)nclouds + 1) ||
        h_vflags_.reserve(nflags))
        return SE3ICP_ERR_OUT_OF_MEMORY;
    a.status = flags;
    a.n_out = flags + nclouds;
    a.error = flags + 2 * (size_t)nclouds;
    a.n_big = a.error + 1;
    a.out = d_out;
    a.out_count = d_count;
    a.out_first = d_first;
    HIPCHK(hipMemcpyAsync(v_clouds_.p, (const VoxelCloud*)h_vclouds_, sizeof(VoxelCloud) * nclouds, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(flags, 0, sizeof(int32_t) * nflags, s));
    launch_voxel(a, max_chunks, N, slots, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync((long long*)h_vout_, a.out_off, sizeof(long long) * ((size_t)nclouds + 1), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync((int32_t*)h_vflags_, flags, sizeof(int32_t) * nflags, hipMemcpyDeviceToHost, s));
    SYNC_STREAM(s);
    for (int c = 0; c < nclouds; ++c) {
        const int32_t st = h_vflags_[c];
        if (st == VOX_NONFINITE) return SE3ICP_ERR_NONFINITE;
        if (st != VOX_OK) return SE3ICP_ERR_INVALID_ARG;  // too small a voxel, or a key past 63 bits
    }
    if (h_vflags_[2 * (size_t)nclouds] != 0) return SE3ICP_ERR_INTERNAL;
    for (int c = 0; c <= nclouds; ++c) out_off[c] = (int64_t)h_vout_[c];
    return 0;
}

int Engine::voxel_downsample_host(const double* xyz, int64_t n, double vs, double* out, int32_t* count, int32_t* first,
                                  int64_t* n_out) {
    if (!ok_) return SE3ICP_ERR_NO_DEVICE;
    if (!xyz || !n_out) return SE3ICP_ERR_INVALID_ARG;
    if (n >= (int64_t)1 << 30) return SE3ICP_ERR_INVALID_ARG;
    HIPCHK(hipSetDevice(dev_));
    double* d_in = ensure<double>(v_in_, 3 * (size_t)n);
    double* d_o = ensure<double>(v_out_, 3 * (size_t)n);
    int32_t* d_c = ensure<int32_t>(v_oc_, (size_t)n);
    int32_t* d_f = ensure<int32_t>(v_of_, (size_t)n);
    if (!d_in || !d_o || !d_c || !d_f) return SE3ICP_ERR_OUT_OF_MEMORY;
    HIPCHK(hipMemcpyAsync(d_in, xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, stream_));
    const int64_t off[2] = {0, n};
    int64_t oo[2] = {0, 0};
    const int rc = voxel_downsample(1, d_in, off, &vs, d_o, oo, d_c, d_f, nullptr);
    if (rc) return rc;
    const size_t m = (size_t)oo[1];
    if (out) HIPCHK(hipMemcpyAsync(out, d_o, sizeof(double) * 3 * m, hipMemcpyDeviceToHost, stream_));
    if (count) HIPCHK(hipMemcpyAsync(count, d_c, sizeof(int32_t) * m, hipMemcpyDeviceToHost, stream_));
    if (first) HIPCHK(hipMemcpyAsync(first, d_f, sizeof(int32_t) * m, hipMemcpyDeviceToHost, stream_));
    if (out || count || first) SYNC_STREAM(stream_);
    *n_out = oo[1];
    return 0;
}

// ----------------------------------------------------------------------------- transform stage
int Engine::transform_device(int nclouds, const double* d_xyz, const int64_t* off, const double* T, double* d_out,
                             hipStream_t user_stream) {
    if (!ok_) return SE3ICP_ERR_NO_DEVICE;
    if (!d_xyz || !d_out || !off || !T || nclouds <= 0) return SE3ICP_ERR_INVALID_ARG;
    if (nclouds > 65535) return SE3ICP_ERR_INVALID_ARG;  // one grid row per cloud
    HIPCHK(hipSetDevice(dev_));
    hipStream_t s = user_stream ? user_stream : stream_;
    if (h_tf_clouds_.reserve(nclouds) || h_tf_poses_.reserve(16 * (size_t)nclouds)) return SE3ICP_ERR_OUT_OF_MEMORY;
    PoseCloud* dc = ensure<PoseCloud>(d_tf_clouds_, nclouds);
    double* dp = ensure<double>(d_tf_poses_, 16 * (size_t)nclouds);
    if (!dc || !dp) return SE3ICP_ERR_OUT_OF_MEMORY;
    int64_t max_n = 0;
    for (int c = 0; c < nclouds; ++c) {
        const int64_t n = off[c + 1] - off[c];
        h_tf_clouds_[c] = PoseCloud{(long long)off[c], (long long)n};
        max_n = std::max(max_n, n);
    }
    std::memcpy((double*)h_tf_poses_, T, sizeof(double) * 16 * (size_t)nclouds);
    const int64_t max_chunks = (max_n + kPoseChunk - 1) / kPoseChunk;
    if (max_chunks > INT32_MAX) return SE3ICP_ERR_INVALID_ARG;
    HIPCHK(hipMemcpyAsync(dc, (const PoseCloud*)h_tf_clouds_, sizeof(PoseCloud) * nclouds, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dp, (const double*)h_tf_poses_, sizeof(double) * 16 * (size_t)nclouds, hipMemcpyHostToDevice, s));
    launch_transform(d_xyz, d_out, dc, dp, nclouds, (int)max_chunks, s);
    HIPCHK(hipGetLastError());
    SYNC_STREAM(s);  // (the pinned tables are the next call's too)
    return 0;
}

Engine* engine_for(int device) {
    static std::mutex reg_mu;
    static std::map<int, std::unique_ptr<Engine>> reg;
    std::lock_guard<std::mutex> lk(reg_mu);
    auto it = reg.find(device);
    if (it != reg.end()) return it->second.get();
    auto e = std::make_unique<Engine>(device & 0xff);  // (slots: see capi.cpp usable_engine)
    Engine* raw = e.get();
    reg[device] = std::move(e);
    return raw;
}

}  // namespace se3icp
