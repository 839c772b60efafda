// capi.cpp — extern "C" boundary of libse3icp.so (declared in include/se3icp.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <mutex>
#include <string>
#include <vector>

#include "engine.hpp"
#include "graph.hpp"
#include "pose.hpp"
#include "se3icp.h"

using se3icp::Engine;
using se3icp::engine_for;
using se3icp::graph_check;
using se3icp::GS_COUNT;

namespace {

const char* kMethodNames[SE3ICP_NUM_METHODS] = {"pt2pt",     "pt2pl",     "gicp",
                                                "se3_pt2pt", "se3_pt2pl", "se3_gicp",
                                                "se3_gicp_with_cf", "se3_pure_pt2pt", "se3_pure_pt2pl",
                                                "se3_pure_gicp"};

int variant_index(const char* v) {
    if (!v) return -1;
    if (!std::strcmp(v, "pt2pt")) return 0;
    if (!std::strcmp(v, "pt2pl")) return 1;
    if (!std::strcmp(v, "gicp")) return 2;
    return -1;
}

int current_device() {
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) return 0;
    return d;
}

// device = ordinal | slot << 8: slot s > 0 is a further engine on the same GPU (its own
// stream and buffers), so independent batches can be queued side by side
Engine* usable_engine(int device) {
    int n = 0;
    const int ord = device & 0xff;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || ord >= n || (device >> 8) > 15) return nullptr;
    return engine_for(device);
}

}  // namespace

struct se3icp_registration {
    std::vector<double> src, tgt;
    se3icp_params prm;
    se3icp_result res;
    // se3icp_request_report: the options of the next run's report, and the last report
    bool want_report = false, have_report = false;
    se3icp_report_options ropts{};
    se3icp_report rep{};
    // se3icp_set_initial_transform: the pose every run_* starts from
    bool have_init = false;
    double init[16] = {};
};

extern "C" {

int se3icp_abi_version(void) { return SE3ICP_ABI_VERSION; }

const char* se3icp_status_string(int status) {
    switch (status) {
        case SE3ICP_OK: return "ok";
        case SE3ICP_ERR_INVALID_ARG: return "invalid argument";
        case SE3ICP_ERR_INVALID_METHOD: return "invalid method name";
        case SE3ICP_ERR_EMPTY_CLOUD: return "empty point cloud";
        case SE3ICP_ERR_K_TOO_LARGE: return "number_of_nn_for_LRF too large (unused since ABI 3: any k is taken)";
        case SE3ICP_ERR_NO_DEVICE: return "no usable HIP device (the engine has no CPU fallback)";
        case SE3ICP_ERR_HIP: return "HIP runtime error";
        case SE3ICP_ERR_NONFINITE: return "non-finite pose";
        case SE3ICP_ERR_OUT_OF_MEMORY: return "out of device memory";
        case SE3ICP_ERR_INTERNAL: return "internal error: a result left unset or out of range";
        default: return "unknown status";
    }
}

int se3icp_method_from_name(const char* name) {
    if (!name) return SE3ICP_ERR_INVALID_METHOD;
    for (int m = 0; m < SE3ICP_NUM_METHODS; ++m)
        if (!std::strcmp(name, kMethodNames[m])) return m;
    return SE3ICP_ERR_INVALID_METHOD;
}

const char* se3icp_method_name(int method) {
    return (method >= 0 && method < SE3ICP_NUM_METHODS) ? kMethodNames[method] : nullptr;
}

// IterativeSE3Registration::IterativeSE3Registration()  ISR.cpp:334-348
void se3icp_default_params(se3icp_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->max_num_iterations = 150;
    p->max_num_se3_iterations = 20;
    p->number_of_nn_for_LRF = 30;
    p->mse = 0.00001;
    p->mse_switch_error = 0.001;
    p->estimated_overlap = 1.0;
    p->alpha_rot = 3.0;
    p->beta_transl = 1.0;
    p->scale_preprocessing = 3.0;
}

int se3icp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------ batch, sweep and report surface
static se3icp_params params_or_defaults(const se3icp_params* params) {
    se3icp_params p;
    if (params) p = *params; else se3icp_default_params(&p);
    return p;
}

// the per-pair pointers and sizes of clouds concatenated in HBM (the *_device entries)
struct PairRanges {
    std::vector<const double*> s, t;
    std::vector<int64_t> ns, nt;
};
static int pair_ranges(int32_t n_pairs, const double* d_src_xyz, const int64_t* src_off, const double* d_tgt_xyz,
                       const int64_t* tgt_off, PairRanges* r) {
    if (n_pairs <= 0 || !d_src_xyz || !d_tgt_xyz || !src_off || !tgt_off) return SE3ICP_ERR_INVALID_ARG;
    r->s.resize(n_pairs); r->t.resize(n_pairs); r->ns.resize(n_pairs); r->nt.resize(n_pairs);
    for (int i = 0; i < n_pairs; ++i) {
        r->s[i] = d_src_xyz + 3 * src_off[i];
        r->t[i] = d_tgt_xyz + 3 * tgt_off[i];
        r->ns[i] = src_off[i + 1] - src_off[i];
        r->nt[i] = tgt_off[i + 1] - tgt_off[i];
    }
    return SE3ICP_OK;
}

static int report_check(const se3icp_report_options* opts, const se3icp_report* reports, bool per_point_allowed) {
    if (!opts || !reports) return SE3ICP_ERR_INVALID_ARG;
    if (std::isnan(opts->max_correspondence_distance)) return SE3ICP_ERR_INVALID_ARG;
    if (!per_point_allowed && (opts->corr_idx || opts->corr_dist)) return SE3ICP_ERR_INVALID_ARG;
    return SE3ICP_OK;
}

// The pairs and the method of a batch or a sweep, and the frames' neighbourhood of `prm` (the
// batch's parameters, null for the defaults, or the sweep's first variant).
static int pairs_check(int32_t n_pairs, const double* const* src, const int64_t* n_src, const double* const* tgt,
                       const int64_t* n_tgt, int method, const se3icp_params* prm, const se3icp_result* results) {
    if (n_pairs <= 0 || !n_src || !n_tgt || !results) return SE3ICP_ERR_INVALID_ARG;
    if (method < 0 || method >= SE3ICP_NUM_METHODS) return SE3ICP_ERR_INVALID_METHOD;
    for (int32_t p = 0; p < n_pairs; ++p)
        if (n_src[p] <= 0 || n_tgt[p] <= 0) return SE3ICP_ERR_EMPTY_CLOUD;
    if (method >= SE3ICP_SE3_PT2PT && prm && prm->number_of_nn_for_LRF <= 0) return SE3ICP_ERR_INVALID_ARG;
    for (int32_t p = 0; p < n_pairs; ++p)
        if (!src[p] || !tgt[p]) return SE3ICP_ERR_INVALID_ARG;
    return SE3ICP_OK;
}

// The four batch entries.  args: the status of the entry's own pointer checks.  The two entries
// without a report look the device up first and leave every other check to the engine; the
// report entries check their arguments first, so a bad call is reported as such on a host
// without a GPU too.
static int batch_run(int device, int args, int32_t n_pairs, const double* const* src, const int64_t* n_src,
                     const double* const* tgt, const int64_t* n_tgt, bool on_device, int method,
                     const se3icp_params* params, se3icp_result* results, void* hip_stream,
                     const se3icp_report_options* opts, se3icp_report* reports, bool with_report) {
    if (with_report) {
        int rc = args ? args : report_check(opts, reports, true);
        if (!rc) rc = pairs_check(n_pairs, src, n_src, tgt, n_tgt, method, params, results);
        if (rc) return rc;
    }
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    if (args) return args;
    const se3icp_params p = params_or_defaults(params);
    std::lock_guard<std::mutex> lk(e->mutex());
    return e->register_batch(n_pairs, src, n_src, tgt, n_tgt, on_device, method, p, results, (hipStream_t)hip_stream,
                             with_report ? opts : nullptr, with_report ? reports : nullptr);
}

// The four sweep entries: all check their arguments before the device is looked up.
static int sweep_run(int device, int args, int32_t n_pairs, const double* const* src, const int64_t* n_src,
                     const double* const* tgt, const int64_t* n_tgt, bool on_device, int method, int32_t n_variants,
                     const se3icp_params* variants, int32_t max_group, se3icp_result* results, void* hip_stream,
                     const se3icp_report_options* opts, se3icp_report* reports, bool with_report) {
    int rc = args;
    if (!rc && with_report) rc = report_check(opts, reports, false);
    if (!rc && (n_variants <= 0 || !variants || max_group < 0)) rc = SE3ICP_ERR_INVALID_ARG;
    if (!rc) rc = pairs_check(n_pairs, src, n_src, tgt, n_tgt, method, variants, results);
    // what shapes the shared setup is common to all variants
    for (int32_t v = 1; !rc && v < n_variants; ++v)
        if (variants[v].number_of_nn_for_LRF != variants[0].number_of_nn_for_LRF ||
            variants[v].scale_preprocessing != variants[0].scale_preprocessing)
            rc = SE3ICP_ERR_INVALID_ARG;
    if (rc) return rc;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    return e->register_sweep(n_pairs, src, n_src, tgt, n_tgt, on_device, method, n_variants, variants, max_group,
                             results, (hipStream_t)hip_stream, with_report ? opts : nullptr,
                             with_report ? reports : nullptr);
}

int se3icp_register_batch(int device, int32_t n_pairs, const double* const* src_xyz, const int64_t* n_src,
                          const double* const* tgt_xyz, const int64_t* n_tgt, int method,
                          const se3icp_params* params, se3icp_result* results) {
    return batch_run(device, SE3ICP_OK, n_pairs, src_xyz, n_src, tgt_xyz, n_tgt, false, method, params, results,
                     nullptr, nullptr, nullptr, false);
}

int se3icp_register_batch_device(int device, int32_t n_pairs, const double* d_src_xyz, const int64_t* src_off,
                                 const double* d_tgt_xyz, const int64_t* tgt_off, int method,
                                 const se3icp_params* params, se3icp_result* results, void* hip_stream) {
    PairRanges r;
    const int args = pair_ranges(n_pairs, d_src_xyz, src_off, d_tgt_xyz, tgt_off, &r);
    return batch_run(device, args, n_pairs, r.s.data(), r.ns.data(), r.t.data(), r.nt.data(), true, method, params,
                     results, hip_stream, nullptr, nullptr, false);
}

int se3icp_register_batch_report(int device, int32_t n_pairs, const double* const* src_xyz, const int64_t* n_src,
                                 const double* const* tgt_xyz, const int64_t* n_tgt, int method,
                                 const se3icp_params* params, se3icp_result* results,
                                 const se3icp_report_options* opts, se3icp_report* reports) {
    const int args = (!src_xyz || !tgt_xyz) ? SE3ICP_ERR_INVALID_ARG : SE3ICP_OK;
    return batch_run(device, args, n_pairs, src_xyz, n_src, tgt_xyz, n_tgt, false, method, params, results, nullptr,
                     opts, reports, true);
}

int se3icp_register_batch_report_device(int device, int32_t n_pairs, const double* d_src_xyz, const int64_t* src_off,
                                        const double* d_tgt_xyz, const int64_t* tgt_off, int method,
                                        const se3icp_params* params, se3icp_result* results, void* hip_stream,
                                        const se3icp_report_options* opts, se3icp_report* reports) {
    PairRanges r;
    const int args = pair_ranges(n_pairs, d_src_xyz, src_off, d_tgt_xyz, tgt_off, &r);
    return batch_run(device, args, n_pairs, r.s.data(), r.ns.data(), r.t.data(), r.nt.data(), true, method, params,
                     results, hip_stream, opts, reports, true);
}

int se3icp_register_sweep(int device, int32_t n_pairs, const double* const* src_xyz, const int64_t* n_src,
                          const double* const* tgt_xyz, const int64_t* n_tgt, int method, int32_t n_variants,
                          const se3icp_params* variants, int32_t max_group, se3icp_result* results) {
    const int args = (!src_xyz || !tgt_xyz) ? SE3ICP_ERR_INVALID_ARG : SE3ICP_OK;
    return sweep_run(device, args, n_pairs, src_xyz, n_src, tgt_xyz, n_tgt, false, method, n_variants, variants,
                     max_group, results, nullptr, nullptr, nullptr, false);
}

int se3icp_register_sweep_device(int device, int32_t n_pairs, const double* d_src_xyz, const int64_t* src_off,
                                 const double* d_tgt_xyz, const int64_t* tgt_off, int method, int32_t n_variants,
                                 const se3icp_params* variants, int32_t max_group, se3icp_result* results,
                                 void* hip_stream) {
    PairRanges r;
    const int args = pair_ranges(n_pairs, d_src_xyz, src_off, d_tgt_xyz, tgt_off, &r);
    return sweep_run(device, args, n_pairs, r.s.data(), r.ns.data(), r.t.data(), r.nt.data(), true, method, n_variants,
                     variants, max_group, results, hip_stream, nullptr, nullptr, false);
}

int se3icp_report_version(void) { return 1; }

int se3icp_register_sweep_report(int device, int32_t n_pairs, const double* const* src_xyz, const int64_t* n_src,
                                 const double* const* tgt_xyz, const int64_t* n_tgt, int method, int32_t n_variants,
                                 const se3icp_params* variants, int32_t max_group, se3icp_result* results,
                                 const se3icp_report_options* opts, se3icp_report* reports) {
    const int args = (!src_xyz || !tgt_xyz) ? SE3ICP_ERR_INVALID_ARG : SE3ICP_OK;
    return sweep_run(device, args, n_pairs, src_xyz, n_src, tgt_xyz, n_tgt, false, method, n_variants, variants,
                     max_group, results, nullptr, opts, reports, true);
}

int se3icp_register_sweep_report_device(int device, int32_t n_pairs, const double* d_src_xyz, const int64_t* src_off,
                                        const double* d_tgt_xyz, const int64_t* tgt_off, int method,
                                        int32_t n_variants, const se3icp_params* variants, int32_t max_group,
                                        se3icp_result* results, void* hip_stream,
                                        const se3icp_report_options* opts, se3icp_report* reports) {
    PairRanges r;
    const int args = pair_ranges(n_pairs, d_src_xyz, src_off, d_tgt_xyz, tgt_off, &r);
    return sweep_run(device, args, n_pairs, r.s.data(), r.ns.data(), r.t.data(), r.nt.data(), true, method, n_variants,
                     variants, max_group, results, hip_stream, opts, reports, true);
}

// ------------------------------------------------------------------ cloud graphs
// Checked before the device is looked up, as the sweeps' arguments are (graph.hpp).
static int graph_run(int device, int32_t n_clouds, const double* const* xyz, const int64_t* n_pts, bool on_device,
                     int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud, int method,
                     const se3icp_params* params, int32_t sharing, se3icp_result* results, void* hip_stream,
                     bool with_report, const se3icp_report_options* opts, se3icp_report* reports,
                     const double* T_init = nullptr) {
    if (with_report) {
        const int rc = report_check(opts, reports, true);
        if (rc) return rc;
    }
    int rc = graph_check(n_clouds, n_pts, nullptr, n_pairs, src_cloud, tgt_cloud, method, SE3ICP_NUM_METHODS, sharing,
                         results);
    if (rc) return rc;
    if (method >= SE3ICP_SE3_PT2PT && params && params->number_of_nn_for_LRF <= 0) return SE3ICP_ERR_INVALID_ARG;
    for (int32_t p = 0; p < n_pairs; ++p)
        if (!xyz[src_cloud[p]] || !xyz[tgt_cloud[p]]) return SE3ICP_ERR_INVALID_ARG;
    if (T_init)
        for (int32_t p = 0; p < n_pairs; ++p)
            if (!se3icp::pose_is_valid(T_init + 16 * (size_t)p)) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    const se3icp_params p = params_or_defaults(params);
    std::lock_guard<std::mutex> lk(e->mutex());
    return e->register_graph(n_clouds, xyz, n_pts, n_pairs, src_cloud, tgt_cloud, on_device, method, p, sharing, results,
                             (hipStream_t)hip_stream, with_report ? opts : nullptr, with_report ? reports : nullptr,
                             T_init);
}

// the per-cloud pointers and sizes of clouds concatenated in HBM
static int cloud_ranges(int32_t n_clouds, const double* d_xyz, const int64_t* off, std::vector<const double*>& x,
                        std::vector<int64_t>& n) {
    if (n_clouds <= 0 || !d_xyz || !off) return SE3ICP_ERR_INVALID_ARG;
    x.resize(n_clouds);
    n.resize(n_clouds);
    for (int32_t c = 0; c < n_clouds; ++c) {
        x[c] = d_xyz + 3 * off[c];
        n[c] = off[c + 1] - off[c];
    }
    return SE3ICP_OK;
}

int se3icp_register_graph(int device, int32_t n_clouds, const double* const* xyz, const int64_t* n_pts,
                          int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud, int method,
                          const se3icp_params* params, int32_t sharing, se3icp_result* results) {
    if (!xyz) return SE3ICP_ERR_INVALID_ARG;
    return graph_run(device, n_clouds, xyz, n_pts, false, n_pairs, src_cloud, tgt_cloud, method, params, sharing, results,
                     nullptr, false, nullptr, nullptr);
}

int se3icp_register_graph_device(int device, int32_t n_clouds, const double* d_xyz, const int64_t* off,
                                 int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud, int method,
                                 const se3icp_params* params, int32_t sharing, se3icp_result* results,
                                 void* hip_stream) {
    std::vector<const double*> x;
    std::vector<int64_t> n;
    const int rc = cloud_ranges(n_clouds, d_xyz, off, x, n);
    if (rc) return rc;
    return graph_run(device, n_clouds, x.data(), n.data(), true, n_pairs, src_cloud, tgt_cloud, method, params, sharing,
                     results, hip_stream, false, nullptr, nullptr);
}

int se3icp_register_graph_report(int device, int32_t n_clouds, const double* const* xyz, const int64_t* n_pts,
                                 int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud, int method,
                                 const se3icp_params* params, int32_t sharing, se3icp_result* results,
                                 const se3icp_report_options* opts, se3icp_report* reports) {
    if (!xyz) return SE3ICP_ERR_INVALID_ARG;
    return graph_run(device, n_clouds, xyz, n_pts, false, n_pairs, src_cloud, tgt_cloud, method, params, sharing, results,
                     nullptr, true, opts, reports);
}

int se3icp_register_graph_report_device(int device, int32_t n_clouds, const double* d_xyz, const int64_t* off,
                                        int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud, int method,
                                        const se3icp_params* params, int32_t sharing, se3icp_result* results,
                                        void* hip_stream, const se3icp_report_options* opts, se3icp_report* reports) {
    std::vector<const double*> x;
    std::vector<int64_t> n;
    const int rc = cloud_ranges(n_clouds, d_xyz, off, x, n);
    if (rc) return rc;
    return graph_run(device, n_clouds, x.data(), n.data(), true, n_pairs, src_cloud, tgt_cloud, method, params, sharing,
                     results, hip_stream, true, opts, reports);
}

// ------------------------------------------------------------------ initial poses
int se3icp_init_version(void) { return 1; }

int se3icp_register_graph_init(int device, int32_t n_clouds, const double* const* xyz, const int64_t* n_pts,
                               int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud, const double* T_init,
                               int method, const se3icp_params* params, int32_t sharing, se3icp_result* results,
                               const se3icp_report_options* opts, se3icp_report* reports) {
    if (!xyz || (opts == nullptr) != (reports == nullptr)) return SE3ICP_ERR_INVALID_ARG;
    return graph_run(device, n_clouds, xyz, n_pts, false, n_pairs, src_cloud, tgt_cloud, method, params, sharing, results,
                     nullptr, opts != nullptr, opts, reports, T_init);
}

int se3icp_register_graph_init_device(int device, int32_t n_clouds, const double* d_xyz, const int64_t* off,
                                      int32_t n_pairs, const int32_t* src_cloud, const int32_t* tgt_cloud,
                                      const double* T_init, int method, const se3icp_params* params, int32_t sharing,
                                      se3icp_result* results, void* hip_stream, const se3icp_report_options* opts,
                                      se3icp_report* reports) {
    if ((opts == nullptr) != (reports == nullptr)) return SE3ICP_ERR_INVALID_ARG;
    std::vector<const double*> x;
    std::vector<int64_t> n;
    const int rc = cloud_ranges(n_clouds, d_xyz, off, x, n);
    if (rc) return rc;
    return graph_run(device, n_clouds, x.data(), n.data(), true, n_pairs, src_cloud, tgt_cloud, method, params, sharing,
                     results, hip_stream, opts != nullptr, opts, reports, T_init);
}

int se3icp_set_pose_seeding(int device, int mode) {
    if (mode < se3icp::kPoseSeedingMin || mode > se3icp::kPoseSeedingMax) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    e->set_pose_seeding(mode);
    return SE3ICP_OK;
}

int se3icp_last_init_stats(int device, int64_t* out, int n) {
    if (!out || n < se3icp::IS_COUNT) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    for (int k = 0; k < se3icp::IS_COUNT; ++k) out[k] = e->init_stats()[k];
    return SE3ICP_OK;
}

int se3icp_transform_points(const double* T, const double* xyz, int64_t n, double* out) {
    if (!T || n < 0 || (n > 0 && (!xyz || !out)) || !se3icp::pose_is_valid(T)) return SE3ICP_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n; ++i) se3icp::apply_pose(T, xyz + 3 * i, out + 3 * i);
    return SE3ICP_OK;
}

int se3icp_transform_device(int device, int32_t n_clouds, const double* d_xyz, const int64_t* off, const double* T,
                            double* d_out, void* hip_stream) {
    if (n_clouds <= 0 || n_clouds > 65535 || !d_xyz || !off || !T || !d_out) return SE3ICP_ERR_INVALID_ARG;
    for (int32_t c = 0; c < n_clouds; ++c)
        if (off[c + 1] < off[c] || !se3icp::pose_is_valid(T + 16 * (size_t)c)) return SE3ICP_ERR_INVALID_ARG;
    // in place, or apart: a partial overlap would have one block read what another has written
    if (d_out != d_xyz) {
        const double* lo = d_xyz + 3 * off[0];
        const double* hi = d_xyz + 3 * off[n_clouds];
        const double* olo = d_out + 3 * off[0];
        const double* ohi = d_out + 3 * off[n_clouds];
        if (olo < hi && lo < ohi) return SE3ICP_ERR_INVALID_ARG;
    }
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    return e->transform_device(n_clouds, d_xyz, off, T, d_out, (hipStream_t)hip_stream);
}

int se3icp_last_graph_stats(int device, int64_t* out, int n) {
    if (!out || n < GS_COUNT) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    for (int k = 0; k < GS_COUNT; ++k) out[k] = e->graph_stats()[k];
    return SE3ICP_OK;
}

int se3icp_set_batch_sharing(int device, int level) {
    if (level < se3icp::kBatchSharingMin || level > se3icp::kBatchSharingMax) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    e->set_batch_sharing(level);
    return SE3ICP_OK;
}

int se3icp_set_lrf_seeding(int device, int mode) {
    if (mode < se3icp::kLrfSeedingMin || mode > se3icp::kLrfSeedingMax) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    e->set_lrf_seeding(mode);
    return SE3ICP_OK;
}

int se3icp_last_seed_stats(int device, int64_t* out, int n) {
    if (!out || n < 4) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    for (int k = 0; k < 4; ++k) out[k] = e->seed_stats()[k];
    return SE3ICP_OK;
}

int se3icp_set_lrf_taking(int device, int mode) {
    if (mode < se3icp::kLrfTakingMin || mode > se3icp::kLrfTakingMax) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    e->set_lrf_taking(mode);
    return SE3ICP_OK;
}

int se3icp_last_take_stats(int device, int64_t* out, int n) {
    if (!out || n < se3icp::TS_COUNT) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    for (int k = 0; k < se3icp::TS_COUNT; ++k) out[k] = e->take_stats()[k];
    return SE3ICP_OK;
}

int se3icp_set_tree_sharing(int device, int mode) {
    if (mode < se3icp::kTreeSharingMin || mode > se3icp::kTreeSharingMax) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    e->set_tree_sharing(mode);
    return SE3ICP_OK;
}

int se3icp_last_tree_stats(int device, int64_t* out, int n) {
    if (!out || n < 4) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    for (int k = 0; k < 4; ++k) out[k] = e->tree_stats()[k];
    return SE3ICP_OK;
}

int se3icp_register(int device, const double* src_xyz, int64_t n_src, const double* tgt_xyz, int64_t n_tgt,
                    int method, const se3icp_params* params, se3icp_result* result) {
    return se3icp_register_batch(device, 1, &src_xyz, &n_src, &tgt_xyz, &n_tgt, method, params, result);
}

// ------------------------------------------------------------------ object surface
se3icp_registration* se3icp_registration_new(void) {
    auto* r = new (std::nothrow) se3icp_registration;
    if (!r) return nullptr;
    se3icp_default_params(&r->prm);
    std::memset(&r->res, 0, sizeof(r->res));
    for (int i = 0; i < 4; ++i) r->res.T[i * 4 + i] = 1.0;
    r->res.num_pure_se3_iterations = -1;  // ISR.cpp:338
    return r;
}

void se3icp_registration_free(se3icp_registration* r) { delete r; }

int se3icp_set_source_cloud(se3icp_registration* r, const double* xyz, int64_t n) {
    if (!r || (n > 0 && !xyz) || n < 0) return SE3ICP_ERR_INVALID_ARG;
    r->src.insert(r->src.end(), xyz, xyz + 3 * n);  // push_back, ISR.cpp:359-362
    return 0;
}

int se3icp_set_target_cloud(se3icp_registration* r, const double* xyz, int64_t n) {
    if (!r || (n > 0 && !xyz) || n < 0) return SE3ICP_ERR_INVALID_ARG;
    r->tgt.insert(r->tgt.end(), xyz, xyz + 3 * n);
    return 0;
}

se3icp_params* se3icp_params_of(se3icp_registration* r) { return r ? &r->prm : nullptr; }

static int run_object(se3icp_registration* r, int method) {
    const int64_t ns = (int64_t)r->src.size() / 3, nt = (int64_t)r->tgt.size() / 3;
    if (ns <= 0 || nt <= 0) return SE3ICP_ERR_EMPTY_CLOUD;
    const double* s = r->src.data();
    const double* t = r->tgt.data();
    se3icp_result res;
    se3icp_report rep;
    if (r->have_init) {
        // (a graph of the two clouds and the one edge: bitwise the batch, se3icp_register_graph)
        const double* const xyz[2] = {s, t};
        const int64_t n[2] = {ns, nt};
        const int32_t es = 0, et = 1;
        const int rc = se3icp_register_graph_init(current_device(), 2, xyz, n, 1, &es, &et, r->init, method, &r->prm, 0,
                                                  &res, r->want_report ? &r->ropts : nullptr,
                                                  r->want_report ? &rep : nullptr);
        if (rc == SE3ICP_OK || rc == SE3ICP_ERR_NONFINITE) {
            r->res = res;
            r->have_report = r->want_report;
            if (r->want_report) r->rep = rep;
        }
        return rc;
    }
    int rc = r->want_report ? se3icp_register_batch_report(current_device(), 1, &s, &ns, &t, &nt, method, &r->prm, &res,
                                                           &r->ropts, &rep)
                            : se3icp_register_batch(current_device(), 1, &s, &ns, &t, &nt, method, &r->prm, &res);
    if (rc == SE3ICP_OK || rc == SE3ICP_ERR_NONFINITE) {
        r->res = res;
        r->have_report = r->want_report;
        if (r->want_report) r->rep = rep;
    }
    return rc;
}

int se3icp_run_icp(se3icp_registration* r, const char* variant) {
    if (!r) return SE3ICP_ERR_INVALID_ARG;
    const int v = variant_index(variant);
    if (v < 0) {  // ISR.cpp:478-480
        std::cerr << "Invalid ICP variant name. Valid names are pt2pt, pt2pl and gicp.\n";
        return SE3ICP_ERR_INVALID_METHOD;
    }
    return run_object(r, SE3ICP_PT2PT + v);
}

int se3icp_run_se3_icp(se3icp_registration* r, const char* variant) {
    if (!r) return SE3ICP_ERR_INVALID_ARG;
    const int v = variant_index(variant);
    if (v < 0) {
        // ISR.cpp:561-563 then 700-703: one iteration, T_i never formed, loop breaks;
        // the de-normalized identity is [I | c_t - c_s].
        std::cerr << "Invalid variant name. Choose one of: pt2pt, pt2pl, gicp \n";
        std::cout << "Unknown optimization strategy for SE(3) \n";
        const int64_t ns = (int64_t)r->src.size() / 3, nt = (int64_t)r->tgt.size() / 3;
        if (ns <= 0 || nt <= 0) return SE3ICP_ERR_EMPTY_CLOUD;
        double cs[3] = {0, 0, 0}, ct[3] = {0, 0, 0};
        for (int64_t i = 0; i < ns; ++i)
            for (int a = 0; a < 3; ++a) cs[a] += r->src[3 * i + a];
        for (int64_t i = 0; i < nt; ++i)
            for (int a = 0; a < 3; ++a) ct[a] += r->tgt[3 * i + a];
        std::memset(r->res.T, 0, sizeof(r->res.T));
        for (int a = 0; a < 4; ++a) r->res.T[a * 4 + a] = 1.0;
        for (int a = 0; a < 3; ++a) r->res.T[a * 4 + 3] = ct[a] / (double)nt - cs[a] / (double)ns;
        r->res.num_iterations = 1;
        r->res.num_pure_se3_iterations = 1;
        r->res.status = SE3ICP_ERR_INVALID_METHOD;
        return SE3ICP_ERR_INVALID_METHOD;
    }
    return run_object(r, SE3ICP_SE3_PT2PT + v);
}

int se3icp_run_se3_icp_with_cf(se3icp_registration* r) {
    if (!r) return SE3ICP_ERR_INVALID_ARG;
    const int rc = run_object(r, SE3ICP_SE3_GICP_WITH_CF);
    if (rc == SE3ICP_OK || rc == SE3ICP_ERR_NONFINITE)  // ISR.cpp:794 (printed once the run returns)
        std::cout << "### scaling factor = " << r->res.scaling_factor << std::endl;
    return rc;
}

int se3icp_run_se3_pure(se3icp_registration* r, const char* variant) {
    if (!r) return SE3ICP_ERR_INVALID_ARG;
    const int v = variant_index(variant);
    if (v < 0) {
        std::cerr << "Invalid variant name. Choose one of: pt2pt, pt2pl, gicp \n";
        return SE3ICP_ERR_INVALID_METHOD;
    }
    const int rc = run_object(r, SE3ICP_SE3_PURE_PT2PT + v);
    if (rc == SE3ICP_OK || rc == SE3ICP_ERR_NONFINITE) std::cout << "pure se3 finished" << std::endl;  // ISR.cpp:1127
    return rc;
}

int se3icp_set_initial_transform(se3icp_registration* r, const double* T) {
    if (!r) return SE3ICP_ERR_INVALID_ARG;
    if (!T) {
        r->have_init = false;
        return 0;
    }
    if (!se3icp::pose_is_valid(T)) return SE3ICP_ERR_INVALID_ARG;
    std::memcpy(r->init, T, sizeof(r->init));
    r->have_init = true;
    return 0;
}

int se3icp_get_result(const se3icp_registration* r, se3icp_result* out) {
    if (!r || !out) return SE3ICP_ERR_INVALID_ARG;
    *out = r->res;
    return 0;
}

int se3icp_request_report(se3icp_registration* r, const se3icp_report_options* opts) {
    if (!r) return SE3ICP_ERR_INVALID_ARG;
    if (!opts) {
        r->want_report = false;
        return 0;
    }
    if (std::isnan(opts->max_correspondence_distance) || opts->outputs_on_device) return SE3ICP_ERR_INVALID_ARG;
    r->ropts = *opts;
    r->want_report = true;
    return 0;
}

int se3icp_get_report(const se3icp_registration* r, se3icp_report* out) {
    if (!r || !out || !r->have_report) return SE3ICP_ERR_INVALID_ARG;
    *out = r->rep;
    return 0;
}

// ------------------------------------------------------------------ stage surface
int se3icp_toldi_frames(int device, const double* xyz, int64_t n, int k, double* frames) {
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    return e->toldi_frames(xyz, n, k, frames);
}

int se3icp_knn_self(int device, const double* xyz, int64_t n, int k, int32_t* idx) {
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    return e->knn_self(xyz, n, k, idx);
}

int se3icp_estimate_normals(int device, const double* xyz, int64_t n, int k, double* normals) {
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    return e->estimate_normals(xyz, n, k, normals);
}

int se3icp_nn(int device, const double* query, int64_t nq, const double* data, int64_t nd, int dim, int32_t* idx,
              double* d2, int32_t* num_rechecked) {
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    return e->nn(query, nq, data, nd, dim, idx, d2, num_rechecked);
}

// The loop's NN prep and search over a given pose sequence (diagnostic).
// Arguments are checked before the device is looked up.
int se3icp_nn_sequence_version(void) { return 1; }

int se3icp_nn_sequence(int device, const double* query, int64_t nq, const double* data, int64_t nd, int dim,
                       double alpha, int32_t n_steps, const double* poses, int32_t restart_at, int32_t* idx,
                       float* dist, float* cert_d1, float* cert_l2, int32_t* cert_iter, int32_t* cert_j,
                       int32_t* searched, int32_t* single, int32_t* rechecked) {
    if (!query || !data || !poses || (dim != 3 && dim != 12) || n_steps <= 0 || !std::isfinite(alpha))
        return SE3ICP_ERR_INVALID_ARG;
    if (restart_at < 0 || restart_at > n_steps) return SE3ICP_ERR_INVALID_ARG;
    for (int32_t k = 0; k < n_steps; ++k)
        if (!se3icp::pose_is_valid(poses + 16 * (size_t)k)) return SE3ICP_ERR_INVALID_ARG;
    if (nq <= 0 || nd <= 0) return SE3ICP_ERR_EMPTY_CLOUD;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    const Engine::NNSequenceOut out{idx, dist, cert_d1, cert_l2, cert_iter, cert_j, searched, single, rechecked};
    return e->nn_sequence(query, nq, data, nd, dim, alpha, n_steps, poses, restart_at, out);
}

// ------------------------------------------------------------------ voxel-grid downsample
// Arguments are checked before the device is looked up, as the sweeps' are (voxel.hpp).
int se3icp_voxel_version(void) { return 1; }

int se3icp_voxel_downsample_device(int device, int32_t n_clouds, const double* d_xyz, const int64_t* off,
                                   const double* voxel_size, double* d_out, int64_t* out_off, int32_t* d_count,
                                   int32_t* d_first, void* hip_stream) {
    const int rc = se3icp::voxel_check_sizes(n_clouds, off, voxel_size, SE3ICP_ERR_INVALID_ARG, SE3ICP_ERR_EMPTY_CLOUD);
    if (rc) return rc;
    if (!d_xyz || !d_out || !out_off) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    return e->voxel_downsample(n_clouds, d_xyz, off, voxel_size, d_out, out_off, d_count, d_first,
                               (hipStream_t)hip_stream);
}

int64_t se3icp_voxel_downsample(int device, const double* xyz, int64_t n, double voxel_size, double* out,
                                int32_t* count, int32_t* first) {
    const int64_t off[2] = {0, n};
    if (n < 0) return SE3ICP_ERR_INVALID_ARG;
    const int rc = se3icp::voxel_check_sizes(1, off, &voxel_size, SE3ICP_ERR_INVALID_ARG, SE3ICP_ERR_EMPTY_CLOUD);
    if (rc) return rc;
    if (!xyz) return SE3ICP_ERR_INVALID_ARG;
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    int64_t n_out = 0;
    const int rc2 = e->voxel_downsample_host(xyz, n, voxel_size, out, count, first, &n_out);
    return rc2 ? rc2 : n_out;
}

// ------------------------------------------------------------------ profiling hooks (not part of the
// reference boundary; used by bench.py to read the per-kernel HIP-event times of the last batch)
int se3icp_set_profiling(int device, int on) {
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    e->set_profiling(on != 0);
    return 0;
}

int se3icp_set_trace(int device, se3icp_trace* trace) {
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    if (trace && (trace->max_iters < 0 || trace->pair < 0)) return SE3ICP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mutex());
    e->set_trace(trace);
    return 0;
}

int se3icp_setup_record_version(void) { return 1; }

int se3icp_set_setup_record(int device, se3icp_setup_record* rec) {
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    if (rec && (rec->pair < 0 || rec->src.cap < 0 || rec->tgt.cap < 0)) return SE3ICP_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(e->mutex());
    e->set_setup_record(rec);
    return 0;
}

int se3icp_tree_record_version(void) { return 1; }

int se3icp_set_tree_record(int device, se3icp_tree_record* rec) {
    if (rec) {  // (the arguments before the device: a bad record is reported on any machine)
        if (rec->pair < 0) return SE3ICP_ERR_INVALID_ARG;
        for (const se3icp_tree_side* t : {&rec->src3, &rec->tgt3, &rec->src12, &rec->tgt12})
            if (t->cap < 0 || t->node_cap < 0) return SE3ICP_ERR_INVALID_ARG;
    }
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    e->set_tree_record(rec);
    return 0;
}

int se3icp_set_lrf_exact(int device, int exact_only) {
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    if (exact_only < 0 || exact_only > 2) return SE3ICP_ERR_INVALID_ARG;
    e->set_lrf_exact(exact_only);
    return 0;
}

int se3icp_set_nn_events(int device, int on) {
    Engine* e = usable_engine(device);
    if (!e) return SE3ICP_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(e->mutex());
    e->set_nn_events(on != 0);
    return 0;
}

int se3icp_last_kernel_times(int device, double* out /* [24] */) {
    double x[SE3ICP_KERNEL_TIMES_N];
    const int rc = se3icp_last_kernel_times_n(device, x, SE3ICP_KERNEL_TIMES_N);
    if (rc == 0)
        for (int i = 0; i < 24; ++i) out[i] = x[i];
    return rc;
}

int se3icp_last_kernel_times_n(int device, double* out, int n) {
    Engine* e = usable_engine(device);
    if (!e || !out) return SE3ICP_ERR_NO_DEVICE;
    if (n < SE3ICP_KERNEL_TIMES_N) return SE3ICP_ERR_INVALID_ARG;
    const auto& k = e->kernel_times();
    out[0] = k.nn_se3_ms;
    out[1] = k.nn_r3_ms;
    out[2] = k.recheck_ms;
    out[3] = k.trim_ms;
    out[4] = k.reduce_ms;
    out[5] = k.setup_ms;
    out[6] = (double)k.nn_se3_launches;
    out[7] = (double)k.nn_r3_launches;
    out[8] = k.se3_dist_evals;
    out[9] = k.se3_box_tests;
    out[10] = k.r3_dist_evals;
    out[11] = k.r3_box_tests;
    out[12] = k.lrf_ms;
    out[13] = k.lrf_queries;
    out[14] = k.lrf_leaves;
    out[15] = k.lrf_merges;
    out[16] = k.lrf_box_tests;
    out[17] = k.lrf_candidates;
    out[18] = k.nn_prep_ms;
    out[19] = k.se3_queries;
    out[20] = k.se3_searched;
    out[21] = k.r3_queries;
    out[22] = k.r3_searched;
    out[23] = k.lrf_fallback;
    out[24] = k.se3_useful_evals;
    out[25] = k.r3_useful_evals;
    return 0;
}

}  // extern "C"
