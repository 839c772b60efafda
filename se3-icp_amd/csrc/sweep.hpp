// sweep.hpp — host-side planning of a parameter sweep (Engine::register_sweep) and the
// launcher of k_sweep.hip.
//
// A sweep registers the same P pairs under V parameter sets ("variants") that share the
// setup: ingest, normalization, 3-D kd-trees, kNN / TOLDI / normals run once over the 2P base
// clouds, with alpha = beta = 1.  The variants then run in groups of G: a group is one batch
// of G * P virtual pairs whose clouds are the base clouds (the group's first variant) and
// G - 1 replicas laid out behind them, replica v at point offset v * N (N: points of the
// base batch).  This header holds the group rule, which needs no device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace se3icp {

// Device bytes the engine holds per point slot of a batch: the per-point arrays of
// alloc_points (436 B), the kd-tree buffers build_tree adds (3-D 68 B, 12-D 120 B), the
// loop's query lists and the tree build's scratch (~40 B), all times the 1.25 growth
// factor of Engine::ensure, rounded up.
constexpr int64_t kSweepBytesPerPoint = 896;
// Device bytes per cloud: node boxes of both trees (f32 and build scratch), at most
// 2^(L+1) nodes of >= 32 points each; tables.  Small against the points for real clouds.
constexpr int64_t kSweepBytesPerCloud = 64 * 1024;
// What the engine picks on its own (max_group = 0), from the measured sweeps (DESIGN.md
// "Parameter sweeps", profiles/sweep_bench.json): more variants in lockstep were faster up
// to the 8 measured while a group stayed within ~2^26 points (8 x 2.0 M points: 0.47 of the
// separate calls against 0.79 at G = 1), and slower beyond (15.7 M points a variant: 0.61 at
// G = 4, 62.8 M points a group, 0.65 at G = 8).
constexpr int kSweepAutoMax = 8;
constexpr int64_t kSweepAutoPoints = (int64_t)1 << 26;
constexpr int64_t kSweepPointLimit = (int64_t)1 << 30;  // Engine::alloc_points

// Variants registered in lockstep at once.
//   n_variants >= 1; max_group: the caller's bound (0: none); points / clouds: of the base
//   batch; budget_bytes: device memory the sweep may fill (free memory plus what the engine
//   already holds).
// Rule: the largest G with  G <= n_variants,  G <= max_group (when given),
// G * points < 2^30,  G * (points * bytes_per_point + clouds * bytes_per_cloud) <= budget,
// and -- when the caller leaves it to the engine -- G <= kSweepAutoMax and
// G * points <= kSweepAutoPoints.  Never below 1: a batch that does not fit alone fails in
// the allocation as a plain batch would.  The groups are then balanced: with
// n = ceil(V / G) groups, G becomes ceil(V / n).
inline int sweep_group_size(int n_variants, int max_group, int64_t points, int64_t clouds, int64_t bytes_per_point,
                            int64_t bytes_per_cloud, int64_t budget_bytes) {
    int64_t g = std::max(1, n_variants);
    if (max_group > 0) g = std::min<int64_t>(g, max_group);
    const int64_t pts = std::max<int64_t>(points, 1);
    g = std::min(g, (kSweepPointLimit - 1) / pts);
    const int64_t per = pts * bytes_per_point + std::max<int64_t>(clouds, 0) * bytes_per_cloud;
    g = std::min(g, std::max<int64_t>(budget_bytes, 0) / std::max<int64_t>(per, 1));
    if (max_group <= 0) g = std::min<int64_t>(std::min<int64_t>(g, kSweepAutoMax), kSweepAutoPoints / pts);
    g = std::max<int64_t>(g, 1);
    const int64_t ngroups = (n_variants + g - 1) / g;
    g = (n_variants + ngroups - 1) / ngroups;
    return (int)std::max<int64_t>(g, 1);
}

// Group k of a sweep of n_variants at group size G: variants [first, first + count).
inline void sweep_group(int n_variants, int G, int k, int* first, int* count) {
    *first = k * G;
    *count = std::max(0, std::min(G, n_variants - k * G));
}
inline int sweep_num_groups(int n_variants, int G) { return (n_variants + G - 1) / G; }

// ---- k_sweep.hip
struct View;
struct SweepWeight { double alpha, beta; };
struct SweepArgs {
    int32_t g;          // variants of this group (>= 1)
    int32_t n;          // points of the base batch (replica v starts at slot v * n)
    int32_t nclouds;    // base clouds (2 P)
    int32_t nnodes3;    // heap slots per cloud of the 3-D trees
    int32_t frames;     // the method has SE(3) frames (rows to weight)
    int32_t cf;         // run_se3_icp_with_cf: targets' f32 translation from the raw point
    const double* raw;  // [n][12] unweighted rows of the shared setup
    const SweepWeight* w;  // [g] device table
    double* scales;     // [g * P] normalization scales (entries >= P written here), or null
    double4* tpt64;     // 3-D trees' point records (writable alias of View::t3.tpt64)
    int32_t* perm3;     // ... and of the other tree arrays the replicas receive
    int32_t* pos3;
    float* tvec3;
    double* tvec64_3;
    float* lo3;
    float* hi3;
};
void launch_sweep_expand(const View& v, const SweepArgs& a, hipStream_t s);

}  // namespace se3icp
