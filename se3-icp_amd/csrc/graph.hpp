// graph.hpp — host-side planning of a registration over a shared cloud set
// (Engine::register_graph) and the launchers of k_graph.hip.
//
// A graph call names C distinct clouds and P edges; edge p registers cloud src[p] onto cloud
// tgt[p].  The loop understands a batch of 2P "use" clouds laid out src 0, tgt 0, src 1, ...
// (use 2p + side), so a cloud that several edges name is materialised once per use -- the
// saving is upload and setup compute, not memory.  What the uses of a cloud can share depends
// on how the edge normalizes it (ISR.cpp:568-582): every use has the cloud's own centroid, but
// the scale is the pair's, scale_pre * (1 / max(r_src, r_tgt)), and the vanilla methods centre
// their f32 copy on the pair's target.  A CLASS is a cloud under one such normalization:
// (cloud, bits of norm_scale, bits of f32_center).  Uses of one class are bitwise the same
// cloud to every setup kernel, so the class's neighbour selection, frames and normals -- the
// bulk of the setup -- run once, at its first use, and are copied to the others.
// The device batch entries find the slots that hold one cloud by content and plan the same
// classes over them (share_candidates, share_clouds, graph_plan_uses below).
// This header holds the plan, which needs no device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "view.hpp"

namespace se3icp {

// sharing levels of se3icp_register_graph
constexpr int kGraphSharingMin = 0, kGraphSharingMax = 3;
// se3icp_last_graph_stats
enum GraphStat : int {
    GS_CLOUDS = 0,      // distinct clouds some edge uses
    GS_USES,            // 2 * edges
    GS_CLASSES,
    GS_FULL,            // classes that ran a full neighbour selection
    GS_ADOPTED,         // queries whose neighbour set was adopted from another class
    GS_REJ_ORDER,       // ... rejected by the order check
    GS_REJ_GAP,         // ... rejected by the gap check
    GS_NO_LIST,         // ... without a list to adopt
    GS_BYTES_UPLOADED,
    GS_COUNT
};

// The pair's normalization scale exactly as k_pair_scales forms it (k_setup.hip).
inline double graph_pair_scale(double scale_pre, double r_src, double r_tgt) {
    const double rmax = std::fmax(r_src, r_tgt);
    return scale_pre * (1.0 / rmax);
}

struct GraphClass {
    int32_t cloud;          // index into the call's cloud array
    int32_t k_nrm;          // the largest EstimateNormals k of its uses
    int32_t n_uses;
    int32_t nrm_from;       // the class whose kNN / normals this one takes (itself: it runs its own)
    double norm_center[3];
    double norm_scale;
    double f32_center[3];
};

struct GraphPlan {
    std::vector<int32_t> use_class;  // [2P]: class of use 2p (source) and 2p + 1 (target)
    std::vector<GraphClass> classes; // in order of first use
    bool normalize = false, dedupe = false;  // as graph_plan_uses was asked
};

// A use as the planner sees it: its cloud, the EstimateNormals k it asks for and the
// normalization it runs under.
struct GraphUse {
    int32_t cloud;
    int32_t k_nrm;
    double norm_center[3];
    double norm_scale;
    double f32_center[3];
};

// Plan the classes of uses 0 .. n_uses - 1 (use 2p the source of pair p, 2p + 1 its target).
// A class is (cloud, bits of norm_center, norm_scale and f32_center).
//   normalize: the run_se3_* preprocessing; otherwise raw coordinates with only the f32 copy
//              centred.
//   dedupe:    false gives every use a class of its own (sharing level 1).
// Without normalization the classes of a cloud differ only in the centre of their f32 copy:
// the exact kNN and the normals are the same bits, so the cloud's first class with normals
// computes them (nrm_from) and the others copy.
inline void graph_plan_uses(int32_t n_uses, const GraphUse* use, bool normalize, bool dedupe, GraphPlan* plan) {
    struct Key {
        int32_t cloud;
        uint64_t b[7];
        bool operator<(const Key& o) const {
            if (cloud != o.cloud) return cloud < o.cloud;
            return std::memcmp(b, o.b, sizeof(b)) < 0;
        }
    };
    std::map<Key, int32_t> seen;
    plan->use_class.assign((size_t)n_uses, -1);
    plan->classes.clear();
    plan->normalize = normalize;
    plan->dedupe = dedupe;
    for (int32_t u = 0; u < n_uses; ++u) {
        GraphClass g{};
        g.cloud = use[u].cloud;
        g.k_nrm = use[u].k_nrm;
        g.n_uses = 1;
        g.norm_scale = use[u].norm_scale;
        for (int a = 0; a < 3; ++a) {
            g.norm_center[a] = use[u].norm_center[a];
            g.f32_center[a] = use[u].f32_center[a];
        }
        Key k{};
        k.cloud = g.cloud;
        std::memcpy(&k.b[0], &g.norm_scale, 8);
        std::memcpy(&k.b[1], g.f32_center, 24);
        std::memcpy(&k.b[4], g.norm_center, 24);
        int32_t id = -1;
        if (dedupe) {
            auto it = seen.find(k);
            if (it != seen.end()) id = it->second;
        }
        if (id < 0) {
            id = (int32_t)plan->classes.size();
            plan->classes.push_back(g);
            if (dedupe) seen[k] = id;
        } else {
            GraphClass& h = plan->classes[id];
            h.k_nrm = h.k_nrm > g.k_nrm ? h.k_nrm : g.k_nrm;
            h.n_uses++;
        }
        plan->use_class[u] = id;
    }
    std::map<int32_t, int32_t> owner;  // cloud -> its first class with normals
    for (int32_t k = 0; k < (int32_t)plan->classes.size(); ++k) {
        GraphClass& g = plan->classes[k];
        g.nrm_from = k;
        if (normalize || !dedupe || g.k_nrm <= 0) continue;
        auto it = owner.find(g.cloud);
        if (it == owner.end()) owner[g.cloud] = k;
        else if (plan->classes[it->second].k_nrm == g.k_nrm) g.nrm_from = it->second;
    }
}

// ---- seeding the selection of a cloud's later classes (Engine::select_by_class, k_lrf8.hip)
// Under the run_se3_* normalization the classes of one cloud are fl(fl(p - c) * s) of the same
// fl(p - c) for different pair scales s, so every squared distance in class b is
// (s_b / s_a)^2 times class a's up to f64 rounding.  The cloud's first selecting class (the
// source) stores every point's Kw-th neighbour distance and a later class starts its own, full
// and self-certifying selection from rho2 times that instead of from infinity.
// se3icp_set_lrf_seeding
constexpr int kLrfSeedingMin = 0, kLrfSeedingMax = 3;
struct SeedClass {
    int32_t from;  // the class whose stored distances seed this one (-1: selects unseeded)
    double rho2;   // (own norm_scale / the source's)^2
};
// k_knn [classes]: the neighbours the class's selection asks for (0: it selects nothing);
// n_pts [classes]: the points of its cloud.  Per cloud the first class that selects is the
// source; a later class is seeded from it when it selects, was centred with the same bits, has
// its f32 copy uncentred (as the source has) and asks for no more neighbours, Kw = min(k_knn, n),
// than the source found.  Nothing is seeded without the normalization or with a class per use
// (sharing level 1).  Returns the seeded classes.
inline int32_t graph_plan_seeds_posed(const GraphPlan& plan, const int32_t* k_knn, const int64_t* n_pts,
                                      const int32_t* raw, const int32_t* rigid, bool cross,
                                      std::vector<SeedClass>* seed, int32_t* n_cross);
inline int32_t graph_plan_seeds(const GraphPlan& plan, const int32_t* k_knn, const int64_t* n_pts,
                                std::vector<SeedClass>* seed) {
    int32_t nv = 0;  // every cloud its own, unposed, variant (graph_plan_seeds_posed)
    for (const GraphClass& g : plan.classes) nv = std::max(nv, g.cloud + 1);
    std::vector<int32_t> raw((size_t)nv), rigid((size_t)nv, 1);
    for (int32_t v = 0; v < nv; ++v) raw[v] = v;
    return graph_plan_seeds_posed(plan, k_knn, n_pts, raw.data(), rigid.data(), true, seed, nullptr);
}

// ---- taking the source's neighbour lists
// A seeded class whose selecting slot has the 3-D tree order of its source's selecting slot names
// every point by the same local tree slot, so it can take the source's Kw neighbours as a list
// and only re-check them under its own scale.  se3icp_set_lrf_taking
constexpr int kLrfTakingMin = 0, kLrfTakingMax = 2;
enum TakeStat : int { TS_CLASSES = 0, TS_TAKEN, TS_REDONE, TS_FAILED, TS_COUNT };
// seed [classes]: graph_plan_seeds' (or graph_plan_seeds_posed's) result; k_knn, n_pts as there;
// home [classes]: the slot that selects for the class; donor: graph_plan_trees' table over the
// slots (empty: no slot adopted an order).  take[k] != 0: class k takes from seed[k].from.  It
// does when it is seeded, is a class of the same cloud (variant) as its source, asks for exactly
// as many neighbours, Kw = min(k_knn, n), and both home slots are the builder or adopters of one
// donor group.  Returns the taking classes.
inline int32_t graph_plan_takes(const GraphPlan& plan, const std::vector<SeedClass>& seed, const int32_t* k_knn,
                                const int64_t* n_pts, const int32_t* home, const std::vector<int32_t>& donor,
                                std::vector<uint8_t>* take) {
    const int32_t K = (int32_t)plan.classes.size();
    take->assign((size_t)K, 0);
    if (!plan.normalize || !plan.dedupe || (int32_t)seed.size() != K || donor.empty()) return 0;
    const int32_t U = (int32_t)donor.size();
    auto group = [&](int32_t u) { return (u < 0 || u >= U) ? -1 : (donor[u] >= 0 ? donor[u] : u); };
    int32_t taking = 0;
    for (int32_t k = 0; k < K; ++k) {
        const int32_t a = seed[k].from;
        if (a < 0 || a >= K || a == k) continue;
        const int64_t kw = k_knn[k] < n_pts[k] ? k_knn[k] : n_pts[k], kwa = k_knn[a] < n_pts[a] ? k_knn[a] : n_pts[a];
        const int32_t gk = group(home[k]), ga = group(home[a]);
        if (plan.classes[k].cloud != plan.classes[a].cloud || n_pts[k] != n_pts[a] || kw != kwa || kw <= 0 || gk < 0 ||
            gk != ga)
            continue;
        (*take)[k] = 1;
        ++taking;
    }
    return taking;
}

// ---- initial poses (se3icp_register_graph_init, pose.hpp)
// A VARIANT is a cloud under one initial pose: (cloud, the 128 bytes of the pose).  The unposed
// variant of a cloud is the cloud itself; a pose that is bitwise the identity means "no pose".
// Everything behind the ingest treats a variant as a cloud of its own: classes, tree orders and
// seeds are planned over variants (GraphClass::cloud is then a variant).
// se3icp_set_pose_seeding
constexpr int kPoseSeedingMin = 0, kPoseSeedingMax = 1;
enum InitStat : int { IS_EDGES = 0, IS_VARIANTS, IS_CROSS_SEEDED, IS_COUNT };
struct VariantPlan {
    std::vector<int32_t> edge_src, edge_tgt;  // [P]: the variant of an edge's source / target
    std::vector<int32_t> cloud;               // [V]: its raw cloud
    std::vector<int32_t> pose_edge;           // [V]: the first edge that carries its pose (-1: unposed)
    int32_t posed_edges = 0, posed_variants = 0;
};
// Variants are numbered in order of first use (edge 0's source, edge 0's target, edge 1's
// source, ...).  T_init: P row-major 4x4 poses, or null (no edge is posed).  Only a source is
// ever posed; -0.0 is not +0.0, so a pose with a -0.0 where another has +0.0 is another variant.
inline void graph_plan_variants(int32_t n_pairs, const int32_t* src, const int32_t* tgt, const double* T_init,
                                VariantPlan* vp) {
    static const double ident[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    struct Key {
        int32_t cloud;
        int32_t posed;
        uint64_t b[16];
        bool operator<(const Key& o) const {
            if (cloud != o.cloud) return cloud < o.cloud;
            if (posed != o.posed) return posed < o.posed;
            return std::memcmp(b, o.b, sizeof(b)) < 0;
        }
    };
    std::map<Key, int32_t> seen;
    vp->edge_src.assign((size_t)n_pairs, -1);
    vp->edge_tgt.assign((size_t)n_pairs, -1);
    vp->cloud.clear();
    vp->pose_edge.clear();
    vp->posed_edges = vp->posed_variants = 0;
    for (int32_t p = 0; p < n_pairs; ++p)
        for (int side = 0; side < 2; ++side) {
            Key k{};
            k.cloud = side == 0 ? src[p] : tgt[p];
            const double* M = (side == 0 && T_init) ? T_init + 16 * (size_t)p : nullptr;
            if (M && std::memcmp(M, ident, sizeof(ident)) == 0) M = nullptr;
            if (M) {
                k.posed = 1;
                std::memcpy(k.b, M, sizeof(k.b));
                vp->posed_edges++;
            }
            auto it = seen.find(k);
            int32_t id;
            if (it == seen.end()) {
                id = (int32_t)vp->cloud.size();
                seen[k] = id;
                vp->cloud.push_back(k.cloud);
                vp->pose_edge.push_back(M ? p : -1);
                vp->posed_variants += M ? 1 : 0;
            } else {
                id = it->second;
            }
            (side == 0 ? vp->edge_src : vp->edge_tgt)[p] = id;
        }
}

// graph_plan_seeds for a plan over variants.  Under the run_se3_* normalization a rigid pose
// preserves distances up to rounding, so the first selecting class of any rigid variant of a raw
// cloud (the unposed one counts as rigid) seeds the later classes of every rigid variant of that
// cloud; a variant whose pose is not rigid seeds within itself only, as does every variant with
// cross = false (se3icp_set_pose_seeding(1)).  The conditions are graph_plan_seeds' except that
// "centred with the same bits" is asked only between classes of one variant.
// raw [variants]: the raw cloud of a variant; rigid [variants]: pose_is_rigid of its pose (nonzero
// for the unposed variant).  *n_cross: the classes seeded from another variant's.  With every
// variant unposed the result is graph_plan_seeds'.
inline int32_t graph_plan_seeds_posed(const GraphPlan& plan, const int32_t* k_knn, const int64_t* n_pts,
                                      const int32_t* raw, const int32_t* rigid, bool cross,
                                      std::vector<SeedClass>* seed, int32_t* n_cross) {
    const int32_t K = (int32_t)plan.classes.size();
    seed->assign((size_t)K, SeedClass{-1, 1.0});
    if (n_cross) *n_cross = 0;
    if (!plan.normalize || !plan.dedupe) return 0;
    auto uncentred = [](const GraphClass& g) { return g.f32_center[0] == 0.0 && g.f32_center[1] == 0.0 && g.f32_center[2] == 0.0; };
    // (raw cloud, -1) for the rigid variants of a cloud together, (raw cloud, variant) otherwise
    std::map<std::pair<int32_t, int32_t>, int32_t> source;
    int32_t seeded = 0;
    for (int32_t k = 0; k < K; ++k) {
        if (k_knn[k] <= 0) continue;
        const GraphClass& g = plan.classes[k];
        const int32_t v = g.cloud;
        const std::pair<int32_t, int32_t> key{raw[v], (cross && rigid[v]) ? -1 : v};
        auto it = source.find(key);
        if (it == source.end()) {
            source[key] = k;
            continue;
        }
        const int32_t a = it->second;
        const GraphClass& ga = plan.classes[a];
        const int64_t kw = k_knn[k] < n_pts[k] ? k_knn[k] : n_pts[k], kwa = k_knn[a] < n_pts[a] ? k_knn[a] : n_pts[a];
        const double rho = g.norm_scale / ga.norm_scale;
        const bool same_variant = ga.cloud == v;
        if ((same_variant && std::memcmp(g.norm_center, ga.norm_center, sizeof(g.norm_center)) != 0) || !uncentred(g) ||
            !uncentred(ga) || n_pts[k] != n_pts[a] || kw > kwa || !(rho > 0.0) || !std::isfinite(rho * rho))
            continue;
        (*seed)[k] = SeedClass{a, rho * rho};
        ++seeded;
        if (!same_variant && n_cross) ++*n_cross;
    }
    return seeded;
}

// ---- one kd-tree order per cloud (build_trees, k_tree.hip)
// The trees are implicit and balanced: node ranges come from the point count alone, every search
// prunes on boxes computed from the points actually in a node, and no result depends on the
// order.  So the later slots of a cloud take the order its first slot built and
// compute only their own tree-ordered vectors and boxes.
// se3icp_set_tree_sharing
constexpr int kTreeSharingMin = 0, kTreeSharingMax = 1;
// cloud [n_slots]: the confirmed cloud of every slot (byte-compared in a device batch, named by
// the caller in a graph), or negative for a slot nothing is known about; n_pts [n_slots].
// donor[u]: -1 where slot u builds its trees, otherwise the first slot of its cloud, whose
// order it adopts -- whatever its class.  A slot adopts only from a slot of the same cloud and
// point count.  share = false (sharing level 1, tree sharing off): every slot builds.  The
// table serves the 3-D trees, and the 12-D trees of a method with an SE(3) phase.  Returns the
// adopters.
inline int32_t graph_plan_trees(int32_t n_slots, const int32_t* cloud, const int64_t* n_pts, bool share,
                                std::vector<int32_t>* donor) {
    donor->assign((size_t)n_slots, -1);
    if (!share) return 0;
    std::map<int32_t, int32_t> first;  // cloud -> its first slot
    int32_t adopters = 0;
    for (int32_t u = 0; u < n_slots; ++u) {
        if (cloud[u] < 0) continue;
        auto it = first.find(cloud[u]);
        if (it == first.end()) {
            first[cloud[u]] = u;
        } else if (n_pts[it->second] == n_pts[u]) {
            (*donor)[u] = it->second;
            ++adopters;
        }
    }
    return adopters;
}

// Plan the classes of P edges over clouds the caller names.
//   normalize: centre on the own centroid, scale by the pair; otherwise the f32 copy is centred
//              on the edge's target.
//   center [3 * n_clouds], radius [n_clouds]: GetCenter and the largest |p - center| of every
//              cloud an edge uses (radius is read only when normalize).
inline void graph_plan(int32_t n_pairs, const int32_t* src, const int32_t* tgt, bool normalize, double scale_pre,
                       const double* center, const double* radius, int k_nrm_src, int k_nrm_tgt, bool dedupe,
                       GraphPlan* plan) {
    std::vector<GraphUse> use(2 * (size_t)n_pairs);
    for (int32_t p = 0; p < n_pairs; ++p) {
        const double scale = normalize ? graph_pair_scale(scale_pre, radius[src[p]], radius[tgt[p]]) : 1.0;
        for (int side = 0; side < 2; ++side) {
            const int32_t c = side == 0 ? src[p] : tgt[p];
            GraphUse& g = use[2 * (size_t)p + side];
            g.cloud = c;
            g.k_nrm = side == 0 ? k_nrm_src : k_nrm_tgt;
            g.norm_scale = scale;
            for (int a = 0; a < 3; ++a) {
                g.norm_center[a] = normalize ? center[3 * c + a] : 0.0;
                g.f32_center[a] = normalize ? 0.0 : center[3 * tgt[p] + a];
            }
        }
    }
    graph_plan_uses(2 * n_pairs, use.data(), normalize, dedupe, plan);
}

// ---- content-detected sharing of a device batch (Engine::setup_pairs_shared)
// The device batch entries take 2P cloud slots and cannot be told that two of them hold the
// same scan, so they look: every slot's raw xyz bytes are hashed on the device (k_share_hash,
// 64 bits, keyed with the point count), slots of equal (n, hash) are candidates, and a
// candidate shares only after a byte-for-byte device compare against the first slot of its
// group (k_share_compare).  Never by pointer, never by batch position.
// se3icp_set_batch_sharing
constexpr int kBatchSharingMin = 0, kBatchSharingMax = 2;

// Two slots of the same point count: without one there is nothing to hash.
inline bool share_any_equal_n(int32_t n_slots, const int64_t* n) {
    std::map<int64_t, int32_t> seen;
    for (int32_t u = 0; u < n_slots; ++u)
        if (++seen[n[u]] > 1) return true;
    return false;
}

// first[u]: the first slot with u's (n, hash) -- u itself where none precedes it.  Returns the
// number of slots with first[u] != u: the compares to run.
inline int32_t share_candidates(int32_t n_slots, const int64_t* n, const uint64_t* hash, std::vector<int32_t>* first) {
    std::map<std::pair<int64_t, uint64_t>, int32_t> seen;
    first->assign((size_t)n_slots, -1);
    int32_t cand = 0;
    for (int32_t u = 0; u < n_slots; ++u) {
        auto it = seen.find({n[u], hash[u]});
        if (it == seen.end()) {
            seen[{n[u], hash[u]}] = u;
            (*first)[u] = u;
        } else {
            (*first)[u] = it->second;
            ++cand;
        }
    }
    return cand;
}

// cloud[u]: the distinct cloud slot u holds, numbered in order of first slot.  same[u] (read
// where first[u] != u): nonzero iff the compare found u's bytes equal to first[u]'s.  A
// hash-equal slot that the compare did not confirm is a cloud of its own -- also against a
// later slot of its group, which was compared with the group's first slot only: a sharing
// missed (after a 64-bit collision), never one made on the hash alone.  Returns the clouds.
inline int32_t share_clouds(int32_t n_slots, const int32_t* first, const int32_t* same, std::vector<int32_t>* cloud) {
    cloud->assign((size_t)n_slots, -1);
    int32_t nc = 0;
    for (int32_t u = 0; u < n_slots; ++u)
        (*cloud)[u] = (first[u] != u && same[u]) ? (*cloud)[first[u]] : nc++;
    return nc;
}

// Argument checks of the graph entries (before the device is looked up).  n_pts may be null
// only when off is given (n_pts[c] = off[c+1] - off[c]).  Returns 0 or a se3icp_status.
inline int graph_check(int32_t n_clouds, const int64_t* n_pts, const int64_t* off, int32_t n_pairs,
                       const int32_t* src, const int32_t* tgt, int method, int n_methods, int32_t sharing,
                       const void* results) {
    if (n_clouds <= 0 || n_pairs <= 0 || (!n_pts && !off) || !src || !tgt || !results) return -1;  // INVALID_ARG
    if (sharing < kGraphSharingMin || sharing > kGraphSharingMax) return -1;
    if (method < 0 || method >= n_methods) return -2;  // INVALID_METHOD
    for (int32_t p = 0; p < n_pairs; ++p)
        if (src[p] < 0 || src[p] >= n_clouds || tgt[p] < 0 || tgt[p] >= n_clouds) return -1;
    for (int32_t p = 0; p < n_pairs; ++p)
        for (int side = 0; side < 2; ++side) {
            const int32_t c = side == 0 ? src[p] : tgt[p];
            const int64_t n = n_pts ? n_pts[c] : off[c + 1] - off[c];
            if (n <= 0) return -3;  // EMPTY_CLOUD
        }
    return 0;
}

// Per destination cloud.  k_graph_normalize: src_off is the cloud's first slot among the raw
// columns.  k_graph_share: src_off / src_cloud are the first slot and the cloud whose SE(3)
// rows it takes (frames != 0), nrm_off the first slot of its normals (its own: none copied).
struct GraphSeg { int32_t src_off; int32_t src_cloud; int32_t nrm_off; int32_t frames; };

// ---- the neighbour selection of planned uses as a value (Engine::select_by_class, setup_knn)
// Everything select_by_class decides before it queues anything.  The engine keeps the call's
// SelectPlan until the call's last synchronisation, because queued copies read its arrays; no
// code reads it as state.
struct SelectSwitches {
    int lrf_seeding, lrf_taking, lrf_exact;  // se3icp_set_lrf_seeding / _taking / _exact
    bool knn_list;                           // the sorted lists are asked for (se3icp_knn_self)
    int pose_seeding;                        // se3icp_set_pose_seeding
};
struct SelectPlan {
    std::vector<int32_t> home;      // [classes]: the class's first use, which selects for it
    // [uses]: the uses' own setup table, and the selection's: k_lrf, k_nrm, k_knn are 0 off a home
    std::vector<CloudSetup> batch, run;
    std::vector<GraphSeg> seg;      // [uses]: k_graph_share's table
    std::vector<ChunkWork> chunks;  // of the uses that take frames or normals from another use
    bool seeds = false, takes = false;
    std::vector<SeedRef> seed_ref;  // [uses] when seeds
    int64_t seed_floats = 0;        // the floats of the seed buffer
    std::vector<int32_t> take_flag; // [uses] when takes: bit 0 stores lists, bit 1 takes
    int take_stride = 0;            // entries per list
    int seed_mode = 0, take_mode = 0;  // the switches' lrf_seeding / lrf_taking, for k_lrf8
    // graph_stats[GS_FULL]; with seeds seed_stats[0], init_stats[IS_CROSS_SEEDED]; with takes
    // take_stats[TS_CLASSES]
    int64_t full = 0, seeded = 0, cross = 0, taking = 0;
};
// clouds, batch [uses]: the uses' layout and setup table; k_lrf: the method's TOLDI k (frames exactly when the plan
// normalizes); tree_donor: graph_plan_trees' table if a slot adopted, else empty; pose_raw /
// pose_rigid: per variant (graph_plan_seeds_posed), empty in a call without a posed edge.
inline SelectPlan graph_plan_selection(const GraphPlan& plan, const CloudDev* clouds, const CloudSetup* batch,
                                       int32_t k_lrf, const SelectSwitches& sw, const std::vector<int32_t>& tree_donor,
                                       const std::vector<int32_t>& pose_raw, const std::vector<int32_t>& pose_rigid) {
    const int32_t U = (int32_t)plan.use_class.size(), K = (int32_t)plan.classes.size();
    const bool se3 = plan.normalize;
    SelectPlan sp;
    sp.seed_mode = sw.lrf_seeding;
    sp.take_mode = sw.lrf_taking;
    sp.home.assign((size_t)K, -1);
    for (int32_t u = 0; u < U; ++u)
        if (sp.home[plan.use_class[u]] < 0) sp.home[plan.use_class[u]] = u;
    sp.batch.assign(batch, batch + U);
    sp.run = sp.batch;
    sp.seg.assign((size_t)U, GraphSeg{});
    for (int32_t u = 0; u < U; ++u) {
        const int32_t k = plan.use_class[u];
        const GraphClass& gc = plan.classes[k];
        // a home use selects for its class (the largest normals k of the class's uses; none
        // where another class of the cloud owns the normals), the others select nothing
        CloudSetup& st = sp.run[u];
        const bool is_home = sp.home[k] == u;
        st.k_lrf = is_home ? k_lrf : 0;
        st.k_nrm = (is_home && gc.nrm_from == k) ? gc.k_nrm : 0;
        st.k_knn = std::max(st.k_lrf, st.k_nrm);
        sp.full += st.k_knn > 0;
        const int32_t hf = sp.home[k], hn = sp.home[gc.nrm_from];  // where its frames / normals are computed
        sp.seg[u] = GraphSeg{clouds[hf].off, hf, clouds[hn].off, (hf != u && se3) ? 1 : 0};
        if ((hf != u && se3) || hn != u)
            for (int64_t p0 = 0; p0 < clouds[u].n; p0 += kChunk) sp.chunks.push_back(ChunkWork{u, (int32_t)p0});
    }
    // seeding: a cloud's later classes start from its first class's neighbour distances
    // (graph_plan_seeds; k_lrf8 only, so not under se3icp_set_lrf_exact)
    if (sw.lrf_seeding == 1 || sw.lrf_exact != 0 || sw.knn_list) return sp;
    std::vector<int32_t> kk((size_t)K);
    std::vector<int64_t> nn((size_t)K);
    for (int32_t k = 0; k < K; ++k) {
        kk[k] = sp.run[sp.home[k]].k_knn;
        nn[k] = clouds[sp.home[k]].n;
    }
    std::vector<SeedClass> sc;
    int32_t cross = 0;
    const int32_t seeded = pose_raw.empty() ? graph_plan_seeds(plan, kk.data(), nn.data(), &sc)
                                            : graph_plan_seeds_posed(plan, kk.data(), nn.data(), pose_raw.data(),
                                                                     pose_rigid.data(), sw.pose_seeding == 0, &sc, &cross);
    int64_t total = 0;
    for (int32_t k = 0; k < K; ++k)
        if (sc[k].from >= 0) total += nn[k];  // (an upper bound of the buffer: a source may seed several)
    if (seeded <= 0 || total > INT32_MAX) return sp;
    sp.seed_ref.assign((size_t)U, SeedRef{-1, -1, 1.0});
    for (int32_t k = 0; k < K; ++k) {
        if (sc[k].from < 0) continue;
        SeedRef& src = sp.seed_ref[sp.home[sc[k].from]];
        if (src.store < 0) {
            src.store = (int32_t)sp.seed_floats;
            sp.seed_floats += nn[k];
        }
        sp.seed_ref[sp.home[k]].load = src.store;
        sp.seed_ref[sp.home[k]].rho2 = sc[k].rho2;
    }
    sp.seeded = seeded;
    sp.cross = cross;
    sp.seeds = true;
    // taking: a seeded class with its source's tree order takes the source's lists
    // (graph_plan_takes); only with both switches at their defaults (taking mode 2 is the
    // default with every bound halved)
    if (sw.lrf_seeding != 0 || sw.lrf_taking == 1 || (int32_t)tree_donor.size() != U) return sp;
    std::vector<uint8_t> tk;
    const int32_t taking = graph_plan_takes(plan, sc, kk.data(), nn.data(), sp.home.data(), tree_donor, &tk);
    int64_t kw_max = 0;
    for (int32_t k = 0; k < K; ++k)
        if (tk[k]) kw_max = std::max<int64_t>(kw_max, std::min<int64_t>(kk[k], nn[k]));
    if (taking <= 0 || 2 * sp.seed_floats > INT32_MAX) return sp;
    sp.take_flag.assign((size_t)U, 0);
    for (int32_t k = 0; k < K; ++k) {
        if (!tk[k]) continue;
        sp.take_flag[sp.home[k]] |= 2;
        sp.take_flag[sp.home[sc[k].from]] |= 1;
    }
    // (lists of Kw <= 128 entries, 16-B aligned; longer ones are never taken)
    sp.take_stride = (int)((std::min<int64_t>(kw_max, kSmallK) + 3) & ~(int64_t)3);
    sp.taking = taking;
    sp.takes = true;
    return sp;
}

// The three wave tables of k_lrf8 over the clouds of a selection, eight queries per wave and
// waves aligned to each cloud's first point: wb[t * (nclouds + 1) + c] is cloud c's first wave
// in table t.  Table 0: the unseeded and the storing clouds; 1: the seeded clouds, in a launch
// of their own behind the one that stores their seeds; 2: the taking clouds among them, a launch
// that takes the stored lists and a seeded one over the same table for the waves that could not.
// A cloud that wants no neighbours gets no waves (the kernel's search for a wave's cloud takes the
// last one that starts at or before it).  sel null: a plain selection, every wave in table 0.
struct WaveTables {
    std::vector<int32_t> wb;  // [3 * (nclouds + 1)]
    int32_t nw, nw_sd, nw_tk;
};
inline WaveTables select_wave_tables(int32_t nclouds, const CloudDev* clouds, const CloudSetup* setup,
                                     const SelectPlan* sel) {
    const int32_t nt = nclouds + 1;
    std::vector<int32_t> wb(3 * (size_t)nt, 0);
    for (int32_t c = 0; c < nclouds; ++c) {
        const int32_t waves = setup[c].k_knn > 0 ? (clouds[c].n + 7) / 8 : 0;
        const bool sd = sel && sel->seeds && sel->seed_ref[c].load >= 0;
        const bool tk = sd && sel->takes && (sel->take_flag[c] & 2);
        wb[c + 1] = wb[c] + (sd ? 0 : waves);
        wb[nt + c + 1] = wb[nt + c] + (sd && !tk ? waves : 0);
        wb[2 * nt + c + 1] = wb[2 * nt + c] + (tk ? waves : 0);
    }
    const int32_t nw = wb[nclouds], nw_sd = wb[nt + nclouds], nw_tk = wb[2 * nt + nclouds];
    return WaveTables{std::move(wb), nw, nw_sd, nw_tk};
}

// ---- k_graph.hip
// k_share_compare: slot's bytes against those of the first slot of its group
struct SharePair { int32_t slot; int32_t first; };
// hash[u] += the content hash of cloud slot u's raw input (the caller clears it)
void launch_share_hash(const View& v, unsigned long long* hash, hipStream_t s);
// same[pair.slot] = 0 where the slot's bytes differ from pair.first's (the caller presets nonzero)
void launch_share_compare(const View& v, const SharePair* pairs, int npairs, int32_t* same, hipStream_t s);
// a use's normalized columns from the shared raw columns: the arithmetic of k_normalize
void launch_graph_normalize(const View& v, const ChunkWork* chunks, int nchunks, const GraphSeg* seg,
                            const double* raw_xyz64, const double* raw_conf64, hipStream_t s);
// the SE(3) rows and normals of the uses that did not compute their own, from their class's
void launch_graph_share(const View& v, const ChunkWork* chunks, int nchunks, const GraphSeg* seg, hipStream_t s);

}  // namespace se3icp
