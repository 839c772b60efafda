// Host build of the initial-pose arithmetic and planning (se3-icp_amd/csrc/pose.hpp, and
// graph_plan_variants / graph_plan_seeds_posed of graph.hpp: what se3icp_register_graph_init and
// Engine::register_graph call) as a small shared library for tests/test_init_host.py, which
// drives it through ctypes and compares with numpy restatements.
#include <cmath>
#include <cstdint>
#include <vector>

#include "graph.hpp"
#include "pose.hpp"

using namespace se3icp;

extern "C" {

void init_host_compose(const double* A, const double* B, double* C) { compose(A, B, C); }

void init_host_apply(const double* T, const double* xyz, int64_t n, double* out) {
    for (int64_t i = 0; i < n; ++i) apply_pose(T, xyz + 3 * i, out + 3 * i);
}

// What a compiler that contracts would make of apply_pose: every product fused into the sum that
// takes it (the first product of a row stands alone).  For the test that the pinned form is not
// this one.
void init_host_apply_fused(const double* T, const double* xyz, int64_t n, double* out) {
    for (int64_t i = 0; i < n; ++i)
        for (int e = 0; e < 3; ++e) {
            const double* p = xyz + 3 * i;
            double r = T[4 * e] * p[0];
            r = std::fma(T[4 * e + 1], p[1], r);
            r = std::fma(T[4 * e + 2], p[2], r);
            r = std::fma(T[4 * e + 3], 1.0, r);
            out[3 * i + e] = r;
        }
}

int init_host_is_identity(const double* T) { return pose_is_identity(T) ? 1 : 0; }
int init_host_is_valid(const double* T) { return pose_is_valid(T) ? 1 : 0; }
int init_host_is_rigid(const double* T) { return pose_is_rigid(T) ? 1 : 0; }

// graph_plan_variants: edge_src / edge_tgt [P], cloud / pose_edge [2P] (the first V are filled),
// counts [2] = {posed edges, posed variants}; returns V
int init_host_variants(int32_t P, const int32_t* src, const int32_t* tgt, const double* T_init, int32_t* edge_src,
                       int32_t* edge_tgt, int32_t* cloud, int32_t* pose_edge, int32_t* counts) {
    VariantPlan vp;
    graph_plan_variants(P, src, tgt, T_init, &vp);
    for (int32_t p = 0; p < P; ++p) {
        edge_src[p] = vp.edge_src[p];
        edge_tgt[p] = vp.edge_tgt[p];
    }
    for (size_t v = 0; v < vp.cloud.size(); ++v) {
        cloud[v] = vp.cloud[v];
        pose_edge[v] = vp.pose_edge[v];
    }
    counts[0] = vp.posed_edges;
    counts[1] = vp.posed_variants;
    return (int)vp.cloud.size();
}

// A hand-made class table: class k is variant `variant[k]` under scale[k], centred on center[3k..]
// with the f32 copy centred on f32c[3k..].  posed != 0: graph_plan_seeds_posed(raw, rigid, cross),
// otherwise graph_plan_seeds.  from [K], rho2 [K]; n_cross [1]; returns the seeded classes.
int init_host_seeds(int32_t K, const int32_t* variant, const double* scale, const double* center, const double* f32c,
                    const int32_t* k_knn, const int64_t* n_pts, int normalize, int dedupe, int posed, const int32_t* raw,
                    const int32_t* rigid, int cross, int32_t* from, double* rho2, int32_t* n_cross) {
    GraphPlan plan;
    plan.normalize = normalize != 0;
    plan.dedupe = dedupe != 0;
    for (int32_t k = 0; k < K; ++k) {
        GraphClass g{};
        g.cloud = variant[k];
        g.k_nrm = 20;
        g.n_uses = 1;
        g.nrm_from = k;
        g.norm_scale = scale[k];
        for (int a = 0; a < 3; ++a) {
            g.norm_center[a] = center[3 * k + a];
            g.f32_center[a] = f32c[3 * k + a];
        }
        plan.classes.push_back(g);
    }
    std::vector<SeedClass> seed;
    int32_t cr = 0;
    const int32_t n = posed ? graph_plan_seeds_posed(plan, k_knn, n_pts, raw, rigid, cross != 0, &seed, &cr)
                            : graph_plan_seeds(plan, k_knn, n_pts, &seed);
    for (int32_t k = 0; k < K; ++k) {
        from[k] = seed[k].from;
        rho2[k] = seed[k].rho2;
    }
    *n_cross = cr;
    return n;
}

}  // extern "C"
