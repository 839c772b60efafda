// Host build of the planning of se3-icp_amd/csrc/graph.hpp (graph_pair_scale, graph_plan,
// graph_check: what se3icp_register_graph and Engine::register_graph call) for
// tests/test_graph_host.py.  Checks, over hand-made edge lists and random graphs:
//   scale     graph_pair_scale is scale_pre * (1 / max(r_src, r_tgt)) to the bit, in both
//             argument orders
//   equal     pairs with the same largest radius give a cloud one class; another radius
//             gives it a second
//   self      a self edge is one class with two uses
//   repeat    a repeated edge adds uses, not classes
//   unused    a cloud no edge names gets no class (and its radius is never read)
//   order     classes are numbered in order of first use; use 2p is the source of edge p
//   level1    without de-duplication every use is a class of its own
//   vanilla   without normalization a class is (cloud, target's centre): scale 1, centre 0,
//             and the normals of a cloud's classes come from its first class with normals
//   cover     random graphs: every use has a class of its own cloud whose fields are the
//             pair's, n_uses sum to 2P, and equal keys share a class
//   args      graph_check: each code, in the order the header documents
// Prints one line per check, "<check> ok" or "<check> FAIL <count>", then "checked <n>";
// exits 1 if any failed.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "graph.hpp"

using namespace se3icp;

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

int main() {
    enum { SCALE, EQUAL, SELF, REPEAT, UNUSED, ORDER, LEVEL1, VANILLA, COVER, ARGS, NCHECK };
    const char* const names[NCHECK] = {"scale", "equal", "self", "repeat", "unused", "order", "level1", "vanilla",
                                       "cover", "args"};
    long bad[NCHECK] = {};
    long checked = 0;
    auto expect = [&](int c, bool ok) {
        ++checked;
        if (!ok) ++bad[c];
    };

    // radii of datasets.kitti_like_sequence(5, seed=4, n_az=200), and made-up centres
    const double rad[6] = {69.15, 74.58, 73.83, 69.71, 71.00, 1e300};
    double cen[18];
    for (int i = 0; i < 18; ++i) cen[i] = 0.25 * i - 1.0;

    // ---- scale
    for (double sp : {3.0, 10.0, 0.01})
        for (int a = 0; a < 5; ++a)
            for (int b = 0; b < 5; ++b) {
                const double rmax = rad[a] > rad[b] ? rad[a] : rad[b];
                const double inv = 1.0 / rmax;
                expect(SCALE, same_bits(graph_pair_scale(sp, rad[a], rad[b]), sp * inv));
                expect(SCALE, same_bits(graph_pair_scale(sp, rad[a], rad[b]), graph_pair_scale(sp, rad[b], rad[a])));
            }

    GraphPlan plan;
    // ---- the sequence: scan i+1 onto scan i
    {
        const int32_t src[4] = {1, 2, 3, 4}, tgt[4] = {0, 1, 2, 3};
        graph_plan(4, src, tgt, true, 3.0, cen, rad, 20, 20, true, &plan);
        // scan 1 has the largest radius of both its pairs: one class; scans 2, 3: two each
        expect(EQUAL, plan.classes.size() == 7);
        expect(EQUAL, plan.use_class[0] == plan.use_class[3]);   // scan 1: source of edge 0, target of edge 1
        expect(EQUAL, plan.use_class[2] != plan.use_class[5]);   // scan 2
        expect(EQUAL, plan.use_class[4] != plan.use_class[7]);   // scan 3
        expect(EQUAL, same_bits(plan.classes[plan.use_class[2]].norm_scale, 3.0 * (1.0 / 74.58)));
        expect(EQUAL, same_bits(plan.classes[plan.use_class[5]].norm_scale, 3.0 * (1.0 / 73.83)));
        const int32_t want[8] = {0, 1, 2, 0, 3, 4, 5, 6};  // first use numbers a class
        for (int u = 0; u < 8; ++u) expect(ORDER, plan.use_class[u] == want[u]);
        for (int u = 0; u < 8; ++u) {
            const GraphClass& g = plan.classes[plan.use_class[u]];
            const int c = (u & 1) ? tgt[u >> 1] : src[u >> 1];
            expect(ORDER, g.cloud == c && same_bits(g.norm_center[1], cen[3 * c + 1]) && g.f32_center[2] == 0.0 &&
                              g.nrm_from == plan.use_class[u]);
        }
        graph_plan(4, src, tgt, true, 3.0, cen, rad, 20, 20, false, &plan);
        expect(LEVEL1, plan.classes.size() == 8);
        for (int u = 0; u < 8; ++u) expect(LEVEL1, plan.use_class[u] == u && plan.classes[u].n_uses == 1);
    }
    // ---- self edge, repeated edge, unused cloud (cloud 5's radius would poison every scale)
    {
        const int32_t src[5] = {0, 2, 1, 0, 3}, tgt[5] = {1, 1, 1, 1, 1};
        graph_plan(5, src, tgt, true, 3.0, cen, rad, 0, 30, true, &plan);
        expect(SELF, plan.use_class[4] == plan.use_class[5]);  // edge 2 = (1, 1)
        expect(SELF, plan.classes[plan.use_class[4]].n_uses == 6);  // five targets and one source
        expect(SELF, plan.classes[plan.use_class[4]].k_nrm == 30);  // the largest of its uses'
        expect(REPEAT, plan.use_class[0] == plan.use_class[6] && plan.use_class[1] == plan.use_class[7]);
        expect(REPEAT, plan.classes[plan.use_class[0]].n_uses == 2 && plan.classes[plan.use_class[0]].k_nrm == 0);
        expect(REPEAT, plan.classes.size() == 4);
        bool any5 = false, huge = false;
        for (const GraphClass& g : plan.classes) {
            any5 |= g.cloud == 5 || g.cloud == 4;
            huge |= !(g.norm_scale > 0.03);
        }
        expect(UNUSED, !any5);
        expect(UNUSED, !huge);
    }
    // ---- vanilla: raw coordinates, the f32 copy centred on the edge's target
    {
        const int32_t src[4] = {1, 2, 3, 4}, tgt[4] = {0, 1, 2, 3};
        graph_plan(4, src, tgt, false, 3.0, cen, nullptr, 20, 20, true, &plan);
        expect(VANILLA, plan.classes.size() == 8);  // scan 1 centred on scan 0, then on itself
        for (int u = 0; u < 8; ++u) {
            const GraphClass& g = plan.classes[plan.use_class[u]];
            const int t = tgt[u >> 1];
            expect(VANILLA, g.norm_scale == 1.0 && g.norm_center[0] == 0.0 && same_bits(g.f32_center[2], cen[3 * t + 2]));
        }
        // the second class of scans 1..3 takes its normals from the first
        expect(VANILLA, plan.classes[plan.use_class[3]].nrm_from == plan.use_class[0]);
        expect(VANILLA, plan.classes[plan.use_class[5]].nrm_from == plan.use_class[2]);
        expect(VANILLA, plan.classes[plan.use_class[0]].nrm_from == plan.use_class[0]);
        // pt2pl: sources have no normals, so a target class owns them
        graph_plan(4, src, tgt, false, 3.0, cen, nullptr, 0, 30, true, &plan);
        for (int u = 0; u < 8; ++u) expect(VANILLA, plan.classes[plan.use_class[u]].nrm_from == plan.use_class[u]);
        // one map: every use of the map is one class
        const int32_t s2[3] = {0, 2, 1}, t2[3] = {1, 1, 1};
        graph_plan(3, s2, t2, false, 3.0, cen, nullptr, 0, 30, true, &plan);
        expect(VANILLA, plan.classes.size() == 3 && plan.use_class[1] == plan.use_class[3] &&
                            plan.use_class[4] == plan.use_class[5]);
    }
    // ---- random graphs
    {
        std::mt19937 gen(11);
        for (int trial = 0; trial < 200; ++trial) {
            const int C = 1 + (int)(gen() % 9), P = 1 + (int)(gen() % 24);
            std::vector<double> r(C), c(3 * C);
            for (int i = 0; i < C; ++i) r[i] = 1.0 + (double)(gen() % 4);  // many equal radii
            for (double& x : c) x = (double)(gen() % 1000) / 7.0;
            std::vector<int32_t> s(P), t(P);
            for (int p = 0; p < P; ++p) {
                s[p] = (int32_t)(gen() % C);
                t[p] = (int32_t)(gen() % C);
            }
            const bool norm = trial & 1;
            graph_plan(P, s.data(), t.data(), norm, 10.0, c.data(), r.data(), 20, 20, true, &plan);
            long uses = 0;
            for (const GraphClass& g : plan.classes) uses += g.n_uses;
            expect(COVER, uses == 2 * P && plan.use_class.size() == (size_t)2 * P);
            for (int u = 0; u < 2 * P; ++u) {
                const int p = u >> 1, cl = (u & 1) ? t[p] : s[p];
                const GraphClass& g = plan.classes[plan.use_class[u]];
                const double sc = norm ? graph_pair_scale(10.0, r[s[p]], r[t[p]]) : 1.0;
                expect(COVER, g.cloud == cl && same_bits(g.norm_scale, sc) &&
                                  same_bits(g.f32_center[0], norm ? 0.0 : c[3 * t[p]]));
                for (int w = 0; w < u; ++w) {  // equal keys share a class, different ones do not
                    const int q = w >> 1, cw = (w & 1) ? t[q] : s[q];
                    const double sw = norm ? graph_pair_scale(10.0, r[s[q]], r[t[q]]) : 1.0;
                    const bool same_key = cw == cl && same_bits(sw, sc) &&
                                          (norm || std::memcmp(&c[3 * t[q]], &c[3 * t[p]], 24) == 0);
                    expect(COVER, same_key == (plan.use_class[w] == plan.use_class[u]));
                }
            }
        }
    }
    // ---- argument checks (se3icp.h: INVALID_ARG -1, INVALID_METHOD -2, EMPTY_CLOUD -3)
    {
        const int64_t n[3] = {5, 0, 7}, off[4] = {0, 5, 5, 12};
        const int32_t s[2] = {0, 2}, t[2] = {2, 0}, s_empty[2] = {0, 1}, s_out[2] = {0, 3}, s_neg[2] = {-1, 0};
        int res = 0;
        expect(ARGS, graph_check(3, n, nullptr, 2, s, t, 5, 10, 0, &res) == 0);  // cloud 1 is empty but unused
        expect(ARGS, graph_check(3, nullptr, off, 2, s, t, 5, 10, 3, &res) == 0);
        expect(ARGS, graph_check(0, n, nullptr, 2, s, t, 5, 10, 0, &res) == -1);
        expect(ARGS, graph_check(3, n, nullptr, 0, s, t, 5, 10, 0, &res) == -1);
        expect(ARGS, graph_check(3, nullptr, nullptr, 2, s, t, 5, 10, 0, &res) == -1);
        expect(ARGS, graph_check(3, n, nullptr, 2, nullptr, t, 5, 10, 0, &res) == -1);
        expect(ARGS, graph_check(3, n, nullptr, 2, s, nullptr, 5, 10, 0, &res) == -1);
        expect(ARGS, graph_check(3, n, nullptr, 2, s, t, 5, 10, 0, nullptr) == -1);
        expect(ARGS, graph_check(3, n, nullptr, 2, s_out, t, 5, 10, 0, &res) == -1);
        expect(ARGS, graph_check(3, n, nullptr, 2, s_neg, t, 5, 10, 0, &res) == -1);
        expect(ARGS, graph_check(3, n, nullptr, 2, s, t, 5, 10, 4, &res) == -1);
        expect(ARGS, graph_check(3, n, nullptr, 2, s, t, 5, 10, -1, &res) == -1);
        expect(ARGS, graph_check(3, n, nullptr, 2, s, t, 10, 10, 0, &res) == -2);
        expect(ARGS, graph_check(3, n, nullptr, 2, s, t, -1, 10, 0, &res) == -2);
        expect(ARGS, graph_check(3, n, nullptr, 2, s_empty, t, 5, 10, 0, &res) == -3);
        expect(ARGS, graph_check(3, nullptr, off, 2, s_empty, t, 5, 10, 0, &res) == -3);
    }

    int rc = 0;
    for (int k = 0; k < NCHECK; ++k) {
        if (bad[k]) {
            std::printf("%s FAIL %ld\n", names[k], bad[k]);
            rc = 1;
        } else {
            std::printf("%s ok\n", names[k]);
        }
    }
    std::printf("checked %ld\n", checked);
    return rc;
}
