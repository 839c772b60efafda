// Host build of the slot grouping of se3-icp_amd/csrc/graph.hpp (share_any_equal_n,
// share_candidates, share_clouds, graph_plan_uses: what Engine::setup_pairs_shared calls between
// its device passes) for tests/test_share_host.py.  Checks:
//   equal_n    share_any_equal_n: true exactly when two slots have one point count
//   group      share_candidates: first[u] is the first slot with u's (n, hash); equal hashes
//              under different counts and equal counts under different hashes stay apart; the
//              return value counts the compares
//   confirm    share_clouds: a confirmed slot takes its group's cloud; a hash-equal slot the
//              compare did not confirm is a cloud of its own, also against a later slot of the
//              group; flags of slots that were not compared are never read; clouds are numbered
//              in order of first slot
//   chain      the expanded scan chain: 2P slots, P + 1 clouds, the interior scans in two slots
//   random     random slot lists against a quadratic reference
//   uses       graph_plan_uses: graph_plan is it over the uses it builds; a class needs equal
//              bits of norm_center too, so slots of one cloud that the device centred
//              differently do not share
// Prints one line per check, "<check> ok" or "<check> FAIL <count>", then "checked <n>";
// exits 1 if any failed.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "graph.hpp"

using namespace se3icp;

int main() {
    enum { EQUAL_N, GROUP, CONFIRM, CHAIN, RANDOM, USES, NCHECK };
    const char* const names[NCHECK] = {"equal_n", "group", "confirm", "chain", "random", "uses"};
    long bad[NCHECK] = {};
    long checked = 0;
    auto expect = [&](int c, bool ok) {
        ++checked;
        if (!ok) ++bad[c];
    };
    std::vector<int32_t> first, cloud;

    // ---- equal_n
    {
        const int64_t a[4] = {5, 6, 7, 8}, b[4] = {5, 6, 7, 5}, c[1] = {9}, d[2] = {9, 9};
        expect(EQUAL_N, !share_any_equal_n(4, a));
        expect(EQUAL_N, share_any_equal_n(4, b));
        expect(EQUAL_N, !share_any_equal_n(1, c));
        expect(EQUAL_N, share_any_equal_n(2, d));
        expect(EQUAL_N, !share_any_equal_n(0, a));
    }
    // ---- group
    {
        //                   0    1    2    3    4    5    6
        const int64_t n[7] = {10, 10, 11, 10, 11, 10, 12};
        const uint64_t h[7] = {7, 8, 7, 7, 7, 8, 0};
        const int cand = share_candidates(7, n, h, &first);
        const int32_t want[7] = {0, 1, 2, 0, 2, 1, 6};
        expect(GROUP, cand == 3);
        for (int u = 0; u < 7; ++u) expect(GROUP, first[u] == want[u]);
        // all 64 bits take part
        const int64_t n2[2] = {4, 4};
        const uint64_t h2[2] = {0x8000000000000001ull, 0x0000000000000001ull};
        expect(GROUP, share_candidates(2, n2, h2, &first) == 0 && first[1] == 1);
    }
    // ---- confirm
    {
        const int32_t f[6] = {0, 1, 0, 0, 1, 0};
        // slots 2, 3, 5 hash as slot 0; the compare confirmed 2 and 5, not 3; slot 4 is slot 1
        const int32_t same[6] = {-7, 0, 1, 0, 1, 0x01010101};  // (slots 0 and 1 were not compared)
        const int nc = share_clouds(6, f, same, &cloud);
        const int32_t want[6] = {0, 1, 0, 2, 1, 0};
        expect(CONFIRM, nc == 3);
        for (int u = 0; u < 6; ++u) expect(CONFIRM, cloud[u] == want[u]);
        // two unconfirmed slots of one group never share with each other on the hash alone
        const int32_t f2[3] = {0, 0, 0}, s2[3] = {1, 0, 0};
        expect(CONFIRM, share_clouds(3, f2, s2, &cloud) == 3 && cloud[1] == 1 && cloud[2] == 2);
        // nothing confirmed at all: every slot its own cloud, in slot order
        const int32_t s3[3] = {0, 0, 0};
        expect(CONFIRM, share_clouds(3, f2, s3, &cloud) == 3 && cloud[0] == 0 && cloud[2] == 2);
    }
    // ---- chain: pair p registers scan p + 1 onto scan p; slot 2p its source, 2p + 1 its target
    for (int P : {1, 2, 8, 64}) {
        std::vector<int64_t> n(2 * P);
        std::vector<uint64_t> h(2 * P);
        for (int p = 0; p < P; ++p) {
            n[2 * p] = 1000 + (p + 1) % 3;      // (point counts repeat across scans)
            h[2 * p] = 0x9E3779B97F4A7C15ull * (uint64_t)(p + 2);
            n[2 * p + 1] = 1000 + p % 3;
            h[2 * p + 1] = 0x9E3779B97F4A7C15ull * (uint64_t)(p + 1);
        }
        const int cand = share_candidates(2 * P, n.data(), h.data(), &first);
        expect(CHAIN, cand == P - 1);
        std::vector<int32_t> same(2 * P, 1);
        expect(CHAIN, share_clouds(2 * P, first.data(), same.data(), &cloud) == P + 1);
        for (int p = 0; p + 1 < P; ++p) expect(CHAIN, cloud[2 * p] == cloud[2 * (p + 1) + 1]);  // scan p + 1
        expect(CHAIN, share_any_equal_n(2 * P, n.data()) == (P > 1));
    }
    // ---- random slot lists
    {
        std::mt19937_64 gen(5);
        for (int trial = 0; trial < 300; ++trial) {
            const int U = 1 + (int)(gen() % 40);
            std::vector<int64_t> n(U);
            std::vector<uint64_t> h(U);
            std::vector<int32_t> same(U);
            for (int u = 0; u < U; ++u) {
                n[u] = 1 + (int64_t)(gen() % 3);
                h[u] = gen() % 4;
                same[u] = (gen() % 4) != 0;
            }
            const int cand = share_candidates(U, n.data(), h.data(), &first);
            int want_cand = 0;
            for (int u = 0; u < U; ++u) {
                int f = u;
                for (int w = 0; w < u; ++w)
                    if (n[w] == n[u] && h[w] == h[u]) {
                        f = w;
                        break;
                    }
                expect(RANDOM, first[u] == f);
                want_cand += f != u;
            }
            expect(RANDOM, cand == want_cand);
            const int nc = share_clouds(U, first.data(), same.data(), &cloud);
            int next = 0;
            for (int u = 0; u < U; ++u) {
                const bool shares = first[u] != u && same[u];
                expect(RANDOM, shares ? cloud[u] == cloud[first[u]] : cloud[u] == next);
                next += !shares;
            }
            expect(RANDOM, nc == next);
            bool any = false;
            for (int u = 0; u < U; ++u)
                for (int w = 0; w < u; ++w) any |= n[w] == n[u];
            expect(RANDOM, share_any_equal_n(U, n.data()) == any);
        }
    }
    // ---- uses
    {
        const double rad[5] = {69.15, 74.58, 73.83, 69.71, 71.00};
        double cen[15];
        for (int i = 0; i < 15; ++i) cen[i] = 0.25 * i - 1.0;
        const int32_t src[4] = {1, 2, 3, 4}, tgt[4] = {0, 1, 2, 3};
        GraphPlan a, b;
        for (int normalize = 0; normalize < 2; ++normalize) {
            graph_plan(4, src, tgt, normalize != 0, 3.0, cen, rad, 20, 20, true, &a);
            std::vector<GraphUse> use(8);
            for (int u = 0; u < 8; ++u) {
                const int p = u >> 1, c = (u & 1) ? tgt[p] : src[p];
                use[u].cloud = c;
                use[u].k_nrm = 20;
                use[u].norm_scale = normalize ? graph_pair_scale(3.0, rad[src[p]], rad[tgt[p]]) : 1.0;
                for (int x = 0; x < 3; ++x) {
                    use[u].norm_center[x] = normalize ? cen[3 * c + x] : 0.0;
                    use[u].f32_center[x] = normalize ? 0.0 : cen[3 * tgt[p] + x];
                }
            }
            graph_plan_uses(8, use.data(), normalize != 0, true, &b);
            expect(USES, a.classes.size() == b.classes.size() && a.use_class == b.use_class);
            expect(USES, a.classes.size() == (normalize ? 7u : 8u));
            for (size_t k = 0; k < a.classes.size() && k < b.classes.size(); ++k)
                expect(USES, a.classes[k].cloud == b.classes[k].cloud && a.classes[k].nrm_from == b.classes[k].nrm_from &&
                                 a.classes[k].n_uses == b.classes[k].n_uses && a.classes[k].k_nrm == b.classes[k].k_nrm);
            if (normalize) {
                // scan 1's two slots (uses 0 and 3) centred one ulp apart: two classes
                use[3].norm_center[1] = std::nextafter(use[3].norm_center[1], 1e9);
                graph_plan_uses(8, use.data(), true, true, &b);
                expect(USES, b.classes.size() == 8 && b.use_class[0] != b.use_class[3]);
            }
        }
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
