// Host build of the tree plan of se3-icp_amd/csrc/graph.hpp (graph_plan_trees: which slots of a
// call build their kd-trees and which adopt the order of their cloud's first slot, what
// Engine::setup_pairs_shared and Engine::register_graph ask before they queue the builds) for
// tests/test_tree_plan_host.py.
// Checks:
//   chain        the five-scan chain: scans 1, 2 and 3 lie in two slots each; the later slot
//                adopts from the earlier one whatever its class, five slots build
//   map          four scans onto one map: the map's first slot builds, its three other slots
//                adopt from it; the same through the classes graph_plan gives register_graph
//   unconfirmed  hash-equal slots the byte compare rejected are clouds of their own
//                (share_clouds) and build; a slot nothing is known about (cloud < 0) builds;
//                slots of one cloud id but different point counts do not adopt
//   level1       sharing level 1 / tree sharing off: every slot builds
//   vanilla      the plan does not depend on the method: the classes of the vanilla methods
//                (f32 copies centred on the pair's target) give the chain's table
//   random       random slot lists: a donor is the first slot of the adopter's cloud, builds
//                itself, comes first and has the adopter's point count; every first slot builds
// Prints one line per check, "<check> ok" or "<check> FAIL <count>", then "checked <n>";
// exits 1 if any failed.
#include <cstdio>
#include <random>
#include <vector>

#include "graph.hpp"

using namespace se3icp;

int main() {
    enum { CHAIN, MAP, UNCONFIRMED, LEVEL1, VANILLA, RANDOM, NCHECK };
    const char* const names[NCHECK] = {"chain", "map", "unconfirmed", "level1", "vanilla", "random"};
    long bad[NCHECK] = {};
    long checked = 0;
    auto expect = [&](int c, bool ok) {
        ++checked;
        if (!ok) ++bad[c];
    };
    std::vector<int32_t> donor;
    // the chain's slots: src 0, tgt 0, src 1, ... = scans 1 0 2 1 3 2 4 3
    const int32_t chain_cloud[8] = {1, 0, 2, 1, 3, 2, 4, 3};
    const int64_t scan_n[5] = {12510, 12534, 12534, 12542, 12535};
    int64_t chain_n[8];
    for (int u = 0; u < 8; ++u) chain_n[u] = scan_n[chain_cloud[u]];
    const int32_t chain_want[8] = {-1, -1, -1, 0, -1, 2, -1, 4};

    // ---- chain
    {
        expect(CHAIN, graph_plan_trees(8, chain_cloud, chain_n, true, &donor) == 3);
        expect(CHAIN, donor.size() == 8);
        for (int u = 0; u < 8; ++u) expect(CHAIN, donor[u] == chain_want[u]);
        // numbered as share_clouds numbers them, in order of first slot
        std::vector<int32_t> first(8), same(8, 1), cloud;
        for (int u = 0; u < 8; ++u) {
            first[u] = u;
            for (int w = 0; w < u; ++w)
                if (chain_cloud[w] == chain_cloud[u]) { first[u] = w; break; }
        }
        expect(CHAIN, share_clouds(8, first.data(), same.data(), &cloud) == 5);
        expect(CHAIN, graph_plan_trees(8, cloud.data(), chain_n, true, &donor) == 3);
        for (int u = 0; u < 8; ++u) expect(CHAIN, donor[u] == chain_want[u]);
    }
    // ---- map: scans 0, 1, 3, 4 onto cloud 2
    {
        const int32_t cl[8] = {0, 2, 1, 2, 3, 2, 4, 2};
        int64_t n[8];
        for (int u = 0; u < 8; ++u) n[u] = scan_n[cl[u]];
        expect(MAP, graph_plan_trees(8, cl, n, true, &donor) == 3);
        const int32_t want[8] = {-1, -1, -1, 1, -1, 1, -1, 1};
        for (int u = 0; u < 8; ++u) expect(MAP, donor[u] == want[u]);
        // as register_graph forms the table: the cloud of every use's class; the map runs under
        // four scales (its radius is the smallest), and its slots adopt all the same
        const double rmap[5] = {69.15, 74.58, 60.0, 69.71, 71.00};
        double cen[15];
        for (int i = 0; i < 15; ++i) cen[i] = 0.25 * i - 1.0;
        const int32_t src[4] = {0, 1, 3, 4}, tgt[4] = {2, 2, 2, 2};
        GraphPlan plan;
        graph_plan(4, src, tgt, true, 3.0, cen, rmap, 20, 20, true, &plan);
        expect(MAP, plan.classes.size() == 8);
        std::vector<int32_t> uc(8);
        for (int u = 0; u < 8; ++u) uc[u] = plan.classes[plan.use_class[u]].cloud;
        expect(MAP, graph_plan_trees(8, uc.data(), n, true, &donor) == 3);
        for (int u = 0; u < 8; ++u) expect(MAP, donor[u] == want[u]);
    }
    // ---- unconfirmed
    {
        // slots 3 and 5 are hash-equal to slots 0 and 2; the compare confirmed 3 and rejected 5
        std::vector<int32_t> first = {0, 1, 2, 0, 4, 2, 6, 2}, same = {1, 1, 1, 1, 1, 0, 1, 1}, cloud;
        const int64_t n[8] = {100, 90, 100, 100, 80, 100, 70, 100};
        expect(UNCONFIRMED, share_clouds(8, first.data(), same.data(), &cloud) == 6);
        expect(UNCONFIRMED, graph_plan_trees(8, cloud.data(), n, true, &donor) == 2);
        const int32_t want[8] = {-1, -1, -1, 0, -1, -1, -1, 2};
        for (int u = 0; u < 8; ++u) expect(UNCONFIRMED, donor[u] == want[u]);
        // nothing confirmed: nothing adopted
        std::vector<int32_t> none(8, 0);
        expect(UNCONFIRMED, share_clouds(8, first.data(), none.data(), &cloud) == 8);
        expect(UNCONFIRMED, graph_plan_trees(8, cloud.data(), n, true, &donor) == 0);
        for (int u = 0; u < 8; ++u) expect(UNCONFIRMED, donor[u] == -1);
        // slots nothing is known about, and one cloud id with two point counts
        const int32_t unknown[4] = {-1, -1, 3, 3};
        const int64_t n4[4] = {50, 50, 60, 61};
        expect(UNCONFIRMED, graph_plan_trees(4, unknown, n4, true, &donor) == 0);
        for (int u = 0; u < 4; ++u) expect(UNCONFIRMED, donor[u] == -1);
    }
    // ---- level 1
    {
        donor.assign(3, 7);
        expect(LEVEL1, graph_plan_trees(8, chain_cloud, chain_n, false, &donor) == 0 && donor.size() == 8);
        for (int u = 0; u < 8; ++u) expect(LEVEL1, donor[u] == -1);
        expect(LEVEL1, graph_plan_trees(0, chain_cloud, chain_n, true, &donor) == 0 && donor.empty());
    }
    // ---- vanilla: eight classes (every use is centred on its pair's target), the chain's table
    {
        const double rad[5] = {69.15, 74.58, 73.83, 69.71, 71.00};
        double cen[15];
        for (int i = 0; i < 15; ++i) cen[i] = 0.25 * i - 1.0;
        const int32_t src[4] = {1, 2, 3, 4}, tgt[4] = {0, 1, 2, 3};
        GraphPlan plan;
        graph_plan(4, src, tgt, false, 3.0, cen, rad, 20, 20, true, &plan);
        expect(VANILLA, plan.classes.size() == 8);
        std::vector<int32_t> uc(8);
        for (int u = 0; u < 8; ++u) uc[u] = plan.classes[plan.use_class[u]].cloud;
        expect(VANILLA, graph_plan_trees(8, uc.data(), chain_n, true, &donor) == 3);
        for (int u = 0; u < 8; ++u) expect(VANILLA, donor[u] == chain_want[u]);
    }
    // ---- random slot lists
    {
        std::mt19937_64 gen(18);
        for (int trial = 0; trial < 400; ++trial) {
            const int U = 1 + (int)(gen() % 24), C = 1 + (int)(gen() % 8);
            std::vector<int32_t> cl(U);
            std::vector<int64_t> n(U);
            for (int u = 0; u < U; ++u) {
                cl[u] = (gen() % 6 == 0) ? -1 : (int32_t)(gen() % C);
                // (a cloud id with a second point count now and then: never adopted across)
                n[u] = cl[u] < 0 ? 40 : 100 + 10 * cl[u] + (gen() % 9 == 0 ? 1 : 0);
            }
            const bool share = gen() % 5 != 0;
            const int na = graph_plan_trees(U, cl.data(), n.data(), share, &donor);
            int count = 0;
            expect(RANDOM, (int)donor.size() == U);
            for (int u = 0; u < U; ++u) {
                int first = -1;
                for (int w = 0; w < u && first < 0; ++w)
                    if (cl[u] >= 0 && cl[w] == cl[u]) first = w;
                const bool may = share && first >= 0 && n[first] == n[u];
                expect(RANDOM, donor[u] == (may ? first : -1));
                if (donor[u] >= 0) {
                    ++count;
                    expect(RANDOM, donor[u] < u && donor[donor[u]] == -1 && cl[donor[u]] == cl[u] && n[donor[u]] == n[u]);
                }
            }
            expect(RANDOM, na == count);
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
