// Host build of the seed plan of se3-icp_amd/csrc/graph.hpp (graph_plan_seeds: which classes of
// a cloud start their neighbour selection from its first class's distances, what
// Engine::select_by_class asks before it queues the selection) for tests/test_seed_host.py.
// Checks:
//   chain      the five-scan chain under the run_se3_* normalization: 7 classes, scans 2 and 3
//              get one seeded class each, scan 1 (one class for both its uses) none
//   map        scans registered onto one map of the smallest radius: the map's first class is
//              the source, every other one is seeded from it with rho2 = (s_b / s_a)^2
//   kw         a class that asks for more neighbours than its cloud's source found is not
//              seeded; one whose larger k the point count cuts to the source's Kw is; a class
//              that selects nothing is neither a source nor seeded; a class centred with other
//              bits or with a centred f32 copy is not seeded
//   vanilla    without the normalization nothing is seeded
//   level1     with a class per use (sharing level 1) nothing is seeded
//   random     random graphs: every seeded class's source is the first class of its cloud
//              that selects, comes before it, and rho2 is the squared ratio of the two scales
// Prints one line per check, "<check> ok" or "<check> FAIL <count>", then "checked <n>";
// exits 1 if any failed.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "graph.hpp"

using namespace se3icp;

int main() {
    enum { CHAIN, MAP, KW, VANILLA, LEVEL1, RANDOM, NCHECK };
    const char* const names[NCHECK] = {"chain", "map", "kw", "vanilla", "level1", "random"};
    long bad[NCHECK] = {};
    long checked = 0;
    auto expect = [&](int c, bool ok) {
        ++checked;
        if (!ok) ++bad[c];
    };
    const double rad[5] = {69.15, 74.58, 73.83, 69.71, 71.00};
    double cen[15];
    for (int i = 0; i < 15; ++i) cen[i] = 0.25 * i - 1.0;
    const int32_t chain_src[4] = {1, 2, 3, 4}, chain_tgt[4] = {0, 1, 2, 3};
    std::vector<SeedClass> seed;
    auto all = [](const GraphPlan& p, int32_t k, int64_t n, std::vector<int32_t>* kk, std::vector<int64_t>* nn) {
        kk->assign(p.classes.size(), k);
        nn->assign(p.classes.size(), n);
    };
    std::vector<int32_t> kk;
    std::vector<int64_t> nn;

    // ---- chain
    {
        GraphPlan plan;
        graph_plan(4, chain_src, chain_tgt, true, 3.0, cen, rad, 20, 20, true, &plan);
        all(plan, 90, 12500, &kk, &nn);
        expect(CHAIN, plan.classes.size() == 7);
        expect(CHAIN, graph_plan_seeds(plan, kk.data(), nn.data(), &seed) == 2);
        int per_cloud[5] = {};
        for (size_t k = 0; k < seed.size(); ++k) {
            if (seed[k].from < 0) {
                expect(CHAIN, seed[k].rho2 == 1.0);
                continue;
            }
            ++per_cloud[plan.classes[k].cloud];
            const GraphClass& a = plan.classes[seed[k].from];
            expect(CHAIN, seed[k].from < (int32_t)k && a.cloud == plan.classes[k].cloud);
            const double rho = plan.classes[k].norm_scale / a.norm_scale;
            expect(CHAIN, seed[k].rho2 == rho * rho && rho != 1.0);
        }
        const int want[5] = {0, 0, 1, 1, 0};
        for (int c = 0; c < 5; ++c) expect(CHAIN, per_cloud[c] == want[c]);
    }
    // ---- map: scans 0, 1, 3, 4 onto cloud 2, whose radius is the smallest
    {
        const double rmap[5] = {69.15, 74.58, 60.0, 69.71, 71.00};
        const int32_t src[4] = {0, 1, 3, 4}, tgt[4] = {2, 2, 2, 2};
        GraphPlan plan;
        graph_plan(4, src, tgt, true, 3.0, cen, rmap, 20, 20, true, &plan);
        all(plan, 90, 9000, &kk, &nn);
        expect(MAP, plan.classes.size() == 8);
        expect(MAP, graph_plan_seeds(plan, kk.data(), nn.data(), &seed) == 3);
        const int32_t first = plan.use_class[1];  // the map's first use
        for (int p = 0; p < 4; ++p) {
            const int32_t ks = plan.use_class[2 * p], kt = plan.use_class[2 * p + 1];
            expect(MAP, seed[ks].from == -1);
            expect(MAP, seed[kt].from == (p == 0 ? -1 : first));
            if (p > 0) {
                const double rho = (3.0 * (1.0 / rmap[src[p]])) / (3.0 * (1.0 / rmap[src[0]]));
                expect(MAP, seed[kt].rho2 == rho * rho);
            }
        }
        // a map of the largest radius is one class: nothing to seed
        const double rbig[5] = {69.15, 74.58, 90.0, 69.71, 71.00};
        graph_plan(4, src, tgt, true, 3.0, cen, rbig, 20, 20, true, &plan);
        all(plan, 90, 9000, &kk, &nn);
        expect(MAP, plan.classes.size() == 5 && graph_plan_seeds(plan, kk.data(), nn.data(), &seed) == 0);
    }
    // ---- kw
    {
        GraphPlan plan;
        graph_plan(4, chain_src, chain_tgt, true, 3.0, cen, rad, 20, 20, true, &plan);
        // the classes of scan 2: the source of pair 1 (use 2), then the target of pair 2 (use 5)
        const int32_t a = plan.use_class[2], b = plan.use_class[5];
        expect(KW, a != b && plan.classes[a].cloud == 2 && plan.classes[b].cloud == 2 && a < b);
        all(plan, 90, 12500, &kk, &nn);
        kk[b] = 91;
        expect(KW, graph_plan_seeds(plan, kk.data(), nn.data(), &seed) == 1 && seed[b].from == -1);
        kk[b] = 89;
        expect(KW, graph_plan_seeds(plan, kk.data(), nn.data(), &seed) == 2 && seed[b].from == a);
        // the point count cuts both to Kw = n
        kk[a] = 100;
        kk[b] = 200;
        nn[a] = nn[b] = 50;
        expect(KW, graph_plan_seeds(plan, kk.data(), nn.data(), &seed) == 2 && seed[b].from == a);
        nn[a] = nn[b] = 150;
        expect(KW, graph_plan_seeds(plan, kk.data(), nn.data(), &seed) == 1 && seed[b].from == -1);
        // a class that selects nothing
        all(plan, 90, 12500, &kk, &nn);
        kk[b] = 0;
        expect(KW, graph_plan_seeds(plan, kk.data(), nn.data(), &seed) == 1 && seed[b].from == -1);
        kk[b] = 90;
        kk[a] = 0;  // (then b is its cloud's first selecting class: a source, not seeded)
        expect(KW, graph_plan_seeds(plan, kk.data(), nn.data(), &seed) == 1 && seed[b].from == -1 && seed[a].from == -1);
        // other centre bits, a centred f32 copy
        all(plan, 90, 12500, &kk, &nn);
        GraphPlan q = plan;
        q.classes[b].norm_center[2] = std::nextafter(q.classes[b].norm_center[2], 1e9);
        expect(KW, graph_plan_seeds(q, kk.data(), nn.data(), &seed) == 1 && seed[b].from == -1);
        q = plan;
        q.classes[b].f32_center[0] = 0.5;
        expect(KW, graph_plan_seeds(q, kk.data(), nn.data(), &seed) == 1 && seed[b].from == -1);
        q = plan;
        q.classes[a].f32_center[1] = -0.5;
        expect(KW, graph_plan_seeds(q, kk.data(), nn.data(), &seed) == 1 && seed[b].from == -1);
    }
    // ---- vanilla, level 1
    for (int which = 0; which < 2; ++which) {
        const int chk = which == 0 ? VANILLA : LEVEL1;
        GraphPlan plan;
        graph_plan(4, chain_src, chain_tgt, which != 0, 3.0, cen, rad, 20, 20, which == 0, &plan);
        all(plan, 90, 12500, &kk, &nn);
        expect(chk, plan.classes.size() == 8);
        expect(chk, graph_plan_seeds(plan, kk.data(), nn.data(), &seed) == 0 && seed.size() == 8);
        for (const SeedClass& s : seed) expect(chk, s.from == -1);
    }
    // ---- random graphs
    {
        std::mt19937_64 gen(11);
        for (int trial = 0; trial < 300; ++trial) {
            const int C = 1 + (int)(gen() % 6), P = 1 + (int)(gen() % 12);
            std::vector<double> r(C), ce(3 * C);
            std::vector<int64_t> npts(C);
            for (int c = 0; c < C; ++c) {
                r[c] = 50.0 + (double)(gen() % 4);  // (radii repeat: classes merge)
                npts[c] = 20 + (int64_t)(gen() % 200);
                for (int a = 0; a < 3; ++a) ce[3 * c + a] = (double)(gen() % 7) - 3.0;
            }
            std::vector<int32_t> src(P), tgt(P);
            for (int p = 0; p < P; ++p) {
                src[p] = (int32_t)(gen() % C);
                tgt[p] = (int32_t)(gen() % C);
            }
            GraphPlan plan;
            graph_plan(P, src.data(), tgt.data(), true, 3.0, ce.data(), r.data(), 20, 20, true, &plan);
            const int K = (int)plan.classes.size();
            kk.resize(K);
            nn.resize(K);
            for (int k = 0; k < K; ++k) {
                kk[k] = (gen() % 5 == 0) ? 0 : 30 + 30 * (int32_t)(gen() % 3);
                nn[k] = npts[plan.classes[k].cloud];
            }
            const int ns = graph_plan_seeds(plan, kk.data(), nn.data(), &seed);
            int count = 0;
            for (int k = 0; k < K; ++k) {
                int first = -1;  // the cloud's first class that selects
                for (int j = 0; j < K && first < 0; ++j)
                    if (plan.classes[j].cloud == plan.classes[k].cloud && kk[j] > 0) first = j;
                if (seed[k].from < 0) {
                    // unseeded: it is the source, selects nothing, or asks for more than the source
                    const bool may = kk[k] > 0 && first >= 0 && first != k &&
                                     std::min<int64_t>(kk[k], nn[k]) <= std::min<int64_t>(kk[first], nn[first]);
                    expect(RANDOM, !may);
                    continue;
                }
                ++count;
                expect(RANDOM, seed[k].from == first && first < k && kk[k] > 0 && kk[first] > 0);
                expect(RANDOM, std::min<int64_t>(kk[k], nn[k]) <= std::min<int64_t>(kk[first], nn[first]));
                const double rho = plan.classes[k].norm_scale / plan.classes[first].norm_scale;
                expect(RANDOM, seed[k].rho2 == rho * rho);
                expect(RANDOM, seed[seed[k].from].from == -1);  // a source is never seeded itself
            }
            expect(RANDOM, ns == count);
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
