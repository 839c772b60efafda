// Host build of the selection plan of se3-icp_amd/csrc/graph.hpp (graph_plan_selection: what
// Engine::select_by_class decides before it queues anything; select_wave_tables: the three wave
// tables of Engine::setup_knn) for tests/test_select_host.py.
// Inputs: the five-scan chain and the map graph of seed_host.cpp, a posed graph with one rigid and
// one non-rigid pose, 300 random graphs; each under the default switches and under every switch
// that disables seeding or taking.
// Checks, each what a kernel relies on:
//   home     every class has exactly one home, its first use, and only homes select
//   seg      a use's segment points at its class's home, and at the home of nrm_from for normals
//   chunks   a use has share chunks, all of them, exactly when one of those is not itself
//   stores   seed store ranges are disjoint, inside [0, seed_floats), as long as the source's cloud
//   loads    every load equals a store of an earlier home of the same raw cloud
//   take     bit 1 only where a load exists, bit 0 only on a source some taker names
//   stride   a multiple of 4, at most kSmallK
//   off      seeding mode 1, an exact mode or knn_list: nothing seeds, nothing takes; seeding
//            modes 2 / 3, taking mode 1 or no donor table: nothing takes
//   waves    the three tables put each selecting cloud's (n + 7) / 8 waves into exactly one table;
//            a cloud with k_knn == 0 gets no wave
//   expected the chain, the map and the posed graph seed and take what DESIGN sections 17 / 21 say
//   planted_overlap / _early / _orphan / _twice   a planted defect is reported by its check
// --plant overlap|early|orphan|twice plants that defect in every plan before it is checked: the
// program must then fail.  Prints "<check> ok" or "<check> FAIL <count>" per check, then
// "checked <n>"; exits 1 if any failed.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "graph.hpp"

using namespace se3icp;

enum { HOME, SEG, CHUNKS, STORES, LOADS, TAKE, STRIDE, OFF, WAVES, EXPECTED, P_OVERLAP, P_EARLY, P_ORPHAN, P_TWICE, NCHECK };
static const char* const kNames[NCHECK] = {"home", "seg", "chunks", "stores", "loads", "take", "stride", "off", "waves", "expected",
                                           "planted_overlap", "planted_early", "planted_orphan", "planted_twice"};
enum Plant { NONE, OVERLAP, EARLY, ORPHAN, TWICE };

struct Tally {
    long bad[NCHECK] = {};
    long checked = 0;
    void expect(int c, bool ok) {
        ++checked;
        if (!ok) ++bad[c];
    }
};

// A graph as the engine hands it to the plan: the uses' layout, the donor table, the variants.
struct Input {
    GraphPlan plan;
    std::vector<CloudDev> clouds;  // [uses]
    std::vector<int32_t> donor, raw, rigid;
    int32_t k_lrf = 0;
};

static Input make_input(const GraphPlan& plan, const std::vector<int64_t>& npts, int32_t k_lrf, bool share_trees,
                        const std::vector<int32_t>& raw = {}, const std::vector<int32_t>& rigid = {}) {
    Input in;
    in.plan = plan;
    in.k_lrf = k_lrf;
    in.raw = raw;
    in.rigid = rigid;
    const int U = (int)plan.use_class.size();
    std::vector<int32_t> ucloud(U);
    std::vector<int64_t> un(U);
    int32_t off = 0;
    for (int u = 0; u < U; ++u) {
        ucloud[u] = plan.classes[plan.use_class[u]].cloud;
        un[u] = npts[ucloud[u]];
        in.clouds.push_back(CloudDev{off, (int32_t)un[u]});
        off += (int32_t)un[u];
    }
    if (graph_plan_trees(U, ucloud.data(), un.data(), share_trees, &in.donor) == 0) in.donor.clear();  // (as the engine keeps it)
    return in;
}

static void plant(Plant what, SelectPlan* sp, WaveTables* wt) {
    const int U = (int)sp->run.size();
    if (what == OVERLAP && sp->seeds) {  // the second store starts inside the first
        int first = -1;
        for (int u = 0; u < U; ++u)
            if (sp->seed_ref[u].store >= 0) {
                if (first < 0) first = u;
                else if (sp->seed_ref[u].store > sp->seed_ref[first].store) {
                    const int32_t was = sp->seed_ref[u].store;
                    for (SeedRef& r : sp->seed_ref)
                        if (r.load == was) r.load = was - 1;
                    sp->seed_ref[u].store = was - 1;
                    return;
                }
            }
    }
    if (what == EARLY && sp->seeds) {  // a source and the use it seeds change places
        for (int u = 0; u < U; ++u)
            if (sp->seed_ref[u].load >= 0)
                for (int a = 0; a < u; ++a)
                    if (sp->seed_ref[a].store == sp->seed_ref[u].load) {
                        std::swap(sp->seed_ref[a], sp->seed_ref[u]);
                        return;
                    }
    }
    if (what == ORPHAN && sp->takes) {  // a taker's source no longer stores lists
        for (int u = 0; u < U; ++u)
            if (sp->take_flag[u] & 1) {
                sp->take_flag[u] &= ~1;
                return;
            }
    }
    if (what == TWICE) {  // the first selecting cloud's waves are in table 1 as well
        const int nt = U + 1;
        for (int c = 0; c < U; ++c)
            if (wt->wb[c + 1] > wt->wb[c]) {
                for (int j = c + 1; j < nt; ++j) wt->wb[nt + j] += wt->wb[c + 1] - wt->wb[c];
                wt->nw_sd = wt->wb[nt + U];
                return;
            }
    }
}

// Every property of a plan and its wave tables; `t` counts what fails.
static void check(const Input& in, const SelectSwitches& sw, const SelectPlan& sp, const WaveTables& wt, Tally* t) {
    const GraphPlan& plan = in.plan;
    const int U = (int)plan.use_class.size(), K = (int)plan.classes.size();
    const bool se3 = plan.normalize;
    auto raw_of = [&](int u) { const int32_t v = plan.classes[plan.use_class[u]].cloud; return in.raw.empty() ? v : in.raw[v]; };
    // home
    t->expect(HOME, (int)sp.home.size() == K && (int)sp.run.size() == U && (int)sp.batch.size() == U);
    std::vector<int> homes(K, 0);
    int64_t full = 0;
    for (int u = 0; u < U; ++u) {
        const int k = plan.use_class[u];
        int first = 0;
        while (plan.use_class[first] != k) ++first;
        const bool is_home = sp.home[k] == u;
        homes[k] += is_home;
        t->expect(HOME, is_home == (first == u));
        t->expect(HOME, is_home || (sp.run[u].k_lrf == 0 && sp.run[u].k_nrm == 0 && sp.run[u].k_knn == 0));
        if (is_home) {
            const int32_t nrm = plan.classes[k].nrm_from == k ? plan.classes[k].k_nrm : 0;
            t->expect(HOME, sp.run[u].k_lrf == in.k_lrf && sp.run[u].k_nrm == nrm && sp.run[u].k_knn == std::max(in.k_lrf, nrm));
        }
        full += sp.run[u].k_knn > 0;
    }
    for (int k = 0; k < K; ++k) t->expect(HOME, homes[k] == 1);
    t->expect(HOME, sp.full == full);
    // seg, chunks
    size_t at = 0;
    for (int u = 0; u < U; ++u) {
        const GraphClass& gc = plan.classes[plan.use_class[u]];
        const int hf = sp.home[plan.use_class[u]], hn = sp.home[gc.nrm_from];
        const GraphSeg& g = sp.seg[u];
        t->expect(SEG, g.src_cloud == hf && g.src_off == in.clouds[hf].off && g.nrm_off == in.clouds[hn].off);
        t->expect(SEG, g.frames == ((hf != u && se3) ? 1 : 0));
        if ((hf != u && se3) || hn != u)
            for (int32_t p0 = 0; p0 < in.clouds[u].n; p0 += kChunk, ++at)
                t->expect(CHUNKS, at < sp.chunks.size() && sp.chunks[at].cloud == u && sp.chunks[at].p0 == p0);
    }
    t->expect(CHUNKS, at == sp.chunks.size());
    // off
    const bool may_seed = sw.lrf_seeding != 1 && sw.lrf_exact == 0 && !sw.knn_list;
    const bool may_take = may_seed && sw.lrf_seeding == 0 && sw.lrf_taking != 1 && (int)in.donor.size() == U;
    t->expect(OFF, may_seed || !sp.seeds);
    t->expect(OFF, may_take || !sp.takes);
    t->expect(OFF, sp.seeds || (!sp.takes && sp.seed_floats == 0 && sp.seeded == 0 && sp.cross == 0));
    t->expect(OFF, sp.takes || (sp.taking == 0 && sp.take_stride == 0));
    t->expect(OFF, sp.seed_mode == sw.lrf_seeding && sp.take_mode == sw.lrf_taking);
    if (sp.seeds) {
        t->expect(STORES, (int)sp.seed_ref.size() == U && sp.seed_floats <= INT32_MAX);
        int64_t loads = 0;
        for (int u = 0; u < U; ++u) {
            const SeedRef& r = sp.seed_ref[u];
            t->expect(STORES, r.store < 0 || r.load < 0);  // a source is never seeded itself
            if (r.store >= 0) {
                t->expect(STORES, sp.run[u].k_knn > 0 && r.store + (int64_t)in.clouds[u].n <= sp.seed_floats);
                for (int w = 0; w < u; ++w)
                    if (sp.seed_ref[w].store >= 0)
                        t->expect(STORES, r.store >= sp.seed_ref[w].store + in.clouds[w].n ||
                                              sp.seed_ref[w].store >= r.store + in.clouds[u].n);
            }
            if (r.load >= 0) {
                ++loads;
                int src = -1;
                for (int a = 0; a < u; ++a)
                    if (sp.seed_ref[a].store == r.load) src = a;
                t->expect(LOADS, sp.run[u].k_knn > 0 && src >= 0 && raw_of(src) == raw_of(u) && in.clouds[src].n == in.clouds[u].n);
                t->expect(LOADS, r.rho2 > 0.0);
            }
        }
        t->expect(LOADS, loads == sp.seeded && sp.cross <= sp.seeded);
    }
    if (sp.takes) {
        t->expect(TAKE, (int)sp.take_flag.size() == U && 2 * sp.seed_floats <= INT32_MAX);
        int64_t takers = 0;
        for (int u = 0; u < U; ++u) {
            const int32_t f = sp.take_flag[u];
            t->expect(TAKE, (f & ~3) == 0);
            if (f & 2) {
                ++takers;
                t->expect(TAKE, sp.seed_ref[u].load >= 0);
                int src = -1;  // its source stores lists
                for (int a = 0; a < U; ++a)
                    if (sp.seed_ref[a].store >= 0 && sp.seed_ref[a].store == sp.seed_ref[u].load) src = a;
                t->expect(TAKE, src >= 0 && (sp.take_flag[src] & 1));
                const int32_t kw = std::min(sp.run[u].k_knn, in.clouds[u].n);
                t->expect(STRIDE, kw > kSmallK || kw <= sp.take_stride);
            }
            if (f & 1) {
                bool named = false;
                for (int b = 0; b < U; ++b) named |= (sp.take_flag[b] & 2) && sp.seed_ref[b].load == sp.seed_ref[u].store;
                t->expect(TAKE, sp.seed_ref[u].store >= 0 && named);
            }
        }
        t->expect(TAKE, takers == sp.taking);
        t->expect(STRIDE, sp.take_stride % 4 == 0 && sp.take_stride <= kSmallK && sp.take_stride >= 0);
    }
    // waves
    const int nt = U + 1;
    t->expect(WAVES, (int)wt.wb.size() == 3 * nt && wt.wb[0] == 0 && wt.wb[nt] == 0 && wt.wb[2 * nt] == 0);
    t->expect(WAVES, wt.nw == wt.wb[U] && wt.nw_sd == wt.wb[nt + U] && wt.nw_tk == wt.wb[2 * nt + U]);
    int64_t all = 0;
    for (int c = 0; c < U; ++c) {
        const int32_t want = sp.run[c].k_knn > 0 ? (in.clouds[c].n + 7) / 8 : 0;
        int32_t w[3], tables = 0;
        for (int tb = 0; tb < 3; ++tb) {
            w[tb] = wt.wb[tb * nt + c + 1] - wt.wb[tb * nt + c];
            tables += w[tb] != 0;
        }
        all += want;
        t->expect(WAVES, w[0] >= 0 && w[1] >= 0 && w[2] >= 0 && w[0] + w[1] + w[2] == want && tables == (want > 0));
        const bool sd = sp.seeds && sp.seed_ref[c].load >= 0, tk = sd && sp.takes && (sp.take_flag[c] & 2);
        t->expect(WAVES, want == 0 || w[tk ? 2 : sd ? 1 : 0] == want);
    }
    t->expect(WAVES, (int64_t)wt.nw + wt.nw_sd + wt.nw_tk == all);
}

static Plant g_plant = NONE;

// Plan `in` under `sw`, check it; with a planted defect asked for on the command line, on the
// defective plan.
static SelectPlan plan_and_check(const Input& in, const SelectSwitches& sw, Tally* t, WaveTables* wt_out = nullptr) {
    const std::vector<CloudSetup> batch(in.clouds.size(), CloudSetup{});
    SelectPlan sp = graph_plan_selection(in.plan, in.clouds.data(), batch.data(), in.k_lrf, sw, in.donor, in.raw, in.rigid);
    const std::vector<CloudSetup>& st = sp.run;
    WaveTables wt = select_wave_tables((int32_t)in.clouds.size(), in.clouds.data(), st.data(), &sp);
    if (!sp.seeds) {  // a plan that seeds nothing lays its waves out as no plan does
        const WaveTables plain = select_wave_tables((int32_t)in.clouds.size(), in.clouds.data(), st.data(), nullptr);
        t->expect(WAVES, plain.wb == wt.wb && plain.nw_sd == 0 && plain.nw_tk == 0);
    }
    plant(g_plant, &sp, &wt);
    check(in, sw, sp, wt, t);
    if (wt_out) *wt_out = wt;
    return sp;
}

static const SelectSwitches kDefault{0, 0, 0, false, 0};
// every setting of the switches: (seeding, taking, exact, knn_list)
static void all_switches(const Input& in, Tally* t) {
    for (int sd = 0; sd <= 3; ++sd)
        for (int tk = 0; tk <= 2; ++tk)
            for (int ex = 0; ex <= 2; ++ex)
                for (int kl = 0; kl <= 1; ++kl)
                    for (int ps = 0; ps <= 1; ++ps) plan_and_check(in, SelectSwitches{sd, tk, ex, kl != 0, ps}, t);
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--plant") {
        const std::string w = argv[2];
        g_plant = w == "overlap" ? OVERLAP : w == "early" ? EARLY : w == "orphan" ? ORPHAN : w == "twice" ? TWICE : NONE;
        if (g_plant == NONE) return 2;
    } else if (argc != 1) {
        return 2;
    }
    Tally t;
    const double rad[5] = {69.15, 74.58, 73.83, 69.71, 71.00};
    double cen[15];
    for (int i = 0; i < 15; ++i) cen[i] = 0.25 * i - 1.0;
    const std::vector<int64_t> npts = {12500, 12501, 12502, 12503, 4099};

    // ---- the chain: scans 2 and 3 run under two scales; their second classes are seeded and take
    Input chain, map;
    {
        const int32_t src[4] = {1, 2, 3, 4}, tgt[4] = {0, 1, 2, 3};
        GraphPlan plan;
        graph_plan(4, src, tgt, true, 3.0, cen, rad, 20, 20, true, &plan);
        chain = make_input(plan, npts, 90, true);
        const SelectPlan sp = plan_and_check(chain, kDefault, &t);
        if (g_plant == NONE) {
            t.expect(EXPECTED, plan.classes.size() == 7 && sp.full == 7 && sp.chunks.size() == 7);  // (scan 1's second use: 7 chunks)
            t.expect(EXPECTED, sp.seeds && sp.seeded == 2 && sp.cross == 0 && sp.seed_floats == 12502 + 12503);
            t.expect(EXPECTED, sp.takes && sp.taking == 2 && sp.take_stride == 92);
        }
        all_switches(chain, &t);
        Input no_trees = make_input(plan, npts, 90, false);
        const SelectPlan off = plan_and_check(no_trees, kDefault, &t);
        if (g_plant == NONE) t.expect(EXPECTED, off.seeds && off.seeded == 2 && !off.takes);
    }
    // ---- the map: scans 0, 1, 3, 4 onto cloud 2 of the smallest radius: three takers of one source
    {
        const double rmap[5] = {69.15, 74.58, 60.0, 69.71, 71.00};
        const int32_t src[4] = {0, 1, 3, 4}, tgt[4] = {2, 2, 2, 2};
        GraphPlan plan;
        graph_plan(4, src, tgt, true, 3.0, cen, rmap, 20, 20, true, &plan);
        map = make_input(plan, npts, 150, true);  // (Kw = 150 > kSmallK: seeded, taken by the plan, stride capped)
        SelectPlan sp = plan_and_check(map, kDefault, &t);
        if (g_plant == NONE) {
            t.expect(EXPECTED, plan.classes.size() == 8 && sp.seeded == 3 && sp.seed_floats == 12502 && sp.chunks.empty());
            t.expect(EXPECTED, sp.takes && sp.taking == 3 && sp.take_stride == kSmallK);
        }
        map.k_lrf = 30;
        sp = plan_and_check(map, kDefault, &t);
        if (g_plant == NONE) t.expect(EXPECTED, sp.taking == 3 && sp.take_stride == 32);
        all_switches(map, &t);
        // vanilla: no frames, the normals of a cloud's first class serve the others
        graph_plan(4, src, tgt, false, 3.0, cen, rmap, 0, 30, true, &plan);
        Input van = make_input(plan, npts, 0, true);
        sp = plan_and_check(van, kDefault, &t);
        if (g_plant == NONE) t.expect(EXPECTED, !sp.seeds && sp.full == 1 && sp.chunks.size() == 3 * 7);
        all_switches(van, &t);
    }
    // ---- posed: variants 0 (cloud 0), 1 (cloud 1), 2 (cloud 0, rigid), 3 (cloud 0, not rigid)
    {
        const int vcloud[6] = {0, 1, 2, 1, 3, 1};
        const double scale[6] = {0.010, 0.010, 0.012, 0.012, 0.014, 0.014};
        std::vector<GraphUse> gu(8, GraphUse{});
        for (int u = 0; u < 6; ++u) {
            gu[u].cloud = vcloud[u];
            gu[u].k_nrm = 20;
            gu[u].norm_scale = scale[u];
            gu[u].norm_center[0] = 0.5 * vcloud[u];
        }
        gu[6] = gu[4];  // the non-rigid variant under a second scale
        gu[6].norm_scale = 0.016;
        gu[7] = gu[1];
        gu[7].norm_scale = 0.016;
        GraphPlan plan;
        graph_plan_uses(8, gu.data(), true, true, &plan);
        const std::vector<int64_t> vn = {3001, 2999, 3001, 3001};
        Input posed = make_input(plan, vn, 30, true, {0, 1, 0, 0}, {1, 1, 1, 0});
        SelectPlan sp = plan_and_check(posed, kDefault, &t);
        if (g_plant == NONE) {
            // variant 2 from variant 0 (across), variant 3's second class from its first, cloud 1's three later classes
            t.expect(EXPECTED, plan.classes.size() == 8 && sp.seeded == 5 && sp.cross == 1);
            t.expect(EXPECTED, sp.seed_ref[2].load == sp.seed_ref[0].store && sp.seed_ref[4].store >= 0 &&
                                   sp.seed_ref[6].load == sp.seed_ref[4].store);
            t.expect(EXPECTED, sp.taking == 4 && !(sp.take_flag[2] & 2));  // (another variant has another tree order)
            sp = plan_and_check(posed, SelectSwitches{0, 0, 0, false, 1}, &t);
            t.expect(EXPECTED, sp.seeded == 4 && sp.cross == 0 && sp.seed_ref[2].load < 0);
        }
        all_switches(posed, &t);
    }
    // ---- random graphs
    {
        std::mt19937_64 gen(23);
        for (int trial = 0; trial < 300; ++trial) {
            const int C = 1 + (int)(gen() % 6), P = 1 + (int)(gen() % 12);
            std::vector<double> r(C), ce(3 * C);
            std::vector<int64_t> n(C);
            for (int c = 0; c < C; ++c) {
                r[c] = 50.0 + (double)(gen() % 4);  // (radii repeat: classes merge)
                n[c] = 1 + (int64_t)(gen() % (trial % 7 == 0 ? 6000 : 300));
                for (int a = 0; a < 3; ++a) ce[3 * c + a] = (double)(gen() % 7) - 3.0;
            }
            std::vector<int32_t> src(P), tgt(P);
            for (int p = 0; p < P; ++p) {
                src[p] = (int32_t)(gen() % C);
                tgt[p] = (int32_t)(gen() % C);
            }
            const bool se3 = gen() % 4 != 0, dedupe = gen() % 5 != 0;
            GraphPlan plan;
            graph_plan(P, src.data(), tgt.data(), se3, 3.0, ce.data(), r.data(), gen() % 2 ? 20 : 0, 20 + 10 * (int)(gen() % 2),
                       dedupe, &plan);
            const Input in = make_input(plan, n, se3 ? 10 + 40 * (int32_t)(gen() % 4) : 0, gen() % 4 != 0);
            plan_and_check(in, kDefault, &t);
            plan_and_check(in, SelectSwitches{(int)(gen() % 4), (int)(gen() % 3), (int)(gen() % 5 == 0), gen() % 7 == 0, 0}, &t);
        }
    }
    // ---- planted defects: each is reported by its check on the chain or the map
    if (g_plant == NONE) {
        const struct { Plant what; int check, reports; const Input* in; } cases[4] = {
            {OVERLAP, P_OVERLAP, STORES, &chain}, {EARLY, P_EARLY, LOADS, &chain}, {ORPHAN, P_ORPHAN, TAKE, &map},
            {TWICE, P_TWICE, WAVES, &chain}};
        for (const auto& c : cases) {
            Tally clean, dirty;
            WaveTables wt;
            SelectPlan sp = plan_and_check(*c.in, kDefault, &clean, &wt);
            plant(c.what, &sp, &wt);
            check(*c.in, kDefault, sp, wt, &dirty);
            long other = 0;
            for (int k = 0; k < NCHECK; ++k) other += clean.bad[k];
            t.expect(c.check, other == 0 && dirty.bad[c.reports] > 0);
        }
    }

    int rc = 0;
    for (int k = 0; k < NCHECK; ++k) {
        if (t.bad[k]) {
            std::printf("%s FAIL %ld\n", kNames[k], t.bad[k]);
            rc = 1;
        } else {
            std::printf("%s ok\n", kNames[k]);
        }
    }
    std::printf("checked %ld\n", t.checked);
    return rc;
}
