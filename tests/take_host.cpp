// take_host.cpp — host checks of taking a source class's neighbour lists:
//   * the plan (se3-icp_amd/csrc/graph.hpp, graph_plan_takes) over graph_plan_seeds' result and
//     graph_plan_trees' donor table: the chain, the map, unequal Kw, another centre, posed
//     variants, tree sharing off, sharing level 1, random graphs against a restatement;
//   * narrow_bound against widen_bound and key_floor (se3-icp_amd/csrc/lrf_bounds.hpp);
//   * the certificate's bound, take_bound, against long double evaluation over random and
//     adversarial coordinates: large norms with tiny distances, scales one ulp apart, rho near 1
//     and far from 1, near-subnormal values.  For each the computed bound never exceeds what the
//     point outside the list really has.
// Prints "<check> ok" per check and "checked <n>"; exits nonzero on a failure.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "graph.hpp"
#include "lrf_bounds.hpp"

using namespace se3icp;

static long g_checked = 0;
static bool g_ok = true;
#define CHECK(c)                                                              \
    do {                                                                      \
        ++g_checked;                                                          \
        if (!(c)) {                                                           \
            if (g_ok) std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            g_ok = false;                                                     \
            ok = false;                                                       \
        }                                                                     \
    } while (0)

// uses over clouds under the run_se3_* normalization: (cloud, scale, centre tag)
struct U { int cloud; double scale; double centre; };

struct Planned {
    GraphPlan plan;
    std::vector<SeedClass> seed;
    std::vector<uint8_t> take;
    std::vector<int32_t> home, donor, kk;
    std::vector<int64_t> nn;
    int taking = 0;
};

static Planned plan_of(const std::vector<U>& uses, const std::vector<int64_t>& npts, const std::vector<int32_t>& k_of_use,
                       bool dedupe, bool share_trees, bool normalize = true) {
    Planned P;
    std::vector<GraphUse> gu(uses.size());
    for (size_t u = 0; u < uses.size(); ++u) {
        gu[u] = GraphUse{};
        gu[u].cloud = uses[u].cloud;
        gu[u].k_nrm = 0;
        gu[u].norm_scale = uses[u].scale;
        gu[u].norm_center[0] = uses[u].centre;
    }
    graph_plan_uses((int32_t)uses.size(), gu.data(), normalize, dedupe, &P.plan);
    const int K = (int)P.plan.classes.size();
    P.home.assign(K, -1);
    for (int u = 0; u < (int)uses.size(); ++u)
        if (P.home[P.plan.use_class[u]] < 0) P.home[P.plan.use_class[u]] = u;
    P.kk.resize(K);
    P.nn.resize(K);
    for (int k = 0; k < K; ++k) {
        P.kk[k] = k_of_use[P.home[k]];
        P.nn[k] = npts[P.plan.classes[k].cloud];
    }
    graph_plan_seeds(P.plan, P.kk.data(), P.nn.data(), &P.seed);
    std::vector<int32_t> ucloud(uses.size());
    std::vector<int64_t> un(uses.size());
    for (size_t u = 0; u < uses.size(); ++u) {
        ucloud[u] = uses[u].cloud;
        un[u] = npts[uses[u].cloud];
    }
    const int nad = graph_plan_trees((int32_t)uses.size(), ucloud.data(), un.data(), share_trees, &P.donor);
    if (nad == 0) P.donor.clear();  // (the engine keeps the table only when a slot adopted)
    P.taking = graph_plan_takes(P.plan, P.seed, P.kk.data(), P.nn.data(), P.home.data(), P.donor, &P.take);
    return P;
}

static int count(const std::vector<uint8_t>& t) {
    int n = 0;
    for (uint8_t x : t) n += x != 0;
    return n;
}

// ------------------------------------------------------------------------------ the plan
static bool check_chain() {
    bool ok = true;
    // scan i+1 onto scan i over five scans: uses src 1, tgt 0, src 2, tgt 1, ...; pair scales differ
    std::vector<U> uses;
    const double sc[4] = {0.011, 0.012, 0.013, 0.014};
    for (int p = 0; p < 4; ++p) {
        uses.push_back(U{p + 1, sc[p], (double)(p + 1)});
        uses.push_back(U{p, sc[p], (double)p});
    }
    const std::vector<int64_t> n = {1000, 1001, 1002, 1003, 1004};
    Planned P = plan_of(uses, n, std::vector<int32_t>(8, 91), true, true);
    CHECK(P.plan.classes.size() == 8);
    CHECK(P.taking == 3 && count(P.take) == 3);  // scans 1, 2, 3: their second class takes from their first
    for (int k = 0; k < 8; ++k) CHECK((P.take[k] != 0) == (P.seed[k].from >= 0));
    for (int k = 0; k < 8; ++k)
        if (P.take[k]) CHECK(P.plan.classes[P.seed[k].from].cloud == P.plan.classes[k].cloud);
    if (ok) std::printf("chain ok\n");
    return ok;
}

static bool check_map() {
    bool ok = true;
    // four scans onto one map: the map (cloud 0) under four scales, three takers of one source
    std::vector<U> uses;
    for (int p = 0; p < 4; ++p) {
        uses.push_back(U{p + 1, 0.01 + 0.001 * p, (double)(p + 1)});
        uses.push_back(U{0, 0.01 + 0.001 * p, 0.0});
    }
    Planned P = plan_of(uses, {5000, 900, 901, 902, 903}, std::vector<int32_t>(8, 30), true, true);
    CHECK(P.taking == 3);
    int src = -1;
    for (int k = 0; k < (int)P.take.size(); ++k)
        if (P.take[k]) {
            CHECK(P.plan.classes[k].cloud == 0);
            CHECK(src < 0 || src == P.seed[k].from);
            src = P.seed[k].from;
        }
    CHECK(src >= 0 && !P.take[src]);
    if (ok) std::printf("map ok\n");
    return ok;
}

static bool check_kw() {
    bool ok = true;
    // cloud 0 under two scales; the second class asks for fewer neighbours: seeded, not taken
    std::vector<U> uses = {U{0, 0.01, 0.0}, U{1, 0.01, 1.0}, U{0, 0.02, 0.0}, U{2, 0.02, 2.0}};
    Planned P = plan_of(uses, {500, 400, 300}, {90, 90, 30, 30}, true, true);
    CHECK(P.seed[P.plan.use_class[2]].from == P.plan.use_class[0]);
    CHECK(P.taking == 0);
    // the same k: taken; k over n on both sides (Kw = n): taken
    P = plan_of(uses, {500, 400, 300}, {90, 90, 90, 90}, true, true);
    CHECK(P.taking == 1 && P.take[P.plan.use_class[2]]);
    P = plan_of(uses, {60, 400, 300}, {90, 90, 150, 150}, true, true);
    CHECK(P.taking == 1);
    if (ok) std::printf("kw ok\n");
    return ok;
}

static bool check_centre() {
    bool ok = true;
    // another centre: not seeded, so not taken
    std::vector<U> uses = {U{0, 0.01, 0.0}, U{1, 0.01, 1.0}, U{0, 0.02, 0.5}, U{2, 0.02, 2.0}};
    Planned P = plan_of(uses, {500, 400, 300}, {90, 90, 90, 90}, true, true);
    CHECK(P.taking == 0 && count(P.take) == 0);
    // no normalization: nothing is seeded or taken
    P = plan_of(uses, {500, 400, 300}, {90, 90, 90, 90}, true, true, false);
    CHECK(P.taking == 0);
    if (ok) std::printf("centre ok\n");
    return ok;
}

static bool check_posed() {
    bool ok = true;
    // Two variants (0: unposed, 3: posed) of raw cloud 0: graph_plan_seeds_posed seeds across them,
    // but a posed variant is another cloud with another tree order, and nothing takes across.
    std::vector<U> uses = {U{0, 0.01, 0.0}, U{1, 0.01, 1.0}, U{3, 0.02, 0.25}, U{2, 0.02, 2.0}, U{3, 0.03, 0.25}, U{1, 0.03, 1.0}};
    std::vector<GraphUse> gu(uses.size());
    for (size_t u = 0; u < uses.size(); ++u) {
        gu[u] = GraphUse{};
        gu[u].cloud = uses[u].cloud;
        gu[u].norm_scale = uses[u].scale;
        gu[u].norm_center[0] = uses[u].centre;
    }
    GraphPlan plan;
    graph_plan_uses((int32_t)uses.size(), gu.data(), true, true, &plan);
    const int K = (int)plan.classes.size();
    std::vector<int32_t> home(K, -1), kk(K, 60);
    for (int u = 0; u < (int)uses.size(); ++u)
        if (home[plan.use_class[u]] < 0) home[plan.use_class[u]] = u;
    const std::vector<int64_t> npts = {700, 600, 500, 700};
    std::vector<int64_t> nn(K);
    for (int k = 0; k < K; ++k) nn[k] = npts[plan.classes[k].cloud];
    const int32_t raw[4] = {0, 1, 2, 0}, rigid[4] = {1, 1, 1, 1};
    std::vector<SeedClass> seed;
    int32_t cross = 0;
    const int seeded = graph_plan_seeds_posed(plan, kk.data(), nn.data(), raw, rigid, true, &seed, &cross);
    CHECK(seeded == 3 && cross == 2);  // variant 3's two classes from variant 0's, cloud 1's second from its first
    std::vector<int32_t> ucloud(uses.size()), donor;
    std::vector<int64_t> un(uses.size());
    for (size_t u = 0; u < uses.size(); ++u) {
        ucloud[u] = uses[u].cloud;
        un[u] = npts[uses[u].cloud];
    }
    graph_plan_trees((int32_t)uses.size(), ucloud.data(), un.data(), true, &donor);
    std::vector<uint8_t> take;
    const int taking = graph_plan_takes(plan, seed, kk.data(), nn.data(), home.data(), donor, &take);
    CHECK(taking == 1);  // cloud 1's second class only
    for (int k = 0; k < K; ++k)
        if (take[k]) CHECK(plan.classes[k].cloud == 1);
    // a plan that names another tree group for a class of the same variant: not taken
    std::vector<int32_t> split = donor;
    for (int32_t& d : split) d = -1;
    CHECK(graph_plan_takes(plan, seed, kk.data(), nn.data(), home.data(), split, &take) == 0);
    if (ok) std::printf("posed ok\n");
    return ok;
}

static bool check_treeoff() {
    bool ok = true;
    std::vector<U> uses = {U{0, 0.01, 0.0}, U{1, 0.01, 1.0}, U{0, 0.02, 0.0}, U{2, 0.02, 2.0}};
    Planned P = plan_of(uses, {500, 400, 300}, {90, 90, 90, 90}, true, false);
    CHECK(P.seed[P.plan.use_class[2]].from >= 0);  // still seeded
    CHECK(P.taking == 0 && count(P.take) == 0);
    if (ok) std::printf("treeoff ok\n");
    return ok;
}

static bool check_level1() {
    bool ok = true;
    std::vector<U> uses = {U{0, 0.01, 0.0}, U{1, 0.01, 1.0}, U{0, 0.02, 0.0}, U{2, 0.02, 2.0}};
    Planned P = plan_of(uses, {500, 400, 300}, {90, 90, 90, 90}, false, false);
    CHECK(P.plan.classes.size() == 4 && P.taking == 0 && count(P.take) == 0);
    P = plan_of(uses, {500, 400, 300}, {90, 90, 90, 90}, false, true);  // (a class per use, whatever the trees do)
    CHECK(P.taking == 0);
    if (ok) std::printf("level1 ok\n");
    return ok;
}

static bool check_random() {
    bool ok = true;
    std::mt19937 rng(7);
    for (int it = 0; it < 400; ++it) {
        const int C = 1 + (int)(rng() % 6), P2 = 2 * (1 + (int)(rng() % 8));
        std::vector<int64_t> n(C);
        for (auto& x : n) x = 5 + (int64_t)(rng() % 200);
        std::vector<U> uses(P2);
        std::vector<int32_t> kuse(P2);
        for (int u = 0; u < P2; ++u) {
            uses[u] = U{(int)(rng() % C), 0.01 * (1 + (int)(rng() % 3)), (rng() % 5 == 0) ? 0.5 : 0.0};
            kuse[u] = (rng() % 4 == 0) ? 30 : 90;
        }
        const bool dedupe = rng() % 5 != 0, share = rng() % 4 != 0;
        Planned P = plan_of(uses, n, kuse, dedupe, share);
        int want = 0;
        for (int k = 0; k < (int)P.take.size(); ++k) {
            const int a = P.seed[k].from;
            bool t = a >= 0 && share && dedupe && !P.donor.empty();
            if (t) {
                const int64_t kw = std::min<int64_t>(P.kk[k], P.nn[k]), kwa = std::min<int64_t>(P.kk[a], P.nn[a]);
                const int hk = P.home[k], ha = P.home[a];
                const int gk = P.donor[hk] >= 0 ? P.donor[hk] : hk, ga = P.donor[ha] >= 0 ? P.donor[ha] : ha;
                t = kw == kwa && gk == ga && P.plan.classes[k].cloud == P.plan.classes[a].cloud;
            }
            CHECK((P.take[k] != 0) == t);
            want += t;
            if (P.take[k]) {  // a taker's source never takes, and they are slots of one cloud
                CHECK(!P.take[a]);
                CHECK(uses[P.home[k]].cloud == uses[P.home[a]].cloud);
            }
        }
        CHECK(P.taking == want);
    }
    if (ok) std::printf("random ok\n");
    return ok;
}

// ------------------------------------------------------------------------------ the bounds
static long double err_ld(long double d, long double S) {
    const long double u = 5.9604645e-08L;
    return 1.25L * (2.L * u * S * sqrtl(d > 0 ? d : 0) + 6.L * u * d + 4.L * u * u * S * S) + 1e-30L;
}

static bool check_narrow() {
    bool ok = true;
    std::mt19937_64 rng(3);
    std::uniform_real_distribution<double> un(0.0, 1.0);
    for (int it = 0; it < 200000; ++it) {
        const float S = (float)std::exp(std::log(1e-3) + un(rng) * std::log(1e6));
        const float b = (float)((double)S * (double)S * std::exp(-un(rng) * 40.0));
        const unsigned t = knn::f32_bits(b) | knn::kIdBits;
        const float T = knn::bits_f32(t);
        const float nb = knn::narrow_bound(t, S);
        // rounded down: at or below the bound minus one error, evaluated in long double
        CHECK((long double)nb <= std::max(0.0L, (long double)T - err_ld(T, S)));
        CHECK(nb >= 0.f && nb <= T);
        // against widen_bound: a list collected under widen_bound(t) leaves out nothing whose exact
        // distance is within the value of t plus one error, so its narrow_bound lies above that
        const unsigned w = knn::widen_bound(t, S);
        // (where the error is small against the bound itself; nearer the f32 noise floor the
        // lower bound may come out 0, which only sends the taker's wave to the redo)
        if (w < knn::kAll && err_ld(T, S) <= 0.125L * T) {
            const float nw = knn::narrow_bound(w, S);
            CHECK((long double)nw >= (long double)T + 0.7L * err_ld(T, S));
            CHECK(nw <= knn::bits_f32(w));
        }
        // key_floor: at least one ulp down, so below every f64 that rounds to the key
        const float kf = knn::key_floor(T);
        if (T > 1e-37f) CHECK(kf < T && (double)kf <= (double)T * (1.0 - 0x1p-24));
    }
    CHECK(knn::narrow_bound(knn::kAll, 1.f) == FLT_MAX);
    CHECK(knn::narrow_bound(0u | knn::kIdBits, 1.f) == 0.f);
    CHECK(knn::narrow_bound(knn::f32_bits(1e-14f), 2.f) == 0.f);  // (below the error: clamped)
    if (ok) std::printf("narrow ok\n");
    return ok;
}

// nanoflann's squared distance as the kernels compute it (no contraction)
static double l2(const double* a, const double* b) {
    volatile double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    volatile double s0 = d0 * d0, s1 = d1 * d1, s2 = d2 * d2;
    volatile double s01 = s0 + s1;
    return s01 + s2;
}
static float f32_down(double x) {
    float f = (float)x;
    if ((double)f > x) f = std::nextafterf(f, -INFINITY);
    return f;
}
static float f32_up(double x) {
    float f = (float)x;
    if ((double)f < x) f = std::nextafterf(f, INFINITY);
    return f;
}

// one outside point p seen from q in class a and class b: the bound from the tightest Lb the
// source could store must not exceed p's computed key in class b, nor its real squared distance
static bool one_case(const double* xq, const double* xp, double sa, double sb, long* n_pos) {
    bool ok = true;
    double Aq[3], Ap[3], Bq[3], Bp[3];
    for (int i = 0; i < 3; ++i) {
        volatile double a = xq[i] * sa, b = xp[i] * sa, c = xq[i] * sb, d = xp[i] * sb;
        Aq[i] = a; Ap[i] = b; Bq[i] = c; Bp[i] = d;
    }
    const double Ka = l2(Aq, Ap), Kb = l2(Bq, Bp);
    if (!std::isfinite(Ka) || !std::isfinite(Kb)) return true;
    const float lb = f32_down(Ka);
    volatile double rho = sb / sa;
    volatile double rho2 = rho * rho;
    long double nq = 0, np = 0, real = 0;
    for (int i = 0; i < 3; ++i) {
        nq += (long double)Bq[i] * Bq[i];
        np += (long double)Bp[i] * Bp[i];
        const long double d = (long double)Bq[i] - (long double)Bp[i];
        real += d * d;
    }
    const float nb = f32_up((double)(sqrtl(nq) + sqrtl(np)) * 1.0001);
    if (!std::isfinite(nb) || !std::isfinite(rho2)) return true;
    const double bound = knn::take_bound(rho2, lb, nb);
    CHECK(bound <= Kb);
    CHECK((long double)bound <= real);
    // halved bounds stay sound, and a bound is never negative or NaN
    CHECK(knn::take_bound(rho2, 0.5f * lb, nb) <= bound && bound >= 0.0);
    if (bound > 0.0) ++*n_pos;
    return ok;
}

static bool check_certificate() {
    bool ok = true;
    std::mt19937_64 rng(5);
    std::uniform_real_distribution<double> un(-1.0, 1.0), u01(0.0, 1.0);
    long n_pos = 0, n_all = 0;
    auto run = [&](double mag, double dist, double sa, double sb) {
        double xq[3], xp[3];
        for (int i = 0; i < 3; ++i) {
            xq[i] = mag * un(rng);
            xp[i] = xq[i] + dist * un(rng);
        }
        ok &= one_case(xq, xp, sa, sb, &n_pos);
        ++n_all;
    };
    for (int it = 0; it < 200000; ++it) {
        // random: coordinates of a scan, scales of normalized pairs
        const double sa = 0.005 + 0.05 * u01(rng), sb = 0.005 + 0.05 * u01(rng);
        run(100.0, std::exp(-12.0 * u01(rng)) * 100.0, sa, sb);
    }
    for (int it = 0; it < 50000; ++it) {
        const double sa = 0.01 + 0.01 * u01(rng);
        // large norms with tiny distances
        run(1e6, 1e-6 * u01(rng), sa, sa * (1.0 + u01(rng)));
        run(1e9, 1e-3, 1.0, 3.0 * u01(rng) + 1e-3);
        // scales one ulp apart, and equal
        run(50.0, 0.5 * u01(rng), sa, std::nextafter(sa, 1.0));
        run(50.0, 0.5 * u01(rng), sa, std::nextafter(sa, 0.0));
        run(50.0, 0.5 * u01(rng), sa, sa);
        // rho near 1 and far from 1
        run(50.0, u01(rng), sa, sa * (1.0 + 1e-9 * un(rng)));
        run(50.0, u01(rng), sa, sa * 1e6);
        run(50.0, u01(rng), sa, sa * 1e-6);
        run(50.0, u01(rng), 1e-3 * sa, 1e5);
        // near-subnormal values: products that leave the normal range, distances whose squares do
        run(1e-150, 1e-152, sa, sa * 0.5);
        run(1e-300, 1e-302, sa, 1e-9);
        run(1e-18, 1e-21, sa, 1.0);
        run(1e-19, 3e-21, 1.0, 0.7);  // (a bound among the subnormal f32)
        run(3e-160, 1e-160 * u01(rng), 1.0, 0.5);
    }
    CHECK(n_pos > n_all / 2);  // (the bound is not vacuous: it is positive for most cases)
    if (ok) std::printf("certificate ok\n");
    return ok;
}

int main() {
    bool all = true;
    all &= check_chain();
    all &= check_map();
    all &= check_kw();
    all &= check_centre();
    all &= check_posed();
    all &= check_treeoff();
    all &= check_level1();
    all &= check_random();
    all &= check_narrow();
    all &= check_certificate();
    std::printf("checked %ld\n", g_checked);
    return all && g_ok ? 0 : 1;
}
