// cert_host.cpp — host checks of the NN certificates' arithmetic (se3-icp_amd/csrc/nn_cert.hpp,
// DESIGN section 23) against long double evaluation:
//   err     |f32 squared distance - exact| <= f32_err for the three ways the kernels sum it (one
//           FMA chain, two half chains and an add, the seed's chain from zero), D = 3 and 12, over
//           random pairs and the corners that make each term of the bound dominate, rounding
//           midpoints, an engineered pair whose seven roundings all err the same way, and the
//           3-D shifted form at centre norms up to 1e7;
//   cert    D1 / L2 of a simulated search (f32 top-2 of a visit set, final threshold thr, skipped
//           targets behind their inflated boxes): winner <= D1, every other target >= L2;
//   delta   settle_dl >= the long-double distance of the f64-rounded queries at two poses;
//   settle  settle_holds implies the long-double inequality and the squared-distance margin;
//   widen   widen_radius is monotone in the margin and stays in [a1 + 3 err(a1), a2 + 3 err(a2)];
//   ring    cert_usable never admits a certificate whose pose-ring row has been rewritten;
//   planted six planted defects, each failing its check on the same inputs.
// Prints "<check> ok" per check, "slack_err <r>" (largest error / bound), "slack_dl <r>" and
// "slack_dl_large <r>" (largest dl / exact - 1 over displacements above 1e-9 |q| and above
// 1e-3 |q|), "checked <n>"; exits nonzero on a failure.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "nn_cert.hpp"

using namespace se3icp;
typedef long double ld;

static long g_checked = 0;
static bool g_ok = true;
static void report(const char* name, bool ok) {
    if (ok) std::printf("%s ok\n", name);
    else { std::printf("%s FAILED\n", name); g_ok = false; }
}

static std::mt19937_64 rng(20260923);
static double uni(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
static double logu(double a, double b) { return std::exp(uni(std::log(a), std::log(b))); }
static void unit(double* v, int D) {
    std::normal_distribution<double> g;
    double n = 0;
    for (int r = 0; r < D; ++r) { v[r] = g(rng); n += v[r] * v[r]; }
    n = std::sqrt(n);
    for (int r = 0; r < D; ++r) v[r] /= n;
}

// ---------------------------------------------------------------- err
typedef float (*ErrFn)(float, float, float, int);
static float err_no_norms(float d, float, float, int D) { return nncert::f32_err(d, 0.f, 0.f, D); }
static float err_d_not_d3(float d, float na, float nb, int D) {
    const float u = 5.9604645e-08f, s = na + nb;
    return 1.25f * (2.f * u * s * sqrtf(fmaxf(d, 0.f)) + (float)D * u * d + 4.f * u * u * s * s) + 1e-30f;
}

struct Pair { int D; double a[12], b[12]; };

static float dist_chain(const float* a, const float* b, int D) {  // acc = e0 e0; fmaf ...
    float e = a[0] - b[0], acc = e * e;
    for (int r = 1; r < D; ++r) { e = a[r] - b[r]; acc = fmaf(e, e, acc); }
    return acc;
}
static float dist_seed(const float* a, const float* b, int D) {  // s = 0; fmaf ...
    float s = 0.f;
    for (int r = 0; r < D; ++r) { const float e = a[r] - b[r]; s = fmaf(e, e, s); }
    return s;
}
static float dist_packed(const float* a, const float* b, int D) {  // even / odd chains and one add
    float s0 = 0.f, s1 = 0.f;
    for (int r = 0; r < D; r += 2) {
        const float e0 = a[r] - b[r], e1 = a[r + 1] - b[r + 1];
        if (r == 0) { s0 = e0 * e0; s1 = e1 * e1; }
        else { s0 = fmaf(e0, e0, s0); s1 = fmaf(e1, e1, s1); }
    }
    return s0 + s1;
}
static double norm_of(const double* a, int D) {
    double n = 0;
    for (int r = 0; r < D; ++r) n += a[r] * a[r];
    return std::sqrt(n);
}

static std::vector<Pair> g_pairs;
static void add_pair(int D, const double* a, const double* b) {
    Pair p;
    p.D = D;
    std::memset(p.a, 0, sizeof(p.a));
    std::memset(p.b, 0, sizeof(p.b));
    std::memcpy(p.a, a, sizeof(double) * D);
    std::memcpy(p.b, b, sizeof(double) * D);
    g_pairs.push_back(p);
}
static double f32_midpoint(double x, double toward) {  // just short of the midpoint next to float(x)
    const float f = (float)x;
    const float g = nextafterf(f, toward > 0 ? INFINITY : -INFINITY);
    return 0.5 * ((double)f + (double)g) * (1.0 - (toward > 0 ? 1 : -1) * (f > 0 ? 1 : -1) * 0x1p-50);
}
static void build_pairs() {
    for (int D : {3, 12}) {
        double a[12], b[12], dir[12];
        for (int i = 0; i < 20000; ++i) {  // random pairs over many scales
            const double sa = logu(1e-3, 1e3), sb = logu(1e-3, 1e3);
            unit(a, D); unit(b, D);
            for (int r = 0; r < D; ++r) { a[r] *= sa * uni(0, 1); b[r] *= sb * uni(0, 1); }
            add_pair(D, a, b);
        }
        for (int i = 0; i < 20000; ++i) {  // norms 10, distances 1e-6 .. 1e-3: the (na + nb) sqrt(d) term
            unit(a, D); unit(dir, D);
            const double dist = logu(1e-6, 1e-3);
            for (int r = 0; r < D; ++r) { a[r] *= 10.0; b[r] = a[r] + dist * dir[r]; }
            add_pair(D, a, b);
        }
        for (int i = 0; i < 20000; ++i) {  // distances comparable to the norms: the (D + 3) u d term
            unit(a, D);
            const double s = logu(1e-2, 1e2);
            for (int r = 0; r < D; ++r) { a[r] *= s; b[r] = -a[r] * uni(0.9, 1.1); }
            add_pair(D, a, b);
        }
        for (int i = 0; i < 10000; ++i) {  // d = 0 and a few f32 ulps of the coordinates: the u^2 term
            unit(a, D);
            const double s = logu(1e-2, 1e2);
            for (int r = 0; r < D; ++r) {
                a[r] *= s;
                const int k = (int)(rng() % 7) - 3;
                b[r] = (i & 1) ? a[r] * (1.0 + k * 0x1p-24) : a[r];
            }
            add_pair(D, a, b);
        }
        for (int i = 0; i < 20000; ++i) {  // coordinates on f32 rounding midpoints, far and near pairs
            unit(a, D); unit(dir, D);
            const double s = logu(1e-1, 1e1), dist = (i & 1) ? logu(1e-5, 1e-2) : s;
            for (int r = 0; r < D; ++r) {
                a[r] = f32_midpoint(a[r] * s, (rng() & 1) ? 1 : -1);
                b[r] = f32_midpoint((i & 2) ? -a[r] : a[r] + dist * dir[r], (rng() & 1) ? 1 : -1);
            }
            add_pair(D, a, b);
        }
    }
    {   // D = 3, every rounding down: inputs (2 x u), the difference (u), the square and both FMAs
        // (3 x u); d ~ 1, true error ~ 7 u d
        const double h = 0x1p-25 * (1.0 - 0x1p-20);
        const double a[3] = {0.5 + 0x1p-24 + h, 0x1p-13, 0x1p-13};
        const double b[3] = {-(0.5 + 0x1p-12 + h), -0x1p-13, -0x1p-13};
        add_pair(3, a, b);
    }
    for (int i = 0; i < 20000; ++i) {  // D = 3 shifted: Q - f32_center at centre norms up to 1e7
        double c[3], a[3], b[3], dir[3];
        unit(c, 3); unit(a, 3); unit(dir, 3);
        const double cn = logu(1.0, 1e7), dist = logu(1e-5, 1.0);
        for (int r = 0; r < 3; ++r) {
            const double Q = c[r] * cn + a[r] * uni(0, 1), T = Q + dist * dir[r];  // (f64-rounded, as stored)
            a[r] = Q - c[r] * cn;
            b[r] = T - c[r] * cn;
        }
        add_pair(3, a, b);
    }
}

// largest |d_f32 - d_exact| / bound over the pairs and the three sums; < 0: a NaN appeared
static double err_ratio(ErrFn fn) {
    double worst = 0;
    for (const Pair& p : g_pairs) {
        float af[12], bf[12];
        ld exact = 0;
        for (int r = 0; r < p.D; ++r) {
            af[r] = (float)p.a[r];
            bf[r] = (float)p.b[r];
            const ld e = (ld)p.a[r] - (ld)p.b[r];
            exact += e * e;
        }
        const float na = (float)norm_of(p.a, p.D) * 1.000001f;          // as the searches set them
        const float nb = (float)(norm_of(p.b, p.D) * (1 + 1e-6));
        const float d[3] = {dist_chain(af, bf, p.D), dist_seed(af, bf, p.D), p.D == 12 ? dist_packed(af, bf, p.D) : dist_chain(af, bf, p.D)};
        for (float df : d) {
            const ld e = fabsl((ld)df - exact);
            const double ratio = (double)(e / (ld)fn(df, na, nb, p.D));
            ++g_checked;
            if (!(ratio <= worst)) worst = ratio;
            if (ratio != ratio) return -1;
        }
    }
    return worst;
}

// ---------------------------------------------------------------- cert
typedef float (*L2Fn)(float, float, float, float, int);
static float l2_no_thr(float d2, float, float na, float nb, int D) {
    return sqrtf(fmaxf(d2 - nncert::f32_err(d2, na, nb, D), 0.f)) * (1.f - 1e-6f);
}
// f32 bound of the target's own box, inflated as k_tree_leafbox does, against the f32 query.
// The kernel's `fabsf(v) * 4.8e-7f + 1e-30f` is contracted to one v_fma_f32: fmaf here, whatever
// this file's own contraction setting (the tree record's tests hold the kernel's boxes to this
// form bit for bit, tests/tree_cases.py)
static float box_lb(const float* q, const float* t, int D) {
    float s = 0.f;
    for (int r = 0; r < D; ++r) {
        const float infl = fmaf(fabsf(t[r]), 4.8e-7f, 1e-30f);
        const float lo = t[r] - infl, hi = t[r] + infl;
        const float e = fmaxf(fmaxf(lo - q[r], q[r] - hi), 0.f);
        s = fmaf(e, e, s);
    }
    return s;
}
// violations of a simulated search's certificate; *used: certificates formed
static long cert_violations(L2Fn l2fn, long* used) {
    std::mt19937_64 r2(77);
    auto U = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(r2); };
    long bad = 0;
    *used = 0;
    for (int trial = 0; trial < 40000; ++trial) {
        const int D = (trial & 1) ? 12 : 3;
        constexpr int NT = 24;
        double q[12], t[NT][12], dir[12];
        const double scale = std::exp(U(std::log(0.1), std::log(10.0)));
        const double r1 = scale * std::exp(U(std::log(1e-4), std::log(0.3)));
        std::normal_distribution<double> g;
        for (int r = 0; r < D; ++r) q[r] = g(r2) * scale / std::sqrt((double)D);
        // the winner at r1, a runner-up somewhat farther, the rest spread about the threshold
        // below (distance r1 (1 + x), x from 1e-7 to 3) on both sides of thr and of d2
        double rad[NT];
        rad[0] = r1;
        const double x0 = std::exp(U(std::log(1e-7), std::log(1.0)));  // (a trial's nearest runner-up: above it, certificates form)
        for (int j = 1; j < NT; ++j) rad[j] = r1 * (1.0 + std::exp(U(std::log(x0), std::log(3.0))));
        for (int j = 0; j < NT; ++j) {
            double n = 0;
            for (int r = 0; r < D; ++r) { dir[r] = g(r2); n += dir[r] * dir[r]; }
            for (int r = 0; r < D; ++r) t[j][r] = q[r] + rad[j] * dir[r] / std::sqrt(n);
        }
        float qf[12], tf[NT][12], df[NT];
        double qn = 0, tn = 0;
        for (int r = 0; r < D; ++r) { qf[r] = (float)q[r]; qn += q[r] * q[r]; }
        for (int j = 0; j < NT; ++j) {
            double n = 0;
            for (int r = 0; r < D; ++r) { tf[j][r] = (float)t[j][r]; n += t[j][r] * t[j][r]; }
            tn = std::max(tn, n);
            df[j] = (D == 12 && (trial & 2)) ? dist_packed(qf, tf[j], D) : dist_chain(qf, tf[j], D);
        }
        const float na = (float)std::sqrt(qn) * 1.000001f, nb = (float)(std::sqrt(tn) * (1 + 1e-6));
        // the final threshold: the widened radius of the best for a random margin, capped by a
        // random one of the other distances (as the second-best seen at the time caps it)
        int w = 0;
        for (int j = 1; j < NT; ++j) if (df[j] < df[w]) w = j;
        const float mrg = (float)(r1 * std::exp(U(std::log(1e-4), std::log(1.0))) * ((trial & 4) ? 1 : 0));
        const float cap = (trial & 8) ? df[1 + (int)(r2() % (NT - 1))] : INFINITY;
        const float thr = nncert::widen_radius(df[w], fmaxf(cap, df[w]), mrg, na, nb, D);
        // visited: every target whose box is not skipped by either form of the box test, and a
        // random half of the rest (leaf mates of visited targets, leaves other lanes wanted)
        bool vis[NT];
        float d1 = INFINITY, d2 = INFINITY;
        int i1 = -1;
        for (int j = 0; j < NT; ++j) {
            const float lb = box_lb(qf, tf[j], D);
            const bool skipped = (lb * (1.f - 2e-6f) >= thr) | !(lb < thr * 1.0000025f);
            vis[j] = !skipped | (bool)(r2() & 1);
            if (vis[j]) {
                if (df[j] < d1) { d2 = d1; d1 = df[j]; i1 = j; }
                else if (df[j] < d2) d2 = df[j];
            }
        }
        if (i1 < 0 || !(d2 - d1 > 2.f * nncert::f32_err(d2, na, nb, D))) continue;  // flagged: no certificate
        ++*used;
        const float D1 = nncert::cert_d1(d1, na, nb, D), L2 = l2fn(d2, thr, na, nb, D);
        for (int j = 0; j < NT; ++j) {
            ld ex = 0;
            for (int r = 0; r < D; ++r) ex += ((ld)q[r] - (ld)t[j][r]) * ((ld)q[r] - (ld)t[j][r]);
            ex = sqrtl(ex);
            ++g_checked;
            if (j == i1) bad += !(ex <= (ld)D1);
            else bad += !(ex >= (ld)L2);
        }
    }
    return bad;
}

// ---------------------------------------------------------------- delta
typedef double (*DlFn)(double, const double*, const double*, double, double, double);
static double dl_no_alpha(double, const double* T, const double* Tr, double dt, double qn, double qr) {
    return nncert::settle_dl(0.0, T, Tr, dt, qn, qr);
}
static double dl_half_frob(double a2, const double* T, const double* Tr, double dt, double qn, double qr) {
    return sqrt(a2 * (0.5 * nncert::rot_frob2(T, Tr)) * (1.0 + 1e-12) + dt * dt) * (1.0 + 1e-12) + 2e-15 * (qn + qr);
}
static void rzryrx(double az, double ay, double ax, double* R) {  // row-major 3x3
    const double cz = cos(az), sz = sin(az), cy = cos(ay), sy = sin(ay), cx = cos(ax), sx = sin(ax);
    const double r[9] = {cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx,
                         sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx,
                         -sy, cy * sx, cy * cx};
    std::memcpy(R, r, sizeof(r));
}
// T <- S * T for the step S = [R | t] (rows 0..2 of 4x4, f64 arithmetic: orthonormal to rounding only)
static void compose(const double* R, const double* t, double* T) {
    double N[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j) N[4 * i + j] = R[3 * i] * T[j] + R[3 * i + 1] * T[4 + j] + R[3 * i + 2] * T[8 + j];
        N[4 * i + 3] += t[i];
    }
    std::memcpy(T, N, sizeof(N));
}
// the f64 queries as the searches form them (loopdev.hpp pose_frame / pose_point), without and
// with FMA contraction
static void pose12(const double* T, const double* m, double* q, bool fma_) {
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r) {
            const double *Tr = T + 4 * r, *mc = m + 3 * c;
            double v;
            if (fma_) v = std::fma(Tr[2], mc[2], std::fma(Tr[1], mc[1], Tr[0] * mc[0]));
            else {
                volatile double p0 = Tr[0] * mc[0], p1 = Tr[1] * mc[1], p2 = Tr[2] * mc[2];
                volatile double s = p0 + p1;
                v = s + p2;
            }
            q[3 * c + r] = c == 3 ? v + Tr[3] : v;
        }
}
static void pose_point_h(const double* T, const double* m, double* q) {  // (prep_settle's own evaluation)
    for (int r = 0; r < 3; ++r) q[r] = T[r * 4 + 0] * m[0] + T[r * 4 + 1] * m[1] + T[r * 4 + 2] * m[2] + T[r * 4 + 3];
}
static long delta_violations(DlFn fn, double* slack, double* slack_large = nullptr) {
    std::mt19937_64 r2(4242);
    auto U = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(r2); };
    const double alphas[5] = {0.0, 0.01, 0.3, 3.0, 1000.0};
    long bad = 0;
    *slack = 0;
    for (int trial = 0; trial < 60000; ++trial) {
        const double alpha = alphas[trial % 5], a2 = alpha * alpha;
        const bool dim3 = (trial % 7) == 0;
        // frame: a signed permutation, exactly orthonormal, or off by up to 2^-52 per entry
        double X[9] = {0};
        {
            int pm[3] = {0, 1, 2};
            std::shuffle(pm, pm + 3, r2);
            for (int c = 0; c < 3; ++c) X[3 * c + pm[c]] = (r2() & 1) ? 1.0 : -1.0;  // column c at X[3c ..]
            if (trial & 1) {
                double R[9], Y[9];
                rzryrx(U(-3, 3), U(-1.5, 1.5), U(-3, 3), R);
                for (int c = 0; c < 3; ++c)
                    for (int r = 0; r < 3; ++r) Y[3 * c + r] = R[3 * r] * X[3 * c] + R[3 * r + 1] * X[3 * c + 1] + R[3 * r + 2] * X[3 * c + 2];
                for (int i = 0; i < 9; ++i) X[i] = Y[i] + ((trial & 2) ? U(-1, 1) * 0x1p-52 : 0.0);
            }
        }
        double m[12];
        for (int i = 0; i < 9; ++i) m[i] = alpha * X[i];
        {
            double d[3];
            std::normal_distribution<double> g;
            double n = 0;
            for (int r = 0; r < 3; ++r) { d[r] = g(r2); n += d[r] * d[r]; }
            const double mn = std::exp(U(std::log(1e-3), std::log(10.0)));
            for (int r = 0; r < 3; ++r) m[9 + r] = d[r] / std::sqrt(n) * mn;
        }
        // T: a composition of a few RzRyRx steps with translations up to 20; T': one more step of
        // angle 1e-12 .. pi and translation 0 .. 20 (or none)
        double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, Tr[12];
        const int nsteps = (int)(r2() % 6);
        for (int s = 0; s < nsteps; ++s) {
            double R[9], t[3] = {U(-20, 20) / 3, U(-20, 20) / 3, U(-20, 20) / 3};
            rzryrx(U(-3.14, 3.14), U(-1.57, 1.57), U(-3.14, 3.14), R);
            compose(R, t, T);
        }
        std::memcpy(Tr, T, sizeof(T));
        {
            const double ang = (trial % 11 == 0) ? 0.0 : std::exp(U(std::log(1e-12), std::log(3.14159)));
            const double tl = (trial % 3 == 0) ? 0.0 : std::exp(U(std::log(1e-12), std::log(20.0)));
            double R[9], ax[3], t[3];
            {
                std::normal_distribution<double> g;
                double n = 0;
                for (int r = 0; r < 3; ++r) { ax[r] = g(r2); n += ax[r] * ax[r]; }
                for (int r = 0; r < 3; ++r) { ax[r] /= std::sqrt(n); t[r] = ax[(r + 1) % 3] * tl; }
            }
            rzryrx(ang * ax[2], ang * ax[1], ang * ax[0], R);
            compose(R, t, T);
        }
        // the header's dl, from what prep_settle computes
        double Qt[3], Qr[3];
        pose_point_h(T, m + 9, Qt);
        pose_point_h(Tr, m + 9, Qr);
        const double rot2 = dim3 ? 0.0 : 3.0 * a2 * (1.0 + 1e-12);
        const double qn = sqrt(rot2 + Qt[0] * Qt[0] + Qt[1] * Qt[1] + Qt[2] * Qt[2]);
        const double qr = sqrt(rot2 + Qr[0] * Qr[0] + Qr[1] * Qr[1] + Qr[2] * Qr[2]);
        const double dt = sqrt((Qt[0] - Qr[0]) * (Qt[0] - Qr[0]) + (Qt[1] - Qr[1]) * (Qt[1] - Qr[1]) + (Qt[2] - Qr[2]) * (Qt[2] - Qr[2]));
        const double dl = fn(dim3 ? 0.0 : a2, T, Tr, dt, qn, qr);
        // the queries the searches form, each evaluation against each
        for (int va = 0; va < 2; ++va)
            for (int vb = 0; vb < 2; ++vb) {
                double qa[12], qb[12];
                pose12(T, m, qa, va);
                pose12(Tr, m, qb, vb);
                ld ex = 0;
                for (int r = dim3 ? 9 : 0; r < 12; ++r) ex += ((ld)qa[r] - (ld)qb[r]) * ((ld)qa[r] - (ld)qb[r]);
                ex = sqrtl(ex);
                ++g_checked;
                bad += !((ld)dl >= ex);
                if (ex > 1e-9L * (ld)qn) *slack = std::max(*slack, (double)((ld)dl / ex - 1));
                if (slack_large && ex > 1e-3L * (ld)qn) *slack_large = std::max(*slack_large, (double)((ld)dl / ex - 1));
            }
    }
    return bad;
}

// ---------------------------------------------------------------- settle
static long settle_violations() {
    std::mt19937_64 r2(99);
    auto U = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(r2); };
    long bad = 0, held = 0, refused_at_zero = 0;
    for (int trial = 0; trial < 200000; ++trial) {
        const float D1 = (float)std::exp(U(std::log(1e-4), std::log(10.0)));
        const double qn = std::exp(U(std::log(1e-2), std::log(2e3)));
        float L2;
        double dl;
        const int kind = trial % 4;
        if (kind == 0) {  // random
            L2 = D1 * (float)(1.0 + std::exp(U(std::log(1e-7), std::log(3.0))));
            dl = (double)D1 * std::exp(U(std::log(1e-9), std::log(1.0)));
        } else {          // a = L2 - dl and b = D1 + dl within a few f64 steps of each other, a == b included
            L2 = D1 * (float)(1.0 + std::exp(U(std::log(1e-6), std::log(1.0))));
            dl = 0.5 * ((double)L2 - (double)D1);
            int k = (int)(r2() % 9) - 4;
            if (kind == 2) {  // the 1e-14 M^2 term deciding: (a - b)(a + b) about 1e-14 M^2
                const double M = 2.0 * qn + 0.5 * ((double)L2 + (double)D1);
                dl -= 0.5 * 1e-14 * M * M / ((double)L2 + (double)D1) * U(0.5, 2.0);
                k = 0;
            }
            for (; k > 0; --k) dl = nextafter(dl, 0.0);
            for (; k < 0; ++k) dl = nextafter(dl, INFINITY);
            if (!(dl >= 0)) continue;
        }
        const int h = nncert::settle_holds(D1, L2, dl, qn);
        const ld a = (ld)L2 - (ld)dl, b = (ld)D1 + (ld)dl, M = 2 * (ld)qn + b;
        ++g_checked;
        if (h) {
            ++held;
            bad += !(b < a);                                         // D1 + dl < L2 - dl in long double
            bad += !((a - b) * (a + b) > 0.8e-14L * M * M);  // the margin (a - b is >= 22 eps a then: its own f64 rounding is below 10 %)
            // ... which covers the f64 rounding of two 12-D squared distances of vectors with |q| + |t| <= M
            bad += !((a - b) * (a + b) > 2 * 15 * 0x1p-53L * M * M);
        } else if (a <= b) {
            ++refused_at_zero;
        }
    }
    bad += !(held > 10000) + !(refused_at_zero > 1000);  // both sides were reached
    return bad;
}

// ---------------------------------------------------------------- widen, ring
static long widen_violations() {
    std::mt19937_64 r2(5);
    auto U = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(r2); };
    long bad = 0;
    for (int trial = 0; trial < 100000; ++trial) {
        const int D = (trial & 1) ? 12 : 3;
        const float na = (float)std::exp(U(std::log(1e-2), std::log(2e3))), nb = (float)std::exp(U(std::log(1e-2), std::log(2e3)));
        const float a1 = (trial % 13 == 0) ? 0.f : (float)std::exp(U(std::log(1e-12), std::log(1e3)));
        const float a2 = (trial % 5 == 0) ? INFINITY : a1 * (float)(1.0 + std::exp(U(std::log(1e-7), std::log(10.0))));
        float prev = nncert::widen_radius(a1, a2, 0.f, na, nb, D);
        const float floor_ = a1 + 3.f * nncert::f32_err(a1, na, nb, D);
        const float ceil_ = a2 + 3.f * nncert::f32_err(a2, na, nb, D);
        bad += !(prev >= floor_) + !(prev <= floor_ * (1.f + 1e-6f) + 1e-30f) + !(prev <= ceil_);  // no margin: the certified radius itself (sqrtf(a1)^2 may round up)
        float mrg = (float)std::exp(U(std::log(1e-9), std::log(1e-3)));
        for (int s = 0; s < 12; ++s, mrg *= 4.f) {
            const float w = nncert::widen_radius(a1, a2, mrg, na, nb, D);
            g_checked += 3;
            bad += !(w >= prev) + !(w >= floor_) + !(w <= ceil_);
            prev = w;
        }
    }
    return bad;
}
typedef bool (*UsableFn)(int, int, int);
static bool usable_leq(int ci, int it, int ps) { return (ci >= ps) & (ci < it) & (it - ci <= kHist); }
static long ring_violations(UsableFn fn) {
    long bad = 0;
    std::vector<int> ring(kHist, 0);
    for (int it = 1; it <= 3 * kHist + 7; ++it) {
        ring[it % kHist] = it;  // the host writes the pose of iteration `it` before its k_nn_prep
        for (int ps : {1, 2, 200, 600})
            for (int ci = -1; ci <= it + 1; ++ci) {
                ++g_checked;
                const bool u = fn(ci, it, ps);
                if (u) bad += !(ring[ci % kHist] == ci) + !(ci >= ps) + !(ci >= 1) + !(ci < it);
                else bad += (ci >= ps && ci >= 1 && ci < it && it - ci < kHist);  // nothing usable is refused
            }
    }
    return bad;
}

int main() {
    build_pairs();
    const double r_err = err_ratio(nncert::f32_err);
    report("err", r_err >= 0 && r_err <= 1.0);
    std::printf("slack_err %.4f\n", r_err);
    long used = 0;
    const long c_bad = cert_violations(nncert::cert_l2, &used);
    report("cert", c_bad == 0 && used > 5000);
    std::printf("cert_used %ld\n", used);
    double slack_dl = 0, slack_dl_large = 0, s2 = 0;
    report("delta", delta_violations(nncert::settle_dl, &slack_dl, &slack_dl_large) == 0);
    std::printf("slack_dl %.3e\n", slack_dl);
    std::printf("slack_dl_large %.3e\n", slack_dl_large);
    report("settle", settle_violations() == 0);
    report("widen", widen_violations() == 0);
    report("ring", ring_violations(nncert::cert_usable) == 0);
    // planted defects: each must fail its check on the same inputs
    const double p1 = err_ratio(err_no_norms), p2 = err_ratio(err_d_not_d3);
    report("planted_err_norms", p1 > 1.0);
    report("planted_err_d", p2 > 1.0);
    std::printf("planted_err_ratios %.3f %.4f\n", p1, p2);
    long u2 = 0;
    report("planted_l2_thr", cert_violations(l2_no_thr, &u2) > 0);
    report("planted_dl_alpha", delta_violations(dl_no_alpha, &s2) > 0);
    report("planted_dl_frob", delta_violations(dl_half_frob, &s2) > 0);
    report("planted_ring", ring_violations(usable_leq) > 0);
    std::printf("checked %ld\n", g_checked);
    return g_ok ? 0 : 1;
}
