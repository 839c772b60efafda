// Host build of se3-icp_amd/csrc/report.hpp (report_expand, report_stop_reason,
// report_all_inliers, report_sum_depth: what Engine::run_loop calls for a registration
// report) and the layout of the report structs of include/se3icp.h, for
// tests/test_report_host.py.
//
//   layout  "sizeof <struct> <bytes>" and "offset <struct>.<field> <bytes>" lines, compared
//           with the ctypes mirrors.
//   expand  report_expand against the direct long-double sum of G^T G over random inlier
//           sets of 1, 2 and 1,000 points, centres 0 and (4.5e5, 5.4e6, 300), scales 0.01
//           and 3 (normalized methods: pivot 0), and the raw frame (scale 1, the pivot at
//           the centre).  The moments are summed in long double and rounded once, so the
//           summation depth is 0 and the bound is
//               |information - direct| <= 4 (0 + 3 + 8) 2^-53 sum |term|
//           entry by entry (sum |term|: the absolute values of the products the direct sum
//           adds; an entry without terms must be exactly 0).  inlier_rmse: the same factor,
//           relative.  One line per case, "expand <case> ok <worst error / bound>" or FAIL.
//   stop    report_stop_reason after pair_close_iteration over every branch of it, one line
//           per row, "stop <row> ok" or FAIL.
// Exits 1 if any check failed.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "report.hpp"

using namespace se3icp;

static int g_bad = 0;

static void layout() {
    std::printf("sizeof se3icp_report_options %zu\n", sizeof(se3icp_report_options));
    std::printf("offset se3icp_report_options.max_correspondence_distance %zu\n", offsetof(se3icp_report_options, max_correspondence_distance));
    std::printf("offset se3icp_report_options.corr_idx %zu\n", offsetof(se3icp_report_options, corr_idx));
    std::printf("offset se3icp_report_options.corr_dist %zu\n", offsetof(se3icp_report_options, corr_dist));
    std::printf("offset se3icp_report_options.outputs_on_device %zu\n", offsetof(se3icp_report_options, outputs_on_device));
    std::printf("offset se3icp_report_options._reserved %zu\n", offsetof(se3icp_report_options, _reserved));
    std::printf("sizeof se3icp_report %zu\n", sizeof(se3icp_report));
    std::printf("offset se3icp_report.fitness %zu\n", offsetof(se3icp_report, fitness));
    std::printf("offset se3icp_report.inlier_rmse %zu\n", offsetof(se3icp_report, inlier_rmse));
    std::printf("offset se3icp_report.information %zu\n", offsetof(se3icp_report, information));
    std::printf("offset se3icp_report.final_mse %zu\n", offsetof(se3icp_report, final_mse));
    std::printf("offset se3icp_report.final_mse_change %zu\n", offsetof(se3icp_report, final_mse_change));
    std::printf("offset se3icp_report.n_inliers %zu\n", offsetof(se3icp_report, n_inliers));
    std::printf("offset se3icp_report.switched %zu\n", offsetof(se3icp_report, switched));
    std::printf("offset se3icp_report.stop_reason %zu\n", offsetof(se3icp_report, stop_reason));
    std::printf("stop_values %d %d %d %d\n", SE3ICP_STOP_CONVERGED, SE3ICP_STOP_MAX_ITERATIONS,
                SE3ICP_STOP_MAX_SE3_ITERATIONS, SE3ICP_STOP_RUNAWAY);
    std::printf("depth %d %d %d %d\n", report_sum_depth(1), report_sum_depth(144), report_sum_depth(145), report_sum_depth(17));
    std::printf("all_inliers %d %d %d %d %d\n", (int)report_all_inliers(0.0), (int)report_all_inliers(-1.0),
                (int)report_all_inliers(INFINITY), (int)report_all_inliers(0.5), (int)report_all_inliers(-INFINITY));
}

// y: the matched target points about the pivot, engine frame
static void expand_case(const char* name, int n, double sf, const double* piv, const double* ctr, unsigned seed) {
    typedef long double ld;
    std::mt19937_64 gen(seed);
    std::uniform_real_distribution<double> U(-3.0, 3.0), D(0.0, 0.05);
    std::vector<double> y(3 * (size_t)n), d2(n);
    for (auto& v : y) v = U(gen);
    for (auto& v : d2) v = D(gen);
    ld m[kRepVals] = {};
    for (int i = 0; i < n; ++i) {
        const double* p = &y[3 * (size_t)i];
        m[0] += 1;
        m[1] += d2[i];
        for (int a = 0; a < 3; ++a) m[2 + a] += p[a];
        m[5] += (ld)p[0] * p[0]; m[6] += (ld)p[0] * p[1]; m[7] += (ld)p[0] * p[2];
        m[8] += (ld)p[1] * p[1]; m[9] += (ld)p[1] * p[2]; m[10] += (ld)p[2] * p[2];
    }
    double sums[kRepVals];
    for (int k = 0; k < kRepVals; ++k) sums[k] = (double)m[k];
    se3icp_report R;
    std::memset(&R, 0, sizeof(R));
    report_expand(sums, sf, piv, ctr, 2 * (int64_t)n, &R);
    // direct: x = (piv + y) / sf + ctr, G = [-[x]x I]
    ld ref[36] = {}, mag[36] = {};
    for (int i = 0; i < n; ++i) {
        ld x[3];
        for (int a = 0; a < 3; ++a) x[a] = ((ld)piv[a] + (ld)y[3 * (size_t)i + a]) / (ld)sf + (ld)ctr[a];
        const ld G[3][6] = {{0, x[2], -x[1], 1, 0, 0}, {-x[2], 0, x[0], 0, 1, 0}, {x[1], -x[0], 0, 0, 0, 1}};
        for (int r = 0; r < 3; ++r)
            for (int a = 0; a < 6; ++a)
                for (int b = 0; b < 6; ++b) {
                    ref[a * 6 + b] += G[r][a] * G[r][b];
                    mag[a * 6 + b] += fabsl(G[r][a] * G[r][b]);
                }
    }
    const ld gamma = 4.0L * (0 + 3 + 8) * ldexpl(1.0L, -53);
    ld worst = 0;
    bool ok = true;
    for (int k = 0; k < 36; ++k) {
        const ld err = fabsl((ld)R.information[k] - ref[k]);
        if (mag[k] == 0) ok = ok && R.information[k] == 0.0;
        else {
            worst = fmaxl(worst, err / (gamma * mag[k]));
            ok = ok && err <= gamma * mag[k];
        }
    }
    const ld rmse = sqrtl(m[1] / (ld)n) / (ld)sf;
    const ld erm = fabsl((ld)R.inlier_rmse - rmse);
    ok = ok && erm <= gamma * rmse;
    ok = ok && R.n_inliers == n && R.fitness == (double)n / (double)(2 * (int64_t)n);
    if (!ok) ++g_bad;
    std::printf("expand %s %s %.3Lf %.3Lf\n", name, ok ? "ok" : "FAIL", worst, erm / (gamma * rmse));
}

static void expand_empty() {
    double sums[kRepVals] = {};
    const double z[3] = {0, 0, 0}, c[3] = {4.5e5, 5.4e6, 300.0};
    se3icp_report R;
    std::memset(&R, 0xff, sizeof(R));
    report_expand(sums, 3.0, z, c, 100, &R);
    bool ok = R.n_inliers == 0 && R.fitness == 0.0 && R.inlier_rmse == 0.0;
    for (int k = 0; k < 36; ++k) ok = ok && R.information[k] == 0.0;
    if (!ok) ++g_bad;
    std::printf("expand empty %s 0 0\n", ok ? "ok" : "FAIL");
}

struct StopRow {
    const char* name;
    int kind, iter, max_iter, max_se3, sw;
    double sf, mse, mse_switch, rel;  // rel: |mse_cur - mse_prev| this iteration produces
    int done, sw_after, reason;       // expected (reason: -1 when the pair goes on)
};

static void stop_rows() {
    const int C = SE3ICP_STOP_CONVERGED, MI = SE3ICP_STOP_MAX_ITERATIONS, MS = SE3ICP_STOP_MAX_SE3_ITERATIONS,
              RA = SE3ICP_STOP_RUNAWAY;
    const StopRow rows[] = {
        {"icp_cap", KIND_ICP, 5, 5, 20, 0, 1.0, 1e-5, 1e-3, 1.0, 1, 0, MI},
        {"icp_criterion", KIND_ICP, 5, 9, 20, 0, 1.0, 1e-5, 1e-3, 1e-6, 1, 0, C},
        {"icp_both", KIND_ICP, 5, 5, 20, 0, 1.0, 1e-5, 1e-3, 1e-6, 1, 0, MI},
        {"icp_neither", KIND_ICP, 5, 9, 20, 0, 1.0, 1e-5, 1e-3, 1.0, 0, 0, -1},
        {"icp_runaway", KIND_ICP, 100000, 150, 20, 0, 1.0, 1e-5, 1e-3, 1.0, 1, 0, RA},
        {"icp_sf_unused", KIND_ICP, 5, 9, 20, 0, 3.0, 1e-5, 1e-3, 2e-5, 0, 0, -1},
        {"pure_cap", KIND_PURE, 3, 150, 3, 0, 3.0, 1e-5, 1e-3, 1.0, 1, 0, MS},
        {"pure_criterion", KIND_PURE, 2, 150, 3, 0, 3.0, 1e-5, 1e-3, 2e-5, 1, 0, C},
        {"pure_both", KIND_PURE, 3, 150, 3, 0, 3.0, 1e-5, 1e-3, 2e-5, 1, 0, MS},
        {"pure_neither", KIND_PURE, 2, 150, 3, 0, 3.0, 1e-5, 1e-3, 1.0, 0, 0, -1},
        {"pure_runaway", KIND_PURE, 100000, 150, 0, 0, 3.0, 1e-5, 1e-3, 1.0, 1, 0, RA},
        {"se3_switch_cap", KIND_SE3, 10, 150, 10, 0, 3.0, 1e-5, 0.0, 1.0, 0, 1, -1},
        {"se3_switch_change", KIND_SE3, 4, 150, 10, 0, 3.0, 1e-5, 1e-3, 1.0, 0, 1, -1},
        {"se3_no_switch", KIND_SE3, 4, 150, 10, 0, 3.0, 1e-5, 0.0, 1e-9, 0, 0, -1},
        {"se3_unswitched_runaway", KIND_SE3, 100000, 150, 0, 0, 3.0, 1e-5, 0.0, 1e-9, 1, 0, RA},
        {"se3_cap", KIND_SE3, 11, 11, 10, 1, 3.0, 1e-5, 1e-3, 1.0, 1, 1, MI},
        {"se3_criterion", KIND_SE3, 12, 150, 10, 1, 3.0, 1e-5, 1e-3, 2e-5, 1, 1, C},
        {"se3_both", KIND_SE3, 11, 11, 10, 1, 3.0, 1e-5, 1e-3, 2e-5, 1, 1, MI},
        {"se3_neither", KIND_SE3, 12, 150, 10, 1, 3.0, 1e-5, 1e-3, 1.0, 0, 1, -1},
        {"se3_runaway", KIND_SE3, 100000, 150, 10, 1, 3.0, 1e-5, 1e-3, 1.0, 1, 1, RA},
        {"se3_cap_passed_by", KIND_SE3, 14, 10, 10, 1, 3.0, 1e-5, 1e-3, 2e-5, 1, 1, C},
        {"cf_cap", KIND_CF, 11, 11, 10, 1, 3.0, 1e-5, 1e-3, 1.0, 1, 1, MI},
        {"cf_criterion", KIND_CF, 12, 150, 10, 1, 3.0, 1e-5, 1e-3, 2e-5, 1, 1, C},
    };
    for (const StopRow& r : rows) {
        PairState S;
        std::memset(&S, 0, sizeof(S));
        S.T = M4::eye();
        S.kind = r.kind;
        S.iter = r.iter;
        S.max_iter = r.max_iter;
        S.max_se3 = r.max_se3;
        S.sw = r.sw;
        S.sf = r.sf;
        S.mse = r.mse;
        S.mse_switch = r.mse_switch;
        S.K = 1.0;
        S.mse_cur = 0.5;  // the previous iteration's MSE
        double acc[kRedVals] = {};
        acc[27] = 0.5 + r.rel;  // this iteration's; no correspondences in the moments: the step is I
        pair_close_iteration(S, EST_PT2PT, acc);
        bool ok = S.done == r.done && S.sw == r.sw_after;
        if (r.done) ok = ok && report_stop_reason(S) == r.reason;
        if (!ok) ++g_bad;
        std::printf("stop %s %s\n", r.name, ok ? "ok" : "FAIL");
    }
    std::printf("stop_rows %zu\n", sizeof(rows) / sizeof(rows[0]));
}

int main() {
    layout();
    const double z[3] = {0, 0, 0}, utm[3] = {4.5e5, 5.4e6, 300.0};
    const int ns[3] = {1, 2, 1000};
    unsigned seed = 1;
    for (int n : ns)
        for (int ci = 0; ci < 2; ++ci) {
            const double* c = ci ? utm : z;
            for (double sf : {0.01, 3.0}) {
                char name[64];
                std::snprintf(name, sizeof(name), "n%d_c%d_s%g", n, ci, sf);
                expand_case(name, n, sf, z, c, seed++);
            }
            char name[64];
            std::snprintf(name, sizeof(name), "n%d_c%d_raw", n, ci);
            expand_case(name, n, 1.0, c, z, seed++);  // the raw frame: the pivot carries the offset
        }
    expand_empty();
    stop_rows();
    std::printf("bad %d\n", g_bad);
    return g_bad ? 1 : 0;
}
