// report.hpp — host side of the registration report (se3icp_report, include/se3icp.h):
// the per-pair sums k_report.hip leaves are expanded into fitness, inlier RMSE and the 6x6
// information matrix, and the loop state the run ended in is named.  Header-only and
// buildable for the host alone (tests/report_host.cpp), like sweep.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pairmath.hpp"
#include "se3icp.h"

namespace se3icp {

// The sums of a pair's inliers (k_report / k_report_final), over the matched target points
// y = x' - pivot in the engine's frame:
//   [0] n   [1] sum d'^2   [2..4] sum y   [5..10] sum y y^T (xx xy xz yy yz zz)
constexpr int kRepVals = 11;
// k_report_final: interleaved chunks of block partials and independent chains per chunk
// (k_reduce_final's layout); longest path of additions of the whole order for a pair of
// `nblocks` k_report blocks: 6 (wave halving) + 2 (the block's four waves) +
// ceil(nblocks / (chunks * chains)) (a chain) + 3 (the eight chains) + chunks (the last pass)
constexpr int kRepFinThreads = 256;
constexpr int kRepChunks = 18, kRepChains = 8;
static_assert(kRepChunks * kRepVals <= kRepFinThreads, "a thread per (chunk, value)");
inline int report_sum_depth(int64_t nblocks) {
    const int64_t per = (int64_t)kRepChunks * kRepChains;
    return 6 + 2 + (int)((nblocks + per - 1) / per) + 3 + kRepChunks;
}

// max_correspondence_distance values that make every point an inlier
inline bool report_all_inliers(double max_d) { return max_d <= 0.0 || (isinf(max_d) && max_d > 0.0); }

// Fill fitness, n_inliers, inlier_rmse and information of R from the sums.
//   sf: the engine frame's scale (x' = (x - ctr) * sf), piv: the pivot the sums were taken
//   about (engine frame), ctr: the target centre (caller's frame), n_src: source points.
// With x = y / sf + o, o = piv / sf + ctr:
//   sum x     = sum y / sf + n o
//   sum x x^T = sum y y^T / sf^2 + (sum y / sf) o^T + o (sum y / sf)^T + n o o^T
// and sum G^T G over G = [-[x]x  I] is [[tr(Sxx) I - Sxx, [Sx]x], [-[Sx]x, n I]].
inline void report_expand(const double* sums, double sf, const double* piv, const double* ctr, int64_t n_src,
                          se3icp_report* R) {
    const double n = sums[0];
    for (int i = 0; i < 36; ++i) R->information[i] = 0.0;
    R->n_inliers = (int64_t)n;
    R->fitness = n_src > 0 ? (double)R->n_inliers / (double)n_src : 0.0;
    R->inlier_rmse = 0.0;
    if (!(n > 0)) return;
    R->inlier_rmse = sqrt(sums[1] / n) / sf;
    const double inv = 1.0 / sf;
    double o[3], sy[3], sx[3];
    for (int a = 0; a < 3; ++a) {
        o[a] = piv[a] * inv + ctr[a];
        sy[a] = sums[2 + a] * inv;
        sx[a] = sy[a] + n * o[a];
    }
    const int ix[3][3] = {{5, 6, 7}, {6, 8, 9}, {7, 9, 10}};
    double sxx[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) {
            // (all parts are of the size of sum |x_a x_b| at most: sum y is small about a
            // pivot near the cloud, so no part is cancelled by another)
            const double far = n * o[a] * o[b] + (sy[a] * o[b] + o[a] * sy[b]);
            sxx[a][b] = sxx[b][a] = far + sums[ix[a][b]] * inv * inv;
        }
    double* I = R->information;
    // rows 0..2, columns 0..2: (sum x^T x) I - sum x x^T
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) I[a * 6 + b] = -sxx[a][b];
    I[0 * 6 + 0] = sxx[1][1] + sxx[2][2];
    I[1 * 6 + 1] = sxx[0][0] + sxx[2][2];
    I[2 * 6 + 2] = sxx[0][0] + sxx[1][1];
    // rows 0..2, columns 3..5: A^T = [x]x summed; rows 3..5, columns 0..2: A = -[x]x
    const double X[3][3] = {{0.0, -sx[2], sx[1]}, {sx[2], 0.0, -sx[0]}, {-sx[1], sx[0], 0.0}};
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            I[a * 6 + 3 + b] = X[a][b];
            I[(3 + a) * 6 + b] = X[b][a];
        }
    for (int a = 0; a < 3; ++a) I[(3 + a) * 6 + 3 + a] = n;
}

// Why the loop ended, from the state it left (pair_close_iteration), in the order of the
// reference's `||` tests: the cap is tested first, so a run whose cap and criterion hold in
// the same iteration reports the cap.  A max_num_iterations the SE(3) phase passed by
//  never equals iter in the R3 phase: such a run ends on its criterion.
inline int report_stop_reason(const PairState& S) {
    if (S.kind == KIND_ICP) {  // ISR.cpp:547-550
        if (S.iter == S.max_iter) return SE3ICP_STOP_MAX_ITERATIONS;
        if (S.rel < S.mse) return SE3ICP_STOP_CONVERGED;
        return SE3ICP_STOP_RUNAWAY;
    }
    if (S.kind == KIND_PURE) {  // ISR.cpp:1118-1119
        if (S.iter == S.max_se3) return SE3ICP_STOP_MAX_SE3_ITERATIONS;
        if (S.rel < S.sf * S.mse) return SE3ICP_STOP_CONVERGED;
        return SE3ICP_STOP_RUNAWAY;
    }
    if (!S.sw) return SE3ICP_STOP_RUNAWAY;  // only the guard ends a run that never switched
    if (S.iter == S.max_iter) return SE3ICP_STOP_MAX_ITERATIONS;  // ISR.cpp:724-729
    if (S.rel < S.sf * S.mse) return SE3ICP_STOP_CONVERGED;
    return SE3ICP_STOP_RUNAWAY;
}

// ---- k_report.hip
struct View;
struct ReportArgs {
    const PairState* state;   // [npairs] the loop's final state (read only)
    double* hist;             // the loop's pose history (View::hist, writable)
    double max_d;             // max_correspondence_distance, caller's units
    int32_t all_inliers;      // report_all_inliers(max_d)
    int32_t _pad;
    int32_t* out_idx;         // optional per-point outputs, compact per pair (device)
    double* out_dist;
    const int64_t* out_off;   // [npairs] first entry of each pair in them (device)
    double* partial;          // [nwork * kRepVals] block partials
    double* out;              // [npairs * kRepVals] sums per pair
    const int32_t* pair_wb;   // the pairs' ranges in the k_reduce work table
    const int32_t* pair_wn;
};
// k_report_open: every pair's PairDev set to an R3 search at its final pose (void certificates)
void launch_report_open(const View& v, const ReportArgs& a, hipStream_t s);
// k_report + k_report_final, after k_nn_prep / k_nn_search<3> have run
void launch_report(const View& v, const ReportArgs& a, hipStream_t s);

}  // namespace se3icp
