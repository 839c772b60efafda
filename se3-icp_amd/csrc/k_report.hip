// k_report.hip — the registration report of every pair of a batch (gfx950), run once after
// the loop (report.hpp, include/se3icp.h):
//
//   k_report_open   one lane per pair: the pair's PairDev becomes an R3 search at the final
//                   pose of its PairState, with every NN certificate void.  PairState is only
//                   read: the results of the batch stay bitwise what they are.
//   (k_nn_prep + k_nn_search<3>, k_nn.hip, unchanged: the exact f64 R3 arg-min of every
//   source point, lowest index on ties, into corr_idx)
//   k_report        over k_reduce's work table, one correspondence per thread: d'^2 in f64
//                   from xyz64, the pose and the target's geometry row; the inliers' count,
//                   sum d'^2 and first and second moments of the matched target points about
//                   the pair's pivot, summed per block in k_reduce's fixed order.
//   k_report_final  one block per pair: the block partials in k_reduce_final's fixed order
//                   (18 interleaved chunks x 8 chains).  No atomics anywhere.
#include <hip/hip_runtime.h>

#include "loopdev.hpp"
#include "pairmath.hpp"
#include "report.hpp"
#include "wave.hpp"

namespace se3icp {

namespace {

using namespace loopdev;

__global__ __launch_bounds__(64) void k_report_open(View v, ReportArgs a) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= v.npairs) return;
    const PairState* S = a.state + p;
    PairDev* P = v.pairs + p;
    const int it = S->iter + 1;  // the report's search is no iteration of the loop: PairState keeps iter
    P->phase = PHASE_R3;
    P->iter = it;
    // a certificate holds from phase_start on (k_nn_prep prep_settle): none does.  Those of a
    // pair whose last phase was R3 were taken at the pose of its last search, one step before
    // the final pose; they are not kept
    P->phase_start = it + 1;
    double* h = a.hist + ((size_t)(it % kHist) * v.npairs + p) * 12;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double t = S->T.m[r][c];
            P->T[r * 4 + c] = t;
            h[r * 4 + c] = t;
        }
}

// Block b: the correspondences q0 + threadIdx.x (below q1) of its pair.
__global__ __launch_bounds__(kRedThreads) void k_report(View v, ReportArgs a) {
    constexpr int NW = kRedThreads / 64;
    static_assert(NW == 4 && kRedPer == 1, "the block sum below is written for four waves of one query a thread");
    __shared__ double red[NW][kRepVals];
    const BlockWork w = v.work[blockIdx.x];
    const PairDev* P = v.pairs + w.pair;
    const double sf = a.state[w.pair].sf;
    const int qi = w.q0 + (int)threadIdx.x;
    const bool live = qi < w.q1;
    const int g = w.s_off + (live ? qi : w.q0);
    const int nt = v.clouds[P->tgt].n;
    const int j = v.corr_idx[g];
    const int jj = ((int)(j >= 0) & (int)(j < nt)) ? j : 0;  // (never outside the target's rows)
    const double2* tr = reinterpret_cast<const double2*>(v.tgeo + (size_t)(w.t_off + jj) * 8);
    const double2 t01 = tr[0], t23 = tr[1];
    const double xt[3] = {t01.x, t01.y, t23.x};
    const size_t ld = v.ld;
    const double xs[3] = {v.xyz64[g], v.xyz64[ld + g], v.xyz64[2 * ld + g]};
    double T[12], vs[3];
    load_T(P, T);
    pose_point(T, xs[0], xs[1], xs[2], vs);
    const double d2 = l2_nanoflann3(vs, xt);  // the search's own f64 distance
    const double lim = a.max_d * sf;
    const bool in = (bool)((int)live & ((int)(a.all_inliers != 0) | (int)(d2 <= lim * lim)));
    if ((int)live & (int)(a.out_idx != nullptr)) a.out_idx[a.out_off[w.pair] + qi] = j;
    if ((int)live & (int)(a.out_dist != nullptr)) a.out_dist[a.out_off[w.pair] + qi] = sqrt(d2) / sf;
    double x[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) x[i] = 0.0;
    if (in) {
        const double y[3] = {xt[0] - P->f32_center[0], xt[1] - P->f32_center[1], xt[2] - P->f32_center[2]};
        x[0] = 1.0;
        x[1] = d2;
        x[2] = y[0]; x[3] = y[1]; x[4] = y[2];
        x[5] = y[0] * y[0]; x[6] = y[0] * y[1]; x[7] = y[0] * y[2];
        x[8] = y[1] * y[1]; x[9] = y[1] * y[2]; x[10] = y[2] * y[2];
    }
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const double sv = wave_sum32(x);  // value lane >> 1 over the wave (wave.hpp)
    if ((int)((lane & 1) == 0) & (int)((lane >> 1) < kRepVals)) red[wid][lane >> 1] = sv;
    __syncthreads();
    if (threadIdx.x < kRepVals) {
        const int i = threadIdx.x;
        a.partial[(size_t)blockIdx.x * kRepVals + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
    }
}

__global__ __launch_bounds__(kRepFinThreads) void k_report_final(View v, ReportArgs a) {
    constexpr int C = kRepChunks, U = kRepChains;
    __shared__ double part[C][kRepVals];
    const int p = blockIdx.x;
    const int i = threadIdx.x % kRepVals, s = threadIdx.x / kRepVals;
    const int wb = a.pair_wb[p], wn = a.pair_wn[p];
    if (s < C) {
        double s8[U];
#pragma unroll
        for (int u = 0; u < U; ++u) s8[u] = 0.0;
        const double* rp = a.partial + (size_t)wb * kRepVals + i;
        int b = s;
        for (; b + (U - 1) * C < wn; b += U * C) {
            double x[U];
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = rp[(size_t)(b + C * u) * kRepVals];
#pragma unroll
            for (int u = 0; u < U; ++u) s8[u] += x[u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (b + C * u < wn) s8[u] += rp[(size_t)(b + C * u) * kRepVals];
        part[s][i] = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
    }
    __syncthreads();
    if (threadIdx.x < kRepVals) {
        double sum = 0;
#pragma unroll
        for (int k = 0; k < C; ++k) sum += part[k][threadIdx.x];
        a.out[(size_t)p * kRepVals + threadIdx.x] = sum;
    }
}

}  // namespace

void launch_report_open(const View& v, const ReportArgs& a, hipStream_t s) {
    if (v.npairs > 0) hipLaunchKernelGGL(k_report_open, dim3((v.npairs + 63) / 64), dim3(64), 0, s, v, a);
}
void launch_report(const View& v, const ReportArgs& a, hipStream_t s) {
    if (v.nwork > 0) hipLaunchKernelGGL(k_report, dim3(v.nwork), dim3(kRedThreads), 0, s, v, a);
    if (v.npairs > 0) hipLaunchKernelGGL(k_report_final, dim3(v.npairs), dim3(kRepFinThreads), 0, s, v, a);
}

}  // namespace se3icp
