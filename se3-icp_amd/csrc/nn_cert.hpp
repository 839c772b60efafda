// nn_cert.hpp — the arithmetic of the NN certificates of k_nn.hip, written
// for the device and the host alike: tests/cert_host.cpp checks every function against long
// double evaluation.  k_nn.hip and loopdev.hpp call these; nothing else forms a certificate.
//
//   search certificate (nn_finish): a searched query keeps D1 = cert_d1 and L2 = cert_l2: the
//     exact distance to its match is <= D1, to every other target >= L2;
//   settle certificate (prep_settle): at a later iteration of the phase the query has moved by at
//     most settle_dl, and settle_holds(D1, L2, dl, |q|) proves the match unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.hpp"

namespace se3icp {
namespace nncert {

// Rigorous bound on |f32 squared distance - exact squared distance of the f64 vectors|
// (DESIGN.md "Certified f32 arg-min"): both vectors rounded to f32 (u = 2^-24), D
// differences and a D-term FMA chain; na, nb bound the two vector norms.
__host__ __device__ __forceinline__ float f32_err(float d, float na, float nb, int D) {
    const float u = 5.9604645e-08f;
    const float s = na + nb;
    return 1.25f * (2.f * u * s * sqrtf(fmaxf(d, 0.f)) + (float)(D + 3) * u * d + 4.f * u * u * s * s) + 1e-30f;
}

// D1 from the winner's f32 squared distance d1: the exact distance to the match is <= D1
__host__ __device__ __forceinline__ float cert_d1(float d1, float na, float nb, int D) {
    return sqrtf(d1 + f32_err(d1, na, nb, D)) * (1.f + 1e-6f);
}
// L2 from the runner-up's f32 squared distance d2 and the final pruning threshold thr: visited
// targets are bounded by the top-2, unvisited ones because every box skipped had a bound >= thr
// at the time (thr only decreases)
// (in two steps, squared bound and root, so that nn_finish keeps its order of operations: the
// squared bound, D1, the root)
__host__ __device__ __forceinline__ float cert_l2_sq(float d2, float thr, float na, float nb, int D) {
    return fminf(d2 - f32_err(d2, na, nb, D), thr * (1.f - 4e-6f));
}
__host__ __device__ __forceinline__ float cert_l2_root(float l2) { return sqrtf(fmaxf(l2, 0.f)) * (1.f - 1e-6f); }
__host__ __device__ __forceinline__ float cert_l2(float d2, float thr, float na, float nb, int D) {
    return cert_l2_root(cert_l2_sq(d2, thr, na, nb, D));
}

// pruning threshold for the best / second-best f32 distances a1 <= a2: the certified radius
// a1 + 3 err, widened by the margin up to (sqrt(a1) + 2 mrg)^2 but never past a2
__host__ __device__ __forceinline__ float widen_radius(float a1, float a2, float mrg, float na, float nb, int D) {
    const float e = sqrtf(a1) + 2.f * mrg;
    const float t = fmaxf(a1, fminf(e * e, a2));
    return t + 3.f * f32_err(t, na, nb, D);
}

// |R - R'|_F^2 of two poses (rows 0..2 of the row-major 4x4)
__host__ __device__ __forceinline__ double rot_frob2(const double* A, const double* B) {
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) s += (A[r * 4 + c] - B[r * 4 + c]) * (A[r * 4 + c] - B[r * 4 + c]);
    return s;
}

// A certificate of iteration ci can be used at iteration it: it is of this phase, older than
// the current iteration and its pose is still in the kHist-row ring (row ci % kHist is
// rewritten at iteration ci + kHist)
__host__ __device__ __forceinline__ bool cert_usable(int ci, int it, int phase_start) {
    return (bool)((int)(ci >= phase_start) & (int)(ci < it) & (int)(it - ci < kHist));
}

// |q_now - q_then| of a query under poses T and Tr, from a2 = alpha^2, dt = the distance of the
// two posed translation parts and the two query norms: padded for the frame's orthonormality
// and the rounding of the two f64 queries the searches used
__host__ __device__ __forceinline__ double settle_dl(double a2, const double* T, const double* Tr, double dt, double qn,
                                                     double qr) {
    return sqrt(a2 * rot_frob2(T, Tr) * (1.0 + 1e-12) + dt * dt) * (1.0 + 1e-12) + 2e-15 * (qn + qr);
}

// D1 + dl < L2 - dl, with a margin for the f64 rounding of the reference's own squared
// distances (|q| + |target| <= M).  (An int, as the kernels' branch-free conditions are: the
// bool form compiled k_nn_prep to other code.)
__host__ __device__ __forceinline__ int settle_holds(float d1, float l2, double dl, double qn) {
    const double a = (double)l2 - dl, b = (double)d1 + dl;
    const double M = 2.0 * qn + b;
    return (int)(a > b) & (int)((a - b) * (a + b) > 1e-14 * M * M);
}

}  // namespace nncert
}  // namespace se3icp
