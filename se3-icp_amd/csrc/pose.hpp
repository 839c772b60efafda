// pose.hpp — the arithmetic of an initial pose (se3icp_register_graph_init, k_pose.hip), for the
// host and the device: a rigid transform applied to a point, two transforms composed, and the
// tests a pose goes through before it is used.
//
// A pose is a row-major 4x4 f64 matrix M, source frame -> target frame, with the bottom row
// (0, 0, 0, 1).  The arithmetic is Open3D's Transform (Eigen's 4x4 * (p, 1), then / w with w = 1)
// as k_apply_reference (k_gen.hip) states it:
//   apply_pose   q[e]    = ((M[4e] * p0 + M[4e+1] * p1) + M[4e+2] * p2) + M[4e+3] * 1.0
//   compose      C[i][j] = ((A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j]) + A[i][3] * B[3][j]
//                for rows 0..2; row 3 is exactly (0, 0, 0, 1)
// Every step is one IEEE f64 operation, never contracted into an FMA, and there is no division,
// so a restatement in any language that rounds to nearest gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SE3ICP_POSE_HD __host__ __device__ inline
#else
#define SE3ICP_POSE_HD inline
#endif

namespace se3icp {

// One rounded product / sum.  Plain operators under the pragma, as k_apply_reference has them:
// the statement carries no licence to contract, also once it is inlined.  (Not __dmul_rn /
// __dadd_rn: those are functions of the runtime's headers, compiled under the default, and
// their product and sum do fuse.)
SE3ICP_POSE_HD double pose_mul(double a, double b) {
#pragma clang fp contract(off)
    const double r = a * b;
    return r;
}
SE3ICP_POSE_HD double pose_add(double a, double b) {
#pragma clang fp contract(off)
    const double r = a + b;
    return r;
}

// q = M (p, 1); q may alias p
SE3ICP_POSE_HD void apply_pose(const double* M, const double* p, double* q) {
    const double p0 = p[0], p1 = p[1], p2 = p[2];
    for (int e = 0; e < 3; ++e)
        q[e] = pose_add(pose_add(pose_add(pose_mul(M[4 * e], p0), pose_mul(M[4 * e + 1], p1)), pose_mul(M[4 * e + 2], p2)),
                        pose_mul(M[4 * e + 3], 1.0));
}

// C = A B; C aliases neither
SE3ICP_POSE_HD void compose(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j)
            C[4 * i + j] = pose_add(pose_add(pose_add(pose_mul(A[4 * i], B[j]), pose_mul(A[4 * i + 1], B[4 + j])),
                                             pose_mul(A[4 * i + 2], B[8 + j])),
                                    pose_mul(A[4 * i + 3], B[12 + j]));
    C[12] = C[13] = C[14] = 0.0;
    C[15] = 1.0;
}

// Bitwise the identity, zeros +0.0: "no pose".  The edge's source is then the raw cloud itself
// (apply_pose(I, p) would turn a -0.0 coordinate into +0.0).
inline bool pose_is_identity(const double* M) {
    static const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    return std::memcmp(M, I, sizeof(I)) == 0;
}

// Every entry finite and the bottom row bitwise (0, 0, 0, 1).  The 3x3 block is not looked at: a
// block that is not orthonormal is applied as given, as Open3D does.
inline bool pose_is_valid(const double* M) {
    static const double bottom[4] = {0, 0, 0, 1};
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(M[i])) return false;
    return std::memcmp(M + 12, bottom, sizeof(bottom)) == 0;
}

// max |R^T R - I| <= 2^-30, in f64: the pose preserves distances up to rounding, which is what
// lets a posed copy of a cloud start its neighbour selection from the raw cloud's distances
// (graph_plan_seeds_posed).
inline bool pose_is_rigid(const double* M) {
    double worst = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double g = 0.0;
            for (int k = 0; k < 3; ++k) g += M[4 * k + i] * M[4 * k + j];
            const double d = std::fabs(g - (i == j ? 1.0 : 0.0));
            if (!(d <= worst)) worst = d;  // (a NaN stays)
        }
    return worst <= 0x1p-30;
}

// ---- k_pose.hip
constexpr int kPoseChunk = 1024;  // points of a block of the transform stage
// cloud c: points off .. off + n of the concatenated input and output
struct PoseCloud { long long off; long long n; };
// out = pose[c] applied to every point of cloud c (grid: cloud x chunk of kPoseChunk points);
// out may be the input itself
void launch_transform(const double* xyz, double* out, const PoseCloud* clouds, const double* poses, int nclouds,
                      int max_chunks, hipStream_t s);

}  // namespace se3icp
