// k_pose.hip — the transform stage of an initial pose (gfx950): one pose per cloud applied to
// clouds resident in HBM, every cloud of the call in one launch (se3icp_transform_device).
//
// A 48 B/point stream: 24 B read, 24 B written.  The points are AoS xyz rows of 24 B, so the three
// f64 of a lane's own point are 16-B aligned for every second point only, and a chunk's first row
// is 8-B aligned, no more: a lane takes its point as three 8-B loads 24 B apart and puts it back
// the same way.  A wavefront's three loads together cover 1,536 contiguous bytes, each 128-B line
// of them touched by all three.  Moving the chunk through LDS as a flat run of doubles instead
// (8 B per lane, 512 contiguous bytes per instruction, two barriers) was built and measured 11 %
// slower on 65 clouds of the C4 scans' size.
// A thread reads its own point and writes the same one, so the output may be the input.
#include <hip/hip_runtime.h>

#include "pose.hpp"

namespace se3icp {

namespace {

__global__ __launch_bounds__(256) void k_transform(const double* xyz_in, double* out,
                                                   const PoseCloud* __restrict__ clouds,
                                                   const double* __restrict__ poses) {
    __shared__ double M[16];
    const PoseCloud cl = clouds[blockIdx.y];
    const long long p0 = (long long)blockIdx.x * kPoseChunk;
    if (p0 >= cl.n) return;  // (uniform: a cloud shorter than the call's longest)
    const int np = (int)(cl.n - p0 < kPoseChunk ? cl.n - p0 : kPoseChunk);
    const size_t base = 3 * (size_t)(cl.off + p0);
    const double* in = xyz_in + base;
    double* o = out + base;
    if (threadIdx.x < 16) M[threadIdx.x] = poses[16 * (size_t)blockIdx.y + threadIdx.x];
    __syncthreads();
    for (int i = threadIdx.x; i < np; i += 256) {
        double q[3];
        apply_pose(M, in + 3 * i, q);
        o[3 * i] = q[0];
        o[3 * i + 1] = q[1];
        o[3 * i + 2] = q[2];
    }
}

}  // namespace

void launch_transform(const double* xyz, double* out, const PoseCloud* clouds, const double* poses, int nclouds,
                      int max_chunks, hipStream_t s) {
    if (nclouds > 0 && max_chunks > 0)
        hipLaunchKernelGGL(k_transform, dim3(max_chunks, nclouds), dim3(256), 0, s, xyz, out, clouds, poses);
}

}  // namespace se3icp
