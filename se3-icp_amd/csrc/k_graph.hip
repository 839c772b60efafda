// k_graph.hip — a registration over a shared cloud set (Engine::register_graph), gfx950.
//
// The graph call ingests every distinct cloud once (raw SoA columns, centroid, radius), lays
// out the 2P use clouds the loop runs on, and lets the first use of every CLASS (graph.hpp: a
// cloud under one normalization) select the class's neighbours.  Two streaming kernels, both
// walking a chunk table (cloud, first local point) of the use layout:
//   k_graph_normalize  a use's normalized f64 columns and f32 copy from the shared raw
//                      columns: the arithmetic of k_normalize (k_setup.hip), p' = (p + (-c)) * s,
//                      so a use is bitwise the cloud a batch normalizes in place;
//   k_graph_share      the SE(3) rows and normals of a use that did not compute its own, from
//                      the use of its class that did.  The f64 row is the class's (the weights
//                      are the call's); the f32 row is formed for the use itself with the
//                      frame kernels' epilogue (store_frame_rows): a cf target's translation
//                      comes from its point, whichever side the computing use was on.
// Raw columns and uses share the column stride (View::ld).  No atomics, no LDS.
// And the two kernels by which a device batch finds the slots that hold one cloud (graph.hpp):
//   k_share_hash       a 64-bit content hash of every slot's raw input (one integer atomic per
//                      wavefront);
//   k_share_compare    a slot's bytes against those of the first slot with its hash.
#include <hip/hip_runtime.h>

#include "devmath.hpp"
#include "graph.hpp"
#include "view.hpp"

namespace se3icp {

namespace {

__global__ __launch_bounds__(kBlock) void k_graph_normalize(View v, const ChunkWork* chunks, const GraphSeg* seg,
                                                            const double* raw, const double* raw_conf) {
    const ChunkWork cw = chunks[blockIdx.x];
    const CloudDev cl = v.clouds[cw.cloud];
    const CloudSetup st = v.setup[cw.cloud];
    const int so = seg[cw.cloud].src_off;
    const double ncx = -st.norm_center[0], ncy = -st.norm_center[1], ncz = -st.norm_center[2];
    const double s = st.norm_scale;
    const size_t ld = (size_t)v.ld;
    const int end = min(cw.p0 + kChunk, cl.n);
    for (int li = cw.p0 + (int)threadIdx.x; li < end; li += kBlock) {
        const int g = cl.off + li, r = so + li;
        const double x = (raw[r] + ncx) * s;
        const double y = (raw[ld + r] + ncy) * s;
        const double z = (raw[2 * ld + r] + ncz) * s;
        v.xyz64[g] = x;
        v.xyz64[ld + g] = y;
        v.xyz64[2 * ld + g] = z;
        const double fx = x - st.f32_center[0], fy = y - st.f32_center[1], fz = z - st.f32_center[2];
        v.xyz32[g] = (float)fx;
        v.xyz32[ld + g] = (float)fy;
        v.xyz32[2 * ld + g] = (float)fz;
        v.cloud_of[g] = cw.cloud;
        if (st.want_conf) v.conf64[g] = raw_conf[r];  // (from the raw z, k_ingest)
    }
}

__global__ __launch_bounds__(kBlock) void k_graph_share(View v, const ChunkWork* chunks, const GraphSeg* seg) {
    const ChunkWork cw = chunks[blockIdx.x];
    const int u = cw.cloud;
    const CloudDev cl = v.clouds[u];
    const GraphSeg sg = seg[u];
    const size_t ld = (size_t)v.ld;
    const bool cf_target = v.setup[u].cf_target != 0;
    const bool normals = sg.nrm_off != cl.off;
    const int end = min(cw.p0 + kChunk, cl.n);
    for (int li = cw.p0 + (int)threadIdx.x; li < end; li += kBlock) {
        const int g = cl.off + li;
        if (normals) {
            const int rn = sg.nrm_off + li;
#pragma unroll
            for (int d = 0; d < 3; ++d) v.nrm64[d * ld + g] = v.nrm64[d * ld + rn];
        }
        if (sg.frames) {
            // the weighted row is the class's (same alpha, beta); its f32 copy is the use's own:
            // a cf target takes the translation from the point (store_frame_rows, as k_lrf8)
            const double2* row = reinterpret_cast<const double2*>(v.fr64 + (size_t)(sg.src_off + li) * 12);
            double f12[12];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const double2 x = row[k];
                f12[2 * k] = x.x;
                f12[2 * k + 1] = x.y;
            }
            store_frame_rows(v.fr64, v.fr32, g, f12, cf_target, v.xyz64[g], v.xyz64[ld + g], v.xyz64[2 * ld + g]);
        }
    }
}

// ---- content-detected sharing of a device batch (Engine::setup_pairs_shared)
// A slot's hash is the sum modulo 2^64 of a mixed word per 8-byte word of its raw xyz, the mix
// keyed with the word's index and the slot's point count: a sum, so the blocks of a slot
// combine in any order to the same value (integer atomics; deterministic).
constexpr int kShareBlocks = 32;  // blocks per slot, grid-strided over its words

__device__ __forceinline__ unsigned long long share_mix(unsigned long long word, unsigned long long index,
                                                        unsigned long long n) {
    unsigned long long x = word + (index + 1) * 0x9E3779B97F4A7C15ull + n * 0xD6E8FEB86659FD93ull;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

__global__ __launch_bounds__(kBlock) void k_share_hash(View v, unsigned long long* hash) {
    const int u = blockIdx.y;
    const unsigned long long n = (unsigned long long)v.clouds[u].n;
    const unsigned long long* in = reinterpret_cast<const unsigned long long*>(v.in_ptr[u]);
    const size_t words = 3 * (size_t)n;
    unsigned long long sum = 0;
    for (size_t w = (size_t)blockIdx.x * kBlock + threadIdx.x; w < words; w += (size_t)kShareBlocks * kBlock)
        sum += share_mix(in[w], w, n);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0 && sum != 0) atomicAdd(hash + u, sum);
}

// same[pair.slot] = 0 where a word of the slot differs from the same word of pair.first (the
// caller presets 1); both hold clouds[pair.slot].n points.  Bytes, not values: -0.0 differs from
// +0.0 and a NaN equals itself.
__global__ __launch_bounds__(kBlock) void k_share_compare(View v, const SharePair* pairs, int32_t* same) {
    const SharePair pr = pairs[blockIdx.y];
    const unsigned long long* a = reinterpret_cast<const unsigned long long*>(v.in_ptr[pr.slot]);
    const unsigned long long* b = reinterpret_cast<const unsigned long long*>(v.in_ptr[pr.first]);
    const size_t words = 3 * (size_t)v.clouds[pr.slot].n;
    bool differ = false;
    for (size_t w = (size_t)blockIdx.x * kBlock + threadIdx.x; w < words; w += (size_t)kShareBlocks * kBlock)
        differ |= a[w] != b[w];
    if (differ) same[pr.slot] = 0;
}

}  // namespace

void launch_share_hash(const View& v, unsigned long long* hash, hipStream_t s) {
    if (v.nclouds > 0) hipLaunchKernelGGL(k_share_hash, dim3(kShareBlocks, v.nclouds), dim3(kBlock), 0, s, v, hash);
}

void launch_share_compare(const View& v, const SharePair* pairs, int npairs, int32_t* same, hipStream_t s) {
    if (npairs > 0)
        hipLaunchKernelGGL(k_share_compare, dim3(kShareBlocks, npairs), dim3(kBlock), 0, s, v, pairs, same);
}

void launch_graph_normalize(const View& v, const ChunkWork* chunks, int nchunks, const GraphSeg* seg,
                            const double* raw_xyz64, const double* raw_conf64, hipStream_t s) {
    if (nchunks > 0)
        hipLaunchKernelGGL(k_graph_normalize, dim3(nchunks), dim3(kBlock), 0, s, v, chunks, seg, raw_xyz64, raw_conf64);
}

void launch_graph_share(const View& v, const ChunkWork* chunks, int nchunks, const GraphSeg* seg, hipStream_t s) {
    if (nchunks > 0) hipLaunchKernelGGL(k_graph_share, dim3(nchunks), dim3(kBlock), 0, s, v, chunks, seg);
}

}  // namespace se3icp
