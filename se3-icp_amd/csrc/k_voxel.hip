// k_voxel.hip — batched voxel-grid downsample of raw clouds in HBM (Open3D
// PointCloud::VoxelDownSample for xyz; arithmetic and key: voxel.hpp).
//
// Every cloud of the call goes through each launch (blockIdx.y = cloud, blockIdx.x = chunk of
// kVoxChunk consecutive points; clouds with fewer chunks leave the surplus blocks at once):
//   k_vox_clear      every table slot free
//   k_vox_bounds     per chunk min / max and the non-finite test
//   k_vox_grid       per cloud: bounds from the chunks in chunk order, then the grid (min_bound,
//                    bits per axis, "too small", the 63-bit rule)
//   k_vox_insert     per point: packed key -> its cloud's open-addressing table (64-bit CAS on
//                    the full key, linear probing bounded by the table size), the voxel's
//                    lowest point index (atomicMin) and its count
//   k_vox_flags      per chunk: how many voxels have their first point here, and their counts
//   k_vox_scan_chunks / k_vox_scan_clouds   exclusive sums over a cloud's chunks, over the clouds
//   k_vox_place      a voxel's rank = first points before its own first point: the output order
//                    is first occurrence.  The same scan over the counts gives its segment of the
//                    member list.
//   k_vox_scatter    every point's index into its voxel's segment (atomic cursor: any order)
//   k_vox_small      one lane per voxel of <= kVoxLane points: adds its members in ascending
//                    index order (repeatedly the smallest index above the last) and divides;
//                    larger voxels go on a list
//   k_vox_big        one block per listed voxel: <= kVoxLds members are ranked in LDS, more are
//                    found by a stable compaction over the cloud; the points are staged in LDS
//                    in input order and one lane adds them.
// The sum of a voxel is one sequential f64 chain in input order whatever the path, the slot a key
// lands in is never part of a result, and no loop waits on another thread: every probe sequence,
// scan and member loop is bounded by a count fixed before the launch.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "voxel.hpp"

namespace se3icp {

namespace {

constexpr int kVoxThreads = 256;
constexpr int kVoxPer = 4;
constexpr int kVoxChunk = kVoxThreads * kVoxPer;
static_assert(kVoxChunk == kVoxChunkPoints, "voxel.hpp: chunk size");
static_assert(kVoxLds % kVoxThreads == 0 && kVoxLane < kVoxLds, "tiers");

__device__ __forceinline__ int wave_incl_scan(int x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// exclusive sums of (a, b) over the block's threads in thread order, and the block totals
// (s_w: 2 * 4 ints; every thread of the block calls)
__device__ __forceinline__ void block_excl_scan2(int a, int b, int* s_w, int& ea, int& eb, int& ta, int& tb) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ia = wave_incl_scan(a), ib = wave_incl_scan(b);
    __syncthreads();  // (s_w may still be read from the caller's previous scan)
    if (lane == 63) {
        s_w[w] = ia;
        s_w[4 + w] = ib;
    }
    __syncthreads();
    int ba = 0, bb = 0;
    ta = 0;
    tb = 0;
#pragma unroll
    for (int k = 0; k < kVoxThreads / 64; ++k) {
        if (k < w) {
            ba += s_w[k];
            bb += s_w[4 + k];
        }
        ta += s_w[k];
        tb += s_w[4 + k];
    }
    ea = ba + ia - a;
    eb = bb + ib - b;
}

// min / max of six values over the block; the result is in thread 0 (s_m: 4 * 6 doubles)
__device__ __forceinline__ void block_minmax(double (&lo)[3], double (&hi)[3], double* s_m) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            lo[a] = fmin(lo[a], __shfl_xor(lo[a], o, 64));
            hi[a] = fmax(hi[a], __shfl_xor(hi[a], o, 64));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s_m[w * 6 + a] = lo[a];
            s_m[w * 6 + 3 + a] = hi[a];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kVoxThreads / 64; ++k)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = fmin(lo[a], s_m[k * 6 + a]);
                hi[a] = fmax(hi[a], s_m[k * 6 + 3 + a]);
            }
    }
}

__global__ __launch_bounds__(kVoxThreads) void k_vox_clear(VoxelSlot* table, int64_t n_slots) {
    const int64_t s = (int64_t)blockIdx.x * kVoxThreads + threadIdx.x;
    if (s >= n_slots) return;
    VoxelSlot e;
    e.key = kVoxEmptyKey;
    e.first = kVoxNoIndex;
    e.count = 0;
    table[s] = e;
}

__global__ __launch_bounds__(kVoxThreads) void k_vox_bounds(VoxelArgs A) {
    __shared__ double s_m[24];
    __shared__ int s_bad;
    const int c = blockIdx.y;
    const VoxelCloud cl = A.clouds[c];
    if ((int)blockIdx.x >= cl.nchunks) return;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    bool bad = false;
    const double* x = A.xyz + 3 * cl.off;
#pragma unroll
    for (int j = 0; j < kVoxPer; ++j) {
        const int64_t i = (int64_t)blockIdx.x * kVoxChunk + j * kVoxThreads + threadIdx.x;
        if (i < cl.n) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double v = x[3 * i + a];
                bad = bad || !(v - v == 0.0);  // NaN or an infinity
                lo[a] = fmin(lo[a], v);
                hi[a] = fmax(hi[a], v);
            }
        }
    }
    if (bad) s_bad = 1;
    block_minmax(lo, hi, s_m);  // (synchronises: s_bad is complete behind it)
    if (threadIdx.x == 0) {
        double* out = A.minmax + 6 * (cl.chunk0 + blockIdx.x);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            out[a] = lo[a];
            out[3 + a] = hi[a];
        }
        if (s_bad) atomicMax(&A.status[c], (int)VOX_NONFINITE);
    }
}

__global__ __launch_bounds__(kVoxThreads) void k_vox_grid(VoxelArgs A) {
    __shared__ double s_m[24];
    const int c = blockIdx.x;
    const VoxelCloud cl = A.clouds[c];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int k = threadIdx.x; k < cl.nchunks; k += kVoxThreads) {
        const double* in = A.minmax + 6 * (cl.chunk0 + k);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], in[a]);
            hi[a] = fmax(hi[a], in[3 + a]);
        }
    }
    block_minmax(lo, hi, s_m);
    if (threadIdx.x == 0) {
        VoxelGrid g;
        if (A.status[c] != VOX_OK) {  // a non-finite coordinate: no grid
            g.voxel_size = cl.voxel_size;
            for (int a = 0; a < 3; ++a) {
                g.min_bound[a] = 0.0;
                g.bits[a] = 0;
            }
            g.status = A.status[c];
        } else {
            voxel_make_grid(lo, hi, cl.voxel_size, &g);
            if (g.status != VOX_OK) A.status[c] = g.status;
        }
        A.grids[c] = g;
    }
}

__global__ __launch_bounds__(kVoxThreads) void k_vox_insert(VoxelArgs A) {
    const int c = blockIdx.y;
    const VoxelCloud cl = A.clouds[c];
    if ((int)blockIdx.x >= cl.nchunks) return;
    const VoxelGrid g = A.grids[c];
    if (g.status != VOX_OK) return;
    const double* x = A.xyz + 3 * cl.off;
    VoxelSlot* tab = A.table + cl.tab;
    const uint64_t mask = (uint64_t)cl.slots - 1;
#pragma unroll
    for (int j = 0; j < kVoxPer; ++j) {
        const int64_t i = (int64_t)blockIdx.x * kVoxChunk + j * kVoxThreads + threadIdx.x;
        if (i >= cl.n) continue;
        const unsigned long long key = voxel_key(g, x[3 * i], x[3 * i + 1], x[3 * i + 2]);
        const uint64_t h = voxel_hash(key);
        int64_t slot = -1;
        for (int64_t p = 0; p < cl.slots; ++p) {  // bounded by the table: a full table is reported, not waited on
            const uint64_t s = (h + (uint64_t)p) & mask;
            unsigned long long cur = __atomic_load_n(&tab[s].key, __ATOMIC_RELAXED);
            if (cur == kVoxEmptyKey) cur = atomicCAS(&tab[s].key, (unsigned long long)kVoxEmptyKey, key);
            if (cur == kVoxEmptyKey || cur == key) {  // the full key, never the hash
                slot = (int64_t)s;
                break;
            }
        }
        if (slot < 0) {
            atomicMax(A.error, 1);
            A.vid[cl.pt0 + i] = -1;
            continue;
        }
        // (the first index only falls: a value at or below i, however old, settles it without an atomic)
        if (__atomic_load_n(&tab[slot].first, __ATOMIC_RELAXED) > (int)i) atomicMin(&tab[slot].first, (int)i);
        atomicAdd(&tab[slot].count, 1);
        A.vid[cl.pt0 + i] = (int32_t)slot;
    }
}

// the point's (is the first of its voxel, that voxel's count) for the two scans; a thread holds
// kVoxPer consecutive points
__device__ __forceinline__ void vox_flags(const VoxelArgs& A, const VoxelCloud& cl, int64_t i0, int (&f)[kVoxPer],
                                          int (&n)[kVoxPer], int& fa, int& na) {
    fa = 0;
    na = 0;
#pragma unroll
    for (int j = 0; j < kVoxPer; ++j) {
        const int64_t i = i0 + j;
        f[j] = 0;
        n[j] = 0;
        if (i < cl.n) {
            const int32_t v = A.vid[cl.pt0 + i];
            if (v >= 0) {
                const VoxelSlot sl = A.table[cl.tab + v];
                if (sl.first == (int)i) {
                    f[j] = 1;
                    n[j] = sl.count;
                }
            }
        }
        fa += f[j];
        na += n[j];
    }
}

__global__ __launch_bounds__(kVoxThreads) void k_vox_flags(VoxelArgs A) {
    __shared__ int s_w[8];
    const int c = blockIdx.y;
    const VoxelCloud cl = A.clouds[c];
    if ((int)blockIdx.x >= cl.nchunks) return;
    int fa = 0, na = 0;
    if (A.status[c] == VOX_OK) {
        int f[kVoxPer], n[kVoxPer];
        vox_flags(A, cl, (int64_t)blockIdx.x * kVoxChunk + (int64_t)threadIdx.x * kVoxPer, f, n, fa, na);
    }
    int ea, eb, ta, tb;
    block_excl_scan2(fa, na, s_w, ea, eb, ta, tb);
    if (threadIdx.x == 0) {
        A.chunk_sums[2 * (cl.chunk0 + blockIdx.x)] = ta;
        A.chunk_sums[2 * (cl.chunk0 + blockIdx.x) + 1] = tb;
    }
}

// one block per cloud: its chunks' sums become exclusive sums in place; the totals are n_out
__global__ __launch_bounds__(kVoxThreads) void k_vox_scan_chunks(VoxelArgs A) {
    __shared__ int s_w[8];
    const int c = blockIdx.x;
    const VoxelCloud cl = A.clouds[c];
    int ca = 0, cb = 0;
    for (int base = 0; base < cl.nchunks; base += kVoxThreads) {
        const int k = base + threadIdx.x;
        int a = 0, b = 0;
        if (k < cl.nchunks) {
            a = A.chunk_sums[2 * (cl.chunk0 + k)];
            b = A.chunk_sums[2 * (cl.chunk0 + k) + 1];
        }
        int ea, eb, ta, tb;
        block_excl_scan2(a, b, s_w, ea, eb, ta, tb);
        if (k < cl.nchunks) {
            A.chunk_sums[2 * (cl.chunk0 + k)] = ca + ea;
            A.chunk_sums[2 * (cl.chunk0 + k) + 1] = cb + eb;
        }
        ca += ta;
        cb += tb;
    }
    if (threadIdx.x == 0) A.n_out[c] = ca;
}

// one block: out_off[c] = voxels of the clouds before c, out_off[n_clouds] = all
__global__ __launch_bounds__(kVoxThreads) void k_vox_scan_clouds(VoxelArgs A) {
    __shared__ int s_w[8];
    long long carry = 0;
    for (int base = 0; base < A.n_clouds; base += kVoxThreads) {
        const int c = base + threadIdx.x;
        const int a = c < A.n_clouds ? A.n_out[c] : 0;
        int ea, eb, ta, tb;
        block_excl_scan2(a, 0, s_w, ea, eb, ta, tb);  // (a tile holds < 2^30 voxels: the call's points)
        if (c < A.n_clouds) A.out_off[c] = carry + ea;
        carry += ta;
    }
    if (threadIdx.x == 0) A.out_off[A.n_clouds] = carry;
}

__global__ __launch_bounds__(kVoxThreads) void k_vox_place(VoxelArgs A) {
    __shared__ int s_w[8];
    const int c = blockIdx.y;
    const VoxelCloud cl = A.clouds[c];
    if ((int)blockIdx.x >= cl.nchunks) return;
    if (A.status[c] != VOX_OK) return;
    const int64_t i0 = (int64_t)blockIdx.x * kVoxChunk + (int64_t)threadIdx.x * kVoxPer;
    int f[kVoxPer], n[kVoxPer], fa, na;
    vox_flags(A, cl, i0, f, n, fa, na);
    int ea, eb, ta, tb;
    block_excl_scan2(fa, na, s_w, ea, eb, ta, tb);
    int r = A.chunk_sums[2 * (cl.chunk0 + blockIdx.x)] + ea;        // rank within the cloud
    int seg = A.chunk_sums[2 * (cl.chunk0 + blockIdx.x) + 1] + eb;  // first member entry within the cloud
    const long long o0 = A.out_off[c];
#pragma unroll
    for (int j = 0; j < kVoxPer; ++j) {
        if (!f[j]) continue;
        const int64_t i = i0 + j;
        const int32_t v = A.vid[cl.pt0 + i];
        VoxelRec rec;
        rec.first = (int32_t)i;
        rec.count = n[j];
        rec.seg = (int32_t)(cl.pt0 + seg);
        rec.cloud = c;
        A.recs[o0 + r] = rec;
        A.table[cl.tab + v].count = (int32_t)(cl.pt0 + seg);  // from here on the segment's cursor (only this thread read the count)
        r += 1;
        seg += n[j];
    }
}

__global__ __launch_bounds__(kVoxThreads) void k_vox_scatter(VoxelArgs A) {
    const int c = blockIdx.y;
    const VoxelCloud cl = A.clouds[c];
    if ((int)blockIdx.x >= cl.nchunks) return;
    if (A.status[c] != VOX_OK) return;
#pragma unroll
    for (int j = 0; j < kVoxPer; ++j) {
        const int64_t i = (int64_t)blockIdx.x * kVoxChunk + j * kVoxThreads + threadIdx.x;
        if (i >= cl.n) continue;
        const int32_t v = A.vid[cl.pt0 + i];
        if (v < 0) continue;
        const int pos = atomicAdd(&A.table[cl.tab + v].count, 1);
        if (pos >= cl.pt0 && pos < cl.pt0 + cl.n) A.members[pos] = (int32_t)i;
        else atomicMax(A.error, 1);
    }
}

__device__ __forceinline__ void vox_write(const VoxelArgs& A, long long g, const VoxelRec& rec, double sx, double sy,
                                          double sz) {
    const double d = (double)rec.count;
    A.out[3 * g] = sx / d;
    A.out[3 * g + 1] = sy / d;
    A.out[3 * g + 2] = sz / d;
    if (A.out_count) A.out_count[g] = rec.count;
    if (A.out_first) A.out_first[g] = rec.first;
}

__global__ __launch_bounds__(kVoxThreads) void k_vox_small(VoxelArgs A) {
#pragma clang fp contract(off)
    const long long g = (long long)blockIdx.x * kVoxThreads + threadIdx.x;
    if (g >= A.out_off[A.n_clouds]) return;
    const VoxelRec rec = A.recs[g];
    if (rec.count > kVoxLane) {
        const int pos = atomicAdd(A.n_big, 1);
        if (pos < A.big_cap) A.big[pos] = (int32_t)g;
        else atomicMax(A.error, 1);
        return;
    }
    const VoxelCloud cl = A.clouds[rec.cloud];
    const double* x = A.xyz + 3 * cl.off;
    const int32_t* m = A.members + rec.seg;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int last = -1;
    for (int j = 0; j < rec.count; ++j) {
        int nxt = 0x7fffffff;
        for (int t = 0; t < rec.count; ++t) {
            const int e = m[t];
            if (e > last && e < nxt) nxt = e;
        }
        if (nxt >= cl.n) {  // (a member list that is not this voxel's: never read past the cloud)
            atomicMax(A.error, 1);
            return;
        }
        sx += x[3 * (int64_t)nxt];
        sy += x[3 * (int64_t)nxt + 1];
        sz += x[3 * (int64_t)nxt + 2];
        last = nxt;
    }
    vox_write(A, g, rec, sx, sy, sz);
}

__global__ __launch_bounds__(kVoxThreads) void k_vox_big(VoxelArgs A) {
#pragma clang fp contract(off)
    __shared__ int32_t s_idx[kVoxLds];
    __shared__ int32_t s_sorted[kVoxLds];
    __shared__ double s_pts[3 * kVoxThreads];
    __shared__ int s_w[4];
    int nbig = *A.n_big;
    if (nbig > A.big_cap) nbig = A.big_cap;
    const int tid = threadIdx.x;
    for (int b = blockIdx.x; b < nbig; b += gridDim.x) {
        const long long g = A.big[b];
        const VoxelRec rec = A.recs[g];
        const VoxelCloud cl = A.clouds[rec.cloud];
        const double* x = A.xyz + 3 * cl.off;
        double sx = 0.0, sy = 0.0, sz = 0.0;  // (thread 0's are the sum)
        __syncthreads();                      // the previous voxel's LDS is done with
        if (rec.count <= kVoxLds) {
            const int32_t* m = A.members + rec.seg;
            for (int e = tid; e < rec.count; e += kVoxThreads) s_idx[e] = m[e];
            __syncthreads();
            // the members are distinct: an entry's rank is the number of smaller ones
            for (int e = tid; e < rec.count; e += kVoxThreads) {
                const int32_t v = s_idx[e];
                int r = 0;
                for (int t = 0; t < rec.count; ++t) r += s_idx[t] < v;
                s_sorted[r] = v;
            }
            __syncthreads();
            for (int base = 0; base < rec.count; base += kVoxThreads) {
                const int e = base + tid;
                if (e < rec.count) {
                    int32_t i = s_sorted[e];
                    if (i < 0 || i >= cl.n) {
                        atomicMax(A.error, 1);
                        i = 0;
                    }
                    s_pts[3 * tid] = x[3 * (int64_t)i];
                    s_pts[3 * tid + 1] = x[3 * (int64_t)i + 1];
                    s_pts[3 * tid + 2] = x[3 * (int64_t)i + 2];
                }
                __syncthreads();
                if (tid == 0) {
                    const int cnt = min(kVoxThreads, rec.count - base);
                    for (int t = 0; t < cnt; ++t) {
                        sx += s_pts[3 * t];
                        sy += s_pts[3 * t + 1];
                        sz += s_pts[3 * t + 2];
                    }
                }
                __syncthreads();
            }
        } else {
            // too many members for LDS: the voxel's points are those of its cloud, in order,
            // whose slot is the voxel's -- a stable compaction, tile by tile
            const int32_t slot = A.vid[cl.pt0 + rec.first];
            const int lane = tid & 63, w = tid >> 6;
            for (int64_t base = 0; base < cl.n; base += kVoxThreads) {
                const int64_t i = base + tid;
                const bool hit = i < cl.n && A.vid[cl.pt0 + i] == slot;
                const unsigned long long bal = __ballot(hit);
                if (lane == 0) s_w[w] = __popcll(bal);
                __syncthreads();
                int pos = __popcll(bal & ((1ull << lane) - 1));
                int cnt = 0;
#pragma unroll
                for (int k = 0; k < kVoxThreads / 64; ++k) {
                    if (k < w) pos += s_w[k];
                    cnt += s_w[k];
                }
                if (hit) {
                    s_pts[3 * pos] = x[3 * i];
                    s_pts[3 * pos + 1] = x[3 * i + 1];
                    s_pts[3 * pos + 2] = x[3 * i + 2];
                }
                __syncthreads();
                if (tid == 0) {
                    for (int t = 0; t < cnt; ++t) {
                        sx += s_pts[3 * t];
                        sy += s_pts[3 * t + 1];
                        sz += s_pts[3 * t + 2];
                    }
                }
                __syncthreads();
            }
        }
        if (tid == 0) vox_write(A, g, rec, sx, sy, sz);
    }
}

}  // namespace

// Queue the whole downsample on s.  A holds the tables of the call (voxel.hpp VoxelArgs), status
// / n_out / error / n_big cleared to 0; n_slots: the slots of all tables (cleared here).
// max_chunks: the most chunks any cloud has; n_points: the call's points.
void launch_voxel(const VoxelArgs& A, int max_chunks, int64_t n_points, int64_t n_slots, hipStream_t s) {
    const dim3 per_chunk((unsigned)max_chunks, (unsigned)A.n_clouds), per_cloud((unsigned)A.n_clouds);
    const dim3 t(kVoxThreads);
    hipLaunchKernelGGL(k_vox_clear, dim3((unsigned)((n_slots + kVoxThreads - 1) / kVoxThreads)), t, 0, s, A.table, n_slots);
    hipLaunchKernelGGL(k_vox_bounds, per_chunk, t, 0, s, A);
    hipLaunchKernelGGL(k_vox_grid, per_cloud, t, 0, s, A);
    hipLaunchKernelGGL(k_vox_insert, per_chunk, t, 0, s, A);
    hipLaunchKernelGGL(k_vox_flags, per_chunk, t, 0, s, A);
    hipLaunchKernelGGL(k_vox_scan_chunks, per_cloud, t, 0, s, A);
    hipLaunchKernelGGL(k_vox_scan_clouds, dim3(1), t, 0, s, A);
    hipLaunchKernelGGL(k_vox_place, per_chunk, t, 0, s, A);
    hipLaunchKernelGGL(k_vox_scatter, per_chunk, t, 0, s, A);
    // (the number of voxels is the device's: one lane per point covers it)
    hipLaunchKernelGGL(k_vox_small, dim3((unsigned)((n_points + kVoxThreads - 1) / kVoxThreads)), t, 0, s, A);
    const int64_t big_blocks = A.big_cap < 2048 ? A.big_cap : 2048;
    hipLaunchKernelGGL(k_vox_big, dim3((unsigned)(big_blocks > 0 ? big_blocks : 1)), t, 0, s, A);
}

}  // namespace se3icp
