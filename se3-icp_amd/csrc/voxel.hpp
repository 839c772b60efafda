// voxel.hpp — the arithmetic of the voxel-grid downsample (k_voxel.hip), for the host and the
// device: a cloud's grid from its bounds, a point's cell, the cell's packed key.
//
// Open3D PointCloud::VoxelDownSample (0.19) for xyz:
//   voxel_min_bound = min(p) - voxel_size * 0.5,  voxel_max_bound = max(p) + voxel_size * 0.5
//   "voxel_size is too small"  iff  voxel_size * INT_MAX < (voxel_max_bound - voxel_min_bound).maxCoeff()
//   cell(p) = floor((p - voxel_min_bound) / voxel_size)      per axis
// Every step is one IEEE f64 operation, never contracted and never a reciprocal multiply, so a
// restatement in any language that rounds to nearest gives the same cells bit for bit.
//
// Key: the three cell indices side by side, x lowest, each in as many bits as the largest index
// of its axis needs (0 bits for an axis with one cell).  The key must stay below 2^63 (the all
// ones word marks an empty table slot): three axes whose bit lengths sum to more than 63 are
// refused.  That is a departure from Open3D, which hashes an Eigen::Vector3i and has no such
// bound; it takes a cloud whose extents, in cells, multiply to more than 2^61.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SE3ICP_VOX_HD __host__ __device__ inline
#else
#define SE3ICP_VOX_HD inline
#endif

namespace se3icp {

constexpr int kVoxKeyBits = 63;
constexpr uint64_t kVoxEmptyKey = ~(uint64_t)0;  // no packed key: those stay below 2^63

// status values of voxel_make_grid (the entries map them to se3icp_status)
enum VoxelGridStatus : int32_t { VOX_OK = 0, VOX_NONFINITE = 1, VOX_TOO_SMALL = 2, VOX_KEY_OVERFLOW = 3 };

struct VoxelGrid {
    double min_bound[3];
    double voxel_size;
    int32_t bits[3];  // bit length of the largest cell index per axis
    int32_t status;   // VoxelGridStatus
};

// bits needed for the indices 0 .. max_index (0 for max_index == 0)
SE3ICP_VOX_HD int voxel_bit_length(uint64_t max_index) {
    int b = 0;
    while (b < 64 && (max_index >> b) != 0) ++b;
    return b;
}

SE3ICP_VOX_HD bool voxel_key_fits(const int32_t bits[3]) {
    return bits[0] >= 0 && bits[1] >= 0 && bits[2] >= 0 && (int64_t)bits[0] + bits[1] + bits[2] <= kVoxKeyBits;
}

// (bits fit, every index within its axis' bits)
SE3ICP_VOX_HD uint64_t voxel_pack(uint64_t ix, uint64_t iy, uint64_t iz, const int32_t bits[3]) {
    uint64_t k = ix;
    if (bits[1] > 0) k |= iy << bits[0];
    if (bits[2] > 0) k |= iz << (bits[0] + bits[1]);
    return k;
}

SE3ICP_VOX_HD void voxel_unpack(uint64_t key, const int32_t bits[3], uint64_t idx[3]) {
    int sh = 0;
    for (int a = 0; a < 3; ++a) {
        idx[a] = bits[a] > 0 ? (key >> sh) & ((((uint64_t)1) << bits[a]) - 1) : 0;
        sh += bits[a];
    }
}

// min(p) - voxel_size * 0.5
SE3ICP_VOX_HD double voxel_min_bound(double pmin, double voxel_size) {
#pragma clang fp contract(off)
    const double half = voxel_size * 0.5;
    return pmin - half;
}

// Open3D's "voxel_size is too small" over the three axes' bounds
SE3ICP_VOX_HD bool voxel_too_small(double voxel_size, const double pmin[3], const double pmax[3]) {
#pragma clang fp contract(off)
    const double half = voxel_size * 0.5;
    double ext = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double lo = pmin[a] - half, hi = pmax[a] + half;
        const double e = hi - lo;
        if (a == 0 || e > ext) ext = e;
    }
    const double reach = voxel_size * 2147483647.0;
    return reach < ext;
}

// floor((p - min_bound) / voxel_size): one subtraction, one division, floor
SE3ICP_VOX_HD double voxel_cell(double p, double min_bound, double voxel_size) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return floor(__ddiv_rn(__dsub_rn(p, min_bound), voxel_size));
#else
    const double d = p - min_bound;
    const double q = d / voxel_size;
    return std::floor(q);
#endif
}

// The grid of a cloud with finite bounds pmin <= pmax and a finite voxel_size > 0.
SE3ICP_VOX_HD void voxel_make_grid(const double pmin[3], const double pmax[3], double voxel_size, VoxelGrid* g) {
    g->voxel_size = voxel_size;
    g->status = VOX_OK;
    for (int a = 0; a < 3; ++a) {
        g->min_bound[a] = 0.0;
        g->bits[a] = 0;
    }
    for (int a = 0; a < 3; ++a)
        if (!(pmin[a] - pmin[a] == 0.0) || !(pmax[a] - pmax[a] == 0.0)) {  // NaN or an infinity
            g->status = VOX_NONFINITE;
            return;
        }
    if (voxel_too_small(voxel_size, pmin, pmax)) {
        g->status = VOX_TOO_SMALL;
        return;
    }
    for (int a = 0; a < 3; ++a) {
        g->min_bound[a] = voxel_min_bound(pmin[a], voxel_size);
        // the cell index is monotone in p, so the largest is the one of max(p); it is below
        // 2^31 + 1 here (not too small), and never negative (p >= min(p) >= min_bound)
        const double top = voxel_cell(pmax[a], g->min_bound[a], voxel_size);
        g->bits[a] = voxel_bit_length(top > 0.0 ? (uint64_t)top : 0);
    }
    if (!voxel_key_fits(g->bits)) g->status = VOX_KEY_OVERFLOW;
}

// the packed key of a point of the grid's cloud
SE3ICP_VOX_HD uint64_t voxel_key(const VoxelGrid& g, double x, double y, double z) {
    const double cx = voxel_cell(x, g.min_bound[0], g.voxel_size);
    const double cy = voxel_cell(y, g.min_bound[1], g.voxel_size);
    const double cz = voxel_cell(z, g.min_bound[2], g.voxel_size);
    return voxel_pack(cx > 0.0 ? (uint64_t)cx : 0, cy > 0.0 ? (uint64_t)cy : 0, cz > 0.0 ? (uint64_t)cz : 0, g.bits);
}

// A table slot for a key: the splitmix64 finalizer, masked to the table's power-of-two size.
SE3ICP_VOX_HD uint64_t voxel_hash(uint64_t k) {
    k ^= k >> 30;
    k *= 0xBF58476D1CE4E5B9ull;
    k ^= k >> 27;
    k *= 0x94D049BB133111EBull;
    k ^= k >> 31;
    return k;
}

// slots of a cloud's table: a power of two, at least twice its points (and at least 64)
inline int64_t voxel_table_slots(int64_t n) {
    int64_t c = 64;
    while (c < 2 * n) c <<= 1;
    return c;
}

// ---- the tables of one call (k_voxel.hip, Engine::voxel_downsample)
constexpr int kVoxChunkPoints = 1024;  // consecutive points of a cloud per block
constexpr int kVoxLane = 32;           // voxels of up to this many points: one lane orders and adds them
constexpr int kVoxLds = 2048;          // up to this many: a block ranks the members in LDS; more: a pass over the cloud

struct VoxelCloud {
    int64_t off;     // first point in the caller's xyz
    int64_t pt0;     // first point in the call's own per-point arrays (clouds back to back from 0)
    int64_t tab;     // first slot of its table
    int64_t slots;   // voxel_table_slots(n)
    int64_t chunk0;  // first of its chunks in the per-chunk arrays
    double voxel_size;
    int32_t n, nchunks;
};

// A table slot: what the passes read and update of a voxel lies in one 16-byte word (one
// memory transaction for the key, the first index and the count).
struct alignas(16) VoxelSlot {
    unsigned long long key;  // the packed key, kVoxEmptyKey while free
    int32_t first;           // lowest point index of the voxel (kVoxNoIndex while free)
    int32_t count;           // its points; from k_vox_place on the cursor of its segment
};
constexpr int32_t kVoxNoIndex = 0x7fffffff;

struct VoxelRec {  // an output voxel
    int32_t first;  // lowest point index, relative to the cloud
    int32_t count;
    int32_t seg;    // first entry of its members in the call's member list
    int32_t cloud;
};

struct VoxelArgs {
    int32_t n_clouds;
    int32_t big_cap;              // entries of `big`
    const double* xyz;            // the caller's clouds
    const VoxelCloud* clouds;
    VoxelGrid* grids;             // [n_clouds]
    double* minmax;               // [chunks][6]
    int32_t* chunk_sums;          // [chunks][2]: first points, and their voxels' counts
    VoxelSlot* table;             // [slots] the clouds' tables back to back
    int32_t* vid;                 // [points] the point's slot within its cloud's table, -1 without one
    int32_t* members;             // [points] point indices, a voxel's in one segment
    VoxelRec* recs;               // [points] the output voxels, in output order
    int32_t* big;                 // output voxels of more than kVoxLane points
    int32_t* status;              // [n_clouds] VoxelGridStatus
    int32_t* n_out;               // [n_clouds]
    int32_t* error;               // a full table or an inconsistent list: SE3ICP_ERR_INTERNAL
    int32_t* n_big;
    long long* out_off;           // [n_clouds + 1]
    double* out;                  // the caller's outputs
    int32_t* out_count;           // (may be null)
    int32_t* out_first;           // (may be null)
};

// The argument checks of the entries, before any device is looked up: 0, or the status.
inline int voxel_check_sizes(int64_t n_clouds, const int64_t* off, const double* voxel_size, int err_invalid,
                             int err_empty) {
    if (n_clouds <= 0 || !off || !voxel_size) return err_invalid;
    for (int64_t c = 0; c < n_clouds; ++c)
        if (!(voxel_size[c] > 0.0) || !std::isfinite(voxel_size[c])) return err_invalid;
    for (int64_t c = 0; c < n_clouds; ++c) {
        if (off[c + 1] < off[c]) return err_invalid;
        if (off[c + 1] == off[c]) return err_empty;
    }
    return 0;
}

}  // namespace se3icp
