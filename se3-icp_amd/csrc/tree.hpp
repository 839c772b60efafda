// tree.hpp — implicit balanced kd-trees (k_tree.hip) and their query helpers.
//
// Tree of a cloud with n points and depth L: node i of level l covers the tree
// positions [n*i/2^l, n*(i+1)/2^l); heap index 2^l - 1 + i; leaves are level L.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "common.hpp"

namespace se3icp {

constexpr int kLeafMax = 64;  // points per leaf (one wavefront)

struct TreeView {
    int32_t D;        // 3 or 12
    int32_t L;        // depth (leaves at level L)
    int32_t nnodes;   // 2^(L+1) nodes reserved per cloud (heap order)
    int32_t nclouds;
    int32_t npts;
    int32_t ld;
    const CloudDev* clouds;
    const int32_t* cloud_of;
    const float* vec;  // input vectors, original order: 12-D [ld][12] rows, 3-D [3][ld] columns
    // the input as [D][ld] columns (3-D: vec itself; 12-D: a copy k_tree_init writes), for the
    // passes that gather ONE coordinate per point (a 4-B column entry, not a 48-B row's sector)
    float* vecT;
    int32_t* perm;     // [ld] tree position (global slot) -> local point index
    int32_t* pos;      // [ld] point (global slot) -> local tree position
    float* tvec;       // vectors in tree order: 3-D [3][ld] columns, 12-D [ld][12] rows (tree_tv_ix)
    const double* vec64;  // optional f64 vectors (original order, the layout of vec) ...
    double* tvec64;       // ... copied into tree order (coalesced leaf / query-chunk loads): [3][ld], the
                          // points (3-D) or the translation rows (12-D: the loop reads whole frames by point)
    double4* tpt64;       // 3-D: the tree-ordered f64 points as (x, y, z, 0) records (one line per gather)
    int32_t vec64_sources_only;  // copy the f64 vectors of even (source) clouds only
    uint32_t* blo;     // [nclouds][nnodes][D] build scratch (orderable bits)
    uint32_t* bhi;
    float* scr;        // [D][ld] build scratch (k_tree_local: the vectors at the level-G positions)
    float* lo;         // [nclouds][nnodes][D] node boxes
    float* hi;
    const int32_t* host_n;  // host copy of the clouds' point counts (level split of the build)
    // Builders and adopters of this build (graph.hpp, graph_plan_trees): a cloud that holds the
    // points of an earlier one takes that cloud's finished order and computes only its own
    // tree-ordered vectors and boxes.  All null / 0: every cloud builds.
    const int32_t* role;  // [nclouds] kTreeBuilds, kTreeAbsent, or the cloud whose order it adopts
    const int32_t* list;  // the builders' cloud ids (nbuild), then the adopters' (nadopt)
    int32_t nbuild, nadopt;
};
constexpr int32_t kTreeBuilds = -1;  // builds its own tree
constexpr int32_t kTreeAbsent = -2;  // takes no part in this build (its tree comes from another one)

// cloud of the j-th builder / (j - nbuild)-th adopter
__device__ __forceinline__ int tree_list_cloud(const TreeView& t, int j) { return t.list ? t.list[j] : j; }
__device__ __forceinline__ bool tree_builds(const TreeView& t, int c) { return !t.role || t.role[c] == kTreeBuilds; }

__host__ __device__ __forceinline__ int tree_first(int n, int level, int i) {
    return (int)(((long long)n * i) >> level);
}
// node of level `level` containing local tree position x
__host__ __device__ __forceinline__ int tree_node_of(int x, int n, int level) {
    const long long v = ((long long)(x + 1) << level) + n - 1;
    return (int)(v / n) - 1;
}
__host__ __device__ __forceinline__ int tree_heap(int level, int i) { return (1 << level) - 1 + i; }
// element d of the input vector at global slot p: the 12-D vectors (SE(3) frames) are
// rows (a gather by the permutation reads one or two cache lines, not twelve), the 3-D
// points columns
__device__ __forceinline__ size_t tree_in_ix(const TreeView& t, int d, int p) {
    return t.D == 12 ? (size_t)p * 12 + d : (size_t)d * t.ld + p;
}
// coordinate d of the input vector at global slot p, from the column copy
__device__ __forceinline__ float tree_in_col(const TreeView& t, int d, int p) { return t.vecT[(size_t)d * t.ld + p]; }

// element d of the tree-ordered vector at global tree slot x: the 12-D vectors are 48-B
// rows (a leaf's 64 targets are one contiguous 3-KB run: three 16-B loads per lane instead
// of twelve strided ones), the 3-D points columns
template <int D>
__host__ __device__ __forceinline__ size_t tree_tv_ix(size_t ld, int x, int d) {
    return D == 12 ? (size_t)x * 12 + d : (size_t)d * ld + x;
}

// largest node of a level: node i holds floor(n (i+1) / 2^l) - floor(n i / 2^l) <= ceil(n / 2^l) points
__host__ __device__ __forceinline__ int tree_max_node(int n, int level) {
    return (int)(((long long)n + (1ll << level) - 1) >> level);
}

inline int tree_depth_for(int max_n) {
    int L = 0;
    while (tree_max_node(max_n, L) > kLeafMax) ++L;
    return L;
}

// The levels below G are built by one workgroup per level-G node (k_tree_local): nodes of
// at most kLocalMax points, split level by level into 2^r sub-nodes each.  A level whose
// sub-nodes fit the register sort of one wave (64 lanes x 2, 4 or kWaveSortPer keys) is
// sorted; a level of larger sub-nodes goes through the LDS partition, whose histograms and
// per-sub-node records are laid out for at most kLocalPartSubs of them.
constexpr int kLocalMax = 4096;     // power of two
constexpr int kWaveSortPer = 8;     // sub-nodes of <= 512 points: register sort by one wave
constexpr int kLocalPartSubs = 4;   // sub-nodes per level-G node the LDS partition can hold
constexpr int kLocalSubsMax = 128;  // sub-nodes per level-G node at the last level (tree_global_levels)
static_assert((kLocalMax & (kLocalMax - 1)) == 0 && kLocalMax <= 4096, "wave-sort keys carry the position in 12 bits");
// ceil(ceil(n / 2^G) / 2^r) = ceil(n / 2^(G+r)): with more than kLocalPartSubs sub-nodes
// (2^r >= 2 kLocalPartSubs) the largest holds <= kLocalMax / (2 kLocalPartSubs) points
static_assert(kLocalMax / (2 * kLocalPartSubs) <= 64 * kWaveSortPer,
              "a level of more than kLocalPartSubs sub-nodes must fit the wave sort");

// Keys per lane of the wave sort that orders the sub-nodes of level `level` (2, 4 or
// kWaveSortPer: networks of 128, 256 and 512 keys), or 0 where the level takes the LDS
// partition.  From the exact bound, the same for every node of the cloud's level.  (An
// estimate from the node's own size, ceil(m / nsub) + 1, read 513 for m = 4089 .. 4096 at
// nsub = 8 and sent eight sub-nodes to the partition.)
__host__ __device__ __forceinline__ int tree_local_sort_per(int n, int level) {
    const int mx = tree_max_node(n, level);
    return mx <= 128 ? 2 : (mx <= 256 ? 4 : (mx <= 64 * kWaveSortPer ? kWaveSortPer : 0));
}

// global levels until every node fits one workgroup's LDS sort (and <= kLocalSubsMax sub-nodes below)
inline int tree_global_levels(int max_n, int L) {
    int G = 0;
    while (G < L && tree_max_node(max_n, G) > kLocalMax) ++G;
    if (L - 1 - G > 7) G = L - 8;
    return G;
}

// qbuf: [npts] u32 scratch, perm_alt: [npts] the second permutation buffer of the global levels
// levels (may be null): [0] G, the global levels of this build, [1] H, how many of them took the
// multi-pass path -- what was launched, for the tree record
int build_trees(TreeView t, void* tmp, size_t tmp_bytes, uint32_t* qbuf, int32_t* perm_alt, hipStream_t s,
                int* levels = nullptr);
size_t tree_build_temp_bytes(int npts, int nclouds, int max_n, int L);
void tree_prof_report();  // (SE3ICP_PROF builds: k_tree_local's phase timeline, then reset)

}  // namespace se3icp
