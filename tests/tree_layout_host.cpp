// Host build of the kd-tree layout arithmetic of se3-icp_amd/csrc/tree.hpp (the
// __host__ __device__ helpers k_tree_local, k_nn_prep and the engine share) for
// tests/test_tree_layout.py.  For a single cloud of n points, every n in 1 .. N (argv[1],
// default 300000) and a handful of sizes around 2^k * kLocalMax up to 2^22, and every level:
//   bound      tree_max_node(n, l) is the brute-force largest tree_first difference of level l
//   partition  a level that takes k_tree_local's LDS partition has <= kLocalPartSubs sub-nodes
//   sort       a level that takes the wave sort has no sub-node larger than its network
//   subs       <= kLocalSubsMax sub-nodes per level-G node, <= kLocalMax points in it, its
//              sample (every 16th point) <= kLocalMax / 16, leaves <= kLeafMax, a chunk
//              (a node of level L - 4) <= kChunkQ positions
//   inverse    tree_node_of inverts tree_first at the first and last position of every node
// Prints one line per check, "<check> ok" or "<check> FAIL <count> sizes: a-b c-d ..." (the
// failing n as ranges), and exits 1 if any failed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "tree.hpp"

using namespace se3icp;

namespace {
enum Check { BOUND, PARTITION, SORT, SUBS, INVERSE, NCHECK };
const char* const kNames[NCHECK] = {"bound", "partition", "sort", "subs", "inverse"};

unsigned check_size(int n) {
    unsigned bad = 0;
    const int L = tree_depth_for(n), G = tree_global_levels(n, L);
    if (G < 0 || G > L) return 1u << SUBS;
    for (int l = 0; l <= L; ++l) {
        int mx = 0;
        for (int i = 0; i < (1 << l); ++i) {
            const int a = tree_first(n, l, i), b = tree_first(n, l, i + 1);
            mx = std::max(mx, b - a);
            if (b > a && (tree_node_of(a, n, l) != i || tree_node_of(b - 1, n, l) != i)) bad |= 1u << INVERSE;
        }
        if (tree_first(n, l, 0) != 0 || tree_first(n, l, 1 << l) != n) bad |= 1u << INVERSE;
        if (mx != tree_max_node(n, l)) bad |= 1u << BOUND;
        if (l >= G && l < L) {  // a level k_tree_local splits: 2^(l - G) sub-nodes per workgroup
            const int nsub = 1 << (l - G);
            const int per = tree_local_sort_per(n, l);
            if (per == 0 && nsub > kLocalPartSubs) bad |= 1u << PARTITION;
            if (per != 0 && (mx > 64 * per || (per != 2 && per != 4 && per != kWaveSortPer))) bad |= 1u << SORT;
            if (nsub > kLocalSubsMax) bad |= 1u << SUBS;
        }
    }
    if (G < L) {
        const int m = tree_max_node(n, G);
        if (m > kLocalMax || (m + 15) / 16 > kLocalMax / 16) bad |= 1u << SUBS;
    }
    if (tree_max_node(n, L) > kLeafMax) bad |= 1u << SUBS;
    if (tree_max_node(n, std::max(0, L - 4)) > kChunkQ) bad |= 1u << SUBS;
    return bad;
}
}  // namespace

int main(int argc, char** argv) {
    const int N = argc > 1 ? std::atoi(argv[1]) : 300000;
    std::vector<int> sizes;
    for (int n = 1; n <= N; ++n) sizes.push_back(n);
    for (int k = 0; k <= 10; ++k)
        for (int d : {-8, -7, -1, 0, 1}) {
            const int n = (kLocalMax << k) + d;
            if (n > N) sizes.push_back(n);
        }
    std::vector<unsigned> bad(sizes.size(), 0u);
    const unsigned nt = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            for (size_t j = t; j < sizes.size(); j += nt) bad[j] = check_size(sizes[j]);
        });
    for (std::thread& x : th) x.join();
    bool fail = false;
    for (int c = 0; c < NCHECK; ++c) {
        std::string ranges;
        long count = 0;
        for (size_t j = 0; j < sizes.size();) {
            if (!((bad[j] >> c) & 1u)) { ++j; continue; }
            size_t e = j;
            while (e + 1 < sizes.size() && ((bad[e + 1] >> c) & 1u) && sizes[e + 1] == sizes[e] + 1) ++e;
            count += (long)(e - j + 1);
            ranges += " " + std::to_string(sizes[j]) + (e > j ? "-" + std::to_string(sizes[e]) : std::string());
            j = e + 1;
        }
        if (count) {
            fail = true;
            std::printf("%s FAIL %ld sizes:%s\n", kNames[c], count, ranges.c_str());
        } else {
            std::printf("%s ok\n", kNames[c]);
        }
    }
    std::printf("checked %zu sizes\n", sizes.size());
    return fail ? 1 : 0;
}
