// Host build of the sweep planning of se3-icp_amd/csrc/sweep.hpp (sweep_group_size,
// sweep_group, sweep_num_groups: what Engine::register_sweep calls) for
// tests/test_sweep_host.py.  Over a grid of variant counts (1 .. 50), caller bounds
// (0 .. 9, 47, 100), batch sizes (1 point .. 2^30 + 1), cloud counts and byte budgets
// (nothing .. 288 GB):
//   range   1 <= G <= n_variants
//   bound   G <= max_group when one is given
//   points  G * points < 2^30 (whenever one variant alone is below it)
//   budget  G * (points * bytes_per_point + clouds * bytes_per_cloud) <= budget (whenever
//           one variant alone fits)
//   cover   the groups hold every variant exactly once, in order, none empty, none over G
//   fill    left to itself (max_group = 0) the engine takes at most kSweepAutoMax variants
//           and kSweepAutoPoints points a group, and the whole sweep when it is within both
// Prints one line per check, "<check> ok" or "<check> FAIL <count>", then "checked <n>";
// exits 1 if any failed.
#include <cstdio>
#include <vector>

#include "sweep.hpp"

using namespace se3icp;

int main() {
    enum { RANGE, BOUND, POINTS, BUDGET, COVER, FILL, NCHECK };
    const char* const names[NCHECK] = {"range", "bound", "points", "budget", "cover", "fill"};
    long bad[NCHECK] = {};
    long checked = 0;
    const int max_groups[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 47, 100};
    const int64_t points[] = {1, 196, 14411, 500000, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, 17000000,
                              ((int64_t)1 << 29) - 1, (int64_t)1 << 29, ((int64_t)1 << 30) - 1, (int64_t)1 << 30,
                              ((int64_t)1 << 30) + 1};
    const int64_t clouds[] = {2, 16, 128};
    const int64_t budgets[] = {0, 1 << 20, (int64_t)1 << 30, (int64_t)16 << 30, (int64_t)288 << 30};
    for (int nv = 1; nv <= 50; ++nv)
        for (int mg : max_groups)
            for (int64_t pts : points)
                for (int64_t cl : clouds)
                    for (int64_t budget : budgets) {
                        ++checked;
                        const int G = sweep_group_size(nv, mg, pts, cl, kSweepBytesPerPoint, kSweepBytesPerCloud, budget);
                        const int64_t per = pts * kSweepBytesPerPoint + cl * kSweepBytesPerCloud;
                        if (G < 1 || G > nv) ++bad[RANGE];
                        if (mg > 0 && G > mg) ++bad[BOUND];
                        if (pts < kSweepPointLimit && (int64_t)G * pts >= kSweepPointLimit) ++bad[POINTS];
                        if (per <= budget && (int64_t)G * per > budget) ++bad[BUDGET];
                        if (per > budget && G != 1) ++bad[BUDGET];
                        if (pts >= kSweepPointLimit && G != 1) ++bad[POINTS];
                        // the groups
                        std::vector<int> seen(nv, 0);
                        const int ng = sweep_num_groups(nv, G);
                        bool cover = ng >= 1;
                        int next = 0;
                        for (int k = 0; k < ng; ++k) {
                            int first = -1, count = -1;
                            sweep_group(nv, G, k, &first, &count);
                            if (first != next || count < 1 || count > G) cover = false;
                            for (int v = first; v < first + count && v >= 0 && v < nv; ++v) ++seen[v];
                            next = first + count;
                        }
                        if (next != nv) cover = false;
                        for (int v = 0; v < nv; ++v)
                            if (seen[v] != 1) cover = false;
                        if (!cover) ++bad[COVER];
                        if (mg == 0) {
                            if (G > kSweepAutoMax) ++bad[FILL];
                            if (G > 1 && (int64_t)G * pts > kSweepAutoPoints) ++bad[FILL];
                            if (nv <= kSweepAutoMax && (int64_t)nv * pts <= kSweepAutoPoints &&
                                (int64_t)nv * per <= budget && G != nv)
                                ++bad[FILL];
                        }
                    }
    bool fail = false;
    for (int c = 0; c < NCHECK; ++c) {
        if (bad[c]) {
            std::printf("%s FAIL %ld\n", names[c], bad[c]);
            fail = true;
        } else {
            std::printf("%s ok\n", names[c]);
        }
    }
    std::printf("checked %ld\n", checked);
    return fail ? 1 : 0;
}
