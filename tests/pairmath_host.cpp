// Host build of se3-icp_amd/csrc/pairmath.hpp (the per-pair solve and loop state machine
// that k_reduce_final runs on the GPU) for tests/test_pairmath.py: reads cases from
// stdin, writes results to stdout, one line per case.
//   U <15 moments> <n>        -> umeyama_from_moments: 16 values (row-major 4x4)
//   N <27 normal-eq values>   -> solve_normal_equations: 16 values
//   S <16 T> <kind> <est> <sw> <iter> <max_iter> <max_se3> <mse> <mse_switch> <sf> <K>
//     <mse_cur> <28 reduced values>
//                             -> pair_close_iteration then pair_open_iteration:
//                                iter pure sw done phase phase_start mse_cur rel + 16 T
//   P <3 pivot> <15 moments about the pivot> <n>
//                             -> pair_close_iteration (pt2pt, from the identity pose): 16 values
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "pairmath.hpp"

using namespace se3icp;

// (operator>> does not read "nan" or "inf": it fails and leaves every later value unset)
static void rd(double& x) {
    std::string t;
    std::cin >> t;
    x = std::strtod(t.c_str(), nullptr);
}

static void print_m4(const M4& T) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) std::printf(" %.17g", T.m[i][j]);
}

int main() {
    std::string tag;
    while (std::cin >> tag) {
        if (tag == "U") {
            double s[15], n;
            for (double& x : s) rd(x);
            rd(n);
            print_m4(umeyama_from_moments(s, n));
        } else if (tag == "N") {
            double a[27];
            for (double& x : a) rd(x);
            print_m4(solve_normal_equations(a));
        } else if (tag == "S") {
            PairState S{};
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) rd(S.T.m[i][j]);
            int est;
            std::cin >> S.kind >> est >> S.sw >> S.iter >> S.max_iter >> S.max_se3;
            rd(S.mse);
            rd(S.mse_switch);
            rd(S.sf);
            rd(S.K);
            rd(S.mse_cur);
            double acc[28];
            for (double& x : acc) rd(x);
            S.phase = PHASE_SE3;
            S.phase_start = 1;
            PairDev P{};
            pair_close_iteration(S, est, acc);
            pair_open_iteration(S, P);
            std::printf("%d %d %d %d %d %d %.17g %.17g", S.iter, S.pure, S.sw, S.done, P.phase, S.phase_start,
                        S.mse_cur, S.rel);
            print_m4(S.T);
        } else if (tag == "P") {
            double piv[3], acc[28] = {};
            for (double& x : piv) rd(x);
            for (int i = 0; i < 16; ++i) rd(acc[i]);
            PairState S{};
            S.T = M4::eye();
            S.kind = KIND_ICP;
            S.K = acc[15];
            S.iter = 1;
            S.max_iter = 2;
            pair_close_iteration(S, EST_PT2PT, acc, piv);
            print_m4(S.T);
        } else {
            return 2;
        }
        std::printf("\n");
    }
    return 0;
}
