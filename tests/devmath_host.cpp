// Host build of se3-icp_amd/csrc/devmath.hpp for tests/test_devmath_host.py.  Two modes, both
// reading decimal or hexadecimal floats from stdin and writing hexadecimal floats:
//   (no argument)  gicp_cov_from_normal (the covariance k_reduce rebuilds from the stored normal
//                  of every GICP correspondence): one normal "x y z" per line; the six entries
//                  xx xy xz yy yz zz per line, with eps = 1e-3.
//   eig            the two eigen-solvers of the setup kernels: one symmetric matrix
//                  "a00 a01 a02 a11 a12 a22" per line; jacobi_smallest_evec's vector, then
//                  fast_eigen3x3's, per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "devmath.hpp"

using namespace se3icp;

static double num(const std::string& t) { return std::strtod(t.c_str(), nullptr); }

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "eig") == 0) {
        std::string t[6];
        while (std::cin >> t[0] >> t[1] >> t[2] >> t[3] >> t[4] >> t[5]) {
            const double a[6] = {num(t[0]), num(t[1]), num(t[2]), num(t[3]), num(t[4]), num(t[5])};
            const d3 j = jacobi_smallest_evec(a[0], a[1], a[2], a[3], a[4], a[5]);
            const d3 f = fast_eigen3x3(a[0], a[1], a[2], a[3], a[4], a[5]);
            std::printf("%a %a %a %a %a %a\n", j.x, j.y, j.z, f.x, f.y, f.z);
        }
        return 0;
    }
    std::string tx, ty, tz;
    while (std::cin >> tx >> ty >> tz) {
        const d3 n{num(tx), num(ty), num(tz)};
        double c[6];
        gicp_cov_from_normal(n, 1e-3, c);
        std::printf("%a %a %a %a %a %a\n", c[0], c[1], c[2], c[3], c[4], c[5]);
    }
    return 0;
}
