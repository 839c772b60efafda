// Host build of gicp_cov_from_normal (se3-icp_amd/csrc/devmath.hpp: the covariance k_reduce
// rebuilds from the stored normal of every GICP correspondence) for tests/test_devmath_host.py:
// reads one normal per line from stdin ("x y z", decimal or hexadecimal floats) and writes the
// six entries xx xy xz yy yz zz as hexadecimal floats, one line per normal, with eps = 1e-3.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "devmath.hpp"

using namespace se3icp;

int main() {
    std::string tx, ty, tz;
    while (std::cin >> tx >> ty >> tz) {
        const d3 n{std::strtod(tx.c_str(), nullptr), std::strtod(ty.c_str(), nullptr), std::strtod(tz.c_str(), nullptr)};
        double c[6];
        gicp_cov_from_normal(n, 1e-3, c);
        std::printf("%a %a %a %a %a %a\n", c[0], c[1], c[2], c[3], c[4], c[5]);
    }
    return 0;
}
