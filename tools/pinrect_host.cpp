// pinrect_host.cpp -- the host side of tools/pinrect_bench.py's comparison: mcc::pnp::undistortPoints (libmcc_host.so),
// one call per point as a caller without the batch entry point would make them, timed on one CPU core.  Built by the
// tool into a shared library of its own and loaded into the tool's process.
#include <chrono>
#include <vector>

#include "mcc_pnp.hpp"

extern "C" double pinrect_host_undistort_ms(const double* px, int n, const double* K, const double* D, int nd, int iterations,
                                            double* out) {
    const std::vector<double> Dv(D, D + nd);
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < n; ++i) mcc::pnp::undistortPoints(px + 2 * (size_t)i, 1, K, Dv, out + 2 * (size_t)i, iterations);
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
