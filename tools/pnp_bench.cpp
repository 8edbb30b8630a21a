// pnp_bench.cpp -- times mcc::pnp::solvePnPBatch (GPU) and mcc::pnp::solvePnP (host, one core) on the
// same 88-corner planar views (tools/pnp_bench.py compiles and runs it).
//   pnp_bench N_VIEWS REPEATS HOST_VIEWS  ->  one line: device ms of each repeat, wall ms of the call,
//   host microseconds per view over the first HOST_VIEWS views, and how the two results compare
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mcc.h"
#include "mcc_pnp.hpp"

namespace {

struct Rng {
    unsigned long long s;
    double uniform() {
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return ((double)(s >> 11) + 0.5) / 9007199254740992.0;
    }
    double normal() { return std::sqrt(-2.0 * std::log(uniform())) * std::cos(6.283185307179586 * uniform()); }
};

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s n_views repeats host_views\n", argv[0]);
        return 2;
    }
    const int n_views = std::atoi(argv[1]), repeats = std::atoi(argv[2]), host_views = std::min(n_views, std::atoi(argv[3]));
    const int n = 88;
    const double K[9] = {1200, 0, 960, 0, 1180, 540, 0, 0, 1};
    const std::vector<double> D = {-0.1, 0.05, 1e-4, -2e-4, 0.01};
    std::vector<double> board;
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 11; ++j) board.insert(board.end(), {40.0 * j, 40.0 * i, 0.0});
    Rng rng{12345};
    std::vector<int> off(1, 0);
    std::vector<double> obj, img((size_t)2 * n * n_views);
    for (int v = 0; v < n_views; ++v) {
        const double r[3] = {0.6 * (rng.uniform() - 0.5), 0.6 * (rng.uniform() - 0.5), 0.6 * (rng.uniform() - 0.5)};
        const double t[3] = {-220 + 100 * (rng.uniform() - 0.5), -140 + 100 * (rng.uniform() - 0.5), 1000 + 800 * rng.uniform()};
        obj.insert(obj.end(), board.begin(), board.end());
        double* p = img.data() + (size_t)2 * n * v;
        mcc::pnp::projectPoints(board.data(), n, r, t, K, D, p);
        for (int k = 0; k < 2 * n; ++k) p[k] += 0.2 * rng.normal();
        off.push_back(off.back() + n);
    }
    try {
        std::vector<double> rv, tv, rms;
        std::vector<int> st;
        std::vector<double> dev, wall;
        for (int k = 0; k < repeats + 1; ++k) {   // the first call loads the code object: not counted
            double ms = 0;
            const double t0 = now_ms();
            mcc::pnp::solvePnPBatch(off, obj.data(), img.data(), nullptr, 1, K, D.data(), (int)D.size(), rv, tv, rms, st,
                                    50, 0, &ms);
            if (k) {
                dev.push_back(ms);
                wall.push_back(now_ms() - t0);
            }
        }
        int solved = 0;
        for (int s : st) solved += s == MCC_PNP_SOLVED;
        double max_rel = 0;
        const double t0 = now_ms();
        std::vector<double> hrms(host_views);
        for (int v = 0; v < host_views; ++v) {
            double r[3], t[3];
            hrms[v] = mcc::pnp::solvePnP(obj.data() + (size_t)3 * n * v, img.data() + (size_t)2 * n * v, n, K, D, r, t);
        }
        const double host_us = (now_ms() - t0) * 1e3 / std::max(host_views, 1);
        for (int v = 0; v < host_views; ++v) max_rel = std::fmax(max_rel, std::fabs(hrms[v] - rms[v]) / hrms[v]);
        std::sort(dev.begin(), dev.end());
        std::sort(wall.begin(), wall.end());
        std::printf("n_views %d corners %d solved %d device_ms_median %.6f device_ms_min %.6f device_ms_max %.6f "
                    "call_wall_ms_median %.6f host_us_per_view %.3f host_views %d max_rel_rms_diff %.3e\n",
                    n_views, n, solved, dev[dev.size() / 2], dev.front(), dev.back(), wall[wall.size() / 2], host_us,
                    host_views, max_rel);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
