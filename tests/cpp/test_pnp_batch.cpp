// test_pnp_batch.cpp -- mcc::pnp::solvePnPBatch (GPU, analytic Jacobian) against mcc::pnp::solvePnP
// (host, central differences) on noisy views (tests/test_pnp_batch_cpp.py compiles and runs it).
//
// Inputs: 0.2 px Gaussian noise, n in {20, 88, 117}, planar and non-planar targets, four poses (one
// oblique: the board tilted 50 degrees), nd in {0, 5, 8}: 72 views.  Both solvers reach the same
// least-squares minimum by different Jacobians and summation orders, so they agree closely but not bit
// for bit.
//
// Bounds: 10 x the largest differences measured on an MI355X over these views (the factor covers the
// inputs of later seeds):
//   measured  relative RMS difference 8.664e-14,  |dr| 2.696e-08 rad,  |dt| 7.699e-07 mm
//   bounds                            8.664e-13        2.696e-07            7.699e-06
// and, whatever is measured, a relative RMS difference above 1e-6 is a different minimum or a run that
// did not converge: a failure, not a tolerance to widen.
//
//   test_pnp_batch selftest   host only: the wrapper throws on a bad argument, with the library's message
//   test_pnp_batch run        prints the three maxima, exit 0 when they are inside the bounds
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "mcc.h"
#include "mcc_pnp.hpp"

namespace {

constexpr double kBoundRelRms = 8.664e-13, kBoundR = 2.696e-7, kBoundT = 7.699e-6;
constexpr double kHardRelRms = 1e-6;

// a generator of its own, so the inputs do not depend on the standard library's distributions
struct Rng {
    unsigned long long s;
    double uniform() {   // (0, 1)
        s = s * 6364136223846793005ULL + 1442695040888963407ULL;
        return ((double)(s >> 11) + 0.5) / 9007199254740992.0;
    }
    double normal() { return std::sqrt(-2.0 * std::log(uniform())) * std::cos(6.283185307179586 * uniform()); }
};

struct View {
    int n, nd;
    std::vector<double> obj, img;
};

const double kK[9] = {1200, 0, 960, 0, 1180, 540, 0, 0, 1};
const double kD[8] = {-0.12, 0.08, 2e-4, 1e-4, 0.01, 0.002, -0.001, 0.003};
const double kPoses[4][6] = {{0.3, -0.4, 0.2, -150, -90, 1300},
                             {-0.2, 0.35, -0.1, -250, -180, 900},
                             {0.05, 0.02, 1.4, 150, -200, 1800},
                             {0.8727, 0.05, 0.0, -200, -100, 1400}};   // the board tilted 50 degrees about x

std::vector<View> make_views(int nd) {
    std::vector<View> views;
    Rng rng{0x9E3779B97F4A7C15ULL + (unsigned)nd};
    const std::vector<double> D(kD, kD + nd);
    for (int n : {20, 88, 117})
        for (int planar = 0; planar < 2; ++planar)
            for (const auto& pose : kPoses) {
                View v;
                v.n = n;
                v.nd = nd;
                int w = 1;
                while (w * w < n) ++w;
                for (int i = 0; i < n; ++i) {
                    const int a = i % w, b = i / w;
                    v.obj.insert(v.obj.end(), {40.0 * a, 40.0 * b,
                                               planar ? 0.0 : 60.0 * std::sin(0.7 * b + 1.3 * a) + 25.0 * std::cos(0.37 * i)});
                }
                v.img.resize(2 * (size_t)n);
                mcc::pnp::projectPoints(v.obj.data(), n, pose, pose + 3, kK, D, v.img.data());
                for (double& p : v.img) p += 0.2 * rng.normal();
                views.push_back(std::move(v));
            }
    return views;
}

int selftest() {
    std::vector<double> r, t, rms;
    std::vector<int> st;
    const double obj[12] = {0, 0, 0, 40, 0, 0, 0, 40, 0, 40, 40, 0}, img[8] = {900, 500, 940, 500, 900, 540, 940, 540};
    int bad = 0;
    auto throws = [&](const std::vector<int>& off, int nd, const int* cam, const char* what) {
        try {
            mcc::pnp::solvePnPBatch(off, obj, img, cam, 1, kK, kD, nd, r, t, rms, st);
        } catch (const std::runtime_error& e) {
            if (std::strstr(e.what(), "(-1)") && std::strstr(e.what(), what)) return;
            std::printf("wrong message: %s\n", e.what());
        }
        ++bad;
        std::printf("FAIL: no MCC_EINVAL for %s\n", what);
    };
    const int cam_bad[1] = {3};
    throws({0, 4}, 6, nullptr, "nd");
    throws({0, 4}, 5, cam_bad, "view_cam");
    throws({4, 0}, 5, nullptr, "monotone");
    throws({0}, 5, nullptr, "n_views");
    if (!bad) std::printf("selftest ok\n");
    return bad ? 1 : 0;
}

int run() {
    double max_rel = 0, max_r = 0, max_t = 0;
    int solved = 0, total = 0;
    for (int nd : {0, 5, 8}) {
        const std::vector<View> views = make_views(nd);
        std::vector<int> off(1, 0);
        std::vector<double> obj, img;
        for (const View& v : views) {
            off.push_back(off.back() + v.n);
            obj.insert(obj.end(), v.obj.begin(), v.obj.end());
            img.insert(img.end(), v.img.begin(), v.img.end());
        }
        std::vector<double> r, t, rms;
        std::vector<int> st;
        mcc::pnp::solvePnPBatch(off, obj.data(), img.data(), nullptr, 1, kK, kD, nd, r, t, rms, st);
        const std::vector<double> D(kD, kD + nd);
        for (size_t i = 0; i < views.size(); ++i, ++total) {
            double hr[3], ht[3];
            const double hrms = mcc::pnp::solvePnP(views[i].obj.data(), views[i].img.data(), views[i].n, kK, D, hr, ht);
            if (st[i] != MCC_PNP_SOLVED || !(hrms > 0)) {
                std::printf("view %zu (nd %d, n %d): status %d, host rms %g\n", i, nd, views[i].n, st[i], hrms);
                continue;
            }
            ++solved;
            // 0.2 px noise on both coordinates: an RMS per corner near 0.28 px
            if (!(hrms > 0.1 && hrms < 0.5)) std::printf("view %zu (nd %d): host rms %g px\n", i, nd, hrms), --solved;
            max_rel = std::fmax(max_rel, std::fabs(rms[i] - hrms) / hrms);
            for (int k = 0; k < 3; ++k) {
                max_r = std::fmax(max_r, std::fabs(r[3 * i + k] - hr[k]));
                max_t = std::fmax(max_t, std::fabs(t[3 * i + k] - ht[k]));
            }
        }
    }
    std::printf("views %d solved %d\n", total, solved);
    std::printf("measured max_rel_rms %.3e max_dr %.3e max_dt %.3e\n", max_rel, max_r, max_t);
    std::printf("bounds   max_rel_rms %.3e max_dr %.3e max_dt %.3e (hard: rel rms %.0e)\n", kBoundRelRms, kBoundR, kBoundT,
                kHardRelRms);
    const bool ok = solved == total && total == 72 && max_rel <= kHardRelRms && max_rel <= kBoundRelRms &&
                    max_r <= kBoundR && max_t <= kBoundT;
    std::printf(ok ? "run ok\n" : "run FAILED\n");
    return ok ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        if (argc == 2 && !std::strcmp(argv[1], "selftest")) return selftest();
        if (argc == 2 && !std::strcmp(argv[1], "run")) return run();
    } catch (const std::exception& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    std::printf("usage: %s selftest | run\n", argv[0]);
    return 2;
}
