// test_pnp_replay.cpp -- the batched solvePnP's per-view arithmetic (csrc/mcc_pnp_device.hpp) replayed
// on the CPU with one lane, against the truth and against the host solver (tests/test_pnp_replay.py).
//
// The kernel's wave primitives are replaced by their one-lane meaning (a sum over the wave is the lane's
// own sum, lane 0's value is the value, no fence), the LDS slice by plain arrays; everything else -- the
// undistortion, both DLTs, the Jacobi in "LDS", the polar factor, the analytic Jacobian and the LM policy
// -- is the code the GPU runs.  It cannot see the lanes' summation order; the GPU tests do.
//
//   exact data (the C++ selftest's camera, its two D vectors and none; four poses; planar n = 4 .. 1 024,
//   non-planar n = 6 .. 117): status 0 and the selftest's bounds rms < 1e-6, |dr| < 1e-7, |dt| < 1e-4,
//   with max_iter = 50 and for the closed-form pose alone (max_iter = 0);
//   0.2 px noise, n >= 20: the same minimum as mcc::pnp::solvePnP (relative RMS difference <= 1e-6);
//   3 points -> status 1, points on a line -> status 2.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#define MCC_PNP_LANES 1
#define MCC_PNP_FN inline
namespace mcc {
inline void pnp_wave_sync() {}
inline double pnp_uniform(double v) { return v; }
inline int pnp_uniform(int v) { return v; }
inline double pnp_wave_sum(double v) { return v; }
}  // namespace mcc
#include "mcc_pnp_device.hpp"
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

const double kK[9] = {1200, 0, 960, 0, 1180, 540, 0, 0, 1};
const std::vector<std::vector<double>> kDs = {{}, {-0.1, 0.05, 1e-4, -2e-4, 0.0},
                                              {-0.12, 0.08, 2e-4, 1e-4, 0.01, 0.002, -0.001, 0.003}};
const double kPoses[4][6] = {{0.3, -0.4, 0.2, -150, -90, 1300},
                             {-0.2, 0.35, -0.1, -250, -180, 900},
                             {0.05, 0.02, 1.4, 150, -200, 1800},
                             {0.8727, 0.05, 0.0, -200, -100, 1400}};

mcc::PnpCam camera(const std::vector<double>& D) {
    double k[12] = {0};
    for (size_t i = 0; i < D.size(); ++i) k[i] = D[i];
    return mcc::PnpCam{kK[0], kK[4], kK[2], kK[5], k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8], k[9], k[10], k[11]};
}

std::vector<double> target(int n, bool planar) {
    std::vector<double> obj;
    int w = 1;
    while (w * w < n) ++w;
    const double pitch = n == 1024 ? 10.0 : 40.0;
    for (int i = 0; i < n; ++i) {
        const int a = i % w, b = i / w;
        obj.insert(obj.end(), {pitch * a, pitch * b, planar ? 0.0 : 60.0 * std::sin(0.7 * b + 1.3 * a) + 25.0 * std::cos(0.37 * i)});
    }
    return obj;
}

int solve(const std::vector<double>& obj, const std::vector<double>& img, const mcc::PnpCam& c, int max_iter, double* r,
          double* t, double& rms) {
    const int n = (int)obj.size() / 3;
    std::vector<double> xy(2 * (size_t)n + 2);
    double A[144], V[144];
    return mcc::pnp_solve_view(obj.data(), img.data(), n, c, max_iter, xy.data(), A, V, 0, r, t, rms);
}

}  // namespace

int main() {
    int bad = 0, cases = 0;
    Rng rng{2024};
    for (const auto& D : kDs)
        for (int planar = 0; planar < 2; ++planar)
            for (int n : {4, 6, 20, 64, 65, 88, 117, 1024})
                for (const auto& pose : kPoses) {
                    if ((!planar && (n < 6 || n == 1024)) || (planar && n == 6)) continue;
                    const std::vector<double> obj = target(n, planar);
                    std::vector<double> img(2 * (size_t)n);
                    mcc::pnp::projectPoints(obj.data(), n, pose, pose + 3, kK, D, img.data());
                    const mcc::PnpCam c = camera(D);
                    for (int max_iter : {50, 0}) {
                        double r[3], t[3], rms;
                        const int st = solve(obj, img, c, max_iter, r, t, rms);
                        double dr = 0, dt = 0;
                        for (int k = 0; k < 3; ++k) {
                            dr = std::fmax(dr, std::fabs(r[k] - pose[k]));
                            dt = std::fmax(dt, std::fabs(t[k] - pose[3 + k]));
                        }
                        ++cases;
                        if (st != 0 || !(rms >= 0 && rms < 1e-6) || !(dr < 1e-7) || !(dt < 1e-4)) {
                            ++bad;
                            std::printf("FAIL exact nd %zu planar %d n %d max_iter %d: status %d rms %.3e dr %.3e dt %.3e\n",
                                        D.size(), planar, n, max_iter, st, rms, dr, dt);
                        }
                    }
                    if (n < 20) continue;
                    for (double& p : img) p += 0.2 * rng.normal();
                    double r[3], t[3], rms, hr[3], ht[3];
                    const int st = solve(obj, img, c, 50, r, t, rms);
                    const double hrms = mcc::pnp::solvePnP(obj.data(), img.data(), n, kK, D, hr, ht);
                    ++cases;
                    if (st != 0 || !(hrms > 0) || !(std::fabs(rms - hrms) <= 1e-6 * hrms)) {
                        ++bad;
                        std::printf("FAIL noisy nd %zu planar %d n %d: status %d rms %.17g host %.17g\n", D.size(), planar, n,
                                    st, rms, hrms);
                    }
                }
    {   // too few points; points on one line
        std::vector<double> obj = target(20, true), img(40);
        for (int i = 0; i < 20; ++i) obj[3 * i + 1] = obj[3 * i] / 3.0;
        mcc::pnp::projectPoints(obj.data(), 20, kPoses[0], kPoses[0] + 3, kK, kDs[1], img.data());
        for (double& p : img) p += 0.2 * rng.normal();
        double r[3], t[3], rms;
        const int line = solve(obj, img, camera(kDs[1]), 50, r, t, rms);
        if (line != mcc::kPnpDegenerate || rms != -1.0) ++bad, std::printf("FAIL collinear: status %d rms %g\n", line, rms);
        obj.resize(9);
        img.resize(6);
        const int few = solve(obj, img, camera(kDs[1]), 50, r, t, rms);
        if (few != mcc::kPnpTooFew || rms != -1.0) ++bad, std::printf("FAIL 3 points: status %d rms %g\n", few, rms);
        const std::vector<double> relief = target(5, false);
        img.resize(10);
        mcc::pnp::projectPoints(relief.data(), 5, kPoses[0], kPoses[0] + 3, kK, kDs[1], img.data());
        const int few5 = solve(relief, img, camera(kDs[1]), 50, r, t, rms);
        if (few5 != mcc::kPnpTooFew) ++bad, std::printf("FAIL 5 points off a plane: status %d\n", few5);
    }
    std::printf("%d cases, %d failed\n", cases, bad);
    if (!bad) std::printf("replay ok\n");
    return bad ? 1 : 0;
}
