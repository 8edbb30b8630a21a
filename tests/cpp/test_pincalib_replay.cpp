// test_pincalib_replay.cpp -- the pinhole calibrateCamera's per-view arithmetic (csrc/mcc_pincalib_device.hpp
// and pnp_rows / pnp_rows_intr of csrc/mcc_pnp_device.hpp) replayed on the CPU with one lane
// (tests/test_pincalib_replay.py), as tests/cpp/test_pnp_replay.cpp does for the batched solvePnP.
//
//   rows: at twelve corners per (pose, distortion) the 2 x 6 pose rows and the 2 x 12 intrinsic rows against
//   central differences of pnp_residual (steps 1e-5 on r, 1e-3 on t and on fx fy cx cy, 1e-6 on the distortion
//   coefficients): every entry within 1e-6 of its row's norm;
//   the masked, aspect-coupled rows of pc_glob_rows: fixed slots are 0 and the fy entry is J_fy + a J_fx;
//   the loop: k_pc_lin / k_pc_try's sequence on exact data (views x corners 3 x 20 and 5 x 88, nd 5 and 8), with
//   the contributions summed in view order, started 2 % off the truth: Levenberg-Marquardt with the kernels'
//   policy reaches rms < 1e-9 px and the true fx fy cx cy to 1e-6 relative.  The lanes' summation order and
//   the tickets exist only on the GPU: tests/test_calibrate_camera.py covers those, and
//   tests/test_calibrate_camera_steps.py compares every step with an independently computed one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#define MCC_PNP_LANES 1
#define MCC_PNP_FN inline
namespace mcc {
inline void pnp_wave_sync() {}
inline double pnp_uniform(double v) { return v; }
inline int pnp_uniform(int v) { return v; }
inline double pnp_wave_sum(double v) { return v; }
}  // namespace mcc
#include "mcc_pincalib_device.hpp"

namespace {

const double kPi = 3.141592653589793;
const double kG[2][12] = {{900, 905, 655, 470, -0.25, 0.08, 1e-3, -5e-4, 0.01, 0, 0, 0},
                          {1200, 1180, 960, 540, -0.12, 0.08, 2e-4, 1e-4, 0.01, 0.002, -0.001, 0.003}};
const double kPoses[7][6] = {{0.3, -0.4, 0.2, -150, -90, 1300},  {-0.2, 0.35, -0.1, -250, -180, 900},
                             {0.05, 0.02, 1.4, 150, -200, 1800}, {0.8727, 0.05, 0.0, -200, -100, 1400},
                             {0, 0, 0, 40, -30, 1300},           {kPi - 1e-4, 0, 0, -35, 30, 1250},
                             {-0.5, -0.3, 0.6, -100, -150, 1100}};

std::vector<double> grid(int n, double relief) {
    std::vector<double> obj;
    int w = 1;
    while (w * w < n) ++w;
    for (int i = 0; i < n; ++i) {
        const int a = i % w, b = i / w;
        obj.insert(obj.end(), {40.0 * a, 40.0 * b, relief * std::sin(0.7 * b + 1.3 * a)});
    }
    return obj;
}

void residual_at(const double* g, const double* pose, const double* X, double u, double v, double* e) {
    mcc::Rot rot;
    mcc::rodrigues_v2m(pose, rot);
    mcc::pnp_residual(mcc::pc_cam(g), rot.R, pose + 3, X, u, v, e[0], e[1]);
}

int rows_check(int& cases) {
    int bad = 0;
    const std::vector<double> obj = grid(20, 60.0);
    for (const auto& g : kG)
        for (const auto& pose : kPoses) {
            const mcc::PnpCam c = mcc::pc_cam(g);
            mcc::Rot rot;
            mcc::rodrigues_v2m(pose, rot);
            double Jl[9];
            mcc::so3_jac(pose, rot, +1.0, Jl);
            for (int i = 0; i < 12; ++i) {
                const double* X = &obj[3 * i];
                const double u = 900.0 + 7.0 * i, v = 500.0 - 5.0 * i;   // the rows do not depend on the observation
                double ju[18], jv[18], eu, ev, fu[18], fv[18];
                mcc::pnp_rows(c, rot.R, Jl, pose + 3, X, u, v, ju, jv, eu, ev);
                mcc::pnp_rows_intr(c, rot.R, pose + 3, X, ju + 6, jv + 6);
                for (int k = 0; k < 18; ++k) {
                    const double h = k < 3 ? 1e-5 : k < 10 ? 1e-3 : 1e-6;
                    double e[2][2];
                    for (int sgn = 0; sgn < 2; ++sgn) {
                        double x[6], gg[12];
                        std::memcpy(x, pose, sizeof x);
                        std::memcpy(gg, g, sizeof gg);
                        (k < 6 ? x[k] : gg[k - 6]) += sgn ? h : -h;
                        residual_at(gg, x, X, u, v, e[sgn]);
                    }
                    fu[k] = -(e[1][0] - e[0][0]) / (2 * h);   // the residual is observed - projected
                    fv[k] = -(e[1][1] - e[0][1]) / (2 * h);
                }
                for (int blk = 0; blk < 2; ++blk) {
                    const int k0 = blk ? 6 : 0, k1 = blk ? 18 : 6;
                    double nu = 0, nv = 0, du = 0, dv = 0;
                    for (int k = k0; k < k1; ++k) {
                        nu += fu[k] * fu[k];
                        nv += fv[k] * fv[k];
                        du = std::fmax(du, std::fabs(ju[k] - fu[k]));
                        dv = std::fmax(dv, std::fabs(jv[k] - fv[k]));
                    }
                    ++cases;
                    if (!(du <= 1e-6 * std::sqrt(nu)) || !(dv <= 1e-6 * std::sqrt(nv))) {
                        ++bad;
                        std::printf("FAIL %s rows fx %g pose (%g %g %g) corner %d: |du| %.3e of %.3e, |dv| %.3e of %.3e\n",
                                    blk ? "intrinsic" : "pose", g[0], pose[0], pose[1], pose[2], i, du, std::sqrt(nu), dv,
                                    std::sqrt(nv));
                    }
                }
                // the solver's view of the global rows: mask 0xDF6 (fx, cy and k4 fixed), aspect 1.25
                const int mask = 0xDF6;
                double mu[12], mv[12];
                mcc::pc_glob_rows(c, rot.R, pose + 3, X, mask, 1.25, mu, mv);
                ++cases;
                for (int k = 0; k < 12; ++k) {
                    const bool fr = (mask >> k) & 1;
                    const double wu = !fr ? 0.0 : k == 1 ? ju[7] + 1.25 * ju[6] : ju[6 + k];
                    const double wv = !fr ? 0.0 : k == 1 ? jv[7] + 1.25 * jv[6] : jv[6 + k];
                    if (mu[k] != wu || mv[k] != wv) {
                        ++bad;
                        std::printf("FAIL masked rows slot %d: %g %g, expected %g %g\n", k, mu[k], mv[k], wu, wv);
                        break;
                    }
                }
            }
        }
    return bad;
}

// the trial loop of mcc_pincalib.hip, one lane, contributions summed in view order
int loop_check(int n_views, int n, const double* gt, int mask, int& cases) {
    const std::vector<double> obj1 = grid(n, 0.0);
    std::vector<double> obj, img(2 * (size_t)n_views * n), x(6 * (size_t)n_views);
    for (int v = 0; v < n_views; ++v) {
        obj.insert(obj.end(), obj1.begin(), obj1.end());
        const double* pose = kPoses[v % 4];
        double p[6];
        for (int k = 0; k < 6; ++k) p[k] = pose[k] + (v / 4) * (k < 3 ? 0.07 : 15.0);
        for (int i = 0; i < n; ++i) {
            double e[2];
            residual_at(gt, p, &obj1[3 * i], 0.0, 0.0, e);
            img[2 * ((size_t)v * n + i)] = -e[0];
            img[2 * ((size_t)v * n + i) + 1] = -e[1];
        }
        for (int k = 0; k < 6; ++k) x[6 * v + k] = p[k] * (k < 3 ? 1.01 : 0.99);
    }
    double g[12];
    for (int k = 0; k < 12; ++k) g[k] = ((mask >> k) & 1) ? gt[k] * (k < 4 ? 1.02 : 0.9) : gt[k];
    auto sumsq = [&](const double* gg, const std::vector<double>& xx) {
        double s = 0;
        for (int v = 0; v < n_views; ++v)
            s += mcc::pc_sumsq(mcc::pc_cam(gg), &xx[6 * v], &xx[6 * v + 3], &obj[3 * (size_t)v * n], &img[2 * (size_t)v * n], n, 0);
        return s;
    };
    double lambda = 1e-3, err = sumsq(g, x);
    int iter = 0, tries = 0;
    bool relin = true;
    std::vector<double> L((size_t)n_views * mcc::PcLin::N), Yz((size_t)n_views * 78), ctr(mcc::PcCtr::N), tot(mcc::PcCtr::N);
    for (int trial = 0; trial < 11 * 100 && iter < 100 && tries < 10; ++trial) {
        std::fill(tot.begin(), tot.end(), 0.0);
        for (int v = 0; v < n_views; ++v) {
            if (relin)
                mcc::pc_linearize(&obj[3 * (size_t)v * n], &img[2 * (size_t)v * n], n, mcc::pc_cam(g), mask, 0.0, &x[6 * v],
                                  &x[6 * v + 3], 0, &L[(size_t)v * mcc::PcLin::N]);
            mcc::pc_eliminate(&L[(size_t)v * mcc::PcLin::N], lambda, 0, &Yz[(size_t)v * 78], ctr.data());
            for (int e = 0; e < mcc::PcCtr::N; ++e) tot[e] += ctr[e];
        }
        double dc[12], gn[12];
        const bool ok = mcc::pc_reduced_solve(tot.data(), lambda, mask, dc);
        mcc::pc_apply(g, dc, 0.0, gn);
        std::vector<double> xn(x.size());
        for (int v = 0; v < n_views; ++v)
            mcc::pc_trial_pose(&x[6 * v], &x[6 * v + 3], &Yz[(size_t)v * 78], dc, &xn[6 * v], &xn[6 * v + 3]);
        const double en = sumsq(gn, xn);
        if (ok && en <= err) {
            std::memcpy(g, gn, sizeof g);
            x = xn;
            err = en;
            lambda = std::fmax(lambda * 0.1, 1e-12);
            ++iter;
            tries = 0;
            relin = true;
        } else {
            lambda *= 10.0;
            ++tries;
            relin = false;
        }
    }
    const double rms = std::sqrt(err / ((double)n_views * n));
    double dk = 0;
    for (int k = 0; k < 4; ++k) dk = std::fmax(dk, std::fabs(g[k] - gt[k]) / gt[k]);
    ++cases;
    if (!(rms < 1e-9) || !(dk < 1e-6)) {
        std::printf("FAIL loop %d x %d mask %x: rms %.3e, K off by %.3e after %d steps\n", n_views, n, mask, rms, dk, iter);
        return 1;
    }
    return 0;
}

}  // namespace

int main() {
    int bad = 0, cases = 0;
    bad += rows_check(cases);
    bad += loop_check(3, 20, kG[0], 0x1FF, cases);
    bad += loop_check(5, 88, kG[0], 0x1FF, cases);
    bad += loop_check(8, 88, kG[1], 0xFFF, cases);
    bad += loop_check(5, 65, kG[0], 0x03C, cases);   // the focal lengths, k3 and the tangential terms fixed
    std::printf("%d cases, %d failed\n", cases, bad);
    if (!bad) std::printf("replay ok\n");
    return bad ? 1 : 0;
}
