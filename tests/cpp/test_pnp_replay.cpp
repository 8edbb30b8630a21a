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
//   3 points -> status 1, points on a line -> status 2;
//   the lists of tests/test_pnp_generic.py, vetted here before a GPU sees them: exact data at nine poses
//   (theta = 0, 1e-9, 5e-3, pi, pi - 1e-7, pi - 1e-4, 3.0, 3.11, a 69 degree tilt), the target centred or
//   moved by r = (0.7, -0.5, 0.3), t = (5000, -3000, 2000), flat or with 60 mm relief, n in {20, 88} and the
//   minima, nd in {0, 4, 5, 8, 12}, max_iter in {50, 0}: the bounds above with |dt| < 1e-4 + 1e-7 |c| (c the
//   centroid: the rotation bound times the lever arm of t = th - R c), rotations compared as matrices for
//   the moved target and above theta = 3.1 (r and -r are one rotation at pi);
//   a relief sweep a in {1e-3 .. 15} mm of the 40 mm grid under 0.2 px noise (nd = 5, six poses, five draws,
//   n in {20, 88}): status 0, the host's rms in (0.1, 0.5) px and the same minimum to 1e-6.  With the
//   planarity test w0 <= 1e-9 w2 that this replaced, 33 of these 540 views came back solved with an rms of
//   0.5 to 55 px from both solvers (a from 0.01 to 3 mm), and with w0 <= 1e-3 w1 still some at a = 3 and 4 mm;
//   pnp_rows, both rows at twelve corners per (pose, nd), against central differences of pnp_residual in
//   (r, t) with steps 1e-5 and 1e-3: every entry within 1e-6 of its row's norm (truncation is h^2 of a smooth
//   function and rounding 1e-16 / h, both orders below that).
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
const unsigned long long kSweepSeed = 2025;
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

// ---- the lists of tests/test_pnp_generic.py
const double kPi = 3.141592653589793;
const std::vector<std::vector<double>> kDg = {{},
                                              {-0.1, 0.05, 1e-4, -2e-4},
                                              {-0.1, 0.05, 1e-4, -2e-4, 0.01},
                                              {-0.12, 0.08, 2e-4, 1e-4, 0.01, 0.002, -0.001, 0.003},
                                              {-0.12, 0.08, 2e-4, 1e-4, 0.01, 0.002, -0.001, 0.003, 1e-3, -5e-4, -8e-4, 3e-4}};
const double kGeneric[9][6] = {{0, 0, 0, 40, -30, 1300},
                               {1e-9, 0, 0, -60, 20, 1100},
                               {0, 5e-3, 0, 25, 45, 1500},
                               {kPi, 0, 0, -35, 30, 1250},
                               {0, kPi - 1e-7, 0, 50, -20, 1400},
                               {2.2, -2.2, 0.01, -20, -40, 1200},
                               {(kPi - 1e-4) * 0.6, (kPi - 1e-4) * 0.8, 0, 30, 25, 1350},
                               {0.1, 0.1, 3.0, -45, 35, 1150},
                               {1.2, 0.1, -0.2, 20, -25, 1450}};
const double kMoveR[3] = {0.7, -0.5, 0.3}, kMoveT[3] = {5000, -3000, 2000};
const double kSweepRelief[9] = {1e-3, 1e-2, 0.1, 0.3, 1.0, 3.0, 4.0, 10.0, 15.0};
const double kSweepPoses[6][6] = {{0.3, -0.4, 0.2, -150, -90, 1300},   {-0.2, 0.35, -0.1, -250, -180, 900},
                                  {0.05, 0.02, 1.4, 150, -200, 1800}, {0.8727, 0.05, 0.0, -200, -100, 1400},
                                  {-0.5, -0.3, 0.6, -100, -150, 1100}, {0.1, -0.7, -0.2, -50, -120, 1500}};

// n points of a near-square grid with z = relief (sin(0.7 b + 1.3 a) + 0.4 cos(0.37 i)), centred in x and y or not
std::vector<double> relief_target(int n, double relief, double pitch, bool centred) {
    std::vector<double> obj;
    int w = 1;
    while (w * w < n) ++w;
    const double cx = centred ? 0.5 * pitch * (std::min(n, w) - 1) : 0.0, cy = centred ? 0.5 * pitch * ((n - 1) / w) : 0.0;
    for (int i = 0; i < n; ++i) {
        const int a = i % w, b = i / w;
        obj.insert(obj.end(), {pitch * a - cx, pitch * b - cy, relief * (std::sin(0.7 * b + 1.3 * a) + 0.4 * std::cos(0.37 * i))});
    }
    return obj;
}

void mul3(const double* A, const double* B, bool b_transposed, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += A[i * 3 + k] * (b_transposed ? B[j * 3 + k] : B[k * 3 + j]);
            C[i * 3 + j] = s;
        }
}

// one exact-data view: obj seen at pose's pixels; with `move` the solver gets the target moved by (Ro, to) and
// must return R' = R Ro^T, t' = t - R' to.  Returns the number of failures (max_iter 50 and 0).
int exact_generic(const std::vector<double>& obj, const double* pose, size_t di, bool move, bool near_planar,
                  const char* what, int& cases) {
    const int n = (int)obj.size() / 3;
    std::vector<double> img(2 * (size_t)n), given = obj;
    mcc::pnp::projectPoints(obj.data(), n, pose, pose + 3, kK, kDg[di], img.data());
    double Rt[9], tt[3] = {pose[3], pose[4], pose[5]};
    mcc::pnp::rodrigues(pose, Rt);
    if (move) {
        double Ro[9], Rn[9];
        mcc::pnp::rodrigues(kMoveR, Ro);
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k)
                given[3 * i + k] = Ro[k * 3] * obj[3 * i] + Ro[k * 3 + 1] * obj[3 * i + 1] + Ro[k * 3 + 2] * obj[3 * i + 2] + kMoveT[k];
        mul3(Rt, Ro, true, Rn);
        for (int k = 0; k < 3; ++k) tt[k] = pose[3 + k] - (Rn[k * 3] * kMoveT[0] + Rn[k * 3 + 1] * kMoveT[1] + Rn[k * 3 + 2] * kMoveT[2]);
        std::memcpy(Rt, Rn, sizeof Rt);
    }
    double c[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) c[k] += given[3 * i + k] / n;
    const double bt = 1e-4 + 1e-7 * std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    const bool as_matrix = move || std::sqrt(pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2]) > 3.1;
    int bad = 0;
    for (int max_iter : {50, 0}) {
        double r[3], t[3], rms, R[9];
        const int st = solve(given, img, camera(kDg[di]), max_iter, r, t, rms);
        mcc::pnp::rodrigues(r, R);
        double dr = 0, dt = 0;
        for (int k = 0; k < 9; ++k)
            if (as_matrix) dr = std::fmax(dr, std::fabs(R[k] - Rt[k]));
        for (int k = 0; k < 3; ++k) {
            if (!as_matrix) dr = std::fmax(dr, std::fabs(r[k] - pose[k]));
            dt = std::fmax(dt, std::fabs(t[k] - tt[k]));
        }
        ++cases;
        // (planar to the solver only: the closed form alone is a homography fitted to points off a plane)
        const bool ok = near_planar && max_iter == 0 ? st == 0 && rms >= 0 && rms < 10.0
                                                     : st == 0 && rms >= 0 && rms < 1e-6 && dr < 1e-7 && dt < bt;
        if (!ok) {
            ++bad;
            std::printf("FAIL generic %s nd %zu n %d moved %d max_iter %d: status %d rms %.3e dr %.3e dt %.3e (%.3e)\n", what,
                        kDg[di].size(), n, (int)move, max_iter, st, rms, dr, dt, bt);
        }
    }
    return bad;
}

int generic_exact(int& cases) {
    int bad = 0;
    char what[64];
    for (size_t di = 0; di < kDg.size(); ++di) {
        for (int ip = 0; ip < 9; ++ip)
            for (int n : {20, 88})
                for (double relief : {0.0, 60.0})
                    for (int move = 0; move < 2; ++move) {
                        std::snprintf(what, sizeof what, "pose %d relief %g", ip, relief);
                        bad += exact_generic(relief_target(n, relief, 40.0, true), kGeneric[ip], di, move, false, what, cases);
                    }
        for (int ip : {0, 3}) {
            std::snprintf(what, sizeof what, "pose %d minimum", ip);
            bad += exact_generic(relief_target(4, 0.0, 160.0, true), kGeneric[ip], di, false, false, what, cases);
            bad += exact_generic(relief_target(6, 60.0, 160.0, true), kGeneric[ip], di, false, false, what, cases);
            bad += exact_generic(relief_target(4, 0.0, 160.0, true), kGeneric[ip], di, true, false, what, cases);
        }
        bad += exact_generic(relief_target(4, 0.3, 160.0, true), kGeneric[8], di, false, true, "pose 8 relief 0.3", cases);
        bad += exact_generic(relief_target(5, 0.3, 160.0, true), kGeneric[8], di, false, true, "pose 8 relief 0.3", cases);
    }
    for (size_t di : {(size_t)0, (size_t)3})   // the non-planar path past two strides of the wave
        for (int n : {129, 200, 1024})
            for (int ip : {8, 7})
                bad += exact_generic(relief_target(n, 60.0, n == 1024 ? 10.0 : 40.0, true), kGeneric[ip], di, false, false,
                                     "long", cases);
    return bad;
}

int relief_sweep(int& cases) {
    int bad = 0;
    Rng rng{kSweepSeed};
    const mcc::PnpCam c = camera(kDg[2]);
    for (double a : kSweepRelief)
        for (int n : {20, 88}) {
            const std::vector<double> obj = relief_target(n, a, 40.0, false);
            for (const auto& pose : kSweepPoses)
                for (int draw = 0; draw < 5; ++draw) {
                    std::vector<double> img(2 * (size_t)n);
                    mcc::pnp::projectPoints(obj.data(), n, pose, pose + 3, kK, kDg[2], img.data());
                    for (double& p : img) p += 0.2 * rng.normal();
                    double r[3], t[3], rms, hr[3], ht[3];
                    const int st = solve(obj, img, c, 50, r, t, rms);
                    const double hrms = mcc::pnp::solvePnP(obj.data(), img.data(), n, kK, kDg[2], hr, ht);
                    ++cases;
                    if (st != 0 || !(hrms > 0.1 && hrms < 0.5) || !(std::fabs(rms - hrms) <= 1e-6 * hrms)) {
                        ++bad;
                        std::printf("FAIL sweep a %g n %d pose (%g %g %g) draw %d: status %d rms %.17g host %.17g\n", a, n, pose[0],
                                    pose[1], pose[2], draw, st, rms, hrms);
                    }
                }
        }
    return bad;
}

// pnp_rows against central differences of pnp_residual
int rows_check(int& cases) {
    int bad = 0;
    const std::vector<double> obj = relief_target(20, 60.0, 40.0, true);
    for (size_t di : {(size_t)0, (size_t)2, (size_t)3, (size_t)4})
        for (const auto& pose : kGeneric) {
            const mcc::PnpCam c = camera(kDg[di]);
            mcc::Rot rot;
            mcc::rodrigues_v2m(pose, rot);
            double Jl[9];
            mcc::so3_jac(pose, rot, +1.0, Jl);
            for (int i = 0; i < 12; ++i) {
                const double* X = &obj[3 * i];
                const double u = 900.0 + 7.0 * i, v = 500.0 - 5.0 * i;   // the rows do not depend on the observation
                double ju[6], jv[6], eu, ev, fu[6], fv[6];
                mcc::pnp_rows(c, rot.R, Jl, pose + 3, X, u, v, ju, jv, eu, ev);
                for (int k = 0; k < 6; ++k) {
                    const double h = k < 3 ? 1e-5 : 1e-3;
                    double e[2][2];
                    for (int sgn = 0; sgn < 2; ++sgn) {
                        double x[6];
                        std::memcpy(x, pose, sizeof x);
                        x[k] += sgn ? h : -h;
                        mcc::Rot rk;
                        mcc::rodrigues_v2m(x, rk);
                        mcc::pnp_residual(c, rk.R, x + 3, X, u, v, e[sgn][0], e[sgn][1]);
                    }
                    fu[k] = -(e[1][0] - e[0][0]) / (2 * h);   // the residual is observed - projected
                    fv[k] = -(e[1][1] - e[0][1]) / (2 * h);
                }
                double nu = 0, nv = 0, du = 0, dv = 0;
                for (int k = 0; k < 6; ++k) {
                    nu += fu[k] * fu[k];
                    nv += fv[k] * fv[k];
                    du = std::fmax(du, std::fabs(ju[k] - fu[k]));
                    dv = std::fmax(dv, std::fabs(jv[k] - fv[k]));
                }
                ++cases;
                if (!(du <= 1e-6 * std::sqrt(nu)) || !(dv <= 1e-6 * std::sqrt(nv))) {
                    ++bad;
                    std::printf("FAIL rows nd %zu pose (%g %g %g) corner %d: |du| %.3e of %.3e, |dv| %.3e of %.3e\n", kDg[di].size(),
                                pose[0], pose[1], pose[2], i, du, std::sqrt(nu), dv, std::sqrt(nv));
                }
            }
        }
    return bad;
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
    bad += generic_exact(cases);
    bad += relief_sweep(cases);
    bad += rows_check(cases);
    std::printf("%d cases, %d failed\n", cases, bad);
    if (!bad) std::printf("replay ok\n");
    return bad ? 1 : 0;
}
