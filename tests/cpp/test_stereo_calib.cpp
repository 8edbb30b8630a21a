// test_stereo_calib.cpp -- the C++ mirror of the pinhole stereo calibration (include/mcc_calib.hpp:
// mcc::calib::stereoCalibrate), tests/test_stereo_calibrate_cpp.py.
//
//   selftest (no GPU): mismatched point lists throw std::invalid_argument; an unsupported flag and the default
//   CALIB_FIX_INTRINSIC with an empty camera matrix throw std::runtime_error with the library's message.
//   run (GPU): six exact views of 88 corners in two cameras 120 mm apart.  With the default flags and the true
//   intrinsics the rig comes back: rms <= 1e-8 px, R within 1e-11 and T within 1e-8 mm (a rotation error d moves a
//   corner at 900 px focal length by 900 d px and a shift d at 700 mm by 900 d / 700 px, so an rms of 1e-8 px allows
//   about 1e-11 and 1e-8); the intrinsics are bitwise the input.  With CALIB_USE_INTRINSIC_GUESS from 1 % off,
//   TermCriteria(COUNT + EPS, 200, 1e-13): rms <= 1e-8 px and fx fy cx cy of both cameras within 1e-9 relative
//   (tests/cpp/test_calib.cpp's bound); E = [T]x R to rounding and F[8] = 1.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "mcc_calib.hpp"
#include "mcc_pnp.hpp"

namespace {

using mcc::calib::Vec2d;
using mcc::calib::Vec3d;
using Mat3 = std::array<double, 9>;

const double kPoses[6][6] = {{0.45, -0.1, 0.2, -90, -90, 900},   {-0.2, 0.5, -0.1, -40, -120, 800},
                             {0.05, -0.6, 1.4, 160, -100, 1000}, {0.7, 0.05, 0.0, -120, -100, 1100},
                             {-0.5, -0.3, 0.6, -40, -150, 700},  {0.3, 0.4, -0.8, -90, 50, 950}};
const double kK1[9] = {900, 0, 655, 0, 905, 470, 0, 0, 1}, kK2[9] = {925, 0, 630, 0, 921, 488, 0, 0, 1};
const std::vector<double> kD1 = {-0.25, 0.08, 1e-3, -5e-4, 0.0}, kD2 = {-0.23, 0.07, -8e-4, 6e-4, 0.0};
const double kOm[3] = {0.02, -0.055, 0.012}, kT[3] = {-120, 3, 6};

Mat3 rodrigues(const double* w) {
    const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    Mat3 R = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th < 1e-300) return R;
    const double x = w[0] / th, y = w[1] / th, z = w[2] / th, c = std::cos(th), s = std::sin(th), c1 = 1 - c;
    R = {c + c1 * x * x,     c1 * x * y - s * z, c1 * x * z + s * y, c1 * x * y + s * z, c + c1 * y * y,
         c1 * y * z - s * x, c1 * x * z - s * y, c1 * y * z + s * x, c + c1 * z * z};
    return R;
}

void views(std::vector<std::vector<Vec3d>>& obj, std::vector<std::vector<Vec2d>>& img1, std::vector<std::vector<Vec2d>>& img2) {
    std::vector<double> o;
    for (int i = 0; i < 88; ++i) o.insert(o.end(), {40.0 * (i % 11), 40.0 * (i / 11), 0.0});
    for (const auto& p : kPoses) {
        const Mat3 Rv = rodrigues(p);
        std::vector<double> px1(2 * 88), px2(2 * 88), o1(3 * 88);
        for (int i = 0; i < 88; ++i)
            for (int k = 0; k < 3; ++k)
                o1[3 * i + k] = Rv[3 * k] * o[3 * i] + Rv[3 * k + 1] * o[3 * i + 1] + Rv[3 * k + 2] * o[3 * i + 2] + p[3 + k];
        mcc::pnp::projectPoints(o.data(), 88, p, p + 3, kK1, kD1, px1.data());
        mcc::pnp::projectPoints(o1.data(), 88, kOm, kT, kK2, kD2, px2.data());   // camera 2 sees R_v X + t_v through the rig
        std::vector<Vec3d> vo(88);
        std::vector<Vec2d> v1(88), v2(88);
        for (int i = 0; i < 88; ++i) {
            vo[i] = {o[3 * i], o[3 * i + 1], o[3 * i + 2]};
            v1[i] = {px1[2 * i], px1[2 * i + 1]};
            v2[i] = {px2[2 * i], px2[2 * i + 1]};
        }
        obj.push_back(vo);
        img1.push_back(v1);
        img2.push_back(v2);
    }
}

template <class E, class F>
bool throws(F f, const char* needle) {
    try {
        f();
    } catch (const E& e) {
        return std::strstr(e.what(), needle) != nullptr;
    } catch (...) {
    }
    return false;
}

int selftest() {
    int bad = 0;
    const mcc::calib::Size size(1280, 960);
    std::vector<std::vector<Vec3d>> obj;
    std::vector<std::vector<Vec2d>> img1, img2;
    views(obj, img1, img2);
    Mat3 K1{}, K2{}, R{}, E{}, F{};
    Vec3d T{};
    std::vector<double> D1, D2;
    auto img_short = img2;
    img_short.pop_back();
    if (!throws<std::invalid_argument>(
            [&] { mcc::calib::stereoCalibrate(obj, img1, img_short, K1, D1, K2, D2, size, R, T, E, F); }, "equal count"))
        ++bad, std::printf("FAIL mismatched lists\n");
    if (!throws<std::runtime_error>(
            [&] { mcc::calib::stereoCalibrate(obj, img1, img2, K1, D1, K2, D2, size, R, T, E, F, 32768); }, "flag"))
        ++bad, std::printf("FAIL unsupported flag\n");
    if (!throws<std::runtime_error>([&] { mcc::calib::stereoCalibrate(obj, img1, img2, K1, D1, K2, D2, size, R, T, E, F); },
                                    "FIX_INTRINSIC"))
        ++bad, std::printf("FAIL the default flag with an empty camera matrix\n");
    if (!bad) std::printf("selftest ok\n");
    return bad;
}

int run() {
    using mcc::calib::TermCriteria;
    const mcc::calib::Size size(1280, 960);
    std::vector<std::vector<Vec3d>> obj;
    std::vector<std::vector<Vec2d>> img1, img2;
    views(obj, img1, img2);
    const Mat3 Rt = rodrigues(kOm);
    const TermCriteria crit(TermCriteria::COUNT + TermCriteria::EPS, 200, 1e-13);
    bool ok = true;
    {   // the default flag: intrinsics given
        Mat3 K1, K2, R{}, E{}, F{};
        std::copy(kK1, kK1 + 9, K1.begin());
        std::copy(kK2, kK2 + 9, K2.begin());
        std::vector<double> D1 = kD1, D2 = kD2;
        Vec3d T{};
        std::vector<std::array<double, 2>> pv;
        mcc::calib::StereoCalibInfo info;
        const double rms = mcc::calib::stereoCalibrate(obj, img1, img2, K1, D1, K2, D2, size, R, T, E, F,
                                                       mcc::calib::CALIB_FIX_INTRINSIC, crit, &pv, &info);
        double dR = 0, dT = 0;
        for (int k = 0; k < 9; ++k) dR = std::fmax(dR, std::fabs(R[k] - Rt[k]));
        for (int k = 0; k < 3; ++k) dT = std::fmax(dT, std::fabs(T[k] - kT[k]));
        const bool same = std::equal(kK1, kK1 + 9, K1.begin()) && std::equal(kK2, kK2 + 9, K2.begin()) && D1 == kD1 && D2 == kD2;
        std::printf("fixed rms %.3e dR %.3e dT %.3e iterations %d status %d views %zu\n", rms, dR, dT, info.iterations,
                    info.status, pv.size());
        ok = ok && rms <= 1e-8 && dR <= 1e-11 && dT <= 1e-8 && same && pv.size() == 6 && info.rvecs.size() == 6;
    }
    {   // all intrinsics free from a guess 1 % off
        Mat3 K1, K2, R{}, E{}, F{};
        for (int k = 0; k < 9; ++k) {
            K1[k] = kK1[k] * (k == 8 ? 1.0 : 1.01);
            K2[k] = kK2[k] * (k == 8 ? 1.0 : 1.01);
        }
        std::vector<double> D1 = kD1, D2 = kD2;
        for (auto* D : {&D1, &D2})
            for (double& x : *D) x *= 1.01;
        Vec3d T{};
        mcc::calib::StereoCalibInfo info;
        const double rms = mcc::calib::stereoCalibrate(obj, img1, img2, K1, D1, K2, D2, size, R, T, E, F,
                                                       mcc::calib::CALIB_USE_INTRINSIC_GUESS, crit, nullptr, &info);
        double dk = 0, dE = 0;
        for (int k : {0, 2, 4, 5}) dk = std::fmax(dk, std::fmax(std::fabs(K1[k] - kK1[k]) / kK1[k], std::fabs(K2[k] - kK2[k]) / kK2[k]));
        const double Tx[9] = {0, -T[2], T[1], T[2], 0, -T[0], -T[1], T[0], 0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                dE = std::fmax(dE, std::fabs(E[3 * i + j] - (Tx[3 * i] * R[j] + Tx[3 * i + 1] * R[3 + j] + Tx[3 * i + 2] * R[6 + j])));
        std::printf("measured rms %.3e dK %.3e dE %.3e F8 %.17g iterations %d status %d nd %zu\n", rms, dk, dE, F[8], info.iterations,
                    info.status, D1.size());
        ok = ok && rms <= 1e-8 && dk <= 1e-9 && dE <= 1e-12 && F[8] == 1.0 && D1.size() == 5 && D2.size() == 5;
    }
    if (ok) std::printf("run ok\n");
    return ok ? 0 : 1;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "selftest";
    try {
        return mode == "run" ? run() : selftest();
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
