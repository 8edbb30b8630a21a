// test_calib.cpp -- the C++ mirror of the pinhole calibration (include/mcc_calib.hpp), tests/test_calibrate_camera_cpp.py.
//
//   selftest (no GPU): initCameraMatrix2D on exact, distortion-free views with the principal point at the image
//   centre returns fx, fy to 1e-8 relative (Zhang's constraints are exact there), with OpenCV's default
//   aspectRatio = 1 it returns fx == fy; mismatched point lists throw std::invalid_argument; an unsupported flag
//   and a non-planar target without a guess throw std::runtime_error with the library's message.
//   run (GPU): calibrateCamera on six exact views of 88 corners (k1 k2 p1 p2, no k3) from the closed-form start,
//   TermCriteria(COUNT + EPS, 200, 1e-13): rms <= 1e-8 px, the issue's gate for exact data, and fx fy cx cy within
//   1e-9 relative: a relative focal error d moves a corner 300 px off the centre by 300 d px, so an rms of 1e-8 px
//   allows about 3e-11, and 1e-9 leaves a factor 30 for the corners nearer the centre.
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

const double kPoses[6][6] = {{0.45, -0.1, 0.2, -150, -90, 900},  {-0.2, 0.5, -0.1, -100, -120, 800},
                             {0.05, -0.6, 1.4, 100, -100, 1000}, {0.7, 0.05, 0.0, -180, -100, 1100},
                             {-0.5, -0.3, 0.6, -100, -150, 700}, {0.3, 0.4, -0.8, -150, 50, 950}};

void views(const double* K, const std::vector<double>& D, std::vector<std::vector<Vec3d>>& obj,
           std::vector<std::vector<Vec2d>>& img) {
    std::vector<double> o;
    for (int i = 0; i < 88; ++i) o.insert(o.end(), {40.0 * (i % 11), 40.0 * (i / 11), 0.0});
    for (const auto& p : kPoses) {
        std::vector<double> px(2 * 88);
        mcc::pnp::projectPoints(o.data(), 88, p, p + 3, K, D, px.data());
        std::vector<Vec3d> vo(88);
        std::vector<Vec2d> vi(88);
        for (int i = 0; i < 88; ++i) {
            vo[i] = {o[3 * i], o[3 * i + 1], o[3 * i + 2]};
            vi[i] = {px[2 * i], px[2 * i + 1]};
        }
        obj.push_back(vo);
        img.push_back(vi);
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
    const double K[9] = {900, 0, 639.5, 0, 905, 479.5, 0, 0, 1};
    std::vector<std::vector<Vec3d>> obj;
    std::vector<std::vector<Vec2d>> img;
    views(K, {}, obj, img);
    const auto K0 = mcc::calib::initCameraMatrix2D(obj, img, size, 0.0);
    if (!(std::fabs(K0[0] / 900 - 1) <= 1e-8) || !(std::fabs(K0[4] / 905 - 1) <= 1e-8) || K0[2] != 639.5 || K0[5] != 479.5)
        ++bad, std::printf("FAIL initCameraMatrix2D: fx %.12g fy %.12g cx %g cy %g\n", K0[0], K0[4], K0[2], K0[5]);
    const auto K1 = mcc::calib::initCameraMatrix2D(obj, img, size);
    if (K1[0] != K1[4] || !(K1[0] > 895 && K1[0] < 910)) ++bad, std::printf("FAIL aspectRatio 1: fx %g fy %g\n", K1[0], K1[4]);
    std::array<double, 9> Kc{};
    std::vector<double> D;
    std::vector<Vec3d> r, t;
    auto img_short = img;
    img_short.pop_back();
    if (!throws<std::invalid_argument>([&] { mcc::calib::calibrateCamera(obj, img_short, size, Kc, D, r, t); }, "equal count"))
        ++bad, std::printf("FAIL mismatched lists\n");
    if (!throws<std::runtime_error>([&] { mcc::calib::calibrateCamera(obj, img, size, Kc, D, r, t, 32768); }, "flag"))
        ++bad, std::printf("FAIL unsupported flag\n");
    auto relief = obj;
    relief[0][3][2] = 5.0;
    if (!throws<std::runtime_error>([&] { mcc::calib::calibrateCamera(relief, img, size, Kc, D, r, t); }, "Z != 0"))
        ++bad, std::printf("FAIL non-planar without a guess\n");
    if (!bad) std::printf("selftest ok\n");
    return bad;
}

int run() {
    const mcc::calib::Size size(1280, 960);
    const double K[9] = {900, 0, 655, 0, 905, 470, 0, 0, 1};
    const std::vector<double> Dt = {-0.25, 0.08, 1e-3, -5e-4, 0.0};
    std::vector<std::vector<Vec3d>> obj;
    std::vector<std::vector<Vec2d>> img;
    views(K, Dt, obj, img);
    std::array<double, 9> Kc{};
    std::vector<double> D;
    std::vector<Vec3d> r, t;
    mcc::calib::CalibInfo info;
    const double rms = mcc::calib::calibrateCamera(
        obj, img, size, Kc, D, r, t, 0,
        mcc::calib::TermCriteria(mcc::calib::TermCriteria::COUNT + mcc::calib::TermCriteria::EPS, 200, 1e-13), &info);
    double dk = 0, dd = 0, dr = 0, dt = 0;
    for (int k : {0, 2, 4, 5}) dk = std::fmax(dk, std::fabs(Kc[k] - K[k]) / K[k]);
    for (size_t k = 0; k < D.size(); ++k) dd = std::fmax(dd, std::fabs(D[k] - Dt[k]));
    for (size_t v = 0; v < r.size(); ++v)
        for (int k = 0; k < 3; ++k) {
            dr = std::fmax(dr, std::fabs(r[v][k] - kPoses[v][k]));
            dt = std::fmax(dt, std::fabs(t[v][k] - kPoses[v][3 + k]));
        }
    std::printf("measured rms %.3e dK %.3e dD %.3e dr %.3e dt %.3e iterations %d status %d views %zu nd %zu\n", rms, dk, dd, dr,
                dt, info.iterations, info.status, r.size(), D.size());
    const bool ok = rms <= 1e-8 && dk <= 1e-9 && r.size() == 6 && D.size() == 5 && info.viewRms.size() == 6;
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
