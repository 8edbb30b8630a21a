// test_pinrect.cpp -- the C++ mirror of the pinhole rectification (include/mcc_calib.hpp: mcc::calib::undistortPoints,
// initUndistortRectifyMap, undistort, stereoRectify), tests/test_pinhole_rectify_cpp.py.
//
//   selftest (no GPU): stereoRectify on the rig of tests/stereo_calib_cases.py's head: R1 is a rotation and
//   R2 = R1 R^T to 1e-14, R2 T lies along x to 1e-12 |T|, P2[3] = (R2 T).x f, the rois at alpha = -1 are the image;
//   wrong sizes throw std::invalid_argument, what the library refuses (alpha > 1, T = 0, a bad nd, iterations 0)
//   throws std::runtime_error with its message; no points is no device call.
//   run <dir> (GPU): stereoRectify, then both map types of camera 1 for a 97 x 61 view, 4097 points through
//   undistortPoints and a 160 x 120 x 3 frame through undistort; everything is written to <dir> as raw arrays, and
//   the Python side holds it to the bars of tests/test_pinhole_rectify.py against the numpy model.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "mcc_calib.hpp"

namespace {

using mcc::calib::Vec2d;
using mcc::calib::Vec3d;
using Mat3 = std::array<double, 9>;

const Mat3 kK1 = {900, 0, 655, 0, 905, 470, 0, 0, 1}, kK2 = {925, 0, 630, 0, 921, 488, 0, 0, 1};
const std::vector<double> kD1 = {-0.25, 0.08, 1e-3, -5e-4, 0.0}, kD2 = {-0.23, 0.07, -8e-4, 6e-4, 0.0};
const double kOm[3] = {0.02, -0.055, 0.012};
const Vec3d kT = {-120, 3, 6};

Mat3 rodrigues(const double* w) {
    const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    Mat3 R = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th < 1e-300) return R;
    const double x = w[0] / th, y = w[1] / th, z = w[2] / th, c = std::cos(th), s = std::sin(th), c1 = 1 - c;
    R = {c + c1 * x * x,     c1 * x * y - s * z, c1 * x * z + s * y, c1 * x * y + s * z, c + c1 * y * y,
         c1 * y * z - s * x, c1 * x * z - s * y, c1 * y * z + s * x, c + c1 * z * z};
    return R;
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

struct Rectified {
    Mat3 R1{}, R2{};
    std::array<double, 12> P1{}, P2{};
    std::array<double, 16> Q{};
    mcc::calib::Rect roi1, roi2;
};

Rectified rectify(double alpha, mcc::calib::Size new_size = mcc::calib::Size()) {
    Rectified r;
    mcc::calib::stereoRectify(kK1, kD1, kK2, kD2, mcc::calib::Size(1280, 960), rodrigues(kOm), kT, r.R1, r.R2, r.P1, r.P2, r.Q,
                              mcc::calib::CALIB_ZERO_DISPARITY, alpha, new_size, &r.roi1, &r.roi2);
    return r;
}

int selftest() {
    int bad = 0;
    const Mat3 R = rodrigues(kOm);
    const Rectified r = rectify(-1);
    double orth = 0, comp = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double a = 0, b = 0;
            for (int k = 0; k < 3; ++k) {
                a += r.R1[3 * i + k] * r.R1[3 * j + k];
                b += r.R1[3 * i + k] * R[3 * j + k];   // (R1 R^T)_ij
            }
            orth = std::fmax(orth, std::fabs(a - (i == j)));
            comp = std::fmax(comp, std::fabs(b - r.R2[3 * i + j]));
        }
    double t[3];
    for (int i = 0; i < 3; ++i) t[i] = r.R2[3 * i] * kT[0] + r.R2[3 * i + 1] * kT[1] + r.R2[3 * i + 2] * kT[2];
    const double nT = std::sqrt(kT[0] * kT[0] + kT[1] * kT[1] + kT[2] * kT[2]);
    std::printf("R1 R1^T - I %.2e, R2 - R1 R^T %.2e, R2 T = (%.17g, %.2e, %.2e), f %.17g\n", orth, comp, t[0], t[1], t[2], r.P1[0]);
    if (!(orth <= 1e-14 && comp <= 1e-14)) ++bad, std::printf("FAIL rotations\n");
    if (!(t[0] < 0 && std::fabs(t[1]) <= 1e-12 * nT && std::fabs(t[2]) <= 1e-12 * nT)) ++bad, std::printf("FAIL baseline\n");
    if (!(std::fabs(r.P2[3] - t[0] * r.P1[0]) <= 1e-12 * std::fabs(r.P2[3]) && r.P2[7] == 0 && r.P1[3] == 0))
        ++bad, std::printf("FAIL P2\n");
    if (!(r.roi1.x == 0 && r.roi1.y == 0 && r.roi1.width == 1280 && r.roi1.height == 960 && r.roi2.width == 1280))
        ++bad, std::printf("FAIL roi\n");
    const Rectified h = rectify(0.5, mcc::calib::Size(640, 480));
    if (!(h.roi1.width > 0 && h.roi1.width <= 640 && h.roi2.height > 0 && h.roi2.height <= 480)) ++bad, std::printf("FAIL roi at alpha 0.5\n");

    std::vector<Vec2d> src(3, Vec2d{10, 20}), dst;
    std::vector<unsigned char> m1, m2;
    if (!throws<std::invalid_argument>([&] { mcc::calib::undistortPoints(src, dst, kK1, kD1, {1, 0, 0}); }, "R must hold"))
        ++bad, std::printf("FAIL R of 3 values\n");
    if (!throws<std::invalid_argument>(
            [&] { mcc::calib::initUndistortRectifyMap(kK1, kD1, {}, {1, 2, 3, 4}, mcc::calib::Size(8, 6), 0, m1, m2); }, "P must hold"))
        ++bad, std::printf("FAIL P of 4 values\n");
    if (!throws<std::runtime_error>([&] { rectify(2.0); }, "alpha")) ++bad, std::printf("FAIL alpha 2\n");
    if (!throws<std::runtime_error>([&] { mcc::calib::undistortPoints(src, dst, kK1, {0.1, 0.2, 0.3}); }, "nd must be"))
        ++bad, std::printf("FAIL nd 3\n");
    if (!throws<std::runtime_error>([&] { mcc::calib::undistortPoints(src, dst, kK1, kD1, {}, {}, 0); }, "iterations"))
        ++bad, std::printf("FAIL iterations 0\n");
    if (!throws<std::runtime_error>([&] {
            Rectified z;
            mcc::calib::stereoRectify(kK1, kD1, kK2, kD2, mcc::calib::Size(1280, 960), R, Vec3d{0, 0, 0}, z.R1, z.R2, z.P1, z.P2, z.Q);
        }, "T is zero"))
        ++bad, std::printf("FAIL T = 0\n");
    src.clear();
    mcc::calib::undistortPoints(src, dst, kK1, kD1);   // no points: no device call
    if (!dst.empty()) ++bad, std::printf("FAIL no points\n");
    if (!bad) std::printf("selftest ok\n");
    return bad;
}

template <class T>
void dump(const std::string& dir, const char* name, const T* p, size_t n) {
    FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
    if (!f || std::fwrite(p, sizeof(T), n, f) != n) throw std::runtime_error(std::string("cannot write ") + name);
    std::fclose(f);
}

int run(const std::string& dir) {
    const int w = 97, h = 61, sw = 160, sh = 120, n = 4097;
    const Rectified r = rectify(0.0, mcc::calib::Size(w, h));
    std::vector<double> rect;
    for (const auto* a : {&r.R1, &r.R2}) rect.insert(rect.end(), a->begin(), a->end());
    for (const auto* a : {&r.P1, &r.P2}) rect.insert(rect.end(), a->begin(), a->end());
    rect.insert(rect.end(), r.Q.begin(), r.Q.end());
    dump(dir, "rect.f64", rect.data(), rect.size());
    const std::vector<double> R1(r.R1.begin(), r.R1.end()), P1(r.P1.begin(), r.P1.end());

    std::vector<unsigned char> m1, m2;
    mcc::calib::initUndistortRectifyMap(kK1, kD1, R1, P1, mcc::calib::Size(w, h), mcc::calib::MAP_32FC1, m1, m2);
    dump(dir, "float_u.f32", m1.data(), m1.size());
    dump(dir, "float_v.f32", m2.data(), m2.size());
    mcc::calib::initUndistortRectifyMap(kK1, kD1, R1, P1, mcc::calib::Size(w, h), mcc::calib::MAP_16SC2, m1, m2);
    dump(dir, "fixed_1.i16", m1.data(), m1.size());
    dump(dir, "fixed_2.u16", m2.data(), m2.size());

    std::vector<Vec2d> src(n), dst;
    for (int i = 0; i < n; ++i) src[i] = {(i * 37 % 1280) + 0.25, (i * 91 % 960) + 0.5};
    mcc::calib::undistortPoints(src, dst, kK1, kD1, R1, P1);
    dump(dir, "points_src.f64", src[0].data(), 2 * (size_t)n);
    dump(dir, "points_dst.f64", dst[0].data(), 2 * (size_t)n);

    // camera 1 at 160 x 120, a 3-channel frame, the rectified view of the maps above at that scale
    const Mat3 Ks = {900 / 8.0, 0, 655 / 8.0, 0, 905 / 8.0, 470 / 8.0, 0, 0, 1};
    const std::vector<double> Pn = {80, 0, 50, 0, 0, 80, 29, 0, 0, 0, 1, 0};
    std::vector<unsigned char> frame((size_t)sw * sh * 3), out((size_t)w * h * 3, 0);
    for (int i = 0; i < sh; ++i)
        for (int j = 0; j < sw; ++j)
            for (int c = 0; c < 3; ++c) frame[((size_t)i * sw + j) * 3 + c] = (unsigned char)((i * 7 + j * 13 + c * 29 + (i * j) % 11) & 255);
    mcc::calib::Image a{frame.data(), sw, sh, 3, 0}, b{out.data(), w, h, 3, 0};
    mcc::calib::undistort(a, b, Ks, kD1, Pn, mcc::calib::Size(w, h), R1);
    mcc::calib::initUndistortRectifyMap(Ks, kD1, R1, Pn, mcc::calib::Size(w, h), mcc::calib::MAP_16SC2, m1, m2);
    dump(dir, "image_src.u8", frame.data(), frame.size());
    dump(dir, "image_dst.u8", out.data(), out.size());
    dump(dir, "image_1.i16", m1.data(), m1.size());
    dump(dir, "image_2.u16", m2.data(), m2.size());
    std::printf("run ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "selftest";
    try {
        if (mode == "run") return argc > 2 ? run(argv[2]) : 2;
        return selftest();
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 2;
    }
}
