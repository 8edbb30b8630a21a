// The C++ mirror of the omnidir rectification calls (include/mcc_omnidir.hpp), driven the way the
// reference's tutorial drives cv::omnidir.  Built and run by tests/test_omnidir_undistort_cpp.py:
//
//   test_omnirect selftest          host only (no GPU): stereoRectify with a matrix and with a
//                                   rotation vector (R1 orthonormal, R1 T21 along +x, R2 = R1 R^T),
//                                   the reference's 0 / 0 baseline and wrong argument sizes throw
//   test_omnirect run <out.bin>     (GPU) on a camera and a frame made here from formulas:
//                                   initUndistortRectifyMap (fixed maps, 3 x 4 P, rotation vector),
//                                   undistortImage into a destination with padded rows, and
//                                   undistortPoints; everything is written to out.bin for the test
//                                   to compare with its numpy model
#include "mcc_omnidir.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

static int g_fail = 0;
#define EXPECT(c)                                                              \
    do {                                                                       \
        if (!(c)) {                                                            \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                          \
        }                                                                      \
    } while (0)

namespace om = mcc::omnidir;

template <class E, class F>
static bool throws(F f) {
    try {
        f();
    } catch (const E&) {
        return true;
    } catch (...) {
    }
    return false;
}

static int selftest() {
    const std::vector<double> rvec{0.02, -0.03, 0.01};
    const om::Vec3d T{-0.3, 0.01, 0.02};
    std::array<double, 9> R{}, R1{}, R2{}, R1m{}, R2m{};
    mcc::pnp::rodrigues(rvec.data(), R.data());
    om::stereoRectify(rvec, T, R1, R2);
    om::stereoRectify(std::vector<double>(R.begin(), R.end()), T, R1m, R2m);
    for (int k = 0; k < 9; ++k) EXPECT(R1[k] == R1m[k] && R2[k] == R2m[k]);
    double t21[3], rt[3];
    for (int c = 0; c < 3; ++c) t21[c] = -(R[c] * T[0] + R[3 + c] * T[1] + R[6 + c] * T[2]);
    for (int r = 0; r < 3; ++r) rt[r] = R1[3 * r] * t21[0] + R1[3 * r + 1] * t21[1] + R1[3 * r + 2] * t21[2];
    EXPECT(rt[0] > 0 && std::fabs(rt[1]) <= 1e-15 && std::fabs(rt[2]) <= 1e-15);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            double g = 0, p = 0;
            for (int k = 0; k < 3; ++k) {
                g += R1[3 * r + k] * R1[3 * c + k];
                p += R1[3 * r + k] * R[3 * c + k];
            }
            EXPECT(std::fabs(g - (r == c)) <= 1e-14);
            EXPECT(std::fabs(p - R2[3 * r + c]) <= 1e-15);
        }
    const std::vector<double> eye{1, 0, 0, 0, 1, 0, 0, 0, 1};
    EXPECT(throws<std::runtime_error>([&] { om::stereoRectify(eye, om::Vec3d{0, 0, 1}, R1, R2); }));
    EXPECT(throws<std::runtime_error>([&] { om::stereoRectify(eye, om::Vec3d{0, 0, 0}, R1, R2); }));
    EXPECT(throws<std::invalid_argument>([&] { om::stereoRectify({1, 2}, T, R1, R2); }));
    // argument sizes are checked before anything else; what the C ABI refuses is a runtime_error
    const std::array<double, 9> K{420, 0.5, 32, 0, 418, 24, 0, 0, 1};
    std::vector<unsigned char> m1, m2, a(8 * 6), b(8 * 6);
    EXPECT(throws<std::invalid_argument>(
        [&] { om::initUndistortRectifyMap(K, {0.1}, 1.6, {}, {}, om::Size(8, 6), om::MAP_16SC2, m1, m2, 1); }));
    EXPECT(throws<std::invalid_argument>(
        [&] { om::initUndistortRectifyMap(K, {}, 1.6, {1, 2, 3, 4}, {}, om::Size(8, 6), om::MAP_16SC2, m1, m2, 1); }));
    EXPECT(throws<std::invalid_argument>(
        [&] { om::initUndistortRectifyMap(K, {}, 1.6, {}, {1, 2, 3}, om::Size(8, 6), om::MAP_16SC2, m1, m2, 1); }));
    EXPECT(throws<std::runtime_error>(
        [&] { om::initUndistortRectifyMap(K, {}, 1.6, {}, {}, om::Size(8, 6), om::MAP_16SC2, m1, m2, 9); }));
    EXPECT(throws<std::runtime_error>(
        [&] { om::initUndistortRectifyMap(K, {}, 1.6, {}, {}, om::Size(0, 6), om::MAP_32FC1, m1, m2, 1); }));
    const om::Image src{a.data(), 8, 6, 1, 0}, small{b.data(), 7, 6, 1, 0}, dst{b.data(), 8, 6, 1, 0};
    EXPECT(throws<std::invalid_argument>([&] { om::undistortImage(src, small, K, {}, 1.6, om::RECTIFY_PERSPECTIVE); }));
    EXPECT(throws<std::runtime_error>([&] {
        om::undistortImage(src, om::Image{b.data(), 8, 6, 1, 7}, K, {}, 1.6, om::RECTIFY_PERSPECTIVE);   // stride < row
    }));
    EXPECT(throws<std::runtime_error>([&] {
        om::undistortImage(src, dst, K, {}, 1.6, om::RECTIFY_PERSPECTIVE, {1, 2, 3, 2, 4, 6, 0, 0, 1});   // singular Knew
    }));
    if (!g_fail) std::printf("selftest ok\n");
    return g_fail ? 1 : 0;
}

// the camera, rig and frame the test restates: keep in step with tests/test_omnidir_undistort_cpp.py
static int run(const char* out_path) {
    const int sw = 160, sh = 120, w = 97, h = 61, c = 3, pad = 5;
    const std::array<double, 9> K{105.2, 0.3, 80.4, 0, 104.6, 59.7, 0, 0, 1};
    const std::vector<double> D{-0.08, 0.02, 0.001, -0.0015}, rvec{0.05, -0.08, 0.03};
    const std::vector<double> P{w / 4.0, 0, w / 2.0, 7, 0, h / 4.0, h / 2.0, 8, 0, 0, 1, 9};   // 3 x 4
    const double xi = 1.6;
    std::vector<unsigned char> src((size_t)sw * sh * c);
    for (int i = 0; i < sh; ++i)
        for (int j = 0; j < sw; ++j)
            for (int k = 0; k < c; ++k) src[((size_t)i * sw + j) * c + k] = (unsigned char)((i * 7 + j * 13 + k * 29 + (i * j) % 11) & 255);
    std::vector<unsigned char> m1, m2;
    om::initUndistortRectifyMap(K, D, xi, rvec, P, om::Size(w, h), om::MAP_16SC2, m1, m2, om::RECTIFY_PERSPECTIVE);
    EXPECT(m1.size() == (size_t)w * h * 4 && m2.size() == (size_t)w * h * 2);
    const long long step = (long long)w * c + pad;
    std::vector<unsigned char> dst((size_t)step * h, 0xAB);
    om::undistortImage(om::Image{src.data(), sw, sh, c, 0}, om::Image{dst.data(), w, h, c, step}, K, D, xi,
                       om::RECTIFY_PERSPECTIVE, P, om::Size(w, h), rvec);
    std::vector<om::Vec2d> px, und;
    for (int k = 0; k < 70; ++k) px.push_back(om::Vec2d{50.0 + 0.87 * k, 80.0 - 0.58 * k});
    om::undistortPoints(px, und, K, {D[0], D[1], D[2], D[3]}, xi, rvec);
    EXPECT(und.size() == px.size());
    std::ofstream f(out_path, std::ios::binary);
    f.write((const char*)m1.data(), (std::streamsize)m1.size());
    f.write((const char*)m2.data(), (std::streamsize)m2.size());
    f.write((const char*)dst.data(), (std::streamsize)dst.size());
    f.write((const char*)und.data(), (std::streamsize)(und.size() * sizeof(om::Vec2d)));
    EXPECT(f.good());
    if (!g_fail) std::printf("run ok\n");
    return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
    try {
        if (argc >= 2 && !std::strcmp(argv[1], "selftest")) return selftest();
        if (argc >= 3 && !std::strcmp(argv[1], "run")) return run(argv[2]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    std::fprintf(stderr, "usage: test_omnirect selftest | run <out.bin>\n");
    return 64;
}
