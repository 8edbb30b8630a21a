// The C++ mirror of cv::omnidir::stereoReconstruct (include/mcc_omnidir.hpp) on the project's cv::Mat,
// driven the way the reference's tutorial drives it.  Built and run by tests/test_omnidir_reconstruct_cpp.py:
//
//   test_omnirecon selftest        host only (no GPU): what the reference's CV_Assert lines check throws
//                                  std::invalid_argument, what the C ABI refuses std::runtime_error
//   test_omnirecon run <case.bin>  (GPU) the image pair, the flag and the point type come from the file,
//                                  with what the test's numpy model expects: the rectified images and the
//                                  disparity must be equal, the cloud's count and order too, its coordinates
//                                  within 2 float32 ulp (perspective) or 16 * 2^-24 * depth (longlati)
#include "mcc_omnidir.hpp"

#include <cmath>
#include <cstdint>
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

static cv::Mat mat64(int r, int c, std::initializer_list<double> v) {
    cv::Mat m(r, c, CV_64F);
    int k = 0;
    for (double x : v) {
        m.ptr<double>(k / c)[k % c] = x;
        ++k;
    }
    return m;
}

// the rig of tests/npsgbm.py (RIG_*): keep in step
struct Rig {
    cv::Mat K1 = mat64(3, 3, {225.0, 0.1, 80.375, 0, 224.0, 59.55, 0, 0, 1});
    cv::Mat K2 = mat64(3, 3, {226.25, -0.075, 79.25, 0, 224.75, 60.775, 0, 0, 1});
    cv::Mat D1 = mat64(1, 4, {-0.08, 0.02, 0.001, -0.0015}), D2 = mat64(1, 4, {-0.06, 0.015, -0.0008, 0.001});
    cv::Mat om = mat64(3, 1, {0.02, -0.03, 0.01}), T = mat64(3, 1, {-0.3, 0.01, 0.02});
    double xi1 = 1.6, xi2 = 1.55;
    cv::Mat knew(int flag, int w, int h) const {
        const double pi = 3.14159265358979323846;
        if (flag == om::RECTIFY_LONGLATI) return mat64(3, 3, {100.0, 0, w / 2 - 50 * pi, 0, 100.0, h / 2 - 50 * pi, 0, 0, 1});
        return mat64(3, 3, {100.0, 0, w / 2.0, 0, 100.0, h / 2.0, 0, 0, 1});
    }
};

static int selftest() {
    const Rig g;
    cv::Mat img(6, 40, CV_8UC3, 0.0), gray(6, 40, CV_8UC1, 0.0), f32(6, 40, CV_32F, 0.0), disp, r1, r2, cloud;
    auto call = [&](const cv::Mat& a, const cv::Mat& b, const cv::Mat& K, const cv::Mat& D, const cv::Mat& R, const cv::Mat& T,
                    int flag, int nd, int bs, int pt) {
        om::stereoReconstruct(a, b, K, D, g.xi1, g.K2, g.D2, g.xi2, R, T, flag, nd, bs, disp, r1, r2, om::Size(40, 6),
                              cv::Mat(), cloud, pt);
    };
    // the CV_Assert lines (:1388-1396)
    EXPECT(throws<std::invalid_argument>([&] { call(img, img, mat64(2, 3, {1, 2, 3, 4, 5, 6}), g.D1, g.om, g.T, 1, 16, 3, 1); }));
    EXPECT(throws<std::invalid_argument>([&] { call(img, img, g.K1, mat64(1, 3, {1, 2, 3}), g.om, g.T, 1, 16, 3, 1); }));
    EXPECT(throws<std::invalid_argument>([&] { call(img, img, g.K1, g.D1, mat64(1, 4, {1, 2, 3, 4}), g.T, 1, 16, 3, 1); }));
    EXPECT(throws<std::invalid_argument>([&] { call(img, img, g.K1, g.D1, g.om, mat64(1, 2, {1, 2}), 1, 16, 3, 1); }));
    EXPECT(throws<std::invalid_argument>([&] { call(f32, img, g.K1, g.D1, g.om, g.T, 1, 16, 3, 1); }));
    EXPECT(throws<std::invalid_argument>([&] { call(img, cv::Mat(), g.K1, g.D1, g.om, g.T, 1, 16, 3, 1); }));
    EXPECT(throws<std::invalid_argument>([&] { call(img, img, cv::Mat(3, 3, CV_8UC1, 1.0), g.D1, g.om, g.T, 1, 16, 3, 1); }));
    // what the C ABI refuses before any device work
    EXPECT(throws<std::runtime_error>([&] { call(img, img, g.K1, g.D1, g.om, g.T, om::RECTIFY_CYLINDRICAL, 16, 3, 1); }));
    EXPECT(throws<std::runtime_error>([&] { call(img, gray, g.K1, g.D1, g.om, g.T, 1, 16, 3, 1); }));
    EXPECT(throws<std::runtime_error>([&] { call(img, img, g.K1, g.D1, g.om, g.T, 1, 24, 3, 1); }));
    EXPECT(throws<std::runtime_error>([&] { call(img, img, g.K1, g.D1, g.om, g.T, 1, 16, 4, 1); }));
    EXPECT(throws<std::runtime_error>([&] { call(img, img, g.K1, g.D1, g.om, g.T, 1, 16, 3, 5); }));
    EXPECT(throws<std::runtime_error>([&] { call(img, img, g.K1, g.D1, g.om, mat64(3, 1, {0, 0, 0}), 1, 16, 3, 1); }));
    // the 8-bit matrices of the shim
    EXPECT(img.elemSize() == 3 && img.step() == 120 && gray.elemSize() == 1 && cv::Mat(2, 2, CV_32FC(6)).elemSize() == 24);
    cv::Mat sat(1, 3, CV_8UC1);
    sat.set(0, 0, 300.0), sat.set(0, 1, -4.0), sat.set(0, 2, 2.5);
    EXPECT(sat.data[0] == 255 && sat.data[1] == 0 && sat.data[2] == 2);
    if (!g_fail) std::printf("selftest ok\n");
    return g_fail ? 1 : 0;
}

static int32_t ordered(float f) {
    int32_t i;
    std::memcpy(&i, &f, 4);
    return i < 0 ? -(i & 0x7fffffff) : i;
}

// case.bin: int32 w, h, cn, flag, point type, n; the two images; the expected rectified images, float
// disparity [h w], cloud [n nf] and depth [n]
static int run(const char* path) {
    std::ifstream f(path, std::ios::binary);
    int32_t hd[6];
    f.read((char*)hd, sizeof(hd));
    const int w = hd[0], h = hd[1], cn = hd[2], flag = hd[3], pt = hd[4], n = hd[5], nf = pt == om::XYZ ? 3 : 6;
    const size_t ib = (size_t)w * h * cn;
    cv::Mat img[2] = {cv::Mat(h, w, CV_MAKETYPE(CV_8U, cn)), cv::Mat(h, w, CV_MAKETYPE(CV_8U, cn))};
    std::vector<unsigned char> rec[2] = {std::vector<unsigned char>(ib), std::vector<unsigned char>(ib)};
    std::vector<float> real((size_t)w * h), cloud((size_t)n * nf), depth(n);
    for (auto& m : img) f.read((char*)m.data, (std::streamsize)ib);
    for (auto& r : rec) f.read((char*)r.data(), (std::streamsize)ib);
    f.read((char*)real.data(), (std::streamsize)(real.size() * 4));
    f.read((char*)cloud.data(), (std::streamsize)(cloud.size() * 4));
    f.read((char*)depth.data(), (std::streamsize)(depth.size() * 4));
    EXPECT(f.good());
    if (g_fail) return 1;

    const Rig g;
    cv::Mat disp, r1, r2, pc;
    om::stereoReconstruct(img[0], img[1], g.K1, g.D1, g.xi1, g.K2, g.D2, g.xi2, g.om, g.T, flag, 32, 5, disp, r1, r2,
                          om::Size(w, h), g.knew(flag, w, h), pc, pt);
    EXPECT(disp.rows == h && disp.cols == w && disp.type() == CV_32F);
    EXPECT(r1.rows == h && r1.cols == w && r1.type() == img[0].type() && r2.type() == img[0].type());
    EXPECT(!std::memcmp(r1.data, rec[0].data(), ib) && !std::memcmp(r2.data, rec[1].data(), ib));
    EXPECT(!std::memcmp(disp.data, real.data(), real.size() * 4));
    EXPECT(pc.rows == n && pc.cols == 1 && pc.type() == CV_32FC(nf));
    if (g_fail) return 1;
    double worst = 0;
    for (int k = 0; k < n; ++k) {
        const float* p = pc.ptr<float>(k);
        for (int c = 0; c < 3; ++c) {
            const float want = cloud[(size_t)k * nf + c];
            const double e = flag == om::RECTIFY_PERSPECTIVE ? std::fabs((double)ordered(p[c]) - ordered(want))
                                                             : std::fabs((double)p[c] - want) / depth[k] * 16777216.0;
            worst = std::max(worst, e);
        }
        for (int c = 3; c < nf; ++c) EXPECT(p[c] == cloud[(size_t)k * nf + c]);
    }
    std::printf("%d points, worst coordinate %.2f %s\n", n, worst, flag == om::RECTIFY_PERSPECTIVE ? "ulp" : "x 2^-24 depth");
    EXPECT(worst <= (flag == om::RECTIFY_PERSPECTIVE ? 2.0 : 16.0));
    // no cloud asked for, and the reference's empty newSize
    cv::Mat d2, a2, b2;
    om::stereoReconstruct(img[0], img[1], g.K1, g.D1, g.xi1, g.K2, g.D2, g.xi2, g.om, g.T, flag, 32, 5, d2, a2, b2,
                          om::Size(), g.knew(flag, w, h));
    EXPECT(d2.rows == h && d2.cols == w && !std::memcmp(a2.data, rec[0].data(), ib));
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
    std::fprintf(stderr, "usage: test_omnirecon selftest | run <case.bin>\n");
    return 64;
}
