// test_pinrecon.cpp -- the C++ mirror of the pinhole reconstruction (include/mcc_calib.hpp: mcc::calib::reprojectImageTo3D,
// stereoReconstruct, Reconstructor), tests/test_pinhole_reconstruct_cpp.py.
//
//   selftest (no GPU): wrong-size and wrong-type cv::Mats throw std::invalid_argument; what the library refuses (a
//   disparity count that is no multiple of 16, a bad point type, 14 distortion coefficients, the cameras in the wrong
//   order) throws std::runtime_error with its message; the cloud rule, run on the host through mcc_pinrecon_host_cloud,
//   gives the points of a hand-written 3 x 3 disparity in column-major order.
//   run <dir> (GPU): reads the rig (rig.f64: K1 D1 K2 D2 R T) and a 160 x 120 pair (image1.u8, image2.u8) from <dir>,
//   runs stereoReconstruct, the same pair twice through a Reconstructor and reprojectImageTo3D on the disparity it got,
//   and writes everything to <dir> as raw arrays; the Python side holds them to bit equality with the numpy model.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "mcc_calib.hpp"

namespace {

using mcc::calib::Vec3d;
using Mat3 = std::array<double, 9>;
namespace mc = mcc::calib;

// the head rig of tests/stereo_calib_cases.py at 160 x 120 (tests/pinrecon_cases.py)
const Mat3 kK1 = {112.5, 0, 81.875, 0, 113.125, 58.75, 0, 0, 1}, kK2 = {115.625, 0, 78.75, 0, 115.125, 61, 0, 0, 1};
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

struct Out {
    cv::Mat disparity, rec1, rec2, cloud, points;
};

int selftest() {
    int bad = 0;
    const Mat3 R = rodrigues(kOm);
    cv::Mat disp(6, 8, CV_32F, 3.0), out, Q = cv::Mat::eye(4, CV_64F);
    if (!throws<std::invalid_argument>([&] { mc::reprojectImageTo3D(disp, out, cv::Mat::eye(3, CV_64F)); }, "Q must be 4 x 4"))
        ++bad, std::printf("FAIL Q of 3 x 3\n");
    if (!throws<std::invalid_argument>([&] { mc::reprojectImageTo3D(cv::Mat(6, 8, CV_64F, 3.0), out, Q); }, "CV_32FC1"))
        ++bad, std::printf("FAIL a CV_64F disparity\n");
    if (!throws<std::invalid_argument>([&] { mc::reprojectImageTo3D(cv::Mat(), out, Q); }, "not empty"))
        ++bad, std::printf("FAIL an empty disparity\n");

    const cv::Mat a(120, 160, CV_8UC1, 50.0), b(120, 160, CV_8UC1, 60.0);
    Out o;
    auto recon = [&](const cv::Mat& i1, const cv::Mat& i2, const Mat3& Rr, const Vec3d& Tt, int D, const std::vector<double>& d1,
                     int pointType) {
        mc::ReconstructOptions opt;
        opt.pointType = pointType;
        mc::stereoReconstruct(i1, i2, kK1, d1, kK2, kD2, Rr, Tt, D, 5, o.disparity, o.rec1, o.rec2, o.cloud, opt);
    };
    if (!throws<std::invalid_argument>([&] { recon(a, cv::Mat(100, 160, CV_8UC1, 1.0), R, kT, 32, kD1, mc::XYZ); }, "160 x 120"))
        ++bad, std::printf("FAIL images of two sizes\n");
    if (!throws<std::invalid_argument>([&] { recon(a, cv::Mat(120, 160, CV_8UC3, 1.0), R, kT, 32, kD1, mc::XYZ); }, "1 channel"))
        ++bad, std::printf("FAIL images of two channel counts\n");
    if (!throws<std::invalid_argument>([&] { recon(cv::Mat(120, 160, CV_32F, 1.0), b, R, kT, 32, kD1, mc::XYZ); }, "CV_8UC1 or CV_8UC3"))
        ++bad, std::printf("FAIL a float image\n");
    if (!throws<std::runtime_error>([&] { recon(a, b, R, kT, 20, kD1, mc::XYZ); }, "multiple of 16")) ++bad, std::printf("FAIL D 20\n");
    if (!throws<std::runtime_error>([&] { recon(a, b, R, kT, 32, kD1, 0); }, "point_type")) ++bad, std::printf("FAIL point type 0\n");
    if (!throws<std::runtime_error>([&] { recon(a, b, R, kT, 32, std::vector<double>(14, 0.0), mc::XYZ); }, "tilted"))
        ++bad, std::printf("FAIL 14 coefficients\n");
    // the inverse rig: camera 2 to the left of camera 1
    Mat3 Ri;
    Vec3d Ti{};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Ri[3 * i + j] = R[3 * j + i];
            Ti[i] -= R[3 * j + i] * kT[j];
        }
    if (!throws<std::runtime_error>([&] { recon(a, b, Ri, Ti, 32, kD1, mc::XYZ); }, "swap the cameras")) ++bad, std::printf("FAIL camera order\n");

    // Z / W = 100 / d, X / W = 10 (x - 1) / d, Y / W = 10 (y - 1) / d; -1, 0, inf and NaN are no points
    const double q[16] = {10, 0, 0, -10, 0, 10, 0, -10, 0, 0, 0, 100, 0, 0, 1, 0};
    const float d[9] = {2, -1, 4, 0, 5, INFINITY, 1, NAN, 10};
    const float want[5][3] = {{-5, -5, 50}, {-10, 10, 100}, {0, 0, 20}, {2.5f, -2.5f, 25}, {1, 1, 10}};   // columns first
    float cloud[9 * 3];
    long long n = -1;
    if (mcc_pinrecon_host_cloud(d, 3, 3, q, nullptr, 1, MCC_XYZ, nullptr, 0.0, cloud, 9, &n) != MCC_OK || n != 5 ||
        std::memcmp(cloud, want, sizeof want) != 0)
        ++bad, std::printf("FAIL the cloud of the 3 x 3 disparity (%lld points)\n", n);
    const int roi[4] = {1, 0, 2, 2};   // x in [1, 3), y in [0, 2): (1, 1) and (2, 0); max_z drops nothing there
    if (mcc_pinrecon_host_cloud(d, 3, 3, q, nullptr, 1, MCC_XYZ, roi, 50.0, cloud, 9, &n) != MCC_OK || n != 2 ||
        std::memcmp(cloud, want[2], 2 * sizeof want[0]) != 0)
        ++bad, std::printf("FAIL the cloud inside the roi (%lld points)\n", n);
    if (mcc_pinrecon_host_cloud(d, 3, 3, q, nullptr, 1, MCC_XYZ, nullptr, 0.0, cloud, 4, &n) != MCC_EINVAL || n != 5)
        ++bad, std::printf("FAIL a capacity one short\n");
    if (!bad) std::printf("selftest ok\n");
    return bad;
}

template <class T>
void dump(const std::string& dir, const char* name, const T* p, size_t n) {
    FILE* f = std::fopen((dir + "/" + name).c_str(), "wb");
    if (!f || std::fwrite(p, sizeof(T), n, f) != n) throw std::runtime_error(std::string("cannot write ") + name);
    std::fclose(f);
}

template <class T>
void load(const std::string& dir, const char* name, T* p, size_t n) {
    FILE* f = std::fopen((dir + "/" + name).c_str(), "rb");
    if (!f || std::fread(p, sizeof(T), n, f) != n) throw std::runtime_error(std::string("cannot read ") + name);
    std::fclose(f);
}

bool same(const cv::Mat& a, const cv::Mat& b) {
    return a.rows == b.rows && a.cols == b.cols && a.type() == b.type() &&
           std::memcmp(a.data, b.data, a.total() * a.elemSize()) == 0;
}

int run(const std::string& dir) {
    const int w = 160, h = 120;
    double rig[40];
    load(dir, "rig.f64", rig, 40);
    Mat3 K1, K2, R;
    std::copy(rig, rig + 9, K1.begin());
    std::copy(rig + 14, rig + 23, K2.begin());
    std::copy(rig + 28, rig + 37, R.begin());
    const std::vector<double> D1(rig + 9, rig + 14), D2(rig + 23, rig + 28);
    const Vec3d T = {rig[37], rig[38], rig[39]};
    cv::Mat a(h, w, CV_8UC1), b(h, w, CV_8UC1);
    load(dir, "image1.u8", a.data, (size_t)w * h);
    load(dir, "image2.u8", b.data, (size_t)w * h);

    Out o;
    mc::ReconstructInfo info;
    mc::stereoReconstruct(a, b, K1, D1, K2, D2, R, T, 32, 5, o.disparity, o.rec1, o.rec2, o.cloud, mc::ReconstructOptions(),
                          &o.points, &info);
    if (info.size.width != w || info.size.height != h || info.transposed) throw std::runtime_error("unexpected output frame");
    std::vector<double> geo;
    for (const auto* m : {&info.R1, &info.R2}) geo.insert(geo.end(), m->begin(), m->end());
    for (const auto* m : {&info.P1, &info.P2}) geo.insert(geo.end(), m->begin(), m->end());
    geo.insert(geo.end(), info.Q.begin(), info.Q.end());
    dump(dir, "geometry.f64", geo.data(), geo.size());
    dump(dir, "disparity.f32", o.disparity.ptr<float>(), (size_t)w * h);
    dump(dir, "rec1.u8", o.rec1.data, (size_t)w * h);
    dump(dir, "rec2.u8", o.rec2.data, (size_t)w * h);
    dump(dir, "points.f32", o.points.ptr<float>(), (size_t)w * h * 3);
    dump(dir, "cloud.f32", o.cloud.ptr<float>(), (size_t)o.cloud.rows * 6);

    // a stream of pairs through one handle: the same bits every time, and after another pair
    mc::Reconstructor rec(K1, D1, K2, D2, mc::Size(w, h), 1, R, T, 32, 5);
    for (int k = 0; k < 3; ++k) {
        Out s;
        if (k == 1) {
            rec.compute(b, a, s.disparity, s.rec1, s.rec2, s.cloud);
            continue;
        }
        rec.compute(a, b, s.disparity, s.rec1, s.rec2, s.cloud, &s.points);
        if (!same(s.disparity, o.disparity) || !same(s.rec1, o.rec1) || !same(s.rec2, o.rec2) || !same(s.cloud, o.cloud) ||
            !same(s.points, o.points))
            throw std::runtime_error("the Reconstructor and stereoReconstruct differ");
    }
    cv::Mat again, Q(4, 4, CV_64F);
    for (int i = 0; i < 16; ++i) Q.ptr<double>(i / 4)[i % 4] = info.Q[i];
    mc::reprojectImageTo3D(o.disparity, again, Q);
    dump(dir, "reprojected.f32", again.ptr<float>(), (size_t)w * h * 3);
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
