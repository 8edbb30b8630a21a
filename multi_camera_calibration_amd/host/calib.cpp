// calib.cpp -- mcc::calib::calibrateCamera and initCameraMatrix2D (include/mcc_calib.hpp): cv::calibrateCamera's
// argument order over mcc_calibrate_camera / mcc_init_camera_matrix (reference call sites
// src/multicalib.cpp:254-256, samples/random_pattern_calibration.cpp:159, src/ccalib.cpp:423).
#include "mcc_calib.hpp"

#include <stdexcept>
#include <string>

namespace mcc {
namespace calib {

namespace {

struct Flat {
    std::vector<int> off;
    std::vector<double> obj, img;
};

Flat flatten(const char* who, const std::vector<std::vector<Vec3d>>& objectPoints,
             const std::vector<std::vector<Vec2d>>& imagePoints) {
    if (objectPoints.empty() || objectPoints.size() != imagePoints.size())
        throw std::invalid_argument(std::string(who) + ": objectPoints and imagePoints must be non-empty and of equal count");
    Flat f;
    f.off.assign(objectPoints.size() + 1, 0);
    for (size_t i = 0; i < objectPoints.size(); ++i) {
        if (objectPoints[i].size() != imagePoints[i].size())
            throw std::invalid_argument(std::string(who) + ": view " + std::to_string(i) + " has mismatched point counts");
        f.off[i + 1] = f.off[i] + (int)objectPoints[i].size();
        for (size_t j = 0; j < objectPoints[i].size(); ++j) {
            f.obj.insert(f.obj.end(), objectPoints[i][j].begin(), objectPoints[i][j].end());
            f.img.insert(f.img.end(), imagePoints[i][j].begin(), imagePoints[i][j].end());
        }
    }
    return f;
}

mcc_calib_desc describe(const Flat& f, Size size) {
    mcc_calib_desc d{};
    d.n_views = (int)f.off.size() - 1;
    d.view_off = f.off.data();
    d.obj = f.obj.data();
    d.img = f.img.data();
    d.image_width = size.width;
    d.image_height = size.height;
    d.nd = 5;
    d.crit_type = MCC_CRIT_COUNT_EPS;
    d.max_count = 30;
    return d;
}

}  // namespace

double calibrateCamera(const std::vector<std::vector<Vec3d>>& objectPoints,
                       const std::vector<std::vector<Vec2d>>& imagePoints, Size imageSize,
                       std::array<double, 9>& cameraMatrix, std::vector<double>& distCoeffs, std::vector<Vec3d>& rvecs,
                       std::vector<Vec3d>& tvecs, int flags, TermCriteria criteria, CalibInfo* info, int device) {
    const Flat f = flatten("calibrateCamera", objectPoints, imagePoints);
    mcc_calib_desc d = describe(f, imageSize);
    d.flags = flags;
    d.nd = (flags & CALIB_RATIONAL_MODEL) ? 8 : 5;
    d.crit_type = criteria.type;
    d.max_count = criteria.maxCount;
    d.eps = criteria.epsilon;
    d.device = device;
    distCoeffs.resize((size_t)d.nd, 0.0);
    const size_t n = (size_t)d.n_views;
    std::vector<double> r(3 * n), t(3 * n), vr(n);
    double rms = 0, ms = 0;
    int iters = 0, status = 0, trials = 0;
    d.trials = &trials;
    const int rc = mcc_calibrate_camera(&d, cameraMatrix.data(), distCoeffs.data(), r.data(), t.data(), vr.data(), &rms,
                                        &iters, &status, &ms);
    if (rc != MCC_OK) throw std::runtime_error(std::string("calibrateCamera: ") + mcc_last_error());
    rvecs.assign(n, Vec3d{});
    tvecs.assign(n, Vec3d{});
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            rvecs[i][k] = r[3 * i + k];
            tvecs[i][k] = t[3 * i + k];
        }
    if (info) {
        info->status = status;
        info->iterations = iters;
        info->trials = trials;
        info->viewRms = vr;
        info->deviceMs = ms;
    }
    return rms;
}

std::array<double, 9> initCameraMatrix2D(const std::vector<std::vector<Vec3d>>& objectPoints,
                                         const std::vector<std::vector<Vec2d>>& imagePoints, Size imageSize,
                                         double aspectRatio) {
    const Flat f = flatten("initCameraMatrix2D", objectPoints, imagePoints);
    const mcc_calib_desc d = describe(f, imageSize);
    std::array<double, 9> K{};
    if (mcc_init_camera_matrix(&d, aspectRatio, K.data()) != MCC_OK)
        throw std::runtime_error(std::string("initCameraMatrix2D: ") + mcc_last_error());
    return K;
}

double stereoCalibrate(const std::vector<std::vector<Vec3d>>& objectPoints,
                       const std::vector<std::vector<Vec2d>>& imagePoints1,
                       const std::vector<std::vector<Vec2d>>& imagePoints2, std::array<double, 9>& cameraMatrix1,
                       std::vector<double>& distCoeffs1, std::array<double, 9>& cameraMatrix2,
                       std::vector<double>& distCoeffs2, Size imageSize, std::array<double, 9>& R, Vec3d& T,
                       std::array<double, 9>& E, std::array<double, 9>& F, int flags, TermCriteria criteria,
                       std::vector<std::array<double, 2>>* perViewErrors, StereoCalibInfo* info, int device) {
    const Flat f1 = flatten("stereoCalibrate", objectPoints, imagePoints1);
    const Flat f2 = flatten("stereoCalibrate", objectPoints, imagePoints2);
    mcc_stereo_calib_desc d{};
    d.n_views = (int)f1.off.size() - 1;
    d.view_off = f1.off.data();
    d.obj = f1.obj.data();
    d.img1 = f1.img.data();
    d.img2 = f2.img.data();
    d.image_width = imageSize.width;
    d.image_height = imageSize.height;
    d.flags = flags;
    d.nd = (flags & CALIB_RATIONAL_MODEL) ? 8 : 5;
    d.crit_type = criteria.type;
    d.max_count = criteria.maxCount;
    d.eps = criteria.epsilon;
    d.device = device;
    distCoeffs1.resize((size_t)d.nd, 0.0);
    distCoeffs2.resize((size_t)d.nd, 0.0);
    const size_t n = (size_t)d.n_views;
    std::vector<double> r(3 * n), t(3 * n), vr(2 * n);
    double rms = 0, ms = 0;
    int iters = 0, status = 0, trials = 0;
    d.trials = &trials;
    const int rc = mcc_stereo_calibrate(&d, cameraMatrix1.data(), distCoeffs1.data(), cameraMatrix2.data(), distCoeffs2.data(),
                                        R.data(), T.data(), E.data(), F.data(), r.data(), t.data(), vr.data(), &rms, &iters,
                                        &status, &ms);
    if (rc != MCC_OK) throw std::runtime_error(std::string("stereoCalibrate: ") + mcc_last_error());
    if (perViewErrors) {
        perViewErrors->assign(n, {0.0, 0.0});
        for (size_t i = 0; i < n; ++i) (*perViewErrors)[i] = {vr[2 * i], vr[2 * i + 1]};
    }
    if (info) {
        info->status = status;
        info->iterations = iters;
        info->trials = trials;
        info->deviceMs = ms;
        info->rvecs.assign(n, Vec3d{});
        info->tvecs.assign(n, Vec3d{});
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) {
                info->rvecs[i][k] = r[3 * i + k];
                info->tvecs[i][k] = t[3 * i + k];
            }
    }
    return rms;
}

}  // namespace calib
}  // namespace mcc
