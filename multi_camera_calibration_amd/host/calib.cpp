// calib.cpp -- mcc::calib::calibrateCamera and initCameraMatrix2D (include/mcc_calib.hpp): cv::calibrateCamera's
// argument order over mcc_calibrate_camera / mcc_init_camera_matrix (reference call sites
// src/multicalib.cpp:254-256, samples/random_pattern_calibration.cpp:159, src/ccalib.cpp:423), stereoCalibrate over
// mcc_stereo_calibrate, and the rectification calls undistortPoints, initUndistortRectifyMap, undistort and stereoRectify
// over mcc_undistort_points, mcc_init_undistort_rectify_map, mcc_undistort_image and mcc_stereo_rectify, and the
// reconstruction calls reprojectImageTo3D, Reconstructor and stereoReconstruct over mcc_reproject_image_to_3d and
// mcc_pinrecon_*.
#include "mcc_calib.hpp"

#include <algorithm>
#include <cstring>
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

// ---------------------------------------------------------------- rectification
namespace {

const double* rotation(const std::vector<double>& R, const char* who) {
    if (R.empty()) return nullptr;
    if (R.size() != 9) throw std::invalid_argument(std::string(who) + ": R must hold 9 values (3 x 3) or none");
    return R.data();
}

// P / newCameraMatrix and its doubles per row
const double* projection(const std::vector<double>& P, int& ld, const char* who) {
    ld = P.size() == 12 ? 4 : 3;
    if (P.empty()) return nullptr;
    if (P.size() != 9 && P.size() != 12) throw std::invalid_argument(std::string(who) + ": P must hold 9 values (3 x 3), 12 (3 x 4) or none");
    return P.data();
}

}  // namespace

void undistortPoints(const std::vector<Vec2d>& src, std::vector<Vec2d>& dst, const std::array<double, 9>& cameraMatrix,
                     const std::vector<double>& distCoeffs, const std::vector<double>& R, const std::vector<double>& P,
                     int iterations, int device) {
    const char* who = "undistortPoints";
    int ld = 3;
    const double* Rp = rotation(R, who);
    const double* Pp = projection(P, ld, who);
    dst.assign(src.size(), Vec2d{});
    const int rc = mcc_undistort_points((int)src.size(), src.empty() ? nullptr : src[0].data(), cameraMatrix.data(),
                                        distCoeffs.empty() ? nullptr : distCoeffs.data(), (int)distCoeffs.size(), Rp, Pp, ld,
                                        iterations, device, dst.empty() ? nullptr : dst[0].data(), nullptr);
    if (rc != MCC_OK) throw std::runtime_error(std::string(who) + ": " + mcc_last_error());
}

void initUndistortRectifyMap(const std::array<double, 9>& cameraMatrix, const std::vector<double>& distCoeffs,
                             const std::vector<double>& R, const std::vector<double>& newCameraMatrix, Size size, int m1type,
                             std::vector<unsigned char>& map1, std::vector<unsigned char>& map2, int device) {
    const char* who = "initUndistortRectifyMap";
    int ld = 3;
    const double* Rp = rotation(R, who);
    const double* Pp = projection(newCameraMatrix, ld, who);
    if (m1type <= 0) m1type = MAP_16SC2;   // as cv::initUndistortRectifyMap
    const size_t px = size.width > 0 && size.height > 0 ? (size_t)size.width * size.height : 0;
    map1.assign(std::max<size_t>(px * 4, 1), 0);
    map2.assign(std::max<size_t>(px * (m1type == MAP_32FC1 ? 4 : 2), 1), 0);
    const int rc = mcc_init_undistort_rectify_map(cameraMatrix.data(), distCoeffs.empty() ? nullptr : distCoeffs.data(),
                                                  (int)distCoeffs.size(), Rp, Pp, ld, size.width, size.height, m1type, device,
                                                  map1.data(), map2.data(), nullptr);
    if (rc != MCC_OK) throw std::runtime_error(std::string(who) + ": " + mcc_last_error());
}

void undistort(const Image& src, const Image& dst, const std::array<double, 9>& cameraMatrix,
               const std::vector<double>& distCoeffs, const std::vector<double>& newCameraMatrix, Size newSize,
               const std::vector<double>& R, int device) {
    const char* who = "undistort";
    int ld = 3;
    const double* Rp = rotation(R, who);
    const double* Pp = projection(newCameraMatrix, ld, who);
    const bool keep = newSize.width <= 0 || newSize.height <= 0;   // Size::empty()
    const int w = keep ? src.width : newSize.width, h = keep ? src.height : newSize.height;
    if (dst.width != w || dst.height != h || dst.channels != src.channels)
        throw std::invalid_argument(std::string(who) + ": dst must be the new size (or src's) with src's channels");
    const int rc = mcc_undistort_image(src.data, src.width, src.height, src.channels, src.stride(), cameraMatrix.data(),
                                       distCoeffs.empty() ? nullptr : distCoeffs.data(), (int)distCoeffs.size(), Rp, Pp, ld, w,
                                       h, device, dst.data, dst.stride());
    if (rc != MCC_OK) throw std::runtime_error(std::string(who) + ": " + mcc_last_error());
}

void stereoRectify(const std::array<double, 9>& cameraMatrix1, const std::vector<double>& distCoeffs1,
                   const std::array<double, 9>& cameraMatrix2, const std::vector<double>& distCoeffs2, Size imageSize,
                   const std::array<double, 9>& R, const Vec3d& T, std::array<double, 9>& R1, std::array<double, 9>& R2,
                   std::array<double, 12>& P1, std::array<double, 12>& P2, std::array<double, 16>& Q, int flags, double alpha,
                   Size newImageSize, Rect* validPixROI1, Rect* validPixROI2) {
    // one nd for both cameras: the shorter vector is padded with zeros
    const size_t nd = std::max(distCoeffs1.size(), distCoeffs2.size());
    std::vector<double> d1(distCoeffs1), d2(distCoeffs2);
    d1.resize(nd, 0.0);
    d2.resize(nd, 0.0);
    int roi[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    const int rc = mcc_stereo_rectify(cameraMatrix1.data(), nd ? d1.data() : nullptr, cameraMatrix2.data(),
                                      nd ? d2.data() : nullptr, (int)nd, imageSize.width, imageSize.height, R.data(), T.data(),
                                      flags, alpha, newImageSize.width, newImageSize.height, R1.data(), R2.data(), P1.data(),
                                      P2.data(), Q.data(), roi[0], roi[1]);
    if (rc != MCC_OK) throw std::runtime_error(std::string("stereoRectify: ") + mcc_last_error());
    Rect* out[2] = {validPixROI1, validPixROI2};
    for (int k = 0; k < 2; ++k)
        if (out[k]) *out[k] = Rect{roi[k][0], roi[k][1], roi[k][2], roi[k][3]};
}

// ---------------------------------------------------------------- reconstruction
void reprojectImageTo3D(const cv::Mat& disparity, cv::Mat& _3dImage, const cv::Mat& Q, bool handleMissingValues, int device) {
    const char* who = "reprojectImageTo3D";
    if (disparity.empty() || disparity.type() != CV_32FC1)
        throw std::invalid_argument(std::string(who) + ": disparity must be CV_32FC1 and not empty");
    if (Q.rows != 4 || Q.cols != 4 || Q.channels() != 1 || (Q.depth() != CV_32F && Q.depth() != CV_64F))
        throw std::invalid_argument(std::string(who) + ": Q must be 4 x 4, CV_32F or CV_64F");
    double q[16];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) q[4 * r + c] = Q.scalar(r, c);
    _3dImage.create(disparity.rows, disparity.cols, CV_32FC3);
    const int rc = mcc_reproject_image_to_3d(disparity.data, MCC_DISP_FLOAT, disparity.cols, disparity.rows,
                                             (long long)disparity.step(), q, handleMissingValues ? 1 : 0, device,
                                             _3dImage.ptr<float>(), nullptr);
    if (rc != MCC_OK) throw std::runtime_error(std::string(who) + ": " + mcc_last_error());
}

namespace {

ReconstructInfo info_of(const mcc_pinrecon_geometry& g) {
    ReconstructInfo i;
    std::copy(g.R1, g.R1 + 9, i.R1.begin());
    std::copy(g.R2, g.R2 + 9, i.R2.begin());
    std::copy(g.P1, g.P1 + 12, i.P1.begin());
    std::copy(g.P2, g.P2 + 12, i.P2.begin());
    std::copy(g.Q, g.Q + 16, i.Q.begin());
    i.roi1 = Rect{g.roi1[0], g.roi1[1], g.roi1[2], g.roi1[3]};
    i.roi2 = Rect{g.roi2[0], g.roi2[1], g.roi2[2], g.roi2[3]};
    i.size = Size(g.width, g.height);
    i.transposed = g.transposed != 0;
    return i;
}

void check_image(const cv::Mat& im, Size size, int channels, const char* who) {
    if (im.empty() || im.depth() != CV_8U || im.channels() != channels || im.cols != size.width || im.rows != size.height)
        throw std::invalid_argument(std::string(who) + ": the images must be CV_8U of " + std::to_string(size.width) + " x " +
                                    std::to_string(size.height) + " with " + std::to_string(channels) + " channel(s)");
}

}  // namespace

Reconstructor::Reconstructor(const std::array<double, 9>& cameraMatrix1, const std::vector<double>& distCoeffs1,
                             const std::array<double, 9>& cameraMatrix2, const std::vector<double>& distCoeffs2, Size imageSize,
                             int channels, const std::array<double, 9>& R, const Vec3d& T, int numDisparities,
                             int SADWindowSize, const ReconstructOptions& o)
    : src_(imageSize), channels_(channels), point_floats_(o.pointType == XYZ ? 3 : 6) {
    // one nd for both cameras: the shorter vector is padded with zeros
    const size_t nd = std::max(distCoeffs1.size(), distCoeffs2.size());
    std::vector<double> d1(distCoeffs1), d2(distCoeffs2);
    d1.resize(nd, 0.0);
    d2.resize(nd, 0.0);
    const mcc_pinrecon_desc d{cameraMatrix1.data(), nd ? d1.data() : nullptr, cameraMatrix2.data(), nd ? d2.data() : nullptr,
                              (int)nd, R.data(), T.data(), imageSize.width, imageSize.height, channels, o.flags, o.alpha,
                              o.newImageSize.width, o.newImageSize.height, numDisparities, SADWindowSize, o.pointType,
                              o.useRoi ? 1 : 0, o.maxZ, o.device};
    if (mcc_pinrecon_create(&h_, &d) != MCC_OK) throw std::runtime_error(std::string("Reconstructor: ") + mcc_last_error());
    mcc_pinrecon_geometry g;
    mcc_pinrecon_info(h_, &g);
    info_ = info_of(g);
}

Reconstructor::~Reconstructor() { mcc_pinrecon_destroy(h_); }

void Reconstructor::compute(const cv::Mat& image1, const cv::Mat& image2, cv::Mat& disparity, cv::Mat& image1Rec,
                            cv::Mat& image2Rec, cv::Mat& pointCloud, cv::Mat* points3d) {
    const char* who = "Reconstructor::compute";
    check_image(image1, src_, channels_, who);
    check_image(image2, src_, channels_, who);
    const int w = info_.size.width, h = info_.size.height;
    disparity.create(h, w, CV_32F);
    image1Rec.create(h, w, image1.type());
    image2Rec.create(h, w, image1.type());
    if (points3d) points3d->create(h, w, CV_32FC3);
    std::vector<float> pts((size_t)w * h * point_floats_);
    long long n = 0;
    const int rc = mcc_pinrecon_compute(h_, image1.data, (long long)image1.step(), image2.data, (long long)image2.step(),
                                        disparity.ptr<float>(), nullptr, image1Rec.data, (long long)image1Rec.step(),
                                        image2Rec.data, (long long)image2Rec.step(), points3d ? points3d->ptr<float>() : nullptr,
                                        pts.data(), (long long)w * h, &n);
    if (rc != MCC_OK) throw std::runtime_error(std::string(who) + ": " + mcc_last_error());
    pointCloud.create((int)n, 1, CV_32FC(point_floats_));
    if (n > 0) std::memcpy(pointCloud.data, pts.data(), sizeof(float) * (size_t)n * point_floats_);
}

double Reconstructor::time(int frames) {
    double ms = 0;
    if (mcc_pinrecon_time(h_, frames, &ms) != MCC_OK) throw std::runtime_error(std::string("Reconstructor::time: ") + mcc_last_error());
    return ms;
}

void stereoReconstruct(const cv::Mat& image1, const cv::Mat& image2, const std::array<double, 9>& cameraMatrix1,
                       const std::vector<double>& distCoeffs1, const std::array<double, 9>& cameraMatrix2,
                       const std::vector<double>& distCoeffs2, const std::array<double, 9>& R, const Vec3d& T,
                       int numDisparities, int SADWindowSize, cv::Mat& disparity, cv::Mat& image1Rec, cv::Mat& image2Rec,
                       cv::Mat& pointCloud, const ReconstructOptions& options, cv::Mat* points3d, ReconstructInfo* info) {
    const char* who = "stereoReconstruct";
    if (image1.empty() || image1.depth() != CV_8U || (image1.channels() != 1 && image1.channels() != 3))
        throw std::invalid_argument(std::string(who) + ": the images must be CV_8UC1 or CV_8UC3 and not empty");
    const Size size(image1.cols, image1.rows);
    check_image(image2, size, image1.channels(), who);
    Reconstructor rec(cameraMatrix1, distCoeffs1, cameraMatrix2, distCoeffs2, size, image1.channels(), R, T, numDisparities,
                      SADWindowSize, options);
    if (info) *info = rec.info();
    rec.compute(image1, image2, disparity, image1Rec, image2Rec, pointCloud, points3d);
}

}  // namespace calib
}  // namespace mcc
