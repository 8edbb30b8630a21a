/*
 * mcc_omnidir.hpp -- C++ mirror of cv::omnidir::calibrate, cv::omnidir::stereoCalibrate and the
 * rectification calls undistortPoints / initUndistortRectifyMap / undistortImage / stereoRectify
 * and stereoReconstruct (all below) over the C ABI (mcc_omnidir.h).  calibrate has
 * the same name, argument order and meaning as include/opencv2/ccalib/omnidir.hpp's
 *
 *   double calibrate(InputArrayOfArrays objectPoints, InputArrayOfArrays imagePoints, Size size,
 *                    InputOutputArray K, InputOutputArray xi, InputOutputArray D,
 *                    OutputArrayOfArrays rvecs, OutputArrayOfArrays tvecs, int flags,
 *                    TermCriteria criteria, OutputArray idx = noArray());
 *
 * (src/omnidir.cpp:1067-1211) with std containers in place of cv::Mat: per-view point lists in,
 * K (3x3 row-major), xi, D (k1, k2, p1, p2), the kept views' rvecs / tvecs and their indices out,
 * the rms reprojection error returned.  The loop runs on the GPU (libmcc.so); the CV_Assert
 * checks of the reference (:1071-1079) throw std::invalid_argument, device / numerical failures
 * std::runtime_error with mcc_last_error().
 */
#ifndef MCC_OMNIDIR_HPP
#define MCC_OMNIDIR_HPP

#include <algorithm>
#include <array>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "mcc_cvmat.hpp"
#include "mcc_multicalib.hpp"
#include "mcc_omnidir.h"
#include "mcc_pnp.hpp"

namespace mcc {
namespace omnidir {

enum {
    CALIB_USE_GUESS = MCC_OMNI_CALIB_USE_GUESS,
    CALIB_FIX_SKEW = MCC_OMNI_CALIB_FIX_SKEW,
    CALIB_FIX_K1 = MCC_OMNI_CALIB_FIX_K1,
    CALIB_FIX_K2 = MCC_OMNI_CALIB_FIX_K2,
    CALIB_FIX_P1 = MCC_OMNI_CALIB_FIX_P1,
    CALIB_FIX_P2 = MCC_OMNI_CALIB_FIX_P2,
    CALIB_FIX_XI = MCC_OMNI_CALIB_FIX_XI,
    CALIB_FIX_GAMMA = MCC_OMNI_CALIB_FIX_GAMMA,
    CALIB_FIX_CENTER = MCC_OMNI_CALIB_FIX_CENTER
};

using Vec3d = std::array<double, 3>;
using Vec2d = std::array<double, 2>;
using Size = multicalib::Size;
using TermCriteria = multicalib::TermCriteria;

inline double calibrate(const std::vector<std::vector<Vec3d>>& objectPoints,
                        const std::vector<std::vector<Vec2d>>& imagePoints, Size size, std::array<double, 9>& K,
                        double& xi, std::array<double, 4>& D, std::vector<Vec3d>& rvecs, std::vector<Vec3d>& tvecs,
                        int flags, TermCriteria criteria, std::vector<int>* idx = nullptr, int device = 0) {
    if (objectPoints.empty() || imagePoints.empty() || objectPoints.size() != imagePoints.size())
        throw std::invalid_argument("omnidir::calibrate: objectPoints and imagePoints must be non-empty and of equal count");
    const int n = (int)objectPoints.size();
    std::vector<int> off(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        if (objectPoints[i].size() != imagePoints[i].size())
            throw std::invalid_argument("omnidir::calibrate: view " + std::to_string(i) + " has mismatched point counts");
        off[i + 1] = off[i] + (int)objectPoints[i].size();
    }
    std::vector<double> obj(3 * (size_t)off[n]), img(2 * (size_t)off[n]);
    for (int i = 0; i < n; ++i)
        for (size_t j = 0; j < objectPoints[i].size(); ++j) {
            for (int k = 0; k < 3; ++k) obj[3 * (off[i] + j) + k] = objectPoints[i][j][k];
            for (int k = 0; k < 2; ++k) img[2 * (off[i] + j) + k] = imagePoints[i][j][k];
        }
    std::vector<double> om(3 * (size_t)n), t(3 * (size_t)n);
    std::vector<int> kept(n);
    int nk = 0, iters = 0;
    double rms = 0;
    const int rc = mcc_omnidir_calibrate(n, off.data(), obj.data(), img.data(), size.width, size.height, flags,
                                         criteria.type, criteria.maxCount, criteria.epsilon, device, K.data(), &xi,
                                         D.data(), om.data(), t.data(), kept.data(), &nk, &rms, &iters);
    if (rc != MCC_OK) throw std::runtime_error(std::string("omnidir::calibrate: ") + mcc_last_error());
    rvecs.assign(nk, Vec3d{});
    tvecs.assign(nk, Vec3d{});
    for (int i = 0; i < nk; ++i)
        for (int k = 0; k < 3; ++k) {
            rvecs[i][k] = om[3 * i + k];
            tvecs[i][k] = t[3 * i + k];
        }
    if (idx) idx->assign(kept.begin(), kept.begin() + nk);
    return rms;
}

/*
 * cv::omnidir::stereoCalibrate (src/omnidir.cpp:1213-1381), the same name, argument order and meaning as
 *
 *   double stereoCalibrate(InputOutputArrayOfArrays objectPoints, InputOutputArrayOfArrays imagePoints1,
 *                          InputOutputArrayOfArrays imagePoints2, const Size& imageSize1, const Size& imageSize2,
 *                          InputOutputArray K1, InputOutputArray xi1, InputOutputArray D1, InputOutputArray K2,
 *                          InputOutputArray xi2, InputOutputArray D2, OutputArray rvec, OutputArray tvec,
 *                          OutputArrayOfArrays rvecsL, OutputArrayOfArrays tvecsL, int flags,
 *                          TermCriteria criteria, OutputArray idx = noArray());
 *
 * (rvec, tvec) maps the first camera's frame to the second's; rvecsL / tvecsL are the first camera's
 * poses of the kept views.  Every view needs the same number of points (std::invalid_argument
 * otherwise); CALIB_USE_GUESS is accepted and ignored, as in calibrate.
 */
inline double stereoCalibrate(const std::vector<std::vector<Vec3d>>& objectPoints,
                              const std::vector<std::vector<Vec2d>>& imagePoints1,
                              const std::vector<std::vector<Vec2d>>& imagePoints2, Size imageSize1, Size imageSize2,
                              std::array<double, 9>& K1, double& xi1, std::array<double, 4>& D1,
                              std::array<double, 9>& K2, double& xi2, std::array<double, 4>& D2, Vec3d& rvec,
                              Vec3d& tvec, std::vector<Vec3d>& rvecsL, std::vector<Vec3d>& tvecsL, int flags,
                              TermCriteria criteria, std::vector<int>* idx = nullptr, int device = 0) {
    if (objectPoints.empty() || objectPoints.size() != imagePoints1.size() || objectPoints.size() != imagePoints2.size())
        throw std::invalid_argument("omnidir::stereoCalibrate: objectPoints, imagePoints1 and imagePoints2 must be "
                                    "non-empty and of equal count");
    const int n = (int)objectPoints.size();
    const size_t np = objectPoints[0].size();
    std::vector<int> off(n + 1, 0);
    for (int i = 0; i < n; ++i) {
        if (objectPoints[i].size() != np || imagePoints1[i].size() != np || imagePoints2[i].size() != np)
            throw std::invalid_argument("omnidir::stereoCalibrate: view " + std::to_string(i) +
                                        " does not hold the point count of view 0 in all three lists");
        off[i + 1] = off[i] + (int)np;
    }
    std::vector<double> obj(3 * (size_t)off[n]), img1(2 * (size_t)off[n]), img2(2 * (size_t)off[n]);
    for (int i = 0; i < n; ++i)
        for (size_t j = 0; j < np; ++j) {
            for (int k = 0; k < 3; ++k) obj[3 * (off[i] + j) + k] = objectPoints[i][j][k];
            for (int k = 0; k < 2; ++k) {
                img1[2 * (off[i] + j) + k] = imagePoints1[i][j][k];
                img2[2 * (off[i] + j) + k] = imagePoints2[i][j][k];
            }
        }
    std::vector<double> om(3 * (size_t)n), t(3 * (size_t)n);
    std::vector<int> kept(n);
    int nk = 0, iters = 0;
    double rms = 0;
    const int rc = mcc_omnidir_stereo_calibrate(n, off.data(), obj.data(), img1.data(), img2.data(), imageSize1.width,
                                                imageSize1.height, imageSize2.width, imageSize2.height, flags,
                                                criteria.type, criteria.maxCount, criteria.epsilon, device, K1.data(),
                                                &xi1, D1.data(), K2.data(), &xi2, D2.data(), rvec.data(), tvec.data(),
                                                om.data(), t.data(), kept.data(), &nk, &rms, &iters);
    if (rc != MCC_OK) throw std::runtime_error(std::string("omnidir::stereoCalibrate: ") + mcc_last_error());
    rvecsL.assign(nk, Vec3d{});
    tvecsL.assign(nk, Vec3d{});
    for (int i = 0; i < nk; ++i)
        for (int k = 0; k < 3; ++k) {
            rvecsL[i][k] = om[3 * i + k];
            tvecsL[i][k] = t[3 * i + k];
        }
    if (idx) idx->assign(kept.begin(), kept.begin() + nk);
    return rms;
}

/*
 * cv::omnidir::undistortPoints (src/omnidir.cpp:249-343), initUndistortRectifyMap (:348-533),
 * undistortImage (:538-546) and stereoRectify (:2190-2227): the same names, argument order and
 * meaning as include/opencv2/ccalib/omnidir.hpp, with std containers and an Image view in place of
 * cv::Mat.  A rotation R is a 3 x 3 matrix (9 values) or a rotation vector (3 values, converted with
 * mcc::pnp::rodrigues of libmcc_host.so) or empty (identity); P / Knew is 3 x 3 (9 values), 3 x 4
 * (12 values, its first three columns are taken) or empty (K); D may be empty (zero) where the
 * reference allows it.  Wrong sizes throw std::invalid_argument, everything the C ABI refuses or
 * the device fails at std::runtime_error with mcc_last_error().
 */
enum {
    RECTIFY_PERSPECTIVE = MCC_OMNI_RECTIFY_PERSPECTIVE,
    RECTIFY_CYLINDRICAL = MCC_OMNI_RECTIFY_CYLINDRICAL,
    RECTIFY_LONGLATI = MCC_OMNI_RECTIFY_LONGLATI,
    RECTIFY_STEREOGRAPHIC = MCC_OMNI_RECTIFY_STEREOGRAPHIC
};
enum { MAP_32FC1 = MCC_OMNI_MAP_FLOAT, MAP_16SC2 = MCC_OMNI_MAP_FIXED };   // m1type

// an 8-bit image of 1 or 3 interleaved channels; step is the row stride in bytes (0: packed rows)
struct Image {
    unsigned char* data = nullptr;
    int width = 0, height = 0, channels = 1;
    long long step = 0;
    long long stride() const { return step ? step : (long long)width * channels; }
};

namespace detail {

// empty -> null; 9 values as they are; 3 values -> Rodrigues
inline const double* rotation(const std::vector<double>& R, std::array<double, 9>& buf, const char* who) {
    if (R.empty()) return nullptr;
    if (R.size() == 3)
        pnp::rodrigues(R.data(), buf.data());
    else if (R.size() == 9)
        std::copy(R.begin(), R.end(), buf.begin());
    else
        throw std::invalid_argument(std::string(who) + ": R must hold 9 values (3 x 3) or 3 (a rotation vector)");
    return buf.data();
}

// empty -> null; 3 x 3 as it is; 3 x 4 -> its first three columns
inline const double* projection(const std::vector<double>& P, std::array<double, 9>& buf, const char* who) {
    if (P.empty()) return nullptr;
    if (P.size() != 9 && P.size() != 12)
        throw std::invalid_argument(std::string(who) + ": P must hold 9 values (3 x 3) or 12 (3 x 4)");
    const size_t cols = P.size() / 3;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) buf[3 * r + c] = P[cols * r + c];
    return buf.data();
}

inline const double* distortion(const std::vector<double>& D, const char* who) {
    if (D.empty()) return nullptr;
    if (D.size() != 4) throw std::invalid_argument(std::string(who) + ": D must hold 4 values (k1, k2, p1, p2)");
    return D.data();
}

}  // namespace detail

inline void undistortPoints(const std::vector<Vec2d>& distorted, std::vector<Vec2d>& undistorted,
                            const std::array<double, 9>& K, const std::array<double, 4>& D, double xi,
                            const std::vector<double>& R = {}, int device = 0) {
    std::array<double, 9> Rb{};
    const double* Rp = detail::rotation(R, Rb, "omnidir::undistortPoints");
    undistorted.assign(distorted.size(), Vec2d{});
    const int rc = mcc_omnidir_undistort_points((int)distorted.size(), distorted.empty() ? nullptr : distorted[0].data(),
                                                K.data(), D.data(), xi, Rp, device,
                                                undistorted.empty() ? nullptr : undistorted[0].data());
    if (rc != MCC_OK) throw std::runtime_error(std::string("omnidir::undistortPoints: ") + mcc_last_error());
}

// m1type MAP_16SC2: map1 holds short[2 w h], map2 unsigned short[w h]; MAP_32FC1: both hold float[w h].
// The maps are returned as raw bytes of those types.
inline void initUndistortRectifyMap(const std::array<double, 9>& K, const std::vector<double>& D, double xi,
                                    const std::vector<double>& R, const std::vector<double>& P, Size size, int m1type,
                                    std::vector<unsigned char>& map1, std::vector<unsigned char>& map2, int flags,
                                    int device = 0) {
    const char* who = "omnidir::initUndistortRectifyMap";
    std::array<double, 9> Rb{}, Pb{};
    const double* Rp = detail::rotation(R, Rb, who);
    const double* Pp = detail::projection(P, Pb, who);
    const double* Dp = detail::distortion(D, who);
    if (m1type <= 0) m1type = MAP_16SC2;   // as the reference (:352)
    const size_t px = size.width > 0 && size.height > 0 ? (size_t)size.width * size.height : 0;
    map1.assign(std::max<size_t>(px * 4, 1), 0);
    map2.assign(std::max<size_t>(px * (m1type == MAP_32FC1 ? 4 : 2), 1), 0);
    const int rc = mcc_omnidir_init_undistort_rectify_map(K.data(), Dp, xi, Rp, Pp, size.width, size.height, m1type,
                                                          flags, device, map1.data(), map2.data());
    if (rc != MCC_OK) throw std::runtime_error(std::string(who) + ": " + mcc_last_error());
}

// undistorted must point at new_size (or, with an empty new_size, distorted's size) pixels of
// distorted's channel count
inline void undistortImage(const Image& distorted, const Image& undistorted, const std::array<double, 9>& K,
                           const std::vector<double>& D, double xi, int flags, const std::vector<double>& Knew = {},
                           Size new_size = Size(), const std::vector<double>& R = {}, int device = 0) {
    const char* who = "omnidir::undistortImage";
    std::array<double, 9> Rb{}, Pb{};
    const double* Rp = detail::rotation(R, Rb, who);
    const double* Pp = detail::projection(Knew, Pb, who);
    const double* Dp = detail::distortion(D, who);
    const bool keep = new_size.width <= 0 || new_size.height <= 0;   // Size::empty()
    const int w = keep ? distorted.width : new_size.width, h = keep ? distorted.height : new_size.height;
    if (undistorted.width != w || undistorted.height != h || undistorted.channels != distorted.channels)
        throw std::invalid_argument(std::string(who) + ": the destination must be " + std::to_string(w) + " x " +
                                    std::to_string(h) + " with the source's channels");
    const int rc = mcc_omnidir_undistort_image(distorted.data, distorted.width, distorted.height, distorted.channels,
                                               distorted.stride(), K.data(), Dp, xi, flags, Pp, w, h, Rp, device,
                                               undistorted.data, undistorted.stride());
    if (rc != MCC_OK) throw std::runtime_error(std::string(who) + ": " + mcc_last_error());
}

inline void stereoRectify(const std::vector<double>& R, const Vec3d& T, std::array<double, 9>& R1,
                          std::array<double, 9>& R2) {
    std::array<double, 9> Rb{};
    const double* Rp = detail::rotation(R, Rb, "omnidir::stereoRectify");
    if (!Rp) throw std::invalid_argument("omnidir::stereoRectify: R must hold 9 values (3 x 3) or 3 (a rotation vector)");
    if (mcc_omnidir_stereo_rectify(Rp, T.data(), R1.data(), R2.data()) != MCC_OK)
        throw std::runtime_error(std::string("omnidir::stereoRectify: ") + mcc_last_error());
}

/*
 * cv::omnidir::stereoReconstruct (src/omnidir.cpp:1383-1539) with the reference's argument order and
 * defaults, on the project's cv::Mat (mcc_cvmat.hpp): 8-bit images of 1 or 3 channels in, the float
 * disparity (CV_32F), both rectified images and the cloud (N x 1, CV_32FC3 for XYZ, CV_32FC(6) for
 * XYZRGB) out.  R is 3 x 3 or a rotation vector, Knew may be empty (K1), an empty newSize keeps the
 * source size and, as in the reference, gives an empty cloud.  The matcher is the project's own
 * restatement of StereoSGBM (mcc_omnidir.h).  What the reference's CV_Assert lines check
 * throws std::invalid_argument, everything the C ABI refuses std::runtime_error.
 */
enum { XYZRGB = MCC_OMNI_XYZRGB, XYZ = MCC_OMNI_XYZ };

namespace detail {

// every scalar of a CV_32F / CV_64F matrix in row-major order, as double; n of them or it throws
inline std::vector<double> scalars(const cv::Mat& m, size_t n, const char* what) {
    std::vector<double> v;
    if (m.depth() == CV_32F || m.depth() == CV_64F)
        for (int r = 0; r < m.rows; ++r)
            for (int c = 0; c < m.cols * m.channels(); ++c) v.push_back(m.scalar(r, c));
    if (v.size() != n)
        throw std::invalid_argument(std::string("omnidir::stereoReconstruct: ") + what + " must hold " + std::to_string(n) +
                                    " CV_32F / CV_64F values");
    return v;
}

inline cv::Mat& no_array() {   // the reference's noArray(): an output nobody asked for
    static thread_local cv::Mat none;
    return none;
}

}  // namespace detail

inline void stereoReconstruct(const cv::Mat& image1, const cv::Mat& image2, const cv::Mat& K1, const cv::Mat& D1, double xi1,
                              const cv::Mat& K2, const cv::Mat& D2, double xi2, const cv::Mat& R, const cv::Mat& T, int flag,
                              int numDisparities, int SADWindowSize, cv::Mat& disparity, cv::Mat& image1Rec,
                              cv::Mat& image2Rec, Size newSize = Size(), const cv::Mat& Knew = cv::Mat(),
                              cv::Mat& pointCloud = detail::no_array(), int pointType = XYZRGB, int device = 0) {
    const char* who = "omnidir::stereoReconstruct";
    const std::vector<double> k1 = detail::scalars(K1, 9, "K1"), k2 = detail::scalars(K2, 9, "K2");
    const std::vector<double> d1 = detail::scalars(D1, 4, "D1"), d2 = detail::scalars(D2, 4, "D2");
    const std::vector<double> t = detail::scalars(T, 3, "T");
    const std::vector<double> rv = detail::scalars(R, R.total() * R.channels() == 3 ? 3 : 9, "R");
    std::array<double, 9> Rb{};
    const double* Rp = detail::rotation(rv, Rb, who);
    std::vector<double> kn;
    if (!Knew.empty()) kn = detail::scalars(Knew, 9, "Knew");
    for (const cv::Mat* im : {&image1, &image2})
        if (im->empty() || im->depth() != CV_8U || (im->channels() != 1 && im->channels() != 3))
            throw std::invalid_argument(std::string(who) + ": the images must be CV_8UC1 or CV_8UC3 and not empty");
    const bool keep = newSize.width <= 0 || newSize.height <= 0;   // Size::empty()
    const int w = keep ? image1.cols : newSize.width, h = keep ? image1.rows : newSize.height;
    const bool cloud = &pointCloud != &detail::no_array() && !keep;
    disparity.create(h, w, CV_32F);
    image1Rec.create(h, w, image1.type());
    image2Rec.create(h, w, image1.type());
    const int nf = pointType == XYZ ? 3 : 6;
    std::vector<float> pts(cloud ? (size_t)w * h * nf : 0);
    long long n = 0;
    const int rc = mcc_omnidir_stereo_reconstruct(
        image1.data, image1.cols, image1.rows, image1.channels(), (long long)image1.step(), image2.data, image2.cols,
        image2.rows, image2.channels(), (long long)image2.step(), k1.data(), d1.data(), xi1, k2.data(), d2.data(), xi2, Rp,
        t.data(), flag, numDisparities, SADWindowSize, keep ? 0 : w, keep ? 0 : h, kn.empty() ? nullptr : kn.data(),
        pointType, device, disparity.ptr<float>(), image1Rec.data, (long long)image1Rec.step(), image2Rec.data,
        (long long)image2Rec.step(), pts.empty() ? nullptr : pts.data(), cloud ? (long long)w * h : 0, &n);
    if (rc != MCC_OK) throw std::runtime_error(std::string(who) + ": " + mcc_last_error());
    if (&pointCloud != &detail::no_array()) {
        pointCloud.create((int)n, 1, CV_32FC(nf));
        if (n > 0) std::memcpy(pointCloud.data, pts.data(), sizeof(float) * (size_t)n * nf);
    }
}

}  // namespace omnidir
}  // namespace mcc

#endif
