/*
 * mcc_calib.hpp -- cv::calibrateCamera and cv::initCameraMatrix2D for one pinhole camera, over
 * mcc_calibrate_camera / mcc_init_camera_matrix (include/mcc.h, libmcc.so); implemented in libmcc_host.so
 * (host/calib.cpp).  Argument order and return value follow
 *
 *   double calibrateCamera(InputArrayOfArrays objectPoints, InputArrayOfArrays imagePoints, Size imageSize,
 *                          InputOutputArray cameraMatrix, InputOutputArray distCoeffs, OutputArrayOfArrays rvecs,
 *                          OutputArrayOfArrays tvecs, int flags = 0,
 *                          TermCriteria criteria = TermCriteria(COUNT + EPS, 30, DBL_EPSILON));
 *   Mat initCameraMatrix2D(InputArrayOfArrays objectPoints, InputArrayOfArrays imagePoints, Size imageSize,
 *                          double aspectRatio = 1.0);
 *
 * The result is the least-squares minimum of the reprojection error through cv::projectPoints' model, found by
 * Levenberg-Marquardt on the GPU; bit parity with OpenCV is not claimed.  distCoeffs has 8 entries
 * with CALIB_RATIONAL_MODEL and 5 otherwise (a vector handed in with another size is resized; its leading entries
 * are the guess under CALIB_USE_INTRINSIC_GUESS).  Thin-prism and tilted-sensor flags throw.
 *
 * cv::stereoCalibrate for a pinhole pair is further down, over mcc_stereo_calibrate, and after it
 * the rectification of what the two return: undistortPoints, initUndistortRectifyMap, undistort, stereoRectify
 * (DESIGN.md 7i), and the reconstruction from a rectified pair: reprojectImageTo3D, stereoReconstruct and the
 * Reconstructor for streams of pairs.
 */
#ifndef MCC_CALIB_HPP
#define MCC_CALIB_HPP

#include <array>
#include <cfloat>
#include <vector>

#include "mcc.h"
#include "mcc_cvmat.hpp"
#include "mcc_multicalib.hpp"

namespace mcc {
namespace calib {

enum {
    CALIB_USE_INTRINSIC_GUESS = MCC_CALIB_USE_INTRINSIC_GUESS,
    CALIB_FIX_ASPECT_RATIO = MCC_CALIB_FIX_ASPECT_RATIO,
    CALIB_FIX_PRINCIPAL_POINT = MCC_CALIB_FIX_PRINCIPAL_POINT,
    CALIB_ZERO_TANGENT_DIST = MCC_CALIB_ZERO_TANGENT_DIST,
    CALIB_FIX_FOCAL_LENGTH = MCC_CALIB_FIX_FOCAL_LENGTH,
    CALIB_FIX_K1 = MCC_CALIB_FIX_K1,
    CALIB_FIX_K2 = MCC_CALIB_FIX_K2,
    CALIB_FIX_K3 = MCC_CALIB_FIX_K3,
    CALIB_FIX_K4 = MCC_CALIB_FIX_K4,
    CALIB_FIX_K5 = MCC_CALIB_FIX_K5,
    CALIB_FIX_K6 = MCC_CALIB_FIX_K6,
    CALIB_RATIONAL_MODEL = MCC_CALIB_RATIONAL_MODEL
};

using Vec3d = std::array<double, 3>;
using Vec2d = std::array<double, 2>;
using Size = multicalib::Size;
using TermCriteria = multicalib::TermCriteria;

// what cv::calibrateCamera does not return: the loop's end (MCC_CALIB_*), accepted steps, per-view RMS, device time
struct CalibInfo {
    int status = 0, iterations = 0, trials = 0;
    std::vector<double> viewRms;
    double deviceMs = 0;
};

// Throws std::invalid_argument for mismatched point lists and std::runtime_error with the library's message
// when the call fails (a bad argument, a view without a pose seed, no GPU).
double calibrateCamera(const std::vector<std::vector<Vec3d>>& objectPoints,
                       const std::vector<std::vector<Vec2d>>& imagePoints, Size imageSize,
                       std::array<double, 9>& cameraMatrix, std::vector<double>& distCoeffs, std::vector<Vec3d>& rvecs,
                       std::vector<Vec3d>& tvecs, int flags = 0,
                       TermCriteria criteria = TermCriteria(TermCriteria::COUNT + TermCriteria::EPS, 30, DBL_EPSILON),
                       CalibInfo* info = nullptr, int device = 0);

// aspectRatio = 0 leaves fx and fy free; OpenCV's default of 1 forces fx = fy.  Host only.
std::array<double, 9> initCameraMatrix2D(const std::vector<std::vector<Vec3d>>& objectPoints,
                                         const std::vector<std::vector<Vec2d>>& imagePoints, Size imageSize,
                                         double aspectRatio = 1.0);

// cv::stereoCalibrate's own flags
enum {
    CALIB_FIX_INTRINSIC = MCC_CALIB_FIX_INTRINSIC,
    CALIB_SAME_FOCAL_LENGTH = MCC_CALIB_SAME_FOCAL_LENGTH,
    CALIB_USE_EXTRINSIC_GUESS = MCC_CALIB_USE_EXTRINSIC_GUESS
};

// what cv::stereoCalibrate does not return: as CalibInfo, and camera 1's pose of every view
struct StereoCalibInfo {
    int status = 0, iterations = 0, trials = 0;
    std::vector<Vec3d> rvecs, tvecs;
    double deviceMs = 0;
};

/*
 *   double stereoCalibrate(InputArrayOfArrays objectPoints, InputArrayOfArrays imagePoints1,
 *                          InputArrayOfArrays imagePoints2, InputOutputArray cameraMatrix1, InputOutputArray distCoeffs1,
 *                          InputOutputArray cameraMatrix2, InputOutputArray distCoeffs2, Size imageSize,
 *                          InputOutputArray R, InputOutputArray T, OutputArray E, OutputArray F, int flags = CALIB_FIX_INTRINSIC,
 *                          TermCriteria criteria = TermCriteria(COUNT + EPS, 30, 1e-6));
 *
 * over mcc_stereo_calibrate: camera 2 sees a view at R R_v, R t_v + T.  perViewErrors (may be null) gets each view's
 * RMS in camera 1 and camera 2, as OpenCV's overload with perViewErrors does.  The result is the least-squares
 * minimum of both cameras' reprojection error under the flags; bit parity with OpenCV is not claimed.
 * Throws as calibrateCamera does.
 */
double stereoCalibrate(const std::vector<std::vector<Vec3d>>& objectPoints,
                       const std::vector<std::vector<Vec2d>>& imagePoints1,
                       const std::vector<std::vector<Vec2d>>& imagePoints2, std::array<double, 9>& cameraMatrix1,
                       std::vector<double>& distCoeffs1, std::array<double, 9>& cameraMatrix2,
                       std::vector<double>& distCoeffs2, Size imageSize, std::array<double, 9>& R, Vec3d& T,
                       std::array<double, 9>& E, std::array<double, 9>& F, int flags = CALIB_FIX_INTRINSIC,
                       TermCriteria criteria = TermCriteria(TermCriteria::COUNT + TermCriteria::EPS, 30, 1e-6),
                       std::vector<std::array<double, 2>>* perViewErrors = nullptr, StereoCalibInfo* info = nullptr,
                       int device = 0);

/*
 * Rectification over mcc_undistort_points, mcc_init_undistort_rectify_map, mcc_undistort_image and
 * mcc_stereo_rectify, with cv::'s names and argument order:
 *
 *   void undistortPoints(InputArray src, OutputArray dst, InputArray cameraMatrix, InputArray distCoeffs,
 *                        InputArray R = noArray(), InputArray P = noArray());
 *   void initUndistortRectifyMap(InputArray cameraMatrix, InputArray distCoeffs, InputArray R, InputArray newCameraMatrix,
 *                                Size size, int m1type, OutputArray map1, OutputArray map2);
 *   void undistort(InputArray src, OutputArray dst, InputArray cameraMatrix, InputArray distCoeffs,
 *                  InputArray newCameraMatrix = noArray());
 *   void stereoRectify(InputArray cameraMatrix1, InputArray distCoeffs1, InputArray cameraMatrix2, InputArray distCoeffs2,
 *                      Size imageSize, InputArray R, InputArray T, OutputArray R1, OutputArray R2, OutputArray P1,
 *                      OutputArray P2, OutputArray Q, int flags = CALIB_ZERO_DISPARITY, double alpha = -1,
 *                      Size newImageSize = Size(), Rect* validPixROI1 = 0, Rect* validPixROI2 = 0);
 *
 * distCoeffs holds 0, 4, 5, 8 or 12 values; R is 3 x 3 (9 values) or empty (identity); P / newCameraMatrix is 3 x 3
 * (9 values), 3 x 4 (12 values, its first three columns are read) or empty (the identity for points, cameraMatrix for
 * maps).  Wrong sizes throw std::invalid_argument; whatever the C ABI refuses or the device fails at throws
 * std::runtime_error with the library's message.  Where 7i and OpenCV differ (20 rounds of the distortion's inverse
 * where OpenCV runs 5), 7i holds.
 */
enum { CALIB_ZERO_DISPARITY = MCC_CALIB_ZERO_DISPARITY };
enum { MAP_32FC1 = MCC_MAP_FLOAT, MAP_16SC2 = MCC_MAP_FIXED };   // m1type

struct Rect {
    int x = 0, y = 0, width = 0, height = 0;
};

// an 8-bit image of 1 or 3 interleaved channels; step is the row stride in bytes (0: packed rows)
struct Image {
    unsigned char* data = nullptr;
    int width = 0, height = 0, channels = 1;
    long long step = 0;
    long long stride() const { return step ? step : (long long)width * channels; }
};

void undistortPoints(const std::vector<Vec2d>& src, std::vector<Vec2d>& dst, const std::array<double, 9>& cameraMatrix,
                     const std::vector<double>& distCoeffs, const std::vector<double>& R = {},
                     const std::vector<double>& P = {}, int iterations = 20, int device = 0);

// m1type MAP_16SC2: map1 holds short[2 w h], map2 unsigned short[w h]; MAP_32FC1: both hold float[w h].
// The maps are returned as raw bytes of those types.
void initUndistortRectifyMap(const std::array<double, 9>& cameraMatrix, const std::vector<double>& distCoeffs,
                             const std::vector<double>& R, const std::vector<double>& newCameraMatrix, Size size,
                             int m1type, std::vector<unsigned char>& map1, std::vector<unsigned char>& map2,
                             int device = 0);

// dst must point at newSize (or, with an empty newSize, src's size) pixels of src's channel count.  With R and
// newCameraMatrix = P1 / P2 this is the remap of one rectified view.
void undistort(const Image& src, const Image& dst, const std::array<double, 9>& cameraMatrix,
               const std::vector<double>& distCoeffs, const std::vector<double>& newCameraMatrix = {},
               Size newSize = Size(), const std::vector<double>& R = {}, int device = 0);

// host only
void stereoRectify(const std::array<double, 9>& cameraMatrix1, const std::vector<double>& distCoeffs1,
                   const std::array<double, 9>& cameraMatrix2, const std::vector<double>& distCoeffs2, Size imageSize,
                   const std::array<double, 9>& R, const Vec3d& T, std::array<double, 9>& R1, std::array<double, 9>& R2,
                   std::array<double, 12>& P1, std::array<double, 12>& P2, std::array<double, 16>& Q,
                   int flags = CALIB_ZERO_DISPARITY, double alpha = -1, Size newImageSize = Size(),
                   Rect* validPixROI1 = nullptr, Rect* validPixROI2 = nullptr);

/*
 * Reconstruction over mcc_reproject_image_to_3d and mcc_pinrecon_*, on the project's cv::Mat
 * (mcc_cvmat.hpp):
 *
 *   void reprojectImageTo3D(InputArray disparity, OutputArray _3dImage, InputArray Q, bool handleMissingValues = false);
 *
 * disparity is CV_32F (the project's cv::Mat has no 16-bit type; the C ABI and Python take the matcher's fixed-point
 * disparity too), Q is 4 x 4 CV_32F or CV_64F, _3dImage comes back CV_32FC3.  stereoReconstruct is the pinhole
 * counterpart of mcc::omnidir::stereoReconstruct: 8-bit images of 1 or 3 channels in; the float disparity (CV_32F),
 * both rectified images, the dense points (CV_32FC3, optional) and the cloud (N x 1, CV_32FC3 for XYZ, CV_32FC(6) for
 * XYZRGB) out.  Camera 2 must lie to the right of camera 1 after rectification, or below it: such a vertical pair
 * comes out in the transposed frame (ReconstructInfo::transposed, 7j).  Wrong sizes and types throw
 * std::invalid_argument, whatever the C ABI refuses std::runtime_error with the library's message.
 */
enum { XYZRGB = MCC_XYZRGB, XYZ = MCC_XYZ };

void reprojectImageTo3D(const cv::Mat& disparity, cv::Mat& _3dImage, const cv::Mat& Q, bool handleMissingValues = false,
                        int device = 0);

// what the pair is rectified with, in the frame of the outputs (mcc_pinrecon_geometry)
struct ReconstructInfo {
    std::array<double, 9> R1{}, R2{};
    std::array<double, 12> P1{}, P2{};
    std::array<double, 16> Q{};
    Rect roi1, roi2;
    Size size;
    bool transposed = false;
};

struct ReconstructOptions {
    int flags = CALIB_ZERO_DISPARITY;   // stereoRectify's
    double alpha = -1;
    Size newImageSize = Size();         // empty: the source size
    int pointType = XYZRGB;
    bool useRoi = false;                // cloud only inside roi1
    double maxZ = 0;                    // <= 0: no limit
    int device = 0;
};

// A stream of pairs: stereoRectify's result, both cameras' maps and every buffer stay on the device (mcc_pinrecon).
class Reconstructor {
public:
    Reconstructor(const std::array<double, 9>& cameraMatrix1, const std::vector<double>& distCoeffs1,
                  const std::array<double, 9>& cameraMatrix2, const std::vector<double>& distCoeffs2, Size imageSize,
                  int channels, const std::array<double, 9>& R, const Vec3d& T, int numDisparities, int SADWindowSize,
                  const ReconstructOptions& options = ReconstructOptions());
    ~Reconstructor();
    Reconstructor(const Reconstructor&) = delete;
    Reconstructor& operator=(const Reconstructor&) = delete;

    // points3d (may be null) gets the dense CV_32FC3 points
    void compute(const cv::Mat& image1, const cv::Mat& image2, cv::Mat& disparity, cv::Mat& image1Rec, cv::Mat& image2Rec,
                 cv::Mat& pointCloud, cv::Mat* points3d = nullptr);
    double time(int frames);   // device milliseconds per pair, no transfers
    const ReconstructInfo& info() const { return info_; }

private:
    mcc_pinrecon* h_ = nullptr;
    ReconstructInfo info_;
    Size src_;
    int channels_ = 1, point_floats_ = 6;
};

// one Reconstructor used once
void stereoReconstruct(const cv::Mat& image1, const cv::Mat& image2, const std::array<double, 9>& cameraMatrix1,
                       const std::vector<double>& distCoeffs1, const std::array<double, 9>& cameraMatrix2,
                       const std::vector<double>& distCoeffs2, const std::array<double, 9>& R, const Vec3d& T,
                       int numDisparities, int SADWindowSize, cv::Mat& disparity, cv::Mat& image1Rec, cv::Mat& image2Rec,
                       cv::Mat& pointCloud, const ReconstructOptions& options = ReconstructOptions(),
                       cv::Mat* points3d = nullptr, ReconstructInfo* info = nullptr);

}  // namespace calib
}  // namespace mcc

#endif
