/*
 * mcc_omnidir.h -- C ABI of the MI355X per-camera intrinsic calibration of the Mei omnidirectional
 * model (libmcc.so): cv::omnidir::calibrate, SURVEY.md 8(f) row 4, and of the joint calibration of
 * a two-camera rig, cv::omnidir::stereoCalibrate (second half of this header).
 *
 * The reference calls it once per camera from MultiCameraCalibration::loadImages
 * (src/multicalib.cpp:273-278, TermCriteria(COUNT + EPS, 300, 1e-7)) before the extrinsic
 * bundle adjustment of mcc.h, and the omnidir tutorial calls it directly
 * (tutorials/omnidir_tutorial.markdown:45-49).  Entry points and the reference code each replaces:
 *
 *   mcc_omnidir_calibrate ....... cv::omnidir::calibrate (include/opencv2/ccalib/omnidir.hpp,
 *                                 src/omnidir.cpp:1067-1211): initialise, then the loop, then the
 *                                 rms of estimateUncertainties.
 *   mcc_omnidir_initialize ...... cv::omnidir::internal::initializeCalibration
 *                                 (src/omnidir.cpp:551-748); host code, no GPU.
 *   mcc_omnicalib_create ........ the per-view point lists calibrate converts to CV_64F
 *                                 (src/omnidir.cpp:1083-1094), deep-copied to the device.
 *   mcc_omnicalib_jacobian ...... cv::omnidir::internal::computeJacobian (src/omnidir.cpp:851-935)
 *                                 and one G of the loop (src/omnidir.cpp:1134-1142).
 *   mcc_omnicalib_optimize ...... the loop of calibrate (src/omnidir.cpp:1126-1149), on the device.
 *   mcc_omnicalib_rms ........... estimateUncertainties' rms (src/omnidir.cpp:1791-1803).
 *   mcc_omnidir_stereo_calibrate  cv::omnidir::stereoCalibrate (src/omnidir.cpp:1213-1381).
 *   mcc_omnidir_stereo_initialize cv::omnidir::internal::initializeStereoCalibration (:750-846).
 *   mcc_omnidir_stereo_encode_init  its host part: getInterset (:2229-2268), the relative poses
 *                                 (:786-797), findMedian3 (:2172-2188), encodeParametersStereo
 *                                 (:1570-1619); no GPU.
 *   mcc_omnistereo_create ....... the per-view point lists stereoCalibrate converts to CV_64F
 *                                 (:1227-1238), deep-copied to the device.
 *   mcc_omnistereo_jacobian ..... cv::omnidir::internal::computeJacobianStereo (:937-1020) with
 *                                 compose_motion (:1023-1065), flags2idxStereo / fillFixedStereo
 *                                 (:2078-2170), and one G of the loop (:1280-1290).
 *   mcc_omnistereo_optimize ..... the loop of stereoCalibrate (:1274-1301), on the device.
 *   mcc_omnistereo_rms .......... estimateUncertaintiesStereo's rms (:1826-1888).
 *   mcc_omnidir_undistort_points  cv::omnidir::undistortPoints (:249-343), on the device.
 *   mcc_omnidir_init_undistort_rectify_map  cv::omnidir::initUndistortRectifyMap (:348-533), on the
 *                                 device, all four RECTIFY_* flags, float or fixed-point maps.
 *   mcc_omnidir_remap ........... the cv::remap call of undistortImage (:545): INTER_LINEAR,
 *                                 BORDER_CONSTANT, fixed-point maps, 8-bit images.
 *   mcc_omnidir_undistort_image . cv::omnidir::undistortImage (:538-546).
 *   mcc_omnidir_stereo_rectify .. cv::omnidir::stereoRectify (:2190-2227); host code, no GPU.
 *   mcc_omnirect_create ......... the maps of undistortImage (:543-544), built once and kept on the
 *                                 device for a stream of frames.
 *   mcc_omnirect_remap .......... its remap (:545) of one frame.
 *   mcc_omnidir_stereo_reconstruct  cv::omnidir::stereoReconstruct (:1383-1539): rectify both images,
 *                                 match them, the float disparity and the point cloud.
 *   mcc_omnidir_sgbm ............ the StereoSGBM::create(...)->compute call in it (:1437-1439), restated.
 *   mcc_omnirecon_create ........ its maps and every buffer, kept on the device for a stream of pairs.
 *   mcc_omnirecon_compute ....... one frame pair through them.
 *
 * Parameters use the reference's encodeParameters layout (src/omnidir.cpp:1541-1568), CV_64F:
 *   x = [om_0(3), T_0(3), ..., om_{n-1}, T_{n-1}, fx, fy, s, cx, cy, xi, k1, k2, p1, p2], P = 6n + 10.
 * The reference's JTJ + epsilon adds epsilon to EVERY entry of the (flag-reduced) dense normal
 * matrix; the device solves it exactly as a block-arrow Schur system plus a Sherman-Morrison
 * correction for the rank-one epsilon * 1 1^T term -- never a dense P x P matrix.
 *
 * Conventions as mcc.h: 0 = OK, negative MCC_E* on error, message in mcc_last_error().
 */
#ifndef MCC_OMNIDIR_H
#define MCC_OMNIDIR_H

#include "mcc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cv::omnidir flags (include/opencv2/ccalib/omnidir.hpp:56-66) */
#define MCC_OMNI_CALIB_USE_GUESS 1
#define MCC_OMNI_CALIB_FIX_SKEW 2
#define MCC_OMNI_CALIB_FIX_K1 4
#define MCC_OMNI_CALIB_FIX_K2 8
#define MCC_OMNI_CALIB_FIX_P1 16
#define MCC_OMNI_CALIB_FIX_P2 32
#define MCC_OMNI_CALIB_FIX_XI 64
#define MCC_OMNI_CALIB_FIX_GAMMA 128
#define MCC_OMNI_CALIB_FIX_CENTER 256

typedef struct mcc_omnicalib mcc_omnicalib;

typedef struct mcc_omnicalib_desc {
    int n_views;
    const int *view_off;   /* [n_views + 1] corner ranges                        */
    const double *obj;     /* [3 * corners] pattern points (x, y, z)             */
    const double *img;     /* [2 * corners] image points (u, v)                  */
    int flags;             /* MCC_OMNI_CALIB_FIX_* (flags2idx semantics)         */
    int device;            /* HIP device ordinal                                 */
} mcc_omnicalib_desc;

int mcc_omnicalib_create(mcc_omnicalib **out, const mcc_omnicalib_desc *desc);
void mcc_omnicalib_destroy(mcc_omnicalib *h);
int mcc_omnicalib_nparams(const mcc_omnicalib *h);

/* computeJacobian at params (P) for loop iteration iter: jte[P] = J^T E before the flag
 * reduction, G[P] = alpha_smooth2 (JTJ + epsilon)^-1 JTE with fixed entries 0 (fillFixed).
 * Either output may be NULL. */
int mcc_omnicalib_jacobian(mcc_omnicalib *h, const double *params, int iter, double *jte, double *G);

/* calibrate's loop from params_inout (P): crit_type MCC_CRIT_COUNT / EPS / COUNT_EPS. */
int mcc_omnicalib_optimize(mcc_omnicalib *h, int crit_type, int max_count, double eps, double *params_inout,
                           int *iters, double *last_change);

/* rms reprojection error at params (estimateUncertainties) */
int mcc_omnicalib_rms(mcc_omnicalib *h, const double *params, double *rms);

/* measurement: n_steps unconditional loop steps (no stop test; iterations 0..n_steps-1 of the
 * alpha / epsilon schedules) from params, graph-launched; ms_per_step = device time per step
 * (one kernel launch) from two HIP events on the handle's stream.  params are not modified. */
int mcc_omnicalib_time_steps(mcc_omnicalib *h, const double *params, int n_steps, double *ms_per_step);

/* initializeCalibration (host): om / t [3 * n_views] of the kept views in idx order, K[9]
 * (row-major), xi, idx[n_views] kept view indices, n_idx. */
int mcc_omnidir_initialize(int n_views, const int *view_off, const double *obj, const double *img, int width,
                           int height, double *om, double *t, double *K, double *xi, int *idx, int *n_idx);

/* cv::omnidir::calibrate: K[9], xi, D[4], om / t [3 * n_views] (kept views), idx, n_idx, rms,
 * iterations (may be NULL). */
int mcc_omnidir_calibrate(int n_views, const int *view_off, const double *obj, const double *img, int width,
                          int height, int flags, int crit_type, int max_count, double eps, int device, double *K,
                          double *xi, double *D, double *om, double *t, int *idx, int *n_idx, double *rms,
                          int *iters);

/* ---------------------------------------------------------------- cv::omnidir::stereoCalibrate
 * Two Mei cameras that see the same pattern views.  Parameters use the reference's
 * encodeParametersStereo layout, CV_64F, P = 6 (n + 1) + 20:
 *   x = [om(3), T(3), omL_0, tL_0, ..., omL_{n-1}, tL_{n-1}, intr_1(10), intr_2(10)],
 *   intr = fx, fy, s, cx, cy, xi, k1, k2, p1, p2.
 * (om, T) maps the left-camera frame to the right-camera frame: the right camera's pose of view i
 * is compose_motion(omL_i, tL_i, om, T), R2 = R(om) R(omL_i), T2 = R(om) tL_i + T.
 *
 * Every view must hold the same number of points (computeJacobianStereo takes n_points from view
 * 0, src/omnidir.cpp:947), at least 3 and at most 2048; anything else is MCC_EINVAL before any
 * device work.  The step kernel walks a view's corners in chunks of 64 or 128 and keeps the Gram in
 * the matrix-core accumulators, so LDS does not bound the corner count; 2048 is an argument check.
 *
 * MCC_OMNI_CALIB_USE_GUESS is handled as the single-camera path handles it: the bit is accepted
 * and ignored.  flags2idxStereo does not look at it, the initialisation always runs, and K / xi /
 * D are outputs only.  The FIX_* flags apply to both cameras' intrinsics; (om, T) and the kept
 * poses are never fixed.  A view whose 6 x 6 pose block is not positive definite fails with
 * MCC_ENOTPD (the reference propagates NaN).  estimateUncertaintiesStereo's `errors` are not
 * computed. */
typedef struct mcc_omnistereo mcc_omnistereo;

typedef struct mcc_omnistereo_desc {
    int n_views;
    const int *view_off;   /* [n_views + 1] corner ranges, all of the same length */
    const double *obj;     /* [3 * corners] pattern points (x, y, z)             */
    const double *img1;    /* [2 * corners] image points of camera 1 (left)      */
    const double *img2;    /* [2 * corners] image points of camera 2 (right)     */
    int flags;             /* MCC_OMNI_CALIB_FIX_* (flags2idxStereo semantics)   */
    int device;            /* HIP device ordinal                                 */
} mcc_omnistereo_desc;

int mcc_omnistereo_create(mcc_omnistereo **out, const mcc_omnistereo_desc *desc);
void mcc_omnistereo_destroy(mcc_omnistereo *h);
int mcc_omnistereo_nparams(const mcc_omnistereo *h);

/* computeJacobianStereo at params (P) for loop iteration iter: jte[P] = J^T E before the flag
 * reduction, G[P] = alpha_smooth2 (JTJ + epsilon)^-1 JTE with fixed entries 0 (fillFixedStereo).
 * Either output may be NULL. */
int mcc_omnistereo_jacobian(mcc_omnistereo *h, const double *params, int iter, double *jte, double *G);

/* stereoCalibrate's loop from params_inout (P): crit_type MCC_CRIT_COUNT / EPS / COUNT_EPS. */
int mcc_omnistereo_optimize(mcc_omnistereo *h, int crit_type, int max_count, double eps, double *params_inout,
                            int *iters, double *last_change);

/* rms reprojection error over both cameras' points at params (estimateUncertaintiesStereo) */
int mcc_omnistereo_rms(mcc_omnistereo *h, const double *params, double *rms);

/* measurement, as mcc_omnicalib_time_steps: n_steps unconditional loop steps, graph-launched. */
int mcc_omnistereo_time_steps(mcc_omnistereo *h, const double *params, int n_steps, double *ms_per_step);

/* The host part of initializeStereoCalibration after its two calibrate calls (no GPU): the
 * intersection of the two kept lists idx1[n1] / idx2[n2] in the first list's order (getInterset),
 * per common view the relative pose R2 R1^T, T2 - R2 R1^T T1 of the two cameras' poses
 * (om1 / t1 [3 * n1], om2 / t2 [3 * n2], in kept order), the reference's median of each component
 * (findMedian: an even count gives the upper-middle element, an odd count the mean of the middle
 * element and the one below it), and encodeParametersStereo with the first camera's poses.
 * params must hold 6 (min(n1, n2) + 1) + 20 doubles, idx min(n1, n2) ints. */
int mcc_omnidir_stereo_encode_init(int n1, const int *idx1, const double *om1, const double *t1, int n2,
                                   const int *idx2, const double *om2, const double *t2, const double *K1, double xi1,
                                   const double *D1, const double *K2, double xi2, const double *D2, double *params,
                                   int *idx, int *n_idx);

/* initializeStereoCalibration: two mcc_omnidir_calibrate runs with TermCriteria(3, 100, 1e-6) and
 * the caller's flags (on the GPU), then mcc_omnidir_stereo_encode_init.  params must hold
 * 6 (n_views + 1) + 20 doubles (6 (n_idx + 1) + 20 are written), idx n_views ints. */
int mcc_omnidir_stereo_initialize(int n_views, const int *view_off, const double *obj, const double *img1,
                                  const double *img2, int width1, int height1, int width2, int height2, int flags,
                                  int device, double *params, int *idx, int *n_idx);

/* cv::omnidir::stereoCalibrate: K1 / K2 [9], xi1 / xi2, D1 / D2 [4], om[3], T[3], omL / tL
 * [3 * n_views] (kept views), idx, n_idx, rms, iterations (may be NULL). */
int mcc_omnidir_stereo_calibrate(int n_views, const int *view_off, const double *obj, const double *img1,
                                 const double *img2, int width1, int height1, int width2, int height2, int flags,
                                 int crit_type, int max_count, double eps, int device, double *K1, double *xi1,
                                 double *D1, double *K2, double *xi2, double *D2, double *om, double *T, double *omL,
                                 double *tL, int *idx, int *n_idx, double *rms, int *iters);

/* ---------------------------------------------------------------- rectification of points and images
 * cv::omnidir::undistortPoints (:249-343), initUndistortRectifyMap (:348-533), undistortImage
 * (:538-546) and stereoRectify (:2190-2227).  K, R, P, Knew are 3 x 3 row-major (of a 3 x 4 P pass
 * the first three columns), D = (k1, k2, p1, p2); NULL stands for the reference's empty array:
 * R = identity, D = 0, P / Knew = K.  Images are 8-bit, 1 or 3 interleaved channels, with a row
 * stride in bytes; bytes of a destination row past width * channels are never written.
 *
 * A fixed-point map pair is OpenCV's CV_16SC2 + CV_16UC1: with iu = cvRound(32 u), iv = cvRound(32 v)
 * map1 = ((short)(iu >> 5), (short)(iv >> 5)) -- the cast wraps -- and map2 = (iv & 31) * 32 + (iu & 31);
 * 32 u outside the int range (or NaN) is unspecified, as in the reference.  The remap is cv::remap
 * with INTER_LINEAR and BORDER_CONSTANT 0 on such maps: fx = map2 & 31, fy = (map2 >> 5) & 31, the
 * tap weights (32 - fx)(32 - fy) 32, fx (32 - fy) 32, (32 - fx) fy 32, fx fy 32, a tap outside the
 * source reads 0, dst = (sum + 16384) >> 15.
 *
 * Bad arguments (a null required pointer, n < 0, a size that is not positive or above 32767, channels
 * other than 1 or 3, a stride shorter than a row, an unknown flag or map type, a singular P R, P or
 * R) are MCC_EINVAL before any device work. */

/* cv::omnidir::RECTIFY_* (include/opencv2/ccalib/omnidir.hpp:68-73) */
#define MCC_OMNI_RECTIFY_PERSPECTIVE 1
#define MCC_OMNI_RECTIFY_CYLINDRICAL 2
#define MCC_OMNI_RECTIFY_LONGLATI 3
#define MCC_OMNI_RECTIFY_STEREOGRAPHIC 4

#define MCC_OMNI_MAP_FLOAT 1   /* CV_32FC1: map1 = (float)u, map2 = (float)v            */
#define MCC_OMNI_MAP_FIXED 2   /* CV_16SC2 + CV_16UC1, see above                         */

/* undistortPoints: n pixels (u, v) -> X/Z, Y/Z of their rays after R; n == 0 touches nothing. */
int mcc_omnidir_undistort_points(int n, const double *distorted, const double *K, const double *D, double xi,
                                 const double *R, int device, double *undistorted);

/* stereoRectify (host, no GPU): R1 with rows e1 = T21 / |T21|, e2 = (-T21.y, T21.x, 0) / |.|,
 * e3 = e1 x e2 / |.| for T21 = -R^T T, and R2 = R1 R^T.  T = 0, or T21 along z (the reference's
 * 0 / 0), is MCC_EINVAL. */
int mcc_omnidir_stereo_rectify(const double *R, const double *T, double *R1, double *R2);

/* initUndistortRectifyMap: MCC_OMNI_MAP_FLOAT writes two float[width * height],
 * MCC_OMNI_MAP_FIXED short[2 * width * height] and unsigned short[width * height]. */
int mcc_omnidir_init_undistort_rectify_map(const double *K, const double *D, double xi, const double *R,
                                           const double *P, int width, int height, int map_type, int flags,
                                           int device, void *map1, void *map2);

/* the remap of undistortImage with host fixed-point maps (short[2 * dst_w * dst_h],
 * unsigned short[dst_w * dst_h]) */
int mcc_omnidir_remap(const unsigned char *src, int src_w, int src_h, int channels, long long src_stride,
                      const short *map1, const unsigned short *map2, int dst_w, int dst_h,
                      unsigned char *dst, long long dst_stride, int device);

/* undistortImage in one call; the maps never leave the device.  new_w == 0 takes the source
 * size. */
int mcc_omnidir_undistort_image(const unsigned char *src, int src_w, int src_h, int channels, long long src_stride,
                                const double *K, const double *D, double xi, int flags, const double *Knew,
                                int new_w, int new_h, const double *R, int device, unsigned char *dst,
                                long long dst_stride);

/* The per-frame case: the fixed-point maps are built once at create and stay on the device with
 * the source and destination images; every remap call is one upload, one kernel, one download. */
typedef struct mcc_omnirect mcc_omnirect;

typedef struct mcc_omnirect_desc {
    const double *K;       /* [9]                                                 */
    const double *D;       /* [4] or NULL                                         */
    double xi;
    const double *R;       /* [9] or NULL                                         */
    const double *P;       /* [9] or NULL (Knew of undistortImage)                */
    int flags;             /* MCC_OMNI_RECTIFY_*                                  */
    int dst_width, dst_height;
    int src_width, src_height;
    int channels;          /* 1 or 3                                              */
    int device;            /* HIP device ordinal                                  */
} mcc_omnirect_desc;

int mcc_omnirect_create(mcc_omnirect **out, const mcc_omnirect_desc *desc);
void mcc_omnirect_destroy(mcc_omnirect *h);
int mcc_omnirect_remap(mcc_omnirect *h, const unsigned char *src, long long src_stride, unsigned char *dst,
                       long long dst_stride);

/* measurement, as mcc_omnicalib_time_steps: n_frames back-to-back remap launches on the resident
 * source (whatever the last remap left there); ms_per_frame = device time per launch from two HIP
 * events on the handle's stream. */
int mcc_omnirect_time_remap(mcc_omnirect *h, int n_frames, double *ms_per_frame);

/* ---------------------------------------------------------------- cv::omnidir::stereoReconstruct
 * (src/omnidir.cpp:1383-1539): stereoRectify, undistortImage of both images with R1 / R2, a semi-global
 * matcher on the rectified pair, the float disparity and the point cloud.
 *
 * The matcher restates StereoSGBM::create(0, numDisparities, SADWindowSize, 8 cn bs^2, 32 cn bs^2) in
 * MODE_SGBM (one pass, five directions; disp12MaxDiff, preFilterCap, uniquenessRatio and the speckle
 * filter at their zero defaults).  Its specification is DESIGN.md 7e and the numpy model
 * tests/npsgbm.py; all of its arithmetic is integer.  Agreement with a real OpenCV build is NOT
 * claimed bit for bit.  Its output is int16 [height][width], disparity x 16, -16 where there is none
 * (always in the columns x < numDisparities).
 *
 * Refused with MCC_EINVAL before any device work: a null pointer; channels other than 1 or 3, or not
 * the same in both images; images of different sizes; a stride shorter than a row; a flag other than
 * MCC_OMNI_RECTIFY_PERSPECTIVE / _LONGLATI; numDisparities <= 0, not a multiple of 16 or above 256; a
 * matched width <= numDisparities or above 65535; SADWindowSize even or < 1; 93 cn bs^2 > 32767 (the
 * block cost would leave 16 bits); a cost volume 2 height (width - numDisparities) numDisparities
 * above MCC_OMNI_SGBM_MAX_COST_BYTES (the handle holds three times that); a point type other than
 * MCC_OMNI_XYZRGB / MCC_OMNI_XYZ; T = 0 or a baseline along z (as mcc_omnidir_stereo_rectify); a
 * singular Knew. */
#define MCC_OMNI_XYZRGB 1   /* cv::omnidir::XYZRGB: 6 floats per point, x y z r g b */
#define MCC_OMNI_XYZ 2      /* cv::omnidir::XYZ: 3 floats per point                */
#define MCC_OMNI_SGBM_MAX_COST_BYTES (1LL << 30)

/* the matcher alone on an already rectified pair; disparity is short[height * width] */
int mcc_omnidir_sgbm(const unsigned char *left, int width, int height, int channels, long long left_stride,
                     const unsigned char *right, int width2, int height2, int channels2, long long right_stride,
                     int num_disparities, int sad_window_size, int device, short *disparity);

/* The per-frame case: both cameras' fixed-point maps, the images, the signal planes, the cost
 * volumes and the cloud stay on the device; compute is two uploads, the kernels and the downloads.
 * new_width == 0 is the reference's empty newSize: the rectified images take the source size and,
 * because the reference's cloud loop runs over newSize, the cloud is empty. */
typedef struct mcc_omnirecon mcc_omnirecon;

typedef struct mcc_omnirecon_desc {
    const double *K1, *D1;  /* [9], [4] or NULL                                   */
    double xi1;
    const double *K2, *D2;
    double xi2;
    const double *R, *T;    /* [9], [3]: the second camera's pose                 */
    int flag;               /* MCC_OMNI_RECTIFY_PERSPECTIVE or _LONGLATI          */
    int num_disparities, sad_window_size;
    int src_width, src_height;
    int channels;           /* 1 or 3                                             */
    int new_width, new_height;
    const double *Knew;     /* [9] or NULL (K1)                                   */
    int point_type;         /* MCC_OMNI_XYZRGB or MCC_OMNI_XYZ                    */
    int device;
} mcc_omnirecon_desc;

int mcc_omnirecon_create(mcc_omnirecon **out, const mcc_omnirecon_desc *desc);
void mcc_omnirecon_destroy(mcc_omnirecon *h);

/* One frame pair.  disparity: float[out_h * out_w] in pixels, -1 without a match, 0 where the first
 * rectified image is black.  rec1 / rec2: the rectified images with their row strides.  cloud: room
 * for capacity points of 3 (XYZ) or 6 (XYZRGB) floats, in the reference's order (columns, then rows);
 * *n_points = the number of points.  If it exceeds capacity the call is MCC_EINVAL, the message names
 * the count needed, *n_points holds it, and the cloud is not written at all (disparity and the
 * rectified images are).  cloud may be NULL with capacity 0. */
int mcc_omnirecon_compute(mcc_omnirecon *h, const unsigned char *image1, long long stride1,
                          const unsigned char *image2, long long stride2, float *disparity, unsigned char *rec1,
                          long long rec1_stride, unsigned char *rec2, long long rec2_stride, float *cloud,
                          long long capacity, long long *n_points);

/* measurement, as mcc_omnirect_time_remap: n_frames back-to-back computes (remap, matcher, cloud; no
 * transfers) on resident random frames; ms_per_frame from two HIP events on the handle's stream. */
int mcc_omnirecon_time(mcc_omnirecon *h, int n_frames, double *ms_per_frame);

/* stereoReconstruct in one call: a handle used once.  Both images' sizes and channel counts are
 * arguments so that a mismatch can be refused. */
int mcc_omnidir_stereo_reconstruct(const unsigned char *image1, int width, int height, int channels,
                                   long long stride1, const unsigned char *image2, int width2, int height2,
                                   int channels2, long long stride2, const double *K1, const double *D1, double xi1,
                                   const double *K2, const double *D2, double xi2, const double *R, const double *T,
                                   int flag, int num_disparities, int sad_window_size, int new_width, int new_height,
                                   const double *Knew, int point_type, int device, float *disparity,
                                   unsigned char *rec1, long long rec1_stride, unsigned char *rec2,
                                   long long rec2_stride, float *cloud, long long capacity, long long *n_points);

#ifdef __cplusplus
}
#endif
#endif
