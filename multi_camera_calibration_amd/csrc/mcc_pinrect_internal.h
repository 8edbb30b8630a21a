// mcc_pinrect_internal.h -- kernel arguments of the pinhole rectification (cv::undistortPoints,
// cv::initUndistortRectifyMap) and the per-point arithmetic that mcc_pinrect.hip and
// mcc_pinrect_api.cpp share.  Not part of the public ABI (include/mcc.h).
//
// pr_undistort is one function for both sides: k_pr_points compiles it for the device and
// mcc_stereo_rectify (host only) calls the host instance for its corner and grid points, so the two
// cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#include "mcc_pnp_device.hpp"

#ifndef MCC_PR_FN
#define MCC_PR_FN __host__ __device__ __forceinline__
#endif

namespace mcc {

// pixel -> ideal point: x0 = (u - cx) / fx, y0 = (v - cy) / fy, `iterations` rounds of pnp_undistort's
// fixed-point update (the count is a runtime bound here, 20 there), then R and the first three
// columns of P (row-major 3 x 3, the identity when the caller has none).  FMA contraction is off, so
// host, device and the numpy model round alike.
MCC_PR_FN void pr_undistort(const PnpCam& c, const double* R, const double* P, int iterations, double u, double v,
                            double& xo, double& yo) {
#pragma clang fp contract(off)
    const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
    double x = x0, y = y0;
    for (int it = 0; it < iterations; ++it) {
        const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
        const double icd = (1 + c.k4 * r2 + c.k5 * r4 + c.k6 * r6) / (1 + c.k1 * r2 + c.k2 * r4 + c.k3 * r6);
        const double dx = 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x) + c.s1 * r2 + c.s2 * r4;
        const double dy = c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y + c.s3 * r2 + c.s4 * r4;
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
    }
    const double X = R[0] * x + R[1] * y + R[2], Y = R[3] * x + R[4] * y + R[5], W = R[6] * x + R[7] * y + R[8];
    x = X / W;
    y = Y / W;
    const double d = P[6] * x + P[7] * y + P[8];
    xo = (P[0] * x + P[1] * y + P[2]) / d;
    yo = (P[3] * x + P[4] * y + P[5]) / d;
}

// k_pr_map: the inverse and the camera are kernel arguments (SGPRs), nothing is loaded
struct PrMapArgs {
    double iPR[9];     // (P R)^-1: destination pixel -> direction in the camera frame
    PnpCam cam;
    int w, h;
    void* map1;        // float[w h]            or short[2 w h]
    void* map2;        // float[w h]            or unsigned short[w h]
};

struct PrPointsArgs {
    PnpCam cam;
    double R[9], P[9];
    const double* src;   // [2n] pixels (u, v)
    double* dst;         // [2n]
    int n, iterations;
};

}  // namespace mcc

// map_type: MCC_MAP_*; rational: any of k4 k5 k6 is not 0 (both checked by the callers)
hipError_t mcc_launch_pr_map(const mcc::PrMapArgs& a, int map_type, bool rational, hipStream_t s);
hipError_t mcc_launch_pr_points(const mcc::PrPointsArgs& a, hipStream_t s);
// the host part of mcc_init_undistort_rectify_map (mcc_pinrect_api.cpp): the argument checks and (P R)^-1, everything
// k_pr_map takes but the maps; MCC_OK or MCC_EINVAL with the message set.  mcc_pinrecon_api.cpp builds its maps with it.
int mcc_pr_map_args(const double* K, const double* D, int nd, const double* R, const double* P, int ld, int w, int h,
                    mcc::PrMapArgs* a, bool* rational);
