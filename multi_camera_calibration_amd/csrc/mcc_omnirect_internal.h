// mcc_omnirect_internal.h -- kernel arguments of the omnidir rectification (cv::omnidir::
// undistortPoints, initUndistortRectifyMap, undistortImage; src/omnidir.cpp:249-546), shared by
// mcc_omnirect.hip and mcc_omnirect_api.cpp.  Not part of the public ABI (include/mcc_omnidir.h).
#pragma once
#include <hip/hip_runtime.h>

#include "mcc_omnicalib_internal.h"

namespace mcc {

// the ten intrinsics every kernel here takes by value: K = [f0 s c0; 0 f1 c1; 0 0 1], xi, D
struct OrIntr {
    double f0, f1, s, c0, c1, xi, k1, k2, p1, p2;
};

// k_or_map: all 27 matrix entries and the intrinsics are kernel arguments (SGPRs), nothing is loaded
struct OrMapArgs {
    double iKR[9];     // (PP RR)^-1: the perspective flag's pixel -> direction
    double iK[9];      // PP^-1: pixel -> (theta, h) of the other three flags
    double iR[9];      // RR^-1: their direction into the camera frame
    OrIntr in;
    int w, h;
    void* map1;        // float[w h]            or short[2 w h]
    void* map2;        // float[w h]            or unsigned short[w h]
};

struct OrRemapArgs {
    const unsigned char* src;
    const short* map1;             // [2 dst_w dst_h] integer source pixel (x, y)
    const unsigned short* map2;    // [dst_w dst_h]   (fy << 5) | fx, 5-bit fractions
    unsigned char* dst;
    long long src_stride, dst_stride;   // bytes per row
    int src_w, src_h, dst_w, dst_h;
};

struct OrPointsArgs {
    OrIntr in;
    double R[9];
    const double* src;   // [2n] pixels (u, v)
    double* dst;         // [2n] X/Z, Y/Z after R
    int n;
};

}  // namespace mcc

// flag: MCC_OMNI_RECTIFY_*, map_type: MCC_OMNI_MAP_*, channels: 1 or 3 (all checked by the callers)
hipError_t mcc_launch_or_map(const mcc::OrMapArgs& a, int flag, int map_type, hipStream_t s);
hipError_t mcc_launch_or_remap(const mcc::OrRemapArgs& a, int channels, hipStream_t s);
hipError_t mcc_launch_or_points(const mcc::OrPointsArgs& a, hipStream_t s);
