// mcc_omnistereo_internal.h -- kernel arguments of the two-camera omnidir calibration
// (cv::omnidir::stereoCalibrate, src/omnidir.cpp:1213-1381), shared by mcc_omnistereo.hip and
// mcc_omnistereo_api.cpp.  Not part of the public ABI (include/mcc_omnidir.h).  The loop state is
// the single-camera OcState.
#pragma once
#include <hip/hip_runtime.h>

#include "mcc_omnicalib_internal.h"

namespace mcc {

constexpr int kOsG = 26;           // global block: om, T (6) | intrinsics of camera 1 (10) | of camera 2 (10)
// The 4N x 32 strip of a view is never staged whole: k_os_step walks the corners in chunks of 64
// or 128 and accumulates the Gram in the MFMA accumulators, so LDS does not bound the corner count.
// The cap is an argument check only (a 64 x 32 board).
constexpr int kOsMaxCorners = 2048;

struct OsArgs {
    OcLoop lp;                                 // x: [6(n+1) + 20] in encodeParametersStereo layout; om, T never fixed
    const double* ox; const double* oy; const double* oz;   // [n * np] SoA pattern points
    const double* iu1; const double* iv1;      // [n * np] image points of camera 1
    const double* iu2; const double* iv2;      // [n * np] image points of camera 2
    int np, chunk;                             // np corners in every view; chunk = 64 or 128 corners
};

struct OsErrArgs {
    const double* ox; const double* oy; const double* oz;
    const double* iu1; const double* iv1; const double* iu2; const double* iv2;
    const double* x;
    double* view_sq;                           // [n] sum of squared errors of both cameras per view
    int n, np;
};

}  // namespace mcc

size_t mcc_os_shmem(int chunk);
hipError_t mcc_os_set_attrs(int chunk);
hipError_t mcc_launch_os_step(const mcc::OsArgs& a, hipStream_t s);
hipError_t mcc_launch_os_err(const mcc::OsErrArgs& a, hipStream_t s);
