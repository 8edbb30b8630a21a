// mcc_omnistereo_internal.h -- kernel arguments of the two-camera omnidir calibration
// (cv::omnidir::stereoCalibrate, src/omnidir.cpp:1213-1381), shared by mcc_omnistereo.hip and
// mcc_omnistereo_api.cpp.  Not part of the public ABI (include/mcc_omnidir.h).  The loop state is
// the single-camera OcState.
#pragma once
#include <hip/hip_runtime.h>

#include "mcc_omnicalib_internal.h"

namespace mcc {

constexpr int kOsG = 26;           // global block: om, T (6) | intrinsics of camera 1 (10) | of camera 2 (10)
constexpr int kOsY = 6 * kOsG;     // Y_v = U_v^-1 W_v, 6 x 26

// packed per-view contribution (and group / total sums) of one loop step
constexpr int kOsS = 0;                     // [351] S_v = V_v - W_v^T U_v^-1 W_v, upper triangle of 26 x 26
constexpr int kOsRb = 351;                  // [26] rc_v - W_v^T U_v^-1 rp_v   (reduced rhs of JTE)
constexpr int kOsWu = kOsRb + kOsG;         // [26] W_v^T U_v^-1 1             (reduced rhs of the ones vector)
constexpr int kOsJc = kOsWu + kOsG;         // [26] rc_v                       (the global JTE)
constexpr int kOsAb = kOsJc + kOsG;         //      1^T U_v^-1 rp_v
constexpr int kOsAu = kOsAb + 1;            //      1^T U_v^-1 1
constexpr int kOsNg = kOsAu + 1;            //      |G_pose|^2 of the update applied in phase 0
constexpr int kOsNx = kOsNg + 1;            //      |x_pose|^2 before it
constexpr int kOsLc = kOsNx + 1;            // 433

// The 4N x 32 strip of a view is never staged whole: k_os_step walks the corners in chunks of 64
// or 128 and accumulates the Gram in the MFMA accumulators, so LDS does not bound the corner count.
// The cap is an argument check only (a 64 x 32 board).
constexpr int kOsMaxCorners = 2048;

struct OsArgs {
    OcState* st;
    const double* ox; const double* oy; const double* oz;   // [n * np] SoA pattern points
    const double* iu1; const double* iv1;      // [n * np] image points of camera 1
    const double* iu2; const double* iv2;      // [n * np] image points of camera 2
    double* x;                                 // [6(n+1) + 20] parameters (encodeParametersStereo layout)
    const double* mask;                        // [26] 1 = free, 0 = fixed (flags2idxStereo; om, T always 1)
    double* Yv;                                // [156 n] Y_v (next step's pose update)
    double* zb; double* zu;                    // [6n] U_v^-1 rp_v, U_v^-1 1
    double* yc;                                // [26] global part of the pending solution
    double* jte;                               // [P] J^T E of the last linearisation
    double* G;                                 // [P] G of the last update
    double* contrib;                           // [n * kOsLc]
    double* gsum;                              // [n_groups * kOsLc]
    int* cnt;                                  // [n_groups + 1] tickets, zero between launches
    int n, np, chunk, group_size, n_groups;    // np corners in every view; chunk = 64 or 128 corners
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
