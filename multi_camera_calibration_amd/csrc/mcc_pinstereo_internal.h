// mcc_pinstereo_internal.h -- device state and kernel arguments of the pinhole stereoCalibrate
// (mcc_stereo_calibrate, include/mcc.h), shared by mcc_pinstereo.hip and mcc_pinstereo_api.cpp.  Not part
// of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "mcc_pincalib_internal.h"

namespace mcc {

constexpr int kPsGlob = 30;           // om T | camera 1's 12 slots | camera 2's
constexpr int kPsLinN = 702;          // PsLin::N  (mcc_pinstereo_device.hpp; asserted in mcc_pinstereo.hip)
constexpr int kPsCtrN = 526;          // PsCtr::N
constexpr int kPsYz = 186;            // Y_v [6][30], z_v [6]

// The loop state is PcState and the policy pc_next (mcc_pincalib_internal.h), shared through
// mcc_pinloop_device.hpp; the writers are k_ps_try's last arriver and, of `fail`, k_ps_lin's.

struct PsArgs {
    int n;                       // views
    const int* view_off;         // [n + 1]
    const double* obj;           // [3 * corners]
    const double* img1;          // [2 * corners]
    const double* img2;          // [2 * corners]
    int mask;                    // bit k: global slot k is free
    int same;                    // SAME_FOCAL_LENGTH: camera 2's fx, fy follow camera 1's
    double aspect1, aspect2;     // fx / fy of each camera under FIX_ASPECT_RATIO, else 0
    double* x;                   // [6 n] poses of the views in camera 1 (rvec, tvec)
    double* xt;                  // [6 n] trial poses
    double* glob;                // [30]
    double* dc;                  // [30] the trial's global step
    double* lin;                 // [n * kPsLinN] the views' undamped sums
    double* Yz;                  // [n * kPsYz]
    double* contrib;             // [n * kPsCtrN]
    double* gsum;                // [n_groups * kPsCtrN]
    double* esq;                 // [2 n] squared error per view and camera at the current parameters
    double* esq_t;               // [2 n] ... at the trial
    double* egs;                 // [n_groups]
    int* cnt;                    // [2 (n_groups + 1)] tickets of the two kernels, zero between launches
    PcState* st;
    int group_size, n_groups;
};

}  // namespace mcc

hipError_t mcc_launch_ps_lin(const mcc::PsArgs& a, hipStream_t s);
hipError_t mcc_launch_ps_try(const mcc::PsArgs& a, hipStream_t s);
