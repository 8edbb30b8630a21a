// mcc_pincalib_internal.h -- device state and kernel arguments of the pinhole calibrateCamera
// (mcc_calibrate_camera, include/mcc.h), shared by mcc_pincalib.hip and mcc_pincalib_api.cpp.  Not
// part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "mcc_omnicalib_internal.h"

namespace mcc {

constexpr int kPcMaxCorners = 1024;   // per view, as mcc_solve_pnp_batch
constexpr int kPcGlob = 12;           // fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
constexpr int kPcLinN = 189;          // PcLin::N  (mcc_pincalib_device.hpp; asserted in mcc_pincalib.hip)
constexpr int kPcCtrN = 103;          // PcCtr::N
constexpr int kPcYz = 78;             // Y_v [6][12], z_v [6]

enum { kPcConverged = 0, kPcCount = 1, kPcStalled = 2, kPcNotFinite = 3 };

// Device-resident Levenberg-Marquardt state.  A trial is k_pc_lin then k_pc_try; the last arriver of
// k_pc_try accepts or rejects it and is the only writer of everything but `fail` (k_pc_lin's last arriver).
struct PcState {
    int iter;        // accepted steps
    int tries;       // rejected trials in a row
    int trials;      // trials run
    int done;
    int status;      // kPc*
    int init;        // 1: the next k_pc_try only evaluates the error of the starting point
    int relin;       // 1: the next k_pc_lin linearises; 0: it reuses the view's stored sums (after a reject)
    int fail;        // the trial's factorisation failed (a view's block or the reduced system)
    int crit_type, max_count;
    double eps;
    double lambda;
    double err;      // sum of squared residuals at the current parameters
    double change;   // |x_new - x_old| / |x_old| of the last accepted step
};

struct PcArgs {
    int n;                       // views
    const int* view_off;         // [n + 1]
    const double* obj;           // [3 * corners]
    const double* img;           // [2 * corners]
    int mask;                    // bit k: global slot k is free
    double aspect;               // fx / fy under FIX_ASPECT_RATIO, else 0
    double* x;                   // [6 n] poses (rvec, tvec)
    double* xt;                  // [6 n] trial poses
    double* glob;                // [12]
    double* dc;                  // [12] the trial's global step
    double* lin;                 // [n * kPcLinN] the views' undamped sums
    double* Yz;                  // [n * kPcYz]
    double* contrib;             // [n * kPcCtrN]
    double* gsum;                // [n_groups * kPcCtrN]
    double* esq;                 // [n] squared error per view at the current parameters
    double* esq_t;               // [n] ... at the trial
    double* egs;                 // [n_groups]
    int* cnt;                    // [2 (n_groups + 1)] tickets of the two kernels, zero between launches
    PcState* st;
    int group_size, n_groups;
};

}  // namespace mcc

hipError_t mcc_launch_pc_lin(const mcc::PcArgs& a, hipStream_t s);
hipError_t mcc_launch_pc_try(const mcc::PcArgs& a, hipStream_t s);
