// mcc_pincalib_internal.h -- device state and kernel arguments of the pinhole calibrateCamera
// (mcc_calibrate_camera, include/mcc.h), shared by mcc_pincalib.hip and mcc_pincalib_api.cpp, and the
// loop state and Levenberg-Marquardt policy that the pinhole stereoCalibrate shares with it
// (mcc_pinloop_device.hpp, mcc_pinloop_host.hpp).  Not part of the public ABI.
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

// The Levenberg-Marquardt policy, once, for both pinhole loops (pin_verdict, mcc_pinloop_device.hpp) and
// for the host (tests/cpp/test_pinloop_policy.cpp): lambda starts at 1e-3 (the host sets it), a trial is
// accepted when its factorisation held and en <= err (so a NaN error is a rejection), lambda / 10 floored at
// 1e-12 on an acceptance and x 10 on a rejection, ten rejections in a row end the loop as stalled.
__host__ __device__ inline bool pc_accepts(const PcState& s, double en) { return !s.fail && en <= s.err; }

// The state after k_*_try's sum en of the trial's squared error: the evaluation of the start (s.init), a
// rejection or an acceptance, with the `done` / `status` they set.  `change` is read on an acceptance only.
__host__ __device__ inline PcState pc_next(PcState s, double en, double change) {
    if (s.init) {
        s.err = en;
        s.init = 0;
        s.relin = 1;
        if (!(fabs(en) < 1.7e308)) { s.done = 1; s.status = kPcNotFinite; }
    } else if (!pc_accepts(s, en)) {
        s.trials = s.trials + 1;
        s.lambda = s.lambda * 10.0;
        s.relin = 0;
        if (s.tries + 1 >= 10) { s.done = 1; s.status = kPcStalled; }
        s.tries = s.tries + 1;
    } else {
        s.trials = s.trials + 1;
        s.tries = 0;
        s.relin = 1;
        s.err = en;
        s.change = change;
        s.lambda = fmax(s.lambda * 0.1, 1e-12);
        if ((s.crit_type & 2) && change < s.eps) { s.done = 1; s.status = kPcConverged; }
        else if ((s.crit_type & 1) && s.iter + 1 >= s.max_count) { s.done = 1; s.status = kPcCount; }
        s.iter = s.iter + 1;
    }
    return s;
}

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
