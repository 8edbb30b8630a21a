// mcc_omnicalib_internal.h -- device state and kernel arguments of the omnidir intrinsic
// calibration (cv::omnidir::calibrate, src/omnidir.cpp:1067-1211), shared by mcc_omnicalib.hip
// and mcc_omnicalib_api.cpp.  Not part of the public ABI (include/mcc_omnidir.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mcc_omnidir.h"

namespace mcc {

// packed per-view contribution (and group / total sums) of one loop step, for a global block of
// G parameters (10: one camera's intrinsics; 26: om, T and two cameras' intrinsics)
template <int G>
struct OcLayout {
    static constexpr int S = 0;                   // [G(G+1)/2] S_v = V_v - W_v^T U_v^-1 W_v, upper triangle, row-major
    static constexpr int Rb = G * (G + 1) / 2;    // [G] rc_v - W_v^T U_v^-1 rp_v   (reduced rhs of JTE)
    static constexpr int Wu = Rb + G;             // [G] W_v^T U_v^-1 1             (reduced rhs of the ones vector)
    static constexpr int Jc = Wu + G;             // [G] rc_v                       (the global JTE)
    static constexpr int Ab = Jc + G;             //     1^T U_v^-1 rp_v
    static constexpr int Au = Ab + 1;             //     1^T U_v^-1 1
    static constexpr int Ng = Au + 1;             //     |G_pose|^2 of the update applied in phase 0
    static constexpr int Nx = Ng + 1;             //     |x_pose|^2 before it
    static constexpr int Lc = Nx + 1;
};
static_assert(OcLayout<10>::Rb == 55 && OcLayout<10>::Wu == 65 && OcLayout<10>::Jc == 75 && OcLayout<10>::Ab == 85 &&
                  OcLayout<10>::Nx == 88 && OcLayout<10>::Lc == 89, "contribution layout of calibrate");
static_assert(OcLayout<26>::Rb == 351 && OcLayout<26>::Wu == 377 && OcLayout<26>::Jc == 403 && OcLayout<26>::Ab == 429 &&
                  OcLayout<26>::Nx == 432 && OcLayout<26>::Lc == 433, "contribution layout of stereoCalibrate");

constexpr int kOcMaxCorners = 512;   // per view (LDS staging of the 2N x 16 Jacobian strip)

// Device-resident loop state (calibrate, src/omnidir.cpp:1126-1149).
struct OcState {
    int iter;          // completed updates k
    int done;          // stop test fired
    int crit_type;     // 0 = never stop (measurement), 1 COUNT, 2 EPS, 3 COUNT+EPS
    int max_count;
    double eps;
    double change;     // |G| / |x| of the last update
    double normG2_c, normX2_c;   // intrinsic parts of the last update
    double alpha2, coef;         // alpha_smooth2 and the Sherman-Morrison factor of the pending update
    int pending;       // a pose update waits for the next step's phase 0
    int error;         // bit 0: a view's 6 x 6 block is not PD
};

// What the shared loop (mcc_omnicalib_device.hpp) works on, the same for both kernels; P is the
// parameter count and G the width of the global block.
// (st sits behind the buffers: in front, k_os_step keeps the whole leading kernarg tuple in
// SGPRs from its first st->done test on and spills it around the 26 x 26 elimination.)
struct OcLoop {
    double* x;                                 // [P] parameters
    const double* mask;                        // [G] 1 = free, 0 = fixed (flags2idx / flags2idxStereo)
    double* Yv;                                // [6 G n] Y_v = U_v^-1 W_v (next step's pose update)
    double* zb; double* zu;                    // [6n] U_v^-1 rp_v, U_v^-1 1
    double* yc;                                // [G] global part of the pending solution
    double* jte;                               // [P] J^T E of the last linearisation
    double* G;                                 // [P] G of the last update
    double* contrib;                           // [n * Lc]
    double* gsum;                              // [n_groups * Lc]
    int* cnt;                                  // [n_groups + 1] tickets, zero between launches
    OcState* st;
    int n, group_size, n_groups;
};

struct OcArgs {
    OcLoop lp;                                 // x: [6n + 10] in encodeParameters layout
    const int* view_off;                       // [n+1]
    const double* ox; const double* oy; const double* oz;   // [corners] SoA pattern points
    const double* iu; const double* iv;        // [corners] image points
    int max_np;
};

struct OcErrArgs {
    const int* view_off;
    const double* ox; const double* oy; const double* oz;
    const double* iu; const double* iv;
    const double* x;
    double* view_sq;                           // [n] sum of squared errors per view
    int n;
};

}  // namespace mcc

size_t mcc_oc_shmem(int max_np);
hipError_t mcc_oc_set_attrs(int max_np);
hipError_t mcc_launch_oc_step(const mcc::OcArgs& a, hipStream_t s);
hipError_t mcc_launch_oc_err(const mcc::OcErrArgs& a, hipStream_t s);
extern "C" __attribute__((visibility("hidden"))) int mcc_internal_fail(int code, const char* msg);
// cvRodrigues2 matrix -> vector with the orthonormalisation of its SVD (host, mcc_api.cpp)
extern "C" __attribute__((visibility("hidden"))) void mcc_internal_rodrigues_m2v(const double* R, double* r);
