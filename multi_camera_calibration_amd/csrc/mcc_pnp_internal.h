// mcc_pnp_internal.h -- kernel arguments of the batched solvePnP (mcc_solve_pnp_batch, include/mcc.h),
// shared by mcc_pnp.hip and mcc_pnp_api.cpp.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include "mcc_omnicalib_internal.h"

namespace mcc {

constexpr int kPnpMaxCorners = 1024;   // per view: the boundary's per-edge limit (mcc_create)
constexpr int kPnpDist = 12;           // k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, zero-padded by the host

struct PnpArgs {
    int n_views;
    const int* view_off;    // [n_views + 1]
    const double* obj;      // [3 * corners]
    const double* img;      // [2 * corners]
    const int* view_cam;    // [n_views] or nullptr (camera 0)
    const double* K;        // [9 * n_cams]
    const double* D;        // [kPnpDist * n_cams]
    int max_iter;
    int max_n;              // corners of the largest view: sizes a view's LDS slice
    double* rvec;           // [3 * n_views]
    double* tvec;           // [3 * n_views]
    double* rms;            // [n_views]
    int* status;            // [n_views]
};

}  // namespace mcc

hipError_t mcc_launch_pnp(const mcc::PnpArgs& a, hipStream_t s);
