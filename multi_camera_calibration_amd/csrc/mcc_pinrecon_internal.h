// mcc_pinrecon_internal.h -- kernel arguments of cv::reprojectImageTo3D and of the tail of the pinhole
// stereoReconstruct, and the per-pixel arithmetic that mcc_pinrecon.hip, mcc_pinrecon_api.cpp
// and the C++ selftest share.  Not part of the public ABI (include/mcc.h).
//
// pn_reproject and pn_is_point are one function each for both sides: the kernels compile them for the
// device, mcc_pinrecon_host_cloud (host only) calls the host instances, so the count kernel, the write
// kernel and the host model cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>

#ifndef MCC_PN_FN
#define MCC_PN_FN __host__ __device__ __forceinline__
#endif

namespace mcc {

// (X, Y, Z, W) = Q (x, y, d, 1): float64, sums left to right, no contraction
MCC_PN_FN void pn_reproject(const double* q, int x, int y, float d, double& X, double& Y, double& Z, double& W) {
#pragma clang fp contract(off)
    const double dd = (double)d;
    X = q[0] * x + q[1] * y + q[2] * dd + q[3];
    Y = q[4] * x + q[5] * y + q[6] * dd + q[7];
    Z = q[8] * x + q[9] * y + q[10] * dd + q[11];
    W = q[12] * x + q[13] * y + q[14] * dd + q[15];
}

// one float64 division, one rounding to float32.  A NaN (0 / 0) is stored as the quiet NaN 0x7FC00000: which NaN a
// divider returns is its own business, and the results are compared as bit patterns
MCC_PN_FN float pn_quotient(double a, double w) {
    const float v = (float)(a / w);
    return v != v ? __builtin_nanf("") : v;
}

// which pixels of the dense image are points of the cloud
struct PnCloudRule {
    double max_z;            // <= 0: no limit
    int use_roi;
    int rx, ry, rw, rh;      // roi1 in the output frame
};

// the cloud rule of 7j: d > 0, W finite and not 0, 0 < Z / W (<= max_z), inside the roi
MCC_PN_FN bool pn_is_point(const double* q, const PnCloudRule& r, int x, int y, float d) {
#pragma clang fp contract(off)
    if (!(d > 0.0f)) return false;
    double X, Y, Z, W;
    pn_reproject(q, x, y, d, X, Y, Z, W);
    if (!(W - W == 0.0) || W == 0.0) return false;   // inf - inf and NaN - NaN are NaN
    const double z = Z / W;
    if (!(z > 0.0)) return false;
    if (r.max_z > 0.0 && !(z <= r.max_z)) return false;
    if (r.use_roi && (x < r.rx || x >= r.rx + r.rw || y < r.ry || y >= r.ry + r.rh)) return false;
    return true;
}

// k_pn_dmin / k_pn_reproject: disp is packed, `type` (MCC_DISP_*) is a template parameter of the kernels
struct PnReprojectArgs {
    double q[16];            // Q, row-major: kernel arguments (SGPRs), nothing is loaded
    const void* disp;        // float[w h] or short[w h] (disparity x 16)
    const float* dmin;       // the image's minimum (handle_missing only)
    float* real;             // float[w h] or NULL: the float disparity, -1 where the short one has no match
    float* points;           // float[3 w h]
    int w, h;
};

constexpr int kPnDminBlocks = 1024;   // partial minima of the first level, at most
constexpr int kPnCloudBatch = 8;      // rows whose loads k_pn_cloud has in flight together

struct PnCloudArgs {
    double q[16];
    PnCloudRule rule;
    const float* real;           // [h][w]
    const unsigned char* rec1;   // first rectified image, packed rows of w * cn bytes
    int* col_count;              // [w n_seg + 1], the layout of SgFinishArgs::col_count
    float* cloud;
    int w, h, cn, point_floats;  // 3 or 6
};

}  // namespace mcc

// type: MCC_DISP_*; missing: handle_missing != 0 (then partial holds kPnDminBlocks + 1 floats and a.dmin points at
// its last one).  All sizes are checked by the callers.
hipError_t mcc_launch_pn_reproject(const mcc::PnReprojectArgs& a, int type, bool missing, float* partial, hipStream_t s);
// the count per column and segment, the scan (k_sg_scan) and the compacted cloud
hipError_t mcc_launch_pn_cloud(const mcc::PnCloudArgs& a, hipStream_t s);
