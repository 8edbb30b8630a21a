// mcc_pinrect.hip -- CDNA4 kernels of the pinhole rectification: cv::initUndistortRectifyMap
// and cv::undistortPoints through cv::projectPoints' model (PnpCam, mcc_pnp_device.hpp).  The per-frame remap
// is k_or_remap (mcc_omnirect.hip), which does not depend on the camera model.  One thread per output
// element, no LDS, no stack, FP64 throughout, FMA contraction off (the numpy model's rounding).
//
//   k_pr_map     one thread per map pixel in 64 x 4 blocks (j on the lane, so the map1 / map2 stores
//                coalesce): (X, Y, W) = (P R)^-1 (j, i, 1) as base_i + j * step, the division by W, the
//                distortion, K.  The map type is a template parameter and so is RATIONAL: without k4 k5 k6
//                the denominator of the radial term is exactly 1 and its division is not compiled.  The nine
//                inverse entries and the sixteen camera doubles are kernel arguments; nothing is loaded.
//   k_pr_points  one thread per point: pr_undistort (mcc_pinrect_internal.h), the iteration count a
//                runtime loop bound.
#include <hip/hip_runtime.h>

#include "../../include/mcc.h"
#include "mcc_pinrect_internal.h"

namespace mcc {

// pnp_distort; with RATIONAL false k4 = k5 = k6 = 0, so its quotient num / 1 is num, bit for bit
template <bool RATIONAL>
__device__ __forceinline__ void pr_distort(const PnpCam& c, double x, double y, double& xd, double& yd) {
#pragma clang fp contract(off)
    if constexpr (RATIONAL) {
        pnp_distort(c, x, y, xd, yd);
    } else {
        const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
        const double cd = 1 + c.k1 * r2 + c.k2 * r4 + c.k3 * r6;
        xd = x * cd + 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x) + c.s1 * r2 + c.s2 * r4;
        yd = y * cd + c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y + c.s3 * r2 + c.s4 * r4;
    }
}

template <int MAP, bool RATIONAL>
__global__ __launch_bounds__(256) void k_pr_map(PrMapArgs a) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (j >= a.w || i >= a.h) return;
    const double X = (i * a.iPR[1] + a.iPR[2]) + j * a.iPR[0];
    const double Y = (i * a.iPR[4] + a.iPR[5]) + j * a.iPR[3];
    const double W = (i * a.iPR[7] + a.iPR[8]) + j * a.iPR[6];
    double xd, yd;
    pr_distort<RATIONAL>(a.cam, X / W, Y / W, xd, yd);
    const double u = a.cam.fx * xd + a.cam.cx, v = a.cam.fy * yd + a.cam.cy;
    const size_t o = (size_t)i * a.w + j;
    if constexpr (MAP == MCC_MAP_FLOAT) {
        ((float*)a.map1)[o] = (float)u;
        ((float*)a.map2)[o] = (float)v;
    } else {
        // cvRound (round half even) of 32 u; the short cast wraps (include/mcc_omnidir.h)
        const int iu = __double2int_rn(u * 32), iv = __double2int_rn(v * 32);
        ((short2*)a.map1)[o] = make_short2((short)(iu >> 5), (short)(iv >> 5));
        ((unsigned short*)a.map2)[o] = (unsigned short)((iv & 31) * 32 + (iu & 31));
    }
}

__global__ __launch_bounds__(256) void k_pr_points(PrPointsArgs a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    const double2 p = ((const double2*)a.src)[t];
    double x, y;
    pr_undistort(a.cam, a.R, a.P, a.iterations, p.x, p.y, x, y);
    ((double2*)a.dst)[t] = make_double2(x, y);
}

}  // namespace mcc

namespace {

template <bool RATIONAL>
void pr_map_launch(const mcc::PrMapArgs& a, int map_type, dim3 grid, hipStream_t s) {
    if (map_type == MCC_MAP_FLOAT)
        hipLaunchKernelGGL((mcc::k_pr_map<MCC_MAP_FLOAT, RATIONAL>), grid, dim3(64, 4), 0, s, a);
    else
        hipLaunchKernelGGL((mcc::k_pr_map<MCC_MAP_FIXED, RATIONAL>), grid, dim3(64, 4), 0, s, a);
}

}  // namespace

hipError_t mcc_launch_pr_map(const mcc::PrMapArgs& a, int map_type, bool rational, hipStream_t s) {
    if (map_type != MCC_MAP_FLOAT && map_type != MCC_MAP_FIXED) return hipErrorInvalidValue;
    const dim3 grid((a.w + 63) / 64, (a.h + 3) / 4);
    if (rational)
        pr_map_launch<true>(a, map_type, grid, s);
    else
        pr_map_launch<false>(a, map_type, grid, s);
    return hipGetLastError();
}

hipError_t mcc_launch_pr_points(const mcc::PrPointsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mcc::k_pr_points, dim3((unsigned)(((long long)a.n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
