// mcc_omnirect.hip -- CDNA4 kernels of the omnidir rectification: cv::omnidir::undistortPoints
// (src/omnidir.cpp:249-343), initUndistortRectifyMap (:348-533) and the cv::remap call of
// undistortImage (:538-546).  All three are one thread per output element, no LDS, no stack.
//
//   k_or_map     one thread per map pixel (j on the lane, so map1 / map2 stores coalesce), FP64.
//                The reference walks a row with running sums (_x += iKR(0,0)); a thread evaluates
//                the closed form base_i + j * step instead.  The flag and the map type are template
//                parameters; the matrices and intrinsics are kernel arguments.
//   k_or_remap   one thread per destination pixel: cv::remap's INTER_LINEAR on fixed-point maps
//                with BORDER_CONSTANT 0, 8-bit, 1 or 3 channels; integer arithmetic throughout.
//   k_or_points  one thread per point: pixel -> plane, the 20 fixed-point iterations of the
//                distortion inverse, the lift to the unit sphere, R, the division by Z.  Compiled
//                without FMA contraction, so every operation rounds as the reference's does.
#include <hip/hip_runtime.h>

#include "mcc_omnirect_internal.h"

namespace mcc {

// unit direction (any length) -> distorted pixel: :423-437 and :501-515
__device__ __forceinline__ void or_project(const OrIntr& in, double x, double y, double w, double& u, double& v) {
    const double r = sqrt(x * x + y * y + w * w);
    const double Xs = x / r, Ys = y / r, Zs = w / r;
    const double xu = Xs / (Zs + in.xi), yu = Ys / (Zs + in.xi);
    const double r2 = xu * xu + yu * yu;
    const double r4 = r2 * r2;
    const double rad = 1 + in.k1 * r2 + in.k2 * r4;
    const double xd = rad * xu + 2 * in.p1 * xu * yu + in.p2 * (r2 + 2 * xu * xu);
    const double yd = rad * yu + in.p1 * (r2 + 2 * yu * yu) + 2 * in.p2 * xu * yu;
    u = in.f0 * xd + in.s * yd + in.c0;
    v = in.f1 * yd + in.c1;
}

template <int FLAG, int MAP>
__global__ __launch_bounds__(256) void k_or_map(OrMapArgs a) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (j >= a.w || i >= a.h) return;
    double x, y, w;
    if constexpr (FLAG == MCC_OMNI_RECTIFY_PERSPECTIVE) {
        x = (i * a.iKR[1] + a.iKR[2]) + j * a.iKR[0];
        y = (i * a.iKR[4] + a.iKR[5]) + j * a.iKR[3];
        w = (i * a.iKR[7] + a.iKR[8]) + j * a.iKR[6];
    } else {
        const double theta = (i * a.iK[1] + a.iK[2]) + j * a.iK[0];
        const double h = (i * a.iK[4] + a.iK[5]) + j * a.iK[3];
        double xt, yt, wt;
        if constexpr (FLAG == MCC_OMNI_RECTIFY_CYLINDRICAL) {
            xt = cos(theta);   // the reference's axis order (:477-479)
            yt = sin(theta);
            wt = h;
        } else if constexpr (FLAG == MCC_OMNI_RECTIFY_LONGLATI) {
            xt = -cos(theta);
            yt = -sin(theta) * cos(h);
            wt = sin(theta) * sin(h);
        } else {   // MCC_OMNI_RECTIFY_STEREOGRAPHIC (:489-495)
            const double q = theta * theta + h * h;
            const double qa = q + 4, qb = -2 * theta * theta - 2 * h * h, qc = q - 4;
            yt = (-qb - sqrt(qb * qb - 4 * qa * qc)) / (2 * qa);
            xt = theta * (1 - yt) / 2;
            wt = h * (1 - yt) / 2;
        }
        x = a.iR[0] * xt + a.iR[1] * yt + a.iR[2] * wt;
        y = a.iR[3] * xt + a.iR[4] * yt + a.iR[5] * wt;
        w = a.iR[6] * xt + a.iR[7] * yt + a.iR[8] * wt;
    }
    double u, v;
    or_project(a.in, x, y, w, u, v);
    const size_t o = (size_t)i * a.w + j;
    if constexpr (MAP == MCC_OMNI_MAP_FLOAT) {
        ((float*)a.map1)[o] = (float)u;
        ((float*)a.map2)[o] = (float)v;
    } else {
        // cvRound (round half even) of u * INTER_TAB_SIZE; the short cast wraps (:441-445)
        const int iu = __double2int_rn(u * 32), iv = __double2int_rn(v * 32);
        ((short2*)a.map1)[o] = make_short2((short)(iu >> 5), (short)(iv >> 5));
        ((unsigned short*)a.map2)[o] = (unsigned short)((iv & 31) * 32 + (iu & 31));
    }
}

// cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) on CV_16SC2 + CV_16UC1 maps, CV_8UC<C>.  The four
// weights (32 - fx)(32 - fy) 32, ... are OpenCV's 16-bit bilinear table (they sum to 1 << 15); a
// tap outside the source reads 0, each tap tested on its own.
template <int C>
__global__ __launch_bounds__(256) void k_or_remap(OrRemapArgs a) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    const int i = blockIdx.y * 4 + threadIdx.y;
    if (j >= a.dst_w || i >= a.dst_h) return;
    const size_t o = (size_t)i * a.dst_w + j;
    const short2 m1 = ((const short2*)a.map1)[o];
    const int m2 = a.map2[o] & 1023;
    const int sx = m1.x, sy = m1.y, fx = m2 & 31, fy = m2 >> 5;
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32,
              w11 = fx * fy * 32;
    const bool x0 = (unsigned)sx < (unsigned)a.src_w, x1 = (unsigned)(sx + 1) < (unsigned)a.src_w;
    const bool y0 = (unsigned)sy < (unsigned)a.src_h, y1 = (unsigned)(sy + 1) < (unsigned)a.src_h;
    const long long o0 = (long long)sy * a.src_stride + (long long)sx * C;   // of tap (sx, sy); read only where inside
    const long long o1 = o0 + a.src_stride;
    unsigned char* d = a.dst + (long long)i * a.dst_stride + (long long)j * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int t00 = (x0 && y0) ? a.src[o0 + c] : 0, t01 = (x1 && y0) ? a.src[o0 + C + c] : 0;
        const int t10 = (x0 && y1) ? a.src[o1 + c] : 0, t11 = (x1 && y1) ? a.src[o1 + C + c] : 0;
        d[c] = (unsigned char)((w00 * t00 + w01 * t01 + w10 * t10 + w11 * t11 + 16384) >> 15);
    }
}

__global__ __launch_bounds__(64) void k_or_points(OrPointsArgs a) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= a.n) return;
    const OrIntr& in = a.in;
    const double2 pi = ((const double2*)a.src)[t];
    // pixel -> plane (:306)
    const double pp0 = (pi.x * in.f1 - in.c0 * in.f1 - in.s * (pi.y - in.c1)) / (in.f0 * in.f1);
    const double pp1 = (pi.y - in.c1) / in.f1;
    double pu0 = pp0, pu1 = pp1;
    // the distortion inverse (:310-316); pu1's update sees the new pu0 and the old r2, as there
#pragma unroll
    for (int k = 0; k < 20; ++k) {
        const double r2 = pu0 * pu0 + pu1 * pu1;
        const double r4 = r2 * r2;
        pu0 = (pp0 - 2 * in.p1 * pu0 * pu1 - in.p2 * (r2 + 2 * pu0 * pu0)) / (1 + in.k1 * r2 + in.k2 * r4);
        pu1 = (pp1 - 2 * in.p2 * pu0 * pu1 - in.p1 * (r2 + 2 * pu1 * pu1)) / (1 + in.k1 * r2 + in.k2 * r4);
    }
    // unit sphere (:319-324)
    const double r2 = pu0 * pu0 + pu1 * pu1;
    const double qa = r2 + 1, qb = 2 * in.xi * r2, qc = r2 * in.xi * in.xi - 1;
    const double Zs = (-qb + sqrt(qb * qb - 4 * qa * qc)) / (2 * qa);
    const double X0 = pu0 * (Zs + in.xi), X1 = pu1 * (Zs + in.xi), X2 = Zs;
    // rotate, back to the sphere, to the plane (:327-333)
    const double W0 = a.R[0] * X0 + a.R[1] * X1 + a.R[2] * X2;
    const double W1 = a.R[3] * X0 + a.R[4] * X1 + a.R[5] * X2;
    const double W2 = a.R[6] * X0 + a.R[7] * X1 + a.R[8] * X2;
    const double nrm = sqrt(W0 * W0 + W1 * W1 + W2 * W2);
    const double S0 = W0 / nrm, S1 = W1 / nrm, S2 = W2 / nrm;
    ((double2*)a.dst)[t] = make_double2(S0 / S2, S1 / S2);
}

}  // namespace mcc

namespace {

template <int FLAG>
void or_map_launch(const mcc::OrMapArgs& a, int map_type, dim3 grid, hipStream_t s) {
    if (map_type == MCC_OMNI_MAP_FLOAT)
        hipLaunchKernelGGL((mcc::k_or_map<FLAG, MCC_OMNI_MAP_FLOAT>), grid, dim3(64, 4), 0, s, a);
    else
        hipLaunchKernelGGL((mcc::k_or_map<FLAG, MCC_OMNI_MAP_FIXED>), grid, dim3(64, 4), 0, s, a);
}

}  // namespace

hipError_t mcc_launch_or_map(const mcc::OrMapArgs& a, int flag, int map_type, hipStream_t s) {
    const dim3 grid((a.w + 63) / 64, (a.h + 3) / 4);
    switch (flag) {
        case MCC_OMNI_RECTIFY_PERSPECTIVE: or_map_launch<MCC_OMNI_RECTIFY_PERSPECTIVE>(a, map_type, grid, s); break;
        case MCC_OMNI_RECTIFY_CYLINDRICAL: or_map_launch<MCC_OMNI_RECTIFY_CYLINDRICAL>(a, map_type, grid, s); break;
        case MCC_OMNI_RECTIFY_LONGLATI: or_map_launch<MCC_OMNI_RECTIFY_LONGLATI>(a, map_type, grid, s); break;
        case MCC_OMNI_RECTIFY_STEREOGRAPHIC: or_map_launch<MCC_OMNI_RECTIFY_STEREOGRAPHIC>(a, map_type, grid, s); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t mcc_launch_or_remap(const mcc::OrRemapArgs& a, int channels, hipStream_t s) {
    const dim3 grid((a.dst_w + 63) / 64, (a.dst_h + 3) / 4);
    if (channels == 1)
        hipLaunchKernelGGL(mcc::k_or_remap<1>, grid, dim3(64, 4), 0, s, a);
    else if (channels == 3)
        hipLaunchKernelGGL(mcc::k_or_remap<3>, grid, dim3(64, 4), 0, s, a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t mcc_launch_or_points(const mcc::OrPointsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mcc::k_or_points, dim3((a.n + 63) / 64), dim3(64), 0, s, a);
    return hipGetLastError();
}
