// mcc_omnicalib_device.hpp -- device helpers shared by the omnidir calibration kernels
// (mcc_omnicalib.hip: calibrate, mcc_omnistereo.hip: stereoCalibrate): the write-through hand-off,
// the fixed-order sums, and the Mei projection of one corner with its 2 x 16 Jacobian rows.
#pragma once
#include <hip/hip_runtime.h>

#include "mcc_device.hpp"
#include "mcc_omnicalib_internal.h"

namespace mcc {

typedef double oc_v4d __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) unsigned long long oc_gu64;
typedef __attribute__((address_space(1))) int oc_gi32;

__device__ __forceinline__ void oc_st(double* p, double v) {
    __hip_atomic_store((oc_gu64*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double oc_ld(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load((oc_gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// write-through hand-off (MI355X_MICROARCH.md "visibility", Valid forms row 1): every handed-off
// double is an 8-B sc1 store, storing waves drain vmcnt(0) before the barrier, one lane takes the
// ticket, the last arriver reads with sc1 loads.  Resets the counter for the next launch.
__device__ __forceinline__ bool oc_arrive(int* counter, int expected) {
    __shared__ int last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = __hip_atomic_fetch_add((oc_gi32*)counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = (t == expected - 1);
        if (last) __hip_atomic_store((oc_gi32*)counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    return last;
}
__device__ __forceinline__ double oc_readlane(double v, int l) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, l);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// sum_{q < n} p[q * kOcLc] in q order; the sc1 loads are issued 16 at a time so a group costs one
// or two memory round trips instead of n dependent ones
__device__ __forceinline__ double oc_sum(const double* p, int n) {
    constexpr int B = 16;
    double v = 0.0;
    for (int q0 = 0; q0 < n; q0 += B) {
        double b[B];
#pragma unroll
        for (int u = 0; u < B; ++u) b[u] = oc_ld(p + (size_t)min(q0 + u, n - 1) * kOcLc);
#pragma unroll
        for (int u = 0; u < B; ++u) v += q0 + u < n ? b[u] : 0.0;
    }
    return v;
}

// packed upper-triangle index of (i, j), i <= j, of a 10 x 10 matrix (row i holds 10 - i entries)
__device__ __forceinline__ int oc_up(int i, int j) { return i * 10 - (i * (i - 1)) / 2 + (j - i); }

struct OcIntr {
    double fx, fy, s, cx, cy, xi, k1, k2, p1, p2;
};

// cv::omnidir::projectPoints for one corner (src/omnidir.cpp:141-244): pixel (pu, pv) and, with
// JAC, the two 16-entry Jacobian rows.  R / T: the view pose; Jl: the left SO(3) Jacobian of om
// (dXc/dom = -[R X]x Jl(om), the same derivative as OpenCV's dXcdR * dRdom^T).
template <bool JAC>
__device__ __forceinline__ void oc_corner(const double* R, const double* Jl, const double* T, const OcIntr& q,
                                          double X, double Y, double Z, double& pu, double& pv, double* ju,
                                          double* jv) {
    const double RX0 = R[0] * X + R[1] * Y + R[2] * Z;
    const double RX1 = R[3] * X + R[4] * Y + R[5] * Z;
    const double RX2 = R[6] * X + R[7] * Y + R[8] * Z;
    const double Xc0 = RX0 + T[0], Xc1 = RX1 + T[1], Xc2 = RX2 + T[2];
    const double nrm = sqrt(Xc0 * Xc0 + Xc1 * Xc1 + Xc2 * Xc2);
    const double r_1 = 1.0 / nrm;
    const double Xs0 = Xc0 * r_1, Xs1 = Xc1 * r_1, Xs2 = Xc2 * r_1;
    const double iden = 1.0 / (Xs2 + q.xi);
    const double xu0 = Xs0 * iden, xu1 = Xs1 * iden;
    const double r2 = xu0 * xu0 + xu1 * xu1, r4 = r2 * r2;
    const double cd = 1.0 + q.k1 * r2 + q.k2 * r4;
    const double xd0 = xu0 * cd + 2.0 * q.p1 * xu0 * xu1 + q.p2 * (r2 + 2.0 * xu0 * xu0);
    const double xd1 = xu1 * cd + q.p1 * (r2 + 2.0 * xu1 * xu1) + 2.0 * q.p2 * xu0 * xu1;
    pu = q.fx * xd0 + q.s * xd1 + q.cx;
    pv = q.fy * xd1 + q.cy;
    if (!JAC) return;
    // dxp/dXc = F * dxd/dxu * dxu/dXs * dXs/dXc
    const double r_3 = r_1 * r_1 * r_1;
    const double S00 = r_1 - Xc0 * Xc0 * r_3, S11 = r_1 - Xc1 * Xc1 * r_3, S22 = r_1 - Xc2 * Xc2 * r_3;
    const double S01 = -(Xc0 * Xc1) * r_3, S02 = -(Xc0 * Xc2) * r_3, S12 = -(Xc1 * Xc2) * r_3;
    // dxu/dXc (2 x 3) = [[iden, 0, -xu0 iden], [0, iden, -xu1 iden]] * dXs/dXc
    const double a0 = iden, a2 = -xu0 * iden, b1 = iden, b2 = -xu1 * iden;
    const double U0 = a0 * S00 + a2 * S02, U1 = a0 * S01 + a2 * S12, U2 = a0 * S02 + a2 * S22;
    const double V0 = b1 * S01 + b2 * S02, V1 = b1 * S11 + b2 * S12, V2 = b1 * S12 + b2 * S22;
    const double temp1 = 2.0 * q.k1 * xu0 + 4.0 * q.k2 * xu0 * r2;
    const double temp2 = 2.0 * q.k1 * xu1 + 4.0 * q.k2 * xu1 * r2;
    const double A00 = q.k2 * r4 + 6.0 * q.p2 * xu0 + 2.0 * q.p1 * xu1 + xu0 * temp1 + q.k1 * r2 + 1.0;
    const double A01 = 2.0 * q.p1 * xu0 + 2.0 * q.p2 * xu1 + xu0 * temp2;
    const double A10 = 2.0 * q.p1 * xu0 + 2.0 * q.p2 * xu1 + xu1 * temp1;
    const double A11 = q.k2 * r4 + 2.0 * q.p2 * xu0 + 6.0 * q.p1 * xu1 + xu1 * temp2 + q.k1 * r2 + 1.0;
    // FA = [[fx, s], [0, fy]] * A
    const double F00 = q.fx * A00 + q.s * A10, F01 = q.fx * A01 + q.s * A11;
    const double F10 = q.fy * A10, F11 = q.fy * A11;
    const double du0 = F00 * U0 + F01 * V0, du1 = F00 * U1 + F01 * V1, du2 = F00 * U2 + F01 * V2;
    const double dv0 = F10 * U0 + F11 * V0, dv1 = F10 * U1 + F11 * V1, dv2 = F10 * U2 + F11 * V2;
    // d/dom = d * dXc/dom with dXc/dom = -[RX]x Jl, -[RX]x = [[0, RX2, -RX1], [-RX2, 0, RX0], [RX1, -RX0, 0]]
    const double mu0 = du1 * (-RX2) + du2 * RX1;
    const double mu1 = du0 * RX2 + du2 * (-RX0);
    const double mu2 = du0 * (-RX1) + du1 * RX0;
    const double mv0 = dv1 * (-RX2) + dv2 * RX1;
    const double mv1 = dv0 * RX2 + dv2 * (-RX0);
    const double mv2 = dv0 * (-RX1) + dv1 * RX0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ju[j] = mu0 * Jl[j] + mu1 * Jl[3 + j] + mu2 * Jl[6 + j];
        jv[j] = mv0 * Jl[j] + mv1 * Jl[3 + j] + mv2 * Jl[6 + j];
    }
    ju[3] = du0; ju[4] = du1; ju[5] = du2;
    jv[3] = dv0; jv[4] = dv1; jv[5] = dv2;
    ju[6] = xd0; ju[7] = 0.0; jv[6] = 0.0; jv[7] = xd1;   // df
    ju[8] = xd1; jv[8] = 0.0;                              // ds
    ju[9] = 1.0; ju[10] = 0.0; jv[9] = 0.0; jv[10] = 1.0;  // dc
    const double dx0 = -xu0 * iden, dx1 = -xu1 * iden;     // dxu/dxi
    ju[11] = F00 * dx0 + F01 * dx1;                        // dxi
    jv[11] = F10 * dx0 + F11 * dx1;
    const double K0 = xu0 * r2, K1 = xu0 * r4, K2 = 2.0 * xu0 * xu1, K3 = r2 + 2.0 * xu0 * xu0;   // dxd0/dkp
    const double L0 = xu1 * r2, L1 = xu1 * r4, L2 = r2 + 2.0 * xu1 * xu1, L3 = 2.0 * xu0 * xu1;  // dxd1/dkp
    ju[12] = q.fx * K0 + q.s * L0; ju[13] = q.fx * K1 + q.s * L1;
    ju[14] = q.fx * K2 + q.s * L2; ju[15] = q.fx * K3 + q.s * L3;
    jv[12] = q.fy * L0; jv[13] = q.fy * L1; jv[14] = q.fy * L2; jv[15] = q.fy * L3;
}

__device__ __forceinline__ void oc_pose(const double* pose, double* R, double* Jl) {
    const double w[3] = {pose[0], pose[1], pose[2]};
    Rot r;
    rodrigues_v2m(w, r);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = r.R[k];
    so3_jac(w, r, +1.0, Jl);
}

}  // namespace mcc
