// mcc_pnp_device.hpp -- one view of the batched solvePnP, as one wave64 runs it (k_pnp, mcc_pnp.hip).
//
// The sequence is host/pnp.cpp's solvePnP: undistort, centroid and covariance, planarity test,
// homography (planar) or 12-vector DLT (non-planar), nearest rotation, rodriguesInv, then
// Levenberg-Marquardt with the host's policy.  The one deliberate difference is the Jacobian, which
// is analytic here (d pixel / d (r, t) through the left SO(3) Jacobian of mcc_device.hpp) where the
// host takes central differences.
//
// Lanes stride over the view's corners (corner i belongs to lane i % 64) and every sum is a lane's
// strided partial in corner order followed by the xor butterfly 32, 16, .. 1, so a view's result
// depends on nothing but the view.  Everything after a sum is computed redundantly by all lanes from
// wave-uniform values: accept, reject and converge are wave-uniform branches.  The 3 x 3 and 6 x 6
// work stays in registers (static indices only, no stack); the 9 x 9 / 12 x 12 normal matrix and its
// eigenvectors live in the view's LDS slice with lane k owning row k.
#pragma once
#include "mcc_device.hpp"

#ifndef MCC_PNP_LANES   // (a host build with 1 lane replays the same arithmetic on a CPU)
#define MCC_PNP_LANES 64
#define MCC_PNP_FN __device__ __forceinline__
namespace mcc {
// orders a lane's LDS writes before the other lanes' reads; a wave runs in lockstep, so no s_barrier
__device__ __forceinline__ void pnp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// lane 0's value as a scalar
__device__ __forceinline__ double pnp_uniform(double v) {
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int pnp_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// fixed-order sum over the wave, the same bits on every lane
__device__ __forceinline__ double pnp_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return pnp_uniform(v);
}
}  // namespace mcc
#endif

namespace mcc {

struct PnpCam {
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4;
};

enum { kPnpSolved = 0, kPnpTooFew = 1, kPnpDegenerate = 2 };

// ---------------------------------------------------------------- camera model (pnp.cpp::distort)
MCC_PNP_FN void pnp_distort(const PnpCam& c, double x, double y, double& xd, double& yd) {
#pragma clang fp contract(off)
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double cd = (1 + c.k1 * r2 + c.k2 * r4 + c.k3 * r6) / (1 + c.k4 * r2 + c.k5 * r4 + c.k6 * r6);
    xd = x * cd + 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x) + c.s1 * r2 + c.s2 * r4;
    yd = y * cd + c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y + c.s3 * r2 + c.s4 * r4;
}

// pnp.cpp::undistortPoints for one pixel
MCC_PNP_FN void pnp_undistort(const PnpCam& c, double u, double v, double& xo, double& yo) {
#pragma clang fp contract(off)
    const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
    double x = x0, y = y0;
    for (int it = 0; it < 20; ++it) {
        const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
        const double icd = (1 + c.k4 * r2 + c.k5 * r4 + c.k6 * r6) / (1 + c.k1 * r2 + c.k2 * r4 + c.k3 * r6);
        const double dx = 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x) + c.s1 * r2 + c.s2 * r4;
        const double dy = c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y + c.s3 * r2 + c.s4 * r4;
        x = (x0 - dx) * icd;
        y = (y0 - dy) * icd;
    }
    xo = x;
    yo = y;
}

// observed - projected, in pnp.cpp::projectPoints' order.  Contraction is off so that the error of
// the current pose and of a trial pose round alike wherever this is inlined (accept is en <= err).
MCC_PNP_FN void pnp_residual(const PnpCam& c, const double* R, const double* t, const double* X, double u, double v,
                             double& eu, double& ev) {
#pragma clang fp contract(off)
    const double Xc = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
    const double Yc = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    const double Zc = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
    const double z = Zc != 0.0 ? 1.0 / Zc : 1.0;
    double xd, yd;
    pnp_distort(c, Xc * z, Yc * z, xd, yd);
    eu = u - (c.fx * xd + c.cx);
    ev = v - (c.fy * yd + c.cy);
}

// pnp.cpp::rms_error
MCC_PNP_FN double pnp_rms(const PnpCam& c, const double* r, const double* t, const double* obj, const double* img,
                          int n, int lane) {
#pragma clang fp contract(off)
    Rot rot;
    rodrigues_v2m(r, rot);
    double s = 0.0;
    for (int i = lane; i < n; i += MCC_PNP_LANES) {
        const double X[3] = {obj[3 * i], obj[3 * i + 1], obj[3 * i + 2]};
        double eu, ev;
        pnp_residual(c, rot.R, t, X, img[2 * i], img[2 * i + 1], eu, ev);
        s += eu * eu + ev * ev;
    }
    s = pnp_wave_sum(s);
    return sqrt(s / (double)n);
}

// The two rows of d pixel / d (r, t) at one corner, and the residual.
//   Xc = R X + t:  d Xc / d t = I,  d Xc / d r = -[R X]x Jl(r)  (R(r + d) = exp([Jl d]x) R(r)),
// so with g = d pixel / d Xc (a row), the rotation part of the row is (R X x g)^T Jl.
MCC_PNP_FN void pnp_rows(const PnpCam& c, const double* R, const double* Jl, const double* t, const double* X,
                         double u, double v, double* ju, double* jv, double& eu, double& ev) {
    const double P[3] = {R[0] * X[0] + R[1] * X[1] + R[2] * X[2], R[3] * X[0] + R[4] * X[1] + R[5] * X[2],
                         R[6] * X[0] + R[7] * X[1] + R[8] * X[2]};
    const double Zc = P[2] + t[2];
    const double z = Zc != 0.0 ? 1.0 / Zc : 1.0;
    const double x = (P[0] + t[0]) * z, y = (P[1] + t[1]) * z;
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double num = 1 + c.k1 * r2 + c.k2 * r4 + c.k3 * r6, den = 1 + c.k4 * r2 + c.k5 * r4 + c.k6 * r6;
    const double iden = 1.0 / den, cd = num * iden;
    // d cd / d r2, and the prism terms' d / d r2
    const double dcd = ((c.k1 + 2 * c.k2 * r2 + 3 * c.k3 * r4) - cd * (c.k4 + 2 * c.k5 * r2 + 3 * c.k6 * r4)) * iden;
    const double dsx = c.s1 + 2 * c.s2 * r2, dsy = c.s3 + 2 * c.s4 * r2;
    const double xd = x * cd + 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x) + c.s1 * r2 + c.s2 * r4;
    const double yd = y * cd + c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y + c.s3 * r2 + c.s4 * r4;
    eu = u - (c.fx * xd + c.cx);
    ev = v - (c.fy * yd + c.cy);
    const double a11 = cd + 2 * x * x * dcd + 2 * c.p1 * y + 6 * c.p2 * x + 2 * x * dsx;
    const double a12 = 2 * x * y * dcd + 2 * c.p1 * x + 2 * c.p2 * y + 2 * y * dsx;
    const double a21 = 2 * x * y * dcd + 2 * c.p1 * x + 2 * c.p2 * y + 2 * x * dsy;
    const double a22 = cd + 2 * y * y * dcd + 6 * c.p1 * y + 2 * c.p2 * x + 2 * y * dsy;
    const double gu[3] = {c.fx * a11 * z, c.fx * a12 * z, -c.fx * (a11 * x + a12 * y) * z};
    const double gv[3] = {c.fy * a21 * z, c.fy * a22 * z, -c.fy * (a21 * x + a22 * y) * z};
    const double wu[3] = {P[1] * gu[2] - P[2] * gu[1], P[2] * gu[0] - P[0] * gu[2], P[0] * gu[1] - P[1] * gu[0]};
    const double wv[3] = {P[1] * gv[2] - P[2] * gv[1], P[2] * gv[0] - P[0] * gv[2], P[0] * gv[1] - P[1] * gv[0]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ju[j] = wu[0] * Jl[j] + wu[1] * Jl[3 + j] + wu[2] * Jl[6 + j];
        jv[j] = wv[0] * Jl[j] + wv[1] * Jl[3 + j] + wv[2] * Jl[6 + j];
        ju[3 + j] = gu[j];
        jv[3 + j] = gv[j];
    }
}

// The two rows of d pixel / d (fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6) at the same corner
// (calibrateCamera's global block, mcc_pincalib_device.hpp; the prism terms are not calibrated).
MCC_PNP_FN void pnp_rows_intr(const PnpCam& c, const double* R, const double* t, const double* X, double* iu,
                              double* iv) {
    const double Xc = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
    const double Yc = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    const double Zc = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
    const double z = Zc != 0.0 ? 1.0 / Zc : 1.0;
    const double x = Xc * z, y = Yc * z;
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double num = 1 + c.k1 * r2 + c.k2 * r4 + c.k3 * r6, den = 1 + c.k4 * r2 + c.k5 * r4 + c.k6 * r6;
    const double iden = 1.0 / den, cd = num * iden;
    const double xd = x * cd + 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x) + c.s1 * r2 + c.s2 * r4;
    const double yd = y * cd + c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y + c.s3 * r2 + c.s4 * r4;
    const double fxx = c.fx * x * iden, fyy = c.fy * y * iden;   // d (fx xd, fy yd) / d num
    const double gxx = -fxx * cd, gyy = -fyy * cd;               // ... / d den
    iu[0] = xd;  iv[0] = 0.0;
    iu[1] = 0.0; iv[1] = yd;
    iu[2] = 1.0; iv[2] = 0.0;
    iu[3] = 0.0; iv[3] = 1.0;
    iu[4] = fxx * r2; iv[4] = fyy * r2;
    iu[5] = fxx * r4; iv[5] = fyy * r4;
    iu[6] = c.fx * (2 * x * y);        iv[6] = c.fy * (r2 + 2 * y * y);
    iu[7] = c.fx * (r2 + 2 * x * x);   iv[7] = c.fy * (2 * x * y);
    iu[8] = fxx * r6; iv[8] = fyy * r6;
    iu[9] = gxx * r2; iv[9] = gyy * r2;
    iu[10] = gxx * r4; iv[10] = gyy * r4;
    iu[11] = gxx * r6; iv[11] = gyy * r6;
}

// ---------------------------------------------------------------- 3 x 3 in registers
MCC_PNP_FN double pnp_det3(const double* M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// the Jacobi rotation that zeroes a_pq: t = tan, c, s (pnp.cpp::jacobi_eig's)
MCC_PNP_FN void pnp_jacobi_cs(double app, double aqq, double apq, double& t, double& c, double& s) {
    const double theta = (aqq - app) / (2.0 * apq);
    t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
}

template <int P, int Q>
MCC_PNP_FN void pnp_rot3(double* A, double* V) {
    constexpr int K = 3 - P - Q;   // the third index
    const double apq = A[P * 3 + Q];
    if (!(fabs(apq) > 1e-300)) return;
    double t, c, s;
    pnp_jacobi_cs(A[P * 3 + P], A[Q * 3 + Q], apq, t, c, s);
    const double akp = A[K * 3 + P], akq = A[K * 3 + Q];
    A[K * 3 + P] = A[P * 3 + K] = c * akp - s * akq;
    A[K * 3 + Q] = A[Q * 3 + K] = s * akp + c * akq;
    A[P * 3 + P] -= t * apq;
    A[Q * 3 + Q] += t * apq;
    A[P * 3 + Q] = A[Q * 3 + P] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vkp = V[k * 3 + P], vkq = V[k * 3 + Q];
        V[k * 3 + P] = c * vkp - s * vkq;
        V[k * 3 + Q] = s * vkp + c * vkq;
    }
}

template <int I, int J>
MCC_PNP_FN void pnp_order3(double* w, double* V) {   // w[I] <= w[J], the columns of V with them
    const bool sw = w[J] < w[I];
    const double a = w[I], b = w[J];
    w[I] = sw ? b : a;
    w[J] = sw ? a : b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = V[k * 3 + I], y = V[k * 3 + J];
        V[k * 3 + I] = sw ? y : x;
        V[k * 3 + J] = sw ? x : y;
    }
}

// cyclic Jacobi on a symmetric 3 x 3: eigenvalues ascending in w, eigenvectors in the columns of V
MCC_PNP_FN void pnp_eig3(const double* S, double* w, double* V) {
    double A[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        A[k] = S[k];
        V[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < 50; ++sweep) {
        const double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
        const double dia = A[0] * A[0] + A[4] * A[4] + A[8] * A[8];
        if (!(off > 1e-40 * dia) || off < 1e-300) break;
        pnp_rot3<0, 1>(A, V);
        pnp_rot3<0, 2>(A, V);
        pnp_rot3<1, 2>(A, V);
    }
    w[0] = A[0]; w[1] = A[4]; w[2] = A[8];
    pnp_order3<0, 1>(w, V);
    pnp_order3<1, 2>(w, V);
    pnp_order3<0, 1>(w, V);
}

// pnp.cpp::nearest_rotation: R = M (M^T M)^-1/2, det +1
MCC_PNP_FN void pnp_nearest_rotation(const double* M, double* R) {
    double MtM[9], w[3], V[9], Si[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) MtM[i * 3 + j] = M[i] * M[j] + M[3 + i] * M[3 + j] + M[6 + i] * M[6 + j];
    pnp_eig3(MtM, w, V);
    double iw[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) iw[k] = 1.0 / sqrt(fmax(w[k], 1e-300));
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Si[i * 3 + j] = V[i * 3] * V[j * 3] * iw[0] + V[i * 3 + 1] * V[j * 3 + 1] * iw[1] +
                            V[i * 3 + 2] * V[j * 3 + 2] * iw[2];
    mat3_mul(M, Si, R);
    if (pnp_det3(R) < 0) {
        R[2] = -R[2]; R[5] = -R[5]; R[8] = -R[8];
    }
}

// pnp.cpp::log_near_pi: the rotation vector of R within 1e-5 rad of pi.  There cvRodrigues2 (rodrigues_m2v's
// s < 1e-5, c <= 0 branch) takes the axis from sqrt((R_ii + 1) / 2) and the angle from acos(c), both good
// to sqrt(eps) = 1e-8 only, which the closed-form pose (max_iter = 0) would carry.  Here the angle is
// atan2(s, c) and the axis the column of (R + R^T) / 2 - c I = (1 - c) k k^T with the largest diagonal
// entry, its sign from the skew part 2 s k (at s = 0, where r and -r are one rotation, the column's own).
MCC_PNP_FN void pnp_log_near_pi(const double* R, double* r) {
    const double vx = R[7] - R[5], vy = R[2] - R[6], vz = R[3] - R[1];
    const double s = 0.5 * sqrt(vx * vx + vy * vy + vz * vz);
    const double c = fmax(-1.0, fmin(1.0, (R[0] + R[4] + R[8] - 1) * 0.5));
    const double d0 = R[0] - c, d1 = R[4] - c, d2 = R[8] - c;
    const double o01 = 0.5 * (R[1] + R[3]), o02 = 0.5 * (R[2] + R[6]), o12 = 0.5 * (R[5] + R[7]);
    const bool c0 = d0 >= d1 && d0 >= d2, c1 = !c0 && d1 >= d2;
    const double k0 = c0 ? d0 : c1 ? o01 : o02, k1 = c0 ? o01 : c1 ? d1 : o12, k2 = c0 ? o02 : c1 ? o12 : d2;
    double sc = atan2(s, c) / sqrt(k0 * k0 + k1 * k1 + k2 * k2);
    if (k0 * vx + k1 * vy + k2 * vz < 0) sc = -sc;
    r[0] = sc * k0;
    r[1] = sc * k1;
    r[2] = sc * k2;
}

// ---------------------------------------------------------------- the DLT's normal matrix, in LDS
// Both DLTs have rows (h, 0, -u h) and (0, h, -v h) with h = (X, Y, 1) or (X, Y, Z, 1), so
//   A^T A = [ S 0 -Su ; 0 S -Sv ; . . Sq ],  S* = sum w h h^T with w = 1, u, v, u^2 + v^2:
// four symmetric M x M sums per lane instead of the (3M)^2 entries.
template <int M>
struct PnpSums {
    static constexpr int kT = M * (M + 1) / 2;
    double s[4][kT];
};

template <int M>
MCC_PNP_FN void pnp_sums_zero(PnpSums<M>& a) {
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int k = 0; k < PnpSums<M>::kT; ++k) a.s[w][k] = 0.0;
}

template <int M>
MCC_PNP_FN void pnp_sums_add(PnpSums<M>& acc, const double* h, double u, double v) {
    const double q = u * u + v * v;
    int k = 0;
#pragma unroll
    for (int a = 0; a < M; ++a)
#pragma unroll
        for (int b = a; b < M; ++b) {
            const double hh = h[a] * h[b];
            acc.s[0][k] += hh;
            acc.s[1][k] += u * hh;
            acc.s[2][k] += v * hh;
            acc.s[3][k] += q * hh;
            ++k;
        }
}

// wave sums, then lane 0 writes the N x N matrix (N = 3M, row-major)
template <int M>
MCC_PNP_FN void pnp_sums_store(PnpSums<M>& acc, double* A, int lane) {
    constexpr int N = 3 * M;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int k = 0; k < PnpSums<M>::kT; ++k) acc.s[w][k] = pnp_wave_sum(acc.s[w][k]);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < M; ++a)
#pragma unroll
            for (int b = 0; b < M; ++b) {
                const int lo = a < b ? a : b, hi = a < b ? b : a;
                const int k = lo * M - lo * (lo - 1) / 2 + (hi - lo);
                A[a * N + b] = acc.s[0][k];
                A[(M + a) * N + M + b] = acc.s[0][k];
                A[a * N + M + b] = 0.0;
                A[(M + a) * N + b] = 0.0;
                A[a * N + 2 * M + b] = -acc.s[1][k];
                A[(2 * M + b) * N + a] = -acc.s[1][k];
                A[(M + a) * N + 2 * M + b] = -acc.s[2][k];
                A[(2 * M + b) * N + M + a] = -acc.s[2][k];
                A[(2 * M + a) * N + 2 * M + b] = acc.s[3][k];
            }
    }
    pnp_wave_sync();
}

// Cyclic Jacobi on the symmetric N x N matrix A in LDS (N = 9 or 12), eigenvectors in the columns of
// V; lane k owns row k of both.  A rotation (p, q) is one phase: every lane reads its row's two
// entries, then writes them and their mirror images in rows p and q, which no other lane reads in
// that phase (lanes p and q work from the three entries read before it).  Returns the index of the
// smallest eigenvalue, and the second smallest and the largest for the rank test.
MCC_PNP_FN int pnp_eig_lds(double* A, double* V, int N, int lane, double& w_second, double& w_max) {
    for (int k = lane; k < N; k += MCC_PNP_LANES)
        for (int j = 0; j < N; ++j) V[k * N + j] = (j == k) ? 1.0 : 0.0;
    pnp_wave_sync();
    for (int sweep = 0; sweep < 40; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int k = lane; k < N; k += MCC_PNP_LANES)
            for (int j = 0; j < N; ++j) {
                const double a = A[k * N + j];
                if (j == k) dia += a * a;
                else off += a * a;
            }
        off = pnp_wave_sum(off);
        dia = pnp_wave_sum(dia);
        if (!(off > 1e-40 * dia)) break;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double app = pnp_uniform(A[p * N + p]), aqq = pnp_uniform(A[q * N + q]);
                const double apq = pnp_uniform(A[p * N + q]);
                if (!(fabs(apq) > 1e-22 * (fabs(app) + fabs(aqq)))) continue;
                double t, c, s;
                pnp_jacobi_cs(app, aqq, apq, t, c, s);
                for (int k = lane; k < N; k += MCC_PNP_LANES) {
                    if (k == p) {
                        A[p * N + p] = app - t * apq;
                        A[p * N + q] = 0.0;
                    } else if (k == q) {
                        A[q * N + q] = aqq + t * apq;
                        A[q * N + p] = 0.0;
                    } else {
                        const double akp = A[k * N + p], akq = A[k * N + q];
                        const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
                        A[k * N + p] = np_;
                        A[p * N + k] = np_;
                        A[k * N + q] = nq_;
                        A[q * N + k] = nq_;
                    }
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - s * vkq;
                    V[k * N + q] = s * vkp + c * vkq;
                }
                pnp_wave_sync();
            }
    }
    int imin = 0;
    double w0 = pnp_uniform(A[0]);
    for (int k = 1; k < N; ++k) {
        const double d = pnp_uniform(A[k * N + k]);
        if (d < w0) {
            w0 = d;
            imin = k;
        }
    }
    w_second = 1e300;
    w_max = 0.0;
    for (int k = 0; k < N; ++k) {
        const double d = pnp_uniform(A[k * N + k]);
        if (k != imin && d < w_second) w_second = d;
        if (d > w_max) w_max = d;
    }
    return imin;
}

// ---------------------------------------------------------------- 6 x 6 in registers
// (J^T J with its diagonal scaled by 1 + lambda) d = J^T e: symmetric positive definite unless a
// parameter has no effect, so elimination without pivoting; false when a pivot is not positive
MCC_PNP_FN bool pnp_solve6(double* A, double* b) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double piv = A[k * 6 + k];
        ok = ok && (piv > 1e-300);
        const double ip = 1.0 / piv;
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            const double f = A[i * 6 + k] * ip;
#pragma unroll
            for (int j = k; j < 6; ++j) A[i * 6 + j] -= f * A[k * 6 + j];
            b[i] -= f * b[k];
        }
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = b[i];
#pragma unroll
        for (int j = i + 1; j < 6; ++j) s -= A[i * 6 + j] * b[j];
        b[i] = s / A[i * 6 + i];
    }
    return ok;
}

MCC_PNP_FN bool pnp_finite6(const double* r, const double* t) {
    const double s = r[0] + r[1] + r[2] + t[0] + t[1] + t[2];
    return fabs(s) < 1.7e308;   // false for NaN and infinities (and a sum past the range)
}

// ---------------------------------------------------------------- one view
// obj / img point at the view's first corner; xy [2n], A [144] and V [144] are the view's LDS slice.
// r / t / rms are valid for status kPnpSolved only.
MCC_PNP_FN int pnp_solve_view(const double* obj, const double* img, int n, const PnpCam& cam, int max_iter,
                              double* xy, double* A, double* V, int lane, double* r, double* t, double& rms) {
    rms = -1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = t[k] = 0.0;
    if (n < 4) return kPnpTooFew;
    const double inv_n = 1.0 / (double)n;

    // centroid and covariance of the object points
    double c[3];
    {
        double s0 = 0, s1 = 0, s2 = 0;
        for (int i = lane; i < n; i += MCC_PNP_LANES) {
            s0 += obj[3 * i];
            s1 += obj[3 * i + 1];
            s2 += obj[3 * i + 2];
        }
        c[0] = pnp_wave_sum(s0) * inv_n;
        c[1] = pnp_wave_sum(s1) * inv_n;
        c[2] = pnp_wave_sum(s2) * inv_n;
    }
    double C[9], w[3], E[9];
    {
        double s[6] = {0, 0, 0, 0, 0, 0};
        for (int i = lane; i < n; i += MCC_PNP_LANES) {
            const double dx = obj[3 * i] - c[0], dy = obj[3 * i + 1] - c[1], dz = obj[3 * i + 2] - c[2];
            s[0] += dx * dx; s[1] += dx * dy; s[2] += dx * dz;
            s[3] += dy * dy; s[4] += dy * dz; s[5] += dz * dz;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] = pnp_wave_sum(s[k]);
        C[0] = s[0]; C[1] = C[3] = s[1]; C[2] = C[6] = s[2];
        C[4] = s[3]; C[5] = C[7] = s[4]; C[8] = s[5];
    }
    pnp_eig3(C, w, E);
    // A plane when the spread across it is below 3e-2 of the smaller spread within it (squared lengths: an
    // rms relief of 17 % of the target's narrow side).  Below that the homography start is close enough for
    // LM, which then works on the true points; the 12-vector DLT, whose normal matrix is nearly
    // rank-deficient on a board that is slightly off its plane, is not: under 0.2 px noise it put LM into a
    // wrong minimum, reported as solved, at ratios from 1e-9 up to 8e-3, and at none from 1.5e-2 up.
    const bool planar = w[0] <= 3e-2 * fmax(w[1], 1e-300);
    // the points lie on one line: no pose (first: on a line w0 and w1 are both rounding noise)
    if (w[1] <= 1e-9 * fmax(w[2], 1e-300)) return kPnpDegenerate;
    if (!planar && n < 6) return kPnpTooFew;

    for (int i = lane; i < n; i += MCC_PNP_LANES) {
        double x, y;
        pnp_undistort(cam, img[2 * i], img[2 * i + 1], x, y);
        xy[2 * i] = x;
        xy[2 * i + 1] = y;
    }
    pnp_wave_sync();

    double R[9];
    if (planar) {
        // plane frame: Rp rows = (e2, e1, e0) (e0 = normal), X_plane = Rp (X - c)
        double Rp[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            Rp[k] = E[k * 3 + 2];
            Rp[3 + k] = E[k * 3 + 1];
            Rp[6 + k] = E[k * 3 + 0];
        }
        if (pnp_det3(Rp) < 0) {
            Rp[6] = -Rp[6]; Rp[7] = -Rp[7]; Rp[8] = -Rp[8];
        }
        // pnp.cpp::homography: normalised DLT of H [X Y 1]^T ~ [x y 1]^T
        double mx, my, mu, mv;
        {
            double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
            for (int i = lane; i < n; i += MCC_PNP_LANES) {
                const double dx = obj[3 * i] - c[0], dy = obj[3 * i + 1] - c[1], dz = obj[3 * i + 2] - c[2];
                s0 += Rp[0] * dx + Rp[1] * dy + Rp[2] * dz;
                s1 += Rp[3] * dx + Rp[4] * dy + Rp[5] * dz;
                s2 += xy[2 * i];
                s3 += xy[2 * i + 1];
            }
            mx = pnp_wave_sum(s0) * inv_n;
            my = pnp_wave_sum(s1) * inv_n;
            mu = pnp_wave_sum(s2) * inv_n;
            mv = pnp_wave_sum(s3) * inv_n;
        }
        double sx, su;
        {
            double s0 = 0, s1 = 0;
            for (int i = lane; i < n; i += MCC_PNP_LANES) {
                const double dx = obj[3 * i] - c[0], dy = obj[3 * i + 1] - c[1], dz = obj[3 * i + 2] - c[2];
                s0 += hypot(Rp[0] * dx + Rp[1] * dy + Rp[2] * dz - mx, Rp[3] * dx + Rp[4] * dy + Rp[5] * dz - my);
                s1 += hypot(xy[2 * i] - mu, xy[2 * i + 1] - mv);
            }
            sx = sqrt(2.0) * n / fmax(pnp_wave_sum(s0), 1e-300);
            su = sqrt(2.0) * n / fmax(pnp_wave_sum(s1), 1e-300);
        }
        {
            PnpSums<3> acc;
            pnp_sums_zero(acc);
            for (int i = lane; i < n; i += MCC_PNP_LANES) {
                const double dx = obj[3 * i] - c[0], dy = obj[3 * i + 1] - c[1], dz = obj[3 * i + 2] - c[2];
                const double h[3] = {(Rp[0] * dx + Rp[1] * dy + Rp[2] * dz - mx) * sx,
                                     (Rp[3] * dx + Rp[4] * dy + Rp[5] * dz - my) * sx, 1.0};
                pnp_sums_add(acc, h, (xy[2 * i] - mu) * su, (xy[2 * i + 1] - mv) * su);
            }
            pnp_sums_store(acc, A, lane);
        }
        double w2nd, wmax;
        const int im = pnp_eig_lds(A, V, 9, lane, w2nd, wmax);
        // the normalised matrix has one null vector; a second one (1e-14: Jacobi's own error is ~1e-16 of
        // the largest eigenvalue) means the correspondences do not determine a homography
        if (!(w2nd > 1e-14 * wmax)) return kPnpDegenerate;
        double Hn[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Hn[k] = pnp_uniform(V[k * 9 + im]);
        // H = Tu^-1 Hn Tx
        const double Tx[9] = {sx, 0, -sx * mx, 0, sx, -sx * my, 0, 0, 1};
        const double Tui[9] = {1 / su, 0, mu, 0, 1 / su, mv, 0, 0, 1};
        double T1[9], H[9];
        mat3_mul(Hn, Tx, T1);
        mat3_mul(Tui, T1, H);
        const double n1 = sqrt(H[0] * H[0] + H[3] * H[3] + H[6] * H[6]);
        const double n2 = sqrt(H[1] * H[1] + H[4] * H[4] + H[7] * H[7]);
        double lam = 1.0 / sqrt(n1 * n2);
        if (H[8] * lam < 0) lam = -lam;   // the plane origin in front of the camera
        const double h1[3] = {H[0] * lam, H[3] * lam, H[6] * lam}, h2[3] = {H[1] * lam, H[4] * lam, H[7] * lam};
        const double h3[3] = {h1[1] * h2[2] - h1[2] * h2[1], h1[2] * h2[0] - h1[0] * h2[2],
                              h1[0] * h2[1] - h1[1] * h2[0]};
        const double Mh[9] = {h1[0], h2[0], h3[0], h1[1], h2[1], h3[1], h1[2], h2[2], h3[2]};
        double Rh[9];
        pnp_nearest_rotation(Mh, Rh);
        // X_cam = Rh Rp (X - c) + th  ->  R = Rh Rp, t = th - R c
        mat3_mul(Rh, Rp, R);
#pragma unroll
        for (int i = 0; i < 3; ++i)
            t[i] = H[3 * i + 2] * lam - (R[i * 3] * c[0] + R[i * 3 + 1] * c[1] + R[i * 3 + 2] * c[2]);
    } else {
        // DLT of P = [R | t] on normalised image coordinates and centred object points
        {
            PnpSums<4> acc;
            pnp_sums_zero(acc);
            for (int i = lane; i < n; i += MCC_PNP_LANES) {
                const double h[4] = {obj[3 * i] - c[0], obj[3 * i + 1] - c[1], obj[3 * i + 2] - c[2], 1.0};
                pnp_sums_add(acc, h, xy[2 * i], xy[2 * i + 1]);
            }
            pnp_sums_store(acc, A, lane);
        }
        // (no rank test here: this matrix is not normalised, as on the host, so its eigenvalues' ratios
        // depend on the object points' unit; a zero or non-finite scale below is the host's own test)
        double w2nd, wmax;
        const int im = pnp_eig_lds(A, V, 12, lane, w2nd, wmax);
        double P[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) P[k] = pnp_uniform(V[k * 12 + im]);
        const double M3[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
        const double sc = cbrt(pnp_det3(M3));
        if (sc == 0 || !(fabs(sc) < 1.7e308)) return kPnpDegenerate;
        const double isc = 1.0 / sc;
        double Ms[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Ms[k] = M3[k] * isc;
        pnp_nearest_rotation(Ms, R);
#pragma unroll
        for (int i = 0; i < 3; ++i)
            t[i] = P[4 * i + 3] * isc - (R[i * 3] * c[0] + R[i * 3 + 1] * c[1] + R[i * 3 + 2] * c[2]);
    }
    {
        double th, s, co;
        int near_pi;
        rodrigues_m2v(R, r, th, s, co, near_pi);
        if (near_pi) pnp_log_near_pi(R, r);
    }
    if (!pnp_finite6(r, t)) return kPnpDegenerate;

    // Levenberg-Marquardt on the reprojection error, pnp.cpp's policy, analytic Jacobian
    double lambda = 1e-3;
    double err = pnp_rms(cam, r, t, obj, img, n, lane);
    for (int it = 0; it < max_iter; ++it) {
        Rot rot;
        rodrigues_v2m(r, rot);
        double Jl[9];
        so3_jac(r, rot, +1.0, Jl);
        double H[21], g[6];
#pragma unroll
        for (int k = 0; k < 21; ++k) H[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = 0.0;
        for (int i = lane; i < n; i += MCC_PNP_LANES) {
            const double X[3] = {obj[3 * i], obj[3 * i + 1], obj[3 * i + 2]};
            double ju[6], jv[6], eu, ev;
            pnp_rows(cam, rot.R, Jl, t, X, img[2 * i], img[2 * i + 1], ju, jv, eu, ev);
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                g[a] += ju[a] * eu + jv[a] * ev;
#pragma unroll
                for (int b = a; b < 6; ++b) H[k++] += ju[a] * ju[b] + jv[a] * jv[b];
            }
        }
#pragma unroll
        for (int k = 0; k < 21; ++k) H[k] = pnp_wave_sum(H[k]);
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = pnp_wave_sum(g[k]);
        bool improved = false, converged = false;
        for (int tries = 0; tries < 10 && !improved; ++tries) {
            double S[36], d[6];
            {
                int k = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    d[a] = g[a];
#pragma unroll
                    for (int b = a; b < 6; ++b) {
                        S[a * 6 + b] = S[b * 6 + a] = (a == b) ? H[k] * (1.0 + lambda) : H[k];
                        ++k;
                    }
                }
            }
            if (!pnp_solve6(S, d)) break;
            const double rn[3] = {r[0] + d[0], r[1] + d[1], r[2] + d[2]};
            const double tn[3] = {t[0] + d[3], t[1] + d[4], t[2] + d[5]};
            const double en = pnp_rms(cam, rn, tn, obj, img, n, lane);
            if (en <= err) {
                const double rel = (err - en) / fmax(err, 1e-300);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    r[k] = rn[k];
                    t[k] = tn[k];
                }
                err = en;
                lambda = fmax(lambda * 0.1, 1e-12);
                improved = true;
                converged = rel < 1e-14;
            } else {
                lambda *= 10.0;
            }
        }
        if (!improved || converged) break;
    }
    if (!pnp_finite6(r, t) || !(fabs(err) < 1.7e308)) return kPnpDegenerate;
    rms = err;
    return kPnpSolved;
}

}  // namespace mcc
