// mcc_omnicalib_device.hpp -- device helpers shared by the omnidir calibration kernels
// (mcc_omnicalib.hip: calibrate, mcc_omnistereo.hip: stereoCalibrate): the write-through hand-off,
// the fixed-order sums, the block-arrow loop step that both kernels run on their view's Gram, and
// the Mei projection of one corner with its 2 x 16 Jacobian rows.
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

// sum_{q < n} p[q * LC] in q order; the sc1 loads are issued 16 at a time so a group costs one
// or two memory round trips instead of n dependent ones
template <int LC>
__device__ __forceinline__ double oc_sum(const double* p, int n) {
    constexpr int B = 16;
    double v = 0.0;
    for (int q0 = 0; q0 < n; q0 += B) {
        double b[B];
#pragma unroll
        for (int u = 0; u < B; ++u) b[u] = oc_ld(p + (size_t)min(q0 + u, n - 1) * LC);
#pragma unroll
        for (int u = 0; u < B; ++u) v += q0 + u < n ? b[u] : 0.0;
    }
    return v;
}

// packed upper-triangle index of (i, j), i <= j, of a G x G matrix (row i holds G - i entries)
template <int G>
__device__ __forceinline__ int oc_up(int i, int j) { return i * G - (i * (i - 1)) / 2 + (j - i); }

// ---------------------------------------------------------------- the block-arrow loop step
// calibrate (src/omnidir.cpp:1126-1149) and stereoCalibrate (:1273-1296) run the same damped
// Gauss-Newton loop on a block-arrow normal matrix: n view pose blocks U_v of 6 x 6, one dense
// global block of G parameters (10 intrinsics; or om, T and 2 x 10 intrinsics = 26), and the
// 6 x G couplings W_v.  A kernel (k_oc_step, k_os_step: one 256-thread workgroup per view) brings
// its view's strip Gram into C (row stride LD: [pose 6 | global G | padding], fixed parameters'
// rows and columns masked to 0 -- subMatrix), J^T E into je (masked) and je_raw, and calls, in order:
//   oc_phase0        the pose update the previous step left pending,
//                    x_v += alpha2 ((U^-1 rp - coef U^-1 1) - Y_v yc), with its |G|^2, |x|^2 partials;
//                    the global parameters and their mask into LDS;
//   oc_pose_inverse  wave 0: U_v^-1 by register Gauss-Jordan (U = JEx^T JEx is SPD), U^-1 rp, U^-1 1;
//   oc_contribute    Y_v = U_v^-1 W_v and the view's packed contribution (OcLayout<G>): the Schur
//                    complement S_v = V_v - W_v^T Y_v, the reduced right-hand sides of JTE and of the
//                    ones vector, the global JTE, the Sherman-Morrison sums and the two norms, written
//                    write-through (sc1);
//   oc_reduce_solve  a two-level fixed-order last-arriver reduction (groups of ~sqrt(n) views, then the
//                    groups); the last arriver's wave 0 runs the stop test on |G| / |x| of the update
//                    applied in phase 0, solves the G x G reduced system for both right-hand sides
//                    (lane = row), applies the rank-one correction of JTJ + epsilon (epsilon added to
//                    EVERY entry, :925 / :1019) and alpha_smooth2, updates the global parameters and
//                    leaves the pose update pending.
// Pos gives the places of a view's pose and of global entry l in x, G and jte: pose(v), glob(l).
// The LDS arrays are the kernels'; the helpers declare none but oc_arrive's flag.  FP64 throughout,
// like the reference.

// Returns st->pending.  pose[6], nrm[2][6], glob[G], msk[G] in LDS; the caller synchronises.
// (fillFixed never touches poses: they are never fixed.)
template <int G, class Pos>
__device__ __forceinline__ int oc_phase0(const OcLoop& a, const Pos pos, int v, double* pose, double* nrm,
                                         double* glob, double* msk) {
    const int tid = threadIdx.x, pending = a.st->pending;
    if (tid < 6) {
        const size_t xi = pos.pose(v) + tid;
        const double xo = a.x[xi];
        double g = 0.0, xn = xo;
        if (pending) {
            const double al = a.st->alpha2, cf = a.st->coef;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < G; ++j) s += a.Yv[6 * G * (size_t)v + tid * G + j] * a.yc[j];
            g = al * ((a.zb[6 * (size_t)v + tid] - cf * a.zu[6 * (size_t)v + tid]) - s);
            xn = xo + g;
            a.x[xi] = xn;
            a.G[xi] = g;
        }
        pose[tid] = xn;
        nrm[tid] = g * g;
        nrm[6 + tid] = xo * xo;
    } else if (tid >= 64 && tid < 64 + G) {
        glob[tid - 64] = a.x[pos.glob(tid - 64)];
        msk[tid - 64] = a.mask[tid - 64];
    }
    return pending;
}

// wave 0: Ui = U^-1 of C[0:6, 0:6], zbl = Ui je[0:6], zul = Ui 1; sets bit 0 of *error if U is not PD
template <int LD>
__device__ __forceinline__ void oc_pose_inverse(const double* C, const double* je, double* Ui, double* zbl,
                                                double* zul, int* error) {
    const int lane = threadIdx.x & 63;
    if (threadIdx.x >= 64) return;
    const int li = lane < 6 ? lane : 0;
    double row[12];
#pragma unroll
    for (int j = 0; j < 6; ++j) { row[j] = C[li * LD + j]; row[6 + j] = li == j ? 1.0 : 0.0; }
    double dii = 1.0;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double piv = oc_readlane(row[k], k);
        bad |= !(piv > 0.0);
        const double pv = piv > 0.0 ? piv : 1.0;
        const double ip = 1.0 / pv;
        if (lane == k) dii = pv;
        const double f = lane == k ? 0.0 : row[k] * ip;
        double pr[12];
#pragma unroll
        for (int j = k + 1; j < 12; ++j) pr[j] = oc_readlane(row[j], k);
#pragma unroll
        for (int j = k + 1; j < 12; ++j) row[j] -= f * pr[j];
    }
    if (lane < 6) {
        const double id = 1.0 / dii;
        double zb = 0.0, zu = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double h = row[6 + j] * id;
            Ui[lane * 6 + j] = h;
            zb += h * je[j];
            zu += h;
        }
        zbl[lane] = zb;
        zul[lane] = zu;
    }
    if (bad && lane == 0) atomicOr(error, 1);
}

// Y = U^-1 W (6 x G, W = C[0:6, 6:6+G]) into Yl and Yv, the view's zb, zu and pose JTE, then the
// packed contribution of view v.  One barrier inside; the stores are drained by oc_arrive.
template <int G, int LD, class Pos>
__device__ __forceinline__ void oc_contribute(const OcLoop& a, const Pos pos, int v, const double* C, const double* je,
                                              const double* je_raw, const double* Ui, const double* zbl,
                                              const double* zul, const double* nrm, double* Yl) {
    using L = OcLayout<G>;
    constexpr int kT = (6 * G + 63) & ~63;   // the first thread past Y's waves
    static_assert(kT + 18 <= 256, "block size");
    const int tid = threadIdx.x;
    if (tid < 6 * G) {
        const int i = tid / G, j = tid % G;
        double y = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) y += Ui[i * 6 + k] * C[k * LD + 6 + j];
        Yl[tid] = y;
        a.Yv[6 * G * (size_t)v + tid] = y;
    } else if (tid >= kT && tid < kT + 6) {
        a.zb[6 * (size_t)v + tid - kT] = zbl[tid - kT];
    } else if (tid >= kT + 6 && tid < kT + 12) {
        a.zu[6 * (size_t)v + tid - (kT + 6)] = zul[tid - (kT + 6)];
    } else if (tid >= kT + 12 && tid < kT + 18) {
        a.jte[pos.pose(v) + tid - (kT + 12)] = je[tid - (kT + 12)];
    }
    __syncthreads();
    double* out = a.contrib + (size_t)v * L::Lc;
    // Where one pass covers the contribution (G = 10) a wave walks several branches in turn, and each
    // stores at once, so that the write latency of one hides under the arithmetic of the next: 0.1 us
    // of a 17 us step.  With two passes (G = 26) one store per pass is the faster form, by 0.25 us.
    constexpr bool kStoreInBranch = L::Lc <= 256;
    for (int e = tid; e < L::Lc; e += 256) {
        double s = 0.0;
        if (e < L::Rb) {
            int i = 0, rem = e;
            while (rem >= G - i) { rem -= G - i; ++i; }
            const int j = i + rem;
            s = C[(6 + i) * LD + 6 + j];
#pragma unroll
            for (int k = 0; k < 6; ++k) s -= C[k * LD + 6 + i] * Yl[k * G + j];
            if (kStoreInBranch) oc_st(out + e, s);
        } else if (e < L::Wu) {
            const int j = e - L::Rb;
            s = je[6 + j];
#pragma unroll
            for (int k = 0; k < 6; ++k) s -= C[k * LD + 6 + j] * zbl[k];
            if (kStoreInBranch) oc_st(out + e, s);
        } else if (e < L::Jc) {
            const int j = e - L::Wu;
#pragma unroll
            for (int k = 0; k < 6; ++k) s += C[k * LD + 6 + j] * zul[k];
            if (kStoreInBranch) oc_st(out + e, s);
        } else if (e < L::Ab) {
            s = je_raw[6 + e - L::Jc];   // J^T E before the flag reduction (computeJacobian's JTE)
            if (kStoreInBranch) oc_st(out + e, s);
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k)
                s += e == L::Ab ? zbl[k] : e == L::Au ? zul[k] : e == L::Ng ? nrm[k] : nrm[6 + k];
            if (kStoreInBranch) oc_st(out + e, s);
        }
        if (!kStoreInBranch) oc_st(out + e, s);
    }
}

// The reduction and, in the last arriver's wave 0, the stop test, the reduced solve and the update
// of the global parameters.  tot[Lc] and msk[G] (as oc_phase0 left it) in LDS.  Ends the kernel.
template <int G, class Pos>
__device__ __forceinline__ void oc_reduce_solve(const OcLoop& a, const Pos pos, int v, int pending, const double* msk,
                                                double* tot) {
    using L = OcLayout<G>;
    constexpr int kSearchUnroll = G <= 10 ? G : 1;   // the 26-wide pivot search and gather stay loops (VGPRs)
    OcState* st = a.st;
    const int tid = threadIdx.x, lane = tid & 63;
    const int grp = v / a.group_size, g0 = grp * a.group_size, gn = min(a.group_size, a.n - g0);
    if (!oc_arrive(&a.cnt[grp], gn)) return;
    for (int e = tid; e < L::Lc; e += 256)
        oc_st(a.gsum + (size_t)grp * L::Lc + e, oc_sum<L::Lc>(a.contrib + (size_t)g0 * L::Lc + e, gn));
    if (!oc_arrive(&a.cnt[a.n_groups], a.n_groups)) return;
    for (int e = tid; e < L::Lc; e += 256) tot[e] = oc_sum<L::Lc>(a.gsum + e, a.n_groups);
    __syncthreads();
    if (tid >= 64) return;

    // stop test (:1129-1132 / :1276-1279)
    const int k = st->iter;
    double change = st->change;
    if (pending) change = sqrt(tot[L::Ng] + st->normG2_c) / sqrt(tot[L::Nx] + st->normX2_c);
    const int ct = st->crit_type;
    const bool stop = (ct == 1 && k >= st->max_count) || (ct == 2 && change <= st->eps) ||
                      (ct == 3 && (change <= st->eps || k >= st->max_count));
    if (lane == 0) st->change = change;
    if (stop) {
        if (lane == 0) { st->done = 1; st->pending = 0; }
        return;
    }
    const double alpha2 = 1.0 - pow(1.0 - 0.01, (double)k + 1.0);   // alpha_smooth2 (:1133 / :1280)
    const double epsilon = 0.01 * pow(0.9, (double)k / 10);          // (:1135 / :1282)
    const int li = lane < G ? lane : 0;
    const bool free_i = msk[li] != 0.0;
    double row[G + 2];
#pragma unroll
    for (int j = 0; j < G; ++j) {
        const double sv = tot[L::S + (li <= j ? oc_up<G>(li, j) : oc_up<G>(j, li))];
        row[j] = free_i ? sv : (j == li ? 1.0 : 0.0);
    }
    row[G] = free_i ? tot[L::Rb + li] : 0.0;
    row[G + 1] = free_i ? 1.0 - tot[L::Wu + li] : 0.0;
    // Gauss-Jordan, lane l keeps row l.  S is symmetric but can turn numerically indefinite (the
    // f / xi coupling of the Mei model makes it near-singular, as is the reference's dense JTJ): a
    // non-positive diagonal pivot falls back to the unused row of largest |entry|; an exactly singular
    // system gives G = 0 for the whole step, as the reference's Mat::inv() (DECOMP_LU) returns a
    // zero matrix then
    bool used = lane >= G, singular = false;
    int pcol = -1;
    double dii = 1.0;
#pragma unroll
    for (int kk = 0; kk < G; ++kk) {
        // the diagonal in natural order while it is positive: the elimination order of the
        // reference's dense LU on this (near-SPD) block, whose rounding the step reproduces
        int pl = kk;
        if (!(oc_readlane(row[kk], kk) > 0.0) || __builtin_amdgcn_readlane((int)used, kk) != 0) {
            pl = -1;
            double best = 0.0;
#pragma unroll kSearchUnroll
            for (int l = 0; l < G; ++l) {
                const double c = fabs(oc_readlane(row[kk], l));
                const bool u = __builtin_amdgcn_readlane((int)used, l) != 0;
                if (!u && c > best) { best = c; pl = l; }
            }
            if (pl < 0) { singular = true; break; }
        }
        const double piv = oc_readlane(row[kk], pl);
        const double ip = 1.0 / piv;
        if (lane == pl) { dii = piv; used = true; pcol = kk; }
        const double f = lane == pl ? 0.0 : row[kk] * ip;
        double pr[G + 2];
#pragma unroll
        for (int j = kk + 1; j < G + 2; ++j) pr[j] = oc_readlane(row[j], pl);
#pragma unroll
        for (int j = kk + 1; j < G + 2; ++j) row[j] -= f * pr[j];
    }
    // lane j takes the solution of column j from the lane that pivoted it
    const double sb = lane < G && !singular ? row[G] / dii : 0.0;
    const double su = lane < G && !singular ? row[G + 1] / dii : 0.0;
    double yb = 0.0, yu = 0.0;
#pragma unroll kSearchUnroll
    for (int j = 0; j < G; ++j) {
        const unsigned long long own = __ballot(pcol == j);
        const int src = own ? (int)__builtin_ctzll(own) : 0;
        const double vb = oc_readlane(sb, src), vu = oc_readlane(su, src);
        if (lane == j) { yb = vb; yu = vu; }
    }
    // 1^T A^-1 b = sum_v 1^T U^-1 rp_v - (sum_v W_v^T U^-1 1)^T yb + 1_free^T yb (and for u)
    const double wm = lane < G ? msk[lane] - tot[L::Wu + lane] : 0.0;
    double s1 = tot[L::Ab], s2 = tot[L::Au];
#pragma unroll
    for (int l = 0; l < G; ++l) {
        s1 += oc_readlane(wm * yb, l);
        s2 += oc_readlane(wm * yu, l);
    }
    double coef = epsilon * s1 / (1.0 + epsilon * s2);
    // A + epsilon 1 1^T singular (Sherman-Morrison denominator 0) or A singular: G = 0 for the step
    const bool skip = singular || !isfinite(coef);
    if (skip) coef = 0.0;
    const double yc = skip ? 0.0 : yb - coef * yu;
    const double a2 = skip ? 0.0 : alpha2;
    const double gc = a2 * yc;
    double ng = 0.0, nx = 0.0;
    double xo = 0.0;
    if (lane < G) {
        const size_t gi = pos.glob(lane);
        xo = a.x[gi];
        a.x[gi] = xo + gc;
        a.yc[lane] = yc;
        a.G[gi] = gc;
        a.jte[gi] = tot[L::Jc + lane];
    }
#pragma unroll
    for (int l = 0; l < G; ++l) {
        ng += oc_readlane(gc * gc, l);
        nx += oc_readlane(xo * xo, l);
    }
    if (lane == 0) {
        st->normG2_c = ng;
        st->normX2_c = nx;
        st->alpha2 = a2;   // 0: the poses' pending G is 0 too
        st->coef = coef;
        st->pending = 1;
        st->iter = k + 1;
    }
}

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
