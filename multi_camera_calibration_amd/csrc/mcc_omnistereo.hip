// mcc_omnistereo.hip -- CDNA4 kernels of the two-camera omnidir calibration
// (cv::omnidir::stereoCalibrate, src/omnidir.cpp:1213-1381; computeJacobianStereo, :937-1020).
//
// Parameters (encodeParametersStereo, :1570-1619): x = [om, T | omL_0, tL_0, ... | intr_1 | intr_2],
// P = 6(n+1) + 20.  View i contributes 4N rows: 2N of camera 1 at pose (omL_i, tL_i) and 2N of
// camera 2 at compose_motion(omL_i, tL_i, om, T).  Its column strip is
//   [own pose 6 | om, T 6 | intr_1 10 | intr_2 10]           (32 columns)
// and the normal matrix is block-arrow: n pose blocks of 6 x 6 and one dense global block of 26.
//
// One loop step = one launch of k_os_step, one 256-thread workgroup per view, built like k_oc_step:
//   phase 0  the pending pose update of this view from the previous step, with its norm partials;
//   pose     wave 0: R, Jl of the left pose; wave 1: the composed right pose (device compose(), with
//            cvRodrigues2's theta ~ pi zeroing of d om3 / d om) and the four chain-rule blocks;
//   phase A  the corners go through in chunks of 64 or 128: thread (camera, corner) projects with
//            oc_corner<true>; left rows keep [pose | intr_1] (16 columns); right rows apply the chain
//            rule of :999-1002 and keep [pose | om, T | 0 x 4] and [intr_2 | 0 x 6] (2 x 16 columns);
//   phase B  per chunk, the Gram of the left rows (one 16 x 16 tile) and of the right rows (three of
//            the 2 x 2 tiles) with v_mfma_f64_16x16x4_f64, accumulated in registers over the chunks;
//            the columns a row half does not touch are never multiplied.  J^T E on the VALU.  The
//            waves' tiles are summed in wave order into the 32 x 32 strip Gram, fixed intrinsics masked;
//   phase C  wave 0 inverts the 6 x 6 pose block; the workgroup forms Y = U^-1 W (6 x 26), the Schur
//            contribution to the 26 x 26 global block (351), the reduced right-hand sides of JTE and
//            of the ones vector, the Sherman-Morrison scalars and the norms; sc1 write-through, then
//            the two-level fixed-order last-arriver reduction;
//   final    stop test, 26 x 26 Gauss-Jordan for both right-hand sides (lane = row, natural-order
//            positive pivots, else the largest unused entry; singular: G = 0), the rank-one
//            correction of JTJ + epsilon (:1019), alpha_smooth2, update of the 26 global parameters.
// FP64 throughout, like the reference.
#include <hip/hip_runtime.h>

#include "mcc_device.hpp"
#include "mcc_omnicalib_device.hpp"
#include "mcc_omnistereo_internal.h"

namespace mcc {

// packed upper-triangle index of (i, j), i <= j, of a 26 x 26 matrix
__device__ __forceinline__ int os_up(int i, int j) { return i * kOsG - (i * (i - 1)) / 2 + (j - i); }

// oc_sum with the stereo contribution stride
__device__ __forceinline__ double os_sum(const double* p, int n) {
    constexpr int B = 16;
    double v = 0.0;
    for (int q0 = 0; q0 < n; q0 += B) {
        double b[B];
#pragma unroll
        for (int u = 0; u < B; ++u) b[u] = oc_ld(p + (size_t)min(q0 + u, n - 1) * kOsLc);
#pragma unroll
        for (int u = 0; u < B; ++u) v += q0 + u < n ? b[u] : 0.0;
    }
    return v;
}

// index of global-block entry l in the parameter vector
__device__ __forceinline__ size_t os_gidx(int l, int n) { return l < 6 ? (size_t)l : 6 * (size_t)(n + 1) + (l - 6); }

// view pose tables in LDS
constexpr int kPoseTab = 21;   // R[9], Jl[9], T[3]
constexpr int kChainTab = 36;  // d om2 / d omL [9], d om2 / d om [9], d T2 / d om [9], d T2 / d tL = R(om) [9]

// the right camera's pose of a view: compose_motion(omL, tL, om, T) (:995), then R and Jl of the
// composed vector as projectPoints recomputes them (:996)
__device__ __forceinline__ void os_right_pose(const double* pl, const double* gl, double* R3, double* J3, double* T3,
                                              Motion& m, double* R2) {
    const double w1[3] = {pl[0], pl[1], pl[2]}, T1[3] = {pl[3], pl[4], pl[5]};
    const double w2[3] = {gl[0], gl[1], gl[2]}, T2[3] = {gl[3], gl[4], gl[5]};
    Rot r1, r2;
    double Jr1[9], Jl2[9];
    rodrigues_v2m(w1, r1);
    so3_jac(w1, r1, -1.0, Jr1);
    rodrigues_v2m(w2, r2);
    so3_jac(w2, r2, +1.0, Jl2);
    double th, s, c;
    compose(r1.R, Jr1, T1, r2.R, Jl2, T2, m, th, s, c);
    if (s < 1e-5 && c > 0) {
        // cvRodrigues2's s < 1e-5, c > 0 branch: om3 = 0 and d om3 / d R3 is the fixed +-0.5 pattern
        // of om3 = vee(R3 - R3^T) / 2, so d om3 / d omL = (tr(R3) I - R3^T) / 2 Jr(omL) and
        // d om3 / d om = (tr(R3) I - R3) / 2 Jl(om); compose()'s closed form at om3 = 0 is the
        // identity there, O(theta) away
        const double tr = m.R[0] + m.R[4] + m.R[8];
        double Pr[9], Pl[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                Pl[i * 3 + j] = 0.5 * ((i == j ? tr : 0.0) - m.R[i * 3 + j]);
                Pr[i * 3 + j] = 0.5 * ((i == j ? tr : 0.0) - m.R[j * 3 + i]);
            }
        mat3_mul(Pr, Jr1, m.A1);
        mat3_mul(Pl, Jl2, m.A2);
    }
    oc_pose(m.om, R3, J3);
#pragma unroll
    for (int k = 0; k < 3; ++k) T3[k] = m.T[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) R2[k] = r2.R[k];
}

// one right-camera row: d / d(om2, T2) and d / d intr_2 in j[16] -> the two 16-column halves
__device__ __forceinline__ void os_right_row(const double* j, const double* ct, double* h0, double* h1) {
    const double* A1 = ct;
    const double* A2 = ct + 9;
    const double* B2 = ct + 18;
    const double* R2 = ct + 27;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        h0[c] = j[0] * A1[c] + j[1] * A1[3 + c] + j[2] * A1[6 + c];          // dxr / d omL (:1001)
        h0[3 + c] = j[3] * R2[c] + j[4] * R2[3 + c] + j[5] * R2[6 + c];      // dxr / d tL  (:1002)
        h0[6 + c] = (j[0] * A2[c] + j[1] * A2[3 + c] + j[2] * A2[6 + c]) +
                    (j[3] * B2[c] + j[4] * B2[3 + c] + j[5] * B2[6 + c]);    // dxr / d om  (:999)
        h0[9 + c] = j[3 + c];                                                // dxr / d T   (:1000)
    }
#pragma unroll
    for (int c = 12; c < 16; ++c) h0[c] = 0.0;
#pragma unroll
    for (int c = 0; c < 10; ++c) h1[c] = j[6 + c];
#pragma unroll
    for (int c = 10; c < 16; ++c) h1[c] = 0.0;
}

__global__ __launch_bounds__(256) void k_os_step(OsArgs a) {
    OcState* st = a.st;
    if (st->done) return;
    const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.n, np = a.np, ch = a.chunk;
    const size_t c0 = (size_t)v * np;
    extern __shared__ double sm[];
    double* JL = sm;                   // [2 ch][16] left rows  [pose 6 | intr_1 10]
    double* JR0 = JL + 32 * ch;        // [2 ch][16] right rows [pose 6 | om, T 6 | 0 x 4]
    double* JR1 = JR0 + 32 * ch;       // [2 ch][16] right rows [intr_2 10 | 0 x 6]
    double* eL = JR1 + 32 * ch;        // [2 ch]
    double* eR = eL + 2 * ch;          // [2 ch]
    double* Cp = sm;                   // after the last chunk: [4 waves][LL, R00, R01, R11][256]
    double* jp = sm + 4096;            //                       [4 waves][L, R0, R1][64]
    __shared__ double pose[6], glob[kOsG], msk[kOsG], nrm[2][6], PL[kPoseTab], PR[kPoseTab], CT[kChainTab];
    __shared__ double C[1024], je[32], je_raw[32], Ui[36], zbl[6], zul[6], Yl[kOsY], tot[kOsLc];

    // ---- phase 0: the pending pose update of the previous step (the kept poses are never fixed)
    const int pending = st->pending;
    if (tid < 6) {
        const size_t xi = 6 + 6 * (size_t)v + tid;
        const double xo = a.x[xi];
        double g = 0.0, xn = xo;
        if (pending) {
            const double al = st->alpha2, cf = st->coef;
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < kOsG; ++j) s += a.Yv[kOsY * (size_t)v + tid * kOsG + j] * a.yc[j];
            g = al * ((a.zb[6 * (size_t)v + tid] - cf * a.zu[6 * (size_t)v + tid]) - s);
            xn = xo + g;
            a.x[xi] = xn;
            a.G[xi] = g;
        }
        pose[tid] = xn;
        nrm[0][tid] = g * g;
        nrm[1][tid] = xo * xo;
    } else if (tid >= 64 && tid < 64 + kOsG) {
        glob[tid - 64] = a.x[os_gidx(tid - 64, n)];
        msk[tid - 64] = a.mask[tid - 64];
    }
    __syncthreads();

    // ---- the two poses of the view, once
    if (wave == 0) {
        double R[9], J[9];
        oc_pose(pose, R, J);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) { PL[k] = R[k]; PL[9 + k] = J[k]; }
#pragma unroll
            for (int k = 0; k < 3; ++k) PL[18 + k] = pose[3 + k];
        }
    } else if (wave == 1) {
        double R3[9], J3[9], T3[3], R2[9];
        Motion m;
        os_right_pose(pose, glob, R3, J3, T3, m, R2);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                PR[k] = R3[k]; PR[9 + k] = J3[k];
                CT[k] = m.A1[k]; CT[9 + k] = m.A2[k]; CT[18 + k] = m.B2[k]; CT[27 + k] = R2[k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) PR[18 + k] = T3[k];
        }
    }
    __syncthreads();

    // ---- phases A and B over corner chunks
    oc_v4d aLL = {0.0, 0.0, 0.0, 0.0}, a00 = aLL, a01 = aLL, a11 = aLL;
    double jL = 0.0, j0 = 0.0, j1 = 0.0;
    const int rr = lane >> 4, cc = lane & 15;
    {
        const int cam = tid / ch, cl = tid - cam * ch;   // threads [0, ch): camera 1, [ch, 2 ch): camera 2
        const double* pt = cam == 1 ? PR : PL;
        double R[9], Jr[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) { R[k] = pt[k]; Jr[k] = pt[9 + k]; }
        const double T[3] = {pt[18], pt[19], pt[20]};
        const double* gi = glob + (cam == 1 ? 16 : 6);
        const OcIntr q{gi[0], gi[1], gi[2], gi[3], gi[4], gi[5], gi[6], gi[7], gi[8], gi[9]};
        const double* iu = cam == 1 ? a.iu2 : a.iu1;
        const double* iv = cam == 1 ? a.iv2 : a.iv1;
        for (int b0 = 0; b0 < np; b0 += ch) {
            const int cn = min(ch, np - b0), rows = 2 * cn, rows4 = (rows + 3) & ~3;
            if (cam < 2 && cl < cn) {
                const size_t g = c0 + b0 + cl;
                double ju[16], jv[16], pu, pv;
                oc_corner<true>(R, Jr, T, q, a.ox[g], a.oy[g], a.oz[g], pu, pv, ju, jv);
                const double eu = iu[g] - pu, ev = iv[g] - pv;
                if (cam == 0) {
                    double* du = JL + 32 * (size_t)cl;
#pragma unroll
                    for (int j = 0; j < 16; ++j) { du[j] = ju[j]; du[16 + j] = jv[j]; }
                    eL[2 * cl] = eu;
                    eL[2 * cl + 1] = ev;
                } else {
                    double h0[16], h1[16];
                    double* d0 = JR0 + 32 * (size_t)cl;
                    double* d1 = JR1 + 32 * (size_t)cl;
                    os_right_row(ju, CT, h0, h1);
#pragma unroll
                    for (int j = 0; j < 16; ++j) { d0[j] = h0[j]; d1[j] = h1[j]; }
                    os_right_row(jv, CT, h0, h1);
#pragma unroll
                    for (int j = 0; j < 16; ++j) { d0[16 + j] = h0[j]; d1[16 + j] = h1[j]; }
                    eR[2 * cl] = eu;
                    eR[2 * cl + 1] = ev;
                }
            }
            for (int r = rows + tid; r < rows4; r += 256) {   // zero rows pad the last block of 4
#pragma unroll
                for (int j = 0; j < 16; ++j) JL[16 * r + j] = JR0[16 * r + j] = JR1[16 * r + j] = 0.0;
                eL[r] = eR[r] = 0.0;
            }
            __syncthreads();
            const int nblk = rows4 >> 2;
            for (int b = wave; b < nblk; b += 4) {
                const int r = 4 * b + rr;
                const double av = JL[16 * r + cc];   // A[cc][rr] = J[r][cc] = B[rr][cc]
                aLL = __builtin_amdgcn_mfma_f64_16x16x4f64(av, av, aLL, 0, 0, 0);
                jL += av * eL[r];
            }
            for (int b = wave; b < nblk; b += 4) {
                const int r = 4 * b + rr;
                const double v0 = JR0[16 * r + cc], v1 = JR1[16 * r + cc], e = eR[r];
                a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(v0, v0, a00, 0, 0, 0);
                a01 = __builtin_amdgcn_mfma_f64_16x16x4f64(v0, v1, a01, 0, 0, 0);
                a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(v1, v1, a11, 0, 0, 0);
                j0 += v0 * e;
                j1 += v1 * e;
            }
            __syncthreads();   // the next chunk (or the tiles below) overwrite the rows
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int o = wave * 1024 + (rr + 4 * i) * 16 + cc;
        Cp[o] = aLL[i];
        Cp[256 + o] = a00[i];
        Cp[512 + o] = a01[i];
        Cp[768 + o] = a11[i];
    }
    jp[wave * 192 + lane] = jL;
    jp[wave * 192 + 64 + lane] = j0;
    jp[wave * 192 + 128 + lane] = j1;
    __syncthreads();
    // the 32 x 32 strip Gram [pose | om, T | intr_1 | intr_2] from the tiles, waves in order; fixed
    // intrinsics (flags2idxStereo) drop out: subMatrix as a 0/1 mask of rows and columns
    for (int e = tid; e < 1024; e += 256) {
        const int i = e >> 5, j = e & 31;
        const int li = i < 6 ? i : (i >= 12 && i < 22 ? i - 6 : -1), lj = j < 6 ? j : (j >= 12 && j < 22 ? j - 6 : -1);
        const int ti = i < 12 ? 0 : (i >= 22 ? 1 : -1), tj = j < 12 ? 0 : (j >= 22 ? 1 : -1);
        const int ci = i < 12 ? i : i - 22, cj = j < 12 ? j : j - 22;
        double s = 0.0;
        if (li >= 0 && lj >= 0) {
            const int o = li * 16 + lj;
            s = ((Cp[o] + Cp[1024 + o]) + Cp[2048 + o]) + Cp[3072 + o];
        }
        if (ti >= 0 && tj >= 0) {
            const int o = ti == 0 ? (tj == 0 ? 256 + ci * 16 + cj : 512 + ci * 16 + cj)
                                  : (tj == 0 ? 512 + cj * 16 + ci : 768 + ci * 16 + cj);
            s += ((Cp[o] + Cp[1024 + o]) + Cp[2048 + o]) + Cp[3072 + o];
        }
        const double mi = i < 6 ? 1.0 : msk[i - 6], mj = j < 6 ? 1.0 : msk[j - 6];
        C[e] = s * (mi * mj);
    }
    if (tid < 32) {
        const int i = tid;
        const int li = i < 6 ? i : (i >= 12 && i < 22 ? i - 6 : -1);
        const int ti = i < 12 ? 0 : (i >= 22 ? 1 : -1), ci = i < 12 ? i : i - 22;
        double s = 0.0;
        if (li >= 0) {
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int q = 0; q < 4; ++q) s += jp[w * 192 + q * 16 + li];
        }
        if (ti >= 0) {
            double s2 = 0.0;
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int q = 0; q < 4; ++q) s2 += jp[w * 192 + 64 + ti * 64 + q * 16 + ci];
            s += s2;
        }
        je_raw[i] = s;   // J^T E before the reduction (computeJacobianStereo's JTE)
        je[i] = i < 6 ? s : s * msk[i - 6];
    }
    __syncthreads();

    // ---- phase C: U^-1 (wave 0 register Gauss-Jordan), Schur pieces
    if (wave == 0) {
        const int li = lane < 6 ? lane : 0;
        double row[12];
#pragma unroll
        for (int j = 0; j < 6; ++j) { row[j] = C[li * 32 + j]; row[6 + j] = li == j ? 1.0 : 0.0; }
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
        if (bad && lane == 0) atomicOr(&st->error, 1);
    }
    __syncthreads();
    if (tid < kOsY) {   // Y = U^-1 W (6 x 26), W = C[0:6, 6:32]
        const int i = tid / kOsG, j = tid % kOsG;
        double y = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) y += Ui[i * 6 + k] * C[k * 32 + 6 + j];
        Yl[tid] = y;
        a.Yv[kOsY * (size_t)v + tid] = y;
    } else if (tid >= 192 && tid < 198) {
        a.zb[6 * (size_t)v + tid - 192] = zbl[tid - 192];
    } else if (tid >= 198 && tid < 204) {
        a.zu[6 * (size_t)v + tid - 198] = zul[tid - 198];
    } else if (tid >= 204 && tid < 210) {
        a.jte[6 + 6 * (size_t)v + tid - 204] = je[tid - 204];
    }
    __syncthreads();
    double* out = a.contrib + (size_t)v * kOsLc;
    for (int e = tid; e < kOsLc; e += 256) {
        double s = 0.0;
        if (e < kOsRb) {
            int i = 0, rem = e;
            while (rem >= kOsG - i) { rem -= kOsG - i; ++i; }
            const int j = i + rem;
            s = C[(6 + i) * 32 + 6 + j];
#pragma unroll
            for (int k = 0; k < 6; ++k) s -= C[k * 32 + 6 + i] * Yl[k * kOsG + j];
        } else if (e < kOsWu) {
            const int j = e - kOsRb;
            s = je[6 + j];
#pragma unroll
            for (int k = 0; k < 6; ++k) s -= C[k * 32 + 6 + j] * zbl[k];
        } else if (e < kOsJc) {
            const int j = e - kOsWu;
#pragma unroll
            for (int k = 0; k < 6; ++k) s += C[k * 32 + 6 + j] * zul[k];
        } else if (e < kOsAb) {
            s = je_raw[6 + e - kOsJc];
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k)
                s += e == kOsAb ? zbl[k] : e == kOsAu ? zul[k] : e == kOsNg ? nrm[0][k] : nrm[1][k];
        }
        oc_st(out + e, s);
    }

    // ---- two-level fixed-order reduction of the contributions
    const int grp = v / a.group_size, g0 = grp * a.group_size, gn = min(a.group_size, n - g0);
    if (!oc_arrive(&a.cnt[grp], gn)) return;
    for (int e = tid; e < kOsLc; e += 256)
        oc_st(a.gsum + (size_t)grp * kOsLc + e, os_sum(a.contrib + (size_t)g0 * kOsLc + e, gn));
    if (!oc_arrive(&a.cnt[a.n_groups], a.n_groups)) return;
    for (int e = tid; e < kOsLc; e += 256) tot[e] = os_sum(a.gsum + e, a.n_groups);
    __syncthreads();
    if (wave != 0) return;

    // ---- final: stop test (:1276-1279), reduced solve, Sherman-Morrison, global update (wave 0)
    const int k = st->iter;
    double change = st->change;
    if (pending) change = sqrt(tot[kOsNg] + st->normG2_c) / sqrt(tot[kOsNx] + st->normX2_c);
    const int ct = st->crit_type;
    const bool stop = (ct == 1 && k >= st->max_count) || (ct == 2 && change <= st->eps) ||
                      (ct == 3 && (change <= st->eps || k >= st->max_count));
    if (lane == 0) st->change = change;
    if (stop) {
        if (lane == 0) { st->done = 1; st->pending = 0; }
        return;
    }
    const double alpha2 = 1.0 - pow(1.0 - 0.01, (double)k + 1.0);   // alpha_smooth2 (:1280)
    const double epsilon = 0.01 * pow(0.9, (double)k / 10);          // (:1282)
    const int li = lane < kOsG ? lane : 0;
    const bool free_i = msk[li] != 0.0;
    double row[kOsG + 2];
#pragma unroll
    for (int j = 0; j < kOsG; ++j) {
        const double sv = tot[kOsS + (li <= j ? os_up(li, j) : os_up(j, li))];
        row[j] = free_i ? sv : (j == li ? 1.0 : 0.0);
    }
    row[kOsG] = free_i ? tot[kOsRb + li] : 0.0;
    row[kOsG + 1] = free_i ? 1.0 - tot[kOsWu + li] : 0.0;
    // Gauss-Jordan, lane l keeps row l, as k_oc_step's 10 x 10: the diagonal in natural order while
    // it is positive, else the unused row of largest |entry|; an exactly singular system gives
    // G = 0 for the whole step, as the reference's Mat::inv() (DECOMP_LU) returns a zero matrix then
    bool used = lane >= kOsG, singular = false;
    int pcol = -1;
    double dii = 1.0;
#pragma unroll
    for (int kk = 0; kk < kOsG; ++kk) {
        int pl = kk;
        if (!(oc_readlane(row[kk], kk) > 0.0) || __builtin_amdgcn_readlane((int)used, kk) != 0) {
            pl = -1;
            double best = 0.0;
#pragma nounroll
            for (int l = 0; l < kOsG; ++l) {
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
        double pr[kOsG + 2];
#pragma unroll
        for (int j = kk + 1; j < kOsG + 2; ++j) pr[j] = oc_readlane(row[j], pl);
#pragma unroll
        for (int j = kk + 1; j < kOsG + 2; ++j) row[j] -= f * pr[j];
    }
    // lane j takes the solution of column j from the lane that pivoted it
    const double sb = lane < kOsG && !singular ? row[kOsG] / dii : 0.0;
    const double su = lane < kOsG && !singular ? row[kOsG + 1] / dii : 0.0;
    double yb = 0.0, yu = 0.0;
#pragma nounroll
    for (int j = 0; j < kOsG; ++j) {
        const unsigned long long own = __ballot(pcol == j);
        const int src = own ? (int)__builtin_ctzll(own) : 0;
        const double vb = oc_readlane(sb, src), vu = oc_readlane(su, src);
        if (lane == j) { yb = vb; yu = vu; }
    }
    // 1^T A^-1 b = sum_v 1^T U^-1 rp_v - (sum_v W_v^T U^-1 1)^T yb + 1_free^T yb (and for u)
    const double wm = lane < kOsG ? msk[lane] - tot[kOsWu + lane] : 0.0;
    double s1 = tot[kOsAb], s2 = tot[kOsAu];
#pragma unroll
    for (int l = 0; l < kOsG; ++l) {
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
    if (lane < kOsG) {
        const size_t gi = os_gidx(lane, n);
        xo = a.x[gi];
        a.x[gi] = xo + gc;
        a.yc[lane] = yc;
        a.G[gi] = gc;
        a.jte[gi] = tot[kOsJc + lane];
    }
#pragma unroll
    for (int l = 0; l < kOsG; ++l) {
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

// estimateUncertaintiesStereo's squared reprojection errors of both cameras, per view (:1826-1864)
__global__ __launch_bounds__(64) void k_os_err(OsErrArgs a) {
    const int v = blockIdx.x, lane = threadIdx.x;
    const int n = a.n, np = a.np;
    const size_t c0 = (size_t)v * np;
    const double* pose = a.x + 6 + 6 * (size_t)v;
    double R1[9], J1[9], R3[9], J3[9], T3[3], R2[9];
    oc_pose(pose, R1, J1);
    const double T1[3] = {pose[3], pose[4], pose[5]};
    Motion m;
    os_right_pose(pose, a.x, R3, J3, T3, m, R2);
    const double* q1 = a.x + 6 * (size_t)(n + 1);
    const double* q2 = q1 + 10;
    const OcIntr i1{q1[0], q1[1], q1[2], q1[3], q1[4], q1[5], q1[6], q1[7], q1[8], q1[9]};
    const OcIntr i2{q2[0], q2[1], q2[2], q2[3], q2[4], q2[5], q2[6], q2[7], q2[8], q2[9]};
    double s = 0.0;
    for (int c = lane; c < np; c += 64) {
        const size_t g = c0 + c;
        double pu, pv;
        oc_corner<false>(R1, J1, T1, i1, a.ox[g], a.oy[g], a.oz[g], pu, pv, nullptr, nullptr);
        const double ex = a.iu1[g] - pu, ey = a.iv1[g] - pv;
        oc_corner<false>(R3, J3, T3, i2, a.ox[g], a.oy[g], a.oz[g], pu, pv, nullptr, nullptr);
        const double fx = a.iu2[g] - pu, fy = a.iv2[g] - pv;
        s += (ex * ex + ey * ey) + (fx * fx + fy * fy);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) a.view_sq[v] = s;
}

}  // namespace mcc

size_t mcc_os_shmem(int chunk) { return sizeof(double) * 100 * (size_t)chunk; }

hipError_t mcc_os_set_attrs(int chunk) {
    return hipFuncSetAttribute((const void*)mcc::k_os_step, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)mcc_os_shmem(chunk));
}

hipError_t mcc_launch_os_step(const mcc::OsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mcc::k_os_step, dim3(a.n), dim3(256), mcc_os_shmem(a.chunk), s, a);
    return hipGetLastError();
}

hipError_t mcc_launch_os_err(const mcc::OsErrArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mcc::k_os_err, dim3(a.n), dim3(64), 0, s, a);
    return hipGetLastError();
}
