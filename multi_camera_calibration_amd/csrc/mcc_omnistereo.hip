// mcc_omnistereo.hip -- CDNA4 kernels of the two-camera omnidir calibration
// (cv::omnidir::stereoCalibrate, src/omnidir.cpp:1213-1381; computeJacobianStereo, :937-1020).
//
// Parameters (encodeParametersStereo, :1570-1619): x = [om, T | omL_0, tL_0, ... | intr_1 | intr_2],
// P = 6(n+1) + 20.  View i contributes 4N rows: 2N of camera 1 at pose (omL_i, tL_i) and 2N of
// camera 2 at compose_motion(omL_i, tL_i, om, T).  Its column strip is
//   [own pose 6 | om, T 6 | intr_1 10 | intr_2 10]           (32 columns)
// and the normal matrix is block-arrow: n pose blocks of 6 x 6 and one dense global block of 26.
//
// One loop step = one launch of k_os_step, one 256-thread workgroup per view.  The loop itself is
// the shared block-arrow step of mcc_omnicalib_device.hpp with G = 26; this file has what is the
// two cameras' own:
//   pose     wave 0: R, Jl of the left pose; wave 1: the composed right pose (device compose(), with
//            cvRodrigues2's theta ~ pi zeroing of d om3 / d om) and the four chain-rule blocks;
//   phase A  the corners go through in chunks of 64 or 128: thread (camera, corner) projects with
//            oc_corner<true>; left rows keep [pose | intr_1] (16 columns); right rows apply the chain
//            rule of :999-1002 and keep [pose | om, T | 0 x 4] and [intr_2 | 0 x 6] (2 x 16 columns);
//   phase B  per chunk, the Gram of the left rows (one 16 x 16 tile) and of the right rows (three of
//            the 2 x 2 tiles) with v_mfma_f64_16x16x4_f64, accumulated in registers over the chunks;
//            the columns a row half does not touch are never multiplied.  J^T E on the VALU.  The
//            waves' tiles are summed in wave order into the 32 x 32 strip Gram, fixed intrinsics masked.
#include <hip/hip_runtime.h>

#include "mcc_device.hpp"
#include "mcc_omnicalib_device.hpp"
#include "mcc_omnistereo_internal.h"

namespace mcc {

// x = [om, T | omL_0, tL_0, ... | intr_1 | intr_2]; the global block is [om, T | intr_1 | intr_2]
struct OsPos {
    int n;
    __device__ size_t pose(int v) const { return 6 + 6 * (size_t)v; }
    __device__ size_t glob(int l) const { return l < 6 ? (size_t)l : 6 * (size_t)(n + 1) + (l - 6); }
};

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
    if (a.lp.st->done) return;
    const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int np = a.np, ch = a.chunk;
    const OsPos pos{a.lp.n};
    const size_t c0 = (size_t)v * np;
    extern __shared__ double sm[];
    double* JL = sm;                   // [2 ch][16] left rows  [pose 6 | intr_1 10]
    double* JR0 = JL + 32 * ch;        // [2 ch][16] right rows [pose 6 | om, T 6 | 0 x 4]
    double* JR1 = JR0 + 32 * ch;       // [2 ch][16] right rows [intr_2 10 | 0 x 6]
    double* eL = JR1 + 32 * ch;        // [2 ch]
    double* eR = eL + 2 * ch;          // [2 ch]
    double* Cp = sm;                   // after the last chunk: [4 waves][LL, R00, R01, R11][256]
    double* jp = sm + 4096;            //                       [4 waves][L, R0, R1][64]
    __shared__ double pose[6], glob[kOsG], msk[kOsG], nrm[12], PL[kPoseTab], PR[kPoseTab], CT[kChainTab];
    __shared__ double C[1024], je[32], je_raw[32], Ui[36], zbl[6], zul[6], Yl[6 * kOsG], tot[OcLayout<kOsG>::Lc];

    const int pending = oc_phase0<kOsG>(a.lp, pos, v, pose, nrm, glob, msk);
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

    oc_pose_inverse<32>(C, je, Ui, zbl, zul, &a.lp.st->error);
    __syncthreads();
    oc_contribute<kOsG, 32>(a.lp, pos, v, C, je, je_raw, Ui, zbl, zul, nrm, Yl);
    oc_reduce_solve<kOsG>(a.lp, pos, v, pending, msk, tot);
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
    hipLaunchKernelGGL(mcc::k_os_step, dim3(a.lp.n), dim3(256), mcc_os_shmem(a.chunk), s, a);
    return hipGetLastError();
}

hipError_t mcc_launch_os_err(const mcc::OsErrArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mcc::k_os_err, dim3(a.n), dim3(64), 0, s, a);
    return hipGetLastError();
}
