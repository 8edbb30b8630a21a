// mcc_omnicalib.hip -- CDNA4 kernels of the omnidir intrinsic calibration (cv::omnidir::calibrate,
// src/omnidir.cpp:1067-1211).
//
// One loop step of calibrate = one launch of k_oc_step, one 256-thread workgroup per view.  The
// loop itself (pending pose update, pose-block inverse, Schur contribution, reduction, reduced
// solve and update) is the shared block-arrow step of mcc_omnicalib_device.hpp with G = 10; this
// file has what is the single camera's own:
//   phase A  every thread projects its corners with the Mei model and writes the 2 x 16 rows of
//            [d/d(om, T) | d/d(fx, fy, s, cx, cy, xi, k1, k2, p1, p2)] (JacobianRow order,
//            src/omnidir.cpp:65-73) and E = img - proj into LDS;
//   phase B  the 16 x 16 Gram J^T J of the view's 2N x 16 strip on the matrix cores: every wave
//            takes every 4th block of 4 rows and issues v_mfma_f64_16x16x4_f64 with the same
//            register as A (J^T, 16 x 4) and B (J, 4 x 16); J^T E rides along as one VALU FMA;
//            the four waves' partial tiles are summed in LDS in wave order, and the rows / columns
//            of fixed intrinsics (flags2idx) masked to 0 (subMatrix).
// FP64 throughout, like the reference (calibrate converts its inputs to CV_64F, :1083-1094).
#include <hip/hip_runtime.h>

#include "mcc_device.hpp"
#include "mcc_omnicalib_device.hpp"
#include "mcc_omnicalib_internal.h"

namespace mcc {

// x = [om_0, T_0, ... | intrinsics] (encodeParameters, :1530-1568)
struct OcPos {
    int n;
    __device__ size_t pose(int v) const { return 6 * (size_t)v; }
    __device__ size_t glob(int l) const { return 6 * (size_t)n + l; }
};

__global__ __launch_bounds__(256) void k_oc_step(OcArgs a) {
    if (a.lp.st->done) return;
    const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const OcPos pos{a.lp.n};
    const int c0 = a.view_off[v], np = a.view_off[v + 1] - c0;
    const int rows = 2 * np, rows4 = (rows + 3) & ~3, r4max = (2 * a.max_np + 3) & ~3;
    extern __shared__ double sm[];
    double* Jl = sm;                  // [r4max][16]
    double* el = Jl + 16 * r4max;     // [r4max]
    double* Cp = el + r4max;          // [4][256] per-wave Gram tiles
    double* jp = Cp + 1024;           // [4][64]  per-wave J^T E partials
    __shared__ double pose[6], intr[10], msk[10], nrm[12];
    __shared__ double C[256], je[16], je_raw[16], Ui[36], zbl[6], zul[6], Yl[60], tot[OcLayout<10>::Lc];

    const int pending = oc_phase0<10>(a.lp, pos, v, pose, nrm, intr, msk);
    __syncthreads();

    // ---- phase A: projection + 2 x 16 Jacobian rows into LDS
    {
        double R[9], Jr[9];
        oc_pose(pose, R, Jr);
        const double T[3] = {pose[3], pose[4], pose[5]};
        const OcIntr q{intr[0], intr[1], intr[2], intr[3], intr[4], intr[5], intr[6], intr[7], intr[8], intr[9]};
        for (int c = tid; c < np; c += 256) {
            const size_t g = (size_t)c0 + c;
            double ju[16], jv[16], pu, pv;
            oc_corner<true>(R, Jr, T, q, a.ox[g], a.oy[g], a.oz[g], pu, pv, ju, jv);
            double* du = Jl + 32 * (size_t)c;
#pragma unroll
            for (int j = 0; j < 16; ++j) { du[j] = ju[j]; du[16 + j] = jv[j]; }
            el[2 * c] = a.iu[g] - pu;
            el[2 * c + 1] = a.iv[g] - pv;
        }
        for (int r = rows + tid; r < rows4; r += 256) {
#pragma unroll
            for (int j = 0; j < 16; ++j) Jl[16 * r + j] = 0.0;
            el[r] = 0.0;
        }
    }
    __syncthreads();

    // ---- phase B: Gram of the 2N x 16 strip on the matrix cores, J^T E on the VALU
    {
        oc_v4d acc = {0.0, 0.0, 0.0, 0.0};
        double jacc = 0.0;
        const int rr = lane >> 4, cc = lane & 15, nblk = rows4 >> 2;
        for (int b = wave; b < nblk; b += 4) {
            const int r = 4 * b + rr;
            const double av = Jl[16 * r + cc];   // A[cc][rr] = J[r][cc] = B[rr][cc]
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, av, acc, 0, 0, 0);
            jacc += av * el[r];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) Cp[wave * 256 + (rr + 4 * i) * 16 + cc] = acc[i];
        jp[wave * 64 + lane] = jacc;
    }
    __syncthreads();
    {   // fixed intrinsics (flags2idx) drop out of the normal equations: subMatrix as a 0/1 mask
        const int i = tid >> 4, j = tid & 15;
        const double mi = i < 6 ? 1.0 : msk[i - 6], mj = j < 6 ? 1.0 : msk[j - 6];
        C[tid] = (((Cp[tid] + Cp[256 + tid]) + Cp[512 + tid]) + Cp[768 + tid]) * (mi * mj);
    }
    if (tid < 16) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int q = 0; q < 4; ++q) s += jp[w * 64 + q * 16 + tid];
        je_raw[tid] = s;   // J^T E before the reduction (computeJacobian's JTE)
        je[tid] = tid < 6 ? s : s * msk[tid - 6];
    }
    __syncthreads();

    oc_pose_inverse<16>(C, je, Ui, zbl, zul, &a.lp.st->error);
    __syncthreads();
    oc_contribute<10, 16>(a.lp, pos, v, C, je, je_raw, Ui, zbl, zul, nrm, Yl);
    oc_reduce_solve<10>(a.lp, pos, v, pending, msk, tot);
}

// estimateUncertainties' squared reprojection errors, per view (src/omnidir.cpp:1766-1803)
__global__ __launch_bounds__(64) void k_oc_err(OcErrArgs a) {
    const int v = blockIdx.x, lane = threadIdx.x;
    const int c0 = a.view_off[v], np = a.view_off[v + 1] - c0;
    const double* pose = a.x + 6 * (size_t)v;
    double R[9], Jr[9];
    oc_pose(pose, R, Jr);
    const double T[3] = {pose[3], pose[4], pose[5]};
    const double* qi = a.x + 6 * (size_t)a.n;
    const OcIntr q{qi[0], qi[1], qi[2], qi[3], qi[4], qi[5], qi[6], qi[7], qi[8], qi[9]};
    double s = 0.0;
    for (int c = lane; c < np; c += 64) {
        const size_t g = (size_t)c0 + c;
        double pu, pv;
        oc_corner<false>(R, Jr, T, q, a.ox[g], a.oy[g], a.oz[g], pu, pv, nullptr, nullptr);
        const double ex = a.iu[g] - pu, ey = a.iv[g] - pv;
        s += ex * ex + ey * ey;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) a.view_sq[v] = s;
}

}  // namespace mcc

size_t mcc_oc_shmem(int max_np) {
    const size_t r4 = (size_t)((2 * max_np + 3) & ~3);
    return sizeof(double) * (17 * r4 + 1024 + 256);
}

hipError_t mcc_oc_set_attrs(int max_np) {
    return hipFuncSetAttribute((const void*)mcc::k_oc_step, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)mcc_oc_shmem(max_np));
}

hipError_t mcc_launch_oc_step(const mcc::OcArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mcc::k_oc_step, dim3(a.lp.n), dim3(256), mcc_oc_shmem(a.max_np), s, a);
    return hipGetLastError();
}

hipError_t mcc_launch_oc_err(const mcc::OcErrArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mcc::k_oc_err, dim3(a.n), dim3(64), 0, s, a);
    return hipGetLastError();
}
