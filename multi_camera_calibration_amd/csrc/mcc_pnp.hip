// mcc_pnp.hip -- batched solvePnP for gfx950 (mcc_solve_pnp_batch, include/mcc.h).
//
//   k_pnp   one wave64 per view, the whole of host/pnp.cpp's solvePnP including the Levenberg-
//           Marquardt loop in one launch (mcc_pnp_device.hpp).  Waves never meet: no workgroup
//           barrier, no atomics, so a view's result does not depend on the rest of the batch.
//
// LDS: a view's slice is its undistorted corners xy [2 max_n] and the DLT's normal matrix and
// eigenvectors A [144], V [144] (12 x 12; the homography's 9 x 9 uses the front of them), all double:
// (2 max_n + 288) * 8 bytes, 18 688 for the largest view (1 024 corners).  The rule for views per
// workgroup: as many slices as fit the 64 KB a workgroup gets without opting in to more, at most 4
// (one wave per SIMD, so each wave keeps the SIMD's whole register file): 3 at max_n = 1 024, 4 up to
// max_n = 880.
#include <hip/hip_runtime.h>

#include "mcc_pnp_device.hpp"
#include "mcc_pnp_internal.h"

namespace mcc {

constexpr int kPnpLdsBytes = 64 * 1024;
constexpr int kPnpMaxWaves = 4;

__host__ __device__ inline int pnp_view_doubles(int max_n) { return 2 * max_n + 288; }

__global__ __launch_bounds__(64 * kPnpMaxWaves) void k_pnp(PnpArgs a) {
    extern __shared__ double pnp_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int v = pnp_uniform((int)(blockIdx.x * (blockDim.x >> 6) + wave));
    if (v >= a.n_views) return;   // a whole wave; nothing below waits for another wave
    double* xy = pnp_lds + (size_t)wave * pnp_view_doubles(a.max_n);
    double* A = xy + 2 * a.max_n;
    double* V = A + 144;
    const int off = a.view_off[v], n = a.view_off[v + 1] - off;
    const int cam = a.view_cam ? a.view_cam[v] : 0;
    const double* K = a.K + 9 * cam;
    const double* D = a.D + kPnpDist * cam;
    const PnpCam c{K[0], K[4], K[2], K[5], D[0], D[1], D[2], D[3], D[4], D[5], D[6], D[7], D[8], D[9], D[10], D[11]};
    double r[3], t[3], rms;
    const int status = pnp_solve_view(a.obj + 3 * (size_t)off, a.img + 2 * (size_t)off, n, c, a.max_iter, xy, A, V,
                                      lane, r, t, rms);
    if (lane == 0) {
        const bool ok = status == kPnpSolved;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a.rvec[3 * v + k] = ok ? r[k] : 0.0;
            a.tvec[3 * v + k] = ok ? t[k] : 0.0;
        }
        a.rms[v] = ok ? rms : -1.0;
        a.status[v] = status;
    }
}

}  // namespace mcc

hipError_t mcc_launch_pnp(const mcc::PnpArgs& a, hipStream_t s) {
    const int bytes = mcc::pnp_view_doubles(a.max_n) * (int)sizeof(double);
    int waves = mcc::kPnpLdsBytes / bytes;
    waves = waves < 1 ? 1 : waves > mcc::kPnpMaxWaves ? mcc::kPnpMaxWaves : waves;
    const int blocks = (a.n_views + waves - 1) / waves;
    hipLaunchKernelGGL(mcc::k_pnp, dim3(blocks), dim3(64 * waves), (size_t)waves * bytes, s, a);
    return hipGetLastError();
}
