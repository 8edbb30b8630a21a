// mcc_pincalib.hip -- pinhole calibrateCamera for gfx950 (mcc_calibrate_camera, include/mcc.h): the
// Levenberg-Marquardt loop over (fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 | one pose per view).
//
// One trial is two launches, one wave64 (one 64-thread workgroup) per view in both:
//   k_pc_lin   linearises the view at the current parameters (three VALU passes over its corners,
//              mcc_pincalib_device.hpp; after a rejected trial the stored sums are reused), damps and
//              eliminates its 6 x 6 pose block, keeps Y_v, z_v for the back-substitution and writes its
//              contribution to the reduced 12 x 12 system.  The contributions are summed in view order
//              by a two-level last-arriver ticket (pin_reduce, mcc_pinloop_device.hpp); the last arriver
//              solves the reduced system for the global step dc.
//   k_pc_try   back-substitutes the view's pose step, evaluates the squared error of the trial
//              parameters and sums it over the views the same way (pin_sum_err); the last arriver
//              accepts or rejects the trial and runs the stop tests (pin_verdict; the policy is pc_next,
//              mcc_pincalib_internal.h).  With st->init it only evaluates the starting point.
// The sums and the verdict are shared with mcc_pinstereo.hip; what is this kernel's own in the verdict is
// how the 12 global slots, still live in g and gt, enter the step's norms and are committed.
// No workgroup waits for another: a hand-off is a ticket or the kernel boundary.  The loop state lives
// in PcState; a launch after `done` returns at once, so the host enqueues trials in batches.
// Hand-offs inside a launch are 8-byte sc1 stores and loads around oc_arrive (mcc_omnicalib_device.hpp).
#include <hip/hip_runtime.h>

#include "mcc_omnicalib_device.hpp"
#include "mcc_pincalib_device.hpp"
#include "mcc_pincalib_internal.h"
#include "mcc_pinloop_device.hpp"

namespace mcc {

static_assert(PcLin::N == kPcLinN && PcCtr::N == kPcCtrN && kPcG == kPcGlob, "layouts of mcc_pincalib_internal.h");

__global__ __launch_bounds__(64) void k_pc_lin(PcArgs a) {
    PcState* st = a.st;
    if (st->done) return;
    const int v = blockIdx.x, lane = threadIdx.x;
    __shared__ double L[PcLin::N], Yz[kPcYz], ctr[PcCtr::N], tot[PcCtr::N];
    const int off = a.view_off[v], n = a.view_off[v + 1] - off;
    const double lambda = st->lambda;
    double* lin = a.lin + (size_t)v * kPcLinN;
    if (st->relin) {
        double g[kPcG];
#pragma unroll
        for (int k = 0; k < kPcG; ++k) g[k] = a.glob[k];
        const double* p = a.x + 6 * (size_t)v;
        const double r[3] = {p[0], p[1], p[2]}, t[3] = {p[3], p[4], p[5]};
        pc_linearize(a.obj + 3 * (size_t)off, a.img + 2 * (size_t)off, n, pc_cam(g), a.mask, a.aspect, r, t, lane, L);
        pnp_wave_sync();
        for (int i = lane; i < PcLin::N; i += 64) lin[i] = L[i];
    } else {
        for (int i = lane; i < PcLin::N; i += 64) L[i] = lin[i];
        pnp_wave_sync();
    }
    pc_eliminate(L, lambda, lane, Yz, ctr);
    for (int i = lane; i < kPcYz; i += 64) a.Yz[(size_t)v * kPcYz + i] = Yz[i];
    for (int e = lane; e < PcCtr::N; e += 64) oc_st(a.contrib + (size_t)v * PcCtr::N + e, ctr[e]);

    if (!pin_reduce<PcCtr::N>(a, v, lane, tot)) return;
    double dc[kPcG];
    const bool ok = pc_reduced_solve(tot, lambda, a.mask, dc);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kPcG; ++k) a.dc[k] = dc[k];
        st->fail = ok ? 0 : 1;
    }
}

__global__ __launch_bounds__(64) void k_pc_try(PcArgs a) {
    PcState* st = a.st;
    if (st->done) return;
    const int v = blockIdx.x, lane = threadIdx.x;
    const int init = st->init;
    const int off = a.view_off[v], n = a.view_off[v + 1] - off;
    double g[kPcG], dc[kPcG], gt[kPcG];
#pragma unroll
    for (int k = 0; k < kPcG; ++k) {
        g[k] = a.glob[k];
        dc[k] = init ? 0.0 : a.dc[k];
    }
    pc_apply(g, dc, a.aspect, gt);
    const double* p = a.x + 6 * (size_t)v;
    const double r[3] = {p[0], p[1], p[2]}, t[3] = {p[3], p[4], p[5]};
    double rn[3] = {r[0], r[1], r[2]}, tn[3] = {t[0], t[1], t[2]};
    if (!init) pc_trial_pose(r, t, a.Yz + (size_t)v * kPcYz, dc, rn, tn);
    const double sq = pc_sumsq(pc_cam(gt), rn, tn, a.obj + 3 * (size_t)off, a.img + 2 * (size_t)off, n, lane);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            oc_st(a.xt + 6 * (size_t)v + k, rn[k]);
            oc_st(a.xt + 6 * (size_t)v + 3 + k, tn[k]);
        }
        oc_st(a.esq_t + v, sq);
    }
    double en;
    if (!pin_sum_err<1>(a, v, lane, en)) return;
    pin_verdict<1>(a, lane, init, en, [&](double& dn, double& xn) {
#pragma unroll
        for (int k = 0; k < kPcG; ++k) {
            const double d = gt[k] - g[k];
            dn += d * d;
            xn += g[k] * g[k];
            if (lane == 0) a.glob[k] = gt[k];
        }
    });
}

}  // namespace mcc

hipError_t mcc_launch_pc_lin(const mcc::PcArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mcc::k_pc_lin, dim3(a.n), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t mcc_launch_pc_try(const mcc::PcArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mcc::k_pc_try, dim3(a.n), dim3(64), 0, s, a);
    return hipGetLastError();
}
