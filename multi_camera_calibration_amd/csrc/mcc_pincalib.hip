// mcc_pincalib.hip -- pinhole calibrateCamera for gfx950 (mcc_calibrate_camera, include/mcc.h): the
// Levenberg-Marquardt loop over (fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 | one pose per view).
//
// One trial is two launches, one wave64 (one 64-thread workgroup) per view in both:
//   k_pc_lin   linearises the view at the current parameters (three VALU passes over its corners,
//              mcc_pincalib_device.hpp; after a rejected trial the stored sums are reused), damps and
//              eliminates its 6 x 6 pose block, keeps Y_v, z_v for the back-substitution and writes its
//              contribution to the reduced 12 x 12 system.  The contributions are summed in view order
//              by a two-level last-arriver ticket (groups of ~sqrt(n) views, then the groups, as the
//              omnidir loop's OcLayout / gsum); the last arriver solves the reduced system for the
//              global step dc.
//   k_pc_try   back-substitutes the view's pose step, evaluates the squared error of the trial
//              parameters and sums it over the views the same way; the last arriver accepts the trial
//              (en <= err: parameters, error and lambda / 10) or rejects it (lambda x 10) and runs the
//              stop tests.  With st->init it only evaluates the starting point.
// No workgroup waits for another: a hand-off is a ticket or the kernel boundary.  The loop state lives
// in PcState; a launch after `done` returns at once, so the host enqueues trials in batches.
// Hand-offs inside a launch are 8-byte sc1 stores and loads around oc_arrive (mcc_omnicalib_device.hpp).
#include <hip/hip_runtime.h>

#include "mcc_omnicalib_device.hpp"
#include "mcc_pincalib_device.hpp"
#include "mcc_pincalib_internal.h"

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

    const int grp = v / a.group_size, g0 = grp * a.group_size, gn = min(a.group_size, a.n - g0);
    if (!oc_arrive(&a.cnt[grp], gn)) return;
    for (int e = lane; e < PcCtr::N; e += 64)
        oc_st(a.gsum + (size_t)grp * PcCtr::N + e, oc_sum<PcCtr::N>(a.contrib + (size_t)g0 * PcCtr::N + e, gn));
    if (!oc_arrive(&a.cnt[a.n_groups], a.n_groups)) return;
    for (int e = lane; e < PcCtr::N; e += 64) tot[e] = oc_sum<PcCtr::N>(a.gsum + e, a.n_groups);
    __syncthreads();
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
    int* cnt = a.cnt + a.n_groups + 1;
    const int grp = v / a.group_size, g0 = grp * a.group_size, gn = min(a.group_size, a.n - g0);
    if (!oc_arrive(&cnt[grp], gn)) return;
    {
        const double gs = oc_sum<1>(a.esq_t + g0, gn);
        if (lane == 0) oc_st(a.egs + grp, gs);
    }
    if (!oc_arrive(&cnt[a.n_groups], a.n_groups)) return;
    const double en = oc_sum<1>(a.egs, a.n_groups);

    // ---- the last arriver: accept or reject, stop tests
    const int iter = st->iter, tries = st->tries, trials = st->trials, fail = st->fail;
    const int crit = st->crit_type, max_count = st->max_count;
    const double eps = st->eps, lambda = st->lambda, err = st->err;
    if (init) {
        for (int i = lane; i < a.n; i += 64) a.esq[i] = oc_ld(a.esq_t + i);
        if (lane == 0) {
            st->err = en;
            st->init = 0;
            st->relin = 1;
            if (!(fabs(en) < 1.7e308)) { st->done = 1; st->status = kPcNotFinite; }
        }
        return;
    }
    const bool accept = !fail && en <= err;   // (a NaN error is a rejection)
    if (!accept) {
        if (lane == 0) {
            st->trials = trials + 1;
            st->lambda = lambda * 10.0;
            st->tries = tries + 1;
            st->relin = 0;
            if (tries + 1 >= 10) { st->done = 1; st->status = kPcStalled; }
        }
        return;
    }
    double dn = 0.0, xn = 0.0;
    for (int i = lane; i < 6 * a.n; i += 64) {
        const double xo = a.x[i], xw = oc_ld(a.xt + i), d = xw - xo;
        dn += d * d;
        xn += xo * xo;
        a.x[i] = xw;
    }
    dn = pnp_wave_sum(dn);
    xn = pnp_wave_sum(xn);
#pragma unroll
    for (int k = 0; k < kPcG; ++k) {
        const double d = gt[k] - g[k];
        dn += d * d;
        xn += g[k] * g[k];
        if (lane == 0) a.glob[k] = gt[k];
    }
    for (int i = lane; i < a.n; i += 64) a.esq[i] = oc_ld(a.esq_t + i);
    const double change = sqrt(dn) / sqrt(xn);
    if (lane == 0) {
        st->trials = trials + 1;
        st->iter = iter + 1;
        st->tries = 0;
        st->relin = 1;
        st->err = en;
        st->change = change;
        st->lambda = fmax(lambda * 0.1, 1e-12);
        if ((crit & 2) && change < eps) { st->done = 1; st->status = kPcConverged; }
        else if ((crit & 1) && iter + 1 >= max_count) { st->done = 1; st->status = kPcCount; }
    }
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
