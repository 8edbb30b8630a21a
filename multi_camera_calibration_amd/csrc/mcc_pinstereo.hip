// mcc_pinstereo.hip -- pinhole stereoCalibrate for gfx950 (mcc_stereo_calibrate, include/mcc.h): the
// Levenberg-Marquardt loop over (om T | camera 1's 12 slots | camera 2's 12 slots | one pose per view), the
// second camera seeing view v at R(om) R_v, R(om) t_v + T.
//
// One trial is two launches, one wave64 (one 64-thread workgroup) per view in both, as mcc_pincalib.hip's:
//   k_ps_lin   linearises the view in each camera (pc_linearize_rj twice: camera 2 at the composed pose, its
//              rotation columns in the tangent), carries camera 2's sums to the view's and the rig's
//              coordinates (ps_assemble, mcc_pinstereo_device.hpp; after a rejected trial the stored arrow is
//              reused), damps and eliminates the 6 x 6 pose block and writes the view's contribution to the
//              reduced 30 x 30 system.  The contributions are summed in view order by the two-level
//              last-arriver ticket (pin_reduce, mcc_pinloop_device.hpp); the last arriver solves the reduced
//              system in LDS for the global step dc.
//   k_ps_try   back-substitutes the view's pose step, evaluates both cameras' squared error of the trial
//              parameters and sums it over the views the same way (pin_sum_err, two slots per view); the last
//              arriver accepts or rejects the trial and runs the stop tests (pin_verdict; the policy is
//              pc_next, mcc_pincalib_internal.h), reloading the 30 slots for its share of the step's norms.
//              With st->init it only evaluates the starting point.
// Everything the kernels index dynamically (the sums, the maps, the 30 x 30) is in LDS, never in a lane's
// private arrays.  The loop state is PcState; a launch after `done` returns at once.
#include <hip/hip_runtime.h>

#include "mcc_omnicalib_device.hpp"
#include "mcc_pinstereo_device.hpp"
#include "mcc_pinloop_device.hpp"
#include "mcc_pinstereo_internal.h"

namespace mcc {

static_assert(PsLin::N == kPsLinN && PsCtr::N == kPsCtrN && kPsG == kPsGlob && kPsYzN == kPsYz,
              "layouts of mcc_pinstereo_internal.h");

__global__ __launch_bounds__(64) void k_ps_lin(PsArgs a) {
    PcState* st = a.st;
    if (st->done) return;
    const int v = blockIdx.x, lane = threadIdx.x;
    __shared__ double L[PsLin::N], L12[2 * PcLin::N], tmp[PsTmp::N], Yz[kPsYz], ctr[PsCtr::N], M[kPsG * kPsG],
        b[kPsG], dcs[kPsG], cp[2 * 21];
    constexpr int kCp = 21;   // cp: per camera R [9], Jl [9], t [3]
    const int off = a.view_off[v], n = a.view_off[v + 1] - off;
    const double lambda = st->lambda;
    double* lin = a.lin + (size_t)v * kPsLinN;
    if (st->relin) {
        {   // the two cameras' poses of the view (R, Jl, t each) and the maps, through LDS: nothing of this
            // stays in registers under the passes over the corners
            const double* p = a.x + 6 * (size_t)v;
            const double r[3] = {p[0], p[1], p[2]}, t[3] = {p[3], p[4], p[5]};
            const double om[3] = {a.glob[0], a.glob[1], a.glob[2]}, T[3] = {a.glob[3], a.glob[4], a.glob[5]};
            Rot rv, ro;
            rodrigues_v2m(r, rv);
            rodrigues_v2m(om, ro);
            double Jv[9], Jo[9], R2[9], t2[3];
            so3_jac(r, rv, +1.0, Jv);
            so3_jac(om, ro, +1.0, Jo);
            ps_compose(ro.R, T, rv.R, t, R2, t2);
            ps_maps(ro.R, Jo, Jv, t, lane, tmp);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    cp[k] = rv.R[k];
                    cp[9 + k] = Jv[k];
                    cp[kCp + k] = R2[k];
                    cp[kCp + 9 + k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    cp[18 + k] = t[k];
                    cp[kCp + 18 + k] = t2[k];
                }
            }
            pnp_wave_sync();
        }
#pragma unroll 1
        for (int c = 0; c < 2; ++c) {
            const double* gp = a.glob + kPsCam1 + kPcG * c;
            double g[kPcG], Rc[9], Jc[9], tc[3];
#pragma unroll
            for (int k = 0; k < kPcG; ++k) g[k] = gp[k];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                Rc[k] = pnp_uniform(cp[c * kCp + k]);
                Jc[k] = pnp_uniform(cp[c * kCp + 9 + k]);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) tc[k] = pnp_uniform(cp[c * kCp + 18 + k]);
            pc_linearize_rj(a.obj + 3 * (size_t)off, (c ? a.img2 : a.img1) + 2 * (size_t)off, n, pc_cam(g),
                            ps_lin_mask(a.mask, a.same, c), c ? a.aspect2 : a.aspect1, Rc, Jc, tc, lane,
                            L12 + c * PcLin::N);
        }
        pnp_wave_sync();
        ps_assemble(L12, L12 + PcLin::N, tmp, a.same, lane, L);
        for (int i = lane; i < PsLin::N; i += 64) lin[i] = L[i];
    } else {
        for (int i = lane; i < PsLin::N; i += 64) L[i] = lin[i];
        pnp_wave_sync();
    }
    ps_eliminate(L, lambda, lane, Yz, ctr);
    for (int i = lane; i < kPsYz; i += 64) a.Yz[(size_t)v * kPsYz + i] = Yz[i];
    for (int e = lane; e < PsCtr::N; e += 64) oc_st(a.contrib + (size_t)v * PsCtr::N + e, ctr[e]);

    double* tot = ctr;   // (the view's own contribution has left for global memory)
    if (!pin_reduce<PsCtr::N>(a, v, lane, tot)) return;
    const bool ok = ps_reduced_solve(tot, lambda, a.mask, lane, M, b, dcs);
    if (lane < kPsG) a.dc[lane] = dcs[lane];
    if (lane == 0) st->fail = ok ? 0 : 1;
}

// the current globals g, the trial's step dc (0 with init) and the trial's globals gt
__device__ __forceinline__ void ps_load_trial(const PsArgs& a, int init, double* g, double* dc, double* gt) {
#pragma unroll
    for (int k = 0; k < kPsG; ++k) {
        g[k] = a.glob[k];
        dc[k] = init ? 0.0 : a.dc[k];
    }
    ps_apply(g, dc, a.aspect1, a.aspect2, a.same, gt);
}

__global__ __launch_bounds__(64) void k_ps_try(PsArgs a) {
    PcState* st = a.st;
    if (st->done) return;
    const int v = blockIdx.x, lane = threadIdx.x;
    const int init = st->init;
    const int off = a.view_off[v], n = a.view_off[v + 1] - off;
    double gt[kPsG], rn[3], tn[3];
    {
        double g[kPsG], dc[kPsG];
        ps_load_trial(a, init, g, dc, gt);
        const double* p = a.x + 6 * (size_t)v;
        const double r[3] = {p[0], p[1], p[2]}, t[3] = {p[3], p[4], p[5]};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            rn[k] = r[k];
            tn[k] = t[k];
        }
        if (!init) ps_trial_pose(r, t, a.Yz + (size_t)v * kPsYz, dc, rn, tn);
    }
    double sq1, sq2;
    ps_view_sumsq(gt, rn, tn, a.obj + 3 * (size_t)off, a.img1 + 2 * (size_t)off, a.img2 + 2 * (size_t)off, n, lane, sq1,
                  sq2);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            oc_st(a.xt + 6 * (size_t)v + k, rn[k]);
            oc_st(a.xt + 6 * (size_t)v + 3 + k, tn[k]);
        }
        oc_st(a.esq_t + 2 * (size_t)v, sq1);
        oc_st(a.esq_t + 2 * (size_t)v + 1, sq2);
    }
    double en;
    if (!pin_sum_err<2>(a, v, lane, en)) return;
    pin_verdict<2>(a, lane, init, en, [&](double& dn, double& xn) {
        {   // the globals once more (the same bits), now that the passes over the corners are done with the registers
            double g[kPsG], dc[kPsG];
            ps_load_trial(a, 0, g, dc, gt);
#pragma unroll
            for (int k = 0; k < kPsG; ++k) {
                const double d = gt[k] - g[k];
                dn += d * d;
                xn += g[k] * g[k];
            }
        }
        pnp_wave_sync();   // every lane has read glob before lane 0 writes it
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < kPsG; ++k) a.glob[k] = gt[k];
        }
    });
}

}  // namespace mcc

hipError_t mcc_launch_ps_lin(const mcc::PsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mcc::k_ps_lin, dim3(a.n), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t mcc_launch_ps_try(const mcc::PsArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mcc::k_ps_try, dim3(a.n), dim3(64), 0, s, a);
    return hipGetLastError();
}
