// mcc_pinloop_device.hpp -- what the trial kernels of the pinhole calibrateCamera (mcc_pincalib.hip) and
// stereoCalibrate (mcc_pinstereo.hip) share: the two-level last-arriver sums and the verdict of a trial.
// Included by those two files only, after mcc_omnicalib_device.hpp (oc_arrive, oc_sum, oc_st, oc_ld) and
// the pnp_wave_* helpers.  The templates take PcArgs or PsArgs and use the fields by name.
//
// The views are summed in view order in groups of a.group_size (~sqrt(n)) and the groups in group order; a
// workgroup that is not the last to arrive at a ticket leaves.  a.cnt holds the tickets of the lin kernel
// ([n_groups + 1]) and then those of the try kernel.
#pragma once
#include "mcc_pincalib_internal.h"

namespace mcc {

// The sum of the views' N-wide contributions into tot (LDS), with the barrier that publishes it.  False
// for every workgroup but the last arriver.
template <int N, class Args>
__device__ __forceinline__ bool pin_reduce(const Args& a, int v, int lane, double* tot) {
    const int grp = v / a.group_size, g0 = grp * a.group_size, gn = min(a.group_size, a.n - g0);
    if (!oc_arrive(&a.cnt[grp], gn)) return false;
    for (int e = lane; e < N; e += 64)
        oc_st(a.gsum + (size_t)grp * N + e, oc_sum<N>(a.contrib + (size_t)g0 * N + e, gn));
    if (!oc_arrive(&a.cnt[a.n_groups], a.n_groups)) return false;
    for (int e = lane; e < N; e += 64) tot[e] = oc_sum<N>(a.gsum + e, a.n_groups);
    __syncthreads();
    return true;
}

// The same for the trial's squared error, PER slots of a.esq_t per view, into en.
template <int PER, class Args>
__device__ __forceinline__ bool pin_sum_err(const Args& a, int v, int lane, double& en) {
    int* cnt = a.cnt + a.n_groups + 1;
    const int grp = v / a.group_size, g0 = grp * a.group_size, gn = min(a.group_size, a.n - g0);
    if (!oc_arrive(&cnt[grp], gn)) return false;
    {
        const double gs = oc_sum<1>(a.esq_t + PER * (size_t)g0, PER * gn);
        if (lane == 0) oc_st(a.egs + grp, gs);
    }
    if (!oc_arrive(&cnt[a.n_groups], a.n_groups)) return false;
    en = oc_sum<1>(a.egs, a.n_groups);
    return true;
}

// The last arriver of a try kernel: accept or reject the trial, stop tests (pc_next).  An accepted trial's
// poses and per-view errors are committed here; globals(dn, xn) is the kernel's own: it adds the global
// slots' share to |dx|^2 and |x|^2 and commits the trial's slots.  Ends the kernel.  Lane 0 is the only
// writer of *a.st, and of the fields a transition can change only: `fail` is the lin kernel's, the criteria
// are the host's, and `done` / `status` are written when the loop ends.
template <int PER, class Args, class Globals>
__device__ __forceinline__ void pin_verdict(const Args& a, int lane, int init, double en, Globals globals) {
    PcState* st = a.st;
    PcState s = *st;
    s.init = init;   // (the kernel read it on entry)
    const bool accept = !init && pc_accepts(s, en);
    double change = 0.0;
    if (accept) {
        double dn = 0.0, xn = 0.0;
        for (int i = lane; i < 6 * a.n; i += 64) {
            const double xo = a.x[i], xw = oc_ld(a.xt + i), d = xw - xo;
            dn += d * d;
            xn += xo * xo;
            a.x[i] = xw;
        }
        dn = pnp_wave_sum(dn);
        xn = pnp_wave_sum(xn);
        globals(dn, xn);
        change = sqrt(dn) / sqrt(xn);
    }
    if (init || accept)   // the per-view errors of the point the loop now stands at
        for (int i = lane; i < PER * a.n; i += 64) a.esq[i] = oc_ld(a.esq_t + i);
    if (lane == 0) {
        const PcState t = pc_next(s, en, change);
        st->iter = t.iter;
        st->tries = t.tries;
        st->trials = t.trials;
        st->init = 0;
        st->relin = t.relin;
        st->lambda = t.lambda;
        st->err = t.err;
        if (accept) st->change = change;
        if (t.done) {
            st->done = 1;
            st->status = t.status;
        }
    }
}

}  // namespace mcc
