// mcc_pnp_api.cpp -- host side of mcc_solve_pnp_batch (include/mcc.h): the batched restatement of
// host/pnp.cpp's solvePnP.  The host checks the descriptor before any device call, pads every
// camera's distortion vector to the twelve coefficients of pnp.cpp::distort, and launches k_pnp
// (mcc_pnp.hip) once for the whole batch.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/mcc.h"
#include "mcc_omnicalib_host.hpp"
#include "mcc_pnp_internal.h"

namespace {

struct PnpEvents {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~PnpEvents() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace

extern "C" int mcc_solve_pnp_batch(const mcc_pnp_desc* d, double* rvec, double* tvec, double* rms, int* status,
                                   double* device_ms) {
    if (!d || !rvec || !tvec || !rms || !status) return oc_fail(MCC_EINVAL, "solve_pnp_batch: null argument");
    if (d->n_views <= 0) return oc_fail(MCC_EINVAL, "solve_pnp_batch: n_views must be positive");
    if (d->n_cams <= 0) return oc_fail(MCC_EINVAL, "solve_pnp_batch: n_cams must be positive");
    const int nd = d->nd;
    if (nd != 0 && nd != 4 && nd != 5 && nd != 8 && nd != 12)
        return oc_fail(MCC_EINVAL, "solve_pnp_batch: nd must be 0, 4, 5, 8 or 12");
    if (d->max_iter < 0) return oc_fail(MCC_EINVAL, "solve_pnp_batch: max_iter must not be negative");
    if (!d->view_off || !d->obj || !d->img || !d->K || (nd > 0 && !d->D))
        return oc_fail(MCC_EINVAL, "solve_pnp_batch: null pointer in the descriptor");
    if (d->view_off[0] < 0) return oc_fail(MCC_EINVAL, "solve_pnp_batch: view_off[0] is negative");
    int max_n = 1;
    for (int v = 0; v < d->n_views; ++v) {
        const int n = d->view_off[v + 1] - d->view_off[v];
        if (n < 0)
            return oc_fail(MCC_EINVAL, "solve_pnp_batch: view_off is not monotone at view " + std::to_string(v));
        if (n > mcc::kPnpMaxCorners)
            return oc_fail(MCC_EINVAL, "solve_pnp_batch: view " + std::to_string(v) + " has " + std::to_string(n) +
                                           " corners, the limit is " + std::to_string(mcc::kPnpMaxCorners));
        if (d->view_cam && (d->view_cam[v] < 0 || d->view_cam[v] >= d->n_cams))
            return oc_fail(MCC_EINVAL, "solve_pnp_batch: view_cam out of range at view " + std::to_string(v));
        max_n = std::max(max_n, n);
    }
    const size_t corners = (size_t)d->view_off[d->n_views], first = (size_t)d->view_off[0];
    std::vector<double> D12((size_t)mcc::kPnpDist * d->n_cams, 0.0);
    for (int c = 0; c < d->n_cams; ++c)
        for (int k = 0; k < nd; ++k) D12[(size_t)mcc::kPnpDist * c + k] = d->D[(size_t)nd * c + k];
    // the views' offsets relative to the first corner that is uploaded
    std::vector<int> off((size_t)d->n_views + 1);
    for (int v = 0; v <= d->n_views; ++v) off[v] = d->view_off[v] - d->view_off[0];

    OCCHK(hipSetDevice(d->device));
    DBuf<int> d_off, d_cam, d_status;
    DBuf<double> d_obj, d_img, d_K, d_D, d_r, d_t, d_rms;
    OCCHK(d_off.upload(off.data(), off.size()));
    if (d->view_cam) OCCHK(d_cam.upload(d->view_cam, (size_t)d->n_views));
    OCCHK(d_obj.upload(d->obj + 3 * first, 3 * (corners - first)));
    OCCHK(d_img.upload(d->img + 2 * first, 2 * (corners - first)));
    OCCHK(d_K.upload(d->K, 9 * (size_t)d->n_cams));
    OCCHK(d_D.upload(D12.data(), D12.size()));
    OCCHK(d_r.alloc(3 * (size_t)d->n_views));
    OCCHK(d_t.alloc(3 * (size_t)d->n_views));
    OCCHK(d_rms.alloc((size_t)d->n_views));
    OCCHK(d_status.alloc((size_t)d->n_views));
    const mcc::PnpArgs a{d->n_views, d_off.p, d_obj.p, d_img.p, d->view_cam ? d_cam.p : nullptr, d_K.p, d_D.p,
                         d->max_iter, max_n, d_r.p, d_t.p, d_rms.p, d_status.p};
    PnpEvents e;
    OCCHK(hipEventCreate(&e.ev[0]));
    OCCHK(hipEventCreate(&e.ev[1]));
    OCCHK(hipEventRecord(e.ev[0], nullptr));
    OCCHK(mcc_launch_pnp(a, nullptr));
    OCCHK(hipEventRecord(e.ev[1], nullptr));
    OCCHK(hipEventSynchronize(e.ev[1]));
    if (device_ms) {
        float ms = 0.f;
        OCCHK(hipEventElapsedTime(&ms, e.ev[0], e.ev[1]));
        *device_ms = (double)ms;
    }
    OCCHK(hipMemcpy(rvec, d_r.p, sizeof(double) * 3 * (size_t)d->n_views, hipMemcpyDeviceToHost));
    OCCHK(hipMemcpy(tvec, d_t.p, sizeof(double) * 3 * (size_t)d->n_views, hipMemcpyDeviceToHost));
    OCCHK(hipMemcpy(rms, d_rms.p, sizeof(double) * (size_t)d->n_views, hipMemcpyDeviceToHost));
    OCCHK(hipMemcpy(status, d_status.p, sizeof(int) * (size_t)d->n_views, hipMemcpyDeviceToHost));
    return MCC_OK;
}
