// mcc_omnicalib_host.hpp -- host helpers shared by mcc_omnicalib_api.cpp and mcc_omnistereo_api.cpp:
// the error path of the C ABI, an owning device buffer, and the handles' common base with the one
// implementation of everything that drives the device loop (state, graphs, step launches and the
// bodies of jacobian / optimize / rms / time_steps).  The pinhole host files include it for the error
// path, DBuf, OcEvents, mul3 and rodrigues_host.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <string>
#include <vector>

#include "mcc_omnicalib_internal.h"

namespace {

int oc_fail(int code, const std::string& msg) { return mcc_internal_fail(code, msg.c_str()); }

#define OCCHK(expr)                                                                          \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) return oc_fail(MCC_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

template <typename T>
struct DBuf {
    T* p = nullptr;
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)); }
    hipError_t upload(const T* h, size_t n) {
        hipError_t e = alloc(n);
        if (e == hipSuccess && n) e = hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
};

// the two events around a timed stretch of device work
struct OcEvents {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~OcEvents() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t create() {
        hipError_t e = hipEventCreate(&ev[0]);
        return e == hipSuccess ? hipEventCreate(&ev[1]) : e;
    }
    hipError_t elapsed(double* ms) {
        hipError_t e = hipEventSynchronize(ev[1]);
        float f = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&f, ev[0], ev[1]);
        *ms = f;
        return e;
    }
};

// C = A B, row-major 3 x 3
void mul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

// de-interleaves C w-tuples (pattern points: 3, image points: 2) into w device arrays
hipError_t oc_upload_soa(const double* src, int w, size_t C, std::initializer_list<DBuf<double>*> dst) {
    std::vector<double> col(C);
    int k = 0;
    for (DBuf<double>* b : dst) {
        for (size_t c = 0; c < C; ++c) col[c] = src[w * c + k];
        const hipError_t e = b->upload(col.data(), C);
        if (e != hipSuccess) return e;
        ++k;
    }
    return hipSuccess;
}

// What the handles of calibrate (mcc_omnicalib) and stereoCalibrate (mcc_omnistereo) have in common:
// the device-resident loop.  A handle type H derives from it and adds its point buffers and
//   kG, kName, kStepName     the global-block width and the names its messages use,
//   launch_step, launch_err  its two kernels on the stream,
//   rms_points               the divisor of rms.
struct OcHandle {
    int n = 0, P = 0, flags = 0, device = 0, group_size = 1, n_groups = 1;
    long long corners = 0;
    hipStream_t stream = nullptr;
    DBuf<double> x, mask, Yv, zb, zu, yc, jte, G, contrib, gsum, view_sq;
    DBuf<int> cnt;
    DBuf<mcc::OcState> st;
    mcc::OcState* h_st = nullptr;
    static constexpr int kGraphSteps = 8;
    hipGraphExec_t gexec[2] = {nullptr, nullptr};   // linear chains of 1 and 8 steps
    hipEvent_t ev[2] = {nullptr, nullptr};

    mcc::OcLoop loop() const {
        return mcc::OcLoop{x.p, mask.p, Yv.p, zb.p, zu.p, yc.p, jte.p, G.p, contrib.p, gsum.p, cnt.p, st.p,
                           n, group_size, n_groups};
    }
};

int oc_set_state(OcHandle* h, int iter, int crit, int max_count, double eps) {
    OCCHK(hipStreamSynchronize(h->stream));
    mcc::OcState s{};
    s.iter = iter;
    s.crit_type = crit;
    s.max_count = max_count;
    s.eps = eps;
    s.change = 1.0;
    *h->h_st = s;
    OCCHK(hipMemcpyAsync(h->st.p, h->h_st, sizeof(mcc::OcState), hipMemcpyHostToDevice, h->stream));
    OCCHK(hipStreamSynchronize(h->stream));
    return MCC_OK;
}

template <class H>
int oc_read_state(H* h) {
    OCCHK(hipMemcpyAsync(h->h_st, h->st.p, sizeof(mcc::OcState), hipMemcpyDeviceToHost, h->stream));
    OCCHK(hipStreamSynchronize(h->stream));
    if (h->h_st->error & 1)
        return oc_fail(MCC_ENOTPD, std::string(H::kName) + ": a view's 6x6 pose block J^T J is not positive definite");
    return MCC_OK;
}

int oc_upload_params(OcHandle* h, const double* params) {
    OCCHK(hipMemcpyAsync(h->x.p, params, sizeof(double) * h->P, hipMemcpyHostToDevice, h->stream));
    return MCC_OK;
}

template <class H>
int oc_build_graphs(H* h) {
    if (h->gexec[0]) return MCC_OK;
    const int counts[2] = {1, OcHandle::kGraphSteps};
    for (int g = 0; g < 2; ++g) {
        hipGraph_t graph;
        OCCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        hipError_t le = hipSuccess;
        for (int s = 0; s < counts[g] && le == hipSuccess; ++s) le = h->launch_step();
        hipError_t ee = hipStreamEndCapture(h->stream, &graph);
        if (le != hipSuccess) return oc_fail(MCC_EHIP, std::string(H::kStepName) + " launch: " + hipGetErrorString(le));
        if (ee != hipSuccess) return oc_fail(MCC_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ee));
        OCCHK(hipGraphInstantiate(&h->gexec[g], graph, nullptr, nullptr, 0));
        OCCHK(hipGraphDestroy(graph));
    }
    return MCC_OK;
}

template <class H>
int oc_launch_steps(H* h, int n) {
    int rc = oc_build_graphs(h);
    if (rc) return rc;
    while (n >= OcHandle::kGraphSteps) {
        OCCHK(hipGraphLaunch(h->gexec[1], h->stream));
        n -= OcHandle::kGraphSteps;
    }
    while (n-- > 0) OCCHK(hipGraphLaunch(h->gexec[0], h->stream));
    return MCC_OK;
}

// the tail of create, after n, P and the mask are set and the points are uploaded
template <class H>
int oc_alloc_loop(H* h) {
    using L = mcc::OcLayout<H::kG>;
    const size_t n = (size_t)h->n;
    h->group_size = std::max(1, (int)std::ceil(std::sqrt((double)h->n)));
    h->n_groups = (h->n + h->group_size - 1) / h->group_size;
    OCCHK(h->x.alloc(h->P));
    OCCHK(h->Yv.alloc(6 * H::kG * n));
    OCCHK(h->zb.alloc(6 * n));
    OCCHK(h->zu.alloc(6 * n));
    OCCHK(h->yc.alloc(H::kG));
    OCCHK(h->jte.alloc(h->P));
    OCCHK(h->G.alloc(h->P));
    OCCHK(h->contrib.alloc(n * L::Lc));
    OCCHK(h->gsum.alloc((size_t)h->n_groups * L::Lc));
    OCCHK(h->view_sq.alloc(n));
    OCCHK(h->cnt.alloc(h->n_groups + 1));
    OCCHK(hipMemset(h->cnt.p, 0, sizeof(int) * (h->n_groups + 1)));
    OCCHK(hipMemset(h->G.p, 0, sizeof(double) * h->P));
    OCCHK(hipMemset(h->jte.p, 0, sizeof(double) * h->P));
    OCCHK(h->st.alloc(1));
    OCCHK(hipHostMalloc((void**)&h->h_st, sizeof(mcc::OcState), hipHostMallocDefault));
    OCCHK(hipEventCreate(&h->ev[0]));
    OCCHK(hipEventCreate(&h->ev[1]));
    return MCC_OK;
}

template <class H>
void oc_destroy(H* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& g : h->gexec)
        if (g) (void)hipGraphExecDestroy(g);
    for (auto& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->h_st) (void)hipHostFree(h->h_st);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;   // the buffers
}

template <class H>
int oc_jacobian(H* h, const double* params, int iter, double* jte, double* G) {
    if (!h || !params || iter < 0) return oc_fail(MCC_EINVAL, "bad argument");
    OCCHK(hipSetDevice(h->device));
    int rc = oc_set_state(h, iter, MCC_CRIT_COUNT, iter + 1, 0.0);
    if (rc) return rc;
    if ((rc = oc_upload_params(h, params))) return rc;
    // step 1 linearises and solves iteration `iter` (the global part of G), step 2 applies the
    // pending pose update (the pose part of G) and stops (iter + 1 >= max_count); JTE is read
    // between the two, because step 2 linearises again at the updated point
    OCCHK(h->launch_step());
    if ((rc = oc_read_state(h))) return rc;
    if (jte) OCCHK(hipMemcpy(jte, h->jte.p, sizeof(double) * h->P, hipMemcpyDeviceToHost));
    OCCHK(h->launch_step());
    if ((rc = oc_read_state(h))) return rc;
    if (G) OCCHK(hipMemcpy(G, h->G.p, sizeof(double) * h->P, hipMemcpyDeviceToHost));
    return MCC_OK;
}

template <class H>
int oc_optimize(H* h, int crit_type, int max_count, double eps, double* params_inout, int* iters,
                double* last_change) {
    if (!h || !params_inout) return oc_fail(MCC_EINVAL, "null argument");
    if (crit_type < 1 || crit_type > 3) return oc_fail(MCC_EINVAL, "crit_type must be 1, 2 or 3");
    OCCHK(hipSetDevice(h->device));
    int rc = oc_set_state(h, 0, crit_type, max_count, eps);
    if (rc) return rc;
    if ((rc = oc_upload_params(h, params_inout))) return rc;
    const long long cap = crit_type == MCC_CRIT_EPS ? 1000000LL : (long long)max_count + 1;
    long long launched = 0;
    while (true) {
        if ((rc = oc_launch_steps(h, OcHandle::kGraphSteps))) return rc;
        launched += OcHandle::kGraphSteps;
        if ((rc = oc_read_state(h))) return rc;
        if (h->h_st->done) break;
        if (launched > cap + OcHandle::kGraphSteps)
            return oc_fail(MCC_EINVAL, std::string(H::kName) + " did not terminate");
    }
    if (iters) *iters = h->h_st->iter;
    if (last_change) *last_change = h->h_st->change;
    OCCHK(hipMemcpy(params_inout, h->x.p, sizeof(double) * h->P, hipMemcpyDeviceToHost));
    return MCC_OK;
}

template <class H>
int oc_rms(H* h, const double* params, double* rms) {
    if (!h || !params || !rms) return oc_fail(MCC_EINVAL, "null argument");
    OCCHK(hipSetDevice(h->device));
    OCCHK(hipStreamSynchronize(h->stream));
    int rc = oc_upload_params(h, params);
    if (rc) return rc;
    OCCHK(h->launch_err());
    std::vector<double> sq(h->n);
    OCCHK(hipMemcpyAsync(sq.data(), h->view_sq.p, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    OCCHK(hipStreamSynchronize(h->stream));
    double s = 0;
    for (int v = 0; v < h->n; ++v) s += sq[v];   // view order
    *rms = std::sqrt(s / h->rms_points());
    return MCC_OK;
}

template <class H>
int oc_time_steps(H* h, const double* params, int n_steps, double* ms_per_step) {
    if (!h || !params || n_steps < 1 || !ms_per_step) return oc_fail(MCC_EINVAL, "bad argument");
    OCCHK(hipSetDevice(h->device));
    int rc = oc_set_state(h, 0, 0, 0, 0.0);
    if (rc) return rc;
    if ((rc = oc_upload_params(h, params))) return rc;
    if ((rc = oc_launch_steps(h, 2))) return rc;   // graph instantiation + first touch
    OCCHK(hipEventRecord(h->ev[0], h->stream));
    if ((rc = oc_launch_steps(h, n_steps))) return rc;
    OCCHK(hipEventRecord(h->ev[1], h->stream));
    OCCHK(hipEventSynchronize(h->ev[1]));
    if ((rc = oc_read_state(h))) return rc;
    float ms = 0.f;
    OCCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    *ms_per_step = (double)ms / n_steps;
    return MCC_OK;
}

// cvRodrigues2 vector -> matrix
void rodrigues_host(const double* om, double* R) {
    const double th = std::sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::copy(I, I + 9, R);
    if (th < 2.220446049250313e-16) return;
    const double c = std::cos(th), s = std::sin(th), c1 = 1 - c;
    const double x = om[0] / th, y = om[1] / th, z = om[2] / th;
    const double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
    const double rx[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    for (int k = 0; k < 9; ++k) R[k] = c * I[k] + c1 * rrt[k] + s * rx[k];
}

// flags2idx (src/omnidir.cpp:2031-2076) for the 10 intrinsics: 1 = free, 0 = fixed.  The cascade
// of >= tests is the reference's (CALIB_USE_GUESS is not handled there either).  flags2idxStereo
// (:2078-2135) applies the same cascade to both cameras' intrinsics.
void intrinsic_mask(int flags, double* m) {
    for (int i = 0; i < 10; ++i) m[i] = 1.0;
    int f = flags;
    if (f >= MCC_OMNI_CALIB_FIX_CENTER) { m[3] = m[4] = 0; f -= MCC_OMNI_CALIB_FIX_CENTER; }
    if (f >= MCC_OMNI_CALIB_FIX_GAMMA) { m[0] = m[1] = 0; f -= MCC_OMNI_CALIB_FIX_GAMMA; }
    if (f >= MCC_OMNI_CALIB_FIX_XI) { m[5] = 0; f -= MCC_OMNI_CALIB_FIX_XI; }
    if (f >= MCC_OMNI_CALIB_FIX_P2) { m[9] = 0; f -= MCC_OMNI_CALIB_FIX_P2; }
    if (f >= MCC_OMNI_CALIB_FIX_P1) { m[8] = 0; f -= MCC_OMNI_CALIB_FIX_P1; }
    if (f >= MCC_OMNI_CALIB_FIX_K2) { m[7] = 0; f -= MCC_OMNI_CALIB_FIX_K2; }
    if (f >= MCC_OMNI_CALIB_FIX_K1) { m[6] = 0; f -= MCC_OMNI_CALIB_FIX_K1; }
    if (f >= MCC_OMNI_CALIB_FIX_SKEW) m[2] = 0;
}

}  // namespace
