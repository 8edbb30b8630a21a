// mcc_omnistereo_api.cpp -- host side of the two-camera omnidir calibration C ABI
// (include/mcc_omnidir.h; cv::omnidir::stereoCalibrate, src/omnidir.cpp:1213-1381).
//
// mcc_omnistereo_* keep the views' corners of both cameras in HBM as structure-of-arrays and run
// stereoCalibrate's loop on the device: one k_os_step launch per iteration, graph-launched 8 at a
// time, the stop test on the device.  initializeStereoCalibration (:750-846) is two
// mcc_omnidir_calibrate runs plus host code (mcc_omnidir_stereo_encode_init).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcc_omnidir.h"
#include "mcc_omnicalib_host.hpp"
#include "mcc_omnistereo_internal.h"

using mcc::OcState;

struct mcc_omnistereo {
    int n = 0, np = 0, P = 0, flags = 0, device = 0, chunk = 64, group_size = 1, n_groups = 1;
    long long corners = 0;
    hipStream_t stream = nullptr;
    DBuf<double> ox, oy, oz, iu1, iv1, iu2, iv2, x, mask, Yv, zb, zu, yc, jte, G, contrib, gsum, view_sq;
    DBuf<int> cnt;
    DBuf<OcState> st;
    OcState* h_st = nullptr;
    static constexpr int kGraphSteps = 8;
    hipGraphExec_t gexec[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};

    mcc::OsArgs args() const {
        return mcc::OsArgs{st.p, ox.p, oy.p, oz.p, iu1.p, iv1.p, iu2.p, iv2.p, x.p, mask.p, Yv.p, zb.p, zu.p, yc.p,
                           jte.p, G.p, contrib.p, gsum.p, cnt.p, n, np, chunk, group_size, n_groups};
    }
};

namespace {

// uniform corner count in [3, kOsMaxCorners]: computeJacobianStereo takes n_points from view 0 (:947)
int os_check_views(int n, const int* off, int* np_out) {
    if (n < 1 || !off) return oc_fail(MCC_EINVAL, "omnidir stereoCalibrate needs at least one view with points");
    if (off[0] != 0) return oc_fail(MCC_EINVAL, "view_off[0] must be 0");
    const int np = off[1] - off[0];
    for (int i = 0; i < n; ++i) {
        const int k = off[i + 1] - off[i];
        if (k < 3) return oc_fail(MCC_EINVAL, "every view needs at least 3 points");
        if (k > mcc::kOsMaxCorners)
            return oc_fail(MCC_EINVAL, "a view holds more than " + std::to_string(mcc::kOsMaxCorners) + " points");
        if (k != np)
            return oc_fail(MCC_EINVAL, "omnidir stereoCalibrate needs the same number of points in every view (view " +
                                           std::to_string(i) + " has " + std::to_string(k) + ", view 0 has " +
                                           std::to_string(np) + ")");
    }
    *np_out = np;
    return MCC_OK;
}

int os_set_state(mcc_omnistereo* h, int iter, int crit, int max_count, double eps) {
    OCCHK(hipStreamSynchronize(h->stream));
    OcState s{};
    s.iter = iter;
    s.crit_type = crit;
    s.max_count = max_count;
    s.eps = eps;
    s.change = 1.0;
    *h->h_st = s;
    OCCHK(hipMemcpyAsync(h->st.p, h->h_st, sizeof(OcState), hipMemcpyHostToDevice, h->stream));
    OCCHK(hipStreamSynchronize(h->stream));
    return MCC_OK;
}

int os_read_state(mcc_omnistereo* h) {
    OCCHK(hipMemcpyAsync(h->h_st, h->st.p, sizeof(OcState), hipMemcpyDeviceToHost, h->stream));
    OCCHK(hipStreamSynchronize(h->stream));
    if (h->h_st->error & 1)
        return oc_fail(MCC_ENOTPD, "omnidir stereoCalibrate: a view's 6x6 pose block J^T J is not positive definite");
    return MCC_OK;
}

int os_upload_params(mcc_omnistereo* h, const double* params) {
    OCCHK(hipMemcpyAsync(h->x.p, params, sizeof(double) * h->P, hipMemcpyHostToDevice, h->stream));
    return MCC_OK;
}

int os_build_graphs(mcc_omnistereo* h) {
    if (h->gexec[0]) return MCC_OK;
    const int counts[2] = {1, mcc_omnistereo::kGraphSteps};
    const mcc::OsArgs a = h->args();
    for (int g = 0; g < 2; ++g) {   // linear chains of 1 and 8 steps
        hipGraph_t graph;
        OCCHK(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        hipError_t le = hipSuccess;
        for (int s = 0; s < counts[g] && le == hipSuccess; ++s) le = mcc_launch_os_step(a, h->stream);
        hipError_t ee = hipStreamEndCapture(h->stream, &graph);
        if (le != hipSuccess) return oc_fail(MCC_EHIP, std::string("k_os_step launch: ") + hipGetErrorString(le));
        if (ee != hipSuccess) return oc_fail(MCC_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ee));
        OCCHK(hipGraphInstantiate(&h->gexec[g], graph, nullptr, nullptr, 0));
        OCCHK(hipGraphDestroy(graph));
    }
    return MCC_OK;
}

int os_launch_steps(mcc_omnistereo* h, int n) {
    int rc = os_build_graphs(h);
    if (rc) return rc;
    while (n >= mcc_omnistereo::kGraphSteps) {
        OCCHK(hipGraphLaunch(h->gexec[1], h->stream));
        n -= mcc_omnistereo::kGraphSteps;
    }
    while (n-- > 0) OCCHK(hipGraphLaunch(h->gexec[0], h->stream));
    return MCC_OK;
}

void rodrigues_host(const double* om, double* R) {   // cvRodrigues2 vector -> matrix
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

// findMedian (:2172-2181) with its even and odd cases as the reference has them: an even count
// returns the upper-middle element, an odd count the mean of the middle element and the one below
double find_median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    if (n % 2 == 0) return v[n / 2];
    return n >= 2 ? 0.5 * (v[n / 2] + v[n / 2 - 1]) : v[0];
}

}  // namespace

extern "C" {

int mcc_omnistereo_create(mcc_omnistereo** out, const mcc_omnistereo_desc* d) {
    if (!out || !d) return oc_fail(MCC_EINVAL, "null argument");
    *out = nullptr;
    if (!d->view_off || !d->obj || !d->img1 || !d->img2)
        return oc_fail(MCC_EINVAL, "omnidir stereoCalibrate needs at least one view with points");
    int np = 0;
    int rc = os_check_views(d->n_views, d->view_off, &np);
    if (rc) return rc;
    const int n = d->n_views;
    auto* h = new mcc_omnistereo();
    h->n = n;
    h->np = np;
    h->P = 6 * (n + 1) + 20;
    h->flags = d->flags;
    h->device = d->device;
    h->chunk = np <= 64 ? 64 : 128;
    h->corners = (long long)n * np;
    h->group_size = std::max(1, (int)std::ceil(std::sqrt((double)n)));
    h->n_groups = (n + h->group_size - 1) / h->group_size;
    auto bail = [&](int code) {
        mcc_omnistereo_destroy(h);
        return code;
    };
#define OSCHK_H(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) return bail(oc_fail(MCC_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e))); \
    } while (0)
    OSCHK_H(hipSetDevice(d->device));
    OSCHK_H(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const size_t C = (size_t)h->corners;
    std::vector<double> soa[7];
    for (auto& s : soa) s.resize(C);
    for (size_t c = 0; c < C; ++c) {
        soa[0][c] = d->obj[3 * c];
        soa[1][c] = d->obj[3 * c + 1];
        soa[2][c] = d->obj[3 * c + 2];
        soa[3][c] = d->img1[2 * c];
        soa[4][c] = d->img1[2 * c + 1];
        soa[5][c] = d->img2[2 * c];
        soa[6][c] = d->img2[2 * c + 1];
    }
    DBuf<double>* pts[7] = {&h->ox, &h->oy, &h->oz, &h->iu1, &h->iv1, &h->iu2, &h->iv2};
    for (int k = 0; k < 7; ++k) OSCHK_H(pts[k]->upload(soa[k].data(), C));
    double m[mcc::kOsG];
    for (int k = 0; k < 6; ++k) m[k] = 1.0;   // om, T and the kept poses are never fixed
    intrinsic_mask(d->flags, m + 6);
    std::copy(m + 6, m + 16, m + 16);
    OSCHK_H(h->mask.upload(m, mcc::kOsG));
    OSCHK_H(h->x.alloc(h->P));
    OSCHK_H(h->Yv.alloc(mcc::kOsY * (size_t)n));
    OSCHK_H(h->zb.alloc(6 * (size_t)n));
    OSCHK_H(h->zu.alloc(6 * (size_t)n));
    OSCHK_H(h->yc.alloc(mcc::kOsG));
    OSCHK_H(h->jte.alloc(h->P));
    OSCHK_H(h->G.alloc(h->P));
    OSCHK_H(h->contrib.alloc((size_t)n * mcc::kOsLc));
    OSCHK_H(h->gsum.alloc((size_t)h->n_groups * mcc::kOsLc));
    OSCHK_H(h->view_sq.alloc(n));
    OSCHK_H(h->cnt.alloc(h->n_groups + 1));
    OSCHK_H(hipMemset(h->cnt.p, 0, sizeof(int) * (h->n_groups + 1)));
    OSCHK_H(hipMemset(h->G.p, 0, sizeof(double) * h->P));
    OSCHK_H(hipMemset(h->jte.p, 0, sizeof(double) * h->P));
    OSCHK_H(h->st.alloc(1));
    OSCHK_H(hipHostMalloc((void**)&h->h_st, sizeof(OcState), hipHostMallocDefault));
    OSCHK_H(mcc_os_set_attrs(h->chunk));
    OSCHK_H(hipEventCreate(&h->ev[0]));
    OSCHK_H(hipEventCreate(&h->ev[1]));
#undef OSCHK_H
    *out = h;
    return MCC_OK;
}

void mcc_omnistereo_destroy(mcc_omnistereo* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& g : h->gexec)
        if (g) (void)hipGraphExecDestroy(g);
    for (auto& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    for (DBuf<double>* b : {&h->ox, &h->oy, &h->oz, &h->iu1, &h->iv1, &h->iu2, &h->iv2, &h->x, &h->mask, &h->Yv,
                            &h->zb, &h->zu, &h->yc, &h->jte, &h->G, &h->contrib, &h->gsum, &h->view_sq})
        b->release();
    h->cnt.release();
    h->st.release();
    if (h->h_st) (void)hipHostFree(h->h_st);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int mcc_omnistereo_nparams(const mcc_omnistereo* h) { return h ? h->P : MCC_EINVAL; }

int mcc_omnistereo_jacobian(mcc_omnistereo* h, const double* params, int iter, double* jte, double* G) {
    if (!h || !params || iter < 0) return oc_fail(MCC_EINVAL, "bad argument");
    OCCHK(hipSetDevice(h->device));
    int rc = os_set_state(h, iter, MCC_CRIT_COUNT, iter + 1, 0.0);
    if (rc) return rc;
    if ((rc = os_upload_params(h, params))) return rc;
    // step 1 linearises and solves iteration `iter` (the global part of G), step 2 applies the
    // pending pose update (the pose part of G) and stops (iter + 1 >= max_count); JTE is read
    // between the two, because step 2 linearises again at the updated point
    const mcc::OsArgs a = h->args();
    OCCHK(mcc_launch_os_step(a, h->stream));
    if ((rc = os_read_state(h))) return rc;
    if (jte) OCCHK(hipMemcpy(jte, h->jte.p, sizeof(double) * h->P, hipMemcpyDeviceToHost));
    OCCHK(mcc_launch_os_step(a, h->stream));
    if ((rc = os_read_state(h))) return rc;
    if (G) OCCHK(hipMemcpy(G, h->G.p, sizeof(double) * h->P, hipMemcpyDeviceToHost));
    return MCC_OK;
}

int mcc_omnistereo_optimize(mcc_omnistereo* h, int crit_type, int max_count, double eps, double* params_inout,
                            int* iters, double* last_change) {
    if (!h || !params_inout) return oc_fail(MCC_EINVAL, "null argument");
    if (crit_type < 1 || crit_type > 3) return oc_fail(MCC_EINVAL, "crit_type must be 1, 2 or 3");
    OCCHK(hipSetDevice(h->device));
    int rc = os_set_state(h, 0, crit_type, max_count, eps);
    if (rc) return rc;
    if ((rc = os_upload_params(h, params_inout))) return rc;
    const long long cap = crit_type == MCC_CRIT_EPS ? 1000000LL : (long long)max_count + 1;
    long long launched = 0;
    while (true) {
        if ((rc = os_launch_steps(h, mcc_omnistereo::kGraphSteps))) return rc;
        launched += mcc_omnistereo::kGraphSteps;
        if ((rc = os_read_state(h))) return rc;
        if (h->h_st->done) break;
        if (launched > cap + mcc_omnistereo::kGraphSteps)
            return oc_fail(MCC_EINVAL, "omnidir stereoCalibrate did not terminate");
    }
    if (iters) *iters = h->h_st->iter;
    if (last_change) *last_change = h->h_st->change;
    OCCHK(hipMemcpy(params_inout, h->x.p, sizeof(double) * h->P, hipMemcpyDeviceToHost));
    return MCC_OK;
}

int mcc_omnistereo_rms(mcc_omnistereo* h, const double* params, double* rms) {
    if (!h || !params || !rms) return oc_fail(MCC_EINVAL, "null argument");
    OCCHK(hipSetDevice(h->device));
    OCCHK(hipStreamSynchronize(h->stream));
    int rc = os_upload_params(h, params);
    if (rc) return rc;
    const mcc::OsErrArgs a{h->ox.p, h->oy.p, h->oz.p, h->iu1.p, h->iv1.p, h->iu2.p, h->iv2.p, h->x.p, h->view_sq.p,
                           h->n, h->np};
    OCCHK(mcc_launch_os_err(a, h->stream));
    std::vector<double> sq(h->n);
    OCCHK(hipMemcpyAsync(sq.data(), h->view_sq.p, sizeof(double) * h->n, hipMemcpyDeviceToHost, h->stream));
    OCCHK(hipStreamSynchronize(h->stream));
    double s = 0;
    for (int v = 0; v < h->n; ++v) s += sq[v];   // view order
    *rms = std::sqrt(s / (2.0 * (double)h->corners));   // over both cameras' points (:1880-1888)
    return MCC_OK;
}

int mcc_omnistereo_time_steps(mcc_omnistereo* h, const double* params, int n_steps, double* ms_per_step) {
    if (!h || !params || n_steps < 1 || !ms_per_step) return oc_fail(MCC_EINVAL, "bad argument");
    OCCHK(hipSetDevice(h->device));
    int rc = os_set_state(h, 0, 0, 0, 0.0);
    if (rc) return rc;
    if ((rc = os_upload_params(h, params))) return rc;
    if ((rc = os_launch_steps(h, 2))) return rc;   // graph instantiation + first touch
    OCCHK(hipEventRecord(h->ev[0], h->stream));
    if ((rc = os_launch_steps(h, n_steps))) return rc;
    OCCHK(hipEventRecord(h->ev[1], h->stream));
    OCCHK(hipEventSynchronize(h->ev[1]));
    if ((rc = os_read_state(h))) return rc;
    float ms = 0.f;
    OCCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    *ms_per_step = (double)ms / n_steps;
    return MCC_OK;
}

int mcc_omnidir_stereo_encode_init(int n1, const int* idx1, const double* om1, const double* t1, int n2,
                                   const int* idx2, const double* om2, const double* t2, const double* K1, double xi1,
                                   const double* D1, const double* K2, double xi2, const double* D2, double* params,
                                   int* idx, int* n_idx) {
    // initializeStereoCalibration after its two calibrate calls (:764-846) and encodeParametersStereo
    if (n1 < 0 || n2 < 0 || (n1 && (!idx1 || !om1 || !t1)) || (n2 && (!idx2 || !om2 || !t2)) || !K1 || !D1 || !K2 ||
        !D2 || !params || !idx || !n_idx)
        return oc_fail(MCC_EINVAL, "bad argument");
    // getInterset (:2229-2250): the order of the first camera's kept list
    std::vector<int> i1, i2;
    for (int i = 0; i < n1; ++i)
        for (int j = 0; j < n2; ++j)
            if (idx1[i] == idx2[j]) {
                i1.push_back(i);
                i2.push_back(j);
            }
    const int n = (int)i1.size();
    if (n < 1) return oc_fail(MCC_EINVAL, "omnidir stereoCalibrate: the two cameras keep no common view");
    std::vector<double> est[6];
    for (int i = 0; i < n; ++i) {
        double R1[9], R2[9], RLR[9], omLR[3];
        rodrigues_host(om1 + 3 * (size_t)i1[i], R1);
        rodrigues_host(om2 + 3 * (size_t)i2[i], R2);
        const double* T1 = t1 + 3 * (size_t)i1[i];
        const double* T2 = t2 + 3 * (size_t)i2[i];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)   // RLR = R2 R1^T (:792)
                RLR[r * 3 + c] = R2[r * 3] * R1[c * 3] + R2[r * 3 + 1] * R1[c * 3 + 1] + R2[r * 3 + 2] * R1[c * 3 + 2];
        mcc_internal_rodrigues_m2v(RLR, omLR);
        for (int r = 0; r < 3; ++r) {
            est[r].push_back(omLR[r]);
            est[3 + r].push_back(T2[r] - (RLR[r * 3] * T1[0] + RLR[r * 3 + 1] * T1[1] + RLR[r * 3 + 2] * T1[2]));
        }
    }
    for (int k = 0; k < 6; ++k) params[k] = find_median(est[k]);   // findMedian3 of om and of T
    for (int i = 0; i < n; ++i) {
        idx[i] = idx1[i1[i]];
        for (int k = 0; k < 3; ++k) {
            params[6 + 6 * i + k] = om1[3 * (size_t)i1[i] + k];
            params[6 + 6 * i + 3 + k] = t1[3 * (size_t)i1[i] + k];
        }
    }
    double* q = params + 6 * (size_t)(n + 1);
    const double* Ks[2] = {K1, K2};
    const double* Ds[2] = {D1, D2};
    const double xis[2] = {xi1, xi2};
    for (int c = 0; c < 2; ++c, q += 10) {
        q[0] = Ks[c][0]; q[1] = Ks[c][4]; q[2] = Ks[c][1]; q[3] = Ks[c][2]; q[4] = Ks[c][5]; q[5] = xis[c];
        std::copy(Ds[c], Ds[c] + 4, q + 6);
    }
    *n_idx = n;
    return MCC_OK;
}

int mcc_omnidir_stereo_initialize(int n_img, const int* off, const double* obj, const double* img1, const double* img2,
                                  int width1, int height1, int width2, int height2, int flags, int device,
                                  double* params, int* idx, int* n_idx) {
    // initializeStereoCalibration (:750-846): both single-camera calibrations run with
    // TermCriteria(3, 100, 1e-6) and the caller's flags (:761-762)
    if (!obj || !img1 || !img2 || !params || !idx || !n_idx) return oc_fail(MCC_EINVAL, "null argument");
    int np = 0;
    int rc = os_check_views(n_img, off, &np);
    if (rc) return rc;
    const size_t n = (size_t)n_img;
    std::vector<double> om[2], t[2];
    std::vector<int> kept[2];
    double K[2][9], D[2][4], xi[2] = {1, 1}, rms = 0;
    int nk[2] = {0, 0};
    const double* img[2] = {img1, img2};
    const int w[2] = {width1, width2}, hgt[2] = {height1, height2};
    for (int c = 0; c < 2; ++c) {
        om[c].resize(3 * n);
        t[c].resize(3 * n);
        kept[c].resize(n);
        rc = mcc_omnidir_calibrate(n_img, off, obj, img[c], w[c], hgt[c], flags, MCC_CRIT_COUNT_EPS, 100, 1e-6, device,
                                   K[c], &xi[c], D[c], om[c].data(), t[c].data(), kept[c].data(), &nk[c], &rms, nullptr);
        if (rc) return rc;
    }
    return mcc_omnidir_stereo_encode_init(nk[0], kept[0].data(), om[0].data(), t[0].data(), nk[1], kept[1].data(),
                                          om[1].data(), t[1].data(), K[0], xi[0], D[0], K[1], xi[1], D[1], params, idx,
                                          n_idx);
}

int mcc_omnidir_stereo_calibrate(int n_img, const int* off, const double* obj, const double* img1, const double* img2,
                                 int width1, int height1, int width2, int height2, int flags, int crit_type,
                                 int max_count, double eps, int device, double* K1, double* xi1, double* D1, double* K2,
                                 double* xi2, double* D2, double* om, double* T, double* omL, double* tL, int* idx,
                                 int* n_idx, double* rms, int* iters) {
    // src/omnidir.cpp:1213-1381: initialise, keep the idx views, the loop, decodeParametersStereo,
    // estimateUncertaintiesStereo's rms
    if (!K1 || !xi1 || !D1 || !K2 || !xi2 || !D2 || !om || !T || !omL || !tL || !idx || !n_idx || !rms)
        return oc_fail(MCC_EINVAL, "null argument");
    if (crit_type < 1 || crit_type > 3) return oc_fail(MCC_EINVAL, "crit_type must be 1, 2 or 3");
    int np = 0;
    int rc = os_check_views(n_img, off, &np);
    if (rc) return rc;
    if (!obj || !img1 || !img2) return oc_fail(MCC_EINVAL, "null argument");
    std::vector<double> para(6 * ((size_t)n_img + 1) + 20);
    int nk = 0;
    rc = mcc_omnidir_stereo_initialize(n_img, off, obj, img1, img2, width1, height1, width2, height2, flags, device,
                                       para.data(), idx, &nk);
    if (rc) return rc;
    std::vector<int> o2(nk + 1, 0);
    std::vector<double> ob2(3 * (size_t)nk * np), im1(2 * (size_t)nk * np), im2(2 * (size_t)nk * np);
    for (int i = 0; i < nk; ++i) {
        o2[i + 1] = o2[i] + np;
        const size_t s = (size_t)off[idx[i]];
        std::copy(obj + 3 * s, obj + 3 * (s + np), &ob2[3 * (size_t)o2[i]]);
        std::copy(img1 + 2 * s, img1 + 2 * (s + np), &im1[2 * (size_t)o2[i]]);
        std::copy(img2 + 2 * s, img2 + 2 * (s + np), &im2[2 * (size_t)o2[i]]);
    }
    mcc_omnistereo_desc d{nk, o2.data(), ob2.data(), im1.data(), im2.data(), flags, device};
    mcc_omnistereo* h = nullptr;
    if ((rc = mcc_omnistereo_create(&h, &d))) return rc;
    int it = 0;
    rc = mcc_omnistereo_optimize(h, crit_type, max_count, eps, para.data(), &it, nullptr);
    if (!rc) rc = mcc_omnistereo_rms(h, para.data(), rms);
    mcc_omnistereo_destroy(h);
    if (rc) return rc;
    std::copy(para.begin(), para.begin() + 3, om);
    std::copy(para.begin() + 3, para.begin() + 6, T);
    for (int i = 0; i < nk; ++i)
        for (int k = 0; k < 3; ++k) {
            omL[3 * i + k] = para[6 + 6 * i + k];
            tL[3 * i + k] = para[6 + 6 * i + 3 + k];
        }
    const double* q = &para[6 * ((size_t)nk + 1)];
    double* Ks[2] = {K1, K2};
    double* Ds[2] = {D1, D2};
    double* xs[2] = {xi1, xi2};
    for (int c = 0; c < 2; ++c, q += 10) {
        const double Kd[9] = {q[0], q[2], q[3], 0, q[1], q[4], 0, 0, 1};
        std::copy(Kd, Kd + 9, Ks[c]);
        *xs[c] = q[5];
        std::copy(q + 6, q + 10, Ds[c]);
    }
    *n_idx = nk;
    if (iters) *iters = it;
    return MCC_OK;
}

}  // extern "C"
