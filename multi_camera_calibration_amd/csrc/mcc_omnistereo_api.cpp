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

struct mcc_omnistereo : OcHandle {
    static constexpr int kG = mcc::kOsG;
    static constexpr const char* kName = "omnidir stereoCalibrate";
    static constexpr const char* kStepName = "k_os_step";
    int np = 0, chunk = 64;
    DBuf<double> ox, oy, oz, iu1, iv1, iu2, iv2;

    hipError_t launch_step() const {
        return mcc_launch_os_step(mcc::OsArgs{loop(), ox.p, oy.p, oz.p, iu1.p, iv1.p, iu2.p, iv2.p, np, chunk}, stream);
    }
    hipError_t launch_err() const {
        return mcc_launch_os_err(
            mcc::OsErrArgs{ox.p, oy.p, oz.p, iu1.p, iv1.p, iu2.p, iv2.p, x.p, view_sq.p, n, np}, stream);
    }
    double rms_points() const { return 2.0 * (double)corners; }   // both cameras' points (:1880-1888)
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
    rc = [&] {
        OCCHK(hipSetDevice(d->device));
        OCCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        const size_t C = (size_t)h->corners;
        OCCHK(oc_upload_soa(d->obj, 3, C, {&h->ox, &h->oy, &h->oz}));
        OCCHK(oc_upload_soa(d->img1, 2, C, {&h->iu1, &h->iv1}));
        OCCHK(oc_upload_soa(d->img2, 2, C, {&h->iu2, &h->iv2}));
        double m[mcc::kOsG];
        for (int k = 0; k < 6; ++k) m[k] = 1.0;   // om, T and the kept poses are never fixed
        intrinsic_mask(d->flags, m + 6);
        std::copy(m + 6, m + 16, m + 16);
        OCCHK(h->mask.upload(m, mcc::kOsG));
        OCCHK(mcc_os_set_attrs(h->chunk));
        return oc_alloc_loop(h);
    }();
    if (rc) {
        mcc_omnistereo_destroy(h);
        return rc;
    }
    *out = h;
    return MCC_OK;
}

void mcc_omnistereo_destroy(mcc_omnistereo* h) { oc_destroy(h); }

int mcc_omnistereo_nparams(const mcc_omnistereo* h) { return h ? h->P : MCC_EINVAL; }

int mcc_omnistereo_jacobian(mcc_omnistereo* h, const double* params, int iter, double* jte, double* G) {
    return oc_jacobian(h, params, iter, jte, G);
}

int mcc_omnistereo_optimize(mcc_omnistereo* h, int crit_type, int max_count, double eps, double* params_inout,
                            int* iters, double* last_change) {
    return oc_optimize(h, crit_type, max_count, eps, params_inout, iters, last_change);
}

int mcc_omnistereo_rms(mcc_omnistereo* h, const double* params, double* rms) { return oc_rms(h, params, rms); }

int mcc_omnistereo_time_steps(mcc_omnistereo* h, const double* params, int n_steps, double* ms_per_step) {
    return oc_time_steps(h, params, n_steps, ms_per_step);
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
