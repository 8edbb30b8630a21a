// mcc_omnirect_host.hpp -- host helpers of the omnidir rectification shared by mcc_omnirect_api.cpp and
// mcc_omnisgbm_api.cpp: the argument checks and the host part of initUndistortRectifyMap
// (src/omnidir.cpp:365-406).
#pragma once
#include <cmath>
#include <string>

#include "../../include/mcc_omnidir.h"
#include "mcc_omnicalib_host.hpp"
#include "mcc_omnirect_internal.h"

namespace {

constexpr int kOrMaxSize = 32767;   // a CV_16SC2 map cannot name a pixel past it

// general 3 x 3 inverse (Gauss-Jordan, partial pivoting); false for a zero pivot or a non-finite result
bool inv3(const double* A, double* X) {
    double m[3][6];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            m[r][c] = A[3 * r + c];
            m[r][3 + c] = r == c ? 1.0 : 0.0;
        }
    for (int k = 0; k < 3; ++k) {
        int p = k;
        for (int r = k + 1; r < 3; ++r)
            if (std::fabs(m[r][k]) > std::fabs(m[p][k])) p = r;
        if (!(std::fabs(m[p][k]) > 0.0)) return false;   // zero or NaN pivot
        if (p != k)
            for (int c = 0; c < 6; ++c) std::swap(m[p][c], m[k][c]);
        const double piv = m[k][k];
        for (int c = 0; c < 6; ++c) m[k][c] /= piv;
        for (int r = 0; r < 3; ++r) {
            if (r == k) continue;
            const double f = m[r][k];
            for (int c = 0; c < 6; ++c) m[r][c] -= f * m[k][c];
        }
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            X[3 * r + c] = m[r][3 + c];
            if (!std::isfinite(X[3 * r + c])) return false;
        }
    return true;
}

const double kEye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};

mcc::OrIntr or_intr(const double* K, const double* D, double xi) {
    mcc::OrIntr in{};
    in.f0 = K[0]; in.s = K[1]; in.c0 = K[2]; in.f1 = K[4]; in.c1 = K[5];
    in.xi = xi;
    if (D) { in.k1 = D[0]; in.k2 = D[1]; in.p1 = D[2]; in.p2 = D[3]; }
    return in;
}

bool or_flag_ok(int flags) { return flags >= MCC_OMNI_RECTIFY_PERSPECTIVE && flags <= MCC_OMNI_RECTIFY_STEREOGRAPHIC; }

int or_check_size(int w, int h, const char* what) {
    if (w < 1 || h < 1) return oc_fail(MCC_EINVAL, std::string(what) + " size must be positive");
    if (w > kOrMaxSize || h > kOrMaxSize)
        return oc_fail(MCC_EINVAL, std::string(what) + " size must not exceed " + std::to_string(kOrMaxSize));
    return MCC_OK;
}

int or_check_image(const void* p, int w, int h, int channels, long long stride, const char* what) {
    if (!p) return oc_fail(MCC_EINVAL, std::string("null ") + what + " image");
    int rc = or_check_size(w, h, what);
    if (rc) return rc;
    if (channels != 1 && channels != 3) return oc_fail(MCC_EINVAL, "channels must be 1 or 3");
    if (stride < (long long)w * channels)
        return oc_fail(MCC_EINVAL, std::string(what) + " stride is smaller than a row");
    return MCC_OK;
}

// the host part of initUndistortRectifyMap (:365-406): everything k_or_map takes but the maps
int or_map_args(const double* K, const double* D, double xi, const double* R, const double* P, int w, int h,
                int flags, mcc::OrMapArgs* a) {
    if (!K) return oc_fail(MCC_EINVAL, "null K");
    if (!or_flag_ok(flags)) return oc_fail(MCC_EINVAL, "flags must be one of MCC_OMNI_RECTIFY_*");
    int rc = or_check_size(w, h, "map");
    if (rc) return rc;
    const double* RR = R ? R : kEye;
    const double* PP = P ? P : K;
    double PR[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            PR[3 * r + c] = PP[3 * r] * RR[c] + PP[3 * r + 1] * RR[3 + c] + PP[3 * r + 2] * RR[6 + c];
    if (!inv3(PR, a->iKR)) return oc_fail(MCC_EINVAL, "P R is singular");
    if (!inv3(PP, a->iK)) return oc_fail(MCC_EINVAL, P ? "P is singular" : "K is singular");
    if (!inv3(RR, a->iR)) return oc_fail(MCC_EINVAL, "R is singular");
    a->in = or_intr(K, D, xi);
    a->w = w;
    a->h = h;
    return MCC_OK;
}

}  // namespace
