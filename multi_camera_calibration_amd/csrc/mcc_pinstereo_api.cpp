// mcc_pinstereo_api.cpp -- host side of mcc_stereo_calibrate, mcc_stereo_calib_mask and
// mcc_stereo_init_extrinsics (include/mcc.h).  The host checks the descriptor before any device call, finds
// the start with the calls the library already has (one pose-seed batch over both cameras' views at the given
// intrinsics, pin_seed_poses, or two mcc_calibrate_camera), takes the rig's start from the views' medians and
// hands the loop to PinLoop (mcc_pinloop_host.hpp) with its two launches, k_ps_lin and k_ps_try
// (mcc_pinstereo.hip).  E and F are computed here from the result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcc.h"
#include "mcc_pinloop_host.hpp"
#include "mcc_pinstereo_internal.h"

namespace {

constexpr int kKnownFlags = kPinCameraFlags | MCC_CALIB_FIX_INTRINSIC | MCC_CALIB_SAME_FOCAL_LENGTH |
                            MCC_CALIB_USE_EXTRINSIC_GUESS;
constexpr int kG = mcc::kPsGlob, kCam1 = 6, kCam2 = 18;

int ps_mask(const char* who, int flags, int nd, int* m, int* tie) {
    if (flags & ~kKnownFlags)
        return oc_fail(MCC_EINVAL, std::string(who) + ": unsupported flag bits " + std::to_string(flags & ~kKnownFlags));
    if (nd != 4 && nd != 5 && nd != 8) return oc_fail(MCC_EINVAL, std::string(who) + ": nd must be 4, 5 or 8");
    int cam[mcc::kPcGlob];
    const int rc = mcc_calib_mask(flags & kPinCameraFlags, nd, cam);
    if (rc) return rc;
    for (int k = 0; k < kG; ++k) {
        m[k] = k < kCam1 ? 1 : cam[(k - kCam1) % mcc::kPcGlob];
        tie[k] = -1;
    }
    if (flags & MCC_CALIB_FIX_INTRINSIC) {
        for (int k = kCam1; k < kG; ++k) m[k] = 0;
        return MCC_OK;
    }
    if (flags & MCC_CALIB_FIX_ASPECT_RATIO) {
        tie[kCam1] = kCam1 + 1;
        tie[kCam2] = kCam2 + 1;
    }
    if (flags & MCC_CALIB_SAME_FOCAL_LENGTH) {
        m[kCam2] = m[kCam2 + 1] = 0;
        tie[kCam2 + 1] = kCam1 + 1;
        if (!(flags & MCC_CALIB_FIX_ASPECT_RATIO)) tie[kCam2] = kCam1;
    }
    return MCC_OK;
}

// the rotation vector of R: the angle from atan2(s, c); the axis from the skew part, or within 1e-5 rad of pi
// from the column of (R + R^T) / 2 - c I with the largest diagonal entry (mcc_pnp_device.hpp's pnp_log_near_pi)
void log_host(const double* R, double* r) {
    const double vx = R[7] - R[5], vy = R[2] - R[6], vz = R[3] - R[1];
    const double s = 0.5 * std::sqrt(vx * vx + vy * vy + vz * vz);
    const double c = std::max(-1.0, std::min(1.0, (R[0] + R[4] + R[8] - 1) * 0.5));
    const double th = std::atan2(s, c);
    if (s >= 1e-5) {
        const double k = th / (2 * s);
        r[0] = k * vx; r[1] = k * vy; r[2] = k * vz;
        return;
    }
    if (c > 0) {   // R = I + [r]x to first order
        r[0] = 0.5 * vx; r[1] = 0.5 * vy; r[2] = 0.5 * vz;
        return;
    }
    const double d0 = R[0] - c, d1 = R[4] - c, d2 = R[8] - c;
    const double o01 = 0.5 * (R[1] + R[3]), o02 = 0.5 * (R[2] + R[6]), o12 = 0.5 * (R[5] + R[7]);
    const bool c0 = d0 >= d1 && d0 >= d2, c1 = !c0 && d1 >= d2;
    const double k0 = c0 ? d0 : c1 ? o01 : o02, k1 = c0 ? o01 : c1 ? d1 : o12, k2 = c0 ? o02 : c1 ? o12 : d2;
    double sc = th / std::sqrt(k0 * k0 + k1 * k1 + k2 * k2);
    if (k0 * vx + k1 * vy + k2 * vz < 0) sc = -sc;
    r[0] = sc * k0; r[1] = sc * k1; r[2] = sc * k2;
}

// the median as cv::stereoCalibrate takes it: the middle one, or the mean of the middle two
double median(std::vector<double> a) {
    std::sort(a.begin(), a.end());
    const size_t n = a.size();
    return n % 2 ? a[n / 2] : 0.5 * (a[n / 2 - 1] + a[n / 2]);
}

// r and r (1 - 2 pi / |r|) are the same rotation.  Within noise of a half turn some views' logarithms come out on
// one side of pi and some on the other, and a component-wise median over both is near 0.  So every view's vector
// is replaced by whichever of its two forms is nearer to a reference view's: the view that asks the fewest others
// to change (the first of equals), which one outlier cannot be unless n = 2.  Away from a half turn nobody changes
// and the columns are what log_host gave.
void same_side_of_pi(int n, std::vector<double>* col) {
    auto alt = [&](int v, double* a) {
        const double th = std::sqrt(col[0][v] * col[0][v] + col[1][v] * col[1][v] + col[2][v] * col[2][v]);
        if (!(th > 0)) return false;
        const double k = 1.0 - 2.0 * M_PI / th;
        for (int i = 0; i < 3; ++i) a[i] = k * col[i][v];
        return true;
    };
    auto nearer = [&](int v, int ref, double* a) {   // is view v's other form nearer to ref's vector than its own?
        if (v == ref || !alt(v, a)) return false;
        double d0 = 0, d1 = 0;
        for (int i = 0; i < 3; ++i) {
            d0 += (col[i][v] - col[i][ref]) * (col[i][v] - col[i][ref]);
            d1 += (a[i] - col[i][ref]) * (a[i] - col[i][ref]);
        }
        return d1 < d0;
    };
    double a[3];
    int ref = 0, fewest = n + 1;
    for (int c = 0; c < n && fewest > 0; ++c) {
        int changes = 0;
        for (int v = 0; v < n; ++v) changes += nearer(v, c, a);
        if (changes < fewest) {
            fewest = changes;
            ref = c;
        }
    }
    if (fewest == 0) return;
    for (int v = 0; v < n; ++v)   // (the reference's own vector stays, so every view is compared with the same one)
        if (nearer(v, ref, a))
            for (int i = 0; i < 3; ++i) col[i][v] = a[i];
}

void init_extrinsics(int n, const double* r1, const double* t1, const double* r2, const double* t2, double* om, double* T) {
    std::vector<double> col[6];
    for (int v = 0; v < n; ++v) {
        double R1[9], R2[9], R1t[9], R[9], o[3];
        rodrigues_host(r1 + 3 * (size_t)v, R1);
        rodrigues_host(r2 + 3 * (size_t)v, R2);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R1t[i * 3 + j] = R1[j * 3 + i];
        mul3(R2, R1t, R);
        log_host(R, o);
        const double* a = t1 + 3 * (size_t)v;
        for (int k = 0; k < 3; ++k) {
            col[k].push_back(o[k]);
            col[3 + k].push_back(t2[3 * (size_t)v + k] - (R[k * 3] * a[0] + R[k * 3 + 1] * a[1] + R[k * 3 + 2] * a[2]));
        }
    }
    same_side_of_pi(n, col);
    for (int k = 0; k < 3; ++k) {
        om[k] = median(col[k]);
        T[k] = median(col[3 + k]);
    }
}

// E = [T]x R and F = K2^-T E K1^-1 scaled to F[8] = 1 (when it is not 0); K as fx fy cx cy
void essential_fundamental(const double* R, const double* T, const double* k1, const double* k2, double* E, double* F) {
    const double Tx[9] = {0, -T[2], T[1], T[2], 0, -T[0], -T[1], T[0], 0};
    double Eh[9];
    mul3(Tx, R, Eh);
    if (E) std::memcpy(E, Eh, sizeof Eh);
    if (!F) return;
    const double K1i[9] = {1 / k1[0], 0, -k1[2] / k1[0], 0, 1 / k1[1], -k1[3] / k1[1], 0, 0, 1};
    const double K2it[9] = {1 / k2[0], 0, 0, 0, 1 / k2[1], 0, -k2[2] / k2[0], -k2[3] / k2[1], 1};
    double A[9], Fh[9];
    mul3(K2it, Eh, A);
    mul3(A, K1i, Fh);
    const double sc = std::fabs(Fh[8]) > 0 ? 1.0 / Fh[8] : 1.0;
    for (int k = 0; k < 9; ++k) F[k] = Fh[k] * sc;
}

// SAME_FOCAL_LENGTH's start: both cameras at the mean of their fx and of their fy, then each camera's own ratio
void same_focal_start(double* g, const double* aspect) {
    const double fx = 0.5 * (g[kCam1] + g[kCam2]), fy = 0.5 * (g[kCam1 + 1] + g[kCam2 + 1]);
    g[kCam1] = g[kCam2] = fx;
    g[kCam1 + 1] = g[kCam2 + 1] = fy;
    for (int c = 0; c < 2; ++c)
        if (aspect[c] > 0) g[kCam1 + mcc::kPcGlob * c] = aspect[c] * g[kCam1 + mcc::kPcGlob * c + 1];
}

}  // namespace

extern "C" int mcc_stereo_calib_mask(int flags, int nd, int* mask, int* tie) {
    if (!mask || !tie) return oc_fail(MCC_EINVAL, "stereo_calib_mask: null argument");
    return ps_mask("stereo_calib_mask", flags, nd, mask, tie);
}

extern "C" int mcc_stereo_init_extrinsics(int n_views, const double* rvec1, const double* tvec1, const double* rvec2,
                                          const double* tvec2, double* om, double* T) {
    if (!rvec1 || !tvec1 || !rvec2 || !tvec2 || !om || !T) return oc_fail(MCC_EINVAL, "stereo_init_extrinsics: null argument");
    if (n_views < 1) return oc_fail(MCC_EINVAL, "stereo_init_extrinsics: n_views must be positive");
    init_extrinsics(n_views, rvec1, tvec1, rvec2, tvec2, om, T);
    return MCC_OK;
}

extern "C" int mcc_stereo_epipolar(const double* R, const double* T, const double* K1, const double* K2, double* E,
                                   double* F) {
    if (!R || !T || !K1 || !K2) return oc_fail(MCC_EINVAL, "stereo_epipolar: null argument");
    const double k1[4] = {K1[0], K1[4], K1[2], K1[5]}, k2[4] = {K2[0], K2[4], K2[2], K2[5]};
    if (F && !(k1[0] != 0.0 && k1[1] != 0.0 && k2[0] != 0.0 && k2[1] != 0.0))
        return oc_fail(MCC_EINVAL, "stereo_epipolar: a zero focal length");
    essential_fundamental(R, T, k1, k2, E, F);
    return MCC_OK;
}

extern "C" int mcc_stereo_calibrate(const mcc_stereo_calib_desc* d, double* K1, double* D1, double* K2, double* D2, double* R,
                                    double* T, double* E, double* F, double* rvec, double* tvec, double* view_rms,
                                    double* rms, int* iterations, int* status, double* device_ms) {
    const std::string w = "stereo_calibrate";
    if (!d || !K1 || !D1 || !K2 || !D2) return oc_fail(MCC_EINVAL, w + ": null argument");
    const double* const img[2] = {d->img1, d->img2};
    int rc = pin_check_views(w, d->n_views, d->view_off, d->obj, img, 2, d->image_width, d->image_height);
    if (rc) return rc;
    const int n = d->n_views, flags = d->flags, nd = d->nd;
    int m[kG], tie[kG];
    if ((rc = ps_mask("stereo_calibrate", flags, nd, m, tie))) return rc;
    if ((rc = pin_check_criteria(w, d->crit_type, d->max_count))) return rc;
    const bool fixi = flags & MCC_CALIB_FIX_INTRINSIC, guess = flags & MCC_CALIB_USE_INTRINSIC_GUESS;
    const bool same = !fixi && (flags & MCC_CALIB_SAME_FOCAL_LENGTH);
    if ((flags & MCC_CALIB_USE_EXTRINSIC_GUESS) && (!R || !T))
        return oc_fail(MCC_EINVAL, w + ": USE_EXTRINSIC_GUESS needs R and T");
    double* Kc[2] = {K1, K2};
    double* Dc[2] = {D1, D2};
    double aspect[2] = {0.0, 0.0};
    for (int c = 0; c < 2; ++c) {
        const double* K = Kc[c];
        if (fixi && !(K[0] != 0.0 && K[4] != 0.0 && std::isfinite(K[0]) && std::isfinite(K[4])))
            return oc_fail(MCC_EINVAL, w + ": FIX_INTRINSIC needs the camera matrices (K" + std::to_string(c + 1) +
                                           " has a zero focal length)");
        if (!fixi && (flags & MCC_CALIB_FIX_ASPECT_RATIO)) {
            if (!(K[0] != 0.0 && K[4] != 0.0 && std::isfinite(K[0] / K[4])))
                return oc_fail(MCC_EINVAL, w + ": FIX_ASPECT_RATIO needs non-zero focal lengths in K" + std::to_string(c + 1));
            aspect[c] = K[0] / K[4];
        }
    }

    // ---- the start: the cameras' slots and both cameras' pose of every view
    double g[kG] = {0};
    std::vector<double> rv[2], tv[2];
    for (auto& a : rv) a.resize(3 * (size_t)n);
    for (auto& a : tv) a.resize(3 * (size_t)n);
    double* const rp[2] = {rv[0].data(), rv[1].data()};
    double* const tp[2] = {tv[0].data(), tv[1].data()};
    if (fixi || guess) {
        for (int c = 0; c < 2; ++c) {
            double* gc = g + kCam1 + mcc::kPcGlob * c;
            pin_pack(Kc[c], Dc[c], nd, gc);
            if (!fixi) pin_start_edits(flags, nd, aspect[c], gc);
        }
        if (same) same_focal_start(g, aspect);   // (before the seeds, so that they are the poses at the start itself)
        if ((rc = pin_seed_poses(w, n, d->view_off, d->obj, img, 2, g + kCam1, d->device, rp, tp))) return rc;
    } else {
        for (int c = 0; c < 2; ++c) {
            mcc_calib_desc cd{};
            cd.n_views = n;
            cd.view_off = d->view_off;
            cd.obj = d->obj;
            cd.img = img[c];
            cd.image_width = d->image_width;
            cd.image_height = d->image_height;
            cd.flags = flags & kPinCameraFlags;
            cd.nd = nd;
            cd.crit_type = d->crit_type;
            cd.max_count = d->max_count;
            cd.eps = d->eps;
            cd.device = d->device;
            double Kt[9], Dt[8] = {0};
            std::memcpy(Kt, Kc[c], sizeof Kt);
            if ((rc = mcc_calibrate_camera(&cd, Kt, Dt, rp[c], tp[c], nullptr, nullptr, nullptr, nullptr, nullptr)))
                return oc_fail(rc, w + ": camera " + std::to_string(c + 1) + ": " + mcc_last_error());
            pin_pack(Kt, Dt, nd, g + kCam1 + mcc::kPcGlob * c);
        }
        if (same) same_focal_start(g, aspect);
    }
    // ---- the rig's start
    if (flags & MCC_CALIB_USE_EXTRINSIC_GUESS) {
        log_host(R, g);
        for (int k = 0; k < 3; ++k) g[3 + k] = T[k];
    } else {
        init_extrinsics(n, rp[0], tp[0], rp[1], tp[1], g, g + 3);
    }
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(g[k])) return oc_fail(MCC_EINVAL, w + ": the rig's start is not finite");
    int mask = 0;
    for (int k = 0; k < kG; ++k) mask |= m[k] << k;

    // ---- the loop
    PinLoop lp;
    const PinShape shape{kG, mcc::kPsLinN, mcc::kPsYz, mcc::kPsCtrN, 2};
    if ((rc = lp.init(d->device, n, d->view_off, d->obj, img, rp[0], tp[0], g, shape, d->crit_type, d->max_count, d->eps)))
        return rc;
    mcc::PsArgs a{};
    lp.fill(a);
    a.img1 = lp.img[0].p;
    a.img2 = lp.img[1].p;
    a.mask = mask;
    a.same = same ? 1 : 0;
    a.aspect1 = aspect[0];
    a.aspect2 = aspect[1];
    if ((rc = lp.run(w, [&] { return mcc_launch_ps_lin(a, nullptr); }, [&] { return mcc_launch_ps_try(a, nullptr); }, d->trials,
                     device_ms)))
        return rc;

    // ---- results
    std::vector<double> esq(2 * (size_t)n);
    if ((rc = lp.download(g, rvec, tvec, esq.data()))) return rc;
    if (!fixi)   // (fixed intrinsics are not rewritten: they stay the caller's bits, K's off-diagonals included)
        for (int c = 0; c < 2; ++c) pin_unpack(g + kCam1 + mcc::kPcGlob * c, nd, Kc[c], Dc[c]);
    double Rh[9];
    rodrigues_host(g, Rh);
    if (R) std::memcpy(R, Rh, sizeof Rh);
    if (T) std::memcpy(T, g + 3, 3 * sizeof(double));
    essential_fundamental(Rh, g + 3, g + kCam1, g + kCam2, E, F);
    if (view_rms)
        for (int v = 0; v < n; ++v)
            for (int c = 0; c < 2; ++c)
                view_rms[2 * (size_t)v + c] = std::sqrt(esq[2 * (size_t)v + c] / (double)(lp.off[v + 1] - lp.off[v]));
    if (rms) *rms = std::sqrt(lp.s.err / (2.0 * (double)lp.corners));
    if (iterations) *iterations = lp.s.iter;
    if (status) *status = lp.s.status;
    return MCC_OK;
}
