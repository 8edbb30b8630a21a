// mcc_pinstereo_api.cpp -- host side of mcc_stereo_calibrate, mcc_stereo_calib_mask and
// mcc_stereo_init_extrinsics (include/mcc.h).  The host checks the descriptor before any device call, finds
// the start with the calls the library already has (one mcc_solve_pnp_batch over both cameras' views at the
// given intrinsics, or two mcc_calibrate_camera), takes the rig's start from the views' medians and then only
// launches trials (k_ps_lin + k_ps_try, mcc_pinstereo.hip) in batches, reading the device-resident loop state
// between batches.  E and F are computed here from the result.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcc.h"
#include "mcc_omnicalib_host.hpp"
#include "mcc_pinstereo_internal.h"

namespace {

constexpr int kCameraFlags = MCC_CALIB_USE_INTRINSIC_GUESS | MCC_CALIB_FIX_ASPECT_RATIO | MCC_CALIB_FIX_PRINCIPAL_POINT |
                             MCC_CALIB_ZERO_TANGENT_DIST | MCC_CALIB_FIX_FOCAL_LENGTH | MCC_CALIB_FIX_K1 |
                             MCC_CALIB_FIX_K2 | MCC_CALIB_FIX_K3 | MCC_CALIB_FIX_K4 | MCC_CALIB_FIX_K5 |
                             MCC_CALIB_FIX_K6 | MCC_CALIB_RATIONAL_MODEL;
constexpr int kKnownFlags = kCameraFlags | MCC_CALIB_FIX_INTRINSIC | MCC_CALIB_SAME_FOCAL_LENGTH |
                            MCC_CALIB_USE_EXTRINSIC_GUESS;
constexpr int kTrialBatch = 8;       // trials enqueued between two reads of the state
constexpr int kEpsOnlyCount = 1000;  // accepted steps at most when the criteria have no count
constexpr int kG = mcc::kPsGlob, kCam1 = 6, kCam2 = 18;

int ps_mask(const char* who, int flags, int nd, int* m, int* tie) {
    if (flags & ~kKnownFlags)
        return oc_fail(MCC_EINVAL, std::string(who) + ": unsupported flag bits " + std::to_string(flags & ~kKnownFlags));
    if (nd != 4 && nd != 5 && nd != 8) return oc_fail(MCC_EINVAL, std::string(who) + ": nd must be 4, 5 or 8");
    int cam[mcc::kPcGlob];
    const int rc = mcc_calib_mask(flags & kCameraFlags, nd, cam);
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

void mul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
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

struct PsEvents {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~PsEvents() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

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
    if (d->n_views < 1) return oc_fail(MCC_EINVAL, w + ": n_views must be positive");
    if (!d->view_off || !d->obj || !d->img1 || !d->img2) return oc_fail(MCC_EINVAL, w + ": null pointer in the descriptor");
    if (d->image_width <= 0 || d->image_height <= 0) return oc_fail(MCC_EINVAL, w + ": the image size must be positive");
    if (d->view_off[0] < 0) return oc_fail(MCC_EINVAL, w + ": view_off[0] is negative");
    const int n = d->n_views, flags = d->flags, nd = d->nd;
    for (int v = 0; v < n; ++v) {
        const int c = d->view_off[v + 1] - d->view_off[v];
        if (c < 4 || c > mcc::kPcMaxCorners)
            return oc_fail(MCC_EINVAL, w + ": view " + std::to_string(v) + " has " + std::to_string(c) + " corners, 4 to " +
                                           std::to_string(mcc::kPcMaxCorners) + " are supported");
    }
    int m[kG], tie[kG], rc;
    if ((rc = ps_mask("stereo_calibrate", flags, nd, m, tie))) return rc;
    if (d->crit_type < 1 || d->crit_type > 3) return oc_fail(MCC_EINVAL, w + ": crit_type must be 1, 2 or 3");
    if ((d->crit_type & MCC_CRIT_COUNT) && d->max_count < 1) return oc_fail(MCC_EINVAL, w + ": max_count must be positive");
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
    const size_t first = (size_t)d->view_off[0], corners = (size_t)d->view_off[n] - first;
    std::vector<int> off((size_t)n + 1);
    for (int v = 0; v <= n; ++v) off[v] = d->view_off[v] - d->view_off[0];
    const double* img[2] = {d->img1 + 2 * first, d->img2 + 2 * first};
    double g[kG] = {0};
    std::vector<double> rv[2], tv[2];
    for (auto& a : rv) a.resize(3 * (size_t)n);
    for (auto& a : tv) a.resize(3 * (size_t)n);
    if (fixi || guess) {
        for (int c = 0; c < 2; ++c) {
            double* gc = g + kCam1 + mcc::kPcGlob * c;
            gc[0] = Kc[c][0]; gc[1] = Kc[c][4]; gc[2] = Kc[c][2]; gc[3] = Kc[c][5];
            for (int k = 0; k < nd; ++k) gc[4 + k] = Dc[c][k];
            if (!fixi) {
                if (flags & MCC_CALIB_ZERO_TANGENT_DIST) gc[6] = gc[7] = 0.0;
                if (nd == 4) gc[8] = 0.0;
                if (aspect[c] > 0) gc[0] = aspect[c] * gc[1];
            }
        }
        if (same) same_focal_start(g, aspect);   // (before the seeds, so that they are the poses at the start itself)
        // one solvePnP batch over 2 n views: camera 1's, then camera 2's
        std::vector<int> off2(2 * (size_t)n + 1), cam(2 * (size_t)n);
        std::vector<double> obj2(6 * corners), img2(4 * corners), Ks(18), Ds(16), r(6 * (size_t)n), t(6 * (size_t)n),
            e(2 * (size_t)n);
        std::vector<int> st(2 * (size_t)n);
        for (int c = 0; c < 2; ++c) {
            const double* gc = g + kCam1 + mcc::kPcGlob * c;
            const double Kn[9] = {gc[0], 0, gc[2], 0, gc[1], gc[3], 0, 0, 1};
            std::memcpy(&Ks[9 * c], Kn, sizeof Kn);
            std::memcpy(&Ds[8 * c], gc + 4, 8 * sizeof(double));
            std::memcpy(&obj2[3 * corners * c], d->obj + 3 * first, 3 * corners * sizeof(double));
            std::memcpy(&img2[2 * corners * c], img[c], 2 * corners * sizeof(double));
            for (int v = 0; v < n; ++v) {
                off2[(size_t)c * n + v] = (int)(corners * c) + off[v];
                cam[(size_t)c * n + v] = c;
            }
        }
        off2[2 * (size_t)n] = (int)(2 * corners);
        mcc_pnp_desc pd{};
        pd.n_views = 2 * n;
        pd.view_off = off2.data();
        pd.obj = obj2.data();
        pd.img = img2.data();
        pd.view_cam = cam.data();
        pd.n_cams = 2;
        pd.K = Ks.data();
        pd.D = Ds.data();
        pd.nd = 8;
        pd.max_iter = 50;
        pd.device = d->device;
        if ((rc = mcc_solve_pnp_batch(&pd, r.data(), t.data(), e.data(), st.data(), nullptr))) return rc;
        for (int c = 0; c < 2; ++c)
            for (int v = 0; v < n; ++v) {
                const size_t i = (size_t)c * n + v;
                if (st[i] != MCC_PNP_SOLVED)
                    return oc_fail(MCC_EINVAL, w + ": no pose seed for view " + std::to_string(v) + " in camera " +
                                                   std::to_string(c + 1) + " (solvePnP status " + std::to_string(st[i]) + ")");
                for (int k = 0; k < 3; ++k) {
                    rv[c][3 * (size_t)v + k] = r[3 * i + k];
                    tv[c][3 * (size_t)v + k] = t[3 * i + k];
                }
            }
    } else {
        for (int c = 0; c < 2; ++c) {
            mcc_calib_desc cd{};
            cd.n_views = n;
            cd.view_off = off.data();
            cd.obj = d->obj + 3 * first;
            cd.img = img[c];
            cd.image_width = d->image_width;
            cd.image_height = d->image_height;
            cd.flags = flags & kCameraFlags;
            cd.nd = nd;
            cd.crit_type = d->crit_type;
            cd.max_count = d->max_count;
            cd.eps = d->eps;
            cd.device = d->device;
            double Kt[9], Dt[8] = {0};
            std::memcpy(Kt, Kc[c], sizeof Kt);
            if ((rc = mcc_calibrate_camera(&cd, Kt, Dt, rv[c].data(), tv[c].data(), nullptr, nullptr, nullptr, nullptr, nullptr)))
                return oc_fail(rc, w + ": camera " + std::to_string(c + 1) + ": " + mcc_last_error());
            double* gc = g + kCam1 + mcc::kPcGlob * c;
            gc[0] = Kt[0]; gc[1] = Kt[4]; gc[2] = Kt[2]; gc[3] = Kt[5];
            for (int k = 0; k < nd; ++k) gc[4 + k] = Dt[k];
        }
        if (same) same_focal_start(g, aspect);
    }
    // ---- the rig's start
    if (flags & MCC_CALIB_USE_EXTRINSIC_GUESS) {
        log_host(R, g);
        for (int k = 0; k < 3; ++k) g[3 + k] = T[k];
    } else {
        init_extrinsics(n, rv[0].data(), tv[0].data(), rv[1].data(), tv[1].data(), g, g + 3);
    }
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(g[k])) return oc_fail(MCC_EINVAL, w + ": the rig's start is not finite");
    std::vector<double> x0(6 * (size_t)n);
    for (int v = 0; v < n; ++v)
        for (int k = 0; k < 3; ++k) {
            x0[6 * (size_t)v + k] = rv[0][3 * (size_t)v + k];
            x0[6 * (size_t)v + 3 + k] = tv[0][3 * (size_t)v + k];
        }
    int mask = 0;
    for (int k = 0; k < kG; ++k) mask |= m[k] << k;

    // ---- device buffers
    const int group_size = std::max(1, (int)std::ceil(std::sqrt((double)n)));
    const int n_groups = (n + group_size - 1) / group_size;
    OCCHK(hipSetDevice(d->device));
    DBuf<int> d_off, d_cnt;
    DBuf<double> d_obj, d_img1, d_img2, d_x, d_xt, d_glob, d_dc, d_lin, d_Yz, d_contrib, d_gsum, d_esq, d_esq_t, d_egs;
    DBuf<mcc::PcState> d_st;
    OCCHK(d_off.upload(off.data(), off.size()));
    OCCHK(d_obj.upload(d->obj + 3 * first, 3 * corners));
    OCCHK(d_img1.upload(img[0], 2 * corners));
    OCCHK(d_img2.upload(img[1], 2 * corners));
    OCCHK(d_x.upload(x0.data(), x0.size()));
    OCCHK(d_xt.alloc(6 * (size_t)n));
    OCCHK(d_glob.upload(g, kG));
    OCCHK(d_dc.alloc(kG));
    OCCHK(d_lin.alloc((size_t)n * mcc::kPsLinN));
    OCCHK(d_Yz.alloc((size_t)n * mcc::kPsYz));
    OCCHK(d_contrib.alloc((size_t)n * mcc::kPsCtrN));
    OCCHK(d_gsum.alloc((size_t)n_groups * mcc::kPsCtrN));
    OCCHK(d_esq.alloc(2 * (size_t)n));
    OCCHK(d_esq_t.alloc(2 * (size_t)n));
    OCCHK(d_egs.alloc((size_t)n_groups));
    OCCHK(d_cnt.alloc(2 * ((size_t)n_groups + 1)));
    OCCHK(hipMemset(d_cnt.p, 0, sizeof(int) * 2 * ((size_t)n_groups + 1)));
    mcc::PcState s{};
    s.init = 1;
    s.relin = 1;
    s.crit_type = d->crit_type;
    s.max_count = (d->crit_type & MCC_CRIT_COUNT) ? d->max_count : kEpsOnlyCount;
    if (!(d->crit_type & MCC_CRIT_COUNT)) s.crit_type |= MCC_CRIT_COUNT;
    s.eps = d->eps;
    s.lambda = 1e-3;
    OCCHK(d_st.upload(&s, 1));
    const mcc::PsArgs a{n, d_off.p, d_obj.p, d_img1.p, d_img2.p, mask, same ? 1 : 0, aspect[0], aspect[1], d_x.p, d_xt.p,
                        d_glob.p, d_dc.p, d_lin.p, d_Yz.p, d_contrib.p, d_gsum.p, d_esq.p, d_esq_t.p, d_egs.p, d_cnt.p,
                        d_st.p, group_size, n_groups};

    // ---- the loop: at most ten rejections per accepted step, so 11 max_count trials in all
    PsEvents ev;
    OCCHK(hipEventCreate(&ev.ev[0]));
    OCCHK(hipEventCreate(&ev.ev[1]));
    OCCHK(hipEventRecord(ev.ev[0], nullptr));
    OCCHK(mcc_launch_ps_try(a, nullptr));   // the error of the start
    const long long cap = 11LL * s.max_count;
    for (long long launched = 0; launched < cap;) {
        for (int b = 0; b < kTrialBatch && launched < cap; ++b, ++launched) {
            OCCHK(mcc_launch_ps_lin(a, nullptr));
            OCCHK(mcc_launch_ps_try(a, nullptr));
        }
        OCCHK(hipMemcpy(&s, d_st.p, sizeof s, hipMemcpyDeviceToHost));
        if (s.done) break;
    }
    OCCHK(hipEventRecord(ev.ev[1], nullptr));
    OCCHK(hipEventSynchronize(ev.ev[1]));
    OCCHK(hipMemcpy(&s, d_st.p, sizeof s, hipMemcpyDeviceToHost));
    if (d->trials) *d->trials = s.trials;
    if (device_ms) {
        float ms = 0.f;
        OCCHK(hipEventElapsedTime(&ms, ev.ev[0], ev.ev[1]));
        *device_ms = (double)ms;
    }
    if (s.status == mcc::kPcNotFinite) return oc_fail(MCC_EINVAL, w + ": the reprojection error of the start is not finite");
    if (!s.done) return oc_fail(MCC_EINVAL, w + ": the loop did not terminate");

    // ---- results
    std::vector<double> esq(2 * (size_t)n);
    OCCHK(hipMemcpy(x0.data(), d_x.p, sizeof(double) * x0.size(), hipMemcpyDeviceToHost));
    OCCHK(hipMemcpy(g, d_glob.p, sizeof g, hipMemcpyDeviceToHost));
    OCCHK(hipMemcpy(esq.data(), d_esq.p, sizeof(double) * esq.size(), hipMemcpyDeviceToHost));
    for (int c = 0; c < 2; ++c) {
        const double* gc = g + kCam1 + mcc::kPcGlob * c;
        const double Kn[9] = {gc[0], 0, gc[2], 0, gc[1], gc[3], 0, 0, 1};
        if (!fixi) {   // (fixed intrinsics are not rewritten: they stay the caller's bits, K's off-diagonals included)
            std::memcpy(Kc[c], Kn, sizeof Kn);
            for (int k = 0; k < nd; ++k) Dc[c][k] = gc[4 + k];
        }
    }
    double Rh[9];
    rodrigues_host(g, Rh);
    if (R) std::memcpy(R, Rh, sizeof Rh);
    if (T) std::memcpy(T, g + 3, 3 * sizeof(double));
    essential_fundamental(Rh, g + 3, g + kCam1, g + kCam2, E, F);
    for (int v = 0; v < n; ++v) {
        for (int k = 0; k < 3; ++k) {
            if (rvec) rvec[3 * (size_t)v + k] = x0[6 * (size_t)v + k];
            if (tvec) tvec[3 * (size_t)v + k] = x0[6 * (size_t)v + 3 + k];
        }
        if (view_rms)
            for (int c = 0; c < 2; ++c) view_rms[2 * (size_t)v + c] = std::sqrt(esq[2 * (size_t)v + c] / (double)(off[v + 1] - off[v]));
    }
    if (rms) *rms = std::sqrt(s.err / (2.0 * (double)corners));
    if (iterations) *iterations = s.iter;
    if (status) *status = s.status;
    return MCC_OK;
}
