// mcc_pincalib_api.cpp -- host side of mcc_calibrate_camera, mcc_init_camera_matrix and mcc_calib_mask
// (include/mcc.h).  The host checks the descriptor before any device call, finds the start (the closed
// form of cv::initCameraMatrix2D, or the caller's guess), seeds the poses (pin_seed_poses) and hands the
// loop to PinLoop (mcc_pinloop_host.hpp) with its two launches, k_pc_lin and k_pc_try (mcc_pincalib.hip);
// what is left here is the start, the unpacking of the slots and the rms.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcc.h"
#include "mcc_pinloop_host.hpp"

namespace {

int pc_mask(const char* who, int flags, int nd, int* m) {
    if (flags & ~kPinCameraFlags)
        return oc_fail(MCC_EINVAL, std::string(who) + ": unsupported flag bits " + std::to_string(flags & ~kPinCameraFlags) +
                                       " (thin prism, tilted sensor and the solver choices are not restated)");
    if (nd != 4 && nd != 5 && nd != 8) return oc_fail(MCC_EINVAL, std::string(who) + ": nd must be 4, 5 or 8");
    const bool focal = !(flags & MCC_CALIB_FIX_FOCAL_LENGTH), pp = !(flags & MCC_CALIB_FIX_PRINCIPAL_POINT);
    const bool tang = !(flags & MCC_CALIB_ZERO_TANGENT_DIST);
    const bool rat = (flags & MCC_CALIB_RATIONAL_MODEL) && nd == 8;
    m[0] = focal && !(flags & MCC_CALIB_FIX_ASPECT_RATIO);
    m[1] = focal;
    m[2] = m[3] = pp;
    m[4] = !(flags & MCC_CALIB_FIX_K1);
    m[5] = !(flags & MCC_CALIB_FIX_K2);
    m[6] = m[7] = tang;
    m[8] = nd >= 5 && !(flags & MCC_CALIB_FIX_K3);
    m[9] = rat && !(flags & MCC_CALIB_FIX_K4);
    m[10] = rat && !(flags & MCC_CALIB_FIX_K5);
    m[11] = rat && !(flags & MCC_CALIB_FIX_K6);
    return MCC_OK;
}

// what both entry points require of the views; *planar = every Z is exactly 0
int pc_check_views(const char* who, const mcc_calib_desc* d, bool* planar) {
    const std::string w(who);
    if (!d) return oc_fail(MCC_EINVAL, w + ": null descriptor");
    const int rc = pin_check_views(w, d->n_views, d->view_off, d->obj, &d->img, 1, d->image_width, d->image_height);
    if (rc) return rc;
    *planar = true;
    for (int i = d->view_off[0]; i < d->view_off[d->n_views]; ++i)
        if (d->obj[3 * (size_t)i + 2] != 0.0) *planar = false;
    return MCC_OK;
}

// cyclic Jacobi on a symmetric 9 x 9: the eigenvector of the smallest eigenvalue
void smallest_eigvec9(const double* A0, double* h) {
    const int n = 9;
    double A[81], V[81];
    std::memcpy(A, A0, sizeof A);
    for (int i = 0; i < 81; ++i) V[i] = (i % 10 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) (i == j ? dia : off) += A[i * n + j] * A[i * n + j];
        if (!(off > 1e-40 * dia)) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (!(std::fabs(apq) > 1e-300)) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq;
                    A[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk;
                    A[q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    int im = 0;
    for (int k = 1; k < n; ++k)
        if (A[k * n + k] < A[im * n + im]) im = k;
    for (int k = 0; k < n; ++k) h[k] = V[k * n + im];
}

// H [X Y 1]^T ~ [u v 1]^T by the normalised DLT (host/pnp.cpp::homography's form, on pixels)
void homography(const double* obj, const double* img, int n, double* H) {
    double mx = 0, my = 0, mu = 0, mv = 0;
    for (int i = 0; i < n; ++i) {
        mx += obj[3 * i]; my += obj[3 * i + 1];
        mu += img[2 * i]; mv += img[2 * i + 1];
    }
    mx /= n; my /= n; mu /= n; mv /= n;
    double sx = 0, su = 0;
    for (int i = 0; i < n; ++i) {
        sx += std::hypot(obj[3 * i] - mx, obj[3 * i + 1] - my);
        su += std::hypot(img[2 * i] - mu, img[2 * i + 1] - mv);
    }
    sx = std::sqrt(2.0) * n / std::max(sx, 1e-300);
    su = std::sqrt(2.0) * n / std::max(su, 1e-300);
    double AtA[81] = {0};
    for (int i = 0; i < n; ++i) {
        const double X = (obj[3 * i] - mx) * sx, Y = (obj[3 * i + 1] - my) * sx;
        const double u = (img[2 * i] - mu) * su, v = (img[2 * i + 1] - mv) * su;
        const double r1[9] = {X, Y, 1, 0, 0, 0, -u * X, -u * Y, -u};
        const double r2[9] = {0, 0, 0, X, Y, 1, -v * X, -v * Y, -v};
        for (int a = 0; a < 9; ++a)
            for (int b = 0; b < 9; ++b) AtA[a * 9 + b] += r1[a] * r1[b] + r2[a] * r2[b];
    }
    double Hn[9], T1[9];
    smallest_eigvec9(AtA, Hn);
    const double Tx[9] = {sx, 0, -sx * mx, 0, sx, -sx * my, 0, 0, 1};
    const double Tui[9] = {1 / su, 0, mu, 0, 1 / su, mv, 0, 0, 1};
    mul3(Hn, Tx, T1);
    mul3(Tui, T1, H);
}

int pc_init_matrix(const char* who, const mcc_calib_desc* d, double aspect, double* K) {
    const double cx = (d->image_width - 1) * 0.5, cy = (d->image_height - 1) * 0.5;
    // normal equations of the 2n x 2 system in (1 / fx^2, 1 / fy^2)
    double a00 = 0, a01 = 0, a11 = 0, b0 = 0, b1 = 0;
    for (int v = 0; v < d->n_views; ++v) {
        const int off = d->view_off[v], n = d->view_off[v + 1] - off;
        double H[9];
        homography(d->obj + 3 * (size_t)off, d->img + 2 * (size_t)off, n, H);
        for (int j = 0; j < 3; ++j) {
            H[j] -= cx * H[6 + j];
            H[3 + j] -= cy * H[6 + j];
        }
        double h[3] = {H[0], H[3], H[6]}, w[3] = {H[1], H[4], H[7]}, d1[3], d2[3];
        for (int k = 0; k < 3; ++k) {
            d1[k] = (h[k] + w[k]) * 0.5;
            d2[k] = (h[k] - w[k]) * 0.5;
        }
        auto unit = [](double* p) {
            const double s = 1.0 / std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
            for (int k = 0; k < 3; ++k) p[k] *= s;
        };
        unit(h); unit(w); unit(d1); unit(d2);
        const double rows[2][3] = {{h[0] * w[0], h[1] * w[1], -h[2] * w[2]}, {d1[0] * d2[0], d1[1] * d2[1], -d1[2] * d2[2]}};
        for (const auto& r : rows) {
            a00 += r[0] * r[0]; a01 += r[0] * r[1]; a11 += r[1] * r[1];
            b0 += r[0] * r[2]; b1 += r[1] * r[2];
        }
    }
    const double det = a00 * a11 - a01 * a01;
    const double f0 = (a11 * b0 - a01 * b1) / det, f1 = (a00 * b1 - a01 * b0) / det;
    double fx = std::sqrt(std::fabs(1.0 / f0)), fy = std::sqrt(std::fabs(1.0 / f1));
    if (!(det > 1e-14 * a00 * a11) || !(fx > 0 && fx < 1e300) || !(fy > 0 && fy < 1e300))
        return oc_fail(MCC_ENOTPD, std::string(who) + ": the views do not determine the focal lengths (every target "
                                                      "parallel to the image plane, or too few views)");
    if (aspect > 0) {
        fy = (fx + fy) / (aspect + 1.0);
        fx = aspect * fy;
    }
    const double g[4] = {fx, fy, cx, cy};
    pin_matrix(g, K);
    return MCC_OK;
}

}  // namespace

extern "C" int mcc_calib_mask(int flags, int nd, int* mask) {
    if (!mask) return oc_fail(MCC_EINVAL, "calib_mask: null argument");
    return pc_mask("calib_mask", flags, nd, mask);
}

extern "C" int mcc_init_camera_matrix(const mcc_calib_desc* d, double aspect_ratio, double* K) {
    if (!K) return oc_fail(MCC_EINVAL, "init_camera_matrix: null argument");
    bool planar = false;
    const int rc = pc_check_views("init_camera_matrix", d, &planar);
    if (rc) return rc;
    if (!planar) return oc_fail(MCC_EINVAL, "init_camera_matrix: an object point has Z != 0 (planar targets only)");
    if (!(aspect_ratio >= 0)) return oc_fail(MCC_EINVAL, "init_camera_matrix: aspect_ratio must not be negative");
    return pc_init_matrix("init_camera_matrix", d, aspect_ratio, K);
}

extern "C" int mcc_calibrate_camera(const mcc_calib_desc* d, double* K, double* D, double* rvec, double* tvec,
                                    double* view_rms, double* rms, int* iterations, int* status, double* device_ms) {
    if (!d || !K || !D) return oc_fail(MCC_EINVAL, "calibrate_camera: null argument");
    bool planar = false;
    int rc = pc_check_views("calibrate_camera", d, &planar);
    if (rc) return rc;
    int m[mcc::kPcGlob];
    if ((rc = pc_mask("calibrate_camera", d->flags, d->nd, m))) return rc;
    if ((rc = pin_check_criteria("calibrate_camera", d->crit_type, d->max_count))) return rc;
    const int flags = d->flags, nd = d->nd, n = d->n_views;
    const bool guess = flags & MCC_CALIB_USE_INTRINSIC_GUESS;
    if (!planar && !guess)
        return oc_fail(MCC_EINVAL, "calibrate_camera: an object point has Z != 0; a non-planar target needs "
                                   "USE_INTRINSIC_GUESS");
    double aspect = 0.0;
    if (flags & MCC_CALIB_FIX_ASPECT_RATIO) {
        if (!(K[0] != 0.0 && K[4] != 0.0 && std::isfinite(K[0] / K[4])))
            return oc_fail(MCC_EINVAL, "calibrate_camera: FIX_ASPECT_RATIO needs non-zero focal lengths in K");
        aspect = K[0] / K[4];
    }

    // ---- the start: g = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
    double g[mcc::kPcGlob] = {0};
    if (guess) {
        pin_pack(K, D, nd, g);
    } else {
        double K0[9];
        if ((rc = pc_init_matrix("calibrate_camera", d, aspect, K0))) return rc;
        pin_pack(K0, nullptr, 0, g);   // the distortion starts at 0
    }
    pin_start_edits(flags, nd, aspect, g);
    int mask = 0;
    for (int k = 0; k < mcc::kPcGlob; ++k) mask |= m[k] << k;

    // ---- pose seeds
    std::vector<double> r0(3 * (size_t)n), t0(3 * (size_t)n);
    double* const rp = r0.data();
    double* const tp = t0.data();
    if ((rc = pin_seed_poses("calibrate_camera", n, d->view_off, d->obj, &d->img, 1, g, d->device, &rp, &tp))) return rc;

    // ---- the loop
    PinLoop lp;
    const PinShape shape{mcc::kPcGlob, mcc::kPcLinN, mcc::kPcYz, mcc::kPcCtrN, 1};
    if ((rc = lp.init(d->device, n, d->view_off, d->obj, &d->img, rp, tp, g, shape, d->crit_type, d->max_count, d->eps)))
        return rc;
    mcc::PcArgs a{};
    lp.fill(a);
    a.img = lp.img[0].p;
    a.mask = mask;
    a.aspect = aspect;
    if ((rc = lp.run("calibrate_camera", [&] { return mcc_launch_pc_lin(a, nullptr); },
                     [&] { return mcc_launch_pc_try(a, nullptr); }, d->trials, device_ms)))
        return rc;

    // ---- results
    std::vector<double> esq((size_t)n);
    if ((rc = lp.download(g, rvec, tvec, esq.data()))) return rc;
    pin_unpack(g, nd, K, D);
    if (view_rms)
        for (int v = 0; v < n; ++v) view_rms[v] = std::sqrt(esq[v] / (double)(lp.off[v + 1] - lp.off[v]));
    if (rms) *rms = std::sqrt(lp.s.err / (double)lp.corners);
    if (iterations) *iterations = lp.s.iter;
    if (status) *status = lp.s.status;
    return MCC_OK;
}
