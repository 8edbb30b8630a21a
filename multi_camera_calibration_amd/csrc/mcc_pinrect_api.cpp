// mcc_pinrect_api.cpp -- host side of the pinhole rectification C ABI (include/mcc.h):
// mcc_undistort_points, mcc_init_undistort_rectify_map, mcc_stereo_rectify, mcc_undistort_image and the
// per-frame handle mcc_pinrect.
//
// The host checks the arguments and inverts P R in double; the per-point and per-pixel work is k_pr_points /
// k_pr_map (mcc_pinrect.hip) and the remap is k_or_remap (mcc_omnirect.hip).  mcc_stereo_rectify makes no
// device call: its few undistorted points go through the host instance of pr_undistort, the function
// k_pr_points compiles.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/mcc.h"
#include "mcc_omnirect_host.hpp"
#include "mcc_pinrect_internal.h"

struct mcc_pinrect {
    int device = 0, channels = 1, src_w = 0, src_h = 0, dst_w = 0, dst_h = 0;
    hipStream_t stream = nullptr;
    DBuf<short> map1;
    DBuf<unsigned short> map2;
    DBuf<unsigned char> src, dst;   // rows packed: width * channels bytes

    size_t src_row() const { return (size_t)src_w * channels; }
    size_t dst_row() const { return (size_t)dst_w * channels; }
};

namespace {

constexpr int kUndistortIters = 20;   // pnp_undistort's count: what stereoRectify's own points use

int pr_camera(const double* K, const double* D, int nd, mcc::PnpCam* c) {
    if (!K) return oc_fail(MCC_EINVAL, "null K");
    if (nd == 14) return oc_fail(MCC_EINVAL, "nd = 14 (tilted sensor) is not supported");
    if (nd != 0 && nd != 4 && nd != 5 && nd != 8 && nd != 12) return oc_fail(MCC_EINVAL, "nd must be 0, 4, 5, 8 or 12");
    if (!(std::fabs(K[0]) > 0.0) || !(std::fabs(K[4]) > 0.0) || !std::isfinite(K[0]) || !std::isfinite(K[4]))
        return oc_fail(MCC_EINVAL, "zero or non-finite focal length in K");
    double k[12] = {0};
    if (D)
        for (int i = 0; i < nd; ++i) k[i] = D[i];
    *c = mcc::PnpCam{K[0], K[4], K[2], K[5], k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7], k[8], k[9], k[10], k[11]};
    return MCC_OK;
}

// the first three columns of P (ld doubles per row), or `none` where the caller has no P
int pr_p3(const double* P, int ld, const double* none, double* out) {
    if (!P) {
        std::memcpy(out, none, sizeof(double) * 9);
        return MCC_OK;
    }
    if (ld != 3 && ld != 4) return oc_fail(MCC_EINVAL, "ld (doubles per row of P) must be 3 or 4");
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[3 * r + c] = P[ld * r + c];
    return MCC_OK;
}

// the host part of initUndistortRectifyMap: everything k_pr_map takes but the maps
int pr_map_args(const double* K, const double* D, int nd, const double* R, const double* P, int ld, int w, int h,
                mcc::PrMapArgs* a, bool* rational) {
    int rc = pr_camera(K, D, nd, &a->cam);
    if (rc) return rc;
    if ((rc = or_check_size(w, h, "map"))) return rc;
    double PP[9], PR[9];
    if ((rc = pr_p3(P, ld, K, PP))) return rc;
    mul3(PP, R ? R : kEye, PR);
    if (!inv3(PR, a->iPR)) return oc_fail(MCC_EINVAL, "P R is singular");
    a->w = w;
    a->h = h;
    *rational = a->cam.k4 != 0.0 || a->cam.k5 != 0.0 || a->cam.k6 != 0.0;
    return MCC_OK;
}

int pr_alloc(mcc_pinrect* h) {
    OCCHK(hipSetDevice(h->device));
    OCCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const size_t px = (size_t)h->dst_w * h->dst_h;
    OCCHK(h->map1.alloc(2 * px));
    OCCHK(h->map2.alloc(px));
    OCCHK(h->src.alloc(h->src_row() * h->src_h));
    OCCHK(h->dst.alloc(h->dst_row() * h->dst_h));
    return MCC_OK;
}

int pr_remap(mcc_pinrect* h, const unsigned char* src, long long src_stride, unsigned char* dst, long long dst_stride) {
    OCCHK(hipSetDevice(h->device));
    OCCHK(hipMemcpy2DAsync(h->src.p, h->src_row(), src, (size_t)src_stride, h->src_row(), h->src_h,
                           hipMemcpyHostToDevice, h->stream));
    OCCHK(mcc_launch_or_remap(mcc::OrRemapArgs{h->src.p, h->map1.p, h->map2.p, h->dst.p, (long long)h->src_row(),
                                               (long long)h->dst_row(), h->src_w, h->src_h, h->dst_w, h->dst_h},
                              h->channels, h->stream));
    OCCHK(hipMemcpy2DAsync(dst, (size_t)dst_stride, h->dst.p, h->dst_row(), h->dst_row(), h->dst_h,
                           hipMemcpyDeviceToHost, h->stream));
    OCCHK(hipStreamSynchronize(h->stream));
    return MCC_OK;
}

// ---------------------------------------------------------------- stereoRectify (host)
double norm3(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// The rotation vector of R, good to rounding at every angle: the angle is atan2(s, c); up to a quarter turn
// the axis is the skew part (2 s k), beyond it the column of (R + R^T) / 2 - c I = (1 - c) k k^T with the
// largest diagonal entry, whose length is at least (1 - c) / sqrt(3), signed by the skew part (at s = 0, where
// r and -r are one rotation, the column's own sign).
void pr_log(const double* R, double* r) {
    const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double s = 0.5 * norm3(v);
    const double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    const double th = std::atan2(s, c);
    if (c > 0) {
        const double k = s > 0 ? th / (2 * s) : 0.5;
        for (int i = 0; i < 3; ++i) r[i] = k * v[i];
        return;
    }
    const double d[3] = {R[0] - c, R[4] - c, R[8] - c};
    const int m = (d[0] >= d[1] && d[0] >= d[2]) ? 0 : (d[1] >= d[2] ? 1 : 2);
    double a[3];
    for (int i = 0; i < 3; ++i) a[i] = i == m ? d[m] : 0.5 * (R[3 * i + m] + R[3 * m + i]);
    double sc = th / norm3(a);
    if (a[0] * v[0] + a[1] * v[1] + a[2] * v[2] < 0) sc = -sc;
    for (int i = 0; i < 3; ++i) r[i] = sc * a[i];
}

struct PrRect {   // a rectangle by its sides
    double l, t, r, b;
};

// the 9 x 9 grid of source pixels through (cam, R, Kn): the rectangle inside every border and the bounding box
void pr_rectangles(const mcc::PnpCam& cam, const double* R, const double* Kn, int w, int h, PrRect* inner, PrRect* outer) {
    const double big = 1.7e308;
    *inner = PrRect{-big, -big, big, big};
    *outer = PrRect{big, big, -big, -big};
    for (int b = 0; b < 9; ++b)
        for (int a = 0; a < 9; ++a) {
            double x, y;
            mcc::pr_undistort(cam, R, Kn, kUndistortIters, a * (w - 1) / 8.0, b * (h - 1) / 8.0, x, y);
            outer->l = std::min(outer->l, x);
            outer->r = std::max(outer->r, x);
            outer->t = std::min(outer->t, y);
            outer->b = std::max(outer->b, y);
            if (a == 0) inner->l = std::max(inner->l, x);
            if (a == 8) inner->r = std::min(inner->r, x);
            if (b == 0) inner->t = std::max(inner->t, y);
            if (b == 8) inner->b = std::min(inner->b, y);
        }
}

}  // namespace

int mcc_pr_map_args(const double* K, const double* D, int nd, const double* R, const double* P, int ld, int w, int h,
                    mcc::PrMapArgs* a, bool* rational) {
    return pr_map_args(K, D, nd, R, P, ld, w, h, a, rational);
}

extern "C" {

int mcc_undistort_points(int n, const double* src, const double* K, const double* D, int nd, const double* R,
                         const double* P, int ld, int iterations, int device, double* dst, double* device_ms) {
    if (n < 0) return oc_fail(MCC_EINVAL, "undistortPoints: n must not be negative");
    mcc::PrPointsArgs a{};
    int rc = pr_camera(K, D, nd, &a.cam);
    if (rc) return rc;
    if (iterations < 1 || iterations > 1000) return oc_fail(MCC_EINVAL, "undistortPoints: iterations must be in 1..1000");
    if ((rc = pr_p3(P, ld, kEye, a.P))) return rc;
    std::memcpy(a.R, R ? R : kEye, sizeof(a.R));
    if (device_ms) *device_ms = 0.0;
    if (n == 0) return MCC_OK;
    if (!src || !dst) return oc_fail(MCC_EINVAL, "undistortPoints: null points");
    a.n = n;
    a.iterations = iterations;
    OCCHK(hipSetDevice(device));
    DBuf<double> in, out;
    OCCHK(in.upload(src, 2 * (size_t)n));
    OCCHK(out.alloc(2 * (size_t)n));
    a.src = in.p;
    a.dst = out.p;
    OcEvents ev;
    OCCHK(ev.create());
    OCCHK(hipEventRecord(ev.ev[0], nullptr));
    OCCHK(mcc_launch_pr_points(a, nullptr));
    OCCHK(hipEventRecord(ev.ev[1], nullptr));
    OCCHK(hipMemcpy(dst, out.p, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost));
    double ms = 0.0;
    OCCHK(ev.elapsed(&ms));
    if (device_ms) *device_ms = ms;
    return MCC_OK;
}

int mcc_init_undistort_rectify_map(const double* K, const double* D, int nd, const double* R, const double* P, int ld,
                                   int width, int height, int map_type, int device, void* map1, void* map2,
                                   double* device_ms) {
    if (!map1 || !map2) return oc_fail(MCC_EINVAL, "null map");
    if (map_type != MCC_MAP_FLOAT && map_type != MCC_MAP_FIXED)
        return oc_fail(MCC_EINVAL, "map_type must be MCC_MAP_FLOAT or MCC_MAP_FIXED");
    mcc::PrMapArgs a{};
    bool rational = false;
    int rc = pr_map_args(K, D, nd, R, P, ld, width, height, &a, &rational);
    if (rc) return rc;
    const size_t px = (size_t)width * height;
    const size_t b1 = px * 4, b2 = px * (map_type == MCC_MAP_FLOAT ? 4 : 2);
    OCCHK(hipSetDevice(device));
    DBuf<unsigned char> m1, m2;
    OCCHK(m1.alloc(b1));
    OCCHK(m2.alloc(b2));
    a.map1 = m1.p;
    a.map2 = m2.p;
    OcEvents ev;
    OCCHK(ev.create());
    OCCHK(hipEventRecord(ev.ev[0], nullptr));
    OCCHK(mcc_launch_pr_map(a, map_type, rational, nullptr));
    OCCHK(hipEventRecord(ev.ev[1], nullptr));
    OCCHK(hipMemcpy(map1, m1.p, b1, hipMemcpyDeviceToHost));
    OCCHK(hipMemcpy(map2, m2.p, b2, hipMemcpyDeviceToHost));
    double ms = 0.0;
    OCCHK(ev.elapsed(&ms));
    if (device_ms) *device_ms = ms;
    return MCC_OK;
}

int mcc_stereo_rectify(const double* K1, const double* D1, const double* K2, const double* D2, int nd, int width,
                       int height, const double* R, const double* T, int flags, double alpha, int new_width,
                       int new_height, double* R1, double* R2, double* P1, double* P2, double* Q, int* roi1, int* roi2) {
    if (!R || !T) return oc_fail(MCC_EINVAL, "stereoRectify: null R or T");
    mcc::PnpCam cam[2];
    int rc = pr_camera(K1, D1, nd, &cam[0]);
    if (rc) return rc;
    if ((rc = pr_camera(K2, D2, nd, &cam[1]))) return rc;
    if ((rc = or_check_size(width, height, "image"))) return rc;
    if (new_width == 0) {
        new_width = width;
        new_height = height;
    }
    if ((rc = or_check_size(new_width, new_height, "new image"))) return rc;
    if (flags != 0 && flags != MCC_CALIB_ZERO_DISPARITY)
        return oc_fail(MCC_EINVAL, "stereoRectify: flags must be 0 or MCC_CALIB_ZERO_DISPARITY");
    if (!(alpha <= 1.0)) return oc_fail(MCC_EINVAL, "stereoRectify: alpha must be negative or in 0..1");
    const double nT = norm3(T);
    if (!(nT > 0.0) || !std::isfinite(nT)) return oc_fail(MCC_EINVAL, "stereoRectify: T is zero or not finite");
    const int w = width, h = height, W = new_width, H = new_height;

    // 1. both cameras turn half of R towards each other, then the baseline onto the nearer of x and y
    double om[3], r[9], rt[9], t[3], Rk[2][9];
    pr_log(R, om);
    const double half[3] = {-0.5 * om[0], -0.5 * om[1], -0.5 * om[2]};
    rodrigues_host(half, r);
    for (int i = 0; i < 3; ++i) {
        t[i] = r[3 * i] * T[0] + r[3 * i + 1] * T[1] + r[3 * i + 2] * T[2];
        for (int j = 0; j < 3; ++j) rt[3 * i + j] = r[3 * j + i];
    }
    const int idx = std::fabs(t[0]) > std::fabs(t[1]) ? 0 : 1;
    const double c = t[idx];
    double uu[3] = {0, 0, 0};
    uu[idx] = c > 0 ? 1.0 : -1.0;
    double ww[3] = {t[1] * uu[2] - t[2] * uu[1], t[2] * uu[0] - t[0] * uu[2], t[0] * uu[1] - t[1] * uu[0]};
    const double nw = norm3(ww);
    if (nw > 0.0) {
        // acos(|c| / |t|), taken as atan2(|t x uu|, t . uu): the same angle, not ill-conditioned near 0
        const double sc = std::atan2(nw, std::fabs(c)) / nw;
        for (double& x : ww) x *= sc;
    }
    double wR[9];
    rodrigues_host(ww, wR);
    mul3(wR, rt, Rk[0]);
    mul3(wR, r, Rk[1]);
    for (int i = 0; i < 3; ++i) t[i] = Rk[1][3 * i] * T[0] + Rk[1][3 * i + 1] * T[1] + Rk[1][3 * i + 2] * T[2];

    // 2. the focal length: the smaller of the two across the baseline, shrunk for barrel distortion
    double fc = 1.7e308;
    for (int k = 0; k < 2; ++k) {
        double f = idx == 0 ? cam[k].fy : cam[k].fx;
        if (cam[k].k1 < 0) f *= 1 + cam[k].k1 * ((double)w * w + (double)h * h) / (4 * f * f);
        fc = std::min(fc, f);
    }

    // 3. the principal points: the image centre minus the mean of the four undistorted corners
    const double Pf[9] = {fc, 0, 0, 0, fc, 0, 0, 0, 1};
    double cc[2][2];
    for (int k = 0; k < 2; ++k) {
        double sx = 0, sy = 0;
        for (int q = 0; q < 4; ++q) {
            double x, y;
            mcc::pr_undistort(cam[k], Rk[k], Pf, kUndistortIters, (q & 1) ? w - 1.0 : 0.0, (q & 2) ? h - 1.0 : 0.0, x, y);
            sx += x;
            sy += y;
        }
        cc[k][0] = (w - 1) / 2.0 - sx / 4;
        cc[k][1] = (h - 1) / 2.0 - sy / 4;
    }
    for (int a = 0; a < 2; ++a)
        if ((flags & MCC_CALIB_ZERO_DISPARITY) || a == 1 - idx) cc[0][a] = cc[1][a] = (cc[0][a] + cc[1][a]) * 0.5;

    // 4. scaled to the new size
    const double sxy[2] = {w > 1 ? (W - 1.0) / (w - 1.0) : 1.0, h > 1 ? (H - 1.0) / (h - 1.0) : 1.0};
    double cn[2][2];
    for (int k = 0; k < 2; ++k)
        for (int a = 0; a < 2; ++a) cn[k][a] = cc[k][a] * sxy[a];

    // 5. alpha: between the scale at which the rectangle inside every border fills the new image and the one at
    // which the bounding box of the source fits it
    double s = 1.0;
    PrRect inner[2], outer[2];
    if (alpha >= 0) {
        double s0 = -1.7e308, s1 = 1.7e308;
        for (int k = 0; k < 2; ++k) {
            const double Kn[9] = {fc, 0, cc[k][0], 0, fc, cc[k][1], 0, 0, 1};
            pr_rectangles(cam[k], Rk[k], Kn, w, h, &inner[k], &outer[k]);
            for (int o = 0; o < 2; ++o) {
                const PrRect& q = o ? outer[k] : inner[k];
                const double ratio[4] = {cn[k][0] / (cc[k][0] - q.l), cn[k][1] / (cc[k][1] - q.t),
                                         (W - 1 - cn[k][0]) / (q.r - cc[k][0]), (H - 1 - cn[k][1]) / (q.b - cc[k][1])};
                for (double v : ratio) {
                    if (o) s1 = std::min(s1, v);
                    else s0 = std::max(s0, v);
                }
            }
        }
        s = s0 * (1 - alpha) + s1 * alpha;
    }
    const double f = fc * s;

    // 6. outputs
    if (R1) std::memcpy(R1, Rk[0], sizeof(double) * 9);
    if (R2) std::memcpy(R2, Rk[1], sizeof(double) * 9);
    double* Pk[2] = {P1, P2};
    for (int k = 0; k < 2; ++k) {
        if (!Pk[k]) continue;
        const double p[12] = {f, 0, cn[k][0], 0, 0, f, cn[k][1], 0, 0, 0, 1, 0};
        std::memcpy(Pk[k], p, sizeof p);
    }
    if (P2) P2[4 * idx + 3] = t[idx] * f;
    if (Q) {
        const double q[16] = {1, 0, 0, -cn[0][0], 0, 1, 0, -cn[0][1], 0, 0, 0, f,
                              0, 0, -1 / t[idx], (cn[0][idx] - cn[1][idx]) / t[idx]};
        std::memcpy(Q, q, sizeof q);
    }
    int* roi[2] = {roi1, roi2};
    for (int k = 0; k < 2; ++k) {
        if (!roi[k]) continue;
        if (alpha < 0) {
            roi[k][0] = roi[k][1] = 0;
            roi[k][2] = W;
            roi[k][3] = H;
            continue;
        }
        // ceil on the low sides, floor on the high sides, clipped to the image; in double first, so that a
        // rectangle far outside cannot overflow an int
        const double lo[2] = {std::ceil((inner[k].l - cc[k][0]) * s + cn[k][0]), std::ceil((inner[k].t - cc[k][1]) * s + cn[k][1])};
        const double hi[2] = {std::floor((inner[k].r - cc[k][0]) * s + cn[k][0]), std::floor((inner[k].b - cc[k][1]) * s + cn[k][1])};
        const int lim[2] = {W, H};
        int o[2], e[2];
        for (int a = 0; a < 2; ++a) {
            o[a] = (int)std::min(std::max(lo[a], 0.0), (double)lim[a]);
            e[a] = (int)std::min(std::max(hi[a], 0.0), (double)lim[a]);
        }
        const bool empty = !(e[0] > o[0]) || !(e[1] > o[1]);
        roi[k][0] = empty ? 0 : o[0];
        roi[k][1] = empty ? 0 : o[1];
        roi[k][2] = empty ? 0 : e[0] - o[0];
        roi[k][3] = empty ? 0 : e[1] - o[1];
    }
    return MCC_OK;
}

int mcc_pinrect_create(mcc_pinrect** out, const mcc_pinrect_desc* d) {
    if (!out || !d) return oc_fail(MCC_EINVAL, "null argument");
    *out = nullptr;
    if (d->channels != 1 && d->channels != 3) return oc_fail(MCC_EINVAL, "channels must be 1 or 3");
    int rc = or_check_size(d->src_width, d->src_height, "source");
    if (rc) return rc;
    mcc::PrMapArgs a{};
    bool rational = false;
    if ((rc = pr_map_args(d->K, d->D, d->nd, d->R, d->P, d->ld, d->dst_width, d->dst_height, &a, &rational))) return rc;
    auto* h = new mcc_pinrect();
    h->device = d->device;
    h->channels = d->channels;
    h->src_w = d->src_width;
    h->src_h = d->src_height;
    h->dst_w = d->dst_width;
    h->dst_h = d->dst_height;
    rc = [&] {
        int r = pr_alloc(h);
        if (r) return r;
        a.map1 = h->map1.p;
        a.map2 = h->map2.p;
        OCCHK(mcc_launch_pr_map(a, MCC_MAP_FIXED, rational, h->stream));
        OCCHK(hipStreamSynchronize(h->stream));
        return (int)MCC_OK;
    }();
    if (rc) {
        mcc_pinrect_destroy(h);
        return rc;
    }
    *out = h;
    return MCC_OK;
}

void mcc_pinrect_destroy(mcc_pinrect* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamDestroy(h->stream);
    }
    delete h;   // the buffers
}

int mcc_pinrect_remap(mcc_pinrect* h, const unsigned char* src, long long src_stride, unsigned char* dst,
                      long long dst_stride) {
    if (!h || !src || !dst) return oc_fail(MCC_EINVAL, "null argument");
    if (src_stride < (long long)h->src_row()) return oc_fail(MCC_EINVAL, "source stride is smaller than a row");
    if (dst_stride < (long long)h->dst_row()) return oc_fail(MCC_EINVAL, "destination stride is smaller than a row");
    return pr_remap(h, src, src_stride, dst, dst_stride);
}

int mcc_undistort_image(const unsigned char* src, int src_w, int src_h, int channels, long long src_stride,
                        const double* K, const double* D, int nd, const double* R, const double* Knew, int ld, int new_w,
                        int new_h, int device, unsigned char* dst, long long dst_stride) {
    int rc = or_check_image(src, src_w, src_h, channels, src_stride, "source");
    if (rc) return rc;
    if (new_w == 0) {
        new_w = src_w;
        new_h = src_h;
    }
    if ((rc = or_check_image(dst, new_w, new_h, channels, dst_stride, "destination"))) return rc;
    const mcc_pinrect_desc d{K, D, nd, R, Knew, ld, new_w, new_h, src_w, src_h, channels, device};
    mcc_pinrect* h = nullptr;
    if ((rc = mcc_pinrect_create(&h, &d))) return rc;
    rc = pr_remap(h, src, src_stride, dst, dst_stride);
    mcc_pinrect_destroy(h);
    return rc;
}

}  // extern "C"
