// mcc_omnirect_api.cpp -- host side of the omnidir rectification C ABI (include/mcc_omnidir.h):
// cv::omnidir::undistortPoints (src/omnidir.cpp:249-343), initUndistortRectifyMap (:348-533),
// undistortImage (:538-546) and stereoRectify (:2190-2227).
//
// The host checks the arguments and inverts the three 3 x 3 matrices in double (:404-406); the
// per-point and per-pixel work is k_or_points / k_or_map / k_or_remap (mcc_omnirect.hip).
// mcc_omnirect keeps the fixed-point maps and both images on the device for a stream of frames;
// mcc_omnidir_undistort_image is one such handle used once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/mcc_omnidir.h"
#include "mcc_omnirect_host.hpp"

struct mcc_omnirect {
    int device = 0, channels = 1, src_w = 0, src_h = 0, dst_w = 0, dst_h = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    DBuf<short> map1;
    DBuf<unsigned short> map2;
    DBuf<unsigned char> src, dst;   // rows packed: width * channels bytes

    size_t src_row() const { return (size_t)src_w * channels; }
    size_t dst_row() const { return (size_t)dst_w * channels; }
    hipError_t launch() const {
        return mcc_launch_or_remap(mcc::OrRemapArgs{src.p, map1.p, map2.p, dst.p, (long long)src_row(),
                                                    (long long)dst_row(), src_w, src_h, dst_w, dst_h},
                                   channels, stream);
    }
};

namespace {

mcc_omnirect* or_new(int device, int channels, int src_w, int src_h, int dst_w, int dst_h) {
    auto* h = new mcc_omnirect();
    h->device = device;
    h->channels = channels;
    h->src_w = src_w;
    h->src_h = src_h;
    h->dst_w = dst_w;
    h->dst_h = dst_h;
    return h;
}

// stream, images and (empty) map buffers of a handle whose sizes are set
int or_alloc(mcc_omnirect* h) {
    OCCHK(hipSetDevice(h->device));
    OCCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    OCCHK(hipEventCreate(&h->ev[0]));
    OCCHK(hipEventCreate(&h->ev[1]));
    const size_t px = (size_t)h->dst_w * h->dst_h;
    OCCHK(h->map1.alloc(2 * px));
    OCCHK(h->map2.alloc(px));
    OCCHK(h->src.alloc(h->src_row() * h->src_h));
    OCCHK(h->dst.alloc(h->dst_row() * h->dst_h));
    OCCHK(hipMemsetAsync(h->src.p, 0, h->src_row() * h->src_h, h->stream));
    return MCC_OK;
}

int or_remap(mcc_omnirect* h, const unsigned char* src, long long src_stride, unsigned char* dst,
             long long dst_stride) {
    OCCHK(hipSetDevice(h->device));
    OCCHK(hipMemcpy2DAsync(h->src.p, h->src_row(), src, (size_t)src_stride, h->src_row(), h->src_h,
                           hipMemcpyHostToDevice, h->stream));
    OCCHK(h->launch());
    OCCHK(hipMemcpy2DAsync(dst, (size_t)dst_stride, h->dst.p, h->dst_row(), h->dst_row(), h->dst_h,
                           hipMemcpyDeviceToHost, h->stream));
    OCCHK(hipStreamSynchronize(h->stream));
    return MCC_OK;
}

}  // namespace

extern "C" {

int mcc_omnidir_stereo_rectify(const double* R, const double* T, double* R1, double* R2) {
    if (!R || !T || !R1 || !R2) return oc_fail(MCC_EINVAL, "null argument");
    double t21[3];   // T21 = -R^T T
    for (int c = 0; c < 3; ++c) t21[c] = -(R[c] * T[0] + R[3 + c] * T[1] + R[6 + c] * T[2]);
    const double n1 = std::sqrt(t21[0] * t21[0] + t21[1] * t21[1] + t21[2] * t21[2]);
    if (!(n1 > 0.0) || !std::isfinite(n1)) return oc_fail(MCC_EINVAL, "omnidir stereoRectify: T is zero or not finite");
    const double n2 = std::sqrt(t21[1] * t21[1] + t21[0] * t21[0]);
    if (!(n2 > 0.0))
        return oc_fail(MCC_EINVAL, "omnidir stereoRectify: the baseline -R^T T lies along z (e2 is 0 / 0)");
    const double e1[3] = {t21[0] / n1, t21[1] / n1, t21[2] / n1};
    const double e2[3] = {-t21[1] / n2, t21[0] / n2, 0.0 / n2};
    double e3[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double n3 = std::sqrt(e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2]);
    for (int k = 0; k < 3; ++k) {
        R1[k] = e1[k];
        R1[3 + k] = e2[k];
        R1[6 + k] = e3[k] / n3;
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)   // R2 = R1 R21, R21 = R^T
            R2[3 * r + c] = R1[3 * r] * R[3 * c] + R1[3 * r + 1] * R[3 * c + 1] + R1[3 * r + 2] * R[3 * c + 2];
    return MCC_OK;
}

int mcc_omnidir_undistort_points(int n, const double* distorted, const double* K, const double* D, double xi,
                                 const double* R, int device, double* undistorted) {
    if (n < 0) return oc_fail(MCC_EINVAL, "n must not be negative");
    if (!K || !D) return oc_fail(MCC_EINVAL, "null K or D");
    if (n == 0) return MCC_OK;
    if (!distorted || !undistorted) return oc_fail(MCC_EINVAL, "null points");
    mcc::OrPointsArgs a{};
    a.in = or_intr(K, D, xi);
    std::memcpy(a.R, R ? R : kEye, sizeof(a.R));
    a.n = n;
    OCCHK(hipSetDevice(device));
    DBuf<double> src, dst;
    OCCHK(src.upload(distorted, 2 * (size_t)n));
    OCCHK(dst.alloc(2 * (size_t)n));
    a.src = src.p;
    a.dst = dst.p;
    OCCHK(mcc_launch_or_points(a, nullptr));
    OCCHK(hipMemcpy(undistorted, dst.p, sizeof(double) * 2 * (size_t)n, hipMemcpyDeviceToHost));
    return MCC_OK;
}

int mcc_omnidir_init_undistort_rectify_map(const double* K, const double* D, double xi, const double* R,
                                           const double* P, int width, int height, int map_type, int flags,
                                           int device, void* map1, void* map2) {
    if (!map1 || !map2) return oc_fail(MCC_EINVAL, "null map");
    if (map_type != MCC_OMNI_MAP_FLOAT && map_type != MCC_OMNI_MAP_FIXED)
        return oc_fail(MCC_EINVAL, "map_type must be MCC_OMNI_MAP_FLOAT or MCC_OMNI_MAP_FIXED");
    mcc::OrMapArgs a{};
    int rc = or_map_args(K, D, xi, R, P, width, height, flags, &a);
    if (rc) return rc;
    const size_t px = (size_t)width * height;
    const size_t b1 = px * 4, b2 = px * (map_type == MCC_OMNI_MAP_FLOAT ? 4 : 2);
    OCCHK(hipSetDevice(device));
    DBuf<unsigned char> m1, m2;
    OCCHK(m1.alloc(b1));
    OCCHK(m2.alloc(b2));
    a.map1 = m1.p;
    a.map2 = m2.p;
    OCCHK(mcc_launch_or_map(a, flags, map_type, nullptr));
    OCCHK(hipMemcpy(map1, m1.p, b1, hipMemcpyDeviceToHost));
    OCCHK(hipMemcpy(map2, m2.p, b2, hipMemcpyDeviceToHost));
    return MCC_OK;
}

int mcc_omnirect_create(mcc_omnirect** out, const mcc_omnirect_desc* d) {
    if (!out || !d) return oc_fail(MCC_EINVAL, "null argument");
    *out = nullptr;
    if (d->channels != 1 && d->channels != 3) return oc_fail(MCC_EINVAL, "channels must be 1 or 3");
    int rc = or_check_size(d->src_width, d->src_height, "source");
    if (rc) return rc;
    mcc::OrMapArgs a{};
    if ((rc = or_map_args(d->K, d->D, d->xi, d->R, d->P, d->dst_width, d->dst_height, d->flags, &a))) return rc;
    mcc_omnirect* h = or_new(d->device, d->channels, d->src_width, d->src_height, d->dst_width, d->dst_height);
    rc = [&] {
        int r = or_alloc(h);
        if (r) return r;
        a.map1 = h->map1.p;
        a.map2 = h->map2.p;
        OCCHK(mcc_launch_or_map(a, d->flags, MCC_OMNI_MAP_FIXED, h->stream));
        OCCHK(hipStreamSynchronize(h->stream));
        return (int)MCC_OK;
    }();
    if (rc) {
        mcc_omnirect_destroy(h);
        return rc;
    }
    *out = h;
    return MCC_OK;
}

void mcc_omnirect_destroy(mcc_omnirect* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;   // the buffers
}

int mcc_omnirect_remap(mcc_omnirect* h, const unsigned char* src, long long src_stride, unsigned char* dst,
                       long long dst_stride) {
    if (!h || !src || !dst) return oc_fail(MCC_EINVAL, "null argument");
    if (src_stride < (long long)h->src_row()) return oc_fail(MCC_EINVAL, "source stride is smaller than a row");
    if (dst_stride < (long long)h->dst_row()) return oc_fail(MCC_EINVAL, "destination stride is smaller than a row");
    return or_remap(h, src, src_stride, dst, dst_stride);
}

int mcc_omnirect_time_remap(mcc_omnirect* h, int n_frames, double* ms_per_frame) {
    if (!h || n_frames < 1 || !ms_per_frame) return oc_fail(MCC_EINVAL, "bad argument");
    OCCHK(hipSetDevice(h->device));
    for (int k = 0; k < 2; ++k) OCCHK(h->launch());   // first touch
    OCCHK(hipEventRecord(h->ev[0], h->stream));
    for (int k = 0; k < n_frames; ++k) OCCHK(h->launch());
    OCCHK(hipEventRecord(h->ev[1], h->stream));
    OCCHK(hipEventSynchronize(h->ev[1]));
    float ms = 0.f;
    OCCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    *ms_per_frame = (double)ms / n_frames;
    return MCC_OK;
}

int mcc_omnidir_remap(const unsigned char* src, int src_w, int src_h, int channels, long long src_stride,
                      const short* map1, const unsigned short* map2, int dst_w, int dst_h, unsigned char* dst,
                      long long dst_stride, int device) {
    int rc = or_check_image(src, src_w, src_h, channels, src_stride, "source");
    if (rc) return rc;
    if ((rc = or_check_image(dst, dst_w, dst_h, channels, dst_stride, "destination"))) return rc;
    if (!map1 || !map2) return oc_fail(MCC_EINVAL, "null map");
    mcc_omnirect* h = or_new(device, channels, src_w, src_h, dst_w, dst_h);
    rc = [&] {
        int r = or_alloc(h);
        if (r) return r;
        const size_t px = (size_t)dst_w * dst_h;
        OCCHK(hipMemcpyAsync(h->map1.p, map1, sizeof(short) * 2 * px, hipMemcpyHostToDevice, h->stream));
        OCCHK(hipMemcpyAsync(h->map2.p, map2, sizeof(unsigned short) * px, hipMemcpyHostToDevice, h->stream));
        return or_remap(h, src, src_stride, dst, dst_stride);
    }();
    mcc_omnirect_destroy(h);
    return rc;
}

int mcc_omnidir_undistort_image(const unsigned char* src, int src_w, int src_h, int channels, long long src_stride,
                                const double* K, const double* D, double xi, int flags, const double* Knew, int new_w,
                                int new_h, const double* R, int device, unsigned char* dst, long long dst_stride) {
    int rc = or_check_image(src, src_w, src_h, channels, src_stride, "source");
    if (rc) return rc;
    if (new_w == 0) {   // new_size.empty(): the source size (:541)
        new_w = src_w;
        new_h = src_h;
    }
    if ((rc = or_check_image(dst, new_w, new_h, channels, dst_stride, "destination"))) return rc;
    const mcc_omnirect_desc d{K, D, xi, R, Knew, flags, new_w, new_h, src_w, src_h, channels, device};
    mcc_omnirect* h = nullptr;
    if ((rc = mcc_omnirect_create(&h, &d))) return rc;
    rc = or_remap(h, src, src_stride, dst, dst_stride);
    mcc_omnirect_destroy(h);
    return rc;
}

}  // extern "C"
