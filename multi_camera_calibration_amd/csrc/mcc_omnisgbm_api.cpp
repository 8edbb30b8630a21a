// mcc_omnisgbm_api.cpp -- host side of cv::omnidir::stereoReconstruct (src/omnidir.cpp:1383-1539) in
// the C ABI (include/mcc_omnidir.h): mcc_omnidir_sgbm, mcc_omnirecon_*, mcc_omnidir_stereo_reconstruct.
//
// The host checks the arguments, runs stereoRectify and inverts Knew in double (:1417, :1471); the
// per-pixel work is the remap of mcc_omnirect.hip and the kernels of mcc_omnisgbm.hip.  mcc_omnirecon
// keeps both cameras' maps, the images, the signal planes, the cost volumes and the cloud on the
// device; the one-shot calls are one such handle used once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/mcc_omnidir.h"
#include "mcc_omnirect_host.hpp"
#include "mcc_omnisgbm_internal.h"

namespace {

// the matcher's own limits on a W x H pair of cn channels
int sg_check(int W, int H, int cn, int D, int bs) {
    if (D <= 0 || D % 16 != 0 || D > 256)
        return oc_fail(MCC_EINVAL, "numDisparities must be a positive multiple of 16, at most 256");
    if (W <= D) return oc_fail(MCC_EINVAL, "the matched width must exceed numDisparities");
    if (W > 65535 || H > 65535) return oc_fail(MCC_EINVAL, "the matched size must not exceed 65535");
    if (bs < 1 || bs % 2 == 0) return oc_fail(MCC_EINVAL, "SADWindowSize must be odd and positive");
    if (93LL * cn * bs * bs > 32767)
        return oc_fail(MCC_EINVAL, "93 * channels * SADWindowSize^2 must not exceed 32767 (16-bit block cost)");
    const long long bytes = 2LL * H * (W - D) * D;
    if (bytes > MCC_OMNI_SGBM_MAX_COST_BYTES)
        return oc_fail(MCC_EINVAL, "the cost volume of " + std::to_string(bytes) + " bytes exceeds MCC_OMNI_SGBM_MAX_COST_BYTES");
    return MCC_OK;
}

int sg_check_pair(const void* a, int w, int h, int c, long long sa, const void* b, int w2, int h2, int c2, long long sb) {
    int rc = or_check_image(a, w, h, c, sa, "first");
    if (rc) return rc;
    if (c2 != c) return oc_fail(MCC_EINVAL, "the two images must have the same number of channels");
    if (w2 != w || h2 != h) return oc_fail(MCC_EINVAL, "the two images must have the same size");
    return or_check_image(b, w2, h2, c2, sb, "second");
}

}  // namespace

struct mcc_omnirecon {
    int device = 0, cn = 1, src_w = 0, src_h = 0, W = 0, H = 0, D = 0, bs = 0;
    int flag = 0, point_type = MCC_OMNI_XYZ, cloud_w = 0, cloud_h = 0;
    bool rectify = true;   // false: the matcher alone, the pair is uploaded into rec
    double kinv[9] = {0}, bf = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    DBuf<short> map1[2];
    DBuf<unsigned short> map2[2];
    DBuf<unsigned char> src[2], rec[2];   // rows packed
    DBuf<mcc::SgSig> sig[2];
    DBuf<unsigned short> cost;
    DBuf<int> sum, col_count;
    DBuf<short> disp;
    DBuf<unsigned int> key2;
    DBuf<float> real, cloud;

    size_t src_row() const { return (size_t)src_w * cn; }
    size_t rec_row() const { return (size_t)W * cn; }
    int point_floats() const { return point_type == MCC_OMNI_XYZ ? 3 : 6; }

    hipError_t launch_match() const {
        mcc::SgArgs a{};
        for (int i = 0; i < 2; ++i) {
            a.img[i] = rec[i].p;
            a.stride[i] = (long long)rec_row();
            a.sig[i] = sig[i].p;
        }
        a.cost = cost.p;
        a.tmp = (unsigned short*)sum.p;
        a.sum = sum.p;
        a.disp = disp.p;
        a.key2 = key2.p;
        a.H = H, a.W = W, a.D = D, a.cn = cn, a.bs = bs;
        return mcc_launch_sg_match(a, stream);
    }
    // remap of both images, the matcher, the float disparity and the cloud
    hipError_t launch_frame() const {
        hipError_t e;
        for (int i = 0; i < 2; ++i)
            if ((e = mcc_launch_or_remap(mcc::OrRemapArgs{src[i].p, map1[i].p, map2[i].p, rec[i].p, (long long)src_row(),
                                                          (long long)rec_row(), src_w, src_h, W, H},
                                         cn, stream)) != hipSuccess)
                return e;
        if ((e = launch_match()) != hipSuccess) return e;
        mcc::SgFinishArgs f{};
        f.disp = disp.p, f.rec1 = rec[0].p, f.real = real.p, f.col_count = col_count.p, f.cloud = cloud.p;
        std::memcpy(f.kinv, kinv, sizeof(f.kinv));
        f.bf = bf;
        f.H = H, f.W = W, f.cn = cn, f.flag = flag, f.point_type = point_type;
        f.cloud_w = cloud_w, f.cloud_h = cloud_h;
        return mcc_launch_sg_finish(f, stream);
    }
};

namespace {

int rc_alloc(mcc_omnirecon* h) {
    OCCHK(hipSetDevice(h->device));
    OCCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    OCCHK(hipEventCreate(&h->ev[0]));
    OCCHK(hipEventCreate(&h->ev[1]));
    const size_t px = (size_t)h->W * h->H, vol = (size_t)h->H * (h->W - h->D) * h->D;
    for (int i = 0; i < 2; ++i) {
        if (h->rectify) {
            OCCHK(h->map1[i].alloc(2 * px));
            OCCHK(h->map2[i].alloc(px));
            OCCHK(h->src[i].alloc(h->src_row() * h->src_h));
        }
        OCCHK(h->rec[i].alloc(px * h->cn));
        OCCHK(h->sig[i].alloc(px * h->cn));
    }
    OCCHK(h->cost.alloc(vol));
    OCCHK(h->sum.alloc(vol));
    OCCHK(h->disp.alloc(px));
    OCCHK(h->key2.alloc(px));
    if (h->rectify) {
        OCCHK(h->real.alloc(px));
        OCCHK(h->col_count.alloc((size_t)h->cloud_w * mcc::sg_cloud_segments(h->cloud_h) + 1));
        OCCHK(h->cloud.alloc((size_t)h->cloud_w * h->cloud_h * h->point_floats()));
    }
    return MCC_OK;
}

int rc_upload(mcc_omnirecon* h, DBuf<unsigned char>* dst, size_t row, int rows, const unsigned char* a, long long sa,
              const unsigned char* b, long long sb) {
    OCCHK(hipMemcpy2DAsync(dst[0].p, row, a, (size_t)sa, row, rows, hipMemcpyHostToDevice, h->stream));
    OCCHK(hipMemcpy2DAsync(dst[1].p, row, b, (size_t)sb, row, rows, hipMemcpyHostToDevice, h->stream));
    return MCC_OK;
}

}  // namespace

extern "C" {

void mcc_omnirecon_destroy(mcc_omnirecon* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;   // the buffers
}

int mcc_omnidir_sgbm(const unsigned char* left, int width, int height, int channels, long long left_stride,
                     const unsigned char* right, int width2, int height2, int channels2, long long right_stride,
                     int num_disparities, int sad_window_size, int device, short* disparity) {
    int rc = sg_check_pair(left, width, height, channels, left_stride, right, width2, height2, channels2, right_stride);
    if (rc) return rc;
    if (!disparity) return oc_fail(MCC_EINVAL, "null disparity");
    if ((rc = sg_check(width, height, channels, num_disparities, sad_window_size))) return rc;
    auto* h = new mcc_omnirecon();
    h->device = device, h->cn = channels, h->W = width, h->H = height, h->D = num_disparities, h->bs = sad_window_size;
    h->rectify = false;
    rc = [&] {
        int r = rc_alloc(h);
        if (r) return r;
        if ((r = rc_upload(h, h->rec, h->rec_row(), height, left, left_stride, right, right_stride))) return r;
        OCCHK(h->launch_match());
        OCCHK(hipMemcpyAsync(disparity, h->disp.p, sizeof(short) * (size_t)width * height, hipMemcpyDeviceToHost,
                             h->stream));
        OCCHK(hipStreamSynchronize(h->stream));
        return (int)MCC_OK;
    }();
    mcc_omnirecon_destroy(h);
    return rc;
}

int mcc_omnirecon_create(mcc_omnirecon** out, const mcc_omnirecon_desc* d) {
    if (!out || !d) return oc_fail(MCC_EINVAL, "null argument");
    *out = nullptr;
    if (!d->K1 || !d->K2 || !d->R || !d->T) return oc_fail(MCC_EINVAL, "null K1, K2, R or T");
    if (d->channels != 1 && d->channels != 3) return oc_fail(MCC_EINVAL, "channels must be 1 or 3");
    if (d->flag != MCC_OMNI_RECTIFY_PERSPECTIVE && d->flag != MCC_OMNI_RECTIFY_LONGLATI)
        return oc_fail(MCC_EINVAL, "flag must be MCC_OMNI_RECTIFY_PERSPECTIVE or MCC_OMNI_RECTIFY_LONGLATI");
    if (d->point_type != MCC_OMNI_XYZRGB && d->point_type != MCC_OMNI_XYZ)
        return oc_fail(MCC_EINVAL, "pointType must be MCC_OMNI_XYZRGB or MCC_OMNI_XYZ");
    int rc = or_check_size(d->src_width, d->src_height, "source");
    if (rc) return rc;
    const bool empty = d->new_width == 0;   // newSize.empty(): the source size, and no cloud
    const int W = empty ? d->src_width : d->new_width, H = empty ? d->src_height : d->new_height;
    if ((rc = or_check_size(W, H, "new"))) return rc;
    if ((rc = sg_check(W, H, d->channels, d->num_disparities, d->sad_window_size))) return rc;
    double R1[9], R2[9];
    if ((rc = mcc_omnidir_stereo_rectify(d->R, d->T, R1, R2))) return rc;
    const double* Knew = d->Knew ? d->Knew : d->K1;
    mcc::OrMapArgs m[2];
    if ((rc = or_map_args(d->K1, d->D1, d->xi1, R1, Knew, W, H, d->flag, &m[0]))) return rc;
    if ((rc = or_map_args(d->K2, d->D2, d->xi2, R2, Knew, W, H, d->flag, &m[1]))) return rc;

    auto* h = new mcc_omnirecon();
    h->device = d->device, h->cn = d->channels, h->src_w = d->src_width, h->src_h = d->src_height;
    h->W = W, h->H = H, h->D = d->num_disparities, h->bs = d->sad_window_size;
    h->flag = d->flag, h->point_type = d->point_type;
    h->cloud_w = empty ? 0 : W, h->cloud_h = empty ? 0 : H;
    if (!inv3(Knew, h->kinv)) {   // or_map_args has inverted it already; kept for the message
        delete h;
        return oc_fail(MCC_EINVAL, "Knew is singular");
    }
    h->bf = std::sqrt(d->T[0] * d->T[0] + d->T[1] * d->T[1] + d->T[2] * d->T[2]) * Knew[0];
    rc = [&] {
        int r = rc_alloc(h);
        if (r) return r;
        for (int i = 0; i < 2; ++i) {
            m[i].map1 = h->map1[i].p;
            m[i].map2 = h->map2[i].p;
            OCCHK(mcc_launch_or_map(m[i], d->flag, MCC_OMNI_MAP_FIXED, h->stream));
            OCCHK(hipMemsetAsync(h->src[i].p, 0, h->src_row() * h->src_h, h->stream));
        }
        OCCHK(hipStreamSynchronize(h->stream));
        return (int)MCC_OK;
    }();
    if (rc) {
        mcc_omnirecon_destroy(h);
        return rc;
    }
    *out = h;
    return MCC_OK;
}

int mcc_omnirecon_compute(mcc_omnirecon* h, const unsigned char* image1, long long stride1, const unsigned char* image2,
                          long long stride2, float* disparity, unsigned char* rec1, long long rec1_stride,
                          unsigned char* rec2, long long rec2_stride, float* cloud, long long capacity,
                          long long* n_points) {
    if (!h || !image1 || !image2 || !disparity || !rec1 || !rec2 || !n_points) return oc_fail(MCC_EINVAL, "null argument");
    if (capacity < 0 || (capacity > 0 && !cloud)) return oc_fail(MCC_EINVAL, "null cloud with a positive capacity");
    if (stride1 < (long long)h->src_row() || stride2 < (long long)h->src_row())
        return oc_fail(MCC_EINVAL, "source stride is smaller than a row");
    if (rec1_stride < (long long)h->rec_row() || rec2_stride < (long long)h->rec_row())
        return oc_fail(MCC_EINVAL, "rectified stride is smaller than a row");
    *n_points = 0;
    OCCHK(hipSetDevice(h->device));
    int rc = rc_upload(h, h->src, h->src_row(), h->src_h, image1, stride1, image2, stride2);
    if (rc) return rc;
    OCCHK(h->launch_frame());
    int total = 0;
    const size_t slots = (size_t)h->cloud_w * mcc::sg_cloud_segments(h->cloud_h);   // the scan leaves the total behind them
    OCCHK(hipMemcpyAsync(&total, h->col_count.p + slots, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    OCCHK(hipMemcpyAsync(disparity, h->real.p, sizeof(float) * (size_t)h->W * h->H, hipMemcpyDeviceToHost, h->stream));
    unsigned char* rec[2] = {rec1, rec2};
    const long long rs[2] = {rec1_stride, rec2_stride};
    for (int i = 0; i < 2; ++i)
        OCCHK(hipMemcpy2DAsync(rec[i], (size_t)rs[i], h->rec[i].p, h->rec_row(), h->rec_row(), h->H,
                               hipMemcpyDeviceToHost, h->stream));
    OCCHK(hipStreamSynchronize(h->stream));
    *n_points = total;
    if (total > capacity)
        return oc_fail(MCC_EINVAL, "the cloud needs room for " + std::to_string(total) + " points, capacity is " +
                                       std::to_string(capacity));
    if (total > 0) {
        OCCHK(hipMemcpyAsync(cloud, h->cloud.p, sizeof(float) * (size_t)total * h->point_floats(), hipMemcpyDeviceToHost,
                             h->stream));
        OCCHK(hipStreamSynchronize(h->stream));
    }
    return MCC_OK;
}

int mcc_omnirecon_time(mcc_omnirecon* h, int n_frames, double* ms_per_frame) {
    if (!h || n_frames < 1 || !ms_per_frame) return oc_fail(MCC_EINVAL, "bad argument");
    OCCHK(hipSetDevice(h->device));
    // resident random frames: a black pair would make every cost tie
    std::mt19937 gen(12345);
    std::vector<unsigned char> frame(h->src_row() * h->src_h);
    for (int i = 0; i < 2; ++i) {
        for (auto& b : frame) b = (unsigned char)(gen() & 255);
        OCCHK(hipMemcpyAsync(h->src[i].p, frame.data(), frame.size(), hipMemcpyHostToDevice, h->stream));
        OCCHK(hipStreamSynchronize(h->stream));
    }
    for (int k = 0; k < 2; ++k) OCCHK(h->launch_frame());   // first touch
    OCCHK(hipEventRecord(h->ev[0], h->stream));
    for (int k = 0; k < n_frames; ++k) OCCHK(h->launch_frame());
    OCCHK(hipEventRecord(h->ev[1], h->stream));
    OCCHK(hipEventSynchronize(h->ev[1]));
    float ms = 0.f;
    OCCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    *ms_per_frame = (double)ms / n_frames;
    return MCC_OK;
}

int mcc_omnidir_stereo_reconstruct(const unsigned char* image1, int width, int height, int channels, long long stride1,
                                   const unsigned char* image2, int width2, int height2, int channels2,
                                   long long stride2, const double* K1, const double* D1, double xi1, const double* K2,
                                   const double* D2, double xi2, const double* R, const double* T, int flag,
                                   int num_disparities, int sad_window_size, int new_width, int new_height,
                                   const double* Knew, int point_type, int device, float* disparity,
                                   unsigned char* rec1, long long rec1_stride, unsigned char* rec2,
                                   long long rec2_stride, float* cloud, long long capacity, long long* n_points) {
    int rc = sg_check_pair(image1, width, height, channels, stride1, image2, width2, height2, channels2, stride2);
    if (rc) return rc;
    if (!disparity || !rec1 || !rec2 || !n_points) return oc_fail(MCC_EINVAL, "null output");
    if (capacity < 0 || (capacity > 0 && !cloud)) return oc_fail(MCC_EINVAL, "null cloud with a positive capacity");
    const int W = new_width == 0 ? width : new_width;
    if (rec1_stride < (long long)W * channels || rec2_stride < (long long)W * channels)
        return oc_fail(MCC_EINVAL, "rectified stride is smaller than a row");
    const mcc_omnirecon_desc d{K1, D1, xi1, K2, D2, xi2, R, T, flag, num_disparities, sad_window_size, width, height,
                               channels, new_width, new_height, Knew, point_type, device};
    mcc_omnirecon* h = nullptr;
    if ((rc = mcc_omnirecon_create(&h, &d))) return rc;
    rc = mcc_omnirecon_compute(h, image1, stride1, image2, stride2, disparity, rec1, rec1_stride, rec2, rec2_stride,
                               cloud, capacity, n_points);
    mcc_omnirecon_destroy(h);
    return rc;
}

}  // extern "C"
