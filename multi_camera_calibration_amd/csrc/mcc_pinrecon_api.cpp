// mcc_pinrecon_api.cpp -- host side of the pinhole reconstruction C ABI (include/mcc.h):
// mcc_reproject_image_to_3d, the per-pair handle mcc_pinrecon, mcc_stereo_reconstruct and the host run of the
// cloud rule, mcc_pinrecon_host_cloud.
//
// The host checks the arguments, runs mcc_stereo_rectify and inverts P R in double (mcc_pr_map_args); the maps are
// k_pr_map, the remap is k_or_remap, the matcher is mcc_launch_sg_match, and the tail is mcc_pinrecon.hip.
// mcc_pinrecon keeps both cameras' maps, the images, the signal planes, the cost volumes, the disparities, the dense
// points and the cloud on the device; the one-shot call is one such handle used once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mcc_omnidir.h"
#include "mcc_omnirect_host.hpp"
#include "mcc_omnisgbm_internal.h"
#include "mcc_pinrect_internal.h"
#include "mcc_pinrecon_internal.h"

static_assert(MCC_XYZRGB == MCC_OMNI_XYZRGB && MCC_XYZ == MCC_OMNI_XYZ, "the neutral point types are aliases");

struct mcc_pinrecon {
    int device = 0, cn = 1, src_w = 0, src_h = 0, W = 0, H = 0, D = 0, bs = 0, point_type = MCC_XYZ;
    mcc_pinrecon_geometry geo{};
    mcc::PnCloudRule rule{};
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
    DBuf<float> real, points, cloud;

    size_t src_row() const { return (size_t)src_w * cn; }
    size_t rec_row() const { return (size_t)W * cn; }
    int point_floats() const { return point_type == MCC_XYZ ? 3 : 6; }

    // remap of both images, the matcher, the float disparity with the dense points, the cloud
    hipError_t launch_frame() const {
        hipError_t e;
        for (int i = 0; i < 2; ++i)
            if ((e = mcc_launch_or_remap(mcc::OrRemapArgs{src[i].p, map1[i].p, map2[i].p, rec[i].p, (long long)src_row(),
                                                          (long long)rec_row(), src_w, src_h, W, H},
                                         cn, stream)) != hipSuccess)
                return e;
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
        if ((e = mcc_launch_sg_match(a, stream)) != hipSuccess) return e;
        mcc::PnReprojectArgs r{};
        std::memcpy(r.q, geo.Q, sizeof(r.q));
        r.disp = disp.p, r.real = real.p, r.points = points.p, r.w = W, r.h = H;
        if ((e = mcc_launch_pn_reproject(r, MCC_DISP_FIXED16, false, nullptr, stream)) != hipSuccess) return e;
        mcc::PnCloudArgs c{};
        std::memcpy(c.q, geo.Q, sizeof(c.q));
        c.rule = rule;
        c.real = real.p, c.rec1 = rec[0].p, c.col_count = col_count.p, c.cloud = cloud.p;
        c.w = W, c.h = H, c.cn = cn, c.point_floats = point_floats();
        return mcc_launch_pn_cloud(c, stream);
    }
};

namespace {

// the matcher's own limits on a W x H pair of cn channels (those of mcc_omnidir_sgbm)
int pn_check_match(int W, int H, int cn, int D, int bs) {
    if (D <= 0 || D % 16 != 0 || D > 256)
        return oc_fail(MCC_EINVAL, "num_disparities must be a positive multiple of 16, at most 256");
    if (W <= D) return oc_fail(MCC_EINVAL, "the matched width must exceed num_disparities");
    if (bs < 1 || bs % 2 == 0) return oc_fail(MCC_EINVAL, "sad_window_size must be odd and positive");
    if (93LL * cn * bs * bs > 32767)
        return oc_fail(MCC_EINVAL, "93 * channels * sad_window_size^2 must not exceed 32767 (16-bit block cost)");
    const long long bytes = 2LL * H * (W - D) * D;
    if (bytes > MCC_OMNI_SGBM_MAX_COST_BYTES)
        return oc_fail(MCC_EINVAL, "the cost volume of " + std::to_string(bytes) + " bytes exceeds MCC_OMNI_SGBM_MAX_COST_BYTES");
    return MCC_OK;
}

int pn_point_type(int t) {
    if (t != MCC_XYZRGB && t != MCC_XYZ) return oc_fail(MCC_EINVAL, "point_type must be MCC_XYZRGB or MCC_XYZ");
    return MCC_OK;
}

mcc::PnCloudRule pn_rule(const int* roi, double max_z) {
    mcc::PnCloudRule r{};
    r.max_z = max_z;
    r.use_roi = roi != nullptr;
    if (roi) r.rx = roi[0], r.ry = roi[1], r.rw = roi[2], r.rh = roi[3];
    return r;
}

// the rectification of a descriptor in the frame of the handle's outputs; host only
int pn_geometry(const mcc_pinrecon_desc* d, mcc_pinrecon_geometry* g) {
    if (!d->K1 || !d->K2 || !d->R || !d->T) return oc_fail(MCC_EINVAL, "null K1, K2, R or T");
    if (d->nd == 14) return oc_fail(MCC_EINVAL, "nd = 14 (tilted sensor) is not supported");
    if (d->channels != 1 && d->channels != 3) return oc_fail(MCC_EINVAL, "channels must be 1 or 3");
    int rc = pn_point_type(d->point_type);
    if (rc) return rc;
    if ((rc = mcc_stereo_rectify(d->K1, d->D1, d->K2, d->D2, d->nd, d->src_width, d->src_height, d->R, d->T,
                                 d->rectify_flags, d->alpha, d->new_width, d->new_height, g->R1, g->R2, g->P1, g->P2, g->Q,
                                 g->roi1, g->roi2)))
        return rc;
    const int W = d->new_width == 0 ? d->src_width : d->new_width, H = d->new_width == 0 ? d->src_height : d->new_height;
    const int idx = g->P2[3] != 0.0 ? 0 : 1;   // the baseline's axis: P2[3] or P2[7] carries T f
    // the matcher finds d = x1 - x2 >= 0 only: camera 2 to the right of (below) camera 1
    double t = 0;
    for (int k = 0; k < 3; ++k) t += g->R2[3 * idx + k] * d->T[k];
    if (!(t < 0.0))
        return oc_fail(MCC_EINVAL, std::string("after rectification camera 2 lies ") + (idx ? "above" : "to the left of") +
                                       " camera 1, where disparities are negative: swap the cameras (and invert R, T)");
    g->transposed = idx;
    g->width = idx ? H : W;
    g->height = idx ? W : H;
    if (idx) {
        // rows 0 and 1 of P1, P2 swapped: the map builder inverts this P R as any other, and the rectified
        // images come out transposed; Q then takes (x, y) in that order too, and so do the rois
        for (double* P : {g->P1, g->P2})
            for (int c = 0; c < 4; ++c) std::swap(P[c], P[4 + c]);
        for (int r = 0; r < 4; ++r) std::swap(g->Q[4 * r], g->Q[4 * r + 1]);
        for (int* roi : {g->roi1, g->roi2}) {
            std::swap(roi[0], roi[1]);
            std::swap(roi[2], roi[3]);
        }
    }
    return pn_check_match(g->width, g->height, d->channels, d->num_disparities, d->sad_window_size);
}

int pn_alloc(mcc_pinrecon* h) {
    OCCHK(hipSetDevice(h->device));
    OCCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    OCCHK(hipEventCreate(&h->ev[0]));
    OCCHK(hipEventCreate(&h->ev[1]));
    const size_t px = (size_t)h->W * h->H, vol = (size_t)h->H * (h->W - h->D) * h->D;
    for (int i = 0; i < 2; ++i) {
        OCCHK(h->map1[i].alloc(2 * px));
        OCCHK(h->map2[i].alloc(px));
        OCCHK(h->src[i].alloc(h->src_row() * h->src_h));
        OCCHK(h->rec[i].alloc(px * h->cn));
        OCCHK(h->sig[i].alloc(px * h->cn));
    }
    OCCHK(h->cost.alloc(vol));
    OCCHK(h->sum.alloc(vol));
    OCCHK(h->disp.alloc(px));
    OCCHK(h->key2.alloc(px));
    OCCHK(h->real.alloc(px));
    OCCHK(h->points.alloc(3 * px));
    OCCHK(h->col_count.alloc((size_t)h->W * mcc::sg_cloud_segments(h->H) + 1));
    OCCHK(h->cloud.alloc(px * h->point_floats()));
    return MCC_OK;
}

}  // namespace

extern "C" {

int mcc_reproject_image_to_3d(const void* disparity, int disparity_type, int width, int height, long long stride_bytes,
                              const double* Q, int handle_missing, int device, float* points, double* device_ms) {
    if (!disparity || !Q || !points) return oc_fail(MCC_EINVAL, "reprojectImageTo3D: null argument");
    if (disparity_type != MCC_DISP_FLOAT && disparity_type != MCC_DISP_FIXED16)
        return oc_fail(MCC_EINVAL, "reprojectImageTo3D: disparity_type must be MCC_DISP_FLOAT or MCC_DISP_FIXED16");
    int rc = or_check_size(width, height, "disparity");
    if (rc) return rc;
    const size_t px_bytes = disparity_type == MCC_DISP_FLOAT ? 4 : 2, row = (size_t)width * px_bytes;
    if (stride_bytes < (long long)row) return oc_fail(MCC_EINVAL, "reprojectImageTo3D: the stride is smaller than a row");
    if (stride_bytes % (long long)px_bytes) return oc_fail(MCC_EINVAL, "reprojectImageTo3D: the stride is not a multiple of the pixel size");
    const size_t px = (size_t)width * height;
    OCCHK(hipSetDevice(device));
    DBuf<unsigned char> in;
    DBuf<float> out, partial;
    OCCHK(in.alloc(row * height));
    OCCHK(out.alloc(3 * px));
    OCCHK(partial.alloc(mcc::kPnDminBlocks + 1));
    OCCHK(hipMemcpy2D(in.p, row, disparity, (size_t)stride_bytes, row, height, hipMemcpyHostToDevice));
    mcc::PnReprojectArgs a{};
    std::memcpy(a.q, Q, sizeof(a.q));
    a.disp = in.p, a.dmin = partial.p + mcc::kPnDminBlocks, a.real = nullptr, a.points = out.p, a.w = width, a.h = height;
    OcEvents ev;
    OCCHK(ev.create());
    OCCHK(hipEventRecord(ev.ev[0], nullptr));
    OCCHK(mcc_launch_pn_reproject(a, disparity_type, handle_missing != 0, partial.p, nullptr));
    OCCHK(hipEventRecord(ev.ev[1], nullptr));
    OCCHK(hipMemcpy(points, out.p, sizeof(float) * 3 * px, hipMemcpyDeviceToHost));
    double ms = 0.0;
    OCCHK(ev.elapsed(&ms));
    if (device_ms) *device_ms = ms;
    return MCC_OK;
}

void mcc_pinrecon_destroy(mcc_pinrecon* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;   // the buffers
}

int mcc_pinrecon_create(mcc_pinrecon** out, const mcc_pinrecon_desc* d) {
    if (!out || !d) return oc_fail(MCC_EINVAL, "null argument");
    *out = nullptr;
    mcc_pinrecon_geometry g{};
    int rc = pn_geometry(d, &g);
    if (rc) return rc;
    const double* K[2] = {d->K1, d->K2};
    const double* D[2] = {d->D1, d->D2};
    const double* R[2] = {g.R1, g.R2};
    const double* P[2] = {g.P1, g.P2};
    mcc::PrMapArgs m[2]{};
    bool rational[2] = {false, false};
    for (int i = 0; i < 2; ++i)
        if ((rc = mcc_pr_map_args(K[i], D[i], d->nd, R[i], P[i], 4, g.width, g.height, &m[i], &rational[i]))) return rc;

    auto* h = new mcc_pinrecon();
    h->device = d->device, h->cn = d->channels, h->src_w = d->src_width, h->src_h = d->src_height;
    h->W = g.width, h->H = g.height, h->D = d->num_disparities, h->bs = d->sad_window_size;
    h->point_type = d->point_type;
    h->geo = g;
    h->rule = pn_rule(d->use_roi ? g.roi1 : nullptr, d->max_z);
    rc = [&] {
        int r = pn_alloc(h);
        if (r) return r;
        for (int i = 0; i < 2; ++i) {
            m[i].map1 = h->map1[i].p;
            m[i].map2 = h->map2[i].p;
            OCCHK(mcc_launch_pr_map(m[i], MCC_MAP_FIXED, rational[i], h->stream));
            OCCHK(hipMemsetAsync(h->src[i].p, 0, h->src_row() * h->src_h, h->stream));
        }
        OCCHK(hipStreamSynchronize(h->stream));
        return (int)MCC_OK;
    }();
    if (rc) {
        mcc_pinrecon_destroy(h);
        return rc;
    }
    *out = h;
    return MCC_OK;
}

int mcc_pinrecon_info(const mcc_pinrecon* h, mcc_pinrecon_geometry* geometry) {
    if (!h || !geometry) return oc_fail(MCC_EINVAL, "null argument");
    *geometry = h->geo;
    return MCC_OK;
}

int mcc_pinrecon_compute(mcc_pinrecon* h, const unsigned char* image1, long long stride1, const unsigned char* image2,
                         long long stride2, float* disparity, short* disparity16, unsigned char* rec1, long long rec1_stride,
                         unsigned char* rec2, long long rec2_stride, float* points, float* cloud, long long capacity,
                         long long* n_points) {
    if (!h || !image1 || !image2 || !disparity || !rec1 || !rec2 || !n_points) return oc_fail(MCC_EINVAL, "null argument");
    if (capacity < 0 || (capacity > 0 && !cloud)) return oc_fail(MCC_EINVAL, "null cloud with a positive capacity");
    if (stride1 < (long long)h->src_row() || stride2 < (long long)h->src_row())
        return oc_fail(MCC_EINVAL, "source stride is smaller than a row");
    if (rec1_stride < (long long)h->rec_row() || rec2_stride < (long long)h->rec_row())
        return oc_fail(MCC_EINVAL, "rectified stride is smaller than a row");
    *n_points = 0;
    OCCHK(hipSetDevice(h->device));
    const unsigned char* img[2] = {image1, image2};
    const long long st[2] = {stride1, stride2};
    for (int i = 0; i < 2; ++i)
        OCCHK(hipMemcpy2DAsync(h->src[i].p, h->src_row(), img[i], (size_t)st[i], h->src_row(), h->src_h, hipMemcpyHostToDevice,
                               h->stream));
    OCCHK(h->launch_frame());
    const size_t px = (size_t)h->W * h->H;
    int total = 0;
    const size_t slots = (size_t)h->W * mcc::sg_cloud_segments(h->H);   // the scan leaves the total behind them
    OCCHK(hipMemcpyAsync(&total, h->col_count.p + slots, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    OCCHK(hipMemcpyAsync(disparity, h->real.p, sizeof(float) * px, hipMemcpyDeviceToHost, h->stream));
    if (disparity16) OCCHK(hipMemcpyAsync(disparity16, h->disp.p, sizeof(short) * px, hipMemcpyDeviceToHost, h->stream));
    if (points) OCCHK(hipMemcpyAsync(points, h->points.p, sizeof(float) * 3 * px, hipMemcpyDeviceToHost, h->stream));
    unsigned char* rec[2] = {rec1, rec2};
    const long long rs[2] = {rec1_stride, rec2_stride};
    for (int i = 0; i < 2; ++i)
        OCCHK(hipMemcpy2DAsync(rec[i], (size_t)rs[i], h->rec[i].p, h->rec_row(), h->rec_row(), h->H, hipMemcpyDeviceToHost,
                               h->stream));
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

int mcc_pinrecon_time(mcc_pinrecon* h, int n_frames, double* ms_per_frame) {
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

int mcc_stereo_reconstruct(const unsigned char* image1, int width, int height, int channels, long long stride1,
                           const unsigned char* image2, int width2, int height2, int channels2, long long stride2,
                           const mcc_pinrecon_desc* desc, mcc_pinrecon_geometry* geometry, float* disparity,
                           short* disparity16, unsigned char* rec1, long long rec1_stride, unsigned char* rec2,
                           long long rec2_stride, float* points, float* cloud, long long capacity, long long* n_points) {
    if (!desc) return oc_fail(MCC_EINVAL, "null descriptor");
    int rc = or_check_image(image1, width, height, channels, stride1, "first");
    if (rc) return rc;
    if (channels2 != channels) return oc_fail(MCC_EINVAL, "the two images must have the same number of channels");
    if (width2 != width || height2 != height) return oc_fail(MCC_EINVAL, "the two images must have the same size");
    if ((rc = or_check_image(image2, width2, height2, channels2, stride2, "second"))) return rc;
    if (desc->src_width != width || desc->src_height != height || desc->channels != channels)
        return oc_fail(MCC_EINVAL, "the images' size or channels differ from the descriptor's");
    if (!disparity || !rec1 || !rec2 || !n_points) return oc_fail(MCC_EINVAL, "null output");
    if (capacity < 0 || (capacity > 0 && !cloud)) return oc_fail(MCC_EINVAL, "null cloud with a positive capacity");
    mcc_pinrecon_geometry g{};
    if ((rc = pn_geometry(desc, &g))) return rc;
    if (rec1_stride < (long long)g.width * channels || rec2_stride < (long long)g.width * channels)
        return oc_fail(MCC_EINVAL, "rectified stride is smaller than a row");
    if (geometry) *geometry = g;
    mcc_pinrecon* h = nullptr;
    if ((rc = mcc_pinrecon_create(&h, desc))) return rc;
    rc = mcc_pinrecon_compute(h, image1, stride1, image2, stride2, disparity, disparity16, rec1, rec1_stride, rec2,
                              rec2_stride, points, cloud, capacity, n_points);
    mcc_pinrecon_destroy(h);
    return rc;
}

int mcc_pinrecon_host_cloud(const float* disparity, int width, int height, const double* Q, const unsigned char* rec1,
                            int channels, int point_type, const int* roi, double max_z, float* cloud, long long capacity,
                            long long* n_points) {
    if (!disparity || !Q || !n_points) return oc_fail(MCC_EINVAL, "null argument");
    int rc = or_check_size(width, height, "disparity");
    if (rc) return rc;
    if ((rc = pn_point_type(point_type))) return rc;
    if (point_type == MCC_XYZRGB && (!rec1 || (channels != 1 && channels != 3)))
        return oc_fail(MCC_EINVAL, "MCC_XYZRGB needs the first rectified image of 1 or 3 channels");
    if (capacity < 0 || (capacity > 0 && !cloud)) return oc_fail(MCC_EINVAL, "null cloud with a positive capacity");
    const mcc::PnCloudRule rule = pn_rule(roi, max_z);
    const int nf = point_type == MCC_XYZ ? 3 : 6;
    for (int pass = 0; pass < 2; ++pass) {   // count, then write: the device's two kernels
        long long n = 0;
        for (int i = 0; i < width; ++i)
            for (int j = 0; j < height; ++j) {
                const size_t o = (size_t)j * width + i;
                if (!mcc::pn_is_point(Q, rule, i, j, disparity[o])) continue;
                if (pass) {
                    double X, Y, Z, W;
                    mcc::pn_reproject(Q, i, j, disparity[o], X, Y, Z, W);
                    float* out = cloud + n * nf;
                    out[0] = mcc::pn_quotient(X, W), out[1] = mcc::pn_quotient(Y, W), out[2] = mcc::pn_quotient(Z, W);
                    if (nf == 6) {
                        const unsigned char* px = rec1 + o * channels;
                        out[3] = px[0], out[4] = px[channels == 3 ? 1 : 0], out[5] = px[channels == 3 ? 2 : 0];
                    }
                }
                ++n;
            }
        if (!pass) {
            *n_points = n;
            if (n > capacity)
                return oc_fail(MCC_EINVAL, "the cloud needs room for " + std::to_string(n) + " points, capacity is " +
                                               std::to_string(capacity));
        }
    }
    return MCC_OK;
}

}  // extern "C"
