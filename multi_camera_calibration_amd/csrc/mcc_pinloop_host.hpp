// mcc_pinloop_host.hpp -- what the host sides of the pinhole calibrateCamera (mcc_pincalib_api.cpp) and
// stereoCalibrate (mcc_pinstereo_api.cpp) share: the checks of the views and of the criteria, one camera's
// K, D <-> 12 slots (fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6), the pose seeds, and PinLoop, the driver of the
// device-resident Levenberg-Marquardt loop (PcState, mcc_pincalib_internal.h; the kernels' share of it is
// mcc_pinloop_device.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mcc.h"
#include "mcc_omnicalib_host.hpp"
#include "mcc_pincalib_internal.h"

namespace {

constexpr int kPinCameraFlags = MCC_CALIB_USE_INTRINSIC_GUESS | MCC_CALIB_FIX_ASPECT_RATIO |
                                MCC_CALIB_FIX_PRINCIPAL_POINT | MCC_CALIB_ZERO_TANGENT_DIST |
                                MCC_CALIB_FIX_FOCAL_LENGTH | MCC_CALIB_FIX_K1 | MCC_CALIB_FIX_K2 | MCC_CALIB_FIX_K3 |
                                MCC_CALIB_FIX_K4 | MCC_CALIB_FIX_K5 | MCC_CALIB_FIX_K6 | MCC_CALIB_RATIONAL_MODEL;
constexpr int kPinTrialBatch = 8;       // trials enqueued between two reads of the state
constexpr int kPinEpsOnlyCount = 1000;  // accepted steps at most when the criteria have no count

// what every entry point requires of the views; img: the n_cams cameras' image points
int pin_check_views(const std::string& w, int n_views, const int* view_off, const double* obj, const double* const* img,
                    int n_cams, int width, int height) {
    if (n_views <= 0) return oc_fail(MCC_EINVAL, w + ": n_views must be positive");
    bool null = !view_off || !obj;
    for (int c = 0; c < n_cams; ++c) null = null || !img[c];
    if (null) return oc_fail(MCC_EINVAL, w + ": null pointer in the descriptor");
    if (width <= 0 || height <= 0) return oc_fail(MCC_EINVAL, w + ": the image size must be positive");
    if (view_off[0] < 0) return oc_fail(MCC_EINVAL, w + ": view_off[0] is negative");
    for (int v = 0; v < n_views; ++v) {
        const int n = view_off[v + 1] - view_off[v];
        if (n < 0) return oc_fail(MCC_EINVAL, w + ": view_off is not monotone at view " + std::to_string(v));
        if (n < 4 || n > mcc::kPcMaxCorners)
            return oc_fail(MCC_EINVAL, w + ": view " + std::to_string(v) + " has " + std::to_string(n) +
                                           " corners, 4 to " + std::to_string(mcc::kPcMaxCorners) + " are supported");
    }
    return MCC_OK;
}

int pin_check_criteria(const std::string& w, int crit_type, int max_count) {
    if (crit_type < 1 || crit_type > 3) return oc_fail(MCC_EINVAL, w + ": crit_type must be 1, 2 or 3");
    if ((crit_type & MCC_CRIT_COUNT) && max_count < 1) return oc_fail(MCC_EINVAL, w + ": max_count must be positive");
    return MCC_OK;
}

// one camera's slots from K and the nd coefficients of D (none where D is null); the others are left alone
void pin_pack(const double* K, const double* D, int nd, double* g) {
    g[0] = K[0]; g[1] = K[4]; g[2] = K[2]; g[3] = K[5];
    for (int k = 0; D && k < nd; ++k) g[4 + k] = D[k];
}

void pin_matrix(const double* g, double* K) {
    const double Kn[9] = {g[0], 0, g[2], 0, g[1], g[3], 0, 0, 1};
    std::memcpy(K, Kn, sizeof Kn);
}

void pin_unpack(const double* g, int nd, double* K, double* D) {
    pin_matrix(g, K);
    for (int k = 0; k < nd; ++k) D[k] = g[4 + k];
}

// what the flags fix at a value of their own, applied to a camera's start
void pin_start_edits(int flags, int nd, double aspect, double* g) {
    if (flags & MCC_CALIB_ZERO_TANGENT_DIST) g[6] = g[7] = 0.0;
    if (nd == 4) g[8] = 0.0;
    if (aspect > 0) g[0] = aspect * g[1];
}

// Every view's pose in each of n_cams (1 or 2) cameras at the slots g [12 n_cams], by one mcc_solve_pnp_batch
// over n_cams n views (camera 1's, then camera 2's; one wave per view, so batching does not change a pose).
// rvec[c], tvec[c]: [3 n].
int pin_seed_poses(const std::string& w, int n, const int* view_off, const double* obj, const double* const* img, int n_cams,
                   const double* g, int device, double* const* rvec, double* const* tvec) {
    const size_t first = (size_t)view_off[0], corners = (size_t)view_off[n] - first, nv = (size_t)n_cams * n;
    std::vector<int> off, cam, st(nv);
    std::vector<double> obj2, img2, Ks(9 * (size_t)n_cams), Ds(8 * (size_t)n_cams), r(3 * nv), t(3 * nv), e(nv);
    for (int c = 0; c < n_cams; ++c) {
        pin_matrix(g + mcc::kPcGlob * c, &Ks[9 * c]);
        std::memcpy(&Ds[8 * c], g + mcc::kPcGlob * c + 4, 8 * sizeof(double));
    }
    mcc_pnp_desc pd{};
    pd.n_views = (int)nv;
    if (n_cams == 1) {   // the caller's arrays as they are
        pd.view_off = view_off;
        pd.obj = obj;
        pd.img = img[0];
    } else {             // a copy of the corners per camera, each view named with its camera
        off.resize(nv + 1);
        cam.resize(nv);
        obj2.resize(3 * corners * n_cams);
        img2.resize(2 * corners * n_cams);
        for (int c = 0; c < n_cams; ++c) {
            std::memcpy(&obj2[3 * corners * c], obj + 3 * first, 3 * corners * sizeof(double));
            std::memcpy(&img2[2 * corners * c], img[c] + 2 * first, 2 * corners * sizeof(double));
            for (int v = 0; v < n; ++v) {
                off[(size_t)c * n + v] = (int)(corners * c) + view_off[v] - view_off[0];
                cam[(size_t)c * n + v] = c;
            }
        }
        off[nv] = (int)(corners * n_cams);
        pd.view_off = off.data();
        pd.obj = obj2.data();
        pd.img = img2.data();
        pd.view_cam = cam.data();
    }
    pd.n_cams = n_cams;
    pd.K = Ks.data();
    pd.D = Ds.data();
    pd.nd = 8;
    pd.max_iter = 50;
    pd.device = device;
    const int rc = mcc_solve_pnp_batch(&pd, r.data(), t.data(), e.data(), st.data(), nullptr);
    if (rc) return rc;
    for (int c = 0; c < n_cams; ++c)
        for (int v = 0; v < n; ++v) {
            const size_t i = (size_t)c * n + v;
            if (st[i] != MCC_PNP_SOLVED)
                return oc_fail(MCC_EINVAL, w + ": no pose seed for view " + std::to_string(v) +
                                               (n_cams > 1 ? " in camera " + std::to_string(c + 1) : std::string()) +
                                               " (solvePnP status " + std::to_string(st[i]) + ")");
            std::memcpy(rvec[c] + 3 * (size_t)v, &r[3 * i], 3 * sizeof(double));
            std::memcpy(tvec[c] + 3 * (size_t)v, &t[3 * i], 3 * sizeof(double));
        }
    return MCC_OK;
}

// The sizes in which the two loops differ (mcc_pincalib_internal.h, mcc_pinstereo_internal.h).
struct PinShape {
    int G, LinN, YzN, CtrN;   // global slots; doubles per view of lin, Yz and contrib
    int cams;                 // cameras: image-point buffers, and error slots per view (one per camera)
};

// The device-resident loop: the buffers both loops have (the image points of sh.cams cameras among them), the
// state, and the driver.  A caller takes the common kernel arguments with fill, sets its own and passes its two
// launches to run.
struct PinLoop {
    int n = 0, group_size = 1, n_groups = 1;
    size_t first = 0, corners = 0;    // the first corner uploaded and their number
    std::vector<int> off;             // [n + 1] the views' offsets from `first`
    PinShape sh{};
    DBuf<int> view_off, cnt;
    DBuf<double> obj, img[2], x, xt, glob, dc, lin, Yz, contrib, gsum, esq, esq_t, egs;
    DBuf<mcc::PcState> st;
    mcc::PcState s{};

    // imgs: the sh.cams cameras' image points; rvec, tvec: [3 n] the poses of the start; g: [G] its global slots
    int init(int device, int n_views, const int* voff, const double* pts, const double* const* imgs, const double* rvec,
             const double* tvec, const double* g, const PinShape& shape, int crit_type, int max_count, double eps) {
        n = n_views;
        sh = shape;
        first = (size_t)voff[0];
        corners = (size_t)voff[n] - first;
        off.resize((size_t)n + 1);
        for (int v = 0; v <= n; ++v) off[v] = voff[v] - voff[0];
        group_size = std::max(1, (int)std::ceil(std::sqrt((double)n)));
        n_groups = (n + group_size - 1) / group_size;
        std::vector<double> x0(6 * (size_t)n);
        for (int v = 0; v < n; ++v)
            for (int k = 0; k < 3; ++k) {
                x0[6 * (size_t)v + k] = rvec[3 * (size_t)v + k];
                x0[6 * (size_t)v + 3 + k] = tvec[3 * (size_t)v + k];
            }
        OCCHK(hipSetDevice(device));
        OCCHK(view_off.upload(off.data(), off.size()));
        OCCHK(obj.upload(pts + 3 * first, 3 * corners));
        for (int c = 0; c < sh.cams; ++c) OCCHK(img[c].upload(imgs[c] + 2 * first, 2 * corners));
        OCCHK(x.upload(x0.data(), x0.size()));
        OCCHK(xt.alloc(6 * (size_t)n));
        OCCHK(glob.upload(g, sh.G));
        OCCHK(dc.alloc(sh.G));
        OCCHK(lin.alloc((size_t)n * sh.LinN));
        OCCHK(Yz.alloc((size_t)n * sh.YzN));
        OCCHK(contrib.alloc((size_t)n * sh.CtrN));
        OCCHK(gsum.alloc((size_t)n_groups * sh.CtrN));
        OCCHK(esq.alloc((size_t)sh.cams * n));
        OCCHK(esq_t.alloc((size_t)sh.cams * n));
        OCCHK(egs.alloc((size_t)n_groups));
        OCCHK(cnt.alloc(2 * ((size_t)n_groups + 1)));
        OCCHK(hipMemset(cnt.p, 0, sizeof(int) * 2 * ((size_t)n_groups + 1)));
        s = mcc::PcState{};
        s.init = 1;
        s.relin = 1;
        s.crit_type = crit_type | MCC_CRIT_COUNT;
        s.max_count = (crit_type & MCC_CRIT_COUNT) ? max_count : kPinEpsOnlyCount;
        s.eps = eps;
        s.lambda = 1e-3;
        OCCHK(st.upload(&s, 1));
        return MCC_OK;
    }

    // the fields PcArgs and PsArgs have in common
    template <class Args>
    void fill(Args& a) const {
        a.n = n;
        a.view_off = view_off.p;
        a.obj = obj.p;
        a.x = x.p;
        a.xt = xt.p;
        a.glob = glob.p;
        a.dc = dc.p;
        a.lin = lin.p;
        a.Yz = Yz.p;
        a.contrib = contrib.p;
        a.gsum = gsum.p;
        a.esq = esq.p;
        a.esq_t = esq_t.p;
        a.egs = egs.p;
        a.cnt = cnt.p;
        a.st = st.p;
        a.group_size = group_size;
        a.n_groups = n_groups;
    }

    // The error of the start, then trials (launch_lin + launch_try) in batches until the state says done: at most
    // ten rejections per accepted step, so 11 max_count trials in all.  Leaves the final state in s.
    template <class Lin, class Try>
    int run(const std::string& w, Lin launch_lin, Try launch_try, int* trials, double* device_ms) {
        OcEvents ev;
        OCCHK(ev.create());
        OCCHK(hipEventRecord(ev.ev[0], nullptr));
        OCCHK(launch_try());
        const long long cap = 11LL * s.max_count;
        for (long long launched = 0; launched < cap;) {
            for (int b = 0; b < kPinTrialBatch && launched < cap; ++b, ++launched) {
                OCCHK(launch_lin());
                OCCHK(launch_try());
            }
            OCCHK(hipMemcpy(&s, st.p, sizeof s, hipMemcpyDeviceToHost));
            if (s.done) break;
        }
        OCCHK(hipEventRecord(ev.ev[1], nullptr));
        double ms = 0.0;
        OCCHK(ev.elapsed(&ms));
        OCCHK(hipMemcpy(&s, st.p, sizeof s, hipMemcpyDeviceToHost));
        if (trials) *trials = s.trials;
        if (device_ms) *device_ms = ms;
        if (s.status == mcc::kPcNotFinite) return oc_fail(MCC_EINVAL, w + ": the reprojection error of the start is not finite");
        if (!s.done) return oc_fail(MCC_EINVAL, w + ": the loop did not terminate");
        return MCC_OK;
    }

    // g: [G]; rvec, tvec: [3 n] or null; view_sq: [cams n] the squared error per view (and camera)
    int download(double* g, double* rvec, double* tvec, double* view_sq) {
        std::vector<double> x0(6 * (size_t)n);
        OCCHK(hipMemcpy(x0.data(), x.p, sizeof(double) * x0.size(), hipMemcpyDeviceToHost));
        OCCHK(hipMemcpy(g, glob.p, sizeof(double) * sh.G, hipMemcpyDeviceToHost));
        OCCHK(hipMemcpy(view_sq, esq.p, sizeof(double) * sh.cams * (size_t)n, hipMemcpyDeviceToHost));
        for (int v = 0; v < n; ++v)
            for (int k = 0; k < 3; ++k) {
                if (rvec) rvec[3 * (size_t)v + k] = x0[6 * (size_t)v + k];
                if (tvec) tvec[3 * (size_t)v + k] = x0[6 * (size_t)v + 3 + k];
            }
        return MCC_OK;
    }
};

}  // namespace
