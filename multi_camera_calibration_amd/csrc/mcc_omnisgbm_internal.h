// mcc_omnisgbm_internal.h -- kernel arguments of the semi-global matcher and of the tail of
// cv::omnidir::stereoReconstruct (src/omnidir.cpp:1383-1539), shared by mcc_omnisgbm.hip and
// mcc_omnisgbm_api.cpp.  Not part of the public ABI (include/mcc_omnidir.h).
//
// The volumes are indexed [y][x - D][d], d fastest; W1 = W - D columns are matched.
#pragma once
#include <hip/hip_runtime.h>

#include "mcc_omnicalib_internal.h"

namespace mcc {

// one signal plane entry per (pixel, channel): the gradient signal with its lo / hi, the raw one with its
struct alignas(8) SgSig {
    unsigned char g, glo, ghi, r, rlo, rhi, pad0, pad1;
};

struct SgArgs {
    const unsigned char* img[2];   // rectified pair, 8-bit, cn interleaved channels
    long long stride[2];           // bytes per row
    SgSig* sig[2];                 // [H][W][cn]
    unsigned short* cost;          // [H][W1][D] pixel cost, then C
    unsigned short* tmp;           // [H][W1][D] row sums of the box filter (the first half of `sum`)
    int* sum;                      // [H][W1][D] Lr of the first four directions, added up
    short* disp;                   // [H][W] disparity x 16
    unsigned int* key2;            // [H][W] ((min S + 32768) << 16) | (65535 - x) of the best left pixel per right column
    int H, W, D, cn, bs;
};

// the cloud is counted and written per column and segment of kSgSegRows rows
constexpr int kSgSegRows = 64;
inline int sg_cloud_segments(int cloud_h) { return (cloud_h + kSgSegRows - 1) / kSgSegRows; }

struct SgFinishArgs {
    const short* disp;             // [H][W]
    const unsigned char* rec1;     // first rectified image, packed rows of W * cn bytes
    float* real;                   // [H][W] disparity in pixels, 0 where rec1 is black
    int* col_count;                // [cloud_w n_seg + 1] points per column and row segment, then their exclusive scan
    float* cloud;                  // [W H] points of 3 or 6 floats
    double kinv[6];                // the first two rows of Knew^-1
    double bf;                     // |T| Knew(0, 0)
    int H, W, cn, flag, point_type;
    int cloud_w, cloud_h;          // newSize: the loop bounds of the cloud (0 x 0 if empty)
};

}  // namespace mcc

// all sizes are checked by the callers; the launches of one frame go to s in this order
hipError_t mcc_launch_sg_match(const mcc::SgArgs& a, hipStream_t s);
hipError_t mcc_launch_sg_finish(const mcc::SgFinishArgs& a, hipStream_t s);
