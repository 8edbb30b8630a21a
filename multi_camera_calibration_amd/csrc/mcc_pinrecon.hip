// mcc_pinrecon.hip -- CDNA4 kernels of cv::reprojectImageTo3D and of the tail of the pinhole stereoReconstruct
// (DESIGN.md 7j).  The remap is k_or_remap (mcc_omnirect.hip), the maps are k_pr_map (mcc_pinrect.hip), the
// matcher is mcc_launch_sg_match (mcc_omnisgbm.hip); none of them is changed.  No LDS but the reduction's 16
// bytes, no stack, no out-of-line calls; FP64 with FMA contraction off (the numpy model's rounding).
//
//   k_pn_dmin       the minimum of the disparity image in two levels: up to kPnDminBlocks workgroups each fold a
//                   grid-strided share into one partial (lanes by shuffles, waves through LDS), then one
//                   workgroup folds the partials.  No atomics; fminf, so the order cannot matter and a NaN is skipped.
//   k_pn_reproject  a 256-wide row tile per workgroup in x, rows in blockIdx.y (as k_sg_real): Q (x, y, d, 1), three
//                   float64 divisions, three float stores.  The disparity type and handle_missing are template
//                   parameters; Q is sixteen kernel arguments.  In the handle it also writes the float disparity
//                   (d16 / 16.0f), so that step needs no pass of its own.
//   k_pn_count / k_pn_cloud   the cloud in k_sg_count's layout (points per column and segment of kSgSegRows rows) and
//                   k_sg_cloud's order, with k_sg_scan between them; both ask pn_is_point, the host model's function.
//                   k_pn_cloud computes a point again from its disparity, with the dense image's functions.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/mcc.h"
#include "mcc_omnisgbm_internal.h"
#include "mcc_pinrecon_internal.h"

namespace mcc {

// defined in mcc_omnisgbm.hip: the exclusive scan of v[0 .. W) in place by one workgroup of 1024; v[W] = the total
__global__ void k_sg_scan(int* v, int W);

template <int TYPE>
__device__ __forceinline__ float pn_load(const void* disp, size_t o) {
    if constexpr (TYPE == MCC_DISP_FLOAT) return ((const float*)disp)[o];
    else return (float)((const short*)disp)[o] / 16.0f;   // exact: a short has 16 bits, a float 24
}

// the minimum of a workgroup of 256 in every thread of its first wave
__device__ __forceinline__ float pn_block_min(float m) {
    __shared__ float part[4];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fminf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    return fminf(fminf(part[0], part[1]), fminf(part[2], part[3]));
}

template <int TYPE>
__global__ __launch_bounds__(256) void k_pn_dmin(const void* disp, long long n, float* partial) {
    float m = __builtin_inff();
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        m = fminf(m, pn_load<TYPE>(disp, (size_t)i));
    m = pn_block_min(m);
    if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// partial[0 .. n) -> partial[kPnDminBlocks]
__global__ __launch_bounds__(256) void k_pn_dmin_fold(float* partial, int n) {
    float m = __builtin_inff();
    for (int i = threadIdx.x; i < n; i += 256) m = fminf(m, partial[i]);
    m = pn_block_min(m);
    if (threadIdx.x == 0) partial[kPnDminBlocks] = m;
}

template <int TYPE, bool MISSING>
__global__ __launch_bounds__(256) void k_pn_reproject(PnReprojectArgs a) {
#pragma clang fp contract(off)
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= a.w) return;
    const size_t o = (size_t)y * a.w + x;
    const float d = pn_load<TYPE>(a.disp, o);
    if (a.real) a.real[o] = d;
    double X, Y, Z, W;
    pn_reproject(a.q, x, y, d, X, Y, Z, W);
    float* p = a.points + o * 3;
    p[0] = pn_quotient(X, W);
    p[1] = pn_quotient(Y, W);
    float z = pn_quotient(Z, W);
    if constexpr (MISSING) {
        if (d <= *a.dmin) z = 10000.0f;
    }
    p[2] = z;
}

__global__ __launch_bounds__(256) void k_pn_count(PnCloudArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x, seg = blockIdx.y;
    if (i >= a.w) return;
    const int j1 = min((seg + 1) * kSgSegRows, a.h);
    int n = 0;
    for (int j = seg * kSgSegRows; j < j1; ++j) n += pn_is_point(a.q, a.rule, i, j, a.real[(size_t)j * a.w + i]) ? 1 : 0;
    a.col_count[(size_t)i * gridDim.y + seg] = n;
}

__global__ __launch_bounds__(256) void k_pn_cloud(PnCloudArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x, seg = blockIdx.y;
    if (i >= a.w) return;
    const int nf = a.point_floats;
    float* out = a.cloud + (size_t)a.col_count[(size_t)i * gridDim.y + seg] * nf;
    const int j1 = min((seg + 1) * kSgSegRows, a.h);
    // Only some 300 waves exist at 1280 x 960, so a thread's walk down its column is bound by load latency: the
    // disparities and colours of kPnCloudBatch rows are loaded together, and a point is computed again from its
    // disparity (pn_reproject and pn_quotient, the dense image's own functions and so its bits) instead of being
    // loaded once the predicate is known.
    for (int j0 = seg * kSgSegRows; j0 < j1; j0 += kPnCloudBatch) {
        float d[kPnCloudBatch];
        unsigned char c[kPnCloudBatch][3];
#pragma unroll
        for (int u = 0; u < kPnCloudBatch; ++u) {
            const size_t o = (size_t)min(j0 + u, j1 - 1) * a.w + i;
            d[u] = j0 + u < j1 ? a.real[o] : -1.0f;   // a row past the segment is no point
            if (nf == 6) {
                const unsigned char* px = a.rec1 + o * a.cn;
                c[u][0] = px[0], c[u][1] = px[a.cn == 3 ? 1 : 0], c[u][2] = px[a.cn == 3 ? 2 : 0];
            }
        }
#pragma unroll
        for (int u = 0; u < kPnCloudBatch; ++u) {
            if (!pn_is_point(a.q, a.rule, i, j0 + u, d[u])) continue;
            double X, Y, Z, W;
            pn_reproject(a.q, i, j0 + u, d[u], X, Y, Z, W);
            out[0] = pn_quotient(X, W), out[1] = pn_quotient(Y, W), out[2] = pn_quotient(Z, W);
            if (nf == 6) out[3] = c[u][0], out[4] = c[u][1], out[5] = c[u][2];
            out += nf;
        }
    }
}

}  // namespace mcc

namespace {

template <int TYPE>
void pn_reproject_launch(const mcc::PnReprojectArgs& a, bool missing, float* partial, hipStream_t s) {
    const dim3 grid((a.w + 255) / 256, a.h);
    if (!missing) {
        hipLaunchKernelGGL((mcc::k_pn_reproject<TYPE, false>), grid, dim3(256), 0, s, a);
        return;
    }
    const long long n = (long long)a.w * a.h;
    const int blocks = (int)std::min<long long>((n + 255) / 256, mcc::kPnDminBlocks);
    hipLaunchKernelGGL((mcc::k_pn_dmin<TYPE>), dim3(blocks), dim3(256), 0, s, a.disp, n, partial);
    hipLaunchKernelGGL(mcc::k_pn_dmin_fold, dim3(1), dim3(256), 0, s, partial, blocks);
    hipLaunchKernelGGL((mcc::k_pn_reproject<TYPE, true>), grid, dim3(256), 0, s, a);
}

}  // namespace

hipError_t mcc_launch_pn_reproject(const mcc::PnReprojectArgs& a, int type, bool missing, float* partial, hipStream_t s) {
    if (a.w < 1 || a.h < 1 || a.h > 65535 || (type != MCC_DISP_FLOAT && type != MCC_DISP_FIXED16)) return hipErrorInvalidValue;
    if (missing && (!partial || a.dmin != partial + mcc::kPnDminBlocks)) return hipErrorInvalidValue;
    if (type == MCC_DISP_FLOAT)
        pn_reproject_launch<MCC_DISP_FLOAT>(a, missing, partial, s);
    else
        pn_reproject_launch<MCC_DISP_FIXED16>(a, missing, partial, s);
    return hipGetLastError();
}

hipError_t mcc_launch_pn_cloud(const mcc::PnCloudArgs& a, hipStream_t s) {
    if (a.w < 1 || a.h < 1 || (a.point_floats != 3 && a.point_floats != 6)) return hipErrorInvalidValue;
    const int n_seg = mcc::sg_cloud_segments(a.h);
    const dim3 grid((a.w + 255) / 256, n_seg);
    hipLaunchKernelGGL(mcc::k_pn_count, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(mcc::k_sg_scan, dim3(1), dim3(1024), 0, s, a.col_count, a.w * n_seg);
    hipLaunchKernelGGL(mcc::k_pn_cloud, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
