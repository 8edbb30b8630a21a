// mcc_omnisgbm.hip -- CDNA4 kernels of the semi-global matcher behind cv::omnidir::stereoReconstruct
// (src/omnidir.cpp:1437-1439: StereoSGBM::create(0, D, bs, 8 cn bs^2, 32 cn bs^2)->compute) and of the
// function's tail (:1441-1538).  The specification is DESIGN.md 7e / tests/npsgbm.py; all matcher
// arithmetic is integer.  Volumes are [y][x - D][d] with d fastest, W1 = W - D columns are matched.
//
//   k_sg_signals   one thread per (pixel, channel) of both images: the gradient and the raw signal with
//                  their Birchfield-Tomasi lo / hi, 8 bytes.
//   k_sg_pix       one thread per (x, four d) of a row (d along the lanes, so the 8-byte volume stores
//                  coalesce): the pixel cost summed over channels.  The left entry is the same for every
//                  d, the right ones are contiguous.
//   k_sg_box       one pass of the bs x bs box sum with clamped taps, along x and then along y, four d
//                  per thread.
//   k_sg_path      one wave per path (per 64 / G paths where D <= 32, G = 16 or 32 lanes each); a lane
//                  owns d = lane + 64 k, k < NV.  Each step takes d +- 1 from the neighbour lanes by a DPP
//                  wave shift and min_d by a DPP butterfly within rows of 16 (two more exchanges across
//                  rows for a whole wave); the costs and sums of the next 8 pixels are always in flight.  The
//                  first four directions add their Lr into an int volume in stream order; the fifth
//                  saturates that sum, adds its own Lr, saturates again, and takes the winner, the
//                  sub-pixel disparity and the left-right key of its pixel without S ever reaching memory.
//   k_sg_lr        the left-right check, one thread per pixel.
//   k_sg_real      disparity / 16 with the black mask, one thread per pixel.
//   k_sg_count / k_sg_scan / k_sg_cloud   the point cloud in the reference's column-major order: points
//                  per column and segment of 64 rows, an exclusive scan by one workgroup, and one thread
//                  per column and segment that writes its points from its offset on.  No atomics hand out slots.
#include <hip/hip_runtime.h>

#include "../../include/mcc_omnidir.h"
#include "mcc_omnisgbm_internal.h"

namespace mcc {

constexpr int kSgBig = 32767;   // Lr(q, -1) = Lr(q, D)

// (gradient signal, raw signal) of channel c at (y, x): both are 15 in the first and the last column
template <int CN>
__device__ __forceinline__ void sg_signal(const unsigned char* img, long long stride, int H, int W, int y, int x, int c,
                                          int& g, int& r) {
    if (x <= 0 || x >= W - 1) {
        g = r = 15;
        return;
    }
    const unsigned char* p0 = img + (long long)y * stride + c;
    const unsigned char* pm = img + (long long)max(y - 1, 0) * stride + c;
    const unsigned char* pp = img + (long long)min(y + 1, H - 1) * stride + c;
    const int xl = (x - 1) * CN, xr = (x + 1) * CN;
    const int v = 2 * ((int)p0[xr] - (int)p0[xl]) + ((int)pm[xr] - (int)pm[xl]) + ((int)pp[xr] - (int)pp[xl]);
    g = min(max(v, -15), 15) + 15;
    r = p0[x * CN];
}

template <int CN>
__global__ __launch_bounds__(256) void k_sg_signals(SgArgs a) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;   // (x, c) of row blockIdx.y
    if (t >= (long long)a.W * CN) return;
    const int x = (int)(t / CN), c = (int)(t % CN), y = blockIdx.y;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int g0, r0, gm = 0, rm = 0, gp = 0, rp = 0;
        sg_signal<CN>(a.img[i], a.stride[i], a.H, a.W, y, x, c, g0, r0);
        int glo = g0, ghi = g0, rlo = r0, rhi = r0;
        if (x > 0) {
            sg_signal<CN>(a.img[i], a.stride[i], a.H, a.W, y, x - 1, c, gm, rm);
            glo = min(glo, (g0 + gm) >> 1), ghi = max(ghi, (g0 + gm) >> 1);
            rlo = min(rlo, (r0 + rm) >> 1), rhi = max(rhi, (r0 + rm) >> 1);
        }
        if (x < a.W - 1) {
            sg_signal<CN>(a.img[i], a.stride[i], a.H, a.W, y, x + 1, c, gp, rp);
            glo = min(glo, (g0 + gp) >> 1), ghi = max(ghi, (g0 + gp) >> 1);
            rlo = min(rlo, (r0 + rp) >> 1), rhi = max(rhi, (r0 + rp) >> 1);
        }
        SgSig s;
        s.g = (unsigned char)g0, s.glo = (unsigned char)glo, s.ghi = (unsigned char)ghi;
        s.r = (unsigned char)r0, s.rlo = (unsigned char)rlo, s.rhi = (unsigned char)rhi;
        s.pad0 = s.pad1 = 0;
        a.sig[i][((size_t)y * a.W + x) * CN + c] = s;
    }
}

__device__ __forceinline__ int sg_bt(int u, int v, int loL, int hiL, int loR, int hiR) {
    const int c0 = max(0, max(u - hiR, loR - u));
    const int c1 = max(0, max(v - hiL, loL - v));
    return min(c0, c1);
}

template <int CN>
__global__ __launch_bounds__(256) void k_sg_pix(SgArgs a) {
    const int W1 = a.W - a.D, D4 = a.D / 4, y = blockIdx.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;   // (x - D, d / 4): a thread owns four d
    if (t >= (long long)W1 * D4) return;
    const int xp = (int)(t / D4), d = (int)(t % D4) * 4;
    const int x = xp + a.D;                                          // the right columns x - d - j >= 1
    const SgSig* L = a.sig[0] + ((size_t)y * a.W + x) * CN;
    const SgSig* R = a.sig[1] + ((size_t)y * a.W + (x - d)) * CN;
    int cost[4] = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < CN; ++c) {
        const SgSig l = L[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const SgSig r = R[c - j * CN];
            cost[j] += sg_bt(l.g, r.g, l.glo, l.ghi, r.glo, r.ghi) + (sg_bt(l.r, r.r, l.rlo, l.rhi, r.rlo, r.rhi) >> 2);
        }
    }
    *(ushort4*)(a.cost + ((size_t)y * W1 + xp) * a.D + d) =
        make_ushort4((unsigned short)cost[0], (unsigned short)cost[1], (unsigned short)cost[2], (unsigned short)cost[3]);
}

// out(y, x, d) = sum over |k| <= r of in at the clamped neighbour along x (ALONG_X) or y; a thread owns four
// consecutive d (D is a multiple of 16, so its 8 bytes are aligned)
template <bool ALONG_X>
__global__ __launch_bounds__(256) void k_sg_box(const unsigned short* in, unsigned short* out, int H, int W1, int D, int r) {
    const int y = blockIdx.y, D4 = D / 4;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)W1 * D4) return;
    const int xp = (int)(t / D4), d = (int)(t % D4) * 4;
    int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int k = -r; k <= r; ++k) {
        const int yy = ALONG_X ? y : min(max(y + k, 0), H - 1);
        const int xx = ALONG_X ? min(max(xp + k, 0), W1 - 1) : xp;
        const ushort4 v = *(const ushort4*)(in + ((size_t)yy * W1 + xx) * D + d);
        s0 += v.x, s1 += v.y, s2 += v.z, s3 += v.w;
    }
    *(ushort4*)(out + ((size_t)y * W1 + xp) * D + d) =
        make_ushort4((unsigned short)s0, (unsigned short)s1, (unsigned short)s2, (unsigned short)s3);
}

// Cross-lane moves of the path step as DPP modifiers (no LDS crossbar round trip): the neighbour lanes by
// a wave shift -- the lanes it leaves without a source (and, between two paths of one wave, the lane it
// feeds from the other path) are the lanes l = 0 / l = G - 1, which the caller overrides -- and the minimum
// of a row of 16 by a butterfly of quad permutes and mirrors, after which every lane of the row holds it.
template <int CTRL>
__device__ __forceinline__ int sg_dpp(int v) {
    return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ int sg_lane_below(int v) { return sg_dpp<0x138>(v); }   // wave_shr:1, lane l - 1
__device__ __forceinline__ int sg_lane_above(int v) { return sg_dpp<0x130>(v); }   // wave_shl:1, lane l + 1

template <int G, typename T>
__device__ __forceinline__ T sg_group_min(T v) {
    v = min(v, (T)sg_dpp<0xB1>((int)v));    // quad_perm [1, 0, 3, 2]
    v = min(v, (T)sg_dpp<0x4E>((int)v));    // quad_perm [2, 3, 0, 1]
    v = min(v, (T)sg_dpp<0x141>((int)v));   // row_half_mirror
    v = min(v, (T)sg_dpp<0x140>((int)v));   // row_mirror
    if constexpr (G >= 32) v = min(v, (T)__shfl_xor((int)v, 16));
    if constexpr (G >= 64) v = min(v, (T)__shfl_xor((int)v, 32));
    return v;
}

constexpr int kSgAhead = 8;   // steps a path's loads run ahead of their use

struct SgPathArgs {
    const unsigned short* cost;
    int* sum;
    short* disp;
    unsigned int* key2;
    int H, W, D, W1;
    int dy, dx;        // the previous pixel of the path; the path itself moves by (-dy, -dx)
    int n_paths;
    int first;         // the first direction stores into sum, the others add
    int P1, P2;
};

// G lanes per path (16, 32 or 64), NV values of d per lane (more than one only with G = 64)
template <int G, int NV, bool LAST>
__global__ __launch_bounds__(256) void k_sg_path(SgPathArgs a) {
    static_assert(G == 64 || NV == 1, "several values per lane only with a whole wave per path");
    const int lane = threadIdx.x & 63, l = lane % G;
    const int path = (blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / G) + lane / G;
    const int W1 = a.W1, D = a.D, sx = -a.dx, sy = -a.dy;
    // where the path enters the image and how many pixels it has
    int y = 0, x = 0, len = 0;
    if (path < a.n_paths) {
        if (sy == 0) {
            y = path;
            x = sx > 0 ? 0 : W1 - 1;
            len = W1;
        } else {
            if (path < W1) {
                x = path;
            } else {   // the diagonals that enter through the left or the right border, below row 0
                y = path - W1 + 1;
                x = sx > 0 ? 0 : W1 - 1;
            }
            len = a.H - y;
            if (sx > 0) len = min(len, W1 - x);
            if (sx < 0) len = min(len, x + 1);
        }
    }
    int steps = len;   // of the longest path in this wave
#pragma unroll
    for (int o = 32; o >= G; o >>= 1) steps = max(steps, __shfl_xor(steps, o));

    int Lp[NV];
    bool valid[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        valid[k] = l + 64 * k < D;
        Lp[k] = valid[k] ? 0 : kSgBig;   // a pixel outside gives C - P2, which is what an all-zero Lr(q) gives
    }
    int m = 0;
    // Neither the costs nor the sums depend on the path's own state, so both are loaded kSgAhead steps
    // before their use: a step then waits for arithmetic, not for memory.  The buffers are indexed by the
    // position in the unrolled group of kSgAhead steps, so they stay in registers.
    const long long stride = ((long long)sy * W1 + sx) * D;   // entries from one pixel of the path to the next
    long long off = ((long long)y * W1 + x) * D;
    const bool need_sum = LAST || !a.first;
    int cb[kSgAhead][NV], sb[kSgAhead][NV];
#pragma unroll
    for (int u = 0; u < kSgAhead; ++u)
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const bool ld = valid[k] && u < len;
            const long long o = off + u * stride + l + 64 * k;
            cb[u][k] = ld ? a.cost[o] : 0;
            sb[u][k] = (ld && need_sum) ? a.sum[o] : 0;
        }

    for (int base = 0; base < steps; base += kSgAhead) {
#pragma unroll
        for (int u = 0; u < kSgAhead; ++u) {
            const int step = base + u;
            const bool act = step < len;
            int Ln[NV];
            int mn = kSgBig;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                int below = sg_lane_below(Lp[k]), above = sg_lane_above(Lp[k]);
                const int wrap_lo = k > 0 ? __builtin_amdgcn_readlane(Lp[k > 0 ? k - 1 : 0], 63) : kSgBig;
                const int wrap_hi = k < NV - 1 ? __builtin_amdgcn_readlane(Lp[k < NV - 1 ? k + 1 : k], 0) : kSgBig;
                if (l == 0) below = wrap_lo;
                if (l == G - 1) above = wrap_hi;
                const int best = min(min(Lp[k], m + a.P2), min(below, above) + a.P1);
                Ln[k] = valid[k] ? cb[u][k] + best - (m + a.P2) : kSgBig;
                mn = min(mn, Ln[k]);
            }
            mn = sg_group_min<G>(mn);

            if constexpr (!LAST) {
                if (act) {
#pragma unroll
                    for (int k = 0; k < NV; ++k)
                        if (valid[k]) a.sum[off + l + 64 * k] = sb[u][k] + Ln[k];   // sb is 0 in the first direction
                }
            } else {
                // S = sat16(sat16(sum of four) + Lr), then the smallest d attaining min S
                int S[NV];
                unsigned int key = 0xffffffffu;
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    S[k] = kSgBig;
                    if (valid[k] && act) {
                        const int four = min(max(sb[u][k], -32768), 32767);
                        S[k] = min(max(four + Ln[k], -32768), 32767);
                        key = min(key, ((unsigned int)(S[k] + 32768) << 16) | (unsigned int)(l + 64 * k));
                    }
                }
                key = sg_group_min<G>(key);
                const int ds = (int)(key & 0xffffu), smin = (int)(key >> 16) - 32768;
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    int sm = sg_lane_below(S[k]), sp = sg_lane_above(S[k]);
                    const int wrap_lo = k > 0 ? __builtin_amdgcn_readlane(S[k > 0 ? k - 1 : 0], 63) : 0;
                    const int wrap_hi = k < NV - 1 ? __builtin_amdgcn_readlane(S[k < NV - 1 ? k + 1 : k], 0) : 0;
                    if (l == 0) sm = wrap_lo;
                    if (l == G - 1) sp = wrap_hi;
                    if (act && valid[k] && l + 64 * k == ds) {   // the lane that owns d*
                        int d16 = 16 * ds;
                        if (ds > 0 && ds < D - 1) {
                            const int den = max(sm + sp - 2 * smin, 1);
                            const int num = (sm - sp) * 16 + den, q = 2 * den;
                            d16 += num >= 0 ? num / q : -((-num + q - 1) / q);   // floor
                        }
                        const int xi = x + D;
                        a.disp[(size_t)y * a.W + xi] = (short)d16;
                        atomicMin(a.key2 + (size_t)y * a.W + (xi - ds),
                                  ((unsigned int)(smin + 32768) << 16) | (unsigned int)(65535 - xi));
                    }
                }
            }

            // this slot's next use is kSgAhead steps on
            const bool ld = step + kSgAhead < len;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const long long o = off + kSgAhead * stride + l + 64 * k;
                cb[u][k] = (valid[k] && ld) ? a.cost[o] : 0;
                sb[u][k] = (valid[k] && ld && need_sum) ? a.sum[o] : 0;
                if (act) Lp[k] = Ln[k];
            }
            if (act) {
                m = mn;
                y += sy;
                x += sx;
                off += stride;
            }
        }
    }
}

// disp2 of a right column is the d* of the left pixel behind key2's minimum; a pixel goes invalid when
// both its floor and its ceiling disparity disagree with disp2 by more than one
__global__ __launch_bounds__(256) void k_sg_lr(SgArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= a.W) return;
    short* row = a.disp + (size_t)y * a.W;
    if (x < a.D) {
        row[x] = -16;
        return;
    }
    const unsigned int* k2 = a.key2 + (size_t)y * a.W;
    const int d1 = row[x];
    const int da = d1 >> 4, db = (d1 + 15) >> 4;
    bool bad = true;
    for (int i = 0; i < 2; ++i) {
        const int d = i ? db : da, xr = x - d;
        if (xr < 0 || xr >= a.W) {
            bad = false;
            continue;
        }
        const unsigned int key = k2[xr];
        const int d2 = key == 0xffffffffu ? -1 : (65535 - (int)(key & 0xffffu)) - xr;
        if (d2 < 0 || abs(d2 - d) <= 1) bad = false;
    }
    if (bad) row[x] = -16;
}

__device__ __forceinline__ int sg_gray(const unsigned char* p, int cn) {
    return cn == 1 ? p[0] : (4899 * p[0] + 9617 * p[1] + 1868 * p[2] + 8192) >> 14;
}

__global__ __launch_bounds__(256) void k_sg_real(SgFinishArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= a.W) return;
    const size_t o = (size_t)y * a.W + x;
    float v = (float)a.disp[o] / 16.0f;
    if (sg_gray(a.rec1 + o * a.cn, a.cn) <= 0) v = 0.0f;
    a.real[o] = v;
}

// points of column i < cloud_w in the rows of segment blockIdx.y (kSgSegRows rows each): slot
// i * n_seg + segment, so that the scan runs in the cloud's order, columns first
__global__ __launch_bounds__(256) void k_sg_count(SgFinishArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x, seg = blockIdx.y;
    if (i >= a.cloud_w) return;
    const int j1 = min((seg + 1) * kSgSegRows, a.cloud_h);
    int n = 0;
    for (int j = seg * kSgSegRows; j < j1; ++j) n += a.real[(size_t)j * a.W + i] > 15.0f ? 1 : 0;
    a.col_count[(size_t)i * gridDim.y + seg] = n;
}

// exclusive scan of v[0 .. W) in place by one workgroup; v[W] = the total
__global__ __launch_bounds__(1024) void k_sg_scan(int* v, int W) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (W + 1023) / 1024, lo = min(t * per, W), hi = min(lo + per, W);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += v[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {   // Hillis-Steele, inclusive
        const int add = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = lo; i < hi; ++i) {
        const int n = v[i];
        v[i] = run;
        run += n;
    }
    if (t == 1023) v[W] = part[1023];
}

__global__ __launch_bounds__(256) void k_sg_cloud(SgFinishArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x, seg = blockIdx.y;
    if (i >= a.cloud_w) return;
    const int nf = a.point_type == MCC_OMNI_XYZ ? 3 : 6;
    float* out = a.cloud + (size_t)a.col_count[(size_t)i * gridDim.y + seg] * nf;
    const int j1 = min((seg + 1) * kSgSegRows, a.cloud_h);
    for (int j = seg * kSgSegRows; j < j1; ++j) {
        const size_t o = (size_t)j * a.W + i;
        const float rd = a.real[o];
        if (!(rd > 15.0f)) continue;
        const float depth = (float)(a.bf / (double)rd);
        const float x = (float)(a.kinv[0] * i + a.kinv[1] * j + a.kinv[2]);
        const float y = (float)(a.kinv[3] * i + a.kinv[4] * j + a.kinv[5]);
        float p0, p1, p2;
        if (a.flag == MCC_OMNI_RECTIFY_LONGLATI) {
            p0 = -cosf(x), p1 = -sinf(x) * cosf(y), p2 = sinf(x) * sinf(y);
        } else {
            p0 = x, p1 = y, p2 = 1.0f;
        }
        out[0] = p0 * depth, out[1] = p1 * depth, out[2] = p2 * depth;
        if (nf == 6) {
            const unsigned char* px = a.rec1 + o * a.cn;
            out[3] = px[0];
            out[4] = px[a.cn == 3 ? 1 : 0];
            out[5] = px[a.cn == 3 ? 2 : 0];
        }
        out += nf;
    }
}

}  // namespace mcc

namespace {

template <int G, int NV>
void sg_path_launch(const mcc::SgPathArgs& p, bool last, hipStream_t s) {
    const int per_block = 4 * (64 / G);
    const dim3 grid((p.n_paths + per_block - 1) / per_block);
    if (last)
        hipLaunchKernelGGL((mcc::k_sg_path<G, NV, true>), grid, dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((mcc::k_sg_path<G, NV, false>), grid, dim3(256), 0, s, p);
}

}  // namespace

hipError_t mcc_launch_sg_match(const mcc::SgArgs& a, hipStream_t s) {
    const int W1 = a.W - a.D;
    if (a.H < 1 || W1 < 1 || a.D < 16 || a.D > 256 || (a.cn != 1 && a.cn != 3) || a.bs < 1) return hipErrorInvalidValue;
    const long long row = (long long)W1 * a.D;
    const dim3 gsig((unsigned)(((long long)a.W * a.cn + 255) / 256), a.H), gvol4((unsigned)((row / 4 + 255) / 256), a.H);
    if (a.cn == 1) {
        hipLaunchKernelGGL(mcc::k_sg_signals<1>, gsig, dim3(256), 0, s, a);
        hipLaunchKernelGGL(mcc::k_sg_pix<1>, gvol4, dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(mcc::k_sg_signals<3>, gsig, dim3(256), 0, s, a);
        hipLaunchKernelGGL(mcc::k_sg_pix<3>, gvol4, dim3(256), 0, s, a);
    }
    if (a.bs > 1) {
        hipLaunchKernelGGL(mcc::k_sg_box<true>, gvol4, dim3(256), 0, s, a.cost, a.tmp, a.H, W1, a.D, a.bs / 2);
        hipLaunchKernelGGL(mcc::k_sg_box<false>, gvol4, dim3(256), 0, s, a.tmp, a.cost, a.H, W1, a.D, a.bs / 2);
    }
    hipError_t e = hipMemsetAsync(a.key2, 0xff, sizeof(unsigned int) * (size_t)a.H * a.W, s);
    if (e != hipSuccess) return e;
    const int dirs[5][2] = {{0, -1}, {-1, -1}, {-1, 0}, {-1, 1}, {0, 1}};
    for (int k = 0; k < 5; ++k) {
        mcc::SgPathArgs p{};
        p.cost = a.cost, p.sum = a.sum, p.disp = a.disp, p.key2 = a.key2;
        p.H = a.H, p.W = a.W, p.D = a.D, p.W1 = W1;
        p.dy = dirs[k][0], p.dx = dirs[k][1];
        p.n_paths = p.dy == 0 ? a.H : (p.dx == 0 ? W1 : W1 + a.H - 1);
        p.first = k == 0;
        p.P1 = 8 * a.cn * a.bs * a.bs, p.P2 = 32 * a.cn * a.bs * a.bs;
        const bool last = k == 4;
        if (a.D <= 16) sg_path_launch<16, 1>(p, last, s);
        else if (a.D <= 32) sg_path_launch<32, 1>(p, last, s);
        else if (a.D <= 64) sg_path_launch<64, 1>(p, last, s);
        else if (a.D <= 128) sg_path_launch<64, 2>(p, last, s);
        else if (a.D <= 192) sg_path_launch<64, 3>(p, last, s);
        else sg_path_launch<64, 4>(p, last, s);
    }
    hipLaunchKernelGGL(mcc::k_sg_lr, dim3((a.W + 255) / 256, a.H), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t mcc_launch_sg_finish(const mcc::SgFinishArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(mcc::k_sg_real, dim3((a.W + 255) / 256, a.H), dim3(256), 0, s, a);
    const int n_seg = mcc::sg_cloud_segments(a.cloud_h);
    const dim3 grid((a.cloud_w + 255) / 256, n_seg);
    if (n_seg > 0 && a.cloud_w > 0) hipLaunchKernelGGL(mcc::k_sg_count, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(mcc::k_sg_scan, dim3(1), dim3(1024), 0, s, a.col_count, a.cloud_w * n_seg);
    if (n_seg > 0 && a.cloud_w > 0) hipLaunchKernelGGL(mcc::k_sg_cloud, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
