// mcc_pinstereo_device.hpp -- one view of the pinhole stereoCalibrate's Levenberg-Marquardt trial, as one
// wave64 runs it (k_ps_lin, k_ps_try: mcc_pinstereo.hip).  Like mcc_pincalib_device.hpp, on which it is
// built, it compiles for the host with one lane (MCC_PNP_LANES 1: tests/cpp/pinstereo_step.cpp).
//
// The global block has kPsG = 30 slots: the rig (om, T) | camera 1's fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 |
// camera 2's.  Camera 2 sees view v at R2 = R R_v, t2 = R t_v + T with R = exp(om).
//
// A camera's rows of a view depend on that camera's pose of the view and its own 12 slots only, which are
// the 189 sums of PcLin: camera 1 is pc_linearize at (r_v, t_v), camera 2 pc_linearize_rj at the composed
// pose with its rotation columns in the left tangent (phi2, dt2) of R2.  With
//   R_v(r + d) = exp([Jl(r) d]x) R_v   and   R(om + d) = exp([Jl(om) d]x) R
// the tangent of camera 2's pose is
//   (phi2, dt2) = A (dr_v, dt_v) + B (dom, dT),   A = blockdiag(R Jl(r_v), R),
//                                                 B = [[Jl(om), 0], [-[R t_v]x Jl(om), I]],
// and the sums are bilinear in the rows, so A and B are applied to camera 2's sums (ps_assemble), not per
// corner.  SAME_FOCAL_LENGTH folds camera 2's fx, fy columns into camera 1's there, which makes the
// camera-1 / camera-2 block of V non-zero: V is a full symmetric 30 x 30, kept as its upper triangle.
//
// ps_eliminate is pc_eliminate 30 wide; ps_reduced_solve is the same symmetric elimination as
// pc_reduced_solve, but on a 30 x 30 in LDS with the lanes over its rows.
#pragma once
#include "mcc_pincalib_device.hpp"

namespace mcc {

constexpr int kPsG = 30;
constexpr int kPsCam1 = 6, kPsCam2 = 18;   // the cameras' first slots; the rig is 0 .. 5

// a view's linearisation in (dr_v, dt_v | the 30 slots), undamped
struct PsLin {
    static constexpr int U = 0;                 // [21] upper triangle, row-major
    static constexpr int Gp = 21;               // [6]
    static constexpr int W = 27;                // [6][30]
    static constexpr int V = 207;               // [465] upper triangle, row-major
    static constexpr int Gc = 672;              // [30]
    static constexpr int N = 702;
};

// a view's packed contribution to the reduced system
struct PsCtr {
    static constexpr int S = 0;                 // [465] V_v - W_v^T Y_v, upper triangle
    static constexpr int Rc = 465;              // [30]  g_c,v - W_v^T z_v
    static constexpr int Dg = 495;              // [30]  diag V_v
    static constexpr int Bad = 525;
    static constexpr int N = 526;
};

// ps_assemble's scratch (LDS): the maps and camera 2's pose block under them, 6 x 6 row-major each
struct PsTmp {
    static constexpr int A = 0, B = 36, UA = 72, UB = 108, N = 144;
};

constexpr int kPsYzN = 6 * kPsG + 6;   // Y_v [6][30], then z_v [6]

// the mask of camera cam's 12 slots as its linearisation takes it: under SAME_FOCAL_LENGTH camera 2's fx, fy
// are fixed slots of the solve but their columns exist (they are added to camera 1's)
MCC_PNP_FN int ps_lin_mask(int mask, int same, int cam) {
    const int m1 = (mask >> kPsCam1) & 0xfff;
    return cam == 0 ? m1 : (((mask >> kPsCam2) & 0xfff) | (same ? (m1 & 3) : 0));
}

// R2 = R Rv, t2 = R tv + T; contraction off, so that the error of the current and of a trial state round alike
MCC_PNP_FN void ps_compose(const double* R, const double* T, const double* Rv, const double* tv, double* R2,
                           double* t2) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R2[i * 3 + j] = R[i * 3] * Rv[j] + R[i * 3 + 1] * Rv[3 + j] + R[i * 3 + 2] * Rv[6 + j];
        t2[i] = R[i * 3] * tv[0] + R[i * 3 + 1] * tv[1] + R[i * 3 + 2] * tv[2] + T[i];
    }
}

// A and B into tmp (lane 0; the caller synchronises).  R, Jo: the rig's rotation and Jl(om); Jv = Jl(r_v)
MCC_PNP_FN void ps_maps(const double* R, const double* Jo, const double* Jv, const double* tv, int lane, double* tmp) {
    if (lane != 0) return;
    double RJ[9], Q[9];
    mat3_mul(R, Jv, RJ);
    const double q[3] = {R[0] * tv[0] + R[1] * tv[1] + R[2] * tv[2], R[3] * tv[0] + R[4] * tv[1] + R[5] * tv[2],
                         R[6] * tv[0] + R[7] * tv[1] + R[8] * tv[2]};
    const double qx[9] = {0, q[2], -q[1], -q[2], 0, q[0], q[1], -q[0], 0};   // -[q]x
    mat3_mul(qx, Jo, Q);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            tmp[PsTmp::A + i * 6 + j] = RJ[i * 3 + j];
            tmp[PsTmp::A + i * 6 + 3 + j] = 0.0;
            tmp[PsTmp::A + (3 + i) * 6 + j] = 0.0;
            tmp[PsTmp::A + (3 + i) * 6 + 3 + j] = R[i * 3 + j];
            tmp[PsTmp::B + i * 6 + j] = Jo[i * 3 + j];
            tmp[PsTmp::B + i * 6 + 3 + j] = 0.0;
            tmp[PsTmp::B + (3 + i) * 6 + j] = Q[i * 3 + j];
            tmp[PsTmp::B + (3 + i) * 6 + 3 + j] = i == j ? 1.0 : 0.0;
        }
}

// (i, j) of the packed upper-triangle index e of a G x G matrix
MCC_PNP_FN void ps_unpack(int e, int G, int& i, int& j) {
    i = 0;
    while (e >= G - i) { e -= G - i; ++i; }
    j = i + e;
}

// sum_m P[m][i] Q[m][j], P with row stride sp and Q with sq
MCC_PNP_FN double ps_dot6(const double* P, int sp, int i, const double* Q, int sq, int j) {
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 6; ++m) s += P[m * sp + i] * Q[m * sq + j];
    return s;
}

// the arrow's entries before the SAME_FOCAL_LENGTH fold, from camera 1's sums L1, camera 2's L2 and tmp
MCC_PNP_FN double ps_w_raw(const double* L1, const double* L2, const double* tmp, int k, int j) {
    if (j < kPsCam1) return ps_dot6(tmp + PsTmp::A, 6, k, tmp + PsTmp::UB, 6, j);                // A^T U2 B
    if (j < kPsCam2) return L1[PcLin::W + k * kPcG + (j - kPsCam1)];                             // W1
    return ps_dot6(tmp + PsTmp::A, 6, k, L2 + PcLin::W, kPcG, j - kPsCam2);                      // A^T W2
}

MCC_PNP_FN double ps_v_raw(const double* L1, const double* L2, const double* tmp, int i, int j) {
    if (i > j) { const int s = i; i = j; j = s; }
    if (i < kPsCam1) {
        if (j < kPsCam1) return ps_dot6(tmp + PsTmp::B, 6, i, tmp + PsTmp::UB, 6, j);            // B^T U2 B
        if (j < kPsCam2) return 0.0;
        return ps_dot6(tmp + PsTmp::B, 6, i, L2 + PcLin::W, kPcG, j - kPsCam2);                  // B^T W2
    }
    if (i < kPsCam2) return j < kPsCam2 ? L1[PcLin::V + pc_up(i - kPsCam1, j - kPsCam1, kPcG)] : 0.0;
    return L2[PcLin::V + pc_up(i - kPsCam2, j - kPsCam2, kPcG)];
}

MCC_PNP_FN double ps_g_raw(const double* L1, const double* L2, const double* tmp, int j) {
    if (j < kPsCam1) return ps_dot6(tmp + PsTmp::B, 6, j, L2 + PcLin::Gp, 1, 0);                 // B^T g2
    return j < kPsCam2 ? L1[PcLin::Gc + j - kPsCam1] : L2[PcLin::Gc + j - kPsCam2];
}

// The view's arrow L [PsLin::N] from the two cameras' sums and the maps ps_maps left in tmp; all in LDS.
// same: camera 2's fx, fy columns are added to camera 1's and are zero themselves.
MCC_PNP_FN void ps_assemble(const double* L1, const double* L2, double* tmp, int same, int lane, double* L) {
    for (int e = lane; e < 72; e += MCC_PNP_LANES) {   // U2 A and U2 B
        const double* Mp = tmp + (e < 36 ? PsTmp::A : PsTmp::B);
        const int i = (e % 36) / 6, j = e % 6;
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 6; ++m) s += L2[PcLin::U + (i <= m ? pc_up(i, m, 6) : pc_up(m, i, 6))] * Mp[m * 6 + j];
        tmp[PsTmp::UA + e] = s;
    }
    pnp_wave_sync();
    for (int e = lane; e < PsLin::N; e += MCC_PNP_LANES) {
        double s;
        if (e < PsLin::Gp) {
            int i, j;
            ps_unpack(e, 6, i, j);
            s = L1[PcLin::U + e] + ps_dot6(tmp + PsTmp::A, 6, i, tmp + PsTmp::UA, 6, j);
        } else if (e < PsLin::W) {
            const int i = e - PsLin::Gp;
            s = L1[PcLin::Gp + i] + ps_dot6(tmp + PsTmp::A, 6, i, L2 + PcLin::Gp, 1, 0);
        } else if (e < PsLin::V) {
            const int k = (e - PsLin::W) / kPsG, j = (e - PsLin::W) % kPsG;
            const bool tied = same && (j == kPsCam2 || j == kPsCam2 + 1), dup = same && (j == kPsCam1 || j == kPsCam1 + 1);
            s = tied ? 0.0 : ps_w_raw(L1, L2, tmp, k, j);
            if (dup) s += ps_w_raw(L1, L2, tmp, k, j + 12);
        } else if (e < PsLin::Gc) {
            int i, j;
            ps_unpack(e - PsLin::V, kPsG, i, j);
            const bool ti = same && (i == kPsCam2 || i == kPsCam2 + 1), tj = same && (j == kPsCam2 || j == kPsCam2 + 1);
            const bool di = same && (i == kPsCam1 || i == kPsCam1 + 1), dj = same && (j == kPsCam1 || j == kPsCam1 + 1);
            s = 0.0;
            if (!ti && !tj) {
                s = ps_v_raw(L1, L2, tmp, i, j);
                if (di) s += ps_v_raw(L1, L2, tmp, i + 12, j);
                if (dj) s += ps_v_raw(L1, L2, tmp, i, j + 12);
                if (di && dj) s += ps_v_raw(L1, L2, tmp, i + 12, j + 12);
            }
        } else {
            const int j = e - PsLin::Gc;
            const bool tied = same && (j == kPsCam2 || j == kPsCam2 + 1), dup = same && (j == kPsCam1 || j == kPsCam1 + 1);
            s = tied ? 0.0 : ps_g_raw(L1, L2, tmp, j);
            if (dup) s += ps_g_raw(L1, L2, tmp, j + 12);
        }
        L[e] = s;
    }
    pnp_wave_sync();
}

// U^ [Y z] = [W g_pose] and the view's contribution: pc_eliminate, 30 wide.  L [PsLin::N], Yz [kPsYzN] and
// ctr [PsCtr::N] in LDS.
MCC_PNP_FN bool ps_eliminate(const double* L, double lambda, int lane, double* Yz, double* ctr) {
    bool ok = true;
    for (int c0 = 0; c0 <= kPsG; c0 += MCC_PNP_LANES) {
        const int c = c0 + lane <= kPsG ? c0 + lane : kPsG;   // columns 0..29 of W, 30 = g_pose
        double A[36], b[6];
        {
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) {
                    const double u = L[PsLin::U + k++];
                    A[i * 6 + j] = A[j * 6 + i] = (i == j) ? u * (1.0 + lambda) : u;
                }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) b[k] = c < kPsG ? L[PsLin::W + k * kPsG + c] : L[PsLin::Gp + k];
        ok = pnp_solve6(A, b) && ok;
        if (c0 + lane <= kPsG) {
#pragma unroll
            for (int k = 0; k < 6; ++k) Yz[c < kPsG ? k * kPsG + c : 6 * kPsG + k] = b[k];
        }
    }
    pnp_wave_sync();
    for (int e = lane; e < PsCtr::N; e += MCC_PNP_LANES) {
        double s;
        if (e < PsCtr::Rc) {
            int i, j;
            ps_unpack(e, kPsG, i, j);
            s = L[PsLin::V + e];
#pragma unroll
            for (int k = 0; k < 6; ++k) s -= L[PsLin::W + k * kPsG + i] * Yz[k * kPsG + j];
        } else if (e < PsCtr::Dg) {
            const int j = e - PsCtr::Rc;
            s = L[PsLin::Gc + j];
#pragma unroll
            for (int k = 0; k < 6; ++k) s -= L[PsLin::W + k * kPsG + j] * Yz[6 * kPsG + k];
        } else if (e < PsCtr::Bad) {
            const int j = e - PsCtr::Dg;
            s = L[PsLin::V + pc_up(j, j, kPsG)];
        } else {
            s = ok ? 0.0 : 1.0;
        }
        ctr[e] = s;
    }
    pnp_wave_sync();
    return ok;
}

// (S + lambda diag V) dc = rhs on the summed contributions tot [PsCtr::N]; tot, M [900], b [30] and dc [30]
// in LDS.  The symmetric elimination of pc_reduced_solve (upper triangle, no pivoting: the pivots are those of
// a Cholesky factorisation), which at 30 x 30 no longer fits a lane's registers: lane i owns row i of M, a
// step is one pass over the rows below the pivot's, and lane 0 back-substitutes.  A fixed slot is the identity
// row with a zero right side, so its dc is exactly 0.  False (on every lane) when a view's block failed or a
// pivot here is not positive.
MCC_PNP_FN bool ps_reduced_solve(const double* tot, double lambda, int mask, int lane, double* M, double* b,
                                 double* dc) {
    bool ok = !(tot[PsCtr::Bad] > 0.0);
    for (int e = lane; e < kPsG * kPsG; e += MCC_PNP_LANES) {
        const int i = e / kPsG, j = e % kPsG;
        const bool fi = (mask >> i) & 1, fj = (mask >> j) & 1;
        double s = tot[PsCtr::S + (i <= j ? pc_up(i, j, kPsG) : pc_up(j, i, kPsG))];
        if (i == j) s = fi ? s + lambda * tot[PsCtr::Dg + i] : 1.0;
        else s = (fi && fj) ? s : 0.0;
        M[e] = s;
    }
    for (int i = lane; i < kPsG; i += MCC_PNP_LANES) b[i] = ((mask >> i) & 1) ? tot[PsCtr::Rc + i] : 0.0;
    pnp_wave_sync();
    for (int k = 0; k < kPsG; ++k) {
        const double piv = pnp_uniform(M[k * kPsG + k]);
        ok = ok && (piv > 1e-300);
        const double ip = 1.0 / piv;
        const double bk = b[k];
        for (int i = k + 1 + lane; i < kPsG; i += MCC_PNP_LANES) {
            const double f = M[k * kPsG + i] * ip;
            for (int j = i; j < kPsG; ++j) M[i * kPsG + j] -= f * M[k * kPsG + j];
            b[i] -= f * bk;
        }
        pnp_wave_sync();
    }
    if (lane == 0) {
        for (int i = kPsG - 1; i >= 0; --i) {
            double s = b[i];
            for (int j = i + 1; j < kPsG; ++j) s -= M[i * kPsG + j] * dc[j];
            dc[i] = ((mask >> i) & 1) ? s / M[i * kPsG + i] : 0.0;
        }
    }
    pnp_wave_sync();
    return ok;
}

// the 30 slots after the step dc (0 at fixed slots), the ties applied: camera 2's fx, fy follow camera 1's
// under SAME_FOCAL_LENGTH, and a camera's fx its own fy where its aspect > 0
MCC_PNP_FN void ps_apply(const double* g, const double* dc, double aspect1, double aspect2, int same, double* gn) {
#pragma unroll
    for (int k = 0; k < kPsG; ++k) gn[k] = g[k] + dc[k];
    if (same) {
        gn[kPsCam2] = gn[kPsCam1];
        gn[kPsCam2 + 1] = gn[kPsCam1 + 1];
    }
    if (aspect1 > 0.0) gn[kPsCam1] = aspect1 * gn[kPsCam1 + 1];
    if (aspect2 > 0.0) gn[kPsCam2] = aspect2 * gn[kPsCam2 + 1];
}

// the view's trial pose: (r, t) + z_v - Y_v dc  (Yz as ps_eliminate left it)
MCC_PNP_FN void ps_trial_pose(const double* r, const double* t, const double* Yz, const double* dc, double* rn,
                              double* tn) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double s = Yz[6 * kPsG + k];
#pragma unroll
        for (int j = 0; j < kPsG; ++j) s -= Yz[k * kPsG + j] * dc[j];
        if (k < 3) rn[k] = r[k] + s;
        else tn[k - 3] = t[k - 3] + s;
    }
}

// sum of squared residuals of one camera's points of the view at (cam, R, t), pnp_residual's rounding
MCC_PNP_FN double ps_sumsq(const PnpCam& c, const double* R, const double* t, const double* obj, const double* img,
                           int n, int lane) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int i = lane; i < n; i += MCC_PNP_LANES) {
        const double X[3] = {obj[3 * i], obj[3 * i + 1], obj[3 * i + 2]};
        double eu, ev;
        pnp_residual(c, R, t, X, img[2 * i], img[2 * i + 1], eu, ev);
        s += eu * eu + ev * ev;
    }
    return pnp_wave_sum(s);
}

// both cameras' squared error of the view at the 30 slots g and the view's pose (r, t)
MCC_PNP_FN void ps_view_sumsq(const double* g, const double* r, const double* t, const double* obj, const double* img1,
                              const double* img2, int n, int lane, double& sq1, double& sq2) {
    Rot rv, ro;
    rodrigues_v2m(r, rv);
    rodrigues_v2m(g, ro);
    double R2[9], t2[3];
    ps_compose(ro.R, g + 3, rv.R, t, R2, t2);
    sq1 = ps_sumsq(pc_cam(g + kPsCam1), rv.R, t, obj, img1, n, lane);
    sq2 = ps_sumsq(pc_cam(g + kPsCam2), R2, t2, obj, img2, n, lane);
}

}  // namespace mcc
