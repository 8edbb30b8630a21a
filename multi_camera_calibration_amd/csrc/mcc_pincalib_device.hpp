// mcc_pincalib_device.hpp -- one view of the pinhole calibrateCamera's Levenberg-Marquardt trial, as
// one wave64 runs it (k_pc_lin, k_pc_try: mcc_pincalib.hip).  Like mcc_pnp_device.hpp, whose camera
// model, rows, wave sums and 6 x 6 solve it uses, it compiles for the host with one lane
// (MCC_PNP_LANES 1: tests/cpp/test_pincalib_replay.cpp).
//
// The normal matrix is block-arrow: a 6 x 6 pose block U_v per view, one global block V of the
// kPcG = 12 slots fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6, and the 6 x 12 couplings W_v.  A view's part
// of it is 189 sums, more than a lane can keep in registers next to the rows that feed them, so the
// corners are walked three times (pc_linearize): U_v and g_v; W_v; V_v and g_c.  Every pass is a
// lane's strided partial in corner order, then the xor butterfly, and lane 0 leaves the sums in the
// view's LDS record PcLin.  Fixed slots have zero columns (the 0/1 mask); under FIX_ASPECT_RATIO the
// fy column is J_fy + a J_fx and fx is a fixed slot that follows fy.
//
// pc_eliminate damps U_v (diagonal times 1 + lambda), solves U^ [Y_v z_v] = [W_v g_v] with lane j
// taking column j, and packs the view's contribution to the reduced system (PcCtr).  pc_reduced_solve
// runs in the last arriver on the sums over the views; pc_trial_pose is the back-substitution and
// pc_sumsq the error of the trial parameters.
#pragma once
#include "mcc_pnp_device.hpp"

namespace mcc {

constexpr int kPcG = 12;

// a view's linearisation, undamped (LDS, and global between a rejected trial and the next)
struct PcLin {
    static constexpr int U = 0;                 // [21] upper triangle, row-major
    static constexpr int Gp = 21;               // [6]  J_pose^T e
    static constexpr int W = 27;                // [6][12]
    static constexpr int V = 99;                // [78] upper triangle, row-major
    static constexpr int Gc = 177;              // [12] J_glob^T e
    static constexpr int N = 189;
};

// a view's packed contribution to the reduced system (and the groups' and the total's sums)
struct PcCtr {
    static constexpr int S = 0;                 // [78] V_v - W_v^T Y_v, upper triangle
    static constexpr int Rc = 78;               // [12] g_c,v - W_v^T z_v
    static constexpr int Dg = 90;               // [12] diag V_v (the damping of the global block)
    static constexpr int Bad = 102;             //      1 where U^_v had a pivot that is not positive
    static constexpr int N = 103;
};

// packed upper-triangle index of (i, j), i <= j, of a G x G matrix
MCC_PNP_FN int pc_up(int i, int j, int G) { return i * G - (i * (i - 1)) / 2 + (j - i); }

MCC_PNP_FN PnpCam pc_cam(const double* g) {
    return PnpCam{g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11], 0.0, 0.0, 0.0, 0.0};
}

// the global slots after the step dc (0 at fixed slots); aspect > 0: fx = aspect fy
MCC_PNP_FN void pc_apply(const double* g, const double* dc, double aspect, double* gn) {
#pragma unroll
    for (int k = 0; k < kPcG; ++k) gn[k] = g[k] + dc[k];
    if (aspect > 0.0) gn[0] = aspect * gn[1];
}

// the global rows of one corner as the solver sees them: aspect coupling, then the mask
MCC_PNP_FN void pc_glob_rows(const PnpCam& c, const double* R, const double* t, const double* X, int mask,
                             double aspect, double* iu, double* iv) {
    pnp_rows_intr(c, R, t, X, iu, iv);
    iu[1] += aspect * iu[0];
    iv[1] += aspect * iv[0];
#pragma unroll
    for (int k = 0; k < kPcG; ++k) {
        const bool fr = (mask >> k) & 1;
        iu[k] = fr ? iu[k] : 0.0;
        iv[k] = fr ? iv[k] : 0.0;
    }
}

// the view's 189 sums at (cam, r, t) into L (LDS); the caller synchronises
MCC_PNP_FN void pc_linearize(const double* obj, const double* img, int n, const PnpCam& cam, int mask, double aspect,
                             const double* r, const double* t, int lane, double* L) {
    Rot rot;
    rodrigues_v2m(r, rot);
    double Jl[9];
    so3_jac(r, rot, +1.0, Jl);
    {   // pass 1: U and g_pose
        double H[21], g[6];
#pragma unroll
        for (int k = 0; k < 21; ++k) H[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = 0.0;
        for (int i = lane; i < n; i += MCC_PNP_LANES) {
            const double X[3] = {obj[3 * i], obj[3 * i + 1], obj[3 * i + 2]};
            double ju[6], jv[6], eu, ev;
            pnp_rows(cam, rot.R, Jl, t, X, img[2 * i], img[2 * i + 1], ju, jv, eu, ev);
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                g[a] += ju[a] * eu + jv[a] * ev;
#pragma unroll
                for (int b = a; b < 6; ++b) H[k++] += ju[a] * ju[b] + jv[a] * jv[b];
            }
        }
#pragma unroll
        for (int k = 0; k < 21; ++k) {
            const double s = pnp_wave_sum(H[k]);
            if (lane == 0) L[PcLin::U + k] = s;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double s = pnp_wave_sum(g[k]);
            if (lane == 0) L[PcLin::Gp + k] = s;
        }
    }
    {   // pass 2: W
        double W[72];
#pragma unroll
        for (int k = 0; k < 72; ++k) W[k] = 0.0;
        for (int i = lane; i < n; i += MCC_PNP_LANES) {
            const double X[3] = {obj[3 * i], obj[3 * i + 1], obj[3 * i + 2]};
            double ju[6], jv[6], iu[kPcG], iv[kPcG], eu, ev;
            pnp_rows(cam, rot.R, Jl, t, X, img[2 * i], img[2 * i + 1], ju, jv, eu, ev);
            pc_glob_rows(cam, rot.R, t, X, mask, aspect, iu, iv);
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int j = 0; j < kPcG; ++j) W[a * kPcG + j] += ju[a] * iu[j] + jv[a] * iv[j];
        }
#pragma unroll
        for (int k = 0; k < 72; ++k) {
            const double s = pnp_wave_sum(W[k]);
            if (lane == 0) L[PcLin::W + k] = s;
        }
    }
    {   // pass 3: V and g_glob
        double V[78], g[kPcG];
#pragma unroll
        for (int k = 0; k < 78; ++k) V[k] = 0.0;
#pragma unroll
        for (int k = 0; k < kPcG; ++k) g[k] = 0.0;
        for (int i = lane; i < n; i += MCC_PNP_LANES) {
            const double X[3] = {obj[3 * i], obj[3 * i + 1], obj[3 * i + 2]};
            double ju[6], jv[6], iu[kPcG], iv[kPcG], eu, ev;
            pnp_rows(cam, rot.R, Jl, t, X, img[2 * i], img[2 * i + 1], ju, jv, eu, ev);
            pc_glob_rows(cam, rot.R, t, X, mask, aspect, iu, iv);
            int k = 0;
#pragma unroll
            for (int a = 0; a < kPcG; ++a) {
                g[a] += iu[a] * eu + iv[a] * ev;
#pragma unroll
                for (int b = a; b < kPcG; ++b) V[k++] += iu[a] * iu[b] + iv[a] * iv[b];
            }
        }
#pragma unroll
        for (int k = 0; k < 78; ++k) {
            const double s = pnp_wave_sum(V[k]);
            if (lane == 0) L[PcLin::V + k] = s;
        }
#pragma unroll
        for (int k = 0; k < kPcG; ++k) {
            const double s = pnp_wave_sum(g[k]);
            if (lane == 0) L[PcLin::Gc + k] = s;
        }
    }
}

// pc_linearize's three passes at (cam, R, t) with the rotation columns of the pose rows taken through Jl:
// the identity gives rows in the left tangent of R, which is what a pose that is a product needs
// (mcc_pinstereo_device.hpp's second camera).  pc_linearize itself stays as it is, so that its results do.
MCC_PNP_FN void pc_linearize_rj(const double* obj, const double* img, int n, const PnpCam& cam, int mask, double aspect,
                                const double* R, const double* Jl, const double* t, int lane, double* L) {
    {   // pass 1: U and g_pose
        double H[21], g[6];
#pragma unroll
        for (int k = 0; k < 21; ++k) H[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) g[k] = 0.0;
        for (int i = lane; i < n; i += MCC_PNP_LANES) {
            const double X[3] = {obj[3 * i], obj[3 * i + 1], obj[3 * i + 2]};
            double ju[6], jv[6], eu, ev;
            pnp_rows(cam, R, Jl, t, X, img[2 * i], img[2 * i + 1], ju, jv, eu, ev);
            int k = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                g[a] += ju[a] * eu + jv[a] * ev;
#pragma unroll
                for (int b = a; b < 6; ++b) H[k++] += ju[a] * ju[b] + jv[a] * jv[b];
            }
        }
#pragma unroll
        for (int k = 0; k < 21; ++k) {
            const double s = pnp_wave_sum(H[k]);
            if (lane == 0) L[PcLin::U + k] = s;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const double s = pnp_wave_sum(g[k]);
            if (lane == 0) L[PcLin::Gp + k] = s;
        }
    }
    {   // pass 2: W
        double W[72];
#pragma unroll
        for (int k = 0; k < 72; ++k) W[k] = 0.0;
        for (int i = lane; i < n; i += MCC_PNP_LANES) {
            const double X[3] = {obj[3 * i], obj[3 * i + 1], obj[3 * i + 2]};
            double ju[6], jv[6], iu[kPcG], iv[kPcG], eu, ev;
            pnp_rows(cam, R, Jl, t, X, img[2 * i], img[2 * i + 1], ju, jv, eu, ev);
            pc_glob_rows(cam, R, t, X, mask, aspect, iu, iv);
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int j = 0; j < kPcG; ++j) W[a * kPcG + j] += ju[a] * iu[j] + jv[a] * iv[j];
        }
#pragma unroll
        for (int k = 0; k < 72; ++k) {
            const double s = pnp_wave_sum(W[k]);
            if (lane == 0) L[PcLin::W + k] = s;
        }
    }
    {   // pass 3: V and g_glob
        double V[78], g[kPcG];
#pragma unroll
        for (int k = 0; k < 78; ++k) V[k] = 0.0;
#pragma unroll
        for (int k = 0; k < kPcG; ++k) g[k] = 0.0;
        for (int i = lane; i < n; i += MCC_PNP_LANES) {
            const double X[3] = {obj[3 * i], obj[3 * i + 1], obj[3 * i + 2]};
            double ju[6], jv[6], iu[kPcG], iv[kPcG], eu, ev;
            pnp_rows(cam, R, Jl, t, X, img[2 * i], img[2 * i + 1], ju, jv, eu, ev);
            pc_glob_rows(cam, R, t, X, mask, aspect, iu, iv);
            int k = 0;
#pragma unroll
            for (int a = 0; a < kPcG; ++a) {
                g[a] += iu[a] * eu + iv[a] * ev;
#pragma unroll
                for (int b = a; b < kPcG; ++b) V[k++] += iu[a] * iu[b] + iv[a] * iv[b];
            }
        }
#pragma unroll
        for (int k = 0; k < 78; ++k) {
            const double s = pnp_wave_sum(V[k]);
            if (lane == 0) L[PcLin::V + k] = s;
        }
#pragma unroll
        for (int k = 0; k < kPcG; ++k) {
            const double s = pnp_wave_sum(g[k]);
            if (lane == 0) L[PcLin::Gc + k] = s;
        }
    }
}

// U^ [Y z] = [W g_pose] and the view's contribution.  L [PcLin::N], Yz [78] (Y [6][12], then z [6]) and
// ctr [PcCtr::N] in LDS.  False (on every lane) when a pivot of U^ is not positive; the outputs are
// then meaningless but written, so the reduction's tickets still complete.
MCC_PNP_FN bool pc_eliminate(const double* L, double lambda, int lane, double* Yz, double* ctr) {
    bool ok = true;
    for (int c0 = 0; c0 <= kPcG; c0 += MCC_PNP_LANES) {
        const int c = c0 + lane <= kPcG ? c0 + lane : kPcG;   // columns 0..11 of W, 12 = g_pose
        double A[36], b[6];
        {
            int k = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) {
                    const double u = L[PcLin::U + k++];
                    A[i * 6 + j] = A[j * 6 + i] = (i == j) ? u * (1.0 + lambda) : u;
                }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) b[k] = c < kPcG ? L[PcLin::W + k * kPcG + c] : L[PcLin::Gp + k];
        ok = pnp_solve6(A, b) && ok;
        if (c0 + lane <= kPcG) {
#pragma unroll
            for (int k = 0; k < 6; ++k) Yz[c < kPcG ? k * kPcG + c : 72 + k] = b[k];
        }
    }
    pnp_wave_sync();
    for (int e = lane; e < PcCtr::N; e += MCC_PNP_LANES) {
        double s;
        if (e < PcCtr::Rc) {
            int i = 0, rem = e;
            while (rem >= kPcG - i) { rem -= kPcG - i; ++i; }
            const int j = i + rem;
            s = L[PcLin::V + e];
#pragma unroll
            for (int k = 0; k < 6; ++k) s -= L[PcLin::W + k * kPcG + i] * Yz[k * kPcG + j];
        } else if (e < PcCtr::Dg) {
            const int j = e - PcCtr::Rc;
            s = L[PcLin::Gc + j];
#pragma unroll
            for (int k = 0; k < 6; ++k) s -= L[PcLin::W + k * kPcG + j] * Yz[72 + k];
        } else if (e < PcCtr::Bad) {
            const int j = e - PcCtr::Dg;
            s = L[PcLin::V + pc_up(j, j, kPcG)];
        } else {
            s = ok ? 0.0 : 1.0;
        }
        ctr[e] = s;
    }
    pnp_wave_sync();
    return ok;
}

// (S + lambda diag V) dc = rhs on the summed contributions tot [PcCtr::N]; every lane the same registers.
// A fixed slot is the identity row with a zero right side, so its dc is exactly 0.  False when a view's
// block failed or a pivot here is not positive.
MCC_PNP_FN bool pc_reduced_solve(const double* tot, double lambda, int mask, double* dc) {
    double S[kPcG * kPcG];
    bool ok = !(tot[PcCtr::Bad] > 0.0);
    {
        int k = 0;
#pragma unroll
        for (int i = 0; i < kPcG; ++i) {
            const bool fi = (mask >> i) & 1;
#pragma unroll
            for (int j = i; j < kPcG; ++j) {
                const bool fj = (mask >> j) & 1;
                double s = tot[PcCtr::S + k++];
                if (i == j) s = fi ? s + lambda * tot[PcCtr::Dg + i] : 1.0;
                else s = (fi && fj) ? s : 0.0;
                S[i * kPcG + j] = s;
            }
            dc[i] = fi ? tot[PcCtr::Rc + i] : 0.0;
        }
    }
    // symmetric elimination on the upper triangle, no pivoting (SPD): the multiplier of row i is S_ki / S_kk
#pragma unroll
    for (int k = 0; k < kPcG; ++k) {
        const double piv = S[k * kPcG + k];
        ok = ok && (piv > 1e-300);
        const double ip = 1.0 / piv;
#pragma unroll
        for (int i = k + 1; i < kPcG; ++i) {
            const double f = S[k * kPcG + i] * ip;
#pragma unroll
            for (int j = i; j < kPcG; ++j) S[i * kPcG + j] -= f * S[k * kPcG + j];
            dc[i] -= f * dc[k];
        }
    }
#pragma unroll
    for (int i = kPcG - 1; i >= 0; --i) {
        double s = dc[i];
#pragma unroll
        for (int j = i + 1; j < kPcG; ++j) s -= S[i * kPcG + j] * dc[j];
        dc[i] = s / S[i * kPcG + i];
    }
    return ok;
}

// sum of squared residuals of the view at (cam, r, t), pnp_residual's rounding
MCC_PNP_FN double pc_sumsq(const PnpCam& c, const double* r, const double* t, const double* obj, const double* img,
                           int n, int lane) {
#pragma clang fp contract(off)
    Rot rot;
    rodrigues_v2m(r, rot);
    double s = 0.0;
    for (int i = lane; i < n; i += MCC_PNP_LANES) {
        const double X[3] = {obj[3 * i], obj[3 * i + 1], obj[3 * i + 2]};
        double eu, ev;
        pnp_residual(c, rot.R, t, X, img[2 * i], img[2 * i + 1], eu, ev);
        s += eu * eu + ev * ev;
    }
    return pnp_wave_sum(s);
}

// the view's trial pose: (r, t) + z_v - Y_v dc  (Yz as pc_eliminate left it)
MCC_PNP_FN void pc_trial_pose(const double* r, const double* t, const double* Yz, const double* dc, double* rn,
                              double* tn) {
    double d[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double s = Yz[72 + k];
#pragma unroll
        for (int j = 0; j < kPcG; ++j) s -= Yz[k * kPcG + j] * dc[j];
        d[k] = s;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        rn[k] = r[k] + d[k];
        tn[k] = t[k] + d[3 + k];
    }
}

}  // namespace mcc
