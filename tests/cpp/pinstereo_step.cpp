// pinstereo_step.cpp -- one Levenberg-Marquardt trial of the pinhole stereoCalibrate on the CPU with one lane
// (tests/test_pinstereo_step_cpu.py), on a case read from a file: what k_ps_lin and k_ps_try run for every
// view (csrc/mcc_pinstereo_device.hpp), with the contributions summed in view order as the tickets sum them.
// The program hands one trial's parameters out, so that the test can compare the step itself with
// tests/npstereocalib.py's lm_step.
//
//   pinstereo_step IN OUT
//   IN   n_views mask same aspect1 aspect2 lambda seed_iters
//        off [n_views + 1], g [30], poses [n_views][6], obj [corners][3], img1 [corners][2], img2 [corners][2]
//        (text, %.17g).  seed_iters > 0: the poses are replaced by pnp_solve_view's (max_iter = seed_iters) of
//        camera 1 at g, as mcc_stereo_calibrate seeds them under a guess
//   OUT  ok                    1 when every view's block and the reduced system factorised
//        err                   the squared error summed over the views and cameras at the start
//        en                    ... at the trial parameters
//        g [30]                the trial's globals (ps_apply)
//        start poses, trial poses [n_views][6] each (ps_trial_pose)
//        the trial's squared error per view and camera [n_views][2]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#define MCC_PNP_LANES 1
#define MCC_PNP_FN inline
namespace mcc {
inline void pnp_wave_sync() {}
inline double pnp_uniform(double v) { return v; }
inline int pnp_uniform(int v) { return v; }
inline double pnp_wave_sum(double v) { return v; }
}  // namespace mcc
#include "mcc_pinstereo_device.hpp"

namespace {

bool read(FILE* f, std::vector<double>& a, size_t n) {
    a.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (std::fscanf(f, "%lf", &a[i]) != 1) return false;
    return true;
}

void write(FILE* f, const double* a, size_t n) {
    for (size_t i = 0; i < n; ++i) std::fprintf(f, "%.17g%c", a[i], i + 1 == n ? '\n' : ' ');
}

}  // namespace

int main(int argc, char** argv) {
    using namespace mcc;
    if (argc != 3) {
        std::fprintf(stderr, "usage: pinstereo_step IN OUT\n");
        return 2;
    }
    FILE* in = std::fopen(argv[1], "r");
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    int n_views = 0, mask = 0, same = 0, seed_iters = 0;
    double aspect1 = 0, aspect2 = 0, lambda = 0;
    if (std::fscanf(in, "%d %d %d %lf %lf %lf %d", &n_views, &mask, &same, &aspect1, &aspect2, &lambda, &seed_iters) != 7 ||
        n_views < 1) {
        std::fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<int> off((size_t)n_views + 1);
    for (int& o : off)
        if (std::fscanf(in, "%d", &o) != 1) return 2;
    if (off[0] != 0) return 2;
    for (int v = 0; v < n_views; ++v)
        if (off[v + 1] - off[v] < 4) return 2;
    const size_t corners = (size_t)off[n_views];
    std::vector<double> g, x, obj, img1, img2;
    if (!read(in, g, kPsG) || !read(in, x, 6 * (size_t)n_views) || !read(in, obj, 3 * corners) || !read(in, img1, 2 * corners) ||
        !read(in, img2, 2 * corners)) {
        std::fprintf(stderr, "short file\n");
        return 2;
    }
    std::fclose(in);

    if (seed_iters > 0)
        for (int v = 0; v < n_views; ++v) {
            const int n = off[v + 1] - off[v];
            std::vector<double> xy(2 * (size_t)n + 2);
            double A[144], V[144], rms;
            if (pnp_solve_view(&obj[3 * (size_t)off[v]], &img1[2 * (size_t)off[v]], n, pc_cam(&g[kPsCam1]), seed_iters, xy.data(),
                               A, V, 0, &x[6 * v], &x[6 * v + 3], rms) != kPnpSolved) {
                std::fprintf(stderr, "no pose seed for view %d\n", v);
                return 3;
            }
        }

    double err = 0.0;
    for (int v = 0; v < n_views; ++v) {
        double s1, s2;
        ps_view_sumsq(g.data(), &x[6 * v], &x[6 * v + 3], &obj[3 * (size_t)off[v]], &img1[2 * (size_t)off[v]],
                      &img2[2 * (size_t)off[v]], off[v + 1] - off[v], 0, s1, s2);
        err += s1;
        err += s2;
    }

    std::vector<double> L(PsLin::N), L12(2 * PcLin::N), tmp(PsTmp::N), Yz((size_t)n_views * kPsYzN), ctr(PsCtr::N),
        tot(PsCtr::N, 0.0);
    const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    Rot ro;
    rodrigues_v2m(g.data(), ro);
    double Jo[9];
    so3_jac(g.data(), ro, +1.0, Jo);
    for (int v = 0; v < n_views; ++v) {
        const int n = off[v + 1] - off[v];
        const double *r = &x[6 * v], *t = &x[6 * v + 3], *X = &obj[3 * (size_t)off[v]];
        Rot rv;
        rodrigues_v2m(r, rv);
        double Jv[9], R2[9], t2[3];
        so3_jac(r, rv, +1.0, Jv);
        ps_compose(ro.R, &g[3], rv.R, t, R2, t2);
        ps_maps(ro.R, Jo, Jv, t, 0, tmp.data());
        pc_linearize_rj(X, &img1[2 * (size_t)off[v]], n, pc_cam(&g[kPsCam1]), ps_lin_mask(mask, same, 0), aspect1, rv.R, Jv, t, 0,
                        L12.data());
        pc_linearize_rj(X, &img2[2 * (size_t)off[v]], n, pc_cam(&g[kPsCam2]), ps_lin_mask(mask, same, 1), aspect2, R2, I3, t2, 0,
                        L12.data() + PcLin::N);
        ps_assemble(L12.data(), L12.data() + PcLin::N, tmp.data(), same, 0, L.data());
        ps_eliminate(L.data(), lambda, 0, &Yz[(size_t)v * kPsYzN], ctr.data());
        for (int e = 0; e < PsCtr::N; ++e) tot[e] += ctr[e];
    }
    double M[kPsG * kPsG], b[kPsG], dc[kPsG], gn[kPsG];
    const bool ok = ps_reduced_solve(tot.data(), lambda, mask, 0, M, b, dc);
    ps_apply(g.data(), dc, aspect1, aspect2, same, gn);
    std::vector<double> xn(x.size()), sq(2 * (size_t)n_views);
    double en = 0.0;
    for (int v = 0; v < n_views; ++v) {
        ps_trial_pose(&x[6 * v], &x[6 * v + 3], &Yz[(size_t)v * kPsYzN], dc, &xn[6 * v], &xn[6 * v + 3]);
        ps_view_sumsq(gn, &xn[6 * v], &xn[6 * v + 3], &obj[3 * (size_t)off[v]], &img1[2 * (size_t)off[v]],
                      &img2[2 * (size_t)off[v]], off[v + 1] - off[v], 0, sq[2 * v], sq[2 * v + 1]);
        en += sq[2 * v];
        en += sq[2 * v + 1];
    }

    FILE* out = std::fopen(argv[2], "w");
    if (!out) {
        std::fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    std::fprintf(out, "%d\n", ok ? 1 : 0);
    write(out, &err, 1);
    write(out, &en, 1);
    write(out, gn, kPsG);
    write(out, x.data(), x.size());
    write(out, xn.data(), xn.size());
    write(out, sq.data(), sq.size());
    return std::fclose(out) ? 2 : 0;
}
