// pincalib_step.cpp -- one Levenberg-Marquardt trial of the pinhole calibrateCamera on the CPU with one lane
// (tests/test_pincalib_step_cpu.py), on a case read from a file: what k_pc_lin and k_pc_try run for every
// view (csrc/mcc_pincalib_device.hpp), with the contributions summed in view order as the tickets sum them.
// tests/cpp/test_pincalib_replay.cpp runs the same sequence on its own exact data and asks whether the loop
// converges; this program hands one trial's parameters out, so that the test can compare the step itself
// with tests/npcalib.py's lm_step.
//
//   pincalib_step IN OUT
//   IN   n_views mask aspect lambda seed_iters
//        off [n_views + 1], g [12], poses [n_views][6], obj [corners][3], img [corners][2]   (text, %.17g)
//        seed_iters > 0: the poses are replaced by pnp_solve_view's (max_iter = seed_iters) at g, as
//        mcc_calibrate_camera seeds them
//   OUT  ok                    1 when every view's block and the reduced system factorised
//        err                   pc_sumsq summed over the views at the start
//        en                    ... at the trial parameters
//        g [12]                the trial's globals (pc_apply)
//        start poses, trial poses [n_views][6] each (pc_trial_pose)
//        the trial's pc_sumsq per view [n_views]
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
#include "mcc_pincalib_device.hpp"

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
    if (argc != 3) {
        std::fprintf(stderr, "usage: pincalib_step IN OUT\n");
        return 2;
    }
    FILE* in = std::fopen(argv[1], "r");
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    int n_views = 0, mask = 0, seed_iters = 0;
    double aspect = 0, lambda = 0;
    if (std::fscanf(in, "%d %d %lf %lf %d", &n_views, &mask, &aspect, &lambda, &seed_iters) != 5 || n_views < 1) {
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
    std::vector<double> g, x, obj, img;
    if (!read(in, g, 12) || !read(in, x, 6 * (size_t)n_views) || !read(in, obj, 3 * corners) || !read(in, img, 2 * corners)) {
        std::fprintf(stderr, "short file\n");
        return 2;
    }
    std::fclose(in);
    const mcc::PnpCam cam = mcc::pc_cam(g.data());

    if (seed_iters > 0)
        for (int v = 0; v < n_views; ++v) {
            const int n = off[v + 1] - off[v];
            std::vector<double> xy(2 * (size_t)n + 2);
            double A[144], V[144], rms;
            if (mcc::pnp_solve_view(&obj[3 * (size_t)off[v]], &img[2 * (size_t)off[v]], n, cam, seed_iters, xy.data(), A, V, 0,
                                    &x[6 * v], &x[6 * v + 3], rms) != mcc::kPnpSolved) {
                std::fprintf(stderr, "no pose seed for view %d\n", v);
                return 3;
            }
        }

    double err = 0.0;
    for (int v = 0; v < n_views; ++v)
        err += mcc::pc_sumsq(cam, &x[6 * v], &x[6 * v + 3], &obj[3 * (size_t)off[v]], &img[2 * (size_t)off[v]],
                             off[v + 1] - off[v], 0);

    std::vector<double> L(mcc::PcLin::N), Yz((size_t)n_views * 78), ctr(mcc::PcCtr::N), tot(mcc::PcCtr::N, 0.0);
    for (int v = 0; v < n_views; ++v) {
        mcc::pc_linearize(&obj[3 * (size_t)off[v]], &img[2 * (size_t)off[v]], off[v + 1] - off[v], cam, mask, aspect, &x[6 * v],
                          &x[6 * v + 3], 0, L.data());
        mcc::pc_eliminate(L.data(), lambda, 0, &Yz[(size_t)v * 78], ctr.data());
        for (int e = 0; e < mcc::PcCtr::N; ++e) tot[e] += ctr[e];
    }
    double dc[12], gn[12];
    const bool ok = mcc::pc_reduced_solve(tot.data(), lambda, mask, dc);
    mcc::pc_apply(g.data(), dc, aspect, gn);
    std::vector<double> xn(x.size()), sq((size_t)n_views);
    double en = 0.0;
    for (int v = 0; v < n_views; ++v) {
        mcc::pc_trial_pose(&x[6 * v], &x[6 * v + 3], &Yz[(size_t)v * 78], dc, &xn[6 * v], &xn[6 * v + 3]);
        sq[v] = mcc::pc_sumsq(mcc::pc_cam(gn), &xn[6 * v], &xn[6 * v + 3], &obj[3 * (size_t)off[v]], &img[2 * (size_t)off[v]],
                              off[v + 1] - off[v], 0);
        en += sq[v];
    }

    FILE* out = std::fopen(argv[2], "w");
    if (!out) {
        std::fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    std::fprintf(out, "%d\n", ok ? 1 : 0);
    write(out, &err, 1);
    write(out, &en, 1);
    write(out, gn, 12);
    write(out, x.data(), x.size());
    write(out, xn.data(), xn.size());
    write(out, sq.data(), sq.size());
    return std::fclose(out) ? 2 : 0;
}
