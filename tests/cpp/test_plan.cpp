// test_plan.cpp -- prints what the host-only step planner (csrc/mcc_plan.cpp) makes of a problem.
// Compiled by tests/test_plan.py with g++ and mcc_plan.cpp alone: no ROCm headers, no libmcc.so.
//
//   test_plan <blob> <n_cu> <n_cu_dev> <scalars|full> [MCC_NAME=value ...]
//
// The blob is tests/test_cpp_host.py::_write_blob's (see tests/cpp/test_multicalib.cpp).  Output, one
// record per line: "validate <rc> <message>", "plan <rc> <message>", then "<name> <count> <values...>"
// for every scalar of the plan and, with "full", every array (Int4 arrays as 4 ints per element).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../multi_camera_calibration_amd/csrc/mcc_plan.hpp"

namespace {

std::map<std::string, std::string> g_env;   // the switches given on the command line

template <class T>
std::vector<T> rd(std::ifstream& f, long long n) {
    if (n < 0) n = 0;
    std::vector<T> v((size_t)n);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    if (!f) throw std::runtime_error("truncated input");
    return v;
}

void put1(const char* name, long long v) { std::printf("%s 1 %lld\n", name, v); }

template <class T>
void put(const char* name, const std::vector<T>& v) {
    std::printf("%s %zu", name, v.size());
    for (const T& x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}
void put(const char* name, const std::vector<float>& v) {
    std::printf("%s %zu", name, v.size());
    for (float x : v) std::printf(" %.9g", (double)x);
    std::printf("\n");
}
void put(const char* name, const std::vector<double>& v) {
    std::printf("%s %zu", name, v.size());
    for (double x : v) std::printf(" %.17g", x);
    std::printf("\n");
}
void put(const char* name, const std::vector<mcc::Int4>& v) {
    std::printf("%s %zu", name, 4 * v.size());
    for (const mcc::Int4& x : v) std::printf(" %d %d %d %d", x.x, x.y, x.z, x.w);
    std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: test_plan <blob> <n_cu> <n_cu_dev> <scalars|full> [MCC_NAME=value ...]\n");
        return 2;
    }
    try {
        std::ifstream f(argv[1], std::ios::binary);
        if (!f) throw std::runtime_error("cannot open input");
        const int n_cu = std::atoi(argv[2]), n_cu_dev = std::atoi(argv[3]);
        const bool full = std::strcmp(argv[4], "full") == 0;
        for (int i = 5; i < argc; ++i) {
            const char* eq = std::strchr(argv[i], '=');
            if (!eq) throw std::runtime_error("switches are NAME=value");
            g_env[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
        }
        const auto h = rd<int>(f, 11);
        if (h[0] != 0x4d434331) throw std::runtime_error("bad magic");
        const int model = h[1], C = h[2], V = h[3], E = h[4], nd = h[5], corners = h[6];
        const bool has_ds = h[7] != 0, has_cp = h[8] != 0;
        (void)rd<double>(f, 1);
        const auto ecam = rd<int>(f, E), ephoto = rd<int>(f, E), eside = rd<int>(f, E), eoff = rd<int>(f, E), en = rd<int>(f, E);
        const auto obj = rd<float>(f, 3LL * corners), img = rd<float>(f, 2LL * corners);
        const auto K = rd<float>(f, 9LL * C), D = rd<float>(f, (long long)nd * C), xi = rd<float>(f, C);
        std::vector<double> dsp;
        std::vector<float> cp;
        if (has_ds) dsp = rd<double>(f, 16);
        if (has_cp) cp = rd<float>(f, 16LL * C);

        mcc_desc d{};
        d.model = model; d.n_cams = C; d.n_photos = V; d.n_edges = E;
        d.edge_cam = ecam.data(); d.edge_photo = ephoto.data(); d.edge_side = eside.data();
        d.edge_off = eoff.data(); d.edge_n = en.data();
        d.obj = obj.data(); d.img = img.data();
        d.nd = nd; d.K = K.data(); d.D = D.data();
        d.xi = model == MCC_MODEL_OMNI ? xi.data() : nullptr;
        d.ds_pose = has_ds ? dsp.data() : nullptr;
        d.cam_pose = has_cp ? cp.data() : nullptr;

        const mcc::Options opt = mcc::Options::from_env([](const char* name) -> const char* {
            auto it = g_env.find(name);
            return it == g_env.end() ? nullptr : it->second.c_str();
        });
        std::string why;
        int rc = mcc::validate(d, &why);
        std::printf("validate %d %s\n", rc, why.c_str());
        if (rc) return 0;
        mcc::Plan p;
        why.clear();
        rc = mcc::plan_problem(d, opt, n_cu, n_cu_dev, &p, &why);
        std::printf("plan %d %s\n", rc, why.c_str());
        if (rc) return 0;

#define S(field) put1(#field, (long long)p.field)
        S(model); S(C); S(V); S(E); S(nd); S(m); S(P); S(corners); S(rational); S(prism); S(has_back);
        S(max_epp); S(max_cpp); S(nblk); S(n_items); S(n_pairs); S(n_pair_doubles); S(n_norm_chunks);
        S(n_pgroups); S(max_gpairs); S(max_gcon); S(max_gedges); S(max_item_slots); S(photo_shmem); S(group_shmem);
        S(group_size); S(n_groups); S(n_prep); S(ntri); S(packed_len); S(prev_stride);
        S(fused); S(use_group); S(group_cap); S(group_lanes); S(prep_lanes); S(schur_one_level); S(small_warm);
        S(gfold); S(fold_direct); S(fold_dyn); S(fold_first); S(warm); S(helper_refine); S(helper_early); S(inv_la);
        S(poison); S(poison_level); S(peer_push); S(warm_poison); S(small_stats); S(fault_photo); S(use_graph); S(graph_sizes);
        S(warm_wait_ticks); S(warm_idle_ticks); S(warm_delay_ticks); S(spare_delay_ticks); S(peer_timeout);
#undef S
        if (!full) return 0;
#define A(field) put(#field, p.field)
        A(obj_x); A(obj_y); A(obj_z); A(img_u); A(img_v); A(info); A(gblock); A(ephoto); A(photo_ptr); A(photo_corner);
        A(pgrp_ptr); A(pgrp_edge); A(edge_lphoto); A(ghdr); A(kintr); A(tilt); A(gpair_ptr); A(gpairs); A(gcon_ptr); A(gcon);
        A(items); A(block_items); A(prep_ptr); A(prep_edge); A(cam_rt); A(ds_rt); A(alpha);
        A(dev2ref_edge); A(dev2ref_corner); A(edge_n_dev);
#undef A
    } catch (const std::exception& e) {
        std::fprintf(stderr, "test_plan: %s\n", e.what());
        return 1;
    }
    return 0;
}
