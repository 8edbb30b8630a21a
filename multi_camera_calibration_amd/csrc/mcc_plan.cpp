// mcc_plan.cpp -- the host-only step planner behind mcc_create (mcc_plan.hpp): options, validation,
// the step-form rules and the index structures, as pure functions of the descriptor and a CU count.
#include "mcc_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <numeric>

namespace mcc {

// ------------------------------------------------------------------------------------------ options

Options Options::from_env(const char* (*get)(const char* name)) {
    Options o;
    auto num = [&](const char* name, int unset) {
        const char* v = get(name);
        return v ? std::atoi(v) : unset;
    };
    auto on = [&](const char* name, bool unset) {
        const char* v = get(name);
        return v ? std::atoi(v) != 0 : unset;
    };
    auto tri = [&](const char* name) {   // -1 unset, else 0 / 1
        const char* v = get(name);
        return v ? (std::atoi(v) != 0 ? 1 : 0) : -1;
    };
    auto ticks = [&](const char* name, double least, double per_unit, long long unset) {
        const char* v = get(name);
        return v ? (long long)(std::max(least, std::atof(v)) * per_unit) : unset;
    };
    if (get("MCC_CUS")) o.cus = std::max(1, num("MCC_CUS", 0));
    o.fused = tri("MCC_FUSED");
    o.group = tri("MCC_GROUP");
    if (get("MCC_GROUP_EDGES")) o.group_edges = std::max(1, std::min(4 * kGroupRound, num("MCC_GROUP_EDGES", 0)));
    o.group_lanes = num("MCC_GROUP_LANES", 32) == 16 ? 16 : 32;
    o.prep_lanes = num("MCC_PREP_LANES", 1) == 4 ? 4 : 1;
    if (get("MCC_ITEM_SLOTS")) o.item_slots = std::max(1, num("MCC_ITEM_SLOTS", 0));
    o.schur_one_level = on("MCC_SCHUR_ONE_LEVEL", true);
    o.small_warm = on("MCC_SMALL_WARM", true);
    o.gfold = on("MCC_GFOLD", true);
    o.fold_direct = on("MCC_FOLD_DIRECT", true);
    o.fold_dyn = tri("MCC_FOLD_DYN");
    o.fold_first = on("MCC_FOLD_CONSUMERS_FIRST", false);
    o.warm = on("MCC_WARM", true);
    o.helper_refine = on("MCC_HELPER_REFINE", true);
    o.helper_poll = tri("MCC_HELPER_POLL");
    o.inv_la = tri("MCC_INV_LA");
    o.use_graph = on("MCC_GRAPH", true);
    if (get("MCC_GRAPH_SIZES")) o.graph_sizes = std::min(kGraphSizes, std::max(1, num("MCC_GRAPH_SIZES", 0)));
    o.peer_push = on("MCC_PEER_PUSH", true);
    o.poison_level = num("MCC_POISON_HANDOFF", 0);
    o.warm_poison = num("MCC_WARM_POISON", 0);
    o.small_stats = on("MCC_SOLVE_STATS", false);
    o.fault_photo = num("MCC_FAULT_PHOTO", -1);
    o.warm_wait_ticks = ticks("MCC_WARM_TIMEOUT_MS", 1.0, 1e5, o.warm_wait_ticks);
    o.warm_delay_ticks = ticks("MCC_WARM_DELAY_US", 0.0, 1e2, 0);
    o.spare_delay_ticks = ticks("MCC_SPARE_DELAY_US", 0.0, 1e2, 0);
    o.peer_timeout_ticks = ticks("MCC_PEER_TIMEOUT_MS", 1.0, 1e5, o.peer_timeout_ticks);
    return o;
}

// --------------------------------------------------------------------------------------- validation

namespace {
int reject(std::string* why, const std::string& msg) {
    if (why) *why = msg;
    return MCC_EINVAL;
}
int global_dim(const mcc_desc& d) { return d.model == MCC_MODEL_DOUBLESIDE ? 6 : 6 * (d.n_cams - 1); }
}  // namespace

int validate(const mcc_desc& d, std::string* why) {
    if (d.model < 0 || d.model > 2) return reject(why, "unknown model");
    if (d.n_cams < 1 || d.n_photos < 0 || d.n_edges < 0) return reject(why, "bad sizes");
    // the reference's meanReProjError is 0 / 0 without observations (src/multicalib.cpp:989), and
    // a photo vertex exists only through an edge (getPhotoVertex, :323-346); a rank of a sharded
    // problem needs photos of its own to take part in the per-step exchange
    if (d.n_photos < 1 || d.n_edges < 1) return reject(why, "no photo vertices / observations");
    if (d.model != MCC_MODEL_DOUBLESIDE && d.n_cams < 2) return reject(why, "need >= 2 cameras");
    if (d.model == MCC_MODEL_OMNI && (d.nd != 4 || !d.xi)) return reject(why, "omni needs nd == 4 and xi");
    if (d.model != MCC_MODEL_OMNI && !(d.nd == 4 || d.nd == 5 || d.nd == 8 || d.nd == 12 || d.nd == 14))
        return reject(why, "pinhole nd must be 4, 5, 8, 12 or 14");
    if (d.model == MCC_MODEL_DOUBLESIDE && !d.cam_pose) return reject(why, "DOUBLESIDE needs cam_pose");
    const int C = d.n_cams, V = d.n_photos, E = d.n_edges;
    for (int e = 0; e < E; ++e) {
        if (d.edge_cam[e] < 0 || d.edge_cam[e] >= C || d.edge_photo[e] < 0 || d.edge_photo[e] >= V ||
            d.edge_n[e] < 1 || d.edge_off[e] < 0)
            return reject(why, "edge " + std::to_string(e) + " out of range");
        if (d.edge_n[e] > 1024) return reject(why, "more than 1024 corners in an edge");
        const int side = d.edge_side ? d.edge_side[e] : MCC_FRONT;
        if (side == MCC_BACK && d.model == MCC_MODEL_PINHOLE && !d.ds_pose)
            return reject(why, "BACK edge without doubleSideTransform (the reference dereferences an empty Mat)");
        if (side == MCC_BACK && d.model == MCC_MODEL_OMNI) return reject(why, "BACK edges are pinhole only");
    }
    // (every step form: the fused step needs <= 64 edges per photo to be chosen at all, and the split
    // step's groups hold one photo's edges in 64 LDS slots)
    std::vector<int> epp(V, 0);
    for (int e = 0; e < E; ++e)
        if (++epp[d.edge_photo[e]] > 64)
            return reject(why, "more than 64 edges (camera observations) of one photo vertex");
    if (global_dim(d) > 128) return reject(why, "global block larger than 128 parameters (22 cameras)");
    if (C > 63) return reject(why, "more than 63 cameras");
    return MCC_OK;
}

// ------------------------------------------------------------------------------- fixed transforms

// Host restatement of cvRodrigues2 matrix -> vector (with the polar re-orthonormalisation)
// used once per problem for fixed transforms (doubleSideTransform2vec,
// src/mymulticalib.cpp:105-117; cameraPose2vec, src/doubleSide.cpp:262-275).
void host_rodrigues_m2v(const double* Rin, double* r) {
    double R[9];
    std::memcpy(R, Rin, sizeof(R));
    for (int it = 0; it < 40; ++it) {
        double cof[9] = {R[4] * R[8] - R[5] * R[7], -(R[3] * R[8] - R[5] * R[6]), R[3] * R[7] - R[4] * R[6],
                         -(R[1] * R[8] - R[2] * R[7]), R[0] * R[8] - R[2] * R[6], -(R[0] * R[7] - R[1] * R[6]),
                         R[1] * R[5] - R[2] * R[4], -(R[0] * R[5] - R[2] * R[3]), R[0] * R[4] - R[1] * R[3]};
        double d = R[0] * cof[0] + R[1] * cof[1] + R[2] * cof[2], delta = 0;
        if (!(std::fabs(d) > 1e-300)) break;
        for (int k = 0; k < 9; ++k) {
            double v = 0.5 * (R[k] + cof[k] / d);
            delta = std::max(delta, std::fabs(v - R[k]));
            R[k] = v;
        }
        if (delta < 1e-15) break;
    }
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    double s = std::sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    c = c > 1. ? 1. : c < -1. ? -1. : c;
    double theta = std::acos(c);
    if (s < 1e-5) {
        if (c > 0) {
            rx = ry = rz = 0;
        } else {
            double t;
            t = (R[0] + 1) * 0.5; rx = std::sqrt(std::max(t, 0.));
            t = (R[4] + 1) * 0.5; ry = std::sqrt(std::max(t, 0.)) * (R[1] < 0 ? -1. : 1.);
            t = (R[8] + 1) * 0.5; rz = std::sqrt(std::max(t, 0.)) * (R[2] < 0 ? -1. : 1.);
            if (std::fabs(rx) < std::fabs(ry) && std::fabs(rx) < std::fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
            theta /= std::sqrt(rx * rx + ry * ry + rz * rz);
            rx *= theta; ry *= theta; rz *= theta;
        }
    } else {
        double vth = 1 / (2 * s) * theta;
        rx *= vth; ry *= vth; rz *= vth;
    }
    r[0] = rx; r[1] = ry; r[2] = rz;
}

// computeTiltProjectionMatrix (OpenCV calib3d, distortion_model.hpp) for the tilted-sensor model of
// cv::projectPoints with 14 coefficients, which src/mymulticalib.cpp:566 reaches with whatever
// Distortion the camera XML holds (:118-132): matTilt = matProjZ * (matRotY * matRotX), row-major,
// Matx products summed left to right from 0
void tilt_matrix(double tx, double ty, double M[9]) {
    const double cx = std::cos(tx), sx = std::sin(tx), cy = std::cos(ty), sy = std::sin(ty);
    const double rx[9] = {1, 0, 0, 0, cx, sx, 0, -sx, cx};
    const double ry[9] = {cy, 0, -sy, 0, 1, 0, sy, 0, cy};
    double rxy[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += ry[3 * i + k] * rx[3 * k + j];
            rxy[3 * i + j] = s;
        }
    const double pz[9] = {rxy[8], 0, -rxy[2], 0, rxy[8], -rxy[5], 0, 0, 1};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += pz[3 * i + k] * rxy[3 * k + j];
            M[3 * i + j] = s;
        }
}

// ------------------------------------------------------------------------------------ the planner

namespace {

// the camera-pair blocks of the reduced system's upper triangle, row-major: (b1, b2), b1 <= b2 < nb
struct Blocks {
    int nb;
    int index(int b1, int b2) const { return b1 * nb - b1 * (b1 - 1) / 2 + (b2 - b1); }
    int row(int b) const {   // the b1 of block b
        int r = 0;
        while (r + 1 < nb && index(r + 1, r + 1) <= b) ++r;
        return r;
    }
    bool diagonal(int b) const { const int r = row(b); return index(r, r) == b; }
};

// Greedy groups of consecutive photos: at most max_photos photos and max_edges edges each (a photo
// with more edges than that is a group of its own).  Returns the first photo of each group and V.
std::vector<int> group_photos(const std::vector<int>& photo_ptr, int max_photos, int max_edges) {
    const int V = (int)photo_ptr.size() - 1;
    std::vector<int> g(1, 0);
    for (int v = 0; v < V;) {
        int w = v, edges = 0;
        while (w < V && w - v < max_photos && (w == v || edges + (photo_ptr[w + 1] - photo_ptr[w]) <= max_edges)) {
            edges += photo_ptr[w + 1] - photo_ptr[w];
            ++w;
        }
        g.push_back(w);
        v = w;
    }
    return g;
}

// distortion specialisation (zero coefficients are exact no-ops in OpenCV's formula)
void plan_distortion(const mcc_desc& d, Plan& p) {
    if (d.model == MCC_MODEL_OMNI) return;
    const int C = p.C;
    for (int c = 0; c < C; ++c)
        for (int q = 5; q < std::min(d.nd, 12); ++q) {
            const float v = d.D[d.nd * c + q];
            if (v != 0.f) {
                if (q < 8) p.rational = true;
                else p.prism = 1;
            }
        }
    // the tilted sensor (tau_x, tau_y: D[12], D[13] of 14): matTilt per camera in FP64, as
    // cvProjectPoints2Internal forms it from the CV_32F coefficients (identity where tau = 0, which
    // the projection then applies exactly: vecTilt = (xd0, yd0, 1), invProj = 1)
    bool tilt = false;
    for (int c = 0; c < C && d.nd == 14; ++c) tilt = tilt || d.D[14 * c + 12] != 0.f || d.D[14 * c + 13] != 0.f;
    if (tilt) {
        p.rational = true;   // zero k4..k6 / s1..s4 are exact no-ops in the 14-term formula
        p.prism = 2;
        p.tilt.resize(9 * (size_t)C);
        for (int c = 0; c < C; ++c) tilt_matrix(d.D[14 * c + 12], d.D[14 * c + 13], p.tilt.data() + 9 * c);
    }
}

// photo-major edge order (stable within a photo: reference edge order), the corner streams in that
// order, and the per-edge records
void plan_order_and_corners(const mcc_desc& d, Plan& p) {
    const int V = p.V, E = p.E;
    p.dev2ref_edge.resize(E);
    std::iota(p.dev2ref_edge.begin(), p.dev2ref_edge.end(), 0);
    std::stable_sort(p.dev2ref_edge.begin(), p.dev2ref_edge.end(),
                     [&](int a, int b) { return d.edge_photo[a] < d.edge_photo[b]; });
    p.photo_ptr.assign(V + 1, 0);
    for (int e = 0; e < E; ++e) p.photo_ptr[d.edge_photo[e] + 1]++;
    for (int v = 0; v < V; ++v) {
        p.max_epp = std::max(p.max_epp, p.photo_ptr[v + 1]);
        p.photo_ptr[v + 1] += p.photo_ptr[v];
    }
    long long ncorner = 0;
    for (int e = 0; e < E; ++e) ncorner += d.edge_n[e];
    p.corners = ncorner;
    for (auto* s : {&p.obj_x, &p.obj_y, &p.obj_z, &p.img_u, &p.img_v}) s->resize(ncorner);
    p.info.resize(E);
    p.gblock.resize(E);
    p.ephoto.resize(E);
    p.dev2ref_corner.resize(ncorner);
    p.edge_n_dev.resize(E);
    long long off = 0;
    for (int de = 0; de < E; ++de) {
        const int e = p.dev2ref_edge[de], n = d.edge_n[e];
        const int side = d.edge_side ? d.edge_side[e] : MCC_FRONT;
        for (int i = 0; i < n; ++i) {
            const long long s = (long long)d.edge_off[e] + i;
            p.obj_x[off + i] = d.obj[3 * s]; p.obj_y[off + i] = d.obj[3 * s + 1]; p.obj_z[off + i] = d.obj[3 * s + 2];
            p.img_u[off + i] = d.img[2 * s]; p.img_v[off + i] = d.img[2 * s + 1];
            p.dev2ref_corner[off + i] = s;
        }
        p.info[de] = Int4{d.edge_cam[e], side, (int)off, n};
        if (side == MCC_BACK) p.has_back = 1;
        p.ephoto[de] = d.edge_photo[e];
        p.edge_n_dev[de] = n;
        if (d.model == MCC_MODEL_DOUBLESIDE) p.gblock[de] = side == MCC_BACK ? 0 : -1;
        else p.gblock[de] = d.edge_cam[e] - 1;
        off += n;
    }
    p.photo_corner.assign(V + 1, 0);
    for (int v = 0; v < V; ++v) {
        p.photo_corner[v + 1] = p.photo_corner[v];
        for (int de = p.photo_ptr[v]; de < p.photo_ptr[v + 1]; ++de) p.photo_corner[v + 1] += p.info[de].w;
        p.max_cpp = std::max(p.max_cpp, p.photo_corner[v + 1] - p.photo_corner[v]);
    }
}

// Which of the step's forms the rig takes -- the fused k_linearize, k_group, or k_prep -> k_edge ->
// k_photo -- and the photo groups of the split forms.
void plan_groups_and_path(const Options& opt, int n_cu, Plan& p) {
    const int V = p.V;
    // small camera blocks and at most two photo workgroups per CU (the fused kernel's occupancy):
    // one kernel per Gauss-Newton step.  More photos than that run the fused kernel's serial
    // per-photo chain in several rounds, and the split step is faster (config4, 1000 views:
    // 43.3 vs 47.4 us; config2, 500 views: 38.2 vs 25.9 us).  MCC_FUSED=1 / 0 forces either.
    // (the tilted sensor takes the split step: the fused kernel's PRISM variants already hold 256 VGPRs,
    // and the tilt's per-corner 3 x 3 map and 2 x 2 chain spill there; k_group / k_edge have room)
    const bool fusable = p.m <= kFusedMaxM && V > 0 && p.max_epp <= 64 && p.prism != 2;
    p.fused = fusable && V <= 2 * n_cu;

    // The split step's photo work (k_group / k_photo) takes groups of consecutive photos (at most
    // kPhotoGroup photos and the cap's edges).
    // k_group takes groups of at most kGroupRound edges (one 16-edge round per workgroup; config4's
    // 1 000 photos -> 250 workgroups, one per CU); k_photo's groups sum more photos (<= 64 edges).
    // k_group (two workgroups per CU) wins while its groups fit the CUs in one wave of workgroups
    // (config4: 32.3 vs 36.9 us per step); with more groups the three-kernel form's higher
    // occupancy wins (config5: 67.3 vs 61.0, config3: 185.5 vs 120.5).  MCC_GROUP=1 / 0 forces.
    p.group_cap = opt.group_edges > 0 ? opt.group_edges : kGroupRound;   // MCC_GROUP_EDGES (A/B; > 16: several rounds)
    p.pgrp_ptr = group_photos(p.photo_ptr, kPhotoGroup, p.group_cap);
    // More 16-edge groups than CUs: wider groups (up to two 16-edge rounds each) while that brings them
    // within one wave of workgroups -- a second wave of groups costs a whole group chain, a second
    // round inside a group only its edge phases (config3's 8-rank shard, 625 views / 4 871 edges:
    // 313 groups of 16 -> 244 of <= 24 edges, 58.4 -> 47.4 us per step against the three kernels;
    // at 64 edges config5's 2 000 views take 65.0 vs 60.2 us, so the widening stops at 32)
    for (int cap = kGroupRound + 8; opt.group_edges < 0 && (int)p.pgrp_ptr.size() - 1 > n_cu && cap <= 2 * kGroupRound;
         cap += 8) {
        std::vector<int> g = group_photos(p.photo_ptr, kPhotoGroup, cap);
        if ((int)g.size() - 1 <= n_cu) {
            p.pgrp_ptr = std::move(g);
            p.group_cap = cap;
        }
    }
    // The fused kernel runs a photo's edges one per wave on its four waves, so photos with more than
    // four edges take it through several dependent rounds; k_group spreads a group's 16 edges over its
    // eight waves in one.  With more than four edges per photo and k_group's groups within the CUs the
    // split step wins (config5's 500-view shard, 8 edges per photo: 28.9 vs 32.5 us per step).
    if (p.fused && p.max_epp > 4 && (int)p.pgrp_ptr.size() - 1 <= n_cu) p.fused = false;
    if (opt.fused >= 0) p.fused = fusable && opt.fused != 0;
    p.use_group = !p.fused && (int)p.pgrp_ptr.size() - 1 <= n_cu;
    if (opt.group >= 0) p.use_group = !p.fused && opt.group != 0;
    if (!p.use_group) {
        p.pgrp_ptr = group_photos(p.photo_ptr, kPhotoGroup, kPhotoGroupEdges);
        p.group_cap = kPhotoGroupEdges;
    }
    p.group_lanes = opt.group_lanes;
    p.n_pgroups = (int)p.pgrp_ptr.size() - 1;
    if (!p.fused && !p.use_group) {
        // k_prep4's groups: consecutive photos, <= kPrepPhotos of them and kPrepEdges edges (or one photo)
        p.prep_lanes = opt.prep_lanes;
        p.prep_ptr = group_photos(p.photo_ptr, kPrepPhotos, kPrepEdges);
        p.prep_edge.resize(p.prep_ptr.size());
        for (size_t g = 0; g < p.prep_ptr.size(); ++g) p.prep_edge[g] = p.photo_ptr[p.prep_ptr[g]];
        p.n_prep = (int)p.prep_ptr.size() - 1;
    }
    // the fused step's two-level reduction: groups of ~sqrt(V) consecutive photos
    p.group_size = std::max(1, (int)std::ceil(std::sqrt((double)std::max(V, 1))));
    p.n_groups = (std::max(V, 1) + p.group_size - 1) / p.group_size;
}

// Schur pair lists.  Each group sums its photos' pair products per camera-pair block: one slot per
// (group, block), block-major over the groups, k_schur sums a block's slots in order.  A
// contribution is one ordered edge pair (e1, e2) of a photo with gblock(e1) <= gblock(e2) (both
// orders within one block), in photo then edge order.  Returns each block's gpairs, group order.
std::vector<std::vector<int>> plan_pair_lists(const Blocks& blocks, Plan& p) {
    const int NG = p.n_pgroups;
    p.gpair_ptr.assign(NG + 1, 0);
    p.gcon_ptr.assign(NG + 1, 0);
    std::vector<std::vector<int>> blk_src(p.nblk);
    std::vector<std::vector<unsigned>> per_blk(p.nblk);
    for (int g = 0; g < NG; ++g) {
        const int ge0 = p.photo_ptr[p.pgrp_ptr[g]];
        std::vector<int> used;
        for (int v = p.pgrp_ptr[g]; v < p.pgrp_ptr[g + 1]; ++v)
            for (int e1 = p.photo_ptr[v]; e1 < p.photo_ptr[v + 1]; ++e1) {
                if (p.gblock[e1] < 0) continue;
                for (int e2 = p.photo_ptr[v]; e2 < p.photo_ptr[v + 1]; ++e2) {
                    if (p.gblock[e2] < 0 || p.gblock[e1] > p.gblock[e2]) continue;
                    const int b = blocks.index(p.gblock[e1], p.gblock[e2]);
                    if (per_blk[b].empty()) used.push_back(b);
                    per_blk[b].push_back((unsigned)(e1 - ge0) | ((unsigned)(e2 - ge0) << 8) |
                                         ((e1 == e2 ? 1u : 0u) << 16) | ((unsigned)(v - p.pgrp_ptr[g]) << 17));
                }
            }
        // the group's block pairs by contribution count, largest first: k_photo's pair tasks of a
        // wave step through their contributions in lock-step, so each wave should hold pairs of
        // similar counts (config3: 15.5 -> 10.8 iterations on a group's busiest wave).  Outputs
        // are unchanged: a pair's slot offset travels with it.
        std::sort(used.begin(), used.end(), [&](int x, int y) {
            return per_blk[x].size() != per_blk[y].size() ? per_blk[x].size() > per_blk[y].size() : x < y;
        });
        const int cbase = (int)p.gcon.size();
        for (int b : used) {
            blk_src[b].push_back((int)p.gpairs.size());
            p.gpairs.push_back(Int4{(int)p.gcon.size() - cbase, (int)per_blk[b].size(), blocks.diagonal(b) ? 2 : 0, -1});
            p.gcon.insert(p.gcon.end(), per_blk[b].begin(), per_blk[b].end());
            per_blk[b].clear();
        }
        p.gpair_ptr[g + 1] = (int)p.gpairs.size();
        p.gcon_ptr[g + 1] = (int)p.gcon.size();
        p.max_gpairs = std::max(p.max_gpairs, p.gpair_ptr[g + 1] - p.gpair_ptr[g]);
        p.max_gcon = std::max(p.max_gcon, p.gcon_ptr[g + 1] - p.gcon_ptr[g]);
        p.max_gedges = std::max(p.max_gedges, p.photo_ptr[p.pgrp_ptr[g + 1]] - ge0);
    }
    return blk_src;
}

// The pairs' slots and k_schur's work items.
// slot sizes: 48 doubles on a diagonal camera-pair block (S entries, r, JTE), 36 off the
// diagonal (no self pair there, so r and JTE would be zeros); pair .w = the slot's offset in
// doubles; item = {block, first slot's offset, slots, slot size}
int plan_slots_and_items(const Options& opt, const Blocks& blocks, const std::vector<std::vector<int>>& blk_src, Plan& p,
                         std::string* why) {
    p.block_items.assign(p.nblk + 1, 0);
    int n_slots = 0;
    size_t n_doubles = 0;
    // m <= 30 with several camera-pair blocks (one hand-off level: the final arriver loads every
    // item's partial in one batch, so more items cost it little): 64 slots per item, four items per
    // 250-slot block at config4 -- 28.4-28.6 vs 29.1-29.2 us per step with 320 (interleaved, round 4;
    // 32: 28.7-28.8, 16: 30.7).  config5's single block (DoubleSide, m = 6) keeps 320 (60.5-60.7 vs
    // 60.8-60.9 at 64)
    const int min_slots = opt.item_slots > 0 ? opt.item_slots : (p.m <= 30 && p.nblk > 1 ? 64 : 320);
    for (int b = 0; b < p.nblk; ++b) {
        const int stride = blocks.diagonal(b) ? 48 : 36;
        const int begin = n_slots;
        const size_t base = n_doubles;
        for (int src : blk_src[b]) {
            p.gpairs[src].w = (int)n_doubles;
            n_doubles += stride;
            ++n_slots;
        }
        if (n_doubles > (size_t)INT32_MAX) {
            if (why) *why = "too many Schur pairs";
            return MCC_EINVAL;
        }
        const int end = n_slots;
        // <= 24 work items per block keeps the last-arriver assembly short; >= min_slots slots per
        // item (MCC_ITEM_SLOTS, default 320) amortises an item's fixed latency (one load round trip, the
        // write-through hand-off and ticket) over more slots (config3, interleaved: 160 -> 320 slots
        // 120.8 -> 119.6 us per step, 640 122.3; configs 4 and 5 within noise)
        // A block of at most min_slots slots is one item, which writes the block's packed entries
        // itself (slot size | kItemSingle): no item hand-off level (config4: every block, k_schur
        // 9.2 -> 8.7 us).  Larger blocks keep >= min_slots per item: config5's one block of 250
        // slots as a single item took 10.7 us against 9.3 as two items and the hand-off.
        // Blocks of (single_max, min_slots] slots take two items (config5's 250-slot block: k_schur
        // 10.5 us as one item vs 9.8 as two under rocprofv3)
        const int nsl = end - begin, single_max = std::min(min_slots, 160);
        int per_item = std::max(min_slots, (nsl + 23) / 24);
        if (nsl > single_max && nsl <= per_item) per_item = (nsl + 1) / 2;
        const int single = (nsl <= per_item) ? kItemSingle : 0;
        for (int s = begin; s < end; s += per_item) {
            p.items.push_back(Int4{b, (int)(base + (size_t)(s - begin) * stride), std::min(end, s + per_item) - s,
                                   stride | single});
            p.max_item_slots = std::max(p.max_item_slots, p.items.back().z);
        }
        // a block no photo couples gets one empty item: it writes the block's zeros (every packed
        // entry is rewritten each step; the all-reduce leaves sums there)
        if (begin == end) p.items.push_back(Int4{b, (int)base, 0, stride | kItemSingle});
        p.block_items[b + 1] = (int)p.items.size();
    }
    p.n_pair_doubles = n_doubles;
    // A camera block without an observation here is accepted: a rank of a photo-sharded problem
    // may hold no photo of some camera while the summed system is fine.  If the whole problem
    // leaves a camera unobserved, the reduced system is singular and the step fails with
    // MCC_ENOTPD (the device positive-definiteness check of the solve).
    p.n_items = (int)p.items.size();
    p.n_pairs = n_slots;
    p.n_norm_chunks = (p.V + 255) / 256;
    return MCC_OK;
}

// what k_group's phase 0 reads instead of chasing indices: the groups' first edges, each edge's photo
// within its group, the per-group headers and the cameras' intrinsics rows
void plan_headers(const mcc_desc& d, Plan& p) {
    const int NG = p.n_pgroups, C = p.C;
    p.pgrp_edge.resize(p.pgrp_ptr.size());
    for (size_t g = 0; g < p.pgrp_ptr.size(); ++g) p.pgrp_edge[g] = p.photo_ptr[p.pgrp_ptr[g]];
    p.edge_lphoto.assign(std::max(p.E, 1), 0);
    for (int g = 0; g < NG; ++g)
        for (int v = p.pgrp_ptr[g]; v < p.pgrp_ptr[g + 1]; ++v)
            for (int e = p.photo_ptr[v]; e < p.photo_ptr[v + 1]; ++e) p.edge_lphoto[e] = (unsigned char)(v - p.pgrp_ptr[g]);
    // k_group's per-group headers (kGHdr*, mcc_layout.hpp): the ranges, the group-relative photo_ptr
    // entries and the first round's edge records at a fixed stride
    p.ghdr.assign((size_t)kGHdrInts * std::max(NG, 1), 0);
    for (int g = 0; g < NG; ++g) {
        int* h = p.ghdr.data() + (size_t)kGHdrInts * g;
        const int p0 = p.pgrp_ptr[g], np = p.pgrp_ptr[g + 1] - p0, ge0 = p.photo_ptr[p0], gne = p.photo_ptr[p0 + np] - ge0;
        h[0] = p0; h[1] = np; h[2] = ge0; h[3] = gne;
        h[4] = p.gpair_ptr[g]; h[5] = p.gpair_ptr[g + 1] - p.gpair_ptr[g];
        h[6] = p.gcon_ptr[g]; h[7] = p.gcon_ptr[g + 1] - p.gcon_ptr[g];
        for (int q = 0; q <= kPhotoGroup; ++q) h[kGHdrPhoto + q] = p.photo_ptr[p0 + std::min(q, np)] - ge0;
        for (int le = 0; le < std::min(gne, kGroupRound); ++le) {
            const Int4 f = p.info[ge0 + le];
            int* hi = h + kGHdrInfo + 4 * le;
            hi[0] = f.x; hi[1] = f.y; hi[2] = f.z; hi[3] = f.w;
            h[kGHdrGb + le] = p.gblock[ge0 + le];
            h[kGHdrEq + le] = p.edge_lphoto[ge0 + le];
        }
    }
    // the cameras' intrinsics rows as k_group keeps them in LDS: fx fy cx cy skew xi k[12] matTilt[9] pad,
    // each the float's exact value in FP64
    p.kintr.assign((size_t)kGIntr * C, 0.0);
    for (int c = 0; c < C; ++c) {
        double* kt = p.kintr.data() + (size_t)kGIntr * c;
        const float* Kc = d.K + 9 * c;
        kt[0] = Kc[0]; kt[1] = Kc[4]; kt[2] = Kc[2]; kt[3] = Kc[5]; kt[4] = Kc[1];
        kt[5] = d.model == MCC_MODEL_OMNI && d.xi ? (double)d.xi[c] : 0.0;
        for (int q = 0; q < 12; ++q) kt[6 + q] = q < d.nd ? (double)d.D[d.nd * c + q] : 0.0;
        if (p.prism == 2) tilt_matrix(d.D[14 * c + 12], d.D[14 * c + 13], kt + 18);
    }
}

// fixed transforms as (rvec, tvec), and the step factors
void plan_fixed_transforms(const mcc_desc& d, Plan& p) {
    const int C = p.C;
    p.cam_rt.assign(6 * (size_t)C, 0.f);
    if (d.model == MCC_MODEL_DOUBLESIDE) {
        for (int c = 0; c < C; ++c) {
            double R[9], r[3];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) R[i * 3 + j] = d.cam_pose[16 * c + i * 4 + j];
            host_rodrigues_m2v(R, r);
            for (int i = 0; i < 3; ++i) {
                p.cam_rt[6 * c + i] = (float)r[i];
                p.cam_rt[6 * c + 3 + i] = d.cam_pose[16 * c + i * 4 + 3];
            }
        }
    }
    p.ds_rt.assign(6, 0.0);
    if (d.ds_pose && d.model == MCC_MODEL_PINHOLE) {
        double R[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i * 3 + j] = d.ds_pose[i * 4 + j];
        host_rodrigues_m2v(R, p.ds_rt.data());
        for (int i = 0; i < 3; ++i) p.ds_rt[3 + i] = d.ds_pose[i * 4 + 3];
    }
    p.alpha.resize(4096);
    for (size_t k = 0; k < p.alpha.size(); ++k) p.alpha[k] = std::pow(0.95, (double)k + 1.0);   // src/multicalib.cpp:483
}

// The rest of the step's form: hand-off levels, LDS sizes, both warm solves, the fold and its
// progress rule, and the switches that travel with the problem.
void plan_flags(const Options& opt, int n_cu_dev, Plan& p) {
    const int parts = p.n_items + p.n_norm_chunks;   // k_schur's grid: the items and the norm chunks
    p.ntri = p.m * (p.m + 1) / 2;
    p.packed_len = p.ntri + 2 * p.m + 2;
    // one hand-off level (m <= 30) while the final arriver loads everything in one batch
    const bool one_fits = p.m <= 30 && 48 * parts + p.m * p.m <= kSchurOneLevelLoads * 256;
    p.schur_one_level = one_fits && opt.schur_one_level;
    p.photo_shmem = photo_lds_bytes(p.max_gedges, p.max_gpairs, p.max_gcon);
    p.group_shmem = group_lds_bytes(p.max_gedges, p.C, p.max_gpairs, p.max_gcon);
    // m <= 30 on k_group -> k_schur (config4): the previous system's inverse from a spare k_group
    // workgroup, refinement in k_schur's final solve (MCC_SMALL_WARM=0: the register Gauss-Jordan
    // only).  With S and the inverse in registers the refinement takes ~1.7 us at m = 18 against the
    // elimination's ~2.6 (config4, interleaved: 28.9 vs 29.4 us per step); round 4's first form, reading
    // them from LDS per product, took ~3 us and lost
    // The fused step (config2) refines with the inverse its previous launch's spare workgroup formed
    // (two updates stale: the spare and the final arriver of one launch run at the same time); its
    // LDS holds the spare's [S | I] and the final arriver's S, r and inverse (mcc_lin_shmem).
    // Two buffers by iteration parity, each tagged with the iteration that made it.
    p.small_warm = ((!p.fused && p.use_group && p.schur_one_level &&
                     p.group_shmem >= (size_t)2 * p.m * p.m * sizeof(double)) ||   // the spare's [S | I] in LDS
                    (p.fused && p.m <= 30)) &&
                   opt.small_warm;
    // the folded reduction: k_group's one-level m <= 30 step with items of at most kSub x kFoldSlots
    // slots (every m <= 30 rig with several camera-pair blocks takes 64; a one-block rig 320: no fold)
    p.gfold = !p.fused && p.use_group && p.schur_one_level && p.max_item_slots <= 5 * 13 &&
              48 * parts + p.m * p.m + 1 <= kSchurOneLevelLoads * 256;
    // Progress of the folded launch does not rest on dispatch order.  Its producers (the groups, the
    // spare) never wait; its consumers (items, norm chunks, the final workgroup) spin until their words
    // land.  Whatever order the dispatcher picks, the launch completes as long as the spinning
    // consumers cannot hold every workgroup slot a producer needs: with at least one slot left over,
    // some producer is always resident or dispatchable, runs to its end and frees its slot.  k_group
    // fits at least one workgroup per CU, so the fold is taken only when the consumers fill at most
    // half of the CUs (the other half stays for producers even when another kernel shares the device);
    // otherwise the step is k_group -> k_schur.  MCC_FOLD_CONSUMERS_FIRST=1 (tests) lays the grid out
    // with the consumers at the lowest indices to exercise exactly that.
    const int fold_spin = parts + 1;
    p.gfold = p.gfold && 2 * fold_spin <= n_cu_dev && opt.gfold;
    p.fold_first = p.gfold && p.model == MCC_MODEL_OMNI && opt.fold_first;   // (a test instantiation, omnidir rigs)
    if (p.gfold) {
        // the final workgroup's LDS (k_schur's one-level layout) within k_group's
        p.group_shmem = std::max(p.group_shmem, schur_lds_bytes(p.m, 1, 1, 1, parts, p.nblk));
        int max_bi = 0;
        for (int b = 0; b < p.nblk; ++b) max_bi = std::max(max_bi, p.block_items[b + 1] - p.block_items[b]);
        const int ivt = 512 - 48 * p.nblk - 2;   // the inverse's threads
        p.fold_direct = p.group_lanes == 32 && max_bi <= 8 && p.n_norm_chunks <= 4 && ivt > 0 && p.m * p.m <= 8 * ivt &&
                        opt.fold_direct;
        // MCC_FOLD_DYN=1: the groups themselves take the items, norm chunks and the final task by ticket
        // once their own work is done, instead of trailing workgroups that wait for a CU the groups free
        // (config5's 500-view shard: the trailing items started 1.5 us after the last group ended).
        // Measured, not the default: config4 26.55 vs 26.41 us per step, config5's shard 29.3 vs 29.5
        // (interleaved) -- the last group's slots, not the items' start, set the tail.
        // With fold_dyn a finished group spins on slots of groups that may not have started, so the
        // whole grid must be resident at once: the groups and the spare within one workgroup per CU.
        p.fold_dyn = opt.fold_dyn > 0 && p.n_pgroups >= 2 * (parts + 1) && p.prism != 2 && p.n_pgroups + 1 <= n_cu_dev;
    }
    // the m > 30 warm solve: the staged system and inverse fit k_solve's LDS up to M = 96
    p.warm = !p.fused && p.m > 30 && p.m <= 96 && opt.warm;
    p.helper_refine = p.warm && opt.helper_refine;   // (single GPU only: warm_ctx, enqueue_step)
    p.helper_early = p.helper_refine && (opt.helper_poll >= 0 ? opt.helper_poll != 0 : !p.use_group);
    // (mcc_kernels.hip gj_inverse_blocked: where the helper's cycle bounds the step)
    p.inv_la = opt.inv_la >= 0 ? opt.inv_la : p.use_group;
    if (p.warm) p.prev_stride = (p.ntri + p.m + 1) & ~1;
    p.warm_wait_ticks = opt.warm_wait_ticks;
    p.warm_delay_ticks = opt.warm_delay_ticks;
    p.spare_delay_ticks = opt.spare_delay_ticks;
    p.peer_timeout = opt.peer_timeout_ticks;
    // the helper outlives a k_solve's longest wait at a peer exchange
    p.warm_idle_ticks = p.warm_wait_ticks + p.peer_timeout + 100000000LL;
    p.use_graph = opt.use_graph;
    p.graph_sizes = opt.graph_sizes;
    p.peer_push = opt.peer_push;
    p.poison_level = opt.poison_level;
    p.poison = p.poison_level != 0;
    p.warm_poison = opt.warm_poison;
    p.small_stats = opt.small_stats;
    p.fault_photo = opt.fault_photo;
}

}  // namespace

int plan_problem(const mcc_desc& d, const Options& opt, int n_cu, int n_cu_dev, Plan* out, std::string* why) {
    Plan& p = *out;
    p = Plan();
    p.model = d.model; p.C = d.n_cams; p.V = d.n_photos; p.E = d.n_edges; p.nd = d.nd;
    p.m = global_dim(d);
    p.P = p.m + 6 * p.V;
    const Blocks blocks{p.m / 6};
    p.nblk = blocks.nb * (blocks.nb + 1) / 2;
    plan_distortion(d, p);
    plan_order_and_corners(d, p);
    plan_groups_and_path(opt, n_cu, p);
    const std::vector<std::vector<int>> blk_src = plan_pair_lists(blocks, p);
    if (int rc = plan_slots_and_items(opt, blocks, blk_src, p, why)) return rc;
    plan_headers(d, p);
    plan_fixed_transforms(d, p);
    plan_flags(opt, n_cu_dev, p);
    return MCC_OK;
}

}  // namespace mcc
