// mcc_plan.hpp -- the host-only half of mcc_create: the environment switches read once (Options), the
// descriptor's validation, and the step planner, which decides the form a rig's Gauss-Newton step takes
// and builds every index structure the kernels rely on (Plan).  Plain C++17 on the descriptor, the
// options and two CU counts: no HIP, no device, so the path rules and the structures can be checked on
// a CPU (tests/test_plan.py drives tests/cpp/test_plan.cpp over it).
#pragma once
#include <string>
#include <vector>

#include "../../include/mcc.h"
#include "mcc_layout.hpp"

namespace mcc {

constexpr int kFusedMaxM = 30;    // the fused single-kernel step's largest global block
constexpr int kGraphSizes = 7;    // update steps per graph launch: 2^k, k < kGraphSizes (up to 64)

// Every MCC_* switch of libmcc.so's bundle-adjustment path, parsed once per mcc_create.  A switch that
// can only narrow a rule is a bool (unset = on); one whose being set matters carries -1 for unset.
struct Options {
    // `get` returns a switch's text or null (std::getenv in the library; a table in the tests)
    static Options from_env(const char* (*get)(const char* name));

    int cus = 0;              // MCC_CUS (test): the path rules at another CU count (0: the device's)
    int fused = -1;           // MCC_FUSED=1 / 0 forces the fused step (where it can run) or the split step
    int group = -1;           // MCC_GROUP=1 / 0 forces k_group or the three kernels on the split step
    int group_edges = -1;     // MCC_GROUP_EDGES: k_group's edges per group, in [1, 4 kGroupRound] (A/B; no widening)
    int group_lanes = 32;     // MCC_GROUP_LANES: k_group's lanes per edge (16, anything else 32)
    int prep_lanes = 1;       // MCC_PREP_LANES=4: k_prep4 (measured slower at configs 3 and 5)
    int item_slots = 0;       // MCC_ITEM_SLOTS: least slots per k_schur item (0: the rule's 64 / 320)
    bool schur_one_level = true;   // MCC_SCHUR_ONE_LEVEL=0 restores k_schur's two hand-off levels
    bool small_warm = true;   // MCC_SMALL_WARM=0: the m <= 30 solve by the register Gauss-Jordan only
    bool gfold = true;        // MCC_GFOLD=0 keeps k_group -> k_schur
    bool fold_direct = true;  // MCC_FOLD_DIRECT=0: the folded final workgroup copies, then sums
    int fold_dyn = -1;        // MCC_FOLD_DYN=1: the groups take the reduction's tasks by ticket
    bool fold_first = false;  // MCC_FOLD_CONSUMERS_FIRST=1 (test, omnidir rigs): consumers at the lowest grid indices
    bool warm = true;         // MCC_WARM=0 turns the m > 30 warm solve off
    bool helper_refine = true;   // MCC_HELPER_REFINE=0: the helper only inverts
    int helper_poll = -1;     // MCC_HELPER_POLL=0 / 1 forces the helper's batch / polled staging
    int inv_la = -1;          // MCC_INV_LA=0 / 1 forces the helper's look-ahead inversion off / on
    bool use_graph = true;    // MCC_GRAPH=0: eager launches
    int graph_sizes = kGraphSizes;   // MCC_GRAPH_SIZES in [1, kGraphSizes] (A/B of the launch granularity)
    bool peer_push = true;    // MCC_PEER_PUSH=0: k_solve's one workgroup sends too
    int poison_level = 0;     // MCC_POISON_HANDOFF (test)
    int warm_poison = 0;      // MCC_WARM_POISON=1 (test): the helper publishes NaN inverses
    bool small_stats = false; // MCC_SOLVE_STATS=1: count the m <= 30 warm solves
    int fault_photo = -1;     // MCC_FAULT_PHOTO (test)
    // s_memrealtime ticks (100 MHz): MCC_WARM_TIMEOUT_MS (default 10 s, at least 1 ms), MCC_WARM_DELAY_US,
    // MCC_SPARE_DELAY_US (tests), MCC_PEER_TIMEOUT_MS (default 30 s, at least 1 ms)
    long long warm_wait_ticks = 1000000000LL, warm_delay_ticks = 0, spare_delay_ticks = 0;
    long long peer_timeout_ticks = 3000000000LL;
};

// The plan's scalars: what mcc_problem keeps of the plan for the life of the problem (it derives from
// this struct; each field is declared here and nowhere else).
struct PlanScalars {
    int model = 0, C = 0, V = 0, E = 0, nd = 0;
    int m = 0, P = 0;        // the global block (6 (C - 1), DoubleSide 6) and the parameter count m + 6 V
    long long corners = 0;
    bool rational = false;
    int prism = 0;   // 1: thin prism s1..s4, 2: + the tilted sensor (nd = 14, tau != 0)
    int has_back = 0;
    int max_epp = 1, nblk = 0, n_items = 0, n_pairs = 0, n_norm_chunks = 0;
    size_t n_pair_doubles = 0;   // Schur pair-product slots (36 or 48 doubles each)
    // split step's k_photo groups (consecutive photos) and their pair / contribution lists
    int n_pgroups = 0, max_gpairs = 0, max_gcon = 0, max_gedges = 0;
    size_t photo_shmem = 0;
    // split step as ONE fused kernel per group (k_group: photo update, edge prologues, sweep, chain,
    // photo Schur work) instead of k_prep -> k_edge -> k_photo; MCC_GROUP=0 selects the three
    int use_group = 1;
    int group_cap = kGroupRound;   // k_group's edges per group (16; widened or MCC_GROUP_EDGES: more)
    size_t group_shmem = 0;   // k_group's LDS (with the fold: at least its final workgroup's, schur_lds_bytes)
    int group_lanes = 32;   // k_group's lanes per edge (32: 512-thread workgroups; 16: 256)
    // fused single-kernel step (m <= kFusedMaxM): photo contributions + two-level reduction
    int fused = 0, group_size = 1, n_groups = 1;
    // m > 30 (or MCC_FUSED=0): the split step k_prep -> k_edge -> k_photo -> k_schur -> k_solve
    int max_cpp = 1;   // most corners of one photo
    // MCC_POISON_HANDOFF=1 (test): every buffer handed between workgroups inside one launch or
    // between the step's kernels is filled with NaN (all-ones bytes) before each step, so that a
    // read of a word its producer has not yet stored this step shows up in the result
    bool poison = false;
    int poison_level = 0;
    bool peer_push = true;   // m > 30 with the peer transport: k_peer_push sends from many workgroups
    int schur_one_level = 0; // k_schur's single hand-off level (m <= 30; MCC_SCHUR_ONE_LEVEL=0 restores two)
    int n_prep = 0, prep_lanes = 1;   // MCC_PREP_LANES=4: k_prep4 (measured slower at configs 3 and 5)
    // the m <= 30 warm solve: a spare workgroup of k_group / k_linearize inverts the previous step's
    // system, the step's final solve refines with it (MCC_SMALL_WARM=0: the register Gauss-Jordan only)
    bool small_warm = false;
    // warm solve (m > 30 split step, MCC_WARM=0 turns it off): a resident helper kernel on a side
    // stream (one per batch of update steps) inverts each step's reduced system while the next step
    // linearises; the next k_solve refines with it (WarmCtx, mcc_internal.h)
    bool warm = false;
    int prev_stride = 0;             // prev2's [S | r] copies: the packed length rounded up to even
    bool helper_refine = false;      // single GPU, m > 30: the helper refines too (MCC_HELPER_REFINE)
    // k_schur publishes the system at its start and the helper polls prev2's words as the blocks land
    // (config3, three-kernel step: 108.4-109.1 -> 107.4-107.6 us per step), else at its end and the helper
    // stages in one batch (k_group's step: config3's 8-rank shard, whose step the helper's cycle bounds,
    // was 0.9 us slower polled); MCC_HELPER_POLL=0/1 forces either
    int helper_early = 0;
    int inv_la = 0;                  // the helper's look-ahead inversion (WarmCtx::inv_la): the k_group path
    int warm_poison = 0;             // MCC_WARM_POISON=1 (test): the helper publishes NaN inverses
    // k_solve's bound on the wait for the helper (MCC_WARM_TIMEOUT_MS, default 10 s; a step that hits
    // it fails with MCC_ETIMEOUT), the helper's idle exit (the wait bound plus the peer timeout: a
    // k_solve may sit in a peer exchange before it publishes), the test delay (MCC_WARM_DELAY_US)
    long long warm_wait_ticks = 1000000000LL, warm_idle_ticks = 4100000000LL, warm_delay_ticks = 0;
    long long spare_delay_ticks = 0;  // MCC_SPARE_DELAY_US (test): the fused step's spare starts this late
    long long peer_timeout = 0;       // the peer exchange's wait bound (MCC_PEER_TIMEOUT_MS), s_memrealtime ticks
    bool small_stats = false;         // MCC_SOLVE_STATS=1: count the m <= 30 warm solves (SolveCtx::sstats)
    // k_group's step with k_schur's reduction and the solve folded into the same launch (LinArgs::fold;
    // MCC_GFOLD=0 keeps k_group -> k_schur): fnorm [4V] and fiv [m^2 + 1] hand-off words, kFoldEmpty
    // between launches like the slots and the item partials
    bool gfold = false;
    int fold_direct = 0;   // the final workgroup sums where the words land (LinArgs::fold_direct)
    int fold_dyn = 0;      // the groups take the reduction's tasks as they finish (LinArgs::fold_dyn)
    int fold_first = 0;    // MCC_FOLD_CONSUMERS_FIRST=1 (test): LinArgs::fold_first
    int max_item_slots = 0;
    int fault_photo = -1;            // MCC_FAULT_PHOTO (test): LinArgs::fault_photo
    int packed_len = 0, ntri = 0;    // the packed system [S upper | r | jte_g | normG2 | normX2], S's triangle
    int graph_sizes = kGraphSizes;   // MCC_GRAPH_SIZES (A/B of the launch granularity)
    bool use_graph = true;
};

struct Int4 { int x, y, z, w; };   // the device's int4, member for member

// The whole plan: the scalars and the host arrays mcc_create uploads (device order: photo-major).
struct Plan : PlanScalars {
    std::vector<float> obj_x, obj_y, obj_z, img_u, img_v;   // [corners] the five corner streams
    std::vector<Int4> info;           // [E] {cam, side, corner offset, n}
    std::vector<int> gblock;          // [E] global block of an edge or -1
    std::vector<int> ephoto;          // [E]
    std::vector<int> photo_ptr;       // [V + 1] edge ranges
    std::vector<int> photo_corner;    // [V + 1] corner ranges
    std::vector<int> pgrp_ptr, pgrp_edge;      // [n_pgroups + 1] first photo / first edge of each group
    std::vector<unsigned char> edge_lphoto;    // [max(E, 1)] an edge's photo within its group
    std::vector<int> ghdr;            // [max(n_pgroups, 1)][kGHdrInts]
    std::vector<double> kintr;        // [C][kGIntr]
    std::vector<double> tilt;         // [C][9] matTilt (prism == 2; empty otherwise)
    std::vector<int> gpair_ptr, gcon_ptr;      // [n_pgroups + 1]
    std::vector<Int4> gpairs;         // {first contribution (group-relative), count, diagonal << 1, slot offset}
    std::vector<unsigned> gcon;       // edge a | edge b << 8 | self << 16 | photo << 17 (group-local)
    std::vector<Int4> items;          // {block, first slot's offset, slots, slot size | kItemSingle}
    std::vector<int> block_items;     // [nblk + 1]
    std::vector<int> prep_ptr, prep_edge;      // [n_prep + 1] k_prep4's groups (three-kernel step; else empty)
    std::vector<float> cam_rt;        // [6C] DOUBLESIDE fixed cameras (rvec, tvec)
    std::vector<double> ds_rt;        // [6] PINHOLE doubleSideTransform (rvec, tvec)
    std::vector<double> alpha;        // [4096] 0.95^(k + 1)
    std::vector<int> dev2ref_edge;    // device edge -> reference edge
    std::vector<long long> dev2ref_corner;
    std::vector<int> edge_n_dev;      // [E] corners per device edge
};

// Every rejection that does not depend on the device: MCC_OK, or MCC_EINVAL with the message in *why.
int validate(const mcc_desc& d, std::string* why);

// The plan of a validated descriptor.  n_cu drives the path rules (MCC_CUS overrides it); n_cu_dev, the
// device's own count, the folded launch's progress rule and fold_dyn's residency rule, which concern
// what the hardware can hold at once.
int plan_problem(const mcc_desc& d, const Options& opt, int n_cu, int n_cu_dev, Plan* out, std::string* why);

// cvRodrigues2 matrix -> vector with the polar re-orthonormalisation (fixed transforms, once per problem)
void host_rodrigues_m2v(const double* R, double* r);
// computeTiltProjectionMatrix: the tilted-sensor model's matTilt, row-major
void tilt_matrix(double tx, double ty, double M[9]);

}  // namespace mcc
