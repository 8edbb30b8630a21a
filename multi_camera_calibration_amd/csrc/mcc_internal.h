// mcc_internal.h -- device state and kernel argument blocks shared by mcc_kernels.hip and
// mcc_api.cpp.  Not part of the public ABI (include/mcc.h).  The constants and LDS layouts that the
// host planner shares with the kernels are in mcc_layout.hpp (no HIP), included here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/mcc.h"
#include "mcc_layout.hpp"

namespace mcc {

constexpr int kStampStride = 32;   // MCC_DIAG: s_memtime / s_memrealtime slots per k_linearize workgroup
constexpr int kSchurStampStride = 16;   // MCC_DIAG: slots per k_schur workgroup (after k_linearize's rows)

// Device-resident loop state of optimizeExtrinsics (src/multicalib.cpp:468-507).
struct State {
    int iter;         // completed updates k
    int done;         // stop test fired
    int crit_type;    // 0 = never stop (bench / linearize-only), 1 COUNT, 2 EPS, 3 COUNT+EPS
    int max_count;
    double eps;
    double change;    // ||G|| / ||x|| of the last update
    double alpha;     // 0.95^(k+1) of the running step
    double cam_normG2, cam_normX2;   // global-block partials of the last update
    int error;        // kErr* bits below
    int pending;      // a solved photo update waits to be applied by the next k_linearize
    unsigned int epoch;   // peer exchanges completed (monotonic over the problem's life)
    long long xchg_ticks; // s_memrealtime ticks (100 MHz) inside peer exchanges, summed (monotonic)
    // the fused step's m <= 30 warm solve (k_linearize's spare workgroup, small_inverse): the spare's
    // acknowledgement of an update launch -- iter + 1 once it holds the launch's inputs (state words,
    // the packed system) in LDS; the launch's final arriver writes neither the packed system nor the
    // state before it has seen it.  Update launches of one optimisation have distinct iter, and
    // set_state clears the word (no launch in flight), so an acknowledgement is never a stale one.
    unsigned int spare_ack;
};
// State::error bits
constexpr int kErrPhotoNotPD = 1;    // a photo's 6 x 6 block (any rank: summed through the exchange)
constexpr int kErrCameraNotPD = 2;   // the reduced camera system
constexpr int kErrPeerTimeout = 4;   // a peer did not deliver its system
constexpr int kErrWarmTimeout = 8;   // the warm-solve helper did not deliver the previous inverse, or
                                     // the fused step's spare did not acknowledge its inputs

// Peer transport (multi-GPU without RCCL in the step): every rank's final arriver writes its packed
// reduced system straight into every peer's inbox over xGMI, then sums all ranks' systems in rank
// order.  LL format (the RCCL low-latency protocol's idea): each 8-B word carries 32 data bits and
// the 32-bit epoch of the exchange, so a reader needs no cross-device ordering or fence, only the
// 8-B single-copy atomicity of an aligned store.  Inbox: [2 slots (epoch parity)][nranks][2 Lc]
// words in uncached device memory; peers[q] is rank q's inbox mapped into this process (IPC).
struct PeerCtx {
    unsigned long long* inbox;
    unsigned long long* const* peers;   // [nranks] device array (peers[rank] == inbox)
    int nranks;                         // 0: transport off
    int rank, Lc;
    long long timeout;                  // s_memrealtime ticks (100 MHz)
};

struct SolveCtx {
    State* state;
    const double* alpha; int n_alpha;
    float* x;
    double* dg;       // [m]
    double* delta;    // [P]
    int m, do_update;
    long long* stamps;   // MCC_DIAG: solve phase stamps (set by k_schur's last arriver)
    // m <= 30 warm-solve statistics (mcc_solve_stats, the m > 30 helper's layout): refinements tried,
    // corrections, refinements that fell back to the elimination, eliminations without an inverse,
    // fused steps whose final arriver waited for the spare.  Null unless MCC_SOLVE_STATS=1: the
    // counters' atomics at the end of the solving workgroup cost ~0.5 us per config2 step
    long long* sstats;
};

struct SchurArgs {
    State* state;
    const int4* items;   // {camera-pair block, first slot's offset in doubles, slot count, slot size 48 | 36}
    const double* pairprod;   // 48 (diagonal block) or 36 doubles per slot, written by k_photo, block-major
    double* item_out;    // [48 * (items + norm chunks)]
    int n_items;
    const double* photo_norm; int n_photos;
    int* counter;        // level-2 ticket over blocks + norm chunks (zero between launches)
    int* cnt_blk;        // [nblk] level-1 tickets: the last item of a camera-pair block sums it
    int nblk;
    const int* block_items;   // [nblk + 1]
    double* packed;
    int m, rank, fuse_solve;
    int one_level;       // m <= 30: one hand-off level (schur_one_level) instead of items -> blocks -> norms
    const double* ssinv; // m <= 30 warm solve: [2][m x m], this step's in buffer iteration & 1 (k_group's spare)
    const int* ssinv_ok; // [2] tags (iteration + 1)
    SolveCtx solve;
    long long* stamps;   // MCC_DIAG builds: [8 * grid]
    PeerCtx peer;        // nranks > 0 (m <= 30, peer transport): the final arriver exchanges, then solves
    double* prev2;       // m > 30 warm solve: [2][prev_stride] copy of [S | r] for the helper (null: off)
    int prev_stride;
    unsigned* wpub;      // m > 30, the helper refines (WarmCtx::refine): k_schur publishes the system
                         // (sync[0] = iteration + 1) when it starts and empties the other prev2 buffer
    int wpub_early;      // (the helper polls prev2's words as they land: the three-kernel step), or with 0
                         // its final arriver once prev2 is complete (k_group's step: mcc_create)
};

struct LinArgs {
    State* state;
    const int* photo_ptr;     // [V+1] photo-major edge ranges
    const int* photo_corner;  // [V+1] photo-major corner ranges (corners of a photo are contiguous)
    int max_cpp;              // most corners of one photo (LDS staging)
    const int4* edge_info;    // [E] {cam, side, corner_off, n}
    const float* obj_x; const float* obj_y; const float* obj_z;   // [corners] photo-major
    const float* img_u; const float* img_v;
    float* x;                 // [P] float32 parameters [global m | photos] (photo part updated in place)
    const float* K; const float* D; const float* xi;
    const double* tilt;       // [C][9] the tilted-sensor matTilt (nd = 14, tau != 0; null otherwise)
    const float* cam_rt;      // DOUBLESIDE fixed cameras (rvec, tvec) [6C]
    const double* ds_rt;      // PINHOLE doubleSideTransform (rvec, tvec) [6]
    int nd, global_dim, n_cams, has_back;
    // outputs
    double* Y;        // [36E] Schur factors Y'_e = Hgp_e Hpp^-1
    // split step: k_photo runs over groups of consecutive photos (<= kPhotoGroup photos and
    // <= kPhotoGroupEdges edges); each group sums its photos' Schur pair products per camera-pair
    // block and writes them at that block's slot (block-major over the groups; k_schur sums them)
    const int* pgrp_ptr;     // [n_pgroups + 1] first photo of each group
    const int* pgrp_edge;    // [n_pgroups + 1] first edge of each group (photo_ptr[pgrp_ptr[g]])
    const unsigned char* edge_lphoto;   // [E] an edge's photo within its group (0 .. kPhotoGroup - 1)
    const int* gpair_ptr;    // [n_pgroups + 1] ranges of gpairs
    const int4* gpairs;      // {first contribution (group-relative), count, diagonal block << 1, slot offset}
    const int* gcon_ptr;     // [n_pgroups + 1] ranges of gcon
    const unsigned* gcon;    // contribution: edge a | edge b << 8 | self << 16 | photo << 17 (group-local)
    double* pairprod;        // per slot {S_ab entries (36), [diagonal block] r_a (6), JTE_a (6)}
    int n_pgroups, max_gpairs, max_gcon, max_gedges;
    double* zp;       // [6V] z' = Hpp^-1 gp
    double* gp_tot;   // [6V] photo JTE
    float* resid;     // optional [2*corners] float32 residuals (debug)
    // pending update of the previous step (fused back-substitution)
    const int* gblock;       // [E] global block of an edge or -1
    const double* dg;        // [m] global-block delta of the previous solve
    double* photo_norm;      // [2V] ||G||^2, ||x||^2 partials of the applied update
    long long* stamps;       // MCC_DIAG builds: [16V] s_memtime per phase
    // fused single-kernel step (m <= 30): every photo writes its packed contribution
    // [S upper | r | jte_g | normG2 | normX2], a fixed-order two-level last-arriver reduction sums
    // them (groups of group_size consecutive photos, then the groups), and the final arriver
    // solves (fuse_solve) or leaves the packed system for the all-reduce + k_solve
    int fused, group_size, n_groups, rank, fuse_solve;
    double* contrib;         // [V * Lc]
    double* gsum;            // [n_groups * Lc]
    int* cnt;                // [n_groups + 1] tickets, zero between launches
    double* packed;          // [Lc]
    double* W;               // [V * 6m] per-photo pending-update matrix (next step's phase 0)
    SolveCtx solve;
    PeerCtx peer;            // nranks > 0: the final arriver exchanges with the peers and solves
    // split step (m > 30): k_prep -> k_edge -> k_photo
    int n_edges, n_photos;
    double* erec;            // [12E] R (9), T (3) of the float32 composed pose (k_prep -> k_edge)
    double* echain;          // [54E] chain-map blocks Gp11, Gp21, Gp22, Gg11, Gg21, Gg22 (k_prep -> k_edge)
    double* eh;              // [90E] Hpp upper (21), Hgg upper (21), Hgp (36), gp (6), gg (6) (k_edge -> k_photo)
    // k_prep4: groups of consecutive photos (<= kPrepPhotos photos and kPrepEdges edges, or one photo)
    const int* prep_ptr;     // [n_prep + 1] first photo of each group
    const int* prep_edge;    // [n_prep + 1] first edge of each group
    int n_prep, prep_lanes;  // prep_lanes: 4 (k_prep4) or 1 (k_prep, one lane per edge)
    int fault_photo;         // test (MCC_FAULT_PHOTO): this local photo's 6 x 6 block is reported not
                             // positive definite (its factor stays finite); -1 off
    // m <= 30 warm solve: k_group's spare workgroup inverts the previous step's packed system
    int fold_first;          // test layout (MCC_FOLD_CONSUMERS_FIRST=1): the spare and the folded reduction's
                             // workgroups take the LOWEST grid indices, the groups the rest -- the
                             // progress invariant must not rest on dispatch order (mcc_create); (placed
                             // in fault_photo's padding: a shifted LinArgs tail cost k_group SGPR spills)
    double* ssinv;           // [2][m x m] by iteration parity (null: off)
    int* ssinv_ok;           // [2] the iteration + 1 whose spare workgroup formed the buffer (0: none)
    // the fused step's spare: its wait bound at the final arriver (s_memrealtime ticks; past it the
    // step fails with kErrWarmTimeout), and a test delay before it reads anything (MCC_SPARE_DELAY_US)
    long long spare_wait, spare_delay;
    // k_group with the step's reduction and solve folded into the same launch (gfold: m <= 30, one
    // hand-off level): after the groups (and the spare) the grid holds fsa.n_items item workgroups,
    // the norm chunks (fold_parts in all) and one final workgroup.  The hand-off words are their own
    // flags: every slot, norm partial, item partial and the spare's inverse holds kFoldEmpty (all-ones,
    // a NaN no arithmetic produces) until its producer's sc1 store lands, and its consumer puts
    // kFoldEmpty back after reading it -- no store drain, ticket or fence on either side.
    int fold, fold_parts;
    int fold_direct;          // the final workgroup sums where the words land (fold_final_direct)
    int fold_dyn;             // the groups take the reduction's tasks by ticket as they finish (no
                              // trailing workgroups: those waited for a CU until the groups ended)
    int* fold_ticket;         // fold_dyn: the tasks' ticket (the last of the n_pgroups takers resets it)
    SchurArgs fsa;            // the reduction (k_schur's arguments: items, slots, partials, packed, solve)
    double* fnorm;            // [4V] per photo ||G||^2, ||x||^2, not-PD flag, pad (the norm chunks' input)
    double* fiv;              // [m^2 + 1] the spare's inverse and its status, +-(iteration + 1) as a double
    // k_group's phase 0 (built once in mcc_create; the topology and the intrinsics never change)
    const int* ghdr;          // [n_pgroups][kGHdrInts] per-group header (kGHdr*, mcc_layout.hpp)
    const double* kintr;      // [C][kGIntr] the cameras' intrinsics rows, the kernel's LDS layout in FP64
};

// k_group's kernel parameters are (the members of GroupLead, one parameter each; LinArgs; GroupHot).
// The leading ones are what the role dispatch (spare / group / item / chunk / final) tests: as
// separate pointer and int parameters at the front of the argument segment they can be preloaded into
// SGPRs at wave start (a struct passed by value is not), so the dispatch waits for no load.  The block
// is padded to 64 bytes: LinArgs, which the other kernels share, keeps its layout and its alignment
// modulo 64 within the segment.
constexpr unsigned kGLeadSsinv = 1u, kGLeadFold = 2u, kGLeadFoldDyn = 4u, kGLeadFoldDirect = 8u;
constexpr int kGLeadPreload = 6;   // the parameters ahead of the padding (8 SGPRs)
struct GroupLead {
    State* state;
    const int* ghdr;
    int n_pgroups;
    unsigned flags;       // kGLead*: ssinv != null, fold, fold_dyn, fold_direct (the last is carried
                          // for the dispatch word's completeness only: no role tests it, the final
                          // workgroup reads LinArgs::fold_direct with the rest of its arguments)
    int n_items;          // fsa.n_items
    int fold_parts;
    long long pad[4];
};
static_assert(sizeof(GroupLead) == 64 && sizeof(GroupLead) % alignof(LinArgs) == 0,
              "k_group: LinArgs follows the leading block at byte 64 of the argument segment");
inline GroupLead group_lead(const LinArgs& a) {
    return {a.state, a.ghdr, a.n_pgroups,
            (a.ssinv ? kGLeadSsinv : 0u) | (a.fold ? kGLeadFold : 0u) | (a.fold_dyn ? kGLeadFoldDyn : 0u) |
                (a.fold_direct ? kGLeadFoldDirect : 0u),
            a.fsa.n_items, a.fold_parts, {0, 0, 0, 0}};
}
// What a group's phase 0 dereferences, contiguous behind LinArgs: the group path reads the block with
// the state words and the header's ranges in ONE scalar round trip at its entry (mcc_group.hpp).
// Every member is the LinArgs field of the same name (group_hot).
struct GroupHot {
    const int4* gpairs;
    const unsigned* gcon;
    const double* dg;
    const double* kintr;
    float* x;
    const float* cam_rt;
    const double* ds_rt;
    double* zp;
    double* photo_norm;
    const int* gblock;
    double* Y;
    const float* obj_x; const float* obj_y; const float* obj_z;
    const float* img_u; const float* img_v;
    long long* stamps;
    // (the later phases' and the cold loops': read here too, or the compiler hoists their loads, and
    // a wait for them, into phase 0's vector batch)
    const int4* edge_info;
    const unsigned char* edge_lphoto;
    double* gp_tot;
    float* resid;
    int global_dim, n_cams;
};
inline GroupHot group_hot(const LinArgs& a) {
    return {a.gpairs, a.gcon, a.dg, a.kintr, a.x, a.cam_rt, a.ds_rt, a.zp, a.photo_norm, a.gblock, a.Y,
            a.obj_x, a.obj_y, a.obj_z, a.img_u, a.img_v, a.stamps, a.edge_info, a.edge_lphoto, a.gp_tot, a.resid,
            a.global_dim, a.n_cams};
}
// k_group's parameter list, ONE definition: the kernel is declared with it (mcc_group.hpp asserts its
// type against GroupKernelFn), and the byte offsets at which the kernel reads LinArgs and GroupHot
// from its argument segment (kernarg_at) are computed from this very list, each parameter at its
// natural alignment as the code object lays them out.  A parameter added, dropped or reordered moves
// the offsets with it, or fails one of the assertions below.
using GroupKernelFn = void (*)(State*, const int*, int, unsigned, int, int, long long, long long, long long, long long,
                               LinArgs, GroupHot);
template <class T, class U> struct GSame { static constexpr bool v = false; };
template <class T> struct GSame<T, T> { static constexpr bool v = true; };
template <class T, class... P>
constexpr int kernarg_offset_of(void (*)(P...)) {   // of the first parameter of type T; -1: none
    const size_t sz[] = {sizeof(P)...}, al[] = {alignof(P)...};
    const bool is[] = {GSame<T, P>::v...};
    size_t off = 0;
    for (size_t i = 0; i < sizeof...(P); ++i) {
        off = (off + al[i] - 1) / al[i] * al[i];
        if (is[i]) return (int)off;
        off += sz[i];
    }
    return -1;
}
constexpr int kGArgLin = kernarg_offset_of<LinArgs>(GroupKernelFn(nullptr));
constexpr int kGArgHot = kernarg_offset_of<GroupHot>(GroupKernelFn(nullptr));
// the same list as a struct (what the host test and the launch function's helpers describe)
struct GroupKernarg {
    GroupLead lead;
    LinArgs a;
    GroupHot hot;
};
static_assert(kGArgLin == (int)offsetof(GroupKernarg, a) && kGArgLin == (int)sizeof(GroupLead) && kGArgLin % 64 == 0,
              "k_group: LinArgs follows the 64-byte leading block");
static_assert(kGArgHot == (int)offsetof(GroupKernarg, hot) && kGArgHot == kGArgLin + (int)sizeof(LinArgs),
              "k_group: GroupHot follows LinArgs without padding");
static_assert(kernarg_offset_of<unsigned>(GroupKernelFn(nullptr)) == (int)offsetof(GroupLead, flags) &&
                  kernarg_offset_of<long long>(GroupKernelFn(nullptr)) == (int)offsetof(GroupLead, pad),
              "k_group: the leading parameters lie as GroupLead's members do");

// The m > 30 solve with the previous step's inverse (the "warm" solve, solve_large in
// mcc_kernels.hip): a resident helper kernel on a side stream (k_sinv_helper) inverts each update
// step's reduced system while the next step linearises; the next k_solve solves its own system by
// iterative refinement preconditioned with that inverse and falls back to the direct elimination
// when the refinement does not converge within kWarmMaxIters corrections.  sinv_ok_sys, sprev and
// sync are uncached device memory (the helper and the k_solve launches hand them over while both
// run); sinv is ordinary memory, written back by the helper (agent release) before its epoch.
// The system itself reaches the helper through prev2: k_schur writes [S | r] to prev2[iter & 1] beside
// the packed system (one more write-through store per entry, spread over the block workgroups), and
// k_solve publishes the epoch e + 1 (iteration e solved) as soon as it holds S_t^-1 in LDS -- no copy
// or store drain of its own.  The double buffer is safe: the step that writes prev2[iter & 1] again
// starts after the next k_solve, which waited for the helper to invert (and so to read) this one.
// Which algorithm a step takes depends only on the systems (the epoch count, the helper's PD flag,
// the refinement's convergence), never on timing: k_solve always waits for the previous system's
// inverse, and a helper that does not deliver within wait_ticks fails the step (error bit 3,
// MCC_ETIMEOUT) instead of switching to the direct elimination.
struct WarmCtx {
    double* sinv;            // [M x M] (M = 16 ceil(m / 16), row-major) the helper's inverse
    int* sinv_ok_sys;        // the helper's elimination found the system positive definite
    double* prev2;           // [2][prev_stride] uncached: the copy of [S | r] per iteration parity
    int prev_stride;         // packed [S | r] rounded up to even
    int copy_prev;           // 1: k_solve writes the copy (sharded: the rank-summed system exists only
                             // after the exchange); 0: k_schur wrote it (single GPU)
    unsigned* sync;          // [8] epochs: systems published (k_solve; refine: k_schur), systems inverted by the
                             // helper; stop; PD; refine: the epoch the helper refined, its status (0 no
                             // inverse, 1 converged, 2 not), its corrections
    long long* stats;        // [5] warm solves, corrections, fallbacks, direct (no inverse yet), waited for the helper
    int poison;              // test (MCC_WARM_POISON=1): the helper publishes a NaN inverse, so every
                             // warm solve must fall back to the direct elimination
    long long wait_ticks;    // k_solve's bound on the wait for the helper (s_memrealtime, 100 MHz)
    long long idle_ticks;    // the helper exits after this long without a new system (a safety net: the
                             // batch's k_solves publish or raise the stop flag, and the host launches the
                             // helper only after the batch's graphs exist)
    long long delay_ticks;   // test (MCC_WARM_DELAY_US): the helper holds each inverse back this long
    int refine;              // single GPU (MCC_HELPER_REFINE): the helper refines with the inverse it holds in
                             // LDS and publishes x (xsol); k_solve only waits for it (or eliminates)
    double* xsol;            // refine: [kWarmN] uncached, the helper's solution of the published system
    int poll;                // refine: k_schur publishes at its start and the helper polls prev2's words
                             // (SchurArgs::wpub_early), else one batch once the system is complete
    long long* hst;          // MCC_DIAG builds: the helper's phase stamps, [4 systems][16] (null otherwise)
    int inv_la;              // the helper inverts with the look-ahead schedule (gj_inverse_blocked<true>)
};
constexpr int kWarmMaxIters = 4;

struct SolveArgs {
    SolveCtx ctx;
    double* packed;
    PeerCtx peer;            // nranks > 0: exchange the packed system with the peers first
    int pushed;              // k_peer_push already sent this rank's system (k_solve only receives)
    WarmCtx warm;            // m > 30: sync == null -> the direct elimination
};

struct BacksubArgs {
    const State* state;
    const int* photo_ptr;
    const int* gblock;
    const double* Y; const double* zp; const double* dg;
    const double* W;         // fused path: per-photo pending-update matrix (else nullptr: Y)
    float* x;
    double* delta;
    double* photo_norm;
    int n_photos, m, do_update;
};

struct ErrArgs {
    const int4* edge_info;
    const int* edge_photo;
    const float* obj_x; const float* obj_y; const float* obj_z;
    const float* img_u; const float* img_v;
    const float* x;
    const float* K; const float* D; const float* xi;
    const double* tilt;      // [C][9] matTilt (null: no tilt)
    const float* cam_pose;   // DOUBLESIDE [16C]
    float* edge_sum;         // [E] device order
    float* corner_err;       // optional [corners] device order: each corner's float32 L2 error
    int nd, m;
};

}  // namespace mcc

// launch wrappers (mcc_kernels.hip)
size_t mcc_lin_shmem(int max_edges_per_photo, int n_cams, int m, int max_cpp);
size_t mcc_solve_shmem(int m);
hipError_t mcc_set_kernel_attrs(int max_epp, int n_cams, int m, int max_cpp, size_t photo_shmem, size_t group_shmem);
hipError_t mcc_launch_group(const mcc::LinArgs& a, int model, bool rational, int prism, int lanes,
                            size_t group_shmem, hipStream_t s);
hipError_t mcc_launch_split(const mcc::LinArgs& a, int model, bool rational, int prism, size_t photo_shmem,
                            hipStream_t s);
hipError_t mcc_launch_linearize(const mcc::LinArgs& a, int model, int n_photos, int max_epp, bool rational, int prism, hipStream_t s);
hipError_t mcc_launch_schur(const mcc::SchurArgs& a, int grid, hipStream_t s);
hipError_t mcc_launch_solve(const mcc::SolveArgs& a, hipStream_t s);
hipError_t mcc_launch_peer_push(const mcc::PeerCtx& pc, const mcc::State* st, const double* vals, hipStream_t s);
hipError_t mcc_launch_debug_solve(const double* packed, double* x, int m, int* err, long long* stamps, hipStream_t s);
hipError_t mcc_launch_sinv_helper(const mcc::WarmCtx& w, int m, int n_systems, hipStream_t s);
hipError_t mcc_launch_backsub(const mcc::BacksubArgs& a, hipStream_t s);
hipError_t mcc_launch_delay(long long ticks, hipStream_t s);
hipError_t mcc_launch_peer_handshake(const mcc::PeerCtx& pc, mcc::State* st, double* out, hipStream_t s);
hipError_t mcc_launch_peer_max(const mcc::PeerCtx& pc, mcc::State* st, double* v, hipStream_t s);
hipError_t mcc_launch_project_error(const mcc::ErrArgs& a, int model, int n_edges, bool rational, int prism, hipStream_t s);
