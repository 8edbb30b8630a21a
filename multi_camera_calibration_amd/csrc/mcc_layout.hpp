// mcc_layout.hpp -- what the host planner (mcc_plan.cpp) and the kernels share: the sizes, strides and
// flags of the index structures mcc_create builds, and the LDS layouts both sides compute.  No HIP:
// it compiles under hipcc (through mcc_internal.h) and under a plain C++17 compiler.
#pragma once
#include <cstddef>

#if defined(__HIP__)   // (the compiler's own macro in HIP mode, where __host__ / __device__ exist)
#define MCC_HD __host__ __device__
#else
#define MCC_HD
#endif

namespace mcc {

// k_group's per-group header (ints, fixed stride): the group's ranges, the group-relative photo_ptr
// entries and the first round's edge records, so that phase 0 chases no index through memory
constexpr int kGHdrRange = 0;     // p0, np, ge0, gne, q0, nq, c0, nc
constexpr int kGHdrPhoto = 8;     // [kPhotoGroup + 1] photo_ptr[p0 + q] - ge0 (entries past np repeat gne)
constexpr int kGHdrInfo = 20;     // int4 [16] edge_info of the first round's edges (16-byte aligned)
constexpr int kGHdrGb = 84;       // [16] gblock
constexpr int kGHdrEq = 100;      // [16] edge_lphoto
constexpr int kGHdrInts = 128;    // stride (512 bytes)
constexpr long long kFoldEmpty = -1LL;

constexpr int kItemSingle = 256;   // k_schur item flag (in .w, over the slot size): the block's only item
constexpr int kPhotoGroup = 8;        // photos per k_photo workgroup, at most
constexpr int kPhotoGroupEdges = 64;  // edges per k_photo workgroup, at most
constexpr int kGroupRound = 16;       // edges per k_group round (4 waves x 4 edges x 16 lanes); its groups' cap
static_assert(kGHdrPhoto + kPhotoGroup + 1 <= kGHdrInfo && kGHdrInfo % 4 == 0 && kGHdrInfo + 4 * kGroupRound == kGHdrGb &&
                  kGHdrGb + kGroupRound == kGHdrEq && kGHdrEq + kGroupRound <= kGHdrInts,
              "k_group header layout");
// k_photo's LDS (doubles, then ints): per edge [Hgg upper 21 | pad | U 36 | gg 6] (64), per photo the
// Hpp / gp sums [28], Hpp's inverse Cholesky factor Li [36] and v [6]; then per edge gblock and
// photo (ints), the group's pairs (int4) and contributions (unsigned)
MCC_HD inline size_t photo_lds_doubles(int gne) {
    return (size_t)64 * gne + (size_t)70 * kPhotoGroup;
}
MCC_HD inline size_t photo_lds_bytes(int gne, int npairs, int ncon) {
    return photo_lds_doubles(gne) * 8 + 4 * (size_t)((2 * gne + 3) & ~3) + 16 * (size_t)npairs + 4 * (size_t)ncon;
}

// k_group (mcc_group.hpp): the fused split step's per-group LDS
constexpr int kGChunk = 96;       // corners of one edge staged in LDS at a time
constexpr int kGIntr = 28;        // k_group's LDS intrinsics row: fx fy cx cy skew xi k[12] matTilt[9] pad
constexpr int kGRecP = 40;        // k_group's per-edge sweep record: R 9 | T 3 | 6 intrinsics | k[12] | matTilt[9] | pad
constexpr int kGRec = 92;         // doubles per group edge: sE (64: Hgg upper 21 | pad | U 36 | gg 6)
                                  // + Hpp upper 21 | gp 6 | pad; the edge's prologue scratch meanwhile

// LDS layout of k_group (offsets in doubles; host and device share it)
struct GroupLayout {
    int rec, s27, sLi, sv, sph, sxn, spart, sdg, ctab, ktab, sds, sP, sGb, sU, ndoubles;
    int iInfo, iGb, iEq, iPh, iPq, iCn, nints;   // int offsets after the doubles
};
MCC_HD inline GroupLayout group_layout(int gne, int C, int nq, int nc) {
    GroupLayout L;
    L.rec = 0;
    L.s27 = L.rec + kGRec * gne;                // [8][28] per-photo Hpp upper 21 | gp 6 sums
    L.sLi = L.s27 + 28 * kPhotoGroup;           // [8][36] Li = L^-1 (Hpp = L L^T)
    L.sv = L.sLi + 36 * kPhotoGroup;            // [8][6]  v = Li gp
    L.sph = L.sv + 6 * kPhotoGroup;             // [8][24] R1 | Jr1 | T1 of the updated photo
    L.sxn = L.sph + 24 * kPhotoGroup;           // [8][16] x (6) | pad | G (6) | pad
    L.spart = L.sxn + 16 * kPhotoGroup;         // [gne][6] Y'_e^T dg partials of the photo update
    L.sdg = L.spart + 6 * gne;                  // [128] the previous solve's global-block delta
    L.ctab = L.sdg + 128;                       // [C][24] camera R | Jl | T
    L.ktab = L.ctab + 24 * C;                   // [C][kGIntr] fx fy cx cy skew xi k[12] matTilt[9]
    L.sds = L.ktab + kGIntr * C;                // [32] double-side transform Rds | Jrds | dst
    L.sP = L.sds + 32;                          // [16][kGRecP] sweep record: R | T | fx fy cx cy skew xi | k[12] | matTilt[9]
    L.sGb = L.sP + kGRecP * kGroupRound;        // [16][56] chain-map blocks [photo 27 | pad | global 27 | pad]
    L.sU = L.sGb + 56 * kGroupRound;            // per wave: corners [5][96][4] floats | chain {A 36, B 8, X 96} x 4
    L.ndoubles = L.sU + 4 * (5 * kGChunk * 4 / 2);
    L.ndoubles = (L.ndoubles + 1) & ~1;         // 16-B aligned int4 area
    L.iInfo = 0;                                // int4 [gne] {cam, side, corner offset, n}
    L.iGb = L.iInfo + 4 * gne;                  // [gne] global block
    L.iEq = L.iGb + gne;                        // [gne] group-local photo
    L.iPh = L.iEq + gne;                        // [kPhotoGroup + 1] group-relative first edge of each photo
    L.iPq = (L.iPh + kPhotoGroup + 1 + 3) & ~3; // int4 [nq] pair tasks
    L.iCn = L.iPq + 4 * nq;                     // [nc] contributions
    L.nints = L.iCn + nc;
    return L;
}
MCC_HD inline size_t group_lds_bytes(int gne, int C, int nq, int nc) {
    const GroupLayout L = group_layout(gne, C, nq, nc);
    return (size_t)L.ndoubles * 8 + (size_t)L.nints * 4;
}

// k_prep4 (mcc_group.hpp): one wave per group of consecutive photos, 4 lanes per edge prologue
constexpr int kPrepEdges = 16;            // edges per round (64 lanes / 4); the groups' edge cap
constexpr int kPrepPhotos = kPhotoGroup;  // photos per group, at most
struct PrepLayout {
    int tab, S, sdg, sxn, scam, ndoubles;   // doubles
    int iInfo, iGb, iPh, nints;             // ints after the doubles
};
// tab: Rodrigues tables (R 9, J 9, T 3, pad) of the photos [kPrepPhotos], cameras [C] and the
// double-side transform; S: per edge slot the prologue's scratch (84 doubles with back-side
// edges, else 42), aliased by the photo update's partial sums (<= 64 edges x 6)
MCC_HD inline PrepLayout prep_layout(int C, bool back) {
    PrepLayout L;
    int o = 0;
    L.tab = o; o += 24 * (kPrepPhotos + C + 1);
    L.S = o; o += kPrepEdges * (back ? 84 : 42);
    L.sdg = o; o += 128;
    L.sxn = o; o += 16 * kPrepPhotos;
    L.scam = o; o += 6 * C + 6;
    L.ndoubles = (o + 1) & ~1;
    int n = 0;
    L.iInfo = n; n += 4 * 64;
    L.iGb = n; n += 64;
    L.iPh = n; n += kPrepPhotos + 1;
    L.nints = n;
    return L;
}
MCC_HD inline size_t prep_lds_bytes(int C, bool back) {
    const PrepLayout L = prep_layout(C, back);
    return (size_t)L.ndoubles * 8 + (size_t)L.nints * 4;
}

// k_schur's dynamic LDS (doubles): the final arriver's S (m x m) and r (m) when the launch solves
// (fuse_solve), the m <= 30 warm solve's inverse (m x m, ssinv), and with one hand-off level the copy
// of every workgroup's partials (48 per item or norm chunk, grid) followed by the block ranges (nblk + 1
// ints) -- all of them loaded in one round trip
MCC_HD inline size_t schur_items_offset(int m, int fuse, int ssinv) {
    return fuse ? (size_t)m * m + m + (ssinv ? (size_t)m * m : 0) : 0;
}
MCC_HD inline size_t schur_lds_bytes(int m, int fuse, int ssinv, int one_level, int grid, int nblk) {
    size_t d = schur_items_offset(m, fuse, ssinv);
    if (one_level) d += 48 * (size_t)grid + (nblk + 2) / 2;
    return d * sizeof(double);
}
// one hand-off level only while the final arriver's copy is one batch of loads: 48 grid + m^2 <=
// kSchurOneLevelLoads x 256 (k_schur's threads)
constexpr int kSchurOneLevelLoads = 16;

}  // namespace mcc
