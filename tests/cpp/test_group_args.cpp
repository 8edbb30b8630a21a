// k_group's kernel arguments (csrc/mcc_internal.h): the leading block is 64 bytes and LinArgs follows
// it at a 64-byte multiple; group_lead packs the role dispatch's words; group_hot fills every pointer
// from the LinArgs field of the same name.  Host only (compiled against the HIP headers, no device).
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "mcc_internal.h"

using namespace mcc;

// the kernel's parameter list as one struct: the argument segment's layout
struct FlatKernarg {
    State* state; const int* ghdr; int n_pgroups; unsigned flags; int n_items; int fold_parts;
    long long pad0, pad1, pad2, pad3;
    LinArgs a;
    GroupHot hot;
};
static_assert(sizeof(GroupLead) == 64, "the leading block is 64 bytes");
static_assert(kGArgLin == (int)offsetof(FlatKernarg, a) && kGArgHot == (int)offsetof(FlatKernarg, hot),
              "the offsets the kernel reads at are those of its parameter list");
static_assert(offsetof(GroupLead, pad) == 32 && kGLeadPreload == 6, "six preloaded parameters in 8 dwords");
static_assert(offsetof(FlatKernarg, a) == sizeof(GroupLead) && offsetof(FlatKernarg, a) % 64 == 0,
              "LinArgs follows the leading block at a 64-byte multiple");
static_assert(offsetof(FlatKernarg, hot) == sizeof(GroupLead) + sizeof(LinArgs), "GroupHot follows LinArgs");
static_assert(offsetof(FlatKernarg, state) == offsetof(GroupLead, state) && offsetof(FlatKernarg, ghdr) == offsetof(GroupLead, ghdr) &&
                  offsetof(FlatKernarg, n_pgroups) == offsetof(GroupLead, n_pgroups) &&
                  offsetof(FlatKernarg, flags) == offsetof(GroupLead, flags) &&
                  offsetof(FlatKernarg, n_items) == offsetof(GroupLead, n_items) &&
                  offsetof(FlatKernarg, fold_parts) == offsetof(GroupLead, fold_parts),
              "separate parameters lie as GroupLead's members do");

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

int main() {
    LinArgs a;
    std::memset(&a, 0, sizeof a);
    // a distinct fake address per LinArgs pointer: its own byte offset within LinArgs, plus a base
    char* base = reinterpret_cast<char*>(0x10000);
#define FAKE(f) a.f = reinterpret_cast<decltype(a.f)>(base + offsetof(LinArgs, f))
    FAKE(gpairs); FAKE(gcon); FAKE(dg); FAKE(kintr); FAKE(x); FAKE(cam_rt); FAKE(ds_rt); FAKE(zp); FAKE(photo_norm);
    FAKE(gblock); FAKE(Y); FAKE(obj_x); FAKE(obj_y); FAKE(obj_z); FAKE(img_u); FAKE(img_v); FAKE(stamps);
    FAKE(edge_info); FAKE(edge_lphoto); FAKE(gp_tot); FAKE(resid);
    FAKE(state); FAKE(ghdr); FAKE(K); FAKE(D); FAKE(xi); FAKE(photo_ptr); FAKE(pairprod); FAKE(W);
    a.global_dim = 24; a.n_cams = 5; a.n_pgroups = 250; a.fold_parts = 37; a.fsa.n_items = 21;
    const GroupHot h = group_hot(a);
#define SAME(f) CHECK(reinterpret_cast<const char*>(h.f) == base + offsetof(LinArgs, f))
    SAME(gpairs); SAME(gcon); SAME(dg); SAME(kintr); SAME(x); SAME(cam_rt); SAME(ds_rt); SAME(zp); SAME(photo_norm);
    SAME(gblock); SAME(Y); SAME(obj_x); SAME(obj_y); SAME(obj_z); SAME(img_u); SAME(img_v); SAME(stamps);
    SAME(edge_info); SAME(edge_lphoto); SAME(gp_tot); SAME(resid);
    CHECK(h.global_dim == 24 && h.n_cams == 5);
    // every byte of GroupHot is one of the above: 21 pointers and 2 ints
    CHECK(sizeof(GroupHot) == 21 * sizeof(void*) + 2 * sizeof(int));

    GroupLead l = group_lead(a);
    CHECK(reinterpret_cast<const char*>(l.state) == base + offsetof(LinArgs, state));
    CHECK(reinterpret_cast<const char*>(l.ghdr) == base + offsetof(LinArgs, ghdr));
    CHECK(l.n_pgroups == 250 && l.n_items == 21 && l.fold_parts == 37 && l.flags == 0);
    for (unsigned m = 0; m < 16; ++m) {   // every combination of the four role flags
        a.ssinv = (m & 1) ? reinterpret_cast<double*>(base) : nullptr;
        a.fold = (m >> 1) & 1; a.fold_dyn = (m >> 2) & 1; a.fold_direct = (m >> 3) & 1;
        l = group_lead(a);
        CHECK(l.flags == (((m & 1) ? kGLeadSsinv : 0u) | ((m & 2) ? kGLeadFold : 0u) | ((m & 4) ? kGLeadFoldDyn : 0u) |
                          ((m & 8) ? kGLeadFoldDirect : 0u)));
    }
    CHECK(kGLeadSsinv != kGLeadFold && kGLeadFold != kGLeadFoldDyn && kGLeadFoldDyn != kGLeadFoldDirect);
    std::printf(fails ? "%d checks failed\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
