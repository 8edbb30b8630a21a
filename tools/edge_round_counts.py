#!/usr/bin/env python3
"""Static instruction counts of k_group's edge round from a device-only assembly listing (CPU only):

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -DMCC_PART=3 --cuda-device-only -S \
        multi_camera_calibration_amd/csrc/mcc_kernels.hip -o part3.s
    python3 tools/edge_round_counts.py part3.s [mangled-name substring] [--hist]

The default kernel is the omnidirectional one at 32 lanes per edge (config4's).  Regions, in the
listing's own order (blocks the compiler moved behind the kernel's end, the cold loops, are not counted):
  prologue   from the third s_barrier (the end of phase 0) to the head of the sweep loop
  sweep      the loop body: the innermost loop with the most FP64 instructions
  chain      from the sweep loop's end to the next s_barrier (butterfly, record scatter, chain)
Per region: VALU instructions, the FP64 ones among them, moves, selects and the remaining (integer,
address, lane-crossing) VALU; --hist adds the FP64 opcode histogram, which a bit-neutral change must
leave equal.  The kernel's VGPR count and SGPR spill count come from the listing's metadata.

    python3 tools/edge_round_counts.py part3.s [mangled-name substring] --entry [listing.txt]

counts the scalar loads and waits of the kernel's entry and of phase 0's vector batch instead (entry()).

    python3 tools/edge_round_counts.py part3.s [mangled-name substring] --photo

counts the photo phase that follows the rounds, up to the group's last slot store (photo())."""
import collections
import re
import sys

DEFAULT = "k_groupILi1ELb0ELi0ELb0ELi32ELb0E"


def kernel_text(lines, pat):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(pat) + r"\S*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def op_of(line):
    t = line.split(";")[0].strip()
    if not t or t.endswith(":") or t.startswith("."):
        return None
    return t.split()[0]


def classify(ops):
    c = collections.Counter()
    for o in ops:
        if not o.startswith("v_"):
            continue
        c["valu"] += 1
        if "_f64" in o:
            c["fp64"] += 1
        elif o.startswith("v_mov_b") or o.startswith("v_accvgpr"):
            c["mov"] += 1
        elif o.startswith("v_cndmask"):
            c["select"] += 1
        elif "permlane" in o or "readlane" in o or "writelane" in o or "readfirstlane" in o or "_dpp" in o:
            c["lane"] += 1
        else:
            c["other"] += 1
    return c


def entry(k, lines, pat, out):
    """--entry [listing.txt]: the scalar side of the kernel's entry and of phase 0's vector batch.  Regions,
    in the listing's order: 'entry' from the kernel's first line to its first global_load, 'batch' from
    there to the end of the first round's corner loads (the second sched_barrier after it).  Counts
    s_load and s_waitcnt lines only (every path the compiler laid out in the region, the other roles'
    dispatch included); listing.txt gets the region's loads, waits, branches, labels and LDS stores up to
    the first s_barrier with their line numbers (profiles/group_phase0's format)."""
    ops = [op_of(l) for l in k]
    first = next(i for i, o in enumerate(ops) if o and o.startswith("global_load"))
    sb = [i for i in range(first, len(k)) if "sched_barrier" in k[i]]
    bar = next(i for i, o in enumerate(ops) if o == "s_barrier")
    end = sb[1] if len(sb) > 1 and sb[1] < bar else bar
    print(f"kernel {pat}: first global_load at line {first + 1}, the batch ends at line {end + 1}, first s_barrier at {bar + 1}")
    print(f"{'region':8s} {'s_load':>7s} {'s_waitcnt lgkmcnt':>18s} {'global_load':>12s} {'s_waitcnt vmcnt':>16s} {'branches':>9s}")
    for name, a, b in (("entry", 0, first), ("batch", first, end)):
        r = [(o, k[i]) for i, o in enumerate(ops[a:b], a) if o]
        print(f"{name:8s} {sum(o.startswith('s_load') for o, _ in r):7d} "
              f"{sum(o == 's_waitcnt' and 'lgkmcnt' in l for o, l in r):18d} "
              f"{sum(o.startswith('global_load') for o, _ in r):12d} "
              f"{sum(o == 's_waitcnt' and 'vmcnt' in l for o, l in r):16d} "
              f"{sum(o.startswith(('s_cbranch', 's_branch')) for o, _ in r):9d}")
    meta = "\n".join(lines)
    for key in ("num_vgpr", "private_seg_size"):
        m = re.search(re.escape(pat) + r"\S*\." + key + r", (\d+)", meta)
        if m:
            print(key, m.group(1))
    for key in ("amdhsa_user_sgpr_kernarg_preload_length", "sgpr_spill_count"):
        m = re.search(re.escape(pat) + r".*?" + key + r":?\s+(\d+)", meta, re.S)
        if m:
            print(key, m.group(1))
    if out:
        keep = re.compile(r"^\s+(s_load|s_waitcnt|s_cbranch|s_branch|global_load|ds_write|s_barrier|s_endpgm|; sched_barrier)|^\.LBB")
        with open(out, "w") as f:
            for i, l in enumerate(k[:bar + 1]):
                if keep.match(l):
                    f.write(f"{i + 1}:{l.split(';')[0].rstrip() if not l.strip().startswith(';') else l}\n")


def photo(k, lines, pat):
    """--photo: the photo phase, from the barrier that ends the rounds (the fourth s_barrier) to the group
    path's last slot store: the last write-through (sc1) global store between the barrier behind U, Y'
    (the seventh) and the next one.  In the listing's own order, as the other modes: a block the
    compiler laid out inside the region counts whether or not the 32-lane shapes take it, so every wait
    and scalar load is printed with its line and the label it stands under, for the reader to place."""
    ops = [op_of(l) for l in k]
    bars = [i for i, o in enumerate(ops) if o == "s_barrier"]
    assert len(bars) > 7, "k_group has at least eight barriers"
    b0, b3 = bars[3], bars[6]
    # task loops: the outermost loops (backward branches) with a global store in their body.  Where the
    # task loops start at the thread's own index they are the first pass and the tasks' only copy;
    # where the first pass stands outside as `if (tid < n) task(tid)`, they are the cold passes after it
    labels = {l.split(":")[0]: i for i, l in enumerate(k) if re.match(r"^\.LBB\d+_\d+:", l)}
    loops = []
    for i in range(b0, bars[7]):
        m = re.match(r"\s+s_cbranch_\S+\s+(\.LBB\d+_\d+)", k[i])
        if m and m.group(1) in labels and b0 <= labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    loops = [(h, e) for h, e in loops if any(ops[j] and ops[j].startswith("global_store") for j in range(h, e))]
    loops = [(h, e) for h, e in loops if not any((h2, e2) != (h, e) and h2 <= h and e <= e2 for h2, e2 in loops)]
    in_loop = lambda i: any(h <= i <= e for h, e in loops)   # noqa: E731
    slots = [i for i in range(b3, bars[7]) if ops[i] and ops[i].startswith("global_store") and " sc1" in k[i].split(";")[0]]
    assert slots, "no write-through store behind the barrier that follows U, Y'"
    # the first pass stands outside the task loops where a 16-byte slot store does; the region then ends
    # at the last write-through store ahead of the pair tasks' cold loop (the last task loop)
    cold = any("dwordx4" in k[i] and not in_loop(i) for i in slots)
    if cold:
        slots = [i for i in slots if not in_loop(i) and i < loops[-1][0]]
    end = slots[-1] + 1
    if cold:
        ops = [None if in_loop(i) else o for i, o in enumerate(ops)]
    print("task loops (a global store inside) at lines " + ", ".join(f"{h + 1}..{e + 1}" for h, e in loops) +
          (": the passes after the first, NOT counted below" if cold else ": the tasks' only copy, counted below"))
    names = ("Hpp sums", "Cholesky", "U, Y'", "pairs + store")
    cuts = [b0, bars[4], bars[5], b3, end]
    print(f"kernel {pat}: photo phase, lines {b0 + 1}..{end} (barriers at {[b + 1 for b in bars[3:7]]}, last slot store at {end})")

    def under(i):
        return next((k[j].split(":")[0] for j in range(i, -1, -1) if re.match(r"^\.LBB\d+_\d+:", k[j])), "-")

    def kind(l):
        t = l.split(";")[0]
        out = []
        m = re.search(r"vmcnt\((\d+)\)", t)
        if m:
            out.append("vmcnt(0)" if m.group(1) == "0" else "vmcnt(n)")
        m = re.search(r"lgkmcnt\((\d+)\)", t)
        if m:
            out.append("lgkmcnt(0)" if m.group(1) == "0" else "lgkmcnt(n)")
        return out

    print(f"{'row':14s} {'VALU':>5s} {'FP64':>5s} {'s_load':>7s} {'vmcnt(0)':>9s} {'vmcnt(n)':>9s} {'lgkmcnt(0)':>11s} {'lgkmcnt(n)':>11s} "
          f"{'ds_bpermute':>12s} {'ds other':>9s} {'v_readlane':>11s} {'dpp/permlane':>13s}")
    for name, a, b in list(zip(names, cuts, cuts[1:])) + [("all", b0, end)]:
        r = [(i, o) for i, o in enumerate(ops[a:b], a) if o]
        c = classify([o for _, o in r])
        w = collections.Counter(x for i, o in r if o == "s_waitcnt" for x in kind(k[i]))
        print(f"{name:14s} {c['valu']:5d} {c['fp64']:5d} {sum(o.startswith('s_load') for _, o in r):7d} {w['vmcnt(0)']:9d} "
              f"{w['vmcnt(n)']:9d} {w['lgkmcnt(0)']:11d} {w['lgkmcnt(n)']:11d} {sum(o.startswith('ds_bpermute') for _, o in r):12d} "
              f"{sum(o.startswith('ds_') and not o.startswith('ds_bpermute') for _, o in r):9d} "
              f"{sum(o == 'v_readlane_b32' for _, o in r):11d} {sum('_dpp' in o or 'permlane' in o for _, o in r):13d}")
    r = [(i, o) for i, o in enumerate(ops[b0:end], b0) if o]
    print("scalar loads and vector-memory waits (line, label above, text):")
    for i, o in r:
        if o.startswith("s_load") or (o == "s_waitcnt" and "vmcnt" in k[i].split(";")[0]):
            print(f"  {i + 1:6d} {under(i):12s} {k[i].split(';')[0].strip()}")
    print("global stores and atomics in order (line, label above, text):")
    for i, o in r:
        if o.startswith(("global_store", "global_atomic", "flat_store", "flat_atomic")):
            print(f"  {i + 1:6d} {under(i):12s} {' '.join(k[i].split(';')[0].split())}")
    h = collections.Counter(o for _, o in r if o.startswith("v_") and "_f64" in o)
    print("FP64: " + "  ".join(f"{o} {n}" for o, n in sorted(h.items())))
    meta = "\n".join(lines)
    for key in ("num_vgpr", "numbered_sgpr", "private_seg_size"):
        m = re.search(re.escape(pat) + r"\S*\." + key + r", (\d+)", meta)
        if m:
            print(key, m.group(1))
    m = re.search(re.escape(pat) + r".*?sgpr_spill_count:?\s+(\d+)", meta, re.S)
    if m:
        print("sgpr_spill_count", m.group(1))
    print(f"whole kernel: v_writelane_b32 {sum('v_writelane_b32' in l for l in k)}  v_readlane_b32 {sum('v_readlane_b32' in l for l in k)}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    hist = "--hist" in sys.argv
    lines = open(args[0]).read().splitlines()
    if "--photo" in sys.argv:
        pat = args[1] if len(args) > 1 else DEFAULT
        photo(kernel_text(lines, pat), lines, pat)
        return
    if "--entry" in sys.argv:
        pat = args[1] if len(args) > 1 and not args[1].endswith(".txt") else DEFAULT
        out = next((a for a in args[1:] if a.endswith(".txt")), None)
        entry(kernel_text(lines, pat), lines, pat, out)
        return
    pat = args[1] if len(args) > 1 else DEFAULT
    k = kernel_text(lines, pat)
    ops = [op_of(l) for l in k]
    bars = [i for i, o in enumerate(ops) if o == "s_barrier"]
    labels = {l.split(":")[0]: i for i, l in enumerate(k) if re.match(r"^\.LBB\d+_\d+:", l)}
    # the loops (backward branches) between the third and the fourth barrier; the sweep is the innermost
    # one (no other loop inside it) with the most FP64 instructions
    assert len(bars) > 3, "k_group has at least four barriers"
    loops = []
    for i in range(bars[2], bars[3]):
        m = re.match(r"\s+s_cbranch_\S+\s+(\.LBB\d+_\d+)", k[i])
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    inner = [(h, e) for h, e in loops if not any((h2, e2) != (h, e) and h <= h2 and e2 <= e for h2, e2 in loops)]
    lh, le = max(inner, key=lambda r: sum(1 for o in ops[r[0]:r[1]] if o and o.startswith("v_") and "_f64" in o))
    b0, b1 = bars[2], bars[3]
    regions = [("prologue", b0, lh), ("sweep body", lh, le + 1), ("chain", le + 1, b1)]
    print(f"kernel {pat}: {len(k)} listing lines, edge round between the barriers at lines {b0} and {b1}, sweep loop {lh}..{le}")
    print(f"{'region':12s} {'VALU':>6s} {'FP64':>6s} {'mov':>6s} {'select':>6s} {'lane':>6s} {'other':>6s} {'SALU':>6s} {'LDS':>6s}")
    for name, a, b in regions:
        r = [o for o in ops[a:b] if o]
        c = classify(r)
        salu = sum(1 for o in r if o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop", "s_barrier")))
        lds = sum(1 for o in r if o.startswith("ds_"))
        print(f"{name:12s} {c['valu']:6d} {c['fp64']:6d} {c['mov']:6d} {c['select']:6d} {c['lane']:6d} {c['other']:6d} {salu:6d} {lds:6d}")
        if hist:
            h = collections.Counter(o for o in r if o.startswith("v_") and "_f64" in o)
            print("   FP64: " + "  ".join(f"{o} {n}" for o, n in sorted(h.items())))
            h = collections.Counter(o for o in r if o.startswith("v_") and "_f64" not in o)
            print("   rest: " + "  ".join(f"{o} {n}" for o, n in h.most_common()))
    meta = "\n".join(lines)
    for key in ("num_vgpr", "numbered_sgpr", "private_seg_size"):
        m = re.search(re.escape(pat) + r"\S*\." + key + r", (\d+)", meta)
        if m:
            print(key, m.group(1))
    sp = [l for l in k if "v_writelane_b32" in l]
    rl = [l for l in k if "v_readlane_b32" in l]
    print(f"whole kernel: v_writelane_b32 {len(sp)}  v_readlane_b32 {len(rl)} (SGPR spills and reloads)")


if __name__ == "__main__":
    main()
