#!/usr/bin/env python3
"""Per-phase s_memtime shares of the split step's kernels (k_prep, k_edge, k_photo) from the
diagnostic build (libmcc_diag.so).  Never quote this build's run time: read its shares.

    MCC_LIB=multi_camera_calibration_amd/libmcc_diag.so python tools/diag_split.py [config] [views]

k_group (the split step's group kernel) group g -> row g slots 0..10 (start, loads, photo update and
Rodrigues, round 0's prologue, sweep, chain, the later rounds, Hpp sums, Cholesky, U / Y', pairs), all
stamped by wave 0; slot 11 wave 0's slot stores issued (slot 10 stands behind a drain of the stores that
only this build has); slots 12 and 13 the clock at the kernel's first instruction as wave 0 and the last wave
read it (printed as "entry -> stamp 0": the role dispatch, the stop test and the scalar loads, which the
phase rows do not cover); slots 16 + w wave w's last round's end and 24 + w its round-0 prologue, sweep and chain
ends, printed per wave half (wave_halves).
Otherwise rows of the stamp buffer (32 slots each): k_photo photo p -> row p slots 0..5 (start, staged,
Cholesky, U / Y', pairs stored; slot 2 unused); k_prep workgroup w -> row w slots 8..11 (start, update,
photo Rodrigues, edges stored); k_edge workgroup w -> row w / 2 slots 16 + 8 (w & 1) + 0..4
(start, corners staged, sweep, butterfly, H stored).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_camera_calibration_amd import api, rig  # noqa: E402


def med(v):
    v = v[v > 0]
    return f"median {np.median(v):8.0f}  p90 {np.percentile(v, 90):8.0f}  (n={len(v)})" if len(v) else "n/a"


def wave_halves(rows, ng):
    """k_group's per-wave round-0 stamps: slot 24 + w holds wave w's prologue, sweep and chain ends as
    cycles since the barrier that ends phase 0 (21 bits each), slot 16 + w its last round's end.  With 32
    lanes per edge waves w and w + 4 share a SIMD: printed per half, with the per-group gap between the
    halves' last waves."""
    rows = rows[:ng].astype(np.int64)
    nw = int(np.count_nonzero(rows[0, 24:32]))
    if nw == 0:
        return
    m21 = (1 << 21) - 1
    pk = rows[:, 24:24 + nw]
    pro, swp, chn = pk & m21, (pk >> 21) & m21, (pk >> 42) & m21
    end = rows[:, 16:16 + nw] - rows[:, 2:3]   # wave 0's stamp 2 stands for every wave's (same barrier)
    halves = [("waves 0-3", slice(0, 4)), ("waves 4-7", slice(4, 8))] if nw == 8 else [(f"waves 0-{nw - 1}", slice(0, nw))]
    print(f"k_group round 0 per wave, cycles since the end of phase 0 ({nw} waves; median over groups of the half's "
          "mean, [min wave, max wave])")
    for name, sl in halves:
        print(f"  {name}")
        for lab, v in (("prologue end", pro), ("sweep end", swp), ("chain end", chn), ("rounds end", end)):
            h = v[:, sl]
            print(f"    {lab:14s} {np.median(h.mean(axis=1)):8.0f}  [{np.median(h.min(axis=1)):8.0f}, "
                  f"{np.median(h.max(axis=1)):8.0f}]")
        d = np.diff(np.stack([np.zeros_like(pro[:, sl]), pro[:, sl], swp[:, sl], chn[:, sl]]), axis=0)
        print("    durations      prologue %.0f  sweep %.0f  butterfly+chain %.0f" %
              tuple(np.median(d[k].mean(axis=1)) for k in range(3)))
    if nw == 8:
        gap = end[:, 4:8].max(axis=1) - end[:, 0:4].max(axis=1)
        print(f"  last wave of 4-7 minus last wave of 0-3: median {np.median(gap):.0f}  p10 {np.percentile(gap, 10):.0f}  "
              f"p90 {np.percentile(gap, 90):.0f}")
        print(f"  last wave's rounds end (stamp 2 -> all waves at the barrier): median {np.median(end.max(axis=1)):.0f}")


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "config3"
    views = int(sys.argv[2]) if len(sys.argv) > 2 else None
    p = rig.make_config(cfg, n_views=views)
    os.environ.setdefault("MCC_FUSED", "0")
    ba = api.BundleAdjuster(p)
    ba.set_params(p.x0)
    ba.step(20)
    ba.synchronize()
    ba.stamps()          # arm
    ba.step(1)
    ba.synchronize()
    raw = ba.stamps().reshape(-1)
    nv = max(p.n_photos, 1)
    s = raw[:32 * nv].reshape(nv, 32).astype(np.float64)

    def phases(cols, names, title):
        blk = s[:, cols]
        ok = (blk > 0).all(axis=1)
        d = np.diff(blk[ok], axis=1)
        print(f"{title}: {ok.sum()} workgroups")
        for k, n in enumerate(names):
            print(f"  {n:22s} {med(d[:, k])}")
        print(f"  {'total':22s} {med(blk[ok][:, -1] - blk[ok][:, 0])}")

    if ba.step_kernels() == "k_group":
        ng = int(np.count_nonzero(s[:, 0]))
        # the kernel's entry (slots 12, 13: wave 0's and the last wave's clock at k_group's first
        # instruction): the role dispatch, the stop test and the scalar loads ahead of stamp 0
        ok = (s[:, 0] > 0) & (s[:, 12] > 0) & (s[:, 13] > 0)
        if ok.any():
            print(f"k_group entry: {ok.sum()} groups")
            print(f"  {'entry -> stamp 0':22s} {med(s[ok, 0] - s[ok, 12])}")
            print(f"  {'entry -> stamp 1':22s} {med(s[ok, 1] - s[ok, 12])}")
            lw = s[ok, 13] - s[ok, 12]
            print(f"  last wave's entry minus wave 0's: median {np.median(lw):.0f}  p10 {np.percentile(lw, 10):.0f}  "
                  f"p90 {np.percentile(lw, 90):.0f}")
        phases(list(range(11)), ["loads (round trip 1)", "photo update+Rodrigues", "edge prologue (r0)", "sweep (r0)",
                                 "butterfly+chain (r0)", "later rounds", "photo Hpp sums", "Cholesky", "U, Y'",
                                 "pairs+store"], f"k_group ({ng} groups)")
        # slot 11: wave 0's slot stores issued (stamp 10 stands behind the diagnostic build's own drain)
        ok = (s[:, 9] > 0) & (s[:, 11] > 0)
        if ok.any():
            print(f"  {'pairs, to the issue':22s} {med(s[ok, 11] - s[ok, 9])}")
            print(f"  {'stamp 0 -> the issue':22s} {med(s[ok, 11] - s[ok, 0])}")
        wave_halves(raw[:32 * nv].reshape(nv, 32), ng)
        return
    phases([0, 1, 3, 4, 5], ["load+stage+sums", "Cholesky, Li", "U, Y'", "pairs+store"], "k_photo")
    phases([8, 9, 10, 11], ["photo update", "photo Rodrigues", "edge prologues"], "k_prep")
    for h in (0, 1):
        base = 16 + 8 * h
        phases([base, base + 1, base + 2, base + 3, base + 4], ["stage corners", "sweep", "butterfly", "chain+store"],
               f"k_edge (half {h})")


if __name__ == "__main__":
    main()
