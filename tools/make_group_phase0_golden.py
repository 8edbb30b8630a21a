#!/usr/bin/env python3
"""Records k_group's outputs on the small rigs of tests/test_group_phase0.py (run on the GPU, from the
repo root):

    MCC_LIB=<libmcc.so of the commit to record> python3 tools/make_group_phase0_golden.py [out.npz]

The fixture tests/golden/group_phase0/parent.npz holds, per case and lane width (MCC_GROUP_LANES 32 / 16,
always MCC_FUSED=0 MCC_GROUP=1): delta and JTE at x0, the optimised parameters and the iteration count
(COUNT+EPS, 200 iterations), and get_params() after set_params(x0); step(24).  It is recorded ONCE from
a build of the commit BEFORE the phase-0 batching of k_group (MCC_LIB points at that build) and never
regenerated from the code under test: the test compares the current build against it bit for bit.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multi_camera_calibration_amd import api, rig  # noqa: E402

# the smallest shapes at which k_group's phase 0 can go wrong
CASES = {
    # one partial group: np < 4, gne < 16, clamped header lanes (11 edges)
    "c4_v3": lambda: rig.make_config("config4", n_views=3),
    # a full group plus a one-photo group (19 edges)
    "c4_v5": lambda: rig.make_config("config4", n_views=5),
    # photos with 1-4 edges, uneven groups, short pair and contribution lists (56 edges)
    "c4_vis": lambda: rig.make_config("config4", n_views=24, visibility=0.5),
    # 117 corners per edge (> kGChunk = 96): second chunk restaged inside the sweep after the deferred commit
    "c4_b13x9": lambda: rig.make_config("config4", n_views=8, board=(13, 9)),
    # 20 corners per edge, fewer than the edge's 32 lanes
    "c4_b5x4": lambda: rig.make_config("config4", n_views=8, board=(5, 4)),
    # 20 edges per photo, m = 114: several rounds per group (edges past the header), 5-coefficient D rows
    "pin_c20": lambda: rig.make_config("config2", n_cams=20, n_views=6),
    # BACK / double-side variant, the transform's thread
    "c5_v6": lambda: rig.make_config("config5", n_views=6),
}
LANES = (32, 16)
STEPS = 24


def eps_of(p):
    return 1e-8 if p.model == rig.DOUBLESIDE else 1e-7   # doubleSide.hpp:105 / mymulticalib.hpp:96


def group_env(lanes):
    env = {"MCC_FUSED": "0", "MCC_GROUP": "1"}
    if lanes == 16:
        env["MCC_GROUP_LANES"] = "16"
    return env


def make(p, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return api.BundleAdjuster(p)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def record(ba, p):
    """What the fixture holds for one (case, lane width)."""
    d, j = ba.compute_jacobian_extrinsic(p.x0)
    x, _, it, _ = ba.optimize_extrinsics(p.x0, crit_type=3, max_count=200, eps=eps_of(p))
    ba.set_params(p.x0)
    ba.step(STEPS)
    ba.check()
    xs = ba.get_params()
    return {"delta": np.asarray(d), "jte": np.asarray(j), "x_opt": np.asarray(x), "iters": np.asarray(it, np.int32),
            "x_step": np.asarray(xs)}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "group_phase0", "parent.npz")
    arrays = {}
    for name in sorted(CASES):
        p = CASES[name]()
        for lanes in LANES:
            ba = make(p, group_env(lanes))
            try:
                assert ba.step_kernels() == "k_group", (name, lanes, ba.step_kernels())
                for k, v in record(ba, p).items():
                    arrays[f"{name}/{lanes}/{k}"] = v
            finally:
                ba.close()
            print(name, lanes, "iters", int(arrays[f"{name}/{lanes}/iters"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
