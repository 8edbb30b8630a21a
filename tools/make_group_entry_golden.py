#!/usr/bin/env python3
"""Records k_group's outputs on the small rigs of tests/test_group_entry.py (run on the GPU, from the
repo root):

    MCC_LIB=<libmcc.so of the commit to record> python3 tools/make_group_entry_golden.py [out.npz]

The fixture tests/golden/group_entry/parent.npz holds, per case and lane width (MCC_GROUP_LANES 32 / 16,
always MCC_FUSED=0 MCC_GROUP=1 plus the case's own settings): delta and JTE at x0, the optimised
parameters and the iteration count (COUNT+EPS, 200 iterations), and get_params() after set_params(x0);
step(24) -- make_group_phase0_golden.py's record; for the stop cases the parameters, the iteration count
and meanReProjError of optimize_extrinsics(crit_type=1, max_count=k), k = 0, 1, 3.  It is recorded ONCE
from a build of the commit BEFORE k_group's entry changed (leading preloaded parameters, one scalar
batch; MCC_LIB points at that build) and never regenerated from the code under test: the test compares
the current build against it bit for bit.
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multi_camera_calibration_amd import api, rig  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_group_phase0_golden",
                                               os.path.join(ROOT, "tools", "make_group_phase0_golden.py"))
P0 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P0)
record, make, group_env, eps_of = P0.record, P0.make, P0.group_env, P0.eps_of

# the smallest rigs at which the entry's role dispatch and range logic can go wrong:
# (rig, settings, what the host planner must report for them -- so that a switch the planner ignores on
# the rig fails the test instead of passing as a copy of another case)
_C4V3 = lambda: rig.make_config("config4", n_views=3)   # noqa: E731  one partial group
_FOLD = {"use_group": 1, "gfold": 1, "small_warm": 1, "fold_dyn": 0, "fold_first": 0}
CASES = {
    # the grid is 1 group + the spare + the folded reduction's trailing workgroups
    "c4_v3": (_C4V3, {}, _FOLD),
    # no trailing roles (k_group -> k_schur)
    "c4_v3_nofold": (_C4V3, {"MCC_GFOLD": "0"}, dict(_FOLD, gfold=0)),
    # no spare: every trailing role's index shifts by one
    "c4_v3_nospare": (_C4V3, {"MCC_SMALL_WARM": "0"}, dict(_FOLD, small_warm=0)),
    # the groups take the reduction's tasks by ticket (no trailing workgroups).  The planner keeps the
    # switch only from twice as many groups as tasks on (8 tasks here): 64 views, 16 groups
    "c4_v64_dyn": (lambda: rig.make_config("config4", n_views=64), {"MCC_FOLD_DYN": "1"},
                   dict(_FOLD, fold_dyn=1, n_pgroups=16)),
    # the FIRST instantiation: the trailing workgroups take the lowest grid indices
    "c4_v3_first": (_C4V3, {"MCC_FOLD_CONSUMERS_FIRST": "1"}, dict(_FOLD, fold_first=1)),
    # a full group plus a one-photo group
    "c4_v5": (lambda: rig.make_config("config4", n_views=5), {}, _FOLD),
    # uneven groups
    "c4_vis": (lambda: rig.make_config("config4", n_views=24, visibility=0.5), {}, _FOLD),
    # m = 114: k_group -> k_schur -> k_solve, several rounds per group
    "pin_c20": (lambda: rig.make_config("config2", n_cams=20, n_views=6), {}, {"use_group": 1, "gfold": 0, "m": 114}),
    # the BACK instantiation
    "c5_v6": (lambda: rig.make_config("config5", n_views=6), {}, {"use_group": 1, "has_back": 1}),
}
# the stop path: COUNT with max_count k; the launches after the stop, up to the end of the 8-step graph,
# must change nothing
STOP_CASE = "c4_v5"
STOP_COUNTS = (0, 1, 3)
LANES = (32, 16)


def case_env(name, lanes):
    return dict(group_env(lanes), **CASES[name][1])


def record_stop(ba, p):
    out = {}
    for k in STOP_COUNTS:
        x, mean, it, _ = ba.optimize_extrinsics(p.x0, crit_type=1, max_count=k)
        out[f"stop{k}_x"] = np.asarray(x)
        out[f"stop{k}_iters"] = np.asarray(it, np.int32)
        out[f"stop{k}_mean"] = np.asarray(mean, np.float64)
    return out


def record_case(ba, p, name):
    got = record(ba, p)
    if name == STOP_CASE:
        got.update(record_stop(ba, p))
    return got


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "group_entry", "parent.npz")
    arrays = {}
    for name in sorted(CASES):
        p = CASES[name][0]()
        for lanes in LANES:
            ba = make(p, case_env(name, lanes))
            try:
                assert ba.step_kernels() == "k_group", (name, lanes, ba.step_kernels())
                for k, v in record_case(ba, p, name).items():
                    arrays[f"{name}/{lanes}/{k}"] = v
            finally:
                ba.close()
            print(name, lanes, "iters", int(arrays[f"{name}/{lanes}/iters"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
