#!/usr/bin/env python3
"""Records the step's end (the final workgroup's sums, stop test, solve and camera update) on the small
rigs of tests/test_fold_step_end.py (run on the GPU, from the repo root):

    MCC_LIB=<libmcc.so of the commit to record> python3 tools/make_fold_step_end_golden.py [out.npz]

The fixture tests/golden/fold_step_end/parent.npz holds, per rig (always MCC_FUSED=0): the parameters
after 1, 2, 3 and 9 free-running steps, the COUNT + EPS optimisation (parameters, iteration count, mean
error, last change), delta and JTE of one linearize_solve at x0; on the 4-camera rig the stop test's
cases (COUNT with max_count 0, 1, 5 and an EPS that stops at the 3rd iteration, each with the
parameters after a further step(4)); on the 12-view rig 4 100 iterations, which cross the end of the
step-factor table (k = 4095 -> 4096).  It is recorded ONCE from a build of the commit BEFORE the solve's
prologue moved ahead of the final workgroup's poll (MCC_LIB points at that build) and never regenerated
from the code under test: the test compares the current build against it bit for bit.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multi_camera_calibration_amd import api, rig  # noqa: E402

# the final workgroup's three thread mappings (m = 6 (cameras - 1))
RIGS = {
    # one camera-pair block, one partial norm chunk
    "c2": lambda: rig.make_config("config4", n_cams=2, n_views=12),
    # 6 blocks, 10 groups: the folded final workgroup sums in registers (fold_final_direct)
    "c4": lambda: rig.make_config("config4", n_views=40),
    # 15 blocks: too many for one entry per thread, the final workgroup polls into LDS (fold_final_u)
    "c6": lambda: rig.make_config("config4", n_cams=6, n_views=24),
}
ENV = {"MCC_FUSED": "0"}
FREE_STEPS = (1, 2, 3, 9)
COUNTS = (0, 1, 5)
TABLE_END_STEPS = 4100   # the step-factor table holds 4 096 entries
EPS_DEFAULT = 1e-7       # mymulticalib.hpp:96


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


def free_steps(ba, p, n):
    ba.set_params(p.x0)
    ba.step(n)
    ba.check()
    return ba.get_params()


def optimize_then_step(ba, p, crit_type, max_count, eps):
    """One optimisation and the parameters after a further step(4) on the same handle."""
    x, mean, it, ch = ba.optimize_extrinsics(p.x0, crit_type=crit_type, max_count=max_count, eps=eps)
    ba.step(4)
    ba.check()
    return {"x": np.asarray(x), "mean": np.float64(mean), "iters": np.int32(it), "change": np.float64(ch),
            "x_step4": ba.get_params()}


def record_rig(ba, p):
    out = {}
    for n in FREE_STEPS:
        out[f"x_step{n}"] = free_steps(ba, p, n)
    x, mean, it, ch = ba.optimize_extrinsics(p.x0, crit_type=3, max_count=200, eps=EPS_DEFAULT)
    out.update({"opt/x": np.asarray(x), "opt/mean": np.float64(mean), "opt/iters": np.int32(it),
                "opt/change": np.float64(ch)})
    d, j = ba.compute_jacobian_extrinsic(p.x0)
    out.update({"delta": np.asarray(d), "jte": np.asarray(j)})
    return out


def record_stop_test(ba, p):
    out = {}
    for mc in COUNTS:
        for k, v in optimize_then_step(ba, p, 1, mc, 0.0).items():
            out[f"count{mc}/{k}"] = v
    # the change of iterations 1, 2, 3 (COUNT stops at k = max_count with the k-th update's change)
    ch = [ba.optimize_extrinsics(p.x0, crit_type=1, max_count=k, eps=0.0)[3] for k in (1, 2, 3)]
    assert ch[2] < min(ch[0], ch[1]), ch
    eps = float(np.sqrt(ch[2] * min(ch[0], ch[1])))   # between the 3rd change and the earlier ones
    out["eps3/changes"] = np.asarray(ch)
    out["eps3/eps"] = np.float64(eps)
    for k, v in optimize_then_step(ba, p, 2, 0, eps).items():
        out[f"eps3/{k}"] = v
    assert int(out["eps3/iters"]) == 3, out["eps3/iters"]
    return out


def record_table_end(ba, p):
    xs = free_steps(ba, p, TABLE_END_STEPS)
    x, mean, it, ch = ba.optimize_extrinsics(p.x0, crit_type=1, max_count=TABLE_END_STEPS, eps=0.0)
    return {"table_end/x_step": xs, "table_end/x": np.asarray(x), "table_end/iters": np.int32(it),
            "table_end/change": np.float64(ch)}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "fold_step_end", "parent.npz")
    arrays = {}
    for name in sorted(RIGS):
        p = RIGS[name]()
        ba = make(p, ENV)
        try:
            assert ba.step_kernels() == "k_group", (name, ba.step_kernels())
            rec = record_rig(ba, p)
            rec["folded"] = np.int32(ba.folded())
            if name == "c4":
                rec.update(record_stop_test(ba, p))
            if name == "c2":
                rec.update(record_table_end(ba, p))
        finally:
            ba.close()
        for k, v in rec.items():
            arrays[f"{name}/{k}"] = v
        print(name, "m", ba.m, "folded", int(rec["folded"]), "iters", int(rec["opt/iters"]), "change", float(rec["opt/change"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
