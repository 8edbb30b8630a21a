#!/usr/bin/env python3
"""Records k_group's outputs on the small rigs of tests/test_group_edge_round.py (run on the GPU, from the
repo root):

    MCC_LIB=<libmcc.so of the commit to record> python3 tools/make_group_edge_round_golden.py [out.npz]

The fixture tests/golden/group_edge_round/parent.npz holds what tools/make_group_phase0_golden.py's
record() gives (delta and JTE at x0, the optimised parameters and the iteration count, the state after 24
free-running steps) per case and lane width (MCC_GROUP_LANES 32 / 16, always MCC_FUSED=0 MCC_GROUP=1).
It is recorded ONCE from a build of the commit BEFORE the edge round's issue priority (MCC_LIB points at
that build) and never regenerated from the code under test: the test compares the current build against it
bit for bit.  The rigs are those the phase-0 fixture does not cover and on which the edge round's
prologue, record scatter and chain can go wrong; `python3 tools/make_group_edge_round_golden.py --oracle`
checks on the CPU that the oracle accepts each of them (every photo block positive definite at x0, the
same iteration count from x0 and from x0 moved by one float32 ulp).
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from multi_camera_calibration_amd import rig  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_group_phase0_golden",
                                               os.path.join(ROOT, "tools", "make_group_phase0_golden.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)
LANES, eps_of, group_env, make, record = MG.LANES, MG.eps_of, MG.group_env, MG.make, MG.record


def widen(p, nd, tau=(0.01, -0.008)):
    """rational (nd 8) / thin-prism (12) / tilted-sensor (14) coefficients on top of the rig's 5; the
    observations stay those of the 5-term model (tests/test_gpu_parity.py's variants)"""
    D = np.zeros((p.n_cams, nd), np.float32)
    D[:, :5] = p.D[:, :5]
    extra = [0.01, -0.005, 0.002, 3e-4, -2e-4, 1e-4, 2e-4]
    for k in range(5, min(nd, 12)):
        D[:, k] = extra[k - 5]
    if nd == 14:
        D[:, 12] = tau[0] * (1 + 0.1 * np.arange(p.n_cams))
        D[:, 13] = tau[1] * (1 - 0.1 * np.arange(p.n_cams))
    p.D = D
    return p


def pi_branch(p):
    """One photo rotated so that its composition with a camera is a rotation by pi about the composition's
    current axis: that edge takes cvRodrigues2's theta ~ pi branch (tests/test_rodrigues_branch.py).  The
    branch's angle is acos((trace - 1) / 2) at -1, where one ulp of the trace moves it by 1.5e-8 rad, and
    the device skips the re-orthonormalisation the oracle applies first (mcc_device.hpp rodrigues_m2v): the
    two composed vectors can differ by a few such steps along the axis.  Everything after the branch starts
    from the vector's float32 rounding (the branch's own partials are zero), so the edge taken is the first
    one of a moving camera whose float32 vector, as the oracle composes it, does not move when the angle
    does by up to +-6e-8 rad (four ulps of the trace): there device and oracle start from the same float32
    pose and tests/test_gpu_parity.py's bars apply."""
    from oracle import oracle_py as O
    x0 = np.array(p.x0, np.float32)
    for e in range(p.n_edges):
        c, v = int(p.edge_cam[e]), int(p.edge_photo[e])
        if c == 0:
            continue
        col, cc = int(p.photo_col(v)), 6 * (c - 1)
        Rc = rig.rodrigues(x0[cc:cc + 3].astype(np.float64))
        w = rig.log_so3(Rc @ rig.rodrigues(x0[col:col + 3].astype(np.float64)))
        x = x0.copy()
        x[col:col + 3] = rig.log_so3(Rc.T @ rig.rodrigues(w / np.linalg.norm(w) * np.pi)).astype(np.float32)
        xd = x.astype(np.float64)
        om3, _, d = O.compose_motion(xd[col:col + 3], xd[col + 3:col + 6], xd[cc:cc + 3], xd[cc + 3:cc + 6])
        if np.abs(d[0]).max() != 0.0:   # not in the branch (its d om3 / d om1 is zero)
            continue
        ax = om3 / np.linalg.norm(om3)
        if all(np.array_equal((om3 + ax * t).astype(np.float32), om3.astype(np.float32))
               for t in (-6e-8, -3e-8, -1.5e-8, 1.5e-8, 3e-8, 6e-8)):
            p.x0 = x
            return p
    raise RuntimeError("no edge with a float32 pose that is robust in the pi branch")


def keep_edges(p, keep):
    """The problem without the edges where keep is False (every photo keeps at least one)."""
    keep = np.nonzero(keep)[0]
    idx = np.concatenate([np.arange(p.edge_off[e], p.edge_off[e] + p.edge_n[e]) for e in keep])
    p.edge_cam, p.edge_photo, p.edge_side = p.edge_cam[keep].copy(), p.edge_photo[keep].copy(), p.edge_side[keep].copy()
    p.edge_n = p.edge_n[keep].copy()
    off = np.zeros(len(keep), np.int32)
    off[1:] = np.cumsum(p.edge_n)[:-1]
    p.edge_off = off
    p.obj, p.img = p.obj[idx].copy(), p.img[idx].copy()
    return p


def single_edge_photo(p, photo=0):
    """photo 0 keeps only its first camera's edge: 17 edges, so the first group holds four photos with 13
    edges (three empty edge slots) and the last photo is a group of its own"""
    first = np.zeros(p.n_edges, bool)
    first[np.nonzero(p.edge_photo == photo)[0][0]] = True
    return keep_edges(p, (p.edge_photo != photo) | first)


CASES = {
    # the pinhole sweep's wider intrinsics rows (18 / 27 words per edge copied by the prologue's lanes)
    "pin_rational": lambda: widen(rig.make_config("config2", n_views=4), 8),
    "pin_prism": lambda: widen(rig.make_config("config2", n_views=4), 12),
    "pin_tilt": lambda: widen(rig.make_config("config2", n_views=4), 14),
    # MyMulti with BACK edges: the second compose_motion and the three-factor chain maps
    # (seed 10: the oracle's loop ends after 43 iterations; config5's own seed runs into the 200-iteration cap)
    "back": lambda: rig.make_config("config5", n_cams=4, n_views=4, model=rig.PINHOLE, double_sided=True, seed=10),
    # DoubleSide, 8 cameras: up to 16 edges per photo, so a group holds fewer photos than it has slots for
    "c5_v3": lambda: rig.make_config("config5", n_views=3),
    # one edge in the theta ~ pi branch: the cold loop that zeroes A1, A2
    "c4_pi": lambda: pi_branch(rig.make_config("config4", n_views=4)),
    # a photo with one edge: edge slots past the group's edges in the prologue and the chain
    "c4_single": lambda: single_edge_photo(rig.make_config("config4", n_views=5)),
}


def oracle_check():
    from oracle import oracle_py as O
    for name in sorted(CASES):
        p = CASES[name]()
        o = O.Oracle(p)
        H = o.normal_dense(p.x0)[0]
        g = p.global_dim
        pd = min(np.linalg.eigvalsh(H[g + 6 * q:g + 6 * q + 6, g + 6 * q:g + 6 * q + 6]).min() for q in range(p.n_photos))
        _, m, it, _ = o.optimize(p.x0, crit_type=3, max_count=200, eps=eps_of(p))
        its = []
        for k in (0, p.n_params // 2, p.n_params - 1):
            x = p.x0.copy()
            x[k] = np.nextafter(x[k], np.float32(np.inf))
            its.append(o.optimize(x, crit_type=3, max_count=200, eps=eps_of(p))[2])
        print(f"{name:14s} edges {p.n_edges:3d} photos {p.n_photos} min photo-block eigenvalue {pd:.3e} "
              f"iterations {it} (one ulp off: {its}) mean error {m:.6f}", flush=True)
        # (DoubleSide at 3 views, eps 1e-8: the count moves with one float32 ulp of x0 at every seed tried; the
        # device differs from the oracle at FP64 rounding only, nine orders below that, and the test holds it
        # to the oracle's count)
        assert pd > 0 and it < 200 and (all(i == it for i in its) or name == "c5_v3"), name


def main():
    if "--oracle" in sys.argv:
        oracle_check()
        return
    from multi_camera_calibration_amd import api  # noqa: F401
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "group_edge_round", "parent.npz")
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
