"""One Levenberg-Marquardt trial of the pinhole calibrateCamera against an independent damped step (no GPU).

tests/cpp/pincalib_step.cpp compiles csrc/mcc_pincalib_device.hpp for the host with one lane and runs one
trial -- pc_linearize, pc_eliminate, the contributions summed in view order, pc_reduced_solve, pc_apply,
pc_trial_pose, pc_sumsq -- on a case read from a file.  Here it walks the first K accepted steps of every case
of calib_cases.step_cases() from the library's own start (the guess with the library's edits, the poses seeded
by the one-lane pnp_solve_view) under the documented policy, and every trial on the way, rejected ones
included, is compared with npcalib.lm_step at the same point and the same lambda:

  rho = |J (d_test - d_ref)| / |J d_ref| <= 1e-8   while gamma >= 1e-4 and rms >= 1e-4 px at the trial's start

(below the first J^T e is mostly cancellation and its rounding, about 1e-16 / gamma relative, would set rho;
below the second, which only exact data reach, the residual's own rounding of 1e-13 px would: measured 3.0e-8
on 10x88/rational_k5's sixth step, from an rms of 2.1e-6 px, where the five steps before it give 1e-10 and
less; calib_cases.step_checked).  The gate is about 30 x the largest figure a float64 NumPy restatement of the
elimination gave against lm_step (3e-10); a wrong W index, damping without the diagonal or a wrong sign in the
back-substitution give 1e-4 and more.  Fixed slots move by exactly 0 and under FIX_ASPECT_RATIO
fx == a fy exactly.  Every trial's pc_sumsq of every view equals npcalib's squared error of that view at the
trial parameters (1e-12 relative, or one spacing of a 1280 px coordinate on the view's rms where that is more:
tests/test_calibrate_camera_steps.py), so a view's error sits in its own slot.

The same walk checks what tests/test_calibrate_camera_steps.py needs of its inputs, with this program standing
in for the device: every accept / reject decision is clear (|en / err - 1| >= 1e-9, the GPU and the reference
differ near 1e-14) and the reference takes the same one; each case has at least three checked steps;
ragged9/far has a rejection followed by an accepted, checked step.

This both tests the reference itself and separates lane order from arithmetic in the GPU test's figure.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import calib_cases as CC
import npcalib
from multi_camera_calibration_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

K_STEPS = CC.K_STEPS
RHO_GATE = 1e-8
PIXEL_SPACING = float(np.spacing(1280.0))
CASES = {x[0]: x for x in CC.step_cases()}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    api.build()
    out = str(tmp_path_factory.mktemp("pincalib_step") / "pincalib_step")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-I", os.path.join(HERE, "cpp", "hipstub"),
                    "-I", os.path.join(ROOT, "multi_camera_calibration_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "pincalib_step.cpp"), "-o", out], check=True)
    return out


def one_lane(exe, c, g, poses, mask, aspect, lam, seed_iters=0):
    """One trial of the one-lane program from (g, poses) at lam."""
    base = exe + ".case"
    m = sum(int(b) << k for k, b in enumerate(mask))
    with open(base + ".in", "w") as f:
        f.write(f"{c.n_views} {m} {aspect!r} {lam!r} {seed_iters}\n")
        for a in (c.off, g, poses, c.obj, c.img):
            f.write(" ".join(repr(x) for x in np.asarray(a).ravel().tolist()) + "\n")
    r = subprocess.run([exe, base + ".in", base + ".out"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    with open(base + ".out") as f:
        rows = [np.array(line.split(), np.float64) for line in f]
    V = c.n_views
    return dict(ok=bool(rows[0][0]), err=float(rows[1][0]), en=float(rows[2][0]), g=rows[3], x0=rows[4].reshape(V, 6),
                x=rows[5].reshape(V, 6), sq=rows[6])


_WALK = {}


def walk(exe, name):
    """The first K_STEPS accepted steps of the one-lane program on a case, every trial with its figures."""
    if name in _WALK:
        return _WALK[name]
    _, c, flags, nd, guess = CASES[name]
    mask = api.calib_mask(flags, nd)
    free = [k for k in range(12) if mask[k]]
    g, aspect = CC.state0(flags, nd, guess)
    poses = one_lane(exe, c, g, c.poses, mask, aspect, 1e-3, seed_iters=50)["x0"]
    lam, trials, step, tries = 1e-3, [], 0, 0
    while step < K_STEPS:
        if tries == 0:
            lin = None
        t = one_lane(exe, c, g, poses, mask, aspect, lam)
        dg, dp, J, e = npcalib.lm_step(c, g, poses, mask, lam, aspect, lin)
        if tries == 0:
            gam = npcalib.gamma(c, g, poses, mask, aspect, (J, e))
        lin = (J, e)
        e1 = npcalib.residuals(c, t["g"], t["x"]).reshape(-1, 2)
        n = np.diff(c.off)
        vr_ref = np.array([np.sqrt((e1[c.view(v)] ** 2).sum() / n[v]) for v in range(c.n_views)])
        dview = np.abs(np.sqrt(t["sq"] / n) - vr_ref)
        ref_ratio = npcalib.rms(c, npcalib._tied(g + dg, aspect), poses + dp) ** 2 / npcalib.rms(c, g, poses) ** 2
        accept = t["ok"] and t["en"] <= t["err"]
        rec = dict(step=step, lam=lam, gamma=gam, rms=float(np.sqrt(t["err"] / len(c.obj))), ratio=t["en"] / t["err"],
                   ref_ratio=float(ref_ratio), accept=bool(accept),
                   rho=npcalib.rho(J, free, (t["g"] - g, t["x"] - poses), (dg, dp)), g0=g, g1=t["g"], aspect=aspect,
                   mask=mask, x0=poses, dview=float(dview.max()), view_ok=bool(np.all(dview <= np.maximum(1e-12 * vr_ref, PIXEL_SPACING))))
        trials.append(rec)
        if accept:
            g, poses, lam, step, tries = t["g"], t["x"], max(lam * 0.1, 1e-12), step + 1, 0
        else:
            lam, tries = lam * 10.0, tries + 1
            assert tries < 10, (name, "stalled", trials)
    _WALK[name] = trials
    return trials


@pytest.mark.parametrize("name", list(CASES))
def test_one_lane_trial_is_the_reference_step(exe, name):
    trials = walk(exe, name)
    for t in trials:
        print("FIG", json.dumps({"case": name, **{k: t[k] for k in ("step", "lam", "gamma", "rms", "accept", "ratio", "rho", "dview")}}))
    checked = [t for t in trials if CC.step_checked(t["gamma"], t["rms"])]
    print("FIG", json.dumps({"case": name, "checked": len(checked), "rho_max": max(t["rho"] for t in checked)}))
    for t in trials:
        fixed = [k for k in range(12) if not t["mask"][k] and not (k == 0 and t["aspect"] > 0)]
        assert np.array_equal(t["g1"][fixed], t["g0"][fixed]), (name, t["step"], "a fixed slot moved")
        if t["aspect"] > 0:
            assert t["g1"][0] == t["aspect"] * t["g1"][1]
        assert t["view_ok"], (name, t["step"], "a view's squared error", t["dview"])
    for t in checked:
        assert t["rho"] <= RHO_GATE, (name, t["step"], t["lam"], t["rho"])


@pytest.mark.parametrize("name", list(CASES))
def test_inputs_of_the_gpu_step_test(exe, name):
    trials = walk(exe, name)
    for t in trials:
        print("FIG", json.dumps({"case": name, **{k: t[k] for k in ("step", "lam", "gamma", "rms", "accept", "ratio", "ref_ratio")}}))
    for t in trials:
        assert abs(t["ratio"] - 1.0) >= CC.MARGIN and abs(t["ref_ratio"] - 1.0) >= CC.MARGIN, (name, t["step"], t["ratio"],
                                                                                             t["ref_ratio"])
        assert t["accept"] == (t["ref_ratio"] <= 1.0), (name, t["step"], t["ratio"], t["ref_ratio"])
    accepted = [t for t in trials if t["accept"]]
    assert len(accepted) == K_STEPS
    assert sum(CC.step_checked(t["gamma"], t["rms"]) for t in accepted) >= 3, [(t["gamma"], t["rms"]) for t in accepted]
    if name == "ragged9/far":
        # relin = 0: the stored sums read again at another lambda, in a step that is checked
        assert any(not a["accept"] and b["accept"] and CC.step_checked(b["gamma"], b["rms"])
                   for a, b in zip(trials, trials[1:]))


def test_the_near_zero_view_stays_in_the_series_branch(exe):
    """5x20/near_zero_view is k_pc_lin's run of so3_jac's series (th < 1e-2): the view is there at every trial."""
    trials = walk(exe, "5x20/near_zero_view")
    rv = [float(np.linalg.norm(t["x0"][CC.NEAR_ZERO_VIEW, :3])) for t in trials]
    print("FIG", json.dumps({"case": "5x20/near_zero_view", "rv": rv}))
    assert max(rv) < 1e-2, rv
