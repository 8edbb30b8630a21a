"""One Levenberg-Marquardt trial of the pinhole stereoCalibrate against an independent damped step (no GPU).

tests/cpp/pinstereo_step.cpp compiles csrc/mcc_pinstereo_device.hpp for the host with one lane and runs one
trial -- pc_linearize_rj per camera, ps_maps, ps_assemble, ps_eliminate, the contributions summed in view
order, ps_reduced_solve, ps_apply, ps_trial_pose, ps_view_sumsq -- on a case read from a file.  Here it walks the
first K accepted steps of every case of stereo_calib_cases.step_cases() from the library's own start (the given
intrinsics and rig with the library's edits, the poses seeded by the one-lane pnp_solve_view in camera 1) under
the documented policy, and every trial on the way, rejected ones included, is compared with
npstereocalib.lm_step at the same point and the same lambda:

  rho = |J (d_test - d_ref)| / |J d_ref| <= RHO_GATE   while calib_cases.step_checked(gamma, rms) holds

RHO_GATE is 10 x the largest figure measured here with one lane (DESIGN.md 7h's table), and never above 1e-6.
Fixed slots are bitwise unchanged, tied slots exactly tied, the rejections are the reference's, and every trial's
squared error of every view in every camera equals npstereocalib's at the trial parameters (1e-12 relative, or
one spacing of a 1280 px coordinate on the view's rms where that is more), so a view's error sits in its own
slot and its own camera.

The same walk checks what tests/test_stereo_calibrate_steps.py needs of its inputs: every accept / reject
decision is clear (|en / err - 1| >= calib_cases.MARGIN) and the reference takes the same one; at least the
first four accepted steps of each case are checked; ragged9/far has a rejection followed by an accepted,
checked step (relin = 0: the stored arrow read again at another lambda).

stereo_calib_cases.rig_step_cases() go through the same walk and assertions with their own measured figure:
rigs on which Jl(om), its transpose and the identity, and R t_v and R^T t_v, are far apart, and one on which both
of k_ps_lin's so3_jac calls take the series (|om| and one view's |r_v| under 1e-2, asserted on every trial).
"""
import json
import os
import subprocess

import numpy as np
import pytest

import calib_cases as CC
import npstereocalib as NS
import stereo_calib_cases as SC
from multi_camera_calibration_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

K_STEPS = SC.K_STEPS
RHO_MEASURED = 6.9e-11                    # the largest rho of a checked trial here, one lane
RHO_GATE = min(10 * RHO_MEASURED, 1e-6)
PIXEL_SPACING = float(np.spacing(1280.0))
CASES = {x[0]: x for x in SC.step_cases()}
# stereo_calib_cases.rig_step_cases(): the same walk on rigs far from the identity, under the same assertions, with
# its own measured figure (RHO_MEASURED stays what step_cases() gave)
RIG_CASES = {x[0]: x for x in SC.rig_step_cases()}
RIG_RHO_MEASURED = 8.8e-11                   # the largest rho of a checked trial of RIG_CASES, one lane
RIG_RHO_GATE = min(10 * RIG_RHO_MEASURED, 1e-6)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    api.build()
    out = str(tmp_path_factory.mktemp("pinstereo_step") / "pinstereo_step")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-I", os.path.join(HERE, "cpp", "hipstub"),
                    "-I", os.path.join(ROOT, "multi_camera_calibration_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "pinstereo_step.cpp"), "-o", out], check=True)
    return out


def one_lane(exe, c, g, poses, mask, ties, lam, seed_iters=0):
    """One trial of the one-lane program from (g, poses) at lam."""
    base = exe + ".case"
    m = sum(int(b) << k for k, b in enumerate(mask))
    with open(base + ".in", "w") as f:
        f.write(f"{c.n_views} {m} {int(ties[2])} {float(ties[0])!r} {float(ties[1])!r} {lam!r} {seed_iters}\n")
        for a in (c.off, g, poses, c.obj, c.img1, c.img2):
            f.write(" ".join(repr(x) for x in np.asarray(a).ravel().tolist()) + "\n")
    r = subprocess.run([exe, base + ".in", base + ".out"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    with open(base + ".out") as f:
        rows = [np.array(line.split(), np.float64) for line in f]
    V = c.n_views
    return dict(ok=bool(rows[0][0]), err=float(rows[1][0]), en=float(rows[2][0]), g=rows[3], x0=rows[4].reshape(V, 6),
                x=rows[5].reshape(V, 6), sq=rows[6].reshape(V, 2))


def check_trial(c, t, g, poses, mask, ties, lam, lin, gam, step):
    """One trial's figures against the reference at the same point and lambda (shared with the GPU walk)."""
    free = [k for k in range(30) if mask[k]]
    dg, dp, J, e = NS.lm_step(c, g, poses, mask, lam, ties, lin)
    if gam is None:
        gam = NS.gamma(c, g, poses, mask, ties, (J, e))
    n = np.diff(c.off)[:, None]
    vr_ref = np.sqrt(NS.view_sq(c, t["g"], t["x"]) / n)
    dview = np.abs(np.sqrt(t["sq"] / n) - vr_ref)
    ref_ratio = NS.rms(c, NS.tied(g + dg, ties), poses + dp) ** 2 / NS.rms(c, g, poses) ** 2
    accept = t["ok"] and t["en"] <= t["err"]
    rec = dict(step=step, lam=lam, gamma=gam, rms=float(np.sqrt(t["err"] / (2 * len(c.obj)))), ratio=t["en"] / t["err"],
               ref_ratio=float(ref_ratio), accept=bool(accept),
               rho=NS.rho(J, free, (t["g"] - g, t["x"] - poses), (dg, dp)), g0=g, g1=t["g"], ties=ties, mask=mask,
               x0=poses, dview=float(dview.max()), view_ok=bool(np.all(dview <= np.maximum(1e-12 * vr_ref, PIXEL_SPACING))))
    return rec, (J, e)


def start_of(name):
    _, c, flags, nd, guess1, guess2, rig = (CASES.get(name) or RIG_CASES[name])
    mask = api.stereo_calib_mask(flags, nd)[0]
    g, ties = SC.state0(flags, nd, guess1, guess2, rig)
    return c, mask, g, ties


_WALK = {}


def walk(exe, name):
    """The first K_STEPS accepted steps of the one-lane program on a case, every trial with its figures."""
    if name in _WALK:
        return _WALK[name]
    c, mask, g, ties = start_of(name)
    poses = one_lane(exe, c, g, c.poses, mask, ties, 1e-3, seed_iters=50)["x0"]
    lam, trials, step, tries, lin, gam = 1e-3, [], 0, 0, None, None
    while step < K_STEPS:
        if tries == 0:
            lin, gam = None, None
        t = one_lane(exe, c, g, poses, mask, ties, lam)
        rec, lin = check_trial(c, t, g, poses, mask, ties, lam, lin, gam, step)
        gam = rec["gamma"]
        trials.append(rec)
        if rec["accept"]:
            g, poses, lam, step, tries = t["g"], t["x"], max(lam * 0.1, 1e-12), step + 1, 0
        else:
            lam, tries = lam * 10.0, tries + 1
            assert tries < 10, (name, "stalled", trials)
    _WALK[name] = trials
    return trials


def assert_trials(name, trials, rho_gate):
    """What both walks (one lane here, the MI355X in tests/test_stereo_calibrate_steps.py) assert of their trials."""
    checked = [t for t in trials if CC.step_checked(t["gamma"], t["rms"])]
    print("FIG", json.dumps({"case": name, "checked": len(checked), "rho_max": max(t["rho"] for t in checked)}))
    for t in trials:
        a1, a2, same = t["ties"]
        followers = [6] * (a1 > 0) + [18] * (a2 > 0 or bool(same)) + [19] * bool(same)
        fixed = [k for k in range(30) if not t["mask"][k] and k not in followers]
        assert np.array_equal(t["g1"][fixed], t["g0"][fixed]), (name, t["step"], "a fixed slot moved")
        if a1 > 0:
            assert t["g1"][6] == a1 * t["g1"][7]
        if same:
            assert t["g1"][19] == t["g1"][7]
            assert t["g1"][18] == (a2 * t["g1"][19] if a2 > 0 else t["g1"][6])
        elif a2 > 0:
            assert t["g1"][18] == a2 * t["g1"][19]
        assert t["view_ok"], (name, t["step"], "a view's squared error", t["dview"])
        assert abs(t["ratio"] - 1.0) >= CC.MARGIN and abs(t["ref_ratio"] - 1.0) >= CC.MARGIN, (name, t["step"], t["ratio"],
                                                                                             t["ref_ratio"])
        assert t["accept"] == (t["ref_ratio"] <= 1.0), (name, t["step"], t["ratio"], t["ref_ratio"])   # the rejections
    for t in checked:
        assert t["rho"] <= rho_gate, (name, t["step"], t["lam"], t["rho"])
    accepted = [t for t in trials if t["accept"]]
    assert len(accepted) == K_STEPS
    assert all(CC.step_checked(t["gamma"], t["rms"]) for t in accepted[:SC.MIN_CHECKED]), [(t["gamma"], t["rms"]) for t in accepted]
    if name == "ragged9/far":
        assert any(not a["accept"] and b["accept"] and CC.step_checked(b["gamma"], b["rms"])
                   for a, b in zip(trials, trials[1:]))


@pytest.mark.parametrize("name", list(CASES))
def test_one_lane_trial_is_the_reference_step(exe, name):
    trials = walk(exe, name)
    for t in trials:
        print("FIG", json.dumps({"case": name, **{k: t[k] for k in ("step", "lam", "gamma", "rms", "accept", "ratio", "ref_ratio",
                                                                     "rho", "dview")}}))
    assert_trials(name, trials, RHO_GATE)


@pytest.mark.parametrize("name", list(RIG_CASES))
def test_one_lane_trial_is_the_reference_step_on_the_rigs(exe, name):
    trials = walk(exe, name)
    for t in trials:
        print("FIG", json.dumps({"case": name, **{k: t[k] for k in ("step", "lam", "gamma", "rms", "accept", "ratio", "ref_ratio",
                                                                     "rho", "dview")}}))
    if name == "5x20/series_poses":
        # both of k_ps_lin's so3_jac calls take the series in every trial: |om| and the near-zero view's |r_v| < 1e-2
        small = [(float(np.linalg.norm(t["g0"][0:3])), float(np.linalg.norm(t["x0"][SC.NEAR_ZERO_VIEW, :3]))) for t in trials]
        print("FIG", json.dumps({"case": name, "om_rv": small}))
        assert all(a < 1e-2 and b < 1e-2 for a, b in small), small
    assert_trials(name, trials, RIG_RHO_GATE)
