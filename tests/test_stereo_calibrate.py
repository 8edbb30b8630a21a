"""mcc_stereo_calibrate on the GPU: cv::stereoCalibrate's least-squares minimum, by Levenberg-Marquardt.

Every test runs with max_count = 200 and eps = 1e-13 unless it is about the criteria, so that convergence is
tested, not OpenCV's default budget.  The reference is tests/npstereocalib.py (dense Gauss-Newton on complex-step
Jacobians, started from the truth); tests/test_stereo_calibrate_cpu.py checks that it handles every noisy case
used here and holds it to stereo_calib_cases.REF_RESOLUTION.

Gates that are fixed: rms <= 1e-8 px on exact data; rms equal to the reference's within 1e-6 relative under
noise; bitwise equality where stated.  The parameter bounds are 10 x the figure measured on an MI355X and
recorded in DESIGN.md 7h (MEASURED below), against the reference 10 x that figure or 10 x the reference's own
resolution, whichever is larger (DESIGN.md 7g's rule, for its reason: a difference below what the reference
resolves says nothing about the device).  Every test prints its figures before it asserts.  Whether each step
on the way is the right one is tests/test_stereo_calibrate_steps.py's question.
"""
import json

import numpy as np
import pytest

import calib_cases as CC
import npcalib
import npstereocalib as NS
import stereo_calib_cases as SC
from multi_camera_calibration_amd import api

pytestmark = pytest.mark.gpu

MAXC, EPS = 200, 1e-13
KEYS = ("dK", "dD", "dom", "dT", "dr", "dt")

# measured on an MI355X: dK max relative error of fx fy cx cy of both cameras, dD max absolute error of
# both D, dom / dT of the rig (rad, mm), dr / dt of the views' poses (rad, mm), against the truth (exact) or
# npstereocalib (noisy)
MEASURED = {
    "exact/3x88/guess": dict(dK=1.51e-15, dD=1.25e-12, dom=8.99e-16, dT=7.86e-13, dr=8.88e-16, dt=5.68e-13),
    "exact/3x88/closed_form": dict(dK=1.91e-15, dD=1.19e-13, dom=1.84e-15, dT=3.67e-13, dr=1.44e-15, dt=1.41e-12),
    "exact/2x20/guess": dict(dK=5.68e-15, dD=9.77e-12, dom=4.81e-15, dT=1.17e-13, dr=3.83e-15, dt=3.18e-12),
    "exact/2x20/closed_form": dict(dK=9.02e-15, dD=3.89e-12, dom=7.71e-15, dT=6.32e-13, dr=4.27e-15, dt=3.52e-12),
    "exact/5x20/guess": dict(dK=1.04e-14, dD=4.81e-12, dom=7.33e-15, dT=1.17e-13, dr=8.05e-15, dt=8.07e-12),
    "exact/5x20/closed_form": dict(dK=1.05e-14, dD=2.46e-12, dom=1.05e-14, dT=1.41e-12, dr=7.38e-15, dt=6.38e-12),
    "exact/10x20/guess": dict(dK=3.61e-15, dD=8.49e-13, dom=3.63e-15, dT=3.66e-13, dr=1.61e-15, dt=2.05e-12),
    "exact/10x20/closed_form": dict(dK=3.84e-15, dD=2.86e-12, dom=2.74e-15, dT=3.69e-13, dr=2.22e-15, dt=2.03e-12),
    "exact/17x64/guess": dict(dK=5.41e-16, dD=2.00e-13, dom=2.88e-16, dT=1.39e-13, dr=5.55e-16, dt=2.56e-13),
    "exact/17x64/closed_form": dict(dK=6.99e-16, dD=1.95e-13, dom=5.13e-16, dT=3.46e-14, dr=6.11e-16, dt=2.27e-13),
    "exact/17x65/guess": dict(dK=5.41e-16, dD=3.01e-14, dom=4.86e-16, dT=4.44e-14, dr=4.44e-16, dt=2.27e-13),
    "exact/17x65/closed_form": dict(dK=8.68e-16, dD=9.63e-15, dom=6.80e-16, dT=9.50e-14, dr=9.44e-16, dt=6.82e-13),
    "exact/ragged9/guess": dict(dK=5.02e-16, dD=1.84e-14, dom=3.54e-16, dT=9.95e-14, dr=1.53e-15, dt=6.82e-13),
    "exact/ragged9/closed_form": dict(dK=3.61e-16, dD=2.40e-14, dom=1.80e-16, dT=4.88e-14, dr=1.51e-15, dt=4.55e-13),
    "exact/65x4/guess": dict(dK=4.51e-15, dD=1.09e-11, dom=5.31e-15, dT=7.73e-14, dr=9.85e-15, dt=2.86e-12),
    "exact/65x4/closed_form": dict(dK=4.96e-14, dD=6.37e-11, dom=4.83e-14, dT=4.12e-12, dr=3.45e-14, dt=3.09e-11),
    "noisy/flags0": dict(dK=3.24e-14, dD=1.43e-13, dom=1.29e-14, dT=5.26e-13, dr=5.88e-15, dt=4.58e-12),
    "noisy/fix_intrinsic": dict(dK=0.00e+00, dD=0.00e+00, dom=7.29e-16, dT=5.40e-13, dr=2.61e-13, dt=2.96e-12),
    "noisy/guess_same_focal": dict(dK=2.58e-10, dD=5.78e-10, dom=3.24e-11, dT=1.44e-08, dr=1.84e-10, dt=2.16e-07),
    "noisy/aspect": dict(dK=8.80e-13, dD=1.02e-11, dom=7.78e-13, dT=4.30e-11, dr=6.15e-13, dt=4.63e-10),
    "noisy/k3_tangent": dict(dK=2.75e-12, dD=9.65e-12, dom=1.53e-12, dT=3.91e-10, dr=1.92e-12, dt=1.88e-09),
    "noisy/nd4": dict(dK=2.20e-14, dD=2.27e-14, dom=1.33e-14, dT=4.41e-13, dr=1.03e-14, dt=1.16e-11),
    "noisy/extrinsic_guess": dict(dK=3.25e-14, dD=1.42e-13, dom=1.41e-14, dT=5.46e-13, dr=7.22e-15, dt=6.21e-12),
    "noisy/ragged9": dict(dK=1.29e-12, dD=8.74e-11, dom=5.71e-13, dT=1.91e-10, dr=1.01e-09, dt=1.11e-08),
    "identical": dict(dr=1.14e-18, dt=0.00e+00),
    "permuted": dict(dK=3.50e-16, dD=2.25e-14, dom=1.32e-16, dT=3.82e-14, dr=9.99e-16, dt=2.27e-13),
}


def run(c, flags=0, nd=5, guess1=None, guess2=None, rig=None, max_count=MAXC, eps=EPS, crit_type=api.MCC_CRIT_COUNT_EPS, **kw):
    K1, D1 = SC.guess_KD(guess1, nd)
    K2, D2 = SC.guess_KD(guess2, nd)
    R, T = SC.rig_RT(rig)
    return api.stereo_calibrate(c.off, c.obj, c.img1, c.img2, SC.SIZE, K1=K1, D1=D1, K2=K2, D2=D2, R=R, T=T, flags=flags, nd=nd,
                                max_count=max_count, eps=eps, crit_type=crit_type, **kw)


def slots(res):
    return SC.globals_of(res[1], res[2], res[3], res[4], res[5], res[6])


def figures(res, g_ref, poses_ref):
    g = slots(res)
    rel = lambda s: float(np.max(np.abs(g[s] - g_ref[s]) / np.abs(g_ref[s])))
    return dict(dK=max(rel(slice(6, 10)), rel(slice(18, 22))),
                dD=float(max(np.abs(g[10:18] - g_ref[10:18]).max(), np.abs(g[22:30] - g_ref[22:30]).max())),
                dom=float(np.abs(g[0:3] - g_ref[0:3]).max()), dT=float(np.abs(g[3:6] - g_ref[3:6]).max()),
                dr=float(np.abs(res[9] - poses_ref[:, :3]).max()), dt=float(np.abs(res[10] - poses_ref[:, 3:]).max()))


def check(name, fig, keys=KEYS, against_reference=False):
    if not keys:
        print("FIG", json.dumps({"case": name, **fig}))
        return
    assert name in MEASURED, f"no measured figures for {name}"
    for k in keys:
        bound = 10.0 * max(MEASURED[name][k], SC.REF_RESOLUTION[k] if against_reference else 0.0)
        assert fig[k] <= bound, (name, k, fig[k], bound)


def consistent(res, c):
    """What every result satisfies: E = [T]x R and F from it, rms from the per-view figures."""
    rms, K1, D1, K2, D2, R, T, E, F, rvec, tvec, vrms = res[:12]
    E2, F2 = api.stereo_epipolar(R, T, K1, K2)
    assert np.array_equal(E, E2) and np.array_equal(F, F2)
    n = np.diff(c.off)[:, None]
    assert abs(np.sqrt((vrms ** 2 * n).sum() / (2 * len(c.obj))) - rms) <= 1e-12 * max(rms, 1e-300) + 1e-300
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14


EXACT = {"3x88": [88] * 3, "2x20": [20] * 2, "5x20": [20] * 5, "10x20": [20] * 10, "17x64": [64] * 17, "17x65": [65] * 17,
         "ragged9": list(CC.RAGGED), "65x4": [4] * 65}


def exact_case(name):
    return SC.make(EXACT[name], seed=900 + len(EXACT[name]) + EXACT[name][0])


@pytest.mark.parametrize("start", ["guess", "closed_form"])
@pytest.mark.parametrize("name", list(EXACT))
def test_exact_data_all_intrinsics_free(name, start):
    c = exact_case(name)
    if start == "guess":
        res = run(c, SC.USE_GUESS, 5, c.g[6:18] * 1.01, c.g[18:30] * 1.01)
    else:
        res = run(c)
    fig = figures(res, c.g, c.poses)
    fig.update(rms=res[0], iterations=res[12], status=res[13])
    key = f"exact/{name}/{start}"
    check(key, fig, keys=())
    assert res[0] <= 1e-8
    assert np.all(np.isfinite(res[11])) and np.all(res[11] <= 1e-8 * np.sqrt(2 * len(c.obj)))
    consistent(res, c)
    check(key, fig)


NOISY = {x[0]: x for x in SC.noisy_cases()}


@pytest.mark.parametrize("name", [n for n in NOISY if n != "rational"])   # (the rational case has its own test below)
def test_noisy_data_reaches_the_reference_minimum(name):
    _, c, flags, nd, guess1, guess2, rig = NOISY[name]
    ref = SC.reference(name)
    res = run(c, flags, nd, guess1, guess2, rig)
    rms, K1, D1, K2, D2 = res[:5]
    g, poses = slots(res), np.hstack([res[9], res[10]])
    fig = figures(res, ref["g"], ref["poses"])
    fig.update(drms=abs(rms - ref["rms"]) / ref["rms"], rms=rms, iterations=res[12], status=res[13])
    print("REF", json.dumps({"case": name, **SC.resolution(ref)}))
    check("noisy/" + name, fig, keys=())
    assert fig["drms"] <= 1e-6
    consistent(res, c)
    # every view's rms in each camera against the reference's projection at the returned parameters
    n = np.diff(c.off)[:, None]
    vr = np.sqrt(NS.view_sq(c, g, poses) / n)
    print("FIG", json.dumps({"case": name, "dview": float(np.max(np.abs(res[11] - vr) / vr))}))
    assert res[11].shape == (c.n_views, 2)
    assert np.all(np.abs(res[11] - vr) <= 1e-9 * vr)
    if name == "fix_intrinsic":
        assert np.array_equal(g[6:30], np.concatenate([guess1, guess2]))         # bit-equal to the input
        assert res[1][0, 1] == 0 and res[1][2, 2] == 1
    if name == "guess_same_focal":
        assert K2[0, 0] == K1[0, 0] and K2[1, 1] == K1[1, 1]
    if name == "aspect":
        for K, gs in ((K1, guess1), (K2, guess2)):
            assert K[0, 0] == (gs[0] / gs[1]) * K[1, 1]
    if name == "k3_tangent":
        assert not D1[2:5].any() and not D2[2:5].any()
    if name == "nd4":
        assert len(D1) == 4 and len(D2) == 4
    check("noisy/" + name, fig, against_reference=True)


def test_rational_model_from_a_guess():
    _, c, flags, nd, guess1, guess2, rig = NOISY["rational"]
    res = run(c, flags, nd, guess1, guess2, rig)
    mask = api.stereo_calib_mask(flags, nd)[0]
    g, x = slots(res), np.hstack([res[9], res[10]])
    # gated on rms, as tests/test_calibrate_camera.py gates its rational case: k4 k5 k6 trade against k1 k2 k3 along a
    # valley that Levenberg-Marquardt descends slowly, so the parameters are not compared.  Recorded beside it: the
    # share of the allowed rms that a step could still remove, |P e| / (1e-6 sqrt(2 corners)).
    e = NS.residuals(c, g, x)
    proj = NS.gamma(c, g, x, mask) * np.linalg.norm(e) / (1e-6 * np.sqrt(2 * len(c.obj)))
    fig = dict(rms=res[0], proj_over_gate=float(proj), iterations=res[12], status=res[13])
    check("rational", fig, keys=())
    assert res[0] <= 1e-6
    consistent(res, c)


def test_identical_cameras_give_the_identity_rig_and_solve_pnp_poses():
    c = exact_case("17x65")
    g1 = c.g[6:18]
    K, D = CC.guess_KD(g1, 5)
    res = api.stereo_calibrate(c.off, c.obj, c.img1, c.img1, SC.SIZE, K1=K, D1=D, K2=K, D2=D, flags=api.CV_CALIB_FIX_INTRINSIC,
                               max_count=MAXC, eps=EPS)
    r, t, e, st = api.solve_pnp(c.obj, c.img1, c.off, K, D)
    assert np.all(st == api.PNP_SOLVED)
    om = SC.rotvec(res[5])
    fig = dict(om=float(np.abs(om).max()), T=float(np.abs(res[6]).max()), dr=float(np.abs(res[9] - r).max()),
               dt=float(np.abs(res[10] - t).max()), rms=res[0], status=res[13])
    check("identical", fig, keys=())
    assert np.array_equal(res[1], K) and np.array_equal(res[3], K) and np.array_equal(res[2], D) and np.array_equal(res[4], D)
    # rounding level: the exact cases' rotations are good to 1e-15 and their translations to 1e-12 mm (MEASURED);
    # three decades above that, whatever is measured here
    assert fig["om"] <= 1e-12 and fig["T"] <= 1e-9
    assert res[0] <= 1e-8
    check("identical", fig, keys=("dr", "dt"))


def test_a_correct_rig_guess_with_fixed_intrinsics_stays():
    c = exact_case("5x20")
    res = run(c, SC.FIX_INTRINSIC | SC.USE_EXTRINSIC_GUESS, 5, c.g[6:18], c.g[18:30], c.g[0:6])
    g = slots(res)
    fig = dict(dom=float(np.abs(g[0:3] - c.g[0:3]).max()), dT=float(np.abs(g[3:6] - c.g[3:6]).max()), rms=res[0],
               iterations=res[12], status=res[13])
    check("rig_stays", fig, keys=())
    assert np.array_equal(g[6:30], c.g[6:30])
    assert res[0] <= 1e-8
    # not beyond the reference's own step: what npstereocalib resolves of a rig (REF_RESOLUTION)
    assert fig["dom"] <= 10 * SC.REF_RESOLUTION["dom"] and fig["dT"] <= 10 * SC.REF_RESOLUTION["dT"]


def test_two_calls_are_bitwise_equal():
    _, c, flags, nd, guess1, guess2, rig = NOISY["ragged9"]
    a, b = run(c, flags, nd, guess1, guess2), run(c, flags, nd, guess1, guess2)
    assert a[0] == b[0] and a[12:] == b[12:]
    for x, y in zip(a[1:12], b[1:12]):
        assert np.array_equal(x, y)
    a, b = run(NOISY["flags0"][1]), run(NOISY["flags0"][1])
    assert a[0] == b[0] and a[12:] == b[12:]
    for x, y in zip(a[1:12], b[1:12]):
        assert np.array_equal(x, y)


def test_permuting_the_views_permutes_the_poses():
    _, c, flags, nd, guess1, guess2, rig = NOISY["ragged9"]
    order = np.random.default_rng(9).permutation(c.n_views)
    a, b = run(c, flags, nd, guess1, guess2), run(c.permuted(order), flags, nd, guess1, guess2)
    fig = figures(b, slots(a), np.hstack([a[9], a[10]])[order])
    fig.update(drms=abs(a[0] - b[0]) / a[0])
    print("FIG", json.dumps({"case": "permuted", **fig}))
    assert fig["drms"] <= 1e-12
    assert np.all(np.abs(a[11][order] - b[11]) <= 1e-9 * a[11][order])     # a view's rms goes with the view
    check("permuted", fig)


def test_the_stop_criteria_one_at_a_time():
    # from a guess: from the closed-form start the two internal calibrateCamera calls have converged already (under
    # the same criteria) and the joint loop ends after one step whatever is set
    c = exact_case("3x88")
    a = (c, SC.USE_GUESS, 5, c.g[6:18] * 1.01, c.g[18:30] * 1.01)
    count = run(*a, max_count=3, eps=1.0, crit_type=api.MCC_CRIT_COUNT)      # eps is not read
    both = run(*a, max_count=3, eps=1.0, crit_type=api.MCC_CRIT_COUNT_EPS)
    eps = run(*a, max_count=1, eps=1e-13, crit_type=api.MCC_CRIT_EPS)        # max_count is not read
    print("FIG", json.dumps({"case": "criteria", "count": count[12:14], "both": both[12:14], "eps": eps[12:14]}))
    assert count[12] == 3 and count[13] == api.CALIB_COUNT
    assert both[12] == 1 and both[13] == api.CALIB_CONVERGED
    assert eps[12] > 1 and eps[13] == api.CALIB_CONVERGED


def test_a_single_fronto_parallel_view_pair_ends():
    c = SC.make([88], seed=41, fronto=True)
    res = run(c, SC.FIX_INTRINSIC, 5, c.g[6:18], c.g[18:30])
    print("FIG", json.dumps({"case": "fronto/fix_intrinsic", "rms": res[0], "iterations": res[12], "status": res[13]}))
    assert res[13] in (api.CALIB_CONVERGED, api.CALIB_COUNT, api.CALIB_STALLED)
    assert all(np.all(np.isfinite(x)) for x in res[:12])
    try:
        res = run(c)     # all intrinsics free: one view does not determine them
    except api.MccError as e:
        print("FIG", json.dumps({"case": "fronto/free", "error": str(e)}))
        assert "(-3)" in str(e) or "(-1)" in str(e)
        return
    print("FIG", json.dumps({"case": "fronto/free", "rms": res[0], "iterations": res[12], "status": res[13]}))
    assert res[13] in (api.CALIB_CONVERGED, api.CALIB_COUNT, api.CALIB_STALLED)
    assert all(np.all(np.isfinite(x)) for x in res[:12])
