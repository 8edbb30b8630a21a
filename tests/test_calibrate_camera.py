"""mcc_calibrate_camera on the GPU: cv::calibrateCamera's least-squares minimum, by Levenberg-Marquardt.

Every test runs with max_count = 200 and eps = 1e-13, so that convergence is tested, not OpenCV's default
budget.  The reference is tests/npcalib.py (dense Gauss-Newton on central differences, started from the truth);
tests/test_calibrate_camera_cpu.py checks that it handles every noisy case used here.

Gates that are fixed: rms <= 1e-8 px on exact data; rms equal to the reference's within 1e-6 relative under
noise (rms is second order in the parameter error); gamma = sqrt(g^T H^-1 g) / |e| never above 1e-4 (an rms
excess of about gamma^2 / 2 then stays far inside the 1e-6 gate).  The parameter bounds, and gamma's tighter
one, are 10 x the figure measured on an MI355X and recorded in DESIGN.md 7g (MEASURED below): two converged
solvers differ by their stopping points.  Against npcalib the recorded figure is the measured difference or the
reference's own resolution, whichever is larger: calib_cases.REF_RESOLUTION, constants measured once (the
largest last Gauss-Newton step and the largest gamma at its own minimum over the noisy cases), which
tests/test_calibrate_camera_cpu.py holds npcalib to; a difference below them says nothing about the device.
Every test prints its figures before it asserts.  Whether each step on the way is the right one is
tests/test_calibrate_camera_steps.py's question.
"""
import json

import numpy as np
import pytest

import calib_cases as CC
import npcalib
from multi_camera_calibration_amd import api

pytestmark = pytest.mark.gpu

MAXC, EPS = 200, 1e-13

# measured on an MI355X: dK max relative error of fx fy cx cy, dD max absolute error of D, dr / dt
# max absolute error of the rotation vectors / translations (mm), against the truth (exact) or npcalib (noisy)
MEASURED = {
    "exact/3x88": dict(dK=1.33e-15, dD=2.06e-14, dr=6.66e-16, dt=7.96e-13),
    "exact/4x6": dict(dK=3.82e-14, dD=6.76e-11, dr=2.94e-14, dt=2.34e-11),
    "exact/4x20": dict(dK=5.02e-15, dD=1.96e-12, dr=2.25e-15, dt=5.00e-12),
    "exact/17x64": dict(dK=2.42e-16, dD=3.70e-14, dr=6.38e-16, dt=2.27e-13),
    "exact/17x65": dict(dK=3.63e-16, dD=1.81e-13, dr=5.00e-16, dt=2.27e-13),
    "exact/17x88": dict(dK=1.26e-16, dD=3.40e-15, dr=6.38e-16, dt=1.14e-13),
    "exact/ragged9": dict(dK=6.05e-16, dD=3.51e-14, dr=2.55e-15, dt=4.55e-13),
    "exact/65x20": dict(dK=1.94e-15, dD=5.49e-14, dr=2.05e-15, dt=1.59e-12),
    "exact/10x20": dict(dK=1.18e-14, dD=9.30e-12, dr=9.38e-15, dt=8.60e-12),
    "exact/24x4": dict(dK=2.43e-14, dD=1.11e-09, dr=4.15e-14, dt=2.66e-11),
    "noisy/17x64": dict(dK=4.10e-09, dD=2.60e-07, dr=2.10e-09, dt=2.56e-06, gamma=3.59e-08),
    "noisy/17x65": dict(dK=1.44e-09, dD=3.37e-08, dr=8.33e-10, dt=9.12e-07, gamma=2.61e-08),
    "noisy/17x88": dict(dK=1.28e-09, dD=2.64e-10, dr=6.62e-10, dt=6.91e-07, gamma=2.69e-08),
    "noisy/k3_tangent": dict(dK=4.63e-10, dD=3.56e-10, dr=3.28e-10, dt=3.50e-07, gamma=1.49e-08),
    "noisy/principal": dict(dK=2.93e-11, dD=7.10e-10, dr=5.02e-11, dt=3.05e-08, gamma=7.80e-10),
    "noisy/aspect": dict(dK=4.19e-10, dD=8.77e-10, dr=2.16e-10, dt=2.26e-07, gamma=2.34e-08),
    "noisy/focal": dict(dK=4.64e-10, dD=1.02e-10, dr=3.40e-10, dt=3.51e-07, gamma=2.18e-08),
    "noisy/relief": dict(dK=3.80e-10, dD=4.08e-10, dr=2.94e-10, dt=3.26e-07, gamma=1.56e-08),
    "noisy/ragged9": dict(dK=6.06e-10, dD=4.54e-09, dr=3.42e-10, dt=3.19e-07, gamma=2.57e-08),
    "noisy/nd4": dict(dK=8.31e-10, dD=3.09e-11, dr=4.18e-10, dt=4.48e-07, gamma=6.38e-09),
    "noisy/fix_k1_k2": dict(dK=3.11e-10, dD=7.24e-11, dr=2.18e-10, dt=2.20e-07, gamma=1.20e-08),
    "all_fixed": dict(dr=0.00e+00, dt=0.00e+00),
    "rational": dict(proj_over_gate=1.37e-05),
    "permuted": dict(dr=1.02e-10, dt=1.14e-07),
}


def run(c, flags=0, nd=5, guess=None, K=None, max_count=MAXC, eps=EPS, crit_type=api.MCC_CRIT_COUNT_EPS):
    D = None
    if guess is not None:
        K, D = CC.guess_KD(guess, nd)
    return api.calibrate_camera(c.off, c.obj, c.img, CC.SIZE, K=K, D=D, flags=flags, nd=nd, max_count=max_count, eps=eps,
                                crit_type=crit_type)


def globals_of(K, D):
    g = np.zeros(12)
    g[:4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    g[4:4 + len(D)] = D
    return g


def figures(res, g_ref, poses_ref):
    rms, K, D, rvec, tvec = res[:5]
    g = globals_of(K, D)
    return dict(dK=float(np.max(np.abs(g[:4] - g_ref[:4]) / np.abs(g_ref[:4]))), dD=float(np.max(np.abs(g[4:] - g_ref[4:]))),
                dr=float(np.max(np.abs(rvec - poses_ref[:, :3]))), dt=float(np.max(np.abs(tvec - poses_ref[:, 3:]))))


def check(name, fig, keys=("dK", "dD", "dr", "dt"), against_reference=False):
    if not keys:
        print("FIG", json.dumps({"case": name, **fig}))
    assert name in MEASURED, f"no measured figures for {name}"
    for k in keys:
        bound = 10.0 * max(MEASURED[name][k], CC.REF_RESOLUTION[k] if against_reference else 0.0)
        assert fig[k] <= bound, (name, k, fig[k], bound)


EXACT = {"3x88": [88] * 3, "4x6": [6] * 4, "4x20": [20] * 4, "17x64": [64] * 17, "17x65": [65] * 17, "17x88": [88] * 17,
         "ragged9": list(CC.RAGGED), "65x20": [20] * 65,
         "10x20": [20] * 10}   # groups of ceil(sqrt(n)) views: 10 = 4 + 4 + 2; 3 = 2 + 1 is one above the group size


@pytest.mark.parametrize("name", list(EXACT))
def test_exact_data_from_the_closed_form_start(name):
    c = CC.make(EXACT[name], seed=300 + len(EXACT[name]) + EXACT[name][0])
    res = run(c)
    fig = figures(res, c.g, c.poses)
    fig.update(rms=res[0], iterations=res[6], status=res[7])
    check("exact/" + name, fig, keys=())
    assert res[0] <= 1e-8
    assert np.all(np.isfinite(res[5])) and np.all(res[5] <= 1e-8 * np.sqrt(len(c.obj)))
    check("exact/" + name, fig)


def test_exact_four_corner_views_from_a_guess():
    """The documented minimum of four corners per view: 24 views, a guess 1 % off."""
    c = CC.make([4] * 24, seed=328)
    res = run(c, CC.USE_GUESS, 5, c.g * 1.01)
    fig = figures(res, c.g, c.poses)
    fig.update(rms=res[0], iterations=res[6], status=res[7])
    check("exact/24x4", fig, keys=())
    assert res[0] <= 1e-8
    assert np.all(np.isfinite(res[5])) and np.all(res[5] <= 1e-8 * np.sqrt(len(c.obj)))
    check("exact/24x4", fig)


NOISY = {x[0]: x for x in CC.noisy_cases()}
_REF = {}


def reference(name):
    """npcalib's minimum for a noisy case, computed once."""
    if name not in _REF:
        _, c, flags, nd, guess = NOISY[name]
        mask = api.calib_mask(flags, nd)
        aspect = c.g[0] / c.g[1] if flags & CC.FIX_ASPECT else 0.0
        g, poses, r, steps, (dg, dp) = npcalib.gauss_newton(c, CC.reference_start(c, flags, mask, guess), c.poses, mask,
                                                            aspect, return_last=True)
        err = dict(dK=float(np.max(np.abs(dg[:4] / g[:4]))), dD=float(np.max(np.abs(dg[4:]))),
                   dr=float(np.max(np.abs(dp[:, :3]))), dt=float(np.max(np.abs(dp[:, 3:]))),
                   gamma=npcalib.gamma(c, g, poses, mask, aspect))
        _REF[name] = (g, poses, r, mask, aspect, err)
    return _REF[name]


@pytest.mark.parametrize("name", list(NOISY))
def test_noisy_data_reaches_the_reference_minimum(name):
    _, c, flags, nd, guess = NOISY[name]
    g_ref, poses_ref, rms_ref, mask, aspect, ref_err = reference(name)
    K_in = np.diag([c.g[0], c.g[1], 1.0]) if flags & CC.FIX_ASPECT else None
    res = run(c, flags, nd, guess, K=K_in)
    rms, K, D, rvec, tvec = res[:5]
    fig = figures(res, g_ref, poses_ref)
    fig.update(gamma=npcalib.gamma(c, globals_of(K, D), np.hstack([rvec, tvec]), mask, aspect),
               drms=abs(rms - rms_ref) / rms_ref, rms=rms, iterations=res[6], status=res[7])
    print("REF", json.dumps({"case": name, **ref_err}))
    check("noisy/" + name, fig, keys=())
    assert fig["drms"] <= 1e-6
    assert fig["gamma"] <= 1e-4
    check("noisy/" + name, fig, keys=("gamma", "dK", "dD", "dr", "dt"), against_reference=True)
    assert abs(np.sqrt((res[5] ** 2 * np.diff(c.off)).sum() / len(c.obj)) - rms) <= 1e-12 * rms
    # every view's rms against the reference's projection at the returned parameters: a view's error in its own slot
    e = npcalib.residuals(c, globals_of(K, D), np.hstack([rvec, tvec])).reshape(-1, 2)
    vr = np.array([np.sqrt((e[c.view(v)] ** 2).sum() / (c.off[v + 1] - c.off[v])) for v in range(c.n_views)])
    print("FIG", json.dumps({"case": name, "dview": float(np.max(np.abs(res[5] - vr) / vr))}))
    assert np.all(np.abs(res[5] - vr) <= 1e-9 * vr)
    if name == "nd4":
        assert len(D) == 4
    if name == "fix_k1_k2":
        assert D[0] == guess[4] and D[1] == guess[5]                # bit-equal to the input
    if name == "principal":
        assert K[0, 2] == guess[2] and K[1, 2] == guess[3]          # bit-equal to the input
    if name == "focal":
        assert K[0, 0] == guess[0] and K[1, 1] == guess[1]
    if name == "aspect":
        a = c.g[0] / c.g[1]
        assert abs(K[0, 0] / K[1, 1] - a) <= np.spacing(a)
    if name == "k3_tangent":
        assert D[2] == 0 and D[3] == 0 and D[4] == 0


def test_everything_fixed_is_solve_pnp():
    c = NOISY["17x88"][1]
    g = c.g.copy()
    g[6:8] = 0.0   # ZERO_TANGENT_DIST
    res = run(c, CC.ALL_FIXED, 5, g)
    rms, K, D, rvec, tvec = res[:5]
    assert np.array_equal(globals_of(K, D), g)
    r, t, e, st = api.solve_pnp(c.obj, c.img, c.off, K, D)
    assert np.all(st == api.PNP_SOLVED)
    rms_pnp = np.sqrt((e ** 2 * np.diff(c.off)).sum() / len(c.obj))
    fig = dict(dr=float(np.abs(rvec - r).max()), dt=float(np.abs(tvec - t).max()), drms=abs(rms - rms_pnp) / rms_pnp)
    check("all_fixed", fig, keys=())
    assert fig["drms"] <= 1e-6
    check("all_fixed", fig, keys=("dr", "dt"))


def test_rational_model_from_a_guess():
    c = CC.make([88] * 40, seed=340, g=CC.G_RATIONAL)
    res = run(c, CC.RATIONAL | CC.USE_GUESS, 8, c.g * 1.01)
    rms, K, D, rvec, tvec = res[:5]
    mask = api.calib_mask(CC.RATIONAL, 8)
    # On exact data |e| is rounding and so is its projection on the Jacobian's column space, so their ratio gamma
    # says nothing.  What is gated instead is that projection against a residual of 1e-6 px, the rms gate:
    # proj_over_gate = |P e| / (1e-6 sqrt(corners)), the share of the allowed rms that a step could still remove.
    x = np.hstack([rvec, tvec])
    e = npcalib.residuals(c, globals_of(K, D), x)
    proj = npcalib.gamma(c, globals_of(K, D), x, mask) * np.linalg.norm(e) / (1e-6 * np.sqrt(len(c.obj)))
    fig = dict(rms=rms, proj_over_gate=float(proj), iterations=res[6], status=res[7])
    check("rational", fig, keys=())
    assert rms <= 1e-6
    assert fig["proj_over_gate"] <= 1e-4
    check("rational", fig, keys=("proj_over_gate",))


def test_two_calls_are_bitwise_equal():
    c = NOISY["17x65"][1]
    a, b = run(c), run(c)
    assert a[0] == b[0] and a[6] == b[6] and a[7] == b[7]
    for x, y in zip(a[1:6], b[1:6]):
        assert np.array_equal(x, y)
    # the same views behind seven corners that belong to no view (view_off[0] = 7): the same bits
    pad = np.full((7, 3), 1e30)
    d = api.calibrate_camera(c.off + 7, np.vstack([pad, c.obj]), np.vstack([pad[:, :2], c.img]), CC.SIZE, max_count=MAXC,
                             eps=EPS)
    assert a[0] == d[0] and a[6] == d[6]
    for x, y in zip(a[1:6], d[1:6]):
        assert np.array_equal(x, y)


def test_permuting_the_views_permutes_the_poses():
    c = NOISY["17x65"][1]
    order = np.random.default_rng(9).permutation(c.n_views)
    a, b = run(c), run(c.permuted(order))
    fig = dict(drms=abs(a[0] - b[0]) / a[0], dr=float(np.abs(a[3][order] - b[3]).max()),
               dt=float(np.abs(a[4][order] - b[4]).max()))
    print("FIG", json.dumps({"case": "permuted", **fig}))
    assert fig["drms"] <= 1e-12
    check("permuted", fig, keys=("dr", "dt"))


def test_one_accepted_step():
    c = NOISY["17x88"][1]
    res = run(c, max_count=1)
    assert res[6] == 1 and res[7] == api.CALIB_COUNT
    assert np.isfinite(res[0]) and res[0] < 10.0   # one step from the closed-form start


def test_the_stop_criteria_one_at_a_time():
    # exact data: a noisy case such as 17x88 ends "stalled" at its minimum when eps is 1e-13 (ten trials in a row
    # that rounding rejects), whichever criteria are set; exact/3x88 converges in 9 steps under both
    c = CC.make(EXACT["3x88"], seed=300 + 3 + 88)
    count = run(c, max_count=3, eps=1.0, crit_type=api.MCC_CRIT_COUNT)      # eps is not read
    both = run(c, max_count=3, eps=1.0, crit_type=api.MCC_CRIT_COUNT_EPS)
    eps = run(c, max_count=1, eps=1e-13, crit_type=api.MCC_CRIT_EPS)        # max_count is not read
    print("FIG", json.dumps({"case": "criteria", "count": count[6:8], "both": both[6:8], "eps": eps[6:8]}))
    assert count[6] == 3 and count[7] == api.CALIB_COUNT
    assert both[6] == 1 and both[7] == api.CALIB_CONVERGED
    assert eps[6] > 1 and eps[7] == api.CALIB_CONVERGED


def test_a_single_fronto_parallel_view_ends():
    X = CC.grid(88)
    img = npcalib.project(X, np.zeros(3), np.array([0.0, 0.0, 800.0]), CC.G_TRUE)
    c = CC.Case(np.array([0, 88], np.int32), X, img, CC.G_TRUE, np.zeros((1, 6)))
    try:
        res = run(c)
    except api.MccError as e:
        print("FIG", json.dumps({"case": "fronto", "error": str(e)}))
        assert "(-3)" in str(e)
        return
    print("FIG", json.dumps({"case": "fronto", "rms": res[0], "iterations": res[6], "status": res[7]}))
    assert res[7] == api.CALIB_STALLED
    assert all(np.all(np.isfinite(x)) for x in res[:6])
