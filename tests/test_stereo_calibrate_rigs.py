"""mcc_stereo_calibrate on the GPU on rigs and view poses off the one rig of tests/test_stereo_calibrate.py.

What k_ps_lin adds over calibrateCamera is the pair of maps A = blockdiag(R Jl(r_v), R) and
B = [[Jl(om), 0], [-[R t_v]x Jl(om), I]].  On that file's rig (0.06 rad, T along -x) Jl(om), its transpose and
the identity are within 3 % of each other, R t_v is close to R^T t_v, and two columns of the dT block hardly carry
weight.  stereo_calib_cases.RIGS has rigs on which they do not: no rotation at all and a rotation under so3_jac's
series threshold, a 23 degree toe-in, a quarter turn about the optical axis with the baseline along y, one camera
ahead of the other, and two half turns, where the rig's start has to take the views' logarithms from one side of
pi (mcc_stereo_init_extrinsics).  `poses` keeps the old rig and has one view almost parallel to the image plane
(|r_v| < 1e-2: the series again) and one rolled by 3.1 rad.

max_count = 200, eps = 1e-13.  Gates that are fixed: rms equal to tests/npstereocalib.py's within 1e-6 relative,
every view_rms within 1e-9 relative of the reference's projection at the returned parameters, rms <= 1e-8 px on
exact data.  The parameter bounds are 10 x the figure measured on an MI355X (MEASURED), against the
reference 10 x that figure or 10 x stereo_calib_cases.RIG_REF_RESOLUTION, whichever is larger.  Rotations, the
rig's and the views', are compared by the angle between them (stereo_calib_cases.rot_angle), never by a difference
of rotation vectors: at a half turn r and r (1 - 2 pi / |r|) are the same rotation.  Every test prints its
figures before it asserts.  The steps on the way: tests/test_stereo_calibrate_steps.py on rig_step_cases().
"""
import json

import numpy as np
import pytest

import npcalib
import npstereocalib as NS
import stereo_calib_cases as SC
from test_stereo_calibrate import consistent, run

pytestmark = pytest.mark.gpu

KEYS = ("dK", "dD", "dom", "dT", "dr", "dt")

# measured on an MI355X: as tests/test_stereo_calibrate.py's, with dom and dr the largest angle (rad)
# between the returned rotation and the reference's
MEASURED = {
    "noisy/rot0/flags0": dict(dK=9.70e-13, dD=5.71e-11, dom=4.43e-13, dT=1.63e-11, dr=1.55e-13, dt=1.06e-10),
    "noisy/rot0/fix_intrinsic": dict(dK=0.00e+00, dD=0.00e+00, dom=3.45e-14, dT=2.50e-11, dr=2.24e-13, dt=3.32e-11),
    "noisy/series/flags0": dict(dK=7.08e-13, dD=3.91e-11, dom=3.13e-13, dT=1.41e-11, dr=1.92e-13, dt=1.76e-10),
    "noisy/series/fix_intrinsic": dict(dK=0.00e+00, dD=0.00e+00, dom=2.20e-15, dT=1.55e-12, dr=2.37e-13, dt=6.59e-12),
    "noisy/toe_in/flags0": dict(dK=2.93e-12, dD=2.23e-12, dom=3.56e-12, dT=5.14e-10, dr=1.47e-12, dt=1.42e-09),
    "noisy/toe_in/fix_intrinsic": dict(dK=0.00e+00, dD=0.00e+00, dom=1.58e-14, dT=9.89e-12, dr=3.97e-11, dt=3.43e-10),
    "noisy/roll90/flags0": dict(dK=6.66e-13, dD=2.25e-11, dom=4.90e-13, dT=1.62e-11, dr=5.88e-13, dt=5.77e-10),
    "noisy/roll90/fix_intrinsic": dict(dK=0.00e+00, dD=0.00e+00, dom=8.78e-11, dT=6.16e-08, dr=1.21e-09, dt=1.56e-07),
    "noisy/forward/flags0": dict(dK=2.05e-13, dD=7.55e-12, dom=1.47e-13, dT=3.92e-12, dr=1.50e-13, dt=1.77e-10),
    "noisy/forward/fix_intrinsic": dict(dK=0.00e+00, dD=0.00e+00, dom=5.45e-15, dT=2.34e-12, dr=3.44e-12, dt=2.50e-10),
    "noisy/upside_down/flags0": dict(dK=9.44e-13, dD=6.31e-11, dom=3.82e-13, dT=7.95e-12, dr=1.78e-13, dt=1.60e-10),
    "noisy/upside_down/fix_intrinsic": dict(dK=0.00e+00, dD=0.00e+00, dom=3.99e-16, dT=2.66e-13, dr=4.28e-14, dt=5.23e-12),
    "noisy/half_turn_tilted/flags0": dict(dK=1.53e-13, dD=2.88e-12, dom=9.17e-14, dT=2.39e-11, dr=4.75e-14, dt=2.39e-11),
    "noisy/half_turn_tilted/fix_intrinsic": dict(dK=0.00e+00, dD=0.00e+00, dom=1.74e-12, dT=1.34e-09, dr=3.79e-12, dt=1.41e-09),
    "noisy/upside_down16/flags0": dict(dK=1.61e-11, dD=2.99e-10, dom=1.39e-11, dT=2.33e-10, dr=1.29e-11, dt=1.39e-08),
    "noisy/upside_down16/fix_intrinsic": dict(dK=0.00e+00, dD=0.00e+00, dom=1.49e-11, dT=9.01e-09, dr=4.66e-11, dt=7.59e-09),
    "noisy/poses/flags0": dict(dK=2.00e-13, dD=2.90e-12, dom=1.27e-13, dT=6.33e-12, dr=4.44e-14, dt=4.31e-11),
    "noisy/poses/fix_intrinsic": dict(dK=0.00e+00, dD=0.00e+00, dom=5.51e-16, dT=1.87e-13, dr=2.43e-13, dt=7.39e-12),
    "exact/5x20/rot0": dict(dom=3.62e-15, dT=8.53e-14),
    "exact/5x20/series": dict(dom=2.69e-16, dT=2.03e-13),
    "exact/5x20/toe_in": dict(dom=5.71e-15, dT=9.09e-13),
    "exact/5x20/roll90": dict(dom=2.14e-15, dT=1.07e-12),
    "exact/5x20/forward": dict(dom=4.40e-15, dT=5.19e-13),
    "exact/5x20/upside_down": dict(dom=5.51e-15, dT=3.57e-13),
    "exact/5x20/half_turn_tilted": dict(dom=8.51e-15, dT=1.11e-12),
    "noisy/same_focal_no_guess": dict(dK=1.92e-09, dD=1.46e-09, dom=9.39e-10, dT=4.58e-08, dr=1.37e-09, dt=1.61e-06),
}


def slots(res):
    """The 30 slots of a result, om as a rotation vector of R at whatever angle."""
    g = np.zeros(30)
    g[0:3], g[3:6] = SC.log_so3(res[5]), res[6]
    for base, K, D in ((6, res[1], res[2]), (18, res[3], res[4])):
        g[base:base + 4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        g[base + 4:base + 4 + len(D)] = D
    return g


def figures(res, g_ref, poses_ref):
    g = slots(res)
    rel = lambda s: float(np.max(np.abs(g[s] - g_ref[s]) / np.abs(g_ref[s])))
    return dict(dK=max(rel(slice(6, 10)), rel(slice(18, 22))),
                dD=float(max(np.abs(g[10:18] - g_ref[10:18]).max(), np.abs(g[22:30] - g_ref[22:30]).max())),
                dom=SC.rot_angle(res[5], npcalib.rodrigues(g_ref[0:3])), dT=float(np.abs(g[3:6] - g_ref[3:6]).max()),
                dr=max(SC.rot_angle(npcalib.rodrigues(a), npcalib.rodrigues(b)) for a, b in zip(res[9], poses_ref[:, :3])),
                dt=float(np.abs(res[10] - poses_ref[:, 3:]).max()))


def check(name, fig, keys, floor):
    assert name in MEASURED, f"no measured figures for {name}"
    for k in keys:
        bound = 10.0 * max(MEASURED[name][k], floor[k] if floor else 0.0)
        assert fig[k] <= bound, (name, k, fig[k], bound)


def against_reference(key, c, res, ref, floor):
    """What every noisy test here asserts of a result, given the reference's minimum."""
    g, poses = slots(res), np.hstack([res[9], res[10]])
    fig = figures(res, ref["g"], ref["poses"])
    fig.update(drms=abs(res[0] - ref["rms"]) / ref["rms"], rms=res[0], iterations=res[12], status=res[13])
    n = np.diff(c.off)[:, None]
    vr = np.sqrt(NS.view_sq(c, g, poses) / n)
    fig.update(dview=float(np.max(np.abs(res[11] - vr) / vr)))
    print("REF", json.dumps({"case": key, **SC.resolution(ref)}))
    print("FIG", json.dumps({"case": key, **fig}))
    assert fig["drms"] <= 1e-6
    consistent(res, c)
    assert res[11].shape == (c.n_views, 2)
    assert np.all(np.abs(res[11] - vr) <= 1e-9 * vr)
    check(key, fig, KEYS, floor)
    return g


RIG_NOISY = {x[0]: x for x in SC.rig_noisy_cases()}


@pytest.mark.parametrize("name", list(RIG_NOISY))
def test_noisy_rig_reaches_the_reference_minimum(name):
    _, c, flags, nd, guess1, guess2, rig = RIG_NOISY[name]
    res = run(c, flags, nd, guess1, guess2, rig)
    g = against_reference("noisy/" + name, c, res, SC.reference(name), SC.RIG_REF_RESOLUTION)
    if flags & SC.FIX_INTRINSIC:
        assert np.array_equal(g[6:30], np.concatenate([guess1, guess2]))         # bit-equal to the input


@pytest.mark.parametrize("rig", list(SC.RIGS))
def test_exact_rig_from_the_median_start(rig):
    """Exact 5 x 20 from intrinsics 1 % off under USE_INTRINSIC_GUESS: the rig starts at mcc_stereo_init_extrinsics
    of the two cameras' solvePnP poses."""
    c = SC.exact_rig(rig)
    res = run(c, SC.USE_GUESS, 5, c.g[6:18] * 1.01, c.g[18:30] * 1.01)
    fig = dict(dom=SC.rot_angle(res[5], npcalib.rodrigues(c.g[0:3])), dT=float(np.abs(res[6] - c.g[3:6]).max()), rms=res[0],
               iterations=res[12], status=res[13])
    key = "exact/5x20/" + rig
    print("FIG", json.dumps({"case": key, **fig}))
    assert res[0] <= 1e-8
    consistent(res, c)
    check(key, fig, ("dom", "dT"), None)


def test_same_focal_length_without_a_guess():
    """SAME_FOCAL_LENGTH from the closed-form start (the mean of two separately converged cameras) on the noisy
    17 x 88 of tests/test_stereo_calibrate.py: the minimum is guess_same_focal's, whatever the start."""
    c = SC.noisy_cases()[0][1]
    res = run(c, SC.SAME_FOCAL, 5)
    against_reference("noisy/same_focal_no_guess", c, res, SC.reference("guess_same_focal"), SC.REF_RESOLUTION)
    assert res[3][0, 0] == res[1][0, 0] and res[3][1, 1] == res[1][1, 1]
