"""mcc_calibrate_camera's Levenberg-Marquardt steps on the GPU, one by one against a dense reference.

tests/test_calibrate_camera.py asks whether the loop ends at the least-squares minimum, which depends only on the
residual and on J^T e: Levenberg-Marquardt absorbs an error in U, W, V, the damping, the column solves, the
packed contribution, the reduced solve, the back-substitution, the reuse of the stored sums after a rejected
trial or the lambda schedule, and converges by another path.  Here every accepted step is compared with the step
npcalib.lm_step takes from the same point (complex-step Jacobian, lstsq on the augmented matrix).

The state after k accepted steps is calibrate_camera(flags | USE_GUESS, max_count = k, eps = 0): two calls are
bitwise equal, so the run to k + 1 passes through the run to k.  State 0 is the guess with the library's edits
(calib_cases.state0) and api.solve_pnp's poses at it.  For k = 0 .. K - 1 (K = 6):

  * iterations == k + 1;
  * r_k = trials_(k+1) - trials_k - 1, the rejections before step k + 1, equals the reference's count from the
    device's state k at lambda_k 10^j (lambda_k by the documented policy); every decision on these walks is clear,
    |en / err - 1| >= 1e-9 (tests/test_pincalib_step_cpu.py), where device and reference differ near 1e-14;
  * while the step is checked (gamma >= 1e-4 and rms >= 1e-4 px at state k: calib_cases.step_checked),
    rho = |J (d_gpu - d_ref)| / |J d_ref| against lm_step(state k, lambda_k 10^r_k) is within 10 x the figure
    measured on an MI355X (MEASURED, DESIGN.md 7g: two correct solvers differ by rounding and summation order),
    and within 1e-6 whatever was measured: two decades under what a wrong W entry, lambda I for lambda diag or a
    dropped corner give (1e-4 to 3e-2);
  * fixed slots are bitwise unchanged, and under FIX_ASPECT_RATIO fx == a fy exactly;
  * rms and every view_rms[v] equal npcalib's at the returned parameters within 1e-12 relative, or within one
    spacing of a 1280 px coordinate (2.3e-13 px) where that is more: a residual is a difference of pixels, so
    a view that fits to 1e-3 px (four-corner views, exact data) is not known to 1e-12 of itself by anyone.  The
    floor is that spacing and not 10 x the measured 3.7e-14 px because it is a property of the number format,
    known before anything is measured, as the 1e-12 it stands next to is: one unit in the last place of the
    largest coordinate a residual is formed from.  It happens to be 6 x the measurement.

Each step starts from the device's own previous iterate, so nothing drifts.  At least three steps per case are
checked.  5x20/near_zero_view has a view with |r_v| < 1e-2 on every step: k_pc_lin's run of so3_jac's series
(tests/test_pincalib_step_cpu.py asserts that it stays there).  Not covered: steps with gamma < 1e-4, the stall path, rational models under noise.
"""
import json

import numpy as np
import pytest

import calib_cases as CC
import npcalib
from multi_camera_calibration_amd import api

pytestmark = pytest.mark.gpu

CASES = {x[0]: x for x in CC.step_cases()}
RHO_CEILING = 1e-6
PIXEL_SPACING = float(np.spacing(1280.0))

# the largest rho over the checked steps, measured on an MI355X
MEASURED = {
    "ragged9/far": 6.95e-10,
    "17x65/aspect": 2.93e-10,
    "5x20/nd4_pp": 1.90e-13,
    "10x88/rational_k5": 6.49e-11,
    "65x4": 1.75e-11,
    "5x20/near_zero_view": 2.83e-11,
}


def globals_of(K, D):
    g = np.zeros(12)
    g[:4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    g[4:4 + len(D)] = D
    return g


def view_rms(c, g, poses):
    e = npcalib.residuals(c, g, poses).reshape(-1, 2)
    return np.array([np.sqrt((e[c.view(v)] ** 2).sum() / (c.off[v + 1] - c.off[v])) for v in range(c.n_views)])


@pytest.mark.parametrize("name", list(CASES))
def test_every_step_is_the_reference_step(name):
    _, c, flags, nd, guess = CASES[name]
    mask = api.calib_mask(flags, nd)
    free = [k for k in range(12) if mask[k]]
    g0, aspect = CC.state0(flags, nd, guess)
    fixed = [k for k in range(12) if not mask[k] and not (k == 0 and aspect > 0)]
    K0, D0 = CC.guess_KD(guess, nd)
    r, t, _, st = api.solve_pnp(c.obj, c.img, c.off, np.array([[g0[0], 0, g0[2]], [0, g0[1], g0[3]], [0, 0, 1.0]]), g0[4:12],
                                max_iter=50)
    assert np.all(st == api.PNP_SOLVED)
    g, poses, trials = g0, np.hstack([r, t]), 0
    lam, figs, fails = 1e-3, [], []
    for k in range(CC.K_STEPS):
        res = api.calibrate_camera(c.off, c.obj, c.img, CC.SIZE, K=K0, D=D0, flags=flags, nd=nd, max_count=k + 1, eps=0.0,
                                   return_ms=True)
        g1, poses1 = globals_of(res[1], res[2]), np.hstack([res[3], res[4]])
        assert res[6] == k + 1 and res[7] == api.CALIB_COUNT, (name, k, res[6], res[7])
        rej = res[9] - trials - 1
        j, (dg, dp, J, e), ratios = npcalib.lm_rejections(c, g, poses, mask, lam, aspect)
        gam, rms0 = npcalib.gamma(c, g, poses, mask, aspect, (J, e)), npcalib.rms(c, g, poses)
        lam_used = lam
        for _ in range(rej):
            lam_used = lam_used * 10.0
        if rej != j:
            dg, dp, J, e = npcalib.lm_step(c, g, poses, mask, lam_used, aspect, (J, e))
        rho = npcalib.rho(J, free, (g1 - g, poses1 - poses), (dg, dp))
        checked = CC.step_checked(gam, rms0)
        rms_ref, vr_ref = npcalib.rms(c, g1, poses1), view_rms(c, g1, poses1)
        fig = dict(case=name, step=k, lam=lam_used, gamma=gam, rms=res[0], rejections=int(rej), ref_rejections=j,
                   ratios=ratios, checked=bool(checked), rho=rho, drms=abs(res[0] - rms_ref) / rms_ref,
                   dview_rel=float(np.max(np.abs(res[5] - vr_ref) / vr_ref)), dview_abs=float(np.max(np.abs(res[5] - vr_ref))))
        print("FIG", json.dumps(fig))
        figs.append(fig)
        if rej != j:
            fails.append((k, "rejections", int(rej), j))
        if checked and not rho <= min(10.0 * MEASURED[name], RHO_CEILING):
            fails.append((k, "rho", rho))
        if not np.array_equal(g1[fixed], g[fixed]):
            fails.append((k, "a fixed slot moved", g1[fixed] - g[fixed]))
        if aspect > 0 and g1[0] != aspect * g1[1]:
            fails.append((k, "fx != a fy", g1[0], aspect * g1[1]))
        if not abs(res[0] - rms_ref) <= max(1e-12 * rms_ref, PIXEL_SPACING):
            fails.append((k, "rms", res[0], rms_ref))
        if not np.all(np.abs(res[5] - vr_ref) <= np.maximum(1e-12 * vr_ref, PIXEL_SPACING)):
            fails.append((k, "view_rms", fig["dview_rel"], fig["dview_abs"]))
        g, poses, trials = g1, poses1, res[9]
        lam = max(lam_used * 0.1, 1e-12)
    n_checked = sum(f["checked"] for f in figs)
    print("FIG", json.dumps(dict(case=name, checked=n_checked, rho_max=max(f["rho"] for f in figs if f["checked"]))))
    assert not fails, fails
    assert n_checked >= 3
    if name == "ragged9/far":
        # relin = 0 mid-run: a rejected trial, then the stored sums at another lambda in a step that is checked
        assert any(f["rejections"] > 0 and f["checked"] and f["step"] > 0 for f in figs)
