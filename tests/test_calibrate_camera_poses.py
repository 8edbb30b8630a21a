"""mcc_calibrate_camera with a view almost parallel to the image plane, and one rolled by 3.1 rad.

calib_cases draws every view tilted by 10 to 45 degrees, so no calibrateCamera test has a view with |r_v| < 1e-2,
where so3_jac (k_pc_lin's Jl(r_v)) takes its series.  Camera 1 of stereo_calib_cases' `poses` case has one
(view NEAR_ZERO_VIEW, 4e-3 rad at the minimum) among 17 x 88 noisy views; view ROLLED_VIEW is rolled by 3.1 rad.
The reference is tests/npcalib.py from the truth, the gates are tests/test_calibrate_camera.py's with this
case's own measured figures, and rotations are compared by the angle between them.  The steps through that
branch one by one: 5x20/near_zero_view of calib_cases.step_cases().
"""
import json

import numpy as np
import pytest

import calib_cases as CC
import npcalib
import stereo_calib_cases as SC
from multi_camera_calibration_amd import api

MAXC, EPS = 200, 1e-13

# measured on an MI355X; dr is the largest angle between a returned view rotation and the reference's
MEASURED = {"noisy/poses": dict(dK=7.25e-10, dD=4.23e-10, dr=3.69e-10, dt=4.46e-07, gamma=7.04e-09)}

_REF = {}


def reference():
    if not _REF:
        c = SC.rig_cases()["poses"].camera(0)
        mask = api.calib_mask(0, 5)
        g, poses, r, steps, (dg, dp) = npcalib.gauss_newton(c, c.g.copy(), c.poses, mask, 0.0, return_last=True)
        err = dict(dK=float(np.max(np.abs(dg[:4] / g[:4]))), dD=float(np.max(np.abs(dg[4:]))), dr=float(np.max(np.abs(dp[:, :3]))),
                   dt=float(np.max(np.abs(dp[:, 3:]))), gamma=npcalib.gamma(c, g, poses, mask, 0.0))
        _REF.update(c=c, g=g, poses=poses, rms=r, steps=steps, mask=mask, err=err)
    return _REF


def test_the_reference_resolves_the_case_and_the_view_is_in_the_series_branch():
    api.build()
    ref = reference()
    nz = float(np.linalg.norm(ref["poses"][SC.NEAR_ZERO_VIEW, :3]))
    print("FIG", json.dumps(dict(case="poses/camera1", steps=ref["steps"], rms=ref["rms"], near_zero_view=nz, **ref["err"])))
    assert ref["steps"] <= 50
    for k, v in ref["err"].items():
        assert v <= CC.REF_RESOLUTION[k], (k, v)
    assert nz < 1e-2


@pytest.mark.gpu
def test_noisy_views_with_a_near_zero_and_a_rolled_one_reach_the_reference_minimum():
    ref = reference()
    c, mask = ref["c"], ref["mask"]
    rms, K, D, rvec, tvec, vrms = api.calibrate_camera(c.off, c.obj, c.img, CC.SIZE, max_count=MAXC, eps=EPS)[:6]
    g = np.zeros(12)
    g[:4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    g[4:4 + len(D)] = D
    x = np.hstack([rvec, tvec])
    fig = dict(dK=float(np.max(np.abs(g[:4] - ref["g"][:4]) / np.abs(ref["g"][:4]))), dD=float(np.max(np.abs(g[4:] - ref["g"][4:]))),
               dr=max(SC.rot_angle(npcalib.rodrigues(a), npcalib.rodrigues(b)) for a, b in zip(rvec, ref["poses"][:, :3])),
               dt=float(np.max(np.abs(tvec - ref["poses"][:, 3:]))), gamma=npcalib.gamma(c, g, x, mask, 0.0),
               drms=abs(rms - ref["rms"]) / ref["rms"], rms=rms, near_zero_view=float(np.linalg.norm(rvec[SC.NEAR_ZERO_VIEW])))
    e = npcalib.residuals(c, g, x).reshape(-1, 2)
    vr = np.array([np.sqrt((e[c.view(v)] ** 2).sum() / (c.off[v + 1] - c.off[v])) for v in range(c.n_views)])
    fig.update(dview=float(np.max(np.abs(vrms - vr) / vr)))
    print("REF", json.dumps({"case": "noisy/poses", **ref["err"]}))
    print("FIG", json.dumps({"case": "noisy/poses", **fig}))
    assert fig["drms"] <= 1e-6
    assert fig["gamma"] <= 1e-4
    assert fig["near_zero_view"] < 1e-2
    assert np.all(np.abs(vrms - vr) <= 1e-9 * vr)
    assert "noisy/poses" in MEASURED, "no measured figures"
    for k in ("gamma", "dK", "dD", "dr", "dt"):
        bound = 10.0 * max(MEASURED["noisy/poses"][k], CC.REF_RESOLUTION[k])
        assert fig[k] <= bound, (k, fig[k], bound)
