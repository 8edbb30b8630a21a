"""Batched solvePnP (api.solve_pnp -> k_pnp) away from the one pose and the one object frame of
tests/test_pnp_batch.py, against references that are not k_pnp: the truth on exact data, and on noisy
data tests/nppnp.py (a Gauss-Newton from the true pose with a central-difference Jacobian, which knows
neither the closed-form start nor the LM policy that k_pnp shares with host/pnp.cpp).

a. Exact data over the regimes of the rotation code (theta = 0, 1e-9, 5e-3: the identity return of
   rodrigues_v2m, the s < 1e-5 / c > 0 branch of rodrigues_m2v, the series of so3_jac; theta = pi,
   pi - 1e-7, pi - 1e-4 about three axes: the diagonal branch of rodrigues_m2v and an LM start of length
   pi; theta = 3.0 and 3.11; a 69 degree tilt), over two object frames (centred and axis-aligned, and the
   same target moved by r = (0.7, -0.5, 0.3), t = (5000, -3000, 2000) mm: the plane frame's eigenvector
   order and det flip, the sign of H[8] * lam, t = th - R c with a centroid 6 m away), planar and with
   60 mm relief, n in {20, 88} plus the minima n = 4 (planar) and n = 6, every accepted nd (0, 4, 5, 8,
   12, the last with non-zero s1..s4), max_iter 50 and 0.  Bounds, those of test_pnp_batch.py: status
   SOLVED, 0 <= rms < 1e-6 px, |dr| < 1e-7, |dt| < 1e-4 + 1e-7 |c| mm (c the target's centroid: the
   rotation bound times the lever arm of t = th - R c).  Where the true angle is above 3.1 the rotations
   are compared as matrices, |R(r) - R(r_true)|_max < 1e-7, since r and -r are one rotation at pi.
   Two views (n = 4 and n = 5, relief 0.3 mm) are planar to the solver only: their closed-form pose
   (max_iter = 0) is a homography fitted to points that are not on a plane, exact for no pose, so at
   max_iter = 0 they are held to status SOLVED and a start LM can use (rms < 10 px; the relief alone is
   worth 0.4 mm * f / Z = 0.3 px, the four-point homography's decomposition multiplies it), and to the
   full bounds at max_iter = 50.
b. 0.2 px noise against nppnp.refine: every view SOLVED, rms in (0.1, 0.5) px (the chi-square argument of
   test_pnp_batch.py), |rms - rms_ref| <= 1e-6 rms_ref (the project's "different minimum" bar), the pose
   within 10 x what mcc::pnp::solvePnP differs from nppnp.refine on these views, and nppnp.stationarity at
   the returned pose within 10 x what it is at the host solver's and at refine's own poses, and below 1e-4
   whatever was measured.  The views: the four targets of (a), four poses (one at pi), n in {20, 88}, nd in
   {0, 5, 12}; and a relief sweep a in {1e-3 .. 15} mm of the 40 mm grid at nd = 5, six poses and five
   draws per cell, which is where the planarity test matters: while it was w0 <= 1e-9 w2 a board some
   micrometres to a few millimetres off its plane went through the 12-vector DLT and came back SOLVED
   with an rms of up to 43 px.
c. The distortion stride and the first offset: three cameras with different K and D; nd in {4, 5, 8, 12}
   equals, bit for bit, the call with D zero-padded to twelve columns; view_off[0] = 7 with seven leading
   NaN corners equals the rebased call.
d. max_n and the workgroup shape: nine noisy views (planar 881 and 1 024, non-planar 880 and 129, five
   of 20 corners) solved together (three waves per workgroup, the LDS slice of 1 024 corners), each alone,
   and the small ones with the 880-corner view (four waves per workgroup): all bitwise equal.
e. The non-planar path past two strides of the wave: exact data at n in {129, 200, 1 024}, nd in {0, 8}.

Measured on the CPU (host solver and NumPy reference only, never k_pnp), seeds SEED_MAIN and SEED_SWEEP:
  mcc::pnp::solvePnP against nppnp.refine over the 636 views of (b)
      rotation 1.285e-07 (rad, or matrix entry at pi), |dt| 4.792e-06 mm centred / 1.038e-03 mm moved target
      (the moved target's centroid is 6.2 m from the origin: its t carries the rotation's difference times that)
  nppnp.stationarity: 5.024e-07 at the host solver's poses, 5.837e-07 at refine's own (a run that stops when
      the sum of squares no longer decreases stops where gamma^2 is near 1e-16 over its own rounding)
The bounds below are 10 x those.  The one-lane CPU replay of k_pnp's arithmetic gives 1.1e-07, 8.5e-06,
5.8e-04 and 9.9e-07 on the same views (for orientation only: the bounds do not come from it), and with the
thin-prism terms dsx of pnp_rows set to zero gamma is 1.7e-05 to 4.4e-05 on 31 of the 32 views with nd = 12.

The sweep has a = 4 and 15 mm beside the issue's seven: with the threshold first tried, w0 <= 1e-3 w1, both
solvers still lost 13 of 360 views at n = 20 and a = 3, 4 and 6 mm (w0 / w1 from 2.1e-3 to 8.4e-3, rms 2.5 to
35 px, SOLVED), so the test became w0 <= 3e-2 w1: a = 10 mm at n = 20 (2.3e-2) is a plane, 15 mm (5.2e-2) is not.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import npmodel as N  # noqa: E402
import nppnp as P  # noqa: E402
from multi_camera_calibration_amd import api  # noqa: E402

K0 = np.array([[1200.0, 0, 960], [0, 1180, 540], [0, 0, 1]])
K3 = np.stack([K0, np.array([[900.0, 0, 640], [0, 905, 360], [0, 0, 1]]),
               np.array([[1500.0, 0, 1000], [0, 1490, 700], [0, 0, 1]])])
_D8 = [-0.12, 0.08, 2e-4, 1e-4, 0.01, 0.002, -0.001, 0.003]
DS = {0: np.zeros(0), 4: np.array([-0.1, 0.05, 1e-4, -2e-4]), 5: np.array([-0.1, 0.05, 1e-4, -2e-4, 0.01]),
      8: np.array(_D8), 12: np.array(_D8 + [1e-3, -5e-4, -8e-4, 3e-4])}
# three cameras' twelve coefficients, none zero, no two columns alike
D3 = np.stack([DS[12], [-0.08, 0.03, -3e-4, 2e-4, 0.004, 0.001, 0.002, -0.001, -6e-4, 2e-4, 5e-4, -3e-4],
               [0.05, -0.02, 1e-4, 3e-4, -0.006, -0.002, 0.001, 0.002, 4e-4, 3e-4, -7e-4, 1e-4]])
PI = np.pi
POSES = [((0.0, 0.0, 0.0), (40.0, -30.0, 1300.0)),
         ((1e-9, 0.0, 0.0), (-60.0, 20.0, 1100.0)),
         ((0.0, 5e-3, 0.0), (25.0, 45.0, 1500.0)),
         ((PI, 0.0, 0.0), (-35.0, 30.0, 1250.0)),
         ((0.0, PI - 1e-7, 0.0), (50.0, -20.0, 1400.0)),
         ((2.2, -2.2, 0.01), (-20.0, -40.0, 1200.0)),
         (((PI - 1e-4) * 0.6, (PI - 1e-4) * 0.8, 0.0), (30.0, 25.0, 1350.0)),
         ((0.1, 0.1, 3.0), (-45.0, 35.0, 1150.0)),
         ((1.2, 0.1, -0.2), (20.0, -25.0, 1450.0))]
POSES = [(np.array(r), np.array(t)) for r, t in POSES]
RO, TO = N.rodrigues([0.7, -0.5, 0.3]), np.array([5000.0, -3000.0, 2000.0])
NEAR_PI = 3.1   # above this true angle the rotations are compared as matrices

BOUND_RMS, BOUND_R, BOUND_T = 1e-6, 1e-7, 1e-4   # exact data (tests/test_pnp_batch.py)
SEED_MAIN, SEED_SWEEP, SEED_CAMS, SEED_SHAPES = 20240917, 20240918, 20240919, 20240920
NOISE = 0.2
# 10 x the CPU measurements of the docstring
BOUND_NOISY_R, BOUND_NOISY_T, BOUND_NOISY_T_MOVED, BOUND_GAMMA = 1.285e-6, 4.792e-5, 1.038e-2, 5.837e-6
HARD_GAMMA = 1e-4


def target(n, relief=0.0, pitch=40.0, centred=True):
    """n points of a near-square grid with z = relief * (sin(0.7 b + 1.3 a) + 0.4 cos(0.37 i)) mm."""
    w = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    a, b = i % w, i // w
    z = relief * (np.sin(0.7 * b + 1.3 * a) + 0.4 * np.cos(0.37 * i))
    obj = np.stack([pitch * a, pitch * b, z], 1)
    if centred:
        obj[:, :2] -= 0.5 * (obj[:, :2].max(0) + obj[:, :2].min(0))
    return obj


def moved(obj, pose):
    """The target moved by (RO, TO), and the pose that sees it at the same pixels."""
    return obj @ RO.T + TO, P.compose_truth(pose, RO, TO)


def _batch(views):
    off = np.concatenate([[0], np.cumsum([len(v["obj"]) for v in views])]).astype(np.int32)
    return np.concatenate([v["obj"] for v in views]), np.concatenate([v["img"] for v in views]), off


def rot_diff(r, r_true):
    """|dr|, or the largest matrix entry's difference where the true angle is near pi."""
    if np.linalg.norm(r_true) > NEAR_PI:
        return np.abs(N.rodrigues(r) - N.rodrigues(r_true)).max()
    return np.abs(np.asarray(r) - r_true).max()


# ---------------------------------------------------------------- a. exact data across the regimes
def exact_views(nd):
    """The views of (a) for one distortion length: dicts of obj, img, the true pose and a label."""
    D, views = DS[nd], []

    def add(obj, pose, label, near_planar=False):
        r, t = pose
        views.append(dict(obj=obj, img=N.project_pinhole(obj, r, t, K0, D), r=np.asarray(r), t=np.asarray(t),
                          label=label, near_planar=near_planar))

    for ip, pose in enumerate(POSES):
        for n in (20, 88):
            for relief in (0.0, 60.0):
                obj = target(n, relief)
                add(obj, pose, f"pose{ip} n{n} relief{relief:g} centred")
                add(*moved(obj, pose), f"pose{ip} n{n} relief{relief:g} moved")
    for ip in (0, 3):
        add(target(4, 0.0, 160.0), POSES[ip], f"pose{ip} n4 planar")
        add(target(6, 60.0, 160.0), POSES[ip], f"pose{ip} n6 relief60")
        add(*moved(target(4, 0.0, 160.0), POSES[ip]), f"pose{ip} n4 planar moved")
    # planar to the solver only (w0 / w1 = 2e-5 and 8e-6): the homography start, then LM on the true points
    add(target(4, 0.3, 160.0), POSES[8], "pose8 n4 relief0.3", near_planar=True)
    add(target(5, 0.3, 160.0), POSES[8], "pose8 n5 relief0.3", near_planar=True)
    return views


def check_exact(views, res, max_iter):
    """The list of views that miss the exact-data bounds (empty when all hold)."""
    rvec, tvec, rms, status = res
    bad = []
    for i, v in enumerate(views):
        dr, dt = rot_diff(rvec[i], v["r"]), np.abs(tvec[i] - v["t"]).max()
        bt = BOUND_T + 1e-7 * np.linalg.norm(v["obj"].mean(0))
        if v["near_planar"] and max_iter == 0:
            ok = status[i] == api.PNP_SOLVED and 0 <= rms[i] < 10.0
        else:
            ok = status[i] == api.PNP_SOLVED and 0 <= rms[i] < BOUND_RMS and dr < BOUND_R and dt < bt
        if not ok:
            bad.append(f"{v['label']} max_iter {max_iter}: status {status[i]} rms {rms[i]:.3e} dr {dr:.3e} "
                       f"dt {dt:.3e} (bound {bt:.3e})")
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [50, 0])
@pytest.mark.parametrize("nd", sorted(DS))
def test_exact_data_across_rotation_regimes_and_object_frames(nd, max_iter):
    api.build()
    views = exact_views(nd)
    obj, img, off = _batch(views)
    res = api.solve_pnp(obj, img, off, K0, DS[nd] if nd else None, max_iter=max_iter)
    bad = check_exact(views, res, max_iter)
    rvec, tvec, rms, status = res
    print(f"nd {nd} max_iter {max_iter}: {len(views)} views, worst rms {rms.max():.3e}")
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- e. non-planar beyond two strides
def long_views(nd):
    views = []
    for n in (129, 200, 1024):
        obj = target(n, 60.0, 10.0 if n == 1024 else 40.0)
        for ip in (8, 7):
            r, t = POSES[ip]
            views.append(dict(obj=obj, img=N.project_pinhole(obj, r, t, K0, DS[nd]), r=r, t=t,
                              label=f"pose{ip} n{n} relief60", near_planar=False))
    return views


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [50, 0])
@pytest.mark.parametrize("nd", [0, 8])
def test_exact_data_non_planar_beyond_two_strides(nd, max_iter):
    api.build()
    views = long_views(nd)
    obj, img, off = _batch(views)
    res = api.solve_pnp(obj, img, off, K0, DS[nd] if nd else None, max_iter=max_iter)
    bad = check_exact(views, res, max_iter)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- b. noisy data against the reference
SWEEP_RELIEF = [1e-3, 1e-2, 0.1, 0.3, 1.0, 3.0, 4.0, 10.0, 15.0]
SWEEP_POSES = [(0.3, -0.4, 0.2, -150, -90, 1300), (-0.2, 0.35, -0.1, -250, -180, 900),
               (0.05, 0.02, 1.4, 150, -200, 1800), (0.8727, 0.05, 0.0, -200, -100, 1400),
               (-0.5, -0.3, 0.6, -100, -150, 1100), (0.1, -0.7, -0.2, -50, -120, 1500)]


def noisy_views():
    """The views of (b): 96 over targets, poses, n and nd, then the relief sweep at nd = 5 (540)."""
    views = []
    rng = np.random.default_rng(SEED_MAIN)
    for nd in (0, 5, 12):
        for ip in (0, 3, 7, 8):
            for n in (20, 88):
                for relief in (0.0, 60.0):
                    for mv in (False, True):
                        obj, pose = target(n, relief), POSES[ip]
                        if mv:
                            obj, pose = moved(obj, pose)
                        img = N.project_pinhole(obj, pose[0], pose[1], K0, DS[nd])
                        views.append(dict(obj=obj, img=img + NOISE * rng.normal(size=img.shape), r=pose[0], t=pose[1],
                                          nd=nd, moved=mv, label=f"nd{nd} pose{ip} n{n} relief{relief:g} moved{int(mv)}"))
    rng = np.random.default_rng(SEED_SWEEP)
    for a in SWEEP_RELIEF:
        for n in (20, 88):
            obj = target(n, a, centred=False)
            for ip, p in enumerate(SWEEP_POSES):
                r, t = np.array(p[:3], float), np.array(p[3:], float)
                img = N.project_pinhole(obj, r, t, K0, DS[5])
                for draw in range(5):
                    views.append(dict(obj=obj, img=img + NOISE * rng.normal(size=img.shape), r=r, t=t, nd=5,
                                      moved=False, label=f"sweep a{a:g} n{n} pose{ip} draw{draw}"))
    return views


def reference(views):
    """nppnp.refine from the true pose, stored in each view as r_ref, t_ref, rms_ref."""
    for v in views:
        v["r_ref"], v["t_ref"], v["rms_ref"] = P.refine(v["obj"], v["img"], K0, DS[v["nd"]], v["r"], v["t"])
    return views


def check_noisy(views, res):
    """Every figure of (b) for the poses in res: the failing views, and the maxima for the record."""
    rvec, tvec, rms, status = res
    bad, top = [], dict(rel=0.0, dr=0.0, dt=0.0, dt_moved=0.0, gamma=0.0)
    for i, v in enumerate(views):
        if status[i] != api.PNP_SOLVED:
            bad.append(f"{v['label']}: status {status[i]}")
            continue
        rel = abs(rms[i] - v["rms_ref"]) / v["rms_ref"]
        dr, dt = rot_diff(rvec[i], v["r_ref"]), np.abs(tvec[i] - v["t_ref"]).max()
        gamma = P.stationarity(v["obj"], v["img"], K0, DS[v["nd"]], rvec[i], tvec[i])
        bt = BOUND_NOISY_T_MOVED if v["moved"] else BOUND_NOISY_T
        for k, x in (("rel", rel), ("dr", dr), ("dt_moved" if v["moved"] else "dt", dt), ("gamma", gamma)):
            top[k] = max(top[k], x)
        if not (0.1 < rms[i] < 0.5 and rel <= 1e-6 and dr <= BOUND_NOISY_R and dt <= bt
                and gamma <= BOUND_GAMMA and gamma < HARD_GAMMA):
            bad.append(f"{v['label']}: rms {rms[i]:.6f} ref {v['rms_ref']:.6f} rel {rel:.3e} dr {dr:.3e} dt {dt:.3e} "
                       f"gamma {gamma:.3e}")
    return bad, top


@pytest.fixture(scope="module")
def noisy():
    api.build()
    views = reference(noisy_views())
    out = [np.zeros((len(views), 3)), np.zeros((len(views), 3)), np.zeros(len(views)), np.zeros(len(views), np.int32)]
    # one launch per distortion length of the first 96 views, two for the sweep
    groups = [[i for i, v in enumerate(views[:96]) if v["nd"] == nd] for nd in (0, 5, 12)]
    groups += [list(range(96, 96 + 270)), list(range(96 + 270, len(views)))]
    for g in groups:
        nd = views[g[0]]["nd"]
        obj, img, off = _batch([views[i] for i in g])
        res = api.solve_pnp(obj, img, off, K0, DS[nd] if nd else None)
        for o, r in zip(out, res):
            o[g] = r
    return views, out


@pytest.mark.gpu
def test_noisy_views_reach_the_reference_minimum(noisy):
    views, res = noisy
    bad, top = check_noisy(views[:96], [x[:96] for x in res])
    print("targets x poses x n x nd:", {k: f"{x:.3e}" for k, x in top.items()})
    assert not bad, f"{len(bad)} of 96\n" + "\n".join(bad[:40])


@pytest.mark.gpu
def test_near_planar_relief_sweep_reaches_the_reference_minimum(noisy):
    views, res = noisy
    bad, top = check_noisy(views[96:], [x[96:] for x in res])
    print("relief sweep:", {k: f"{x:.3e}" for k, x in top.items()})
    assert not bad, f"{len(bad)} of {len(views) - 96}\n" + "\n".join(bad[:40])


# ---------------------------------------------------------------- c. distortion stride and first offset
@pytest.fixture(scope="module")
def three_cams():
    api.build()
    rng = np.random.default_rng(SEED_CAMS)
    views, cams = [], []
    for v in range(30):
        cam, n = v % 3, (20, 88)[(v // 3) % 2]
        obj = target(n, 60.0 if (v // 6) % 2 else 0.0)
        r, t = POSES[8][0] + rng.uniform(-0.2, 0.2, 3), POSES[8][1] + rng.uniform(-50, 50, 3)
        views.append(dict(obj=obj, r=r, t=t, noise=NOISE * rng.normal(size=(n, 2))))
        cams.append(cam)
    return views, np.array(cams, np.int32)


def _project_all(views, cams, D):
    for v, c in zip(views, cams):
        v["img"] = N.project_pinhole(v["obj"], v["r"], v["t"], K3[c], D[c]) + v["noise"]
    return _batch(views)


@pytest.mark.gpu
@pytest.mark.parametrize("nd", [4, 5, 8, 12])
def test_short_distortion_rows_equal_the_rows_padded_to_twelve(three_cams, nd):
    views, cams = three_cams
    D = np.ascontiguousarray(D3[:, :nd])
    obj, img, off = _project_all(views, cams, D)
    pad = np.zeros((3, 12))
    pad[:, :nd] = D
    a = api.solve_pnp(obj, img, off, K3, D, view_cam=cams)
    b = api.solve_pnp(obj, img, off, K3, pad, view_cam=cams)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    # the coefficients were used at all: every camera's views are solved to the noise, none to more
    assert (a[3] == api.PNP_SOLVED).all() and (a[2] > 0.1).all() and (a[2] < 0.5).all(), (a[3], a[2])


@pytest.mark.gpu
def test_a_first_offset_of_seven_equals_the_rebased_call(three_cams):
    views, cams = three_cams
    obj, img, off = _project_all(views, cams, D3)
    a = api.solve_pnp(obj, img, off, K3, D3, view_cam=cams)
    obj7 = np.concatenate([np.full((7, 3), np.nan), obj])
    img7 = np.concatenate([np.full((7, 2), np.nan), img])
    b = api.solve_pnp(obj7, img7, off + 7, K3, D3, view_cam=cams)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert (a[3] == api.PNP_SOLVED).all() and np.isfinite(a[0]).all()


# ---------------------------------------------------------------- d. max_n and the workgroup shape
@pytest.mark.gpu
def test_result_does_not_depend_on_max_n_or_the_workgroup_shape():
    api.build()
    rng = np.random.default_rng(SEED_SHAPES)
    views = []
    for n, relief in [(881, 0.0), (20, 0.0), (1024, 0.0), (20, 60.0), (880, 60.0), (20, 0.0), (129, 60.0), (20, 60.0),
                      (20, 0.0)]:
        obj = target(n, relief, 10.0 if n > 200 else 40.0)
        r, t = POSES[8][0] + rng.uniform(-0.2, 0.2, 3), POSES[8][1] + rng.uniform(-50, 50, 3)
        img = N.project_pinhole(obj, r, t, K0, DS[8]) + NOISE * rng.normal(size=(n, 2))
        views.append(dict(obj=obj, img=img))
    obj, img, off = _batch(views)
    full = api.solve_pnp(obj, img, off, K0, DS[8])
    assert (full[3] == api.PNP_SOLVED).all() and (full[2] > 0.1).all() and (full[2] < 0.5).all(), (full[3], full[2])

    def same(res, j, i):
        return all(x[j:j + 1].tobytes() == y[i:i + 1].tobytes() for x, y in zip(res, full))

    for i, v in enumerate(views):
        one = api.solve_pnp(v["obj"], v["img"], [0, len(v["obj"])], K0, DS[8])
        assert same(one, 0, i), (i, len(v["obj"]), [x[0] for x in one], [x[i] for x in full])
    sub = [i for i, v in enumerate(views) if len(v["obj"]) in (20, 880)]   # max_n = 880: four waves per workgroup
    obj, img, off = _batch([views[i] for i in sub])
    res = api.solve_pnp(obj, img, off, K0, DS[8])
    for j, i in enumerate(sub):
        assert same(res, j, i), (i, [x[j] for x in res], [x[i] for x in full])
