"""Seeded synthetic stereo views for the pinhole stereoCalibrate tests (tests/test_stereo_calibrate*.py,
tests/test_pinstereo_step_cpu.py), built from calib_cases' grid and pose distribution.

Camera 1 is calib_cases.G_TRUE; camera 2 is a second intrinsic set a few percent off, 120 mm to the right of
camera 1 and turned by about 3.5 degrees.  A view's pose is drawn as calib_cases.make draws it and drawn again
until every corner is in front of both cameras and inside 1280 x 960 in both.

RIGS, rig_cases() and rig_step_cases() are other rigs (no rotation, a toe-in, a quarter turn, one camera ahead,
two half turns) and `poses`, views off that pose distribution; the tests on them compare rotations by rot_angle.
"""
from __future__ import annotations

import dataclasses

import numpy as np

import calib_cases as CC
import npcalib
import npstereocalib as NS

SIZE = CC.SIZE
G1_TRUE = CC.G_TRUE
G2_TRUE = np.array([925.0, 921.0, 630.0, 488.0, -0.23, 0.07, -8e-4, 6e-4, 0.0, 0.0, 0.0, 0.0])
G2_RATIONAL = np.array([925.0, 921.0, 630.0, 488.0, -0.23, 0.07, -8e-4, 6e-4, 0.012, 0.018, -0.008, 0.004])
OM_TRUE = np.array([0.02, -0.055, 0.012])
T_TRUE = np.array([-120.0, 3.0, 6.0])

# cv::CALIB_* (include/mcc.h: MCC_CALIB_*)
FIX_INTRINSIC, SAME_FOCAL, USE_EXTRINSIC_GUESS = 256, 512, 1 << 22
USE_GUESS, FIX_ASPECT, FIX_PP, ZERO_TANGENT, FIX_FOCAL = CC.USE_GUESS, CC.FIX_ASPECT, CC.FIX_PP, CC.ZERO_TANGENT, CC.FIX_FOCAL
FIX_K1, FIX_K2, FIX_K3, FIX_K4, FIX_K5, FIX_K6, RATIONAL = CC.FIX_K1, CC.FIX_K2, CC.FIX_K3, CC.FIX_K4, CC.FIX_K5, CC.FIX_K6, CC.RATIONAL
CAMERA_FLAGS = USE_GUESS | FIX_ASPECT | FIX_PP | ZERO_TANGENT | FIX_FOCAL | FIX_K1 | FIX_K2 | FIX_K3 | FIX_K4 | FIX_K5 | FIX_K6 | RATIONAL


@dataclasses.dataclass
class StereoCase:
    off: np.ndarray     # [V + 1]
    obj: np.ndarray     # [C, 3]
    img1: np.ndarray    # [C, 2]
    img2: np.ndarray    # [C, 2]
    g: np.ndarray       # [30] the parameters the pixels were made with: om T | camera 1 | camera 2
    poses: np.ndarray   # [V, 6] (rvec, tvec) of the views in camera 1

    @property
    def n_views(self):
        return len(self.off) - 1

    def view(self, v):
        return slice(int(self.off[v]), int(self.off[v + 1]))

    def permuted(self, order):
        sl = [self.view(v) for v in order]
        off = np.concatenate([[0], np.cumsum([s.stop - s.start for s in sl])]).astype(np.int32)
        cat = lambda a: np.concatenate([a[s] for s in sl])
        return StereoCase(off, cat(self.obj), cat(self.img1), cat(self.img2), self.g, self.poses[list(order)])

    def camera(self, c):
        """One camera's views as a calib_cases.Case (poses: the view's pose in that camera)."""
        if c == 0:
            return CC.Case(self.off, self.obj, self.img1, self.g[6:18], self.poses)
        R = npcalib.rodrigues(self.g[0:3])
        poses = np.array([np.concatenate([rotvec(R @ npcalib.rodrigues(p[:3])), R @ p[3:] + self.g[3:6]]) for p in self.poses])
        return CC.Case(self.off, self.obj, self.img2, self.g[18:30], poses)


def rotvec(R):
    """The rotation vector of R (angles well inside (0, pi) here)."""
    c = np.clip((np.trace(R) - 1.0) * 0.5, -1.0, 1.0)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = 0.5 * np.linalg.norm(v)
    th = np.arctan2(s, c)
    return v * (0.5 if th < 1e-12 else th / (2.0 * s))


def rot_angle(Ra, Rb):
    """The angle of Ra Rb^T, from atan2: good at 0 and at pi alike, and blind to which of a rotation's vectors
    (r, or r (1 - 2 pi / |r|)) either side was made from."""
    D = np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T
    s = 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return float(np.arctan2(s, (np.trace(D) - 1.0) * 0.5))


def log_so3(R):
    """A rotation vector of R at any angle in [0, pi]: rotvec's form while sin(angle) >= 0.1; nearer to a half turn
    the axis from the symmetric part, (R + R^T) / 2 = c I + (1 - c) a a^T, with the sign of the skew part."""
    R = np.asarray(R, np.float64)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.linalg.norm(v), (np.trace(R) - 1.0) * 0.5
    if s >= 0.1 or c > 0:
        return rotvec(R)
    S = 0.5 * (R + R.T) - c * np.eye(3)
    a = S[:, int(np.argmax(np.diag(S)))]
    a = a / np.linalg.norm(a)
    return (-a if a @ v < 0 else a) * np.arctan2(s, c)


def _inside(p):
    return bool(np.all(p[:, 0] > 0) and np.all(p[:, 0] < SIZE[0] - 1) and np.all(p[:, 1] > 0) and np.all(p[:, 1] < SIZE[1] - 1))


def make(corners, seed, noise=0.0, g1=G1_TRUE, g2=G2_TRUE, om=OM_TRUE, T=T_TRUE, fronto=False, x_mean=60.0, view_r=None):
    """One view pair per entry of `corners`.  fronto: targets parallel to camera 1's image plane.  x_mean: the mean x
    (mm, camera 1) of the target's position.  view_r: {view: rotation vector, or a function of the drawn one} for
    views whose rotation is prescribed; their position is still drawn (and drawn again) as every view's."""
    view_r = view_r or {}
    rng = np.random.default_rng(seed)
    g = np.concatenate([om, T, g1, g2]).astype(np.float64)
    R = npcalib.rodrigues(om)
    obj, img1, img2, poses, off = [], [], [], [], [0]
    for v, n in enumerate(corners):
        X = CC.grid(n)
        for _ in range(1000):
            tilt = 0.0 if fronto else np.deg2rad(rng.uniform(10.0, 45.0))
            phi = 2.399963 * v + rng.uniform(0.0, 0.5)
            r = np.array([tilt * np.cos(phi), tilt * np.sin(phi), 0.0 if fronto else rng.uniform(-0.3, 0.3)])
            if v in view_r:
                r = np.asarray(view_r[v](r) if callable(view_r[v]) else view_r[v], np.float64)
            t = np.array([rng.uniform(-60.0, 60.0) + x_mean, rng.uniform(-40.0, 40.0), rng.uniform(500.0, 1200.0)])
            pose = np.concatenate([r, t])
            p1, p2 = NS.project2(X, g, pose)
            Z1 = (X @ npcalib.rodrigues(r).T + t)
            Z2 = Z1 @ R.T + T
            if Z1[:, 2].min() > 100 and Z2[:, 2].min() > 100 and _inside(p1) and _inside(p2):
                break
        else:
            raise RuntimeError(f"no pose for view {v}")
        obj.append(X)
        img1.append(p1)
        img2.append(p2)
        poses.append(pose)
        off.append(off[-1] + n)
    img1, img2 = np.concatenate(img1), np.concatenate(img2)
    if noise:
        img1 = img1 + noise * rng.standard_normal(img1.shape)
        img2 = img2 + noise * rng.standard_normal(img2.shape)
    return StereoCase(np.asarray(off, np.int32), np.concatenate(obj), img1, img2, g, np.asarray(poses))


# ---------------------------------------------------------------- the rules of mcc_stereo_calib_mask, in Python
def mask_rules(flags, nd):
    """(mask [30], tie [30]): mask is 1 at a free slot; tie[k] is the slot that slot k follows (-1: none).
    Under FIX_ASPECT_RATIO a camera's fx follows its own fy; under SAME_FOCAL_LENGTH camera 2's fy follows camera
    1's fy and its fx camera 1's fx (its own fy by its own ratio when FIX_ASPECT_RATIO is set as well)."""
    mask, tie = np.zeros(30, np.int32), -np.ones(30, np.int32)
    mask[0:6] = 1
    focal, pp, tang = not flags & FIX_FOCAL, not flags & FIX_PP, not flags & ZERO_TANGENT
    rat = bool(flags & RATIONAL) and nd == 8
    cam = [focal and not flags & FIX_ASPECT, focal, pp, pp, not flags & FIX_K1, not flags & FIX_K2, tang, tang,
           nd >= 5 and not flags & FIX_K3, rat and not flags & FIX_K4, rat and not flags & FIX_K5, rat and not flags & FIX_K6]
    for base in (6, 18):
        mask[base:base + 12] = [int(bool(x)) for x in cam]
        if flags & FIX_ASPECT:
            tie[base] = base + 1
    if flags & SAME_FOCAL:
        mask[18] = mask[19] = 0
        tie[19] = 7
        if not flags & FIX_ASPECT:
            tie[18] = 6
    if flags & FIX_INTRINSIC:
        mask[6:30] = 0
        tie[:] = -1
    return mask, tie


def state0(flags, nd, guess1, guess2, rig):
    """The 30 slots mcc_stereo_calibrate starts from when the intrinsics and the rig are given (FIX_INTRINSIC or
    USE_INTRINSIC_GUESS, with USE_EXTRINSIC_GUESS), and the ties it holds (NS's form)."""
    if flags & FIX_INTRINSIC:
        g = np.concatenate([rig, pad12(guess1, nd), pad12(guess2, nd)])
        return g, NS.NO_TIES
    c1, a1 = CC.state0(flags, nd, guess1)
    c2, a2 = CC.state0(flags, nd, guess2)
    same = 1 if flags & SAME_FOCAL else 0
    if same:
        c1[0:2] = c2[0:2] = 0.5 * (c1[0:2] + c2[0:2])
    ties = (a1, a2, same)
    return NS.tied(np.concatenate([rig, c1, c2]), ties), ties


def pad12(guess, nd):
    g = np.zeros(12)
    g[:4 + nd] = np.asarray(guess, np.float64)[:4 + nd]
    return g


def reference_start(c, flags, mask, guess1, guess2):
    """The slots tests/npstereocalib.py starts from: the truth at the free slots, and at the fixed ones what the
    library holds there (the guess, or zero distortion without one)."""
    g = c.g.copy()
    for base, guess in ((6, guess1), (18, guess2)):
        for k in range(12):
            if not mask[base + k]:
                g[base + k] = guess[k] if guess is not None else (0.0 if k >= 4 else g[base + k])
    return g


def ties_of(flags, K1, K2):
    """NS's ties for a library call with these flags and input camera matrices."""
    if flags & FIX_INTRINSIC:
        return NS.NO_TIES
    a = lambda K: float(K[0, 0] / K[1, 1]) if flags & FIX_ASPECT and K is not None else 0.0
    return (a(K1), a(K2), 1 if flags & SAME_FOCAL else 0)


# What tests/npstereocalib.py resolves on the noisy cases below, measured once: its largest last
# Gauss-Newton step (dK relative in fx fy cx cy, dD, the rig's dom and dT in mm, the poses' dr and dt in mm) and
# its largest gamma at its own minimum.
# Measured maxima over the cases: dK 3.0e-10 (guess_same_focal), dD 2.3e-9, dr 2.5e-8, dt 2.8e-7, gamma 2.2e-9 (ragged9),
# dom 1.9e-10, dT 1.7e-8 (guess_same_focal); recorded here rounded up to one digit.
REF_RESOLUTION = dict(dK=4e-10, dD=3e-9, dom=2e-10, dT=2e-8, dr=3e-8, dt=3e-7, gamma=3e-9)


def noisy_cases():
    """(name, case, flags, nd, guess1, guess2, rig) of every noisy input of tests/test_stereo_calibrate.py: guess
    is the 12-vector handed over as K and D (None: zeros), rig the (om, T) handed over as R, T (None: none)."""
    c = make([88] * 17, seed=288, noise=0.2)
    g1, g2 = c.g[6:18], c.g[18:30]
    rig5 = np.concatenate([c.g[0:3] * 1.05, c.g[3:6] * 1.05])
    rat = make([88] * 40, seed=340, g1=CC.G_RATIONAL, g2=G2_RATIONAL)
    return [("flags0", c, 0, 5, None, None, None),
            ("fix_intrinsic", c, FIX_INTRINSIC, 5, g1, g2, None),
            ("guess_same_focal", c, USE_GUESS | SAME_FOCAL, 5, g1 * 1.01, g2 * 1.01, None),
            ("aspect", c, FIX_ASPECT, 5, g1, g2, None),
            ("k3_tangent", c, FIX_K3 | ZERO_TANGENT, 5, None, None, None),
            ("nd4", c, 0, 4, None, None, None),
            ("extrinsic_guess", c, USE_EXTRINSIC_GUESS, 5, None, None, rig5),
            ("ragged9", make(CC.RAGGED, seed=277, noise=0.2), USE_GUESS, 5, g1 * 1.01, g2 * 1.01, None),
            ("rational", rat, USE_GUESS | RATIONAL, 8, rat.g[6:18] * 1.01, rat.g[18:30] * 1.01, None)]


def step_cases():
    """(name, case, flags, nd, guess1, guess2, rig) of tests/test_stereo_calibrate_steps.py and
    tests/test_pinstereo_step_cpu.py: the smallest inputs whose Levenberg-Marquardt trajectory reaches each path
    of the trial kernels.  Every one gives the intrinsics and the rig, so that state 0 is known."""
    far = make(CC.RAGGED, seed=77, noise=0.2)
    f1, f2 = far.g[6:18].copy(), far.g[18:30].copy()
    f1[0:2] *= 1.5                  # far enough for a rejected trial: the stored arrow is read again
    f2[0:2] *= 1.5
    asp = make([65] * 17, seed=165, noise=0.2)
    fix = make([20] * 5, seed=129, noise=0.2)           # groups of 3 + 2 views
    four = make([4] * 65, seed=465, noise=0.2)          # groups of 9 views, the last of 2
    rig = lambda c, s: np.concatenate([c.g[0:3] * s, c.g[3:6] * s])
    E = USE_EXTRINSIC_GUESS
    return [("ragged9/far", far, USE_GUESS | E, 5, f1, f2, rig(far, 1.05)),
            ("17x65/aspect_same", asp, USE_GUESS | E | FIX_ASPECT | SAME_FOCAL, 5, asp.g[6:18] * 1.05, asp.g[18:30] * 1.05,
             rig(asp, 1.1)),
            # with the intrinsics fixed the problem is close to linear and a start 30 % off is at its minimum after
            # three steps; from half a radian and twice the baseline off all six steps are far from it, and the sixth
            # comes after seven rejections in a row
            ("5x20/fix_intrinsic_nd4", fix, FIX_INTRINSIC | E, 4, fix.g[6:18], fix.g[18:30],
             np.concatenate([fix.g[0:3] + [0.5, -0.6, 0.4], fix.g[3:6] * 2.0])),
            ("65x4/pp", four, USE_GUESS | E | FIX_PP, 5, four.g[6:18] * 1.01, four.g[18:30] * 1.01, rig(four, 1.05))]


# ---------------------------------------------------------------- rigs other than the one above
# name: (om, camera 2's centre C2 in camera 1's frame in mm, the mean x of the target's position); T = -R C2
RIGS = {
    "rot0": ((0.0, 0.0, 0.0), (120.0, 0.0, 0.0), 60.0),               # rodrigues_v2m's theta < eps branch, so3_jac's series
    "series": ((3e-3, -4e-3, 2e-3), (120.0, -3.0, 5.0), 60.0),         # so3_jac's series at a generic small vector
    "toe_in": ((0.03, 0.40, 0.02), (300.0, 5.0, 40.0), 150.0),         # a large Jl(om); R far from I in A and in [R t_v]x
    "roll90": ((0.02, -0.03, np.pi / 2), (10.0, 150.0, 0.0), 60.0),    # x and y exchanged, the baseline along y
    "forward": ((0.01, 0.02, -0.015), (5.0, -8.0, 150.0), 60.0),       # the baseline along z: the dT block's third column
    "upside_down": ((0.004, -0.006, np.pi - 5e-4), (120.0, 4.0, -3.0), 60.0),                 # within noise of a half turn
    "half_turn_tilted": (tuple(np.pi * np.array([np.sin(0.1), 0.0, np.cos(0.1)])), (200.0, 0.0, 0.0), 100.0),
}
HALF_TURN = ("upside_down", "half_turn_tilted")


def rig_of(name):
    """(om, T, x_mean) of a rig of RIGS."""
    om, C2, x_mean = RIGS[name]
    om = np.array(om, np.float64)
    return om, -npcalib.rodrigues(om) @ np.array(C2, np.float64), x_mean


def make_rig(name, corners, seed, noise=0.0, **kw):
    om, T, x_mean = rig_of(name)
    return make(corners, seed, noise, om=om, T=T, x_mean=x_mean, **kw)


def exact_rig(name):
    """Exact 5 x 20 (groups of 3 + 2 views) of a rig."""
    return make_rig(name, [20] * 5, seed=905)


_RIG_CASES = {}


def rig_cases():
    """{name: case}: noisy 17 x 88 of every rig of RIGS (seed 300, 0.2 px), upside_down once more with 16 views, and
    `poses` (below)."""
    if not _RIG_CASES:
        for name in RIGS:
            _RIG_CASES[name] = make_rig(name, [88] * 17, seed=300, noise=0.2)
        _RIG_CASES["upside_down16"] = make_rig("upside_down", [88] * 16, seed=300, noise=0.2)
        _RIG_CASES["poses"] = poses_case([88] * 17, seed=300)
    return _RIG_CASES


NEAR_ZERO_VIEW, ROLLED_VIEW = 2, 5
ROLL = 3.1


def rolled(r):
    """The drawn rotation turned by ROLL about the optical axis."""
    return log_so3(npcalib.rodrigues([0.0, 0.0, ROLL]) @ npcalib.rodrigues(r))


def near_zero(seed):
    """A view rotation N(0, 2e-3) per component: |r_v| under so3_jac's series threshold of 1e-2."""
    return np.random.default_rng(seed).normal(0.0, 2e-3, 3)


def poses_case(corners, seed, noise=0.2, **kw):
    """The rig of the module's head with two views off calib_cases' pose distribution: view NEAR_ZERO_VIEW almost
    parallel to camera 1's image plane, view ROLLED_VIEW rolled by 3.1 rad on top of its tilt."""
    return make(corners, seed, noise, view_r={NEAR_ZERO_VIEW: near_zero(seed + 1), ROLLED_VIEW: rolled}, **kw)


def rig_noisy_cases():
    """(name, case, flags, nd, guess1, guess2, rig) in noisy_cases()' form: every case of rig_cases() with flags 0 and
    with FIX_INTRINSIC at the true intrinsics."""
    out = []
    for name, c in rig_cases().items():
        out += [(name + "/flags0", c, 0, 5, None, None, None),
                (name + "/fix_intrinsic", c, FIX_INTRINSIC, 5, c.g[6:18], c.g[18:30], None)]
    return out


# What tests/npstereocalib.py resolves on rig_noisy_cases(), measured as REF_RESOLUTION was and rounded up to one digit.
# Measured maxima over the cases: dK 1.3e-10, dD 2.4e-9 (upside_down/flags0), dom 8.6e-11 (upside_down/flags0), dT 2.0e-8
# (toe_in/flags0), dr 1.2e-8 (toe_in/fix_intrinsic), dt 1.6e-7, gamma 7.9e-10 (upside_down16/fix_intrinsic).
RIG_REF_RESOLUTION = dict(dK=2e-10, dD=3e-9, dom=9e-11, dT=2e-8, dr=2e-8, dt=2e-7, gamma=8e-10)


def rig_step_cases():
    """step_cases()' form on the rigs of RIGS: the smallest inputs on which the two maps of k_ps_lin are far from
    what they are on the rig of the module's head."""
    E = USE_EXTRINSIC_GUESS
    rig = lambda c, s: np.concatenate([c.g[0:3] * s, c.g[3:6] * s])
    toe = make_rig("toe_in", [20] * 5, seed=520, noise=0.2)                     # groups of 3 + 2 views
    # the draw (of 39 tried) on which the 5 x 20 minimum keeps |om| and the near-zero view's |r_v| under 1e-2 all the
    # way: 20 noisy corners hold a view's tilt and five views the rig's rotation to about 2e-2 only
    ser = make_rig("series", [20] * 5, seed=527, noise=0.2, view_r={NEAR_ZERO_VIEW: near_zero(528)})
    r90 = make_rig("roll90", [20] * 9, seed=523, noise=0.2)                     # groups of 3 views
    fwd = make_rig("forward", [20] * 5, seed=524, noise=0.2)
    return [("5x20/toe_in", toe, USE_GUESS | E, 5, toe.g[6:18] * 1.05, toe.g[18:30] * 1.05, rig(toe, 1.1)),
            # Jl(om) and Jl(r_v) of view NEAR_ZERO_VIEW both from so3_jac's series in one trial
            ("5x20/series_poses", ser, USE_GUESS | E, 5, ser.g[6:18] * 1.01, ser.g[18:30] * 1.01, rig(ser, 1.05)),
            # SAME_FOCAL_LENGTH without FIX_ASPECT_RATIO: camera 2's fx follows camera 1's fx, not its own fy
            ("9x20/roll90_same", r90, USE_GUESS | E | SAME_FOCAL, 5, r90.g[6:18] * 1.05, r90.g[18:30] * 1.05, rig(r90, 1.1)),
            # 0.5 rad and 2 x T off, as 5x20/fix_intrinsic_nd4 is: from 0.3 rad and 1.5 x T the walk is at its minimum
            # after four steps and the sixth decision is inside the margin (|en / err - 1| = 2e-11)
            ("5x20/forward_fix", fwd, FIX_INTRINSIC | E, 5, fwd.g[6:18], fwd.g[18:30],
             np.concatenate([fwd.g[0:3] + np.array([0.2, -0.15, 0.17]) * (0.5 / 0.3), fwd.g[3:6] * 2.0]))]


_REF = {}


def reference(name):
    """tests/npstereocalib.py's minimum of a noisy case, computed once and shared: a dict with g [30], poses, rms,
    steps, last (the last Gauss-Newton step: dg, dposes), gamma at the minimum, mask and ties."""
    if name not in _REF:
        table = rig_noisy_cases() if "/" in name else noisy_cases()
        _, c, flags, nd, guess1, guess2, _rig = {x[0]: x for x in table}[name]
        mask, _ = mask_rules(flags, nd)
        K1, K2 = (guess_KD(gs, nd)[0] for gs in (guess1, guess2))
        ties = ties_of(flags, K1, K2)
        g0 = NS.tied(reference_start(c, flags, mask, guess1, guess2), ties)
        g, poses, r, steps, last = NS.gauss_newton(c, g0, c.poses, mask, ties, return_last=True)
        _REF[name] = dict(g=g, poses=poses, rms=r, steps=steps, last=last, gamma=NS.gamma(c, g, poses, mask, ties),
                          mask=mask, ties=ties)
    return _REF[name]


def resolution(ref):
    """The reference's last step in REF_RESOLUTION's units."""
    dg, dp = ref["last"]
    g = ref["g"]
    rel = lambda s: float(np.max(np.abs(dg[s]) / np.abs(g[s])))
    return dict(dK=max(rel(slice(6, 10)), rel(slice(18, 22))), dD=float(max(np.abs(dg[10:18]).max(), np.abs(dg[22:30]).max())),
                dom=float(np.abs(dg[0:3]).max()), dT=float(np.abs(dg[3:6]).max()), dr=float(np.abs(dp[:, :3]).max()),
                dt=float(np.abs(dp[:, 3:]).max()), gamma=ref["gamma"])


def globals_of(K1, D1, K2, D2, R, T):
    """The 30 slots of a result of api.stereo_calibrate."""
    g = np.zeros(30)
    g[0:3], g[3:6] = rotvec(np.asarray(R)), T
    for base, K, D in ((6, K1, D1), (18, K2, D2)):
        g[base:base + 4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        g[base + 4:base + 4 + len(D)] = D
    return g


K_STEPS = 6
MIN_CHECKED = 4    # at least the first four accepted steps of every step case are compared (calib_cases.step_checked)


def guess_KD(guess, nd):
    if guess is None:
        return None, None
    return CC.guess_KD(guess, nd)


def rig_RT(rig):
    if rig is None:
        return None, None
    return npcalib.rodrigues(rig[:3]), np.asarray(rig[3:], np.float64).copy()
