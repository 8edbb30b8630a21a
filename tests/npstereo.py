"""numpy restatement of cv::omnidir::stereoCalibrate (src/omnidir.cpp:1213-1381), the test-side
reference of include/mcc_omnidir.h's mcc_omnistereo_* / mcc_omnidir_stereo_* entry points.

Built only from oracle primitives: O.omni_project_full (the 2 x 16 projection rows),
O.compose_motion (internal::compose_motion's eight partials, in its order), O.rodrigues_v2m /
O.rodrigues_m2v, and O.omni_calibrate for the two initial single-camera calibrations.

Two forms of one loop step, as tests/test_omnidir_calib.py has for one camera:
  dense_G   as computeJacobianStereo assembles it (:937-1020): the dense 4Nn x P Jacobian,
            subMatrix, JTJ + epsilon on EVERY entry, a dense solve;
  block_G   the device's algebra: per view the 6 x 6 pose block U and its coupling W (6 x 26) to the
            global block [om, T | intr_1 | intr_2], the Schur complement summed over the views, a
            26 x 26 solve for the right-hand sides JTE and ones, and Sherman-Morrison for epsilon 1 1^T.
"""
import numpy as np

from oracle import oracle_py as O

FIX_SKEW, FIX_K1, FIX_K2, FIX_P1, FIX_P2, FIX_XI, FIX_GAMMA, FIX_CENTER = 2, 4, 8, 16, 32, 64, 128, 256
FIX_DIST = FIX_K1 | FIX_K2 | FIX_P1 | FIX_P2


class StereoViews:
    """The views both cameras see: off[n+1] corner ranges (all of one length), obj (corners x 3),
    img1 / img2 (corners x 2)."""

    def __init__(self, off, obj, img1, img2):
        self.off = np.ascontiguousarray(off, np.int32)
        self.obj = np.ascontiguousarray(obj, np.float64).reshape(-1, 3)
        self.img1 = np.ascontiguousarray(img1, np.float64).reshape(-1, 2)
        self.img2 = np.ascontiguousarray(img2, np.float64).reshape(-1, 2)
        self.n = len(self.off) - 1

    @property
    def n_params(self):
        return 6 * (self.n + 1) + 20

    def subset(self, idx):
        sel = np.concatenate([np.arange(self.off[i], self.off[i + 1]) for i in idx])
        off = np.concatenate([[0], np.cumsum([self.off[i + 1] - self.off[i] for i in idx])])
        return StereoViews(off, self.obj[sel], self.img1[sel], self.img2[sel])

    def cam(self, c):
        return O.OmniViews(self.off, self.obj, self.img1 if c == 0 else self.img2)


def flags2idx_stereo(flags, n):
    """flags2idxStereo (:2078-2135): the >= cascade on both cameras' intrinsics; 1 = free."""
    idx = np.ones(6 * (n + 1) + 20, np.int32)
    o1 = 6 * (n + 1)
    f = flags
    for bit, cols in ((FIX_CENTER, (3, 4)), (FIX_GAMMA, (0, 1)), (FIX_XI, (5,)), (FIX_P2, (9,)), (FIX_P1, (8,)),
                      (FIX_K2, (7,)), (FIX_K1, (6,))):
        if f >= bit:
            for c in cols:
                idx[o1 + c] = idx[o1 + 10 + c] = 0
            f -= bit
    if f >= FIX_SKEW:
        idx[o1 + 2] = idx[o1 + 12] = 0
    return idx


def _intr(p, n, c):
    q = p[6 * (n + 1) + 10 * c:6 * (n + 1) + 10 * c + 10]
    return q[0:5], q[5], q[6:10]


def view_strip(v: StereoViews, p, i):
    """View i's rows of J and E (:968-1009): (J [4N, 32] over the columns [own pose 6 | om, T 6 |
    intr_1 10 | intr_2 10], E [4N]); the 2N left rows first."""
    n = v.n
    sl = slice(v.off[i], v.off[i + 1])
    N = v.off[i + 1] - v.off[i]
    om, T = p[0:3], p[3:6]
    om1, T1 = p[6 + 6 * i:9 + 6 * i], p[9 + 6 * i:12 + 6 * i]
    J = np.zeros((4 * N, 32))
    kin, xi, D = _intr(p, n, 0)
    proj1, j1 = O.omni_project_full(v.obj[sl], om1, T1, kin, xi, D)
    J[:2 * N, 0:6] = j1[:, 0:6]
    J[:2 * N, 12:22] = j1[:, 6:16]
    om2, T2, d = O.compose_motion(om1, T1, om, T)
    dom2dom1, dom2dT1, dom2dom, dom2dT, dT2dom1, dT2dT1, dT2dom, dT2dT = d
    kin, xi, D = _intr(p, n, 1)
    proj2, j2 = O.omni_project_full(v.obj[sl], om2, T2, kin, xi, D)
    J[2 * N:, 6:9] = j2[:, 0:3] @ dom2dom + j2[:, 3:6] @ dT2dom      # dxrdom  (:999)
    J[2 * N:, 9:12] = j2[:, 0:3] @ dom2dT + j2[:, 3:6] @ dT2dT       # dxrdT   (:1000)
    J[2 * N:, 0:3] = j2[:, 0:3] @ dom2dom1 + j2[:, 3:6] @ dT2dom1    # dxrdom1 (:1001)
    J[2 * N:, 3:6] = j2[:, 0:3] @ dom2dT1 + j2[:, 3:6] @ dT2dT1      # dxrdT1  (:1002)
    J[2 * N:, 22:32] = j2[:, 6:16]
    E = np.concatenate([(v.img1[sl] - proj1).reshape(-1), (v.img2[sl] - proj2).reshape(-1)])
    return J, E


def strip_cols(n, i):
    """The parameter indices of view i's 32 strip columns."""
    return np.r_[6 + 6 * i:12 + 6 * i, 0:6, 6 * (n + 1):6 * (n + 1) + 20]


def dense_J(v: StereoViews, p):
    rows = 4 * int(v.off[1] - v.off[0])
    J = np.zeros((rows * v.n, v.n_params))
    E = np.zeros(rows * v.n)
    for i in range(v.n):
        Ji, Ei = view_strip(v, p, i)
        J[rows * i:rows * (i + 1), strip_cols(v.n, i)] = Ji
        E[rows * i:rows * (i + 1)] = Ei
    return J, E


def schedule(it):
    """(alpha_smooth2, epsilon) of loop iteration it (:1280-1282)."""
    return 1 - (1 - 0.01) ** (it + 1), 0.01 * 0.9 ** (it / 10)


def dense_G(v: StereoViews, p, flags, it):
    """(G, JTE before the flag reduction) as the reference assembles them."""
    J, E = dense_J(v, p)
    JTJ, JTE = J.T @ J, J.T @ E
    idx = flags2idx_stereo(flags, v.n).astype(bool)
    a2, eps = schedule(it)
    G = np.zeros(v.n_params)
    G[idx] = a2 * np.linalg.solve(JTJ[np.ix_(idx, idx)] + eps, JTE[idx])
    return G, JTE


def block_G(v: StereoViews, p, flags, it):
    """(G, JTE) by per-view Schur elimination, a 26 x 26 solve and Sherman-Morrison."""
    n = v.n
    mask = flags2idx_stereo(flags, n)[np.r_[0:6, 6 * (n + 1):6 * (n + 1) + 20]].astype(float)
    S, rb, wu = np.zeros((26, 26)), np.zeros(26), np.zeros(26)
    ab = au = 0.0
    keep = []
    JTE = np.zeros(v.n_params)
    for i in range(n):
        J, E = view_strip(v, p, i)
        JTE[strip_cols(n, i)] += J.T @ E
        J = J.copy()
        J[:, 6:] *= mask
        U, W, V = J[:, :6].T @ J[:, :6], J[:, :6].T @ J[:, 6:], J[:, 6:].T @ J[:, 6:]
        rp, rc = J[:, :6].T @ E, J[:, 6:].T @ E
        Ui = np.linalg.inv(U)
        Y, zb, zu = Ui @ W, Ui @ rp, Ui @ np.ones(6)
        S += V - W.T @ Y
        rb += rc - W.T @ zb
        wu += W.T @ zu
        ab += zb.sum()
        au += zu.sum()
        keep.append((Y, zb, zu))
    fixed = mask == 0
    S[fixed, :] = 0
    S[:, fixed] = 0
    S[fixed, fixed] = 1
    ycb = np.linalg.solve(S, rb * mask)
    ycu = np.linalg.solve(S, (mask - wu) * mask)
    s1 = ab + (mask - wu) @ ycb
    s2 = au + (mask - wu) @ ycu
    a2, eps = schedule(it)
    coef = eps * s1 / (1 + eps * s2)
    yc = ycb - coef * ycu
    G = np.zeros(v.n_params)
    for i, (Y, zb, zu) in enumerate(keep):
        G[6 + 6 * i:12 + 6 * i] = a2 * ((zb - coef * zu) - Y @ yc)
    G[0:6] = a2 * yc[0:6]
    G[6 * (n + 1):] = a2 * yc[6:]
    return G, JTE


def disagreement(Ga, Gb):
    """d of the issue: the largest disagreement of two step vectors, relative to max |G|."""
    return float(np.abs(Ga - Gb).max() / np.abs(Ga).max())


def optimize(v: StereoViews, p, flags=0, crit_type=3, max_count=200, eps=1e-4, step=dense_G):
    """stereoCalibrate's loop (:1272-1301): (params, iterations, last change)."""
    p = np.array(p, np.float64, copy=True)
    change, it = 1.0, 0
    while True:
        if (crit_type == 1 and it >= max_count) or (crit_type == 2 and change <= eps) or \
                (crit_type == 3 and (change <= eps or it >= max_count)):
            break
        G = step(v, p, flags, it)[0]
        change = np.linalg.norm(G) / np.linalg.norm(p)
        p = p + G
        it += 1
    return p, it, change


def rms(v: StereoViews, p):
    """estimateUncertaintiesStereo's rms (:1826-1888): over both cameras' points."""
    n = v.n
    s = 0.0
    for i in range(n):
        sl = slice(v.off[i], v.off[i + 1])
        om1, T1 = p[6 + 6 * i:9 + 6 * i], p[9 + 6 * i:12 + 6 * i]
        kin, xi, D = _intr(p, n, 0)
        s += ((v.img1[sl] - O.omni_project_full(v.obj[sl], om1, T1, kin, xi, D, jac=False)[0]) ** 2).sum()
        R, R1 = O.rodrigues_v2m(p[0:3])[0], O.rodrigues_v2m(om1)[0]
        om2 = O.rodrigues_m2v(R @ R1)[0]
        T2 = R @ T1 + p[3:6]
        kin, xi, D = _intr(p, n, 1)
        s += ((v.img2[sl] - O.omni_project_full(v.obj[sl], om2, T2, kin, xi, D, jac=False)[0]) ** 2).sum()
    return float(np.sqrt(s / (2 * v.off[-1])))


def find_median(x):
    """findMedian (:2172-2181), with its even and odd cases as the reference has them."""
    t = np.sort(np.asarray(x, np.float64))
    k = len(t)
    if k % 2 == 0:
        return t[k // 2]
    return 0.5 * (t[k // 2] + t[k // 2 - 1])


def encode_init(idx1, om1, t1, idx2, om2, t2, K1, xi1, D1, K2, xi2, D2):
    """initializeStereoCalibration after its two calibrate calls (:764-846) + encodeParametersStereo:
    (params, kept view indices)."""
    pairs = [(i, j) for i in range(len(idx1)) for j in range(len(idx2)) if idx1[i] == idx2[j]]   # getInterset
    omE, tE = [], []
    for i, j in pairs:
        R1, R2 = O.rodrigues_v2m(om1[i])[0], O.rodrigues_v2m(om2[j])[0]
        RLR = R2 @ R1.T
        omE.append(O.rodrigues_m2v(RLR)[0])
        tE.append(t2[j] - RLR @ t1[i])
    omE, tE = np.array(omE), np.array(tE)
    om = [find_median(omE[:, k]) for k in range(3)]
    T = [find_median(tE[:, k]) for k in range(3)]
    poses = np.concatenate([np.r_[om1[i], t1[i]] for i, _ in pairs])

    def intr(K, xi, D):
        K = np.asarray(K, np.float64).reshape(3, 3)
        return np.r_[K[0, 0], K[1, 1], K[0, 1], K[0, 2], K[1, 2], xi, np.asarray(D, np.float64)]
    return (np.concatenate([om, T, poses, intr(K1, xi1, D1), intr(K2, xi2, D2)]),
            np.array([idx1[i] for i, _ in pairs], np.int32))


def mono_calibrations(v: StereoViews, size1, size2, flags=0):
    """The two omnidir::calibrate runs of initializeStereoCalibration, TermCriteria(3, 100, 1e-6) (:761-762)."""
    out = []
    for c, size in ((0, size1), (1, size2)):
        _, K, xi, D, om, t, idx, _ = O.omni_calibrate(v.cam(c), int(size[0]), int(size[1]), flags, 3, 100, 1e-6)
        out.append((idx, om, t, K, xi, D))
    return out


def stereo_init(v: StereoViews, size1, size2, flags=0):
    (i1, o1, t1, K1, x1, D1), (i2, o2, t2, K2, x2, D2) = mono_calibrations(v, size1, size2, flags)
    return encode_init(i1, o1, t1, i2, o2, t2, K1, x1, D1, K2, x2, D2)


def stereo_calibrate(v: StereoViews, size1, size2, flags=0, crit_type=3, max_count=200, eps=1e-4):
    """(rms, final params, kept idx, iterations, start params)"""
    p0, idx = stereo_init(v, size1, size2, flags)
    vk = v.subset(idx)
    p, it, _ = optimize(vk, p0, flags, crit_type, max_count, eps)
    return rms(vk, p), p, idx, it, p0


def start_params(s, seed=0, pose_sigma=1e-3):
    """A start for a synthetic rig (rig.OmniStereoViews): the truth with focal lengths 1 % up, xi
    2 % down, half the distortion, and Gaussian noise of pose_sigma on (om, T) and the poses."""
    rng = np.random.default_rng(seed)
    sc = np.array([[1.01, 1, 1], [1, 1.01, 1], [1, 1, 1]])

    def intr(K, xi, D):
        K = K * sc
        return np.r_[K[0, 0], K[1, 1], K[0, 1], K[0, 2], K[1, 2], xi * 0.98, D * 0.5]
    p = np.concatenate([s.om, s.T, np.c_[s.omL, s.tL].reshape(-1), intr(s.K1, s.xi1, s.D1), intr(s.K2, s.xi2, s.D2)])
    p[:6 * (s.n_views + 1)] += rng.normal(scale=pose_sigma, size=6 * (s.n_views + 1))
    return p
