"""numpy model of the pinhole rectification (include/mcc.h: mcc_undistort_points, mcc_init_undistort_rectify_map,
mcc_stereo_rectify), written from the rules of DESIGN.md 7i and from nothing else: it shares no code with the
library.  The remap is the camera-independent one of tests/npundistort.py.

Every function takes a `dtype`, np.float64 or np.longdouble: the tests bound the library by what float64 costs
this arithmetic, |float64 model - long double model|.

  undistort_points(px, K, D, R, P, iterations, dtype)   pixel -> ideal point, then R, then P
  map_uv(K, D, R, P, size, dtype)                       (u, v) [h, w] of initUndistortRectifyMap: the closed form
                                                        base_i + j * step, the division, distort, K
  init_undistort_rectify_map(K, D, R, P, size, map_type)
  stereo_rectify(K1, D1, K2, D2, size, R, T, flags, alpha, new_size, dtype)
                                                        -> dict R1 R2 P1 P2 Q roi1 roi2 idx inner outer s
"""
import numpy as np

import npundistort as U

ZERO_DISPARITY = 1024
MAP_FLOAT, MAP_FIXED = U.MAP_FLOAT, U.MAP_FIXED


def _coeffs(D, t):
    """k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 from a D of 0, 4, 5, 8 or 12 entries (None: 0)"""
    d = np.zeros(12, t)
    if D is not None:
        D = np.asarray(D, np.float64).reshape(-1)
        assert D.size in (0, 4, 5, 8, 12)
        d[:D.size] = D.astype(t)
    return d


def _mat(M, t, none):
    if M is None:
        return none.astype(t)
    return np.asarray(M)[:, :3].astype(t)   # (a long double R1 / P1 of this module keeps its bits)


def rodrigues(w, dtype=np.float64):
    t = dtype
    w = np.asarray(w, t)
    th = np.sqrt(w @ w)
    if th == 0:
        return np.eye(3, dtype=t)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], t)
    return np.eye(3, dtype=t) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def log_so3(R, dtype=np.float64):
    """The rotation vector of R, exact to rounding at every angle: the angle from atan2(s, c); the axis from the skew
    part up to a quarter turn and beyond it from the symmetric part (R + R^T) / 2 - c I = (1 - c) a a^T, its column with
    the largest diagonal entry, signed by the skew part."""
    t = dtype
    R = np.asarray(R, t)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], t)
    s, c = np.sqrt(v @ v) / 2, (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    th = np.arctan2(s, c)
    if c > 0:
        return v * (th / (2 * s) if s > 0 else t(0.5))
    S = (R + R.T) / 2 - c * np.eye(3, dtype=t)
    a = S[:, int(np.argmax(np.diag(S)))]
    a = a / np.sqrt(a @ a)
    return (-a if a @ v < 0 else a) * th


def undistort_points(px, K, D=None, R=None, P=None, iterations=20, dtype=np.float64):
    t = dtype
    px = np.asarray(px, np.float64).reshape(-1, 2).astype(t)
    K = np.asarray(K, np.float64).astype(t)
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coeffs(D, t)
    RR, PP = _mat(R, t, np.eye(3)), _mat(P, t, np.eye(3))
    x0, y0 = (px[:, 0] - K[0, 2]) / K[0, 0], (px[:, 1] - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        icd = (1 + k4 * r2 + k5 * r4 + k6 * r6) / (1 + k1 * r2 + k2 * r4 + k3 * r6)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r4
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r4
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    X, Y, W = (RR[r, 0] * x + RR[r, 1] * y + RR[r, 2] for r in range(3))
    x, y = X / W, Y / W
    d = PP[2, 0] * x + PP[2, 1] * y + PP[2, 2]
    return np.stack([(PP[0, 0] * x + PP[0, 1] * y + PP[0, 2]) / d, (PP[1, 0] * x + PP[1, 1] * y + PP[1, 2]) / d], -1)


def distort(x, y, D, dtype=np.float64):
    """cv::projectPoints' distortion of ideal points (tests/npcalib.py::project's, with the prism terms)"""
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coeffs(D, dtype)
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    cd = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r4
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r4
    return xd, yd


def inv3(M):
    """3 x 3 inverse by cofactors, in M's dtype (np.linalg.inv has no long double)"""
    a, b, c, d, e, f, g, h, i = M.ravel()
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    return np.array([[e * i - f * h, c * h - b * i, b * f - c * e],
                     [f * g - d * i, a * i - c * g, c * d - a * f],
                     [d * h - e * g, b * g - a * h, a * e - b * d]], M.dtype) / det


def map_uv(K, D, R, P, size, dtype=np.float64):
    t = dtype
    w, h = size
    K = np.asarray(K, np.float64).astype(t)
    RR, PP = _mat(R, t, np.eye(3)), _mat(P, t, np.asarray(K, np.float64))
    iPR = inv3(PP @ RR)
    i, j = np.arange(h, dtype=t)[:, None], np.arange(w, dtype=t)[None, :]
    X, Y, W = ((i * iPR[r, 1] + iPR[r, 2]) + j * iPR[r, 0] for r in range(3))
    xd, yd = distort(X / W, Y / W, D, t)
    return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]


def init_undistort_rectify_map(K, D, R, P, size, map_type):
    u, v = map_uv(K, D, R, P, size)
    if map_type == MAP_FLOAT:
        return u.astype(np.float32), v.astype(np.float32)
    return U.fixed_maps(*U.fixed_units(u, v))


def _rectangles(K, D, R, Kn, size, t):
    """inner (left, top, right, bottom) and outer of the 9 x 9 grid of source pixels through (K, D, R, Kn)"""
    w, h = size
    a, b = np.meshgrid(np.arange(9), np.arange(9))            # a along x, b along y; [b, a]
    px = np.stack([a.ravel() * (w - 1) / 8, b.ravel() * (h - 1) / 8], -1)
    p = undistort_points(px, K, D, R, Kn, 20, t).reshape(9, 9, 2)
    inner = (p[:, 0, 0].max(), p[0, :, 1].max(), p[:, 8, 0].min(), p[8, :, 1].min())
    outer = (p[..., 0].min(), p[..., 1].min(), p[..., 0].max(), p[..., 1].max())
    return inner, outer


def stereo_rectify(K1, D1, K2, D2, size, R, T, flags=0, alpha=-1.0, new_size=None, dtype=np.float64):
    t = dtype
    w, h = size
    W, H = size if new_size is None else new_size
    Ks = [np.asarray(K, np.float64).astype(t) for K in (K1, K2)]
    Ds = [_coeffs(D, t) for D in (D1, D2)]
    R, T = np.asarray(R, np.float64).astype(t), np.asarray(T, np.float64).astype(t)
    alpha = t(alpha)
    # 1
    om = log_so3(R, t)
    r = rodrigues(-om / 2, t)
    tt = r @ T
    idx = 0 if abs(tt[0]) > abs(tt[1]) else 1
    c = tt[idx]
    uu = np.zeros(3, t)
    uu[idx] = 1 if c > 0 else -1
    ww = np.cross(tt, uu).astype(t)
    nw = np.sqrt(ww @ ww)
    if nw > 0:
        ww = ww * (np.arccos(abs(c) / np.sqrt(tt @ tt)) / nw)
    wR = rodrigues(ww, t)
    Rk = [wR @ r.T, wR @ r]
    tt = Rk[1] @ T
    # 2
    fc = None
    for K, D in zip(Ks, Ds):
        f = K[1, 1] if idx == 0 else K[0, 0]
        if D[0] < 0:
            f = f * (1 + D[0] * (w * w + h * h) / (4 * f * f))
        fc = f if fc is None else min(fc, f)
    # 3
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float64)
    Pf = np.diag(np.array([fc, fc, 1], t))
    cc = []
    for k in range(2):
        p = undistort_points(corners, Ks[k], Ds[k], Rk[k], Pf, 20, t)
        cc.append(np.array([t(w - 1) / 2 - (p[0, 0] + p[1, 0] + p[2, 0] + p[3, 0]) / 4,
                            t(h - 1) / 2 - (p[0, 1] + p[1, 1] + p[2, 1] + p[3, 1]) / 4], t))
    for a in range(2):
        if (flags & ZERO_DISPARITY) or a == 1 - idx:
            cc[0][a] = cc[1][a] = (cc[0][a] + cc[1][a]) / 2
    # 4
    sc = np.array([t(W - 1) / t(w - 1), t(H - 1) / t(h - 1)], t)
    cn = [c_ * sc for c_ in cc]
    # 5
    s, inner, outer = t(1), [None, None], [None, None]
    if alpha >= 0:
        s0, s1 = [], []
        for k in range(2):
            Kn = np.array([[fc, 0, cc[k][0]], [0, fc, cc[k][1]], [0, 0, 1]], t)
            inner[k], outer[k] = _rectangles(Ks[k], Ds[k], Rk[k], Kn, size, t)
            for rect, out in ((inner[k], s0), (outer[k], s1)):
                out += [cn[k][0] / (cc[k][0] - rect[0]), cn[k][1] / (cc[k][1] - rect[1]),
                        (W - 1 - cn[k][0]) / (rect[2] - cc[k][0]), (H - 1 - cn[k][1]) / (rect[3] - cc[k][1])]
        s = max(s0) * (1 - alpha) + min(s1) * alpha
    f = fc * s
    # 6
    Ps = [np.array([[f, 0, cn[k][0], 0], [0, f, cn[k][1], 0], [0, 0, 1, 0]], t) for k in range(2)]
    Ps[1][idx, 3] = tt[idx] * f
    Q = np.array([[1, 0, 0, -cn[0][0]], [0, 1, 0, -cn[0][1]], [0, 0, 0, f],
                  [0, 0, -1 / tt[idx], (cn[0][idx] - cn[1][idx]) / tt[idx]]], t)
    rois = []
    for k in range(2):
        if alpha < 0:
            rois.append((0, 0, W, H))
            continue
        l, tp, rr, b = inner[k]
        x0, y0 = int(np.ceil((l - cc[k][0]) * s + cn[k][0])), int(np.ceil((tp - cc[k][1]) * s + cn[k][1]))
        x1, y1 = int(np.floor((rr - cc[k][0]) * s + cn[k][0])), int(np.floor((b - cc[k][1]) * s + cn[k][1]))
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
        rois.append((x0, y0, x1 - x0, y1 - y0) if x1 > x0 and y1 > y0 else (0, 0, 0, 0))
    return dict(R1=Rk[0], R2=Rk[1], P1=Ps[0], P2=Ps[1], Q=Q, roi1=rois[0], roi2=rois[1], idx=idx, inner=inner,
                outer=outer, s=s)
