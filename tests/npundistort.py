"""numpy restatement of cv::omnidir::undistortPoints (src/omnidir.cpp:249-343),
initUndistortRectifyMap (:348-533), undistortImage (:538-546) and stereoRectify (:2190-2227), and of
the cv::remap call undistortImage makes -- the test-side reference of the rectification entry points
of include/mcc_omnidir.h.

Built on oracle primitives where they exist: O.rodrigues_v2m for a rotation vector, and
O.omni_project_full (at the identity pose) for the tail every map pixel shares -- normalise, divide
by Zs + xi, distort, apply K (:423-437, :501-515).

The map model walks a row as the reference does, with running sums (_x += iKR(0,0), theta +=
iK(0,0)): np.cumsum adds left to right in double, exactly that loop.  The device evaluates the closed
form base_i + j * step instead; the tests bound the difference.

The remap is OpenCV's documented INTER_LINEAR on CV_16SC2 + CV_16UC1 maps with BORDER_CONSTANT 0, in
integer arithmetic.  Neither OpenCV nor cv2 is available to the suite, so its agreement with a real
cv::remap is not pinned by any test.
"""
import numpy as np

from oracle import oracle_py as O

RECTIFY_PERSPECTIVE, RECTIFY_CYLINDRICAL, RECTIFY_LONGLATI, RECTIFY_STEREOGRAPHIC = 1, 2, 3, 4
MAP_FLOAT, MAP_FIXED = 1, 2


def rotation(R):
    """None -> identity, a 3-vector -> cv::Rodrigues, a 3 x 3 matrix as it is."""
    if R is None:
        return np.eye(3)
    R = np.asarray(R, np.float64)
    return O.rodrigues_v2m(R.reshape(3))[0] if R.size == 3 else R.reshape(3, 3)


def undistort_points(distorted, K, D, xi, R=None, dtype=np.float64):
    """undistortPoints in `dtype` arithmetic, operation for operation (:303-342)."""
    t = dtype
    pi = np.asarray(distorted, np.float64).reshape(-1, 2).astype(t)
    K = np.asarray(K, np.float64).astype(t)
    f0, f1, c0, c1, s = K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 1]
    k1, k2, p1, p2 = np.asarray(D, np.float64).reshape(4).astype(t)
    xi = t(xi)
    RR = rotation(R).astype(t)
    pp0 = (pi[:, 0] * f1 - c0 * f1 - s * (pi[:, 1] - c1)) / (f0 * f1)
    pp1 = (pi[:, 1] - c1) / f1
    pu0, pu1 = pp0.copy(), pp1.copy()
    for _ in range(20):
        r2 = pu0 * pu0 + pu1 * pu1
        r4 = r2 * r2
        pu0 = (pp0 - 2 * p1 * pu0 * pu1 - p2 * (r2 + 2 * pu0 * pu0)) / (1 + k1 * r2 + k2 * r4)
        pu1 = (pp1 - 2 * p2 * pu0 * pu1 - p1 * (r2 + 2 * pu1 * pu1)) / (1 + k1 * r2 + k2 * r4)   # the new pu0
    r2 = pu0 * pu0 + pu1 * pu1
    a, b, cc = r2 + 1, 2 * xi * r2, r2 * xi * xi - 1
    Zs = (-b + np.sqrt(b * b - 4 * a * cc)) / (2 * a)
    X = [pu0 * (Zs + xi), pu1 * (Zs + xi), Zs]
    W = [RR[r, 0] * X[0] + RR[r, 1] * X[1] + RR[r, 2] * X[2] for r in range(3)]
    nrm = np.sqrt(W[0] * W[0] + W[1] * W[1] + W[2] * W[2])
    S = [w / nrm for w in W]
    return np.stack([S[0] / S[2], S[1] / S[2]], -1)


def _walk(base, step, w):
    """base[i], then + step per column, summed left to right as `for (j...; _x += step)` does."""
    inc = np.full((base.shape[0], w), step, np.float64)
    inc[:, 0] = base
    return np.cumsum(inc, axis=1)


def map_uv(K, D, xi, R, P, size, flags):
    """(u, v) [h, w] float64 of initUndistortRectifyMap before the conversion to a map type."""
    w, h = size
    K = np.asarray(K, np.float64).reshape(3, 3)
    D = np.zeros(4) if D is None else np.asarray(D, np.float64).reshape(4)
    RR = rotation(R)
    PP = K if P is None else np.asarray(P, np.float64)[:, :3]
    iKR, iK, iR = np.linalg.inv(PP @ RR), np.linalg.inv(PP), np.linalg.inv(RR)
    i = np.arange(h, dtype=np.float64)
    if flags == RECTIFY_PERSPECTIVE:
        x, y, ww = (_walk(i * iKR[r, 1] + iKR[r, 2], iKR[r, 0], w) for r in range(3))
    else:
        theta = _walk(i * iK[0, 1] + iK[0, 2], iK[0, 0], w)
        hh = _walk(i * iK[1, 1] + iK[1, 2], iK[1, 0], w)
        if flags == RECTIFY_CYLINDRICAL:
            xt, yt, wt = np.cos(theta), np.sin(theta), hh
        elif flags == RECTIFY_LONGLATI:
            xt, yt, wt = -np.cos(theta), -np.sin(theta) * np.cos(hh), np.sin(theta) * np.sin(hh)
        elif flags == RECTIFY_STEREOGRAPHIC:
            a = theta * theta + hh * hh + 4
            b = -2 * theta * theta - 2 * hh * hh
            c2 = theta * theta + hh * hh - 4
            yt = (-b - np.sqrt(b * b - 4 * a * c2)) / (2 * a)
            xt = theta * (1 - yt) / 2
            wt = hh * (1 - yt) / 2
        else:
            raise ValueError("unknown rectification flag")
        x, y, ww = (iR[r, 0] * xt + iR[r, 1] * yt + iR[r, 2] * wt for r in range(3))
    kin = [K[0, 0], K[1, 1], K[0, 1], K[0, 2], K[1, 2]]
    uv, _ = O.omni_project_full(np.stack([x, y, ww], -1).reshape(-1, 3), np.zeros(3), np.zeros(3), kin, float(xi), D,
                                jac=False)
    return uv[:, 0].reshape(h, w), uv[:, 1].reshape(h, w)


def fixed_units(u, v):
    """iu = cvRound(32 u), iv = cvRound(32 v) (round half even), int64; 32 u outside the int range or
    NaN is unspecified in the reference and must not occur in a test."""
    su, sv = u * 32, v * 32
    assert np.isfinite(su).all() and np.isfinite(sv).all()
    assert np.abs(su).max(initial=0) < 2 ** 31 - 1 and np.abs(sv).max(initial=0) < 2 ** 31 - 1
    return np.rint(su).astype(np.int64), np.rint(sv).astype(np.int64)


def fixed_maps(iu, iv):
    """CV_16SC2 + CV_16UC1 from the 1/32 px units: the short cast wraps (:443-445)."""
    m1 = np.stack([(iu >> 5).astype(np.int16), (iv >> 5).astype(np.int16)], -1)   # astype wraps
    m2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return m1, m2


def init_undistort_rectify_map(K, D, xi, R, P, size, map_type, flags):
    u, v = map_uv(K, D, xi, R, P, size, flags)
    if map_type == MAP_FLOAT:
        return u.astype(np.float32), v.astype(np.float32)
    return fixed_maps(*fixed_units(u, v))


def remap(src, map1, map2):
    """cv::remap(src, map1, map2, INTER_LINEAR, BORDER_CONSTANT 0) on fixed-point maps; src uint8
    [h, w] or [h, w, c]."""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    img = src[:, :, None] if src.ndim == 2 else src
    sh, sw = img.shape[:2]
    sx, sy = map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64)
    m2 = map2.astype(np.int64) & 1023
    fx, fy = m2 & 31, m2 >> 5

    def tap(x, y):
        ok = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        t = img[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)].astype(np.int64)
        return np.where(ok[..., None], t, 0)

    acc = ((32 - fx) * (32 - fy) * 32)[..., None] * tap(sx, sy) + (fx * (32 - fy) * 32)[..., None] * tap(sx + 1, sy) \
        + ((32 - fx) * fy * 32)[..., None] * tap(sx, sy + 1) + (fx * fy * 32)[..., None] * tap(sx + 1, sy + 1)
    out = ((acc + 16384) >> 15).astype(np.uint8)
    return out[:, :, 0] if src.ndim == 2 else out


def undistort_image(src, K, D, xi, flags, Knew=None, new_size=None, R=None):
    size = (src.shape[1], src.shape[0]) if new_size is None else new_size
    return remap(src, *init_undistort_rectify_map(K, D, xi, R, Knew, size, MAP_FIXED, flags))


def stereo_rectify(R, T):
    """stereoRectify (:2213-2225); raises where the reference divides 0 by 0."""
    R = rotation(R)
    T21 = -R.T @ np.asarray(T, np.float64).reshape(3)
    n1 = np.linalg.norm(T21)
    n2 = np.hypot(T21[0], T21[1])
    if not n1 > 0 or not n2 > 0:
        raise ValueError("T = 0 or the baseline along z")
    e1 = T21 / n1
    e2 = np.array([-T21[1], T21[0], 0.0]) / n2
    e3 = np.cross(e1, e2)
    e3 = e3 / np.linalg.norm(e3)
    R1 = np.stack([e1, e2, e3])
    return R1, R1 @ R.T
