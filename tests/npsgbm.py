"""numpy model of the semi-global matcher behind mcc_omnidir_sgbm and of the tail of
cv::omnidir::stereoReconstruct (src/omnidir.cpp:1383-1539): the executable form of the specification
in DESIGN.md 7e.  All matcher arithmetic is integer (int64 here, so nothing wraps unseen).

The matcher restates StereoSGBM's MODE_SGBM as the reference calls it,
StereoSGBM::create(0, D, bs, 8 cn bs^2, 32 cn bs^2): five directions, disp12MaxDiff, preFilterCap,
uniquenessRatio and the speckle filter at their zero defaults.  Agreement with a real OpenCV is not
claimed bit for bit; the device is compared against this file and nothing else.

Notation: D = numDisparities, bs = SADWindowSize, r = bs // 2, cn channels, P1 = 8 cn bs^2,
P2 = 32 cn bs^2, images H x W with W > D; the left columns x in [D, W) are matched, W1 = W - D, and
the volumes below are indexed [y, x - D, d].
"""
import numpy as np

XYZRGB, XYZ = 1, 2
RECTIFY_PERSPECTIVE, RECTIFY_LONGLATI = 1, 3
BIG = 32767          # Lr(q, -1) = Lr(q, D)
INVALID = -16        # disparity x 16 of a pixel without a match
# the previous pixel (dy, dx) of the five paths, in the order S adds them
DIRECTIONS = ((0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1))


def penalties(cn, bs):
    return 8 * cn * bs * bs, 32 * cn * bs * bs


# ------------------------------------------------------------------ 1. signals
def channels_of(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    return [img.astype(np.int64)] if img.ndim == 2 else [img[:, :, c].astype(np.int64) for c in range(img.shape[2])]


def signals(p):
    """one channel p [H, W] -> (gradient signal, raw signal); both are 15 at x = 0 and x = W - 1"""
    H, W = p.shape
    up, dn = p[np.clip(np.arange(H) - 1, 0, H - 1)], p[np.clip(np.arange(H) + 1, 0, H - 1)]
    g = np.full((H, W), 15, np.int64)
    g[:, 1:-1] = np.clip(2 * (p[:, 2:] - p[:, :-2]) + (up[:, 2:] - up[:, :-2]) + (dn[:, 2:] - dn[:, :-2]), -15, 15) + 15
    raw = p.copy()
    raw[:, 0] = raw[:, -1] = 15
    return g, raw


def lo_hi(s):
    """the interval a signal sweeps half a pixel to either side (Birchfield-Tomasi); floor halves"""
    lo, hi = s.copy(), s.copy()
    left = (s[:, 1:] + s[:, :-1]) // 2      # (s[x] + s[x - 1]) / 2 for x > 0
    lo[:, 1:], hi[:, 1:] = np.minimum(lo[:, 1:], left), np.maximum(hi[:, 1:], left)
    lo[:, :-1], hi[:, :-1] = np.minimum(lo[:, :-1], left), np.maximum(hi[:, :-1], left)   # and for x < W - 1
    return lo, hi


# ------------------------------------------------------------------ 2. pixel cost
def bt_cost(u, v, loL, hiL, loR, hiR):
    c0 = np.maximum(0, np.maximum(u - hiR, loR - u))
    c1 = np.maximum(0, np.maximum(v - hiL, loL - v))
    return np.minimum(c0, c1)


def pixel_cost(left, right, D):
    """pix [H, W1, D]"""
    L, R = channels_of(left), channels_of(right)
    H, W = L[0].shape
    assert W > D and len(L) == len(R) and R[0].shape == (H, W)
    xs = np.arange(D, W)
    pix = np.zeros((H, W - D, D), np.int64)
    for pl, pr in zip(L, R):
        for sl, sr, shift in zip(signals(pl), signals(pr), (0, 2)):
            (loL, hiL), (loR, hiR) = lo_hi(sl), lo_hi(sr)
            for d in range(D):
                xr = xs - d
                pix[:, :, d] += bt_cost(sl[:, xs], sr[:, xr], loL[:, xs], hiL[:, xs], loR[:, xr], hiR[:, xr]) >> shift
    return pix


# ------------------------------------------------------------------ 3. block cost
def block_cost(pix, bs):
    H, W1, _ = pix.shape
    r = bs // 2
    C = np.zeros_like(pix)
    for dy in range(-r, r + 1):
        yy = np.clip(np.arange(H) + dy, 0, H - 1)
        for dx in range(-r, r + 1):
            C += pix[yy][:, np.clip(np.arange(W1) + dx, 0, W1 - 1)]
    return C


# ------------------------------------------------------------------ 4. paths
def path_step(Cp, Lq, P1, P2):
    """Lr(p, .) from C(p, .) and Lr(q, .), arrays [..., D]"""
    big = np.full(Lq.shape[:-1] + (1,), BIG, np.int64)
    m = Lq.min(-1, keepdims=True)
    below = np.concatenate([big, Lq[..., :-1]], -1) + P1
    above = np.concatenate([Lq[..., 1:], big], -1) + P1
    return Cp + np.minimum(np.minimum(Lq, m + P2), np.minimum(below, above)) - (m + P2)


def path(C, dy, dx, P1, P2):
    """Lr [H, W1, D] of the paths whose previous pixel is (y + dy, x + dx)"""
    H, W1, _ = C.shape
    L = np.zeros_like(C)
    if dy == 0:
        for x in (range(W1) if dx < 0 else range(W1 - 1, -1, -1)):
            q = x + dx
            L[:, x] = path_step(C[:, x], L[:, q], P1, P2) if 0 <= q < W1 else C[:, x] - P2
        return L
    for y in range(H):
        if y == 0:
            L[0] = C[0] - P2
            continue
        q = np.arange(W1) + dx
        inside = (q >= 0) & (q < W1)
        L[y] = path_step(C[y], L[y - 1][np.clip(q, 0, W1 - 1)], P1, P2)
        L[y][~inside] = C[y][~inside] - P2
    return L


def sat16(a):
    return np.clip(a, -32768, 32767)


def aggregate(C, P1, P2, saturate=True, stats=None):
    """S [H, W1, D]: int16 saturation after the first four directions, and again after the fifth"""
    Ls = [path(C, dy, dx, P1, P2) for dy, dx in DIRECTIONS]
    four = Ls[0] + Ls[1] + Ls[2] + Ls[3]
    if stats is not None:
        stats["max_four"] = int(four.max())
        stats["max_five"] = int((four + Ls[4]).max())
    if not saturate:
        return four + Ls[4]
    return sat16(sat16(four) + Ls[4])


# ------------------------------------------------------------------ 5. winner
def winner_row(S):
    """S [n, D] -> (disp x 16 [n], d* [n], min S [n]): the smallest d attaining the minimum, then the
    parabola through its neighbours with a floor division"""
    D = S.shape[-1]
    ds = S.argmin(-1)
    n = np.arange(S.shape[0])
    mn = S[n, ds]
    disp = 16 * ds
    mid = (ds > 0) & (ds < D - 1)
    sm, sp = S[n, np.maximum(ds - 1, 0)], S[n, np.minimum(ds + 1, D - 1)]
    den = np.maximum(sm + sp - 2 * mn, 1)
    sub = ((sm - sp) * 16 + den) // (2 * den)
    return np.where(mid, disp + sub, disp), ds, mn


# ------------------------------------------------------------------ 6. left-right check
def disp2_row(ds, mn, D, W):
    """disp2 [W] of one row from d* and min S over x' = x - D: per right column the d* of the left
    pixel with the smallest min S, ties to the larger x; -1 where no left pixel maps"""
    disp2 = np.full(W, -1, np.int64)
    best = np.zeros(W, np.int64)
    for xp in range(len(ds)):          # x ascending, <= : a tie goes to the larger x
        x = xp + D
        xr = x - int(ds[xp])
        if disp2[xr] < 0 or mn[xp] <= best[xr]:
            disp2[xr], best[xr] = ds[xp], mn[xp]
    return disp2


def lr_check_row(disp, disp2, D):
    """disp [W] (x 16; columns < D are INVALID) -> the same with the pixels that fail both tests INVALID"""
    W = len(disp)
    out = disp.copy()
    for x in range(D, W):
        d1 = int(disp[x])
        a, b = d1 >> 4, (d1 + 15) >> 4
        xa, xb = x - a, x - b
        if (0 <= xa < W and disp2[xa] >= 0 and abs(disp2[xa] - a) > 1 and
                0 <= xb < W and disp2[xb] >= 0 and abs(disp2[xb] - b) > 1):
            out[x] = INVALID
    return out


def disparity_from_S(S, D, W):
    H = S.shape[0]
    out = np.full((H, W), INVALID, np.int64)
    for y in range(H):
        disp, ds, mn = winner_row(S[y])
        out[y, D:] = disp
        out[y] = lr_check_row(out[y], disp2_row(ds, mn, D, W), D)
    return out.astype(np.int16)


def sgbm(left, right, D, bs, saturate=True, stats=None):
    """int16 [H, W]: disparity x 16 of the left image, INVALID where there is none"""
    left, right = np.asarray(left), np.asarray(right)
    cn = 1 if left.ndim == 2 else left.shape[2]
    P1, P2 = penalties(cn, bs)
    C = block_cost(pixel_cost(left, right, D), bs)
    assert C.max() <= 32767
    return disparity_from_S(aggregate(C, P1, P2, saturate, stats), D, left.shape[1])


# ------------------------------------------------------------------ the tail of stereoReconstruct
def gray_of(img):
    """cvtColor(COLOR_RGB2GRAY) of an 8-bit image in OpenCV's fixed point; a 1-channel image is its own gray"""
    if img.ndim == 2:
        return img
    c = img.astype(np.int64)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def real_disparity(disp16, rec1):
    """float32 disparity: disp / 16, then 0 where the first rectified image is black"""
    real = disp16.astype(np.float32) / np.float32(16.0)
    real[gray_of(rec1) <= 0] = np.float32(0.0)
    return real


def point_cloud(real, rec1, Knew, T, flag, point_type, new_size):
    """float32 [n, 3] or [n, 6]: the reference's loop `for i < new_size.width: for j < new_size.height`
    (column-major; an empty new_size gives no points), a point wherever real > 15.  Also returns the
    float32 depth of every point (the bar of the longlati coordinates is stated in it)."""
    w, h = (0, 0) if new_size is None else new_size
    Knew = np.asarray(Knew, np.float64).reshape(3, 3)
    Kinv = np.linalg.inv(Knew)
    bf = float(np.linalg.norm(np.asarray(T, np.float64))) * Knew[0, 0]
    ii, jj = np.nonzero(real[:h, :w].T > 15)          # sorted by i, then j
    rd = real[jj, ii]
    depth = (bf / rd.astype(np.float64)).astype(np.float32)
    x = (Kinv[0, 0] * ii + Kinv[0, 1] * jj + Kinv[0, 2]).astype(np.float32)
    y = (Kinv[1, 0] * ii + Kinv[1, 1] * jj + Kinv[1, 2]).astype(np.float32)
    if flag == RECTIFY_LONGLATI:
        xyz = np.stack([-np.cos(x), -np.sin(x) * np.cos(y), np.sin(x) * np.sin(y)], -1).astype(np.float32)
    else:
        xyz = np.stack([x, y, np.ones_like(x)], -1)
    xyz = xyz * depth[:, None]
    assert xyz.dtype == np.float32
    if point_type == XYZ:
        return xyz, depth
    px = rec1[jj, ii]
    rgb = np.repeat(px[:, None], 3, 1) if rec1.ndim == 2 else px
    return np.concatenate([xyz, rgb.astype(np.float32)], 1), depth


# ------------------------------------------------------------------ scenes the tests share
def texture(rng, H, W, cn=1):
    return rng.integers(0, 256, (H, W) if cn == 1 else (H, W, cn), dtype=np.uint8)


def shifted_pair(rng, H, W, shift, cn=1):
    """a random texture seen at one disparity: left[x] = right[x - shift]"""
    wide = texture(rng, H, W + shift, cn)
    return np.ascontiguousarray(wide[:, :W]), np.ascontiguousarray(wide[:, shift:shift + W])


def two_level_pair(rng, H, W, d_left, d_right, split, cn=1):
    """disparity d_left left of column `split` of the left image and d_right (> d_left) from it on: the
    right image is a texture, the left image copies it from x - d; the near half occludes"""
    right = texture(rng, H, W + d_right, cn)[:, :W]
    wide = texture(rng, H, W + d_right, cn)
    wide[:, :W] = right
    x = np.arange(W)
    src = np.where(x < split, x - d_left, x - d_right)
    fill = texture(rng, H, W, cn)
    left = np.where((src >= 0).reshape((1, W) + (1,) * (right.ndim - 2)), right[:, np.clip(src, 0, W - 1)], fill)
    return np.ascontiguousarray(left.astype(np.uint8)), np.ascontiguousarray(right)


# ------------------------------------------------------------------ a rig whose rectification is the identity
# Two pinhole cameras (xi = 0, no distortion) side by side: R = I and T along -x give R1 = R2 = I, so with
# Knew = K the rectified image is the source and every pixel of `real` can be set through the public entry.
IDENT_F = 100.0
IDENT_T = np.array([-0.3, 0.0, 0.0])      # bf = 0.3 * 100 = 30: a 20 px shift lies at depth 1.5
IDENT_D = np.zeros(4)
SEG_ROWS = 64                             # rows of one column segment of the device's cloud stage


def ident_k(w, h, dx=0.0, dy=0.0):
    """the identity rig's camera matrix for a w x h image: the principal point a quarter pixel off the
    centre, moved by (dx, dy).  Off the pixel grid on purpose: in the column and the row of a principal
    point that lies on a pixel the cloud's x or y is 0 in exact arithmetic, what comes out is the rounding
    residue of Kinv00 * i + Kinv02 (0 or some 1e-17, depending on how the inverse was rounded), and a
    distance in ulp between two such residues means nothing"""
    return np.array([[IDENT_F, 0, w / 2 + 0.25 + dx], [0, IDENT_F, h / 2 + 0.25 + dy], [0, 0, 1]])


def cloud_scene(kind, H, W, cn=1, seed=7):
    """the pairs of tests/test_omnidir_cloud.py: a texture seen at 20 px (15 px for `threshold`, the
    cloud's own bar), with parts of the left image black -- black left pixels have real = 0"""
    left, right = shifted_pair(np.random.default_rng(seed), H, W, 15 if kind == "threshold" else 20, cn)
    if kind == "black":
        left[:] = 0
    elif kind == "bands":          # every other band of five columns, and the whole second segment of rows
        left[:, (np.arange(W) // 5) % 2 == 1] = 0
        left[SEG_ROWS:2 * SEG_ROWS] = 0
    elif kind == "tail":           # three pixels at the very end of the cloud's order
        keep = left[H - 1, W - 3:].copy()
        left[:] = 0
        left[H - 1, W - 3:] = keep
    else:
        assert kind in ("dense", "threshold"), kind
    return left, right


def slot_counts(real, new_size):
    """int [w, n_seg]: points per column and segment of SEG_ROWS rows, in the order the device scans them"""
    w, h = new_size
    n_seg = (h + SEG_ROWS - 1) // SEG_ROWS
    pts = np.zeros((n_seg * SEG_ROWS, w), np.int64)
    pts[:h] = real[:h, :w] > 15
    return pts.reshape(n_seg, SEG_ROWS, w).sum(1).T


# ------------------------------------------------------------------ a rendered stereo pair
# the two Mei cameras of test_rectified_stereo_pair_rows_agree at 160 x 120
RIG_SIZE = (160, 120)
RIG_K = [np.array([[225.0, 0.1, 80.375], [0, 224.0, 59.55], [0, 0, 1]]),
         np.array([[226.25, -0.075, 79.25], [0, 224.75, 60.775], [0, 0, 1]])]
RIG_XI = [1.6, 1.55]
RIG_D = [np.array([-0.08, 0.02, 0.001, -0.0015]), np.array([-0.06, 0.015, -0.0008, 0.001])]
RIG_OM, RIG_T = np.array([0.02, -0.03, 0.01]), np.array([-0.3, 0.01, 0.02])
PLANE_Z, PLANE_HALF = 1.5, (0.6, 0.45)   # a textured rectangle facing the first camera; black around it


def rig_knew(flag):
    """100 px per unit (perspective) or per radian (longlati), the optical axis at the image centre: the
    plane's disparity is 0.3 * 100 / 1.5 = 20 px, above the cloud's threshold of 15"""
    w, h = RIG_SIZE
    if flag == RECTIFY_LONGLATI:
        return np.array([[100.0, 0, w / 2 - 50 * np.pi], [0, 100.0, h / 2 - 50 * np.pi], [0, 0, 1]])
    return np.array([[100.0, 0, w / 2], [0, 100.0, h / 2], [0, 0, 1]])


def render_plane_pair(seed, cn):
    """both cameras' views of the plane by inverse mapping: each pixel's ray (the inverse of the oracle's
    projection, npundistort.undistort_points) is cut with the plane and a random texture of 0.03-unit
    texels is read there bilinearly; values 40 .. 255 on the plane, 0 off it"""
    import npundistort as U
    rng = np.random.default_rng(seed)
    w, h = RIG_SIZE
    tex = rng.integers(40, 256, (64, 64, cn)).astype(np.float64)
    jj, ii = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    px = np.stack([jj.ravel(), ii.ravel()], -1)
    R = U.rotation(RIG_OM)
    out = []
    for c in range(2):
        xy = U.undistort_points(px, RIG_K[c], RIG_D[c], RIG_XI[c])
        ray = np.concatenate([xy, np.ones((len(xy), 1))], 1)
        if c == 0:
            org, dirs = np.zeros(3), ray
        else:               # X2 = R X1 + T: the ray in the first camera's frame
            org, dirs = -R.T @ RIG_T, ray @ R
        t = (PLANE_Z - org[2]) / dirs[:, 2]
        P = org + t[:, None] * dirs
        on = (np.abs(P[:, 0]) <= PLANE_HALF[0]) & (np.abs(P[:, 1]) <= PLANE_HALF[1]) & (t > 0)
        u = np.clip((P[:, 0] + 1.0) / 0.03, 0, 62.999)
        v = np.clip((P[:, 1] + 1.0) / 0.03, 0, 62.999)
        u0, v0 = u.astype(int), v.astype(int)
        fu, fv = (u - u0)[:, None], (v - v0)[:, None]
        val = ((1 - fu) * (1 - fv) * tex[v0, u0] + fu * (1 - fv) * tex[v0, u0 + 1] +
               (1 - fu) * fv * tex[v0 + 1, u0] + fu * fv * tex[v0 + 1, u0 + 1])
        img = np.where(on[:, None], np.rint(val), 0).astype(np.uint8).reshape(h, w, cn)
        out.append(np.ascontiguousarray(img[:, :, 0] if cn == 1 else img))
    return out


def model_rectify(img, c, R, flag):
    """undistortImage by the numpy model: its own fixed-point maps, then its remap"""
    import npundistort as U
    u, v = U.map_uv(RIG_K[c], RIG_D[c], RIG_XI[c], R, rig_knew(flag), RIG_SIZE, flag)
    return U.remap(img, *U.fixed_maps(*U.fixed_units(u, v)))


def plane_pixels(flag, R1):
    """bool [h, w]: the rectified first image's pixels whose ray meets the plane's rectangle"""
    w, h = RIG_SIZE
    Kinv = np.linalg.inv(rig_knew(flag))
    jj, ii = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x = Kinv[0, 0] * jj + Kinv[0, 1] * ii + Kinv[0, 2]
    y = Kinv[1, 0] * jj + Kinv[1, 1] * ii + Kinv[1, 2]
    if flag == RECTIFY_LONGLATI:
        d = np.stack([-np.cos(x), -np.sin(x) * np.cos(y), np.sin(x) * np.sin(y)], -1)
    else:
        d = np.stack([x, y, np.ones_like(x)], -1)
    d = d @ R1                      # rectified frame -> the first camera's frame (R1^T d)
    t = PLANE_Z / d[..., 2]
    P = t[..., None] * d
    return (t > 0) & (np.abs(P[..., 0]) <= PLANE_HALF[0] - 0.05) & (np.abs(P[..., 1]) <= PLANE_HALF[1] - 0.05)
