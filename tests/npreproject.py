"""numpy model of the pinhole reconstruction (include/mcc.h: mcc_reproject_image_to_3d, mcc_pinrecon_*,
mcc_stereo_reconstruct), written from the rules of DESIGN.md 7j and from nothing else: it shares no code with the
library.  It composes with tests/nprectify.py (maps), tests/npundistort.py (the remap) and tests/npsgbm.py (the
matcher) into a model of a whole compute.

  to_float(disp)                        a float32 disparity as is, an int16 one / 16 (exact)
  reproject(disp, Q, handle_missing)    float32 [h, w, 3]: float64 Q products summed left to right, one division, one
                                        rounding; a NaN is the quiet NaN 0x7FC00000
  cloud_mask(real, Q, roi, max_z)       bool [h, w]: the cloud rule
  cloud(real, points, rec1, Q, point_type, roi, max_z)   the points in column-major order
  output_frame(geo)                     the transposed-frame rule for a vertical pair
  compute(...)                          remap twice, match, float disparity, dense points, cloud
"""
import numpy as np

import nprectify as N
import npsgbm as M
import npundistort as U

XYZRGB, XYZ = M.XYZRGB, M.XYZ
BIG_Z = np.float32(10000.0)
QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def to_float(disp):
    disp = np.asarray(disp)
    if disp.dtype == np.int16:
        return disp.astype(np.float32) / np.float32(16.0)
    assert disp.dtype == np.float32
    return disp


def q_rows(Q, x, y, d):
    """(X, Y, Z, W) in float64: ((Q0 x + Q1 y) + Q2 d) + Q3 per row of Q, for float64 x, y, d that broadcast"""
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    with np.errstate(invalid="ignore"):   # 0 * inf for an infinite disparity
        return np.stack([((Q[r, 0] * x + Q[r, 1] * y) + Q[r, 2] * d) + Q[r, 3] for r in range(4)])


def homogeneous(real, Q):
    """(X, Y, Z, W) [4, h, w] of a disparity image"""
    h, w = real.shape
    x, y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    return q_rows(Q, x, y, real.astype(np.float64))


def reproject_points(x, y, d, Q):
    """float64 [n, 3]: the rule at arbitrary float64 positions and disparities, without the rounding to float32"""
    X, Y, Z, W = q_rows(Q, np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(d, np.float64))
    return np.stack([X / W, Y / W, Z / W], -1)


def reproject(disp, Q, handle_missing=False):
    real = to_float(disp)
    X, Y, Z, W = homogeneous(real, Q)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.stack([X / W, Y / W, Z / W], -1).astype(np.float32)
    out[np.isnan(out)] = QNAN
    if handle_missing:
        dmin = np.fmin.reduce(real.ravel())            # a NaN does not take part
        with np.errstate(invalid="ignore"):
            out[..., 2][real <= dmin] = BIG_Z
    return out


def cloud_mask(real, Q, roi=None, max_z=0.0):
    _, _, Z, W = homogeneous(real, Q)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = Z / W
        ok = (real > 0) & np.isfinite(W) & (W != 0) & (z > 0)
        if max_z > 0:
            ok &= z <= max_z
    if roi is not None:
        rx, ry, rw, rh = roi
        inside = np.zeros(real.shape, bool)
        inside[ry:ry + rh, rx:rx + rw] = True
        ok &= inside
    return ok


def cloud(real, points, rec1, Q, point_type, roi=None, max_z=0.0):
    """float32 [n, 3 or 6]: columns first, then rows; the dense point, then rectified image 1's colour"""
    ii, jj = np.nonzero(cloud_mask(real, Q, roi, max_z).T)      # sorted by column i, then row j
    xyz = points[jj, ii]
    if point_type == XYZ:
        return xyz
    px = rec1[jj, ii]
    rgb = np.repeat(px[:, None], 3, 1) if rec1.ndim == 2 else px
    return np.concatenate([xyz, rgb.astype(np.float32)], 1)


def output_frame(geo, new_size):
    """dict(R1 R2 P1 P2 Q roi1 roi2) of stereo_rectify for new_size = (W, H) -> the same in the frame of the handle's
    outputs, with size and transposed: a vertical pair (P2[1, 3] carries T f) has rows 0 and 1 of P1 and P2 swapped,
    columns 0 and 1 of Q swapped, the rois transposed and H x W outputs"""
    W, H = new_size
    P2 = np.asarray(geo["P2"], np.float64)
    vertical = P2[0, 3] == 0
    out = {k: np.array(geo[k], np.float64) for k in ("R1", "R2", "P1", "P2", "Q")}
    out["roi1"], out["roi2"] = tuple(geo["roi1"]), tuple(geo["roi2"])
    out["size"], out["transposed"] = (W, H), False
    if vertical:
        for k in ("P1", "P2"):
            out[k] = out[k][[1, 0, 2]]
        out["Q"] = out["Q"][:, [1, 0, 2, 3]]
        for k in ("roi1", "roi2"):
            x, y, w, h = out[k]
            out[k] = (y, x, h, w)
        out["size"], out["transposed"] = (H, W), True
    return out


def rectify(img, K, D, R, P, size):
    """one view through the model's own fixed-point maps and remap"""
    return U.remap(np.ascontiguousarray(img), *N.init_undistort_rectify_map(K, D, R, P, size, N.MAP_FIXED))


def compute(image1, image2, K1, D1, K2, D2, frame, num_disparities, sad_window_size, point_type=XYZRGB, use_roi=False,
            max_z=0.0):
    """frame: output_frame's dict (or PinholeReconstructor.info(), the same thing from the library)"""
    rec1 = rectify(image1, K1, D1, frame["R1"], frame["P1"], frame["size"])
    rec2 = rectify(image2, K2, D2, frame["R2"], frame["P2"], frame["size"])
    return tail(rec1, rec2, frame, num_disparities, sad_window_size, point_type, use_roi, max_z)


def tail(rec1, rec2, frame, num_disparities, sad_window_size, point_type=XYZRGB, use_roi=False, max_z=0.0):
    """everything after the remap"""
    disp16 = M.sgbm(rec1, rec2, num_disparities, sad_window_size)
    real = to_float(disp16)
    points = reproject(real, frame["Q"])
    pts = cloud(real, points, rec1, frame["Q"], point_type, frame["roi1"] if use_roi else None, max_z)
    return dict(rec1=rec1, rec2=rec2, disparity16=disp16, disparity=real, points=points, cloud=pts)
