"""Measures the pinhole calibrateCamera (mcc_calibrate_camera: k_pc_lin + k_pc_try per trial) on one machine.

    python tools/calib_bench.py [--repeats 5] [--stereo]

Prints one JSON line.  Per view count -- 50 and 500 views of 88 corners (the 11 x 8 board, 0.2 px noise, five
distortion coefficients, from the closed-form start, cv::calibrateCamera's default criteria 30 / DBL_EPSILON) --
device_ms (HIP events around the whole loop: the evaluation of the start, every trial, and the host's read of the
loop state after each batch of eight trials; median of --repeats calls after one uncounted call that loads the
code object), the accepted steps, the trials run, device microseconds per trial from the two, the wall time of the
whole call (closed-form start, pose seeds by mcc_solve_pnp_batch, uploads, loop, downloads) and the rms.

With --stereo the same figures for the pinhole stereoCalibrate (mcc_stereo_calibrate: k_ps_lin + k_ps_try per trial) on
50 and 500 view pairs of the same board seen by two cameras 120 mm apart, all intrinsics free (flags 0: the start is
two calibrateCamera calls, whose time is in the wall time and not in device_ms), cv::stereoCalibrate's default criteria
30 / 1e-6."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from multi_camera_calibration_amd import api  # noqa: E402

SIZE = (1280, 960)
G = (900.0, 905.0, 655.0, 470.0, -0.25, 0.08, 1e-3, -5e-4)   # fx fy cx cy k1 k2 p1 p2


def views(n_views, seed):
    """n_views noisy views of the 11 x 8 board (40 mm), tilted 10-45 degrees about turning axes, 0.5-1.2 m away."""
    rng = np.random.default_rng(seed)
    i = np.arange(88)
    X = np.stack([40.0 * (i % 11 - 5.0), 40.0 * (i // 11 - 3.5), np.zeros(88)], axis=1)
    fx, fy, cx, cy, k1, k2, p1, p2 = G
    img = []
    for v in range(n_views):
        tilt, phi = np.deg2rad(rng.uniform(10.0, 45.0)), 2.399963 * v
        w = np.array([tilt * np.cos(phi), tilt * np.sin(phi), rng.uniform(-0.3, 0.3)])
        th = np.linalg.norm(w)
        k = w / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        Xc = X @ R.T + np.array([rng.uniform(-60, 60), rng.uniform(-40, 40), rng.uniform(500, 1200)])
        x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
        r2 = x * x + y * y
        cd = 1 + k1 * r2 + k2 * r2 * r2
        xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        img.append(np.stack([fx * xd + cx, fy * yd + cy], axis=1) + 0.2 * rng.standard_normal((88, 2)))
    return np.arange(n_views + 1, dtype=np.int32) * 88, np.tile(X, (n_views, 1)), np.concatenate(img)


G2 = (925.0, 921.0, 630.0, 488.0, -0.23, 0.07, -8e-4, 6e-4)   # the second camera of --stereo
RIG = (np.array([0.02, -0.055, 0.012]), np.array([-120.0, 3.0, 6.0]))


def rot(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def pixels(Xc, g):
    fx, fy, cx, cy, k1, k2, p1, p2 = g
    x, y = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r2 = x * x + y * y
    cd = 1 + k1 * r2 + k2 * r2 * r2
    xd = x * cd + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * cd + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([fx * xd + cx, fy * yd + cy], axis=1)


def stereo_views(n_views, seed):
    """views()'s board and poses (60 mm to the right, between the cameras) as two cameras 120 mm apart see them."""
    rng = np.random.default_rng(seed)
    i = np.arange(88)
    X = np.stack([40.0 * (i % 11 - 5.0), 40.0 * (i // 11 - 3.5), np.zeros(88)], axis=1)
    R = rot(RIG[0])
    img1, img2 = [], []
    for v in range(n_views):
        tilt, phi = np.deg2rad(rng.uniform(10.0, 45.0)), 2.399963 * v
        w = np.array([tilt * np.cos(phi), tilt * np.sin(phi), rng.uniform(-0.3, 0.3)])
        Xc = X @ rot(w).T + np.array([rng.uniform(0, 120), rng.uniform(-40, 40), rng.uniform(500, 1200)])
        img1.append(pixels(Xc, G) + 0.2 * rng.standard_normal((88, 2)))
        img2.append(pixels(Xc @ R.T + RIG[1], G2) + 0.2 * rng.standard_normal((88, 2)))
    return np.arange(n_views + 1, dtype=np.int32) * 88, np.tile(X, (n_views, 1)), np.concatenate(img1), np.concatenate(img2)


def stereo(repeats):
    out = {"workload": "stereoCalibrate, 88-corner planar view pairs, 0.2 px noise, nd = 5, flags 0, criteria 30 / 1e-6"}
    for n_views in (50, 500):
        off, obj, img1, img2 = stereo_views(n_views, seed=800 + n_views)
        ms, wall = [], []
        for rep in range(repeats + 1):
            t0 = time.perf_counter()
            r = api.stereo_calibrate(off, obj, img1, img2, SIZE, flags=0, return_ms=True)
            if rep:
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(r[14])
        med = statistics.median(ms)
        out[f"views_{n_views}"] = {"n_views": n_views, "device_ms_median": med, "device_ms_min": min(ms),
                                   "device_ms_max": max(ms), "iterations": r[12], "trials": r[15], "status": r[13],
                                   "device_us_per_trial": med * 1e3 / max(r[15], 1),
                                   "wall_ms_median": statistics.median(wall), "rms": r[0]}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stereo", action="store_true", help="measure mcc_stereo_calibrate instead")
    args = ap.parse_args()
    api.build()
    if args.stereo:
        return stereo(args.repeats)
    out = {"workload": "calibrateCamera, 88-corner planar views, 0.2 px noise, nd = 5, flags 0, criteria 30 / DBL_EPSILON"}
    for n_views in (50, 500):
        off, obj, img = views(n_views, seed=700 + n_views)
        ms, wall = [], []
        for rep in range(args.repeats + 1):
            t0 = time.perf_counter()
            r = api.calibrate_camera(off, obj, img, SIZE, return_ms=True)
            if rep:
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(r[8])
        med = statistics.median(ms)
        out[f"views_{n_views}"] = {"n_views": n_views, "device_ms_median": med, "device_ms_min": min(ms),
                                   "device_ms_max": max(ms), "iterations": r[6], "trials": r[9], "status": r[7],
                                   "device_us_per_trial": med * 1e3 / max(r[9], 1),
                                   "wall_ms_median": statistics.median(wall), "rms": r[0]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
