"""Measures the pinhole rectification (include/mcc.h): one JSON line per workload, each the median of
--repeats runs with their range, after one warm-up run.

    python tools/pinrect_bench.py [--repeats 5] [--points 1000000]
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/pinrect_bench.py

  map build     device_ms (HIP events around k_pr_map) at 1920x1080 and 1280x960, nd 5 and nd 8, float and fixed maps;
                the camera is tests/calib_cases.py's, scaled to the frame, rectified by a small rotation
  points        device_ms (around k_pr_points) of --points pixels at 20 iterations, nd 5
  remap         one PinholeRectifier.remap at 1280x960, 1 and 3 channels: wall time of the call (one upload, one
                kernel, one download)
  comparison    in the same process: api.omnidir_init_undistort_rectify_map (perspective, 1280x960, fixed maps), wall
                time of the call next to the pinhole call's wall time (the omnidir entry point reports no device time;
                the kernels' own times are in a rocprofv3 run of this tool), and mcc::pnp::undistortPoints on the host,
                one call per point (tools/pinrect_host.cpp, one CPU core)
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from multi_camera_calibration_amd import api  # noqa: E402

G = np.array([900.0, 905.0, 655.0, 470.0])                 # fx fy cx cy at 1280 x 960
D5 = np.array([-0.25, 0.08, 1e-3, -5e-4, 0.0])
D8 = np.array([-0.25, 0.08, 1e-3, -5e-4, 0.01, 0.02, -0.01, 0.005])
OM = np.array([0.05, -0.08, 0.03])


def camera(w):
    s = w / 1280.0
    return np.array([[G[0] * s, 0, G[2] * s], [0, G[1] * s, G[3] * s], [0, 0, 1.0]])


def stats(runs, unit):
    return {f"median_{unit}": statistics.median(runs), f"min_{unit}": min(runs), f"max_{unit}": max(runs), f"runs_{unit}": runs}


def measure(fn, repeats):
    """fn() -> a time; one warm-up, then `repeats` runs"""
    fn()
    return [fn() for _ in range(repeats)]


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def host_library():
    libdir = os.path.dirname(api.LIB_PATH)
    out = os.path.join(tempfile.mkdtemp(prefix="pinrect_bench_"), "libpinrect_host.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "pinrect_host.cpp"), "-L", libdir, "-lmcc_host", "-lmcc",
                    f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    H = ctypes.CDLL(out)
    f64p = ctypes.POINTER(ctypes.c_double)
    H.pinrect_host_undistort_ms.argtypes = [f64p, ctypes.c_int, f64p, f64p, ctypes.c_int, ctypes.c_int, f64p]
    H.pinrect_host_undistort_ms.restype = ctypes.c_double
    return H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=1000000)
    args = ap.parse_args()
    api.build()
    rep = args.repeats
    for (w, h) in ((1920, 1080), (1280, 960)):
        K = camera(w)
        for nd, D in ((5, D5), (8, D8)):
            for name, mt in (("float", api.MAP_FLOAT), ("fixed", api.MAP_FIXED)):
                runs = measure(lambda: api.init_undistort_rectify_map(K, D, OM, K, (w, h), mt, return_ms=True)[2], rep)
                print(json.dumps({"workload": f"k_pr_map {w}x{h} nd {nd} {name}", **stats(runs, "device_ms")}), flush=True)
    rng = np.random.default_rng(0)
    px = np.stack([rng.uniform(0, 1279, args.points), rng.uniform(0, 959, args.points)], -1)
    K = camera(1280)
    runs = measure(lambda: api.undistort_points(px, K, D5, OM, K, 20, return_ms=True)[1], rep)
    print(json.dumps({"workload": f"k_pr_points {args.points} points, 20 iterations, nd 5", **stats(runs, "device_ms")}), flush=True)
    for c in (1, 3):
        r = api.PinholeRectifier(K, D5, (1280, 960), channels=c, R=OM, P=K)
        frame = rng.integers(0, 256, (960, 1280) if c == 1 else (960, 1280, c), dtype=np.uint8)
        dst = np.zeros_like(frame)
        runs = measure(lambda: wall_ms(lambda: r.remap(frame, dst=dst)), rep)
        r.close()
        print(json.dumps({"workload": f"PinholeRectifier.remap 1280x960, {c} channel(s), upload + kernel + download",
                          **stats(runs, "wall_ms")}), flush=True)
    # comparison: the omnidir perspective map build through its entry point, next to the pinhole one the same way
    Ko = np.array([[420.5, 0.9, 640.3], [0.0, 418.7, 479.6], [0.0, 0.0, 1.0]])
    Do, Kn = np.array([-0.08, 0.02, 0.001, -0.0015]), np.array([[320.0, 0, 640], [0, 240.0, 480], [0, 0, 1]])
    runs = measure(lambda: wall_ms(lambda: api.omnidir_init_undistort_rectify_map(Ko, Do, 1.6, OM, Kn, (1280, 960), api.MAP_FIXED,
                                                                                  api.RECTIFY_PERSPECTIVE)), rep)
    print(json.dumps({"workload": "comparison: omnidir_init_undistort_rectify_map 1280x960 perspective fixed, whole call",
                      **stats(runs, "wall_ms")}), flush=True)
    runs = measure(lambda: wall_ms(lambda: api.init_undistort_rectify_map(K, D5, OM, K, (1280, 960), api.MAP_FIXED)), rep)
    print(json.dumps({"workload": "comparison: init_undistort_rectify_map 1280x960 nd 5 fixed, whole call", **stats(runs, "wall_ms")}),
          flush=True)
    H = host_library()
    f64p = ctypes.POINTER(ctypes.c_double)
    n = min(args.points, 200000)
    sub, out = np.ascontiguousarray(px[:n]), np.zeros((n, 2))
    Kc = np.ascontiguousarray(K)
    runs = measure(lambda: H.pinrect_host_undistort_ms(sub.ctypes.data_as(f64p), n, Kc.ctypes.data_as(f64p), D5.ctypes.data_as(f64p),
                                                       5, 20, out.ctypes.data_as(f64p)) * (args.points / n), rep)
    dev = api.undistort_points(sub, K, D5)
    print(json.dumps({"workload": f"comparison: mcc::pnp::undistortPoints on the host, one call per point, scaled from {n} to "
                                  f"{args.points} points", **stats(runs, "wall_ms"),
                      "max_abs_host_minus_device": float(np.abs(out - dev).max())}), flush=True)


if __name__ == "__main__":
    main()
