"""Measures the pinhole reconstruction on the device (include/mcc.h) at one frame size: a rectified pair to
depth through mcc_pinrecon_*, and cv::reprojectImageTo3D alone through mcc_reproject_image_to_3d.

    python tools/pinrecon_bench.py [--size 1280x960] [--disparities 128] [--window 5] [--frames 100]
                                   [--repeats 5] [--calls 10] [--out profiles/pinhole_reconstruct/bench.jsonl]
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \
        python tools/pinrecon_bench.py --profile 3 --channels 1

Without --profile, one JSON line per shape:

  per channel count (1, 3)   the device time of one pair (mcc_pinrecon_time: HIP events around --frames back-to-back
                  computes -- both remaps, the matcher, the float disparity with the dense points, the cloud, no
                  transfers -- on resident random frames; median of --repeats runs with the range), and the wall time
                  of one compute() with its two uploads and its downloads (median of --calls, after one warm-up call).
  per disparity type         device_ms of mcc_reproject_image_to_3d with handle_missing off and on (median of --repeats
                  calls after one warm-up), beside the bytes it must move: 4 or 2 in and 12 out per pixel, and the
                  disparity once more for the minimum.

With --profile N: N computes through one handle and nothing printed to measure; each kernel's device time is read from
rocprofv3's kernel statistics (a run of its own, as above)."""
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

# the head rig of tests/stereo_calib_cases.py: 1280 x 960 cameras 120 mm apart
G1 = (900.0, 905.0, 655.0, 470.0, -0.25, 0.08, 1e-3, -5e-4, 0.0)
G2 = (925.0, 921.0, 630.0, 488.0, -0.23, 0.07, -8e-4, 6e-4, 0.0)
OM, T = np.array([0.02, -0.055, 0.012]), np.array([-120.0, 3.0, 6.0])
HBM_BYTES_PER_S = 8.0e12   # the datasheet peak, as tools/omnirecon_bench.py uses


def camera(g, w, h):
    s = w / 1280.0
    return np.array([[g[0] * s, 0, g[2] * s], [0, g[1] * s, h / 2 + (g[3] - 480.0) * s], [0, 0, 1.0]]), np.array(g[4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x960")
    ap.add_argument("--disparities", type=int, default=128)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--channels", type=int, nargs="*", default=[1, 3])
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w, h = (int(x) for x in args.size.split("x"))
    api.build()
    rng = np.random.default_rng(0)
    (K1, D1), (K2, D2) = camera(G1, w, h), camera(G2, w, h)
    lines = []
    for c in args.channels:
        rec = api.PinholeReconstructor(K1, D1, K2, D2, OM, T, args.disparities, args.window, (w, h), channels=c,
                                       point_type=api.XYZRGB)
        try:
            frames = [rng.integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8) for _ in range(2)]
            if args.profile:
                for _ in range(args.profile):
                    rec.compute(*frames)
                continue
            ms = [rec.time(args.frames) for _ in range(args.repeats)]
            rec.compute(*frames)
            wall = []
            for _ in range(args.calls):
                t0 = time.perf_counter()
                rec.compute(*frames)
                wall.append((time.perf_counter() - t0) * 1e3)
        finally:
            rec.close()
        lines.append(json.dumps({
            "workload": f"pinhole stereoReconstruct, {w}x{h}, {c} channel(s), D={args.disparities}, bs={args.window}",
            "ms_per_frame": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "ms_runs": ms, "frames": args.frames,
            "call_ms_with_copies": statistics.median(wall), "call_ms_min": min(wall), "call_ms_max": max(wall),
            "calls": args.calls, "cost_volume_entries": h * (w - args.disparities) * args.disparities}))
        print(lines[-1], flush=True)
    if not args.profile:
        Q = api.stereo_rectify(K1, D1, K2, D2, (w, h), OM, T)[4]
        d16 = rng.integers(-16, 16 * args.disparities, (h, w)).astype(np.int16)
        for name, disp in (("float", d16.astype(np.float32) / np.float32(16.0)), ("fixed16", d16)):
            for missing in (False, True):
                api.reproject_image_to_3d(disp, Q, missing)
                ms = [api.reproject_image_to_3d(disp, Q, missing, return_ms=True)[1] for _ in range(args.repeats)]
                m = statistics.median(ms)
                moved = w * h * (disp.itemsize * (2 if missing else 1) + 12)
                lines.append(json.dumps({
                    "workload": f"reprojectImageTo3D, {w}x{h}, {name} disparity, handle_missing {'on' if missing else 'off'}",
                    "device_ms": m, "ms_min": min(ms), "ms_max": max(ms), "ms_runs": ms, "bytes_moved": moved,
                    "achieved_GBps": moved / (m * 1e-3) / 1e9, "hbm_frac": moved / (m * 1e-3) / HBM_BYTES_PER_S}))
                print(lines[-1], flush=True)
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
