"""Measures the omnidir rectification kernels (include/mcc_omnidir.h) at one frame size.

    python tools/omnirect_bench.py [--size 1280x960] [--frames 2000] [--repeats 5]
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \
        python tools/omnirect_bench.py --maps 20

Without --maps: per channel count (1, 3) one JSON line with the device time of k_or_remap per frame
(mcc_omnirect_time_remap: HIP events around --frames back-to-back launches on a resident random
frame, median of --repeats runs) and its share of the HBM roofline.  Bytes a frame needs: the maps
(6 B per destination pixel), the destination (channels B per pixel) and the source, counted once
(channels B per source pixel; the four taps of neighbouring pixels share cache lines).  The map is
RECTIFY_PERSPECTIVE with Knew = [w/4 0 w/2; 0 h/4 h/2], which reads most of the source.

With --maps N: builds the fixed-point map of every RECTIFY_* flag N times and prints nothing to
measure; k_or_map's device time per flag is read from rocprofv3's kernel statistics (a run of its
own, as above)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from multi_camera_calibration_amd import api  # noqa: E402

XI, D, OM = 1.6, np.array([-0.08, 0.02, 0.001, -0.0015]), np.array([0.05, -0.08, 0.03])
HBM_BYTES_PER_S = 8.0e12   # the datasheet peak, as tools/omnicalib_bench.py uses


def camera(w, h):
    return np.array([[0.33 * w, 0.9, 0.5 * w + 0.3], [0, 0.327 * w, 0.5 * h - 0.4], [0, 0, 1.0]])


def knew(flags, w, h):
    if flags in (api.RECTIFY_PERSPECTIVE, api.RECTIFY_STEREOGRAPHIC):
        return np.array([[w / 4, 0, w / 2], [0, h / 4, h / 2], [0, 0, 1.0]])
    return np.array([[w / np.pi, 0, 0], [0, h / np.pi, 0], [0, 0, 1.0]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x960")
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--maps", type=int, default=0)
    args = ap.parse_args()
    w, h = (int(x) for x in args.size.split("x"))
    api.build()
    K = camera(w, h)
    if args.maps:
        for flags in (api.RECTIFY_PERSPECTIVE, api.RECTIFY_CYLINDRICAL, api.RECTIFY_LONGLATI, api.RECTIFY_STEREOGRAPHIC):
            for _ in range(args.maps):
                api.omnidir_init_undistort_rectify_map(K, D, XI, OM, knew(flags, w, h), (w, h), api.MAP_FIXED, flags)
        return
    rng = np.random.default_rng(0)
    flags = api.RECTIFY_PERSPECTIVE
    for c in (1, 3):
        r = api.OmniRectifier(K, D, XI, flags, (w, h), channels=c, P=knew(flags, w, h), R=OM)
        out = r.remap(rng.integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8))
        ms = [r.time_remap(args.frames) for _ in range(args.repeats)]
        r.close()
        m = statistics.median(ms)
        alg = w * h * (6 + c) + w * h * c
        print(json.dumps({"workload": f"omnidir undistortImage remap, {w}x{h}, {c} channel(s), perspective",
                          "us_per_frame": m * 1e3, "us_runs": [x * 1e3 for x in ms], "frames": args.frames,
                          "nonzero_output_share": float((out != 0).mean()), "alg_bytes_per_frame": alg,
                          "achieved_GBps": alg / (m * 1e-3) / 1e9, "hbm_frac": alg / (m * 1e-3) / HBM_BYTES_PER_S}))


if __name__ == "__main__":
    main()
