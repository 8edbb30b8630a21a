"""Measures cv::omnidir::stereoReconstruct on the device (include/mcc_omnidir.h, mcc_omnirecon_*) at one
frame size.

    python tools/omnirecon_bench.py [--size 1280x960] [--disparities 128] [--window 5] [--frames 100]
                                    [--repeats 5] [--out profiles/omnidir_reconstruct/bench.jsonl]
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \
        python tools/omnirecon_bench.py --profile 3 --channels 1

Without --profile: per channel count (1, 3) one JSON line with the device time of one frame pair
(mcc_omnirecon_time: HIP events around --frames back-to-back computes -- both remaps, the matcher, the
float disparity and the cloud, no transfers -- on resident random frames; median of --repeats runs with
the range) and the bytes the matcher's kernels must move, per kernel and in all, with the share of the
HBM peak the whole frame reaches.  With N = height (width - D) D entries of the cost volume:

    k_sg_signals   reads both images, writes 8 B per pixel and channel of each
    k_sg_pix       reads those planes, writes 2 N
    k_sg_box       twice (bs > 1): reads 2 N, writes 2 N
    k_sg_path      first direction: reads 2 N, writes 4 N; the next three: read 6 N, write 4 N;
                   the fifth (with the winner): reads 6 N

With --profile N: N computes through one handle and nothing printed to measure; each kernel's device time
is read from rocprofv3's kernel statistics (a run of its own, as above)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from multi_camera_calibration_amd import api  # noqa: E402

XI = (1.6, 1.55)
DIST = (np.array([-0.08, 0.02, 0.001, -0.0015]), np.array([-0.06, 0.015, -0.0008, 0.001]))
OM, T = np.array([0.02, -0.03, 0.01]), np.array([-0.3, 0.01, 0.02])
HBM_BYTES_PER_S = 8.0e12   # the datasheet peak, as tools/omnirect_bench.py uses


def camera(w, h, k):
    return np.array([[0.33 * w + k, 0.9 - k, 0.5 * w + 0.3 - 2 * k], [0, 0.327 * w + k, 0.5 * h - 0.4 + 3 * k], [0, 0, 1.0]])


def matcher_bytes(w, h, c, D, bs):
    n = h * (w - D) * D
    out = {"k_sg_signals": 2 * w * h * c * (1 + 8), "k_sg_pix": 2 * w * h * c * 8 + 2 * n,
           "k_sg_box": (2 * 4 * n) if bs > 1 else 0, "k_sg_path(first)": 6 * n, "k_sg_path(2-4)": 3 * 10 * n,
           "k_sg_path(fifth)": 6 * n}
    return out, sum(out.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1280x960")
    ap.add_argument("--disparities", type=int, default=128)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--channels", type=int, nargs="*", default=[1, 3])
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w, h = (int(x) for x in args.size.split("x"))
    api.build()
    rng = np.random.default_rng(0)
    Knew = np.array([[w / 4, 0, w / 2], [0, h / 4, h / 2], [0, 0, 1.0]])
    lines = []
    for c in args.channels:
        rec = api.OmniReconstructor(camera(w, h, 0), DIST[0], XI[0], camera(w, h, 1), DIST[1], XI[1], OM, T,
                                    api.RECTIFY_PERSPECTIVE, args.disparities, args.window, (w, h), channels=c,
                                    new_size=(w, h), Knew=Knew, point_type=api.XYZRGB)
        try:
            if args.profile:
                frames = [rng.integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8) for _ in range(2)]
                for _ in range(args.profile):
                    rec.compute(*frames)
                continue
            ms = [rec.time(args.frames) for _ in range(args.repeats)]
        finally:
            rec.close()
        m = statistics.median(ms)
        per_kernel, alg = matcher_bytes(w, h, c, args.disparities, args.window)
        lines.append(json.dumps({
            "workload": f"omnidir stereoReconstruct, {w}x{h}, {c} channel(s), D={args.disparities}, bs={args.window}, perspective",
            "ms_per_frame": m, "ms_min": min(ms), "ms_max": max(ms), "ms_runs": ms, "frames": args.frames,
            "cost_volume_entries": h * (w - args.disparities) * args.disparities, "matcher_bytes_per_kernel": per_kernel,
            "matcher_bytes_per_frame": alg, "achieved_GBps": alg / (m * 1e-3) / 1e9,
            "hbm_frac": alg / (m * 1e-3) / HBM_BYTES_PER_S}))
        print(lines[-1], flush=True)
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
