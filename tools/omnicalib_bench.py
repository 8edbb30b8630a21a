"""Measures the device loop of cv::omnidir::calibrate (include/mcc_omnidir.h) on one config-4-shape
camera: n views of an 11x8 board (88 corners), one k_oc_step launch per loop iteration.

    python tools/omnicalib_bench.py [--views 1000] [--steps 200]
    python tools/omnicalib_bench.py --stereo [--views 1000] [--board 11x8] [--steps 200]

Prints one JSON line: ms per loop step (HIP events around graph-launched steps), corner
residual + Jacobian evals/s (2 x 16 Jacobian rows per corner), and the HBM roofline fraction of the
step's algorithmic bytes (40 B/corner of CV_64F obj xyz + img uv, plus 8 x (60 + 12 + 89 + 6) B
per view of Y / z / contribution / pose traffic).

--stereo measures cv::omnidir::stereoCalibrate's loop step (k_os_step, mcc_omnistereo_time_steps) on
a synthetic two-camera rig (rig.make_omni_stereo_views) and, in the same process, the single-camera
step (k_oc_step) on the left camera's views of the same shape.  Each figure is the median of
--repeats timed runs of --steps graph-launched steps.  Algorithmic bytes of a stereo step: 56
B/corner (obj xyz + two image points) plus 8 x (156 + 12 + 433 + 6) B per view."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from multi_camera_calibration_amd import api, rig  # noqa: E402


def stereo(args):
    import statistics
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import npstereo as S
    from oracle import oracle_py as O
    board = tuple(int(x) for x in args.board.split("x"))
    s = rig.make_omni_stereo_views(args.views, board=board, seed=4)
    N = int(s.off[1])
    p = S.start_params(s, pose_sigma=0.0)
    os_ = api.OmniStereoCalibrator(s.off, s.obj, s.img1, s.img2)
    oc = api.OmniCalibrator(s.off, s.obj, s.img1)
    p1 = O.omni_encode(s.omL, s.tL, s.K1, s.xi1, s.D1)
    ms2, ms1 = [], []
    for _ in range(args.repeats):   # alternately, so both see the same machine state
        ms2.append(os_.time_steps(p, args.steps))
        ms1.append(oc.time_steps(p1, args.steps))
    corners = int(s.off[-1])
    alg = 56 * corners + 8 * (156 + 12 + 433 + 6) * args.views
    m2, m1 = statistics.median(ms2), statistics.median(ms1)
    print(json.dumps({"workload": f"omnidir stereoCalibrate loop, {args.views} views x {N} corners, two cameras",
                      "stereo_us_per_step": m2 * 1e3, "stereo_us_runs": [x * 1e3 for x in ms2],
                      "mono_us_per_step": m1 * 1e3, "mono_us_runs": [x * 1e3 for x in ms1], "ratio": m2 / m1,
                      "steps": args.steps, "alg_bytes_per_step": alg, "achieved_GBps": alg / (m2 * 1e-3) / 1e9,
                      "hbm_frac": alg / (m2 * 1e-3) / 8.0e12}))
    os_.close()
    oc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--stereo", action="store_true")
    ap.add_argument("--board", default="11x8")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if args.stereo:
        return stereo(args)
    s = rig.make_omni_views(args.views, seed=4)
    from oracle import oracle_py as O
    p = O.omni_encode(s.om, s.t, s.K, s.xi, s.D)
    oc = api.OmniCalibrator(s.off, s.obj, s.img)
    ms = oc.time_steps(p, args.steps)
    corners = int(s.off[-1])
    alg = 40 * corners + 8 * (60 + 12 + 89 + 6) * args.views
    t0 = time.time()
    rms, K, xi, D, om, t, idx, iters = api.omnidir_calibrate(s.off, s.obj, s.img, s.image_size, 0, 3, 300, 1e-7)
    wall = time.time() - t0
    print(json.dumps({"workload": f"omnidir calibrate loop, {args.views} views x 88 corners (config-4 camera)",
                      "ms_per_step": ms, "corner_evals_per_s": corners / (ms * 1e-3),
                      "alg_bytes_per_step": alg, "achieved_GBps": alg / (ms * 1e-3) / 1e9,
                      "hbm_frac": alg / (ms * 1e-3) / 8.0e12,
                      "calibrate": {"iters": iters, "rms": rms, "wall_s": wall, "kept": int(len(idx))}}))
    oc.close()


if __name__ == "__main__":
    main()
