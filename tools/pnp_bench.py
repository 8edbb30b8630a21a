"""Measures the batched solvePnP (mcc_solve_pnp_batch, k_pnp) against the host solver on one machine.

    python tools/pnp_bench.py [--repeats 7] [--host-views 2000]

Prints one JSON line.  Per batch size -- config2's 2 000 edges and config3's 40 000 -- of 88-corner
planar views (the 11 x 8 board, 0.2 px noise, 5 distortion coefficients, poses drawn around the rig's):
device_ms (HIP events around the launch alone, median of --repeats calls after one uncounted call that
loads the code object), views per second from it, the wall time of the whole call (uploads, launch,
downloads), and the host's mcc::pnp::solvePnP microseconds per view on the first --host-views of the same
views (one CPU core of the same machine).  tools/pnp_bench.cpp does the timing; this builds and runs it."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from multi_camera_calibration_amd import api  # noqa: E402

BATCHES = {"config2": 2000, "config3": 40000}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-views", type=int, default=2000)
    args = ap.parse_args()
    api.build()
    libdir = os.path.dirname(api.LIB_PATH)
    out = {"workload": "solvePnP, 88-corner planar views, 0.2 px noise, nd = 5, max_iter = 50"}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "pnp_bench")
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "pnp_bench.cpp"), "-L", libdir, "-lmcc_host", "-lmcc",
                        f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
        for name, n_views in BATCHES.items():
            r = subprocess.run([exe, str(n_views), str(args.repeats), str(args.host_views)], capture_output=True,
                               text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(r.stdout + r.stderr)
            t = r.stdout.split()
            kv = {t[i]: float(t[i + 1]) for i in range(0, len(t), 2)}
            kv["views_per_s"] = kv["n_views"] / (kv["device_ms_median"] * 1e-3)
            kv["device_us_per_view"] = kv["device_ms_median"] * 1e3 / kv["n_views"]
            kv["host_over_device"] = kv["host_us_per_view"] / kv["device_us_per_view"]
            out[name] = kv
    print(json.dumps(out))


if __name__ == "__main__":
    main()
