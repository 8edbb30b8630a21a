"""The batched solvePnP's device arithmetic on the CPU (no GPU needed).

tests/cpp/test_pnp_replay.cpp compiles csrc/mcc_pnp_device.hpp -- the code one wavefront of k_pnp runs
for a view -- for the host with one lane (tests/cpp/hipstub stands in for the HIP header) and checks it on
exact data against the truth (the C++ selftest's bounds, with and without the LM refinement), on noisy data
against mcc::pnp::solvePnP (the same minimum), and on views that cannot be solved (status 1 and 2).  It also
runs the pose, target and distortion lists of tests/test_pnp_generic.py and its near-planar relief sweep, so
that a case that fails is known to be the arithmetic's before a GPU sees it, and holds pnp_rows, the analytic
Jacobian, to central differences of pnp_residual entry by entry.  The
lanes' summation order and the LDS phases exist only on the GPU: tests/test_pnp_batch.py covers those."""
import os
import subprocess

from multi_camera_calibration_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_device_arithmetic_replayed_on_the_host(tmp_path):
    api.build()
    libdir = os.path.dirname(api.LIB_PATH)
    exe = str(tmp_path / "test_pnp_replay")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-I", os.path.join(HERE, "cpp", "hipstub"),
                    "-I", os.path.join(ROOT, "multi_camera_calibration_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "test_pnp_replay.cpp"), "-L", libdir, "-lmcc_host", "-lmcc",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "replay ok" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
