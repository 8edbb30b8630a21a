"""The pinhole calibrateCamera's device arithmetic on the CPU (no GPU needed).

tests/cpp/test_pincalib_replay.cpp compiles csrc/mcc_pincalib_device.hpp -- what one wavefront of k_pc_lin
and k_pc_try runs for a view -- for the host with one lane and checks the analytic pose and intrinsic rows
against central differences of pnp_residual, the masked and aspect-coupled global rows, and the whole
Levenberg-Marquardt trial sequence (three-pass linearisation, damped elimination, reduced 12 x 12 solve,
back-substitution, accept / reject) on exact data.  The lanes' summation order and the tickets exist only on
the GPU: tests/test_calibrate_camera.py covers those, and tests/test_calibrate_camera_steps.py compares every
step with an independent one (tests/test_pincalib_step_cpu.py does that for one lane)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_device_arithmetic_replayed_on_the_host(tmp_path):
    exe = str(tmp_path / "test_pincalib_replay")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-I", os.path.join(HERE, "cpp", "hipstub"),
                    "-I", os.path.join(ROOT, "multi_camera_calibration_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "test_pincalib_replay.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "replay ok" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
