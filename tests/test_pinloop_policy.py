"""The Levenberg-Marquardt policy of the pinhole loops on the CPU (no GPU needed).

csrc/mcc_pincalib_internal.h holds the policy once: pc_accepts and pc_next, the transition of the device-resident
PcState that the last arriver of k_pc_try and of k_ps_try makes (pin_verdict, csrc/mcc_pinloop_device.hpp).
tests/cpp/test_pinloop_policy.cpp compiles it for the host and drives it through a table: the start with a finite,
an infinite and a NaN error; a rejection, the tenth in a row, a failed factorisation and a NaN error; an acceptance
at en == err and below, lambda at its floor; and the stop tests under criteria 1, 2 and 3."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_policy_table(tmp_path):
    exe = str(tmp_path / "test_pinloop_policy")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                    "-ffp-contract=off", "-I", os.path.join(HERE, "cpp", "hipstub"),
                    "-I", os.path.join(ROOT, "multi_camera_calibration_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(HERE, "cpp", "test_pinloop_policy.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "policy ok" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
