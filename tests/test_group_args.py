"""k_group's kernel arguments on the host (no GPU): tests/cpp/test_group_args.cpp is compiled with g++
against csrc/mcc_internal.h and the HIP headers.  Its static_asserts hold the argument segment's
layout (the leading block is 64 bytes, LinArgs follows it at a 64-byte multiple, GroupHot follows
LinArgs); run, it checks that the launch function's helpers fill every hot pointer from the LinArgs
field of the same name and pack the role dispatch's words."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multi_camera_calibration_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_group_kernel_arguments(tmp_path):
    exe = str(tmp_path / "test_group_args")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "test_group_args.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
