"""The C++ mirror of the pinhole stereo calibration (include/mcc_calib.hpp: mcc::calib::stereoCalibrate, implemented
in libmcc_host.so).

tests/cpp/test_stereo_calib.cpp is compiled with g++ against libmcc.so and libmcc_host.so.  CPU: it builds without
warnings and its host-only selftest passes (the wrapper's exceptions with the library's message).  GPU: its `run`
mode calibrates six exact view pairs, with the default CALIB_FIX_INTRINSIC and with all intrinsics free from a guess,
and holds the rms to 1e-8 px and the parameters to the bounds derived in its header."""
import os
import re
import subprocess

import pytest

from multi_camera_calibration_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpp", "test_stereo_calib.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    api.build()
    libdir = os.path.dirname(api.LIB_PATH)
    out = str(tmp_path_factory.mktemp("cpp") / "test_stereo_calib")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    SRC, "-L", libdir, "-lmcc_host", "-lmcc", f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    return out


def test_cpp_mirror_selftest(exe):
    r = subprocess.run([exe, "selftest"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "selftest ok" in r.stdout


@pytest.mark.gpu
def test_stereo_calibrate_on_exact_views(exe):
    r = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    m = re.search(r"measured rms (\S+) dK (\S+)", r.stdout)
    assert m, r.stdout + r.stderr
    assert float(m.group(1)) <= 1e-8
    assert r.returncode == 0 and "run ok" in r.stdout, r.stdout + r.stderr
