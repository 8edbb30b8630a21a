"""The C++ mirror of the pinhole rectification (include/mcc_calib.hpp: mcc::calib::undistortPoints,
initUndistortRectifyMap, undistort, stereoRectify, implemented in libmcc_host.so).

tests/cpp/test_pinrect.cpp is compiled with g++ against libmcc.so and libmcc_host.so.  CPU: it builds without warnings
and its host-only selftest passes (stereoRectify's algebra, the wrapper's exceptions with the library's message).
GPU: its `run` mode writes the maps, points and image it got through the mirror, and they are held here to the bars
of tests/test_pinhole_rectify.py against the numpy model: float maps within 1 float32 ulp, fixed maps within 1 unit,
at most max(2, 1e-4 w h) pixels different, points within 16 x |float64 model - long double model|, the image
bit-equal to the model's remap through the device's own fixed maps."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import nprectify as N  # noqa: E402
import npundistort as U  # noqa: E402
from multi_camera_calibration_amd import api  # noqa: E402
from ulp import f32_ulp_diff  # noqa: E402

SRC = os.path.join(HERE, "cpp", "test_pinrect.cpp")
K1 = np.array([[900.0, 0, 655], [0, 905, 470], [0, 0, 1]])
D1 = np.array([-0.25, 0.08, 1e-3, -5e-4, 0.0])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    api.build()
    libdir = os.path.dirname(api.LIB_PATH)
    out = str(tmp_path_factory.mktemp("cpp") / "test_pinrect")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    SRC, "-L", libdir, "-lmcc_host", "-lmcc", f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    return out


def test_cpp_mirror_selftest(exe):
    r = subprocess.run([exe, "selftest"], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "selftest ok" in r.stdout


@pytest.mark.gpu
def test_cpp_mirror_on_the_device(exe, tmp_path):
    r = subprocess.run([exe, "run", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "run ok" in r.stdout, r.stdout + r.stderr
    w, h, sw, sh = 97, 61, 160, 120
    load = lambda name, t: np.fromfile(os.path.join(str(tmp_path), name), t)   # noqa: E731
    rect = load("rect.f64", np.float64)
    R1, P1 = rect[0:9].reshape(3, 3), rect[18:30].reshape(3, 4)
    # maps
    u, v = N.map_uv(K1, D1, R1, P1, (w, h))
    fu, fv = load("float_u.f32", np.float32).reshape(h, w), load("float_v.f32", np.float32).reshape(h, w)
    du, dv = f32_ulp_diff(fu, u.astype(np.float32)), f32_ulp_diff(fv, v.astype(np.float32))
    assert du.max() <= 1 and dv.max() <= 1 and int(((du > 0) | (dv > 0)).sum()) <= max(2, 1e-4 * w * h)
    iu, iv = U.fixed_units(u, v)
    m1, m2 = load("fixed_1.i16", np.int16).reshape(h, w, 2), load("fixed_2.u16", np.uint16).reshape(h, w)
    gu, gv = m1[..., 0].astype(np.int64) * 32 + (m2 & 31), m1[..., 1].astype(np.int64) * 32 + (m2 >> 5)
    du, dv = np.abs(gu - iu), np.abs(gv - iv)
    assert du.max() <= 1 and dv.max() <= 1 and int(((du > 0) | (dv > 0)).sum()) <= max(2, 1e-4 * w * h)
    # points
    src, got = load("points_src.f64", np.float64).reshape(-1, 2), load("points_dst.f64", np.float64).reshape(-1, 2)
    assert len(src) == 4097
    m64 = N.undistort_points(src, K1, D1, R1, P1, 20)
    mld = N.undistort_points(src, K1, D1, R1, P1, 20, dtype=np.longdouble)
    tol = 16 * float(np.abs(m64.astype(np.longdouble) - mld).max())
    err = float(np.abs(got - m64).max())
    print(f"C++ undistortPoints: |device - float64 model| = {err:.3e}, bar = {tol:.3e}")
    assert err <= tol
    # image: through the device's own fixed maps
    frame = load("image_src.u8", np.uint8).reshape(sh, sw, 3)
    i1, i2 = load("image_1.i16", np.int16).reshape(h, w, 2), load("image_2.u16", np.uint16).reshape(h, w)
    want = U.remap(frame, i1, i2)
    assert want.any()
    assert np.array_equal(load("image_dst.u8", np.uint8).reshape(h, w, 3), want)
