"""The C++ mirror of cv::omnidir::stereoReconstruct (include/mcc_omnidir.hpp, on the project's cv::Mat).

tests/cpp/test_omnirecon.cpp is compiled with g++ against libmcc.so and libmcc_host.so.  CPU: it builds
without warnings and its host-only selftest passes (the throws, the shim's 8-bit matrices).  GPU: its
`run` mode reads a rendered pair and what the numpy model (tests/npsgbm.py) expects from a file this test
writes -- the model's matcher and tail applied to the device's own rectified images, as in
tests/test_omnidir_reconstruct.py -- calls stereoReconstruct and compares with the same bars: images and
disparity equal, the cloud's count and order equal, coordinates within 2 float32 ulp (perspective) or
16 * 2^-24 * depth (longlati), colours equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import npsgbm as M  # noqa: E402
from multi_camera_calibration_amd import api  # noqa: E402

SRC = os.path.join(HERE, "cpp", "test_omnirecon.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    api.build()
    libdir = os.path.dirname(api.LIB_PATH)
    out = str(tmp_path_factory.mktemp("cpp") / "test_omnirecon")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    SRC, "-L", libdir, "-lmcc_host", "-lmcc", f"-Wl,-rpath,{libdir}", "-o", out], check=True)
    return out


def test_cpp_mirror_selftest(exe):
    r = subprocess.run([exe, "selftest"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "selftest ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("flag,cn,point_type", [(M.RECTIFY_PERSPECTIVE, 3, M.XYZRGB), (M.RECTIFY_LONGLATI, 1, M.XYZ)],
                         ids=["perspective-rgb", "longlati-gray"])
def test_cpp_mirror_on_device(exe, tmp_path, flag, cn, point_type):
    a, b = M.render_plane_pair(11, cn)
    w, h = M.RIG_SIZE
    # the device's own rectified images, then the model's matcher and tail on them
    _, rec1, rec2, _ = api.omnidir_stereo_reconstruct(a, b, M.RIG_K[0], M.RIG_D[0], M.RIG_XI[0], M.RIG_K[1], M.RIG_D[1],
                                                      M.RIG_XI[1], M.RIG_OM, M.RIG_T, flag, 32, 5, new_size=M.RIG_SIZE,
                                                      Knew=M.rig_knew(flag), point_type=point_type)
    real = M.real_disparity(M.sgbm(rec1, rec2, 32, 5), rec1)
    cloud, depth = M.point_cloud(real, rec1, M.rig_knew(flag), M.RIG_T, flag, point_type, M.RIG_SIZE)
    assert len(cloud) > 1000
    case = str(tmp_path / "case.bin")
    with open(case, "wb") as f:
        f.write(np.array([w, h, cn, flag, point_type, len(cloud)], np.int32).tobytes())
        for arr in (a, b, rec1, rec2, real, cloud, depth):
            f.write(np.ascontiguousarray(arr).tobytes())
    r = subprocess.run([exe, "run", case], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "run ok" in r.stdout
