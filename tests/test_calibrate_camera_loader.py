"""MultiCameraCalibration(PINHOLE, ...) over a corner-file list: loadImages calibrates every camera with
cv::calibrateCamera on the GPU (reference src/multicalib.cpp:254-262), where it used to throw.

A two-camera pinhole rig is written as "cameraIdx-timestamp.yaml" files by tests/sample_data.py's writer and run
through build/multi_cameras_calibration --list --cameras 2 (no --omni): loadImages, initialize, optimizeExtrinsics.
The loaded intrinsics equal api.calibrate_camera on each camera's views (the finder's float32 points, _flags = 0,
cv::calibrateCamera's default criteria) cast to float32; the edges are the omni flow's for the same visibility:
camera by camera in list order, a photo vertex per timestamp in order of first appearance."""
import os
import subprocess

import numpy as np
import pytest

import sample_data as SD
from multi_camera_calibration_amd import api, rig


@pytest.fixture(scope="module")
def sample():
    api.build()
    return api.SAMPLE_PATH


def _rig():
    return rig.make_rig(n_cams=2, n_views=24, seed=13, visibility=0.8)


def test_pinhole_list_reaches_the_device_without_gpu(sample, tmp_path):
    """Without a GPU the flow fails at the first device call, loudly, and no longer at the loader's own throw."""
    if os.path.exists("/dev/kfd"):
        pytest.skip("checks the no-GPU failure mode")
    p = _rig()
    lst, _, _ = SD.write_omni_list(p, str(tmp_path / "pin"))
    r = subprocess.run([sample, "--list", lst, "--cameras", "2", "--init-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "error" in r.stderr
    assert "not restated" not in r.stderr and "calibrateCamera" in r.stderr, r.stderr


@pytest.mark.gpu
def test_pinhole_base_class_flow(sample, tmp_path):
    p = _rig()
    lst, files, stamps = SD.write_omni_list(p, str(tmp_path / "pin"))
    dump, res, out = str(tmp_path / "p.bin"), str(tmp_path / "r.txt"), str(tmp_path / "res.xml")
    r = subprocess.run([sample, "--list", lst, "--cameras", "2", "--min-matches", "20", "--dump-problem", dump,
                        "--dump-result", res, "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    q, ts = SD.read_dump(dump)
    assert q.model == rig.PINHOLE and q.n_cams == 2 and q.D.shape[1] == 5
    # intrinsics: mcc_calibrate_camera on each camera's views in list order
    for c in range(2):
        es = [e for e in range(p.n_edges) if int(p.edge_cam[e]) == c]
        obj = np.concatenate([p.obj[p.edge_off[e]:p.edge_off[e] + p.edge_n[e]] for e in es]).astype(np.float32)
        img = np.concatenate([p.img[p.edge_off[e]:p.edge_off[e] + p.edge_n[e]] for e in es]).astype(np.float32)
        off = np.cumsum([0] + [int(p.edge_n[e]) for e in es]).astype(np.int32)
        rms, K, D, rvec, tvec, vrms, it, st = api.calibrate_camera(off, obj.astype(np.float64), img.astype(np.float64),
                                                                   p.image_size, flags=0, nd=5, max_count=30,
                                                                   eps=np.finfo(np.float64).eps)
        print("camera", c, "rms", rms, "iterations", it, "status", st, "K", K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        assert rms < 0.5   # the corner noise (0.2 px per axis)
        np.testing.assert_array_equal(q.K[c], K.astype(np.float32))
        np.testing.assert_array_equal(q.D[c], D.astype(np.float32))
    # edges: camera by camera in list order; photo vertices by first appearance of their timestamp
    want_cam, want_ts = [], []
    for c in range(2):
        for e in range(p.n_edges):
            if int(p.edge_cam[e]) == c:
                want_cam.append(c)
                want_ts.append(int(stamps[int(p.edge_photo[e])]))
    assert list(q.edge_cam) == want_cam
    assert [int(ts[v]) for v in q.edge_photo] == want_ts
    assert list(q.edge_n) == [int(p.edge_n[e]) for c in range(2) for e in range(p.n_edges) if int(p.edge_cam[e]) == c]
    got = SD.read_result(res)
    assert got["iterations"] >= 1 and np.isfinite(got["error"]) and got["error"] < 1.0
