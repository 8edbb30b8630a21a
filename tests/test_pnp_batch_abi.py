"""mcc_solve_pnp_batch at the C-ABI boundary, without a GPU (include/mcc.h).

* every invalid descriptor the header lists returns MCC_EINVAL with a message.  The checks run before
  any device call: on a host without a GPU they still answer MCC_EINVAL, not MCC_EHIP;
* a valid call on a host without a GPU fails loudly with MCC_EHIP (no CPU fallback);
* the Python mirror raises MccError with the same code.
(tests/test_abi.py and tests/test_code_object.py cover the export list and the kernel's resources.)"""
import ctypes
import os

import numpy as np
import pytest

from multi_camera_calibration_amd import api

MCC_EINVAL, MCC_EHIP = -1, -2
_f64p, _i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def L():
    api.build()
    return api.lib()


class _Call:
    """A valid two-view call (4 and 6 corners, two cameras, nd = 5) whose pieces a test replaces."""

    def __init__(self):
        self.off = np.array([0, 4, 10], np.int32)
        g = np.arange(10, dtype=np.float64)
        self.obj = np.stack([40 * (g % 3), 40 * (g // 3), 10 * np.sin(g)], 1)
        self.img = np.stack([900 + 30 * (g % 3), 500 + 30 * (g // 3)], 1)
        self.cam = np.array([0, 1], np.int32)
        self.K = np.tile(np.array([1200.0, 0, 960, 0, 1180, 540, 0, 0, 1]), 2)
        self.D = np.zeros(10)
        self.nd, self.n_views, self.n_cams, self.max_iter = 5, 2, 2, 50
        self.rvec, self.tvec = np.zeros(6), np.zeros(6)
        self.rms, self.status = np.zeros(2), np.zeros(2, np.int32)
        self.null = set()

    def _p(self, name, t):
        a = getattr(self, name)
        return None if name in self.null or a is None else a.ctypes.data_as(t)

    def run(self, L, desc=True):
        d = api._PnpDesc(self.n_views, self._p("off", _i32p), self._p("obj", _f64p), self._p("img", _f64p),
                         self._p("cam", _i32p), self.n_cams, self._p("K", _f64p), self._p("D", _f64p), self.nd,
                         self.max_iter, 0)
        return L.mcc_solve_pnp_batch(ctypes.byref(d) if desc else None, self._p("rvec", _f64p), self._p("tvec", _f64p),
                                     self._p("rms", _f64p), self._p("status", _i32p), None)


def _bad_null_desc(c):
    return dict(desc=False)


def _bad(name):
    def f(c):
        c.null.add(name)
    return f


def _set(**kw):
    def f(c):
        for k, v in kw.items():
            setattr(c, k, v)
    return f


BAD = {
    "null_desc": _bad_null_desc,
    "null_rvec": _bad("rvec"), "null_tvec": _bad("tvec"), "null_rms": _bad("rms"), "null_status": _bad("status"),
    "null_view_off": _bad("off"), "null_obj": _bad("obj"), "null_img": _bad("img"), "null_K": _bad("K"),
    "null_D_with_nd": _bad("D"),
    "no_views": _set(n_views=0), "negative_views": _set(n_views=-3),
    "view_off_decreases": _set(off=np.array([0, 6, 4], np.int32)),
    "nd_6": _set(nd=6), "nd_14": _set(nd=14), "nd_negative": _set(nd=-1),
    "view_cam_high": _set(cam=np.array([0, 2], np.int32)), "view_cam_negative": _set(cam=np.array([-1, 0], np.int32)),
    "too_many_corners": _set(off=np.array([0, 4, 4 + 1025], np.int32)),
}


@pytest.mark.parametrize("bad", sorted(BAD))
def test_invalid_descriptor_is_einval_with_a_message(L, bad):
    c = _Call()
    kw = BAD[bad](c) or {}
    assert c.run(L, **kw) == MCC_EINVAL
    msg = L.mcc_last_error().decode()
    assert "solve_pnp_batch" in msg and len(msg) > 20, msg


def test_python_mirror_raises_einval():
    g = np.arange(6, dtype=np.float64)
    obj, img = np.stack([g, g * g, g], 1), np.stack([g, g], 1)
    K = np.array([[1200.0, 0, 960], [0, 1180, 540], [0, 0, 1]])
    with pytest.raises(api.MccError) as ei:
        api.solve_pnp(obj, img, [0, 6], K, np.zeros(6))           # nd = 6
    assert "(-1)" in str(ei.value) and "nd" in str(ei.value)
    with pytest.raises(api.MccError) as ei:
        api.solve_pnp(obj, img, [0, 6], K, None, view_cam=[1])    # one camera, view_cam = 1
    assert "(-1)" in str(ei.value) and "view_cam" in str(ei.value)
    with pytest.raises(api.MccError) as ei:
        api.solve_pnp(obj, img, [0], K, None)                     # no views
    assert "(-1)" in str(ei.value)


# (no torch here: its bundled HIP runtime shares SONAMEs with /opt/rocm's and would shadow it)
@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_no_gpu_fails_loudly(L):
    assert _Call().run(L) == MCC_EHIP
    assert L.mcc_last_error()
    g = np.arange(6, dtype=np.float64)
    with pytest.raises(api.MccError) as ei:
        api.solve_pnp(np.stack([g, g * g, g], 1), np.stack([g, g], 1), [0, 6],
                      np.array([[1200.0, 0, 960], [0, 1180, 540], [0, 0, 1]]), None)
    assert "(-2)" in str(ei.value)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_loader_with_gpu_pnp_fails_loudly_without_a_gpu(tmp_path):
    """--gpu-pnp never falls back to the host solver: without a GPU the sample stops with the library's
    MCC_EHIP message, while the default loader still loads the same data."""
    import subprocess

    import sample_data as SD
    from multi_camera_calibration_amd import rig

    api.build()
    p = rig.make_rig(n_cams=2, n_views=6, seed=3)
    serials, data, config, _, _ = SD.write_dataset(p, str(tmp_path))
    args = [api.SAMPLE_PATH, "--serials", ",".join(serials), "--data", data, "--config", config, "--init-only"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "loaded:" in r.stdout, r.stdout + r.stderr
    r = subprocess.run(args + ["--gpu-pnp"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "mcc_solve_pnp_batch failed (-2)" in r.stderr, r.stdout + r.stderr
