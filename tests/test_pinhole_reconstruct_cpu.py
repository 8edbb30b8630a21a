"""Pinhole reprojectImageTo3D and stereoReconstruct (include/mcc.h) without a GPU: the numpy model
tests/npreproject.py on scenes with a known answer, and the library's host side.

  geometry   the composed model (nprectify's maps, npundistort's remap, npsgbm's matcher, npreproject) on a rendered
             pair of the `head` rig at 160 x 120, alpha 0, 32 disparities, window 5: the depth of every cloud pixel
             inside roi1, taken back to camera 1's frame, against the plane it sees.  Measured when this was written
             (the only error source is the matcher's sub-pixel interpolation, 1/16 px steps at a disparity of 12-20 px):
                 plane (Z = 800 mm)               median 5.64 mm, 95th percentile 13.76 mm
                 step (700 mm left of 40 mm, 1000 mm behind)   median 5.47 mm, 95th percentile 19.63 mm
             The bars are twice those figures.
  Q          points X of camera 1's frame through P1 and P2, the exact disparity through the model's rule in float64:
             R1 X to 1e-8 mm (the bar DESIGN.md 7i has for Q), for every rig of tests/test_pinhole_rectify.py -- four
             with the baseline along x, three along y, those through the transposed frame.
  cloud      mcc_pinrecon_host_cloud -- the function the count and the write kernel compile, run on the host -- bit-equal
             to the model's cloud on the model's own disparity, with and without roi, max_z and colours, and on a 3 x 3
             disparity by hand.
  EINVAL     every refusal of the header's list, before any device work; MCC_EHIP without a GPU.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import nprectify as N  # noqa: E402
import npreproject as R  # noqa: E402
import pinrecon_cases as C  # noqa: E402
import stereo_calib_cases as SC  # noqa: E402
from multi_camera_calibration_amd import api  # noqa: E402

MCC_EINVAL, MCC_EHIP = -1, -2
SIZE = (160, 120)
RIG_NAMES = ["head"] + [n for n in SC.RIGS if n != "forward"]
VERTICAL = ("roll90", "upside_down", "half_turn_tilted")
# twice the figures of the module docstring
DEPTH_BARS = {"plane": (C.PLANE, 2 * 5.64, 2 * 13.76), "step": (C.STEP, 2 * 5.47, 2 * 19.63)}


@pytest.fixture(scope="module")
def L():
    api.build()
    return api.lib()


def model_frame(rig_name, size=SIZE, flags=N.ZERO_DISPARITY, alpha=0.0, new_size=None):
    K1, D1, K2, D2 = C.cameras(size)
    Rm, T = C.rig(rig_name)
    geo = N.stereo_rectify(K1, D1, K2, D2, size, Rm, T, flags, alpha, new_size)
    return R.output_frame(geo, size if new_size is None else new_size)


# ------------------------------------------------------------------ the model against known geometry
@pytest.mark.parametrize("name", list(DEPTH_BARS))
def test_model_recovers_the_planes_depth(name):
    scene, bar_median, bar_p95 = DEPTH_BARS[name]
    K1, D1, K2, D2 = C.cameras(SIZE)
    frame = model_frame("head")
    out = R.compute(*C.render(scene), K1, D1, K2, D2, frame, 32, 5, R.XYZ, use_roi=True)
    mask = R.cloud_mask(out["disparity"], frame["Q"], frame["roi1"])
    assert mask.sum() == len(out["cloud"]) >= 0.6 * mask.size
    with np.errstate(invalid="ignore"):
        z = (out["points"].astype(np.float64) @ frame["R1"])[..., 2]     # R1^T p: back in camera 1's frame
    err = np.abs(z - C.true_depth(scene, frame, frame["R1"]))[mask]
    median, p95 = float(np.median(err)), float(np.percentile(err, 95))
    print(f"{name}: {int(mask.sum())} points, depth error median {median:.2f} mm, 95th percentile {p95:.2f} mm")
    assert median <= bar_median and p95 <= bar_p95


# ------------------------------------------------------------------ Q against P1, P2
@pytest.mark.parametrize("name", RIG_NAMES)
def test_q_returns_the_point(name):
    K1, D1, K2, D2 = C.cameras(SC.SIZE)
    Rm, T = C.rig(name)
    geo = N.stereo_rectify(K1, D1, K2, D2, SC.SIZE, Rm, T, N.ZERO_DISPARITY)
    frame = R.output_frame(geo, SC.SIZE)
    assert frame["transposed"] == (name in VERTICAL)
    rng = np.random.default_rng(31)
    X = np.stack([rng.uniform(-500, 500, 300), rng.uniform(-400, 400, 300), rng.uniform(500, 1200, 300)], -1)
    Xr = np.concatenate([X @ geo["R1"].astype(np.float64).T, np.ones((len(X), 1))], 1)
    p1, p2 = Xr @ frame["P1"].T, Xr @ frame["P2"].T
    p1, p2 = p1[:, :2] / p1[:, 2:], p2[:, :2] / p2[:, 2:]
    assert np.abs(p1[:, 1] - p2[:, 1]).max() <= 1e-9       # in the output frame the pair is horizontal
    got = R.reproject_points(p1[:, 0], p1[:, 1], p1[:, 0] - p2[:, 0], frame["Q"])
    err = float(np.abs(got - Xr[:, :3]).max())
    print(f"{name}: Q (x, y, d, 1) - R1 X = {err:.2e} mm")
    assert err <= 1e-8


# ------------------------------------------------------------------ the cloud rule on the host
def test_host_cloud_by_hand(L):
    # Z / W = 100 / d, X / W = (x - 1) / d * 10, Y / W = (y - 1) / d * 10
    Q = np.array([[10.0, 0, 0, -10], [0, 10.0, 0, -10], [0, 0, 0, 100.0], [0, 0, 1.0, 0]])
    d = np.array([[2.0, -1.0, 4.0],
                  [0.0, 5.0, np.inf],
                  [1.0, np.nan, 10.0]], np.float32)
    rec1 = np.arange(9, dtype=np.uint8).reshape(3, 3) * 10
    # columns first: (0, 0) (2, 0) | (1, 1) | (0, 2) (2, 2); -1, 0, inf and NaN are no points
    want = np.array([[-5, -5, 50, 0, 0, 0], [-10, 10, 100, 60, 60, 60], [0, 0, 20, 40, 40, 40],
                     [2.5, -2.5, 25, 20, 20, 20], [1, 1, 10, 80, 80, 80]], np.float32)
    got = api.pinhole_cloud_host(d, Q, rec1, api.XYZRGB)
    assert np.array_equal(got, want)
    assert np.array_equal(R.cloud(d, R.reproject(d, Q), rec1, Q, R.XYZRGB), want)
    # max_z = 50 drops the 100, the roi x in [1, 3), y in [0, 2) keeps (1, 1) and (2, 0)
    assert np.array_equal(api.pinhole_cloud_host(d, Q, None, api.XYZ, max_z=50.0), want[[0, 2, 3, 4], :3])
    assert np.array_equal(api.pinhole_cloud_host(d, Q, None, api.XYZ, roi=(1, 0, 2, 2)), want[[2, 3], :3])
    # capacity one short: the count comes back, the buffer is untouched
    cloud, n = np.full((4, 3), 7.0, np.float32), ctypes.c_longlong(0)
    rc = L.mcc_pinrecon_host_cloud(_p(d, _f32), 3, 3, _p(Q), None, 1, api.XYZ, None, 0.0, _p(cloud, _f32), 4, ctypes.byref(n))
    assert rc == MCC_EINVAL and n.value == 5 and (cloud == 7.0).all()


@pytest.mark.parametrize("cn", [1, 3])
def test_host_cloud_matches_the_model(L, cn):
    K1, D1, K2, D2 = C.cameras(SIZE)
    frame = model_frame("head", alpha=0.5)
    assert frame["roi1"] != (0, 0) + SIZE and frame["roi1"][2] > 0
    out = R.compute(*C.render(C.STEP, cn=cn), K1, D1, K2, D2, frame, 32, 5, R.XYZRGB)
    real, Q = out["disparity"], frame["Q"]
    full = api.pinhole_cloud_host(real, Q, out["rec1"], api.XYZRGB)
    assert len(full) > 5000 and np.array_equal(full, out["cloud"])
    for roi, max_z in ((frame["roi1"], 0.0), (None, 850.0), (frame["roi1"], 850.0)):
        want = R.cloud(real, out["points"], out["rec1"], Q, R.XYZ, roi, max_z)
        assert 0 < len(want) < len(full)
        assert np.array_equal(api.pinhole_cloud_host(real, Q, None, api.XYZ, roi=roi, max_z=max_z), want)


# ------------------------------------------------------------------ bad arguments, no device work
def _p(a, t=ctypes.c_double):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


_u8, _f32, _i16 = ctypes.c_ubyte, ctypes.c_float, ctypes.c_short


class Raw:
    """Valid arguments of every entry point, with one replaced at a time."""

    def __init__(self, L):
        self.L = L
        self.K1, self.D1, self.K2, self.D2 = C.cameras((40, 30))
        self.R, self.T = C.rig("head")
        self.K0 = self.K1.copy()
        self.K0[0, 0] = 0.0
        self.img = np.zeros((30, 40, 3), np.uint8)
        self.rec = np.zeros((30, 40, 3), np.uint8)
        self.real, self.d16 = np.zeros((30, 40), np.float32), np.zeros((30, 40), np.int16)
        self.points, self.cloud = np.zeros((30, 40, 3), np.float32), np.zeros((1200, 6), np.float32)
        self.Q = np.eye(4)
        self.n = ctypes.c_longlong(0)
        self.keep = None

    def desc(self, **kw):
        a = dict(K1=self.K1, D1=self.D1, K2=self.K2, D2=self.D2, nd=5, R=self.R, T=self.T, sw=40, sh=30, c=3, fl=0, alpha=-1.0,
                 nw=0, nh=0, D=16, bs=3, pt=api.XYZRGB, roi=0, max_z=0.0)
        a.update(kw)
        d = api._PinReconDesc()
        d.K1, d.D1, d.K2, d.D2, d.R, d.T = (_p(a[k]) for k in ("K1", "D1", "K2", "D2", "R", "T"))
        d.nd, d.src_width, d.src_height, d.channels, d.rectify_flags, d.alpha = a["nd"], a["sw"], a["sh"], a["c"], a["fl"], a["alpha"]
        d.new_width, d.new_height, d.num_disparities, d.sad_window_size = a["nw"], a["nh"], a["D"], a["bs"]
        d.point_type, d.use_roi, d.max_z, d.device = a["pt"], a["roi"], a["max_z"], 0
        self.keep = a
        return d

    def create(self, null_out=False, null_desc=False, **kw):
        d = self.desc(**kw)
        h = ctypes.c_void_p()
        rc = self.L.mcc_pinrecon_create(None if null_out else ctypes.byref(h), None if null_desc else ctypes.byref(d))
        assert rc != 0 and not h.value
        return rc

    def recon(self, desc_kw=None, null_desc=False, **kw):
        a = dict(i1=self.img, w=40, h=30, c=3, s1=120, i2=self.img, w2=40, h2=30, c2=3, s2=120, real=self.real, r1=self.rec,
                 rs1=120, r2=self.rec, rs2=120, cloud=self.cloud, cap=1200, n=ctypes.byref(self.n))
        a.update(kw)
        d = self.desc(**(desc_kw or {}))
        return self.L.mcc_stereo_reconstruct(
            _p(a["i1"], _u8), a["w"], a["h"], a["c"], a["s1"], _p(a["i2"], _u8), a["w2"], a["h2"], a["c2"], a["s2"],
            None if null_desc else ctypes.byref(d), None, _p(a["real"], _f32), _p(self.d16, _i16), _p(a["r1"], _u8), a["rs1"],
            _p(a["r2"], _u8), a["rs2"], _p(self.points, _f32), _p(a["cloud"], _f32), a["cap"], a["n"])

    def reproject(self, **kw):
        a = dict(d=self.real, t=api.DISP_FLOAT, w=40, h=30, s=160, Q=self.Q, out=self.points)
        a.update(kw)
        return self.L.mcc_reproject_image_to_3d(None if a["d"] is None else a["d"].ctypes.data_as(ctypes.c_void_p), a["t"],
                                                a["w"], a["h"], a["s"], _p(a["Q"]), 0, 0, _p(a["out"], _f32), None)


LEFT = -C.rig("head")[0].T @ C.rig("head")[1]     # the inverse rig's T: camera 2 to the left of camera 1
ABOVE = -C.rig("roll90")[0].T @ C.rig("roll90")[1]
BAD = {
    # reprojectImageTo3D
    "reproject null disparity": lambda r: r.reproject(d=None),
    "reproject null Q": lambda r: r.reproject(Q=None),
    "reproject null points": lambda r: r.reproject(out=None),
    "reproject type 0": lambda r: r.reproject(t=0),
    "reproject type 3": lambda r: r.reproject(t=3),
    "reproject width 0": lambda r: r.reproject(w=0),
    "reproject height < 0": lambda r: r.reproject(h=-1),
    "reproject width 32768": lambda r: r.reproject(w=32768, s=4 * 32768),
    "reproject stride short": lambda r: r.reproject(s=156),
    "reproject stride short, fixed": lambda r: r.reproject(d=r.d16, t=api.DISP_FIXED16, s=78),
    "reproject stride not a multiple of 4": lambda r: r.reproject(s=162),
    "reproject stride odd, fixed": lambda r: r.reproject(d=r.d16, t=api.DISP_FIXED16, s=81),
    # the handle: what mcc_stereo_rectify refuses
    "create null out": lambda r: r.create(null_out=True),
    "create null desc": lambda r: r.create(null_desc=True),
    "create null K1": lambda r: r.create(K1=None),
    "create null K2": lambda r: r.create(K2=None),
    "create null R": lambda r: r.create(R=None),
    "create null T": lambda r: r.create(T=None),
    "create nd 7": lambda r: r.create(nd=7),
    "create nd 14 (tilt)": lambda r: r.create(nd=14),
    "create zero fx": lambda r: r.create(K2=r.K0),
    "create src width 0": lambda r: r.create(sw=0),
    "create src height 40000": lambda r: r.create(sh=40000),
    "create new width < 0": lambda r: r.create(nw=-1, nh=5),
    "create new height 0": lambda r: r.create(nw=40, nh=0),
    "create flags 1": lambda r: r.create(fl=1),
    "create alpha 1.5": lambda r: r.create(alpha=1.5),
    "create alpha NaN": lambda r: r.create(alpha=float("nan")),
    "create T = 0": lambda r: r.create(T=np.zeros(3)),
    # the handle: what mcc_omnidir_sgbm refuses
    "create channels 0": lambda r: r.create(c=0),
    "create channels 2": lambda r: r.create(c=2),
    "create channels 4": lambda r: r.create(c=4),
    "create D 0": lambda r: r.create(D=0),
    "create D -16": lambda r: r.create(D=-16),
    "create D 24": lambda r: r.create(D=24),
    "create D 272": lambda r: r.create(D=272, nw=400, nh=30),
    "create width == D": lambda r: r.create(D=32, nw=32, nh=30),
    "create width < D": lambda r: r.create(D=48),
    "create window even": lambda r: r.create(bs=4),
    "create window 0": lambda r: r.create(bs=0),
    "create window -3": lambda r: r.create(bs=-3),
    "create 93 cn bs^2 > 32767": lambda r: r.create(bs=11),
    "create 93 bs^2 > 32767, 1 channel": lambda r: r.create(c=1, bs=19),
    "create cost volume over the budget": lambda r: r.create(c=1, nw=30000, nh=200, D=256),
    "create vertical pair: the matched width is the new height": lambda r: r.create(R=C.rig("roll90")[0], T=C.rig("roll90")[1],
                                                                                     nw=40, nh=16),
    # the handle's own
    "create point type 0": lambda r: r.create(pt=0),
    "create point type 3": lambda r: r.create(pt=3),
    "create camera 2 on the left": lambda r: r.create(R=C.rig("head")[0].T.copy(), T=LEFT),
    "create camera 2 above": lambda r: r.create(R=C.rig("roll90")[0].T.copy(), T=ABOVE),
    "info null handle": lambda r: r.L.mcc_pinrecon_info(None, ctypes.byref(api._PinReconGeometry())),
    "compute null handle": lambda r: r.L.mcc_pinrecon_compute(None, _p(r.img, _u8), 120, _p(r.img, _u8), 120, _p(r.real, _f32),
                                                              None, _p(r.rec, _u8), 120, _p(r.rec, _u8), 120, None,
                                                              _p(r.cloud, _f32), 1200, ctypes.byref(r.n)),
    "time null handle": lambda r: r.L.mcc_pinrecon_time(None, 3, ctypes.byref(ctypes.c_double())),
    # the one-call form
    "recon null desc": lambda r: r.recon(null_desc=True),
    "recon null image1": lambda r: r.recon(i1=None),
    "recon null image2": lambda r: r.recon(i2=None),
    "recon null disparity": lambda r: r.recon(real=None),
    "recon null rec1": lambda r: r.recon(r1=None),
    "recon null rec2": lambda r: r.recon(r2=None),
    "recon null count": lambda r: r.recon(n=None),
    "recon null cloud with a capacity": lambda r: r.recon(cloud=None),
    "recon capacity < 0": lambda r: r.recon(cap=-1),
    "recon channels differ": lambda r: r.recon(c2=1),
    "recon widths differ": lambda r: r.recon(w2=38),
    "recon heights differ": lambda r: r.recon(h2=29),
    "recon size differs from the descriptor's": lambda r: r.recon(desc_kw=dict(sw=48)),
    "recon channels differ from the descriptor's": lambda r: r.recon(desc_kw=dict(c=1)),
    "recon image1 stride short": lambda r: r.recon(s1=119),
    "recon image2 stride short": lambda r: r.recon(s2=100),
    "recon rec1 stride short": lambda r: r.recon(rs1=119),
    "recon rec2 stride short for the new size": lambda r: r.recon(desc_kw=dict(nw=48, nh=30)),
    "recon D 20": lambda r: r.recon(desc_kw=dict(D=20)),
    "recon nd 14 (tilt)": lambda r: r.recon(desc_kw=dict(nd=14)),
    "recon point type 7": lambda r: r.recon(desc_kw=dict(pt=7)),
    "recon camera 2 on the left": lambda r: r.recon(desc_kw=dict(R=C.rig("head")[0].T.copy(), T=LEFT)),
}


@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_refused_before_device_work(L, case):
    """MCC_EINVAL (never MCC_EHIP, which a machine without a GPU gives the first device call)"""
    assert BAD[case](Raw(L)) == MCC_EINVAL, case
    assert L.mcc_last_error()


def test_camera_order_message_says_to_swap(L):
    assert Raw(L).create(R=C.rig("head")[0].T.copy(), T=LEFT) == MCC_EINVAL
    assert b"swap the cameras" in L.mcc_last_error()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_no_gpu_fails_loudly(L):
    r = Raw(L)
    assert r.create() == MCC_EHIP
    assert r.create(R=C.rig("roll90")[0], T=C.rig("roll90")[1]) == MCC_EHIP   # a vertical pair passes every host check
    assert r.recon() == MCC_EHIP
    assert r.reproject() == MCC_EHIP
    with pytest.raises(api.MccError) as ei:
        api.PinholeReconstructor(r.K1, r.D1, r.K2, r.D2, r.R, r.T, 16, 3, (40, 30))
    assert "(-2)" in str(ei.value)
