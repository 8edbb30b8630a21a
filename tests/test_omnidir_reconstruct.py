"""cv::omnidir::stereoReconstruct (src/omnidir.cpp:1383-1539) on the GPU: the semi-global matcher
(mcc_omnidir_sgbm), the reconstruction built on it (mcc_omnidir_stereo_reconstruct) and the resident
handle (mcc_omnirecon_*), against the numpy model tests/npsgbm.py, the executable form of DESIGN.md 7e.

CPU: the model on scenes with a known answer, its rules on hand-made inputs, every bad argument refused
with MCC_EINVAL before any device work, MCC_EHIP without a GPU.

GPU (bars, all set before any run):
  matcher      integer arithmetic: bit-equal to the model, no tolerance.
  rectified    bit-equal to api.omnidir_undistort_image with R1 / R2.
  disparity    bit-equal to the model's matcher and tail applied to the DEVICE's own rectified images (so
               a one-unit map difference cannot leak into it).
  cloud        count and column-major order equal to the model's; perspective coordinates within 2 float32
               ulp (everything is exact float32 arithmetic but Knew^-1, whose double entries may differ in
               the last bit between two inverses); longlati coordinates within 16 * 2^-24 * depth absolute
               (five float32 roundings plus two sinf / cosf of at most 2 ulp each, |trig| <= 1); colours equal.
  geometry     the median z of the points on the plane within 5 % of its true depth; the same bar is
               asserted on the model's own output on the CPU first.

The two-level scene uses seed 2: the band of columns that is invalid in every row is 65-72 or 65-73
depending on the texture (seeds 0-3 tried on the model); the bar names 65-73, so a texture that gives
it was chosen, the bar was not moved.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import npsgbm as M  # noqa: E402
import npundistort as U  # noqa: E402
from multi_camera_calibration_amd import api  # noqa: E402
from ulp import f32_ulp_diff  # noqa: E402

MCC_EINVAL, MCC_EHIP = -1, -2
PERSPECTIVE, LONGLATI = M.RECTIFY_PERSPECTIVE, M.RECTIFY_LONGLATI
FLAG_NAME = {PERSPECTIVE: "perspective", LONGLATI: "longlati"}


@pytest.fixture(scope="module")
def L():
    api.build()
    return api.lib()


def within_one(disp, D, truth):
    """(share of the pixels x >= D within 1 px of truth, share valid, share of the valid within 1 px)"""
    d = disp[:, D:]
    valid = d >= 0
    ok = np.abs(d / 16.0 - truth[None, D:]) <= 1
    return ok.mean(), valid.mean(), (ok & valid).sum() / max(valid.sum(), 1)


# ------------------------------------------------------------------ CPU: the model on scenes with a known answer
def test_model_identical_images_give_zero():
    for cn, bs in ((1, 5), (3, 3)):
        img = M.texture(np.random.default_rng(5 + cn), 9, 60, cn)
        assert (M.sgbm(img, img, 16, bs)[:, 16:] == 0).all()
        assert (M.sgbm(img, img, 16, bs)[:, :16] == M.INVALID).all()


@pytest.mark.parametrize("cn,bs", [(1, 5), (3, 3)])
def test_model_constant_shift(cn, bs):
    H, W, D = 40, 112, 32
    left, right = M.shifted_pair(np.random.default_rng(0), H, W, 9, cn)
    disp = M.sgbm(left, right, D, bs)
    share, valid, _ = within_one(disp, D, np.full(W, 9.0))
    print(f"constant shift cn={cn} bs={bs}: {share:.4f} within 1 px, {valid:.4f} valid")
    assert share >= 0.98


@functools.lru_cache(maxsize=None)
def two_level(H=40, W=112, split=70, cn=1):
    left, right = M.two_level_pair(np.random.default_rng(2), H, W, 6, 17, split, cn)
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


def test_model_two_level_scene():
    H, W, D = 40, 112, 32
    left, right = two_level()
    disp = M.sgbm(left, right, D, 5)
    _, valid, share = within_one(disp, D, np.where(np.arange(W) < 70, 6.0, 17.0))
    print(f"two levels: {valid:.4f} valid, {share:.4f} of them within 1 px")
    assert share >= 0.95
    assert valid >= 0.80
    assert (disp[:, 65:74] == M.INVALID).all()     # the occluded band, columns 65-73


# ------------------------------------------------------------------ CPU: the rules on hand-made inputs
def test_model_signal_row_by_hand():
    p = np.array([[10, 20, 40, 40, 0]], np.int64)   # one row: the rows above and below are the row itself
    g, raw = M.signals(p)
    # 4 (p[x + 1] - p[x - 1]) clamped to +-15, plus 15; 15 in both border columns
    assert g.tolist() == [[15, 30, 30, 0, 15]]
    assert raw.tolist() == [[15, 20, 40, 40, 15]]
    lo, hi = M.lo_hi(raw)
    # halves: (15+20)/2 = 17, (20+40)/2 = 30, (40+40)/2 = 40, (40+15)/2 = 27
    assert lo.tolist() == [[15, 17, 30, 27, 15]]
    assert hi.tolist() == [[17, 30, 40, 40, 27]]


def test_model_bt_cost_by_hand():
    # c0 = max(0, 50 - 30, 18 - 50) = 20, c1 = max(0, 20 - 55, 45 - 20) = 25
    assert int(M.bt_cost(np.int64(50), np.int64(20), 45, 55, 18, 30)) == 20
    assert int(M.bt_cost(np.int64(25), np.int64(20), 45, 55, 18, 30)) == 0    # u inside [loR, hiR]


def test_model_path_step_by_hand():
    Lq, C = np.array([10, 3, 20, 50]), np.array([5, 5, 5, 5])
    # m = 3, m + P2 = 35; candidates (Lq[d], Lq[d-1] + 8, Lq[d+1] + 8, 35) with 32767 outside:
    # d0: min(10, 32775, 11, 35) = 10; d1: min(3, 18, 28, 35) = 3; d2: min(20, 11, 58, 35) = 11; d3: min(50, 28, 32775, 35) = 28
    assert M.path_step(C, Lq, 8, 32).tolist() == [5 + 10 - 35, 5 + 3 - 35, 5 + 11 - 35, 5 + 28 - 35]
    # a previous pixel outside the image: C - P2, which is what an all-zero Lr(q) gives
    assert M.path(C.reshape(1, 1, 4), 0, -1, 8, 32).ravel().tolist() == [5 - 32] * 4
    assert M.path_step(C, np.zeros(4, np.int64), 8, 32).tolist() == [5 - 32] * 4


def test_model_winner_and_subpixel_by_hand():
    S = np.array([[10, 4, 4, 9],      # two minima: the smaller d; den = 10 + 4 - 8 = 6, (6 * 16 + 6) // 12 = 8
                  [5, 4, 9, 9],       # den = 6, (-4 * 16 + 6) // 12 = -58 // 12 = -5 (a floor; truncation gives -4)
                  [1, 4, 9, 9],       # d* = 0: no interpolation
                  [9, 9, 4, 1],       # d* = D - 1: none either
                  [7, 3, 7, 9]])      # symmetric: den = 8, (0 + 8) // 16 = 0
    disp, ds, mn = M.winner_row(S)
    assert ds.tolist() == [1, 1, 0, 3, 1] and mn.tolist() == [4, 4, 1, 1, 3]
    assert disp.tolist() == [16 + 8, 16 - 5, 0, 48, 16]


def test_model_disp2_tie_and_check_by_hand():
    D, W = 2, 6
    ds, mn = np.array([0, 1, 0, 1]), np.array([5, 5, 7, 5])      # the left pixels x = 2 .. 5
    # x = 2 and x = 3 both land on column 2 with min S 5: the larger x wins; x = 5 beats x = 4 on column 4
    disp2 = M.disp2_row(ds, mn, D, W)
    assert disp2.tolist() == [-1, -1, 1, -1, 1, -1]
    # the check: x = 5 claims 3 px (d1 = 48): column 2 holds 1, |1 - 3| > 1 for floor and ceiling -> invalid;
    # x = 4 claims 2.5 px: the floor 2 lands on column 2 (|1 - 2| = 1, fine) -> kept; x = 3 lands on column 3,
    # which no left pixel maps to -> kept
    disp = np.array([M.INVALID, M.INVALID, 0, 0, 40, 48])
    assert M.lr_check_row(disp, disp2, D).tolist() == [M.INVALID, M.INVALID, 0, 0, 40, M.INVALID]


def test_model_saturation_case_saturates():
    left, right = saturating_pair()
    stats = {}
    sat = M.sgbm(left, right, 16, 9, stats=stats)
    print(f"saturation case: max of the four-direction sum {stats['max_four']}, of all five {stats['max_five']}")
    assert stats["max_four"] > 32767                                   # the first clamp acts
    assert not np.array_equal(sat, M.sgbm(left, right, 16, 9, saturate=False))   # and it shows in the output


def test_model_geometry_of_the_rendered_plane():
    R1, R2 = U.stereo_rectify(M.RIG_OM, M.RIG_T)
    for flag in (PERSPECTIVE, LONGLATI):
        a, b = rendered(1)
        rec1, rec2 = M.model_rectify(a, 0, R1, flag), M.model_rectify(b, 1, R2, flag)
        real = M.real_disparity(M.sgbm(rec1, rec2, 32, 5), rec1)
        cloud, _ = M.point_cloud(real, rec1, M.rig_knew(flag), M.RIG_T, flag, M.XYZ, M.RIG_SIZE)
        check_geometry(real, cloud, flag, R1)


# ------------------------------------------------------------------ shared scenes
@functools.lru_cache(maxsize=None)
def saturating_pair():
    """black and white bars of period 4 in 3 channels at a 9 x 9 window, seen at 4 px.  At d = 2 (mod 4)
    every pixel mismatches: the raw cost is 127 >> 2 = 31 and the gradient cost 15 per channel, so
    C = 46 * 3 * 81 = 11178, while d = 0 (mod 4) costs nothing.  A path then keeps Lr = C at d = 2, and four
    directions give 44712 > 32767.  A tenth of the pixels is flipped so that the winners' neighbours differ."""
    rng = np.random.default_rng(21)
    wide = np.broadcast_to(((np.arange(44) // 2) % 2 * 255).astype(np.uint8)[None, :, None], (12, 44, 3)).copy()
    flip = rng.random(wide.shape) < 0.1
    wide[flip] = 255 - wide[flip]
    left, right = np.ascontiguousarray(wide[:, :40]), np.ascontiguousarray(wide[:, 4:44])
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=None)
def rendered(cn):
    a, b = M.render_plane_pair(11, cn)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def check_geometry(real, cloud, flag, R1):
    on = M.plane_pixels(flag, R1)
    ii, jj = np.nonzero(real.T > 15)
    sel = on[jj, ii]
    z = float(np.median(cloud[sel, 2]))
    print(f"{FLAG_NAME[flag]}: {len(cloud)} points, {int(sel.sum())} of the plane's {int(on.sum())} pixels, median z {z:.4f}")
    assert sel.sum() >= 0.8 * on.sum()
    assert abs(z - M.PLANE_Z) <= 0.05 * M.PLANE_Z


# ------------------------------------------------------------------ CPU: the C ABI without a device
def _p(a, t=ctypes.c_double):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(t))


_u8, _f32, _i16 = ctypes.c_ubyte, ctypes.c_float, ctypes.c_short


class Raw:
    """Valid arguments of every entry point, with one replaced at a time."""

    def __init__(self, L):
        self.L = L
        self.img = np.zeros((6, 40, 3), np.uint8)
        self.disp16 = np.zeros((6, 40), np.int16)
        self.K, self.D, self.R, self.T = M.RIG_K[0].copy(), M.RIG_D[0].copy(), U.rotation(M.RIG_OM), M.RIG_T.copy()
        self.sing = np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]])
        self.real = np.zeros((6, 40), np.float32)
        self.rec = np.zeros((6, 40, 3), np.uint8)
        self.cloud = np.zeros((240, 6), np.float32)
        self.n = ctypes.c_longlong(0)

    def sgbm(self, **kw):
        a = dict(l=self.img, w=40, h=6, c=3, ls=120, r=self.img, w2=40, h2=6, c2=3, rs=120, D=16, bs=3, out=self.disp16)
        a.update(kw)
        return self.L.mcc_omnidir_sgbm(_p(a["l"], _u8), a["w"], a["h"], a["c"], a["ls"], _p(a["r"], _u8), a["w2"], a["h2"],
                                       a["c2"], a["rs"], a["D"], a["bs"], 0, _p(a["out"], _i16))

    def recon(self, **kw):
        a = dict(i1=self.img, w=40, h=6, c=3, s1=120, i2=self.img, w2=40, h2=6, c2=3, s2=120, K1=self.K, K2=self.K,
                 R=self.R, T=self.T, fl=PERSPECTIVE, D=16, bs=3, nw=40, nh=6, Kn=None, pt=M.XYZRGB, real=self.real,
                 r1=self.rec, rs1=120, r2=self.rec, rs2=120, cloud=self.cloud, cap=240, n=ctypes.byref(self.n))
        a.update(kw)
        return self.L.mcc_omnidir_stereo_reconstruct(
            _p(a["i1"], _u8), a["w"], a["h"], a["c"], a["s1"], _p(a["i2"], _u8), a["w2"], a["h2"], a["c2"], a["s2"],
            _p(a["K1"]), _p(self.D), 1.6, _p(a["K2"]), _p(self.D), 1.55, _p(a["R"]), _p(a["T"]), a["fl"], a["D"], a["bs"],
            a["nw"], a["nh"], _p(a["Kn"]), a["pt"], 0, _p(a["real"], _f32), _p(a["r1"], _u8), a["rs1"], _p(a["r2"], _u8),
            a["rs2"], _p(a["cloud"], _f32), a["cap"], a["n"])

    def create(self, null_out=False, null_desc=False, **kw):
        a = dict(K1=self.K, K2=self.K, R=self.R, T=self.T, fl=PERSPECTIVE, D=16, bs=3, sw=40, sh=6, c=3, nw=40, nh=6,
                 Kn=None, pt=M.XYZ)
        a.update(kw)
        d = api._OmniReconDesc()
        d.K1, d.D1, d.K2, d.D2, d.R, d.T, d.Knew = _p(a["K1"]), _p(self.D), _p(a["K2"]), _p(self.D), _p(a["R"]), _p(a["T"]), _p(a["Kn"])
        d.xi1, d.xi2, d.flag, d.device = 1.6, 1.55, a["fl"], 0
        d.num_disparities, d.sad_window_size, d.src_width, d.src_height = a["D"], a["bs"], a["sw"], a["sh"]
        d.channels, d.new_width, d.new_height, d.point_type = a["c"], a["nw"], a["nh"], a["pt"]
        h = ctypes.c_void_p()
        rc = self.L.mcc_omnirecon_create(None if null_out else ctypes.byref(h), None if null_desc else ctypes.byref(d))
        assert rc != 0 and not h.value
        return rc


BAD = {
    # the matcher
    "sgbm null left": lambda r: r.sgbm(l=None),
    "sgbm null right": lambda r: r.sgbm(r=None),
    "sgbm null disparity": lambda r: r.sgbm(out=None),
    "sgbm channels 2": lambda r: r.sgbm(c=2, c2=2),
    "sgbm channels 4": lambda r: r.sgbm(c=4, c2=4, ls=160, rs=160),
    "sgbm channels differ": lambda r: r.sgbm(c2=1),
    "sgbm widths differ": lambda r: r.sgbm(w2=39),
    "sgbm heights differ": lambda r: r.sgbm(h2=5),
    "sgbm left stride short": lambda r: r.sgbm(ls=119),
    "sgbm right stride short": lambda r: r.sgbm(rs=100),
    "sgbm D 0": lambda r: r.sgbm(D=0),
    "sgbm D -16": lambda r: r.sgbm(D=-16),
    "sgbm D 24": lambda r: r.sgbm(D=24),
    "sgbm D 272": lambda r: r.sgbm(D=272, w=300, w2=300, ls=900, rs=900),
    "sgbm width == D": lambda r: r.sgbm(D=32, w=32, w2=32),
    "sgbm width < D": lambda r: r.sgbm(D=48),
    "sgbm window even": lambda r: r.sgbm(bs=4),
    "sgbm window 0": lambda r: r.sgbm(bs=0),
    "sgbm window -3": lambda r: r.sgbm(bs=-3),
    "sgbm 93 cn bs^2 > 32767": lambda r: r.sgbm(bs=11),                       # 93 * 3 * 121 = 33759
    "sgbm 93 bs^2 > 32767, 1 channel": lambda r: r.sgbm(c=1, c2=1, bs=19),    # 93 * 361 = 33573
    "sgbm width > 65535": lambda r: r.sgbm(w=65536, w2=65536, c=1, c2=1, ls=65536, rs=65536),
    "sgbm cost volume over the budget": lambda r: r.sgbm(w=30000, w2=30000, h=200, h2=200, c=1, c2=1, ls=30000,
                                                         rs=30000, D=256),   # 2 * 200 * 29744 * 256 = 3.0e9
    # the one-shot reconstruction
    "recon null image1": lambda r: r.recon(i1=None),
    "recon null image2": lambda r: r.recon(i2=None),
    "recon null K1": lambda r: r.recon(K1=None),
    "recon null K2": lambda r: r.recon(K2=None),
    "recon null R": lambda r: r.recon(R=None),
    "recon null T": lambda r: r.recon(T=None),
    "recon null disparity": lambda r: r.recon(real=None),
    "recon null rec1": lambda r: r.recon(r1=None),
    "recon null rec2": lambda r: r.recon(r2=None),
    "recon null count": lambda r: r.recon(n=None),
    "recon null cloud with a capacity": lambda r: r.recon(cloud=None),
    "recon channels 2": lambda r: r.recon(c=2, c2=2),
    "recon channels differ": lambda r: r.recon(c2=1),
    "recon sizes differ": lambda r: r.recon(w2=38),
    "recon flag cylindrical": lambda r: r.recon(fl=2),
    "recon flag stereographic": lambda r: r.recon(fl=4),
    "recon flag 0": lambda r: r.recon(fl=0),
    "recon D 0": lambda r: r.recon(D=0),
    "recon D 20": lambda r: r.recon(D=20),
    "recon D 512": lambda r: r.recon(D=512),
    "recon new width <= D": lambda r: r.recon(nw=16, rs1=48, rs2=48),
    "recon source width <= D, empty newSize": lambda r: r.recon(nw=0, nh=0, D=48),
    "recon window even": lambda r: r.recon(bs=2),
    "recon window too large": lambda r: r.recon(bs=11),
    "recon point type 0": lambda r: r.recon(pt=0),
    "recon point type 3": lambda r: r.recon(pt=3),
    "recon T zero": lambda r: r.recon(T=np.zeros(3)),
    "recon baseline along z": lambda r: r.recon(R=np.eye(3), T=np.array([0.0, 0.0, 0.7])),
    "recon singular Knew": lambda r: r.recon(Kn=r.sing),
    "recon rec1 stride short": lambda r: r.recon(rs1=119),
    # the handle
    "create null out": lambda r: r.create(null_out=True),
    "create null desc": lambda r: r.create(null_desc=True),
    "create null K1": lambda r: r.create(K1=None),
    "create channels 0": lambda r: r.create(c=0),
    "create flag 2": lambda r: r.create(fl=2),
    "create D 8": lambda r: r.create(D=8),
    "create window 4": lambda r: r.create(bs=4),
    "create point type 7": lambda r: r.create(pt=7),
    "create T zero": lambda r: r.create(T=np.zeros(3)),
    "create new height < 0": lambda r: r.create(nh=-2),
    "compute null handle": lambda r: r.L.mcc_omnirecon_compute(None, _p(r.img, _u8), 120, _p(r.img, _u8), 120,
                                                               _p(r.real, _f32), _p(r.rec, _u8), 120, _p(r.rec, _u8), 120,
                                                               _p(r.cloud, _f32), 240, ctypes.byref(r.n)),
    "time null handle": lambda r: r.L.mcc_omnirecon_time(None, 3, ctypes.byref(ctypes.c_double())),
}


@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_refused_before_device_work(L, case):
    """MCC_EINVAL (never MCC_EHIP, which a machine without a GPU gives the first device call)"""
    assert BAD[case](Raw(L)) == MCC_EINVAL, case
    assert L.mcc_last_error()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_no_gpu_fails_loudly(L):
    r = Raw(L)
    assert r.sgbm() == MCC_EHIP
    assert r.recon() == MCC_EHIP
    assert r.create() == MCC_EHIP
    with pytest.raises(api.MccError) as ei:
        api.OmniReconstructor(r.K, r.D, 1.6, r.K, r.D, 1.55, r.R, r.T, PERSPECTIVE, 16, 3, (40, 6))
    assert "(-2)" in str(ei.value)


# ------------------------------------------------------------------ GPU: the matcher, bit-equal
def padded(img, pad):
    """the same pixels with rows pad bytes apart beyond the row"""
    if not pad:
        return img
    h, w = img.shape[:2]
    c = 1 if img.ndim == 2 else img.shape[2]
    buf = np.full((h, w * c + pad), 0xAB, np.uint8)
    buf[:, :w * c] = img.reshape(h, w * c)
    shape, strides = ((h, w), (w * c + pad, 1)) if c == 1 else ((h, w, c), (w * c + pad, c, 1))
    return np.ndarray(shape, np.uint8, buffer=buf, strides=strides)


def scene(kind, H, W, D, cn, seed):
    rng = np.random.default_rng(seed)
    if kind == "shift":
        return M.shifted_pair(rng, H, W, min(9, D - 2), cn)
    if kind == "two":
        return M.two_level_pair(rng, H, W, 6, min(17, D - 2), D + (W - D) // 2, cn)
    if kind == "zeros":      # every cost ties: the smallest d, and the larger x in disp2
        z = np.zeros((H, W) if cn == 1 else (H, W, cn), np.uint8)
        return z, z.copy()
    return M.texture(rng, H, W, cn), M.texture(rng, H, W, cn)   # noise: nothing matches


# (D, H, W, bs, cn, pad, kind): D 16 / 32 put 4 / 2 paths in a wave, 48 and 64 one (48 with idle lanes), 80 a
# partial second value per lane, 128 / 192 / 256 two to four; H x W: one pixel column, two rows, odd, many blocks
SGBM_CASES = [
    (16, 1, 17, 1, 1, 0, "noise"), (16, 2, 18, 3, 3, 5, "zeros"), (16, 37, 39, 5, 1, 0, "shift"),
    (32, 37, 55, 5, 3, 0, "two"), (48, 37, 71, 3, 1, 0, "shift"),
    (64, 1, 65, 5, 3, 0, "noise"), (64, 2, 66, 1, 1, 0, "shift"), (64, 37, 87, 3, 1, 3, "two"), (64, 48, 400, 5, 1, 0, "two"),
    (80, 1, 81, 3, 1, 0, "zeros"), (80, 2, 82, 5, 1, 0, "shift"), (80, 37, 103, 3, 3, 0, "noise"), (80, 37, 103, 1, 1, 7, "zeros"),
    (128, 37, 151, 5, 1, 0, "noise"), (192, 37, 215, 3, 1, 0, "shift"),
    (256, 1, 257, 3, 1, 0, "zeros"), (256, 2, 258, 1, 3, 0, "noise"), (256, 37, 279, 5, 1, 0, "shift"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SGBM_CASES, ids=lambda c: "D{}-{}x{}-bs{}-cn{}-pad{}-{}".format(*c))
def test_sgbm_bit_equal(L, case):
    D, H, W, bs, cn, pad, kind = case
    left, right = scene(kind, H, W, D, cn, 1000 + D + H + bs)
    want = M.sgbm(left, right, D, bs)
    got = api.omnidir_sgbm(padded(left, pad), padded(right, pad), D, bs)
    assert got.shape == (H, W) and got.dtype == np.int16
    differ = int((got != want).sum())
    print(f"sgbm {case}: {differ} of {H * W} pixels differ, {int((want[:, D:] < 0).sum())} invalid")
    assert differ == 0


@pytest.mark.gpu
def test_sgbm_saturation_bit_equal(L):
    """S saturates (test_model_saturation_case_saturates shows that it does, and that it changes the output)"""
    left, right = saturating_pair()
    assert np.array_equal(api.omnidir_sgbm(left, right, 16, 9), M.sgbm(left, right, 16, 9))


# ------------------------------------------------------------------ GPU: stereoReconstruct
def model_tail(rec1, rec2, D, bs, flag, point_type, new_size):
    real = M.real_disparity(M.sgbm(rec1, rec2, D, bs), rec1)
    cloud, depth = M.point_cloud(real, rec1, M.rig_knew(flag), M.RIG_T, flag, point_type, new_size)
    return real, cloud, depth


def reconstruct(cn, flag, point_type, new_size=M.RIG_SIZE, **kw):
    a, b = rendered(cn)
    return api.omnidir_stereo_reconstruct(a, b, M.RIG_K[0], M.RIG_D[0], M.RIG_XI[0], M.RIG_K[1], M.RIG_D[1], M.RIG_XI[1],
                                          M.RIG_OM, M.RIG_T, flag, 32, 5, new_size=new_size, Knew=M.rig_knew(flag),
                                          point_type=point_type, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("flag", [PERSPECTIVE, LONGLATI], ids=["perspective", "longlati"])
def test_stereo_reconstruct(L, flag, cn):
    a, b = rendered(cn)
    R1, R2 = api.omnidir_stereo_rectify(M.RIG_OM, M.RIG_T)
    Kn = M.rig_knew(flag)
    # both point types with both flags and both channel counts over the four cases
    point_type = M.XYZRGB if (flag == PERSPECTIVE) == (cn == 1) else M.XYZ
    real, rec1, rec2, cloud = reconstruct(cn, flag, point_type)
    # rectified images: undistortImage with R1 / R2
    for img, c, R, rec in ((a, 0, R1, rec1), (b, 1, R2, rec2)):
        want = api.omnidir_undistort_image(img, M.RIG_K[c], M.RIG_D[c], M.RIG_XI[c], flag, Knew=Kn, new_size=M.RIG_SIZE, R=R)
        assert np.array_equal(rec, want)
    assert (M.gray_of(rec1) > 0).sum() > 2000 and (M.gray_of(rec1) == 0).sum() > 2000   # the plane and the black around it
    # disparity and cloud: the model's tail on the device's own rectified images
    wreal, wcloud, depth = model_tail(rec1, rec2, 32, 5, flag, point_type, M.RIG_SIZE)
    assert real.dtype == np.float32 and np.array_equal(real, wreal)
    assert (real == 0).any() and (real == -1).any() and (real > 15).any()
    assert cloud.shape == wcloud.shape and len(cloud) > 1000
    if flag == PERSPECTIVE:
        ulp = f32_ulp_diff(cloud[:, :3], wcloud[:, :3])
        print(f"perspective cn={cn}: {len(cloud)} points, max {int(ulp.max())} ulp")
        assert ulp.max() <= 2
    else:
        err = np.abs(cloud[:, :3].astype(np.float64) - wcloud[:, :3]) / depth[:, None].astype(np.float64)
        print(f"longlati cn={cn}: {len(cloud)} points, max error {err.max() * 2 ** 24:.2f} x 2^-24 depth")
        assert err.max() <= 16 * 2.0 ** -24
    if point_type == M.XYZRGB:
        assert np.array_equal(cloud[:, 3:], wcloud[:, 3:])
    check_geometry(real, cloud, flag, R1)


@pytest.mark.gpu
def test_stereo_reconstruct_empty_new_size(L):
    """the reference's cloud loop runs over newSize: an empty one gives full-size images and no points"""
    real, rec1, rec2, cloud = reconstruct(1, PERSPECTIVE, M.XYZ, new_size=None)
    w, h = M.RIG_SIZE
    assert real.shape == (h, w) and rec1.shape == (h, w) and rec2.shape == (h, w) and cloud.shape == (0, 3)
    R1, _ = api.omnidir_stereo_rectify(M.RIG_OM, M.RIG_T)
    assert np.array_equal(rec1, api.omnidir_undistort_image(rendered(1)[0], M.RIG_K[0], M.RIG_D[0], M.RIG_XI[0], PERSPECTIVE,
                                                            Knew=M.rig_knew(PERSPECTIVE), R=R1))
    assert np.array_equal(real, M.real_disparity(M.sgbm(rec1, rec2, 32, 5), rec1))


@pytest.mark.gpu
def test_stereo_reconstruct_capacity_too_small(L):
    a, b = rendered(1)
    w, h = M.RIG_SIZE
    _, _, _, full = reconstruct(1, PERSPECTIVE, M.XYZ)
    n, cap = len(full), len(full) - 1
    real, rec = np.zeros((h, w), np.float32), [np.zeros((h, w), np.uint8) for _ in range(2)]
    cloud = np.full((cap + 8, 3), 12345.0, np.float32)      # guard words: before, in and after the capacity
    count = ctypes.c_longlong(0)
    R, Kn = U.rotation(M.RIG_OM), M.rig_knew(PERSPECTIVE)
    rc = L.mcc_omnidir_stereo_reconstruct(
        _p(a, _u8), w, h, 1, w, _p(b, _u8), w, h, 1, w, _p(M.RIG_K[0]), _p(M.RIG_D[0]), M.RIG_XI[0], _p(M.RIG_K[1]),
        _p(M.RIG_D[1]), M.RIG_XI[1], _p(R), _p(M.RIG_T), PERSPECTIVE, 32, 5, w, h, _p(Kn), M.XYZ, 0, _p(real, _f32),
        _p(rec[0], _u8), w, _p(rec[1], _u8), w, _p(cloud, _f32), cap, ctypes.byref(count))
    assert rc == MCC_EINVAL and str(n).encode() in L.mcc_last_error()
    assert count.value == n
    assert (cloud == 12345.0).all()
    with pytest.raises(api.MccError):
        reconstruct(1, PERSPECTIVE, M.XYZ, capacity=cap)
    assert len(reconstruct(1, PERSPECTIVE, M.XYZ, capacity=n)[3]) == n


@pytest.mark.gpu
def test_reconstructor_handle_keeps_no_state(L):
    """two different pairs through one handle equal two one-shot calls bit for bit"""
    pairs = [rendered(1), tuple(np.ascontiguousarray(np.roll(x, 7, axis=1)[::-1]) for x in rendered(1))]
    Kn = M.rig_knew(LONGLATI)
    args = (M.RIG_K[0], M.RIG_D[0], M.RIG_XI[0], M.RIG_K[1], M.RIG_D[1], M.RIG_XI[1], M.RIG_OM, M.RIG_T, LONGLATI, 32, 5)
    once = [api.omnidir_stereo_reconstruct(a, b, *args, new_size=M.RIG_SIZE, Knew=Kn) for a, b in pairs]
    assert not np.array_equal(once[0][0], once[1][0])
    rec = api.OmniReconstructor(*args, M.RIG_SIZE, channels=1, new_size=M.RIG_SIZE, Knew=Kn)
    try:
        for k in (0, 1, 0):
            got = rec.compute(*pairs[k])
            for g, w in zip(got, once[k]):
                assert g.dtype == w.dtype and np.array_equal(g, w)
        ms = rec.time(3)
        assert np.isfinite(ms) and ms > 0
        got = rec.compute(*pairs[1])      # the timed random frames leave nothing behind either
        assert all(np.array_equal(g, w) for g, w in zip(got, once[1]))
    finally:
        rec.close()
