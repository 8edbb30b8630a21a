"""Python binding of libmcc.so (include/mcc.h) -- the MI355X hot path behind the reference's
optimiser seam.

Mirrors the reference's operator interface for this path (cv::multicalib, include/opencv2/ccalib/
multicalib.hpp:155-188):

    BundleAdjuster.optimize_extrinsics(...)       -> MultiCameraCalibration::optimizeExtrinsics
    BundleAdjuster.compute_jacobian_extrinsic(x)  -> computeJacobianExtrinsic(x, JTJ_inv, JTE, deltaX)
    BundleAdjuster.compute_project_error(x)       -> computeProjectError(x)

There is no CPU fallback: if libmcc.so is missing or the device is unusable the calls raise.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np

from . import rig as _rig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCC_LIB") or os.path.join(_HERE, "libmcc.so")   # MCC_LIB: libmcc_diag.so for stamps
HEADER = os.path.join(os.path.dirname(_HERE), "include", "mcc.h")
HEADERS = [HEADER, os.path.join(os.path.dirname(_HERE), "include", "mcc_omnidir.h")]   # the C ABI of libmcc.so

_i32p = ctypes.POINTER(ctypes.c_int)
_f32p = ctypes.POINTER(ctypes.c_float)
_f64p = ctypes.POINTER(ctypes.c_double)
_u8p = ctypes.POINTER(ctypes.c_ubyte)
_i16p = ctypes.POINTER(ctypes.c_short)
_u16p = ctypes.POINTER(ctypes.c_ushort)

MCC_CRIT_COUNT, MCC_CRIT_EPS, MCC_CRIT_COUNT_EPS = 1, 2, 3


class MccError(RuntimeError):
    pass


class _Desc(ctypes.Structure):
    _fields_ = [("model", ctypes.c_int), ("n_cams", ctypes.c_int), ("n_photos", ctypes.c_int),
                ("n_edges", ctypes.c_int), ("edge_cam", _i32p), ("edge_photo", _i32p),
                ("edge_side", _i32p), ("edge_off", _i32p), ("edge_n", _i32p),
                ("obj", _f32p), ("img", _f32p), ("nd", ctypes.c_int), ("K", _f32p),
                ("D", _f32p), ("xi", _f32p), ("ds_pose", _f64p), ("cam_pose", _f32p),
                ("device", ctypes.c_int)]


class _OmniDesc(ctypes.Structure):
    _fields_ = [("n_views", ctypes.c_int), ("view_off", _i32p), ("obj", _f64p), ("img", _f64p),
                ("flags", ctypes.c_int), ("device", ctypes.c_int)]


class _OmniStereoDesc(ctypes.Structure):
    _fields_ = [("n_views", ctypes.c_int), ("view_off", _i32p), ("obj", _f64p), ("img1", _f64p), ("img2", _f64p),
                ("flags", ctypes.c_int), ("device", ctypes.c_int)]


class _OmniRectDesc(ctypes.Structure):
    _fields_ = [("K", _f64p), ("D", _f64p), ("xi", ctypes.c_double), ("R", _f64p), ("P", _f64p),
                ("flags", ctypes.c_int), ("dst_width", ctypes.c_int), ("dst_height", ctypes.c_int),
                ("src_width", ctypes.c_int), ("src_height", ctypes.c_int), ("channels", ctypes.c_int),
                ("device", ctypes.c_int)]


class _OmniReconDesc(ctypes.Structure):
    _fields_ = [("K1", _f64p), ("D1", _f64p), ("xi1", ctypes.c_double), ("K2", _f64p), ("D2", _f64p),
                ("xi2", ctypes.c_double), ("R", _f64p), ("T", _f64p), ("flag", ctypes.c_int),
                ("num_disparities", ctypes.c_int), ("sad_window_size", ctypes.c_int), ("src_width", ctypes.c_int),
                ("src_height", ctypes.c_int), ("channels", ctypes.c_int), ("new_width", ctypes.c_int),
                ("new_height", ctypes.c_int), ("Knew", _f64p), ("point_type", ctypes.c_int), ("device", ctypes.c_int)]


class _PnpDesc(ctypes.Structure):
    _fields_ = [("n_views", ctypes.c_int), ("view_off", _i32p), ("obj", _f64p), ("img", _f64p), ("view_cam", _i32p),
                ("n_cams", ctypes.c_int), ("K", _f64p), ("D", _f64p), ("nd", ctypes.c_int), ("max_iter", ctypes.c_int),
                ("device", ctypes.c_int)]


PNP_SOLVED, PNP_TOO_FEW, PNP_DEGENERATE = 0, 1, 2


class _CalibDesc(ctypes.Structure):
    _fields_ = [("n_views", ctypes.c_int), ("view_off", _i32p), ("obj", _f64p), ("img", _f64p),
                ("image_width", ctypes.c_int), ("image_height", ctypes.c_int), ("flags", ctypes.c_int),
                ("nd", ctypes.c_int), ("crit_type", ctypes.c_int), ("max_count", ctypes.c_int), ("eps", ctypes.c_double),
                ("device", ctypes.c_int), ("trials", _i32p)]


# cv::CALIB_* values (include/mcc.h: MCC_CALIB_*)
CV_CALIB_USE_INTRINSIC_GUESS, CV_CALIB_FIX_ASPECT_RATIO, CV_CALIB_FIX_PRINCIPAL_POINT, CV_CALIB_ZERO_TANGENT_DIST = 1, 2, 4, 8
CV_CALIB_FIX_FOCAL_LENGTH, CV_CALIB_FIX_K1, CV_CALIB_FIX_K2, CV_CALIB_FIX_K3 = 16, 32, 64, 128
CV_CALIB_FIX_K4, CV_CALIB_FIX_K5, CV_CALIB_FIX_K6, CV_CALIB_RATIONAL_MODEL = 2048, 4096, 8192, 16384
CALIB_CONVERGED, CALIB_COUNT, CALIB_STALLED = 0, 1, 2
# cv::stereoCalibrate's own (mcc_stereo_calibrate)
CV_CALIB_FIX_INTRINSIC, CV_CALIB_SAME_FOCAL_LENGTH, CV_CALIB_USE_EXTRINSIC_GUESS = 256, 512, 1 << 22
CV_CALIB_ZERO_DISPARITY = 1024   # cv::stereoRectify's (mcc_stereo_rectify)


class _StereoCalibDesc(ctypes.Structure):
    _fields_ = [("n_views", ctypes.c_int), ("view_off", _i32p), ("obj", _f64p), ("img1", _f64p), ("img2", _f64p),
                ("image_width", ctypes.c_int), ("image_height", ctypes.c_int), ("flags", ctypes.c_int),
                ("nd", ctypes.c_int), ("crit_type", ctypes.c_int), ("max_count", ctypes.c_int), ("eps", ctypes.c_double),
                ("device", ctypes.c_int), ("trials", _i32p)]


class _PinRectDesc(ctypes.Structure):
    _fields_ = [("K", _f64p), ("D", _f64p), ("nd", ctypes.c_int), ("R", _f64p), ("P", _f64p), ("ld", ctypes.c_int),
                ("dst_width", ctypes.c_int), ("dst_height", ctypes.c_int), ("src_width", ctypes.c_int),
                ("src_height", ctypes.c_int), ("channels", ctypes.c_int), ("device", ctypes.c_int)]


class _PinReconDesc(ctypes.Structure):
    _fields_ = [("K1", _f64p), ("D1", _f64p), ("K2", _f64p), ("D2", _f64p), ("nd", ctypes.c_int), ("R", _f64p),
                ("T", _f64p), ("src_width", ctypes.c_int), ("src_height", ctypes.c_int), ("channels", ctypes.c_int),
                ("rectify_flags", ctypes.c_int), ("alpha", ctypes.c_double), ("new_width", ctypes.c_int),
                ("new_height", ctypes.c_int), ("num_disparities", ctypes.c_int), ("sad_window_size", ctypes.c_int),
                ("point_type", ctypes.c_int), ("use_roi", ctypes.c_int), ("max_z", ctypes.c_double),
                ("device", ctypes.c_int)]


class _PinReconGeometry(ctypes.Structure):
    _fields_ = [("R1", ctypes.c_double * 9), ("R2", ctypes.c_double * 9), ("P1", ctypes.c_double * 12),
                ("P2", ctypes.c_double * 12), ("Q", ctypes.c_double * 16), ("roi1", ctypes.c_int * 4),
                ("roi2", ctypes.c_int * 4), ("width", ctypes.c_int), ("height", ctypes.c_int),
                ("transposed", ctypes.c_int)]


DISP_FLOAT, DISP_FIXED16 = 1, 2   # include/mcc.h: MCC_DISP_*

_LIB = None


HOST_LIB_PATH = os.path.join(_HERE, "libmcc_host.so")
SAMPLE_PATH = os.path.join(_HERE, "build", "multi_cameras_calibration")
OMNI_SAMPLE_PATH = os.path.join(_HERE, "build", "omni_calibration")
OMNI_STEREO_SAMPLE_PATH = os.path.join(_HERE, "build", "omni_stereo_calibration")
# the reference's samples/multi_cameras_calibration.cpp compiled unchanged against
# include/opencv2/ccalib/*.hpp (built only where the reference tree exists; the binary travels)
REF_SAMPLE_SRC = "/root/reference/samples/multi_cameras_calibration.cpp"
REF_SAMPLE_PATH = os.path.join(_HERE, "build", "ref_multi_cameras_calibration")


def build(force: bool = False) -> str:
    """Compile libmcc.so in-tree for gfx950 (hipcc cross-compiles without a GPU), and the host
    side of the sample flow (libmcc_host.so, build/multi_cameras_calibration) with g++."""
    inc = os.path.dirname(HEADER)
    srcs = [os.path.join(_HERE, d, f) for d in ("csrc", "host", "samples") for f in os.listdir(os.path.join(_HERE, d))]
    srcs += [os.path.join(inc, f) for f in os.listdir(inc)]
    outs = [LIB_PATH, HOST_LIB_PATH, SAMPLE_PATH, OMNI_SAMPLE_PATH, OMNI_STEREO_SAMPLE_PATH]
    stale = any(not os.path.exists(o) for o in outs) or any(
        os.path.getmtime(s) > min(os.path.getmtime(o) for o in outs) for s in srcs)
    if force or stale:
        subprocess.run(["make", "-s", "--no-print-directory", "-C", _HERE, "-j8", "all"], check=True)
    if os.path.exists(REF_SAMPLE_SRC):
        # optional: the reference's sample compiled against the compatibility headers (the test
        # that needs it, tests/test_reference_sample.py, builds it itself and reports a failure);
        # a drifted header must not keep libmcc.so from loading
        r = subprocess.run(["make", "-s", "--no-print-directory", "-C", _HERE, "ref_sample"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            import warnings
            warnings.warn(f"reference sample build failed (libmcc.so is unaffected):\n{r.stdout[-2000:]}")
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise MccError(f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        L = ctypes.CDLL(LIB_PATH)
        L.mcc_last_error.restype = ctypes.c_char_p
        L.mcc_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(_Desc)]
        for name in ("mcc_nparams", "mcc_global_dim"):
            getattr(L, name).argtypes = [ctypes.c_void_p]
        L.mcc_destroy.argtypes = [ctypes.c_void_p]
        L.mcc_destroy.restype = None
        L.mcc_set_params.argtypes = [ctypes.c_void_p, _f32p, ctypes.c_int]
        L.mcc_get_params.argtypes = [ctypes.c_void_p, _f32p, ctypes.c_int]
        L.mcc_linearize_solve.argtypes = [ctypes.c_void_p, _f64p, _f64p]
        L.mcc_optimize.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, _f32p,
                                   _i32p, _f64p]
        L.mcc_step.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.mcc_synchronize.argtypes = [ctypes.c_void_p]
        L.mcc_check.argtypes = [ctypes.c_void_p]
        L.mcc_project_error.argtypes = [ctypes.c_void_p, _f32p, _f32p, _f64p]
        L.mcc_debug_residuals.argtypes = [ctypes.c_void_p, _f32p, _f32p]
        # (round-6 entry points: absent from an older build loaded through MCC_LIB for an A/B)
        if hasattr(L, "mcc_optimize_profile"):
            L.mcc_optimize_profile.argtypes = [ctypes.c_void_p, _f64p, _f64p, _i32p, _i32p, _i32p]
        if hasattr(L, "mcc_debug_delays"):
            L.mcc_debug_delays.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double]
        L.mcc_timing_begin.argtypes = [ctypes.c_void_p]
        L.mcc_timing_end.argtypes = [ctypes.c_void_p, _f64p, _f64p, _i32p]
        L.mcc_timing_exchange.argtypes = [ctypes.c_void_p, _f64p, _i32p]
        L.mcc_timing_windows.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _f64p, _i32p]
        L.mcc_timing_linearize.argtypes = [ctypes.c_void_p, ctypes.c_int, _f64p]
        L.mcc_project_error_detail.argtypes = [ctypes.c_void_p, _f32p, _f32p, _f32p, _f32p,
                                               ctypes.POINTER(ctypes.c_longlong), _f64p]
        L.mcc_problem_stats.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_longlong)] * 4
        L.mcc_solve_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong)]
        L.mcc_problem_path.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.mcc_comm_unique_id.argtypes = [ctypes.c_char_p]
        L.mcc_comm_init.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
        L.mcc_comm_allreduce_max.argtypes = [ctypes.c_void_p, _f64p]
        L.mcc_comm_barrier.argtypes = [ctypes.c_void_p]
        L.mcc_partition_photos.argtypes = [ctypes.c_int, ctypes.c_int, _i32p, _i32p, ctypes.c_int, _i32p]
        L.mcc_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
        L.mcc_debug_solve.argtypes = [ctypes.c_int, ctypes.c_int, _f64p, _f64p, ctypes.c_int, _f64p,
                                      ctypes.POINTER(ctypes.c_longlong)]
        L.mcc_peer_handle.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        L.mcc_peer_init.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
        L.mcc_peer_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
        # include/mcc_omnidir.h
        for pre, desc in (("omnicalib", _OmniDesc), ("omnistereo", _OmniStereoDesc)):
            f = {k: getattr(L, f"mcc_{pre}_{k}")
                 for k in ("create", "destroy", "nparams", "jacobian", "optimize", "rms", "time_steps")}
            f["create"].argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(desc)]
            f["destroy"].argtypes = [ctypes.c_void_p]
            f["destroy"].restype = None
            f["nparams"].argtypes = [ctypes.c_void_p]
            f["jacobian"].argtypes = [ctypes.c_void_p, _f64p, ctypes.c_int, _f64p, _f64p]
            f["optimize"].argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, _f64p, _i32p, _f64p]
            f["rms"].argtypes = [ctypes.c_void_p, _f64p, _f64p]
            f["time_steps"].argtypes = [ctypes.c_void_p, _f64p, ctypes.c_int, _f64p]
        L.mcc_omnidir_initialize.argtypes = [ctypes.c_int, _i32p, _f64p, _f64p, ctypes.c_int, ctypes.c_int, _f64p,
                                             _f64p, _f64p, _f64p, _i32p, _i32p]
        L.mcc_omnidir_calibrate.argtypes = [ctypes.c_int, _i32p, _f64p, _f64p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                            _f64p, _f64p, _f64p, _f64p, _f64p, _i32p, _i32p, _f64p, _i32p]
        L.mcc_omnidir_stereo_encode_init.argtypes = [ctypes.c_int, _i32p, _f64p, _f64p, ctypes.c_int, _i32p, _f64p,
                                                     _f64p, _f64p, ctypes.c_double, _f64p, _f64p, ctypes.c_double,
                                                     _f64p, _f64p, _i32p, _i32p]
        L.mcc_omnidir_stereo_initialize.argtypes = [ctypes.c_int, _i32p, _f64p, _f64p, _f64p] + [ctypes.c_int] * 6 + [
            _f64p, _i32p, _i32p]
        L.mcc_omnidir_stereo_calibrate.argtypes = [ctypes.c_int, _i32p, _f64p, _f64p, _f64p] + [ctypes.c_int] * 7 + [
            ctypes.c_double, ctypes.c_int] + [_f64p] * 10 + [_i32p, _i32p, _f64p, _i32p]
        # (the rectification entry points: absent from an older build loaded through MCC_LIB for an A/B)
        _ll = ctypes.c_longlong
        for name, args in (
                ("mcc_omnidir_undistort_points", [ctypes.c_int, _f64p, _f64p, _f64p, ctypes.c_double, _f64p, ctypes.c_int,
                                                  _f64p]),
                ("mcc_omnidir_stereo_rectify", [_f64p] * 4),
                ("mcc_omnidir_init_undistort_rectify_map", [_f64p, _f64p, ctypes.c_double, _f64p, _f64p] +
                 [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2),
                ("mcc_omnidir_remap", [_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _ll, _i16p, _u16p, ctypes.c_int,
                                       ctypes.c_int, _u8p, _ll, ctypes.c_int]),
                ("mcc_omnidir_undistort_image", [_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _ll, _f64p, _f64p,
                                                 ctypes.c_double, ctypes.c_int, _f64p, ctypes.c_int, ctypes.c_int, _f64p,
                                                 ctypes.c_int, _u8p, _ll]),
                ("mcc_omnirect_create", [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(_OmniRectDesc)]),
                ("mcc_omnirect_destroy", [ctypes.c_void_p]),
                ("mcc_omnirect_remap", [ctypes.c_void_p, _u8p, _ll, _u8p, _ll]),
                ("mcc_omnirect_time_remap", [ctypes.c_void_p, ctypes.c_int, _f64p]),
                ("mcc_omnidir_sgbm", [_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _ll] * 2 + [ctypes.c_int] * 3 + [_i16p]),
                ("mcc_omnirecon_create", [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(_OmniReconDesc)]),
                ("mcc_omnirecon_destroy", [ctypes.c_void_p]),
                ("mcc_omnirecon_compute", [ctypes.c_void_p, _u8p, _ll, _u8p, _ll, _f32p, _u8p, _ll, _u8p, _ll, _f32p, _ll,
                                           ctypes.POINTER(_ll)]),
                ("mcc_omnirecon_time", [ctypes.c_void_p, ctypes.c_int, _f64p]),
                ("mcc_omnidir_stereo_reconstruct", [_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _ll] * 2 +
                 [_f64p, _f64p, ctypes.c_double] * 2 + [_f64p, _f64p] + [ctypes.c_int] * 5 + [_f64p, ctypes.c_int,
                                                                                             ctypes.c_int, _f32p, _u8p, _ll,
                                                                                             _u8p, _ll, _f32p, _ll,
                                                                                             ctypes.POINTER(_ll)]),
                ("mcc_solve_pnp_batch", [ctypes.POINTER(_PnpDesc), _f64p, _f64p, _f64p, _i32p, _f64p]),
                ("mcc_calib_mask", [ctypes.c_int, ctypes.c_int, _i32p]),
                ("mcc_init_camera_matrix", [ctypes.POINTER(_CalibDesc), ctypes.c_double, _f64p]),
                ("mcc_calibrate_camera", [ctypes.POINTER(_CalibDesc), _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p,
                                          _i32p, _f64p]),
                ("mcc_stereo_calib_mask", [ctypes.c_int, ctypes.c_int, _i32p, _i32p]),
                ("mcc_stereo_init_extrinsics", [ctypes.c_int] + [_f64p] * 6),
                ("mcc_stereo_epipolar", [_f64p] * 6),
                ("mcc_stereo_calibrate", [ctypes.POINTER(_StereoCalibDesc)] + [_f64p] * 12 + [_i32p, _i32p, _f64p]),
                ("mcc_undistort_points", [ctypes.c_int, _f64p, _f64p, _f64p, ctypes.c_int, _f64p, _f64p] +
                 [ctypes.c_int] * 3 + [_f64p, _f64p]),
                ("mcc_init_undistort_rectify_map", [_f64p, _f64p, ctypes.c_int, _f64p, _f64p] + [ctypes.c_int] * 5 +
                 [ctypes.c_void_p] * 2 + [_f64p]),
                ("mcc_stereo_rectify", [_f64p] * 4 + [ctypes.c_int] * 3 + [_f64p, _f64p, ctypes.c_int, ctypes.c_double,
                                                                          ctypes.c_int, ctypes.c_int] + [_f64p] * 5 +
                 [_i32p, _i32p]),
                ("mcc_undistort_image", [_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _ll, _f64p, _f64p, ctypes.c_int,
                                         _f64p, _f64p] + [ctypes.c_int] * 4 + [_u8p, _ll]),
                ("mcc_pinrect_create", [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(_PinRectDesc)]),
                ("mcc_pinrect_destroy", [ctypes.c_void_p]),
                ("mcc_pinrect_remap", [ctypes.c_void_p, _u8p, _ll, _u8p, _ll]),
                ("mcc_reproject_image_to_3d", [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _ll, _f64p,
                                               ctypes.c_int, ctypes.c_int, _f32p, _f64p]),
                ("mcc_pinrecon_create", [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(_PinReconDesc)]),
                ("mcc_pinrecon_destroy", [ctypes.c_void_p]),
                ("mcc_pinrecon_info", [ctypes.c_void_p, ctypes.POINTER(_PinReconGeometry)]),
                ("mcc_pinrecon_compute", [ctypes.c_void_p, _u8p, _ll, _u8p, _ll, _f32p, _i16p, _u8p, _ll, _u8p, _ll, _f32p,
                                          _f32p, _ll, ctypes.POINTER(_ll)]),
                ("mcc_pinrecon_time", [ctypes.c_void_p, ctypes.c_int, _f64p]),
                ("mcc_stereo_reconstruct", [_u8p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _ll] * 2 +
                 [ctypes.POINTER(_PinReconDesc), ctypes.POINTER(_PinReconGeometry), _f32p, _i16p, _u8p, _ll, _u8p, _ll,
                  _f32p, _f32p, _ll, ctypes.POINTER(_ll)]),
                ("mcc_pinrecon_host_cloud", [_f32p, ctypes.c_int, ctypes.c_int, _f64p, _u8p, ctypes.c_int, ctypes.c_int,
                                             _i32p, ctypes.c_double, _f32p, _ll, ctypes.POINTER(_ll)])):
            if hasattr(L, name):
                getattr(L, name).argtypes = args
        for name in ("mcc_omnirect_destroy", "mcc_omnirecon_destroy", "mcc_pinrect_destroy", "mcc_pinrecon_destroy"):
            if hasattr(L, name):
                getattr(L, name).restype = None
        _LIB = L
    return _LIB


def debug_solve(S, r, reps=0, stamps=False, device=0):
    """k_solve's m > 30 elimination alone on the SPD system S x = r (mcc_debug_solve): returns x,
    the average device microseconds per solve over `reps` launches (None without reps) and, with
    stamps, the first launch's 64 per-phase s_memtime stamps."""
    S = np.asarray(S, np.float64)
    m = S.shape[0]
    iu = np.triu_indices(m)
    packed = np.ascontiguousarray(np.concatenate([S[iu], np.asarray(r, np.float64)]))
    x = np.zeros(m, np.float64)
    us = np.zeros(1, np.float64)
    st = np.zeros(64, np.int64)
    _check(lib().mcc_debug_solve(device, m, _ptr(packed, _f64p), _ptr(x, _f64p), int(reps), _ptr(us, _f64p),
                                 st.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)) if stamps else None),
           "mcc_debug_solve")
    return x, (float(us[0]) if reps else None), (st if stamps else None)


def declared_symbols():
    """Every function the C-ABI headers of libmcc.so (include/mcc.h, include/mcc_omnidir.h) declare."""
    txt = "".join(open(h).read() for h in HEADERS)
    return sorted(set(re.findall(r"^\s*(?:int|void|const char \*)\s*\*?\s*(mcc_[a-z_]+)\s*\(", txt, re.M)))


def _check(rc, what):
    if rc != 0:
        raise MccError(f"{what} failed ({rc}): {lib().mcc_last_error().decode()}")


def _ptr(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def solve_pnp(obj, img, off, K, D, view_cam=None, max_iter=50, device=0, return_ms=False):
    """cv::solvePnP (SOLVEPNP_ITERATIVE, as host/pnp.cpp restates it) for a batch of views in one GPU
    launch (mcc_solve_pnp_batch): the pose seeds x0 that optimizeExtrinsics starts from.

    View v owns corners off[v]:off[v + 1] of obj [corners, 3] and img [corners, 2] (pixels) and is seen by
    camera view_cam[v] (camera 0 without view_cam) of K [n_cams, 3, 3] (or one 3 x 3) and D [n_cams, nd]
    (or one vector, or None), nd in {0, 4, 5, 8, 12}.  Returns (rvec [V, 3], tvec [V, 3], rms [V],
    status [V]): status PNP_SOLVED, PNP_TOO_FEW (rms -1) or PNP_DEGENERATE (rms -1); a view's result
    does not depend on the rest of the batch.  max_iter = 0 returns the closed-form initial poses.  With
    return_ms the launch's device milliseconds are appended."""
    off = np.ascontiguousarray(off, np.int32).reshape(-1)
    obj = np.ascontiguousarray(obj, np.float64).reshape(-1, 3)
    img = np.ascontiguousarray(img, np.float64).reshape(-1, 2)
    K = np.ascontiguousarray(K, np.float64).reshape(-1, 3, 3)
    n_cams = K.shape[0]
    D = np.zeros((n_cams, 0)) if D is None else np.ascontiguousarray(D, np.float64).reshape(n_cams, -1)
    n_views = len(off) - 1
    if n_views >= 1 and (len(obj) < off[-1] or len(img) < off[-1]):
        raise MccError(f"solve_pnp: off names {off[-1]} corners, obj has {len(obj)} and img {len(img)}")
    cam = None
    if view_cam is not None:
        cam = np.ascontiguousarray(view_cam, np.int32).reshape(-1)
        if len(cam) != n_views:
            raise MccError(f"solve_pnp: view_cam has {len(cam)} entries for {n_views} views")
    nv = max(n_views, 1)
    rvec, tvec = np.zeros((nv, 3)), np.zeros((nv, 3))
    rms, status, ms = np.zeros(nv), np.zeros(nv, np.int32), np.zeros(1)
    d = _PnpDesc(n_views, _ptr(off, _i32p), _ptr(obj, _f64p), _ptr(img, _f64p), _ptr(cam, _i32p), n_cams,
                 _ptr(K, _f64p), _ptr(D, _f64p) if D.shape[1] else None, D.shape[1], int(max_iter), int(device))
    _check(lib().mcc_solve_pnp_batch(ctypes.byref(d), _ptr(rvec, _f64p), _ptr(tvec, _f64p), _ptr(rms, _f64p),
                                     _ptr(status, _i32p), _ptr(ms, _f64p)), "mcc_solve_pnp_batch")
    out = (rvec, tvec, rms, status)
    return out + (float(ms[0]),) if return_ms else out


def calib_mask(flags=0, nd=5):
    """The 0/1 mask of free slots over fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 that cv::calibrateCamera's flags
    and the distortion width nd give (mcc_calib_mask)."""
    m = np.zeros(12, np.int32)
    _check(lib().mcc_calib_mask(int(flags), int(nd), _ptr(m, _i32p)), "mcc_calib_mask")
    return m


def _calib_desc(off, obj, img, image_size, flags, nd, crit_type, max_count, eps, device):
    off = np.ascontiguousarray(off, np.int32).reshape(-1)
    obj = np.ascontiguousarray(obj, np.float64).reshape(-1, 3)
    img = np.ascontiguousarray(img, np.float64).reshape(-1, 2)
    n_views = len(off) - 1
    if n_views >= 1 and (len(obj) < off[-1] or len(img) < off[-1]):
        raise MccError(f"calibrate_camera: off names {off[-1]} corners, obj has {len(obj)} and img {len(img)}")
    d = _CalibDesc(n_views, _ptr(off, _i32p), _ptr(obj, _f64p), _ptr(img, _f64p), int(image_size[0]), int(image_size[1]),
                   int(flags), int(nd), int(crit_type), int(max_count), float(eps), int(device), None)
    return d, (off, obj, img)   # (the arrays the descriptor points into)


def init_camera_matrix(off, obj, img, image_size, aspect_ratio=0.0):
    """cv::initCameraMatrix2D (mcc_init_camera_matrix): the closed-form K of a planar target's views, image_size
    = (width, height); aspect_ratio > 0 forces fx = aspect_ratio fy.  Host only."""
    d, keep = _calib_desc(off, obj, img, image_size, 0, 5, MCC_CRIT_COUNT_EPS, 30, 0.0, 0)
    K = np.zeros((3, 3))
    _check(lib().mcc_init_camera_matrix(ctypes.byref(d), float(aspect_ratio), _ptr(K, _f64p)), "mcc_init_camera_matrix")
    return K


def calibrate_camera(off, obj, img, image_size, K=None, D=None, flags=0, nd=5, max_count=30, eps=2.2e-16, device=0,
                     return_ms=False, crit_type=MCC_CRIT_COUNT_EPS):
    """cv::calibrateCamera for one pinhole camera on the GPU (mcc_calibrate_camera): view v owns corners
    off[v]:off[v + 1] of obj [corners, 3] and img [corners, 2] (pixels); image_size = (width, height); flags are
    cv::CALIB_*'s (CV_CALIB_* above; the omnidir CALIB_* below are another set); nd in {4, 5, 8}.  K and D are the guess with CV_CALIB_USE_INTRINSIC_GUESS (K also
    gives the ratio under CV_CALIB_FIX_ASPECT_RATIO).  Returns (rms, K [3, 3], D [nd], rvec [V, 3], tvec [V, 3],
    view_rms [V], iterations, status): the least-squares minimum of the reprojection error by Levenberg-Marquardt,
    stopped after max_count accepted steps or a relative step below eps (crit_type: MCC_CRIT_COUNT, MCC_CRIT_EPS or
    both; with MCC_CRIT_EPS alone max_count is not read); status CALIB_CONVERGED, CALIB_COUNT or CALIB_STALLED.
    With return_ms the loop's device milliseconds and its number of trials are appended."""
    d, keep = _calib_desc(off, obj, img, image_size, flags, nd, crit_type, max_count, eps, device)
    Kio = np.zeros((3, 3)) if K is None else np.array(K, np.float64).reshape(3, 3)
    Dio = np.zeros(max(int(nd), 1))
    if D is not None:
        Din = np.asarray(D, np.float64).reshape(-1)
        Dio[:min(len(Din), len(Dio))] = Din[:len(Dio)]
    nv = max(d.n_views, 1)
    rvec, tvec, vrms = np.zeros((nv, 3)), np.zeros((nv, 3)), np.zeros(nv)
    rms, ms, it, st, tr = np.zeros(1), np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    d.trials = _ptr(tr, _i32p)
    _check(lib().mcc_calibrate_camera(ctypes.byref(d), _ptr(Kio, _f64p), _ptr(Dio, _f64p), _ptr(rvec, _f64p),
                                      _ptr(tvec, _f64p), _ptr(vrms, _f64p), _ptr(rms, _f64p), _ptr(it, _i32p),
                                      _ptr(st, _i32p), _ptr(ms, _f64p)), "mcc_calibrate_camera")
    out = (float(rms[0]), Kio, Dio[:int(nd)], rvec, tvec, vrms, int(it[0]), int(st[0]))
    return out + (float(ms[0]), int(tr[0])) if return_ms else out


def stereo_calib_mask(flags=CV_CALIB_FIX_INTRINSIC, nd=5):
    """(mask [30], tie [30]) of cv::stereoCalibrate's flags over the slots om T | camera 1's fx fy cx cy k1 k2 p1 p2
    k3 k4 k5 k6 | camera 2's (mcc_stereo_calib_mask): mask is 1 at a free slot, tie[k] the slot that slot k follows
    (-1: none)."""
    m, t = np.zeros(30, np.int32), np.zeros(30, np.int32)
    _check(lib().mcc_stereo_calib_mask(int(flags), int(nd), _ptr(m, _i32p), _ptr(t, _i32p)), "mcc_stereo_calib_mask")
    return m, t


def stereo_init_extrinsics(rvec1, tvec1, rvec2, tvec2):
    """The rig's start (om [3], T [3]) from both cameras' poses of every view, [V, 3] each: cv::stereoCalibrate's
    component-wise median (mcc_stereo_init_extrinsics).  Host only."""
    a = [np.ascontiguousarray(x, np.float64).reshape(-1, 3) for x in (rvec1, tvec1, rvec2, tvec2)]
    if len({len(x) for x in a}) != 1:
        raise MccError("stereo_init_extrinsics: the four pose arrays differ in length")
    om, T = np.zeros(3), np.zeros(3)
    _check(lib().mcc_stereo_init_extrinsics(len(a[0]), *[_ptr(x, _f64p) for x in a], _ptr(om, _f64p), _ptr(T, _f64p)),
           "mcc_stereo_init_extrinsics")
    return om, T


def stereo_epipolar(R, T, K1, K2):
    """(E, F) of a rig as stereo_calibrate returns them: E = [T]x R, F = K2^-T E K1^-1 scaled to F[2, 2] = 1
    (mcc_stereo_epipolar).  Host only."""
    a = [np.ascontiguousarray(x, np.float64).reshape(n) for x, n in ((R, 9), (T, 3), (K1, 9), (K2, 9))]
    E, F = np.zeros((3, 3)), np.zeros((3, 3))
    _check(lib().mcc_stereo_epipolar(*[_ptr(x, _f64p) for x in a], _ptr(E, _f64p), _ptr(F, _f64p)), "mcc_stereo_epipolar")
    return E, F


def stereo_calibrate(off, obj, img1, img2, image_size, K1=None, D1=None, K2=None, D2=None, R=None, T=None,
                     flags=CV_CALIB_FIX_INTRINSIC, nd=5, max_count=30, eps=1e-6, crit_type=MCC_CRIT_COUNT_EPS, device=0,
                     return_ms=False):
    """cv::stereoCalibrate for a pinhole pair on the GPU (mcc_stereo_calibrate): view v owns corners
    off[v]:off[v + 1] of obj [corners, 3], img1 and img2 [corners, 2] (pixels); flags are cv::CALIB_*'s (CV_CALIB_*
    above); nd in {4, 5, 8}.  K1 D1 K2 D2 are the intrinsics with CV_CALIB_FIX_INTRINSIC (the default) or the guess
    with CV_CALIB_USE_INTRINSIC_GUESS; R [3, 3] and T [3] are the rig's start with CV_CALIB_USE_EXTRINSIC_GUESS.
    Returns (rms, K1, D1, K2, D2, R, T, E, F, rvec [V, 3], tvec [V, 3], view_rms [V, 2], iterations, status): camera
    2 sees view v at R R_v, R t_v + T; rvec, tvec are the views' poses in camera 1; status CALIB_CONVERGED,
    CALIB_COUNT or CALIB_STALLED.  With return_ms the loop's device milliseconds and its number of trials are
    appended."""
    off = np.ascontiguousarray(off, np.int32).reshape(-1)
    obj = np.ascontiguousarray(obj, np.float64).reshape(-1, 3)
    img1 = np.ascontiguousarray(img1, np.float64).reshape(-1, 2)
    img2 = np.ascontiguousarray(img2, np.float64).reshape(-1, 2)
    n_views = len(off) - 1
    if n_views >= 1 and min(len(obj), len(img1), len(img2)) < off[-1]:
        raise MccError(f"stereo_calibrate: off names {off[-1]} corners, obj has {len(obj)}, img1 {len(img1)} and img2 {len(img2)}")
    tr = np.zeros(1, np.int32)
    d = _StereoCalibDesc(n_views, _ptr(off, _i32p), _ptr(obj, _f64p), _ptr(img1, _f64p), _ptr(img2, _f64p),
                         int(image_size[0]), int(image_size[1]), int(flags), int(nd), int(crit_type), int(max_count),
                         float(eps), int(device), _ptr(tr, _i32p))

    def _D(D):
        out = np.zeros(max(int(nd), 1))
        if D is not None:
            Din = np.asarray(D, np.float64).reshape(-1)
            out[:min(len(Din), len(out))] = Din[:len(out)]
        return out

    Ks = [np.zeros((3, 3)) if K is None else np.array(K, np.float64).reshape(3, 3) for K in (K1, K2)]
    Ds = [_D(D1), _D(D2)]
    Rio = np.eye(3) if R is None else np.array(R, np.float64).reshape(3, 3)
    Tio = np.zeros(3) if T is None else np.array(T, np.float64).reshape(3)
    E, F = np.zeros((3, 3)), np.zeros((3, 3))
    nv = max(n_views, 1)
    rvec, tvec, vrms = np.zeros((nv, 3)), np.zeros((nv, 3)), np.zeros((nv, 2))
    rms, ms, it, st = np.zeros(1), np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32)
    _check(lib().mcc_stereo_calibrate(ctypes.byref(d), _ptr(Ks[0], _f64p), _ptr(Ds[0], _f64p), _ptr(Ks[1], _f64p),
                                      _ptr(Ds[1], _f64p), _ptr(Rio, _f64p), _ptr(Tio, _f64p), _ptr(E, _f64p), _ptr(F, _f64p),
                                      _ptr(rvec, _f64p), _ptr(tvec, _f64p), _ptr(vrms, _f64p), _ptr(rms, _f64p),
                                      _ptr(it, _i32p), _ptr(st, _i32p), _ptr(ms, _f64p)), "mcc_stereo_calibrate")
    out = (float(rms[0]), Ks[0], Ds[0][:int(nd)], Ks[1], Ds[1][:int(nd)], Rio, Tio, E, F, rvec, tvec, vrms, int(it[0]),
           int(st[0]))
    return out + (float(ms[0]), int(tr[0])) if return_ms else out


def partition_photos(prob, nranks):
    """Greedy corner-count balance of photo vertices over ranks (mcc_partition_photos)."""
    out = np.zeros(prob.n_photos, np.int32)
    ep = np.ascontiguousarray(prob.edge_photo, np.int32)
    en = np.ascontiguousarray(prob.edge_n, np.int32)
    _check(lib().mcc_partition_photos(prob.n_photos, prob.n_edges, _ptr(ep, _i32p), _ptr(en, _i32p),
                                      nranks, _ptr(out, _i32p)), "mcc_partition_photos")
    return out


def file_allgather(directory: str, rank: int, world: int, payload: bytes, timeout: float = 300.0) -> list:
    """All-gather of small byte strings among the processes of one node through files in
    `directory` (RCCL unique id and peer inbox handles; no torch, no RCCL needed)."""
    import time
    os.makedirs(directory, exist_ok=True)
    tmp = os.path.join(directory, f".r{rank}.tmp")
    with open(tmp, "wb") as f:
        f.write(payload)
    os.replace(tmp, os.path.join(directory, f"r{rank}"))
    out, t0 = [None] * world, time.time()
    while any(v is None for v in out):
        for q in range(world):
            fn = os.path.join(directory, f"r{q}")
            if out[q] is None and os.path.exists(fn):
                with open(fn, "rb") as f:
                    out[q] = f.read()
        if time.time() - t0 > timeout:
            raise MccError(f"timed out waiting for {world} ranks in {directory}")
        time.sleep(0.02)
    return out


def unique_id() -> bytes:
    buf = ctypes.create_string_buffer(128)
    _check(lib().mcc_comm_unique_id(buf), "mcc_comm_unique_id")
    return buf.raw


class BundleAdjuster:
    """One mcc_problem: the reference's BA state for one (local) set of photo vertices."""

    def __init__(self, prob: "_rig.Problem", device: int = 0):
        self.prob = prob
        self._keep = []

        def arr(a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            self._keep.append(a)
            return a
        d = _Desc()
        d.model, d.n_cams, d.n_photos, d.n_edges = prob.model, prob.n_cams, prob.n_photos, prob.n_edges
        d.edge_cam = _ptr(arr(prob.edge_cam, np.int32), _i32p)
        d.edge_photo = _ptr(arr(prob.edge_photo, np.int32), _i32p)
        d.edge_side = _ptr(arr(prob.edge_side, np.int32), _i32p)
        d.edge_off = _ptr(arr(prob.edge_off, np.int32), _i32p)
        d.edge_n = _ptr(arr(prob.edge_n, np.int32), _i32p)
        d.obj = _ptr(arr(prob.obj, np.float32), _f32p)
        d.img = _ptr(arr(prob.img, np.float32), _f32p)
        d.nd = prob.nd
        d.K = _ptr(arr(prob.K, np.float32), _f32p)
        d.D = _ptr(arr(prob.D, np.float32), _f32p)
        d.xi = _ptr(arr(prob.xi, np.float32), _f32p) if prob.model == _rig.OMNI else None
        d.ds_pose = _ptr(arr(prob.ds_pose, np.float64), _f64p) if prob.ds_pose is not None else None
        d.cam_pose = _ptr(arr(prob.cam_pose, np.float32), _f32p) if prob.cam_pose is not None else None
        d.device = device
        h = ctypes.c_void_p()
        _check(lib().mcc_create(ctypes.byref(h), ctypes.byref(d)), "mcc_create")
        self.h = h
        self.P = lib().mcc_nparams(h)
        self.m = lib().mcc_global_dim(h)

    def close(self):
        if getattr(self, "h", None):
            lib().mcc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state
    def set_params(self, x):
        x = np.ascontiguousarray(x, np.float32)
        _check(lib().mcc_set_params(self.h, _ptr(x, _f32p), x.size), "mcc_set_params")

    def get_params(self):
        x = np.zeros(self.P, np.float32)
        _check(lib().mcc_get_params(self.h, _ptr(x, _f32p), self.P), "mcc_get_params")
        return x

    # -- the reference seam
    def compute_jacobian_extrinsic(self, x):
        """(deltaX, JTE) of one linearisation at x (computeJacobianExtrinsic)."""
        self.set_params(x)
        delta = np.zeros(self.P)
        jte = np.zeros(self.P)
        _check(lib().mcc_linearize_solve(self.h, _ptr(delta, _f64p), _ptr(jte, _f64p)), "mcc_linearize_solve")
        return delta, jte

    def optimize_extrinsics(self, x0, crit_type=MCC_CRIT_COUNT_EPS, max_count=200, eps=1e-7):
        """optimizeExtrinsics: returns (x, meanReProjError, iterations, last change)."""
        x = np.array(x0, np.float32, copy=True)
        it = ctypes.c_int(0)
        ch = ctypes.c_double(0)
        _check(lib().mcc_optimize(self.h, crit_type, max_count, eps, _ptr(x, _f32p), ctypes.byref(it),
                                  ctypes.byref(ch)), "mcc_optimize")
        _, mean = self.compute_project_error(x)
        return x, mean, it.value, ch.value

    def compute_project_error(self, x):
        x = np.ascontiguousarray(x, np.float32)
        err = np.zeros(self.prob.n_edges, np.float32)
        mean = ctypes.c_double(0)
        _check(lib().mcc_project_error(self.h, _ptr(x, _f32p), _ptr(err, _f32p), ctypes.byref(mean)),
               "mcc_project_error")
        return err, mean.value

    # -- throughput path
    def step(self, n):
        _check(lib().mcc_step(self.h, n), "mcc_step")

    def synchronize(self):
        _check(lib().mcc_synchronize(self.h), "mcc_synchronize")

    def check(self):
        """Raise if an enqueued step failed on the device (peer timeout, not positive definite)."""
        _check(lib().mcc_check(self.h), "mcc_check")

    def residuals(self, x):
        x = np.ascontiguousarray(x, np.float32)
        r = np.zeros(2 * self.prob.n_corners, np.float32)
        _check(lib().mcc_debug_residuals(self.h, _ptr(x, _f32p), _ptr(r, _f32p)), "mcc_debug_residuals")
        return r

    def optimize_profile(self):
        """The last optimize_extrinsics as the caller saw it (mcc_optimize_profile): host phases (ms),
        device ms from the first step launch to the end of the last, steps launched, updates, polls."""
        hm = np.zeros(4, np.float64)
        dev = ctypes.c_double(0)
        n, it, polls = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _check(lib().mcc_optimize_profile(self.h, _ptr(hm, _f64p), ctypes.byref(dev), ctypes.byref(n),
                                          ctypes.byref(it), ctypes.byref(polls)), "mcc_optimize_profile")
        return {"host_setup_ms": hm[0], "host_steps_ms": hm[1], "host_finish_ms": hm[2], "host_call_ms": hm[3],
                "device_ms": dev.value, "steps_launched": n.value, "iters": it.value, "stop_polls": polls.value}

    def debug_delays(self, spare_delay_us=-1.0, warm_delay_us=-1.0, warm_timeout_ms=-1.0):
        """test only: change the injected warm-solve delays / wait bound of this handle (-1 keeps one)"""
        _check(lib().mcc_debug_delays(self.h, float(spare_delay_us), float(warm_delay_us), float(warm_timeout_ms)),
               "mcc_debug_delays")

    def timing_begin(self):
        _check(lib().mcc_timing_begin(self.h), "mcc_timing_begin")

    def timing_end(self):
        lin = ctypes.c_double(0)
        st = ctypes.c_double(0)
        n = ctypes.c_int(0)
        _check(lib().mcc_timing_end(self.h, ctypes.byref(lin), ctypes.byref(st), ctypes.byref(n)), "mcc_timing_end")
        return lin.value, st.value, n.value

    def timing_windows(self, n_windows, steps):
        """Device time (ms) of each of n_windows back-to-back windows of `steps` free-running steps
        (mcc_timing_windows), and whether they ran graph-launched."""
        out = np.zeros(n_windows)
        g = ctypes.c_int(0)
        _check(lib().mcc_timing_windows(self.h, n_windows, steps, _ptr(out, _f64p), ctypes.byref(g)), "mcc_timing_windows")
        return out, bool(g.value)

    def project_error_detail(self, x):
        """(edge errors, per-corner L2 errors in reference order, totalError, totalNPoints, mean)."""
        x = np.ascontiguousarray(x, np.float32)
        err = np.zeros(self.prob.n_edges, np.float32)
        cerr = np.zeros(self.prob.n_corners, np.float32)
        tot = ctypes.c_float(0)
        npts = ctypes.c_longlong(0)
        mean = ctypes.c_double(0)
        _check(lib().mcc_project_error_detail(self.h, _ptr(x, _f32p), _ptr(err, _f32p), _ptr(cerr, _f32p),
                                              ctypes.byref(tot), ctypes.byref(npts), ctypes.byref(mean)),
               "mcc_project_error_detail")
        return err, cerr, tot.value, npts.value, mean.value

    def timing_linearize(self, launches: int) -> float:
        """Split step: ms per launch of the linearisation kernels alone, `launches` of them in one
        captured graph between two HIP events (mcc_timing_linearize)."""
        ms = ctypes.c_double()
        _check(lib().mcc_timing_linearize(self.h, launches, ctypes.byref(ms)), "mcc_timing_linearize")
        return ms.value

    def timing_exchange(self):
        """(ms per data-path exchange, exchanges) over the last timing window (mcc_timing_exchange)."""
        ms = ctypes.c_double(0)
        n = ctypes.c_int(0)
        _check(lib().mcc_timing_exchange(self.h, ctypes.byref(ms), ctypes.byref(n)), "mcc_timing_exchange")
        return ms.value, n.value

    def stats(self):
        v = [ctypes.c_longlong(0) for _ in range(4)]
        _check(lib().mcc_problem_stats(self.h, *[ctypes.byref(t) for t in v]), "mcc_problem_stats")
        return dict(corners=v[0].value, edges=v[1].value, photos=v[2].value, alg_bytes=v[3].value)

    def solve_stats(self):
        """The warm solves (mcc_solve_stats; m > 30: the helper kernel's inverse, m <= 30: the spare
        workgroup's): solves by refinement with the previous system's inverse, their refinement
        corrections, refinements that fell back to the direct elimination, direct solves for want of an
        inverse, steps that waited for the inverse's producer (the choice of solve never depends on the
        wait; all zero on the direct-only paths)."""
        v = (ctypes.c_longlong * 5)()
        _check(lib().mcc_solve_stats(self.h, v), "mcc_solve_stats")
        return dict(warm=v[0], corrections=v[1], fallbacks=v[2], direct=v[3], waited=v[4])

    def path(self):
        """'fused' (one kernel per step) or 'split' (k_prep, k_edge, k_photo, k_schur, k_solve)."""
        sp = ctypes.c_int(0)
        ng = ctypes.c_int(0)
        _check(lib().mcc_problem_path(self.h, ctypes.byref(sp), ctypes.byref(ng)), "mcc_problem_path")
        return "split" if sp.value else "fused"

    def step_kernels(self):
        """The kernels of one step's linearisation: 'k_linearize' (fused), 'k_group' (the split step's
        fused group kernel) or 'k_prep+k_edge+k_photo' (MCC_GROUP=0)."""
        sp = ctypes.c_int(0)
        ng = ctypes.c_int(0)
        _check(lib().mcc_problem_path(self.h, ctypes.byref(sp), ctypes.byref(ng)), "mcc_problem_path")
        return {0: "k_linearize", 1: "k_prep+k_edge+k_photo", 2: "k_group", 3: "k_group"}[sp.value]

    def photo_groups(self):
        """The split step's photo-group workgroups (mcc_problem_path; 0 on the fused step)."""
        sp = ctypes.c_int(0)
        ng = ctypes.c_int(0)
        _check(lib().mcc_problem_path(self.h, ctypes.byref(sp), ctypes.byref(ng)), "mcc_problem_path")
        return ng.value

    def folded(self):
        """True when a step is ONE k_group launch: the Schur reduction and the m <= 30 solve folded
        into the group kernel's grid (mcc_problem_path 3; MCC_GFOLD=0 turns it off)."""
        sp = ctypes.c_int(0)
        _check(lib().mcc_problem_path(self.h, ctypes.byref(sp), None), "mcc_problem_path")
        return sp.value == 3

    def stamps(self):
        """libmcc_diag.so only: first call arms, later calls return [n_photos, 32] s_memtime stamps
        followed by k_schur's [workgroups, 8]."""
        out = np.zeros(32 * max(self.prob.n_photos, 1) + 8 * 65536, np.int64)
        _check(lib().mcc_debug_stamps(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), out.size),
               "mcc_debug_stamps")
        return out

    # -- multi-GPU
    def comm_init(self, uid: bytes, nranks: int, rank: int):
        _check(lib().mcc_comm_init(self.h, uid, nranks, rank), "mcc_comm_init")

    def allreduce_max(self, v: float) -> float:
        d = ctypes.c_double(v)
        _check(lib().mcc_comm_allreduce_max(self.h, ctypes.byref(d)), "mcc_comm_allreduce_max")
        return d.value

    def barrier(self):
        _check(lib().mcc_comm_barrier(self.h), "mcc_comm_barrier")

    def peer_handle(self) -> bytes:
        buf = ctypes.create_string_buffer(64)
        _check(lib().mcc_peer_handle(self.h, buf), "mcc_peer_handle")
        return buf.raw

    def peer_init(self, handles, nranks: int, rank: int):
        """Collective: map the peers' inboxes and handshake (raises MccError on every rank if the
        transport does not work)."""
        blob = b"".join(handles)
        _check(lib().mcc_peer_init(self.h, blob, nranks, rank), "mcc_peer_init")

    def peer_enable(self, on: bool):
        _check(lib().mcc_peer_enable(self.h, int(bool(on))), "mcc_peer_enable")


# ---------------------------------------------------------------- cv::omnidir::calibrate
# include/mcc_omnidir.h; the reference's names: cv::omnidir::calibrate (src/omnidir.cpp:1067-1211),
# internal::initializeCalibration (:551-748), internal::computeJacobian (:851-935).
CALIB_USE_GUESS, CALIB_FIX_SKEW, CALIB_FIX_K1, CALIB_FIX_K2 = 1, 2, 4, 8
CALIB_FIX_P1, CALIB_FIX_P2, CALIB_FIX_XI, CALIB_FIX_GAMMA, CALIB_FIX_CENTER = 16, 32, 64, 128, 256


def _views(off, obj, img):
    off = np.ascontiguousarray(off, np.int32)
    obj = np.ascontiguousarray(obj, np.float64).reshape(-1, 3)
    img = np.ascontiguousarray(img, np.float64).reshape(-1, 2)
    if off.ndim != 1 or off.size < 2 or off[0] != 0 or off[-1] != obj.shape[0] or obj.shape[0] != img.shape[0]:
        raise MccError("view offsets / points mismatch")
    return off, obj, img


class _OmniLoop:
    """What OmniCalibrator and OmniStereoCalibrator share: the handle's life and the calls into the
    device loop, mcc_<_prefix>_* of include/mcc_omnidir.h."""
    _prefix = None

    def _call(self, name, *args):
        fn = f"mcc_{self._prefix}_{name}"
        _check(getattr(lib(), fn)(self.h, *args), fn)

    def close(self):
        if getattr(self, "h", None):
            getattr(lib(), f"mcc_{self._prefix}_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def compute_jacobian(self, params, it=0):
        p = np.ascontiguousarray(params, np.float64)
        jte, G = np.zeros(self.P), np.zeros(self.P)
        self._call("jacobian", _ptr(p, _f64p), it, _ptr(jte, _f64p), _ptr(G, _f64p))
        return jte, G

    def optimize(self, params, crit_type=MCC_CRIT_COUNT_EPS, max_count=200, eps=1e-4):
        p = np.array(params, np.float64, copy=True)
        it, ch = ctypes.c_int(0), ctypes.c_double(0)
        self._call("optimize", crit_type, max_count, eps, _ptr(p, _f64p), ctypes.byref(it), ctypes.byref(ch))
        return p, it.value, ch.value

    def rms(self, params):
        p = np.ascontiguousarray(params, np.float64)
        r = ctypes.c_double(0)
        self._call("rms", _ptr(p, _f64p), ctypes.byref(r))
        return r.value

    def time_steps(self, params, n_steps):
        p = np.ascontiguousarray(params, np.float64)
        ms = ctypes.c_double(0)
        self._call("time_steps", _ptr(p, _f64p), n_steps, ctypes.byref(ms))
        return ms.value


class OmniCalibrator(_OmniLoop):
    """The device-resident state of cv::omnidir::calibrate's loop for one camera's views
    (CV_64F pattern / image points, parameters in encodeParameters layout, P = 6n + 10)."""
    _prefix = "omnicalib"

    def __init__(self, off, obj, img, flags: int = 0, device: int = 0):
        self.off, self.obj, self.img = _views(off, obj, img)
        d = _OmniDesc()
        d.n_views = self.off.size - 1
        d.view_off = _ptr(self.off, _i32p)
        d.obj = _ptr(self.obj, _f64p)
        d.img = _ptr(self.img, _f64p)
        d.flags, d.device = flags, device
        h = ctypes.c_void_p()
        _check(lib().mcc_omnicalib_create(ctypes.byref(h), ctypes.byref(d)), "mcc_omnicalib_create")
        self.h = h
        self.P = lib().mcc_omnicalib_nparams(h)

    def compute_jacobian(self, params, it=0):
        """(JTE before the flag reduction, G of loop iteration `it`) at params (computeJacobian)."""
        return super().compute_jacobian(params, it)

    def optimize(self, params, crit_type=MCC_CRIT_COUNT_EPS, max_count=200, eps=1e-4):
        """calibrate's loop: (params, iterations, last change)."""
        return super().optimize(params, crit_type, max_count, eps)


def omnidir_initialize(off, obj, img, image_size):
    """initializeCalibration: (om[k, 3], t[k, 3], K 3x3, xi, idx[k]) -- host code, no GPU."""
    off, obj, img = _views(off, obj, img)
    n = off.size - 1
    om, t, K = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(9)
    xi, nk = ctypes.c_double(0), ctypes.c_int(0)
    idx = np.zeros(n, np.int32)
    _check(lib().mcc_omnidir_initialize(n, _ptr(off, _i32p), _ptr(obj, _f64p), _ptr(img, _f64p), int(image_size[0]),
                                        int(image_size[1]), _ptr(om, _f64p), _ptr(t, _f64p), _ptr(K, _f64p),
                                        ctypes.byref(xi), _ptr(idx, _i32p), ctypes.byref(nk)),
           "mcc_omnidir_initialize")
    k = nk.value
    return om[:k], t[:k], K.reshape(3, 3), xi.value, idx[:k].copy()


def omnidir_calibrate(off, obj, img, image_size, flags=0, crit_type=MCC_CRIT_COUNT_EPS, max_count=200, eps=1e-4,
                      device=0):
    """cv::omnidir::calibrate: (rms, K, xi, D, om[k, 3], t[k, 3], idx[k], iterations)."""
    off, obj, img = _views(off, obj, img)
    n = off.size - 1
    K, D = np.zeros(9), np.zeros(4)
    om, t = np.zeros((n, 3)), np.zeros((n, 3))
    xi, rms, nk, it = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0), ctypes.c_int(0)
    idx = np.zeros(n, np.int32)
    _check(lib().mcc_omnidir_calibrate(n, _ptr(off, _i32p), _ptr(obj, _f64p), _ptr(img, _f64p), int(image_size[0]),
                                       int(image_size[1]), flags, crit_type, max_count, eps, device, _ptr(K, _f64p),
                                       ctypes.byref(xi), _ptr(D, _f64p), _ptr(om, _f64p), _ptr(t, _f64p),
                                       _ptr(idx, _i32p), ctypes.byref(nk), ctypes.byref(rms), ctypes.byref(it)),
           "mcc_omnidir_calibrate")
    k = nk.value
    return rms.value, K.reshape(3, 3), xi.value, D, om[:k], t[:k], idx[:k].copy(), it.value


# ---------------------------------------------------------------- cv::omnidir::stereoCalibrate
# include/mcc_omnidir.h; the reference's names: cv::omnidir::stereoCalibrate (src/omnidir.cpp:1213-1381),
# internal::initializeStereoCalibration (:750-846), internal::computeJacobianStereo (:937-1020).
def _stereo_views(off, obj, img1, img2):
    off, obj, img1 = _views(off, obj, img1)
    img2 = np.ascontiguousarray(img2, np.float64).reshape(-1, 2)
    if img2.shape[0] != img1.shape[0]:
        raise MccError("view offsets / points mismatch")
    return off, obj, img1, img2


class OmniStereoCalibrator(_OmniLoop):
    """The device-resident state of cv::omnidir::stereoCalibrate's loop for the views both cameras
    see (CV_64F points, the same corner count in every view; parameters in encodeParametersStereo
    layout, P = 6(n + 1) + 20)."""
    _prefix = "omnistereo"

    def __init__(self, off, obj, img1, img2, flags: int = 0, device: int = 0):
        self.off, self.obj, self.img1, self.img2 = _stereo_views(off, obj, img1, img2)
        d = _OmniStereoDesc()
        d.n_views = self.off.size - 1
        d.view_off = _ptr(self.off, _i32p)
        d.obj = _ptr(self.obj, _f64p)
        d.img1 = _ptr(self.img1, _f64p)
        d.img2 = _ptr(self.img2, _f64p)
        d.flags, d.device = flags, device
        h = ctypes.c_void_p()
        _check(lib().mcc_omnistereo_create(ctypes.byref(h), ctypes.byref(d)), "mcc_omnistereo_create")
        self.h = h
        self.P = lib().mcc_omnistereo_nparams(h)

    def compute_jacobian(self, params, it=0):
        """(JTE before the flag reduction, G of loop iteration `it`) at params (computeJacobianStereo)."""
        return super().compute_jacobian(params, it)

    def optimize(self, params, crit_type=MCC_CRIT_COUNT_EPS, max_count=200, eps=1e-4):
        """stereoCalibrate's loop: (params, iterations, last change)."""
        return super().optimize(params, crit_type, max_count, eps)


def omnidir_stereo_encode_init(idx1, om1, t1, idx2, om2, t2, K1, xi1, D1, K2, xi2, D2):
    """The host part of initializeStereoCalibration from the two cameras' calibrate results (kept
    indices, poses in kept order, intrinsics): (params, idx of the common views) -- no GPU."""
    idx1, idx2 = np.ascontiguousarray(idx1, np.int32), np.ascontiguousarray(idx2, np.int32)
    a = [np.ascontiguousarray(v, np.float64) for v in (om1, t1, om2, t2, K1, D1, K2, D2)]
    if a[0].size != 3 * idx1.size or a[1].size != 3 * idx1.size or a[2].size != 3 * idx2.size or \
            a[3].size != 3 * idx2.size or a[4].size != 9 or a[6].size != 9 or a[5].size != 4 or a[7].size != 4:
        raise MccError("kept lists / poses / intrinsics mismatch")
    m = max(min(idx1.size, idx2.size), 1)
    params, idx, nk = np.zeros(6 * (m + 1) + 20), np.zeros(m, np.int32), ctypes.c_int(0)
    _check(lib().mcc_omnidir_stereo_encode_init(idx1.size, _ptr(idx1, _i32p), _ptr(a[0], _f64p), _ptr(a[1], _f64p),
                                                idx2.size, _ptr(idx2, _i32p), _ptr(a[2], _f64p), _ptr(a[3], _f64p),
                                                _ptr(a[4], _f64p), float(xi1), _ptr(a[5], _f64p), _ptr(a[6], _f64p),
                                                float(xi2), _ptr(a[7], _f64p), _ptr(params, _f64p), _ptr(idx, _i32p),
                                                ctypes.byref(nk)), "mcc_omnidir_stereo_encode_init")
    k = nk.value
    return params[:6 * (k + 1) + 20].copy(), idx[:k].copy()


def omnidir_stereo_initialize(off, obj, img1, img2, image_size1, image_size2, flags=0, device=0):
    """initializeStereoCalibration: (params in encodeParametersStereo layout, idx of the kept views);
    the two single-camera calibrations run on the GPU."""
    off, obj, img1, img2 = _stereo_views(off, obj, img1, img2)
    n = off.size - 1
    params, idx, nk = np.zeros(6 * (n + 1) + 20), np.zeros(n, np.int32), ctypes.c_int(0)
    _check(lib().mcc_omnidir_stereo_initialize(n, _ptr(off, _i32p), _ptr(obj, _f64p), _ptr(img1, _f64p),
                                               _ptr(img2, _f64p), int(image_size1[0]), int(image_size1[1]),
                                               int(image_size2[0]), int(image_size2[1]), flags, device,
                                               _ptr(params, _f64p), _ptr(idx, _i32p), ctypes.byref(nk)),
           "mcc_omnidir_stereo_initialize")
    k = nk.value
    return params[:6 * (k + 1) + 20].copy(), idx[:k].copy()


def omnidir_stereo_calibrate(off, obj, img1, img2, image_size1, image_size2, flags=0, crit_type=MCC_CRIT_COUNT_EPS,
                             max_count=200, eps=1e-4, device=0):
    """cv::omnidir::stereoCalibrate:
    (rms, K1, xi1, D1, K2, xi2, D2, om, T, omL[k, 3], tL[k, 3], idx[k], iterations)."""
    off, obj, img1, img2 = _stereo_views(off, obj, img1, img2)
    n = off.size - 1
    K1, K2, D1, D2, om, T = np.zeros(9), np.zeros(9), np.zeros(4), np.zeros(4), np.zeros(3), np.zeros(3)
    omL, tL = np.zeros((n, 3)), np.zeros((n, 3))
    xi1, xi2, rms = np.zeros(1), np.zeros(1), ctypes.c_double(0)
    nk, it = ctypes.c_int(0), ctypes.c_int(0)
    idx = np.zeros(n, np.int32)
    _check(lib().mcc_omnidir_stereo_calibrate(n, _ptr(off, _i32p), _ptr(obj, _f64p), _ptr(img1, _f64p),
                                              _ptr(img2, _f64p), int(image_size1[0]), int(image_size1[1]),
                                              int(image_size2[0]), int(image_size2[1]), flags, crit_type, max_count,
                                              eps, device, _ptr(K1, _f64p), _ptr(xi1, _f64p), _ptr(D1, _f64p),
                                              _ptr(K2, _f64p), _ptr(xi2, _f64p), _ptr(D2, _f64p), _ptr(om, _f64p),
                                              _ptr(T, _f64p), _ptr(omL, _f64p), _ptr(tL, _f64p), _ptr(idx, _i32p),
                                              ctypes.byref(nk), ctypes.byref(rms), ctypes.byref(it)),
           "mcc_omnidir_stereo_calibrate")
    k = nk.value
    return (rms.value, K1.reshape(3, 3), float(xi1[0]), D1, K2.reshape(3, 3), float(xi2[0]), D2, om, T, omL[:k],
            tL[:k], idx[:k].copy(), it.value)


# ---------------------------------------------------------------- cv::omnidir rectification
# include/mcc_omnidir.h; the reference's names: cv::omnidir::undistortPoints (src/omnidir.cpp:249-343),
# initUndistortRectifyMap (:348-533), undistortImage (:538-546), stereoRectify (:2190-2227).
RECTIFY_PERSPECTIVE, RECTIFY_CYLINDRICAL, RECTIFY_LONGLATI, RECTIFY_STEREOGRAPHIC = 1, 2, 3, 4
MAP_FLOAT, MAP_FIXED = 1, 2
XYZRGB, XYZ = 1, 2   # cv::omnidir's point types of stereoReconstruct


def _mat3(a, what, vector_ok=False):
    """None, a 3 x 3 matrix (or the first three columns of a 3 x 4 one), or a rotation vector."""
    if a is None:
        return None
    a = np.asarray(a, np.float64)
    if vector_ok and a.size == 3:
        return np.ascontiguousarray(_rig.rodrigues(a.reshape(3)))
    if a.shape == (3, 4):
        a = a[:, :3]
    if a.size != 9:
        raise MccError(f"{what} must be 3 x 3")
    return np.ascontiguousarray(a.reshape(3, 3))


def _vec(a, n, what):
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    if a.size != n:
        raise MccError(f"{what} must hold {n} values")
    return a


def _image(img, what):
    """uint8 [h, w] or [h, w, c] with contiguous pixels (rows may be strided): (array, w, h, c, stride)."""
    if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise MccError(f"{what} must be a uint8 array [h, w] or [h, w, channels]")
    c = 1 if img.ndim == 2 else img.shape[2]
    if img.strides[-1] != 1 or (img.ndim == 3 and img.strides[1] != c) or img.strides[0] < 0:
        img = np.ascontiguousarray(img)
    return img, img.shape[1], img.shape[0], c, img.strides[0]


def omnidir_undistort_points(distorted, K, D, xi, R=None, device=0):
    """cv::omnidir::undistortPoints: pixels [n, 2] -> X/Z, Y/Z [n, 2] of their rays after R (a 3 x 3
    matrix or a rotation vector)."""
    pts = np.ascontiguousarray(distorted, np.float64).reshape(-1, 2)
    K, D, R = _mat3(K, "K"), _vec(D, 4, "D"), _mat3(R, "R", True)
    out = np.zeros_like(pts)
    _check(lib().mcc_omnidir_undistort_points(pts.shape[0], _ptr(pts, _f64p), _ptr(K, _f64p), _ptr(D, _f64p),
                                              float(xi), _ptr(R, _f64p), device, _ptr(out, _f64p)),
           "mcc_omnidir_undistort_points")
    return out


def omnidir_stereo_rectify(R, T):
    """cv::omnidir::stereoRectify: (R1, R2) of the rig whose second camera is at (R, T) -- host code, no GPU."""
    R, T = _mat3(R, "R", True), _vec(T, 3, "T")
    R1, R2 = np.zeros((3, 3)), np.zeros((3, 3))
    _check(lib().mcc_omnidir_stereo_rectify(_ptr(R, _f64p), _ptr(T, _f64p), _ptr(R1, _f64p), _ptr(R2, _f64p)),
           "mcc_omnidir_stereo_rectify")
    return R1, R2


def omnidir_init_undistort_rectify_map(K, D, xi, R, P, size, map_type=MAP_FIXED, flags=RECTIFY_PERSPECTIVE, device=0):
    """cv::omnidir::initUndistortRectifyMap for size = (width, height): MAP_FLOAT gives two float32
    [h, w] maps (u, v), MAP_FIXED int16 [h, w, 2] and uint16 [h, w] (CV_16SC2 + CV_16UC1)."""
    K, D, R, P = _mat3(K, "K"), _vec(D, 4, "D"), _mat3(R, "R", True), _mat3(P, "P")
    w, h = int(size[0]), int(size[1])
    shape = (max(h, 0), max(w, 0))
    if map_type == MAP_FLOAT:
        m1, m2 = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    else:
        m1, m2 = np.zeros(shape + (2,), np.int16), np.zeros(shape, np.uint16)
    _check(lib().mcc_omnidir_init_undistort_rectify_map(_ptr(K, _f64p), _ptr(D, _f64p), float(xi), _ptr(R, _f64p),
                                                        _ptr(P, _f64p), w, h, map_type, flags, device,
                                                        m1.ctypes.data_as(ctypes.c_void_p),
                                                        m2.ctypes.data_as(ctypes.c_void_p)),
           "mcc_omnidir_init_undistort_rectify_map")
    return m1, m2


def _dst_image(dst, w, h, c, squeeze):
    if dst is None:
        dst = np.zeros((h, w) if squeeze else (h, w, c), np.uint8)
    d, dw, dh, dc, stride = _image(dst, "dst")
    if d is not dst or (dw, dh, dc) != (w, h, c):
        raise MccError(f"dst must be a uint8 array of {h} x {w} x {c} with contiguous pixels")
    return dst, stride


def omnidir_remap(src, map1, map2, dst=None, device=0):
    """cv::remap(src, map1, map2, INTER_LINEAR, BORDER_CONSTANT) for fixed-point maps (int16 [h, w, 2],
    uint16 [h, w]) and a uint8 image of 1 or 3 channels.  A given dst (rows may be strided) is written
    in place: only width * channels bytes of each row."""
    src, sw, sh, c, sstride = _image(src, "src")
    map1, map2 = np.ascontiguousarray(map1, np.int16), np.ascontiguousarray(map2, np.uint16)
    if map1.ndim != 3 or map1.shape[2] != 2 or map2.shape != map1.shape[:2]:
        raise MccError("map1 must be int16 [h, w, 2] and map2 uint16 [h, w]")
    h, w = map2.shape
    dst, dstride = _dst_image(dst, w, h, c, src.ndim == 2)
    _check(lib().mcc_omnidir_remap(_ptr(src, _u8p), sw, sh, c, sstride, _ptr(map1, _i16p), _ptr(map2, _u16p), w, h,
                                   _ptr(dst, _u8p), dstride, device), "mcc_omnidir_remap")
    return dst


def omnidir_undistort_image(src, K, D, xi, flags, Knew=None, new_size=None, R=None, dst=None, device=0):
    """cv::omnidir::undistortImage: the fixed-point maps and the remap in one call; new_size =
    (width, height), None for the source size."""
    src, sw, sh, c, sstride = _image(src, "src")
    K, D, Knew, R = _mat3(K, "K"), _vec(D, 4, "D"), _mat3(Knew, "Knew"), _mat3(R, "R", True)
    w, h = (sw, sh) if new_size is None else (int(new_size[0]), int(new_size[1]))
    dst, dstride = _dst_image(dst, w, h, c, src.ndim == 2)
    _check(lib().mcc_omnidir_undistort_image(_ptr(src, _u8p), sw, sh, c, sstride, _ptr(K, _f64p), _ptr(D, _f64p),
                                             float(xi), flags, _ptr(Knew, _f64p), w, h, _ptr(R, _f64p), device,
                                             _ptr(dst, _u8p), dstride), "mcc_omnidir_undistort_image")
    return dst


class OmniRectifier:
    """The per-frame case of undistortImage (mcc_omnirect): the fixed-point maps of (K, D, xi, R, P,
    flags) for dst_size are built once and stay on the device with the two images."""

    def __init__(self, K, D, xi, flags, src_size, channels=1, P=None, dst_size=None, R=None, device=0):
        self._keep = [_mat3(K, "K"), _vec(D, 4, "D"), _mat3(R, "R", True), _mat3(P, "P")]
        self.src_size = (int(src_size[0]), int(src_size[1]))
        self.dst_size = self.src_size if dst_size is None else (int(dst_size[0]), int(dst_size[1]))
        self.channels = int(channels)
        d = _OmniRectDesc()
        d.K, d.D, d.R, d.P = (_ptr(a, _f64p) for a in self._keep)
        d.xi, d.flags, d.device = float(xi), flags, device
        d.dst_width, d.dst_height = self.dst_size
        d.src_width, d.src_height = self.src_size
        d.channels = self.channels
        h = ctypes.c_void_p()
        _check(lib().mcc_omnirect_create(ctypes.byref(h), ctypes.byref(d)), "mcc_omnirect_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().mcc_omnirect_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def remap(self, src, dst=None):
        """One frame (uint8 [h, w] or [h, w, channels] of src_size) through the resident maps."""
        src, sw, sh, c, sstride = _image(src, "src")
        if (sw, sh) != self.src_size or c != self.channels:
            raise MccError(f"src must be {self.src_size[1]} x {self.src_size[0]} x {self.channels}")
        dst, dstride = _dst_image(dst, self.dst_size[0], self.dst_size[1], c, src.ndim == 2)
        _check(lib().mcc_omnirect_remap(self.h, _ptr(src, _u8p), sstride, _ptr(dst, _u8p), dstride),
               "mcc_omnirect_remap")
        return dst

    def time_remap(self, n_frames):
        """Device milliseconds per frame over n_frames back-to-back remap launches on the resident source."""
        ms = ctypes.c_double(0)
        _check(lib().mcc_omnirect_time_remap(self.h, int(n_frames), ctypes.byref(ms)), "mcc_omnirect_time_remap")
        return ms.value


# ---------------------------------------------------------------- pinhole rectification
# include/mcc.h: cv::undistortPoints, cv::initUndistortRectifyMap, cv::undistort, cv::stereoRectify for the K, D, R, T
# of calibrate_camera and stereo_calibrate.
def _dist(D):
    """(D as float64 or None, nd)"""
    if D is None:
        return None, 0
    D = np.ascontiguousarray(D, np.float64).reshape(-1)
    return (D, D.size) if D.size else (None, 0)


def _proj(P, what):
    """(P as a contiguous 3 x 3 or 3 x 4 array or None, its doubles per row)"""
    if P is None:
        return None, 3
    P = np.ascontiguousarray(P, np.float64)
    if P.shape not in ((3, 3), (3, 4)):
        raise MccError(f"{what} must be 3 x 3 or 3 x 4")
    return P, P.shape[1]


def undistort_points(src, K, D=None, R=None, P=None, iterations=20, device=0, return_ms=False):
    """cv::undistortPoints (mcc_undistort_points): pixels [n, 2] -> ideal points [n, 2], after R (a 3 x 3 matrix or a
    rotation vector) and through P (3 x 3 or 3 x 4) when given.  D holds 0, 4, 5, 8 or 12 coefficients.  The inverse
    of the distortion runs `iterations` fixed-point rounds (20, as solve_pnp's; OpenCV runs 5)."""
    pts = np.ascontiguousarray(src, np.float64).reshape(-1, 2)
    K, R = _mat3(K, "K"), _mat3(R, "R", True)
    (D, nd), (P, ld) = _dist(D), _proj(P, "P")
    out, ms = np.zeros_like(pts), np.zeros(1)
    _check(lib().mcc_undistort_points(pts.shape[0], _ptr(pts, _f64p), _ptr(K, _f64p), _ptr(D, _f64p), nd, _ptr(R, _f64p),
                                      _ptr(P, _f64p), ld, int(iterations), device, _ptr(out, _f64p), _ptr(ms, _f64p)),
           "mcc_undistort_points")
    return (out, float(ms[0])) if return_ms else out


def init_undistort_rectify_map(K, D, R, P, size, map_type=MAP_FIXED, device=0, return_ms=False):
    """cv::initUndistortRectifyMap for size = (width, height) (mcc_init_undistort_rectify_map): MAP_FLOAT gives two
    float32 [h, w] maps (u, v), MAP_FIXED int16 [h, w, 2] and uint16 [h, w] (CV_16SC2 + CV_16UC1).  R None is the
    identity, P None is K."""
    K, R = _mat3(K, "K"), _mat3(R, "R", True)
    (D, nd), (P, ld) = _dist(D), _proj(P, "P")
    w, h = int(size[0]), int(size[1])
    shape = (max(h, 0), max(w, 0))
    if map_type == MAP_FLOAT:
        m1, m2 = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
    else:
        m1, m2 = np.zeros(shape + (2,), np.int16), np.zeros(shape, np.uint16)
    ms = np.zeros(1)
    _check(lib().mcc_init_undistort_rectify_map(_ptr(K, _f64p), _ptr(D, _f64p), nd, _ptr(R, _f64p), _ptr(P, _f64p), ld, w, h,
                                                map_type, device, m1.ctypes.data_as(ctypes.c_void_p),
                                                m2.ctypes.data_as(ctypes.c_void_p), _ptr(ms, _f64p)),
           "mcc_init_undistort_rectify_map")
    return (m1, m2, float(ms[0])) if return_ms else (m1, m2)


def stereo_rectify(K1, D1, K2, D2, image_size, R, T, flags=CV_CALIB_ZERO_DISPARITY, alpha=-1.0, new_size=None):
    """cv::stereoRectify (mcc_stereo_rectify; host code, no GPU): (R1, R2, P1 [3, 4], P2 [3, 4], Q [4, 4], roi1, roi2)
    of the pair whose second camera sees X at R X + T; a roi is (x, y, width, height).  D1 and D2 hold the same number
    of coefficients.  flags is 0 or CV_CALIB_ZERO_DISPARITY, alpha negative (keep the focal length) or in 0..1,
    new_size = (width, height) or None for image_size."""
    K1, K2, R, T = _mat3(K1, "K1"), _mat3(K2, "K2"), _mat3(R, "R", True), _vec(T, 3, "T")
    (D1, nd), (D2, nd2) = _dist(D1), _dist(D2)
    if D1 is not None and D2 is not None and nd != nd2:
        raise MccError("stereo_rectify: D1 and D2 must hold the same number of coefficients")
    nw, nh = (0, 0) if new_size is None else (int(new_size[0]), int(new_size[1]))
    R1, R2, P1, P2, Q = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 4)), np.zeros((3, 4)), np.zeros((4, 4))
    roi1, roi2 = np.zeros(4, np.int32), np.zeros(4, np.int32)
    _check(lib().mcc_stereo_rectify(_ptr(K1, _f64p), _ptr(D1, _f64p), _ptr(K2, _f64p), _ptr(D2, _f64p), max(nd, nd2),
                                    int(image_size[0]), int(image_size[1]), _ptr(R, _f64p), _ptr(T, _f64p), int(flags),
                                    float(alpha), nw, nh, *[_ptr(a, _f64p) for a in (R1, R2, P1, P2, Q)],
                                    _ptr(roi1, _i32p), _ptr(roi2, _i32p)), "mcc_stereo_rectify")
    return R1, R2, P1, P2, Q, tuple(int(v) for v in roi1), tuple(int(v) for v in roi2)


def undistort_image(src, K, D=None, Knew=None, new_size=None, R=None, dst=None, device=0):
    """cv::undistort, or with R and Knew = P1 / P2 the remap of one rectified view (mcc_undistort_image): the
    fixed-point maps and the remap in one call; new_size = (width, height), None for the source size."""
    src, sw, sh, c, sstride = _image(src, "src")
    K, R = _mat3(K, "K"), _mat3(R, "R", True)
    (D, nd), (Knew, ld) = _dist(D), _proj(Knew, "Knew")
    w, h = (sw, sh) if new_size is None else (int(new_size[0]), int(new_size[1]))
    dst, dstride = _dst_image(dst, w, h, c, src.ndim == 2)
    _check(lib().mcc_undistort_image(_ptr(src, _u8p), sw, sh, c, sstride, _ptr(K, _f64p), _ptr(D, _f64p), nd, _ptr(R, _f64p),
                                     _ptr(Knew, _f64p), ld, w, h, device, _ptr(dst, _u8p), dstride), "mcc_undistort_image")
    return dst


class PinholeRectifier:
    """The per-frame case of undistort_image (mcc_pinrect): the fixed-point maps of (K, D, R, P) for dst_size are built
    once and stay on the device with the two images."""

    def __init__(self, K, D, src_size, channels=1, R=None, P=None, dst_size=None, device=0):
        (D, nd), (P, ld) = _dist(D), _proj(P, "P")
        self._keep = [_mat3(K, "K"), D, _mat3(R, "R", True), P]
        self.src_size = (int(src_size[0]), int(src_size[1]))
        self.dst_size = self.src_size if dst_size is None else (int(dst_size[0]), int(dst_size[1]))
        self.channels = int(channels)
        d = _PinRectDesc()
        d.K, d.D, d.R, d.P = (_ptr(a, _f64p) for a in self._keep)
        d.nd, d.ld, d.device = nd, ld, device
        d.dst_width, d.dst_height = self.dst_size
        d.src_width, d.src_height = self.src_size
        d.channels = self.channels
        h = ctypes.c_void_p()
        _check(lib().mcc_pinrect_create(ctypes.byref(h), ctypes.byref(d)), "mcc_pinrect_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().mcc_pinrect_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def remap(self, src, dst=None):
        """One frame (uint8 [h, w] or [h, w, channels] of src_size) through the resident maps."""
        src, sw, sh, c, sstride = _image(src, "src")
        if (sw, sh) != self.src_size or c != self.channels:
            raise MccError(f"src must be {self.src_size[1]} x {self.src_size[0]} x {self.channels}")
        dst, dstride = _dst_image(dst, self.dst_size[0], self.dst_size[1], c, src.ndim == 2)
        _check(lib().mcc_pinrect_remap(self.h, _ptr(src, _u8p), sstride, _ptr(dst, _u8p), dstride), "mcc_pinrect_remap")
        return dst


def omnidir_sgbm(left, right, num_disparities, sad_window_size, device=0):
    """The semi-global matcher of stereoReconstruct alone (tests/npsgbm.py) on a rectified
    uint8 pair of 1 or 3 channels: int16 [h, w], disparity x 16, -16 where there is none."""
    left, w, h, c, ls = _image(left, "left")
    right, w2, h2, c2, rs = _image(right, "right")
    disp = np.zeros((max(h, 0), max(w, 0)), np.int16)
    _check(lib().mcc_omnidir_sgbm(_ptr(left, _u8p), w, h, c, ls, _ptr(right, _u8p), w2, h2, c2, rs, int(num_disparities),
                                  int(sad_window_size), device, _ptr(disp, _i16p)), "mcc_omnidir_sgbm")
    return disp


class OmniReconstructor:
    """The per-frame case of stereoReconstruct (mcc_omnirecon): both cameras' fixed-point maps, the
    images, the cost volumes and the cloud stay on the device for a stream of frame pairs.

    new_size = (width, height), or None for the reference's empty newSize: the rectified images take
    the source size and the cloud is empty, because the reference's cloud loop runs over newSize."""

    def __init__(self, K1, D1, xi1, K2, D2, xi2, R, T, flag, num_disparities, sad_window_size, src_size, channels=1,
                 new_size=None, Knew=None, point_type=XYZRGB, device=0):
        self._keep = [_mat3(K1, "K1"), _vec(D1, 4, "D1"), _mat3(K2, "K2"), _vec(D2, 4, "D2"), _mat3(R, "R", True),
                      _vec(T, 3, "T"), _mat3(Knew, "Knew")]
        self.src_size = (int(src_size[0]), int(src_size[1]))
        self.out_size = self.src_size if new_size is None else (int(new_size[0]), int(new_size[1]))
        self.channels, self.point_type = int(channels), int(point_type)
        d = _OmniReconDesc()
        d.K1, d.D1, d.K2, d.D2, d.R, d.T, d.Knew = (_ptr(a, _f64p) for a in self._keep)
        d.xi1, d.xi2, d.flag, d.device = float(xi1), float(xi2), int(flag), device
        d.num_disparities, d.sad_window_size = int(num_disparities), int(sad_window_size)
        d.src_width, d.src_height = self.src_size
        d.new_width, d.new_height = (0, 0) if new_size is None else self.out_size
        d.channels, d.point_type = self.channels, self.point_type
        h = ctypes.c_void_p()
        _check(lib().mcc_omnirecon_create(ctypes.byref(h), ctypes.byref(d)), "mcc_omnirecon_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib().mcc_omnirecon_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def compute(self, image1, image2, capacity=None):
        """One frame pair -> (disparity float32 [h, w], rec1, rec2, cloud float32 [n, 3 or 6]).  capacity
        bounds the number of points (default: every pixel); too small a one raises MccError."""
        image1, w1, h1, c1, s1 = _image(image1, "image1")
        image2, w2, h2, c2, s2 = _image(image2, "image2")
        if (w1, h1) != self.src_size or (w2, h2) != self.src_size or c1 != self.channels or c2 != self.channels:
            raise MccError(f"both images must be {self.src_size[1]} x {self.src_size[0]} x {self.channels}")
        w, h = self.out_size
        nf = 3 if self.point_type == XYZ else 6
        cap = w * h if capacity is None else int(capacity)
        disp = np.zeros((h, w), np.float32)
        rec1, rs1 = _dst_image(None, w, h, c1, image1.ndim == 2)
        rec2, rs2 = _dst_image(None, w, h, c1, image1.ndim == 2)
        cloud = np.zeros((max(cap, 0), nf), np.float32)
        n = ctypes.c_longlong(0)
        _check(lib().mcc_omnirecon_compute(self.h, _ptr(image1, _u8p), s1, _ptr(image2, _u8p), s2, _ptr(disp, _f32p),
                                           _ptr(rec1, _u8p), rs1, _ptr(rec2, _u8p), rs2,
                                           _ptr(cloud, _f32p) if cap > 0 else None, cap, ctypes.byref(n)),
               "mcc_omnirecon_compute")
        return disp, rec1, rec2, cloud[:n.value].copy()

    def time(self, n_frames):
        """Device milliseconds per frame pair over n_frames back-to-back computes on resident random frames."""
        ms = ctypes.c_double(0)
        _check(lib().mcc_omnirecon_time(self.h, int(n_frames), ctypes.byref(ms)), "mcc_omnirecon_time")
        return ms.value


def omnidir_stereo_reconstruct(image1, image2, K1, D1, xi1, K2, D2, xi2, R, T, flag, num_disparities, sad_window_size,
                               new_size=None, Knew=None, point_type=XYZRGB, capacity=None, device=0):
    """cv::omnidir::stereoReconstruct: (disparity, image1Rec, image2Rec, pointCloud).  R is a 3 x 3 matrix
    or a rotation vector; new_size and capacity as OmniReconstructor."""
    image1, w, h, c, _ = _image(image1, "image1")
    image2, w2, h2, c2, _ = _image(image2, "image2")
    if (w2, h2, c2) != (w, h, c):
        raise MccError("the two images must have the same size and number of channels")
    rec = OmniReconstructor(K1, D1, xi1, K2, D2, xi2, R, T, flag, num_disparities, sad_window_size, (w, h), c, new_size,
                            Knew, point_type, device)
    try:
        return rec.compute(image1, image2, capacity)
    finally:
        rec.close()


# ---------------------------------------------------------------- pinhole reconstruction
# include/mcc.h: cv::reprojectImageTo3D and a rectified pinhole pair to depth, for the K, D, R, T of stereo_calibrate.
def reproject_image_to_3d(disparity, Q, handle_missing=False, device=0, return_ms=False):
    """cv::reprojectImageTo3D (mcc_reproject_image_to_3d): float32 [h, w, 3] = Q (x, y, d, 1) dehomogenised, per pixel
    of a float32 disparity [h, w] or of an int16 one, which holds disparity x 16 as the matcher writes it and is
    divided by 16 here (OpenCV takes a CV_16S disparity raw).  Rows may be strided.  With handle_missing every pixel
    at the image's minimum gets Z = 10000."""
    d = disparity
    if not isinstance(d, np.ndarray) or d.ndim != 2 or d.dtype not in (np.float32, np.int16):
        raise MccError("disparity must be a float32 or int16 array [h, w]")
    if d.strides[1] != d.itemsize or d.strides[0] < 0:
        d = np.ascontiguousarray(d)
    h, w = d.shape
    Q = np.ascontiguousarray(Q, np.float64)
    if Q.shape != (4, 4):
        raise MccError("Q must be 4 x 4")
    out, ms = np.zeros((max(h, 0), max(w, 0), 3), np.float32), np.zeros(1)
    _check(lib().mcc_reproject_image_to_3d(d.ctypes.data_as(ctypes.c_void_p), DISP_FLOAT if d.dtype == np.float32 else DISP_FIXED16,
                                           w, h, d.strides[0], _ptr(Q, _f64p), int(bool(handle_missing)), device,
                                           _ptr(out, _f32p), _ptr(ms, _f64p)), "mcc_reproject_image_to_3d")
    return (out, float(ms[0])) if return_ms else out


def _geometry(g):
    """mcc_pinrecon_geometry as a dict of arrays"""
    return dict(R1=np.array(g.R1).reshape(3, 3), R2=np.array(g.R2).reshape(3, 3), P1=np.array(g.P1).reshape(3, 4),
                P2=np.array(g.P2).reshape(3, 4), Q=np.array(g.Q).reshape(4, 4), roi1=tuple(g.roi1), roi2=tuple(g.roi2),
                size=(g.width, g.height), transposed=bool(g.transposed))


def pinhole_cloud_host(disparity, Q, rec1=None, point_type=XYZ, roi=None, max_z=0.0):
    """The cloud rule of 7j on the host (mcc_pinrecon_host_cloud; no GPU), through the function the device's count and
    write kernels compile: float32 [n, 3 or 6] of a float32 disparity [h, w]."""
    d = np.ascontiguousarray(disparity, np.float32)
    h, w = d.shape
    Q = np.ascontiguousarray(Q, np.float64).reshape(4, 4)
    c = 1
    if rec1 is not None:
        rec1, rw, rh, c, _ = _image(np.ascontiguousarray(rec1), "rec1")
        if (rw, rh) != (w, h):
            raise MccError("rec1 must have the disparity's size")
    roi = None if roi is None else np.ascontiguousarray(roi, np.int32)
    nf = 3 if point_type == XYZ else 6
    cloud = np.zeros((w * h, nf), np.float32)
    n = ctypes.c_longlong(0)
    _check(lib().mcc_pinrecon_host_cloud(_ptr(d, _f32p), w, h, _ptr(Q, _f64p), _ptr(rec1, _u8p), c, int(point_type),
                                         _ptr(roi, _i32p), float(max_z), _ptr(cloud, _f32p), w * h, ctypes.byref(n)),
           "mcc_pinrecon_host_cloud")
    return cloud[:n.value].copy()


def _pinrecon_desc(K1, D1, K2, D2, R, T, num_disparities, sad_window_size, src_size, channels, flags, alpha, new_size,
                   point_type, use_roi, max_z, device):
    """(mcc_pinrecon_desc, the arrays it points into)"""
    (D1, nd), (D2, nd2) = _dist(D1), _dist(D2)
    if D1 is not None and D2 is not None and nd != nd2:
        raise MccError("D1 and D2 must hold the same number of coefficients")
    keep = [_mat3(K1, "K1"), D1, _mat3(K2, "K2"), D2, _mat3(R, "R", True), _vec(T, 3, "T")]
    d = _PinReconDesc()
    d.K1, d.D1, d.K2, d.D2, d.R, d.T = (_ptr(a, _f64p) for a in keep)
    d.nd, d.device = max(nd, nd2), int(device)
    d.src_width, d.src_height = int(src_size[0]), int(src_size[1])
    d.channels, d.point_type = int(channels), int(point_type)
    d.rectify_flags, d.alpha = int(flags), float(alpha)
    d.new_width, d.new_height = (0, 0) if new_size is None else (int(new_size[0]), int(new_size[1]))
    d.num_disparities, d.sad_window_size = int(num_disparities), int(sad_window_size)
    d.use_roi, d.max_z = int(bool(use_roi)), float(max_z)
    return d, keep


class _PinReconOutputs:
    """the host buffers of one compute for outputs of out_size = (width, height)"""

    def __init__(self, out_size, channels, point_type, squeeze, capacity, dense):
        w, h = out_size
        self.cap = w * h if capacity is None else int(capacity)
        self.disp, self.disp16 = np.zeros((h, w), np.float32), np.zeros((h, w), np.int16)
        (self.rec1, self.rs1), (self.rec2, self.rs2) = (_dst_image(None, w, h, channels, squeeze) for _ in range(2))
        self.points = np.zeros((h, w, 3), np.float32) if dense else None
        self.cloud = np.zeros((max(self.cap, 0), 3 if point_type == XYZ else 6), np.float32)
        self.n = ctypes.c_longlong(0)

    def args(self):
        return [_ptr(self.disp, _f32p), _ptr(self.disp16, _i16p), _ptr(self.rec1, _u8p), self.rs1, _ptr(self.rec2, _u8p),
                self.rs2, _ptr(self.points, _f32p), _ptr(self.cloud, _f32p) if self.cap > 0 else None, self.cap,
                ctypes.byref(self.n)]

    def result(self, **extra):
        return dict(disparity=self.disp, disparity16=self.disp16, rec1=self.rec1, rec2=self.rec2, points=self.points,
                    cloud=self.cloud[:self.n.value].copy(), **extra)


class PinholeReconstructor:
    """The per-pair case of stereo_reconstruct (mcc_pinrecon): stereo_rectify's result, both cameras' fixed-point maps,
    the images, the matcher's volumes, the dense points and the cloud stay on the device for a stream of frame pairs.

    Camera 2 must lie to the right of camera 1 after rectification (below it for a vertical pair).  A vertical pair
    comes out in the transposed frame: info()["transposed"], and every output has info()["size"] = (width, height)."""

    def __init__(self, K1, D1, K2, D2, R, T, num_disparities, sad_window_size, src_size, channels=1,
                 flags=CV_CALIB_ZERO_DISPARITY, alpha=-1.0, new_size=None, point_type=XYZRGB, use_roi=False, max_z=0.0,
                 device=0):
        d, self._keep = _pinrecon_desc(K1, D1, K2, D2, R, T, num_disparities, sad_window_size, src_size, channels, flags,
                                       alpha, new_size, point_type, use_roi, max_z, device)
        self.src_size, self.channels, self.point_type = (d.src_width, d.src_height), d.channels, d.point_type
        h = ctypes.c_void_p()
        _check(lib().mcc_pinrecon_create(ctypes.byref(h), ctypes.byref(d)), "mcc_pinrecon_create")
        self.h = h
        g = _PinReconGeometry()
        _check(lib().mcc_pinrecon_info(self.h, ctypes.byref(g)), "mcc_pinrecon_info")
        self._info = _geometry(g)
        self.out_size = self._info["size"]

    def close(self):
        if getattr(self, "h", None):
            lib().mcc_pinrecon_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """R1 R2 P1 P2 Q roi1 roi2 in the frame of the outputs, their size (width, height) and `transposed`."""
        return dict(self._info)

    def compute(self, image1, image2, capacity=None, dense=True):
        """One frame pair -> dict(disparity float32 [h, w], disparity16 int16 [h, w] (x 16, -16: no match), rec1, rec2,
        points float32 [h, w, 3] (None without dense), cloud float32 [n, 3 or 6]).  capacity bounds the number of points
        (default: every pixel); too small a one raises MccError."""
        image1, w1, h1, c1, s1 = _image(image1, "image1")
        image2, w2, h2, c2, s2 = _image(image2, "image2")
        if (w1, h1) != self.src_size or (w2, h2) != self.src_size or c1 != self.channels or c2 != self.channels:
            raise MccError(f"both images must be {self.src_size[1]} x {self.src_size[0]} x {self.channels}")
        o = _PinReconOutputs(self.out_size, self.channels, self.point_type, image1.ndim == 2, capacity, dense)
        _check(lib().mcc_pinrecon_compute(self.h, _ptr(image1, _u8p), s1, _ptr(image2, _u8p), s2, *o.args()),
               "mcc_pinrecon_compute")
        return o.result()

    def time(self, n_frames):
        """Device milliseconds per frame pair over n_frames back-to-back computes on resident random frames."""
        ms = ctypes.c_double(0)
        _check(lib().mcc_pinrecon_time(self.h, int(n_frames), ctypes.byref(ms)), "mcc_pinrecon_time")
        return ms.value


def stereo_reconstruct(image1, image2, K1, D1, K2, D2, R, T, num_disparities, sad_window_size,
                       flags=CV_CALIB_ZERO_DISPARITY, alpha=-1.0, new_size=None, point_type=XYZRGB, use_roi=False, max_z=0.0,
                       capacity=None, dense=True, device=0):
    """A rectified pair to depth in one call (mcc_stereo_reconstruct, a handle used once): PinholeReconstructor.compute's
    dict plus "info".  The arguments are PinholeReconstructor's."""
    image1, w, h, c, s1 = _image(image1, "image1")
    image2, w2, h2, c2, s2 = _image(image2, "image2")
    d, keep = _pinrecon_desc(K1, D1, K2, D2, R, T, num_disparities, sad_window_size, (w, h), c, flags, alpha, new_size,
                             point_type, use_roi, max_z, device)
    # the size of the outputs: the new size, transposed for a vertical pair (stereo_rectify is host code)
    P2 = stereo_rectify(keep[0], keep[1], keep[2], keep[3], (w, h), keep[4], keep[5], flags, alpha, new_size)[3]
    W, H = (w, h) if new_size is None else (d.new_width, d.new_height)
    o = _PinReconOutputs((W, H) if P2[0, 3] != 0 else (H, W), c, d.point_type, image1.ndim == 2, capacity, dense)
    g = _PinReconGeometry()
    _check(lib().mcc_stereo_reconstruct(_ptr(image1, _u8p), w, h, c, s1, _ptr(image2, _u8p), w2, h2, c2, s2, ctypes.byref(d),
                                        ctypes.byref(g), *o.args()), "mcc_stereo_reconstruct")
    return o.result(info=_geometry(g))
