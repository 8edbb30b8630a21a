"""Generates the cv::omnidir::calibrate fixtures tests/golden/omnidir/*.npz.

Run from the repo root:
    python tests/golden/make_golden_omnidir.py

Inputs:
  omni_calib_data ... the reference's own real corner data, tutorials/data/omni_calib_data.xml
                      (kept as tests/golden/tutorial/omni_calib_data.xml)
                      (15 views of a 9x6 board, 1280x960; pattern points CV_64F, image points as
                      stored), the data tutorials/omnidir_tutorial.markdown:40-49 calibrates with
                      TermCriteria(COUNT + EPS, 200, 1e-4) and flags 0;
  synth_v16 ......... 16 synthetic views of an 11x8 board seen by a config-4 Mei camera
                      (rig.make_omni_views, seed 4), calibrated with the loadImages criteria
                      (COUNT + EPS, 300, 1e-7, src/multicalib.cpp:275-277);
  synth_v16_fix ..... the same views with CALIB_FIX_SKEW + CALIB_FIX_P1 + CALIB_FIX_P2 (the
                      flags2idx / fillFixed path).
Outputs are the CPU oracle's (oracle/mcc_oracle_omnicalib.c): initializeCalibration (init_*),
computeJacobian's JTE and the loop's G at iteration 0 and 7 from the initial parameters
(jte0, G0, G7), and calibrate (rms, K, xi, D, om, t, idx, iters).  The reference itself needs
OpenCV and is unbuildable here, so these vectors freeze the restatement (parity against OpenCV
is unpinned; the restatement is pinned by finite differences and the reference's own data).
"""
import os
import sys
import xml.etree.ElementTree as ET

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from multi_camera_calibration_amd import rig  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "omnidir")
TUTORIAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tutorial", "omni_calib_data.xml")


def read_opencv_mats(path, key):
    """A FileStorage sequence of opencv-matrix nodes -> list of (rows*cols, channels) float64."""
    root = ET.parse(path).getroot()
    out = []
    for m in root.find(key):
        rows, cols = int(m.find("rows").text), int(m.find("cols").text)
        dt = m.find("dt").text.strip().strip('"')
        ch = int(dt[0]) if dt[0].isdigit() else 1
        out.append(np.array(m.find("data").text.split(), np.float64).reshape(rows * cols, ch))
    return out


def tutorial_inputs():
    obj = read_opencv_mats(TUTORIAL, "objectPoints")
    img = read_opencv_mats(TUTORIAL, "imagePoints")
    size = tuple(int(v) for v in ET.parse(TUTORIAL).getroot().find("imageSize").text.split())
    off = np.cumsum([0] + [len(o) for o in obj]).astype(np.int32)
    return off, np.concatenate(obj), np.concatenate(img), size


def generate(off, obj, img, size, flags, crit):
    v = O.OmniViews(off, obj, img)
    out = dict(off=off, obj=obj, img=img, image_size=np.array(size, np.int64), flags=np.int64(flags),
               crit=np.array(crit[:2], np.int64), crit_eps=np.float64(crit[2]))
    om, t, K, xi, idx = O.omni_init(v, *size)
    out.update(init_om=om, init_t=t, init_K=K, init_xi=np.float64(xi), init_idx=idx)
    vk = v.subset(idx)
    p0 = O.omni_encode(om, t, K, xi)
    out["p0"] = p0
    out["jte0"] = O.omni_jacobian(vk, p0, flags, 0.0, inverse=False)[0]
    out["G0"] = O.omni_step(vk, p0, flags, 0)
    out["G7"] = O.omni_step(vk, p0, flags, 7)
    rms, K, xi, D, om, t, idx, iters = O.omni_calibrate(v, *size, flags, *crit)
    out.update(rms=np.float64(rms), K=K, xi=np.float64(xi), D=D, om=om, t=t, idx=idx, iters=np.int64(iters))
    return out


def cases():
    yield "omni_calib_data", tutorial_inputs(), 0, (3, 200, 1e-4)
    s = rig.make_omni_views(16, seed=4)
    yield "synth_v16", (s.off, s.obj, s.img, s.image_size), 0, (3, 300, 1e-7)
    yield "synth_v16_fix", (s.off, s.obj, s.img, s.image_size), 2 + 16 + 32, (3, 300, 1e-7)


def main():
    os.makedirs(HERE, exist_ok=True)
    for name, (off, obj, img, size), flags, crit in cases():
        out = generate(off, obj, img, size, flags, crit)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: views={len(off) - 1} kept={len(out['idx'])} iters={int(out['iters'])} "
              f"rms={float(out['rms']):.6f} -> {os.path.getsize(path) // 1024} KiB")


if __name__ == "__main__":
    main()
