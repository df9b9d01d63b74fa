"""The reference's own LK tracker, executed: oracle/_ref/liblk_reference.so is calcOpticalFlowPyrLKStereo compiled from the
reference tree (src/slam/src/opencv/CvLKStereo.cpp) against the OpenCV stand-in of tests/cpp/mock_opencv, with
oracle/lk_reference_driver.cpp for the padded pyramid planes (oracle/Makefile). TEST INFRASTRUCTURE ONLY.

It pins the TRACKER given the pyramid: the levels and derivative planes come from lk_stereo_ref.pyramid and stay RECALLED. The
disparity gate of computeCorrespondences is not part of it.

    available()                        (True, "") or (False, why): the library is there, or it is not and neither is the tree
    track(left, right, pts, params)    -> (right_pts, status, err), calcOpticalFlowPyrLKStereo's own outputs (no gate);
                                       criteria_type is cv::TermCriteria's type (COUNT | EPS, as computeCorrespondences sets it)

The library is built where the reference tree is present and travels with the working tree elsewhere; this module never reads the
reference tree. Where the tree is present and the library cannot be built, loading raises: that is a failure, not a skip.
"""
import ctypes
import pathlib
import re

import numpy as np

import lk_stereo_ref
import oracle_lib

NAME = "_ref/liblk_reference.so"
COUNT, EPS = 1, 2
_LIB = None


def _source():
    """The tracker's source file, by the Makefile's own default (or its override in the environment, as make reads it)."""
    import os

    d = os.environ.get("REFERENCE_DIR")
    if d is None:
        d = re.search(r"^REFERENCE_DIR \?= (.*)$", (oracle_lib.HERE / "Makefile").read_text(), re.M).group(1).strip()
    return pathlib.Path(d) / "src" / "slam" / "src" / "opencv" / "CvLKStereo.cpp"


def available():
    try:
        tree = _source().exists()
    except OSError:
        tree = False
    if (oracle_lib.HERE / NAME).exists() or tree:
        return True, ""
    return False, "oracle/_ref/liblk_reference.so is not built and there is no reference tree to build it from"


def lib():
    global _LIB
    if _LIB is None:
        ok, why = available()
        if not ok:
            raise FileNotFoundError(why)
        path = oracle_lib.make(NAME)          # a no-op without the tree; with it, the Makefile decides what is stale
        if not path.exists():
            raise RuntimeError("the reference tree is present and oracle/_ref/liblk_reference.so was not built")
        L = ctypes.CDLL(str(path))
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.lk_reference_track.argtypes = [vp, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, cd, ci, cd, vp, vp, vp]
        _LIB = L
    return _LIB


def track(left, right, pts, p=None, criteria_type=COUNT | EPS):
    p = p or lk_stereo_ref.params()
    pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 2))
    lv, dv = lk_stereo_ref.pyramid(left, p)
    rv, _ = lk_stereo_ref.pyramid(right, p, with_deriv=False)
    lw = np.array([a.shape[1] for a in lv], np.int32)
    lh = np.array([a.shape[0] for a in lv], np.int32)
    fl = np.concatenate([a.reshape(-1) for a in lv])
    fr = np.concatenate([a.reshape(-1) for a in rv])
    fd = np.concatenate([a.reshape(-1) for a in dv])
    n = len(pts)
    out = np.zeros((n, 2), np.float32)
    status = np.zeros(n, np.uint8)
    err = np.zeros(n, np.float32)
    r = lib().lk_reference_track(fl.ctypes.data, fr.ctypes.data, fd.ctypes.data, lw.ctypes.data, lh.ctypes.data, len(lv),
                                 pts.ctypes.data, n, p.win_width, p.win_height, p.max_level, criteria_type, p.max_count,
                                 float(p.epsilon), p.flags, p.min_eig_threshold, out.ctypes.data, status.ctypes.data, err.ctypes.data)
    if r != 0:
        raise RuntimeError("calcOpticalFlowPyrLKStereo raised an assertion")
    return out, status, err
