"""ctypes binding of the CPU restatement of cv::StereoSGBM (oracle/libsgbm_ref.so). TEST INFRASTRUCTURE ONLY.

compute() runs sgbm_ref.c (costs, paths, selection, LR check, median) and then the block matcher's speckle restatement
(sbm_oracle.filter_speckles) with newVal = (minDisparity - 1) * 16 and maxDiff = 16 * speckleRange, as
cv::StereoSGBM::compute does.
"""
import ctypes

import numpy as np

import oracle_lib
import sbm_oracle

_LIB = None

MODE_SGBM, MODE_HH, MODE_SGBM_3WAY, MODE_HH4 = 0, 1, 2, 3
READ_NO_MEDIAN, READ_BOTTOM_CLAMPED = 32, 64


class SgbmParams(ctypes.Structure):
    """Mirror of `sbm_sgbm_params` (include/sbm.h)."""

    _fields_ = [(n, ctypes.c_int32) for n in ("min_disparity", "num_disparities", "block_size", "p1", "p2", "disp12_max_diff",
                                                "prefilter_cap", "uniqueness_ratio", "speckle_window_size", "speckle_range", "mode")]


def make_params(minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0, uniquenessRatio=0,
                speckleWindowSize=0, speckleRange=0, mode=MODE_SGBM):
    """cv::StereoSGBM::create argument order and defaults."""
    return SgbmParams(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio,
                      speckleWindowSize, speckleRange, mode)


def effective(p):
    """The values computeDisparitySGBM works with."""
    P1 = p.p1 if p.p1 > 0 else 2
    return dict(bs=2 * ((p.block_size if p.block_size > 0 else 5) // 2) + 1, ftzero=max(p.prefilter_cap, 15) | 1, P1=P1,
                P2=max(p.p2 if p.p2 > 0 else 5, P1 + 1), uniq=p.uniqueness_ratio if p.uniqueness_ratio >= 0 else 10,
                d12=p.disp12_max_diff if p.disp12_max_diff > 0 else 1)


def envelope(p):
    e = effective(p)
    return e["bs"] ** 2 * (2 * e["ftzero"] + 63) + e["P2"]


def width1(p, w):
    return w + min(p.min_disparity, 0) - max(p.min_disparity + p.num_disparities, 0)


def lib():
    global _LIB
    if _LIB is None:
        L = oracle_lib.load("libsgbm_ref.so")
        vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        L.sgbmr_compute.argtypes = [ctypes.POINTER(SgbmParams), vp, sz, vp, sz, ci, ci, vp, vp, vp, vp, ci]
        L.sgbmr_compute.restype = ci
        _LIB = L
    return _LIB


def compute(p, left, right, reading=0, stages=False, pre_only=False):
    """cv::StereoSGBM::compute restated. Returns the int16 map, or (map, dict(C, S, pre)) with stages=True; C and S are
    (H, width1, numDisparities) int16 (None when width1 < 1). pre_only=True returns (map, pre) and keeps no C or S volume on
    the host (MODE_SGBM then holds one row of them)."""
    left = np.ascontiguousarray(left, dtype=np.uint8)
    right = np.ascontiguousarray(right, dtype=np.uint8)
    assert left.shape == right.shape and left.ndim == 2
    assert p.mode in (MODE_SGBM, MODE_HH) and p.num_disparities > 0 and p.num_disparities % 16 == 0
    assert envelope(p) <= 32767 and p.prefilter_cap <= 63, "outside the exactness envelope"
    h, w = left.shape
    disp = np.empty((h, w), np.int16)
    w1 = width1(p, w)
    C = S = None
    if stages and w1 >= 1:
        C = np.empty((h, w1, p.num_disparities), np.int16)
        S = np.empty_like(C)
    pre = np.empty((h, w), np.int16)
    st = lib().sgbmr_compute(ctypes.byref(p), left.ctypes.data, w, right.ctypes.data, w, w, h, disp.ctypes.data,
                             None if C is None else C.ctypes.data, None if S is None else S.ctypes.data, pre.ctypes.data, reading)
    if st != 0:
        raise MemoryError("sgbmr_compute could not allocate its buffers")
    if p.speckle_window_size > 0:
        disp = sbm_oracle.filter_speckles(disp, (p.min_disparity - 1) * 16, p.speckle_window_size, 16 * p.speckle_range)
    if stages:
        return disp, dict(C=C, S=S, pre=pre)
    if pre_only:
        return disp, pre
    return disp
