"""The sequential CPU restatement of the reference's DEPTH_METHOD_CV_LK path (include/sbm.h, "pyramidal LK stereo"):
oracle/liblk_stereo_ref.so (from oracle/lk_stereo_ref.c) through ctypes, and an independent numpy transcription of the
RECALLED half (the pyramid of cv::buildOpticalFlowPyramid) that the C file is held to.
TEST INFRASTRUCTURE ONLY.

    params(...)                                   the reference's constants by default (lk_ref_params)
    levels(w, h, p) / level_sizes(w, h, p)        index of the last level / [(w_l, h_l)] of every level
    pyramid(img, p) / pyramid_np(img, p)          -> ([uint8 (h_l, w_l)], [int16 (h_l, w_l, 2)]) per level
    track(left, right, pts, p)                    the tracker without the gate -> (right_pts, status, err, info, hist);
                                                  info[:, 0] is the level-0 exit (CONVERGED ... OSCILLATION), info[:, 1] its
                                                  iterations; hist[level, iterations] counts points
    correspondences(left, right, pts, p)          tracker and gate -> (right_pts, status, err)
    keypoints3d(pts, right_pts, status, model, min_depth, max_depth)   -> float32 (n, 3), NaN where invalid
"""
import ctypes

import numpy as np

import oracle_lib
from sbm_oracle import StereoModel

GET_MIN_EIGENVALS = 8
CONVERGED, PREV_OUT, MIN_EIG, NEXT_OUT, MAX_COUNT, OSCILLATION = range(6)
MAX_LEVELS = 16
_LIB = None


class Params(ctypes.Structure):
    _fields_ = [("win_width", ctypes.c_int32), ("win_height", ctypes.c_int32), ("max_level", ctypes.c_int32),
                ("max_count", ctypes.c_int32), ("epsilon", ctypes.c_float), ("flags", ctypes.c_int32),
                ("min_eig_threshold", ctypes.c_double), ("min_disparity", ctypes.c_float), ("max_disparity", ctypes.c_float)]


def params(win_width=15, win_height=3, max_level=5, max_count=30, epsilon=0.01, flags=GET_MIN_EIGENVALS, min_eig_threshold=1e-4,
           min_disparity=0.5, max_disparity=128.0):
    return Params(win_width, win_height, max_level, max_count, epsilon, flags, min_eig_threshold, min_disparity, max_disparity)


def lib():
    global _LIB
    if _LIB is None:
        L = oracle_lib.load("liblk_stereo_ref.so")
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        pp = ctypes.POINTER(Params)
        L.lk_ref_levels.argtypes = [ci, ci, ci, ci, ci]
        L.lk_ref_pyramid.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp]
        L.lk_ref_track.argtypes = [vp, vp, ci, ci, vp, ci, pp, vp, vp, vp, vp, vp]
        L.lk_ref_gate.argtypes = [vp, vp, vp, ci, cf, cf]
        L.lk_ref_gate.restype = None
        L.lk_ref_correspondences.argtypes = [vp, vp, ci, ci, vp, ci, pp, vp, vp, vp]
        L.lk_ref_keypoints3d.argtypes = [vp, vp, vp, ci, ctypes.POINTER(StereoModel), cf, cf, vp]
        L.lk_ref_keypoints3d.restype = None
        _LIB = L
    return _LIB


def _img(img):
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 2 or img.shape[0] < 2 or img.shape[1] < 2:
        raise ValueError("img must be an (H, W) uint8 array, at least 2 x 2")
    return img


def _pts(pts):
    return np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 2))


def level_sizes(w, h, p=None):
    """[(w_l, h_l)] of the levels buildOpticalFlowPyramid keeps (written here from the header's text, not through the C file)."""
    p = p or params()
    out = [(w, h)]
    while len(out) <= p.max_level:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= p.win_width or h <= p.win_height:
            break
        out.append((w, h))
    return out


def levels(w, h, p=None):
    p = p or params()
    return lib().lk_ref_levels(w, h, p.win_width, p.win_height, p.max_level)


def pyramid(img, p=None, with_deriv=True):
    """The C restatement: ([level planes], [derivative planes]) (the second list empty without with_deriv)."""
    p = p or params()
    img = _img(img)
    h, w = img.shape
    sizes = level_sizes(w, h, p)
    total = sum(a * b for a, b in sizes)
    lv = np.zeros(total, np.uint8)
    dv = np.zeros(total * 2, np.int16) if with_deriv else None
    L = lib().lk_ref_pyramid(img.ctypes.data, w, h, p.win_width, p.win_height, p.max_level, lv.ctypes.data,
                             dv.ctypes.data if with_deriv else None)
    assert L == len(sizes) - 1, (L, sizes)
    planes, ders, off = [], [], 0
    for lw, lh in sizes:
        planes.append(lv[off:off + lw * lh].reshape(lh, lw).copy())
        if with_deriv:
            ders.append(dv[2 * off:2 * (off + lw * lh)].reshape(lh, lw, 2).copy())
        off += lw * lh
    return planes, ders


# ---- the numpy transcription of the RECALLED text ---------------------------------------------------------------------------
def _reflect_index(i, n):
    """BORDER_REFLECT_101 of an index array into [0, n)."""
    i = np.asarray(i).copy()
    if n == 1:
        return np.zeros_like(i)
    for _ in range(64):
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * n - 2 - i, i)
        if ((i >= 0) & (i < n)).all():
            return i
    raise AssertionError("reflection did not settle")


def pyr_down_np(src):
    """(s + 128) >> 8 of the separable [1 4 6 4 1] at the even samples, BORDER_REFLECT_101."""
    h, w = src.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    s = src.astype(np.int64)
    rows = sum(k * s[:, _reflect_index(2 * np.arange(dw) + i - 2, w)] for i, k in enumerate((1, 4, 6, 4, 1)))
    both = sum(k * rows[_reflect_index(2 * np.arange(dh) + j - 2, h), :] for j, k in enumerate((1, 4, 6, 4, 1)))
    return ((both + 128) >> 8).astype(np.uint8)


def scharr_np(src):
    """int16 (h, w, 2): (dx, dy), taps (3, 10, 3) x (-1, 0, 1), BORDER_REFLECT_101."""
    h, w = src.shape
    s = src.astype(np.int64)
    ys, xs = np.arange(h), np.arange(w)
    up, dn = s[_reflect_index(ys - 1, h), :], s[_reflect_index(ys + 1, h), :]
    lf, rt = _reflect_index(xs - 1, w), _reflect_index(xs + 1, w)
    hd = s[:, rt] - s[:, lf]                                   # horizontal difference, then smoothed down the column
    dx = 3 * hd[_reflect_index(ys - 1, h), :] + 10 * hd + 3 * hd[_reflect_index(ys + 1, h), :]
    vd = dn - up                                               # vertical difference, then smoothed along the row
    dy = 3 * vd[:, lf] + 10 * vd + 3 * vd[:, rt]
    return np.stack([dx, dy], axis=2).astype(np.int16)


def pyramid_np(img, p=None, with_deriv=True):
    p = p or params()
    img = _img(img)
    h, w = img.shape
    planes = [img.copy()]
    for lw, lh in level_sizes(w, h, p)[1:]:
        planes.append(pyr_down_np(planes[-1]))
        assert planes[-1].shape == (lh, lw)
    return planes, ([scharr_np(a) for a in planes] if with_deriv else [])


# ---- tracker, gate, 3-D ---------------------------------------------------------------------------------------------------------
def track(left, right, pts, p=None):
    p = p or params()
    left, right, pts = _img(left), _img(right), _pts(pts)
    if left.shape != right.shape:
        raise ValueError("left and right differ in size")
    h, w = left.shape
    n = len(pts)
    out = np.zeros((n, 2), np.float32)
    status = np.zeros(n, np.uint8)
    err = np.zeros(n, np.float32)
    info = np.zeros((n, 2), np.int32)
    hist = np.zeros((MAX_LEVELS, 102), np.int32)
    L = lib().lk_ref_track(left.ctypes.data, right.ctypes.data, w, h, pts.ctypes.data, n, ctypes.byref(p), out.ctypes.data,
                           status.ctypes.data, err.ctypes.data, info.ctypes.data, hist.ctypes.data)
    if L < 0:
        raise MemoryError("lk_ref_track")
    return out, status, err, info, hist[:L + 1]


def gate(pts, right_pts, status, p=None):
    p = p or params()
    pts, right_pts = _pts(pts), _pts(right_pts)
    status = np.ascontiguousarray(status, np.uint8).copy()
    lib().lk_ref_gate(pts.ctypes.data, right_pts.ctypes.data, status.ctypes.data, len(pts), p.min_disparity, p.max_disparity)
    return status


def correspondences(left, right, pts, p=None):
    p = p or params()
    left, right, pts = _img(left), _img(right), _pts(pts)
    h, w = left.shape
    n = len(pts)
    out = np.zeros((n, 2), np.float32)
    status = np.zeros(n, np.uint8)
    err = np.zeros(n, np.float32)
    if lib().lk_ref_correspondences(left.ctypes.data, right.ctypes.data, w, h, pts.ctypes.data, n, ctypes.byref(p), out.ctypes.data,
                                    status.ctypes.data, err.ctypes.data) < 0:
        raise MemoryError("lk_ref_correspondences")
    return out, status, err


def make_model(fx=700.0, fy=705.0, cx=320.5, cy=241.25, baseline=0.12, cx_r=None, local=None):
    """A StereoCameraModel in the reference's convention: Tx_l = 0, Tx_r = -fx * baseline."""
    m = StereoModel()
    m.fx_l, m.fy_l, m.cx_l, m.cy_l, m.Tx_l = fx, fy, cx, cy, 0.0
    m.fx_r, m.fy_r, m.cx_r, m.Tx_r = fx, fy, cx if cx_r is None else cx_r, -fx * baseline
    if local is not None:
        m.local[:] = [float(v) for v in np.asarray(local, np.float32).reshape(12)]
        m.has_local = 1
    return m


def keypoints3d(pts, right_pts, status, model, min_depth=0.0, max_depth=0.0):
    pts, right_pts = _pts(pts), _pts(right_pts)
    status = np.ascontiguousarray(status, np.uint8)
    xyz = np.zeros((len(pts), 3), np.float32)
    lib().lk_ref_keypoints3d(pts.ctypes.data, right_pts.ctypes.data, status.ctypes.data, len(pts), ctypes.byref(model), min_depth,
                             max_depth, xyz.ctypes.data)
    return xyz
