"""The sequential CPU restatement of the reference's generateKeypoints (cv::goodFeaturesToTrack as include/sbm.h states it):
oracle/libgftt_cv_ref.so through ctypes, and an independent numpy transcription of the header's text that the C file is
held to. TEST INFRASTRUCTURE ONLY.

    set_reading(bits)                                              the SBM_CV_READING bits of both (512)
    eig_map(img) / eig_map_np(img)                                 -> (float32 map (H, W), float32 maximum)
    detect(img, max_features=1500, quality_level=0.01, min_distance=7.0) / detect_np(...)
                                                                   -> (points float32 (k, 2), map, maximum, candidates)
    select(eig, mx, ...) / select_np(eig, mx, ...)                 the selection alone -> (points, candidates)
    sqrtf(x)                                                       the C library's float square root, element by element
"""
import ctypes

import numpy as np

import oracle_lib

_LIB = None
_READING = 0
READ_FUSED = 512


def lib():
    global _LIB
    if _LIB is None:
        L = oracle_lib.load("libgftt_cv_ref.so")
        vp, ci, cd, sz, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t, ctypes.c_long
        L.gftt_cv_ref_set_reading.argtypes = [ci]
        L.gftt_cv_ref_set_reading.restype = None
        L.gftt_cv_ref_sqrtf.argtypes = [ctypes.c_float]
        L.gftt_cv_ref_sqrtf.restype = ctypes.c_float
        L.gftt_cv_ref_map.argtypes = [vp, sz, ci, ci, vp, vp]
        L.gftt_cv_ref_detect.argtypes = [vp, sz, ci, ci, ci, cd, cd, vp, vp, vp, vp, cl]
        L.gftt_cv_ref_detect.restype = cl
        L.gftt_cv_ref_select.argtypes = [vp, ctypes.c_float, ci, ci, ci, cd, cd, vp, vp, cl]
        L.gftt_cv_ref_select.restype = cl
        _LIB = L
    return _LIB


def set_reading(bits):
    """Both restatements follow these SBM_CV_READING bits from now on (only 512 means anything here)."""
    global _READING
    _READING = int(bits)
    lib().gftt_cv_ref_set_reading(_READING)


def _img(img):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1 or img.shape[0] < 3 or img.shape[1] < 3:
        raise ValueError("img must be an (H, W) uint8 array with dense rows, at least 3 x 3")
    return img


def capacity(max_features, w, h):
    return max_features if max_features > 0 else (w - 2) * (h - 2)


# ---- the C restatement ---------------------------------------------------------------------------------------------------
def sqrtf(x):
    L = lib()
    return np.array([L.gftt_cv_ref_sqrtf(float(v)) for v in np.asarray(x, np.float32).ravel()], np.float32)


def eig_map(img):
    img = _img(img)
    h, w = img.shape
    eig = np.empty((h, w), np.float32)
    mx = np.zeros(1, np.float32)
    if lib().gftt_cv_ref_map(img.ctypes.data, img.strides[0], w, h, eig.ctypes.data, mx.ctypes.data):
        raise MemoryError
    return eig, mx[0]


def detect(img, max_features=1500, quality_level=0.01, min_distance=7.0):
    img = _img(img)
    h, w = img.shape
    cap = max(capacity(max_features, w, h), 1)
    eig = np.empty((h, w), np.float32)
    mx = np.zeros(1, np.float32)
    nc = ctypes.c_long(0)
    out = np.zeros((cap, 2), np.float32)
    k = lib().gftt_cv_ref_detect(img.ctypes.data, img.strides[0], w, h, int(max_features), float(quality_level),
                                 float(min_distance), eig.ctypes.data, mx.ctypes.data, ctypes.addressof(nc), out.ctypes.data, cap)
    if k < 0:
        raise MemoryError
    return out[:k].copy(), eig, mx[0], int(nc.value)


def select(eig, mx, max_features=1500, quality_level=0.01, min_distance=7.0):
    """The selection alone on a float32 map and its maximum -> (points, candidates)."""
    eig = np.ascontiguousarray(eig, np.float32)
    h, w = eig.shape
    cap = max(capacity(max_features, w, h), 1)
    nc = ctypes.c_long(0)
    out = np.zeros((cap, 2), np.float32)
    k = lib().gftt_cv_ref_select(eig.ctypes.data, float(mx), w, h, int(max_features), float(quality_level), float(min_distance),
                                 ctypes.addressof(nc), out.ctypes.data, cap)
    if k < 0:
        raise MemoryError
    return out[:k].copy(), int(nc.value)


# ---- the numpy transcription of include/sbm.h ----------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on float32 arrays: a * b is exact in double; the double sum is turned into its round-to-odd value with the exact
    error of the addition (TwoSum), so the final rounding to float32 rounds the exact a * b + c once."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def _tap(c, q, f0, f1):
    c, q = np.asarray(c, np.float32), np.asarray(q, np.float32)
    if _READING & READ_FUSED:
        return _fma32(f1, q, f0 * c)
    return f1 * q + f0 * c


def _pad101(a):
    return np.pad(a, 1, mode="reflect")


def eig_map_np(img):
    img = _img(img)
    h, w = img.shape
    f1 = np.float32(1.0 / (4.0 * 3.0 * 255.0))
    f0 = np.float32(2.0) * f1
    p = _pad101(img.astype(np.int32))                     # p[y + 1][x + 1] is the pixel (y, x)
    d = p[:, 2:] - p[:, :-2]                              # (h + 2, w): row differences of rows -1 .. h
    dx = _tap(d[1:-1], d[:-2] + d[2:], f0, f1)
    r = _tap(p[:, 1:-1], p[:, :-2] + p[:, 2:], f0, f1)    # (h + 2, w): smoothed rows -1 .. h
    dy = (r[2:] - r[:-2]).astype(np.float32)
    planes = [dx * dx, dx * dy, dy * dy]
    box = []
    for pl in planes:
        assert pl.dtype == np.float32
        q = _pad101(pl).astype(np.float64)
        rows = (q[:, :-2] + q[:, 1:-1]) + q[:, 2:]        # left to right
        box.append(((rows[:-2] + rows[1:-1]) + rows[2:]).astype(np.float32))   # top to bottom, one rounding
    a, b, c = box[0] * np.float32(0.5), box[1], box[2] * np.float32(0.5)
    dd = a - c
    rad = _fma32(dd, dd, b * b) if _READING & READ_FUSED else dd * dd + b * b
    eig = ((a + c) - np.sqrt(rad)).astype(np.float32)
    # the maximum in the order "numeric, -0 below +0"
    mx = eig.max()
    if mx == 0 and not np.any((eig == 0) & ~np.signbit(eig)):
        mx = np.float32(-0.0)
    return eig, np.float32(mx)


def detect_np(img, max_features=1500, quality_level=0.01, min_distance=7.0):
    eig, mx = eig_map_np(img)
    pts, nc = select_np(eig, mx, max_features, quality_level, min_distance)
    return pts, eig, mx, nc


def select_np(eig, mx, max_features=1500, quality_level=0.01, min_distance=7.0):
    eig = np.asarray(eig, np.float32)
    h, w = eig.shape
    thr = np.float32(np.float64(mx) * np.float64(quality_level))
    t = np.where(eig > thr, eig, np.float32(0)).astype(np.float32)
    dil = t.copy()
    dil[1:-1, 1:-1] = np.max([t[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    cand = np.zeros((h, w), bool)
    cand[1:-1, 1:-1] = (t[1:-1, 1:-1] != 0) & (t[1:-1, 1:-1] == dil[1:-1, 1:-1])
    idx = np.flatnonzero(cand)
    vals = t.ravel()[idx]
    order = np.lexsort((-idx, -vals.astype(np.float64)))   # value descending, then raster index descending
    idx = idx[order]
    pts = []
    if min_distance >= 1:
        cell = int(np.rint(min_distance))                  # cvRound: half to even
        gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
        grid = {}
        md2 = float(min_distance) * float(min_distance)
        for i in idx:
            y, x = divmod(int(i), w)
            xc, yc = x // cell, y // cell
            good = True
            for yy in range(max(yc - 1, 0), min(yc + 1, gh - 1) + 1):
                for xx in range(max(xc - 1, 0), min(xc + 1, gw - 1) + 1):
                    for (px, py) in grid.get((xx, yy), ()):
                        ddx, ddy = np.float32(x - px), np.float32(y - py)
                        if float(ddx * ddx + ddy * ddy) < md2:
                            good = False
                            break
                    if not good:
                        break
                if not good:
                    break
            if good:
                grid.setdefault((xc, yc), []).append((x, y))
                pts.append((x, y))
                if max_features > 0 and len(pts) == max_features:
                    break
    else:
        for i in idx:
            y, x = divmod(int(i), w)
            pts.append((x, y))
            if max_features > 0 and len(pts) == max_features:
                break
    return np.array(pts, np.float32).reshape(-1, 2), int(idx.size)
