"""ctypes binding of the CPU restatement of generateKeypoints2 (oracle/libgftt_select_ref.so). TEST INFRASTRUCTURE ONLY.

select(eig, max_eig, ...) takes one uint16 (H, W) map, dense or with a row stride, and returns float32 (k, 2) points (x, y) in
acceptance order. The defaults are the reference's constants (GFTT.cpp:50-53).
"""
import ctypes

import numpy as np

import oracle_lib

_LIB = None

DEFAULTS = dict(max_features=1500, quality_level=0.01, min_distance=7.0, block_size=3)


def lib():
    global _LIB
    if _LIB is None:
        L = oracle_lib.load("libgftt_select_ref.so")
        vp, sz, ci, cd = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_double
        L.gfsr_select.argtypes = [vp, sz, ci, ci, ctypes.c_uint, ci, cd, cd, vp, ctypes.c_long]
        L.gfsr_select.restype = ctypes.c_long
        L.gfsr_candidates.argtypes = [vp, sz, ci, ci, ctypes.c_uint, cd]
        L.gfsr_candidates.restype = ctypes.c_long
        _LIB = L
    return _LIB


def _map(eig):
    eig = np.asarray(eig)
    if eig.dtype != np.uint16 or eig.ndim != 2 or eig.strides[1] != 2 or eig.strides[0] % 2 or eig.strides[0] < 2 * eig.shape[1]:
        raise ValueError("expected a uint16 (H, W) map with dense rows and a positive row stride")
    return eig


def candidates(eig, max_eig, quality_level=0.01):
    eig = _map(eig)
    h, w = eig.shape
    return int(lib().gfsr_candidates(eig.ctypes.data, eig.strides[0] // 2, w, h, int(max_eig) & 0xffff, quality_level))


def select(eig, max_eig, max_features=1500, quality_level=0.01, min_distance=7.0):
    eig = _map(eig)
    h, w = eig.shape
    cap = max_features if max_features > 0 else max((w - 2) * (h - 2), 0)
    out = np.zeros((max(cap, 1), 2), np.float32)
    k = lib().gfsr_select(eig.ctypes.data, eig.strides[0] // 2, w, h, int(max_eig) & 0xffff, max_features, quality_level,
                          min_distance, out.ctypes.data, cap)
    if k < 0:
        raise MemoryError("gfsr_select: out of memory")
    return out[:k].copy()
