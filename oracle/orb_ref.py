"""The CPU restatement of computeDescriptor (oracle/liborb_ref.so) through ctypes, and a literal numpy transcription of the
same steps that the C file is held to. TEST INFRASTRUCTURE ONLY.

    describe(img, kpts, pattern, angle=-1.0, edge=19, half_up=False) -> (kept (k, 2) float32, desc (k, 32) uint8, blur (H, W))
    describe_np(...)                                                 -> the same, in numpy
    blur(img, half_up=False) / blur_np(...)                          -> the blurred frame (W, H >= 24)
    taps() / taps_np()                                               -> the seven integer taps, derived

`pattern` is 512 (x, y) points, as (512, 2) or (1024,) ints; pairs of consecutive points are compared. blur is None when every
keypoint is erased by the size rule (W or H <= 2 edge).
"""
import ctypes
import math

import numpy as np

import oracle_lib

_LIB = None
BORDER = 23


def lib():
    global _LIB
    if _LIB is None:
        L = oracle_lib.load("liborb_ref.so")
        vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        L.orb_taps.argtypes = [vp]
        L.orb_taps.restype = None
        L.orb_blur.argtypes = [vp, sz, ci, ci, ci, vp]
        L.orb_describe.argtypes = [vp, sz, ci, ci, vp, ci, vp, ctypes.c_float, ci, ci, vp, vp, vp]
        _LIB = L
    return _LIB


def _pattern(pattern):
    p = np.ascontiguousarray(np.asarray(pattern, dtype=np.int32).reshape(-1))
    assert p.size == 1024
    return p


def taps():
    k = np.zeros(7, np.int32)
    lib().orb_taps(k.ctypes.data)
    return k


def blur(img, half_up=False):
    img = np.asarray(img, dtype=np.uint8)
    assert img.strides[1] == 1
    h, w = img.shape
    out = np.zeros((h, w), np.uint8)
    assert lib().orb_blur(img.ctypes.data, img.strides[0], w, h, int(bool(half_up)), out.ctypes.data) == 0
    return out


def describe(img, kpts, pattern, angle=-1.0, edge=19, half_up=False):
    img = np.asarray(img, dtype=np.uint8)
    assert img.strides[1] == 1
    h, w = img.shape
    kp = np.ascontiguousarray(np.asarray(kpts, dtype=np.float32).reshape(-1, 2))
    n = kp.shape[0]
    out = np.zeros((max(n, 1), 2), np.float32)
    desc = np.zeros((max(n, 1), 32), np.uint8)
    bl = np.zeros((h, w), np.uint8)
    pat = _pattern(pattern)
    k = lib().orb_describe(img.ctypes.data, img.strides[0], w, h, kp.ctypes.data, n, pat.ctypes.data, float(angle), int(edge),
                           int(bool(half_up)), out.ctypes.data, desc.ctypes.data, bl.ctypes.data)
    assert k >= 0
    return out[:k].copy(), desc[:k].copy(), (bl if (w > 2 * edge and h > 2 * edge) else None)


# ---- numpy transcription ----------------------------------------------------------------------------------------------------
def taps_np():
    """getGaussianKernel(7, 2) in double, stored as float32, then cvRound(256 k)."""
    x = np.arange(7, dtype=np.float64) - 3
    g = np.exp(-0.5 / (2.0 * 2.0) * x * x)
    g = (g / g.sum()).astype(np.float32)
    return np.rint(g.astype(np.float64) * 256.0).astype(np.int64)


def _round_shift16(s, half_up):
    q, rem = s >> 16, s & 0xFFFF
    if half_up:
        q = q + (rem >= 0x8000)
    else:
        q = q + ((rem > 0x8000) | ((rem == 0x8000) & ((q & 1) == 1)))
    return np.minimum(q, 255).astype(np.uint8)


def blur_np(img, half_up=False):
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    ext = np.pad(img, BORDER, mode="reflect").astype(np.int64)   # numpy's "reflect" is BORDER_REFLECT_101
    k = taps_np()
    rows = ext[BORDER - 3:BORDER + h + 3]
    r = sum(k[i] * rows[:, BORDER - 3 + i:BORDER - 3 + i + w] for i in range(7))
    s = sum(k[j] * r[j:j + h] for j in range(7))
    return _round_shift16(s, half_up)


def offsets_np(pattern, angle=-1.0):
    """(dx, dy) of the 512 points, float32 arithmetic without contraction, cvRound half to even."""
    p = _pattern(pattern).reshape(512, 2).astype(np.float32)
    ang = np.float32(angle) * np.float32(math.pi / 180.0)
    a, b = np.float32(math.cos(float(ang))), np.float32(math.sin(float(ang)))
    x = p[:, 0] * a - p[:, 1] * b
    y = p[:, 0] * b + p[:, 1] * a
    return np.rint(x).astype(np.int64), np.rint(y).astype(np.int64)


def describe_np(img, kpts, pattern, angle=-1.0, edge=19, half_up=False):
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    kp = np.asarray(kpts, dtype=np.float32).reshape(-1, 2)
    if not (w > 2 * edge and h > 2 * edge):
        return np.zeros((0, 2), np.float32), np.zeros((0, 32), np.uint8), None
    with np.errstate(invalid="ignore"):
        rx, ry = np.rint(kp[:, 0]), np.rint(kp[:, 1])
        keep = (rx >= edge) & (rx < w - edge) & (ry >= edge) & (ry < h - edge)
    kept = kp[keep]
    bl = blur_np(img, half_up)
    dx, dy = offsets_np(pattern, angle)
    cx = np.rint(kept[:, 0]).astype(np.int64)
    cy = np.rint(kept[:, 1]).astype(np.int64)
    v = bl[cy[:, None] + dy[None, :], cx[:, None] + dx[None, :]]   # (k, 512)
    bits = (v[:, 0::2] < v[:, 1::2]).astype(np.uint8).reshape(-1, 32, 8)
    desc = (bits << np.arange(8, dtype=np.uint8)).sum(axis=2).astype(np.uint8)
    return kept.copy(), desc, bl
