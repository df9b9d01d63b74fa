"""The CPU restatement of matchingNoGuess / matchingGuess (oracle/libmatch_ref.so) through ctypes, and a literal numpy
transcription of the Registration.cpp loops that the C file is held to. TEST INFRASTRUCTURE ONLY.

    match(desc_from, desc_to, proj=None, kpts_to=None, radius=40.0, nndr=0.8, fused=False) -> (pairs (k, 2) int32, rec (nf, 4))
    match_np(...)                                                                            -> the same, in numpy
    project(xyz, T, K, W, H) / project_np(...)                                               -> (n, 2) float32, NaN = not valid
    hamming(a, b)                                                                            -> int

Descriptors are (n, 32) uint8 rows. rec holds per from-row (best, d0, d1, candidates) with 257 for a missing distance. In
match_np, guided candidates come in radiusMatch's order (by distance), so rec's best may name another row of equal distance when
d0 == d1 -- NNDR rejects every such query, and the pairs are the same (test_match_restatement.py).
"""
import ctypes
import math
from fractions import Fraction

import numpy as np

import oracle_lib

_LIB = None
NONE = 257


def lib():
    global _LIB
    if _LIB is None:
        L = oracle_lib.load("libmatch_ref.so")
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.match_ref_hamming.argtypes = [vp, vp]
        L.match_ref_project.argtypes = [vp, ci, vp, vp, ci, ci, vp]
        L.match_ref_project.restype = None
        L.match_ref_match.argtypes = [vp, ci, vp, ci, vp, vp, cf, cf, ci, vp, vp]
        _LIB = L
    return _LIB


def _rows(d):
    d = np.ascontiguousarray(np.asarray(d, dtype=np.uint8).reshape(-1, 32))
    return d


def hamming(a, b):
    a, b = _rows(a), _rows(b)
    return lib().match_ref_hamming(a.ctypes.data, b.ctypes.data)


def project(xyz, T, K, W, H):
    xyz = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    T = np.ascontiguousarray(np.asarray(T, np.float32).reshape(12))
    K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(4))
    out = np.empty((xyz.shape[0], 2), np.float32)
    lib().match_ref_project(xyz.ctypes.data, xyz.shape[0], T.ctypes.data, K.ctypes.data, int(W), int(H), out.ctypes.data)
    return out


def match(desc_from, desc_to, proj=None, kpts_to=None, radius=40.0, nndr=0.8, fused=False):
    a, b = _rows(desc_from), _rows(desc_to)
    nf, nt = a.shape[0], b.shape[0]
    rec = np.zeros((max(nf, 1), 4), np.int32)
    pairs = np.zeros((max(nf, 1), 2), np.int32)
    pp = kp = None
    if proj is not None:
        pp = np.ascontiguousarray(np.asarray(proj, np.float32).reshape(-1, 2))
        kp = np.ascontiguousarray(np.asarray(kpts_to, np.float32).reshape(-1, 2))
        if kp.shape[0] == 0:
            kp = np.zeros((1, 2), np.float32)
    k = lib().match_ref_match(a.ctypes.data, nf, b.ctypes.data, nt, None if pp is None else pp.ctypes.data,
                              None if kp is None else kp.ctypes.data, float(radius), float(nndr), 1 if fused else 0,
                              rec.ctypes.data, pairs.ctypes.data)
    if k < 0:
        raise MemoryError("match_ref_match")
    return pairs[:k].copy(), rec[:nf].copy()


# ---- the literal transcription ------------------------------------------------------------------------------------------------
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _dist(q, train):
    """NORM_HAMMING distances of one 32-byte query to every train row."""
    return _POP[np.bitwise_xor(train, q[None, :])].sum(axis=1)


def _knn2(q, train, idx):
    """BFMatcher(NORM_HAMMING).knnMatch(q, train rows idx, 2): batchDistance's insertion over idx in the given order."""
    best, d0, d1 = -1, NONE, NONE
    if len(idx):
        ds = _dist(q, train[np.asarray(idx)])
        for j, d in zip(idx, ds.tolist()):
            if d < d0:
                best, d0, d1 = j, d, d0
            elif d < d1:
                d1 = d
    return best, d0, d1


def _nndr(d0, d1, nndr):
    return np.float32(d0) < np.float32(nndr) * np.float32(d1)


def fma_f32(a, b, c):
    """fmaf(a, b, c): the exact a * b + c rounded once to float32, to nearest even."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    g = np.float32(float(exact))                 # within one float32 step of the answer
    cands = [np.nextafter(g, np.float32(-np.inf)), g, np.nextafter(g, np.float32(np.inf))]
    best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


def project_np(xyz, T, K, W, H):
    """matchingGuess_Projection: transformPoint(p, guessCameraRef).z in float, projectPoints' pinhole model in double."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    T = np.asarray(T, np.float32).reshape(12)
    fx, fy, cx, cy = (float(v) for v in np.asarray(K, np.float64).reshape(4))
    out = np.full((xyz.shape[0], 2), np.nan, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, (x, y, z) in enumerate(xyz):
            zc = T[8] * x + T[9] * y + T[10] * z + T[11]                     # float32 scalars, left to right
            X, Y, Z = float(x), float(y), float(z)
            xc = float(T[0]) * X + float(T[1]) * Y + float(T[2]) * Z + float(T[3])
            yc = float(T[4]) * X + float(T[5]) * Y + float(T[6]) * Z + float(T[7])
            wc = float(T[8]) * X + float(T[9]) * Y + float(T[10]) * Z + float(T[11])
            inv = 1.0 / wc if wc != 0.0 else 1.0
            u, v = np.float32(xc * inv * fx + cx), np.float32(yc * inv * fy + cy)
            if 0.0 < u < np.float32(W - 1) and 0.0 < v < np.float32(H - 1) and zc > 0.0:
                out[i] = (u, v)
    return out


def match_np(desc_from, desc_to, proj=None, kpts_to=None, radius=40.0, nndr=0.8, fused=False):
    a, b = _rows(desc_from), _rows(desc_to)
    nf, nt = a.shape[0], b.shape[0]
    rec = np.tile(np.array([-1, NONE, NONE, 0], np.int32), (nf, 1))
    matched = []                   # std::multimap<int, int>, inserted at the end in increasing from
    added = set()                  # std::set<int>
    if proj is None:               # matchingNoGuess
        for i in range(nf):
            best, d0, d1 = _knn2(a[i], b, list(range(nt)))
            rec[i] = (best, d0, d1, nt)
            if nt >= 2 and _nndr(d0, d1, nndr):   # nt == 1: matches[i][1] does not exist; defined as no match
                if best not in added:
                    added.add(best)
                    matched.append((i, best))
    else:                          # matchingGuess
        proj = np.asarray(proj, np.float32).reshape(-1, 2)
        kp = np.asarray(kpts_to, np.float32).reshape(-1, 2)
        r = np.float32(radius)
        for i in range(nf):        # projectedIndex: the valid points in increasing from-index
            px, py = proj[i]
            if math.isnan(px) or math.isnan(py):
                continue
            hits = []              # radiusMatch(NORM_L2): (distance, train index) with distance < radius
            for j in range(nt):
                dx, dy = np.float32(px - kp[j, 0]), np.float32(py - kp[j, 1])
                if fused:
                    d2 = fma_f32(dy, dy, np.float32(dx * dx))
                else:
                    d2 = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
                d = np.sqrt(d2, dtype=np.float32)
                if d < r:
                    hits.append((float(d), j))
            indices = [j for _, j in sorted(hits)]   # radiusMatch sorts each row by distance
            best, d0, d1 = _knn2(a[i], b, indices)
            rec[i] = (best, d0, d1, len(indices))
            to = -1                                  # matchingGuess_search
            if len(indices) == 1:
                to = indices[0]
            elif len(indices) >= 2 and _nndr(d0, d1, nndr):
                to = best
            if to >= 0 and to not in added:
                added.add(to)
                matched.append((i, to))
    return np.array(matched, np.int32).reshape(-1, 2), rec


# ---- radius-edge cases for the tests ------------------------------------------------------------------------------------------
def sq_dist(px, py, kx, ky, fused):
    """The guided test's squared distance of one (projection, keypoint) pair in float32, as both restatements compute it."""
    dx, dy = np.float32(np.float32(px) - np.float32(kx)), np.float32(np.float32(py) - np.float32(ky))
    xx = np.float32(dx * dx)
    return fma_f32(dy, dy, xx) if fused else np.float32(xx + np.float32(dy * dy))


def inside(d2, radius=40.0):
    """radiusMatch's test: the correctly rounded float square root, strictly below the radius."""
    return bool(np.sqrt(np.float32(d2), dtype=np.float32) < np.float32(radius))


def radius_edge_cases(count=8, seed=0, radius=40.0):
    """(projection, keypoint) float32 pairs on the radius edge with dy != 0, one per 256 x 256 grid cell, of three kinds
    (count of each): 'band_unfused' / 'band_fused' -- the squared distance under that reading is below radius^2 but its rounded
    square root reaches the radius (so `d2 < radius^2` would wrongly take it); 'readings_differ' -- the two readings of the sum
    decide the radius test differently. Returns (proj (k, 2), kpts (k, 2), kinds list). The search runs at the radius scaled
    into [32, 64) by a power of two and every coordinate is scaled back at the end: both steps are exact in float32 and commute
    with the squares, the sums and the rounded square root, so the kinds hold at the radius asked for (at 40 the scale is 1).
    The band kinds exist only for a radius r at which the least float whose rounded root reaches r lies below fl(r * r)."""
    rng = np.random.default_rng(seed)
    scale = np.float32(2.0 ** (math.floor(math.log2(float(np.float32(radius)))) - 5))
    radius = float(np.float32(radius) / scale)
    r = np.float32(radius)
    r2 = np.float32(np.float64(r) * np.float64(r))
    N = 400000
    q = 2.0 ** -12      # every coordinate on this grid: the cell shifts below (multiples of 256, sums < 4096) stay exact
    px = (256.0 + np.round(rng.uniform(0, 1, N) / q) * q).astype(np.float32)
    py = (256.0 + np.round(rng.uniform(0, 1, N) / q) * q).astype(np.float32)
    th = rng.uniform(0.2, 1.35, N)                                  # both dx and dy far from 0
    kx = (np.round((px + radius * np.cos(th)) / q) * q).astype(np.float32)
    ky = (np.round((py + radius * np.sin(th)) / q) * q).astype(np.float32)
    dx, dy = px - kx, py - ky
    xx = dx * dx
    un = xx + dy * dy
    fu = (dy.astype(np.float64) * dy.astype(np.float64) + xx.astype(np.float64)).astype(np.float32)   # screening only
    want = {"band_unfused": [], "band_fused": [], "readings_differ": []}
    for i in np.flatnonzero((un < r2) | (fu < r2)):
        if all(len(v) >= count for v in want.values()):
            break
        a = (px[i], py[i], kx[i], ky[i])
        du, df = sq_dist(*a, False), sq_dist(*a, True)
        iu, jf = inside(du, radius), inside(df, radius)
        if du < r2 and not iu and len(want["band_unfused"]) < count:
            want["band_unfused"].append(a)
        elif df < r2 and not jf and len(want["band_fused"]) < count:
            want["band_fused"].append(a)
        elif iu != jf and len(want["readings_differ"]) < count:
            want["readings_differ"].append(a)
    proj, kpts, kinds = [], [], []
    for kind, cases in want.items():
        for a in cases:
            c = len(proj)
            ox, oy = np.float32(256 * (c % 8)), np.float32(256 * (c // 8))   # exact shifts: the same dx, dy
            proj.append((a[0] + ox, a[1] + oy))
            kpts.append((a[2] + ox, a[3] + oy))
            kinds.append(kind)
    return np.array(proj, np.float32) * scale, np.array(kpts, np.float32) * scale, kinds
