"""The CPU restatement of cv::StereoSGBM (oracle/sgbm_ref.c) against an independently written numpy textbook form, bit for bit.

The textbook form below shares no code with oracle/sgbm_ref.c: per-pixel Birchfield-Tomasi costs on whole arrays, an
explicit (2r+1)^2 box sum, one explicit loop per path direction, S = min(32767, sum of the path costs) (the envelope argument
of include/sbm.h), the selection loop with x descending, the LR check, a 3x3 median by sorting and a flood-fill speckle filter.
"""
import numpy as np
import pytest

import sgbm_ref

HH, SG = sgbm_ref.MODE_HH, sgbm_ref.MODE_SGBM


def _channels(img, ftzero):
    img = img.astype(np.int64)
    H, W = img.shape
    up = img[np.maximum(np.arange(H) - 1, 0)]
    dn = img[np.minimum(np.arange(H) + 1, H - 1)]
    sob = np.full((H, W), ftzero, np.int64)
    raw = np.full((H, W), ftzero, np.int64)
    if W > 2:
        s = (img[:, 2:] - img[:, :-2]) * 2 + up[:, 2:] - up[:, :-2] + dn[:, 2:] - dn[:, :-2]
        sob[:, 1:-1] = np.clip(s, -ftzero, ftzero) + ftzero
        raw[:, 1:-1] = img[:, 1:-1]
    return [sob, raw]


def _lohi(ch):
    left = ch.copy()
    left[:, 1:] = (ch[:, 1:] + ch[:, :-1]) // 2
    right = ch.copy()
    right[:, :-1] = (ch[:, :-1] + ch[:, 1:]) // 2
    return np.minimum(np.minimum(left, right), ch), np.maximum(np.maximum(left, right), ch)


def _flood_speckles(img, new_val, max_size, max_diff):
    H, W = img.shape
    out = img.copy()
    seen = np.zeros((H, W), bool)
    for y0 in range(H):
        for x0 in range(W):
            if seen[y0, x0] or img[y0, x0] == new_val:
                continue
            comp, stack = [], [(y0, x0)]
            seen[y0, x0] = True
            while stack:
                y, x = stack.pop()
                comp.append((y, x))
                for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= yy < H and 0 <= xx < W and not seen[yy, xx] and img[yy, xx] != new_val \
                            and abs(int(img[yy, xx]) - int(img[y, x])) <= max_diff:
                        seen[yy, xx] = True
                        stack.append((yy, xx))
            if len(comp) <= max_size:
                for y, x in comp:
                    out[y, x] = new_val
    return out


def _trunc_div(a, b):
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def textbook(L, R, minD=0, nd=16, bs=3, P1=0, P2=0, d12=0, cap=0, uniq=0, sws=0, sr=0, mode=SG, reading=0, stages=False):
    P1 = P1 if P1 > 0 else 2
    P2 = max(P2 if P2 > 0 else 5, P1 + 1)
    bs = bs if bs > 0 else 5
    r = bs // 2
    ft = max(cap, 15) | 1
    uniq = uniq if uniq >= 0 else 10
    d12 = d12 if d12 > 0 else 1
    H, W = L.shape
    D = nd
    minX1, maxX1 = max(minD + nd, 0), W + min(minD, 0)
    w1 = maxX1 - minX1
    inv = (minD - 1) * 16
    if w1 < 1:
        return np.full((H, W), inv, np.int16), None
    # pixel costs P[y, x, d] for image column X = minX1 + x, right column X - (minD + d)
    P = np.zeros((H, w1, D), np.int64)
    X = minX1 + np.arange(w1)[:, None]
    X2 = X - (minD + np.arange(D)[None, :])
    for c, (cl, cr) in enumerate(zip(_channels(L, ft), _channels(R, ft))):
        l0, l1 = _lohi(cl)
        r0, r1 = _lohi(cr)
        u, u0, u1 = cl[:, X], l0[:, X], l1[:, X]
        v, v0, v1 = cr[:, X2], r0[:, X2], r1[:, X2]
        c0 = np.maximum(np.maximum(0, u - v1), v0 - u)
        c1 = np.maximum(np.maximum(0, v - u1), u0 - v)
        P += np.minimum(c0, c1) >> (2 if c else 0)
    # box sum, columns clamped to the computable range, rows clamped
    xs = np.clip(np.arange(w1)[:, None] + np.arange(-r, r + 1)[None, :], 0, w1 - 1)
    Hs = P[:, xs, :].sum(axis=2)
    C = np.empty((H, w1, D), np.int64)
    for y in range(H):
        if y > 0 and y + r >= H and not (reading & sgbm_ref.READ_BOTTOM_CLAMPED):
            C[y] = P2 if mode == HH else C[y - 1]
            continue
        ys = np.clip(np.arange(y - r, y + r + 1), 0, H - 1)
        C[y] = P2 + Hs[ys].sum(axis=0)
    BIG = 1 << 30

    def step(Cpix, Lp, minLp):
        pad = np.full(Lp.shape[:-1] + (D + 2,), BIG, np.int64)
        pad[..., 1:-1] = Lp
        delta = minLp[..., None] + P2
        best = np.minimum(np.minimum(Lp, pad[..., :-2] + P1), np.minimum(pad[..., 2:] + P1, delta))
        return Cpix + best - delta

    dirs = [(1, 0), (1, 1), (0, 1), (-1, 1)] + ([(-1, 0), (-1, -1), (0, -1), (1, -1)] if mode == HH else [(-1, 0)])
    total = np.zeros((H, w1, D), np.int64)
    for sx, sy in dirs:
        Lr = np.zeros((H, w1, D), np.int64)
        if sy == 0:
            order = range(w1) if sx > 0 else range(w1 - 1, -1, -1)
            for x in order:
                px = x - sx
                if 0 <= px < w1:
                    Lp = Lr[:, px]
                else:
                    Lp = np.zeros((H, D), np.int64)
                Lr[:, x] = step(C[:, x], Lp, Lp.min(axis=-1))
        else:
            order = range(H) if sy > 0 else range(H - 1, -1, -1)
            for y in order:
                py = y - sy
                Lp = np.zeros((w1, D), np.int64)
                if 0 <= py < H:
                    src = np.arange(w1) - sx
                    ok = (src >= 0) & (src < w1)
                    Lp[ok] = Lr[py, src[ok]]
                Lr[y] = step(C[y], Lp, Lp.min(axis=-1))
        assert Lr.min() >= 0
        total += Lr
    S = np.minimum(total, 32767)
    pre = np.full((H, W), inv, np.int64)
    ar = np.arange(D)
    for y in range(H):
        d2cost = np.full(W, 32767)
        d2 = np.full(W, inv)
        row = pre[y]
        for x in range(w1 - 1, -1, -1):
            s = S[y, x]
            m = int(s.min())
            b = int(np.argmin(s)) if m < 32767 else -1   # strict `<` from a start of 32767: no winner when all saturate
            if np.any((s * (100 - uniq) < m * 100) & (np.abs(ar - b) > 1)):
                continue
            x2 = x + minX1 - b - minD
            if m < 32767 and d2cost[x2] > m:
                d2cost[x2] = m
                d2[x2] = b + minD
            if 0 < b < D - 1:
                den = max(int(s[b - 1]) + int(s[b + 1]) - 2 * m, 1)
                val = b * 16 + _trunc_div((int(s[b - 1]) - int(s[b + 1])) * 16 + den, 2 * den)
            else:
                val = b * 16
            row[x + minX1] = val + minD * 16
        for X in range(minX1, maxX1):
            d1 = int(row[X])
            if d1 == inv:
                continue
            lo, hi = d1 >> 4, (d1 + 15) >> 4
            a, b2 = X - lo, X - hi
            if 0 <= a < W and d2[a] >= minD and abs(d2[a] - lo) > d12 and 0 <= b2 < W and d2[b2] >= minD and abs(d2[b2] - hi) > d12:
                row[X] = inv
    out = pre.copy()
    if not (reading & sgbm_ref.READ_NO_MEDIAN):
        padded = np.pad(pre, 1, mode="edge")
        nb = np.stack([padded[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
        out = np.sort(nb, axis=0)[4]
    out = out.astype(np.int16)
    if sws > 0:
        out = _flood_speckles(out, inv, sws, 16 * sr)
    return out, dict(C=C, S=S, pre=pre.astype(np.int16))


def _pair(seed, H, W, kind="noise"):
    rng = np.random.default_rng(seed)
    if kind == "binary":   # high-contrast uncorrelated pairs: some pixels saturate S at every disparity
        rng = np.random.default_rng(seed)
        return ((rng.integers(0, 2, (H, W)) * 255).astype(np.uint8), (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8))
    if kind == "flat":
        L = np.full((H, W), 100, np.uint8)
        L[:, W // 2:] = 120
        R = np.roll(L, -3, axis=1)
        return L, R
    if kind == "far":   # a smooth pair shifted by a third to two thirds of the width: winners in the upper disparities
        shift = int(rng.integers(W // 3, 2 * W // 3))
        base = (np.cumsum(rng.integers(-6, 7, (H, W + 40 + shift)), axis=1) % 256).astype(np.uint8)
        return np.ascontiguousarray(base[:, 20:20 + W]), np.ascontiguousarray(base[:, 20 + shift:20 + shift + W])
    base = rng.integers(0, 256, (H, W + 40)).astype(np.uint8)
    if kind == "smooth":
        base = (np.cumsum(rng.integers(-6, 7, (H, W + 40)), axis=1) % 256).astype(np.uint8)
    shift = int(rng.integers(1, 12))
    L = base[:, 20:20 + W]
    R = base[:, 20 + shift:20 + shift + W].copy()
    R = np.clip(R.astype(int) + rng.integers(-3, 4, R.shape), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(L), R


# (minD, nd, bs, P1, P2, d12, cap, uniq, sws, sr, mode, H, W, kind)
CASES = [
    (0, 16, 3, 0, 0, 0, 0, 0, 0, 0, SG, 12, 40, "noise"),         # create() defaults
    (0, 16, 3, 0, 0, 0, 0, 0, 0, 0, HH, 12, 40, "noise"),
    (-8, 32, 5, 8, 32, 1, 0, 15, 0, 0, HH, 14, 56, "smooth"),
    (-8, 32, 5, 8, 32, 1, 0, 15, 20, 2, SG, 14, 56, "smooth"),
    (1, 16, 1, 4, 40, -1, 31, 0, 0, 0, HH, 10, 48, "noise"),
    (2, 16, 7, 0, 0, 32, 0, 15, 0, 0, SG, 13, 44, "smooth"),     # minD >= 2: unclaimed entries pass the >= minD test
    (3, 48, 11, 100, 1000, 32, 0, 15, 30, 16, HH, 16, 80, "smooth"),
    (-64, 64, 9, 10, 120, 2, 63, 0, 0, 0, HH, 12, 88, "noise"),
    (0, 32, 9, 10, 14000, 1, 63, 0, 0, 0, HH, 12, 50, "noise"),   # S saturates: 81 * 189 + 14000 = 29309
    (0, 16, 11, 100, 1000, 32, 0, 15, 6, 1, SG, 8, 40, "flat"),  # ties everywhere; bottom rows past half the block
    (0, 64, 3, 0, 0, 0, 0, 15, 0, 0, SG, 6, 64, "noise"),         # width1 = 0: the whole map invalid
    (-16, 32, 3, 0, 0, 0, 0, 15, 0, 0, HH, 6, 33, "noise"),       # width1 = 1
    (0, 16, 4, 3, 9, 0, 20, 5, 0, 0, SG, 9, 36, "noise"),         # even block size
    (0, 32, 11, 50, 9000, 1, 63, 0, 0, 0, HH, 20, 120, "binary"),  # S saturated at every disparity: no winner
    (0, 32, 11, 50, 9000, 1, 63, 0, 0, 0, SG, 20, 120, "binary"),
    (-3, 32, 11, 50, 9000, 1, 63, 15, 0, 0, HH, 20, 120, "binary"),
    # every lane layout of the GPU kernels (NV = 2 / 4 / 8 disparities per lane, partly masked) on tiny frames
    (0, 80, 3, 8, 72, 1, 0, 10, 0, 0, HH, 6, 110, "far"),         # width1 = 30
    (-20, 144, 5, 0, 0, 4, 0, 15, 0, 0, SG, 5, 180, "far"),       # width1 = 36
    (3, 272, 1, 4, 40, 32, 31, 0, 10, 1, HH, 4, 300, "far"),      # width1 = 25
    (-4, 272, 11, 100, 1000, 0, 0, 15, 0, 0, SG, 6, 310, "smooth"),
    (0, 512, 3, 0, 0, 0, 0, 15, 0, 0, HH, 3, 542, "far"),         # width1 = 30
    (-256, 512, 7, 10, 200, 0, 0, 0, 20, 2, SG, 6, 540, "far"),   # width1 = 28
    (5, 512, 5, 8, 64, 4, 63, 0, 0, 0, HH, 5, 560, "noise"),
    # frames one, two and three rows tall
    (0, 32, 3, 0, 0, 0, 0, 0, 0, 0, HH, 1, 60, "smooth"),
    (-4, 16, 5, 4, 40, 1, 0, 15, 0, 0, SG, 1, 45, "noise"),
    (-4, 16, 5, 4, 40, 1, 0, 15, 0, 0, HH, 2, 50, "smooth"),
    (2, 48, 7, 0, 0, 32, 0, 10, 4, 1, SG, 2, 90, "far"),
    (2, 48, 7, 0, 0, 32, 0, 10, 4, 1, HH, 3, 90, "far"),
    (-8, 80, 9, 8, 300, 4, 0, 0, 0, 0, SG, 3, 120, "smooth"),
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("reading", [0, sgbm_ref.READ_NO_MEDIAN | sgbm_ref.READ_BOTTOM_CLAMPED])
def test_restatement_equals_textbook(case, reading):
    minD, nd, bs, P1, P2, d12, cap, uniq, sws, sr, mode, H, W, kind = CASES[case]
    L, R = _pair(case, H, W, kind)
    p = sgbm_ref.make_params(minD, nd, bs, P1, P2, d12, cap, uniq, sws, sr, mode)
    got, st = sgbm_ref.compute(p, L, R, reading=reading, stages=True)
    want, tb = textbook(L, R, minD, nd, bs, P1, P2, d12, cap, uniq, sws, sr, mode, reading=reading)
    if tb is not None:
        np.testing.assert_array_equal(st["C"], tb["C"])
        np.testing.assert_array_equal(st["S"], tb["S"])
        np.testing.assert_array_equal(st["pre"], tb["pre"])
    np.testing.assert_array_equal(got, want)


def test_cases_cover_the_interesting_ground():
    L, R = _pair(8, 12, 50, "noise")
    p = sgbm_ref.make_params(*CASES[8][:11])
    _, st = sgbm_ref.compute(p, L, R, stages=True)
    assert (st["S"] == 32767).any(), "the saturation case must saturate"
    assert sgbm_ref.envelope(p) <= 32767
    assert sgbm_ref.width1(sgbm_ref.make_params(*CASES[10][:11]), 64) < 1
    assert sgbm_ref.width1(sgbm_ref.make_params(*CASES[11][:11]), 33) == 1
    # minD >= 2 with unclaimed claim-table entries: the LR check rejects pixels a minD <= 1 reading would keep
    L, R = _pair(5, 13, 44, "smooth")
    p = sgbm_ref.make_params(*CASES[5][:11])
    _, st = sgbm_ref.compute(p, L, R, stages=True)
    assert (st["pre"] == 16).any() and (st["pre"] > 16).any()


@pytest.mark.parametrize("case", [13, 14])
def test_all_saturated_pixels_have_no_winner(case):
    minD, nd, bs, P1, P2, d12, cap, uniq, sws, sr, mode, H, W, kind = CASES[case]
    L, R = _pair(case, H, W, kind)
    p = sgbm_ref.make_params(minD, nd, bs, P1, P2, d12, cap, uniq, sws, sr, mode)
    assert sgbm_ref.envelope(p) <= 32767
    _, st = sgbm_ref.compute(p, L, R, stages=True)
    full = (st["S"] == 32767).all(axis=2)
    assert full.any(), "the case must saturate S at every disparity of some pixels"
    ys, xs = np.nonzero(full)
    assert (st["pre"][ys, xs + max(minD + nd, 0)] == (minD - 1) * 16).all()


@pytest.mark.parametrize("mode", [SG, HH])
def test_readings_change_the_map(mode):
    L, R = _pair(3, 12, 48, "smooth")
    p = sgbm_ref.make_params(0, 16, 7, 8, 64, 1, 0, 0, 0, 0, mode)
    a = sgbm_ref.compute(p, L, R)
    assert not np.array_equal(a, sgbm_ref.compute(p, L, R, reading=sgbm_ref.READ_NO_MEDIAN))
    assert not np.array_equal(a, sgbm_ref.compute(p, L, R, reading=sgbm_ref.READ_BOTTOM_CLAMPED))
