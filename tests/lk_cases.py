"""Inputs the LK stereo tests share (CPU restatement, GPU engine, pin kit): the pyramid sizes the issue names, the point grid on
the golden pair, and small frames with points at the corners, at fractional positions and outside. TEST INFRASTRUCTURE ONLY."""
import numpy as np

# (width, height, index of the last level with the reference's 15 x 3 window and max_level 5)
PYRAMID_SIZES = [(16, 4, 0), (17, 5, 0), (33, 9, 1), (37, 11, 1), (160, 120, 3), (640, 480, 5)]
OUTSIDE = [(-20.0, 5.0), (700.0, 10.0), (5.0, -30.0), (100.0, 600.0)]
# (width, height, index of the last level under max_level >= 7). The height ends a pyramid as the width does: 2048 x 40 and
# 2047 x 33 stop at level 3 (256 x 5; the next level would be 3 rows, no more than the window), and only a frame of at least 385
# rows keeps what 2048 columns allow, level 7 at 16 x 4 -- the last level the engine can hold.
DEEP_SIZES = [(2048, 40, 3), (2047, 33, 3), (2048, 512, 7), (2047, 385, 7)]


def grid_points():
    """x = 4.25 + 24 i, y = 4.25 + 24 j on 640 x 480 (540 points), then four points outside the frame."""
    pts = [(4.25 + 24 * i, 4.25 + 24 * j) for j in range(20) for i in range(27)]
    return np.array(pts + OUTSIDE, np.float32)


def noise_frame(w, h, seed=None):
    rng = np.random.default_rng(w * 1000 + h if seed is None else seed)
    return rng.integers(0, 256, (h, w)).astype(np.uint8)


def small_pair(w, h):
    """A smooth textured frame and the same one moved 1.5 px to the left (a disparity inside the gate), both w x h."""
    ys, xs = np.mgrid[0:h, 0:w + 4].astype(np.float64)
    f = 120 + 60 * np.sin(xs * 0.9) * np.cos(ys * 1.3) + 40 * np.sin(xs * 0.23 + ys * 0.51)
    rng = np.random.default_rng(w * 7 + h)
    f = np.clip(f + rng.integers(-6, 7, f.shape), 0, 255)
    left = f[:, 2:w + 2]
    right = 0.5 * (f[:, 3:w + 3] + f[:, 4:w + 4])
    return np.round(left).astype(np.uint8), np.round(right).astype(np.uint8)


def small_points(w, h):
    """Corners, the fractional positions .0 / .5 / .999 along both axes, and points outside on every side."""
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    for fx in (0.0, 0.5, 0.999):
        for fy in (0.0, 0.5, 0.999):
            pts += [(w // 2 + fx, h // 2 + fy), (1 + fx, 1 + fy), (w - 2 + fx, h - 2 + fy)]
    pts += [(-8.0, 1.0), (-8.001, 1.0), (-9.5, 1.0), (w + 7.0, 1.0), (w + 6.999, 1.0), (w + 30.0, 1.0), (3.0, -2.0), (3.0, -2.001),
            (3.0, h + 0.999), (3.0, h + 1.0), (3.0, h + 5.0), (-100.0, -100.0)]
    return np.array(pts, np.float32)


def deep_pair(w, h, d=11):
    """Texture at every scale from 6 to 1500 columns, so that the coarsest levels still pass the eigenvalue test, and the same
    one moved d columns to the left: right(x) = left(x + d)."""
    ys, xs = np.mgrid[0:h, 0:w + d].astype(np.float64)
    f = 128.0 + sum(a * np.sin(xs * (2 * np.pi / per) + ph) * np.cos(ys * (2 * np.pi / (per * 0.37)) + 0.3 * ph)
                    for per, a, ph in ((6.0, 14, 0.1), (23.0, 16, 1.0), (97.0, 18, 2.0), (410.0, 22, 0.5), (1500.0, 26, 1.7)))
    f = np.clip(f + np.random.default_rng(w + 3 * h).integers(-5, 6, f.shape), 0, 255)
    f = np.round(f).astype(np.uint8)
    return np.ascontiguousarray(f[:, :w]), np.ascontiguousarray(f[:, d:w + d])


def bound_points(w, h, last, win=(15, 3)):
    """Points whose window start iprev = floor(pt / 2^l - halfWin) is EXACTLY each bound of the level-skip test, at level 0 and at
    level `last` (cols, rows: that level's size): iprev.x = -win_w (kept), -win_w - 1 (skipped), cols - 1 (kept), cols (skipped), and
    iprev.y the same with win_h and rows. (v + halfWin) * 2^l is exact in float, so the floor sees an integer."""
    ww, wh = win
    hx, hy = (ww - 1) // 2, (wh - 1) // 2          # halfWin = (7, 1): whole numbers for the 15 x 3 window
    pts = []
    for l in sorted({0, last}):
        s = 1 << l
        cols, rows = w, h
        for _ in range(l):
            cols, rows = (cols + 1) // 2, (rows + 1) // 2
        for v in (-ww, -ww - 1, cols - 1, cols):
            pts += [((v + hx) * s, (rows // 2) * s), ((v + hx) * s + 0.5, (rows // 2) * s + 0.25)]
        for v in (-wh, -wh - 1, rows - 1, rows):
            pts += [((cols // 2) * s, (v + hy) * s), ((cols // 2) * s + 0.75, (v + hy) * s + 0.5)]
    return np.array(pts, np.float32)


def edge_points(w, h, last):
    """Points whose positions at level `last` fall on that level's first and last columns and rows, and half a column inside."""
    s = 1 << last
    xs = [0.0, s * 0.5, s - 1.0, s, w - s, w - s * 0.5, w - 1.0, w * 0.5, w * 0.5 + 0.25]
    ys = [0.0, h * 0.5 + 0.5, h - 1.0]
    return np.array([(x, y) for y in ys for x in xs], np.float32)


def tie_points(w=640, h=480):
    """A grid whose fractional parts make every cvRound of the bilinear weights a TIE at level 0: with a = m / 128 and b = n / 256
    (m, n odd), (1 - a)(1 - b) * 16384 = (128 - m)(256 - n) / 2 is an odd number of halves, exact in float -- and so are a(1 - b)
    and (1 - a) b. Round-half-to-even and round-half-away differ on each tie whose floor is even. (Quarters and halves alone
    never tie: (1 - a)(1 - b) is then a multiple of 1 / 16 and the weight a whole number; they are in the set all the same, for
    the coarser levels, where the scale 2^-l turns them into finer fractions.)"""
    pts = []
    k = 0
    for j in range(h // 24 - 1):
        for i in range(w // 24 - 1):
            m, n = 2 * ((7 * k) % 64) + 1, 2 * ((11 * k) % 128) + 1
            pts.append((16 + 24 * i + m / 128.0, 16 + 24 * j + n / 256.0))
            k += 1
    for i, a in enumerate((0.5, 0.25, 0.75)):
        for j, b in enumerate((0.5, 0.25, 0.75)):
            pts.append((200 + 40 * i + a, 120 + 40 * j + b))
    return np.array(pts, np.float32)


def weight_ties(pts, last, win=(15, 3)):
    """How many of the three rounded weights of the FIRST image's window are exact ties, summed over the points and the levels
    0..last, in the tracker's own float steps (prev = pt * 2^-l - halfWin; a, b its fractional parts)."""
    pts = np.asarray(pts, np.float32)
    half = np.array([(win[0] - 1) * 0.5, (win[1] - 1) * 0.5], np.float32)
    n = 0
    for l in range(last + 1):
        prev = pts * np.float32(1.0 / (1 << l)) - half
        ab = prev - np.floor(prev)
        a, b = ab[:, 0].astype(np.float32), ab[:, 1].astype(np.float32)
        one = np.float32(1)
        for t in ((one - a) * (one - b), a * (one - b), (one - a) * b):
            t = (t * np.float32(16384)).astype(np.float32)
            n += int((t - np.floor(t) == 0.5).sum())
    return n


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
