"""Inputs the LK stereo tests share (CPU restatement, GPU engine, pin kit): the pyramid sizes the issue names, the point grid on
the golden pair, and small frames with points at the corners, at fractional positions and outside. TEST INFRASTRUCTURE ONLY."""
import numpy as np

# (width, height, index of the last level with the reference's 15 x 3 window and max_level 5)
PYRAMID_SIZES = [(16, 4, 0), (17, 5, 0), (33, 9, 1), (37, 11, 1), (160, 120, 3), (640, 480, 5)]
OUTSIDE = [(-20.0, 5.0), (700.0, 10.0), (5.0, -30.0), (100.0, 600.0)]


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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
