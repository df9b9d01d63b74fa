"""Shared inputs of the OpenCV-flavour GFTT tests (generateKeypoints, include/sbm.h "GFTT keypoints of OpenCV"): crafted frames,
random cases and the reading bits. Imported by the test files, not collected."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
from gftt_select_cases import PARAM_EDGES  # noqa: E402,F401

READINGS = (0, 512)


def crafted_frames(H=40, W=52):
    """name -> uint8 frame. `tie_corners`: two identical isolated corners, so the two strongest responses tie exactly.
    `periodic`: f(x) + g(y) of a period-6 pattern that reflect-101 continues, so the responses repeat exactly: many tied local
    maxima and tied 3 x 3 plateaus. (No frame makes EVERY interior pixel a candidate: the reflected border forces dx = 0 in column
    0 and dy = 0 in row 0, so the box sums next to the border differ from the ones further in; that case enters through the
    map-level selection, see plateau_maps.)"""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    out = {}
    out["constant"] = np.full((H, W), 93, np.uint8)
    step = np.zeros((H, W), np.uint8)
    step[:, W // 2:] = 200
    out["step_edge"] = step
    out["checkerboard"] = (((xx // 4 + yy // 4) & 1) * 255).astype(np.uint8)
    out["checkerboard_1px"] = (((xx + yy) & 1) * 255).astype(np.uint8)
    tie = np.full((H, W), 10, np.uint8)
    tie[8:16, 8:16] = 250
    tie[8:16, 30:38] = 250
    out["tie_corners"] = tie
    pat = np.array([0, 1, 2, 3, 2, 1]) * 40
    out["periodic"] = (pat[xx % 6] + pat[yy % 6]).astype(np.uint8)
    out["noise"] = rng.integers(0, 256, (H, W)).astype(np.uint8)
    out["noise_low"] = rng.integers(100, 104, (H, W)).astype(np.uint8)
    return out


def plateau_maps(H=40, W=52):
    """name -> (float32 map, maximum) for the map-level selection: every interior pixel a candidate, and friends."""
    rng = np.random.default_rng(6)
    out = {}
    out["plateau"] = (np.full((H, W), 0.25, np.float32), np.float32(0.25))
    out["zeros"] = (np.zeros((H, W), np.float32), np.float32(0))
    two = np.where(rng.random((H, W)) < 0.5, 0.5, 0.125).astype(np.float32)
    out["two_levels"] = (two, np.float32(0.5))
    neg = np.full((H, W), -1e-9, np.float32)
    neg[5, 7] = -1e-10
    out["negative"] = (neg, np.float32(-1e-10))
    rnd = (rng.random((H, W)) ** 8).astype(np.float32)
    out["random"] = (rnd, rnd.max())
    out["max_above"] = (rnd, np.float32(7.0))
    return out


def random_case(rng):
    H, W = int(rng.integers(3, 90)), int(rng.integers(3, 120))
    kind = rng.integers(0, 4)
    if kind == 0:
        img = rng.integers(0, 256, (H, W))
    elif kind == 1:
        img = rng.integers(0, 4, (H, W)) * 80
    elif kind == 2:
        img = np.kron(rng.integers(0, 256, ((H + 4) // 5, (W + 4) // 5)), np.ones((5, 5), np.int64))[:H, :W]
    else:
        img = np.clip(rng.normal(128, 3, (H, W)), 0, 255)
    mf = int(rng.choice([-1, 0, 1, 7, 100, 1500]))
    q = float(rng.choice([0.0, 1e-4, 0.01, 0.2, 0.9, 1.0]))
    md = float(rng.choice([0.0, 0.99, 1.0, 1.5, 2.5, 3.0, 7.0, 7.4, 20.0]))
    return img.astype(np.uint8), mf, q, md
