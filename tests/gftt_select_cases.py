"""Shared inputs of the GFTT keypoint-selection tests: a literal Python transcription of generateKeypoints2
(src/slam/src/core/GFTT.cpp:41-170), the crafted maps and the parameter edges. Imported by the test files, not collected."""
import math

import numpy as np

# (max_features, quality_level, min_distance)
PARAM_EDGES = ([(1500, 0.01, d) for d in (0.0, 0.99, 1.0, 2.5, 3.5, 7.0, 7.4, 255.0)] +
               [(1500, q, 7.0) for q in (0.0, 1.0, 2.0)] +
               [(m, 0.01, 7.0) for m in (-1, 0, 1, 10 ** 6)] +
               [(m, 0.0, 2.5) for m in (-1, 1, 37)])


def literal_generate_keypoints2(eig, mx, nfeatures=1500, qualityLevel=0.01, minDistance=7.0):
    """GFTT.cpp:41-170 line by line. Addresses are raster indices y * W + x (the order of a strided map's addresses too)."""
    H, W = eig.shape
    thr = float(int(mx) & 0xffff) * qualityLevel
    tmp = []
    for y in range(1, H - 1):
        for x in range(1, W - 1):
            val = float(np.float32(eig[y, x]))
            if val >= thr:
                tmp.append((int(eig[y, x]), y * W + x))
    tmp.sort(key=lambda t: (-t[0], -t[1]))          # greaterThanPtr
    corners = []
    if minDistance >= 1:
        cell = int(round(minDistance))               # cvRound: half to even, as Python's round
        gw, gh = (W + cell - 1) // cell, (H + cell - 1) // cell
        grid = [[] for _ in range(gw * gh)]
        md2 = minDistance * minDistance
        for _, ofs in tmp:
            y, x = divmod(ofs, W)
            good = True
            xc, yc = x // cell, y // cell
            x1, y1, x2, y2 = max(0, xc - 1), max(0, yc - 1), min(gw - 1, xc + 1), min(gh - 1, yc + 1)
            for yy in range(y1, y2 + 1):
                for xx in range(x1, x2 + 1):
                    for (px, py) in grid[yy * gw + xx]:
                        dx, dy = np.float32(x - px), np.float32(y - py)
                        if float(dx * dx + dy * dy) < md2:
                            good = False
                            break
                    if not good:
                        break
                if not good:
                    break
            if good:
                grid[yc * gw + xc].append((float(x), float(y)))
                corners.append((float(x), float(y)))
                if nfeatures > 0 and len(corners) == nfeatures:
                    break
    else:
        for _, ofs in tmp:
            y, x = divmod(ofs, W)
            corners.append((float(x), float(y)))
            if nfeatures > 0 and len(corners) == nfeatures:
                break
    return np.array(corners, np.float32).reshape(-1, 2)


def crafted_maps(H=40, W=52):
    """name -> (map, max register)"""
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W]
    out = {}
    out["zeros_max0"] = (np.zeros((H, W), np.uint16), 0)
    out["constant"] = (np.full((H, W), 777, np.uint16), 777)
    out["ramp_x"] = ((xx * 40 + 5).astype(np.uint16), int(xx.max() * 40 + 5))
    out["ramp_xy"] = ((xx * 13 + yy * 7).astype(np.uint16), int((xx * 13 + yy * 7).max()))
    plate = rng.integers(0, 4, (H, W)).astype(np.uint16) * 1000        # large tied plateaus
    out["plateaus"] = (plate, int(plate.max()))
    rnd = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    out["max_above"] = (rnd, 65535)                                      # register above the true maximum
    out["max_below"] = (rnd, int(rnd.max()) // 3)                        # below it: more candidates
    out["max_high_bits"] = (rnd, 0x12340000 | int(rnd.max()))            # only the low 16 bits count
    sparse = np.where(rng.random((H, W)) < 0.05, rng.integers(1, 65536, (H, W)), 0).astype(np.uint16)
    out["sparse_peaks"] = (sparse, int(sparse.max()))
    return out


def random_case(rng):
    """A seeded (map, max, params) draw for the fuzz."""
    H, W = int(rng.integers(3, 48)), int(rng.integers(3, 64))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        m = rng.integers(0, 65536, (H, W))
    elif kind == 1:
        m = rng.integers(0, 6, (H, W)) * int(rng.integers(1, 10000))
    elif kind == 2:
        m = rng.integers(0, 300, (H, W))
    else:
        m = np.where(rng.random((H, W)) < 0.2, rng.integers(0, 65536, (H, W)), rng.integers(0, 3, (H, W)))
    m = m.astype(np.uint16)
    mx = int(m.max()) if rng.random() < 0.7 else int(rng.integers(0, 65536))
    mf = int(rng.choice([-1, 0, 1, 5, 50, 1500]))
    q = float(rng.choice([0.0, 0.01, 0.1, 0.5, 1.0, float(rng.random())]))
    md = float(rng.choice([0.0, 0.5, 1.0, 1.5, 2.5, 3.5, 5.0, 7.0, 7.4, 12.6, 30.0, float(rng.random() * 20)]))
    return m, mx, mf, q, md
