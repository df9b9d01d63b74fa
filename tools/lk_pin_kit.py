#!/usr/bin/env python3
"""Pin kit for the pyramidal LK stereo path (include/sbm.h, "pyramidal LK stereo"): what this engine computes for a 160 x 120
crop of the golden pair and 64 points, for whoever has an OpenCV at hand.

    python tools/lk_pin_kit.py                        writes tests/golden/pin_kit_lk.npz
    python tools/verify_lk_with_opencv.py [kit]       (numpy + cv2 only) compares cv2.buildOpticalFlowPyramid level by level

The kit holds the pair, the points, every pyramid level of both images, every derivative plane of the left one, and the tracker's
outputs before the gate (right points, status, err) and the status after it -- all from the CPU restatement
(oracle/lk_stereo_ref); tests/test_lk_pin_kit.py regenerates them bit for bit. The pyramid is the half nothing in the reference
pins (it is OpenCV's); the tracker is the reference's own source. Deterministic."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
OUT = ROOT / "tests" / "golden" / "pin_kit_lk.npz"
CROP = (slice(180, 300), slice(240, 400))   # rows, columns of the golden pair: 160 x 120


def inputs():
    g = np.load(ROOT / "tests" / "golden" / "ref_pair_640x480.npz")
    left, right = np.ascontiguousarray(g["rect_l"][CROP]), np.ascontiguousarray(g["rect_r"][CROP])
    # an 8 x 8 grid at quarter-pixel offsets, the corners pulled to the frame's edge
    pts = np.array([(6.25 + 21 * i + 0.25 * (j % 4), 5.5 + 15.5 * j + 0.25 * (i % 3)) for j in range(8) for i in range(8)], np.float32)
    pts[0], pts[7], pts[56], pts[63] = (0.0, 0.0), (159.0, 0.0), (0.0, 119.0), (159.0, 119.0)
    return left, right, pts


def build():
    import lk_stereo_ref as ref

    left, right, pts = inputs()
    p = ref.params()
    kit = {"version": np.int32(1), "left": left, "right": right, "points": pts,
           "params": np.array([p.win_width, p.win_height, p.max_level, p.max_count, p.epsilon, p.flags, p.min_eig_threshold,
                               p.min_disparity, p.max_disparity], np.float64)}
    lv_l, dv_l = ref.pyramid(left, p)
    lv_r, _ = ref.pyramid(right, p, with_deriv=False)
    kit["levels"] = np.int32(len(lv_l) - 1)
    for k, (a, b, d) in enumerate(zip(lv_l, lv_r, dv_l)):
        kit[f"left/level{k}"], kit[f"right/level{k}"], kit[f"left/deriv{k}"] = a, b, d
    out, st, err, info, _ = ref.track(left, right, pts, p)
    kit["track/right_pts"], kit["track/status"], kit["track/err"], kit["track/exit"] = out, st, err, info
    kit["gated/status"] = ref.gate(pts, out, st, p)
    assert st.sum() >= 8 and (st == 0).sum() >= 4
    return kit


def main():
    kit = build()
    np.savez_compressed(OUT, **kit)
    print("wrote", OUT, "with", len(kit), "arrays,", OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
