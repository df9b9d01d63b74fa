#!/usr/bin/env python3
"""Name the reading of cv::goodFeaturesToTrack's arithmetic that a given OpenCV implements, from
tests/golden/pin_kit_gftt_cv.npz. Needs numpy and cv2 only (no import from this repository).

    python tools/verify_gftt_cv_with_opencv.py [tests/golden/pin_kit_gftt_cv.npz]

Per frame it runs cv2.cornerMinEigenVal(img, 3, ksize=3) and compares the float map bit for bit with the kit's map under every
reading, then cv2.goodFeaturesToTrack at the kit's parameters and compares the points in order (and, where the order differs,
as sets: a stock OpenCV leaves ties to std::sort). Prints one line per frame and a SUMMARY line; exit status 0 when every frame
matches reading 0, 1 when another single reading matches everywhere, 2 otherwise.

cv2 is not installed where this project is developed, so the cv2 calls below have never run against a real OpenCV; the script's
logic is exercised with a stand-in module (tests/test_gftt_cv_pin_kit.py)."""
import sys

import numpy as np


def main():
    import cv2

    path = sys.argv[1] if len(sys.argv) > 1 else "tests/golden/pin_kit_gftt_cv.npz"
    kit = np.load(path)
    readings = [int(r) for r in kit["readings"]]
    mf, q, md = int(kit["params"][0]), float(kit["params"][1]), float(kit["params"][2])
    names = sorted({k.split("/")[0] for k in kit.files if "/" in k})
    everywhere = set(readings)
    for name in names:
        img = kit[f"{name}/img"]
        eig = np.asarray(cv2.cornerMinEigenVal(img, 3, ksize=3), np.float32)
        pts = cv2.goodFeaturesToTrack(img, mf, q, md, blockSize=3, useHarrisDetector=False)
        pts = np.zeros((0, 2), np.float32) if pts is None else np.asarray(pts, np.float32).reshape(-1, 2)
        hit = []
        notes = []
        for r in readings:
            want = kit[f"{name}/map_r{r}"]
            same_map = eig.shape == want.shape and np.array_equal(eig.view(np.uint32), want.view(np.uint32))
            kp = kit[f"{name}/kpts_r{r}"]
            same_pts = kp.shape == pts.shape and np.array_equal(kp, pts)
            same_set = sorted(map(tuple, kp.tolist())) == sorted(map(tuple, pts.tolist()))
            if same_map:
                hit.append(r)
                notes.append(f"r{r}: map equal, points {'equal' if same_pts else 'same set, other order' if same_set else 'DIFFER'}")
            else:
                bad = int((eig.view(np.uint32) != want.view(np.uint32)).sum()) if eig.shape == want.shape else -1
                notes.append(f"r{r}: map differs in {bad} pixels")
        everywhere &= set(hit)
        print(f"{name}: " + "; ".join(notes))
    if 0 in everywhere:
        print("SUMMARY: this OpenCV implements SBM_CV_READING 0 (the default) on every frame")
        return 0
    if len(everywhere) == 1:
        print(f"SUMMARY: this OpenCV implements SBM_CV_READING {everywhere.pop()} on every frame: set that bit, or flip the default")
        return 1
    print("SUMMARY: no single reading matches every frame: the restated arithmetic needs another look (include/sbm.h)")
    return 2


if __name__ == "__main__":
    sys.exit(main())
