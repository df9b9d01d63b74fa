#!/usr/bin/env python3
"""Holds the RECALLED half of the LK stereo contract (include/sbm.h, "pyramidal LK stereo": the pyramid of
cv::buildOpticalFlowPyramid) against a real OpenCV. numpy + cv2 only; nothing of this repository is imported.

    python tools/verify_lk_with_opencv.py [tests/golden/pin_kit_lk.npz]

For the kit's pair it builds cv2.buildOpticalFlowPyramid(img, (15, 3), 5, withDerivatives=True) and compares, level by level, the
level count, the image plane and the derivative plane with the kit's arrays, and names the first step that disagrees (the two
paddings live in the parent matrices of OpenCV's levels, which the Python binding does not expose; they are not judged). It then runs cv2.calcOpticalFlowPyrLK on the kit's points for orientation only: OpenCV's
tracker also moves in y, so equality with the reference's x-only tracker is not expected and not judged. Exit status 0 = every
pyramid step agrees, 1 = a step disagrees, 2 = the kit could not be read."""
import pathlib
import sys

import numpy as np


def main():
    import cv2

    path = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else pathlib.Path(__file__).resolve().parents[1] / "tests" / "golden" / "pin_kit_lk.npz"
    try:
        kit = np.load(path)
        prm = kit["params"]
    except Exception as e:   # noqa: BLE001
        print("cannot read the kit:", e)
        return 2
    ww, wh, max_level = int(prm[0]), int(prm[1]), int(prm[2])
    want_levels = int(kit["levels"])
    bad = []
    for side, deriv in (("left", True), ("right", False)):
        got_levels, pyr = cv2.buildOpticalFlowPyramid(kit[side], (ww, wh), max_level if side == "left" else want_levels,
                                                      withDerivatives=deriv)
        step = 2 if deriv else 1
        print(f"{side}: OpenCV returns maxLevel {got_levels}, the kit holds {want_levels}")
        if got_levels != want_levels:
            bad.append(f"{side}: level count (OpenCV {got_levels}, kit {want_levels}): the stop rule differs")
            continue
        for k in range(want_levels + 1):
            img = np.asarray(pyr[k * step])
            want = kit[f"{side}/level{k}"]
            if img.shape != want.shape:
                bad.append(f"{side} level {k}: size (OpenCV {img.shape[::-1]}, kit {want.shape[::-1]}): the size rule differs")
                break
            if not np.array_equal(img, want):
                bad.append(f"{side} level {k}: {int((img != want).sum())} pixels differ: pyrDown's taps, border or rounding differ")
                break
            if deriv:
                d = np.asarray(pyr[k * step + 1]).reshape(want.shape + (2,))
                wd = kit[f"{side}/deriv{k}"]
                if not np.array_equal(d, wd):
                    which = "dx" if not np.array_equal(d[..., 0], wd[..., 0]) else "dy"
                    bad.append(f"{side} level {k}: the derivative plane differs first in {which}: Scharr taps or border differ")
                    break
    for b in bad:
        print("DISAGREES:", b)
    pts = kit["points"].reshape(-1, 1, 2)
    nxt, st, err = cv2.calcOpticalFlowPyrLK(kit["left"], kit["right"], pts, None, winSize=(ww, wh), maxLevel=max_level,
                                            criteria=(cv2.TERM_CRITERIA_COUNT + cv2.TERM_CRITERIA_EPS, int(prm[3]), float(prm[4])),
                                            flags=cv2.OPTFLOW_LK_GET_MIN_EIGENVALS, minEigThreshold=float(prm[6]))
    st = st.reshape(-1)
    same = st == kit["track/status"]
    print(f"orientation only: cv2.calcOpticalFlowPyrLK (x and y) agrees with the x-only tracker's status on {int(same.sum())} of "
          f"{len(st)} points; err (level-0 min eigenvalue, independent of the y update) equal on "
          f"{int((err.reshape(-1).view(np.uint32) == kit['track/err'].view(np.uint32)).sum())}")
    print("SUMMARY:", "every pyramid step agrees with this text" if not bad else f"first disagreement: {bad[0]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
