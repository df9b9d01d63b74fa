#!/usr/bin/env python3
"""Name the rounding reading of the ORB blur that a given OpenCV implements, from tests/golden/pin_kit_orb.npz. Needs numpy and
cv2 only (no import from this repository).

    python tools/verify_orb_with_opencv.py [tests/golden/pin_kit_orb.npz]

The reference blurs the image-sized ROI of its reflect-101 bordered buffer (a sub-matrix, no BORDER_ISOLATED). Python cannot hand
OpenCV a sub-matrix with its parent, so this script runs what that call is expected to reduce to: cv2.sepFilter2D on the whole
bordered buffer with getGaussianKernel(7, 2) in float32 (8-bit in, 8-bit out: OpenCV's fixed-point taps cvRound(256 g)), then
crops the ROI; the pixels around the ROI are the buffer's own, as in the reference. For every column it reports whether the
result matches the kit's half-to-even frame (SBM_CV_READING 0), its half-up frame (bit 128), both (no tie in that column), or
neither. As a second opinion it also runs cv2.GaussianBlur on a dense copy, which may take OpenCV's bit-exact path instead; a
frame that matches neither reading there says so."""
import sys

import numpy as np


def main():
    import cv2

    path = sys.argv[1] if len(sys.argv) > 1 else "tests/golden/pin_kit_orb.npz"
    kit = np.load(path)
    names = sorted({k.split("/")[0] for k in kit.files if "/" in k})
    g = cv2.getGaussianKernel(7, 2.0, ktype=cv2.CV_32F)
    verdict = set()
    for name in names:
        img = kit[f"{name}/img"]
        even, up = kit[f"{name}/blur_r0"], kit[f"{name}/blur_r128"]
        ext = cv2.copyMakeBorder(img, 23, 23, 23, 23, cv2.BORDER_REFLECT_101)
        sep = cv2.sepFilter2D(ext, cv2.CV_8U, g, g, borderType=cv2.BORDER_REFLECT_101)[23:-23, 23:-23]
        dense = cv2.GaussianBlur(img.copy(), (7, 7), 2.0, sigmaY=2.0, borderType=cv2.BORDER_REFLECT_101)
        for label, out in (("sepFilter2D (the reference's path)", sep), ("GaussianBlur on a dense copy", dense)):
            cols = []
            for x in range(img.shape[1]):
                e = np.array_equal(out[:, x], even[:, x])
                u = np.array_equal(out[:, x], up[:, x])
                cols.append("both" if e and u else "half_even" if e else "half_up" if u else "neither")
            kinds = {c: cols.count(c) for c in set(cols)}
            print(f"{name} {label}: columns {kinds}")
            if label.startswith("sep"):
                verdict |= set(cols) - {"both"}
    if verdict == {"half_even"}:
        print("VERDICT: half to even -- the default reading (SBM_CV_READING bit 128 clear)")
    elif verdict == {"half_up"}:
        print("VERDICT: half up -- set bit 128 of SBM_CV_READING, or flip the default")
    else:
        print(f"VERDICT: per-column mixture or neither: {sorted(verdict)}")


if __name__ == "__main__":
    main()
