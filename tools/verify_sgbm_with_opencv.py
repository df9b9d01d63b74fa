#!/usr/bin/env python3
"""Stand-alone check of the SGBM pin kit against the real cv::StereoSGBM. Needs numpy and cv2 (any OpenCV >= 3) -- nothing from
this repository.  usage: python verify_sgbm_with_opencv.py pin_kit_sgbm.npz

For every case it runs cv2.StereoSGBM_create with the stored parameters on the stored pair and compares the CV_16S map with the
engine's map under each stored reading of SBM_CV_READING (bit 32: no medianBlur stage, bit 64: bottom rows with a clamped
window). It prints, per case, the readings that agree (or the pixel count of the closest one), and at the end the reading that
agrees on every case -- the engine's default is 0; any other value is a default flip (u96-slam_amd/csrc/sbm_common.h
kReadSgbm*, oracle/sgbm_ref.c SGBMR_READ_*). Exit code 0 = reading 0 agrees everywhere."""
import sys

import numpy as np


def main():
    import cv2

    kit = np.load(sys.argv[1])
    readings = [int(r) for r in kit["readings"]]
    names = sorted({k.split("/")[0] for k in kit.files if "/" in k})
    agree_all = set(readings)
    for name in names:
        a = [int(v) for v in kit[f"{name}/params"]]
        sg = cv2.StereoSGBM_create(minDisparity=a[0], numDisparities=a[1], blockSize=a[2], P1=a[3], P2=a[4], disp12MaxDiff=a[5],
                                   preFilterCap=a[6], uniquenessRatio=a[7], speckleWindowSize=a[8], speckleRange=a[9], mode=a[10])
        disp = np.asarray(sg.compute(kit[f"{name}/left"], kit[f"{name}/right"]), dtype=np.int16)
        diffs = {r: int((disp != kit[f"{name}/r{r}"]).sum()) for r in readings}
        ok = {r for r, d in diffs.items() if d == 0}
        agree_all &= ok
        if ok:
            print(f"{name}: agrees under reading(s) {sorted(ok)}")
        else:
            r = min(diffs, key=diffs.get)
            print(f"{name}: NO reading agrees; closest {r} with {diffs[r]} differing pixels")
    if agree_all:
        print(f"SUMMARY: this OpenCV implements SBM_CV_READING {sorted(agree_all)[0]}" +
              ("" if 0 in agree_all else " -- flip the engine's default to it"))
    else:
        print("SUMMARY: no stored reading agrees on every case")
    return 0 if 0 in agree_all else 1


if __name__ == "__main__":
    sys.exit(main())
