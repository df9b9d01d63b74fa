#!/usr/bin/env python3
"""Pin kit for the OpenCV-flavour keypoint detector (include/sbm.h, "GFTT keypoints of OpenCV"): what this engine computes for a
few small frames under reading 0 and under bit 512 of SBM_CV_READING (fused multiply-adds in the scaled three-tap and in the
radicand), for whoever has an OpenCV at hand.

    python tools/gftt_cv_pin_kit.py                        writes tests/golden/pin_kit_gftt_cv.npz
    python tools/verify_gftt_cv_with_opencv.py [kit]       (numpy + cv2 only) names the reading a given OpenCV implements

Per frame and reading the kit holds the float map of cornerMinEigenVal(img, 3, 3), its maximum, and the keypoints of
goodFeaturesToTrack(img, 1500, 0.01, 7.0, blockSize 3) in order -- all from the CPU restatement (oracle/gftt_cv_ref);
tests/test_gftt_cv_pin_kit.py regenerates them bit for bit. The frames: a crop of the golden left frame, noise, noise of low
contrast (small derivatives: where a fused sum differs most often), and two identical corners whose responses tie exactly (the
order of a tie is the reference's greaterThanPtr; a stock OpenCV may order it differently, and the verifier says so).
Deterministic."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
OUT = ROOT / "tests" / "golden" / "pin_kit_gftt_cv.npz"
READINGS = (0, 512)
PARAMS = (1500, 0.01, 7.0)


def frames():
    g = np.load(ROOT / "tests" / "golden" / "ref_pair_640x480.npz")
    rng = np.random.default_rng(31)
    tie = np.full((40, 52), 10, np.uint8)
    tie[8:16, 8:16] = 250
    tie[8:16, 30:38] = 250
    return {"golden_crop": np.ascontiguousarray(g["rect_l"][300:396, 300:428]),
            "noise": rng.integers(0, 256, (48, 64)).astype(np.uint8),
            "noise_low": rng.integers(100, 104, (48, 64)).astype(np.uint8),
            "tie_corners": tie}


def build():
    import gftt_cv_ref as ref

    kit = {"version": np.int32(1), "readings": np.array(READINGS, np.int32), "params": np.array(PARAMS, np.float64)}
    try:
        for name, img in frames().items():
            kit[f"{name}/img"] = img
            for r in READINGS:
                ref.set_reading(r)
                pts, e, m, _ = ref.detect(img, int(PARAMS[0]), PARAMS[1], PARAMS[2])
                kit[f"{name}/map_r{r}"] = e
                kit[f"{name}/max_r{r}"] = np.float32(m)
                kit[f"{name}/kpts_r{r}"] = pts
    finally:
        ref.set_reading(0)
    assert any(not np.array_equal(kit[f"{n}/map_r0"].view(np.uint32), kit[f"{n}/map_r512"].view(np.uint32)) for n in frames())
    return kit


def main():
    kit = build()
    np.savez_compressed(OUT, **kit)
    print("wrote", OUT, "with", len(kit), "arrays")


if __name__ == "__main__":
    main()
