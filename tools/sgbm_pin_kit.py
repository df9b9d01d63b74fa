#!/usr/bin/env python3
"""Write tests/golden/pin_kit_sgbm.npz: inputs, cv::StereoSGBM parameters and this engine's outputs (via the CPU restatement
it is bit-exact against, oracle/sgbm_ref.c) under every combination of the SGBM readings nobody could pin (SBM_CV_READING bits
32 = no medianBlur, 64 = bottom rows with a clamped window). tools/verify_sgbm_with_opencv.py runs a real OpenCV on the kit
and names the reading it implements.

Layout: `<case>/left`, `<case>/right` (uint8), `<case>/params` (int32, cv::StereoSGBM::create argument order),
`<case>/r<bits>` (int16 map under SBM_CV_READING = bits), `readings` (the bit combinations), `version`.

  python tools/sgbm_pin_kit.py [out.npz]
"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
import sgbm_ref  # noqa: E402

READINGS = (0, sgbm_ref.READ_NO_MEDIAN, sgbm_ref.READ_BOTTOM_CLAMPED, sgbm_ref.READ_NO_MEDIAN | sgbm_ref.READ_BOTTOM_CLAMPED)
REF_ARGS = (-64, 128, 11, 100, 1000, 32, 0, 15, 1000, 16, sgbm_ref.MODE_HH)   # main.cpp:219-230, positionally


def _synthetic(seed, H, W, shift):
    rng = np.random.default_rng(seed)
    base = (np.cumsum(rng.integers(-9, 10, (H, W + 48)), axis=1) % 256).astype(np.uint8)
    return np.ascontiguousarray(base[:, 24:24 + W]), np.ascontiguousarray(base[:, 24 + shift:24 + shift + W])


def cases():
    g = np.load(ROOT / "tests" / "golden" / "ref_pair_640x480.npz")
    yield "ref_pair_callsite", g["rect_l"], g["rect_r"], REF_ARGS
    L, R = _synthetic(1, 48, 120, 7)
    yield "default_create_sgbm", L, R, (0, 16, 3, 0, 0, 0, 0, 0, 0, 0, sgbm_ref.MODE_SGBM)
    yield "hh_mind2_claims", L, R, (2, 32, 5, 8, 96, 1, 0, 10, 0, 0, sgbm_ref.MODE_HH)
    L, R = _synthetic(2, 37, 160, 12)
    yield "sgbm_w9_cap63_saturating", L, R, (0, 48, 9, 50, 14000, 2, 63, 5, 40, 2, sgbm_ref.MODE_SGBM)
    yield "hh_w7_negative_mind", L, R, (-16, 64, 7, 10, 200, 4, 31, 15, 30, 1, sgbm_ref.MODE_HH)


def build():
    out = {"version": np.int32(1), "readings": np.array(READINGS, np.int32)}
    for name, L, R, args in cases():
        p = sgbm_ref.make_params(*args)
        out[f"{name}/left"] = L
        out[f"{name}/right"] = R
        out[f"{name}/params"] = np.array(args, np.int32)
        for r in READINGS:
            out[f"{name}/r{r}"] = sgbm_ref.compute(p, L, R, reading=r)
    return out


def main():
    path = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "pin_kit_sgbm.npz"
    np.savez_compressed(path, **build())
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
