#!/usr/bin/env python3
"""Pin kit for the ORB descriptor's one unpinned reading: how the blur's column filter rounds S / 65536 when it is a tie
(include/sbm.h, sbm_orb_params; bit 128 of SBM_CV_READING).

    python tools/orb_pin_kit.py                       writes tests/golden/pin_kit_orb.npz
    python tools/verify_orb_with_opencv.py [kit]      (numpy + cv2 only) names the reading a given OpenCV implements

The frames are crafted: each is a grid of disjoint 7 x 7 blocks, and every block's centre is a tie (S = 65536 q + 32768) whose q
alternates between even (the readings differ there) and odd (they agree). The kit holds, per frame, the blurred frame under
both readings and, for every pixel that survives the border rule as a keypoint, the descriptors under both readings -- all from
the CPU restatement (oracle/orb_ref.c); tests/test_gpu_orb.py holds the engine to the same arrays. Deterministic (fixed
seeds): rerunning reproduces the committed kit bit for bit."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
OUT = ROOT / "tests" / "golden" / "pin_kit_orb.npz"
BLOCKS = 10   # 10 x 10 blocks: 70 x 70 frames


def tie_blocks(rng, count):
    """`count` 7 x 7 u8 blocks whose centre sum S is a tie, alternately with q = S >> 16 even and odd."""
    import orb_ref

    k = orb_ref.taps_np()
    w = np.outer(k, k).reshape(-1)
    found = {0: [], 1: []}
    while min(len(found[0]), len(found[1])) < (count + 1) // 2:
        cand = rng.integers(0, 256, (400000, 49), dtype=np.int64)
        s = cand @ w
        hit = (s & 0xFFFF) == 0x8000
        for c, q in zip(cand[hit], (s[hit] >> 16)):
            if q < 255:
                found[int(q & 1)].append(c.reshape(7, 7).astype(np.uint8))
    out = []
    for i in range(count):
        out.append(found[i & 1][i // 2])
    return out


def build():
    import orb_ref

    pat = np.load(ROOT / "tests" / "golden" / "orb_pattern.npz")["pattern"]
    kit = {"version": np.int32(1), "pattern": pat.astype(np.int32)}
    n = 7 * BLOCKS
    ys, xs = np.mgrid[0:n, 0:n]
    kpts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    for f in range(2):
        rng = np.random.default_rng(100 + f)
        blocks = tie_blocks(rng, BLOCKS * BLOCKS)
        img = np.zeros((n, n), np.uint8)
        for i, b in enumerate(blocks):
            by, bx = divmod(i, BLOCKS)
            img[7 * by:7 * by + 7, 7 * bx:7 * bx + 7] = b
        name = f"ties{f}"
        kit[f"{name}/img"] = img
        for hu in (0, 1):
            kk, dd, bl = orb_ref.describe(img, kpts, pat, half_up=bool(hu))
            assert np.array_equal(bl, orb_ref.blur_np(img, bool(hu)))
            kit[f"{name}/blur_r{128 * hu}"] = bl
            kit[f"{name}/desc_r{128 * hu}"] = dd
        kit[f"{name}/kpts"] = kk
        assert not np.array_equal(kit[f"{name}/blur_r0"], kit[f"{name}/blur_r128"])
        assert not np.array_equal(kit[f"{name}/desc_r0"], kit[f"{name}/desc_r128"])
    return kit


def main():
    kit = build()
    np.savez_compressed(OUT, **kit)
    print("wrote", OUT, "with", len(kit), "arrays")


if __name__ == "__main__":
    main()
