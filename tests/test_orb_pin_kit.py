"""The ORB pin kit (tests/golden/pin_kit_orb.npz) reproduces from the CPU restatement and tells the two readings of the blur's
tie rounding apart where it should: only at ties with an even quotient."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
KIT = ROOT / "tests" / "golden" / "pin_kit_orb.npz"
sys.path.insert(0, str(ROOT / "tools"))


def test_kit_reproduces_from_restatement():
    import orb_pin_kit

    kit = np.load(KIT)
    fresh = orb_pin_kit.build()
    assert sorted(fresh) == sorted(kit.files)
    for k in kit.files:
        np.testing.assert_array_equal(kit[k], fresh[k], err_msg=k)


def test_readings_differ_exactly_at_even_ties():
    import orb_ref

    kit = np.load(KIT)
    k = orb_ref.taps_np()
    for name in ("ties0", "ties1"):
        img = kit[f"{name}/img"].astype(np.int64)
        ext = np.pad(img, 3, mode="reflect")
        h, w = img.shape
        r = sum(k[i] * ext[:, i:i + w] for i in range(7))
        s = sum(k[j] * r[j:j + h] for j in range(7))
        even_tie = ((s & 0xFFFF) == 0x8000) & (((s >> 16) & 1) == 0) & ((s >> 16) < 255)
        diff = kit[f"{name}/blur_r0"] != kit[f"{name}/blur_r128"]
        assert np.array_equal(diff, even_tie)
        assert diff.sum() >= 50   # dense in ties of both parities: half of the 100 block centres, at least
        assert (((s & 0xFFFF) == 0x8000) & (((s >> 16) & 1) == 1)).sum() >= 50
