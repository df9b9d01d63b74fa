"""The LK stereo pin kit (tests/golden/pin_kit_lk.npz) reproduces bit for bit from the CPU restatement, and holds what its
verifier reads."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
KIT = ROOT / "tests" / "golden" / "pin_kit_lk.npz"
sys.path.insert(0, str(ROOT / "tools"))


def test_kit_reproduces_from_restatement():
    import lk_pin_kit

    kit = np.load(KIT)
    fresh = lk_pin_kit.build()
    assert sorted(fresh) == sorted(kit.files)
    for k in kit.files:
        a, b = kit[k], np.asarray(fresh[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k
    assert KIT.stat().st_size <= 150 * 1024


def test_kit_contents():
    kit = np.load(KIT)
    assert kit["left"].shape == kit["right"].shape == (120, 160) and kit["points"].shape == (64, 2)
    last = int(kit["levels"])
    assert last == 3
    w, h = 160, 120
    for k in range(last + 1):
        assert kit[f"left/level{k}"].shape == kit[f"right/level{k}"].shape == (h, w)
        assert kit[f"left/deriv{k}"].shape == (h, w, 2) and kit[f"left/deriv{k}"].dtype == np.int16
        w, h = (w + 1) // 2, (h + 1) // 2
    assert np.array_equal(kit["left/level0"], kit["left"])
    st, gs = kit["track/status"], kit["gated/status"]
    assert st.sum() >= 8 and (st == 0).sum() >= 4 and (gs <= st).all()
