"""The detector's pin kit (tests/golden/pin_kit_gftt_cv.npz) reproduces bit for bit from the CPU restatement, and its verifier
runs end to end with a stand-in cv2 module that answers with the restatement under a chosen reading."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
KIT = ROOT / "tests" / "golden" / "pin_kit_gftt_cv.npz"
sys.path.insert(0, str(ROOT / "tools"))


def test_kit_reproduces_from_restatement():
    import gftt_cv_pin_kit

    kit = np.load(KIT)
    fresh = gftt_cv_pin_kit.build()
    assert sorted(fresh) == sorted(kit.files)
    for k in kit.files:
        a, b = kit[k], np.asarray(fresh[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k
    names = {k.split("/")[0] for k in kit.files if "/" in k}
    assert any(kit[f"{n}/map_r0"].tobytes() != kit[f"{n}/map_r512"].tobytes() for n in names)
    assert KIT.stat().st_size < 400 * 1024


STAND_IN = '''
import os, sys
sys.path.insert(0, {ref!r})
import numpy as np
import gftt_cv_ref

def cornerMinEigenVal(img, blockSize, ksize=3):
    assert blockSize == 3 and ksize == 3
    gftt_cv_ref.set_reading(int(os.environ["STAND_IN_READING"]))
    return gftt_cv_ref.eig_map(img)[0]

def goodFeaturesToTrack(img, maxCorners, qualityLevel, minDistance, blockSize=3, useHarrisDetector=False):
    gftt_cv_ref.set_reading(int(os.environ["STAND_IN_READING"]))
    p = gftt_cv_ref.detect(img, maxCorners, qualityLevel, minDistance)[0]
    return p.reshape(-1, 1, 2) if len(p) else None
'''


@pytest.mark.parametrize("reading", [0, 512])
def test_verifier_names_the_reading(tmp_path, reading):
    (tmp_path / "cv2.py").write_text(STAND_IN.format(ref=str(ROOT / "oracle")))
    env = dict(os.environ, PYTHONPATH=str(tmp_path), STAND_IN_READING=str(reading))
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "verify_gftt_cv_with_opencv.py"), str(KIT)], capture_output=True,
                       text=True, env=env, timeout=300)
    assert f"SUMMARY: this OpenCV implements SBM_CV_READING {reading}" in r.stdout, r.stdout + r.stderr
    assert r.returncode == (0 if reading == 0 else 1)
