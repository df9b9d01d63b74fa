"""The SGBM pin kit (tests/golden/pin_kit_sgbm.npz) reproduces from the CPU restatement, and its verifier runs end to end with a
stand-in cv2 module that answers with the restatement under a chosen reading."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
KIT = ROOT / "tests" / "golden" / "pin_kit_sgbm.npz"
sys.path.insert(0, str(ROOT / "tools"))


def test_kit_reproduces_from_restatement():
    import sgbm_pin_kit

    kit = np.load(KIT)
    fresh = sgbm_pin_kit.build()
    assert sorted(fresh) == sorted(kit.files)
    for k in kit.files:
        np.testing.assert_array_equal(kit[k], fresh[k], err_msg=k)
    # the readings are distinguishable on the kit: every pair of readings differs on some case
    names = {k.split("/")[0] for k in kit.files if "/" in k}
    rs = [int(r) for r in kit["readings"]]
    for i, a in enumerate(rs):
        for b in rs[i + 1:]:
            assert any(not np.array_equal(kit[f"{n}/r{a}"], kit[f"{n}/r{b}"]) for n in names), (a, b)


STAND_IN = '''
import os, sys
sys.path.insert(0, {ref!r})
import numpy as np
import sgbm_ref

class _SGBM:
    def __init__(self, **kw):
        self.p = sgbm_ref.make_params(kw["minDisparity"], kw["numDisparities"], kw["blockSize"], kw["P1"], kw["P2"],
                                      kw["disp12MaxDiff"], kw["preFilterCap"], kw["uniquenessRatio"], kw["speckleWindowSize"],
                                      kw["speckleRange"], kw["mode"])
    def compute(self, left, right):
        return sgbm_ref.compute(self.p, left, right, reading=int(os.environ["STAND_IN_READING"]))

def StereoSGBM_create(**kw):
    return _SGBM(**kw)
'''


@pytest.mark.parametrize("reading", [0, 32, 64, 96])
def test_verifier_names_the_reading(tmp_path, reading):
    (tmp_path / "cv2.py").write_text(STAND_IN.format(ref=str(ROOT / "oracle")))
    env = dict(os.environ, PYTHONPATH=str(tmp_path), STAND_IN_READING=str(reading))
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "verify_sgbm_with_opencv.py"), str(KIT)], capture_output=True,
                       text=True, env=env, timeout=300)
    assert f"SUMMARY: this OpenCV implements SBM_CV_READING {reading}" in r.stdout, r.stdout + r.stderr
    assert r.returncode == (0 if reading == 0 else 1)
