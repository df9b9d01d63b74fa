"""The pin kit (tools/pin_kit.py, tests/golden/pin_kit.npz) against this engine: the kit holds the engine's stage-by-stage
outputs for every risk case of SURVEY.md A.7, and these tests keep it current. The comparison with the real cv::StereoBM
(SURVEY.md 8c last row) needs OpenCV, which no machine this suite runs on has
(profiles/r02_opencv_probe.txt): it is made off-box with `python tools/verify_with_opencv.py tests/golden/pin_kit.npz`
(numpy + cv2 only)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- the pin kit (tools/pin_kit.py): one case per risk item of SURVEY.md A.7 + getValidDisparityROI's "- minDisparity" --------
def _kit():
    import pathlib

    path = pathlib.Path(__file__).resolve().parents[1] / "tests" / "golden" / "pin_kit.npz"
    if not path.exists():
        pytest.skip("tests/golden/pin_kit.npz not generated yet (python tools/pin_kit.py on a GPU box)")
    return np.load(path)


def _engine(pkg, q):
    bm = pkg.StereoBM.create(q["num_disparities"], q["block_size"])
    bm.setPreFilterType(q["prefilter_type"]); bm.setPreFilterSize(q["prefilter_size"]); bm.setPreFilterCap(q["prefilter_cap"])
    bm.setMinDisparity(q["min_disparity"]); bm.setTextureThreshold(q["texture_threshold"]); bm.setUniquenessRatio(q["uniqueness_ratio"])
    bm.setSpeckleWindowSize(q["speckle_window_size"]); bm.setSpeckleRange(q["speckle_range"]); bm.setDisp12MaxDiff(q["disp12_max_diff"])
    bm.setROI1((q["roi1_x"], q["roi1_y"], q["roi1_w"], q["roi1_h"])); bm.setROI2((q["roi2_x"], q["roi2_y"], q["roi2_w"], q["roi2_h"]))
    return bm


def _stage(p, st):
    q = dict(p)
    if st == "s0_wta":
        q.update(uniqueness_ratio=0, texture_threshold=0, disp12_max_diff=-1, speckle_window_size=0, speckle_range=0)
    elif st == "s1_uniq":
        q.update(disp12_max_diff=-1, speckle_window_size=0, speckle_range=0)
    elif st == "s2_lr":
        q.update(speckle_window_size=0, speckle_range=0)
    return q


def test_engine_reproduces_the_pin_kit(pkg):
    """No OpenCV needed: the committed kit is what THIS engine computes today (a kernel change that moves a single pixel of any
    risk case fails here, before anybody spends an OpenCV box on a stale kit)."""
    kit = _kit()
    fields = [str(f) for f in kit["fields"]]
    for name in kit["names"]:
        name = str(name)
        p = dict(zip(fields, kit[f"{name}/params"].tolist()))
        for st in kit["stages"]:
            got = _engine(pkg, _stage(p, str(st))).compute(kit[f"{name}/left"], kit[f"{name}/right"])
            assert np.array_equal(got, kit[f"{name}/{st}"]), (name, str(st), int((got != kit[f"{name}/{st}"]).sum()))


def test_engine_reproduces_the_alternative_readings_of_the_kit(pkg, monkeypatch):
    """Kit v2: the engine under each bit of SBM_CV_READING (the alternative reading of a cv::StereoBM behaviour nobody could pin)
    still produces what the kit stores for the cases that tell the readings apart."""
    kit = _kit()
    fields = [str(f) for f in kit["fields"]]
    n = 0
    for b, cs in zip(kit["risk_bits"].tolist(), kit["risk_cases"].tolist()):
        monkeypatch.setenv("SBM_CV_READING", str(int(b)))
        for name in str(cs).split(","):
            p = dict(zip(fields, kit[f"{name}/params"].tolist()))
            for st in kit["stages"]:
                got = _engine(pkg, _stage(p, str(st))).compute(kit[f"{name}/left"], kit[f"{name}/right"])
                want = kit[f"{name}/alt{b}/{st}"]
                assert np.array_equal(got, want), (name, int(b), str(st), int((got != want).sum()))
                n += 1
    assert n >= 4 * 9
