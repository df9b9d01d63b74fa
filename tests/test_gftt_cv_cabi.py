"""The OpenCV-flavour detector's C-ABI without a GPU: the reference's constants as defaults, a status code for every validation
failure, the limits, and the C++ adaptor compiling against the library (plain, and with the reference's signature against the
OpenCV mocks)."""
import math
import pathlib

import pytest

from gpu_support import build_callsite

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_defaults_are_the_reference_constants(pkg):
    p = pkg.GfttCvParams()
    pkg.gftt_cv_validate(p, 3, 3)   # binds the argument types
    pkg.load_library().sbm_gftt_cv_params_default(p)
    assert (p.max_features, p.quality_level, p.min_distance, p.block_size, p.use_harris, p.k) == (1500, 0.01, 7.0, 3, 0, 0.04)
    assert pkg.gftt_cv_validate(p, 640, 480) == 0
    q = pkg.gftt_cv_params()
    assert bytes(p) == bytes(q)


@pytest.mark.parametrize("change,w,h,code", [
    ({}, 3, 3, 0), ({}, 2, 3, -2), ({}, 3, 2, -2), ({}, 0, 10, -2), ({}, 10, -1, -2),
    ({}, 2048, 2048, 0), ({}, 2049, 10, -23), ({}, 10, 2049, -23),
    ({"quality_level": 0.0}, 64, 10, 0), ({"quality_level": 1e300}, 64, 10, 0), ({"quality_level": -1e-9}, 64, 10, -23),
    ({"quality_level": math.inf}, 64, 10, -23), ({"quality_level": math.nan}, 64, 10, -23),
    ({"min_distance": 0.0}, 64, 10, 0), ({"min_distance": 255.0}, 64, 10, 0), ({"min_distance": 255.0001}, 64, 10, -23),
    ({"min_distance": -0.5}, 64, 10, -23), ({"min_distance": math.inf}, 64, 10, -23), ({"min_distance": math.nan}, 64, 10, -23),
    ({"max_features": -5}, 64, 10, 0), ({"max_features": 0}, 64, 10, 0),
    ({"block_size": 0}, 64, 10, -23), ({"block_size": 5}, 64, 10, -23), ({"block_size": 3}, 64, 10, 0),
    ({"use_harris": 1}, 64, 10, -23), ({"k": 0.5}, 64, 10, 0),
])
def test_validate_status_codes(pkg, change, w, h, code):
    p = pkg.gftt_cv_params()
    for k, v in change.items():
        setattr(p, k, v)
    assert pkg.gftt_cv_validate(p, w, h) == code


def test_null_arguments(pkg):
    L = pkg.load_library()
    pkg.gftt_cv_validate(pkg.gftt_cv_params(), 3, 3)
    assert L.sbm_gftt_cv_params_validate(None, 64, 64) == -1
    L.sbm_gftt_cv_params_default(None)   # tolerated
    p = pkg.gftt_cv_params()
    import ctypes
    assert L.sbm_gftt_cv_eig_device(None, 1, None, 64, 64, None, None, 1) == -1
    assert L.sbm_gftt_cv_detect_device(None, 1, None, 64, 64, ctypes.byref(p), None, None, None, None, 1) == -1
    assert L.sbm_gftt_cv_select_device(None, 1, None, None, 64, 64, ctypes.byref(p), None, None, 1) == -1
    assert L.sbm_gftt_cv_detect(None, None, 64, 64, 64, ctypes.byref(p), None, 0, None) == -1
    assert L.sbm_orb_features_cv_device(None, 1, None, 64, 64, ctypes.byref(p), None, None, None, None, None, None, None, None,
                                        1) == -1


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_opencv"])
def test_adaptor_compiles_and_links(tmp_path, pkg, mock):
    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")] if mock else []
    _, r = build_callsite(tmp_path, "gftt_cv_callsite_main.cpp", extra, flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr
