"""The LK stereo C-ABI without a GPU: the reference's constants as defaults, a status code for every validation failure, the
limits, null arguments, and the C++ adaptor compiling against the library (plain, and with the reference's signature against
the OpenCV mocks)."""
import ctypes
import math
import pathlib
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
from gpu_support import build_callsite  # noqa: E402


def test_defaults_are_the_reference_constants(pkg):
    p = pkg.LkParams()
    pkg.lk_validate(p, 16, 4)   # binds the argument types
    pkg.load_library().sbm_lk_params_default(p)
    assert (p.win_width, p.win_height, p.max_level, p.max_count, p.flags) == (15, 3, 5, 30, pkg.LK_GET_MIN_EIGENVALS)
    assert p.epsilon == ctypes.c_float(0.01).value and p.min_eig_threshold == 1e-4
    assert (p.min_disparity, p.max_disparity) == (0.5, 128.0)
    assert pkg.lk_validate(p, 640, 480) == 0
    assert bytes(p) == bytes(pkg.lk_params())
    assert ctypes.sizeof(p) == 40


def test_struct_matches_the_restatements():
    import lk_stereo_ref as ref

    assert [f[0] for f in ref.Params._fields_] == ["win_width", "win_height", "max_level", "max_count", "epsilon", "flags",
                                                   "min_eig_threshold", "min_disparity", "max_disparity"]
    assert ctypes.sizeof(ref.Params) == 40


@pytest.mark.parametrize("change,w,h,code", [
    ({}, 16, 4, 0), ({}, 2, 2, 0), ({}, 1, 10, -2), ({}, 10, 1, -2), ({}, 0, 10, -2), ({}, 10, -1, -2),
    ({}, 2048, 2048, 0), ({}, 2049, 10, -23), ({}, 10, 2049, -23),
    ({"win_width": 2}, 64, 48, -2), ({"win_height": 2}, 64, 48, -2), ({"max_level": -1}, 64, 48, -2),
    ({"win_width": 21}, 64, 48, -23), ({"win_height": 5}, 64, 48, -23), ({"win_width": 3, "win_height": 15}, 64, 48, -23),
    ({"max_level": 0}, 64, 48, 0), ({"max_level": 50}, 64, 48, 0),
    ({"max_count": -5}, 64, 48, 0), ({"max_count": 0}, 64, 48, 0), ({"max_count": 1000}, 64, 48, 0),
    ({"epsilon": 0.0}, 64, 48, 0), ({"epsilon": -1.0}, 64, 48, 0), ({"epsilon": 50.0}, 64, 48, 0),
    ({"epsilon": math.inf}, 64, 48, -23), ({"epsilon": math.nan}, 64, 48, -23),
    ({"flags": 0}, 64, 48, -23), ({"flags": 4}, 64, 48, -23), ({"flags": 12}, 64, 48, -23), ({"flags": 9}, 64, 48, -23),
    ({"min_eig_threshold": 0.0}, 64, 48, 0), ({"min_eig_threshold": math.nan}, 64, 48, -23),
    ({"min_eig_threshold": math.inf}, 64, 48, -23),
    ({"max_disparity": -1.0}, 64, 48, 0), ({"max_disparity": math.nan}, 64, 48, -23), ({"min_disparity": math.nan}, 64, 48, -23),
    ({"min_disparity": -5.0}, 64, 48, 0),
])
def test_validate_status_codes(pkg, change, w, h, code):
    p = pkg.lk_params()
    for k, v in change.items():
        setattr(p, k, v)
    assert pkg.lk_validate(p, w, h) == code


def test_null_arguments(pkg):
    L = pkg.load_library()
    p = pkg.lk_params()
    pkg.lk_validate(p, 16, 4)
    assert L.sbm_lk_params_validate(None, 64, 64) == -1
    L.sbm_lk_params_default(None)   # tolerated
    assert L.sbm_lk_pyramid_device(None, 1, None, 64, 64, 1, ctypes.byref(p), None, None, None) == -1
    assert L.sbm_lk_stereo_device(None, 1, None, None, 64, 64, None, None, 10, ctypes.byref(p), None, None, None, 1) == -1
    assert L.sbm_lk_stereo(None, None, 64, None, 64, 64, 64, None, 0, ctypes.byref(p), None, None, None) == -1
    assert L.sbm_keypoints3d_lk_device(None, 1, None, None, None, None, 10, None, 0.0, 0.0, None, 1) == -1


def test_level_sizes_of_the_mirror_follow_the_restatement(pkg):
    import lk_stereo_ref as ref
    from lk_cases import PYRAMID_SIZES

    for w, h, last in PYRAMID_SIZES + [(2048, 2048, 5), (2048, 16, 2)]:
        assert pkg.lk_level_sizes(pkg.lk_params(), w, h) == ref.level_sizes(w, h) and len(ref.level_sizes(w, h)) - 1 == last
    assert len(pkg.lk_level_sizes(pkg.lk_params(max_level=50), 2048, 2048)) == 8 == ref.levels(2048, 2048, ref.params(max_level=50)) + 1


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_opencv"])
def test_adaptor_compiles_and_links(tmp_path, pkg, mock):
    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")] if mock else []
    _, r = build_callsite(tmp_path, "lk_callsite_main.cpp", extra, flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr
