"""The ORB descriptor C-ABI without a GPU: the reference's values as defaults, a status code for every validation failure, and
the C++ adaptor compiling against the library (plain, and with the reference's signature against the OpenCV mock of
tests/cpp/mock_opencv)."""
import ctypes
import math
import pathlib

import numpy as np
import pytest

from gpu_support import build_callsite

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_defaults_are_the_reference_values(pkg):
    L = pkg.load_library()
    p = pkg.OrbParams()
    L.sbm_orb_params_default(p)
    assert (p.edge_threshold, p.angle, p.blur_ksize, p.blur_sigma) == (19, -1.0, 7, 2.0)
    assert pkg.orb_validate(p) == 0


@pytest.mark.parametrize("change,code", [
    ({}, 0), ({"edge_threshold": 18}, 0), ({"edge_threshold": 17}, -23), ({"edge_threshold": 4096}, 0),
    ({"edge_threshold": 4097}, -23), ({"angle": 0.0}, 0), ({"angle": 1e30}, 0), ({"angle": math.inf}, -23),
    ({"angle": math.nan}, -23), ({"blur_ksize": 5}, -23), ({"blur_sigma": 2.0000001}, -23), ({"blur_sigma": 0.0}, -23),
])
def test_validate_status_codes(pkg, change, code):
    p = pkg.orb_params()
    for k, v in change.items():
        setattr(p, k, v)
    assert pkg.orb_validate(p) == code


def test_null_arguments(pkg):
    L = pkg.load_library()
    p = pkg.orb_params()
    pat = np.zeros(1024, np.int32)
    assert L.sbm_orb_params_validate(None) == -1
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)
    assert L.sbm_orb_describe_device(None, 1, a, 64, 64, 4, a, a, pat.ctypes.data, ctypes.byref(p), a, a, a, None, 1) == -1
    assert L.sbm_orb_describe_device(None, 1, a, 64, 64, 4, a, a, None, ctypes.byref(p), a, a, a, None, 1) == -1
    cnt = ctypes.c_int()
    assert L.sbm_orb_describe(None, a, 64, 64, 64, a, 1, pat.ctypes.data, ctypes.byref(p), a, ctypes.byref(cnt), a) == -1
    gp = pkg.gftt_select_params()
    assert L.sbm_orb_features_device(None, 1, a, 64, 64, ctypes.byref(gp), pat.ctypes.data, ctypes.byref(p), a, a, a, a, a, None,
                                     1) == -1


def test_the_profile_names_are_documented():
    h = (ROOT / "include" / "sbm.h").read_text()
    for k in ("orb_blur", "orb_desc", "orb_total"):
        assert f'"{k}"' in h
    assert "bit 128" in h


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_opencv"])
def test_cpp_adaptor_compiles(tmp_path, mock):
    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")] if mock else []
    _, r = build_callsite(tmp_path, "orb_callsite_main.cpp", extra, flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr[-3000:]
