"""The keypoint-matching C-ABI without a GPU: the reference's values as defaults, a status code for every validation failure, and
the C++ adaptor compiling against the library (plain, and with the reference's types against the OpenCV mock of
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
    p = pkg.MatchParams()
    L.sbm_match_params_default(p)
    assert (p.nndr, p.radius) == (np.float32(0.8), 40.0)
    assert pkg.match_validate(p) == 0


@pytest.mark.parametrize("change,code", [
    ({}, 0), ({"nndr": 1.0}, 0), ({"nndr": 1.0000001}, -23), ({"nndr": 1e-30}, 0), ({"nndr": 0.0}, -23), ({"nndr": -0.5}, -23),
    ({"nndr": math.nan}, -23), ({"nndr": math.inf}, -23), ({"radius": 1e-30}, 0), ({"radius": 0.0}, -23), ({"radius": -1.0}, -23),
    ({"radius": 3e38}, 0), ({"radius": math.inf}, -23), ({"radius": math.nan}, -23),
])
def test_validate_status_codes(pkg, change, code):
    p = pkg.match_params()
    for k, v in change.items():
        setattr(p, k, v)
    assert pkg.match_validate(p) == code


def test_null_arguments(pkg):
    L = pkg.load_library()
    p = pkg.match_params()
    assert L.sbm_match_params_validate(None) == -1
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)
    jobs = np.zeros(2, np.int32)
    j = jobs.ctypes.data
    assert L.sbm_match_device(None, 1, 1, j, a, a, 4, ctypes.byref(p), a, a, None, 1) == -1
    assert L.sbm_match_device(None, 1, 1, None, a, a, 4, ctypes.byref(p), a, a, None, 1) == -1
    assert L.sbm_match_guess_device(None, 1, 1, j, a, a, 4, a, a, ctypes.byref(p), a, a, None, 1) == -1
    T = np.zeros(12, np.float32)
    K = np.zeros(4)
    assert L.sbm_project_points_device(None, 1, 1, j, a, a, 4, T.ctypes.data, K.ctypes.data, 8, 8, a, 1) == -1
    k = ctypes.c_int()
    assert L.sbm_match(None, a, 32, 1, a, 32, 1, ctypes.byref(p), a, ctypes.byref(k)) == -1
    assert L.sbm_match_guess(None, a, a, a, 32, 1, a, 32, 1, T.ctypes.data, K.ctypes.data, 8, 8, ctypes.byref(p), a,
                             ctypes.byref(k)) == -1


def test_plan_null_and_size_checks(pkg):
    L = pkg.load_library()
    pl = pkg.MatchPlanInfo()
    size = ctypes.sizeof(pl)
    assert size == 40
    assert L.sbm_match_plan(300, 1, None, size) == -1
    assert L.sbm_match_plan(0, 0, None, 0) == -1                      # the null check comes first
    for wrong in (0, size - 8, size - 1, size + 1, 2 * size):
        pl.nslice = 77
        assert L.sbm_match_plan(300, 1, ctypes.byref(pl), wrong) == -2
        assert pl.nslice == 77                                        # a mirror of another size is not written to
    assert L.sbm_match_plan(300, 1, ctypes.byref(pl), size) == 0
    assert (pl.qtiles, pl.nslice, pl.slice_rows, pl.jobs_per_launch, pl.launches) == (5, 5, 64, 1, 1)
    assert (pl.proj_jobs_per_launch, pl.proj_launches, pl.pad, pl.scratch_bytes) == (1, 1, 0, 300 * 88)
    assert L.sbm_match_plan(65536, 1, ctypes.byref(pl), size) == -2   # a refused shape leaves a zeroed plan
    assert (pl.nslice, pl.slice_rows, pl.scratch_bytes) == (0, 0, 0)
    got = pkg.match_plan(300, 65)
    assert (got.jobs_per_launch, got.launches, got.proj_launches) == (64, 2, 3)


def test_the_contract_is_documented():
    h = (ROOT / "include" / "sbm.h").read_text()
    assert "sbm_match_plan_info" in h and "int sbm_match_plan(int cap, int m" in h
    for k in ("match_knn", "match_unique", "match_total", "match_project"):
        assert f'"{k}"' in h
    assert "bit 256" in h and "nt == 1" in h and "NOT reproduced" in h


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_opencv"])
def test_cpp_adaptor_compiles(tmp_path, mock):
    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")] if mock else []
    _, r = build_callsite(tmp_path, "match_callsite_main.cpp", extra, flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr[-3000:]
