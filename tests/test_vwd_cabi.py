"""The visual-word dictionary C-ABI without a GPU: structure layout against the mirror, the reference's constants as defaults, one
status code per validation failure, null arguments, limitKeypoints against the multimap transcription, the C++ adaptor compiling
against the library (plain, and with the reference's types against the OpenCV mock), and what include/sbm.h must say."""
import ctypes
import math
import pathlib

import numpy as np
import pytest

import vwd_cases as vc
from gpu_support import build_callsite

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_struct_layout_and_defaults(pkg):
    p = pkg.VwdParams()
    assert pkg.vwd_validate(pkg.vwd_params()) == 0   # binds the argument types
    pkg.load_library().sbm_vwd_params_default(p)
    assert (p.metric, p.nndr, p.slices) == (pkg.VWD_L1, np.float32(0.8), 0)
    assert bytes(p) == bytes(pkg.vwd_params())
    assert ctypes.sizeof(p) == 12
    assert (pkg.VwdParams.metric.offset, pkg.VwdParams.nndr.offset, pkg.VwdParams.slices.offset) == (0, 4, 8)
    assert (pkg.VWD_L1, pkg.VWD_L2, pkg.VWD_NONE, pkg.ERR_VWD_FULL) == (vc.L1, vc.L2, vc.NONE, -26)
    assert b"visual-word dictionary full" in pkg.load_library().sbm_strerror(-26)


@pytest.mark.parametrize("change,code", [
    ({}, 0), ({"metric": 1}, 0), ({"nndr": 1.0}, 0), ({"nndr": 1e-6}, 0), ({"slices": 1}, 0), ({"slices": 65535}, 0),
    ({"nndr": math.nan}, -23), ({"nndr": 0.0}, -23), ({"nndr": -0.8}, -23), ({"nndr": 1.0000001}, -23), ({"nndr": math.inf}, -23),
    ({"metric": 2}, -23), ({"metric": -1}, -23), ({"slices": -1}, -23), ({"slices": 65536}, -23),
])
def test_validate_status_codes(pkg, change, code):
    p = pkg.vwd_params()
    for k, v in change.items():
        setattr(p, k, v)
    assert pkg.vwd_validate(p) == code


def test_null_arguments(pkg):
    L = pkg.load_library()
    p = pkg.vwd_params()
    out = ctypes.c_void_p()
    n = ctypes.c_size_t()
    v = ctypes.c_uint64()
    k = ctypes.c_int()
    f = ctypes.c_float()
    ids = np.zeros(4, np.int32)
    rows = np.zeros((4, 32), np.uint8)
    assert L.sbm_vwd_params_validate(None) == -1
    L.sbm_vwd_params_default(None)   # tolerated
    L.sbm_vwd_destroy(None)          # tolerated
    assert L.sbm_vwd_create(None, 64, ctypes.byref(p), ctypes.byref(out)) == -1
    assert L.sbm_vwd_reset(None) == -1
    assert L.sbm_vwd_size(None, ctypes.byref(n)) == -1 and L.sbm_vwd_overflow(None, ctypes.byref(v)) == -1
    assert L.sbm_vwd_add_words_device(None, rows.ctypes.data, 4, 1, 4, ids.ctypes.data) == -1
    assert L.sbm_vwd_add_words(None, rows.ctypes.data, 32, 4, 1, 4, ids.ctypes.data) == -1
    assert L.sbm_vwd_search_device(None, rows.ctypes.data, 4, rows.ctypes.data, 1) == -1
    assert L.sbm_vwd_fetch_words(None, 0, 1, rows.ctypes.data) == -1
    assert L.sbm_vwd_references(None, 0, ids.ctypes.data, ids.ctypes.data, 4, ctypes.byref(k)) == -1
    assert L.sbm_vwd_likelihood(None, 1, ids.ctypes.data, 4, 4, rows.ctypes.data, ctypes.byref(k), ctypes.byref(f)) == -1
    r = np.ones(3, np.float32)
    keep = np.zeros(3, np.uint8)
    assert L.sbm_vwd_limit_keypoints(None, 3, 2, keep.ctypes.data) == -1
    assert L.sbm_vwd_limit_keypoints(r.ctypes.data, 3, 2, None) == -1
    assert L.sbm_vwd_limit_keypoints(None, 0, 2, None) == 0
    assert L.sbm_vwd_limit_keypoints(r.ctypes.data, -1, 2, keep.ctypes.data) == -2
    r[1] = np.nan
    assert L.sbm_vwd_limit_keypoints(r.ctypes.data, 3, 2, keep.ctypes.data) == -23


def limit_cases():
    rng = np.random.default_rng(17)
    yield "distinct", rng.normal(size=40).astype(np.float32), 12
    yield "ties", rng.integers(0, 4, 60).astype(np.float32), 25          # every cut falls inside a run of equal responses
    yield "all_equal", np.full(9, 2.5, np.float32), 4
    yield "negative", np.array([-3, 3, -1, 1, -3, 2, -2, 3, 0, -0.0], np.float32), 5   # |r| ties across signs
    yield "n_below_max", rng.normal(size=7).astype(np.float32), 8
    yield "n_equals_max", rng.normal(size=8).astype(np.float32), 8
    yield "max_zero", rng.normal(size=8).astype(np.float32), 0
    yield "max_negative", rng.normal(size=8).astype(np.float32), -3
    yield "max_one", np.array([1, 5, 5, 2], np.float32), 1
    yield "empty", np.zeros(0, np.float32), 3
    yield "reference_750", rng.integers(0, 300, 1000).astype(np.float32), 750


@pytest.mark.parametrize("name,resp,mx", list(limit_cases()), ids=[c[0] for c in limit_cases()])
def test_limit_keypoints_equals_the_multimap_transcription(pkg, name, resp, mx):
    want = vc.limit_keypoints(resp, mx)
    got = pkg.limit_keypoints(resp, mx)
    assert got.dtype == bool and np.array_equal(got, want)
    if mx > 0 and len(resp) > mx:
        assert got.sum() == mx
    else:
        assert got.all()
    if name == "max_one":
        assert list(got) == [False, False, True, False]   # of two equal responses the higher index wins


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_opencv"])
def test_cpp_adaptor_compiles(tmp_path, mock):
    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")] if mock else []
    _, r = build_callsite(tmp_path, "vwd_callsite_main.cpp", extra, flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr


def test_header_states_the_readings():
    text = (ROOT / "include" / "sbm.h").read_text()
    for phrase in ('"vwd_search"', '"vwd_append"', '"vwd_total"', "exhaustive", "L1", "node 0"):
        assert phrase in text, phrase
