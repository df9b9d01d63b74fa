"""The semi-global matcher's C-ABI without a GPU: defaults, parameter validation and its limits, and the C++ adaptor compiling
against the library (plain, and through the cv::InputArray overload against the OpenCV mock)."""
import pathlib
import subprocess

import pytest

from gpu_support import build_callsite

ROOT = pathlib.Path(__file__).resolve().parents[1]
SG, HH, SG3, HH4 = 0, 1, 2, 3


def test_defaults_equal_create(pkg):
    p = pkg.SgbmParams()
    pkg.sgbm_validate(p, 1, 1)   # binds the argument types
    pkg.load_library().sbm_sgbm_params_default(p, 0, 16, 3)
    assert [getattr(p, f) for f, _ in p._fields_] == [0, 16, 3, 0, 0, 0, 0, 0, 0, 0, SG]
    pkg.load_library().sbm_sgbm_params_default(p, -64, 128, 11)
    assert (p.min_disparity, p.num_disparities, p.block_size, p.mode) == (-64, 128, 11, SG)


def test_reference_call_is_valid(pkg):
    p = pkg.sgbm_params(-64, 128, 11, 100, 1000, 32, 0, 15, 1000, 16, HH)
    assert pkg.sgbm_validate(p, 640, 480) == 0


@pytest.mark.parametrize("change,w,h,code", [
    ({}, 0, 10, -2), ({}, 10, -1, -2),
    ({"num_disparities": 0}, 64, 10, -7), ({"num_disparities": 24}, 64, 10, -7), ({"num_disparities": -16}, 64, 10, -7),
    ({"mode": SG3}, 64, 10, -23), ({"mode": HH4}, 64, 10, -23), ({"mode": 7}, 64, 10, -23),
    ({"num_disparities": 512}, 600, 10, 0), ({"num_disparities": 528}, 600, 10, -23),
    ({}, 8192, 10, 0), ({}, 8193, 10, -23), ({}, 64, 65535, 0), ({}, 64, 65536, -23),
    ({"prefilter_cap": 63}, 64, 10, 0), ({"prefilter_cap": 64}, 64, 10, -23), ({"prefilter_cap": -5}, 64, 10, 0),
    ({"uniqueness_ratio": 65535}, 64, 10, 0), ({"uniqueness_ratio": 65536}, 64, 10, -23), ({"uniqueness_ratio": -3}, 64, 10, 0),
    ({"speckle_window_size": 5, "speckle_range": -1}, 64, 10, -23), ({"speckle_range": -1}, 64, 10, 0),
    ({"min_disparity": -2047}, 64, 10, 0), ({"min_disparity": -2048}, 64, 10, -23),
    ({"min_disparity": 2031}, 64, 10, 0), ({"min_disparity": 2032}, 64, 10, -23),
    # the exactness envelope: blockSize_eff^2 * (2 * ftzero + 63) + P2_eff <= 32767
    ({"block_size": 11, "prefilter_cap": 63, "p1": 100, "p2": 9898}, 64, 20, 0),
    ({"block_size": 11, "prefilter_cap": 63, "p1": 100, "p2": 9899}, 64, 20, -23),
    ({"block_size": 17, "p2": 0}, 64, 20, 0),                      # 289 * 93 + 5 = 26 882
    ({"block_size": 18, "p2": 0}, 64, 20, -23),                    # even: a 19 x 19 window, 361 * 93 + 5
    ({"block_size": 19}, 64, 20, -23),
    ({"block_size": 0, "p2": 32767 - 25 * 93}, 64, 20, 0),         # blockSize <= 0 -> 5
    ({"block_size": 0, "p2": 32768 - 25 * 93}, 64, 20, -23),
    ({"p1": 32000, "p2": 0, "block_size": 1}, 64, 20, 0),          # P2_eff = P1 + 1 = 32001; 93 + 32001 = 32094
    ({"p1": 32700, "p2": 0, "block_size": 1}, 64, 20, -23),
])
def test_validate_status_codes(pkg, change, w, h, code):
    p = pkg.sgbm_params()
    for k, v in change.items():
        setattr(p, k, v)
    assert pkg.sgbm_validate(p, w, h) == code


def test_strerror_unchanged_for_sgbm_codes(pkg):
    L = pkg.load_library()
    assert L.sbm_strerror(-23).decode() == "configuration outside this build's limits"
    assert L.sbm_strerror(-7).decode() == "numDisparities must be positive and divisible by 16"


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_opencv"])
def test_sgbm_adaptor_compiles_and_links(tmp_path, pkg, mock):
    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")] if mock else []
    _, r = build_callsite(tmp_path, "sgbm_callsite_main.cpp", extra, flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr
    src = tmp_path / "t.cpp"
    src.write_text(r'''
#include "sbm_stereosgbm.hpp"
int main() {
  sbm_sgbm_params p; sbm_sgbm_params_default(&p, 0, 16, 3);
  if (p.mode != sbm::StereoSGBM::MODE_SGBM || p.block_size != 3) return 1;
  if (sbm_sgbm_params_validate(&p, 640, 480) != SBM_OK) return 2;
  p.mode = sbm::StereoSGBM::MODE_HH4;
  if (sbm_sgbm_params_validate(&p, 640, 480) != SBM_ERR_UNSUPPORTED) return 3;
  return 0;
}
''')
    exe, r = build_callsite(tmp_path, src, exe="t")
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0
