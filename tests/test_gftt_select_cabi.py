"""The keypoint selection's C-ABI without a GPU: the reference's constants as defaults, a status code for every validation
failure, and the C++ adaptor compiling against the library (plain, and with the reference's signature against the OpenCV mock)."""
import math
import pathlib
import subprocess

import pytest

from gpu_support import build_callsite

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_defaults_are_the_reference_constants(pkg):
    p = pkg.GfttSelectParams()
    pkg.gftt_select_validate(p, 3, 3)   # binds the argument types
    pkg.load_library().sbm_gftt_select_params_default(p)
    assert (p.max_features, p.quality_level, p.min_distance, p.block_size) == (1500, 0.01, 7.0, 3)
    assert pkg.gftt_select_validate(p, 640, 480) == 0


@pytest.mark.parametrize("change,w,h,code", [
    ({}, 3, 3, 0), ({}, 2, 3, -2), ({}, 3, 2, -2), ({}, 0, 10, -2), ({}, 10, -1, -2),
    ({}, 2048, 2048, 0), ({}, 2049, 10, -23), ({}, 10, 2049, -23),
    ({"quality_level": 0.0}, 64, 10, 0), ({"quality_level": 1e300}, 64, 10, 0), ({"quality_level": -1e-9}, 64, 10, -23),
    ({"quality_level": math.inf}, 64, 10, -23), ({"quality_level": math.nan}, 64, 10, -23),
    ({"min_distance": 0.0}, 64, 10, 0), ({"min_distance": 255.0}, 64, 10, 0), ({"min_distance": 255.0001}, 64, 10, -23),
    ({"min_distance": -0.5}, 64, 10, -23), ({"min_distance": math.inf}, 64, 10, -23), ({"min_distance": math.nan}, 64, 10, -23),
    ({"max_features": -5}, 64, 10, 0), ({"max_features": 0}, 64, 10, 0), ({"block_size": 0}, 64, 10, 0),
])
def test_validate_status_codes(pkg, change, w, h, code):
    p = pkg.gftt_select_params()
    for k, v in change.items():
        setattr(p, k, v)
    assert pkg.gftt_select_validate(p, w, h) == code


def test_null_params(pkg):
    L = pkg.load_library()
    pkg.gftt_select_validate(pkg.gftt_select_params(), 3, 3)
    assert L.sbm_gftt_select_params_validate(None, 64, 64) == -1


def test_capacity(pkg):
    assert pkg.gftt_select_capacity(pkg.gftt_select_params(), 640, 480) == 1500
    assert pkg.gftt_select_capacity(pkg.gftt_select_params(max_features=0), 640, 480) == 638 * 478
    assert pkg.gftt_select_capacity(pkg.gftt_select_params(max_features=-1), 3, 3) == 1


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_opencv"])
def test_gftt_adaptor_compiles_and_links(tmp_path, pkg, mock):
    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")] if mock else []
    _, r = build_callsite(tmp_path, "gftt_callsite_main.cpp", extra, flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr
    src = tmp_path / "t.cpp"
    src.write_text(r'''
#include "sbm_gftt.hpp"
int main() {
  sbm_gftt_select_params p; sbm_gftt_select_params_default(&p);
  if (p.max_features != 1500 || p.min_distance != 7.0 || p.block_size != 3) return 1;
  p.min_distance = 256;
  if (sbm_gftt_select_params_validate(&p, 640, 480) != SBM_ERR_UNSUPPORTED) return 2;
  return 0;
}
''')
    exe, r = build_callsite(tmp_path, src, exe="t")
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0
