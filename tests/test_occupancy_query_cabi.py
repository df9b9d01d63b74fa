"""The occupancy map's query C-ABI without a GPU: declarations against exports, the structure layout against the mirror,
castRay's defaults, a status code for every validation failure, null arguments, the constants against the transcription, the
C++ adaptor compiling against the library, and what include/sbm.h must say. The argument checks that need a map are in
tests/test_gpu_occupancy_query.py."""
import ctypes
import math
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_query_cases as qc  # noqa: E402
from gpu_support import build_callsite  # noqa: E402

CALLS = ("sbm_occ_query_params_default", "sbm_occ_query_params_validate", "sbm_occ_search_device", "sbm_occ_search",
         "sbm_occ_cast_rays_device", "sbm_occ_cast_rays", "sbm_occ_cast_view_device")


def test_declarations_against_exports(pkg):
    text = (ROOT / "include" / "sbm.h").read_text()
    declared = set(re.findall(r"^(?:int|void) (sbm_occ_\w+)\(", text, re.M))
    assert set(CALLS) <= declared
    r = subprocess.run(["nm", "-D", "--defined-only", str(pkg.library_path())], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in r.stdout.splitlines() if " T " in line}
    assert declared == {s for s in exported if s.startswith("sbm_occ_")}
    L = pkg.load_library()
    for name in CALLS:
        assert getattr(L, name).argtypes is not None, name


def test_struct_layout_defaults_and_constants(pkg):
    p = pkg.OccQueryParams()
    assert pkg.occ_query_validate(pkg.occ_query_params()) == 0
    pkg.load_library().sbm_occ_query_params_default(p)
    assert (p.max_range, p.occupancy_thres_log, p.ignore_unknown) == (-1.0, 0.0, 0)
    assert bytes(p) == bytes(pkg.occ_query_params())
    assert ctypes.sizeof(p) == 16
    assert (pkg.OccQueryParams.max_range.offset, pkg.OccQueryParams.occupancy_thres_log.offset,
            pkg.OccQueryParams.ignore_unknown.offset) == (0, 8, 12)
    assert (pkg.OCC_CELL_OUT, pkg.OCC_CELL_UNKNOWN, pkg.OCC_CELL_FREE, pkg.OCC_CELL_OCCUPIED) == \
        (qc.CELL_OUT, qc.CELL_UNKNOWN, qc.CELL_FREE, qc.CELL_OCCUPIED) == (-1, 0, 1, 2)
    assert (pkg.OCC_RAY_NONE, pkg.OCC_RAY_HIT, pkg.OCC_RAY_RANGE, pkg.OCC_RAY_UNKNOWN, pkg.OCC_RAY_BOUNDS) == \
        (qc.RAY_NONE, qc.RAY_HIT, qc.RAY_RANGE, qc.RAY_UNKNOWN, qc.RAY_BOUNDS)
    text = (ROOT / "include" / "sbm.h").read_text()
    for name, value in (("SBM_OCC_CELL_OUT", -1), ("SBM_OCC_CELL_UNKNOWN", 0), ("SBM_OCC_CELL_FREE", 1), ("SBM_OCC_CELL_OCCUPIED", 2),
                        ("SBM_OCC_RAY_NONE", qc.RAY_NONE), ("SBM_OCC_RAY_HIT", qc.RAY_HIT), ("SBM_OCC_RAY_RANGE", qc.RAY_RANGE),
                        ("SBM_OCC_RAY_UNKNOWN", qc.RAY_UNKNOWN), ("SBM_OCC_RAY_BOUNDS", qc.RAY_BOUNDS)):
        assert f"{name} = {value}" in text, name
    assert float(pkg.occ_ray_logodds()[4]) == p.occupancy_thres_log      # the default threshold is that of the default probabilities


@pytest.mark.parametrize("change,code", [
    ({}, 0), ({"max_range": 0.0}, 0), ({"max_range": -math.inf}, 0), ({"max_range": math.inf}, 0), ({"max_range": 1e-300}, 0),
    ({"occupancy_thres_log": math.inf}, 0), ({"occupancy_thres_log": -3.5}, 0), ({"ignore_unknown": 1}, 0), ({"ignore_unknown": -7}, 0),
    ({"max_range": math.nan}, -2), ({"occupancy_thres_log": math.nan}, -2),
])
def test_validate_status_codes(pkg, change, code):
    p = pkg.occ_query_params()
    for k, v in change.items():
        setattr(p, k, v)
    assert pkg.occ_query_validate(p) == code


def test_null_arguments(pkg):
    L = pkg.load_library()
    q = pkg.occ_query_params()
    m = pkg.StereoModel()
    a = np.zeros(12, np.float32)
    s = np.zeros(4, np.int32)
    assert L.sbm_occ_query_params_validate(None) == -1
    L.sbm_occ_query_params_default(None)   # tolerated
    assert L.sbm_occ_search_device(None, 1, a.ctypes.data, 0.0, s.ctypes.data, None, 1) == -1
    assert L.sbm_occ_search(None, 1, a.ctypes.data, 0.0, s.ctypes.data, None) == -1
    assert L.sbm_occ_search(None, 0, None, 0.0, None, None) == -1
    assert L.sbm_occ_cast_rays_device(None, 1, a.ctypes.data, 1, a.ctypes.data, ctypes.byref(q), s.ctypes.data, None, 1) == -1
    assert L.sbm_occ_cast_rays(None, 1, a.ctypes.data, 0, a.ctypes.data, ctypes.byref(q), s.ctypes.data, None) == -1
    assert L.sbm_occ_cast_view_device(None, 4, 4, 1, ctypes.byref(m), a.ctypes.data, ctypes.byref(q), s.ctypes.data, None, 1) == -1


def test_cpp_adaptor_compiles(tmp_path, pkg):
    _, r = build_callsite(tmp_path, "occupancy_query_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr


def test_header_states_the_readings():
    text = (ROOT / "include" / "sbm.h").read_text()
    for phrase in ('"occ_search"', '"occ_cast"', "occupancy map: queries", "DOUBLE", "BEFORE the advance", "isNodeOccupied",
                   "reads as UNKNOWN", "EXACTLY", "shared_origin"):
        assert phrase in text, phrase
    free_space = text[text.index("occupancy map: ray-cast free space"):text.index("occupancy map: queries")]
    line = next(ln for ln in free_space.splitlines() if "Not provided" in ln)
    assert "castRay" not in line and "insertPointCloudRays" in line
