"""The occupancy-map C-ABI without a GPU: structure layout against the mirror and the restatement, the reference's constants
as defaults, a status code for every validation failure, null arguments, the host writer of the .bt stream against the bytes
the reference's octomap wrote and against the restatement's writer, and the C++ adaptor compiling against the library."""
import ctypes
import math
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_ref as occ  # noqa: E402
from gpu_support import build_callsite  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "occupancy_octomap.npz"


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def test_struct_layout_and_defaults(pkg):
    p = pkg.OccParams()
    assert pkg.occ_validate(pkg.occ_params()) == 0   # binds the argument types
    pkg.load_library().sbm_occ_params_default(p)
    assert (p.resolution, p.range_max, p.tree_depth) == (0.1, 5.0, 16)
    assert bytes(p) == bytes(pkg.occ_params()) == bytes(occ.params())
    assert ctypes.sizeof(p) == 16 == ctypes.sizeof(occ.Params)
    assert [(f[0], f[1]) for f in pkg.OccParams._fields_] == [(f[0], f[1]) for f in occ.Params._fields_]
    assert (pkg.OccParams.resolution.offset, pkg.OccParams.range_max.offset, pkg.OccParams.tree_depth.offset) == (0, 8, 12)
    assert ctypes.sizeof(pkg.StereoModel) == ctypes.sizeof(occ.StereoModel) == 128
    assert [f[0] for f in pkg.StereoModel._fields_] == [f[0] for f in occ.StereoModel._fields_]
    assert pkg.ERR_OCC_FULL == -25
    assert b"occupancy map full" in pkg.load_library().sbm_strerror(-25)


@pytest.mark.parametrize("change,code", [
    ({}, 0), ({"resolution": 0.05}, 0), ({"resolution": 1e-300}, 0), ({"resolution": 0.0}, -2), ({"resolution": -0.1}, -2),
    ({"resolution": math.inf}, -2), ({"resolution": math.nan}, -2), ({"resolution": 5e-324}, -2),
    ({"range_max": 0.0}, 0), ({"range_max": math.inf}, 0), ({"range_max": -1.0}, -2), ({"range_max": math.nan}, -2),
    ({"tree_depth": 15}, -23), ({"tree_depth": 17}, -23), ({"tree_depth": 0}, -23),
])
def test_validate_status_codes(pkg, change, code):
    p = pkg.occ_params()
    for k, v in change.items():
        setattr(p, k, v)
    assert pkg.occ_validate(p) == code


def test_null_arguments(pkg, tmp_path):
    L = pkg.load_library()
    p = pkg.occ_params()
    m = pkg.StereoModel()
    out = ctypes.c_void_p()
    n = ctypes.c_size_t()
    v = ctypes.c_uint64()
    assert L.sbm_occ_params_validate(None) == -1
    L.sbm_occ_params_default(None)   # tolerated
    L.sbm_occ_destroy(None)          # tolerated
    assert L.sbm_occ_create(None, ctypes.byref(p), 64, ctypes.byref(out)) == -1
    assert L.sbm_occ_reset(None) == -1
    assert L.sbm_occ_insert_device(None, 1, None, 4, 4, 1, ctypes.byref(m), None, 1) == -1
    assert L.sbm_occ_insert(None, 1, None, 4, 4, 1, ctypes.byref(m), None) == -1
    assert L.sbm_occ_size(None, ctypes.byref(n)) == -1 and L.sbm_occ_overflow(None, ctypes.byref(v)) == -1
    assert L.sbm_occ_fetch_device(None, None, None, 0, ctypes.byref(n)) == -1
    assert L.sbm_occ_fetch(None, None, None, 0, ctypes.byref(n)) == -1
    k = np.zeros(1, np.uint64)
    assert L.sbm_occ_write_binary(k.ctypes.data, 1, 0.1, None) == -1
    assert L.sbm_occ_write_binary(None, 1, 0.1, str(tmp_path / "x.bt").encode()) == -1
    assert L.sbm_occ_write_binary(k.ctypes.data, 1, 0.0, str(tmp_path / "x.bt").encode()) == -2
    k[0] = 1 << 48
    assert L.sbm_occ_write_binary(k.ctypes.data, 1, 0.1, str(tmp_path / "x.bt").encode()) == -2
    k[0] = 5
    assert L.sbm_occ_write_binary(k.ctypes.data, 1, 0.1, str(tmp_path / "no" / "such" / "x.bt").encode()) == -23


def fixture_keys(fx, bit):
    take = (fx["norm"] <= 25.0) & (fx["ok"] == 1) & ((fx["group"] >> bit) & 1 == 1)
    return np.unique(occ.pack(fx["keys"][take]))


@pytest.mark.parametrize("name,bit", [("all", 0), ("blocks", 1), ("empty", 2)])
def test_write_binary_equals_octomap_and_the_restatement(pkg, fx, tmp_path, name, bit):
    keys = fixture_keys(fx, bit)
    assert (len(keys) == 0) == (name == "empty")
    path = tmp_path / f"{name}.bt"
    pkg.occ_write_binary(keys, path, float(fx["resolution"]))
    data = path.read_bytes()
    assert data == fx[f"bt_{name}"].tobytes()
    assert data == occ.write_binary(keys, float(fx["resolution"]))[0]
    # any order, duplicates allowed
    rng = np.random.default_rng(9)
    pkg.occ_write_binary(rng.permutation(np.concatenate([keys, keys[:7]])), path, float(fx["resolution"]))
    assert path.read_bytes() == data


def test_write_binary_on_shapes_the_fixture_lacks(pkg, tmp_path):
    """Deeper collapses, the key range's corners and another resolution, against the restatement's pointer octree."""
    rng = np.random.default_rng(21)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    cases = {
        "cube8": occ.pack(g + [4096, 8, 65528]),                                   # collapses three levels
        "cube8_minus": occ.pack(np.delete(g, 77, axis=0) + [4096, 8, 65528]),
        "corners": occ.pack([[0, 0, 0], [65535, 65535, 65535], [0, 65535, 0], [32767, 32768, 32767]]),
        "one": occ.pack([[32768, 32768, 32768]]),
        "random": occ.pack(rng.integers(32000, 33500, (5000, 3))),
        "slab": occ.pack(np.stack(np.meshgrid(np.arange(30), np.arange(30), np.arange(3), indexing="ij"), -1).reshape(-1, 3) + 32761),
    }
    for name, keys in cases.items():
        for res in (0.1, 0.05, 2.5):
            path = tmp_path / f"{name}.bt"
            pkg.occ_write_binary(keys, path, res)
            want, nodes, leafs = occ.write_binary(keys, res)
            assert path.read_bytes() == want, (name, res)
    assert occ.write_binary(cases["cube8"])[2] == 1 and occ.write_binary(cases["cube8_minus"])[2] == 7 + 7 + 7


def test_adaptor_compiles_and_links(tmp_path, pkg):
    _, r = build_callsite(tmp_path, "occupancy_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr
