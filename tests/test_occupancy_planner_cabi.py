"""The C-ABI of the occupancy map's read side for planners without a GPU: declarations against exports and bindings, every argument
check that comes before a device is touched in its documented order, the C++ adaptor compiling against the library, and what
include/sbm.h must say. The checks that need a tree are in tests/test_gpu_occupancy_planner.py."""
import ctypes
import pathlib
import re
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
from gpu_support import build_callsite  # noqa: E402

CALLS = ("sbm_occ_bbx_leaves_device", "sbm_occ_bbx_leaves", "sbm_occ_bbx_leaves_points_device", "sbm_occ_bbx_leaves_points",
         "sbm_occ_unknown_device", "sbm_occ_unknown", "sbm_occ_metric", "sbm_occ_ray_intersections_device", "sbm_occ_ray_intersections")
NULL, SIZE = -1, -2


def test_declarations_against_exports_and_bindings(pkg):
    text = (ROOT / "include" / "sbm.h").read_text()
    declared = set(re.findall(r"^(?:int|void) (sbm_occ_\w+)\(", text, re.M))
    r = subprocess.run(["nm", "-D", "--defined-only", str(pkg.library_path())], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in r.stdout.splitlines() if " T " in line}
    assert set(CALLS) <= exported and {e for e in exported if e.startswith("sbm_occ_")} == declared
    assert not any(re.match(r"sbm_occ_(ot|tree)_", c) for c in CALLS)        # those prefixes are closed sets of their sections
    L = pkg.load_library()
    for name in CALLS:
        assert getattr(L, name).argtypes is not None, name
    flat = " ".join(text.split())
    order = {"sbm_occ_bbx_leaves_device": "sbm_occ_tree* tree, const uint16_t min_key[3], const uint16_t max_key[3], int max_depth, void* d_keys, "
                                          "void* d_depth, void* d_value, size_t cap, size_t* count",
             "sbm_occ_bbx_leaves_points": "sbm_occ_tree* tree, const float min[3], const float max[3], int max_depth, uint64_t* keys",
             "sbm_occ_unknown_device": "sbm_occ_tree* tree, const float pmin[3], const float pmax[3], int depth, void* d_xyz, size_t cap, size_t* count",
             "sbm_occ_metric": "sbm_occ_tree* tree, double min[3], double max[3]",
             "sbm_occ_ray_intersections_device": "sbm_occ_map* map, size_t n, const void* origins, int shared_origin, const void* d_dirs, "
                                                 "const void* d_centres, double delta, void* d_xyz, void* d_found, int sync"}
    for name, args in order.items():
        assert f"{name}({args}" in flat, name


def test_argument_checks_before_any_device_in_their_documented_order(pkg):
    """A null tree or map is looked at first, so nothing here reaches a device."""
    L = pkg.load_library()
    k = np.zeros(3, np.uint16)
    p = np.zeros(3, np.float32)
    keys, depth, xyz = np.zeros(4, np.uint64), np.zeros(4, np.int32), np.zeros(12, np.float32)
    m = np.zeros(6, np.float64)
    n = ctypes.c_size_t(7)
    K, P = k.ctypes.data, p.ctypes.data
    for call, lo in ((L.sbm_occ_bbx_leaves_device, K), (L.sbm_occ_bbx_leaves, K), (L.sbm_occ_bbx_leaves_points_device, P), (L.sbm_occ_bbx_leaves_points, P)):
        assert call(None, lo, lo, 0, keys.ctypes.data, depth.ctypes.data, None, 4, ctypes.byref(n)) == NULL
        assert call(None, lo, lo, 17, None, None, None, 0, ctypes.byref(n)) == NULL           # before the depth is looked at
        assert call(None, None, None, 0, None, None, None, 0, None) == NULL
    for call in (L.sbm_occ_unknown_device, L.sbm_occ_unknown):
        assert call(None, P, P, 0, xyz.ctypes.data, 4, ctypes.byref(n)) == NULL
        assert call(None, P, P, 17, None, 0, ctypes.byref(n)) == NULL
    assert L.sbm_occ_metric(None, m.ctypes.data, m.ctypes.data + 24) == NULL
    X = xyz.ctypes.data
    assert L.sbm_occ_ray_intersections_device(None, 1, X, 0, X, X, 0.0, X, None, 1) == NULL
    assert L.sbm_occ_ray_intersections_device(None, 0, None, 0, None, None, float("nan"), None, None, 1) == NULL     # n == 0 needs a map too
    assert L.sbm_occ_ray_intersections(None, 1, X, 1, X, X, 0.0, X, None) == NULL
    assert L.sbm_occ_ray_intersections(None, 0, None, 1, None, None, float("nan"), None, None) == NULL
    assert n.value == 7 and not keys.any() and not depth.any() and not xyz.any() and not m.any()      # no refused call wrote through a pointer


def test_cpp_adaptor_compiles(tmp_path, pkg):
    _, r = build_callsite(tmp_path, "occupancy_planner_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr


def test_header_states_the_contract():
    text = (ROOT / "include" / "sbm.h").read_text()
    part = text[text.index("occupancy map: the read side for planners"):text.index("visual-word dictionary: addNewWords")]
    for phrase in ("begin_leafs_bbx", "getUnknownLeafCenters", "getMetricMin", "getMetricMax", "getRayIntersection", "SNAPSHOT",
                   "min <= c + off && max >= c - off", "LOOSE BY ONE KEY", "The root itself is never tested",
                   "A node's own test implies its ancestors' tests", "visits the root once", "incremented BEFORE the query",
                   "x outermost and z innermost", "refused with SBM_ERR_SIZE", "more than 2^30 cells", "An empty tree answers six zeros",
                   "no float atomics", "cached in the tree until the next build", "float(resolution / 2.0)", "NOT normalised",
                   "0x7FC00000", "getNormals is NOT provided", '"occ_tree_query"', '"occ_cast"', "Checked in this order"):
        assert phrase in part, phrase
    tree = text[text.index("occupancy map: the octree above the voxels"):text.index("occupancy map: load a .bt stream")]
    assert "the read side for planners" in tree and "bounding-box iterators" not in tree      # the "Not here" sentence is up to date
    design = (ROOT / "DESIGN.md").read_text()
    assert "bounding-box iterators are not provided" not in design and "bounding-box iterators are not provided" not in design.replace("\n", " ")
