"""The occupancy tree's C-ABI without a GPU: declarations against exports, the structure layout against the mirror, the constants
against the transcription, whatever the entry points check before they touch a device (null arguments, n == 0 among them), the
C++ adaptor compiling against the library, and what include/sbm.h must say. The checks that need a tree are in
tests/test_gpu_occupancy_tree.py."""
import ctypes
import pathlib
import re
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_tree_cases as tc  # noqa: E402
from gpu_support import build_callsite  # noqa: E402

CALLS = ("sbm_occ_tree_create", "sbm_occ_tree_destroy", "sbm_occ_tree_build", "sbm_occ_tree_info", "sbm_occ_tree_search_device",
         "sbm_occ_tree_search", "sbm_occ_tree_leaves_device", "sbm_occ_tree_leaves", "sbm_occ_tree_binary_device",
         "sbm_occ_tree_write_binary")
NULL = -1


def test_declarations_against_exports(pkg):
    text = (ROOT / "include" / "sbm.h").read_text()
    declared = set(re.findall(r"^(?:int|void) (sbm_occ_tree_\w+)\(", text, re.M))
    assert declared == set(CALLS)
    r = subprocess.run(["nm", "-D", "--defined-only", str(pkg.library_path())], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in r.stdout.splitlines() if " T " in line}
    assert declared == {s for s in exported if s.startswith("sbm_occ_tree_")}
    L = pkg.load_library()
    for name in CALLS:
        assert getattr(L, name).argtypes is not None, name
    # the argument order of the header is the one the mirror calls with
    order = {"sbm_occ_tree_build": "tree, int reading, const sbm_occ_ray_params* params, int sync",
             "sbm_occ_tree_search_device": "tree, size_t n, const void* d_xyz, int depth, float occupancy_thres_log, void* d_state",
             "sbm_occ_tree_leaves_device": "tree, int max_depth, void* d_keys, void* d_depth, void* d_value, size_t cap, size_t* count",
             "sbm_occ_tree_binary_device": "tree, void* d_bytes, size_t cap, size_t* nbytes"}
    flat = " ".join(text.split())
    for name, args in order.items():
        assert f"{name}(sbm_occ_tree* {args}" in flat, name


def test_struct_layout_and_constants(pkg):
    c = pkg.OccTreeCounts
    assert ctypes.sizeof(c) == 3 * 8 + 2 * 17 * 8 + 2 * 3 * 2 + 4 == 312
    assert (c.voxels.offset, c.nodes.offset, c.leaves.offset, c.nodes_at.offset, c.leaves_at.offset, c.key_min.offset, c.key_max.offset) == \
        (0, 8, 16, 24, 160, 296, 302)
    assert (pkg.OCC_TREE_LOGODDS, pkg.OCC_TREE_MAXLIKELIHOOD) == (tc.LOGODDS, tc.MAXLIKELIHOOD) == (0, 1)
    text = (ROOT / "include" / "sbm.h").read_text()
    assert "SBM_OCC_TREE_LOGODDS = 0, SBM_OCC_TREE_MAXLIKELIHOOD = 1" in text
    for field in ("uint64_t voxels;", "uint64_t nodes, leaves;", "uint64_t nodes_at[17];", "uint64_t leaves_at[17];", "uint16_t key_min[3];",
                  "uint16_t key_max[3];"):
        assert field in text, field
    assert (tc.CELL_OUT, tc.CELL_UNKNOWN, tc.CELL_FREE, tc.CELL_OCCUPIED) == \
        (pkg.OCC_CELL_OUT, pkg.OCC_CELL_UNKNOWN, pkg.OCC_CELL_FREE, pkg.OCC_CELL_OCCUPIED)


def test_null_arguments_come_first_also_for_n_zero(pkg):
    L = pkg.load_library()
    rp = pkg.occ_ray_params()
    a = np.zeros(12, np.float32)
    s = np.zeros(4, np.int32)
    k = np.zeros(4, np.uint64)
    n = ctypes.c_size_t(7)
    out = ctypes.c_void_p(1)
    info = pkg.OccTreeCounts()
    assert L.sbm_occ_tree_create(None, ctypes.byref(out)) == NULL
    L.sbm_occ_tree_destroy(None)   # tolerated
    assert L.sbm_occ_tree_build(None, 0, None, 1) == NULL
    assert L.sbm_occ_tree_build(None, 7, ctypes.byref(rp), 1) == NULL           # before the reading is looked at
    assert L.sbm_occ_tree_info(None, ctypes.byref(info)) == NULL
    assert L.sbm_occ_tree_search_device(None, 1, a.ctypes.data, 0, 0.0, s.ctypes.data, None, None, 1) == NULL
    assert L.sbm_occ_tree_search_device(None, 0, None, 17, float("nan"), None, None, None, 1) == NULL     # n == 0 needs a tree too
    assert L.sbm_occ_tree_search(None, 1, a.ctypes.data, 0, 0.0, s.ctypes.data, None, None) == NULL
    assert L.sbm_occ_tree_search(None, 0, None, 0, 0.0, None, None, None) == NULL
    assert L.sbm_occ_tree_leaves_device(None, 0, k.ctypes.data, s.ctypes.data, None, 4, ctypes.byref(n)) == NULL
    assert L.sbm_occ_tree_leaves(None, 17, k.ctypes.data, s.ctypes.data, None, 4, ctypes.byref(n)) == NULL
    assert L.sbm_occ_tree_binary_device(None, k.ctypes.data, 32, ctypes.byref(n)) == NULL
    assert L.sbm_occ_tree_write_binary(None, b"x.bt") == NULL
    assert n.value == 7 and not a.any() and not s.any() and not k.any()          # no refused call wrote through a pointer


def test_cpp_adaptor_compiles(tmp_path, pkg):
    _, r = build_callsite(tmp_path, "occupancy_tree_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr


def test_header_states_the_contract():
    text = (ROOT / "include" / "sbm.h").read_text()
    part = text[text.index("occupancy map: the octree above the voxels"):text.index("visual-word dictionary: addNewWords")]
    for phrase in ('"occ_tree_build"', '"occ_tree_query"', "SNAPSHOT", "toMaxLikelihood", "isNodeCollapsible", "adjustKeyAtDepth",
                   "computeChildIdx", "no collapsed proper ancestor", "calcNumNodes", "begin_leafs(maxDepth)", "float ==",
                   "not even a root", "0x7FC00000", "depth 0 means 16", "byte for byte", "getMetricMin", "never built"):
        assert phrase in part, phrase
