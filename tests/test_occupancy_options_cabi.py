"""The insert options' C-ABI without a GPU: declarations against exports and bindings, the checks that need no device, the C++
adaptor compiling against the library with -Wall -Werror, and what include/sbm.h and the fixture kit must say. The checks that
need a map are in tests/test_gpu_occupancy_options.py."""
import ctypes
import pathlib
import re
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
from gpu_support import build_callsite  # noqa: E402

CALLS = ("sbm_occ_set_bbx", "sbm_occ_use_bbx_limit", "sbm_occ_get_bbx", "sbm_occ_enable_change_detection",
         "sbm_occ_change_detection_enabled", "sbm_occ_reset_change_detection", "sbm_occ_num_changes", "sbm_occ_fetch_changes_device",
         "sbm_occ_fetch_changes", "sbm_occ_insert_cloud_discrete_device", "sbm_occ_insert_cloud_discrete",
         "sbm_occ_insert_rays_discrete_device", "sbm_occ_insert_rays_discrete")
NULL = -1


def test_declarations_against_exports_and_bindings(pkg):
    text = (ROOT / "include" / "sbm.h").read_text()
    declared = set(re.findall(r"^(?:int|void) (sbm_occ_\w+)\(", text, re.M))
    assert set(CALLS) <= declared
    r = subprocess.run(["nm", "-D", "--defined-only", str(pkg.library_path())], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in r.stdout.splitlines() if " T " in line}
    assert set(CALLS) <= exported and {e for e in exported if e.startswith("sbm_occ_")} == declared
    L = pkg.load_library()
    for name in CALLS:
        assert getattr(L, name).argtypes is not None, name
    assert L.sbm_occ_insert_cloud_discrete_device.argtypes == L.sbm_occ_insert_cloud_device.argtypes
    assert L.sbm_occ_insert_rays_discrete.argtypes == L.sbm_occ_insert_rays.argtypes
    flat = " ".join(text.split())
    for decl in ("int sbm_occ_set_bbx(sbm_occ_map* map, const float min[3], const float max[3]);",
                 "int sbm_occ_get_bbx(sbm_occ_map* map, float min[3], float max[3], uint16_t min_key[3], uint16_t max_key[3], int* enabled);",
                 "int sbm_occ_fetch_changes_device(sbm_occ_map* map, void* d_keys, void* d_created, size_t cap, size_t* count);",
                 "int sbm_occ_fetch_changes(sbm_occ_map* map, uint64_t* keys, uint8_t* created, size_t cap, size_t* count);"):
        assert decl in flat, decl
    for m in ("set_bbx", "use_bbx_limit", "bbx", "enable_change_detection", "reset_change_detection", "num_changes", "changes",
              "changes_device"):
        assert callable(getattr(pkg.OccupancyMap, m)), m


def test_null_arguments_come_first(pkg):
    L = pkg.load_library()
    three, n, on = (ctypes.c_float * 3)(), ctypes.c_size_t(7), ctypes.c_int(7)
    rp = pkg.occ_ray_params()
    model = pkg.StereoModel()
    assert L.sbm_occ_set_bbx(None, three, three) == NULL
    assert L.sbm_occ_use_bbx_limit(None, 1) == NULL and L.sbm_occ_get_bbx(None, None, None, None, None, None) == NULL
    assert L.sbm_occ_enable_change_detection(None, 1) == NULL and L.sbm_occ_change_detection_enabled(None, ctypes.byref(on)) == NULL
    assert L.sbm_occ_reset_change_detection(None) == NULL and L.sbm_occ_num_changes(None, ctypes.byref(n)) == NULL
    assert L.sbm_occ_fetch_changes_device(None, None, None, 0, ctypes.byref(n)) == NULL
    assert L.sbm_occ_fetch_changes(None, None, None, 0, ctypes.byref(n)) == NULL
    assert L.sbm_occ_insert_cloud_discrete_device(None, 0, None, three, ctypes.byref(rp), 1) == NULL
    assert L.sbm_occ_insert_cloud_discrete(None, 0, None, three, ctypes.byref(rp)) == NULL
    assert L.sbm_occ_insert_rays_discrete_device(None, 1, three, 1, 1, 1, ctypes.byref(model), three, ctypes.byref(rp), 1) == NULL
    assert L.sbm_occ_insert_rays_discrete(None, 1, three, 1, 1, 1, ctypes.byref(model), three, ctypes.byref(rp)) == NULL
    assert n.value == 7 and on.value == 7


def test_python_insert_pops_discretize_before_the_ray_parameters(pkg):
    import inspect

    for f in (pkg.OccupancyMap.insert_cloud, pkg.OccupancyMap.insert_rays):
        src = inspect.getsource(f)
        assert src.index('kw.pop("discretize"') < src.index("self._ray_params(params, kw)")


def test_cpp_adaptor_compiles_with_warnings_as_errors(tmp_path):
    _, r = build_callsite(tmp_path, "occupancy_options_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr
    hpp = (ROOT / "include" / "sbm_occupancy.hpp").read_text()
    for name in ("setBBXMin", "setBBXMax", "useBBXLimit", "bbxSet", "getBBXMin", "getBBXMax", "inBBX(const float p[3])",
                 "inBBX(const uint16_t key[3])", "enableChangeDetection", "isChangeDetectionEnabled", "resetChangeDetection",
                 "numChangesDetected", "changedKeys()", "double maxrange = -1., bool lazy_eval = false,"):
        assert name in hpp, name


def test_header_states_the_contract():
    text = (ROOT / "include" / "sbm.h").read_text()
    assert text.index("occupancy map: the .ot format") < text.index("occupancy map: insert options, discretize")
    part = text[text.index("occupancy map: insert options, discretize"):text.index("visual-word dictionary: addNewWords")]
    flat = " ".join(re.sub(r"\n \*", " ", part).split())       # the comment's line breaks are not part of a phrase
    for phrase in ("computeDiscreteUpdate", "UNCHECKED coordToKey", "wraps modulo 65536", "key 232, centre -3253.55", "fits no int, is dropped",
                   "see the voxel centre, not the original point", "does not depend on which duplicate wins", "coordToKeyChecked",
                   "leaves the box as it was", "min > max on an axis is accepted", "in FLOAT", "by KEY, inclusive", "ENDS THE RAY",
                   "An origin outside the box therefore frees nothing", "free -= occupied", "none -> flipped, flipped -> none",
                   "created stays", "keeps what is recorded", "A voxel lost to overflow records nothing", "DIVERGENCE",
                   "survive a reset", "The loaders record nothing", "accepts the flag and ignores it", "a hit insert", "in hit mode",
                   "allocated by the first enable", "without an atomic", "64-bit compare-and-swap", "cleared per scan in stream order",
                   "No float atomics, no spin waits, no grid barriers", "no new names", '"occ_rays_mark"', '"occ_fetch"',
                   "DESIGN.md section 25"):
        assert phrase in flat, phrase
    free_space = text[text.index("occupancy map: ray-cast free space"):text.index("occupancy map: queries")]
    line = next(ln for ln in free_space.splitlines() if "Not provided" in ln)
    assert "insertPointCloudRays" in line and "insert options" in line and "discretize" not in line


def test_the_kit_runs_later_fixtures_after_the_closed_list():
    import octomap_kit as kit

    assert list(kit.FIXTURES) == ["octomap", "rays", "query", "tree", "load", "ot"] and list(kit.LATER_FIXTURES) == ["options"]
    for tool in kit.LATER_FIXTURES.values():
        assert (ROOT / "tools" / tool).exists()
    assert "LATER_FIXTURES" in kit.__doc__
    assert np.array_equal(kit.load("rays", "options")["names"], np.load(ROOT / "tests" / "golden" / "occupancy_rays.npz")["names"])
    assert (ROOT / "tools" / "octomap_drivers" / "options.cpp").exists()
