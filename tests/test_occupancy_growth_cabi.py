"""The occupancy map's growth C-ABI without a GPU: declarations against exports and bindings, the checks that need no device,
the policy sbm_occ_growth_step over a table of cases, the C++ adaptor compiling against the library with -Wall -Werror, and
what include/sbm.h must say. The checks that need a map are in tests/test_gpu_occupancy_growth.py."""
import ctypes
import inspect
import pathlib
import re
import subprocess
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
from gpu_support import build_callsite  # noqa: E402

CALLS = ("sbm_occ_capacity", "sbm_occ_reserve", "sbm_occ_set_growth", "sbm_occ_get_growth", "sbm_occ_growth_step")
OK, NULL, UNSUPPORTED, OCC_FULL = 0, -1, -23, -25
LIMIT = 1 << 30


def test_declarations_against_exports_and_bindings(pkg):
    text = (ROOT / "include" / "sbm.h").read_text()
    declared = set(re.findall(r"^(?:int|void) (sbm_occ_\w+)\(", text, re.M))
    assert set(CALLS) <= declared
    r = subprocess.run(["nm", "-D", "--defined-only", str(pkg.library_path())], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in r.stdout.splitlines() if " T " in line}
    assert set(CALLS) <= exported and {e for e in exported if e.startswith("sbm_occ_")} == declared
    assert not any(re.match(r"sbm_occ_(ot|tree)_", c) for c in CALLS)
    L = pkg.load_library()
    for name in CALLS:
        assert getattr(L, name).argtypes is not None, name
    flat = " ".join(text.split())
    for decl in ("int sbm_occ_capacity(sbm_occ_map* map, size_t* capacity);", "int sbm_occ_reserve(sbm_occ_map* map, size_t capacity);",
                 "int sbm_occ_set_growth(sbm_occ_map* map, int enable, size_t max_capacity);",
                 "int sbm_occ_get_growth(sbm_occ_map* map, sbm_occ_growth_info* out);",
                 "int sbm_occ_growth_step(size_t capacity, size_t need, size_t max_capacity, size_t* next);"):
        assert decl in flat, decl
    assert ctypes.sizeof(pkg.OccGrowthInfo) == 56          # int32 enabled, int32 reserved, six uint64: a fixed size
    struct = flat[flat.index("typedef struct sbm_occ_growth_info {"):flat.index("} sbm_occ_growth_info;")]
    assert [n for n, _ in pkg.OccGrowthInfo._fields_] == re.findall(r"(?:int32_t|uint64_t) (\w+);", struct)
    for m in ("reserve", "set_growth", "growth"):
        assert callable(getattr(pkg.OccupancyMap, m)), m
    assert isinstance(pkg.OccupancyMap.capacity, property)


def test_null_arguments_come_first(pkg):
    L = pkg.load_library()
    n = ctypes.c_size_t(7)
    info = pkg.OccGrowthInfo(7, 7, 7, 7, 7, 7, 7, 7)
    assert L.sbm_occ_capacity(None, ctypes.byref(n)) == NULL and L.sbm_occ_reserve(None, 8) == NULL
    assert L.sbm_occ_reserve(None, LIMIT + 1) == NULL                     # before the limit is looked at
    assert L.sbm_occ_set_growth(None, 1, 0) == NULL and L.sbm_occ_set_growth(None, 1, LIMIT + 1) == NULL
    assert L.sbm_occ_get_growth(None, ctypes.byref(info)) == NULL
    assert L.sbm_occ_growth_step(1, 1, 0, None) == NULL and L.sbm_occ_growth_step(LIMIT, 1, 0, None) == NULL
    assert n.value == 7 and [getattr(info, f) for f, _ in info._fields_] == [7] * 8


STEPS = [  # capacity, need, max_capacity -> the next capacity, or None for SBM_ERR_OCC_FULL
    (1, 0, 0, 2), (1, 2, 0, 2), (2, 3, 0, 4), (64, 65, 0, 128), (1000, 1001, 0, 2000),          # it doubles
    (1, 32611, 0, 32611), (64, 129, 0, 129), (4096, 3 * 4096, 0, 3 * 4096),                     # it reaches at least `need`
    (32, 33, 48, 48), (32, 1000, 64, 64), (1, 100, 64, 64), (63, 0, 64, 64),                    # it clamps to the ceiling
    (LIMIT // 2 + 1, 0, 0, LIMIT), (LIMIT - 1, LIMIT + 5, 0, LIMIT), (3, 0, LIMIT + 9, 6),      # ... and to 2^30; a ceiling above it is 2^30
    (LIMIT - 1, 0, LIMIT + 9, LIMIT),
    (64, 65, 64, None), (65, 0, 64, None), (LIMIT, LIMIT + 1, 0, None), (LIMIT + 7, 0, 0, None),  # already at the ceiling
    (8, 0, 0, 16), (8, 0, 12, 12), (0, 0, 0, 1), (0, 5, 0, 5),                                  # need 0 is a plain doubling
]


@pytest.mark.parametrize("capacity,need,ceiling,want", STEPS)
def test_growth_step_is_the_policy(pkg, capacity, need, ceiling, want):
    L = pkg.load_library()
    nxt = ctypes.c_size_t(7)
    st = L.sbm_occ_growth_step(capacity, need, ceiling, ctypes.byref(nxt))
    if want is None:
        assert st == OCC_FULL and nxt.value == 7
        with pytest.raises(pkg.StereoBMError) as e:
            pkg.occ_growth_step(capacity, need, ceiling)
        assert e.value.code == pkg.ERR_OCC_FULL
    else:
        assert st == OK and nxt.value == want == pkg.occ_growth_step(capacity, need, ceiling)
        assert nxt.value > capacity and nxt.value <= (ceiling if 0 < ceiling < LIMIT else LIMIT)


def test_steps_from_one_voxel_only_double(pkg):
    c, seen = 1, []
    while c < LIMIT:
        c = pkg.occ_growth_step(c, c + 1)
        seen.append(c)
    assert seen == [1 << k for k in range(1, 31)]


def test_python_constructor_pops_the_growth_keywords_before_the_map_parameters(pkg):
    src = inspect.getsource(pkg.OccupancyMap.__init__)
    assert src.index('kw.pop("grow"') < src.index("occ_params(**kw)") and src.index('kw.pop("max_capacity"') < src.index("occ_params(**kw)")
    assert src.index('kw.pop("grow"') < src.index("if params is not None and kw")


def test_cpp_adaptor_compiles_with_warnings_as_errors(tmp_path):
    _, r = build_callsite(tmp_path, "occupancy_growth_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr
    hpp = (ROOT / "include" / "sbm_occupancy.hpp").read_text()
    for name in ("void reserve(size_t capacity)", "size_t capacity()", "void setGrowth(bool enable, size_t max_capacity = 0)",
                 "sbm_occ_growth_info growth()"):
        assert name in hpp, name


def test_header_states_the_contract():
    text = (ROOT / "include" / "sbm.h").read_text()
    assert text.index("occupancy map: insert options, discretize") < text.index("occupancy map: growth") < \
        text.index("visual-word dictionary: addNewWords")
    part = text[text.index("occupancy map: growth"):text.index("visual-word dictionary: addNewWords")]
    flat = " ".join(re.sub(r"\n \*", " ", part).split())       # the comment's line breaks are not part of a phrase
    for phrase in ("octomap has no full map", "bit for bit, what the same calls produce on a map created large enough",
                   "Off by default", "growth-off maps launch the same kernels", "a step doubles the capacity", "clamps to the ceiling",
                   "0 is the create limit of 2^30", "the power of two >= 2 * capacity", "at or below one half",
                   "max(the created capacity, 4 * size)", "between MARK and APPLY", "MARK is idempotent",
                   "only when its flag word was clear", '"created this scan" among them', "the touched list is rebuilt",
                   "goes back to its value before the scan", "then APPLY runs once", "cannot run twice", "preceded by a claim pass",
                   "adds no hit", "the unchanged insert kernel finds every key", "they reserve it", "a count above the ceiling still does",
                   "exactly as a growth-off call on the table it has", "sbm_last_hip_error holds the allocation's error",
                   "sync == 0 calls may synchronise internally", "NOT capturable in a graph", "With growth off nothing changes",
                   "beside the old one", "A tree built before a growth answers as built", "DIVERGENCE", "DESIGN.md section 26",
                   "64-bit compare-and-swap", "No float atomics, no spin waits, no grid barriers", "no new names", '"occ_rays_mark"',
                   '"occ_insert"', '"occ_load"', "an explicit sbm_occ_reserve records nothing", "It never shrinks",
                   "the map stays exactly as it was", "Survives sbm_occ_reset", "*next is left alone"):
        assert phrase in flat, phrase
