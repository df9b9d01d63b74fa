"""The colours' C-ABI without a GPU: declarations against exports and bindings, the checks that come before any launch, the host
parser of the ColorOcTree stream against the restatement and under the sanitizers, the C++ adaptor compiling with -Wall -Werror,
and what include/sbm.h, the fixture and the fixture kit must say. The checks that need a map are in
tests/test_gpu_occupancy_color.py."""
import ctypes
import hashlib
import json
import pathlib
import re
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import occupancy_color_cases as cc  # noqa: E402
from gpu_support import build_callsite  # noqa: E402

CALLS = ("sbm_occ_color_keys_device", "sbm_occ_color_keys", "sbm_occ_color_points_device", "sbm_occ_color_points", "sbm_occ_color_last",
         "sbm_occ_color_search_device", "sbm_occ_color_search", "sbm_occ_color_fetch_device", "sbm_occ_color_fetch",
         "sbm_occ_color_leaves_device", "sbm_occ_color_leaves", "sbm_occ_color_ot_body_device", "sbm_occ_color_ot_write",
         "sbm_occ_color_ot_info", "sbm_occ_color_ot_leaves", "sbm_occ_color_ot_load", "sbm_occ_color_ot_read")
# the closed prefixes, as tests/test_occupancy_tree_cabi.py and tests/test_occupancy_ot_cabi.py pin them
TREE = {"sbm_occ_tree_create", "sbm_occ_tree_destroy", "sbm_occ_tree_build", "sbm_occ_tree_info", "sbm_occ_tree_search_device", "sbm_occ_tree_search",
        "sbm_occ_tree_leaves_device", "sbm_occ_tree_leaves", "sbm_occ_tree_binary_device", "sbm_occ_tree_write_binary"}
OT = {"sbm_occ_ot_body_device", "sbm_occ_ot_write", "sbm_occ_ot_info", "sbm_occ_ot_leaves", "sbm_occ_ot_load", "sbm_occ_ot_read"}
NULL, SIZE, UNSUPPORTED = -1, -2, -23


def test_declarations_against_exports_and_bindings(pkg):
    text = (ROOT / "include" / "sbm.h").read_text()
    declared = set(re.findall(r"^(?:int|void) (sbm_occ_\w+)\(", text, re.M))
    assert set(CALLS) <= declared and {d for d in declared if d.startswith("sbm_occ_color_")} == set(CALLS)
    r = subprocess.run(["nm", "-D", "--defined-only", str(pkg.library_path())], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in r.stdout.splitlines() if " T " in line}
    assert set(CALLS) <= exported and {e for e in exported if e.startswith("sbm_occ_")} == declared
    assert {e for e in exported if e.startswith("sbm_occ_tree_")} == TREE and {e for e in exported if e.startswith("sbm_occ_ot_")} == OT
    L = pkg.load_library()
    for name in CALLS:
        assert getattr(L, name).argtypes is not None, name
    assert L.sbm_occ_color_points_device.argtypes == L.sbm_occ_color_keys_device.argtypes and L.sbm_occ_color_points.argtypes == L.sbm_occ_color_keys.argtypes
    flat = " ".join(text.split())
    for decl in ("int sbm_occ_color_keys_device(sbm_occ_map* map, size_t n, const void* d_keys, const void* d_rgb, int op, int sync);",
                 "int sbm_occ_color_keys(sbm_occ_map* map, size_t n, const uint64_t* keys, const uint32_t* rgb, int op);",
                 "int sbm_occ_color_points(sbm_occ_map* map, size_t n, const float* xyz, const uint32_t* rgb, int op);",
                 "int sbm_occ_color_last(sbm_occ_map* map, sbm_occ_color_info* out);",
                 "int sbm_occ_color_ot_load(sbm_occ_map* map, const void* bytes, size_t n, int sync);",
                 "int sbm_occ_color_ot_write(sbm_occ_tree* tree, const char* path);",
                 "enum { SBM_OCC_COLOR_SET = 0, SBM_OCC_COLOR_AVERAGE = 1 };", "#define SBM_OCC_COLOR_WHITE 0x00FFFFFFu"):
        assert decl in flat, decl
    assert (pkg.OCC_COLOR_SET, pkg.OCC_COLOR_AVERAGE, pkg.OCC_COLOR_WHITE) == (0, 1, 0xFFFFFF) == (cc.SET, cc.AVERAGE, cc.WHITE)
    assert ctypes.sizeof(pkg.OccColorInfo) == 32 and [f[0] for f in pkg.OccColorInfo._fields_] == ["items", "found", "unknown", "skipped"]
    for m in ("set_colors", "average_colors", "search_colors", "fetch_colors", "load_color_ot", "last_colors"):
        assert callable(getattr(pkg.OccupancyMap, m)), m
    for m in ("leaves_colors", "color_ot", "write_color_ot", "color_ot_body"):
        assert callable(getattr(pkg.OccupancyTree, m)), m


def test_null_arguments_come_first(pkg):
    L = pkg.load_library()
    odd = ctypes.c_void_p(3)
    info = pkg.OccColorInfo(7, 7, 7, 7)
    n = ctypes.c_size_t(5)
    assert L.sbm_occ_color_keys_device(None, 1, odd, odd, 9, 1) == NULL and L.sbm_occ_color_keys(None, 1, odd, odd, 9) == NULL
    assert L.sbm_occ_color_points_device(None, 1, odd, odd, 9, 1) == NULL and L.sbm_occ_color_points(None, 1, odd, odd, 9) == NULL
    assert L.sbm_occ_color_last(None, ctypes.byref(info)) == NULL and info.items == 7 and info.skipped == 7
    assert L.sbm_occ_color_search_device(None, 1, odd, float("nan"), odd, odd, odd, 1) == NULL
    assert L.sbm_occ_color_search(None, 1, odd, float("nan"), odd, odd, odd) == NULL
    assert L.sbm_occ_color_fetch_device(None, odd, odd, odd, 1, ctypes.byref(n)) == NULL and L.sbm_occ_color_fetch(None, odd, odd, odd, 1, ctypes.byref(n)) == NULL
    assert L.sbm_occ_color_leaves(None, 99, odd, odd, odd, odd, 1, ctypes.byref(n)) == NULL
    assert L.sbm_occ_color_leaves_device(None, 99, odd, odd, odd, odd, 1, ctypes.byref(n)) == NULL
    assert L.sbm_occ_color_ot_body_device(None, odd, 1, ctypes.byref(n)) == NULL and L.sbm_occ_color_ot_write(None, b"x") == NULL
    assert L.sbm_occ_color_ot_load(None, odd, 1, 1) == NULL and L.sbm_occ_color_ot_read(None, b"x", 1) == NULL and n.value == 5
    assert L.sbm_occ_color_ot_info(None, 0, None) == NULL and L.sbm_occ_color_ot_leaves(None, 0, None, None, None, None, 0, None) == NULL


def test_every_check_before_a_launch_has_its_code():
    src = (ROOT / "u96-slam_amd" / "csrc" / "sbm_occ_color.hip").read_text()
    call = src[src.index("static int occ_color_call("):src.index("static OccColorRead occ_color_read(")]
    assert call.index("SBM_ERR_NULL") < call.index("op != SBM_OCC_COLOR_SET") < call.index("map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED") < \
        call.index("& 7)") < call.index("dscope.enter()") < call.index("occ_color_alloc(map)") < call.index("occ_color_chunk_run(")
    chunk = src[src.index("static int occ_color_chunk_run("):src.index("static int occ_color_call(")]
    assert chunk.index("occ_color_find_kernel") < chunk.index("occ_sort_run(") < chunk.index("occ_color_apply_kernel")
    assert "occ_find_or_claim" not in src[:src.index("occ_color_expand_kernel")], "a colour batch looks up, it never claims"
    load = src[src.index("static int occ_color_load_body("):src.index("static int occ_color_load_run(")]
    assert load.index("occ_color_ot_parse(") < load.index("SBM_ERR_OCC_FULL") < load.index("*touched = true") < load.index("occ_clear(map)")
    # the colourless paths: the table's move and clear touch the words only where they exist, and the tree's pass runs only then
    grow = (ROOT / "u96-slam_amd" / "csrc" / "sbm_occ_grow.hip").read_text()
    assert "if (e == hipSuccess && map->color.p) e = b->color.grow(" in grow and "r.old_colors = color.p ?" in grow
    assert "if (map->color.p) HIPCHK(h, hipMemsetD32Async(" in (ROOT / "u96-slam_amd" / "csrc" / "sbm_occupancy.hip").read_text()
    assert "if (st == SBM_OK && map->color.p) st = occ_color_tree_run(t);" in (ROOT / "u96-slam_amd" / "csrc" / "sbm_occ_tree.hip").read_text()
    mk = (ROOT / "Makefile").read_text()
    assert mk.count("sbm_occ_color.o") == 1 and mk.count("sbm_occ_color_host.o") == 1 and "$(OCC_OBJS): HIPFLAGS += -ffp-contract=off" in mk


def test_the_host_parser_equals_the_restatement(pkg):
    for name in cc.NAMES:
        for step in cc.recorded(name):
            if not isinstance(step[0], list):
                continue
            data = step[1]
            p = cc.parse(data, 0.1)
            info = pkg.occ_color_ot_info(data)
            assert p.status == cc.OK and info["size"] == info["nodes"] == p.size == p.nodes and info["leaves"] == len(p.leaves)
            keys, depth, value, color = pkg.occ_color_ot_leaves(data)
            first = np.array([cc.tc.centre_key(c, cc.tc.DEPTH) for c, _, _, _ in p.leaves], np.uint64)
            assert np.array_equal(keys, first) and np.array_equal(depth, [d for _, d, _, _ in p.leaves])
            assert np.array_equal(value.view(np.uint32), [v for _, _, v, _ in p.leaves]) and np.array_equal(color, [w for _, _, _, w in p.leaves])
    good = cc.recorded("blocks")[2][1]
    L = pkg.load_library()
    h = pkg.OccOtHeader()
    for bad, status in ((good.replace(b"id ColorOcTree", b"id OcTree"), UNSUPPORTED), (good[:-1], SIZE), (good.replace(b"res 0.1", b"res 0"), SIZE),
                        (good.replace(b"# Octomap OcTree file", b"# Octomap OcTree binary file"), UNSUPPORTED)):
        buf = np.frombuffer(bad, np.uint8)
        assert L.sbm_occ_color_ot_info(buf.ctypes.data, len(buf), ctypes.byref(h)) == status == cc.parse(bad, 0.1).status
    buf = np.frombuffer(good, np.uint8)
    assert L.sbm_occ_ot_info(buf.ctypes.data, len(buf), ctypes.byref(h)) == UNSUPPORTED, "the plain parser keeps refusing the colour stream"


def test_the_sanitizer_program_runs_clean(tmp_path):
    exe = tmp_path / "occ_color_san"
    csrc = ROOT / "u96-slam_amd" / "csrc"
    r = subprocess.run(["g++", "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                        str(ROOT / "include"), str(csrc / "sbm_occ_bt.hip"), str(csrc / "sbm_occ_color_host.hip"),
                        str(ROOT / "tools" / "occupancy_color_sanitize.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = []
    for name in ("run300", "blocks", "reborn"):
        path = tmp_path / f"{name}.ot"
        path.write_bytes(cc.recorded(name)[-1][1])
        files.append(str(path))
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=300, env={"ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and "inconsistent" not in r.stdout and "top byte" not in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    calls, accepted = (int(x) for x in re.search(r"calls (\d+) accepted (\d+)", r.stdout).groups())
    assert calls > 7000 and 0 < accepted < calls


def test_cpp_adaptor_compiles_with_warnings_as_errors(tmp_path):
    _, r = build_callsite(tmp_path, "occupancy_color_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr
    hpp = (ROOT / "include" / "sbm_occupancy.hpp").read_text()
    for name in ("bool setNodeColor(uint64_t key, uint8_t r, uint8_t g, uint8_t b)", "bool setNodeColor(const float point[3], uint8_t r, uint8_t g, uint8_t b)",
                 "bool averageNodeColor(uint64_t key, uint8_t r, uint8_t g, uint8_t b)", "bool averageNodeColor(const float point[3], uint8_t r, uint8_t g, uint8_t b)",
                 "int search(float x, float y, float z, float* logodds, uint32_t* color)", "void writeColor(const std::string& path)",
                 "bool readColor(const std::string& filename)", "bool readColor(const void* bytes, size_t n)", "sbm_occ_color_info lastColor()",
                 "std::vector<OccupancyLeaf> leavesColors(std::vector<uint32_t>& colors, unsigned max_depth = 0)"):
        assert name in hpp, name
    assert "integrateNodeColor is not provided" in hpp


def test_header_states_the_contract():
    text = (ROOT / "include" / "sbm.h").read_text()
    head = "---- occupancy map: colour per voxel"
    assert text.index("---- occupancy map: the read side for planners") < text.index(head) < text.index("---- visual-word dictionary: addNewWords")
    part = text[text.index(head):text.index("---- visual-word dictionary: addNewWords")]
    flat = " ".join(re.sub(r"\n \*", " ", part).split())
    for phrase in ("ColorOcTree.cpp:96-105, 146-161", "r | g << 8 | b << 16", "isColorSet() == false", "there is no separate flag",
                   "white given as a colour UNSETS the voxel", "SBM_ERR_UNSUPPORTED on a hit map", "allocates nothing and launches exactly what it launched before",
                   "growth and the deletes' move carry the word with the key", "leave every voxel white", "deleted and created again",
                   "Both ops search(key) first", "does nothing", "a bit above 47", "(prev + new) / 2 in int", "a chain that passes through white starts over",
                   "take effect in item order", "a look-up, never a claim", "found from the sorted keys, not from lane position",
                   "no closed form: the white restart breaks it", "DIVERGENCE, pruning during inserts", "lazy_eval = true", "never smeared",
                   "the iteration order of an unordered_set", "unless expand() is called first", "Not provided: integrateNodeColor", "a double exp per voxel",
                   "sits on an integer boundary", "has not been measured and cannot be assumed", "isNodeCollapsible ignores colour",
                   "a collapsed node whose child 0 is white is white even if its siblings are coloured", "The pass runs only when the map has colours",
                   "`id ColorOcTree`", "eight bytes per node", "parses on the host in one pass", "a refused stream leaves the map as it was",
                   "no new names", '"occ_rays_apply"', '"occ_search"', '"occ_fetch"', "DESIGN.md section 29"):
        assert phrase in flat, phrase
    assert "Not provided: ColorOcTree" not in text and "written and read by sbm_occ_color_ot_*" in text
    design = (ROOT / "DESIGN.md").read_text()
    assert "## 29. Occupancy map: a colour per voxel" in design
    assert "averageNodeColor" in (ROOT / "README.md").read_text() and "set_colors" in (ROOT / "INTEGRATION.md").read_text()


def test_the_fixture_is_the_committed_one_and_the_kit_runs_its_generator():
    import octomap_kit as kit

    npz = ROOT / "tests" / "golden" / "occupancy_color.npz"
    want, name = (ROOT / "tests" / "golden" / "occupancy_color.sha256").read_text().split()
    assert name == npz.name and hashlib.sha256(npz.read_bytes()).hexdigest() == want
    assert npz.stat().st_size < 1 << 20
    cpu = json.loads((ROOT / "tests" / "golden" / "occupancy_color_cpu.json").read_text())
    assert set(cpu["calls"]["frame_average"]) == {"color_batch_ms", "prune_update_ms", "write_ms", "read_ms"} and cpu["threads"] == 1
    assert all(v > 0 for v in cpu["calls"]["frame_average"].values()) and "across two machines" in cpu["what"]
    assert kit.MORE_FIXTURES["color"] == "make_occupancy_color_fixtures.py" and list(kit.MORE_FIXTURES)[:2] == ["edit", "planner"]
    assert (ROOT / "tools" / kit.MORE_FIXTURES["color"]).exists() and (ROOT / "tools" / "octomap_drivers" / "color.cpp").exists()
    assert np.array_equal(kit.load("octomap", "color")["scene_disp"], np.load(ROOT / "tests" / "golden" / "occupancy_octomap.npz")["scene_disp"])
    driver = (ROOT / "tools" / "octomap_drivers" / "color.cpp").read_text()
    assert "lazy_eval = true" in driver and "This project's text; it calls octomap's API only." in driver
