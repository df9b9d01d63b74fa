"""The time stamps' C-ABI without a GPU: declarations against exports and bindings, the checks that come before any launch, the
C++ adaptor compiling with -Wall -Werror, and what include/sbm.h, the sources, the fixture and the fixture kit must say. The checks
that need a map are in tests/test_gpu_occupancy_stamped.py."""
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
import occupancy_stamped_cases as sc  # noqa: E402
from gpu_support import build_callsite  # noqa: E402

CALLS = ("sbm_occ_stamp_enable", "sbm_occ_stamp_enabled", "sbm_occ_stamp_set_time", "sbm_occ_stamp_time", "sbm_occ_stamp_degrade",
         "sbm_occ_stamp_forget", "sbm_occ_stamp_search_device", "sbm_occ_stamp_search", "sbm_occ_stamp_fetch_device", "sbm_occ_stamp_fetch",
         "sbm_occ_stamp_leaves_device", "sbm_occ_stamp_leaves", "sbm_occ_stamp_root", "sbm_occ_stamp_ot_write", "sbm_occ_stamp_ot_info",
         "sbm_occ_stamp_ot_leaves", "sbm_occ_stamp_ot_load", "sbm_occ_stamp_ot_read")
# the closed prefixes, as tests/test_occupancy_tree_cabi.py, tests/test_occupancy_ot_cabi.py and tests/test_occupancy_color_cabi.py pin them
TREE = {"sbm_occ_tree_create", "sbm_occ_tree_destroy", "sbm_occ_tree_build", "sbm_occ_tree_info", "sbm_occ_tree_search_device", "sbm_occ_tree_search",
        "sbm_occ_tree_leaves_device", "sbm_occ_tree_leaves", "sbm_occ_tree_binary_device", "sbm_occ_tree_write_binary"}
OT = {"sbm_occ_ot_body_device", "sbm_occ_ot_write", "sbm_occ_ot_info", "sbm_occ_ot_leaves", "sbm_occ_ot_load", "sbm_occ_ot_read"}
COLOR = 17
NULL, SIZE, UNSUPPORTED = -1, -2, -23
CSRC = ROOT / "u96-slam_amd" / "csrc"


def test_declarations_against_exports_and_bindings(pkg):
    text = (ROOT / "include" / "sbm.h").read_text()
    declared = set(re.findall(r"^(?:int|void) (sbm_occ_\w+)\(", text, re.M))
    assert {d for d in declared if d.startswith("sbm_occ_stamp_")} == set(CALLS), "the sbm_occ_stamp_ set is closed"
    r = subprocess.run(["nm", "-D", "--defined-only", str(pkg.library_path())], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in r.stdout.splitlines() if " T " in line}
    assert set(CALLS) <= exported and {e for e in exported if e.startswith("sbm_occ_")} == declared
    assert {e for e in exported if e.startswith("sbm_occ_tree_")} == TREE and {e for e in exported if e.startswith("sbm_occ_ot_")} == OT
    assert len({e for e in exported if e.startswith("sbm_occ_color_")}) == COLOR
    L = pkg.load_library()
    for name in CALLS:
        assert getattr(L, name).argtypes is not None, name
    flat = " ".join(text.split())
    for decl in ("int sbm_occ_stamp_enable(sbm_occ_map* map);", "int sbm_occ_stamp_enabled(const sbm_occ_map* map, int* enabled);",
                 "int sbm_occ_stamp_set_time(sbm_occ_map* map, uint32_t clock);", "int sbm_occ_stamp_time(const sbm_occ_map* map, uint32_t* clock);",
                 "int sbm_occ_stamp_degrade(sbm_occ_map* map, uint32_t time_thres, const sbm_occ_ray_params* params, uint64_t* degraded);",
                 "int sbm_occ_stamp_forget(sbm_occ_map* map, uint32_t time_thres, uint64_t* removed);",
                 "int sbm_occ_stamp_fetch(sbm_occ_map* map, uint64_t* keys, float* logodds, uint32_t* stamps, size_t cap, size_t* count);"):
        assert decl in flat, decl
    for m in ("leaves_stamps", "leaves_stamps_device", "last_update_time", "write_stamped_ot", "stamped_ot"):
        assert callable(getattr(pkg.OccupancyTree, m)), m
    assert callable(pkg.OccupancyMap.load_stamped_ot) and callable(pkg.occ_stamped_ot_info) and callable(pkg.occ_stamped_ot_leaves)
    for m in ("enable_stamps", "stamps_enabled", "set_time", "time", "degrade_outdated", "forget_older_than", "search_stamps", "fetch_stamps", "fetch_stamps_device"):
        assert callable(getattr(pkg.OccupancyMap, m)), m


def test_null_arguments_come_first(pkg):
    L = pkg.load_library()
    odd = ctypes.c_void_p(3)
    n = ctypes.c_size_t(5)
    c = ctypes.c_uint32(7)
    on = ctypes.c_int(7)
    count = ctypes.c_uint64(7)
    assert L.sbm_occ_stamp_enable(None) == NULL and L.sbm_occ_stamp_enabled(None, ctypes.byref(on)) == NULL and on.value == 7
    assert L.sbm_occ_stamp_set_time(None, 1) == NULL and L.sbm_occ_stamp_time(None, ctypes.byref(c)) == NULL and c.value == 7
    assert L.sbm_occ_stamp_degrade(None, 0, odd, ctypes.byref(count)) == NULL and L.sbm_occ_stamp_forget(None, 0, ctypes.byref(count)) == NULL and count.value == 7
    assert L.sbm_occ_stamp_search_device(None, 1, odd, float("nan"), odd, odd, odd, 1) == NULL
    assert L.sbm_occ_stamp_search(None, 1, odd, float("nan"), odd, odd, odd) == NULL
    assert L.sbm_occ_stamp_fetch_device(None, odd, odd, odd, 1, ctypes.byref(n)) == NULL and L.sbm_occ_stamp_fetch(None, odd, odd, odd, 1, ctypes.byref(n)) == NULL
    assert L.sbm_occ_stamp_leaves(None, 99, odd, odd, odd, odd, 1, ctypes.byref(n)) == NULL and L.sbm_occ_stamp_leaves_device(None, 99, odd, odd, odd, odd, 1, ctypes.byref(n)) == NULL
    assert L.sbm_occ_stamp_root(None, ctypes.byref(c)) == NULL and L.sbm_occ_stamp_ot_write(None, b"x") == NULL
    assert L.sbm_occ_stamp_ot_load(None, odd, 1, 1) == NULL and L.sbm_occ_stamp_ot_read(None, b"x", 1) == NULL
    assert L.sbm_occ_stamp_ot_info(None, 0, None) == NULL and L.sbm_occ_stamp_ot_leaves(None, 0, None, None, None, 0, None) == NULL
    assert n.value == 5 and c.value == 7


def test_every_check_before_a_launch_has_its_code():
    src = (CSRC / "sbm_occ_stamp.hip").read_text()
    enable = src[src.index("int sbm_occ_stamp_enable("):src.index("int sbm_occ_stamp_enabled(")]
    assert enable.index("SBM_ERR_NULL") < enable.index("map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED") < \
        enable.index("if (map->color.p) return SBM_ERR_UNSUPPORTED") < enable.index("dscope.enter()") < enable.index("words.grow(") < \
        enable.index("hipMemsetAsync(words.p, 0,") < enable.index("SBM_ERR_NOMEM") < enable.index("occ_logodds_alloc(map)") < \
        enable.index("std::swap(map->stamp, words)") < enable.index("map->mode = kOccModeLogOdds"), "the words first: a refused allocation leaves the map as it was"
    occ = (CSRC / "sbm_occupancy.hip").read_text()
    assert occ.count("if (map->stamp.p) return SBM_ERR_UNSUPPORTED;   // stamp words belong to a log-odds map") == 2, "both hit inserts refuse a map with stamp words"
    degrade = src[src.index("int sbm_occ_stamp_degrade("):src.index("int sbm_occ_stamp_search_device(")]
    assert degrade.index("SBM_ERR_NULL") < degrade.index("occ_ray_params_check(params)") < degrade.index("!map->stamp.p") < degrade.index("dscope.enter()") < \
        degrade.index("occ_stamp_degrade_kernel")
    assert "atomic" not in src[src.index("occ_stamp_degrade_kernel(OccStampDegrade g)"):src.index("occ_wave_count(degraded")], "plain stores on the words"
    assert "time(" not in src.replace("sbm_occ_stamp_set_time(", "").replace("sbm_occ_stamp_time(", ""), "the library never reads the wall clock"
    edit = (CSRC / "sbm_occ_edit.hip").read_text()
    forget = edit[edit.index("int sbm_occ_stamp_forget("):edit.index("int sbm_occ_last_edit(")]
    assert forget.index("SBM_ERR_NULL") < forget.index("!map->stamp.p") < forget.index("dscope.enter()") < forget.index("occ_delete_call(") < forget.index("occ_mark_older_kernel")
    color = (CSRC / "sbm_occ_color.hip").read_text()
    call = color[color.index("static int occ_color_call("):color.index("static OccColorRead occ_color_read(")]
    assert call.index("map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED") < call.index("if (map->stamp.p) return SBM_ERR_UNSUPPORTED") < call.index("dscope.enter()")
    load = color[color.index("static int occ_color_load_run("):]
    assert load.index("if (map->stamp.p) return SBM_ERR_UNSUPPORTED") < load.index("occ_color_load_body(")
    # the paths of a map without stamps: the switch is a template parameter of the two APPLY kernels whose plain instantiations keep
    # their names, the move and the clear touch the words only where they exist
    rays = (CSRC / "sbm_occ_rays.hip").read_text()
    assert "template <bool kTrack> __global__ void __launch_bounds__(256) occ_rays_apply_kernel(OccRay g, OccTable t) {\n  occ_rays_apply<kTrack, false>(g, t, nullptr, 0u);" in rays
    assert "occ_rays_apply<kTrack, true>(g, t, stamps, clock);" in rays and "if (map->stamp.p)   // the clock as it is at this call" in rays
    assert "__global__ void __launch_bounds__(256) occ_edit_apply_kernel(OccEdit e) { occ_edit_apply<false>(e, nullptr, 0u); }" in edit
    assert "if (map->stamp.p) hipLaunchKernelGGL(occ_edit_apply_stamped_kernel," in edit
    grow = (CSRC / "sbm_occ_grow.hip").read_text()
    assert "if (e == hipSuccess && map->stamp.p) e = b->stamp.grow(" in grow and "const unsigned* old_stamps = stamp.p ?" in grow
    assert "else if (old_stamps) hipLaunchKernelGGL(occ_rehash_stamped_kernel," in grow
    assert "if (map->stamp.p) HIPCHK(h, hipMemsetAsync(map->stamp.p, 0," in (CSRC / "sbm_occupancy.hip").read_text()
    for text in (src, rays, edit, grow):
        assert not re.search(r"atomic\w*\(&?\w*stamps?\b", text), "no atomics on stamp words"
    mk = (ROOT / "Makefile").read_text()
    assert mk.count("sbm_occ_stamp.o") == 1 and mk.count("sbm_occ_stamp.hip") == 1 and "$(OCC_OBJS): HIPFLAGS += -ffp-contract=off" in mk


def test_the_stream_parsers_refuse_each_others_ids(pkg):
    """plain and colour parsers on the stamped id and vice versa; the stamped parser equals the restatement on the recorded streams"""
    import occupancy_color_cases as cc
    L = pkg.load_library()
    h = pkg.OccOtHeader()
    stamped = sc.recorded("blocks")[2][4][0][2]
    plain = stamped.replace(b"id OcTreeStamped\n", b"id OcTree\n")
    colour = cc.recorded("blocks")[2][1]

    def status(call, data):
        buf = np.frombuffer(data, np.uint8)
        return call(buf.ctypes.data, len(buf), ctypes.byref(h))

    assert status(L.sbm_occ_ot_info, stamped) == UNSUPPORTED and status(L.sbm_occ_color_ot_info, stamped) == UNSUPPORTED
    assert status(L.sbm_occ_stamp_ot_info, plain) == UNSUPPORTED == sc.parse(plain, 0.1).status and status(L.sbm_occ_stamp_ot_info, colour) == UNSUPPORTED
    assert status(L.sbm_occ_stamp_ot_info, stamped) == 0 == sc.parse(stamped, 0.1).status and status(L.sbm_occ_ot_info, plain) == 0
    assert status(L.sbm_occ_stamp_ot_info, stamped[:-1]) == SIZE == sc.parse(stamped[:-1], 0.1).status
    for name in ("blocks", "resume"):
        for step in sc.recorded(name):
            if len(step) < 5:
                continue
            data = step[4][0][2]
            p = sc.parse(data, 0.1)
            info = pkg.occ_stamped_ot_info(data)
            assert info["size"] == info["nodes"] == p.size == len(step[4][0][0][0]) and info["leaves"] == len(p.leaves) == int(step[4][0][0][4].sum())
            keys, depth, value = pkg.occ_stamped_ot_leaves(data)
            assert np.array_equal(depth, [d for _, d, _ in p.leaves]) and np.array_equal(value.view(np.uint32), [v for _, _, v in p.leaves])
    tree = (CSRC / "sbm_occ_tree.hip").read_text()
    assert "__global__ void __launch_bounds__(256) occ_tree_parents_kernel(OccLevel c, OccLevel p, const unsigned* __restrict__ tile_off, int leaves) {\n  occ_tree_parents<false>(c, p, tile_off, leaves, nullptr, nullptr, 0u);" in tree
    assert "if (kStamp) equal = equal && cs[j] == cs[i];" in tree and "if (kStamp) ps[at] = collapsed ? cs[i] : clock;" in tree
    assert "const bool stamped = map->stamp.p != nullptr;   // only over a map with stamps" in tree


def test_cpp_adaptor_compiles_with_warnings_as_errors(tmp_path):
    _, r = build_callsite(tmp_path, "occupancy_stamped_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr
    hpp = (ROOT / "include" / "sbm_occupancy.hpp").read_text()
    for name in ("void enableStamps()", "bool stampsEnabled()", "void setTime(uint32_t clock)", "uint32_t time()", "uint64_t degradeOutdatedNodes(unsigned int time_thres)",
                 "uint64_t forgetOlderThan(unsigned int time_thres)", "int searchStamped(float x, float y, float z, float* logodds, uint32_t* stamp)",
                 "std::vector<uint64_t> leavesStamped(std::vector<float>& logodds, std::vector<uint32_t>& stamps)", "unsigned int getLastUpdateTime()",
                 "std::vector<OccupancyLeaf> leavesStamped(std::vector<uint32_t>& stamps, unsigned max_depth = 0)", "void writeStamped(const std::string& path)",
                 "bool readStamped(const std::string& filename)", "bool readStamped(const void* bytes, size_t n)"):
        assert name in hpp, name


def test_header_states_the_contract():
    text = (ROOT / "include" / "sbm.h").read_text()
    head = "---- occupancy map: time stamps per voxel"
    assert text.index("---- occupancy map: colour per voxel") < text.index(head) < text.index("---- visual-word dictionary: addNewWords")
    part = text[text.index(head):text.index("---- visual-word dictionary: addNewWords")]
    flat = " ".join(re.sub(r"\n \*", " ", part).split())
    for phrase in ("OcTreeStamped.cpp:43-68", "One uint32 per slot", "the library never reads the wall clock", "nothing requires the clock to be monotone",
                   "existing voxels have stamp 0, as after a load", "a hit map is refused with SBM_ERR_UNSUPPORTED", "a map is one octomap class",
                   "allocates nothing and launches exactly what it launched before", "UNLESS updateNode's early return applies", "OccupancyOcTreeBase.hxx:307-317",
                   "(update >= 0 and value >= clamp max) or (update <= 0 and value <= clamp min)", "An update of exactly 0 tests both",
                   "saturates at the fifth hit and keeps stamp 1004", "restated, not repaired", "take effect in item order", "never stamps, and a voxel it creates has stamp 0",
                   "it starts from stamp 0", "Growth and the deletes' move carry the word with the key", "leave stamp 0 everywhere", "does not override writeData / readData",
                   "(uint32)(clock - stamp) > time_thres", "a clock below a stamp makes a huge age", "The stamp is untouched and change detection is untouched",
                   "One lane per slot, plain stores", "an extension, not octomap", "whatever its value", "then deleteNode of each", "no atomics on stamp words",
                   "lazy_eval = true", "builds octomap's STAMPED pruned tree, in both readings", "compares value AND stamp", "keep refusing `id OcTreeStamped`",
                   "16 nodes and 1 leaf", "24 nodes and 8 leaves", "NOT the plain tree's", "common stamp (copyData)", "the map's clock at build time",
                   "getLastUpdateTime() (sbm_occ_stamp_root)", "a template switch of the level kernel", "does not override writeData", "a tree read back has stamp 0 everywhere",
                   "refuse every other id", "a refused stream leaves the map as it was",
                   "no new names", '"occ_rays_apply"', '"occ_search"', '"occ_fetch"', "DESIGN.md section 30"):
        assert phrase in flat, phrase
    assert "Not provided either: OcTreeStamped" not in text
    design = (ROOT / "DESIGN.md").read_text()
    assert "## 30. Occupancy map: a time stamp per voxel" in design
    assert "degradeOutdatedNodes" in (ROOT / "README.md").read_text() and "enable_stamps" in (ROOT / "INTEGRATION.md").read_text()


def test_the_fixture_is_the_committed_one_and_the_kit_runs_its_generator():
    import octomap_kit as kit

    npz = ROOT / "tests" / "golden" / "occupancy_stamped.npz"
    want, name = (ROOT / "tests" / "golden" / "occupancy_stamped.sha256").read_text().split()
    assert name == npz.name and hashlib.sha256(npz.read_bytes()).hexdigest() == want
    assert npz.stat().st_size < 200 << 10
    cpu = json.loads((ROOT / "tests" / "golden" / "occupancy_stamped_cpu.json").read_text())
    assert set(cpu["calls"]["frames"]) == {"insert_ms", "prune_update_ms", "degrade_ms", "forget_ms"} and cpu["threads"] == 1 and "across two machines" in cpu["what"]
    assert kit.MORE_FIXTURES["stamped"] == "make_occupancy_stamped_fixtures.py" and list(kit.MORE_FIXTURES)[:3] == ["edit", "planner", "color"]
    assert (ROOT / "tools" / kit.MORE_FIXTURES["stamped"]).exists()
    driver = (ROOT / "tools" / "octomap_drivers" / "stamped.cpp").read_text()
    assert "lazy_eval = true" in driver and "This project's text; it calls octomap's API only." in driver and 'extern "C" time_t time(time_t* t)' in driver
    assert sc.NAMES == [str(n) for n in np.load(npz)["names"]]
