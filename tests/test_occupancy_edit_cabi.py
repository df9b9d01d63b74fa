"""The edits' C-ABI without a GPU: declarations against exports and bindings, the checks that come before any launch, the C++
adaptor compiling against the library with -Wall -Werror, and what include/sbm.h, the fixture and the fixture kit must say. The
checks that need a map are in tests/test_gpu_occupancy_edit.py."""
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
from gpu_support import build_callsite  # noqa: E402

CALLS = ("sbm_occ_edit_device", "sbm_occ_edit", "sbm_occ_edit_points_device", "sbm_occ_edit_points", "sbm_occ_delete_device",
         "sbm_occ_delete", "sbm_occ_delete_box", "sbm_occ_last_edit")
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
    assert L.sbm_occ_edit_points_device.argtypes == L.sbm_occ_edit_device.argtypes and L.sbm_occ_edit_points.argtypes == L.sbm_occ_edit.argtypes
    flat = " ".join(text.split())
    for decl in ("int sbm_occ_edit_device(sbm_occ_map* map, size_t n, const void* d_keys, const void* d_ops, const void* d_values, "
                 "const sbm_occ_ray_params* params, int sync);",
                 "int sbm_occ_edit(sbm_occ_map* map, size_t n, const uint64_t* keys, const uint8_t* ops, const float* values, "
                 "const sbm_occ_ray_params* params);",
                 "int sbm_occ_delete_device(sbm_occ_map* map, size_t n, const void* d_keys, int depth);",
                 "int sbm_occ_delete(sbm_occ_map* map, size_t n, const uint64_t* keys, int depth);",
                 "int sbm_occ_delete_box(sbm_occ_map* map, const uint16_t min_key[3], const uint16_t max_key[3], int outside);",
                 "int sbm_occ_last_edit(sbm_occ_map* map, sbm_occ_edit_info* out);",
                 "enum { SBM_OCC_EDIT_UPDATE = 0, SBM_OCC_EDIT_SET = 1, SBM_OCC_EDIT_DELETE = 2 };", "#define SBM_OCC_EDIT_CHUNK 2097152"):
        assert decl in flat, decl
    assert (pkg.OCC_EDIT_UPDATE, pkg.OCC_EDIT_SET, pkg.OCC_EDIT_DELETE, pkg.OCC_EDIT_CHUNK) == (0, 1, 2, 2097152)
    assert ctypes.sizeof(pkg.OccEditInfo) == 40 and [f[0] for f in pkg.OccEditInfo._fields_] == ["items", "skipped", "lost", "created", "removed"]
    for m in ("update_nodes", "set_node_values", "delete_nodes", "delete_box", "edit", "last_edit"):
        assert callable(getattr(pkg.OccupancyMap, m)), m


def test_null_arguments_come_first(pkg):
    """Every entry point answers SBM_ERR_NULL for a missing map before it looks at anything else: the other arguments here are
    ones a later check would refuse (a misaligned pointer, invalid parameters, a depth of 99)."""
    L = pkg.load_library()
    bad = pkg.occ_ray_params(prob_hit=2.0)
    odd = ctypes.c_void_p(3)
    info = pkg.OccEditInfo(7, 7, 7, 7, 7)
    assert L.sbm_occ_edit_device(None, 1, odd, odd, odd, ctypes.byref(bad), 1) == NULL
    assert L.sbm_occ_edit(None, 1, odd, odd, odd, ctypes.byref(bad)) == NULL
    assert L.sbm_occ_edit_points_device(None, 1, odd, odd, odd, ctypes.byref(bad), 1) == NULL
    assert L.sbm_occ_edit_points(None, 1, odd, odd, odd, ctypes.byref(bad)) == NULL
    assert L.sbm_occ_delete_device(None, 1, odd, 99) == NULL and L.sbm_occ_delete(None, 1, odd, 99) == NULL
    assert L.sbm_occ_delete_box(None, None, None, 0) == NULL
    assert L.sbm_occ_last_edit(None, ctypes.byref(info)) == NULL and info.items == 7 and info.removed == 7


def test_every_check_before_a_launch_has_its_code():
    """The order of the family: NULL first, then sizes (the parameters), then what is unsupported (the count, alignment, the
    mode, the depth), read off the entry points' text, since a map needs a GPU."""
    src = (ROOT / "u96-slam_amd" / "csrc" / "sbm_occ_edit.hip").read_text()
    check = src[src.index("static int occ_edit_check("):src.index("static int occ_edit_call(")]
    assert check.index("SBM_ERR_NULL") < check.index("occ_ray_params_check(p)") < check.index("n > kOccEditMax") < check.index("SBM_ERR_UNSUPPORTED")
    for name in ("sbm_occ_edit_device", "sbm_occ_edit_points_device"):
        body = src[src.index(f"int {name}("):]
        body = body[:body.index("\n}\n")]
        assert body.index("occ_edit_check(") < body.index("& 3)") < body.index("SBM_ERR_UNSUPPORTED") < body.index("occ_edit_call(")
    call = src[src.index("static int occ_edit_call("):]
    assert call.index("map->mode == kOccModeHits) return SBM_ERR_UNSUPPORTED") < call.index("dscope.enter()") < call.index("occ_logodds_alloc")
    body = src[src.index("int sbm_occ_delete_device("):]
    assert body.index("SBM_ERR_NULL") < body.index("& 7) return SBM_ERR_UNSUPPORTED") < body.index("occ_delete_keys(")
    keys = src[src.index("static int occ_delete_keys("):]
    assert keys.index("occ_depth_mask(depth, &mask)) return SBM_ERR_UNSUPPORTED") < keys.index("n > kOccEditMax) return SBM_ERR_UNSUPPORTED") < \
        keys.index("dscope.enter()")
    # the move's table comes before anything is applied, and a refusal leaves through SBM_ERR_NOMEM with the error kept
    chunk = src[src.index("static int occ_edit_chunk_run("):src.index("static int occ_edit_check(")]
    assert chunk.index("occ_move_alloc(") < chunk.index("occ_edit_claim_kernel") < chunk.index("occ_edit_apply_kernel")
    grow = (ROOT / "u96-slam_amd" / "csrc" / "sbm_occ_grow.hip").read_text()
    alloc = grow[grow.index("int occ_move_alloc("):grow.index("int occ_move_run(")]
    assert "h->last_hip = (int)e" in alloc and "SBM_ERR_NOMEM" in alloc and "hipLaunchKernelGGL" not in alloc and "Memset" not in alloc


def test_cpp_adaptor_compiles_with_warnings_as_errors(tmp_path):
    _, r = build_callsite(tmp_path, "occupancy_edit_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr
    hpp = (ROOT / "include" / "sbm_occupancy.hpp").read_text()
    for name in ("void updateNode(uint64_t key, float log_odds_update, bool lazy_eval = false)",
                 "void updateNode(const float point[3], float log_odds_update, bool lazy_eval = false)",
                 "void updateNode(uint64_t key, bool occupied, bool lazy_eval = false)",
                 "void updateNode(const float point[3], bool occupied, bool lazy_eval = false)",
                 "void updateNode(const std::vector<uint64_t>& keys, const std::vector<float>& log_odds_updates, bool lazy_eval = false)",
                 "void updateNode(const std::vector<uint64_t>& keys, bool occupied, bool lazy_eval = false)",
                 "void setNodeValue(uint64_t key, float log_odds_value, bool lazy_eval = false)",
                 "void setNodeValue(const float point[3], float log_odds_value, bool lazy_eval = false)",
                 "bool deleteNode(uint64_t key, unsigned depth = 0)", "bool deleteNode(const float point[3], unsigned depth = 0)",
                 "void deleteBBX(const uint16_t min[3], const uint16_t max[3], bool outside = false)",
                 "void deleteBBX(const float min[3], const float max[3], bool outside = false)", "sbm_occ_edit_info lastEdit()"):
        assert name in hpp, name


def test_header_states_the_contract():
    text = (ROOT / "include" / "sbm.h").read_text()
    head = "---- occupancy map: edit voxels by key"
    assert text.index("---- occupancy map: growth") < text.index(head) < text.index("---- visual-word dictionary: addNewWords")
    part = text[text.index(head):text.index("---- visual-word dictionary: addNewWords")]
    flat = " ".join(re.sub(r"\n \*", " ", part).split())       # the comment's line breaks are not part of a phrase
    for phrase in ("OccupancyOcTreeBase.hxx:273-285, 307-327, 373-433, 1097-1107", "OcTreeBaseImpl.hxx:501-509, 681-716",
                   "IEEE binary32 as written, with no contraction", "EARLY ABORT", "(u >= 0 && v >= cmax) or (u <= 0 && v <= cmin)",
                   "nothing happens at all, and no change record is made either", "an absent voxel is created at 0",
                   "v = cmin if v < cmin, else cmax if v > cmax", "The C-ABI takes floats only", "so a NaN stays NaN",
                   "d 0 means 16", "in their top d bits", "Deleting what is not there is not an error",
                   "none -> flipped, flipped -> none, and created stays", "is skipped, where octomap returns NULL or false",
                   "An item with a bit above 47 set is skipped", "cannot be checked on the host for device arrays",
                   "take effect in item order", "set then update differs from update then set", "delete then update creates again from 0",
                   "Items of different voxels do not interact", "Calls take effect in call order",
                   "DIVERGENCE, deleting the last voxel", "octomap keeps a childless root, which its search then returns for every key",
                   "DIVERGENCE, a deleted voxel's change record", "std::map::insert then does not overwrite it",
                   "they fix the mode of a fresh map", "leave the map as it was", "serve both modes", "a hit map loses the key and its count",
                   "n is up to 2^30", "SBM_OCC_EDIT_CHUNK = 2097152 items, in item order", "that voxel gets none of its items",
                   "every other voxel gets all of its own", "the claim pass is idempotent", "same capacity", "it never shrinks",
                   "there are no tombstones", "allocated before anything is applied", "SBM_ERR_NOMEM", "the map is exactly as it was",
                   "cannot be captured in a graph", "the overflow counter is unchanged", "a tree built earlier is a snapshot",
                   "found from the sorted keys, not from lane position", "it is stable, so item order inside a voxel's run survives",
                   "plain vector stores", "No float atomics, no spin waits, no grid barriers", "no new names", '"occ_rays_mark"',
                   '"occ_rays_apply"', '"occ_insert"', "DESIGN.md section 27"):
        assert phrase in flat, phrase
    free_space = text[text.index("occupancy map: ray-cast free space"):text.index("occupancy map: queries")]
    assert "The table never frees a slot -- the one exception is a delete" in " ".join(re.sub(r"\n \*", " ", free_space).split())
    design = (ROOT / "DESIGN.md").read_text()
    for section in ("## 19.", "## 20."):
        at = design.index(section)
        limits = design[at:design.index("\n## ", at + 1)]
        for line in limits.splitlines():
            if "ot provided" in line or "imits" in line[:12]:
                assert "deleteNode" not in line, line
    assert "## 27. Occupancy map: edit and forget voxels" in design


def test_the_fixture_is_the_committed_one_and_the_kit_runs_its_generator_last():
    import octomap_kit as kit

    npz = ROOT / "tests" / "golden" / "occupancy_edit.npz"
    want, name = (ROOT / "tests" / "golden" / "occupancy_edit.sha256").read_text().split()
    assert name == npz.name and hashlib.sha256(npz.read_bytes()).hexdigest() == want
    assert npz.stat().st_size < 1 << 20
    cpu = json.loads((ROOT / "tests" / "golden" / "occupancy_edit_cpu.json").read_text())
    assert {"all_distinct", "sixteen_per_voxel", "sixty_four_voxels", "box_delete_half"} <= set(cpu["calls"]) and cpu["threads"] == 1
    assert all(c["ms"] > 0 for c in cpu["calls"].values())
    # an open mapping behind the two closed ones: the chain runs it last, load() orders it after both
    assert "edit" in kit.MORE_FIXTURES and not set(kit.MORE_FIXTURES) & (set(kit.FIXTURES) | set(kit.LATER_FIXTURES))
    for tool in kit.MORE_FIXTURES.values():
        assert (ROOT / "tools" / tool).exists()
    src = (ROOT / "tools" / "octomap_kit.py").read_text()
    assert "list(FIXTURES.values()) + list(LATER_FIXTURES.values()) + list(MORE_FIXTURES.values())" in src and "MORE_FIXTURES" in kit.__doc__
    assert np.array_equal(kit.load("options", "edit")["names"], np.load(ROOT / "tests" / "golden" / "occupancy_options.npz")["names"])
    assert np.array_equal(kit.load("octomap", "edit")["scene_disp"], np.load(npz)["scene_disp"])
    try:
        kit.load("edit", "options")
    except AssertionError:
        pass
    else:
        raise AssertionError("an earlier fixture's generator may not read a later fixture")
    assert (ROOT / "tools" / "octomap_drivers" / "edit.cpp").exists()
