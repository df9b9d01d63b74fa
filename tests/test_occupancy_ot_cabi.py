"""The .ot entry points' C-ABI without a GPU: declarations against exports, the structure layout against the mirror, null
arguments first, the host parser (sbm_occ_ot_info / sbm_occ_ot_leaves) on every recorded stream against what octomap's read() left,
on malformed streams and on trees far beyond any map, the C++ adaptor compiling against the library, and what include/sbm.h must
say. The checks that need a map or a tree are in tests/test_gpu_occupancy_ot.py."""
import ctypes
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_ot_cases as oc  # noqa: E402
from gpu_support import build_callsite  # noqa: E402

CALLS = ("sbm_occ_ot_body_device", "sbm_occ_ot_write", "sbm_occ_ot_info", "sbm_occ_ot_leaves", "sbm_occ_ot_load", "sbm_occ_ot_read")
FX = oc.fixture()
NAMES = [str(n) for n in FX["names"]]
SCANS = [(n, s) for n in NAMES for s in range(len(FX[f"{n}_search_found"]))]
GOOD = bytes(FX["scene_ot_0"])
BAD = oc.malformed(GOOD)


def code_of(call, *args):
    try:
        call(*args)
    except Exception as e:      # StereoBMError
        return e.code
    return oc.OK


def test_declarations_against_exports(pkg):
    text = (ROOT / "include" / "sbm.h").read_text()
    declared = set(re.findall(r"^(?:int|void) (sbm_occ_\w+)\(", text, re.M))
    assert set(CALLS) <= declared and not any(c.startswith("sbm_occ_tree_") for c in CALLS)
    r = subprocess.run(["nm", "-D", "--defined-only", str(pkg.library_path())], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in r.stdout.splitlines() if " T " in line}
    assert {e for e in exported if e.startswith("sbm_occ_ot_")} == set(CALLS)
    assert {e for e in exported if e.startswith("sbm_occ_")} == declared
    L = pkg.load_library()
    for name in CALLS:
        assert getattr(L, name).argtypes is not None, name
    flat = " ".join(text.split())
    for decl in ("int sbm_occ_ot_body_device(sbm_occ_tree* tree, void* d_bytes, size_t cap, size_t* nbytes);",
                 "int sbm_occ_ot_write(sbm_occ_tree* tree, const char* path);",
                 "int sbm_occ_ot_info(const void* bytes, size_t n, sbm_occ_ot_header* out);",
                 "int sbm_occ_ot_leaves(const void* bytes, size_t n, uint64_t* first_key, int32_t* depth, float* value, size_t cap, "
                 "size_t* count);",
                 "int sbm_occ_ot_load(sbm_occ_map* map, const void* bytes, size_t n, int sync);",
                 "int sbm_occ_ot_read(sbm_occ_map* map, const char* path, int sync);"):
        assert decl in flat, decl


def test_struct_layout_and_constants(pkg):
    h = pkg.OccOtHeader
    assert ctypes.sizeof(h) == 8 + 4 * 8 + 17 * 8 + 2 * 4 + 2 * 3 * 2 + 4 == 200
    assert (h.resolution.offset, h.size.offset, h.nodes.offset, h.leaves.offset, h.voxels.offset, h.leaves_at.offset, h.value_min.offset,
            h.value_max.offset, h.key_min.offset, h.key_max.offset) == (0, 8, 16, 24, 32, 40, 176, 180, 184, 190)
    text = (ROOT / "include" / "sbm.h").read_text()
    part = text[text.index("typedef struct sbm_occ_ot_header {"):text.index("} sbm_occ_ot_header;")]
    fields = re.findall(r"^\s+(\w+ [\w\[\], ]+);", part, re.M)
    assert fields == ["double resolution", "uint64_t size", "uint64_t nodes", "uint64_t leaves", "uint64_t voxels", "uint64_t leaves_at[17]",
                      "float value_min", "float value_max", "uint16_t key_min[3]", "uint16_t key_max[3]", "uint32_t pad"]
    from importlib import import_module
    abi = import_module(pkg.__name__ + "._abi")
    assert int(re.search(r"#define SBM_OCC_OT_FAN (\d+)", text).group(1)) == abi.OCC_OT_FAN == oc.FAN
    assert int(re.search(r"#define SBM_OCC_OT_SCAN_TILE (\d+)", text).group(1)) == abi.OCC_OT_SCAN_TILE == oc.SCAN_TILE
    assert (oc.OK, oc.NULL, oc.SIZE, oc.UNSUPPORTED, oc.OCC_FULL) == (0, -1, -2, -23, pkg.ERR_OCC_FULL)


def test_null_arguments_come_first(pkg):
    L = pkg.load_library()
    b = np.frombuffer(GOOD, np.uint8)
    k, d, v = np.zeros(4, np.uint64), np.zeros(4, np.int32), np.zeros(4, np.float32)
    n = ctypes.c_size_t(7)
    h = pkg.OccOtHeader()
    assert L.sbm_occ_ot_info(b.ctypes.data, len(b), None) == oc.NULL
    assert L.sbm_occ_ot_info(None, len(b), ctypes.byref(h)) == oc.NULL
    assert L.sbm_occ_ot_info(None, 0, ctypes.byref(h)) == oc.UNSUPPORTED          # an empty stream is no .ot
    assert L.sbm_occ_ot_leaves(b.ctypes.data, len(b), k.ctypes.data, d.ctypes.data, v.ctypes.data, 4, None) == oc.NULL
    assert L.sbm_occ_ot_leaves(None, len(b), k.ctypes.data, d.ctypes.data, v.ctypes.data, 4, ctypes.byref(n)) == oc.NULL
    for hole in range(3):
        args = [k.ctypes.data, d.ctypes.data, v.ctypes.data]
        args[hole] = None
        assert L.sbm_occ_ot_leaves(b.ctypes.data, len(b), *args, 4, ctypes.byref(n)) == oc.NULL
    assert L.sbm_occ_ot_load(None, b.ctypes.data, len(b), 1) == oc.NULL
    assert L.sbm_occ_ot_load(None, None, 0, 1) == oc.NULL
    assert L.sbm_occ_ot_read(None, b"/nonexistent/x.ot", 1) == oc.NULL             # before the file is looked for
    assert L.sbm_occ_ot_read(None, None, 0) == oc.NULL
    assert L.sbm_occ_ot_body_device(None, None, 0, ctypes.byref(n)) == oc.NULL
    assert L.sbm_occ_ot_write(None, b"/nonexistent/x.ot") == oc.NULL
    assert n.value == 7 and not k.any() and not d.any() and not v.any()            # no refused call wrote through a pointer


def test_leaves_capacity(pkg):
    L = pkg.load_library()
    b = np.frombuffer(GOOD, np.uint8)
    want = oc.leaf_arrays(oc.parse(GOOD))
    count = len(want[0])
    k, d, v = np.zeros(count, np.uint64), np.zeros(count, np.int32), np.zeros(count, np.float32)
    n = ctypes.c_size_t(0)
    assert L.sbm_occ_ot_leaves(b.ctypes.data, len(b), k.ctypes.data, d.ctypes.data, v.ctypes.data, count - 1, ctypes.byref(n)) == oc.SIZE
    assert n.value == count and not k.any() and not d.any() and not v.any()        # the count, and nothing written
    assert L.sbm_occ_ot_leaves(b.ctypes.data, len(b), k.ctypes.data, d.ctypes.data, v.ctypes.data, count, ctypes.byref(n)) == oc.OK
    assert np.array_equal(k, want[0]) and np.array_equal(d, want[1]) and np.array_equal(v.view(np.uint32), want[2])


def centre_to_first(keys, depths):
    """octomap's centre keys -> the packed key of each cube's lowest voxel"""
    keys, out = np.asarray(keys, np.uint64), np.zeros(len(keys), np.uint64)
    for shift in (32, 16, 0):
        k = (keys >> np.uint64(shift)) & np.uint64(0xFFFF)
        level = (16 - np.asarray(depths)).astype(np.uint64)
        out |= ((k >> level) << level) << np.uint64(shift)
    return out


def recorded(tag):
    """(stream, octomap's size, calcNumNodes, leaf keys, depths, value bits) of a per-scan or hand-built stream"""
    if isinstance(tag, tuple):
        n, s = tag
        return (bytes(FX[f"{n}_ot_{s}"]), int(FX[f"{n}_size_{s}"]), int(FX[f"{n}_num_nodes_{s}"]), FX[f"{n}_leaf_key_{s}"],
                FX[f"{n}_leaf_depth_{s}"], FX[f"{n}_leaf_value_{s}"].view(np.uint32))
    return (bytes(FX[f"hand_{tag}"]), int(FX[f"hand_{tag}_size"]), int(FX[f"hand_{tag}_num_nodes"]), FX[f"hand_{tag}_leaf_key"],
            FX[f"hand_{tag}_leaf_depth"], FX[f"hand_{tag}_leaf_value"].view(np.uint32))


@pytest.mark.parametrize("tag", NAMES + ["hand"])
def test_info_and_leaves_against_octomap(pkg, tag):
    """On every recorded stream: the counts, and the leaves octomap's begin_leafs() reported after read()"""
    tags = [(tag, s) for n, s in SCANS if n == tag] if tag != "hand" else [str(n) for n in FX["hand_built"]]
    assert tags
    for t in tags:
        data, size, num_nodes, keys, depth, value = recorded(t)
        i = pkg.occ_ot_info(data)
        assert i["size"] == i["nodes"] == num_nodes and i["leaves"] == len(keys) and i["resolution"] == 0.1, t
        assert i["leaves_at"] == np.bincount(depth, minlength=17).tolist(), t
        assert i["voxels"] == sum(8 ** (16 - int(d)) for d in depth), t
        v = value.view(np.float32)
        assert (np.float32(i["value_min"]), np.float32(i["value_max"])) == (v.min(), v.max()), t
        k, d, got = pkg.occ_ot_leaves(data)
        assert np.array_equal(k, centre_to_first(keys, depth)) and np.array_equal(d, depth) and np.array_equal(got.view(np.uint32), value), t
        first = [np.array([(int(x) >> s) & 0xFFFF for x in k]) for s in (32, 16, 0)]
        assert i["key_min"] == [int(a.min()) for a in first], t
        assert i["key_max"] == [int((a + (1 << (16 - d)) - 1).max()) for a in first], t


@pytest.mark.parametrize("name", sorted(BAD))
def test_malformed_streams(pkg, name):
    """Each with its code, and with what octomap itself answered for it (recorded: 1 an OcTree, 2 another tree, 0 refused)"""
    data, code = BAD[name]
    assert bytes(FX[f"bad_{name}"]) == data and int(FX[f"bad_{name}_code"]) == code
    octomap = {"cut_in_header": 0, "bt_first_line": 0, "res_zero": 0, "color_id": 2}      # it reads everything else
    assert int(FX[f"bad_{name}_octomap"]) == octomap.get(name, 1)
    assert oc.parse(data).status == code
    assert code_of(pkg.occ_ot_info, data) == code and code_of(pkg.occ_ot_leaves, data) == code


def test_every_truncation_of_a_small_stream_is_refused(pkg):
    data = bytes(FX["short_ot_0"])
    body = data.index(b"data\n") + 5
    assert body + 10 <= len(data) <= 400
    for cut in range(len(data)):
        want = oc.UNSUPPORTED if cut < len(oc.MAGIC) else oc.SIZE
        assert code_of(pkg.occ_ot_info, data[:cut]) == want == oc.parse(data[:cut]).status, cut
    assert pkg.occ_ot_info(data + b"trailing bytes are ignored")["nodes"] == pkg.occ_ot_info(data)["nodes"]


def test_header_forms(pkg):
    body = GOOD[GOOD.index(b"data\n") + 5:]
    size = oc.parse(GOOD).size
    forms = {
        b"# Octomap OcTree file, written elsewhere\nres 0.1 size %d\n# a comment\nid OcTree\ndata\n" % size: oc.OK,
        b"# Octomap OcTree file\nid 1\nsize %d\nres 1e-1\nunknown keyword here\ndata\n" % size: oc.OK,
        b"# Octomap OcTree file\nid OcTree\nsize %d\nres -0.1\ndata\n" % size: oc.SIZE,
        b"# Octomap OcTree file\nid OcTree\nsize x%d\nres 0.1\ndata\n" % size: oc.SIZE,
        b"# Octomap OcTree file\nid OcTree\nsize 4294967296\nres 0.1\ndata\n": oc.SIZE,
        b"# Octomap OcTree file\nid OcTree\nsize %d\nres 0.1\n" % size: oc.SIZE,                    # no `data`
        b"# Octomap OcTree file\nsize %d\nres 0.1\ndata\n" % size: oc.UNSUPPORTED,                   # no id
        b"# Octomap OcTree file\nid OcTreeStamped\nsize %d\nres 0.1\ndata\n" % size: oc.UNSUPPORTED,
        b"# Octomap OcTree binary file\nid OcTree\nsize %d\nres 0.1\ndata\n" % size: oc.UNSUPPORTED,    # the .bt header
    }
    for head, code in forms.items():
        assert oc.parse(head + body).status == code, head
        assert code_of(pkg.occ_ot_info, head + body) == code, head
        if code == oc.OK:
            assert pkg.occ_ot_info(head + body)["leaves"] == len(oc.parse(GOOD).leaves)
    assert code_of(pkg.occ_binary_info, GOOD) == oc.UNSUPPORTED          # and the .bt parser refuses an .ot


def test_trees_beyond_any_map_are_counted(pkg):
    """A depth-1 leaf is 2^45 voxels and a childless root 2^48: counted in 64 bits, never expanded"""
    kids = [None] * 8
    kids[3] = oc.leaf(0.5)
    one = pkg.occ_ot_info(oc.of_records((0.5, kids)))
    assert one["voxels"] == 1 << 45 and one["leaves"] == 1 and one["leaves_at"][1] == 1 and one["nodes"] == 2
    assert one["key_min"] == [32768, 32768, 0] and one["key_max"] == [65535, 65535, 32767]
    k, d, v = pkg.occ_ot_leaves(oc.of_records((0.5, kids)))
    assert k.tolist() == [32768 << 32 | 32768 << 16] and d.tolist() == [1] and v.tolist() == [0.5]
    eight = pkg.occ_ot_info(bytes(FX["hand_eight_leaves"]))
    assert eight["voxels"] == 1 << 48 and eight["leaves_at"][1] == 8 and eight["nodes"] == 9
    root = pkg.occ_ot_info(bytes(FX["hand_childless_root"]))
    assert root["voxels"] == 1 << 48 and root["leaves_at"][0] == 1 and root["nodes"] == root["size"] == 1
    assert root["key_min"] == [0, 0, 0] and root["key_max"] == [65535, 65535, 65535]
    assert int(FX["hand_childless_root_num_nodes"]) == 1 and FX["hand_childless_root_leaf_depth"].tolist() == [0]
    empty = pkg.occ_ot_info(oc.stream(0, b""))
    assert empty["voxels"] == empty["leaves"] == empty["nodes"] == 0 and empty["key_min"] == [65535] * 3 and empty["key_max"] == [0] * 3


def test_cpp_adaptor_compiles(tmp_path, pkg):
    _, r = build_callsite(tmp_path, "occupancy_ot_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr


def test_header_states_the_contract():
    text = (ROOT / "include" / "sbm.h").read_text()
    part = text[text.index("occupancy map: the .ot format"):text.index("visual-word dictionary: addNewWords")]
    assert "occupancy map: load a .bt stream" not in part and "occupancy map: queries" not in part
    flat = " ".join(re.sub(r"\n \*", " ", part).split())       # the comment's line breaks are not part of a phrase
    for phrase in ('"occ_load"', '"occ_tree_query"', "# Octomap OcTree file", "readNodesRecurs", "computeChildIdx", "little-endian binary32",
                   "in depth-first pre-order", "A leaf of the pruned tree writes mask 0", "an empty tree writes `size 0` and no body",
                   "Bytes after record `size` are ignored", "is not kept", "stored as it is", "only for values inside the clamp interval",
                   "exactly as it was", "SBM_ERR_OCC_FULL", "size 0 leaves an empty map with no mode", "a record at depth 16 has a child bit",
                   "the largest j < i with D[j] <= D[i]", "SBM_OCC_OT_HOST_PARSE", "whole dwords", "no atomics",
                   "a bound that does not depend on the stream", "never compares `size`"):
        assert phrase in flat, phrase
    assert "SBM_OCC_OT_HOST_PARSE" in text[:text.index("#ifndef SBM_H_")]      # listed with the other variables
    for old in ("bounding-box iterators, the .ot format,", "Not provided: the .ot format"):
        assert old not in text
