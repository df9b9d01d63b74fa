"""The .bt loader's C-ABI without a GPU: declarations against exports, the structure layout against the mirror, whatever the
entry points check before they touch a device (null arguments first), the host parser on malformed streams and on trees far
beyond any map, the C++ adaptor compiling against the library, and what include/sbm.h must say. The checks that need a map are in
tests/test_gpu_occupancy_load.py."""
import ctypes
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_load_cases as lc  # noqa: E402
from gpu_support import build_callsite  # noqa: E402

CALLS = ("sbm_occ_binary_info", "sbm_occ_binary_leaves", "sbm_occ_load_binary", "sbm_occ_read_binary")
FX, STREAMS = lc.fixture()
GOOD = STREAMS["tree_scene"][0]
BAD = lc.malformed(GOOD)


def test_declarations_against_exports(pkg):
    text = (ROOT / "include" / "sbm.h").read_text()
    declared = set(re.findall(r"^(?:int|void) (sbm_occ_\w+)\(", text, re.M))
    assert set(CALLS) <= declared and not any(c.startswith("sbm_occ_tree_") for c in CALLS)
    r = subprocess.run(["nm", "-D", "--defined-only", str(pkg.library_path())], capture_output=True, text=True, check=True)
    exported = {line.split()[-1] for line in r.stdout.splitlines() if " T " in line}
    assert set(CALLS) <= exported
    L = pkg.load_library()
    for name in CALLS:
        assert getattr(L, name).argtypes is not None, name
    flat = " ".join(text.split())
    for decl in ("int sbm_occ_binary_info(const void* bytes, size_t n, sbm_occ_binary_header* out);",
                 "int sbm_occ_binary_leaves(const void* bytes, size_t n, uint64_t* first_key, int32_t* depth, uint8_t* occupied, size_t cap, "
                 "size_t* count);",
                 "int sbm_occ_load_binary(sbm_occ_map* map, const void* bytes, size_t n, const sbm_occ_ray_params* params, int sync);",
                 "int sbm_occ_read_binary(sbm_occ_map* map, const char* path, const sbm_occ_ray_params* params, int sync);"):
        assert decl in flat, decl


def test_struct_layout(pkg):
    h = pkg.OccBinaryHeader
    assert ctypes.sizeof(h) == 8 + 5 * 8 + 17 * 8 + 2 * 3 * 2 + 4 == 200
    assert (h.resolution.offset, h.size.offset, h.nodes.offset, h.leaves.offset, h.occupied.offset, h.voxels.offset, h.leaves_at.offset,
            h.key_min.offset, h.key_max.offset) == (0, 8, 16, 24, 32, 40, 48, 184, 190)
    text = (ROOT / "include" / "sbm.h").read_text()
    part = text[text.index("typedef struct sbm_occ_binary_header {"):text.index("} sbm_occ_binary_header;")]
    fields = re.findall(r"^\s+(\w+ [\w\[\], ]+);", part, re.M)
    assert fields == ["double resolution", "uint64_t size", "uint64_t nodes", "uint64_t leaves", "uint64_t occupied", "uint64_t voxels",
                      "uint64_t leaves_at[17]", "uint16_t key_min[3]", "uint16_t key_max[3]", "uint32_t pad"]
    assert (lc.OK, lc.NULL, lc.SIZE, lc.UNSUPPORTED, lc.OCC_FULL) == (0, -1, -2, -23, pkg.ERR_OCC_FULL)


def test_null_arguments_come_first(pkg):
    L = pkg.load_library()
    rp = pkg.occ_ray_params()
    bad = pkg.occ_ray_params(clamp_min=0.99)       # fails sbm_occ_ray_params_validate
    b = np.frombuffer(GOOD, np.uint8)
    k, d, o = np.zeros(4, np.uint64), np.zeros(4, np.int32), np.zeros(4, np.uint8)
    n = ctypes.c_size_t(7)
    h = pkg.OccBinaryHeader()
    assert L.sbm_occ_binary_info(b.ctypes.data, len(b), None) == lc.NULL
    assert L.sbm_occ_binary_info(None, len(b), ctypes.byref(h)) == lc.NULL
    assert L.sbm_occ_binary_info(None, 0, ctypes.byref(h)) == lc.UNSUPPORTED          # an empty stream is no .bt
    assert L.sbm_occ_binary_leaves(b.ctypes.data, len(b), k.ctypes.data, d.ctypes.data, o.ctypes.data, 4, None) == lc.NULL
    assert L.sbm_occ_binary_leaves(None, len(b), k.ctypes.data, d.ctypes.data, o.ctypes.data, 4, ctypes.byref(n)) == lc.NULL
    for hole in range(3):
        args = [k.ctypes.data, d.ctypes.data, o.ctypes.data]
        args[hole] = None
        assert L.sbm_occ_binary_leaves(b.ctypes.data, len(b), *args, 4, ctypes.byref(n)) == lc.NULL
    assert L.sbm_occ_load_binary(None, b.ctypes.data, len(b), ctypes.byref(rp), 1) == lc.NULL
    assert L.sbm_occ_load_binary(None, b.ctypes.data, len(b), ctypes.byref(bad), 1) == lc.NULL    # before the parameters are looked at
    assert L.sbm_occ_load_binary(None, None, 0, None, 1) == lc.NULL
    assert L.sbm_occ_read_binary(None, b"/nonexistent/x.bt", ctypes.byref(rp), 1) == lc.NULL      # before the file is looked for
    assert L.sbm_occ_read_binary(None, None, None, 0) == lc.NULL
    assert n.value == 7 and not k.any() and not d.any() and not o.any()          # no refused call wrote through a pointer


def test_leaves_capacity(pkg):
    L = pkg.load_library()
    b = np.frombuffer(GOOD, np.uint8)
    want = lc.leaf_arrays(lc.parse(GOOD))
    count = len(want[0])
    k, d, o = np.zeros(count, np.uint64), np.zeros(count, np.int32), np.zeros(count, np.uint8)
    n = ctypes.c_size_t(0)
    assert L.sbm_occ_binary_leaves(b.ctypes.data, len(b), k.ctypes.data, d.ctypes.data, o.ctypes.data, count - 1, ctypes.byref(n)) == lc.SIZE
    assert n.value == count and not k.any() and not d.any() and not o.any()       # the count, and nothing written
    assert L.sbm_occ_binary_leaves(b.ctypes.data, len(b), None, None, None, 0, ctypes.byref(n)) == lc.SIZE and n.value == count
    assert L.sbm_occ_binary_leaves(b.ctypes.data, len(b), k.ctypes.data, d.ctypes.data, o.ctypes.data, count, ctypes.byref(n)) == lc.OK
    assert np.array_equal(k, want[0]) and np.array_equal(d, want[1]) and np.array_equal(o, want[2])


@pytest.mark.parametrize("name", sorted(BAD))
def test_malformed_streams(pkg, name):
    """Each with its code, and with what octomap itself answered for it (recorded, and not always a refusal)"""
    data, code = BAD[name]
    assert bytes(FX[f"bad_{name}"]) == data and int(FX[f"bad_{name}_code"]) == code
    refused_by_octomap = {"cut_in_record", "cut_between_records", "cut_in_header", "size_plus_one", "size_minus_one", "no_data", "res_zero"}
    assert (int(FX[f"bad_{name}_octomap"]) == 0) == (name in refused_by_octomap)
    assert lc.parse(data).status == code
    with pytest.raises(pkg.StereoBMError) as e:
        pkg.occ_binary_info(data)
    assert e.value.code == code
    with pytest.raises(pkg.StereoBMError) as e:
        pkg.occ_binary_leaves(data)
    assert e.value.code == code


def test_every_truncation_of_a_small_stream_is_refused(pkg):
    data = STREAMS["tree_cube63"][0]
    body = data.index(b"data\n") + 5
    for cut in range(len(data)):
        with pytest.raises(pkg.StereoBMError) as e:
            pkg.occ_binary_info(data[:cut])
        want = lc.UNSUPPORTED if cut < len(lc.MAGIC) else lc.SIZE
        assert e.value.code == want == lc.parse(data[:cut]).status, cut
    assert pkg.occ_binary_info(data + b"trailing bytes are ignored")["nodes"] == pkg.occ_binary_info(data)["nodes"]
    assert body < len(data)


def test_header_forms(pkg):
    body = GOOD[GOOD.index(b"data\n") + 5:]
    size = lc.parse(GOOD).size
    forms = {
        b"# Octomap OcTree binary file, written elsewhere\nres 0.1 size %d\n# a comment\nid OcTree\ndata\n" % size: lc.OK,
        b"# Octomap OcTree binary file\nid 1\nsize %d\nres 1e-1\nunknown keyword here\ndata\n" % size: lc.OK,
        b"# Octomap OcTree binary file\nid OcTree\nsize %d\nres -0.1\ndata\n" % size: lc.SIZE,
        b"# Octomap OcTree binary file\nid OcTree\nsize x%d\nres 0.1\ndata\n" % size: lc.SIZE,
        b"# Octomap OcTree binary file\nid OcTree\nsize 4294967296\nres 0.1\ndata\n": lc.SIZE,
        b"# Octomap OcTree binary file\nsize %d\nres 0.1\ndata\n" % size: lc.UNSUPPORTED,
        b"# Octomap OcTree file\nid OcTree\nsize %d\nres 0.1\ndata\n" % size: lc.UNSUPPORTED,          # the .ot header
    }
    for head, code in forms.items():
        assert lc.parse(head + body).status == code, head
        if code == lc.OK:
            assert pkg.occ_binary_info(head + body)["leaves"] == len(lc.parse(GOOD).leaves)
        else:
            with pytest.raises(pkg.StereoBMError) as e:
                pkg.occ_binary_info(head + body)
            assert e.value.code == code, head


def test_trees_beyond_any_map_are_counted(pkg):
    """A depth-1 leaf is 2^45 voxels and a childless root 2^48: counted in 64 bits, never expanded"""
    one = pkg.occ_binary_info(lc.stream(2, bytes((0x80, 0))))          # child 3 of the root: an occupied leaf
    assert one["voxels"] == 1 << 45 and one["leaves"] == one["occupied"] == 1 and one["leaves_at"][1] == 1 and one["nodes"] == 2
    assert one["key_min"] == [32768, 32768, 0] and one["key_max"] == [65535, 65535, 32767]
    k, d, o = pkg.occ_binary_leaves(lc.stream(2, bytes((0x80, 0))))
    assert k.tolist() == [32768 << 32 | 32768 << 16] and d.tolist() == [1] and o.tolist() == [1]
    free = pkg.occ_binary_info(lc.stream(9, bytes((0x55, 0x55))))      # eight free depth-1 leaves
    assert free["voxels"] == 1 << 48 and free["occupied"] == 0 and free["leaves_at"][1] == 8
    root = pkg.occ_binary_info(lc.stream(1, bytes((0, 0))))
    assert root["voxels"] == 1 << 48 and root["leaves_at"][0] == 1 and root["occupied"] == 1 and root["nodes"] == root["size"] == 1
    assert root["key_min"] == [0, 0, 0] and root["key_max"] == [65535, 65535, 65535]
    assert int(FX["size1_ret"]) == 1 and int(FX["size1_num_nodes"]) == 1 and FX["size1_leaf_depth"].tolist() == [0]
    empty = pkg.occ_binary_info(lc.stream(0, b""))
    assert empty["voxels"] == empty["leaves"] == empty["nodes"] == 0 and empty["key_min"] == [65535] * 3 and empty["key_max"] == [0] * 3


def test_cpp_adaptor_compiles(tmp_path, pkg):
    _, r = build_callsite(tmp_path, "occupancy_load_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr


def test_header_states_the_contract():
    text = (ROOT / "include" / "sbm.h").read_text()
    part = text[text.index("occupancy map: load a .bt stream"):text.index("visual-word dictionary: addNewWords")]
    flat = " ".join(re.sub(r"\n \*", " ", part).split())       # the comment's line breaks are not part of a phrase
    for phrase in ('"occ_load"', "# Octomap OcTree binary file", "readBinaryNode", "computeChildIdx", "calcNumNodes() against size",
                   "legacy binary header", "Bytes after the last record are ignored", "6 significant digits", "key set of a loaded map is",
                   "exactly as it was", "SBM_ERR_OCC_FULL", "size 0 leaves an empty map with no mode", "one output voxel per lane",
                   "no spin waits", "a slot has one writer", "depth 17"):
        assert phrase in flat, phrase
