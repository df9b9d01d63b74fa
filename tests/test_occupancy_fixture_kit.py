"""tools/octomap_kit.py without reference, compiler or GPU: what its writers put on the wire its Reader takes off again, its
.npz writer is deterministic and keeps dtype and shape, and every committed occupancy .sha256 belongs to its .npz."""
import hashlib
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import octomap_kit as kit  # noqa: E402


@pytest.mark.parametrize("npoints", [0, 3])
def test_scan_round_trip(npoints):
    origin = np.float32([0.3, -0.2, 3276.75])
    pts = (np.arange(3 * npoints, dtype=np.float32) * np.float32(0.37) - 1).reshape(npoints, 3)
    r = kit.Reader(kit.head() + kit.scans([(origin, -1.0, pts), (origin, 25.0, pts[:1])]) + kit.points(pts))
    assert r.take("<f8", 5).tolist() == kit.DEFAULT_PROBS and r.one("<f8") == kit.RESOLUTION
    assert r.one("<i4") == 2
    for max_range, p in ((-1.0, pts), (25.0, pts[:1])):
        assert np.array_equal(r.take("<f4", 3), origin) and r.one("<f8") == max_range
        n = r.one("<i4")
        assert n == len(p) and np.array_equal(r.take("<f4", 3 * n).reshape(n, 3), p)
    n = r.one("<i4")
    assert n == npoints and np.array_equal(r.take("<f4", 3 * n).reshape(n, 3), pts)
    r.done()


def test_node_and_key_lists_round_trip():
    keys = np.array([[0, 65535, 7], [65535, 0, 65535], [32768, 32768, 32768]], np.uint16)
    depth, value = np.array([0, 16, 9]), np.float32([-2.0, 3.5, np.nan])
    packed = (keys[:, 0].astype(np.uint64) << np.uint64(32)) | (keys[:, 1].astype(np.uint64) << np.uint64(16)) | keys[:, 2].astype(np.uint64)
    nodes = np.zeros(3, kit.NODE)
    nodes["k"], nodes["depth"], nodes["value"] = keys, depth, value
    wire = kit.hits(packed, [1, 2, 70000]) + kit.hits(packed[:1]) + 2 * (np.uint32(3).tobytes() + nodes.tobytes())
    r = kit.Reader(wire)
    assert r.one("<i4") == 3 and np.array_equal(r.take("<u2", 9).reshape(3, 3), keys) and r.take("<u4", 3).tolist() == [1, 2, 70000]
    assert r.one("<i4") == 1 and np.array_equal(r.take("<u2", 3), keys[0]) and r.take("<u4", 1).tolist() == [1]
    for depth_type in (np.uint8, np.int32):
        k, d, v = r.leaves(depth_type)
        assert k.dtype == np.uint64 and d.dtype == depth_type and v.dtype == np.float32
        assert np.array_equal(k, packed) and np.array_equal(d, depth) and np.array_equal(kit.bits(v), kit.bits(value))
    r.done()


def test_voxels_and_search_records():
    keys = np.array([[5, 0, 0], [0, 65535, 1], [0, 0, 2]], np.uint16)
    values = np.float32([1.0, 2.0, 3.0])
    found = np.array([(1, 0x3F800000, 16), (0, 0, -1)], kit.FOUND_VALUE_DEPTH)
    r = kit.Reader(keys.tobytes() + values.tobytes() + found.tobytes() + np.array([(1, 0x3F800000), (0, 0)], kit.FOUND_VALUE).tobytes())
    k, v = r.voxels(3)
    assert k.tolist() == [2, (65535 << 16) | 1, 5 << 32] and v.tolist() == [3.0, 2.0, 1.0]
    rec = r.take(kit.FOUND_VALUE_DEPTH, 2)
    assert rec["found"].tolist() == [1, 0] and rec["value"].tolist() == [0x3F800000, 0] and rec["depth"].tolist() == [16, -1]
    rec = r.take(kit.FOUND_VALUE, 2)
    assert rec["found"].tolist() == [1, 0] and rec["value"].tolist() == [0x3F800000, 0]
    r.done()


@pytest.mark.parametrize("data", [b"", b"# Octomap OcTree binary file\n\x00\xff"])
def test_stream_round_trip(data):
    r = kit.Reader(kit.stream(data) + kit.ints(-1, 0x7FFFFFFF))
    s = r.stream()
    assert s.dtype == np.uint8 and s.tobytes() == data
    assert r.take("<i4", 2).tolist() == [-1, 0x7FFFFFFF]
    r.done()
    with pytest.raises(AssertionError):
        kit.Reader(kit.stream(data) + b"\0").done()


def test_write_npz_is_deterministic_and_keeps_dtype_and_shape(tmp_path):
    arrays = dict(scalar=np.float64(0.1), count=np.uint32(7), empty=np.zeros((0, 3), np.float32), names=np.array(["box", "scene"]),
                  keys=np.arange(5, dtype=np.uint64) << np.uint64(40), value=np.float32([[np.nan, -0.0], [1.5, np.inf]]))
    kit.write_npz(tmp_path / "a.npz", arrays)
    kit.write_npz(tmp_path / "b.npz", dict(arrays))
    assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()
    back = np.load(tmp_path / "a.npz")
    assert list(back.files) == list(arrays)
    for k, v in arrays.items():
        v = np.asarray(v)
        assert back[k].dtype == v.dtype and back[k].shape == v.shape and back[k].tobytes() == v.tobytes(), k
    assert back["scalar"].shape == () and back["empty"].shape == (0, 3)
    kit.write_sha256(tmp_path / "a.npz")
    assert (tmp_path / "a.sha256").read_text() == hashlib.sha256((tmp_path / "a.npz").read_bytes()).hexdigest() + "  a.npz\n"


def test_small_arithmetic():
    assert kit.up(0.1) > np.float32(0.1) > kit.down(0.1) and kit.up(0.1).dtype == np.float32
    assert kit.voxel(0) == 0.05 and kit.voxel((3, -2), np.float32).dtype == np.float32
    assert np.array_equal(kit.centres([[32768, 0, 65535]]), np.float32([[0.05, -3276.75, 3276.75]]))
    assert list(kit.FIXTURES) == ["octomap", "rays", "query", "tree", "load", "ot"]
    with pytest.raises(AssertionError):
        kit.load("tree", "query")


@pytest.mark.parametrize("name", list(kit.FIXTURES))
def test_committed_sha256_matches_its_npz(name):
    digest, file = (kit.GOLDEN / f"occupancy_{name}.sha256").read_text().split()
    assert file == f"occupancy_{name}.npz" and hashlib.sha256((kit.GOLDEN / file).read_bytes()).hexdigest() == digest
