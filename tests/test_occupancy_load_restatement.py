"""The .bt reader's host half without a GPU: sbm_occ_binary_info and sbm_occ_binary_leaves against the transcription
tests/occupancy_load_cases.py, and the transcription against what the reference's own octomap read from the same streams
(tests/golden/occupancy_load.npz, written by tools/make_occupancy_load_fixtures.py)."""
import hashlib
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_load_cases as lc  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402
from occupancy_tree_cases import unmorton  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
FX, STREAMS = lc.fixture()
NAMES = sorted(STREAMS)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_fixture_is_the_committed_one():
    digest, name = (GOLDEN / "occupancy_load.sha256").read_text().split()
    assert name == "occupancy_load.npz" and hashlib.sha256((GOLDEN / name).read_bytes()).hexdigest() == digest
    assert len(STREAMS) == 36 and sum(1 for n in NAMES if n.startswith(("tree_", "rays_", "octomap_"))) == 35


@pytest.mark.parametrize("name", NAMES)
def test_transcription_against_octomap(name):
    data, rp = STREAMS[name]
    p = lc.parse(data)
    assert p.status == lc.OK and int(FX[f"{name}_ret"]) == 1
    assert p.size == p.nodes == int(FX[f"{name}_size"]) == int(FX[f"{name}_num_nodes"])
    keys, depth = lc.centre_leaves(p)
    assert np.array_equal(keys, FX[f"{name}_leaf_key"]) and np.array_equal(depth, FX[f"{name}_leaf_depth"])
    c = rc.constants(rp)
    want = np.where(lc.leaf_arrays(p)[2] > 0, rc.F(c[3]), rc.F(c[2]))
    assert np.array_equal(bits(want), bits(FX[f"{name}_leaf_value"]))


@pytest.mark.parametrize("name", NAMES)
def test_library_against_transcription(pkg, name):
    data, _ = STREAMS[name]
    p = lc.parse(data)
    info = pkg.occ_binary_info(data)
    lo, hi = p.key_bounds()
    assert info == dict(resolution=p.resolution, size=p.size, nodes=p.nodes, leaves=len(p.leaves), occupied=p.occupied, voxels=p.voxels,
                        leaves_at=p.leaves_at, key_min=lo, key_max=hi)
    assert info["resolution"] == 0.1
    got = pkg.occ_binary_leaves(np.frombuffer(data, np.uint8))
    want = lc.leaf_arrays(p)
    assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))


@pytest.mark.parametrize("name", [n for n in NAMES if f"{n}_search_found" in FX and n != "size1"])
def test_search_on_the_expanded_leaves_is_octomaps(name):
    data, rp = STREAMS[name]
    c = rc.constants(rp)
    src = dict(np.load(GOLDEN / "occupancy_tree.npz"))
    points = src[name[len("tree_"):] + "_points"]
    keys, vals = lc.expand(lc.parse(data), c[2], c[3])
    voxels = dict(zip(keys.tolist(), vals))
    for i, pt in enumerate(points):
        key = rc.key3([rc.F(x) for x in pt], 10.0)
        v = voxels.get(rc.pack3(key)) if key is not None else None
        assert bool(FX[f"{name}_search_found"][i]) == (v is not None), i
        assert v is None or FX[f"{name}_search_value"][i] == bits(v), i


@pytest.mark.parametrize("name", [str(s).split(":")[0] for s in FX["post_scan"]])
def test_one_more_scan_on_the_loaded_tree(name):
    """insertPointCloud on what readBinary left: per voxel, the transcription of the inserts on the expanded leaves"""
    data, rp = STREAMS[name]
    index = int(dict(str(s).split(":") for s in FX["post_scan"])[name])
    rays = dict(np.load(GOLDEN / "occupancy_rays.npz"))
    n = rays["scene_npoints"]
    end = int(np.cumsum(n)[index])
    c = rc.constants(rp)
    rp.max_range = float(rays["scene_params"][5])
    t = rc.Tree(rp, 0.1)
    keys, vals = lc.expand(lc.parse(data), c[2], c[3])
    t.v = dict(zip(keys.tolist(), (rc.F(x) for x in vals)))
    t.insert(rays["scene_points"][end - int(n[index]):end], rays["scene_origins"][index])
    wk, wv = t.leaves()
    gk, gv = lc.expand_centres(FX[f"{name}_post_key"], FX[f"{name}_post_depth"], FX[f"{name}_post_value"])
    assert np.array_equal(gk, wk) and np.array_equal(bits(gv), bits(wv))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_round_trip_through_the_writer(pkg, tmp_path, seed):
    """The leaves of write_binary_logodds(keys, values) expand back to keys, with state values >= threshold: random key sets
    with whole sibling groups at depths 15, 14 and 13"""
    rng = np.random.default_rng(seed)
    codes = set(int(c) for c in rng.integers(0, 1 << 48, 300))
    for depth, count in ((15, 6), (14, 3), (13, 2)):
        m = 8 ** (16 - depth)
        for prefix in rng.integers(0, 1 << (3 * depth), count):
            codes.update(range(int(prefix) * m, int(prefix) * m + m))
    codes = np.array(sorted(codes), np.uint64)
    keys = lc._unmorton_array(codes)
    values = rng.choice(np.float32([-2.0, -0.4, 0.0, 0.85, 3.5]), len(keys))
    block = codes >> np.uint64(9)                           # whole depth-13 cubes get one state, so that some of them collapse
    values[(block % np.uint64(2) == 0) & (rng.random(len(keys)) < 0.9)] = np.float32(0.85)
    thres = 0.0
    path = tmp_path / "rt.bt"
    pkg.occ_write_binary_logodds(keys, values, path, 0.1, thres)
    data = path.read_bytes()
    assert data == rc.write_binary(keys, values, 0.1, thres)[0]
    first, depth, occ = pkg.occ_binary_leaves(data)
    assert (depth < 16).any() and pkg.occ_binary_info(data)["voxels"] == len(keys)
    first_codes = [rc.morton(int(k)) for k in first]
    got_keys, got_state = lc.expand_leaves(first_codes, depth, occ.astype(np.float32))
    order = np.argsort(keys)
    assert np.array_equal(got_keys, keys[order])
    assert np.array_equal(got_state > 0, values[order] >= np.float32(thres))
    assert all(unmorton(c)[a] == (int(k) >> s & 0xFFFF) for c, k in zip(first_codes[:5], first[:5]) for a, s in ((0, 32), (1, 16), (2, 0)))
