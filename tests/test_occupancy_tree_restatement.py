"""The transcription of the occupancy tree (tests/occupancy_tree_cases.py) against what the reference's own octomap holds above
the voxels (tests/golden/occupancy_tree.npz, written by tools/make_occupancy_tree_fixtures.py) and, independently of that
fixture, against the .bt streams and node counts octomap wrote for the earlier fixtures. No GPU, no library. Everything is
compared for exact equality: integers, orders, float bits and bytes."""
import hashlib
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_ray_cases as rc  # noqa: E402
import occupancy_ref as occ  # noqa: E402
import occupancy_tree_cases as tc  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
FX = dict(np.load(GOLDEN / "occupancy_tree.npz"))
FXQ = dict(np.load(GOLDEN / "occupancy_query.npz"))
FXR = dict(np.load(GOLDEN / "occupancy_rays.npz"))
FXO = dict(np.load(GOLDEN / "occupancy_octomap.npz"))
TREES = [str(t) for t in FX["trees"]]
MAX_DEPTHS = [int(d) for d in FX["max_depths"]]
SEARCH_DEPTHS = [int(d) for d in FX["search_depths"]]
RES = float(FX["resolution"])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def voxels_of(tree):
    src = FX if f"{tree}_keys" in FX else FXQ
    keys = src[f"{tree}_keys"]
    if int(FX[f"{tree}_hits"]):
        return {int(k): 1 for k in keys}, tc.HITS
    return dict(zip((int(k) for k in keys), src[f"{tree}_logodds"])), tc.LOGODDS_MODE


def test_sha256_and_size():
    data = (GOLDEN / "occupancy_tree.npz").read_bytes()
    assert (GOLDEN / "occupancy_tree.sha256").read_text().split()[0] == hashlib.sha256(data).hexdigest()
    assert len(data) < 512 * 1024
    assert (GOLDEN / "occupancy_tree_cpu.json").exists()


def test_fixture_covers_its_cases():
    assert set(TREES) >= {"one", "sib8", "sib8_mixed", "cube64", "cube63", "straddle", "corners", "box", "scene", "scene_hits"} | \
        {f"shift_{k}" for k in range(8)}
    assert MAX_DEPTHS == [0, 15, 14, 12, 8, 1] and SEARCH_DEPTHS == [0, 16, 15, 14, 12, 8, 1]
    assert int(FX["sib8_lo_num_nodes"]) == 16 and int(FX["sib8_mixed_lo_num_nodes"]) == 24 and int(FX["sib8_mixed_ml_num_nodes"]) == 16
    assert FX["cube64_lo_tree_depth"].max() == 14 and int(FX["cube64_lo_num_leaves"]) == 1
    assert int(FX["straddle_lo_num_nodes"]) == 1 + 8 * 16 and FX["straddle_lo_tree_leaf"].sum() == 8
    assert {int(k) for k in FX["corners_keys"]} == {rc.pack3((x, y, z)) for x in (0, 65535) for y in (0, 65535) for z in (0, 65535)}
    for k in range(8):                                        # k lone voxels, then whole sibling groups: every boundary modulo 8
        codes = sorted(rc.morton(int(q)) for q in FX[f"shift_{k}_keys"])
        assert len(codes) == k + 8 * 640 and [c >> 3 for c in codes[:k]] == list(range(k))
        assert all(codes[k + 8 * g + j] == codes[k + 8 * g] + j and codes[k + 8 * g] % 8 == 0 for g in range(0, 640, 37) for j in range(8))
    for tree in ("box", "scene"):                             # free and occupied leaves, and pruned blocks of both kinds
        depth, leaf, value = FX[f"{tree}_lo_tree_depth"], FX[f"{tree}_lo_tree_leaf"] == 1, FX[f"{tree}_lo_tree_value"]
        thres = FX[f"{tree}_constants"][4]
        assert (value[leaf] >= thres).any() and (value[leaf] < thres).any() and (leaf & (depth < 16)).any() and (leaf & (depth == 16)).any()
    assert "scene_hits_lo_num_nodes" not in FX and int(FX["scene_hits_hits"]) == 1
    found = np.concatenate([FX[f"{t}_lo_search_found"].reshape(-1) for t in TREES if f"{t}_lo_search_found" in FX])
    assert found.any() and not found.all()
    d16 = FX["box_lo_search_depth"][SEARCH_DEPTHS.index(16)]              # search at depth 16 ends at a pruned block above it
    assert ((d16 >= 0) & (d16 < 16)).any() and (d16 == 16).any()


@pytest.mark.parametrize("tree", TREES)
def test_the_transcription_reproduces_octomap(tree):
    voxels, mode = voxels_of(tree)
    consts = FX[f"{tree}_constants"]
    pts = FX[f"{tree}_points"]
    for tag in ("lo", "ml"):
        if tag == "lo" and mode == tc.HITS:
            continue
        rec = tc.unpack_stage(FX, tree, tag, MAX_DEPTHS, SEARCH_DEPTHS)
        t = tc.Tree(voxels if tag == "lo" else tc.max_likelihood(voxels, mode, consts), RES)
        keys, depth, value, leaf = t.all_nodes()                                          # begin_tree()
        assert np.array_equal(keys, rec["tree_key"]) and np.array_equal(depth, rec["tree_depth"]) and np.array_equal(leaf, rec["tree_leaf"])
        assert np.array_equal(bits(value), bits(rec["tree_value"]))
        assert t.size == int(rec["num_nodes"]) and t.num_leaves == int(rec["num_leaves"])  # calcNumNodes(), getNumLeafNodes()
        assert t.nodes_at == np.bincount(depth, minlength=17).tolist() and t.leaves_at == np.bincount(depth[leaf == 1], minlength=17).tolist()
        for md in MAX_DEPTHS:                                                              # begin_leafs(maxDepth)
            k, d, v = t.leaves(md)
            assert np.array_equal(k, rec[f"leafs{md}_key"]) and np.array_equal(d, rec[f"leafs{md}_depth"]), (tag, md)
            assert np.array_equal(bits(v), bits(rec[f"leafs{md}_value"])), (tag, md)
        for sd in SEARCH_DEPTHS:                                                           # search(point, depth)
            state, word, found = t.search_all(pts, sd, consts[4])
            hit = rec[f"search{sd}_found"].astype(bool)
            assert np.array_equal(state > 0, hit) and np.array_equal(word[hit], rec[f"search{sd}_value"][hit]), (tag, sd)
            assert (word[~hit] == 0x7FC00000).all() and np.array_equal(found, rec[f"search{sd}_depth"]), (tag, sd)
            assert np.array_equal(state[hit] == tc.CELL_OCCUPIED, word[hit].view(np.float32) >= consts[4])
    assert t.stream(consts[3]) == FX[f"{tree}_bt"].tobytes()                               # writeBinary after toMaxLikelihood


def accepted_keys(bit):
    gate = FXO["norm"] <= float(np.float32(FXO["range_max"]) * np.float32(FXO["range_max"]))
    take = gate & (FXO["ok"] == 1) & ((FXO["group"] >> bit) & 1 == 1)
    return np.unique(occ.pack(FXO["keys"][take]))


@pytest.mark.parametrize("name,bit", [("all", 0), ("blocks", 1), ("empty", 2)])
def test_the_hit_fixture_streams_and_sizes(name, bit):
    """Recorded before this transcription existed: the hit-mode tree of buildOccupancyGridMap."""
    consts = rc.constants(rc.RayParams())
    t = tc.Tree(tc.max_likelihood({int(k): 1 for k in accepted_keys(bit)}, tc.HITS, consts), float(FXO["resolution"]))
    assert t.size == int(FXO[f"size_{name}"]) and t.num_leaves == int(FXO[f"leafs_{name}"])
    assert t.stream(consts[3]) == FXO[f"bt_{name}"].tobytes()


@pytest.mark.parametrize("name", [str(n) for n in FXR["names"]])
def test_the_ray_fixture_streams_and_sizes(name):
    """Recorded before this transcription existed: insertPointCloud trees with free and occupied leaves."""
    n = int(FXR[f"{name}_nleaves"][-1])
    keys, logodds = FXR[f"{name}_keys"][-n:], FXR[f"{name}_logodds"][-n:]
    consts = FXR[f"{name}_constants"]
    t = tc.Tree(tc.max_likelihood(dict(zip((int(k) for k in keys), logodds)), tc.LOGODDS_MODE, consts), float(FXR["resolution"]))
    assert t.size == int(FXR[f"{name}_size"])
    assert t.stream(consts[3]) == FXR[f"{name}_bt"].tobytes()
    assert t.stream(consts[3]) == rc.write_binary(keys, logodds, float(FXR["resolution"]), consts[4])[0]   # the earlier transcription


def test_expanding_the_leaves_gives_back_the_voxels():
    voxels, _ = voxels_of("scene")
    t = tc.Tree(voxels, RES)
    back = t.expanded()
    assert sorted(back) == sorted(voxels) and all(np.float32(back[k]).view(np.uint32) == np.float32(voxels[k]).view(np.uint32) for k in voxels)
    assert tc.Tree({}, RES).size == 0 and tc.Tree({}, RES).leaves()[0].size == 0 and tc.Tree({}, RES).binary(3.5) == b""
    assert tc.Tree({}, RES).stream(3.5) == FXO["bt_empty"].tobytes()
