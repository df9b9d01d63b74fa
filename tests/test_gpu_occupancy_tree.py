"""The GPU occupancy tree (u96-slam_amd/csrc/sbm_occ_tree.hip: occ_tree_*_kernel) against what the reference's own octomap
holds above the voxels (tests/golden/occupancy_tree.npz), against the .bt streams octomap wrote for the earlier fixtures, and,
for shapes the fixtures do not hold, against the transcription tests/occupancy_tree_cases.py, which
tests/test_occupancy_tree_restatement.py pins to the same fixtures. Every map is built through the existing inserts and its
fetched voxels must equal the recorded ones. Everything is compared for exact equality: integers, orders, float bits and bytes."""
import ctypes
import functools
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_ray_cases as rc  # noqa: E402
import occupancy_ref as occ  # noqa: E402
import occupancy_tree_cases as tc  # noqa: E402
from gpu_support import bm, build_callsite, dev, torch_cuda  # noqa: E402,F401

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
FX = dict(np.load(GOLDEN / "occupancy_tree.npz"))
FXQ = dict(np.load(GOLDEN / "occupancy_query.npz"))
FXR = dict(np.load(GOLDEN / "occupancy_rays.npz"))
FXO = dict(np.load(GOLDEN / "occupancy_octomap.npz"))
TREES = [str(t) for t in FX["trees"]]
MAX_DEPTHS = [int(d) for d in FX["max_depths"]]
SEARCH_DEPTHS = [int(d) for d in FX["search_depths"]]
RES = float(FX["resolution"])
FAR = FX["far_origin"]
NULL, SIZE, UNSUPPORTED = -1, -2, -23
NAN_BITS = 0x7FC00000
LO, ML = 0, 1


def host(a):
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a)


def bits(a):
    return np.ascontiguousarray(host(a)).view(np.uint32)


def unpack(keys):
    k = np.asarray(keys, np.uint64)
    return np.stack([(k >> np.uint64(32)) & np.uint64(0xFFFF), (k >> np.uint64(16)) & np.uint64(0xFFFF), k & np.uint64(0xFFFF)], 1).astype(np.int64)


def centres(keys3):
    return ((np.asarray(keys3, np.float64) - 32768 + 0.5) * RES).astype(np.float32)


def gpu_model(pkg, m):
    g = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(g), ctypes.byref(m), ctypes.sizeof(g))
    return g


def is_hits(tree):
    return bool(int(FX[f"{tree}_hits"]))


def voxels_of(tree):
    """(keys, log-odds or None): box, scene and scene_hits are the trees of the query fixture"""
    src = FX if f"{tree}_keys" in FX else FXQ
    return src[f"{tree}_keys"], (None if is_hits(tree) else src[f"{tree}_logodds"])


def scans_of(tree):
    if f"{tree}_npoints" in FXQ:
        n = FXQ[f"{tree}_npoints"]
        ends = np.cumsum(n)
        return [(FXQ[f"{tree}_origins"][i], float(FXQ[f"{tree}_scan_range"][i]), FXQ[f"{tree}_points"][e - k:e])
                for i, (k, e) in enumerate(zip(n, ends))]
    if f"{tree}_scan_keys" in FX:            # several scans from an origin without a key: each point marks its own voxel
        ends = np.cumsum(FX[f"{tree}_scan_n"])
        return [(FAR, -1.0, centres(FX[f"{tree}_scan_keys"][e - k:e])) for k, e in zip(FX[f"{tree}_scan_n"], ends)]
    return [(FAR, -1.0, centres(unpack(FX[f"{tree}_keys"])))]


def lay(pkg, bm, tree, capacity=1 << 14):
    """The tree's map through the existing inserts -> (map, ray params); its fetched voxels equal the recorded ones."""
    omap = pkg.OccupancyMap(bm, capacity)
    rp = pkg.occ_ray_params(*[float(v) for v in FX[f"{tree}_params"]])
    keys, logodds = voxels_of(tree)
    if is_hits(tree):
        omap.insert(dev(FXQ["scene_disp"]), gpu_model(pkg, occ.model_from_array(FXQ["scene_model"])), FXQ["scene_poses"], int(FXQ["scene_scale"]))
        assert np.array_equal(omap.keys()[0], keys)
        return omap, rp
    for i, (o, max_range, p) in enumerate(scans_of(tree)):
        omap.insert_cloud(dev(p) if i % 2 == 0 else p, o, pkg.occ_ray_params(*[float(v) for v in FX[f"{tree}_params"]], max_range=max_range))
    got = omap.fetch_logodds()
    assert np.array_equal(got[0], keys) and np.array_equal(bits(got[1]), bits(logodds))
    assert np.array_equal(pkg.occ_ray_logodds(rp), FX[f"{tree}_constants"])
    return omap, rp


def has_key(points):
    return np.array([rc.key3([np.float32(c) for c in p], 1.0 / RES) is not None for p in points])


def check_leaves(got, want, what):
    k, d, v = (host(a) for a in got)
    assert len(k) == len(want[0]), (what, len(k), len(want[0]))
    assert np.array_equal(k.view(np.uint64), np.asarray(want[0], np.uint64)), (what, "keys")
    assert np.array_equal(d, np.asarray(want[1], np.int32)), (what, "depths")
    assert np.array_equal(bits(v), bits(np.asarray(want[2], np.float32))), (what, "values")


def check_counts(info, nodes_at, leaves_at, keys):
    assert info["nodes_at"] == list(nodes_at) and info["leaves_at"] == list(leaves_at)
    assert info["nodes"] == sum(nodes_at) and info["leaves"] == sum(leaves_at) and info["voxels"] == len(keys)
    k3 = unpack(keys)
    assert info["key_min"] == (k3.min(axis=0).tolist() if len(keys) else [65535] * 3)
    assert info["key_max"] == (k3.max(axis=0).tolist() if len(keys) else [0] * 3)


@pytest.mark.parametrize("tree", TREES)
def test_every_fixture_tree_under_both_readings(pkg, bm, tree, tmp_path):
    omap, rp = lay(pkg, bm, tree)
    t = None
    try:
        thres = float(FX[f"{tree}_constants"][4])
        pts = FX[f"{tree}_points"]
        keyed = has_key(pts)
        for reading, tag in ((LO, "lo"), (ML, "ml")):
            if reading == LO and is_hits(tree):
                continue
            rec = tc.unpack_stage(FX, tree, tag, MAX_DEPTHS, SEARCH_DEPTHS)
            t = omap.tree(reading, rp) if t is None else t.build(reading, rp)
            info = t.info()
            assert info["nodes"] == int(rec["num_nodes"]) and info["leaves"] == int(rec["num_leaves"])          # calcNumNodes, getNumLeafNodes
            check_counts(info, np.bincount(rec["tree_depth"], minlength=17),
                         np.bincount(rec["tree_depth"][rec["tree_leaf"] == 1], minlength=17), voxels_of(tree)[0])
            for md in MAX_DEPTHS:
                want = rec[f"leafs{md}_key"], rec[f"leafs{md}_depth"], rec[f"leafs{md}_value"]
                check_leaves(t.leaves(md), want, (tree, tag, md, "host"))
                check_leaves(t.leaves_device(md), want, (tree, tag, md, "device"))
            for sd in SEARCH_DEPTHS:
                found = rec[f"search{sd}_found"].astype(bool)
                value = np.where(found, rec[f"search{sd}_value"], np.uint32(NAN_BITS)).astype(np.uint32)
                occupied = found & (value.view(np.float32) >= np.float32(thres))
                state = np.where(found, np.where(occupied, pkg.OCC_CELL_OCCUPIED, pkg.OCC_CELL_FREE),
                                 np.where(keyed, pkg.OCC_CELL_UNKNOWN, pkg.OCC_CELL_OUT))
                for got in (t.search(dev(pts), sd, thres), t.search(pts, sd, thres)):
                    assert np.array_equal(host(got[0]), state), (tree, tag, sd, "state")
                    assert np.array_equal(bits(got[1]), value), (tree, tag, sd, "value")
                    assert np.array_equal(host(got[2]), rec[f"search{sd}_depth"]), (tree, tag, sd, "found depth")
        head = (tc.HEADER % (int(rec["num_nodes"]), RES)).encode()
        bt = FX[f"{tree}_bt"].tobytes()
        assert bt.startswith(head)
        assert host(t.binary()).tobytes() == bt[len(head):]
        t.write_binary(tmp_path / "tree.bt")
        assert (tmp_path / "tree.bt").read_bytes() == bt
        if is_hits(tree):                                     # and what the map's own writers write for the fetched voxels
            omap.write_binary(tmp_path / "map.bt")
        else:
            omap.write_binary_logodds(tmp_path / "map.bt", rp)
        assert (tmp_path / "map.bt").read_bytes() == bt
    finally:
        if t is not None:
            t.close()
        omap.close()


def final_leaves(name):
    n = int(FXR[f"{name}_nleaves"][-1])
    return FXR[f"{name}_keys"][-n:], FXR[f"{name}_logodds"][-n:]


@pytest.mark.parametrize("name", [str(n) for n in FXR["names"]])
def test_the_bt_streams_of_the_ray_fixture(pkg, bm, name, tmp_path):
    omap = pkg.OccupancyMap(bm, 1 << 16)
    try:
        rp = pkg.occ_ray_params(*[float(v) for v in FXR[f"{name}_params"]])
        n = FXR[f"{name}_npoints"]
        for i, e in enumerate(np.cumsum(n)):
            omap.insert_cloud(dev(FXR[f"{name}_points"][e - n[i]:e]), FXR[f"{name}_origins"][i], rp)
        keys, lo = omap.fetch_logodds()
        want = final_leaves(name)
        assert np.array_equal(keys, want[0]) and np.array_equal(bits(lo), bits(want[1]))
        t = omap.tree(ML, rp)
        try:
            assert t.info()["nodes"] == int(FXR[f"{name}_size"])
            t.write_binary(tmp_path / "tree.bt")
            omap.write_binary_logodds(tmp_path / "map.bt", rp)
            assert (tmp_path / "tree.bt").read_bytes() == FXR[f"{name}_bt"].tobytes() == (tmp_path / "map.bt").read_bytes()
        finally:
            t.close()
    finally:
        omap.close()


def test_the_bt_streams_of_the_hit_fixture(pkg, bm, tmp_path):
    fx, scale = FXO, int(FXO["scale"])
    omap = pkg.OccupancyMap(bm, 8192, resolution=float(fx["resolution"]), range_max=float(fx["range_max"]))
    blocks = pkg.OccupancyMap(bm, 8192)
    t = b = None
    try:
        m, me = gpu_model(pkg, occ.model_from_array(fx["model"])), gpu_model(pkg, occ.model_from_array(fx["model_edge"]))
        t = omap.tree(ML, pkg.occ_ray_params())                      # nothing inserted yet: the empty tree
        t.write_binary(tmp_path / "empty.bt")
        assert (tmp_path / "empty.bt").read_bytes() == fx["bt_empty"].tobytes() and t.info()["nodes"] == int(fx["size_empty"]) == 0
        omap.insert(dev(fx["scene_disp"]), m, fx["scene_poses"], scale)
        omap.insert(dev(np.tile(fx["edge_disp"][None], (len(fx["edge_poses"]), 1, 1))), m, fx["edge_poses"], scale)
        omap.insert(dev(np.tile(fx["edge_disp"][None], (len(fx["norm_poses"]), 1, 1))), me, fx["norm_poses"], scale)
        t.build(ML, pkg.occ_ray_params())
        assert t.info()["nodes"] == int(fx["size_all"]) and t.info()["leaves"] == int(fx["leafs_all"])
        t.write_binary(tmp_path / "all.bt")
        omap.write_binary(tmp_path / "map.bt")
        assert (tmp_path / "all.bt").read_bytes() == fx["bt_all"].tobytes() == (tmp_path / "map.bt").read_bytes()
        # the blocks alone, laid down as a log-odds map by one scan from an origin without a key
        keys = np.unique(occ.pack(fx["keys"][(fx["group"] >> 1) & 1 == 1]))
        blocks.insert_cloud(dev(centres(unpack(keys))), FAR)
        assert np.array_equal(blocks.fetch_logodds()[0], keys)
        b = blocks.tree(ML)
        assert b.info()["nodes"] == int(fx["size_blocks"]) and b.info()["leaves"] == int(fx["leafs_blocks"])
        b.write_binary(tmp_path / "blocks.bt")
        assert (tmp_path / "blocks.bt").read_bytes() == fx["bt_blocks"].tobytes()
    finally:
        for x in (t, b):
            if x is not None:
                x.close()
        omap.close()
        blocks.close()


@functools.lru_cache(maxsize=None)
def large_keys():
    """About 20 000 voxels: a filled 20 x 20 x 20 block, not aligned to any cube, and a scatter around it; every seventh voxel
    is hit a second time."""
    rng = np.random.default_rng(77)
    g = np.arange(20)
    block = np.stack(np.meshgrid(g + 32761, g + 32775, g + 32749, indexing="ij"), -1).reshape(-1, 3)
    scatter = rng.integers(32700, 32828, (14000, 3))
    keys = np.unique(np.concatenate([block, scatter]), axis=0)
    return keys, keys[::7]


def compare_with_the_transcription(pkg, omap, rp, points):
    keys, lo = omap.fetch_logodds()
    voxels = dict(zip((int(k) for k in keys), lo))
    thres = float(pkg.occ_ray_logodds(rp)[4])
    for reading in (LO, ML):
        values = voxels if reading == LO else tc.max_likelihood(voxels, tc.LOGODDS_MODE, pkg.occ_ray_logodds(rp))
        want = tc.Tree(values, RES)
        t = omap.tree(reading, rp)
        try:
            check_counts(t.info(), want.nodes_at, want.leaves_at, keys)
            k, d, v = t.leaves(0)
            assert d.min() >= 1 and len(k) == want.num_leaves
            cover = {}                                          # every leaf expanded to the voxels of its cube
            for key, depth, value in zip(unpack(k), d, v):
                half = 1 << (16 - depth) >> 1
                lo3 = key - half
                side = np.arange(max(2 * half, 1))
                cube = np.stack(np.meshgrid(lo3[0] + side, lo3[1] + side, lo3[2] + side, indexing="ij"), -1).reshape(-1, 3)
                for c in occ.pack(cube):
                    cover[int(c)] = value
            assert sorted(cover) == sorted(values) and all(np.float32(cover[q]).view(np.uint32) == np.float32(values[q]).view(np.uint32) for q in values)
            for md in (0, 15, 13, 11, 1):
                check_leaves(t.leaves_device(md), want.leaves(md), ("large", reading, md))
            for sd in (16, 14, 9):
                got, ref = t.search(dev(points), sd, thres), want.search_all(points, sd, thres)
                for g, r in zip(got, ref):
                    assert np.array_equal(host(g).view(r.dtype), r), ("large", reading, sd)
            if reading == LO:                                   # depth 16 is the map's own search
                st, val = omap.search(dev(points), thres)
                got = t.search(dev(points), 16, thres)
                assert np.array_equal(host(got[0]), host(st)) and np.array_equal(bits(got[1]), bits(val))
            else:
                assert host(t.binary()).tobytes() == want.binary(pkg.occ_ray_logodds(rp)[3])
        finally:
            t.close()


def test_a_larger_map_agrees_with_its_voxels_the_transcription_and_the_map(pkg, bm):
    rp = pkg.occ_ray_params(max_range=6.0)
    omap = pkg.OccupancyMap(bm, 1 << 14)
    try:                                                        # the three 40 x 30 scene planes as rays
        omap.insert_rays(dev(FXQ["scene_disp"]), gpu_model(pkg, occ.model_from_array(FXQ["scene_model"])), FXQ["scene_poses"],
                         int(FXQ["scene_scale"]), rp)
        compare_with_the_transcription(pkg, omap, rp, FXQ["scene_search_points"])
    finally:
        omap.close()
    keys, twice = large_keys()
    rng = np.random.default_rng(5)
    points = (centres(keys[rng.integers(0, len(keys), 384)]) + rng.uniform(-0.3, 0.3, (384, 3))).astype(np.float32)
    rp = pkg.occ_ray_params()
    omap = pkg.OccupancyMap(bm, 1 << 16)
    try:                                                        # several tiles of the radix sort and of the head scan
        omap.insert_cloud(dev(centres(keys)), FAR, rp)
        omap.insert_cloud(dev(centres(twice)), FAR, rp)
        assert omap.size() == len(keys) > 19000
        compare_with_the_transcription(pkg, omap, rp, points)
    finally:
        omap.close()


def test_an_empty_map_and_a_tree_never_built(pkg, bm, tmp_path):
    omap = pkg.OccupancyMap(bm, 1 << 10)
    never = pkg.OccupancyTree(omap)
    built = omap.tree(ML, pkg.occ_ray_params())
    try:
        pts = FX["box_points"]
        state = np.where(has_key(pts), pkg.OCC_CELL_UNKNOWN, pkg.OCC_CELL_OUT)
        for t in (never, built, pkg.OccupancyTree(omap).build(LO)):
            check_counts(t.info(), [0] * 17, [0] * 17, np.zeros(0, np.uint64))
            for md in (0, 16, 3):
                assert all(len(a) == 0 for a in t.leaves(md)) and all(len(a) == 0 for a in t.leaves_device(md))
            for sd in (0, 16, 1):
                for got in (t.search(dev(pts), sd), t.search(pts, sd)):
                    assert np.array_equal(host(got[0]), state) and (bits(got[1]) == NAN_BITS).all() and (host(got[2]) == -1).all()
            assert len(t.search(pts[:0])[0]) == 0 and len(t.search(dev(pts[:0]))[0]) == 0           # n == 0 launches nothing
        for t, name in ((never, "never.bt"), (built, "built.bt")):
            assert len(t.binary()) == 0
            t.write_binary(tmp_path / name)
            assert (tmp_path / name).read_bytes() == FXO["bt_empty"].tobytes()
    finally:
        never.close()
        built.close()
        omap.close()


def test_a_tree_is_a_snapshot(pkg, bm):
    omap, rp = lay(pkg, bm, "sib8")
    t = omap.tree(LO, rp)
    try:
        before = t.info(), [host(a).copy() for a in t.leaves(0)], host(t.search(dev(FX["sib8_points"]), 0)[1]).copy()
        assert before[0]["nodes"] == 16
        omap.insert_cloud(centres(unpack(FX["sib8_keys"][5:6])), FAR, rp)        # sib8 becomes sib8_mixed
        omap.insert_cloud(centres(np.array([[40000, 100, 65000]])), FAR, rp)
        assert t.info() == before[0]
        assert all(np.array_equal(host(a), b) for a, b in zip(t.leaves(0), before[1]))
        assert np.array_equal(host(t.search(dev(FX["sib8_points"]), 0)[1]), before[2])
        t.build(LO, rp)                                                          # a rebuild is the update
        after = t.info()
        assert after["voxels"] == 9 and after["nodes"] == 24 + 16 and after["leaves"] == 9
        assert after["key_max"] == [40000, int(unpack(FX["sib8_keys"])[:, 1].max()), 65000]
    finally:
        t.close()
        omap.close()


def test_readings_and_argument_checks_in_their_documented_order(pkg, bm, torch_cuda):
    torch = torch_cuda
    L = pkg.load_library()
    hits, rp = lay(pkg, bm, "scene_hits")
    omap, _ = lay(pkg, bm, "sib8")
    t = omap.tree(LO)
    ht = pkg.OccupancyTree(hits)
    try:
        R, bad = ctypes.byref(rp), ctypes.byref(pkg.occ_ray_params(prob_hit=0.2))
        # build: null, then the reading and the parameters, then what is unsupported
        assert L.sbm_occ_tree_build(None, LO, None, 1) == NULL
        assert L.sbm_occ_tree_build(ht._t, ML, None, 1) == NULL
        assert L.sbm_occ_tree_build(ht._t, 2, bad, 1) == SIZE
        assert L.sbm_occ_tree_build(ht._t, LO, bad, 1) == SIZE
        assert L.sbm_occ_tree_build(ht._t, LO, R, 1) == UNSUPPORTED              # a hit-mode map has no log-odds
        assert L.sbm_occ_tree_build(ht._t, LO, None, 1) == UNSUPPORTED
        assert ht.info()["nodes"] == 0                                           # no refused build built anything
        assert L.sbm_occ_tree_build(ht._t, ML, R, 1) == 0 and ht.info()["voxels"] == len(FXQ["scene_hits_keys"])
        # binary needs the maximum-likelihood reading
        n = ctypes.c_size_t()
        a = torch.zeros((8, 3), dtype=torch.float32, device="cuda:0")
        s = torch.zeros((8,), dtype=torch.int32, device="cuda:0")
        k = torch.zeros((64,), dtype=torch.int64, device="cuda:0")
        P, S, K = a.data_ptr(), s.data_ptr(), k.data_ptr()
        assert L.sbm_occ_tree_binary_device(t._t, K, 512, ctypes.byref(n)) == UNSUPPORTED
        assert L.sbm_occ_tree_write_binary(t._t, b"/nonexistent/x.bt") == UNSUPPORTED
        assert L.sbm_occ_tree_binary_device(t._t, K, 512, None) == NULL
        with pytest.raises(pkg.StereoBMError) as e:
            t.binary()
        assert e.value.code == UNSUPPORTED
        # search: null, then the depth and the threshold, then the count and the alignment
        nan = float("nan")
        assert L.sbm_occ_tree_search_device(t._t, 8, None, 17, nan, S, None, None, 1) == NULL
        assert L.sbm_occ_tree_search_device(t._t, 8, P, 17, nan, None, None, None, 1) == NULL
        assert L.sbm_occ_tree_search_device(t._t, (1 << 30) + 1, P + 2, 17, 0.0, S, None, None, 1) == SIZE
        assert L.sbm_occ_tree_search_device(t._t, 8, P, -1, 0.0, S, None, None, 1) == SIZE
        assert L.sbm_occ_tree_search_device(t._t, (1 << 30) + 1, P + 2, 3, nan, S, None, None, 1) == SIZE
        assert L.sbm_occ_tree_search_device(t._t, (1 << 30) + 1, P, 3, 0.0, S, None, None, 1) == UNSUPPORTED
        for ptrs in ((P + 2, S, None, None), (P, S + 1, None, None), (P, S, S + 2, None), (P, S, None, S + 3)):
            assert L.sbm_occ_tree_search_device(t._t, 8, ptrs[0], 16, 0.0, ptrs[1], ptrs[2], ptrs[3], 1) == UNSUPPORTED
        assert L.sbm_occ_tree_search_device(t._t, 0, None, 16, 0.0, None, None, None, 1) == 0
        h = np.zeros((8, 3), np.float32)
        hs = np.zeros(8, np.int32)
        assert L.sbm_occ_tree_search(t._t, 8, None, 17, 0.0, hs.ctypes.data, None, None) == NULL
        assert L.sbm_occ_tree_search(t._t, 8, h.ctypes.data, 17, 0.0, hs.ctypes.data, None, None) == SIZE
        assert L.sbm_occ_tree_search(t._t, (1 << 30) + 1, h.ctypes.data, 0, 0.0, hs.ctypes.data, None, None) == UNSUPPORTED
        # leaves: null, then the depth, then the alignment; a capacity that is too small reports the count
        assert L.sbm_occ_tree_leaves_device(t._t, 17, K, S, None, 8, None) == NULL
        assert L.sbm_occ_tree_leaves_device(t._t, 17, None, S, None, 8, ctypes.byref(n)) == NULL
        assert L.sbm_occ_tree_leaves_device(t._t, 17, K + 4, S, None, 8, ctypes.byref(n)) == SIZE
        assert L.sbm_occ_tree_leaves_device(t._t, 0, K + 4, S, None, 8, ctypes.byref(n)) == UNSUPPORTED
        assert L.sbm_occ_tree_leaves_device(t._t, 0, K, S + 2, None, 8, ctypes.byref(n)) == UNSUPPORTED
        assert L.sbm_occ_tree_leaves_device(t._t, 0, K, S, S + 1, 8, ctypes.byref(n)) == UNSUPPORTED
        assert L.sbm_occ_tree_leaves_device(t._t, 16, None, None, None, 0, ctypes.byref(n)) == SIZE and n.value == 1
        assert L.sbm_occ_tree_leaves(t._t, 16, None, None, None, 0, ctypes.byref(n)) == SIZE and n.value == 1
        assert L.sbm_occ_tree_leaves_device(t._t, 16, K, S, None, 8, ctypes.byref(n)) == 0 and n.value == 1
        assert int(s[0]) == 15 and not bool(s[1:].any()) and not bool(k[1:].any())      # one entry written, nothing beyond
        assert L.sbm_occ_tree_binary_device(ht._t, K, 4, ctypes.byref(n)) == SIZE and n.value == 2 * (ht.info()["nodes"] - ht.info()["leaves"])
        assert not a.cpu().numpy().any()
        with pytest.raises(pkg.StereoBMError) as e:
            t.search(h, 17)
        assert e.value.code == SIZE
    finally:
        t.close()
        ht.close()
        omap.close()
        hits.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wavefront_and_workgroup_edges_of_search(pkg, bm, torch_cuda, n):
    torch = torch_cuda
    omap, rp = lay(pkg, bm, "scene")
    t = omap.tree(LO, rp)
    try:
        thres = float(FX["scene_constants"][4])
        rec = tc.unpack_stage(FX, "scene", "lo", MAX_DEPTHS, SEARCH_DEPTHS)
        pts = FX["scene_points"][:n]
        out = [torch.full((n + 64,), -7, dtype=torch.int32, device="cuda:0") for _ in range(3)]
        p = dev(pts)
        L = pkg.load_library()
        assert L.sbm_occ_tree_search_device(t._t, n, p.data_ptr(), 14, thres, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), 1) == 0
        found = rec["search14_found"][:n].astype(bool)
        assert np.array_equal(host(out[0][:n]) > 0, found)
        assert np.array_equal(bits(out[1][:n])[found], rec["search14_value"][:n][found])
        assert np.array_equal(host(out[2][:n]), rec["search14_depth"][:n])
        assert all(bool((o[n:] == -7).all()) for o in out)                       # nothing beyond n is written
        assert L.sbm_occ_tree_search_device(t._t, n, p.data_ptr(), 14, thres, out[0].data_ptr(), None, None, 1) == 0
    finally:
        t.close()
        omap.close()


def test_the_two_profile_names_fill_and_leave_the_others_alone(pkg):
    eng = pkg.StereoBM.create(64, 21)
    omap = pkg.OccupancyMap(eng, 1 << 14)
    t = None
    try:
        eng.set_profiling(True)
        omap.insert_cloud(dev(centres(unpack(FX["cube63_keys"]))), FAR)
        first = omap.profile()
        t = omap.tree(ML)
        built = t.profile()
        assert built["occ_tree_build"] > 0 and built["occ_tree_query"] == 0
        t.leaves(0)
        asked = t.profile()
        assert asked["occ_tree_query"] > 0 and asked["occ_tree_build"] == built["occ_tree_build"]
        for call in (lambda: t.search(dev(FX["cube63_points"]), 15), lambda: t.binary()):
            call()
            assert t.profile()["occ_tree_query"] > 0
        assert omap.profile() == first                                           # the map's own stages keep their last times
        v = ctypes.c_float()
        for name in ("occ_tree", "occ_tree_buildx", "occ_tree_quer"):
            assert eng._L.sbm_get_profile(eng._h, name.encode(), ctypes.byref(v)) == UNSUPPORTED, name
    finally:
        eng.set_profiling(False)
        if t is not None:
            t.close()
        omap.close()
        eng.close()


def test_cpp_call_site_lists_searches_and_writes_as_octomap(pkg, bm, tmp_path):
    exe, built = build_callsite(tmp_path, "occupancy_tree_callsite_main.cpp")
    assert built.returncode == 0, built.stderr
    cloud = np.concatenate([np.concatenate([np.float32([len(p)]), o, p.reshape(-1)]) for o, _, p in scans_of("scene")]).astype(np.float32)
    cloud.tofile(tmp_path / "cloud.raw")
    pts = np.ascontiguousarray(FX["scene_points"][:32])
    pts.tofile(tmp_path / "points.raw")
    r = subprocess.run([str(exe), str(tmp_path / "cloud.raw"), str(len(cloud)), "6.0", str(1 << 14), "14", str(tmp_path / "points.raw"),
                        str(len(pts)), "12", str(tmp_path / "out.raw"), str(tmp_path / "slam.bt")], capture_output=True, text=True, timeout=120)
    lo = tc.unpack_stage(FX, "scene", "lo", MAX_DEPTHS, SEARCH_DEPTHS)
    ml = tc.unpack_stage(FX, "scene", "ml", MAX_DEPTHS, SEARCH_DEPTHS)
    n = len(lo["leafs14_key"])
    assert r.returncode == 0 and r.stdout.split() == [
        "voxels", str(len(FXQ["scene_keys"])), "size", str(int(lo["num_nodes"])), "leaves", str(int(lo["num_leaves"])), "listed", str(n),
        "bt_size", str(int(ml["num_nodes"])), "bt_leaves", str(int(ml["num_leaves"]))], r.stdout + r.stderr
    assert (tmp_path / "slam.bt").read_bytes() == FX["scene_bt"].tobytes()
    raw = (tmp_path / "out.raw").read_bytes()
    leaves = np.frombuffer(raw, np.dtype([("key", "<u8"), ("depth", "<i4"), ("value", "<u4")]), n)
    assert np.array_equal(leaves["key"], lo["leafs14_key"]) and np.array_equal(leaves["depth"], lo["leafs14_depth"])
    assert np.array_equal(leaves["value"], bits(lo["leafs14_value"]))
    found = np.frombuffer(raw, np.dtype([("state", "<i4"), ("value", "<u4"), ("depth", "<i4")]), len(pts), 16 * n)
    hit = lo["search12_found"][:32].astype(bool)
    assert np.array_equal(found["state"] > 0, hit) and np.array_equal(found["value"][hit], lo["search12_value"][:32][hit])
    assert np.array_equal(found["depth"], lo["search12_depth"][:32])
