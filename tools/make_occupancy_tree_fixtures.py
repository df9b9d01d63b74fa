#!/usr/bin/env python3
"""Writes tests/golden/occupancy_tree.npz (+ .sha256): what the reference's OWN octomap holds above the voxels of a few small
trees -- every node of begin_tree(), begin_leafs(maxDepth) for maxDepth 0, 15, 14, 12, 8 and 1, calcNumNodes() and
getNumLeafNodes(), and search(point, depth) for depths 0, 16, 15, 14, 12, 8 and 1 -- once after updateInnerOccupancy(); prune();
(the LOGODDS reading) and once after toMaxLikelihood(); prune(); (the MAXLIKELIHOOD reading), there with the writeBinary stream.
Beside it, tests/golden/occupancy_tree_cpu.json holds octomap's milliseconds for updateInnerOccupancy + prune + writeBinary to
memory and for one full leaf iteration on the scene of tools/bench_occupancy_rays.py (kept out of the .npz so that the .npz
regenerates to the same bytes).

Run by hand, never by a test:

    python tools/make_occupancy_tree_fixtures.py --reference /path/to/U96-SLAM [--out DIR]

It compiles its driver, tools/octomap_drivers/tree.cpp (this project's text; it calls octomap's API only), against the octomap
sources vendored in the reference tree (tools/octomap_kit.py builds them once, outside the history), and keeps only inputs and
recorded outputs. The generator asserts that the
transcription tests/occupancy_tree_cases.py reproduces every recorded value before it writes the file.

A scan whose origin has no key -- (1e6, 1e6, 1e6) at 0.1 m -- casts no ray, and every point of it still marks its own voxel as
occupied: that is how exact voxel sets are laid down, in octomap and through insert_cloud. Trees (log-odds, insertPointCloud,
unless said otherwise):

    one          a single voxel
    sib8         eight siblings hit once each: they collapse to depth 15
    sib8_mixed   the same eight, one of them hit twice: no collapse under LOGODDS, a collapse under MAXLIKELIHOOD
    cube64       a full depth-14 cube: collapses twice
    cube63       the same cube with one voxel missing
    straddle     the 2 x 2 x 2 voxels around key (32768, 32768, 32768): adjacent, not siblings; eight root children
    corners      the voxels at keys 0 and 65535 on every axis combination
    shift_k      k = 0..7: k lone voxels low in Morton order, then 640 complete sibling groups -- together a sibling-group
                 boundary at every position modulo 8
    box, scene   the scans of the same names in tests/golden/occupancy_query.npz: free leaves and mixed pruned blocks
    scene_hits   the hit-mode scene, recorded after toMaxLikelihood only
"""
import numpy as np

import octomap_kit as kit
from octomap_kit import BENCH_PLANES, BENCH_RANGE, PROBS, RESOLUTION, centres, rc
import occupancy_tree_cases as tc

MAX_DEPTHS = (0, 15, 14, 12, 8, 1)
SEARCH_DEPTHS = (0, 16, 15, 14, 12, 8, 1)
FAR = np.float32([1e6, 1e6, 1e6])           # an origin without a key
SHIFT_GROUPS, SHIFT_FIRST = 640, 1000       # complete sibling groups of a shift tree, and the first one's depth-15 Morton prefix


def unmorton_keys(codes):
    return np.array([tc.unmorton(int(c)) for c in codes], np.int64).reshape(-1, 3)


def key_scans(*key_lists):
    return [(FAR, -1.0, centres(k)) for k in key_lists]


def probe_points(keys, rng):
    """A small search set for a tree laid down from keys: voxel centres, their neighbours, points nowhere near, no key"""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    take = keys[np.unique(np.linspace(0, len(keys) - 1, 24).astype(int))]
    near = np.clip(take + rng.integers(-2, 3, take.shape), 0, 65535)
    far = np.array([[32768, 32768, 32768], [0, 0, 0], [65535, 65535, 65535], [100, 40000, 7], [32767, 32768, 32769]])
    pts = centres(np.concatenate([take, near, far]))
    odd = np.float32([[np.nan, 0, 0], [0, np.inf, 0], [3276.85, 0, 0], [0, 0, -3276.81]])
    return np.concatenate([pts, odd]).astype(np.float32)


def make_trees(q):
    """q: the query fixture"""
    rng = np.random.default_rng(41)
    trees = {}

    def add(name, *key_lists):
        trees[name] = dict(params=rc.RayParams(), scans=key_scans(*key_lists), scan_keys=[np.asarray(k, np.uint16) for k in key_lists],
                           points=probe_points(np.concatenate(key_lists), rng))

    sib = np.array([(32770 + x, 32772 + y, 32774 + z) for z in (0, 1) for y in (0, 1) for x in (0, 1)])
    cube = np.array([(33000 + x, 32500 + y, 32900 + z) for z in range(4) for y in range(4) for x in range(4)])
    add("one", [(32773, 32765, 32775)])
    add("sib8", sib)
    add("sib8_mixed", sib, sib[5:6])
    add("cube64", cube)
    add("cube63", np.delete(cube, 37, axis=0))
    add("straddle", [(32767 + x, 32767 + y, 32767 + z) for z in (0, 1) for y in (0, 1) for x in (0, 1)])
    add("corners", [(x, y, z) for z in (0, 65535) for y in (0, 65535) for x in (0, 65535)])
    groups = unmorton_keys(np.arange(8 * SHIFT_FIRST, 8 * (SHIFT_FIRST + SHIFT_GROUPS)))
    for k in range(8):
        add(f"shift_{k}", np.concatenate([unmorton_keys(8 * np.arange(k)), groups]))
    for name in ("box", "scene"):
        trees[name] = dict(params=rc.RayParams(*[float(v) for v in q[f"{name}_params"]]), scans=kit.scans_of(q, name),
                           points=q[f"{name}_search_points"])
    trees["scene_hits"] = dict(params=rc.RayParams(), hit_keys=q["scene_hits_keys"], hit_counts=q["scene_hits_counts"],
                               points=q["scene_hits_search_points"])
    trees["bench"] = dict(params=rc.RayParams(), timing=True, points=np.zeros((0, 3), np.float32), scans=kit.bench_scans())
    return trees


def take_stage(r, npoints):
    """what the driver's record() wrote -> dict of arrays"""
    out = {}
    out["tree_key"], out["tree_depth"], out["tree_value"] = r.leaves(np.int32)
    out["tree_leaf"] = r.take(np.uint8, len(out["tree_key"])).copy()
    for md in MAX_DEPTHS:
        out[f"leafs{md}_key"], out[f"leafs{md}_depth"], out[f"leafs{md}_value"] = r.leaves(np.int32)
    out["num_nodes"], out["num_leaves"] = (np.uint64(v) for v in r.take("<u8", 2))
    for d in SEARCH_DEPTHS:
        rec = r.take(kit.FOUND_VALUE_DEPTH, npoints)
        out[f"search{d}_found"] = rec["found"].astype(np.uint8)
        out[f"search{d}_value"] = rec["value"].copy()
        out[f"search{d}_depth"] = rec["depth"].astype(np.int8)
    return out


def pack_stage(rec):
    """One reading's records as few arrays: the six leaf lists end to end with their lengths, the seven searches as rows.
    tests/occupancy_tree_cases.py unpack_stage is the inverse."""
    out = {k: rec[k] for k in ("tree_key", "tree_value", "tree_leaf", "num_nodes", "num_leaves")}
    out["tree_depth"] = rec["tree_depth"].astype(np.uint8)
    out["leafs_n"] = np.array([len(rec[f"leafs{md}_key"]) for md in MAX_DEPTHS], np.int32)
    for k, dt in (("key", np.uint64), ("depth", np.uint8), ("value", np.float32)):
        out[f"leafs_{k}"] = np.concatenate([rec[f"leafs{md}_{k}"] for md in MAX_DEPTHS]).astype(dt)
    for k in ("found", "value", "depth"):
        out[f"search_{k}"] = np.stack([rec[f"search{d}_{k}"] for d in SEARCH_DEPTHS])
    return out


def check_stage(name, rec, tree, points, thres):
    """The transcription reproduces everything octomap recorded for one reading"""
    keys, depth, value, leaf = tree.all_nodes()
    same = lambda a, b: np.array_equal(np.asarray(a), np.asarray(b))   # noqa: E731
    assert same(keys, rec["tree_key"]) and same(depth, rec["tree_depth"]) and same(leaf, rec["tree_leaf"]), (name, "begin_tree")
    assert same(value.view(np.uint32), rec["tree_value"].view(np.uint32)), (name, "begin_tree values")
    assert tree.size == int(rec["num_nodes"]) and tree.num_leaves == int(rec["num_leaves"]), (name, "counts")
    for md in MAX_DEPTHS:
        k, d, v = tree.leaves(md)
        assert same(k, rec[f"leafs{md}_key"]) and same(d, rec[f"leafs{md}_depth"]), (name, "begin_leafs", md)
        assert same(v.view(np.uint32), rec[f"leafs{md}_value"].view(np.uint32)), (name, "begin_leafs values", md)
    for sd in SEARCH_DEPTHS:
        state, bits, found = tree.search_all(points, sd, thres)
        hit = rec[f"search{sd}_found"].astype(bool)
        assert same(state > 0, hit), (name, "search found", sd)
        assert same(bits[hit], rec[f"search{sd}_value"][hit]) and same(found, rec[f"search{sd}_depth"]), (name, "search", sd)


def main():
    args = kit.arguments(__doc__)
    q_fixture = kit.load("query", "tree")
    trees = make_trees(q_fixture)

    def write(f):
        f.write(kit.ints(len(trees)))
        for t in trees.values():
            hits = "hit_keys" in t
            f.write(kit.head(t["params"]) + kit.ints(hits, t.get("timing", False)))
            f.write((kit.hits(t["hit_keys"], t["hit_counts"]) if hits else kit.scans(t["scans"])) + kit.points(t["points"]))

    code, raw = kit.run(kit.build(args.reference, "tree"), "tree", write)
    assert code == 0, code
    out = dict(resolution=np.float64(RESOLUTION), trees=np.array([n for n, t in trees.items() if not t.get("timing")]),
               max_depths=np.array(MAX_DEPTHS, np.int32), search_depths=np.array(SEARCH_DEPTHS, np.int32), far_origin=FAR)
    r, report, cpu = kit.Reader(raw), [], {}
    for name, t in trees.items():
        consts = r.take("<f4", 5).copy()
        if t.get("timing"):
            write_ms, iterate_ms = (float(v) for v in r.take("<f8", 2))
            leaves, voxels, nbytes = (int(v) for v in r.take("<u8", 3))
            cpu = dict(scene="tools/bench_occupancy_rays.py synth_planes", planes=BENCH_PLANES, insert_max_range=BENCH_RANGE, voxels=voxels,
                       pruned_leaves=leaves, bt_bytes=nbytes, octomap_inner_prune_write_ms=write_ms, octomap_leaf_iteration_ms=iterate_ms,
                       note="octomap's updateInnerOccupancy + prune + writeBinary to memory from the expanded tree, and one "
                            "begin_leafs() pass over the pruned tree; one thread, -O1, on the CPU of the machine that made the fixture")
            report.append(f"{name}: {voxels} voxels, {write_ms:.1f} ms to the stream, {iterate_ms:.1f} ms per leaf iteration")
            continue
        hits = "hit_keys" in t
        vk, _, vv = r.leaves()
        order = np.argsort(vk)
        vk, vv = vk[order], vv[order]
        if hits:
            voxels = {int(k): int(c) for k, c in zip(t["hit_keys"], t["hit_counts"])}
            assert np.array_equal(vk, np.array(sorted(voxels), np.uint64)), (name, "keys")
        else:
            m = rc.Tree(t["params"], RESOLUTION)
            for o, mr, p in t["scans"]:
                m.rp.max_range = mr
                m.insert(p, o)
            voxels = dict(m.v)
            assert np.array_equal(vk, np.array(sorted(voxels), np.uint64)), (name, "keys")
            assert np.array_equal(vv.view(np.uint32), np.array([voxels[int(k)] for k in vk], np.float32).view(np.uint32)), (name, "values")
            out[f"{name}_logodds"] = vv
        out[f"{name}_keys"] = vk
        out[f"{name}_hits"] = np.int32(hits)
        out[f"{name}_params"] = np.array([getattr(t["params"], k) for k in PROBS], np.float64)
        out[f"{name}_constants"] = consts
        out[f"{name}_points"] = np.asarray(t["points"], np.float32)
        if "scan_keys" in t and len(t["scan_keys"]) > 1:      # a tree of one key-less-origin scan is laid down from its keys
            out[f"{name}_scan_keys"] = np.concatenate(t["scan_keys"]).astype(np.uint16)
            out[f"{name}_scan_n"] = np.array([len(k) for k in t["scan_keys"]], np.int32)
        npts = len(t["points"])
        readings = ([] if hits else [("lo", tc.Tree({k: v for k, v in voxels.items()}, RESOLUTION))]) + \
                   [("ml", tc.Tree(tc.max_likelihood(voxels, tc.HITS if hits else tc.LOGODDS_MODE, consts), RESOLUTION))]
        for tag, tree in readings:
            rec = take_stage(r, npts)
            check_stage((name, tag), rec, tree, t["points"], consts[4])
            back = tc.unpack_stage({f"{name}_{tag}_{k}": v for k, v in pack_stage(rec).items()}, name, tag, MAX_DEPTHS, SEARCH_DEPTHS)
            assert all(np.array_equal(back[k], v) for k, v in rec.items()), (name, tag, "packing")
            for k, v in pack_stage(rec).items():
                out[f"{name}_{tag}_{k}"] = v
        bt = r.stream()
        assert readings[-1][1].stream(consts[3]) == bt.tobytes(), (name, "writeBinary")
        out[f"{name}_bt"] = bt
        ml = readings[-1][1]
        report.append(f"{name}: {len(vk)} voxels, {ml.size} nodes / {ml.num_leaves} leaves after toMaxLikelihood" +
                      ("" if hits else f", {readings[0][1].size} / {readings[0][1].num_leaves} before"))
    r.done()
    assert int(out["sib8_lo_num_nodes"]) == 16 and int(out["sib8_mixed_lo_num_nodes"]) == 24 and int(out["sib8_mixed_ml_num_nodes"]) == 16
    assert int(out["cube64_lo_num_leaves"]) == 1 and out["cube64_lo_tree_depth"].max() == 14
    for name in ("box", "scene"):          # the voxels are those of the query fixture, which the tests build the maps from
        assert np.array_equal(out.pop(f"{name}_keys"), q_fixture[f"{name}_keys"])
        assert np.array_equal(out.pop(f"{name}_logodds").view(np.uint32), q_fixture[f"{name}_logodds"].view(np.uint32))
    assert np.array_equal(out.pop("scene_hits_keys"), q_fixture["scene_hits_keys"])
    assert int(out["straddle_lo_num_nodes"]) == 1 + 8 * 16
    OUT = kit.save(args.out, "tree", out, cpu=cpu)
    print(f"{OUT}: {OUT.stat().st_size} bytes\n  " + "\n  ".join(report))


if __name__ == "__main__":
    main()
