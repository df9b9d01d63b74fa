#!/usr/bin/env python3
"""Times the occupancy tree (sbm_occ_tree_build, sbm_occ_tree_leaves_device, sbm_occ_tree_search_device,
sbm_occ_tree_write_binary) on the scene of tools/bench_occupancy_rays.py and writes profiles/occupancy_tree_bench.json.

    python tools/bench_occupancy_tree.py [--repeat 20]

Scene: the first 4 synthetic key frames of bench_occupancy_rays.synth_planes (160 x 120, scale 4, depths of 5 to 17 m) inserted
in log-odds mode at max_range 25, the tree tools/make_occupancy_tree_fixtures.py timed octomap on. Per call, the wall clock
(median of --repeat synchronous calls after one warm-up call) and the device clock (the stage time of sbm_get_profile, median of
--repeat profiled calls):

    build          one snapshot under each reading
    leaves(0)      every leaf of the pruned tree, into device memory
    search         2^20 random points of the scene's box at depth 16 and at depth 12
    .bt            build(MAXLIKELIHOOD) + write_binary through the tree, against the host path for the same map: fetch_logodds +
                   sbm_occ_write_binary_logodds; the two alternate, and both files must be the same bytes. Repeated for maps from
                   the top 15 rows of one key frame to 8 whole key frames, to see where the two paths cross.
    floor          build of a one-voxel map: every level is one small launch, so this is what the launches alone cost

The CPU figures beside them are what the fixture tool recorded for octomap's own updateInnerOccupancy + prune + writeBinary and for
one leaf iteration (one thread, -O1, on the CPU of the machine that made the fixture), from tests/golden/occupancy_tree_cpu.json.
"""
import argparse
import ctypes
import json
import pathlib
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import bench_occupancy_rays as scene  # noqa: E402

PLANES, RANGE = 4, 25.0
SWEEP = ((1, 15), (1, 60), (1, 120), (4, 120), (8, 120))     # (key frames, rows of each) of the maps the .bt paths are timed on
N = 1 << 20
LO, ML = 0, 1


def timed(call, repeat, torch):
    call()
    wall = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall)), wall


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_tree_bench.json"))
    args = ap.parse_args()
    import torch

    import _pkg
    if not torch.cuda.is_available():
        raise SystemExit("bench_occupancy_tree.py needs a GPU")
    pkg = _pkg.load()
    planes, poses = scene.synth_planes(max(n for n, _ in SWEEP))
    ref = scene.synth_model()
    m = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(m), ctypes.byref(ref), ctypes.sizeof(m))
    bm = pkg.StereoBM.create(64, 15, device=0)
    rp = pkg.occ_ray_params(max_range=RANGE)
    d_planes = torch.from_numpy(planes).to("cuda:0")

    def stage(call, tree, name):
        bm.set_profiling(True)
        ms = []
        for _ in range(args.repeat):
            call()
            ms.append(tree.profile()[name])
        bm.set_profiling(False)
        return float(np.median(ms))

    def bt_paths(n_planes, rows, tmp):
        """Both ways to the .bt of a map of the top `rows` rows of n_planes key frames, alternating -> figures"""
        omap = pkg.OccupancyMap(bm, 1 << 23)
        omap.insert_rays(d_planes[:n_planes, :rows].contiguous(), m, poses[:n_planes], scene.SCALE, rp)
        tree = pkg.OccupancyTree(omap)
        a, b = tmp / "tree.bt", tmp / "host.bt"

        def through_tree():
            tree.build(ML, rp).write_binary(a)

        def through_host():
            omap.write_binary_logodds(b, rp)

        through_tree(), through_host()
        assert a.read_bytes() == b.read_bytes(), "the two paths write different files"
        wall = {"tree": [], "host": []}
        for _ in range(args.repeat):
            for name, call in (("tree", through_tree), ("host", through_host)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
        res = dict(planes=n_planes, rows=rows, voxels=int(omap.size()), nodes=tree.info()["nodes"], bt_bytes=a.stat().st_size,
                   tree_wall_ms=float(np.median(wall["tree"])), host_wall_ms=float(np.median(wall["host"])),
                   tree_wall_ms_all=wall["tree"], host_wall_ms_all=wall["host"])
        tree.close()
        omap.close()
        return res

    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        sweep = [bt_paths(n, rows, tmp) for n, rows in SWEEP]
    omap = pkg.OccupancyMap(bm, 1 << 22)
    omap.insert_rays(d_planes[:PLANES], m, poses[:PLANES], scene.SCALE, rp)
    keys, lo = omap.fetch_logodds()
    tree = pkg.OccupancyTree(omap)
    results = {}
    for reading, name in ((ML, "build_maxlikelihood"), (LO, "build_logodds")):
        ms, ms_all = timed(lambda: tree.build(reading, rp), args.repeat, torch)
        results[name] = dict(wall_ms=ms, wall_ms_all=ms_all, stage_ms=stage(lambda: tree.build(reading, rp), tree, "occ_tree_build"))
    info = tree.info()

    def leaves():
        return tree.leaves_device(0)

    ms, ms_all = timed(leaves, args.repeat, torch)
    k, d, v = leaves()
    assert len(k) == info["leaves"]
    # the leaves, expanded by their volume, are the voxels
    assert int((8 ** (16 - d.cpu().numpy().astype(np.int64))).sum()) == len(keys)
    results["leaves"] = dict(entries=len(k), wall_ms=ms, wall_ms_all=ms_all, stage_ms=stage(leaves, tree, "occ_tree_query"),
                             entries_per_s=len(k) / (ms * 1e-3))
    unpacked = np.stack([(keys >> np.uint64(32)) & np.uint64(0xFFFF), (keys >> np.uint64(16)) & np.uint64(0xFFFF), keys & np.uint64(0xFFFF)], 1)
    lo_c, hi_c = (unpacked.min(0).astype(np.float64) - 32768) * 0.1, (unpacked.max(0).astype(np.float64) - 32767) * 0.1
    rng = np.random.default_rng(5)
    pts = rng.uniform(lo_c, hi_c, (N, 3)).astype(np.float32)
    d_p = torch.from_numpy(pts).to("cuda:0")
    pk = np.floor(pts.astype(np.float64) * (1.0 / omap.resolution)).astype(np.int64) + 32768      # every point of the box has a key

    def expected(depth):
        """(found, value bits) per point: the maximum over the voxels below the point's node of that depth, by numpy"""
        sh = 16 - depth
        pack = lambda k3: (k3[:, 0] >> sh) << 32 | (k3[:, 1] >> sh) << 16 | (k3[:, 2] >> sh)   # noqa: E731
        node = pack(unpacked.astype(np.int64))
        order = np.argsort(node, kind="stable")
        uniq, first = np.unique(node[order], return_index=True)
        best = np.maximum.reduceat(lo[order], first)
        at = np.searchsorted(uniq, pack(pk)).clip(0, len(uniq) - 1)
        found = uniq[at] == pack(pk)
        return found, np.where(found, best[at].view(np.uint32), np.uint32(0x7FC00000))

    for depth in (16, 12):
        def search():
            return tree.search(d_p, depth, 0.0)

        ms, ms_all = timed(search, args.repeat, torch)
        got = search()
        found, word = expected(depth)
        assert np.array_equal(got[0].cpu().numpy() > 0, found) and np.array_equal(got[1].cpu().numpy().view(np.uint32), word), depth
        if depth == 16:                                  # and the map's own search
            st, val = omap.search(d_p, 0.0)
            assert bool((st == got[0]).all()) and bool((val == got[1]).all())
        results[f"search_depth{depth}"] = dict(points=N, wall_ms=ms, wall_ms_all=ms_all, stage_ms=stage(search, tree, "occ_tree_query"),
                                               points_per_s=N / (ms * 1e-3), states=np.bincount(got[0].cpu().numpy() + 1, minlength=4).tolist())
    ms, ms_all = timed(lambda: omap.search(d_p, 0.0), args.repeat, torch)
    results["map_search_for_comparison"] = dict(points=N, wall_ms=ms, wall_ms_all=ms_all)
    one = pkg.OccupancyMap(bm, 1 << 10)
    one.insert_cloud(np.float32([[0.05, 0.05, 0.05]]), np.float32([1e6, 1e6, 1e6]))
    floor = pkg.OccupancyTree(one)
    ms, ms_all = timed(lambda: floor.build(LO), args.repeat, torch)
    results["floor_one_voxel_build"] = dict(wall_ms=ms, wall_ms_all=ms_all, stage_ms=stage(lambda: floor.build(LO), floor, "occ_tree_build"))
    floor.close()
    one.close()
    cpu = json.loads((ROOT / "tests" / "golden" / "occupancy_tree_cpu.json").read_text())
    doc = dict(device=torch.cuda.get_device_name(0), planes=PLANES, insert_max_range=RANGE, voxels=int(omap.size()),
               overflow=int(omap.overflow()), nodes=info["nodes"], leaves=info["leaves"], nodes_at=info["nodes_at"], repeat=args.repeat,
               results=results, bt_paths=sweep, octomap_cpu=cpu)
    tree.close()
    omap.close()
    bm.close()
    pathlib.Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    brief = {k: {q: w for q, w in r.items() if not q.endswith("_all")} for k, r in results.items()}
    print(json.dumps(dict(results=brief, bt_paths=[{q: w for q, w in s.items() if not q.endswith("_all")} for s in sweep], octomap_cpu=cpu)))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
