#!/usr/bin/env python3
"""Times the occupancy map's edits (sbm_occ_edit_device, sbm_occ_delete_box) and writes profiles/occupancy_edit_bench_synth.json.

    python tools/bench_occupancy_edit.py [--repeat 3]

The map is that of the first four synthetic key frames of tools/bench_occupancy_rays.py at max_range 25. Two questions:

  update     2^20 updateNode items (ops NULL, keys and values in device memory) three ways -- all_distinct: every item its own
             voxel, a 128 x 128 x 64 block of keys in a seeded order; sixteen_per_voxel: a 64 x 64 x 16 block, every voxel sixteen
             times; sixty_four_voxels: all items on a 4 x 4 x 4 block. Wall ms (median of --repeat, each on a fresh copy of the
             map), the two stage times from a profiled run (occ_rays_mark: CLAIM; occ_rays_apply: ORDER and APPLY), and beside them
             octomap's own CPU time for the same calls from tests/golden/occupancy_edit_cpu.json: a figure ACROSS TWO MACHINES
             (one thread, the flags of tools/octomap_kit.py, on the CPU of the machine that made the fixture).
  box_delete sbm_occ_delete_box of half that map (every voxel with y key below 32768) against sbm_occ_reserve moving the same map
             into a table twice as large in the same run: the growth's move is the yardstick. The ratio, and what the mark pass and
             the counter read add. The map's removal mask and counts are allocated by an empty-box delete before the clock starts, as
             they are from a mapper's second window on.
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "oracle"))

ITEMS = 1 << 20
BATCHES = {"all_distinct": (128, 128, 64), "sixteen_per_voxel": (64, 64, 16), "sixty_four_voxels": (4, 4, 4)}
PLANES, MAX_RANGE, CAPACITY = 4, 25.0, 1 << 22


def batch(name, seed=5):
    """-> (packed keys uint64, float32 updates) of ITEMS items: the block's voxels, each ITEMS / voxels times, in a seeded order; the
    updates are octomap's hit and miss log-odds, two hits to one miss"""
    nx, ny, nz = BATCHES[name]
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    keys = ((32768 + 20 + i).astype(np.uint64) << np.uint64(32) | (32768 - ny // 2 + j).astype(np.uint64) << np.uint64(16) |
            (32768 - nz // 4 + k).astype(np.uint64)).reshape(-1)
    rng = np.random.default_rng(seed)
    keys = np.repeat(keys, ITEMS // len(keys))[rng.permutation(ITEMS)]
    hit, miss = np.float32(np.log(0.7 / 0.3)), np.float32(np.log(0.4 / 0.6))
    return keys, np.where(rng.random(ITEMS) < 2 / 3, hit, miss).astype(np.float32)


def half_box():
    """-> (min key, max key) of the box delete"""
    return (0, 0, 0), (65535, 32767, 65535)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_edit_bench_synth.json"))
    args = ap.parse_args()

    import ctypes

    import torch

    import _pkg
    import bench_occupancy_rays as rays

    pkg = _pkg.load()
    bm = pkg.StereoBM.create(64, 15, device=0)
    ref = rays.synth_model()
    m = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(m), ctypes.byref(ref), ctypes.sizeof(m))
    planes, poses = rays.synth_planes(PLANES)
    d_planes = torch.from_numpy(planes).to("cuda:0")
    params = pkg.occ_ray_params(max_range=MAX_RANGE)
    cpu = json.loads((ROOT / "tests" / "golden" / "occupancy_edit_cpu.json").read_text())
    results = []

    def emit(**row):
        results.append(row)
        print(json.dumps(row), flush=True)

    def fresh(capacity=CAPACITY):
        omap = pkg.OccupancyMap(bm, capacity)
        omap.insert_rays(d_planes, m, poses, rays.SCALE, params=params)
        return omap

    def clock(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name in BATCHES:
        keys, values = batch(name)
        d_keys, d_values = torch.from_numpy(keys.view(np.int64)).to("cuda:0"), torch.from_numpy(values).to("cuda:0")
        wall, info, voxels = [], None, 0
        for r in range(args.repeat + 1):          # the first run allocates the scratch
            omap = fresh()
            before = omap.size()
            wall.append(clock(lambda: omap.update_nodes(d_keys, d_values, params=params, sync=False)))
            info, voxels = omap.last_edit(), omap.size()
            assert omap.overflow() == 0 and voxels == before + info["created"]
            omap.close()
        bm.set_profiling(True)
        omap = fresh()
        omap.update_nodes(d_keys, d_values, params=params)
        stages = omap.profile()
        bm.set_profiling(False)
        omap.close()
        ms = float(np.median(wall[1:]))
        emit(question="update", batch=name, items=ITEMS, voxels_named=int(np.prod(BATCHES[name])), created=info["created"], voxels=int(voxels),
             wall_ms=ms, wall_ms_all=wall[1:], items_per_s=ITEMS / (ms * 1e-3), claim_ms=stages["occ_rays_mark"],
             order_apply_ms=stages["occ_rays_apply"], octomap_cpu_ms=cpu["calls"][name]["ms"],
             note="octomap_cpu_ms is a figure across two machines: " + cpu["what"] + ", " + cpu["build"])

    lo, hi = half_box()
    box_ms, move_ms, removed = [], [], 0
    for r in range(args.repeat + 1):
        omap = fresh()
        voxels = omap.size()
        omap.delete_box((1, 0, 0), (0, 0, 0))          # the empty box, outside the clock: the map's mask and counts exist, as in a mapper's second window
        box_ms.append(clock(lambda: omap.delete_box(lo, hi)))
        removed = omap.last_edit()["removed"]
        assert omap.size() == voxels - removed
        omap.close()
        omap = fresh()
        move_ms.append(clock(lambda: omap.reserve(2 * CAPACITY)))
        assert omap.size() == voxels
        omap.close()
    b, g = float(np.median(box_ms[1:])), float(np.median(move_ms[1:]))
    emit(question="box_delete", voxels=int(voxels), removed=int(removed), capacity=CAPACITY, box_delete_ms=b, box_delete_ms_all=box_ms[1:],
         reserve_ms=g, reserve_ms_all=move_ms[1:], ratio_over_reserve=b / g, octomap_cpu_ms=cpu["calls"]["box_delete_half"]["ms"],
         note="box_delete (after an untimed empty-box delete that allocated the map's mask) = one byte per slot cleared, the mark pass, a counter read, then the move into a table of the SAME size; reserve = the "
         "move into a table twice as large, which clears twice the slots; both allocate and free their tables inside the clock")
    bm.close()
    out = pathlib.Path(args.out)
    out.write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), results=results), indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
