#!/usr/bin/env python3
"""Times the occupancy map's read side for planners and writes profiles/occupancy_planner_bench_synth.json.

    python tools/bench_occupancy_planner.py [--repeat 3]

The map is that of the first four synthetic key frames of tools/bench_occupancy_rays.py at max_range 25, its tree built once
under the log-odds reading. Each figure is host wall ms around the call and a synchronisation, the median of --repeat after one
untimed run:

  leaves_bbx         a 64^3-voxel key box around the last pose (sbm_occ_bbx_leaves_device), against leaves(0) of the whole tree
  unknown_16 / _14   a 128^3-voxel box around the last pose at depth 16 and at depth 14 (sbm_occ_unknown_device)
  metric             the metric bounds on a tree built again before every call, so that no call answers from the cache
  ray_intersections  2^20 ray entries (sbm_occ_ray_intersections_device): the rays of a 640 x 480 cast_view from the last pose,
                     their end points as centres, repeated to 2^20

Beside each goes octomap's own loop for the same work from tests/golden/occupancy_planner_cpu.json: a figure ACROSS TWO MACHINES
(one thread, the flags of tools/octomap_kit.py, on the CPU of the machine that made the fixture; its rays are the fixture's
recorded cases repeated, not the view's).
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

PLANES, MAX_RANGE, CAPACITY = 4, 25.0, 1 << 22
BOX, UNKNOWN, RAYS = 64, 128, 1 << 20
VIEW_W, VIEW_H = 640, 480


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_planner_bench_synth.json"))
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
    params = pkg.occ_ray_params(max_range=MAX_RANGE)
    cpu = json.loads((ROOT / "tests" / "golden" / "occupancy_planner_cpu.json").read_text())
    note = "octomap_cpu_ms is a figure across two machines: " + cpu["what"] + ", " + cpu["build"]
    results = []

    def emit(**row):
        results.append(row)
        print(json.dumps(row), flush=True)

    def clock(run, before=None):
        wall = []
        for _ in range(args.repeat + 1):          # the first run allocates the scratch
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(wall[1:])), wall[1:]

    omap = pkg.OccupancyMap(bm, CAPACITY)
    omap.insert_rays(torch.from_numpy(planes).to("cuda:0"), m, poses, rays.SCALE, params=params)
    tree = omap.tree(pkg.OCC_TREE_LOGODDS)
    info = tree.info()
    origin = np.asarray(poses[-1], np.float32).reshape(12)[[3, 7, 11]]
    key = np.floor(origin.astype(np.float64) * 10.0).astype(np.int64) + 32768
    lo, hi = key - BOX // 2, key + BOX // 2 - 1
    assert [int(v) for v in list(lo) + list(hi)] == cpu["bbx_keys"], "the box octomap was timed on"
    centre = ((key - 32768 + 0.5) * 0.1).astype(np.float32)
    half = np.float32(0.1 * UNKNOWN / 2)
    pmin, pmax = centre - half, centre + half
    assert np.array_equal(np.concatenate([pmin, pmax]), np.float32(cpu["unknown_box"])), "the box octomap was timed on"

    out = {}
    ms, every = clock(lambda: out.update(all=tree.leaves_device(0)))
    emit(question="leaves", voxels=info["voxels"], entries=len(out["all"][0]), wall_ms=ms, wall_ms_all=every,
         octomap_cpu_ms=cpu["calls"]["leaves"]["ms"], octomap_entries=cpu["calls"]["leaves"]["count"], note=note)
    ms, every = clock(lambda: out.update(box=tree.leaves_bbx_device(lo, hi)))
    emit(question="leaves_bbx", box_voxels=BOX ** 3, entries=len(out["box"][0]), wall_ms=ms, wall_ms_all=every,
         octomap_cpu_ms=cpu["calls"]["leaves_bbx"]["ms"], octomap_entries=cpu["calls"]["leaves_bbx"]["count"], note=note)
    for depth in (16, 14):
        ms, every = clock(lambda: out.update(unknown=tree.unknown_centers_device(pmin, pmax, depth)))
        emit(question=f"unknown_{depth}", box_voxels=UNKNOWN ** 3, depth=depth, centres=len(out["unknown"]), wall_ms=ms, wall_ms_all=every,
             octomap_cpu_ms=cpu["calls"][f"unknown_{depth}"]["ms"], octomap_centres=cpu["calls"][f"unknown_{depth}"]["count"], note=note)
    ms, every = clock(lambda: out.update(metric=tree.metric_min_max()), before=lambda: tree.build(pkg.OCC_TREE_LOGODDS))
    emit(question="metric", leaves=info["leaves"], min=[float(v) for v in out["metric"][0]], max=[float(v) for v in out["metric"][1]], wall_ms=ms,
         wall_ms_all=every, octomap_cpu_ms=cpu["calls"]["metric"]["ms"], octomap_leaves=cpu["calls"]["metric"]["count"], note=note)
    status, end = omap.cast_view(VIEW_W, VIEW_H, m, poses[-1], 1, max_range=MAX_RANGE)
    hit = torch.isfinite(end).all(dim=2).reshape(-1)
    centres = end.reshape(-1, 3)[hit]
    dirs = centres - torch.from_numpy(origin).to("cuda:0")
    assert len(centres) > 0
    at = torch.arange(RAYS, device="cuda:0") % len(centres)
    centres, dirs = centres[at].contiguous(), dirs[at].contiguous()
    ms, every = clock(lambda: out.update(rays=omap.ray_intersections(origin, dirs, centres, 1e-3, sync=False)))
    emit(question="ray_intersections", rays=RAYS, view_rays_with_an_end=int(hit.sum()), found=int(out["rays"][0].sum()), wall_ms=ms,
         wall_ms_all=every, rays_per_s=RAYS / (ms * 1e-3), octomap_cpu_ms=cpu["calls"]["ray_intersections"]["ms"],
         octomap_rays=cpu["calls"]["ray_intersections"]["count"], note=note)
    tree.close()
    omap.close()
    bm.close()
    path = pathlib.Path(args.out)
    path.write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), results=results), indent=1) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
