#!/usr/bin/env python3
"""Times the occupancy map's time stamps and writes profiles/occupancy_stamped_bench_synth.json.

    python tools/bench_occupancy_stamped.py [--repeat 3]

The scans are the first four synthetic key frames of tools/bench_occupancy_rays.py at max_range 25, as a cloud each. Three questions:

  scan     the four scans into a stamped map and into a map without stamps, ALTERNATING in one job (--repeat rounds of one after
           the other, each into a fresh map, the clock set before every scan): wall ms of the four inserts (median over the rounds)
           and the two stage times of a profiled round ("occ_rays_mark", "occ_rays_apply"). The stamped scan's cost over the plain
           one is their ratio.
  tree     the build of a LOGODDS tree over the stamped map of those scans (the stamped pruned tree: one stamp look-up per voxel, the
           stamp test and one store per node in the sixteen level launches) against the build over the same scans without stamps.
  forget   degrade_outdated and forget_older_than over the stamped map of those scans, with thresholds that degrade the voxels of
           the first three frames and forget those of the first two: wall ms on a fresh map per round.

Beside them octomap's own CPU times for the same work from tests/golden/occupancy_stamped_cpu.json: figures ACROSS TWO MACHINES
(one thread, the flags of tools/octomap_kit.py, on the CPU of the machine that made the fixture).
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
sys.path.insert(0, str(ROOT / "tests"))

PLANES, MAX_RANGE, CAPACITY = 4, 25.0, 1 << 22


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_stamped_bench_synth.json"))
    args = ap.parse_args()

    import torch

    import _pkg
    import bench_occupancy_rays as rays
    import occupancy_ray_cases as rc

    pkg = _pkg.load()
    bm = pkg.StereoBM.create(64, 15, device=0)
    planes, poses = rays.synth_planes(PLANES)
    model = rays.synth_model()
    clouds = [torch.from_numpy(np.ascontiguousarray(rc.plane_points(d, rays.SCALE, model, pose), np.float32)).to("cuda:0") for d, pose in zip(planes, poses)]
    origins = [pose[[3, 7, 11]] for pose in poses]
    params = pkg.occ_ray_params(max_range=MAX_RANGE)
    cpu_path = ROOT / "tests" / "golden" / "occupancy_stamped_cpu.json"
    cpu = json.loads(cpu_path.read_text()) if cpu_path.exists() else dict(calls={}, what="", build="")
    theirs = cpu["calls"].get("frames", {})
    note = "octomap_cpu_* are figures across two machines: " + cpu["what"] + ", " + cpu["build"]
    results = []

    def emit(**row):
        results.append(row)
        print(json.dumps(row), flush=True)

    def clock(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def scans(omap, stamped):
        for i, (c, o) in enumerate(zip(clouds, origins)):
            if stamped:
                omap.set_time(1000 + 10 * i)
            omap.insert_cloud(c, o, params, sync=False)

    def fresh(stamped):
        omap = pkg.OccupancyMap(bm, CAPACITY)
        if stamped:
            omap.enable_stamps()
        return omap

    wall = {True: [], False: []}
    for _ in range(args.repeat + 1):             # the first round allocates
        for stamped in (True, False):
            omap = fresh(stamped)
            wall[stamped].append(clock(lambda: scans(omap, stamped)))
            voxels = omap.size()
            omap.close()
    stages = {}
    bm.set_profiling(True)
    for stamped in (True, False):
        omap = fresh(stamped)
        mark = apply = 0.0
        for i, (c, o) in enumerate(zip(clouds, origins)):
            omap.set_time(1000 + 10 * i)
            omap.insert_cloud(c, o, params)
            prof = omap.profile()
            mark, apply = mark + prof["occ_rays_mark"], apply + prof["occ_rays_apply"]
        stages[stamped] = dict(mark_ms=mark, apply_ms=apply)
        omap.close()
    bm.set_profiling(False)
    a, b = float(np.median(wall[True][1:])), float(np.median(wall[False][1:]))
    emit(question="scan", scans=PLANES, points=[int(c.shape[0]) for c in clouds], voxels=voxels, stamped_wall_ms=a, stamped_wall_ms_all=wall[True][1:],
         plain_wall_ms=b, plain_wall_ms_all=wall[False][1:], stamped_over_plain=a / b, stamped_stage_ms=stages[True], plain_stage_ms=stages[False],
         octomap_cpu_insert_ms=theirs.get("insert_ms"), note=note)

    st_map, pl_map = fresh(True), fresh(False)
    scans(st_map, True), scans(pl_map, False)
    st_map.set_time(1100)
    t_st, t_pl = st_map.tree(params=params), pl_map.tree(params=params)
    st_ms, pl_ms = [], []
    for _ in range(args.repeat + 1):
        st_ms.append(clock(lambda: t_st.build(params=params, sync=False)))
        pl_ms.append(clock(lambda: t_pl.build(params=params, sync=False)))
    a, b = float(np.median(st_ms[1:])), float(np.median(pl_ms[1:]))
    emit(question="tree", voxels=voxels, stamped_nodes=t_st.info()["nodes"], plain_nodes=t_pl.info()["nodes"], stamped_build_ms=a, stamped_build_ms_all=st_ms[1:],
         plain_build_ms=b, plain_build_ms_all=pl_ms[1:], stamped_over_plain=a / b, octomap_cpu_prune_update_ms=theirs.get("prune_update_ms"), note=note)
    for x in (t_st, t_pl, st_map, pl_map):
        x.close()

    deg, forg, counts = [], [], None
    for _ in range(args.repeat + 1):
        omap = fresh(True)
        scans(omap, True)
        omap.set_time(1100)
        n = [0, 0]
        deg.append(clock(lambda: n.__setitem__(0, omap.degrade_outdated(75, params))))
        forg.append(clock(lambda: n.__setitem__(1, omap.forget_older_than(85))))
        counts = dict(degraded=n[0], forgotten=n[1], left=omap.size())
        omap.close()
    emit(question="forget", voxels=voxels, degrade_ms=float(np.median(deg[1:])), degrade_ms_all=deg[1:], forget_ms=float(np.median(forg[1:])),
         forget_ms_all=forg[1:], octomap_cpu_degrade_ms=theirs.get("degrade_ms"), octomap_cpu_forget_ms=theirs.get("forget_ms"), note=note, **counts)
    bm.close()
    out = pathlib.Path(args.out)
    out.write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), results=results), indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
