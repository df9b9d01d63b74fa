#!/usr/bin/env python3
"""Times the occupancy map's growth (sbm_occ_set_growth, sbm_occ_reserve) and writes profiles/occupancy_growth_bench_synth.json.

    python tools/bench_occupancy_growth.py [--planes 64] [--repeat 3]

The log-odds shapes are the synthetic key frames of tools/bench_occupancy_rays.py (160 x 120, scale 4, max_range 5 and 25), the hit
insert is the walk of tools/bench_occupancy.py. Three questions:

  ample      growth on beside growth off in a table that never has to grow (2^24 voxels for the rays; for the hit insert 2^21,
             which holds every pixel, and 2^18, which holds the voxels but cannot be shown to hold the pixels, so that every launch
             is preceded by a claim pass): what the counter read per scan, and the claim pass, cost. Wall ms, median of --repeat.
  from_one   the same calls into a map created for ONE voxel (and, for the rays, for 2^16 voxels, about one key frame at 5 m:
             "from_a_key_frame"): growth steps, slots moved, scans or launches redone, the final capacity, and the wall time
             beside the pre-sized map's.
  rehash     sbm_occ_reserve alone on the range-25 map (created for 2^23 voxels, moved to 2^24): ms, old slots per second, and the
             bytes the move touches: per old slot its key and flag word read (12 B) and per stored voxel its value read (4 B) and
             key, value written (12 B), plus the memsets of the new table (16 B per new slot) -- against the time.
"""
import argparse
import ctypes
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "oracle"))


def median_wall(torch, run, repeat, prepare=lambda: None):
    prepare()
    run()   # the first call allocates
    wall = []
    for _ in range(repeat):
        prepare()   # outside the clock
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run()
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall)), wall, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_growth_bench_synth.json"))
    args = ap.parse_args()

    import torch

    import _pkg
    import bench_occupancy
    import bench_occupancy_rays as rays

    pkg = _pkg.load()
    bm = pkg.StereoBM.create(64, 15, device=0)

    def model_of(ref):
        m = pkg.StereoModel()
        ctypes.memmove(ctypes.byref(m), ctypes.byref(ref), ctypes.sizeof(m))
        return m

    planes, poses = rays.synth_planes(args.planes)
    m = model_of(rays.synth_model())
    d_planes = torch.from_numpy(planes).to("cuda:0")
    results = []

    def emit(**row):
        results.append(row)
        print(json.dumps(row), flush=True)

    # ---- log-odds inserts ------------------------------------------------------------------------------------------------------
    for max_range in rays.RANGES:
        params = pkg.occ_ray_params(max_range=max_range)
        for per_call in (args.planes, 1):
            def scans(omap):
                for a in range(0, args.planes, per_call):
                    omap.insert_rays(d_planes[a:a + per_call], m, poses[a:a + per_call], rays.SCALE, params=params, sync=False)
                return omap.size()

            wall = {}
            for grow in (False, True):
                omap = pkg.OccupancyMap(bm, 1 << 24, grow=grow)

                def run():
                    omap.reset()
                    return scans(omap)

                wall[grow], all_ms, voxels = median_wall(torch, run, args.repeat)
                g = omap.growth()
                assert g["grown"] == 0 and omap.overflow() == 0
                omap.close()
                emit(question="ample", mode="rays", max_range=max_range, planes=args.planes, planes_per_call=per_call, growth=grow,
                     capacity=1 << 24, wall_ms=wall[grow], wall_ms_all=all_ms, voxels=int(voxels))
            emit(question="ample", mode="rays", max_range=max_range, planes_per_call=per_call, ratio_on_over_off=wall[True] / wall[False])

            for created in (1, 1 << 16):
                made = []

                def fresh():
                    for old in made:
                        old.close()
                    made[:] = [pkg.OccupancyMap(bm, created, grow=True)]

                ms, all_ms, voxels = median_wall(torch, lambda: scans(made[0]), args.repeat, fresh)
                g = made[0].growth()
                assert made[0].overflow() == 0
                made[0].close()
                emit(question="from_one" if created == 1 else "from_a_key_frame", mode="rays", max_range=max_range, planes=args.planes,
                     planes_per_call=per_call, created_capacity=created, wall_ms=ms, wall_ms_all=all_ms, pre_sized_wall_ms=wall[False],
                     ratio_over_pre_sized=ms / wall[False], voxels=int(voxels), capacity=g["capacity"], slots=g["slots"],
                     steps=g["grown"], slots_moved=g["moved"], redone=g["redone"])

    # ---- the rehash alone --------------------------------------------------------------------------------------------------------
    params = pkg.occ_ray_params(max_range=25.0)
    rehash = []
    for _ in range(args.repeat):
        omap = pkg.OccupancyMap(bm, 1 << 23)
        omap.insert_rays(d_planes, m, poses, rays.SCALE, params=params)
        voxels, old_slots = omap.size(), omap.growth()["slots"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        omap.reserve(1 << 24)
        rehash.append((time.perf_counter() - t0) * 1e3)
        g = omap.growth()
        assert g["moved"] == voxels and omap.size() == voxels and omap.overflow() == 0
        omap.close()
    ms = float(np.median(rehash))
    moved_bytes = old_slots * 12 + voxels * 16 + g["slots"] * 16
    emit(question="rehash", mode="rays", voxels=int(voxels), old_slots=int(old_slots), new_slots=int(g["slots"]), wall_ms=ms, wall_ms_all=rehash,
         old_slots_per_s=old_slots / (ms * 1e-3), voxels_per_s=voxels / (ms * 1e-3), bytes_touched=int(moved_bytes),
         gb_per_s=moved_bytes / (ms * 1e-3) / 1e9, note="wall time of sbm_occ_reserve: five allocations, four memsets, the kernel, one "
         "counter read and five frees")

    # ---- hit inserts ---------------------------------------------------------------------------------------------------------------
    hplanes, hposes = bench_occupancy.walk(args.planes)
    import occupancy_ref as occ

    hm = model_of(occ.model(local=[0, 0, 1, 0.05, -1, 0, 0, 0, 0, -1, 0, 0.2]))
    d_h = torch.from_numpy(hplanes).to("cuda:0")
    base = None
    for capacity, grow in ((1 << 21, False), (1 << 21, True), (1 << 18, False), (1 << 18, True), (1, True)):
        made = []

        def fresh_hits():
            for old in made:
                old.close()
            made[:] = [pkg.OccupancyMap(bm, capacity, grow=grow)]

        def run_hits():
            made[0].insert(d_h, hm, hposes, 4, sync=False)
            return made[0].size()

        ms, all_ms, voxels = median_wall(torch, run_hits, args.repeat, fresh_hits)
        g = made[0].growth()
        assert made[0].overflow() == 0
        made[0].close()
        if not grow:
            base = ms
        emit(question="from_one" if capacity == 1 else "ample", mode="hits", planes=args.planes, created_capacity=capacity, growth=grow,
             wall_ms=ms, wall_ms_all=all_ms, ratio_over_growth_off=ms / base, voxels=int(voxels), capacity=g["capacity"], steps=g["grown"],
             slots_moved=g["moved"], redone=g["redone"], note="one insert call of all planes into a new map + size()")
    bm.close()
    out = pathlib.Path(args.out)
    out.write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), results=results), indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
