#!/usr/bin/env python3
"""Times the occupancy map's insert options on the synthetic key frames of tools/bench_occupancy_rays.py and writes
profiles/occupancy_options_bench_synth.json.

    python tools/bench_occupancy_options.py [--planes 64] [--repeat 3]

Per max_range (5 and 25) four variants, one plane per call:

    plain       sbm_occ_insert_rays_device, every switch off
    discrete    sbm_occ_insert_rays_discrete_device: one ray per end voxel
    box         the bounding box on, a 10 m cube around the first pose
    detect      change detection on, reset and one change fetch (sbm_occ_fetch_changes_device) after every plane

Figures per variant: wall ms (median of --repeat, all of them beside it), the two stage times occ_rays_mark and occ_rays_apply
and, for detect, occ_fetch (from a second, profiled run), the ray steps counted by the restatement
tests/occupancy_option_cases.py on plane 0 and scaled by the plane count (every plane has the same depths; for the box this is
an upper bound, because later poses leave the cube's centre), the points and the distinct end voxels of plane 0, voxels stored.
"""
import argparse
import ctypes
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tools"), str(ROOT / "oracle")]
VARIANTS = ("plain", "discrete", "box", "detect")
CUBE = 10.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_options_bench_synth.json"))
    args = ap.parse_args()
    import torch

    import _pkg
    import bench_occupancy_rays as rays
    import occupancy_option_cases as oc
    import occupancy_ray_cases as rc

    pkg = _pkg.load()
    planes, poses = rays.synth_planes(args.planes)
    ref = rays.synth_model()
    m = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(m), ctypes.byref(ref), ctypes.sizeof(m))
    origin = poses[0][[3, 7, 11]]
    cube = (origin - np.float32(CUBE / 2), origin + np.float32(CUBE / 2))
    points = rc.plane_points(planes[0], rays.SCALE, ref, poses[0])
    centres = oc.discretize(points, 0.1)
    bm = pkg.StereoBM.create(64, 15, device=0)
    d_planes = torch.from_numpy(planes).to("cuda:0")
    results = []
    for max_range in rays.RANGES:
        box = oc.Box()
        assert box.set(*cube)
        steps = {}
        for v, (p, b) in dict(plain=(points, None), discrete=(centres, None), box=(points, box)).items():
            census = {}
            oc.scan_sets(p, origin, max_range, 0.1, b, census)
            steps[v] = census.get("steps", 0) * args.planes
        steps["detect"] = steps["plain"]
        for variant in VARIANTS:
            omap = pkg.OccupancyMap(bm, 1 << 24)
            params = pkg.occ_ray_params(max_range=max_range)
            omap.set_bbx(*cube)
            omap.use_bbx_limit(variant == "box")
            omap.enable_change_detection(variant == "detect")

            def run(stage=None):
                omap.reset()
                changes = 0
                for a in range(args.planes):
                    omap.insert_rays(d_planes[a:a + 1], m, poses[a:a + 1], rays.SCALE, params=params, sync=stage is not None,
                                     discretize=variant == "discrete")
                    if stage is not None:
                        for k in ("occ_rays_mark", "occ_rays_apply"):
                            stage[k] += omap.profile()[k]
                    if variant == "detect":
                        changes += len(omap.changes_device()[0])
                        if stage is not None:
                            stage["occ_fetch"] += omap.profile()["occ_fetch"]
                        omap.reset_change_detection()
                return omap.size(), changes

            run()   # the first call allocates
            wall = []
            for _ in range(args.repeat):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                voxels, changes = run()
                wall.append((time.perf_counter() - t0) * 1e3)
            bm.set_profiling(True)
            stage = {"occ_rays_mark": 0.0, "occ_rays_apply": 0.0, "occ_fetch": 0.0}
            run(stage)
            bm.set_profiling(False)
            overflow = omap.overflow()
            omap.close()
            results.append(dict(variant=variant, planes=args.planes, planes_per_call=1, width=rays.W, height=rays.H, scale=rays.SCALE,
                                max_range=max_range, wall_ms=float(np.median(wall)), wall_ms_all=wall, stage_ms=stage,
                                ray_steps=steps[variant], points_plane0=len(points), end_voxels_plane0=len(centres), voxels=int(voxels),
                                changes=int(changes), overflow=int(overflow)))
            print(json.dumps(results[-1]))
    bm.close()
    out = pathlib.Path(args.out)
    out.write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), cube_m=CUBE, results=results), indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
