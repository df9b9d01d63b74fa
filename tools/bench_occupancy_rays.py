#!/usr/bin/env python3
"""Times the occupancy map's log-odds mode (sbm_occ_insert_rays_device) on synthetic key frames and writes
profiles/occupancy_rays_bench_synth.json.

    python tools/bench_occupancy_rays.py [--planes 64] [--repeat 3]

Shapes: `--planes` decimated VGA key frames (160 x 120, scale 4, depths of 5 to 17 m, one pose each along a gentle arc) at
max_range 5 and 25, all planes in one call and one plane per call. Figures per shape: wall ms and the two stage times
(occ_rays_mark, occ_rays_apply, from a second, profiled run), ray steps per second (the steps are counted by the restatement
tests/occupancy_ray_cases.py on plane 0 and scaled by the plane count: every plane has the same depths), voxels stored.
The CPU figure beside them is what tools/make_occupancy_ray_fixtures.py recorded for octomap's own insertPointCloud on plane 0
(one thread, -O1, on the CPU of the machine that made the fixture), read from tests/golden/occupancy_rays.npz.
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
W, H, SCALE = 160, 120, 4
RANGES = (5.0, 25.0)


def synth_planes(n, seed=7):
    """-> (planes int16 (n, H, W), poses float32 (n, 12)). fx * baseline = 48: a disparity of 16 * 48 / z is a depth of z."""
    rng = np.random.default_rng(seed)
    rows, cols = np.mgrid[0:H, 0:W]
    z = 11.0 + 6.0 * np.sin(cols / 23.0) * np.cos(rows / 17.0)            # 5 .. 17 m
    d = np.round(16.0 * 48.0 / z).astype(np.int16)
    d[rng.random((H, W)) < 0.03] = -16
    planes = np.repeat(d[None], n, axis=0)
    poses = []
    for k in range(n):
        yaw = 0.02 * k
        c, s = np.cos(yaw), np.sin(yaw)
        poses.append([c, -s, 0, 0.25 * k, s, c, 0, 0.05 * k, 0, 0, 1, 0.0])
    return planes, np.asarray(poses, np.float32)


def synth_model():
    sys.path.insert(0, str(ROOT / "oracle"))
    import occupancy_ref as occ
    # camera (z forward, x right, y down) -> body (x forward, y left, z up), lifted 0.2 m
    return occ.model(local=[0, 0, 1, 0.05, -1, 0, 0, 0, 0, -1, 0, 0.2])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_rays_bench_synth.json"))
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import ctypes

    import torch

    import _pkg
    import occupancy_ray_cases as rc

    pkg = _pkg.load()
    planes, poses = synth_planes(args.planes)
    ref = synth_model()
    m = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(m), ctypes.byref(ref), ctypes.sizeof(m))
    fixture = np.load(ROOT / "tests" / "golden" / "occupancy_rays.npz")
    bm = pkg.StereoBM.create(64, 15, device=0)
    d_planes = torch.from_numpy(planes).to("cuda:0")
    results = []
    for max_range in RANGES:
        census = {}
        rc.scan_sets(rc.plane_points(planes[0], SCALE, ref, poses[0]), poses[0][[3, 7, 11]], max_range, 0.1, census)
        steps = census["steps"] * args.planes
        for per_call in (args.planes, 1):
            omap = pkg.OccupancyMap(bm, 1 << 24)
            params = pkg.occ_ray_params(max_range=max_range)

            def run():
                omap.reset()
                for a in range(0, args.planes, per_call):
                    omap.insert_rays(d_planes[a:a + per_call], m, poses[a:a + per_call], SCALE, params=params, sync=False)
                return omap.size()

            run()   # the first call allocates
            wall = []
            for _ in range(args.repeat):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                voxels = run()
                wall.append((time.perf_counter() - t0) * 1e3)
            bm.set_profiling(True)
            stage = {"occ_rays_mark": 0.0, "occ_rays_apply": 0.0}
            omap.reset()
            for a in range(0, args.planes, per_call):
                omap.insert_rays(d_planes[a:a + per_call], m, poses[a:a + per_call], SCALE, params=params)
                for k, v in omap.profile().items():
                    if k in stage:
                        stage[k] += v
            bm.set_profiling(False)
            overflow = omap.overflow()
            omap.close()
            ms = float(np.median(wall))
            results.append(dict(planes=args.planes, planes_per_call=per_call, width=W, height=H, scale=SCALE, max_range=max_range,
                                wall_ms=ms, wall_ms_all=wall, stage_ms=stage, ray_steps=steps, ray_steps_per_s=steps / (ms * 1e-3),
                                voxels=int(voxels), overflow=int(overflow),
                                octomap_cpu_ms_one_plane=float(fixture[f"bench_cpu_ms_{int(max_range)}"]),
                                octomap_cpu_note="octomap's insertPointCloud on plane 0, one thread, -O1, on the CPU of the "
                                                 "machine that made tests/golden/occupancy_rays.npz; not measured by this run"))
            print(json.dumps(results[-1]))
    bm.close()
    out = pathlib.Path(args.out)
    out.write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), results=results), indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
