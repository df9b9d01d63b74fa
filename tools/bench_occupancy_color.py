#!/usr/bin/env python3
"""Times the occupancy map's colours and writes profiles/occupancy_color_bench_synth.json.

    python tools/bench_occupancy_color.py [--repeat 3]

The map is that of the first four synthetic key frames of tools/bench_occupancy_rays.py at max_range 25. Three questions:

  batch   one averageNodeColor batch of the first frame's points (640 x 480 pixels; the points with a disparity) by point, colours
          and points in device memory: wall ms (median of --repeat) and the stage time of a profiled run ("occ_rays_apply").
  tree    the build of a LOGODDS tree over the map with colours against the build over the same map without: the difference is
          the colour pass (one look-up per voxel, sixteen level launches).
  stream  the ColorOcTree stream written to a file (ranking, body, copy, file) against the plain .ot of the same tree, and
          load_color_ot of those bytes against load_ot of the plain ones.

Beside them octomap's own CPU times for the same work from tests/golden/occupancy_color_cpu.json: figures ACROSS TWO MACHINES (one
thread, the flags of tools/octomap_kit.py, on the CPU of the machine that made the fixture).
"""
import argparse
import json
import pathlib
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))

PLANES, MAX_RANGE, CAPACITY = 4, 25.0, 1 << 22


def frame_batch(seed=7):
    """-> (points float32 (n, 3), colour words uint32 (n,)) of the first key frame: every pixel with a disparity, in pixel order"""
    import bench_occupancy_rays as rays
    import occupancy_ray_cases as rc
    planes, poses = rays.synth_planes(1)
    pts = rc.plane_points(planes[0], rays.SCALE, rays.synth_model(), poses[0])
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(pts, np.float32), rng.integers(0, 1 << 24, len(pts)).astype(np.uint32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_color_bench_synth.json"))
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
    cpu_path = ROOT / "tests" / "golden" / "occupancy_color_cpu.json"
    cpu = json.loads(cpu_path.read_text()) if cpu_path.exists() else dict(calls={}, what="", build="")
    theirs = cpu["calls"].get("frame_average", {})
    note = "octomap_cpu_* are figures across two machines: " + cpu["what"] + ", " + cpu["build"]
    results = []

    def emit(**row):
        results.append(row)
        print(json.dumps(row), flush=True)

    def fresh():
        omap = pkg.OccupancyMap(bm, CAPACITY)
        omap.insert_rays(d_planes, m, poses, rays.SCALE, params=params)
        return omap

    def clock(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    pts, words = frame_batch()
    d_pts, d_words = torch.from_numpy(pts).to("cuda:0"), torch.from_numpy(words.view(np.int32)).to("cuda:0")
    omap = fresh()
    wall = [clock(lambda: omap.average_colors(d_pts, d_words, sync=False)) for _ in range(args.repeat + 1)]   # the first allocates
    info = omap.last_colors()
    bm.set_profiling(True)
    omap.average_colors(d_pts, d_words)
    stage = omap.profile()["occ_rays_apply"]
    bm.set_profiling(False)
    ms = float(np.median(wall[1:]))
    emit(question="batch", items=len(pts), found=info["found"], voxels=omap.size(), wall_ms=ms, wall_ms_all=wall[1:], items_per_s=len(pts) / (ms * 1e-3),
         stage_ms=stage, octomap_cpu_ms=theirs.get("color_batch_ms"), note=note)

    plain = fresh()
    t_col, t_plain = omap.tree(), plain.tree()
    col_ms = [clock(lambda: t_col.build(sync=False)) for _ in range(args.repeat + 1)]
    plain_ms = [clock(lambda: t_plain.build(sync=False)) for _ in range(args.repeat + 1)]
    a, b = float(np.median(col_ms[1:])), float(np.median(plain_ms[1:]))
    emit(question="tree", voxels=omap.size(), nodes=t_col.info()["nodes"], colored_build_ms=a, colored_build_ms_all=col_ms[1:], plain_build_ms=b,
         plain_build_ms_all=plain_ms[1:], color_pass_ms=a - b, octomap_cpu_prune_update_ms=theirs.get("prune_update_ms"), note=note)

    with tempfile.TemporaryDirectory() as tmp:
        p_col, p_plain = str(pathlib.Path(tmp) / "c.ot"), str(pathlib.Path(tmp) / "p.ot")
        w_col = [clock(lambda: t_col.write_color_ot(p_col)) for _ in range(args.repeat + 1)]
        w_plain = [clock(lambda: t_plain.write_ot(p_plain)) for _ in range(args.repeat + 1)]
        data_col, data_plain = pathlib.Path(p_col).read_bytes(), pathlib.Path(p_plain).read_bytes()
    target = pkg.OccupancyMap(bm, CAPACITY)
    l_col = [clock(lambda: target.load_color_ot(data_col)) for _ in range(args.repeat + 1)]
    assert target.size() == omap.size()
    l_plain = [clock(lambda: target.load_ot(data_plain)) for _ in range(args.repeat + 1)]
    emit(question="stream", color_bytes=len(data_col), plain_bytes=len(data_plain), write_color_ms=float(np.median(w_col[1:])), write_color_ms_all=w_col[1:],
         write_plain_ms=float(np.median(w_plain[1:])), load_color_ms=float(np.median(l_col[1:])), load_color_ms_all=l_col[1:],
         load_plain_ms=float(np.median(l_plain[1:])), octomap_cpu_write_ms=theirs.get("write_ms"), octomap_cpu_read_ms=theirs.get("read_ms"),
         note=note + "; load_plain parses on the device, load_color on the host")
    for x in (t_col, t_plain, omap, plain, target):
        x.close()
    bm.close()
    out = pathlib.Path(args.out)
    out.write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), results=results), indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
