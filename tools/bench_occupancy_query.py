#!/usr/bin/env python3
"""Times the occupancy map's queries (sbm_occ_cast_view_device, sbm_occ_cast_rays_device, sbm_occ_search_device) on the scene
of tools/bench_occupancy_rays.py and writes profiles/occupancy_query_bench_synth.json.

    python tools/bench_occupancy_query.py [--repeat 20]

Scene: the first 4 synthetic key frames of bench_occupancy_rays.synth_planes (160 x 120, scale 4, depths of 5 to 17 m) inserted
in log-odds mode at max_range 25, the tree tools/make_occupancy_query_fixtures.py timed octomap on. Workloads, all with
ignore_unknown = 1 and max_range 25: a 640 x 480 view from pose 0 (one ray per pixel, built on the device), 2^20 random rays
from around the sensor origins, 2^20 searches of random points in the scene's box. Figures per workload: wall ms (median of
--repeat, one synchronous call each), the stage time from sbm_get_profile (device events; median of --repeat profiled calls), rays or points per second,
and cell steps per second: the steps are counted by the transcription tests/occupancy_query_cases.py on a subsample of the rays
and scaled. The CPU figure beside them is what the fixture tool recorded for octomap's own castRay (one thread, -O1, on the CPU
of the machine that made the fixture) on the 160 x 120 view of this scene, read from tests/golden/occupancy_query_cpu.json.

The view kernel's two lane orders: the library maps a wavefront to an 8 x 8 pixel tile. A second library with the row order (64
consecutive pixels of a row per wavefront) is built by hand,

    hipcc <the Makefile's HIPFLAGS> -ffp-contract=off -DSBM_OCC_VIEW_TILED=0 -c u96-slam_amd/csrc/sbm_occ_query.hip -o occ_rows.o
    hipcc --offload-arch=gfx950 --offload-compress -shared -fPIC -o u96-slam_amd/lib/libsbm_hip_occ_rows.so occ_rows.o <the other objects>

and where it exists this tool times the view with it too, in a child process (SBM_LIB_AB), and checks that both orders answer
the same.
"""
import argparse
import ctypes
import hashlib
import json
import os
import pathlib
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import bench_occupancy_rays as scene  # noqa: E402

PLANES, RANGE, VIEW = 4, 25.0, (640, 480, 1)
ROWS_LIB = "libsbm_hip_occ_rows.so"
N = 1 << 20


def timed(call, repeat, torch):
    call()
    wall = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall)), wall


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--view-only", action="store_true", help="time the view alone and print one JSON line (the child run)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_query_bench_synth.json"))
    args = ap.parse_args()
    import torch

    import _pkg
    import occupancy_query_cases as qc

    pkg = _pkg.load()
    planes, poses = scene.synth_planes(PLANES)
    ref = scene.synth_model()
    m = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(m), ctypes.byref(ref), ctypes.sizeof(m))
    bm = pkg.StereoBM.create(64, 15, device=0)
    omap = pkg.OccupancyMap(bm, 1 << 22)
    omap.insert_rays(torch.from_numpy(planes).to("cuda:0"), m, poses, scene.SCALE, max_range=RANGE)
    q = pkg.occ_query_params(RANGE, 0.0, True)
    w, h, scale = VIEW
    # the camera model of the decimated planes serves a 640 x 480 view at scale 1: the same field of view, 16 times the rays

    def stage(call, name):
        bm.set_profiling(True)
        ms = []
        for _ in range(args.repeat):
            call()
            ms.append(omap.profile()[name])
        bm.set_profiling(False)
        return float(np.median(ms))

    def view():
        return omap.cast_view(w, h, m, poses[0], scale, q)

    view_ms, view_all = timed(view, args.repeat, torch)
    st, end = view()
    digest = hashlib.sha256(st.cpu().numpy().tobytes() + end.cpu().numpy().tobytes()).hexdigest()
    view_res = dict(library=os.environ.get("SBM_LIB_AB", "libsbm_hip.so"),
                    width=w, height=h, scale=scale, rays=w * h, wall_ms=view_ms, wall_ms_all=view_all,
                    stage_ms=stage(view, "occ_cast"), statuses=np.bincount(st.cpu().numpy().reshape(-1), minlength=5).tolist(),
                    answers_sha256=digest)
    if args.view_only:
        print(json.dumps(view_res))
        return
    keys, lo = omap.fetch_logodds()
    tmap = qc.Map(dict(zip((int(k) for k in keys), lo)), qc.LOGODDS, 0.0, omap.resolution)

    def steps_of(origins, dirs, total):
        census = {}
        pick = np.random.default_rng(1).choice(len(dirs), 256, replace=False)
        want = tmap.cast_rays(origins[pick], dirs[pick], True, RANGE, census)
        return census.get("steps", 0) / 256 * total, pick, want

    rows, cols = np.random.default_rng(2).integers(0, h, 256), np.random.default_rng(3).integers(0, w, 256)
    vo, vd = qc.view_rays(w, h, scale, ref, poses[0], pixels=list(zip(rows, cols)))   # 256 pixels by the header's formula
    census = {}
    want = tmap.cast_rays(vo, vd, True, RANGE, census)
    got_s, got_e = st.cpu().numpy()[rows, cols], end.cpu().numpy()[rows, cols]
    assert np.array_equal(got_s, want[0]) and np.array_equal(got_e[want[0] != 0].view(np.uint32), want[1][want[0] != 0].view(np.uint32))
    view_steps = census.get("steps", 0) / 256 * w * h
    view_res.update(order="tiles 8x8", cell_steps=view_steps, rays_per_s=w * h / (view_ms * 1e-3), cell_steps_per_s=view_steps / (view_ms * 1e-3))
    results = dict(view=view_res)
    if (pkg.library_path().parent / ROWS_LIB).exists() and "SBM_LIB_AB" not in os.environ:
        r = subprocess.run([sys.executable, __file__, "--view-only", "--repeat", str(args.repeat)], env=dict(os.environ, SBM_LIB_AB=ROWS_LIB),
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("the row-order run failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        rows_res = json.loads(r.stdout.strip().splitlines()[-1])
        assert rows_res["answers_sha256"] == digest, "the two lane orders answer differently"
        rows_res.update(order="rows of 64", cell_steps=view_steps, rays_per_s=w * h / (rows_res["wall_ms"] * 1e-3),
                        cell_steps_per_s=view_steps / (rows_res["wall_ms"] * 1e-3))
        results["view_rows"] = rows_res
    else:
        results["view_rows"] = None

    rng = np.random.default_rng(5)
    ro = (poses[rng.integers(0, PLANES, N)][:, [3, 7, 11]] + rng.uniform(-0.2, 0.2, (N, 3))).astype(np.float32)
    rd = rng.normal(size=(N, 3))
    rd[:, 2] *= 0.3
    rd = rd.astype(np.float32)
    d_o, d_d = torch.from_numpy(ro).to("cuda:0"), torch.from_numpy(rd).to("cuda:0")

    def rays():
        return omap.cast_rays(d_o, d_d, q)

    ms, ms_all = timed(rays, args.repeat, torch)
    st, end = rays()
    steps, pick, want = steps_of(ro, rd, N)
    assert np.array_equal(st.cpu().numpy()[pick], want[0])
    results["random_rays"] = dict(rays=N, wall_ms=ms, wall_ms_all=ms_all, stage_ms=stage(rays, "occ_cast"), cell_steps=steps,
                                  rays_per_s=N / (ms * 1e-3), cell_steps_per_s=steps / (ms * 1e-3),
                                  statuses=np.bincount(st.cpu().numpy(), minlength=5).tolist())
    unpacked = np.stack([(keys >> np.uint64(32)) & np.uint64(0xFFFF), (keys >> np.uint64(16)) & np.uint64(0xFFFF), keys & np.uint64(0xFFFF)], 1)
    lo_c, hi_c = (unpacked.min(0).astype(np.float64) - 32768) * 0.1, (unpacked.max(0).astype(np.float64) - 32767) * 0.1
    pts = rng.uniform(lo_c, hi_c, (N, 3)).astype(np.float32)
    d_p = torch.from_numpy(pts).to("cuda:0")

    def search():
        return omap.search(d_p, 0.0)

    ms, ms_all = timed(search, args.repeat, torch)
    state, _ = search()
    pick = rng.choice(N, 4096, replace=False)
    assert np.array_equal(state.cpu().numpy()[pick], tmap.search_all(pts[pick])[0])
    results["search"] = dict(points=N, wall_ms=ms, wall_ms_all=ms_all, stage_ms=stage(search, "occ_search"), points_per_s=N / (ms * 1e-3),
                             states=np.bincount(state.cpu().numpy() + 1, minlength=4).tolist())
    cpu = json.loads((ROOT / "tests" / "golden" / "occupancy_query_cpu.json").read_text())
    doc = dict(device=torch.cuda.get_device_name(0), planes=PLANES, insert_max_range=RANGE, max_range=RANGE, ignore_unknown=1,
               voxels=int(omap.size()), overflow=int(omap.overflow()), results=results, octomap_cpu=cpu)
    omap.close()
    bm.close()
    pathlib.Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
