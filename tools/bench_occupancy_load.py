#!/usr/bin/env python3
"""Times the .bt loader (sbm_occ_load_binary) on the maps of tools/bench_occupancy_tree.py's .bt table and writes
profiles/occupancy_load_bench.json.

    python tools/bench_occupancy_load.py [--repeat 20]

Maps: the five of bench_occupancy_tree.SWEEP, from the top 15 rows of one synthetic key frame to 8 whole key frames (160 x 120,
scale 4, inserted in log-odds mode at max_range 25). Each is written through the maximum-likelihood tree (tree.write_binary) and
its stream is loaded into a second map of 2^23 voxels. Figures per map:

    wall_ms        one synchronous load_binary from bytes in memory: parse, upload, reset, expansion (median of --repeat after a
                   warm-up call)
    parse_ms       one sbm_occ_binary_leaves call on the same bytes into arrays of the right size: the host pass of the load, plus
                   the key bounds and the copy into the three output arrays, which the load does not need
    host_ms        wall_ms - stage_ms: the call is synchronous, so this is the host's part -- the parse, the prefix array, the
                   upload and its wait, the final read of the counters
    stage_ms       "occ_load" of sbm_get_profile: the reset of the table and the expansion kernel, by device events
    reset_ms       the same stage for a stream with ONE leaf in the same map: the reset alone, to the launch of a 1-voxel kernel
    fit_stage_ms   the stage when the map is created for exactly the stream's voxels (the smallest table that takes it)
    voxels_per_s   voxels over wall_ms
    upload_bytes   12 per leaf

and a fetch of the loaded map is compared with the source map's voxels under the threshold, so that what is timed is known to be
right. The CPU figure beside them is what the fixture tool recorded for octomap's own readBinary of its stream for the 4-frame
scene (one thread, -O1, on the CPU of the machine that made the fixture), from tests/golden/occupancy_load_cpu.json: a figure
from another machine.

The expansion's two leaf searches: the library searches the prefix array per lane. A second library whose wavefronts share the
search (lane 0 finds its leaf, lane l looks at most l leaves on) is built by hand,

    hipcc <the Makefile's HIPFLAGS> -ffp-contract=off -DSBM_OCC_LOAD_SHARED=1 -c u96-slam_amd/csrc/sbm_occ_load.hip -o occ_shared.o
    hipcc --offload-arch=gfx950 --offload-compress -shared -fPIC -o u96-slam_amd/lib/libsbm_hip_occ_load_shared.so occ_shared.o <the other objects>

and where it exists this tool times every map with it too, in a child process (SBM_LIB_AB), and checks that both load the same
voxels.
"""
import argparse
import ctypes
import hashlib
import json
import os
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import bench_occupancy_rays as scene  # noqa: E402
from bench_occupancy_tree import RANGE, SWEEP  # noqa: E402

SHARED_LIB = "libsbm_hip_occ_load_shared.so"
CAPACITY = 1 << 23


def timed(call, repeat, sync):
    call()
    wall = []
    for _ in range(repeat):
        sync()
        t0 = time.perf_counter()
        call()
        sync()
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall)), wall


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--child", action="store_true", help="time the loads alone and print one JSON line (the second library's run)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_load_bench.json"))
    args = ap.parse_args()
    import torch

    import _pkg
    if not torch.cuda.is_available():
        raise SystemExit("bench_occupancy_load.py needs a GPU")
    pkg = _pkg.load()
    planes, poses = scene.synth_planes(max(n for n, _ in SWEEP))
    ref = scene.synth_model()
    m = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(m), ctypes.byref(ref), ctypes.sizeof(m))
    bm = pkg.StereoBM.create(64, 15, device=0)
    rp = pkg.occ_ray_params(max_range=RANGE)
    c = pkg.occ_ray_logodds(rp)
    d_planes = torch.from_numpy(planes).to("cuda:0")
    target = pkg.OccupancyMap(bm, CAPACITY)
    one_leaf = (b"# Octomap OcTree binary file\nid OcTree\nsize 17\nres 0.1\ndata\n" + bytes((3, 0)) * 15 + bytes((2, 0)))

    def stage(call, omap):
        bm.set_profiling(True)
        ms = []
        for _ in range(args.repeat):
            call()
            ms.append(omap.profile()["occ_load"])
        bm.set_profiling(False)
        return float(np.median(ms))

    rows_out = []
    with tempfile.TemporaryDirectory() as tmp:
        for n_planes, rows in SWEEP:
            src = pkg.OccupancyMap(bm, CAPACITY)
            src.insert_rays(d_planes[:n_planes, :rows].contiguous(), m, poses[:n_planes], scene.SCALE, rp)
            keys, lo = src.fetch_logodds()
            tree = src.tree(pkg.OCC_TREE_MAXLIKELIHOOD, rp)
            path = pathlib.Path(tmp) / "map.bt"
            tree.write_binary(path)
            tree.close()
            src.close()
            data = path.read_bytes()
            info = pkg.occ_binary_info(data)
            assert info["voxels"] == len(keys)

            def load():
                target.load_binary(data, rp)

            wall, wall_all = timed(load, args.repeat, torch.cuda.synchronize)
            got = target.fetch_logodds()                      # what was timed is right: the source's voxels under the threshold
            assert np.array_equal(got[0], keys) and np.array_equal(got[1].view(np.uint32), np.where(lo >= c[4], c[3], c[2]).view(np.uint32))
            assert target.overflow() == 0
            digest = hashlib.sha256(got[0].tobytes() + got[1].tobytes()).hexdigest()
            L, raw = pkg.load_library(), np.frombuffer(data, np.uint8)
            pk, pd, po = np.empty(info["leaves"], np.uint64), np.empty(info["leaves"], np.int32), np.empty(info["leaves"], np.uint8)
            count = ctypes.c_size_t()
            parse, parse_all = timed(lambda: L.sbm_occ_binary_leaves(raw.ctypes.data, len(raw), pk.ctypes.data, pd.ctypes.data, po.ctypes.data,
                                                                     len(pk), ctypes.byref(count)), args.repeat, lambda: None)
            assert count.value == info["leaves"]
            res = dict(planes=n_planes, rows=rows, voxels=len(keys), bt_bytes=len(data), leaves=info["leaves"], leaves_at=info["leaves_at"],
                       upload_bytes=12 * info["leaves"], wall_ms=wall, wall_ms_all=wall_all, parse_ms=parse, parse_ms_all=parse_all,
                       parse_share=parse / wall, stage_ms=stage(load, target), voxels_per_s=len(keys) / (wall * 1e-3), loaded_sha256=digest)
            res["host_ms"] = wall - res["stage_ms"]               # a synchronous call: what is not the device stage is the host's
            if not args.child:
                res["reset_ms"] = stage(lambda: target.load_binary(one_leaf, rp), target)
                fit = pkg.OccupancyMap(bm, len(keys))
                res["fit_stage_ms"] = stage(lambda: fit.load_binary(data, rp), fit)
                res["fit_wall_ms"], _ = timed(lambda: fit.load_binary(data, rp), args.repeat, torch.cuda.synchronize)
                fit.close()
            rows_out.append(res)
    target.close()
    bm.close()
    library = os.environ.get("SBM_LIB_AB", "libsbm_hip.so")
    if args.child:
        print(json.dumps(dict(library=library, maps=rows_out)))
        return
    doc = dict(device=torch.cuda.get_device_name(0), repeat=args.repeat, capacity=CAPACITY, insert_max_range=RANGE, library=library,
               leaf_search="per lane", maps=rows_out,
               octomap_cpu=json.loads((ROOT / "tests" / "golden" / "occupancy_load_cpu.json").read_text()))
    if (pkg.library_path().parent / SHARED_LIB).exists() and "SBM_LIB_AB" not in os.environ:
        r = subprocess.run([sys.executable, __file__, "--child", "--repeat", str(args.repeat)], env=dict(os.environ, SBM_LIB_AB=SHARED_LIB),
                           capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError("the shared-search run failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
        other = json.loads(r.stdout.strip().splitlines()[-1])
        for a, b in zip(rows_out, other["maps"]):
            assert a["loaded_sha256"] == b["loaded_sha256"], "the two leaf searches load different maps"
        doc["wavefront_shared_search"] = other
    pathlib.Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    brief = lambda rows: [{k: v for k, v in r.items() if not k.endswith("_all") and k not in ("leaves_at", "loaded_sha256")} for r in rows]  # noqa: E731
    print(json.dumps(dict(maps=brief(rows_out), shared=brief(doc.get("wavefront_shared_search", {}).get("maps", [])),
                          octomap_cpu=doc["octomap_cpu"])))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
