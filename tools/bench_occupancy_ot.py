#!/usr/bin/env python3
"""Times the .ot writer and loader (sbm_occ_ot_body_device / sbm_occ_ot_write, sbm_occ_ot_load) on the five maps of
tools/bench_occupancy_tree.py's .bt table and writes profiles/occupancy_ot_bench.json.

    python tools/bench_occupancy_ot.py [--repeat 20]

Maps: the five of bench_occupancy_tree.SWEEP (160 x 120 synthetic key frames, scale 4, log-odds mode, max_range 25). Medians of
--repeat calls after a warm-up call, per map:

  (a) write   ot_body_ms        "occ_tree_query" of one body call on a built LOGODDS tree whose ranks exist (device events)
              ot_first_body_ms  the same for the first body call after a build: the ranking passes included
              ot_write_wall_ms  tree.write_ot(path): body, copy to the host, the file
  (b) load    ot_wall_ms / ot_stage_ms            one synchronous load_ot from bytes, device parse; its "occ_load" stage, which is
                                                  the upload of the records, the parse, the reset and the expansion
              ot_host_wall_ms / ot_host_stage_ms  the same load with SBM_OCC_OT_HOST_PARSE=1; its stage is reset + expansion alone
              ot_device_parse_ms                  ot_stage_ms - ot_host_stage_ms: upload + parse on the device
              ot_host_parse_ms                    one sbm_occ_ot_leaves call on the same bytes: the host pass
  (c) scale   bt_write_wall_ms, bt_body_ms, bt_load_wall_ms, bt_load_stage_ms, tree_build_ms (MAXLIKELIHOOD, "occ_tree_build"):
              the existing .bt path of the same map on the same build

and a fetch of every loaded map is compared with the source map, so that what is timed is known to be right.

Per-kernel times of the device parse come from a run of their own,

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_occupancy_ot.py --kernels

which loads the largest map --repeat times and nothing else.
"""
import argparse
import ctypes
import json
import os
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
from bench_occupancy_tree import RANGE, SWEEP  # noqa: E402

CAPACITY = 1 << 23
ENV = "SBM_OCC_OT_HOST_PARSE"


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
    ap.add_argument("--kernels", action="store_true", help="load the largest map --repeat times and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "occupancy_ot_bench.json"))
    args = ap.parse_args()
    import torch

    import _pkg
    if not torch.cuda.is_available():
        raise SystemExit("bench_occupancy_ot.py needs a GPU")
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
    sync = torch.cuda.synchronize

    def stage(call, prof, key):
        bm.set_profiling(True)
        ms = []
        for _ in range(args.repeat):
            call()
            ms.append(prof()[key])
        bm.set_profiling(False)
        return float(np.median(ms)), ms

    def host(on):
        os.environ[ENV] = "1" if on else "0"

    rows_out = []
    sweep = SWEEP[-1:] if args.kernels else SWEEP
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        for n_planes, rows in sweep:
            src = pkg.OccupancyMap(bm, CAPACITY)
            src.insert_rays(d_planes[:n_planes, :rows].contiguous(), m, poses[:n_planes], scene.SCALE, rp)
            keys, lo = src.fetch_logodds()
            res = dict(planes=n_planes, rows=rows, voxels=len(keys))
            # (c) the .bt path
            ml = pkg.OccupancyTree(src)
            res["tree_build_ms"], res["tree_build_ms_all"] = stage(lambda: ml.build(pkg.OCC_TREE_MAXLIKELIHOOD, rp), ml.profile, "occ_tree_build")
            res["bt_body_ms"], _ = stage(ml.binary, ml.profile, "occ_tree_query")
            res["bt_write_wall_ms"], _ = timed(lambda: ml.write_binary(tmp / "map.bt"), args.repeat, sync)
            bt = (tmp / "map.bt").read_bytes()
            ml.close()
            res["bt_bytes"] = len(bt)
            if not args.kernels:
                res["bt_load_wall_ms"], res["bt_load_wall_ms_all"] = timed(lambda: target.load_binary(bt, rp), args.repeat, sync)
                res["bt_load_stage_ms"], _ = stage(lambda: target.load_binary(bt, rp), target.profile, "occ_load")
                got = target.fetch_logodds()
                assert np.array_equal(got[0], keys) and np.array_equal(got[1].view(np.uint32), np.where(lo >= c[4], c[3], c[2]).view(np.uint32))
            # (a) the .ot writer
            tree = pkg.OccupancyTree(src)
            first = []
            bm.set_profiling(True)
            for _ in range(args.repeat):
                tree.build(pkg.OCC_TREE_LOGODDS)
                tree.ot_body()
                first.append(tree.profile()["occ_tree_query"])
            bm.set_profiling(False)
            res["ot_first_body_ms"] = float(np.median(first))
            res["ot_body_ms"], res["ot_body_ms_all"] = stage(tree.ot_body, tree.profile, "occ_tree_query")
            res["ot_write_wall_ms"], _ = timed(lambda: tree.write_ot(tmp / "map.ot"), args.repeat, sync)
            ot = (tmp / "map.ot").read_bytes()
            info = pkg.occ_ot_info(ot)
            res.update(ot_bytes=len(ot), nodes=info["nodes"], leaves=info["leaves"])
            assert info["voxels"] == len(keys) and tree.ot() == ot
            tree.close()
            src.close()
            # (b) the .ot loader, both parses
            if args.kernels:
                host(False)
                for _ in range(args.repeat):
                    target.load_ot(ot)
                rows_out.append(res)
                continue
            for on, tag in ((False, "ot"), (True, "ot_host")):
                host(on)
                res[f"{tag}_wall_ms"], res[f"{tag}_wall_ms_all"] = timed(lambda: target.load_ot(ot), args.repeat, sync)
                res[f"{tag}_stage_ms"], _ = stage(lambda: target.load_ot(ot), target.profile, "occ_load")
                got = target.fetch_logodds()
                assert np.array_equal(got[0], keys) and np.array_equal(got[1].view(np.uint32), lo.view(np.uint32)) and target.overflow() == 0
            host(False)
            res["ot_device_parse_ms"] = res["ot_stage_ms"] - res["ot_host_stage_ms"]
            L, raw = pkg.load_library(), np.frombuffer(ot, np.uint8)
            pk, pd, pv = np.empty(info["leaves"], np.uint64), np.empty(info["leaves"], np.int32), np.empty(info["leaves"], np.float32)
            count = ctypes.c_size_t()
            res["ot_host_parse_ms"], _ = timed(lambda: L.sbm_occ_ot_leaves(raw.ctypes.data, len(raw), pk.ctypes.data, pd.ctypes.data,
                                                                           pv.ctypes.data, len(pk), ctypes.byref(count)), args.repeat, lambda: None)
            rows_out.append(res)
    target.close()
    bm.close()
    library = os.environ.get("SBM_LIB_AB", "libsbm_hip.so")
    if args.kernels:
        print("loaded the largest map", args.repeat, "times")
        return
    doc = dict(device=torch.cuda.get_device_name(0), repeat=args.repeat, capacity=CAPACITY, insert_max_range=RANGE, library=library, maps=rows_out)
    pathlib.Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")
    brief = lambda rows: [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items() if not k.endswith("_all")} for r in rows]  # noqa: E731
    print(json.dumps(dict(maps=brief(rows_out))))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
