"""Measure the occupancy map (buildOccupancyGridMap at the reference's constants: 0.1 m voxels, rangeMax 5.0f) on --n planes of
160 x 120 (a VGA map decimated by 4) of a walk through a synthetic room -- sloped floor and walls, ~7 % invalid pixels, poses
that advance and turn a little per key frame, so that most points of a frame fall into voxels an earlier frame filled -- and
print one JSON line:

  insert_ms            device time of one sbm_occ_insert_device call on the --n planes into an EMPTY map, between two events on
                       the engine's stream (median over --steps; the reset before it is outside the events)
  insert_again_ms      the same call into the map that already holds them (every key found, no slot claimed)
  fetch_ms             sbm_occ_fetch_device (compaction + 6 radix passes), host wall time (it synchronises)
  points / accepted / voxels / duplicate_rate   pixels fed, points kept by the gate and the key, distinct voxels, 1 - voxels/accepted
  restatement_1core_ms oracle/occupancy_ref (sequential C, per-pixel keys) + numpy's unique on the same input, one core
  equal                the device's sorted keys and hit counts equal the restatement's

  python tools/bench_occupancy.py [--n 64] [--steps 20] [--warmup 3] [--capacity 262144] [--out FILE]
"""
import argparse
import ctypes
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))


def walk(n, h=120, w=160, seed=0):
    rng = np.random.default_rng(seed)
    rows, cols = np.mgrid[0:h, 0:w]
    planes, poses = [], []
    for k in range(n):
        # depth grows towards the top of the image (floor below, wall ahead), a slanted wall on one side
        d = 40 + (700 * rows) // (h - 1) + (cols * (k % 7)) // 8 + rng.integers(0, 3, (h, w))
        d = d.astype(np.int16)
        d[rng.random((h, w)) < 0.05] = -16
        d[rng.random((h, w)) < 0.02] = 0
        yaw = 0.02 * k
        c, s = np.cos(yaw), np.sin(yaw)
        poses.append([c, -s, 0, 0.05 * k, s, c, 0, 0.01 * k, 0, 0, 1, 0.0])
        planes.append(d)
    return np.stack(planes), np.asarray(poses, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--capacity", type=int, default=1 << 18)
    ap.add_argument("--out")
    a = ap.parse_args()

    import occupancy_ref as occ

    planes, poses = walk(a.n)
    n, H, W = planes.shape
    m = occ.model(local=[0, 0, 1, 0.05, -1, 0, 0, 0, 0, -1, 0, 0.2])
    res = {"tool": "bench_occupancy", "n": n, "width": W, "height": H, "scale": 4, "capacity": a.capacity}
    occ.lib()
    t0 = time.perf_counter()
    want_k, want_h = occ.insert(planes, 4, m, poses)
    res["restatement_1core_ms"] = (time.perf_counter() - t0) * 1e3
    res["points"], res["accepted"], res["voxels"] = int(planes.size), int(want_h.sum()), int(len(want_k))
    res["duplicate_rate"] = 1.0 - len(want_k) / max(int(want_h.sum()), 1)

    import torch

    import _pkg

    pkg = _pkg.load()
    bm = pkg.StereoBM.create(64, 21)
    L = bm._L
    omap = pkg.OccupancyMap(bm, a.capacity)
    gm = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(gm), ctypes.byref(m), ctypes.sizeof(gm))
    d = torch.from_numpy(planes).to("cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.ExternalStream(L.sbm_stream(bm._h), device="cuda:0")

    def check(s):
        if s != 0:
            raise RuntimeError(f"status {s}")

    def timed_insert(reset):
        if reset:
            omap.reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        check(L.sbm_occ_insert_device(omap._m, n, d.data_ptr(), W, H, 4, ctypes.byref(gm), poses.ctypes.data, 0))
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        timed_insert(True)
    res["insert_ms"] = statistics.median(timed_insert(True) for _ in range(a.steps))
    res["insert_again_ms"] = statistics.median(timed_insert(False) for _ in range(a.steps))
    omap.reset()
    omap.insert(d, gm, poses, 4)
    fetch = []
    for _ in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        keys, hits = omap.keys_device()
        fetch.append((time.perf_counter() - t0) * 1e3)
    res["fetch_ms"] = statistics.median(fetch[a.warmup:])
    res["equal"] = bool(np.array_equal(keys.cpu().numpy().view(np.uint64), want_k) and
                        np.array_equal(hits.cpu().numpy().view(np.uint32), want_h))
    res["overflow"] = omap.overflow()
    omap.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
