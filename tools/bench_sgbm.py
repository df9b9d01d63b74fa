"""Measure the semi-global matcher at the reference's parameters (main.cpp:219-230: MODE_HH, 128 disparities, 11 x 11) on
640 x 480 pairs and print one JSON line:

  step_ms / per_pair_ms       device time of one n-pair sbm_sgbm_compute_device call (events on the engine's stream), median
  single_device_ms            the same for one pair
  single_host_call_ms         wall time of the host entry point for one pair (the main.cpp:233 shape: copies in and out)
  stages_ms                   per-stage device time of one n-pair call (sbm_get_profile "sgbm_*", synchronised per chunk)
  algorithmic                 bytes the stages must move and path-update lane operations, and the bound they imply
  restatement_host_ms         the CPU restatement (oracle/sgbm_ref.c, single-threaded C) on one pair: a port, for scale only

  python tools/bench_sgbm.py --pairs 64 --steps 5 --warmup 2 [--out profiles/sgbm_bench.json]

--step-only runs the timed n-pair steps and nothing else (no single-pair, host, profiled or restatement calls), so that a
kernel trace or counter run of it holds exactly (warmup + steps) n-pair calls.
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))

REF_ARGS = (-64, 128, 11, 100, 1000, 32, 0, 15, 1000, 16, 1)
HBM_TBS = 6.29   # measured copy bandwidth of the MI355X (profiles/hbm_calibration.json)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--no-restatement", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be >= 1")
    import numpy as np
    import torch

    import _pkg

    pkg = _pkg.load()
    from u96_slam_amd import synth

    n, W, H = a.pairs, a.width, a.height
    Ls, Rs = synth.make_batch(0, n, W, H, 64)
    dl, dr = torch.from_numpy(Ls).cuda(), torch.from_numpy(Rs).cuda()
    out = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
    sg = pkg.StereoSGBM.create(*REF_ARGS)
    stream = torch.cuda.ExternalStream(pkg.load_library().sbm_stream(sg.handle))

    def device_ms(left, right, dst, reps, warm):
        times = []
        for i in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sg.compute_device(left, right, dst, sync=False)
            e1.record(stream)
            sg.synchronize()
            if i >= warm:
                times.append(e0.elapsed_time(e1))
        return times

    steps = device_ms(dl, dr, out, a.steps, a.warmup)
    if a.step_only:
        print(json.dumps(dict(metric="sgbm_ref640_hh", pairs=n, width=W, height=H, step_only=True,
                              step_ms_all=[round(t, 3) for t in steps])))
        return
    single = device_ms(dl[:1], dr[:1], out[:1], max(a.steps, 5), a.warmup)
    host = []
    for i in range(a.warmup + max(a.steps, 5)):
        t = time.perf_counter()
        sg.compute(Ls[0], Rs[0])
        if i >= a.warmup:
            host.append((time.perf_counter() - t) * 1e3)
    sg.set_profiling(1)
    sg.compute_device(dl, dr, out)
    stages = {k: round(sg.profile("sgbm_" + k), 3) for k in ("cost", "aggregate", "select", "median", "speckle", "total")}
    sg.set_profiling(0)

    D = REF_ARGS[1]
    w1 = W + min(REF_ARGS[0], 0) - max(REF_ARGS[0] + D, 0)
    cells = w1 * H * D
    ndir = 8
    # hsum write, C: hsum read + C write, paths: C read + S write (first) / C read + S read + S write, select: S read
    bytes_pair = 2 * cells * (1 + 2 + 2 + 3 * (ndir - 1) + 1)
    ops_pair = cells * ndir * 12   # lane operations per path update (loads, 3 mins, adds, saturating add, reduction share)
    step_med = statistics.median(steps)
    res = dict(
        metric="sgbm_ref640_hh", pairs=n, width=W, height=H, params=dict(zip(
            ("minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff", "preFilterCap", "uniquenessRatio",
             "speckleWindowSize", "speckleRange", "mode"), REF_ARGS)),
        step_ms=round(step_med, 3), step_ms_all=[round(t, 3) for t in steps], per_pair_ms=round(step_med / n, 4),
        single_device_ms=round(statistics.median(single), 3), single_host_call_ms=round(statistics.median(host), 3),
        stages_ms=stages,
        algorithmic=dict(width1=w1, cells_per_pair=cells, bytes_per_pair=bytes_pair, lane_ops_per_pair=ops_pair,
                         hbm_floor_ms_per_pair=round(bytes_pair / (HBM_TBS * 1e12) * 1e3, 4),
                         achieved_tbs=round(bytes_pair * n / (step_med * 1e-3) / 1e12, 3)),
    )
    if not a.no_restatement:
        import sgbm_ref

        p = sgbm_ref.make_params(*REF_ARGS)
        t = time.perf_counter()
        sgbm_ref.compute(p, Ls[0], Rs[0])
        res["restatement_host_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        res["restatement_note"] = "CPU port of the algorithm (single-threaded C), not OpenCV"
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
