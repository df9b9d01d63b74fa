"""Times estimate_motion (include/sbm.h) on the MI355X and the sequential C restatement on the host.

    python tools/bench_pnp.py [--reps 20] [--out profiles/pnp_bench.json]

Legs: 64 and 1 jobs of synthetic scenes at N = 150, 500 and 1 500 matches with 30 % outliers (the reference's parameters);
the golden pair's left frame through orb_features -> keypoints3d -> match with itself -> estimate_motion (64 copies of the job);
and the C restatement on 1 and 16 host processes for the same synthetic jobs, warmed up, doing only the reference's work (no
hypotheses beyond those its RANSAC loop reaches). Prints one JSON object.
"""
import argparse
import json
import math
import os
import pathlib
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))

K = np.array([718.856, 718.856, 607.1928, 185.2157])


def rot(a):
    a = np.asarray(a, float)
    th = np.linalg.norm(a)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def synth(rng, n, m, outliers=0.3):
    """m jobs over 2m frames of n points each: (xyz, kpts, count, pairs, npairs, jobs)."""
    xyz = np.full((2 * m, n, 3), np.nan, np.float32)
    kp = np.zeros((2 * m, n, 2), np.float32)
    for j in range(m):
        R, t = rot(rng.normal(0, 0.05, 3) + 1e-3), rng.normal(0, 0.3, 3)
        P = np.c_[rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(4, 40, n)].astype(np.float32)
        X = (R @ P.astype(np.float64).T).T + t
        uv = np.c_[K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]]
        uv += rng.normal(0, 0.3, uv.shape)
        bad = rng.random(n) < outliers
        uv[bad] += rng.uniform(20, 80, (bad.sum(), 2)) * rng.choice([-1, 1], (bad.sum(), 2))
        xyz[2 * j], kp[2 * j + 1], xyz[2 * j + 1] = P, uv.astype(np.float32), X.astype(np.float32)
    count = np.full(2 * m, n, np.int32)
    pairs = np.broadcast_to(np.c_[np.arange(n), np.arange(n)].astype(np.int32), (m, n, 2)).copy()
    npairs = np.full(m, n, np.int32)
    jobs = [(2 * j, 2 * j + 1) for j in range(m)]
    return xyz, kp, count, pairs, npairs, jobs


def time_gpu(bm, args, reps):
    import torch

    bm.estimate_motion(*args)   # warm-up: scratch and code objects
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        bm.estimate_motion(*args)
        ts.append((time.perf_counter() - t0) * 1e3)
    bm.set_profiling(1)
    bm.estimate_motion(*args)
    prof = bm.pnp_profile()
    bm.set_profiling(0)
    return {"wall_ms_median": float(np.median(ts)), "wall_ms_min": float(np.min(ts)), **{k: round(v, 4) for k, v in prof.items()}}


def _ref_job(a):
    import pnp_ref

    x, k, xt, pr = a
    # without the hypothesis buffer: only the work the reference does (the loop's own hypotheses, no others)
    return int(pnp_ref.estimate(x, k, xt, pr, K, hyp=False)[0]["status"])


def time_cpu(xyz, kp, pairs, npairs, jobs, procs):
    items = [(xyz[f], kp[t], xyz[t], pairs[j, :npairs[j]]) for j, (f, t) in enumerate(jobs)]
    if procs == 1:
        _ref_job(items[0])   # warm-up: the library is built (make) and loaded before the clock starts
        t0 = time.perf_counter()
        for it in items:
            _ref_job(it)
        return (time.perf_counter() - t0) * 1e3
    with ProcessPoolExecutor(procs) as ex:
        list(ex.map(_ref_job, items[:procs]))   # warm-up: the library is loaded in every worker
        t0 = time.perf_counter()
        list(ex.map(_ref_job, items))
        return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--cpu-procs", type=int, nargs="*", default=[1, 16])
    a = ap.parse_args()
    import torch

    import _pkg

    pkg = _pkg.load()
    bm = pkg.StereoBM.create(64, 21)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")  # noqa: E731
    out = {"device": torch.cuda.get_device_name(0), "synthetic": [], "golden": None, "cpu": []}
    rng = np.random.default_rng(0)
    for n in (150, 500, 1500):
        xyz, kp, count, pairs, npairs, jobs = synth(rng, n, 64)
        d = (dev(xyz), dev(kp), dev(count), dev(pairs), dev(npairs))
        for m in (64, 1):
            r = time_gpu(bm, (*d, jobs[:m], K), a.reps)
            res, _ = bm.estimate_motion(*d, jobs[:m], K)
            rec = pkg.pnp_records(res)
            r.update({"n": n, "jobs": m, "ok": int((rec["status"] == 0).sum()),
                      "mean_inliers": float(rec["num_inliers"].mean()), "mean_niters": float(rec["niters"].mean())})
            out["synthetic"].append(r)
            print(json.dumps(r), file=sys.stderr)
        for procs in a.cpu_procs:
            m = 16 if procs == 1 else 64
            ms = time_cpu(xyz, kp, pairs, npairs, jobs[:m], procs)
            out["cpu"].append({"n": n, "procs": procs, "jobs": m, "ms_total": ms, "ms_per_job": ms / m})
            print(json.dumps(out["cpu"][-1]), file=sys.stderr)
    # the golden pair through the front end
    import sbm_oracle

    g = np.load(ROOT / "tests" / "golden" / "ref_pair_640x480.npz")
    pattern = np.load(ROOT / "tests" / "golden" / "orb_pattern.npz")["pattern"]
    disp = bm.compute(dev(g["rect_l"]), dev(g["rect_r"]))
    desc, kpts, count = bm.orb_features(dev(g["rect_l"][None]), pattern)
    k = int(count.cpu()[0])
    mo = sbm_oracle.make_model()
    mg = pkg.StereoModel()
    import ctypes

    ctypes.memmove(ctypes.byref(mg), ctypes.byref(mo), ctypes.sizeof(mg))
    xyz = torch.full((1, kpts.shape[1], 3), float("nan"), dtype=torch.float32, device="cuda:0")
    xyz[0, :k] = bm.keypoints3d(disp, kpts[0, :k].contiguous(), mg, 0.0, 0.0)
    pairs, npairs = bm.match(desc, count, [(0, 0)] * 64)
    Kg = (mo.fx_l, mo.fy_l, mo.cx_l, mo.cy_l)
    r = time_gpu(bm, (xyz.contiguous(), kpts, count, pairs, npairs, [(0, 0)] * 64, Kg, mg), a.reps)
    res, _ = bm.estimate_motion(xyz.contiguous(), kpts, count, pairs, npairs, [(0, 0)] * 64, Kg, mg)
    rec = pkg.pnp_records(res)
    r.update({"keypoints": k, "pairs": int(npairs.cpu()[0]), "matches": int(rec["num_matches"][0]),
              "inliers": int(rec["num_inliers"][0]), "status": int(rec["status"][0]), "jobs": 64})
    out["golden"] = r
    bm.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    main()
