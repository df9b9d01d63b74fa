#!/usr/bin/env python3
"""Times the pose-graph optimiser on synthetic trajectories of 500, 4541 (KITTI 00) and 50 000 vertices: one loop closure per 40
vertices onto a stretch passed 30 vertices earlier, directed new -> old as the reference builds them, one in ten of them a gross
outlier. Per size and coupling: the partition, milliseconds per Levenberg-Marquardt iteration (wall, over `--num` iterations) with
the stage split of sbm_get_profile for the last iteration; the whole robust call (sizes up to --robust-max); and, with
--restatement, the same robust call through the dense numpy restatement of tests/pgo_cases.py (sizes up to --restatement-max: its
matrix is dense). A size whose junctions pass the cap is recorded as unsupported. Writes profiles/pgo_bench_synth.json; a part
that was not run keeps what the file already holds, so the device part and the restatement part may come from two runs.

    python tools/bench_pgo.py [--sizes 500 4541 50000] [--num 3] [--device] [--restatement] [--out profiles/pgo_bench_synth.json]"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import pgo_cases as pc  # noqa: E402


def hom(R, t):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return M


def trajectory_graph(n, seed=0):
    """ids 1..n; odometry k -> k+1 with small noise; closures (k, k - 30) every 40 vertices, every tenth one grossly wrong. The
    initial poses are the odometry integrated. Information: 1e4 I on odometry, 100 I on closures. Links in multimap order."""
    r = np.random.default_rng(seed)
    T = [np.eye(4)]
    for k in range(n - 1):
        T.append(T[-1] @ hom(pc.rot([0.05 * r.normal(), 0.05 * r.normal(), 1], 3.0 + r.normal()), [0.8, 0.02 * r.normal(), 0.01 * r.normal()]))
    noise = lambda s: hom(pc.rot(r.normal(size=3), s * 57.3 * r.normal()), s * r.normal(size=3))  # noqa: E731
    links, meas, info = [], [], []
    for k in range(1, n):
        links.append((k, k + 1)), meas.append(np.linalg.solve(T[k - 1], T[k]) @ noise(1e-3)), info.append(1e4 * np.eye(6))
    nc = 0
    for k in range(40, n + 1, 40):
        d = np.linalg.solve(T[k - 1], T[k - 31]) @ noise(1e-3)
        nc += 1
        if nc % 10 == 0:
            d = d @ hom(pc.rot([0.3, 1, 0.2], 25.0), [3.0, -2.0, 1.0])
        links.append((k, k - 30)), meas.append(d), info.append(100.0 * np.eye(6))
    order = sorted(range(len(links)), key=lambda i: links[i][0])
    P = [np.eye(4)]
    for k in range(n - 1):
        P.append(P[-1] @ meas[k])
    return dict(ids=np.arange(1, n + 1), poses=np.stack(P)[:, :3, :], frm=np.array([links[i][0] for i in order]),
                to=np.array([links[i][1] for i in order]), meas=np.stack([meas[i] for i in order])[:, :3, :],
                info=np.stack([info[i] for i in order])), nc


def device_part(sizes, num, robust_max):
    import _pkg
    pkg = _pkg.load()
    bm = pkg.StereoBM.create(16, 9)
    out = {}
    try:
        for n in sizes:
            c, nc = trajectory_graph(n)
            row = {"vertices": n, "edges": int(len(c["frm"])), "closures": nc}
            for name, coupling in (("reference", pc.REFERENCE), ("symmetric", pc.SYMMETRIC)):
                p = pkg.pgo_params(num=num, coupling=coupling)
                try:
                    info = pkg.pgo_plan(p, *pc.args(c))[0]
                except pkg.StereoBMError as e:
                    row[name] = {"unsupported": f"status {e.code}: junctions over the cap"}
                    continue
                g = pkg.PoseGraph(bm, p)
                g.optimize(*pc.args(c))                       # first call: allocations
                bm.set_profiling(1)
                t0 = time.perf_counter()
                err = g.optimize(*pc.args(c))[0]
                wall = (time.perf_counter() - t0) * 1e3
                stages = {k: round(v, 4) for k, v in g.profile().items()}
                bm.set_profiling(0)
                row[name] = {"junctions": info.n_junctions, "runs": info.n_runs, "schur_size": info.schur_size,
                             "ms_per_iteration_wall": round(wall / num, 3), "iterations": num, "stage_ms_last_iteration": stages,
                             "chi2_after": err}
                if n <= robust_max:
                    t0 = time.perf_counter()
                    rerr, ids, _, removed = pkg.PoseGraph(bm, num=20, coupling=coupling).optimize_robust(*pc.args(c))
                    row[name]["robust_call_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    row[name]["robust_removed"] = len(removed)
                    row[name]["robust_err"] = rerr
                print(n, name, json.dumps(row[name]), flush=True)
            out[str(n)] = row
    finally:
        bm.close()
    return out


def restatement_part(sizes, restatement_max):
    out = {}
    for n in sizes:
        if n > restatement_max:
            out[str(n)] = {"not_run": "the restatement's matrix is dense: (6 n)^2 doubles"}
            continue
        c, _ = trajectory_graph(n)
        t0 = time.perf_counter()
        err, ids, _, removed = pc.run_optimize_robust(*pc.args(c), 20)
        out[str(n)] = {"robust_call_ms": round((time.perf_counter() - t0) * 1e3, 1), "robust_removed": len(removed), "robust_err": err,
                       "coupling": "reference", "what": "numpy, dense matrix, numpy.linalg.solve; a CPU time of the machine it ran on"}
        print(n, "restatement", json.dumps(out[str(n)]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 4541, 50000])
    ap.add_argument("--num", type=int, default=3)
    ap.add_argument("--robust-max", type=int, default=4541)
    ap.add_argument("--restatement-max", type=int, default=500)
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--out", type=pathlib.Path, default=ROOT / "profiles" / "pgo_bench_synth.json")
    a = ap.parse_args()
    doc = json.loads(a.out.read_text()) if a.out.exists() else {}
    doc["workload"] = "synthetic trajectories; a closure (k, k - 30) every 40 vertices, every tenth an outlier; see tools/bench_pgo.py"
    if a.device:
        doc["device"] = device_part(a.sizes, a.num, a.robust_max)
    if a.restatement:
        doc["restatement"] = restatement_part(a.sizes, a.restatement_max)
    a.out.write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
