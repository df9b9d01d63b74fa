#!/usr/bin/env python3
"""Times the visual-word dictionary's addNewWords on the device: ms per add_words call on 750 device rows against a dictionary
of about 10^4, 10^5 and 10^6 words, for both metrics, with the search / decide + append split of sbm_get_profile, and the numpy
restatement's time for one such call beside it. The first call of each run is checked bit for bit (word ids, new rows, size)
against the restatement (tests/vwd_cases.py). Writes profiles/vwd_bench_synth.json.

    python tools/bench_vwd.py [--sizes 10000 100000 1000000] [--reps 5] [--out profiles/vwd_bench_synth.json]"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import _pkg  # noqa: E402
import vwd_cases as vc  # noqa: E402

N_QUERY = 750      # the reference's maxFeatures
SEED_ROWS = 65535  # rows per seeding call


def queries(rng, words):
    """750 rows as a key frame brings them: half revisit words (a few bytes nudged), half are new."""
    q = rng.integers(0, 256, (N_QUERY, 32), dtype=np.uint8)
    src = words[rng.integers(0, len(words), N_QUERY // 2)].astype(np.int16)
    src[np.arange(len(src)), rng.integers(0, 32, len(src))] += rng.integers(-9, 10, len(src))
    q[::2] = np.clip(src, 0, 255).astype(np.uint8)
    return q


def run(pkg, bm, torch, metric, N, reps):
    rng = np.random.default_rng(1000 + N + metric)
    d = pkg.VWDictionary(bm, N + SEED_ROWS + N_QUERY * (reps + 2), metric=metric)
    try:
        t0 = time.perf_counter()
        node = 1
        while d.size() < N:   # random rows through add_words itself: nearly all of them become words
            rows = rng.integers(0, 256, (min(SEED_ROWS, N - d.size()), 32), dtype=np.uint8)
            d.add_words(torch.from_numpy(rows).to("cuda:0"), node)
            node += 1
        seed_s = time.perf_counter() - t0
        size = d.size()
        words = d.words()
        # the first call, against the restatement
        q = queries(rng, words)
        t0 = time.perf_counter()
        rec = vc.search(q, words, metric, chunk=4096)
        restatement_ms = (time.perf_counter() - t0) * 1e3
        unique = vc.is_unique(rec)
        want = np.where(unique, size + np.cumsum(unique) - 1, rec[:, 0]).astype(np.int32)
        ids = d.add_words(torch.from_numpy(q).to("cuda:0"), node)
        exact = bool(np.array_equal(ids, want) and d.size() == size + int(unique.sum())
                     and np.array_equal(d.words(size), q[unique]))
        if not exact:
            raise SystemExit(f"metric {metric} N {N}: the first call differs from the restatement")
        # timed calls: fresh queries each, wall clock of the whole synchronous call and the device stages
        wall, stages = [], []
        for k in range(reps):
            dq = torch.from_numpy(queries(rng, words)).to("cuda:0")
            torch.cuda.synchronize()
            bm.set_profiling(0)
            t0 = time.perf_counter()
            d.add_words(dq, node + 1 + k)
            wall.append((time.perf_counter() - t0) * 1e3)
            bm.set_profiling(1)
            d.add_words(torch.from_numpy(queries(rng, words)).to("cuda:0"), node + 100 + k)
            stages.append(d.profile())
        bm.set_profiling(0)
        med = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
        return {"metric": "L1" if metric == vc.L1 else "L2", "words": size, "queries": N_QUERY, "new_words_first_call": int(unique.sum()),
                "add_words_ms": float(np.median(wall)), "add_words_ms_min": float(np.min(wall)), **med,
                "restatement_search_ms": restatement_ms, "first_call_exact": exact, "seed_seconds": seed_s}
    finally:
        d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vwd_bench_synth.json"))
    a = ap.parse_args()
    import torch

    pkg = _pkg.load()
    bm = pkg.StereoBM.create(16, 9)
    rows = []
    try:
        for metric in (vc.L1, vc.L2):
            for N in a.sizes:
                r = run(pkg, bm, torch, metric, N, a.reps)
                print(json.dumps(r), flush=True)
                rows.append(r)
    finally:
        bm.close()
    pathlib.Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "runs": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
