"""The motion-estimation restatement on the CPU: the C file (oracle/pnp_ref.c) against the literal transcription of the reference's
loops (pnp_ref.py) -- RNG and subsets, the RANSAC replay, the refine loop and its swap rule --, the RANSACUpdateNumIters walk that
makes niters library-independent, EPnP and the whole job against known poses, and the C-ABI's parameters without a GPU."""
import ctypes
import math
import pathlib

import numpy as np
import pytest

import pnp_ref
from gpu_support import build_callsite

ROOT = pathlib.Path(__file__).resolve().parents[1]

K = np.array([718.856, 718.856, 607.1928, 185.2157])


def rot(a):
    a = np.asarray(a, float)
    th = np.linalg.norm(a)
    if th == 0:
        return np.eye(3)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def scene(rng, n, R, t, outliers=0.0):
    """Points in front of the camera (float32) and their projections under (R, t) (float32), a fraction moved 20..80 px."""
    P = np.c_[rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(4, 40, n)].astype(np.float32)
    Xc = (R @ P.astype(np.float64).T).T + t
    uv = np.c_[K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]].astype(np.float32)
    bad = rng.random(n) < outliers
    uv[bad] += (rng.uniform(20, 80, (bad.sum(), 2)) * rng.choice([-1, 1], (bad.sum(), 2))).astype(np.float32)
    return P, uv, bad


@pytest.mark.parametrize("n", list(range(6, 120)) + [255, 256, 257, 1000, 1499, 1500, 2000])
def test_draws_equal_the_transcription(n):
    assert np.array_equal(pnp_ref.draw(n, 40), pnp_ref.draw_np(n, 40))


def test_draws_of_full_jobs_equal_the_transcription():
    for n in (7, 20, 150, 500, 1500):
        assert np.array_equal(pnp_ref.draw(n, 300), pnp_ref.draw_np(n, 300))


def test_draws_cover_every_n_up_to_2000():
    for n in range(6, 2001):
        assert np.array_equal(pnp_ref.draw(n, 3), pnp_ref.draw_np(n, 3)), n


def test_replay_equals_the_transcription():
    rng = np.random.default_rng(5)
    for trial in range(3000):
        n = int(rng.integers(7, 2000))
        iters = int(rng.choice([1, 2, 10, 300]))
        hi = int(rng.choice([6, 20, n]))
        counts = rng.integers(0, hi + 1, iters)
        if trial % 3 == 0:   # long flat runs: ties keep the earliest
            counts = np.sort(counts)
        assert pnp_ref.replay(counts, n) == pnp_ref.replay_np(list(counts), n), (n, iters)


def test_replay_ties_and_the_floor_of_six():
    assert pnp_ref.replay([5, 5, 5], 100) == (-1, 3, 0)                 # 5 never beats max(0, 5)
    assert pnp_ref.replay([6, 6, 7, 7], 100)[::2] == (2, 7)             # a tie keeps the earlier; 7 beats 6
    assert pnp_ref.replay([6, 6, 7, 7], 100) == pnp_ref.replay_np([6, 6, 7, 7], 100)


@pytest.mark.parametrize("rounds", [0, 1, 2, 3])
def test_refine_walk_equals_the_transcription(rounds):
    rng = np.random.default_rng(rounds)
    seen = set()
    for trial in range(2000):
        base = sorted(rng.choice(60, int(rng.integers(4, 40)), replace=False).tolist())
        sets, cur = [], base
        for _ in range(max(rounds, 1)):
            kind = int(rng.integers(0, 3))
            if kind == 0:        # same set: break on "unchanged"
                nxt = list(cur)
            elif kind == 1:      # a small set: break on "too few"
                nxt = sorted(rng.choice(60, int(rng.integers(0, 10)), replace=False).tolist())
            else:                # a new set
                nxt = sorted(rng.choice(60, int(rng.integers(10, 50)), replace=False).tolist())
            sets.append(nxt)
            cur = nxt
        got = pnp_ref.refine_walk(base, sets, rounds, 10)
        want = pnp_ref.refine_walk_np(base, sets, rounds, 10)
        assert [int(v) for v in got[0]] == want[0] and got[1:] == want[1:], (base, sets)
        seen.add(want[2])
    if rounds:
        assert seen == {0, 1, 2}   # normal exit and both breaks were walked


def test_refine_walk_swap_rule():
    # one round, normal exit: the list is the set the solve ran on (the RANSAC set), not the new one
    assert pnp_ref.refine_walk_np([1, 2, 3], [[4, 5, 6, 7]], 1, 2)[0] == [1, 2, 3]
    # two rounds: the set the second solve ran on
    assert pnp_ref.refine_walk_np([1, 2, 3], [[4, 5, 6, 7], [8, 9, 10]], 2, 2)[0] == [4, 5, 6, 7]
    # break on too few: the set the reprojection produced
    assert pnp_ref.refine_walk_np([1, 2, 3], [[4]], 1, 2)[0] == [4]


def test_update_num_iters_never_lands_near_a_half_integer():
    """num / denom of RANSACUpdateNumIters(0.99, (N - good) / N, 6, .) for every N <= 4096 and 6 <= good < N lies farther than
    1e-9 from every multiple of 0.5 (where it can decide the result: below 1001, the largest iterations count), so cvRound and
    the comparison with maxIters cannot differ between two log / pow implementations that differ by a few ulps."""
    num = math.log(1 - 0.99)
    worst = 1.0
    for n in range(7, 4097):
        good = np.arange(6, n, dtype=np.float64)
        ep = (n - good) / n
        with np.errstate(divide="ignore", invalid="ignore"):
            denom = np.log(1.0 - np.power(1.0 - ep, 6))
            r = num / denom
        r = r[np.isfinite(r) & (r < 1001.0)]
        if r.size:
            d = np.abs(r * 2 - np.rint(r * 2)) / 2
            worst = min(worst, float(d.min()))
    assert worst > 1e-9, worst
    # and the C restatement computes what the transcription does
    for n, good in ((7, 6), (20, 13), (150, 100), (500, 301), (1500, 700), (4096, 4095)):
        for mx in (300, 17, 1):
            assert pnp_ref.update_num_iters(0.99, (n - good) / n, 6, mx) == pnp_ref.update_num_iters_np(0.99, (n - good) / n, 6, mx)[0]
    assert pnp_ref.update_num_iters(0.99, 0.0, 6, 300) == 0


def test_epnp_recovers_known_poses():
    rng = np.random.default_rng(11)
    for trial in range(200):
        R = rot(rng.normal(0, 0.3, 3))
        t = rng.normal(0, 0.5, 3)
        P, uv, _ = scene(rng, 6, R, t)
        Re, te = pnp_ref.epnp6(P, uv, K)
        # the inputs are float32: that rounding, not EPnP, sets the floor
        assert np.abs(Re - R).max() < 1e-6 and np.abs(te - t).max() < 1e-5, trial


def test_rodrigues_round_trip():
    rng = np.random.default_rng(3)
    for _ in range(100):
        rv = rng.normal(0, 0.8, 3)
        if np.linalg.norm(rv) >= math.pi:   # the inverse returns the equivalent vector of angle < pi
            continue
        R = pnp_ref.rodrigues(rv)
        assert np.allclose(R, rot(rv), atol=1e-14)
        assert np.allclose(pnp_ref.rodrigues_inv(R), rv, atol=1e-12)


@pytest.mark.parametrize("outliers", [0.0, 0.3, 0.6])
def test_estimate_recovers_known_poses(outliers):
    rng = np.random.default_rng(int(outliers * 10))
    R = rot([0.02, -0.05, 0.01])
    t = np.array([0.3, -0.1, 0.5])
    P, uv, bad = scene(rng, 400, R, t, outliers)
    pairs = np.c_[np.arange(400), np.arange(400)]
    r, inl, ran, hyp, ex = pnp_ref.estimate(P, uv, P, pairs, K)
    assert r["status"] == 0 and r["num_matches"] == 400
    assert np.abs(r["R"].reshape(3, 3) - R).max() < 1e-6 and np.abs(r["tvec"] - t).max() < 1e-6
    assert set(inl.tolist()) == set(np.flatnonzero(~bad).tolist())
    assert hyp[r["best_iteration"]]["count"] == r["ransac_inliers"] == len(ran)


def test_statuses():
    rng = np.random.default_rng(2)
    R, t = rot([0.01, 0.02, 0.03]), np.array([0.1, 0.0, 0.2])
    P, uv, _ = scene(rng, 30, R, t)
    pr = np.c_[np.arange(30), np.arange(30)]
    assert pnp_ref.estimate(P, uv, P, pr[:19], K)[0]["status"] == 1           # 19 < 20 matches
    Pn = P.copy()
    Pn[:15, 1] = np.nan
    r = pnp_ref.estimate(Pn, uv, P, pr, K)[0]
    assert r["status"] == 1 and r["num_matches"] == 15                        # NaN points are dropped
    junk = rng.uniform(0, 1000, (30, 2)).astype(np.float32)
    assert pnp_ref.estimate(P, junk, P, pr, K)[0]["status"] in (2, 3)       # all outliers


# ---- the C-ABI without a GPU ------------------------------------------------------------------------------------------
def test_defaults_are_the_reference_values(pkg):
    L = pkg.load_library()
    p = pkg.PnpParams()
    L.sbm_pnp_params_default(p)
    assert (p.min_inliers, p.refine_iterations, p.iterations, p.reprojection_error, p.refine_sigma, p.confidence) == (
        20, 1, 300, 2.0, 3.0, 0.99)
    assert pkg.pnp_validate(p) == 0
    assert ctypes.sizeof(pkg.PnpParams) == 32
    assert pkg.PNP_RESULT_DTYPE.itemsize == 216 and pkg.PNP_HYP_DTYPE.itemsize == 128


@pytest.mark.parametrize("change,code", [
    ({}, 0), ({"min_inliers": 6}, 0), ({"min_inliers": 5}, -23), ({"min_inliers": 65535}, 0), ({"min_inliers": 65536}, -23),
    ({"refine_iterations": 0}, 0), ({"refine_iterations": -1}, -23), ({"refine_iterations": 100}, 0),
    ({"refine_iterations": 101}, -23), ({"iterations": 1}, 0), ({"iterations": 0}, -23), ({"iterations": 1000}, 0),
    ({"iterations": 1001}, -23), ({"reprojection_error": 0.0}, -23), ({"reprojection_error": math.inf}, -23),
    ({"reprojection_error": math.nan}, -23), ({"reprojection_error": 1e-3}, 0), ({"refine_sigma": 0.0}, 0),
    ({"refine_sigma": -1.0}, -23), ({"refine_sigma": math.nan}, -23), ({"confidence": 0.0}, -23), ({"confidence": 1.0}, -23),
    ({"confidence": math.nan}, -23), ({"confidence": 0.5}, 0),
])
def test_validate_status_codes(pkg, change, code):
    p = pkg.pnp_params()
    for k, v in change.items():
        setattr(p, k, v)
    assert pkg.pnp_validate(p) == code


def test_null_and_limit_arguments(pkg):
    L = pkg.load_library()
    p = pkg.pnp_params()
    assert L.sbm_pnp_params_validate(None) == -1
    buf = ctypes.create_string_buffer(4096)
    a = ctypes.addressof(buf)
    K4 = (ctypes.c_double * 4)(*K)
    jobs = (ctypes.c_int * 2)(0, 0)
    args = [None, 1, 1, jobs, a, a, a, 8, a, a, K4, None, ctypes.byref(p), a, a, None, 1]
    assert L.sbm_estimate_motion_device(*args) == -1                  # null handle
    r = pkg.load_library().sbm_estimate_motion(None, None, 0, None, None, 0, None, 0, K4, None, ctypes.byref(p), a, a)
    assert r == -1


def test_gather_and_the_work_without_hypotheses():
    """The restatement's gather is the reference's (finite from-points, pairs in order), and without the hypothesis buffer it
    does only the reference's work with the same outcome."""
    rng = np.random.default_rng(8)
    R, t = rot([0.03, -0.02, 0.01]), np.array([0.2, 0.1, -0.3])
    P, uv, _ = scene(rng, 300, R, t, 0.3)
    P[rng.random(300) < 0.2, 1] = np.nan
    keep = rng.random(300) < 0.9
    pr = np.c_[np.flatnonzero(keep), np.flatnonzero(keep)]
    a = pnp_ref.estimate(P, uv, P, pr, K)
    b = pnp_ref.estimate(P, uv, P, pr, K, hyp=False)
    fin = pr[np.isfinite(P[pr[:, 0]]).all(axis=1), 0]
    assert np.array_equal(a[4]["matches"], fin) and np.array_equal(a[4]["xyz"], P[fin]) and np.array_equal(a[4]["uv"], uv[fin])
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and b[3] is None
    assert a[4]["gate_margin"] > 0


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_opencv"])
def test_cpp_adaptor_compiles(tmp_path, mock):
    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")] if mock else []
    _, r = build_callsite(tmp_path, "pnp_callsite_main.cpp", extra, flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr[-3000:]
