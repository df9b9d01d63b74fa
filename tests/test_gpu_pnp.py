"""estimate_motion on the MI355X against the sequential C restatement (oracle/pnp_ref): subsets, hypotheses and counts bit for
bit, the RANSAC outcome exactly, the refined pose to 1e-9, the transform and covariance scales to float ulps, status and inlier
lists exactly; synthetic scenes against their true pose; the golden pair through the whole front end."""
import ctypes
import math
import pathlib

import numpy as np
import pytest

import pnp_ref
from gpu_support import bm, build_callsite, dev  # noqa: F401

ROOT = pathlib.Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu

K = np.array([718.856, 718.856, 607.1928, 185.2157])
LOCAL = [0, 0, 1, 0.1, -1, 0, 0, 0.05, 0, -1, 0, 1.2]   # camera -> base: z forward becomes x
GATE = 1e-6                                              # px around a refine round's threshold


def rot(a):
    a = np.asarray(a, float)
    th = np.linalg.norm(a)
    if th == 0:
        return np.eye(3)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def model(pkg, local):
    m = pkg.StereoModel()
    m.fx_l, m.fy_l, m.cx_l, m.cy_l = K
    if local is not None:
        m.local[:] = [float(v) for v in local]
        m.has_local = 1
    return m


class Store:
    """Frames 2k (from: points) and 2k + 1 (to: keypoints = the points seen under pose k, some moved; to-points = the points
    in the to-camera), cap slots each; jobs and their pair lists."""

    def __init__(self, rng, sizes, cap, outliers=0.3, nan=0.0, noise=0.0):
        self.cap = cap
        nfr = 2 * len(sizes)
        self.xyz = np.full((nfr, cap, 3), np.nan, np.float32)
        self.kpts = np.zeros((nfr, cap, 2), np.float32)
        self.count = np.zeros(nfr, np.int32)
        self.poses = []
        for k, n in enumerate(sizes):
            R, t = rot(rng.normal(0, 0.05, 3)), rng.normal(0, 0.3, 3)
            P = np.c_[rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(4, 40, n)].astype(np.float32)
            Xc = (R @ P.astype(np.float64).T).T + t
            uv = np.c_[K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]].astype(np.float32)
            if noise:
                uv += rng.normal(0, noise, uv.shape).astype(np.float32)
            bad = rng.random(n) < outliers
            uv[bad] += (rng.uniform(20, 80, (bad.sum(), 2)) * rng.choice([-1, 1], (bad.sum(), 2))).astype(np.float32)
            if nan:
                P[rng.random(n) < nan, int(rng.integers(0, 3))] = np.nan
            self.xyz[2 * k, :n], self.kpts[2 * k + 1, :n], self.xyz[2 * k + 1, :n] = P, uv, Xc.astype(np.float32)
            self.count[2 * k] = self.count[2 * k + 1] = n
            self.poses.append((R, t))

    def pairs_for(self, jobs, rng, shuffle=True):
        m = len(jobs)
        pairs = np.full((m, self.cap, 2), -1, np.int32)
        npairs = np.zeros(m, np.int32)
        for j, (f, t) in enumerate(jobs):
            n = min(self.count[f], self.count[t])
            idx = np.arange(n)
            if shuffle:   # some from-points unmatched, as the matcher leaves them
                idx = idx[rng.random(n) < 0.95]
            pairs[j, :len(idx)] = np.c_[idx, idx]
            npairs[j] = len(idx)
        return pairs, npairs


def reference(store, jobs, pairs, npairs, local=None, params=None):
    out = []
    for j, (f, t) in enumerate(jobs):
        out.append(pnp_ref.estimate(store.xyz[f, :store.count[f]], store.kpts[t, :store.count[t]],
                                    store.xyz[t, :store.count[t]], pairs[j, :npairs[j]], K, local, params))
    return out


def check(pkg, store, jobs, pairs, npairs, res, inl, hyp, local=None, params=None, what=""):
    p = params if params is not None else pkg.pnp_params()
    recs = pkg.pnp_records(res)
    hy = pkg.pnp_records(hyp, pkg.PNP_HYP_DTYPE) if hyp is not None else None
    inl = inl.cpu().numpy()
    ref = reference(store, jobs, pairs, npairs, local, p)
    edge = 0
    for j, (r_ref, inl_ref, ran_ref, hyp_ref, ex) in enumerate(ref):
        g = recs[j]
        w = f"{what} job {j}"
        for k in ("num_matches", "ransac_inliers", "best_iteration", "niters"):
            assert g[k] == r_ref[k], (w, k, g[k], r_ref[k])
        if hy is not None:
            assert np.array_equal(hy[j]["subset"], hyp_ref["subset"]), w
            assert np.array_equal(hy[j]["count"], hyp_ref["count"]), w
            for k in ("R", "t"):   # bit for bit, NaN included
                assert hy[j][k].tobytes() == hyp_ref[k].tobytes(), (w, k, np.flatnonzero((hy[j][k] != hyp_ref[k]).any(axis=1)))
        # a point whose residual in some refine round lies within GATE of that round's threshold (the restatement tracks the
        # threshold and pose of every round) may be decided differently by ulps of the pose: exempt, counted, and expected to be none
        if ex["gate_margin"] < GATE:
            edge += 1
            continue
        for k in ("status", "num_inliers", "refine_solves", "refine_exit"):
            assert g[k] == r_ref[k], (w, k, g[k], r_ref[k])
        assert np.array_equal(inl[j, :g["num_inliers"]], inl_ref), w
        # the RANSAC inlier set itself: the final list when no refine ran, or after one round with a normal exit (the swap rule)
        if r_ref["best_iteration"] >= 0 and (r_ref["refine_exit"] == -1 or (r_ref["refine_exit"] == 0 and r_ref["refine_solves"] == 1)):
            assert np.array_equal(inl[j, :g["num_inliers"]], ex["matches"][ran_ref]), w
            assert len(ran_ref) == g["ransac_inliers"], w
        if not np.abs(r_ref["tvec"]).max() < 1e6:
            continue   # a degenerate job (every image point alike): the refine runs the pose off to infinity (sbm.h)
        if r_ref["best_iteration"] >= 0:
            for k in ("rvec", "tvec", "R"):
                assert np.allclose(g[k], r_ref[k], rtol=1e-9, atol=1e-12), (w, k, g[k], r_ref[k])
        scale = max(1.0, float(np.abs(r_ref["transform"]).max()))
        assert np.abs(g["transform"] - r_ref["transform"]).max() <= 4 * scale * np.finfo(np.float32).eps, w
        for k in ("cov_dist", "cov_angle"):
            assert abs(g[k] - r_ref[k]) <= 4 * abs(r_ref[k]) * np.finfo(np.float32).eps + 1e-12, (w, k, g[k], r_ref[k])
    print(f"{what}: {edge} job(s) with a point within {GATE} px of a refine threshold")
    assert edge == 0
    return recs


def run(bm, pkg, store, jobs, pairs, npairs, local=None, params=None, hyp=True, sync=True):
    return bm.estimate_motion(dev(store.xyz), dev(store.kpts), dev(store.count), dev(pairs), dev(npairs), jobs, K,
                              model(pkg, local), params, hyp=hyp, sync=sync)


@pytest.mark.parametrize("local", [None, LOCAL])
@pytest.mark.parametrize("outliers", [0.0, 0.3, 0.6])
def test_synthetic_scenes(bm, pkg, local, outliers):
    rng = np.random.default_rng(int(outliers * 10) + (local is not None))
    st = Store(rng, [150, 500, 1500, 40], 1500, outliers)
    jobs = [(0, 1), (2, 3), (4, 5), (6, 7)]
    pairs, npairs = st.pairs_for(jobs, rng)
    res, inl, hyp = run(bm, pkg, st, jobs, pairs, npairs, local)
    recs = check(pkg, st, jobs, pairs, npairs, res, inl, hyp, local, what=f"synthetic {outliers}")
    for j, (R, t) in enumerate(st.poses):
        # at 60 % outliers 300 draws may miss every all-inlier subset (0.4^6 per draw), or leave fewer than 20 inliers: the
        # reference fails those jobs too, and parity is what check() asserted
        assert recs[j]["status"] == 0 or outliers > 0.3
        if recs[j]["status"] == 0:
            assert np.abs(recs[j]["R"].reshape(3, 3) - R).max() < 1e-5 and np.abs(recs[j]["tvec"] - t).max() < 1e-4


def test_noise_free_ground_truth(bm, pkg):
    rng = np.random.default_rng(7)
    st = Store(rng, [300, 800], 800, 0.0)
    jobs = [(0, 1), (2, 3)]
    pairs, npairs = st.pairs_for(jobs, rng, shuffle=False)
    res, inl = run(bm, pkg, st, jobs, pairs, npairs, hyp=False)
    recs = pkg.pnp_records(res)
    for j, (R, t) in enumerate(st.poses):
        assert recs[j]["status"] == 0 and recs[j]["num_inliers"] == npairs[j]
        assert np.abs(recs[j]["R"].reshape(3, 3) - R).max() < 1e-6 and np.abs(recs[j]["tvec"] - t).max() < 1e-6


@pytest.mark.parametrize("n", [5, 6, 7, 19, 20, 21])
def test_small_n(bm, pkg, n):
    rng = np.random.default_rng(n)
    st = Store(rng, [n, n], 64, 0.0)
    jobs = [(0, 1), (2, 3)]
    pairs, npairs = st.pairs_for(jobs, rng, shuffle=False)
    for mi in (6, 20):
        p = pkg.pnp_params(min_inliers=mi)
        res, inl, hyp = run(bm, pkg, st, jobs, pairs, npairs, params=p)
        recs = check(pkg, st, jobs, pairs, npairs, res, inl, hyp, params=p, what=f"n={n} min={mi}")
        assert (recs["status"] == 1).all() == (n < mi)


def test_at_the_cap_and_edge_jobs(bm, pkg):
    rng = np.random.default_rng(21)
    st = Store(rng, [1500, 300, 300], 1500, 0.4, nan=0.2, noise=0.7)
    st.kpts[5, :300] = rng.uniform(0, 1200, (300, 2)).astype(np.float32)   # frame 5: every keypoint junk
    jobs = [(0, 1), (2, 3), (4, 5), (0, 1), (1, 0), (2, 2)]
    pairs, npairs = st.pairs_for(jobs, rng)
    p = pkg.pnp_params(refine_iterations=3)
    res, inl, hyp = run(bm, pkg, st, jobs, pairs, npairs, LOCAL, p)
    recs = check(pkg, st, jobs, pairs, npairs, res, inl, hyp, LOCAL, p, what="cap/edges")
    assert recs[2]["status"] in (2, 3) and recs[0]["status"] == 0 and recs[3]["status"] == 0


@pytest.mark.parametrize("rounds", [0, 2, 3])
def test_refine_rounds(bm, pkg, rounds):
    rng = np.random.default_rng(30 + rounds)
    st = Store(rng, [400, 400, 120, 60], 400, 0.3, noise=0.8)
    jobs = [(0, 1), (2, 3), (4, 5), (6, 7)]
    pairs, npairs = st.pairs_for(jobs, rng)
    p = pkg.pnp_params(refine_iterations=rounds)
    res, inl, hyp = run(bm, pkg, st, jobs, pairs, npairs, params=p)
    recs = check(pkg, st, jobs, pairs, npairs, res, inl, hyp, params=p, what=f"rounds {rounds}")
    # with these seeds: no refine (0 rounds), normal exits (2 rounds), and a break on too few inliers (3 rounds, job 3)
    assert set(recs["refine_exit"].tolist()) == {0: {-1}, 2: {0}, 3: {0, 1}}[rounds]


@pytest.mark.parametrize("m", [1, 64, 65])
def test_job_counts_and_launch_groups(bm, pkg, m):
    rng = np.random.default_rng(100 + m)
    st = Store(rng, [200, 90, 60], 200, 0.3)
    base = [(0, 1), (2, 3), (4, 5), (0, 1), (3, 2)]
    jobs = [base[int(i)] for i in rng.integers(0, len(base), m)]
    pairs, npairs = st.pairs_for(jobs, rng)
    res, inl, hyp = run(bm, pkg, st, jobs, pairs, npairs, LOCAL)
    check(pkg, st, jobs, pairs, npairs, res, inl, hyp, LOCAL, what=f"m={m}")


def test_async_then_stream_sync(bm, pkg):
    import torch

    rng = np.random.default_rng(9)
    st = Store(rng, [500, 500], 500, 0.3)
    jobs = [(0, 1), (2, 3)]
    pairs, npairs = st.pairs_for(jobs, rng)
    torch.cuda.synchronize()
    res, inl = run(bm, pkg, st, jobs, pairs, npairs, hyp=False, sync=False)
    torch.cuda.ExternalStream(bm.stream(), device="cuda:0").synchronize()
    check(pkg, st, jobs, pairs, npairs, res, inl, None, what="async")
    bm.synchronize()


def test_host_form(bm, pkg):
    rng = np.random.default_rng(12)
    st = Store(rng, [600], 600, 0.3, nan=0.05)
    pairs, npairs = st.pairs_for([(0, 1)], rng)
    pr = pairs[0, :npairs[0]]
    r, inl = bm.estimate_motion_host(st.xyz[0, :600], st.kpts[1, :600], st.xyz[1, :600], pr, K, model(pkg, LOCAL))
    r_ref, inl_ref, _, _, _ = pnp_ref.estimate(st.xyz[0, :600], st.kpts[1, :600], st.xyz[1, :600], pr, K, LOCAL)
    assert r["status"] == r_ref["status"] == 0 and r["best_iteration"] == r_ref["best_iteration"]
    assert np.array_equal(inl, inl_ref)
    assert np.allclose(r["rvec"], r_ref["rvec"], rtol=1e-9, atol=1e-12)
    # no pairs at all: too few matches, nothing else
    r0, i0 = bm.estimate_motion_host(st.xyz[0, :10], st.kpts[1, :10], st.xyz[1, :10], np.zeros((0, 2), np.int32), K)
    assert r0["status"] == 1 and r0["num_matches"] == 0 and len(i0) == 0


def test_profile_names(bm, pkg):
    rng = np.random.default_rng(4)
    st = Store(rng, [300], 300, 0.3)
    pairs, npairs = st.pairs_for([(0, 1)], rng)
    bm.set_profiling(1)
    try:
        run(bm, pkg, st, [(0, 1)], pairs, npairs, hyp=False)
        prof = bm.pnp_profile()
    finally:
        bm.set_profiling(0)
    assert set(prof) == {"pnp_hyp", "pnp_score", "pnp_refine", "pnp_total"} and prof["pnp_total"] > 0


def test_limits_on_the_device(bm, pkg):
    import torch

    L = pkg.load_library()
    p = pkg.pnp_params()
    st_x = torch.zeros((2, 8, 3), dtype=torch.float32, device="cuda:0")
    st_k = torch.zeros((2, 8, 2), dtype=torch.float32, device="cuda:0")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    pr = torch.zeros((1, 8, 2), dtype=torch.int32, device="cuda:0")
    npr = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    res = torch.zeros((1, 216), dtype=torch.uint8, device="cuda:0")
    inl = torch.zeros((1, 8), dtype=torch.int32, device="cuda:0")
    K4 = (ctypes.c_double * 4)(*K)
    jobs = (ctypes.c_int * 2)(0, 1)

    def call(n=2, m=1, jb=jobs, cap=8, Kx=K4, x=st_x.data_ptr(), r=res.data_ptr(), pp=p):
        return L.sbm_estimate_motion_device(bm._h, n, m, jb, x, st_k.data_ptr(), cnt.data_ptr(), cap, pr.data_ptr(),
                                            npr.data_ptr(), Kx, None, ctypes.byref(pp), r, inl.data_ptr(), None, 1)

    assert call() == 0
    assert pkg.pnp_records(res)[0]["status"] == 1
    assert call(n=0) == -24 and call(m=0) == -24
    assert call(cap=0) == -2 and call(cap=65536) == -2
    assert call(jb=(ctypes.c_int * 2)(0, 2)) == -2
    assert call(Kx=(ctypes.c_double * 4)(0, 1, 1, 1)) == -23
    assert call(Kx=(ctypes.c_double * 4)(1, 1, math.nan, 1)) == -23
    assert call(x=st_x.data_ptr() + 2) == -23 and call(r=res.data_ptr() + 4) == -23
    assert call(pp=pkg.pnp_params(min_inliers=5)) == -23


def test_golden_pair_end_to_end(bm, pkg, golden, oracle):
    """orb_features -> keypoints3d (the engine's disparity map) -> match of the left frame with itself -> estimate_motion: the
    identity pose, and the localTransform's inverse as the transform."""
    import torch

    pattern = np.load(ROOT / "tests" / "golden" / "orb_pattern.npz")["pattern"]
    Lm, Rm = golden["rect_l"], golden["rect_r"]
    disp = bm.compute(dev(Lm), dev(Rm))
    desc, kpts, count = bm.orb_features(dev(Lm[None]), pattern)
    k = int(count.cpu()[0])
    mo = oracle.make_model()
    mg = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(mg), ctypes.byref(mo), ctypes.sizeof(mg))
    xyz = torch.full((1, kpts.shape[1], 3), float("nan"), dtype=torch.float32, device="cuda:0")
    xyz[0, :k] = bm.keypoints3d(disp, kpts[0, :k].contiguous(), mg, 0.0, 0.0)
    pairs, npairs = bm.match(desc, count, [(0, 0)])
    Kg = (mo.fx_l, mo.fy_l, mo.cx_l, mo.cy_l)
    for local in (None, LOCAL):
        mm = pkg.StereoModel()
        ctypes.memmove(ctypes.byref(mm), ctypes.byref(mo), ctypes.sizeof(mm))
        if local is not None:
            mm.local[:] = [float(v) for v in local]
            mm.has_local = 1
        res, inl = bm.estimate_motion(xyz.contiguous(), kpts, count, pairs, npairs, [(0, 0)], Kg, mm)
        r = pkg.pnp_records(res)[0]
        assert r["status"] == 0 and r["num_matches"] > 20, r
        assert np.abs(r["R"].reshape(3, 3) - np.eye(3)).max() < 1e-6 and np.abs(r["tvec"]).max() < 1e-6, r
        want = np.eye(4)[:3] if local is None else np.linalg.inv(np.r_[np.asarray(local, float).reshape(3, 4), [[0, 0, 0, 1]]])[:3]
        assert np.abs(r["transform"].reshape(3, 4) - want).max() < 1e-5, r["transform"]
        # and the restatement agrees on the same inputs
        x_h, k_h = xyz[0, :k].cpu().numpy(), kpts[0, :k].cpu().numpy()
        pr = pairs[0, :int(npairs.cpu()[0])].cpu().numpy()
        r_ref, inl_ref, _, _, _ = pnp_ref.estimate(x_h, k_h, x_h, pr, Kg, local)
        assert r["num_inliers"] == r_ref["num_inliers"] and np.array_equal(inl[0, :r["num_inliers"]].cpu().numpy(), inl_ref)


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_opencv"])
def test_cpp_callsite_through_the_adaptor(tmp_path, mock):
    """estimateMotion's body as sbm::estimateMotion3DTo2D over the reference's std::map types (or the plain form): ids that are
    not consecutive, ids without a from-point (absent from words3A), without a to-point; against the restatement."""
    import subprocess

    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")] if mock else []
    exe, r = build_callsite(tmp_path, "pnp_callsite_main.cpp", extra, flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(77)
    st = Store(rng, [500], 500, 0.3, nan=0.1, noise=0.5)
    n = 500
    ids = np.sort(rng.choice(100000, n, replace=False)).astype(np.int32)
    xa, kb, xb = st.xyz[0, :n].copy(), st.kpts[1, :n].copy(), st.xyz[1, :n].copy()
    xa[np.isnan(xa).any(axis=1)] = np.nan        # NaN from-points are ids words3A does not hold
    xb[rng.random(n) < 0.1] = np.nan             # to-points without depth
    for local in (None, LOCAL):
        files = {}
        lt = np.zeros(0, np.float32) if local is None else np.asarray(local, np.float32)
        for name, arr in (("ids", ids), ("xa", xa), ("kb", kb), ("xb", xb), ("K", K.astype(np.float64)), ("lt", lt)):
            files[name] = tmp_path / f"{name}.raw"
            arr.tofile(files[name])
        out = tmp_path / "out.raw"
        r = subprocess.run([str(exe), *(str(files[k]) for k in ("ids", "xa", "kb", "xb", "K", "lt")), "20", "1", str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        raw = out.read_bytes()
        status = np.frombuffer(raw[:4], np.int32)[0]
        T = np.frombuffer(raw[4:52], np.float32)
        cov = np.frombuffer(raw[52:340], np.float64).reshape(6, 6)
        rest = np.frombuffer(raw[340:], np.int32)
        nm = rest[0]
        matches, ni = rest[1:1 + nm], rest[1 + nm]
        inliers = rest[2 + nm:2 + nm + ni]
        pr = np.c_[np.arange(n), np.arange(n)]
        r_ref, inl_ref, _, _, ex = pnp_ref.estimate(xa, kb, xb, pr, K, local)
        assert status == r_ref["status"] == 0
        assert np.array_equal(matches, ids[ex["matches"]])
        assert np.array_equal(inliers, ids[inl_ref])
        assert np.abs(T - r_ref["transform"]).max() <= 4 * max(1.0, float(np.abs(r_ref["transform"]).max())) * np.finfo(np.float32).eps
        want = np.diag([r_ref["cov_dist"]] * 3 + [r_ref["cov_angle"]] * 3)
        assert np.allclose(cov, want, rtol=4 * np.finfo(np.float32).eps, atol=0)
