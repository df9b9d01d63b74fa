"""GPU keypoint matching (u96-slam_amd/csrc/sbm_match.hip) bit for bit against the CPU restatement of matchingNoGuess /
matchingGuess (oracle/match_ref.c): every k-NN record, pair and count, in both modes and under both readings of the radius test, on
descriptors the engine itself computed from the golden pair, synthetic frames at the 1 500-point cap, crafted sets, and through
the projection, host, asynchronous and C++ entry points."""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import match_ref as ref
from gpu_support import bm, build_callsite, dev  # noqa: F401

ROOT = pathlib.Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu
READINGS = [False, True]
RIDS = ["unfused", "fused"]
K = (320.0, 321.5, 319.5, 239.25)
W, H = 640, 480


@pytest.fixture
def fused(monkeypatch, request):
    if request.param:
        monkeypatch.setenv("SBM_CV_READING", "256")
    else:
        monkeypatch.delenv("SBM_CV_READING", raising=False)
    return request.param


def store(frames, cap=None, marker=0xA5):
    """Per-frame (k, 32) descriptor lists -> (n, cap, 32) uint8 with a marker past each count, and the counts."""
    cap = cap or max(1, max(len(f) for f in frames))
    d = np.full((len(frames), cap, 32), marker, np.uint8)
    c = np.zeros(len(frames), np.int32)
    for i, f in enumerate(frames):
        d[i, :len(f)] = f
        c[i] = len(f)
    return d, c


def planted(rng, n, nt, flips=(0, 3, 20, 60)):
    """nt random rows, and n query rows that are near-duplicates of some of them (and a few random ones)."""
    to = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    fr = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for i in range(0, n, 2):
        if nt == 0:
            break
        row = to[rng.integers(0, nt)].copy()
        bits = np.unpackbits(row)
        k = flips[(i // 2) % len(flips)]
        idx = rng.choice(256, k, replace=False)
        bits[idx] ^= 1
        fr[i] = np.packbits(bits)
    return fr, to


def check_job(pairs, npairs, rec, j, dfrom, dto, proj=None, kto=None, fused=False, what="", radius=40.0, nndr=0.8):
    want_p, want_r = ref.match(dfrom, dto, proj, kto, radius=radius, nndr=nndr, fused=fused)
    k = int(npairs[j])
    assert k == len(want_p), (what, j, k, len(want_p))
    assert np.array_equal(pairs[j, :k], want_p), (what, j)
    assert np.all(pairs[j, k:] == -1), (what, j)
    if rec is not None:
        nf = len(dfrom)
        assert np.array_equal(rec[j, :nf], want_r), (what, j, np.argwhere((rec[j, :nf] != want_r).any(1))[:5])
        assert np.all(rec[j, nf:] == np.array([-1, 257, 257, 0])), (what, j)


def run_noguess(bm, frames, jobs, cap=None, counts=None):
    d, c = store(frames, cap)
    if counts is not None:
        c = np.asarray(counts, np.int32)
    p, n, r = bm.match(dev(d), dev(c), jobs, knn=True)
    return p.cpu().numpy(), n.cpu().numpy(), r.cpu().numpy()


# ---- no-guess ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf,nt", [(0, 5), (5, 0), (7, 1), (7, 2), (1, 1), (200, 300), (300, 200), (1500, 1500)])
def test_noguess_sizes(bm, nf, nt):
    rng = np.random.default_rng(nf * 7 + nt)
    fr, to = planted(rng, nf, nt)
    p, n, r = run_noguess(bm, [fr, to], [(0, 1), (1, 0)])
    check_job(p, n, r, 0, fr, to, what="0->1")
    check_job(p, n, r, 1, to, fr, what="1->0")


def test_noguess_crafted(bm):
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    equal = np.repeat(base[:1], 30, axis=0)                    # all-equal rows: every query ties
    claim = np.repeat(base[3:4], 12, axis=0)                   # several queries claim one train row
    claim[::3, 0] ^= 1
    frames = [base, equal, claim, base[::-1].copy()]
    jobs = [(0, 0), (1, 1), (1, 0), (0, 1), (2, 0), (3, 0), (0, 3), (2, 2)]
    p, n, r = run_noguess(bm, frames, jobs, cap=64)
    for j, (a, b) in enumerate(jobs):
        check_job(p, n, r, j, frames[a], frames[b], what=str((a, b)))
    assert n[0] == 40   # self-matching of distinct rows: each row is its own unique best


def test_noguess_64_jobs_repeating_frames(bm):
    rng = np.random.default_rng(11)
    frames = []
    for i in range(6):
        fr, _ = planted(rng, int(rng.integers(100, 700)), 0)
        frames.append(fr)
    for i in range(1, 6):                                      # make neighbouring frames share rows
        k = min(len(frames[i]), len(frames[i - 1])) // 2
        frames[i][:k] = frames[i - 1][:k]
    jobs = [(int(rng.integers(0, 6)), int(rng.integers(0, 6))) for _ in range(64)]
    p, n, r = run_noguess(bm, frames, jobs, cap=700)
    for j, (a, b) in enumerate(jobs):
        check_job(p, n, r, j, frames[a], frames[b], what=str((j, a, b)))


def test_noguess_counts_above_cap_are_clamped(bm):
    rng = np.random.default_rng(3)
    fr, to = planted(rng, 50, 50)
    d, c = store([fr, to], cap=50)
    c = np.array([50 + 1000, 1 << 30], np.int32)
    p, n, r = bm.match(dev(d), dev(c), [(0, 1)], knn=True)
    check_job(p.cpu().numpy(), n.cpu().numpy(), r.cpu().numpy(), 0, fr, to)
    c = np.array([-5, 50], np.int32)
    p, n = bm.match(dev(d), dev(c), [(0, 1)])
    assert int(n.cpu()[0]) == 0


def test_cap_one_and_cap_limit(bm):
    rng = np.random.default_rng(8)
    a = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    p, n, r = run_noguess(bm, [a, a], [(0, 1)], cap=1)
    check_job(p, n, r, 0, a, a)
    fr, to = planted(rng, 3000, 2500)
    p, n, r = run_noguess(bm, [fr, to], [(0, 1)], cap=65535)
    check_job(p, n, r, 0, fr, to, what="cap 65535")


def test_golden_descriptors_from_the_device(bm, golden, monkeypatch):
    import torch

    pattern = np.load(ROOT / "tests" / "golden" / "orb_pattern.npz")["pattern"]
    imgs = np.stack([golden["rect_l"], golden["rect_r"]])
    desc, kpts, count = bm.orb_features(dev(imgs), pattern)
    torch.cuda.synchronize()
    cn = count.cpu().numpy()
    dn, kn = desc.cpu().numpy(), kpts.cpu().numpy()
    p, n, r = bm.match(desc, count, [(0, 1), (1, 0), (0, 0)], knn=True)
    p, n, r = p.cpu().numpy(), n.cpu().numpy(), r.cpu().numpy()
    fr, to = dn[0, :cn[0]], dn[1, :cn[1]]
    check_job(p, n, r, 0, fr, to, what="golden L->R")
    check_job(p, n, r, 1, to, fr, what="golden R->L")
    check_job(p, n, r, 2, fr, fr, what="golden L->L")
    assert n[0] > 50
    # guided: the right frame's points seen from the left camera shifted by a few pixels
    xyz = np.full((2, kn.shape[1], 3), np.nan, np.float32)
    k0 = kn[0, :cn[0]]
    z = np.float32(4.0) + (k0[:, 0] % 7).astype(np.float32)
    xyz[0, :cn[0], 0] = (k0[:, 0] - K[2]) * z / K[0]
    xyz[0, :cn[0], 1] = (k0[:, 1] - K[3]) * z / K[1]
    xyz[0, :cn[0], 2] = z
    T = np.array([[1, 0, 0, -0.05, 0, 1, 0, 0.01, 0, 0, 1, 0.02]], np.float32)
    proj = bm.project_points(dev(xyz), count, [0], T, K, (W, H))
    pn = proj.cpu().numpy()
    want = ref.project(xyz[0, :cn[0]], T[0], K, W, H)
    assert np.array_equal(pn[0, :cn[0]], want, equal_nan=True)
    assert np.all(np.isnan(pn[0, cn[0]:]))
    for fu in (False, True):
        monkeypatch.setenv("SBM_CV_READING", "256" if fu else "0")
        p, n, r = bm.match_guess(desc, count, kpts, proj, [(0, 1)], knn=True)
        check_job(p.cpu().numpy(), n.cpu().numpy(), r.cpu().numpy(), 0, fr, to, pn[0, :cn[0]],
                  kn[1, :cn[1]], fused=fu, what=f"golden guided fused={fu}")


# ---- guided --------------------------------------------------------------------------------------------------------------
def edge_counts_disagree_with_1600(cands, P, Kt, fused):
    """How many radius-edge queries the device decided otherwise than `d2 < 1600` would."""
    d2 = np.array([ref.sq_dist(*P[i], *Kt[i], fused) for i in range(len(P))], np.float32)
    return int(((cands > 0) != (d2 < np.float32(1600.0))).sum())


def test_guided_radius_edges_on_the_device(bm, monkeypatch):
    """Queries whose only possible candidate sits on the radius edge (dy != 0): squared distances below 1 600 whose rounded
    square root is 40, and pairs the two readings of the sum decide differently. The device's candidate counts equal the
    restatement's under each reading, differ from `d2 < 1600`, and differ between the readings."""
    P, Kt, kinds = ref.radius_edge_cases()
    n = len(P)
    rng = np.random.default_rng(77)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d, c = store([desc, desc], cap=32)
    kp = np.zeros((2, 32, 2), np.float32)
    kp[1, :n] = Kt
    pr = np.full((1, 32, 2), np.nan, np.float32)
    pr[0, :n] = P
    cands = {}
    for fu in READINGS:
        monkeypatch.setenv("SBM_CV_READING", "256" if fu else "0")
        p, m, r = bm.match_guess(dev(d), dev(c), dev(kp), dev(pr), [(0, 1)], knn=True)
        p, m, r = p.cpu().numpy(), m.cpu().numpy(), r.cpu().numpy()
        check_job(p, m, r, 0, desc, desc, P, Kt, fused=fu, what=f"edges fused={fu}")
        cands[fu] = r[0, :n, 3]
        assert set(cands[fu].tolist()) == {0, 1}
        assert edge_counts_disagree_with_1600(cands[fu], P, Kt, fu) >= 8
    assert int((cands[False] != cands[True]).sum()) >= 8


@pytest.mark.parametrize("fused", READINGS, ids=RIDS, indirect=True)
def test_guided_crafted_and_edges(bm, fused):
    rng = np.random.default_rng(21)
    bp, bk, _ = ref.radius_edge_cases()                         # at 256 and beyond: far from the random points below
    nb = len(bp)
    fr, to = planted(rng, 120, 150)
    proj = rng.uniform(0, 150, (120, 2)).astype(np.float32)   # with the +-50 below, every point stays below 200
    kto = rng.uniform(0, 150, (150, 2)).astype(np.float32)
    proj[:nb] = bp
    kto[:nb] = bk
    proj[nb: nb + 10] = np.nan                                 # not queries
    kto[nb + 10: nb + 40] = proj[nb + 10: nb + 40] + rng.uniform(-50, 50, (30, 2)).astype(np.float32)
    to[nb + 10: nb + 40] = fr[nb + 10: nb + 40]
    kto[nb + 40: nb + 45] = proj[nb + 40: nb + 45]            # exactly one candidate, no NNDR
    d, c = store([fr, to], cap=160)
    kp = np.zeros((2, 160, 2), np.float32)
    kp[1, :150] = kto
    pr = np.full((2, 160, 2), np.nan, np.float32)
    pr[0, :120] = proj
    pr[1, :120] = proj[::-1]
    p, n, r = bm.match_guess(dev(d), dev(c), dev(kp), dev(pr), [(0, 1), (0, 1)], knn=True)
    p, n, r = p.cpu().numpy(), n.cpu().numpy(), r.cpu().numpy()
    check_job(p, n, r, 0, fr, to, proj, kto, fused=fused, what="crafted")
    check_job(p, n, r, 1, fr, to, proj[::-1].copy(), kto, fused=fused, what="crafted reversed")
    # the radius-edge queries: the device does not decide them as d2 < 1600 would
    assert edge_counts_disagree_with_1600(r[0, :nb, 3], bp, bk, fused) >= 8


@pytest.mark.parametrize("fused", READINGS, ids=RIDS, indirect=True)
def test_guided_synthetic_at_the_cap(bm, fused):
    rng = np.random.default_rng(33)
    nframe, cap = 4, 1500
    frames, kps = [], []
    for i in range(nframe):
        fr, _ = planted(rng, cap, 0)
        frames.append(fr)
        kps.append(rng.uniform(0, 640, (cap, 2)).astype(np.float32))
    for i in range(1, nframe):
        frames[i][:700] = frames[i - 1][:700]
        kps[i][:700] = kps[i - 1][:700] + rng.normal(0, 15, (700, 2)).astype(np.float32)
    d, c = store(frames, cap)
    kp = np.stack(kps)
    jobs = [(i, (i + 1) % nframe) for i in range(nframe)] * 16      # m = 64
    pr = np.stack([kps[a] + rng.normal(0, 3, (cap, 2)).astype(np.float32) for a, _ in jobs])
    p, n, r = bm.match_guess(dev(d), dev(c), dev(kp), dev(pr), jobs, knn=True)
    p, n, r = p.cpu().numpy(), n.cpu().numpy(), r.cpu().numpy()
    for j in (0, 1, 2, 3, 37, 63):
        a, b = jobs[j]
        check_job(p, n, r, j, frames[a], frames[b], pr[j], kps[b], fused=fused, what=f"job {j}")
    p1, n1, r1 = bm.match_guess(dev(d), dev(c), dev(kp), dev(pr[:1]), jobs[:1], knn=True)
    assert np.array_equal(p1.cpu().numpy()[0], p[0]) and np.array_equal(r1.cpu().numpy()[0], r[0])


def test_projection_edges(bm):
    T = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    Kx = (100.0, 100.0, 50.0, 40.0)
    pts = np.array([
        [np.nan, 0, 1], [0, 0, -1], [0, 0, 0], [0, 0, -0.0], [-0.5, 0, 1], [0.5, 0.1, 1], [0.49, 0.1, 1], [0.1, 0.2, 2],
        [0.1, -0.4, 1], [0.1, 0.39, 1], [0.1, 0.38, 1], [1e-30, 1e-30, 1e-30], [3, 2, 1e9], [-0.49, 0.1, 1],
    ], np.float32)
    xyz = np.full((1, 32, 3), 7.0, np.float32)
    xyz[0, :len(pts)] = pts
    cnt = np.array([len(pts)], np.int32)
    Ts = np.stack([T, np.array([0.9, -0.1, 0.05, 0.3, 0.1, 0.95, 0, -0.2, 0.01, 0, 1, 0.5], np.float32)])
    proj = bm.project_points(dev(xyz), dev(cnt), [0, 0], Ts, Kx, (101, 81)).cpu().numpy()
    for j in range(2):
        want = ref.project(pts, Ts[j], Kx, 101, 81)
        assert np.array_equal(proj[j, :len(pts)], want, equal_nan=True), j
        assert np.all(np.isnan(proj[j, len(pts):]))
    want = ref.project(pts, T, Kx, 101, 81)
    assert np.isnan(want[:4]).all() and np.isnan(want[4]).all() and np.isnan(want[5]).all()   # u = 0 and u = W - 1 excluded


# ---- host, asynchronous and C++ entry points ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", READINGS, ids=RIDS, indirect=True)
def test_host_forms(bm, fused):
    rng = np.random.default_rng(44)
    fr, to = planted(rng, 300, 280)
    wide = np.zeros((280, 48), np.uint8)
    wide[:, :32] = to
    got = bm.match_host(fr, wide[:, :32])
    assert np.array_equal(got, ref.match(fr, to)[0])
    xyz = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    xyz[:, 2] = rng.uniform(0.5, 4, 300)
    xyz[::17] = np.nan
    T = np.array([0.99, -0.02, 0.01, 0.05, 0.02, 0.99, 0, -0.03, -0.01, 0, 1, 0.1], np.float32)
    Kx = (300.0, 300.0, 320.0, 240.0)
    proj = ref.project(xyz, T, Kx, W, H)
    kto = np.where(np.isnan(proj[:280]), 100.0, proj[:280]).astype(np.float32) + rng.normal(0, 8, (280, 2)).astype(np.float32)
    got = bm.match_guess_host(xyz, kto, fr, to, T, Kx, (W, H))
    assert np.array_equal(got, ref.match(fr, to, proj, kto, fused=fused)[0])
    assert bm.match_host(fr[:0], to).shape == (0, 2) and bm.match_host(fr, to[:1]).shape == (0, 2)


def test_async_then_stream_sync(bm):
    import torch

    rng = np.random.default_rng(55)
    fr, to = planted(rng, 900, 1000)
    d, c = store([fr, to])
    dd, dc = dev(d), dev(c)
    torch.cuda.synchronize()
    p, n, r = bm.match(dd, dc, [(0, 1)] * 3, knn=True, sync=False)
    torch.cuda.ExternalStream(bm.stream(), device="cuda:0").synchronize()
    check_job(p.cpu().numpy(), n.cpu().numpy(), r.cpu().numpy(), 2, fr, to)
    bm.synchronize()


def test_profile_names(bm):
    rng = np.random.default_rng(1)
    fr, to = planted(rng, 100, 100)
    d, c = store([fr, to])
    bm.set_profiling(1)
    try:
        bm.match(dev(d), dev(c), [(0, 1)])
        prof = bm.match_profile()
    finally:
        bm.set_profiling(0)
    assert prof["match_knn"] > 0 and prof["match_total"] >= prof["match_knn"]


def test_limits_on_the_device(bm, pkg):
    import torch

    L, h = bm._L, bm._h
    mp = pkg.match_params()
    mib = 1 << 20
    buf = torch.zeros(4 * mib, dtype=torch.uint8, device="cuda:0")
    a = buf.data_ptr()
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    jobs = np.zeros(2 * 65536, np.int32)

    def call(n, m, cap, desc=a, pairs=a + mib, npairs=a + 2 * mib, knn=None):
        return L.sbm_match_device(h, n, m, jobs.ctypes.data, desc, cnt.data_ptr(), cap, ctypes.byref(mp), pairs, npairs, knn, 1)

    assert call(1, 1, 1) == 0
    assert call(1, 1, 0) == -2
    assert call(1, 1, 65536) == -2
    assert call(1, 65535, 1) == 0                     # the largest job count, cap 1: 512 KiB of pairs, 256 KiB of counts
    assert call(1, 65536, 1) == -23
    assert call(0, 1, 1) == -24
    jobs[1] = 1
    assert call(1, 1, 1) == -2                        # to frame 1 of a 1-frame store
    assert call(2, 1, 1) == 0
    jobs[1] = 0
    assert call(1, 1, 1, desc=a + 16) == 0
    assert call(1, 1, 1, desc=a + 8) == -23
    assert call(1, 1, 1, pairs=a + mib + 4) == -23
    assert call(1, 1, 1, npairs=a + 2 * mib + 2) == -23
    assert call(1, 1, 1, knn=a + 3 * mib + 8) == -23
    assert call(1, 1, 1, knn=a + 3 * mib + 16) == 0

    def guess(kpts=a + 3 * mib, proj=a + 3 * mib + 256):
        return L.sbm_match_guess_device(h, 1, 1, jobs.ctypes.data, a, cnt.data_ptr(), 1, kpts, proj, ctypes.byref(mp), a + mib,
                                        a + 2 * mib, None, 1)

    assert guess() == 0
    assert guess(kpts=a + 3 * mib + 8) == 0
    assert guess(kpts=a + 3 * mib + 4) == -23
    assert guess(proj=a + 3 * mib + 264) == 0
    assert guess(proj=a + 3 * mib + 260) == -23
    T = np.zeros(12 * 2, np.float32)
    Kd = np.array([1.0, 1.0, 0.0, 0.0])
    fr = np.zeros(2, np.int32)

    def proj(n, m, cap, w=8, hh=8, out=a + mib, xyz=a):
        return L.sbm_project_points_device(h, n, m, fr.ctypes.data, xyz, cnt.data_ptr(), cap, T.ctypes.data, Kd.ctypes.data, w, hh,
                                           out, 1)

    assert proj(1, 1, 1) == 0
    assert proj(1, 1, 65535) == 0
    assert proj(1, 1, 65536) == -2
    assert proj(1, 1, 1, w=0) == -2
    assert proj(1, 1, 1, out=a + mib + 4) == -23
    assert proj(1, 1, 1, xyz=a + 2) == -23
    fr[0] = 1
    assert proj(1, 1, 1) == -2
    assert proj(2, 1, 1) == 0


def test_cpp_callsite_through_the_adaptor(tmp_path):
    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")]
    exe, r = build_callsite(tmp_path, "match_callsite_main.cpp", extra, flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(66)
    fr, to = planted(rng, 400, 350)
    xyz = rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    xyz[:, 2] = rng.uniform(0.5, 4, 400)
    T = np.array([1, 0, 0, 0.02, 0, 1, 0, 0, 0, 0, 1, 0.05], np.float32)
    Kx = np.array([300.0, 300.0, 320.0, 240.0])
    proj = ref.project(xyz, T, Kx, W, H)
    kto = np.where(np.isnan(proj[:350]), 50.0, proj[:350]).astype(np.float32) + rng.normal(0, 10, (350, 2)).astype(np.float32)
    files = {}
    for name, arr in (("df", fr), ("dt", to), ("xyz", xyz), ("kt", kto), ("T", T), ("K", Kx.astype(np.float64))):
        files[name] = tmp_path / f"{name}.raw"
        arr.tofile(files[name])
    out = tmp_path / "out.raw"
    r = subprocess.run([str(exe), *(str(files[k]) for k in ("df", "dt", "xyz", "kt", "T", "K")), str(W), str(H), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    o = np.fromfile(out, np.int32)
    k0 = o[0]
    got0 = o[1:1 + 2 * k0].reshape(-1, 2)
    k1 = o[1 + 2 * k0]
    got1 = o[2 + 2 * k0:2 + 2 * k0 + 2 * k1].reshape(-1, 2)
    assert np.array_equal(got0, ref.match(fr, to)[0])
    assert np.array_equal(got1, ref.match(fr, to, proj, kto)[0])
