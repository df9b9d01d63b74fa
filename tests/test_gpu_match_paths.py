"""The keypoint matcher (u96-slam_amd/csrc/sbm_match.hip) on every path its host code can take, bit for bit against the CPU
restatement (oracle/match_ref.c): both sides of every slice boundary in both forms, the widest store, counts against the plan,
scratch left by a larger call, every launch after the first, NNDR values and radii other than the defaults, and claims from
different blocks. Each test reads sbm_match_plan first and asserts the shape it was written for; the inputs come from
tests/match_cases.py, whose guarantees tests/test_match_cases_restatement.py checks without a device."""
import numpy as np
import pytest

import match_cases as mc
import match_ref as ref
from gpu_support import bm, dev  # noqa: F401
from test_gpu_match import H, K, READINGS, RIDS, W, check_job, fused, planted  # noqa: F401

pytestmark = pytest.mark.gpu


def plan_is(pkg, cap, m, nslice, slice_rows, launches=None):
    pl = pkg.match_plan(cap, m)
    assert (pl.nslice, pl.slice_rows) == (nslice, slice_rows), (cap, m, pl.nslice, pl.slice_rows)
    assert pl.jobs_per_launch == min(m, 64)
    if launches is not None:
        assert pl.launches == launches
    return pl


def pack(jobs, cap):
    """Jobs -> a store: every distinct from-array one frame, every job its own to-frame. Descriptor slots past a count hold a
    marker; in the guided form the from-frames' keypoint slots (never to be read) and the to-frames' slots past the count hold
    the job's first finite projection, which would be a candidate. Returns (desc, count, (from, to) list, kpts, proj)."""
    frames, index, pairs = [], {}, []
    for j in jobs:
        if id(j.frm) not in index:
            index[id(j.frm)] = len(frames)
            frames.append(j.frm)
        pairs.append((index[id(j.frm)], len(frames)))
        frames.append(j.to)
    n = len(frames)
    d = np.full((n, cap, 32), 0xA5, np.uint8)
    c = np.zeros(n, np.int32)
    for i, f in enumerate(frames):
        d[i, :len(f)] = f
        c[i] = len(f)
    kp = pr = None
    if jobs[0].proj is not None:
        kp = np.zeros((n, cap, 2), np.float32)
        pr = np.full((len(jobs), cap, 2), np.nan, np.float32)
        for k, (j, (a, b)) in enumerate(zip(jobs, pairs)):
            finite = j.proj[np.isfinite(j.proj).all(1)]
            lure = finite[0] if len(finite) else np.zeros(2, np.float32)
            kp[a] = lure
            kp[b] = lure
            kp[b, :len(j.kto)] = j.kto
            pr[k, :len(j.proj)] = j.proj
    return d, c, pairs, kp, pr


def run(bm, jobs, cap, params=None, each=False):
    """All jobs in one call (or, with each, one call of m = 1 per job over one upload). Returns (pairs, npairs, records)."""
    d, c, pairs, kp, pr = pack(jobs, cap)
    dd, dc = dev(d), dev(c)
    guided = kp is not None
    if guided:
        dk, dp = dev(kp), dev(pr)
    calls = [[k] for k in range(len(jobs))] if each else [list(range(len(jobs)))]
    outs = []
    for ks in calls:
        jl = [pairs[k] for k in ks]
        if guided:
            o = bm.match_guess(dd, dc, dk, dp[ks[0]:ks[-1] + 1].contiguous(), jl, params=params, knn=True)
        else:
            o = bm.match(dd, dc, jl, params=params, knn=True)
        outs.append([t.cpu().numpy() for t in o])
    return [np.concatenate([o[i] for o in outs]) for i in range(3)]


def check_all(out, jobs, fused=False, **kw):
    p, n, r = out
    assert len(n) == len(jobs)
    for k, j in enumerate(jobs):
        check_job(p, n, r, k, j.frm, j.to, j.proj, j.kto, fused=fused, what=j.what, **kw)


# ---- 1, 2: slice boundaries ------------------------------------------------------------------------------------------------
def test_slice_boundaries_noguess(bm, pkg):
    jobs = mc.pairs_and_ties(300, 64) + mc.triples(300, 64)
    assert len(jobs) == 135 + 30
    plan_is(pkg, 300, len(jobs), 5, 64, launches=3)
    check_all(run(bm, jobs, 300), jobs)
    ties = [j for j in jobs if j.tie]
    plan_is(pkg, 300, len(ties), 5, 64)
    out = run(bm, ties, 300, params=pkg.match_params(nndr=1.0))
    check_all(out, ties, nndr=1.0)
    assert not np.isin(out[0][:, :, 0], mc.QROWS).any()              # a tied query is in no pair even at nndr 1


def test_slice_boundaries_noguess_two_stages_per_slice(bm, pkg):
    plan_is(pkg, 2100, 1, 17, 128)
    jobs = mc.pairs_and_ties(2100, 128, spot_pairs=mc.sparse_spot_pairs(2100, 128))
    jobs += mc.triples(2100, 128, spot_sets=mc.spot_triples(2100, 128)[::5])
    check_all(run(bm, jobs, 2100, each=True), jobs)


@pytest.mark.parametrize("fused", READINGS, ids=RIDS, indirect=True)
def test_slice_boundaries_guided(bm, pkg, fused):
    jobs = mc.guided_slices(300, 64)
    plan_is(pkg, 300, len(jobs), 5, 64)
    out = run(bm, jobs, 300)
    check_all(out, jobs, fused=fused)
    plan_is(pkg, 300, 1, 5, 64)
    check_all(run(bm, jobs[:12], 300, each=True), jobs[:12], fused=fused)


# ---- 3: the widest store ---------------------------------------------------------------------------------------------------
def test_widest_store(bm, pkg):
    plan_is(pkg, 65535, 1, 8, 8192)
    job = mc.widest_store()
    out = run(bm, [job], 65535)
    check_all(out, [job])
    assert out[1][0] == 16


# ---- 4: counts against the plan --------------------------------------------------------------------------------------------
def test_counts_against_the_plan(bm, pkg):
    cap, nts, nfs = 300, [1, 2, 63, 64, 65, 128, 129, 299, 300], [1, 64, 65, 300]
    rng = np.random.default_rng(41)
    fr, to = planted(rng, cap, cap, flips=(3, 20, 60))
    frames, counts = [], []
    for nf in nfs:
        frames.append(fr)
        counts.append(nf)
    for nt in nts:
        t = to.copy()
        t[nt:] = fr[:cap - nt]          # past the count: exact copies of the first queries, which must never be read
        frames.append(t)
        counts.append(nt)
    jobs = [(a, len(nfs) + b) for a in range(len(nfs)) for b in range(len(nts))]
    plan_is(pkg, cap, len(jobs), 5, 64)
    d = np.stack(frames)
    p, n, r = bm.match(dev(d), dev(np.array(counts, np.int32)), jobs, knn=True)
    p, n, r = p.cpu().numpy(), n.cpu().numpy(), r.cpu().numpy()
    for k, (a, b) in enumerate(jobs):
        check_job(p, n, r, k, frames[a][:counts[a]], frames[b][:counts[b]], what=f"nf {counts[a]} nt {counts[b]}")
    assert n.max() > 50


# ---- 5: scratch left by a larger call --------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided,reading", [(False, False), (True, False), (True, True)], ids=["noguess", "guided", "guided_fused"])
def test_scratch_of_a_larger_call_is_not_read(bm, pkg, monkeypatch, guided, reading):
    monkeypatch.setenv("SBM_CV_READING", "256" if reading else "0")
    fused = reading
    cap = 300
    plan_is(pkg, cap, 1, 5, 64)
    rng = np.random.default_rng(51)
    fr, to = planted(rng, cap, cap, flips=(3, 20, 60))
    big = to.copy()
    big[128:] = fr[np.arange(cap - 128) % 70]      # slices 2 to 4 hold exact copies of queries 0..69: their records have d0 = 0
    proj = kbig = ksmall = None
    if guided:
        proj = rng.uniform(100, 120, (cap, 2)).astype(np.float32)      # all within the radius of one another
        kbig = rng.uniform(100, 120, (cap, 2)).astype(np.float32)
        ksmall = kbig[:100]
    first = mc.Job(fr, big, proj, kbig, what="the larger call")
    out = run(bm, [first], cap)
    check_all(out, [first], fused=fused)
    assert np.all(out[2][0, :70, 1] == 0) and np.all(out[2][0, :70, 0] >= 128)
    second = mc.Job(fr[:70], to[:100], None if proj is None else proj[:70], ksmall, what="the smaller call")
    out = run(bm, [second], cap)
    check_all(out, [second], fused=fused)
    assert np.all(out[2][0, :70, 1] >= 3)


# ---- 6: launches after the first -------------------------------------------------------------------------------------------
def split_frames(rng, nframe, cap):
    """Frames of differing counts whose first halves are rows of one base frame, seen a few pixels from the base's places."""
    base, base_kp = planted(rng, cap, 0)[0], rng.uniform(0, 320, (cap, 2)).astype(np.float32)
    frames, kps = [], []
    for i in range(nframe):
        n = cap if i % 3 == 0 else int(rng.integers(cap // 2, cap))
        f, kp = planted(rng, n, 0)[0], rng.uniform(0, 320, (n, 2)).astype(np.float32)
        f[:n // 2] = base[:n // 2]
        kp[:n // 2] = base_kp[:n // 2] + rng.normal(0, 6, (n // 2, 2)).astype(np.float32)
        frames.append(f)
        kps.append(kp)
    return frames, kps


@pytest.mark.parametrize("fused", READINGS, ids=RIDS, indirect=True)
@pytest.mark.parametrize("cap,m,nslice,launches", [(200, 130, 4, 3), (300, 65, 5, 2)])
def test_launch_splits(bm, pkg, cap, m, nslice, launches, fused):
    plan_is(pkg, cap, m, nslice, 64, launches=launches)
    rng = np.random.default_rng(cap + m)
    frames, kps = split_frames(rng, 7, cap)
    pairs = [(j % 7, (3 * j + 1) % 7) for j in range(m)]
    assert all(pairs[j] != pairs[j + 64] for j in range(m - 64))    # the same in-launch position, another job
    jobs = []
    for a, b in pairs:
        na = len(frames[a])
        pr = (kps[a] + rng.normal(0, 6, (na, 2))).astype(np.float32)
        pr[rng.integers(0, na, 5)] = np.nan
        jobs.append(mc.Job(frames[a], frames[b], pr, kps[b], what=f"{a}->{b}"))
    plain = [mc.Job(j.frm, j.to, what=j.what) for j in jobs]
    out = run(bm, plain, cap)
    check_all(out, plain)
    assert (out[1] > 0).sum() > m // 2
    out = run(bm, jobs, cap)
    check_all(out, jobs, fused=fused)
    assert (out[1] > 0).sum() > m // 2
    assert any(not np.array_equal(out[2][j], out[2][j + 64]) for j in range(m - 64))


@pytest.mark.parametrize("m", [32, 33, 64, 65])
def test_projection_launch_splits(bm, pkg, m):
    cap = 40
    assert pkg.match_plan(cap, m).proj_launches == -(-m // 32)
    rng = np.random.default_rng(m)
    cnt = rng.integers(1, cap + 1, m).astype(np.int32)
    cnt[:2] = (cap, 0)
    xyz = rng.uniform(-2, 2, (m, cap, 3)).astype(np.float32)
    xyz[:, :, 2] = rng.uniform(0.5, 6, (m, cap))
    xyz[:, ::9] = np.nan
    frm = [(7 * j + 3) % m for j in range(m)]                         # a permutation: a distinct from-frame per job
    assert len(set(frm)) == m
    T = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (m, 1))
    T += rng.normal(0, 0.05, (m, 12)).astype(np.float32)
    proj = bm.project_points(dev(xyz), dev(cnt), frm, T, K, (W, H)).cpu().numpy()
    valid = 0
    for j in range(m):
        k = cnt[frm[j]]
        want = ref.project(xyz[frm[j], :k], T[j], K, W, H)
        assert np.array_equal(proj[j, :k], want, equal_nan=True), j
        assert np.all(np.isnan(proj[j, k:])), j
        valid += int(np.isfinite(want[:, 0]).sum())
    assert valid > m


# ---- 7, 8: parameters other than the defaults ------------------------------------------------------------------------------
@pytest.mark.parametrize("nndr", mc.NNDRS)
def test_nndr_boundaries(bm, pkg, nndr):
    jobs = mc.nndr_boundaries(nndr)
    pl = plan_is(pkg, 2, len(jobs), 1, 64)
    assert pl.launches >= 7
    out = run(bm, jobs, 2, params=pkg.match_params(nndr=nndr))
    check_all(out, jobs, nndr=nndr)
    held = np.array([0 in out[0][k, :out[1][k], 0] for k in range(len(jobs))])
    assert np.array_equal(held, np.array([j.accept for j in jobs]))


@pytest.mark.parametrize("fused", READINGS, ids=RIDS, indirect=True)
@pytest.mark.parametrize("radius", mc.RADII_BELOW + mc.RADII_AT)
def test_radii(bm, pkg, radius, fused):
    job, at, below = mc.radius_threshold_cases(radius, fused)
    out = run(bm, [job], 8, params=pkg.match_params(radius=radius))
    check_all(out, [job], fused=fused, radius=radius)
    cands = out[2][0, :, 3]
    want = ref.match(job.frm, job.to, job.proj, job.kto, radius=radius, fused=fused)[1][:, 3]
    assert np.array_equal(cands, want) and set(cands.tolist()) == {0, 1}
    d2 = np.array([ref.sq_dist(*job.proj[i], *job.kto[i], fused) for i in range(len(cands))], np.float32)
    naive = d2 < mc.square_f32(radius)
    if radius in mc.RADII_BELOW:
        assert np.all((cands[at] > 0) != naive[at])                  # `d2 < fl(r * r)` would take every T(r) query
    assert np.array_equal(cands[below] > 0, naive[below])


# ---- 9: claims from different blocks ---------------------------------------------------------------------------------------
def test_cross_block_claims(bm, pkg):
    job = mc.cross_block_claims()
    plan_is(pkg, 600, 1, 10, 64)
    out = run(bm, [job], 600)
    check_all(out, [job])
    assert out[1][0] == 300
