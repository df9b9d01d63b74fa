"""The CPU restatement of matchingNoGuess / matchingGuess (oracle/match_ref.c) held to its literal numpy transcription of the
Registration.cpp loops (match_ref.py), and the facts the restatement rests on: the NNDR rule as integers, the radius test at
squared distances around 1 600 under both readings, and the projection's edge cases."""
import numpy as np
import pytest

import match_ref as ref


def same(a, b, guided):
    pa, ra = a
    pb, rb = b
    assert np.array_equal(pa, pb)
    assert np.array_equal(ra[:, 1:], rb[:, 1:])
    # the best index may differ only where the two best tie, and NNDR rejects every such query
    tie = ra[:, 1] == ra[:, 2]
    assert np.array_equal(ra[~tie, 0], rb[~tie, 0])
    if not guided:
        assert np.array_equal(ra[:, 0], rb[:, 0])


def near(rng, n, nt):
    to = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    fr = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for i in range(0, n, 2):
        if nt:
            bits = np.unpackbits(to[rng.integers(0, nt)])
            bits[rng.choice(256, int(rng.integers(0, 40)), replace=False)] ^= 1
            fr[i] = np.packbits(bits)
    return fr, to


@pytest.mark.parametrize("seed", range(4))
def test_random_and_planted(seed):
    rng = np.random.default_rng(seed)
    fr, to = near(rng, 120, 150)
    same(ref.match(fr, to), ref.match_np(fr, to), False)
    same(ref.match(to, fr), ref.match_np(to, fr), False)
    fr2 = rng.integers(0, 256, (60, 32), dtype=np.uint8)
    same(ref.match(fr2, to), ref.match_np(fr2, to), False)


@pytest.mark.parametrize("nt", [0, 1, 2])
def test_small_train_sets(nt):
    rng = np.random.default_rng(nt)
    fr, to = near(rng, 9, nt)
    p, r = ref.match(fr, to)
    same((p, r), ref.match_np(fr, to), False)
    if nt < 2:
        assert len(p) == 0           # nt == 1 is defined as no pairs
    assert np.all(r[:, 3] == nt)


def test_all_equal_rows_and_shared_claims():
    rng = np.random.default_rng(9)
    base = rng.integers(0, 256, (20, 32), dtype=np.uint8)
    eq = np.repeat(base[:1], 10, axis=0)
    p, r = ref.match(eq, eq)
    assert len(p) == 0 and np.all(r[:, 1] == 0) and np.all(r[:, 0] == 0)   # ties: lower index first, NNDR rejects
    same((p, r), ref.match_np(eq, eq), False)
    claim = np.repeat(base[2:3], 8, axis=0)
    claim[1::2, 5] ^= 3
    p, r = ref.match(claim, base)
    assert p.tolist() == [[0, 2]]                    # the first claimant keeps row 2; the others do not fall back
    same((p, r), ref.match_np(claim, base), False)


def test_self_matching():
    rng = np.random.default_rng(12)
    a = rng.integers(0, 256, (80, 32), dtype=np.uint8)
    p, _ = ref.match(a, a)
    assert p.tolist() == [[i, i] for i in range(80)]
    same(ref.match(a, a), ref.match_np(a, a), False)


def test_nndr_table_equals_the_integer_rule():
    d0, d1 = np.meshgrid(np.arange(257), np.arange(257), indexing="ij")
    f = d0.astype(np.float32) < np.float32(0.8) * d1.astype(np.float32)
    assert np.array_equal(f, 5 * d0 < 4 * d1)
    assert not f[np.arange(257), np.arange(257)].any()     # a tie between the two best is never accepted


def radius_cases():
    """(projected point, to-keypoint) pairs at squared distances just below, at and above 1 600."""
    P, Kt = [], []
    b = np.float32(200.0)
    r = np.float32(40.0)
    for k in range(-3, 4):
        x = r
        for _ in range(abs(k)):
            x = np.nextafter(x, np.float32(np.inf) if k > 0 else np.float32(0))
        P.append((b, b))
        Kt.append((b + x, b))
    d2 = np.float32(1600.0)
    for _ in range(4):
        d2 = np.nextafter(d2, np.float32(0))
        P.append((b, b))
        Kt.append((b + np.float32(np.sqrt(np.float64(d2))), b))
    P.append((np.float32(130), np.float32(125)))
    Kt.append((np.float32(106), np.float32(93)))                 # 24^2 + 32^2 == 1600
    P.append((np.float32(0.1), np.float32(0.2)))
    Kt.append((np.float32(0.1 + 28.284271), np.float32(0.2 + 28.284271)))
    return np.array(P, np.float32), np.array(Kt, np.float32)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_radius_edges(fused):
    P, Kt = radius_cases()
    rng = np.random.default_rng(1)
    fr = rng.integers(0, 256, (len(P), 32), dtype=np.uint8)
    to = fr.copy()
    for i in range(len(P)):              # one query per to-keypoint: project each query onto its own candidate only
        pr = np.full((len(P), 2), np.nan, np.float32)
        pr[i] = P[i]
        a, b = ref.match(fr, to, pr, Kt, fused=fused), ref.match_np(fr, to, pr, Kt, fused=fused)
        same(a, b, True)
    pr = P.copy()
    p_c, r_c = ref.match(fr, to, pr, Kt, fused=fused)
    same((p_c, r_c), ref.match_np(fr, to, pr, Kt, fused=fused), True)
    # the rounded square root, not d2 < 1600: some d2 below 1600 are outside the radius
    d2 = np.float32(1600.0)
    outside = 0
    for _ in range(4):
        d2 = np.nextafter(d2, np.float32(0))
        outside += not (np.sqrt(d2, dtype=np.float32) < np.float32(40.0))
    assert outside >= 1


def test_fused_and_unfused_readings_differ_somewhere():
    rng = np.random.default_rng(2)
    dx = rng.uniform(20, 40, 20000).astype(np.float32)
    dy = np.sqrt(np.float32(1600.0) - dx * dx).astype(np.float32)
    unf = (dx * dx + dy * dy).astype(np.float32)
    fus = np.array([ref.fma_f32(b, b, np.float32(a * a)) for a, b in zip(dx[:3000], dy[:3000])], np.float32)
    assert (unf[:3000] != fus).any()


def test_guided_random():
    rng = np.random.default_rng(4)
    fr, to = near(rng, 150, 170)
    pr = rng.uniform(0, 120, (150, 2)).astype(np.float32)
    kt = rng.uniform(0, 120, (170, 2)).astype(np.float32)
    pr[::11] = np.nan
    for fused in (False, True):
        same(ref.match(fr, to, pr, kt, fused=fused), ref.match_np(fr, to, pr, kt, fused=fused), True)
    same(ref.match(fr, to[:0], pr, kt[:0]), ref.match_np(fr, to[:0], pr, kt[:0]), True)
    same(ref.match(fr, to[:1], pr, kt[:1]), ref.match_np(fr, to[:1], pr, kt[:1]), True)


def test_projection_edges():
    T = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    K = (100.0, 100.0, 50.0, 40.0)
    pts = np.array([
        [np.nan, 0, 1],        # NaN point
        [0, 0, -1],            # zc < 0
        [0, 0, 0],             # Z == 0: inv = 1, zc = +0 (not > 0)
        [0, 0, -0.0],          # zc = -0
        [-0.5, 0, 1],          # u == 0 exactly
        [0.5, 0.1, 1],         # u == W - 1 exactly (W = 101)
        [0.49, 0.1, 1],        # inside
        [0.1, -0.4, 1],        # v == 0
        [0.1, 0.4, 1],         # v == H - 1 (H = 81)
        [0.1, 0.2, 2],
        [1e-30, 1e-30, 1e-30],  # zc > 0 but u = 150: outside
    ], np.float32)
    c, n = ref.project(pts, T, K, 101, 81), ref.project_np(pts, T, K, 101, 81)
    assert np.array_equal(c, n, equal_nan=True)
    valid = ~np.isnan(c[:, 0])
    assert valid.tolist() == [False, False, False, False, False, False, True, False, False, True, False]
    T2 = np.array([0.9, -0.1, 0.05, 0.3, 0.1, 0.95, 0, -0.2, 0.01, 0, 1, 0.5], np.float32)
    rng = np.random.default_rng(7)
    xyz = rng.uniform(-2, 2, (500, 3)).astype(np.float32)
    assert np.array_equal(ref.project(xyz, T2, K, 101, 81), ref.project_np(xyz, T2, K, 101, 81), equal_nan=True)


def test_radius_edge_cases_tell_the_readings_apart():
    """Pairs with dy != 0 on the radius edge: under each reading some squared distances lie below 1 600 although their rounded
    square root is 40 (outside), and some pairs are inside under one reading and outside under the other. The C restatement
    and the numpy transcription decide every one of them alike, under both readings."""
    P, Kt, kinds = ref.radius_edge_cases()
    n = len(P)
    assert n == 24
    d2 = {fu: np.array([ref.sq_dist(*P[i], *Kt[i], fu) for i in range(n)], np.float32) for fu in (False, True)}
    ins = {fu: np.array([ref.inside(v) for v in d2[fu]]) for fu in (False, True)}
    for fu in (False, True):
        assert ((d2[fu] < np.float32(1600.0)) & ~ins[fu]).sum() >= 8      # d2 < 1600 would take these; sqrtf does not
    assert (ins[False] != ins[True]).sum() >= 8
    assert (ins[False] & ~ins[True]).any() or (~ins[False] & ins[True]).any()
    rng = np.random.default_rng(3)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for fu in (False, True):
        pc, rc = ref.match(desc, desc, P, Kt, fused=fu)
        pn, rn = ref.match_np(desc, desc, P, Kt, fused=fu)
        assert np.array_equal(pc, pn) and np.array_equal(rc, rn)
        assert np.array_equal(rc[:, 3], ins[fu].astype(np.int32))       # one candidate per query, decided by the edge
    assert not np.array_equal(ref.match(desc, desc, P, Kt)[1][:, 3], ref.match(desc, desc, P, Kt, fused=True)[1][:, 3])
