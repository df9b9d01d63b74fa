"""The case builders of tests/match_cases.py held to the properties they promise, with the CPU restatement alone (ref.match, and
its numpy transcription ref.match_np on a subset): the GPU tests built on them cannot pass because an input missed its path."""
import numpy as np
import pytest

import match_cases as mc
import match_ref as ref

SHAPES = [(300, 64), (2100, 128)]     # (nt = cap, slice_rows) of the plans the GPU tests run them at


def test_spots():
    assert mc.spots(300, 64) == [0, 63, 64, 127, 128, 191, 192, 255, 256, 299]
    assert mc.spots(64, 64) == [0, 63] and mc.spots(65, 64) == [0, 63, 64] and mc.spots(1, 64) == [0]
    s = mc.spots(65535, 8192)
    assert len(s) == 16 and s[-1] == 65534 and s[1:3] == [8191, 8192]


@pytest.mark.parametrize("nt,rows", SHAPES)
def test_pairs_and_ties(nt, rows):
    jobs = mc.pairs_and_ties(nt, rows, spot_pairs=mc.sparse_spot_pairs(nt, rows) if nt == 2100 else None)
    ties = [j for j in jobs if j.tie]
    assert ties and len(ties) < len(jobs)
    if nt == 300:
        assert len(jobs) == 90 + 45
    for k, j in enumerate(jobs):
        mc.verify(j)
        if j.tie:
            p, r = mc.verify(j, nndr=1.0)            # d0 == d1: rejected even at nndr 1
            assert 0 not in p[:, 0] and 64 not in p[:, 0]
        if k % 20 == 0:
            mc.verify(j, match=ref.match_np)
    # both orders across every slice boundary, and pairs far apart
    seen = {tuple(j.rec[0][:1]) for j in jobs}
    assert len(seen) >= 10


@pytest.mark.parametrize("nt,rows", SHAPES)
def test_triples(nt, rows):
    sets = mc.spot_triples(nt, rows)
    if nt == 2100:
        sets = sets[::5]
    jobs = mc.triples(nt, rows, spot_sets=sets)
    assert len(jobs) == 6 * len(sets)
    later = 0
    for k, j in enumerate(jobs):
        _, r = mc.verify(j)
        assert r[0, 2] == 2 and r[64, 2] == 2
        if k % 12 == 0:
            mc.verify(j, match=ref.match_np)
    for sp in sets[1:]:
        assert sp[0] // rows < sp[1] // rows == sp[2] // rows      # both leaders in one later slice, the third before it
        later += 1
    assert later >= 2


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_guided_slices(fused):
    jobs = mc.guided_slices(300, 64)
    kinds = {j.what.split()[1] for j in jobs}
    assert kinds == {"none", "one", "two"}
    for k, j in enumerate(jobs):
        p, r = mc.verify(j, fused=fused)
        assert np.all(r[1:64] == np.array(mc.NONE))               # only the query rows have candidates
        assert all(t >= 64 for _, t in p)                         # and only in late slices
        if k % 6 == 0:
            mc.verify(j, fused=fused, match=ref.match_np)
    two = [j for j in jobs if " two " in j.what]
    assert any(j.pair[0] == -1 for j in two) and any(j.pair[0] >= 0 for j in two)
    order = [tuple(int(x) for x in j.what.split()[2].split(",")) for j in two]
    assert any(p0 > p1 for p0, p1 in order) and any(p0 < p1 for p0, p1 in order)     # the best in the later slice, and in the earlier


def test_cross_block_claims():
    j = mc.cross_block_claims()
    p, r = mc.verify(j)
    assert p.tolist() == [[q, q] for q in range(300)]
    assert np.array_equal(r[300:], r[:300]) and np.all(r[:, 1] == 1)     # the higher query had the same best: no fall-back
    mc.verify(j, match=ref.match_np)


@pytest.mark.parametrize("nndr", mc.NNDRS)
def test_nndr_boundaries(nndr):
    jobs = mc.nndr_boundaries(nndr)
    acc = [j for j in jobs if j.accept]
    rej = [j for j in jobs if not j.accept]
    assert len(acc) == 256 and len(rej) >= 200
    for k, j in enumerate(jobs):
        p, _ = mc.verify(j, nndr=nndr)
        assert (0 in p[:, 0]) == j.accept
        if k % 40 == 0:
            mc.verify(j, nndr=nndr, match=ref.match_np)
    if nndr == 1.0:
        assert all(j.rec[0][1] == j.rec[0][2] for j in rej)       # at nndr 1 only the tie is rejected


def test_nndr_values_differ_where_they_should():
    """0.8f and the float above it decide (4 k, 5 k) differently: the rule is evaluated in float, not as 5 d0 < 4 d1."""
    up = mc.NNDRS[3]
    assert np.float32(up) > np.float32(0.8)
    assert not ref._nndr(4, 5, 0.8)
    a = {j.what.split()[2] for j in mc.nndr_boundaries(0.8) if j.accept}
    b = {j.what.split()[2] for j in mc.nndr_boundaries(up) if j.accept}
    assert a != b


def test_widest_store():
    j = mc.widest_store()
    p, r = mc.verify(j)
    assert len(p) == 16 and sorted(p[:, 1].tolist()) == mc.spots(65535, 8192)
    assert len({int(t) // 8192 for t in p[:, 1]}) == 8             # every slice holds a winner


def test_radius_classes():
    for r in mc.RADII_BELOW:
        assert mc.radius_threshold(r) == np.nextafter(mc.square_f32(r), np.float32(0)), r
    for r in mc.RADII_AT:
        assert mc.radius_threshold(r) == mc.square_f32(r), r
    for r in mc.RADII_BELOW + mc.RADII_AT:
        T = mc.radius_threshold(r)
        assert np.sqrt(T, dtype=np.float32) >= np.float32(r) > np.sqrt(np.nextafter(T, np.float32(0)), dtype=np.float32)


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("radius", mc.RADII_BELOW + mc.RADII_AT)
def test_radius_threshold_cases(radius, fused):
    job, at, below = mc.radius_threshold_cases(radius, fused)
    assert len(at) >= 4 and len(below) >= 4
    _, r = mc.verify(job, radius=radius, fused=fused)
    assert np.all(r[at, 3] == 0) and np.all(r[below, 3] == 1)
    mc.verify(job, radius=radius, fused=fused, match=ref.match_np)
    d2 = np.array([ref.sq_dist(*job.proj[i], *job.kto[i], fused) for i in range(len(job.proj))], np.float32)
    assert np.all(d2[at] == mc.radius_threshold(radius))
    assert not any(ref.inside(v, radius) for v in d2[at]) and all(ref.inside(v, radius) for v in d2[below])
    naive = d2 < mc.square_f32(radius)
    if radius in mc.RADII_BELOW:
        assert np.all(naive[at])                                  # d2 < fl(r * r) would wrongly admit every T(r) query
    else:
        assert not naive[at].any()
    assert np.all(naive[below])


@pytest.mark.parametrize("radius", mc.RADII_BELOW)     # the band kinds exist only where T(r) lies below fl(r * r)
def test_generalised_edge_cases_keep_their_kinds(radius):
    P, Kt, kinds = ref.radius_edge_cases(radius=radius)
    assert len(P) == 24
    for i, kind in enumerate(kinds):
        du, df = ref.sq_dist(*P[i], *Kt[i], False), ref.sq_dist(*P[i], *Kt[i], True)
        iu, jf = ref.inside(du, radius), ref.inside(df, radius)
        r2 = mc.square_f32(radius)
        if kind == "band_unfused":
            assert du < r2 and not iu
        elif kind == "band_fused":
            assert df < r2 and not jf
        else:
            assert iu != jf
