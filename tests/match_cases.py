"""Crafted inputs for the keypoint matcher's paths, each with the property it guarantees. TEST INFRASTRUCTURE ONLY.

A builder returns `Job`s: descriptor rows of the from- and to-frame (and for the guided form the projections and to-keypoints),
`rec` = the k-NN record the restatement must give for some queries, `pair` = the to-row those queries must hold a pair with
(-1: the query is in no pair). tests/test_match_cases_restatement.py checks every guarantee with oracle/match_ref alone, so
that tests/test_gpu_match_paths.py, which compares the device with the same restatement, cannot pass because an input missed
the path it was written for.

The query of the slice cases sits at from-rows 0 and 64 (two query tiles); row 64 repeats row 0, so where row 0 is accepted row
64 claims the same to-row and must lose it without falling back."""
import itertools
import math
from dataclasses import dataclass, field

import numpy as np

import match_ref as ref

QROWS = (0, 64)
NONE = (-1, 257, 257, 0)


@dataclass
class Job:
    frm: np.ndarray                 # (nf, 32) uint8
    to: np.ndarray                  # (nt, 32) uint8
    proj: np.ndarray = None         # (nf, 2) float32, guided only
    kto: np.ndarray = None          # (nt, 2) float32, guided only
    rec: dict = field(default_factory=dict)     # query -> (best, d0, d1, candidates)
    pair: dict = field(default_factory=dict)    # query -> to-row of its pair, or -1 for "in no pair"
    what: str = ""
    tie: bool = False               # the two best tie: in no pair at any nndr
    accept: bool = None             # NNDR cases: whether query 0 passes


def verify(job, radius=40.0, nndr=0.8, fused=False, match=None):
    """The guarantees of one job against the restatement (ref.match, or ref.match_np). Returns (pairs, rec)."""
    pairs, rec = (match or ref.match)(job.frm, job.to, job.proj, job.kto, radius=radius, nndr=nndr, fused=fused)
    for q, want in job.rec.items():
        assert tuple(rec[q]) == tuple(want), (job.what, q, tuple(rec[q]), want)
    held = {int(a): int(b) for a, b in pairs}
    for q, t in job.pair.items():
        assert held.get(q, -1) == t, (job.what, q, held.get(q, -1), t)
    return pairs, rec


def flip(row, bits):
    b = np.unpackbits(row)
    b[list(bits)] ^= 1
    return np.packbits(b)


def spots(nt, slice_rows):
    """0, nt - 1, and the rows either side of every slice boundary below nt."""
    s = {0, nt - 1}
    for b in range(slice_rows, nt, slice_rows):
        s |= {b - 1, b}
    return sorted(s)


def sparse_spot_pairs(nt, slice_rows, step=3):
    """A subset of the ordered spot pairs for stores with many slices: both orders across every step-th gap between
    neighbouring spots, and the two ends in both orders."""
    s = spots(nt, slice_rows)
    out = [(a, b) for i in range(0, len(s) - 1, step) for a, b in ((s[i], s[i + 1]), (s[i + 1], s[i]))]
    return out + [(s[0], s[-1]), (s[-1], s[0])]


def frame_pair(nt, seed):
    """(from-frame of 65 rows with the query at rows 0 and 64, random to-frame of nt rows): every random row is more than 64
    bits from every other, so rows planted within a few bits of the query are its nearest."""
    rng = np.random.default_rng(seed)
    frm = rng.integers(0, 256, (65, 32), dtype=np.uint8)
    frm[64] = frm[0]
    to = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    d = ref._POP[np.bitwise_xor(to, frm[0][None, :])].sum(axis=1)
    assert d.min() > 64
    return frm, to


def _both(v):
    return {q: v for q in QROWS}


def pairs_and_ties(nt, slice_rows, seed=1, spot_pairs=None):
    """One to-frame per ordered pair of spots: the nearest row (1 bit) at p0, the second (2 bits) at p1; where p0 < p1 also
    the tie, both at 1 bit. Records (p0, 1, 2, nt) / (min, 1, 1, nt); a tied query is in no pair."""
    frm, base = frame_pair(nt, seed)
    q = frm[0]
    jobs = []
    for p0, p1 in (spot_pairs or itertools.permutations(spots(nt, slice_rows), 2)):
        to = base.copy()
        to[p0], to[p1] = flip(q, [0]), flip(q, [1, 2])
        jobs.append(Job(frm, to, rec=_both((p0, 1, 2, nt)), pair={0: p0, 64: -1}, what=f"pair {p0},{p1}"))
        if p0 < p1:
            to = to.copy()
            to[p1] = flip(q, [1])
            jobs.append(Job(frm, to, rec=_both((p0, 1, 1, nt)), pair=_both(-1), what=f"tie {p0},{p1}", tie=True))
    return jobs


def spot_triples(nt, slice_rows):
    """Three spots each: the ends and a middle boundary, and for every later slice its two end rows with the last row of the
    slice before (both leaders in one later slice, the third in an earlier one, in the orders that put it there)."""
    s = spots(nt, slice_rows)
    out = [(s[0], s[len(s) // 2], s[-1])]
    for b in range(slice_rows, nt, slice_rows):
        last = min(b + slice_rows, nt) - 1
        if last > b:
            out.append((b - 1, b, last))
    return out


def triples(nt, slice_rows, seed=2, spot_sets=None):
    """Rows at 1, 2 and 3 bits on three spots, in all six orders: d1 == 2 whichever slice holds which."""
    frm, base = frame_pair(nt, seed)
    q = frm[0]
    near = {1: flip(q, [0]), 2: flip(q, [1, 2]), 3: flip(q, [3, 4, 5])}
    jobs = []
    for sp in (spot_sets or spot_triples(nt, slice_rows)):
        for order in itertools.permutations((1, 2, 3)):
            to = base.copy()
            for p, d in zip(sp, order):
                to[p] = near[d]
            best = sp[order.index(1)]
            jobs.append(Job(frm, to, rec=_both((best, 1, 2, nt)), pair={0: best, 64: -1}, what=f"triple {sp} {order}"))
    return jobs


def guided_slices(nt, slice_rows, seed=3):
    """The radius gate admits to-rows of late slices only. To-row 1 repeats the query outside the radius and is never a
    candidate. One admitted row: taken without NNDR, however far its descriptor. Two in different slices at 4 and 5 bits
    (5 * 4 >= 4 * 5): rejected; at 1 and 2 bits: accepted. None: the empty record."""
    frm, base = frame_pair(nt, seed)
    q = frm[0]
    base[1] = q
    s = spots(nt, slice_rows)
    late = [p for p in s if p >= slice_rows]
    assert late and len(frm) == 65
    proj = np.full((65, 2), np.nan, np.float32)
    proj[0::2] = (5000.0, 5000.0)                          # queries without a candidate; the odd rows are no queries
    proj[0] = proj[64] = (100.0, 100.0)
    far = np.stack([2000.0 + np.arange(nt), np.full(nt, 3000.0)], 1).astype(np.float32)
    inside = np.array([[103.0, 96.0], [97.5, 104.25]], np.float32)      # 5 px and about 4.9 px from the query
    jobs = [Job(frm, base.copy(), proj, far, rec=_both(NONE), pair=_both(-1), what="guided none")]
    for p in late:
        kto = far.copy()
        kto[p] = inside[0]
        d = int(ref._POP[np.bitwise_xor(base[p], q)].sum())
        jobs.append(Job(frm, base.copy(), proj, kto, rec=_both((p, d, 257, 1)), pair={0: p, 64: -1}, what=f"guided one {p}"))
    cross = [(a, b) for a, b in itertools.permutations(late, 2) if a // slice_rows != b // slice_rows]
    step = max(1, len(cross) // 12)
    for p0, p1 in cross[::step]:
        for bits, ok in (((4, 5), False), ((1, 2), True)):
            to, kto = base.copy(), far.copy()
            to[p0], to[p1] = flip(q, range(bits[0])), flip(q, range(10, 10 + bits[1]))
            kto[p0], kto[p1] = inside
            jobs.append(Job(frm, to, proj, kto, rec=_both((p0, bits[0], bits[1], 2)), pair={0: p0 if ok else -1, 64: -1},
                            what=f"guided two {p0},{p1} {bits}"))
    return jobs


def cross_block_claims(seed=4):
    """600 queries, 300 to-rows: queries q and q + 300 are the same row, one bit from to-row q, so both claim it from different
    256-lane blocks of the claim kernel. The lower holds the pair; the higher is in no pair and does not fall back."""
    rng = np.random.default_rng(seed)
    half = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    frm = np.concatenate([half, half])
    to = np.stack([flip(r, [i % 256]) for i, r in enumerate(half)])
    assert all(q // 256 != (q + 300) // 256 for q in range(300))
    pair = {q: q for q in range(300)}
    pair.update({q + 300: -1 for q in range(300)})
    return Job(frm, to, pair=pair, what="cross-block claims")


NNDRS = [0.5, 0.7, 0.8, float(np.nextafter(np.float32(0.8), np.float32(1.0))), 1.0]


def nndr_boundaries(nndr):
    """For every d1 in 1..256 the largest d0 the float rule accepts and the next one up (d0 <= d1): to-frames of two rows at
    exactly those distances from the zero query (from-row 0; row 1, all ones, rides along). One job per case, cap = 2."""
    frm = np.zeros((2, 32), np.uint8)
    frm[1] = 255
    jobs = []
    for d1 in range(1, 257):
        ok = [d0 for d0 in range(d1 + 1) if ref._nndr(d0, d1, nndr)]
        assert ok and ok == list(range(len(ok)))           # the accepted d0 are 0..d0*
        for d0 in (ok[-1], ok[-1] + 1):
            if d0 > d1:
                continue
            rows = {d: np.packbits(np.arange(256) < d) for d in (d0, d1)}
            first = (d0 + d1) % 2                          # the nearer row at index 0 or 1
            to = np.stack([rows[d1], rows[d0]] if first else [rows[d0], rows[d1]])
            best = first if d0 < d1 else 0
            accept = d0 <= ok[-1]
            jobs.append(Job(frm, to, rec={0: (best, d0, d1, 2)}, pair={0: best if accept else -1}, what=f"nndr {nndr} {d0}/{d1}",
                            accept=accept))
    return jobs


def widest_store(seed=5):
    """cap = nt = 65535, 64 queries: to-rows at the 16 spots of eight slices of 8192 are the base row with one of 16 groups of
    8 bits set; query i has 7 bits of group k0 and 6 (the last 16 queries: 7, a tie) of group k1, so its two nearest are the
    spots k0 (7 bits off) and k1 (9, or 8). Queries that share k0 contend for one to-row."""
    nt = 65535
    rng = np.random.default_rng(seed)
    to = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    sp = spots(nt, 8192)
    assert len(sp) == 16
    for k, p in enumerate(sp):
        to[p] = flip(base, range(8 * k, 8 * k + 8))
    frm = np.zeros((64, 32), np.uint8)
    rec, pair = {}, {}
    for i in range(64):
        k0, k1, tie = i % 16, (i % 16 + (1, 5, 9, 13)[i // 16]) % 16, i >= 48
        n1 = 7 if tie else 6
        frm[i] = flip(base, list(range(8 * k0, 8 * k0 + 7)) + list(range(8 * k1, 8 * k1 + n1)))
        if tie:
            rec[i] = (min(sp[k0], sp[k1]), 8, 8, nt)
            pair[i] = -1
        else:
            rec[i] = (sp[k0], 7, 9, nt)
            pair[i] = sp[k0] if i < 16 else -1              # 5 * 7 < 4 * 9; the first 16 queries hold the 16 spots
    return Job(frm, to, rec=rec, pair=pair, what="widest store")


# ---- the radius test at any radius ------------------------------------------------------------------------------------------
RADII_BELOW = [5.0, 12.3, 40.0]          # the threshold is one float below fl(r * r)
RADII_AT = [0.75, 7.25, 33.3, 1000.0]    # the threshold is fl(r * r)


def f32_bits(b):
    return np.array([b], np.uint32).view(np.float32)[0]


def radius_threshold(r):
    """T(r): the least float32 whose float32 square root reaches r, by bisection over the bit patterns (the rounded square root
    is monotone, and so are the bit patterns of the non-negative floats)."""
    r = np.float32(r)
    lo, hi = 0, 0x7F800000
    while lo < hi:
        mid = (lo + hi) // 2
        if np.sqrt(f32_bits(mid), dtype=np.float32) >= r:
            hi = mid
        else:
            lo = mid + 1
    return f32_bits(lo)


def square_f32(r):
    r = np.float32(r)
    return np.float32(np.float64(r) * np.float64(r))


def radius_threshold_cases(radius, fused, count=4, seed=0):
    """Single-candidate queries on the radius edge under one reading of the sum: `count` whose squared distance is exactly T(r)
    (outside) and `count` at the float just below (inside). Searched with the radius scaled into [32, 64) by a power of two
    and scaled back, which is exact. Returns (job, index array of the T(r) queries, index array of the others)."""
    r = np.float32(radius)
    s = 2.0 ** (math.floor(math.log2(float(r))) - 5)
    rs = np.float32(float(r) / s)
    assert 32 <= rs < 64 and float(rs) * s == float(r)
    T, Ts = radius_threshold(r), radius_threshold(rs)
    rng = np.random.default_rng(seed)
    N, g = 400000, 2.0 ** -12    # every coordinate on this grid: the cell shifts below (multiples of 256, sums < 4096) stay exact
    px = (256.0 + np.round(rng.uniform(0, 1, N) / g) * g).astype(np.float32)
    py = (256.0 + np.round(rng.uniform(0, 1, N) / g) * g).astype(np.float32)
    th = rng.uniform(0.2, 1.35, N)
    kx = (np.round((px + float(rs) * np.cos(th)) / g) * g).astype(np.float32)
    ky = (np.round((py + float(rs) * np.sin(th)) / g) * g).astype(np.float32)
    dx, dy = px - kx, py - ky
    xx = dx * dx
    if fused:    # screening only: ref.sq_dist below decides
        d2 = (dy.astype(np.float64) * dy.astype(np.float64) + xx.astype(np.float64)).astype(np.float32)
    else:
        d2 = xx + dy * dy
    found = []
    for val in (Ts, np.nextafter(Ts, np.float32(0))):
        hits = []
        for i in np.flatnonzero(d2 == val):
            a = (px[i], py[i], kx[i], ky[i])
            if ref.sq_dist(*a, fused) == val:
                hits.append(a)
            if len(hits) == count:
                break
        assert len(hits) == count, (radius, fused, len(hits))
        found.append(hits)
    P, Kt = [], []
    for a in found[0] + found[1]:
        c = len(P)
        ox, oy = np.float32(256 * (c % 8)), np.float32(256 * (c // 8))   # one cell per query: the other keypoints are far
        P.append(((a[0] + ox) * np.float32(s), (a[1] + oy) * np.float32(s)))
        Kt.append(((a[2] + ox) * np.float32(s), (a[3] + oy) * np.float32(s)))
    P, Kt = np.array(P, np.float32), np.array(Kt, np.float32)
    n = len(P)
    at, below = np.arange(count), np.arange(count, n)
    d2 = np.array([ref.sq_dist(*P[i], *Kt[i], fused) for i in range(n)], np.float32)
    assert np.all(d2[at] == T) and np.all(d2[below] == np.nextafter(T, np.float32(0)))
    desc = np.random.default_rng(seed + 1).integers(0, 256, (n, 32), dtype=np.uint8)
    rec = {int(i): NONE for i in at}
    rec.update({int(i): (int(i), 0, 257, 1) for i in below})
    pair = {int(i): -1 for i in at}
    pair.update({int(i): int(i) for i in below})
    return Job(desc, desc, P, Kt, rec=rec, pair=pair, what=f"radius {radius} fused={fused}"), at, below
