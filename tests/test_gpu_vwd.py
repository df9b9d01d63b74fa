"""The visual-word dictionary on the device against the numpy restatement (tests/vwd_cases.py): word ids, the store's rows, the
size and the 2-NN records are equal exactly, for both metrics; the likelihood against a float64 evaluation of the same sum.
For every exact-equality input the restatement first checks that no query's third neighbour ties with its second."""
import itertools
import pathlib

import numpy as np
import pytest

import vwd_cases as vc
from gpu_support import bm, dev, torch_cuda  # noqa: F401

ROOT = pathlib.Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.gpu
METRICS = pytest.mark.parametrize("metric", [vc.L1, vc.L2], ids=["L1", "L2"])


class Pair:
    """A device dictionary and the restatement, fed the same calls and compared after each."""

    def __init__(self, pkg, bm, metric, capacity=4096, slices=0, nndr=0.8):
        self.d = pkg.VWDictionary(bm, capacity, metric=metric, slices=slices, nndr=nndr)
        self.r = vc.Dictionary(metric, nndr=nndr, capacity=capacity)
        self.pkg = pkg

    def close(self):
        self.d.close()

    def seed(self, words):
        """Into the empty dictionary every row is a new word, in row order (node 1)."""
        self.d.reset()
        self.r = vc.Dictionary(self.r.metric, nndr=self.r.nndr, capacity=self.r.capacity)
        ids = self.d.add_words(np.ascontiguousarray(words), 1)
        want, _ = self.r.add_new_words(words, 1)
        assert np.array_equal(ids, want) and np.array_equal(ids, np.arange(len(words)))
        return self

    def search(self, q):
        assert vc.no_third_tie(q, self.r.words, self.r.metric).all()
        rec = self.d.search(dev(q)).cpu().numpy()
        want = vc.search(q, self.r.words, self.r.metric)
        assert np.array_equal(rec, want), np.flatnonzero((rec != want).any(axis=1))[:8]
        return rec

    def add(self, q, node, total=None, device=True):
        assert vc.no_third_tie(q, self.r.words, self.r.metric).all()
        want, _ = self.r.add_new_words(q, node, total)
        if want is None:
            with pytest.raises(self.pkg.StereoBMError) as e:
                self.d.add_words(dev(q) if device else q, node, total)
            assert e.value.code == self.pkg.ERR_VWD_FULL
        else:
            ids = self.d.add_words(dev(q) if device else q, node, total)
            assert np.array_equal(ids, want), np.flatnonzero(ids != want)[:8]
        assert self.d.size() == len(self.r.words) and self.d.overflow() == self.r.overflow
        assert np.array_equal(self.d.words(), self.r.words)
        return want

    def check_refs(self):
        for w, refs in enumerate(self.r.refs):
            assert self.d.references(w) == refs, w


@METRICS
@pytest.mark.parametrize("N", [0, 1, 2, 63, 64, 65, 129])
def test_sizes_with_automatic_slices(pkg, bm, metric, N):
    p = Pair(pkg, bm, metric)
    try:
        for n in (1, 63, 64, 65, 130):
            words, q = vc.make_case(1000 * N + n, n, N, metric)
            p.seed(words)
            p.search(q)
            ids = p.add(q, 2)
            if N >= 2 and n > 1:
                assert (ids < N).any() and (ids >= N).any()   # both kinds of row are present
            p.check_refs()
    finally:
        p.close()


def near(row, byte, by):
    out = row.copy()
    out[byte] = out[byte] + by if out[byte] < 128 else out[byte] - by
    return out


@METRICS
@pytest.mark.parametrize("slices", [1, 2, 5])
def test_neighbours_at_the_ends_and_either_side_of_each_slice_boundary(pkg, bm, metric, slices):
    """N = 300: slices 5 gives slices of 64 words (boundaries 64, 128, 192, 256), slices 2 gives 192 and 108, slices 1 one."""
    N = 300
    base, q = vc.make_case(77, 1, N, metric)
    q[0] = np.random.default_rng(78).integers(100, 156, 32, dtype=np.uint8)
    spots = [0, 63, 64, 127, 128, 191, 192, 255, 256, 299]
    p, ties = Pair(pkg, bm, metric, slices=slices), Pair(pkg, bm, metric, slices=slices, nndr=1.0)
    try:
        for p0, p1 in itertools.permutations(spots, 2):
            words = base.copy()
            words[p0] = near(q[0], 3, 1)                 # the nearest
            words[p1] = near(q[0], 9, 2)                 # the second nearest
            rec = p.seed(words).search(q)
            assert (rec[0, 0], rec[0, 2]) == (p0, p1) and rec[0, 1] < rec[0, 3]
            if p0 < p1:                                  # two equally distant words: the older one ranks first
                words[p1] = near(q[0], 9, 1)
                rec = p.seed(words).search(q)
                assert (rec[0, 0], rec[0, 2]) == (p0, p1) and rec[0, 1] == rec[0, 3]
                assert p.add(q, 2)[0] == N               # d > 0.8f * d: unique
                assert ties.seed(words).add(q, 2)[0] == p0   # nndr 1: d > d is false, and the row goes to the older word
    finally:
        p.close()
        ties.close()


@METRICS
def test_duplicates_and_identical_rows(pkg, bm, metric):
    words, q = vc.make_case(5, 6, 200, metric)
    words[150] = words[20]                               # duplicate dictionary rows
    words[199] = words[70]
    q[0] = near(words[20], 4, 1)
    q[1] = words[70]                                     # identical to two words: d0 = d1 = 0
    q[2] = words[100]                                    # identical to one word: d0 = 0 < d1
    p = Pair(pkg, bm, metric, slices=4)
    try:
        p.seed(words)
        rec = p.search(q)
        assert list(rec[0, [0, 2]]) == [20, 150] and list(rec[1]) == [70, 0, 199, 0] and list(rec[2, :2]) == [100, 0]
        ids = p.add(q, 2)
        assert list(ids[:3]) == [200, 70, 100]               # d0 = d1 = 1 is unique (1 > 0.8f); d0 = d1 = 0 goes to the older word
        p.check_refs()
        # duplicate query rows in one call into an empty dictionary: both become words
        two = np.stack([q[3], q[3], q[4], q[3]])
        assert list(p.seed(two).d.words().tolist()) == two.tolist() and p.d.size() == 4
        # a dictionary of one word: every row is unique, the identical one too
        assert list(p.seed(q[5:6]).add(np.stack([q[5], q[4]]), 2)) == [1, 2]
    finally:
        p.close()


@METRICS
def test_nndr_boundary_pairs(pkg, bm, metric):
    """Words at distances (d0, d1) from the zero query with 5 d0 == 4 d1, and one step either side of it, spread over the metric's
    range with both ends: on the boundary the row is not unique (as the float test of the CPU file says), one above it is."""
    pairs = vc.boundary_pairs(metric)
    pick = np.unique(np.concatenate([np.linspace(0, len(pairs) - 1, 40).astype(int), np.arange(8)]))
    q = np.zeros((1, 32), np.uint8)
    p = Pair(pkg, bm, metric)
    done = 0
    try:
        for d0, d1 in pairs[pick]:
            for step in (-1, 0, 1):
                w0, w1 = vc.row_at_distance(int(d0) + step, metric), vc.row_at_distance(int(d1), metric)
                if w0 is None or w1 is None or d0 + step > d1:
                    continue
                p.seed(np.stack([w0, w1]))
                assert list(p.search(q)[0]) == [0, d0 + step, 1, d1]
                unique = bool(vc.float_test(np.array([d0 + step]), np.array([d1]))[0])
                assert unique == (step > 0)
                assert p.add(q, 2)[0] == (2 if unique else 0)
                done += step == 0
        assert done >= 40
    finally:
        p.close()


def tie_free_frames(metric, seed, frames, accept=lambda r: True):
    """frames(rng) -> [(rows, node)]: the first seed from `seed` on whose calls, fed in order, never meet a tie between a second
    and a third neighbour, and whose dictionary has the shape the test wants (random rows can fall to a word by chance)."""
    for s in range(seed, seed + 200):
        calls = frames(np.random.default_rng(s))
        r = vc.Dictionary(metric)
        ok = True
        for rows, node in calls:
            ok = ok and vc.no_third_tie(rows, r.words, metric).all()
            r.add_new_words(rows, node)
        if ok and accept(r):
            return calls
    raise AssertionError("no tie-free input found")


def fresh(pkg, bm, metric, **kw):
    p = Pair(pkg, bm, metric, **kw)
    p.d.reset()
    return p


@METRICS
def test_three_calls_and_a_repeated_frame(pkg, bm, metric):
    def frames(rng):
        a = rng.integers(0, 256, (90, 32), dtype=np.uint8)
        b = rng.integers(0, 256, (70, 32), dtype=np.uint8)
        for i in range(0, 70, 2):                              # every other row of b is a nudged row of a
            b[i] = near(a[i], i % 32, 1)
        return [(a, 4), (b, 9), (a, 2)]

    (a, _), (b, _), _ = tie_free_frames(metric, 31, frames)
    p = fresh(pkg, bm, metric)
    try:
        assert list(p.add(a, 4, 120)) == list(range(90))       # node 4: every row is new; 30 keypoints were cut
        ids = p.add(b, 9, device=False)                        # node 9, the host form: every other row goes to node 4's words
        assert list(ids[0::2]) == list(range(0, 70, 2)) and (ids[1::2] >= 90).sum() > 20
        size = p.d.size()
        ids = p.add(a, 2)                                      # node 2 repeats node 4's descriptors: references only
        assert p.d.size() == size > 110 and list(ids) == list(range(90))
        p.check_refs()
        assert p.d.references(0) == {2: 1, 4: 1, 9: 1} and p.d.references(1) == {2: 1, 4: 1} and 9 in p.d.references(90)
    finally:
        p.close()


@METRICS
def test_scratch_and_staging_of_a_larger_call_are_not_read(pkg, bm, metric):
    """Large, small, large through the host form on one handle: partial records, merged records and flags are placed anew in
    scratch that only grows, the rows in staging that only grows."""
    def frames(rng):
        a = rng.integers(0, 256, (130, 32), dtype=np.uint8)
        b = rng.integers(0, 256, (130, 32), dtype=np.uint8)
        return [(a, 2), (b[:1], 3), (b[1:18], 4), (np.concatenate([b[18:], a[:40]]), 5)]

    p = fresh(pkg, bm, metric)
    try:
        for rows, node in tie_free_frames(metric, 61, frames):
            p.add(rows, node, device=False)
        p.check_refs()
    finally:
        p.close()


@METRICS
def test_overflow_adds_nothing(pkg, bm, metric):
    _, rows = vc.make_case(41, 130, 0, metric)
    p = Pair(pkg, bm, metric, capacity=100)
    try:
        p.seed(rows[:80])
        assert p.add(rows[80:110], 2) is None                  # 30 new words do not fit: refused, nothing changes
        assert p.d.size() == 80 and p.d.overflow() == 1
        with pytest.raises(pkg.StereoBMError):
            p.d.likelihood(2, [1], 2)                           # the refused node is unknown
        mixed = np.concatenate([rows[80:100], rows[:10]])       # 20 new words fit exactly, 10 rows are references
        ids = p.add(mixed, 3)
        assert p.d.size() == 100 and list(ids[20:]) == list(range(10))
        assert p.add(rows[100:101], 5) is None and p.d.overflow() == 2
        p.check_refs()
    finally:
        p.close()


def test_device_rows_straight_from_orb_describe(pkg, bm, golden, torch_cuda):
    """The golden pair's descriptors stay on the device between sbm_orb_features_device and the dictionary. Rows whose second and
    third neighbours tie are left out of a call (a gather on the device); a call without such rows passes the tensor's own memory."""
    pattern = np.load(ROOT / "tests" / "golden" / "orb_pattern.npz")["pattern"]
    imgs = np.stack([golden["rect_l"], golden["rect_r"]])
    desc, kpts, count = bm.orb_features(dev(imgs), pattern)
    cn = count.cpu().numpy()
    host = desc.cpu().numpy()
    assert cn.min() > 100
    for metric in (vc.L1, vc.L2):
        p = fresh(pkg, bm, metric)
        try:
            for node, f in ((1, 0), (2, 1), (3, 0)):
                keep = vc.no_third_tie(host[f, :cn[f]], p.r.words, metric)
                print("metric", metric, "frame", f, "rows", cn[f], "kept", int(keep.sum()))
                assert keep.mean() > 0.8
                rows = desc[f, :cn[f]] if keep.all() else desc[f, :cn[f]][torch_cuda.from_numpy(keep).to(desc.device)]
                want, _ = p.r.add_new_words(host[f, :cn[f]][keep], node)
                ids = p.d.add_words(rows, node)
                assert np.array_equal(ids, want)
                assert p.d.size() == len(p.r.words) and np.array_equal(p.d.words(), p.r.words)
            assert (want < len(p.r.words) - 0).all() and p.d.size() == len(p.r.words)
            p.check_refs()
        finally:
            p.close()


# ---- likelihood ----------------------------------------------------------------------------------------------------------------
TOTALS = {1: 101, 2: 140, 3: 111, 4: 101, 5: 126, 6: 900}   # nodes 2 and 6 had keypoints cut by the limit


def likelihood_frames(rng):
    pool = rng.integers(0, 256, (400, 32), dtype=np.uint8)
    everywhere = pool[399]
    return [(np.concatenate([pool[0:100], everywhere[None]]), 1),
            (np.concatenate([pool[0:70], pool[100:120], everywhere[None]]), 2),
            (np.concatenate([pool[60:90], pool[120:200], everywhere[None]]), 3),
            (np.concatenate([pool[200:300], everywhere[None]]), 4),
            (np.concatenate([pool[5:95], pool[5:30], pool[300:310], everywhere[None]]), 5),   # words counted twice in one node
            (np.concatenate([pool[0:1], pool[310:330], everywhere[None]]), 6)]


def likelihood_pair(pkg, bm):
    """Six nodes over shared material: nodes 2 and 5 repeat most of node 1's rows, node 3 some, node 4 none; word 0 is referenced
    by nodes 1, 2 and 6 only; one word is referenced by every node."""
    def accept(r):   # node 6 shares word 0 and the word of every node with the others, and nothing else
        others = set().union(*(r.nodes[k][0] for k in range(1, 6)))
        return r.nodes[6][0][0] == 0 and set(r.nodes[6][0]) & others == {0, r.nodes[1][0][-1]} and r.refs[0].keys() == {1, 2, 6}

    p = fresh(pkg, bm, vc.L2)
    for rows, node in tie_free_frames(vc.L2, 91, likelihood_frames, accept):
        p.add(rows, node, TOTALS[node], device=node % 2 == 0)
    return p


def test_likelihood_scores_and_best_hypothesis(pkg, bm):
    p = likelihood_pair(pkg, bm)
    try:
        for node, cands, n_nodes in [(5, [1, 2, 3, 4, 6], 6), (2, [6, 4, 3, 1], 6), (1, [2, 3, 4, 5, 6], 40), (3, [1, 2], 7),
                                     (4, [1, 2, 3], 6), (6, [1, 2, 3, 4, 5], 6), (1, [], 6), (1, [2, 3], 0)]:
            scores, best, best_score = p.d.likelihood(node, cands, n_nodes)
            f64 = p.r.likelihood_f64(node, cands, n_nodes)
            want, want_best, want_score = p.r.likelihood(node, cands, n_nodes)
            bounds = []
            for c, s in zip(cands, scores):
                exact, sum_abs, T = f64[c]
                bound = vc.likelihood_bound(sum_abs, T)
                bounds.append(bound)
                print(node, c, float(s), exact, abs(float(s) - exact), bound, T)
                assert abs(float(s) - exact) <= bound, (node, c)
            top = sorted((f64[c][0] for c in cands if c > 0), reverse=True)
            if len(top) >= 2 and top[0] - top[1] > 2 * max(bounds) and top[0] > 2 * max(bounds):
                assert best == max(cands, key=lambda c: f64[c][0]) == want_best and best_score == scores[cands.index(best)]
            if not cands or n_nodes == 0:
                assert (best, best_score) == (0, 0.0) and not scores.any()
        # the inputs above decide the best hypothesis for the nodes that share words
        assert p.d.likelihood(5, [1, 2, 3, 4, 6], 6)[1] == 1 and p.d.likelihood(2, [6, 4, 3, 1], 6)[1] == 1
    finally:
        p.close()


def test_likelihood_properties(pkg, bm):
    p = likelihood_pair(pkg, bm)
    try:
        assert p.r.nodes[6][0][0] == 0 and p.r.refs[0].keys() == {1, 2, 6}
        shared = p.r.nodes[1][0][-1]
        assert set(p.r.refs[shared]) == {1, 2, 3, 4, 5, 6}
        # node 6 shares only word 0 and the word of every node with node 1: neither contributes
        scores, best, best_score = p.d.likelihood(6, [1, 2, 3, 4, 5], 6)
        assert not scores.any() and (best, best_score) == (0, 0.0)
        # with more nodes in the map than reference it, the shared word does contribute, word 0 still does not
        scores7, _, _ = p.d.likelihood(6, [1, 4], 7)
        f64 = p.r.likelihood_f64(6, [1, 4], 7)
        assert scores7[0] > 0 and f64[1][2] == 1 and f64[4][2] == 1
        # negative ids (keypoints cut by the limit) never reach the store: they count in ni only
        assert min(p.r.nodes[6][0]) >= 0 and p.r.nodes[6][1] == 900
        cut = p.r.terms(1, [6], 7)[6]
        assert cut and all(ni == 900 for _, _, ni in cut)
        assert p.r.terms(1, [6], 7, words=p.r.nodes[1][0] + [-1, -2, -3]) == p.r.terms(1, [6], 7)
        # candidates absent from the list get no score and are never the best
        full, best, _ = p.d.likelihood(5, [1, 2, 3, 4, 6], 6)
        part, best_part, _ = p.d.likelihood(5, [3, 4], 6)
        assert best == 1 and best_part == 3 and list(part) == [full[2], full[3]]
        # a repeated candidate is one candidate; a candidate the dictionary has not seen scores nothing
        rep, _, _ = p.d.likelihood(5, [3, 3, 77], 6)
        assert rep[0] == rep[1] == full[2] and rep[2] == 0
        for node, code in ((0, -23), (-4, -23), (77, -2)):
            with pytest.raises(pkg.StereoBMError) as e:
                p.d.likelihood(node, [1], 6)
            assert e.value.code == code
        with pytest.raises(pkg.StereoBMError) as e:
            p.d.add_words(np.zeros((1, 32), np.uint8), 0)
        assert e.value.code == -23
    finally:
        p.close()
