"""The numpy restatement of the visual-word dictionary family and the inputs its tests share. TEST INFRASTRUCTURE ONLY.

A literal transcription of the loops include/sbm.h states ("visual-word dictionary"): VWDictionary::addNewWords with an exhaustive
2-NN search ordered by (distance, dictionary index) in place of FLANN, computeLikelihood with detectLoopClosure's choice of the
highest hypothesis, and SensorData::limitKeypoints with its multimap. Nothing here looks at the engine."""
import bisect
import math

import numpy as np

L1, L2 = 0, 1
NONE = 2147483647
MAX_DIST = {L1: 32 * 255, L2: 32 * 255 * 255}
NNDR = np.float32(0.8)


def distances(q, words, metric):
    """int64 (n, N): sum of absolute (L1) or squared (L2) byte differences."""
    if metric == L1:
        d = q.astype(np.int16)[:, None, :] - words.astype(np.int16)[None, :, :]
        return np.abs(d, out=d).sum(axis=2, dtype=np.int64)
    d = q.astype(np.int32)[:, None, :] - words.astype(np.int32)[None, :, :]
    return np.multiply(d, d, out=d).sum(axis=2, dtype=np.int64)


def search(q, words, metric, chunk=1 << 16):
    """Exhaustive 2-NN of every row of q: int32 (n, 4) records (i0, d0, i1, d1) ordered by (distance, index); -1 / NONE where the
    dictionary has no such word. The first minimum of a row is its lowest index; the second is the first minimum of the rest."""
    n, N = len(q), len(words)
    rec = np.empty((n, 4), np.int32)
    rec[:, 0::2] = -1
    rec[:, 1::2] = NONE
    rows = np.arange(n)
    for c0 in range(0, N, chunk):   # a later chunk replaces a neighbour only when strictly nearer
        d = distances(q, words[c0:c0 + chunk], metric)
        for _ in range(min(2, d.shape[1])):
            j = d.argmin(axis=1)
            dj = d[rows, j]
            first = dj < rec[:, 1]
            second = ~first & (dj < rec[:, 3])
            rec[first, 2:] = rec[first, :2]
            rec[first, 0], rec[first, 1] = (c0 + j)[first], dj[first]
            rec[second, 2], rec[second, 3] = (c0 + j)[second], dj[second]
            d[rows, j] = np.iinfo(np.int64).max
    return rec


def is_unique(rec, nndr=NNDR):
    """addNewWords' decision per record: fewer than two neighbours, or d0 > nndr * d1 as one float multiply and one compare."""
    lim = np.float32(nndr) * rec[:, 3].astype(np.float32)
    return (rec[:, 2] < 0) | (rec[:, 1].astype(np.float32) > lim)


class Dictionary:
    """VWDictionary and the nodes' words, as the engine defines them."""

    def __init__(self, metric=L1, nndr=NNDR, capacity=None):
        self.metric, self.nndr, self.capacity = metric, np.float32(nndr), capacity
        self.words = np.zeros((0, 32), np.uint8)
        self.refs = []        # per word: {node: count}
        self.nodes = {}       # node -> [word ids in row order, ni]
        self.overflow = 0

    def add_new_words(self, desc, node_id, n_keypoints_total=None):
        """Returns (word ids, records), or (None, records) when the new words do not fit: then nothing is added."""
        assert node_id >= 1
        desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        rec = search(desc, self.words, self.metric)   # against the dictionary as it was before the call
        unique = is_unique(rec, self.nndr)
        if self.capacity is not None and len(self.words) + int(unique.sum()) > self.capacity:
            self.overflow += 1
            return None, rec
        ids = []
        for i in range(len(desc)):
            if unique[i]:
                ids.append(len(self.refs))             # getNextId()
                self.refs.append({node_id: 1})         # VisualWord(id, row, nodeId)
            else:
                w = int(rec[i, 0])
                self.refs[w][node_id] = self.refs[w].get(node_id, 0) + 1   # addRef
                ids.append(w)
        self.words = np.concatenate([self.words, desc[unique]])
        node = self.nodes.setdefault(node_id, [[], 0])
        node[0] += ids
        node[1] += len(desc) if n_keypoints_total is None else n_keypoints_total
        return np.array(ids, np.int32).reshape(-1), rec

    def terms(self, node_id, candidates, n_nodes, words=None):
        """computeLikelihood's walk: per candidate the list of (nwi, N / nw as a float, ni) it accumulates, in the order it does.
        words: the node's word ids where they are not the stored ones (negative ids of cut keypoints)."""
        out = {int(c): [] for c in candidates}
        ids = sorted(set(self.nodes[node_id][0] if words is None else words))
        N = np.float32(n_nodes)
        if N:
            for w in ids:
                if w <= 0:
                    continue
                refs = self.refs[w]
                ratio = np.float32(N / np.float32(len(refs)))
                if np.log10(ratio) == 0:
                    continue
                for j in sorted(refs):
                    if j in out and j in self.nodes:
                        out[j].append((refs[j], ratio, self.nodes[j][1]))
        return out

    def likelihood(self, node_id, candidates, n_nodes, words=None):
        """({candidate: float32 score}, best id, best score) in float, as the reference computes them."""
        score = {}
        for c, ts in self.terms(node_id, candidates, n_nodes, words).items():
            s = np.float32(0)
            for nwi, ratio, ni in ts:
                s = np.float32(s + np.float32(np.float32(np.float32(nwi) * np.log10(ratio)) / np.float32(ni)))
            score[c] = s
        best = (0, np.float32(0))
        for c in sorted(score):
            if c > 0 and score[c] > best[1]:
                best = (c, score[c])
        return score, best[0], best[1]

    def likelihood_f64(self, node_id, candidates, n_nodes, words=None):
        """{candidate: (the same sum in float64, sum of |term|, number of terms)}."""
        out = {}
        for c, ts in self.terms(node_id, candidates, n_nodes, words).items():
            t = [nwi * math.log10(float(ratio)) / ni for nwi, ratio, ni in ts]
            out[c] = (math.fsum(t), math.fsum(abs(x) for x in t), len(t))
        return out


def likelihood_bound(sum_abs, nterms):
    """(T + 3) * 2^-23 * sum |term|: three roundings and log10f's last place per term, T - 1 additions."""
    return (nterms + 3) * 2.0 ** -23 * sum_abs


def limit_keypoints(responses, max_keypoints):
    """SensorData::limitKeypoints: std::multimap<float, int> insertion (after every equal key) and the walk from rbegin()."""
    n = len(responses)
    if max_keypoints > 0 and n > max_keypoints:
        keys, idx = [], []
        for i in range(n):
            k = abs(np.float32(responses[i]))
            at = bisect.bisect_right(keys, k)
            keys.insert(at, k)
            idx.insert(at, i)
        keep = np.zeros(n, bool)
        for k in range(max_keypoints):
            keep[idx[n - 1 - k]] = True
        return keep
    return np.ones(n, bool)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def no_third_tie(q, words, metric):
    """True where a query's third neighbour is not tied with its second: the (distance, index) rule then fixes its record."""
    if len(words) < 3:
        return np.ones(len(q), bool)
    d = np.sort(distances(q, words, metric), axis=1)
    return d[:, 2] != d[:, 1]


def make_case(seed, n, N, metric):
    """(words (N, 32), queries (n, 32)): half of the queries are words with a few bytes nudged (near a word: not unique), the
    rest random (unique). Queries whose second and third neighbours tie are drawn again."""
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for attempt in range(100):
        if N:
            near = np.arange(n) % 2 == 0
            src = words[rng.integers(0, N, n)].astype(np.int64)
            src[np.arange(n), rng.integers(0, 32, n)] += rng.integers(-9, 10, n)
            fresh = np.where(near[:, None], np.clip(src, 0, 255).astype(np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8))
        else:
            fresh = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        bad = ~no_third_tie(q, words, metric) if attempt else np.ones(n, bool)
        if not bad.any():
            break
        q[bad] = fresh[bad]
    assert no_third_tie(q, words, metric).all()
    return words, q


def boundary_pairs(metric):
    """Every (d0, d1) with 5 * d0 == 4 * d1 up to the metric's maximum: int64 (k, 2)."""
    k = np.arange(1, MAX_DIST[metric] // 5 + 1, dtype=np.int64)
    return np.stack([4 * k, 5 * k], axis=1)


def float_test(d0, d1, nndr=NNDR):
    return d0.astype(np.float32) > np.float32(nndr) * d1.astype(np.float32)


_TWO = None


def _two_squares():
    global _TWO
    if _TWO is None:
        _TWO = {}
        for a in range(256):
            for b in range(a, 256):
                _TWO.setdefault(a * a + b * b, (a, b))
    return _TWO


def row_at_distance(d, metric):
    """A 32-byte row at distance d from the zero row, or None where this construction finds none."""
    row = np.zeros(32, np.uint8)
    if metric == L1:
        if d > MAX_DIST[L1]:
            return None
        row[:d // 255] = 255
        if d % 255:
            row[d // 255] = d % 255
        return row
    two = _two_squares()
    full = min(d // 65025, 32)
    for t in range(full, max(full - 5, -1), -1):   # t bytes of 255, the rest as four squares
        rem = d - t * 65025
        if rem == 0:
            row[:t] = 255
            return row
        if t + 4 > 32:
            continue
        a = min(math.isqrt(rem), 255)
        for x in range(a, max(a - 40, -1), -1):
            r1 = rem - x * x
            b = min(math.isqrt(r1), 255)
            for y in range(b, max(b - 40, -1), -1):
                if r1 - y * y in two:
                    row[:t] = 255
                    row[t:t + 4] = (x, y) + two[r1 - y * y]
                    return row
    return None
