"""The numpy restatement of the visual-word dictionary (tests/vwd_cases.py) held to independent statements of the same rules: its
exhaustive search against a direct sort over (distance, index), and the NNDR test in float against the rational one on every
pair that sits exactly on the boundary."""
import numpy as np
import pytest

import vwd_cases as vc


@pytest.mark.parametrize("metric", [vc.L1, vc.L2], ids=["L1", "L2"])
def test_search_equals_a_sort_over_distance_then_index(metric):
    rng = np.random.default_rng(4)
    for N in (0, 1, 2, 3, 70):
        words = rng.integers(0, 4, (N, 32), dtype=np.uint8)   # few values: many equal distances
        q = rng.integers(0, 4, (50, 32), dtype=np.uint8)
        if N > 2:
            words[N // 2] = words[0]                          # duplicate rows
            q[0] = words[0]
        for chunk in (1 << 16, 1, 7):
            rec = vc.search(q, words, metric, chunk=chunk)
            d = vc.distances(q, words, metric)
            for i in range(len(q)):
                order = np.lexsort((np.arange(N), d[i]))      # by distance, then by index
                want = [-1, vc.NONE, -1, vc.NONE]
                for k in range(min(2, N)):
                    want[2 * k], want[2 * k + 1] = order[k], d[i, order[k]]
                assert list(rec[i]) == want, (N, chunk, i)
    assert vc.MAX_DIST == {vc.L1: 8160, vc.L2: 2080800}


@pytest.mark.parametrize("metric", [vc.L1, vc.L2], ids=["L1", "L2"])
def test_float_nndr_on_every_boundary_pair(metric):
    """On 5 d0 == 4 d1 the rational test d0 > 0.8 d1 is false. 0.8f lies above 4/5 by 1.49e-8 of it, less than half a unit in the
    last place of any float, so 0.8f * d1 rounds to d0 itself or above and the float test is false too: no pair differs. The
    product of a 24-bit and a 21-bit integer significand is exact in double, so rounding it once to float is the float product."""
    pairs = vc.boundary_pairs(metric)
    assert len(pairs) == vc.MAX_DIST[metric] // 5 and (5 * pairs[:, 0] == 4 * pairs[:, 1]).all()
    f32 = vc.float_test(pairs[:, 0], pairs[:, 1])
    exact = pairs[:, 0].astype(np.float64) > (float(vc.NNDR) * pairs[:, 1].astype(np.float64)).astype(np.float32).astype(np.float64)
    rational = 5 * pairs[:, 0] > 4 * pairs[:, 1]
    differ = int((f32 != rational).sum())
    print(f"metric {metric}: {len(pairs)} boundary pairs, float test differs from the rational one on {differ}")
    assert np.array_equal(f32, exact)
    assert differ == int((exact != rational).sum()) == 0
    # one step either side the two tests agree as well, and say different things
    up, down = vc.float_test(pairs[:, 0] + 1, pairs[:, 1]), vc.float_test(pairs[:, 0] - 1, pairs[:, 1])
    assert up.all() and not down.any()


def test_rows_at_a_distance():
    for metric in (vc.L1, vc.L2):
        for d in (0, 1, 254, 255, 256, 4080, 8160, 65025, 65026, 130051, 1664640, 2080800):
            if d > vc.MAX_DIST[metric]:
                continue
            row = vc.row_at_distance(d, metric)
            assert row is not None and vc.distances(np.zeros((1, 32), np.uint8), row[None], metric)[0, 0] == d
