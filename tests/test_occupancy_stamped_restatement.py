"""tests/occupancy_stamped_cases.py, the numpy transcription of the time stamps' contract in include/sbm.h, against what the
reference's own octomap (OcTreeStamped) recorded in tests/golden/occupancy_stamped.npz: equal in every integer and float bit,
after every step of every case. And the hand-built cases the contract text itself names. No GPU, no library."""
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_stamped_cases as sc  # noqa: E402


def test_the_fixture_names_its_cases():
    assert sc.NAMES == ["scans", "scans_discrete", "scans_box", "scans_detect", "degrade", "edits", "blocks", "resume", "older"]
    assert float(sc.FX["resolution"]) == 0.1


@pytest.mark.parametrize("name", sc.NAMES)
def test_the_restatement_equals_octomap_after_every_step(name):
    case, theirs = sc.case_of(name), sc.recorded(name)
    mine = sc.run_case(case)
    assert len(mine) == len(theirs) == len(case["steps"])
    for i, (a, b) in enumerate(zip(mine, theirs)):
        assert sc.same(a, b), (name, i)
    m = sc.Map(case["params"])
    assert np.array_equal(np.float32([m.hit, m.miss, m.cmin, m.cmax, m.thres]).view(np.uint32), sc.FX[f"{name}_constants"].view(np.uint32))


def test_what_the_cases_show():
    """The consequences the contract names are in the recording, not only in the restatement"""
    m = sc.Map(sc.case_of("scans")["params"])
    keys, lo, stamps, _ = sc.recorded("scans")[2]                     # after the scans at 1000, 1010, 1020 from one origin
    assert ((lo == m.cmax) & (stamps == 1010)).sum() > 20, "a wall keeps the stamp of its saturating hit: older than the last scan that hit it"
    assert ((lo == m.cmin) & (stamps == 1010)).sum() > 100, "a region that is only ever free saturates at clamp min"
    assert (stamps == 1020).sum() > 50, "beside voxels the third scan did stamp"
    steps, rec = sc.case_of("degrade")["steps"], sc.recorded("degrade")
    kinds = [s["kind"] for s in steps]
    first = kinds.index(sc.DEGRADE)
    assert (rec[first - 1][2] == 0).sum() == 6 and steps[first - 1]["kind"] == sc.EDIT, "setNodeValue creates voxels of stamp 0"
    assert any(s["kind"] == sc.DEGRADE and s["thres"] == 0 for s in steps)
    below = [i for i, s in enumerate(steps) if s["kind"] == sc.DEGRADE and s["clock"] < 1000]
    assert below and rec[below[0]][3] > 100, "a clock below the stamps: the wrap makes a huge age"
    counts = [rec[i][3] for i, k in enumerate(kinds) if k == sc.DEGRADE]
    assert 0 in counts[1:] and counts[-1] > 0, "repeated until nothing is occupied; after a hit it degrades again"
    for i in range(first, len(steps)):
        if kinds[i] == sc.DEGRADE:
            assert np.array_equal(rec[i][2], rec[i - 1][2]) and np.array_equal(rec[i][0], rec[i - 1][0]), "a degrade touches no stamp"
    e = sc.recorded("edits")
    assert sorted(set(map(int, e[0][2]))) == [0, 2000] and sorted(set(map(int, e[1][2]))) == [0, 2000, 2500]
    o = sc.recorded("older")
    assert [r[3] for r in o[-3:]] == [len(o[-4][0]) - len(o[-3][0]), len(o[-3][0]) - len(o[-2][0]), len(o[-2][0]) - len(o[-1][0])] and len(o[-1][0]) > 0


def test_eight_siblings_collapse_only_where_the_stamps_agree():
    """sbm.h: eight siblings of equal value and equal stamps are 16 nodes and 1 leaf, with one stamp different 24 nodes and 8 leaves"""
    keys = [sc.rc.pack3((32768 + 10 + (c & 1), 32768 + 20 + (c >> 1 & 1), 32768 + 30 + (c >> 2 & 1))) for c in range(8)]
    v = {k: np.float32(3.5) for k in keys}
    t = sc.StampedTree(v, {k: 100 for k in keys}, 200)
    assert (t.size, t.num_leaves, t.root_stamp) == (16, 1, 200) and list(t.leaves_stamps()[3]) == [100] and list(t.leaves_stamps()[1]) == [15]
    for odd in (0, 7):
        t = sc.StampedTree(v, {k: 101 if i == odd else 100 for i, k in enumerate(keys)}, 200)
        assert (t.size, t.num_leaves) == (24, 8) and list(t.leaves_stamps(15)[3]) == [200], odd
        assert sorted(t.leaves_stamps()[3]) == [100] * 7 + [101]
    plain = sc.tc.Tree(v)
    assert (plain.size, plain.num_leaves) == (16, 1), "the plain tree ignores the stamps"
    t = sc.StampedTree({**v, keys[0]: np.float32(1.0)}, {k: 100 for k in keys}, 200)
    assert (t.size, t.num_leaves) == (24, 8), "and unequal values do not collapse either"
    assert sc.OT_HEADER.count("id OcTreeStamped") == 1 and sc.StampedTree(v, {k: 100 for k in keys}, 200).ot().endswith(sc.otc.body(plain))


def test_what_the_tree_cases_show():
    rec = sc.recorded("blocks")
    (nodes1, root1, ot1), (ml1, mroot1, bt1) = rec[2][4]
    (nodes2, root2, ot2), _ = rec[4][4]
    assert root1 == mroot1 == 3010 and root2 == 3020 and len(nodes1[0]) == 105 and len(nodes2[0]) == 73
    assert b"\nid OcTreeStamped\n" in ot1 and b"\nid OcTreeStamped\n" in bt1 and len(ot1) - ot1.index(b"data\n") - 5 == 5 * 105
    assert set(map(int, nodes1[3][nodes1[4] == 0])) == {3010}, "every open inner node has the clock of the build"
    assert set(map(int, nodes2[3][(nodes2[4] == 1) & (nodes2[1] < 16)])) == {3000}, "every collapsed node has its children's common stamp"
    r = sc.recorded("resume")
    kinds = [s["kind"] for s in sc.case_of("resume")["steps"]]
    i = kinds.index(sc.RESUME)
    assert not r[i][2].any() and np.array_equal(r[i][0], r[i - 1][0]) and r[i - 1][2].any(), "a tree read back has stamp 0 everywhere"
    assert r[i + 1][2].any() and (r[i + 1][2] == 0).any()


def test_ten_hits_saturate_at_the_fifth_and_keep_its_clock():
    """sbm.h: a wall hit ten times at clocks 1000..1009 saturates at the fifth hit and keeps stamp 1004; the degrade degrades it
    although it was seen a second ago; after that it is below the clamp and the next hit stamps it again"""
    m = sc.Map()                                   # octomap's defaults: hit 0.85, clamp max 3.5
    key = sc.rc.pack3((32768, 32768, 32768))
    stamps = []
    for c in range(1000, 1010):
        m.clock = c
        m.update_node(key, m.hit)
        stamps.append(m.s[key])
    assert stamps == [1000, 1001, 1002, 1003, 1004] + [1004] * 5 and m.v[key] == m.cmax
    m.clock = 1010
    assert m.degrade(5) == 1 and m.s[key] == 1004 and m.v[key] == np.float32(m.cmax + m.miss)
    m.update_node(key, m.hit)
    assert m.s[key] == 1010 and m.v[key] == m.cmax
    # the same through a scan's one update per voxel
    n = sc.Map()
    p = np.float32([[0.15, 0.25, 0.35]])
    for c in range(1000, 1010):
        n.clock = c
        n.insert(p, p[0])
    assert list(n.stamped()[2]) == [1004]


def test_the_two_inequalities_and_the_calls_that_never_stamp():
    m = sc.Map()
    a, b, c = (sc.rc.pack3((32768 + i, 32768, 32768)) for i in range(3))
    m.clock = 10
    m.set_node_value(a, 100.0)                     # clamp max, stamp 0
    m.set_node_value(b, -100.0)                    # clamp min, stamp 0
    m.update_node(c, 0.0)                          # a voxel that does not exist: created, stamped
    assert (m.s[a], m.s[b], m.s[c]) == (0, 0, 10) and m.v[c] == 0
    m.clock = 11
    m.update_node(a, 0.0), m.update_node(b, 0.0), m.update_node(c, 0.0)   # an update of exactly 0 tests both inequalities
    assert (m.s[a], m.s[b], m.s[c]) == (0, 0, 11)
    m.update_node(a, -0.5), m.update_node(b, 0.5)
    assert (m.s[a], m.s[b]) == (11, 11)
    m.clock = 12
    m.set_node_value(a, 1.0)                       # on an existing voxel: the stamp stays
    assert m.s[a] == 11
    m.edit([c, c], [sc.ec.DELETE, sc.ec.SET], [0.0, 1.0])
    assert m.s[c] == 0, "deleted and created again inside one batch: from stamp 0"
    m.clock = 5                                    # nothing requires the clock to be monotone
    assert sc.age(5, 11) == (1 << 32) - 6 and m.degrade(1000) == 1 and m.forget((1 << 32) - 7) == 2 and sorted(m.v) == [c]
