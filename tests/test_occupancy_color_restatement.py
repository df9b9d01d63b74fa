"""The restatement tests/occupancy_color_cases.py against every recording of tests/golden/occupancy_color.npz (what the reference's
own ColorOcTree answered), and what the cases claim about themselves. No GPU, no library. Every comparison is exact."""
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_color_cases as cc  # noqa: E402


def test_the_fixture_holds_the_cases():
    assert cc.NAMES == ["scans", "run300", "blocks", "reborn", "resume"]
    kinds = {name: [s["kind"] for s in cc.case_of(name)["steps"]] for name in cc.NAMES}
    assert all(k[-1] == cc.SNAPSHOT for k in kinds.values()) and cc.RESUME in kinds["resume"] and kinds["scans"].count(cc.SCAN) == 3
    assert all(len(s["points"]) <= 2000 for name in cc.NAMES for s in cc.case_of(name)["steps"])
    run = cc.case_of("run300")["steps"][1]
    assert (run["keys"] == run["keys"][0]).sum() == 300 and (run["keys"] >> np.uint64(48)).any() and (run["words"] == cc.WHITE).any()
    ops = [s["op"] for s in cc.case_of("run300")["steps"] if s["kind"] == cc.COLOR]
    assert ops == [cc.AVERAGE, cc.SET, cc.AVERAGE, cc.SET]
    reborn = cc.case_of("reborn")["steps"][2]
    assert reborn["kind"] == cc.EDIT and reborn["ops"][:2].tolist() == [cc.ec.DELETE, cc.ec.SET] and reborn["keys"][0] == reborn["keys"][1]
    pts = cc.case_of("scans")["steps"][1]["points"]
    assert not np.isfinite(pts).all() and (np.abs(pts[np.isfinite(pts).all(axis=1)]) > 3276.8).any(), "points outside the key space"


@pytest.mark.parametrize("name", cc.NAMES)
def test_the_restatement_equals_every_recording(name):
    mine, theirs = cc.run_case(cc.case_of(name)), cc.recorded(name)
    assert len(mine) == len(theirs) > 0
    for i, (a, b) in enumerate(zip(mine, theirs)):
        assert cc.same(a, b), (name, i)
    snaps = [b for b in theirs if isinstance(b[0], list)]
    assert snaps and all(len(s[0]) == len(cc.DEPTHS) and s[1].startswith(b"# Octomap OcTree file") and b"\nid ColorOcTree\n" in s[1] for s in snaps)


def test_the_designed_blocks_collapse_as_stated():
    case = cc.case_of("blocks")
    m = cc.Map(case["params"])
    for s in case["steps"][:2]:
        cc.apply_step(m, s)
    t = m.tree()
    keys, depth, _, words = t.leaves_colors(16)
    at = {(int(k), int(d)): int(w) for k, d, w in zip(keys, depth, words)}
    K = lambda i, j, k: cc.rc.pack3((32768 + i, 32768 + j, 32768 + k))                      # noqa: E731
    assert at[(K(65, -31, 17), 15)] == cc.WHITE, "child 0 white, siblings coloured: the collapsed node is white"
    sibs = [m.c.get(K(64 + i, -32 + j, 16 + k), cc.WHITE) for k in (0, 1) for j in (0, 1) for i in (0, 1)]
    assert sibs[0] == cc.WHITE and all(w != cc.WHITE for w in sibs[1:])
    kids = [m.c.get(K(-20 + i, 40 + j, 8 + k), cc.WHITE) for k in (0, 1) for j in (0, 1) for i in (0, 1)]
    assert kids[0] != cc.WHITE and kids.count(cc.WHITE) == 3 and at[(K(-19, 41, 9), 15)] == cc.average_child_color(kids) != cc.WHITE
    assert (K(130, 66, 34), 14) in at, "the 4^3 block collapses over two levels"
    assert not any(d == 15 and k == K(-63, -63, -63) for k, d in at) and sum(1 for k, d in at if d == 16) == 8, "the open block stays eight voxels"
    k15 = t.leaves_colors(15)
    inner = {(int(k), int(d)): int(w) for k, d, w in zip(k15[0], k15[1], k15[3])}[(K(-63, -63, -63), 15)]
    open_kids = [m.c.get(K(-64 + i, -64 + j, -64 + k), cc.WHITE) for k in (0, 1) for j in (0, 1) for i in (0, 1)]
    assert open_kids[0] == cc.WHITE and inner == cc.average_child_color(open_kids) != cc.WHITE, "a node that is not collapsed takes the average"


def test_averaging_is_order_dependent_and_restarts_at_white():
    a, b, c = cc.word(10, 20, 30), cc.word(200, 100, 0), cc.word(3, 3, 3)
    assert cc.step_color(cc.step_color(a, b, cc.AVERAGE), c, cc.AVERAGE) != cc.step_color(cc.step_color(a, c, cc.AVERAGE), b, cc.AVERAGE)
    assert cc.step_color(cc.WHITE, b, cc.AVERAGE) == b and cc.step_color(a, cc.word(255, 255, 255), cc.SET) == cc.WHITE
    assert cc.step_color(cc.word(255, 254, 255), cc.word(255, 255, 255), cc.AVERAGE) == cc.word(255, 254, 255), "(254 + 255) / 2 truncates"
    m = cc.Map()
    m.set_node_value(5, 1.0)
    m.color([5, 5, 5, 6, 5 | 1 << 48], [a, cc.WHITE, c, c, c], cc.SET)
    assert m.c == {5: c} and m.last_color == dict(items=5, found=3, unknown=1, skipped=1)
    m.delete([5])
    m.set_node_value(5, 1.0)
    assert m.colored()[2].tolist() == [cc.WHITE], "a voxel created again is white"
