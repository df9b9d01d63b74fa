"""The transcription tests/occupancy_planner_cases.py against what the reference's own octomap answered
(tests/golden/occupancy_planner.npz, made by tools/make_occupancy_planner_fixtures.py): begin_leafs_bbx by keys and by points,
getUnknownLeafCenters, the metric bounds expanded and pruned, and getRayIntersection, every recorded answer bit for bit. No GPU, no
library. The trees are rebuilt from the earlier fixtures, as the generator built them."""
import hashlib
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "tests"), str(ROOT / "oracle")]
import occupancy_planner_cases as pc  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402
import occupancy_tree_cases as tc  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
FX = dict(np.load(GOLDEN / "occupancy_planner.npz"))
FXT = dict(np.load(GOLDEN / "occupancy_tree.npz"))
FXQ = dict(np.load(GOLDEN / "occupancy_query.npz"))
TREES = [str(t) for t in FX["trees"]]
RES = float(FX["resolution"])


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def voxels_of(name):
    """{packed key: float32} under the reading the fixture used: the log-odds, or clamp max for the hit-mode tree"""
    if name == "empty":
        return {}
    if int(FX[f"{name}_hits"]):
        return tc.max_likelihood({int(k): 0 for k in FXQ["scene_hits_keys"]}, tc.HITS, FXT[f"{name}_constants"])
    src = FXT if f"{name}_keys" in FXT else FXQ
    return dict(zip((int(k) for k in src[f"{name}_keys"]), src[f"{name}_logodds"]))


_TREES = {}


def tree_of(name):
    if name not in _TREES:
        _TREES[name] = tc.Tree(voxels_of(name), RES)
    return _TREES[name]


def recorded_boxes(name):
    """[(by points, lo, hi, max depth, (keys, depths, values))] of one tree"""
    ends = np.cumsum(FX[f"{name}_bbx_n"])
    rows = [(False, tuple(int(v) for v in b[:3]), tuple(int(v) for v in b[3:6]), int(b[6])) for b in FX[f"{name}_bbx_boxes"]]
    rows += [(True, b[:3], b[3:], int(d)) for b, d in zip(FX[f"{name}_bbx_point_boxes"], FX[f"{name}_bbx_point_depths"])]
    assert len(rows) == len(ends)
    return [row + ((FX[f"{name}_bbx_key"][e - n:e], FX[f"{name}_bbx_depth"][e - n:e].astype(np.int32), FX[f"{name}_bbx_value"][e - n:e]),)
            for row, n, e in zip(rows, FX[f"{name}_bbx_n"], ends)]


def recorded_unknown(name):
    ends = np.cumsum(FX[f"{name}_unknown_n"])
    return [(b[:3], b[3:], int(d), tuple(int(s) for s in steps), FX[f"{name}_unknown_xyz"][e - n:e])
            for b, d, steps, n, e in zip(FX[f"{name}_unknown_boxes"], FX[f"{name}_unknown_depths"], FX[f"{name}_unknown_steps"],
                                         FX[f"{name}_unknown_n"], ends)]


def test_the_fixture_is_the_committed_one():
    want = (GOLDEN / "occupancy_planner.sha256").read_text().split()[0]
    assert hashlib.sha256((GOLDEN / "occupancy_planner.npz").read_bytes()).hexdigest() == want
    assert (GOLDEN / "occupancy_planner.npz").stat().st_size <= max(p.stat().st_size for p in GOLDEN.glob("occupancy_*.npz") if "planner" not in p.name)


@pytest.mark.parametrize("name", TREES)
def test_metric_bounds_expanded_and_pruned(name):
    t = tree_of(name)
    want = [pc.metric(t, False), pc.metric_calc(t, False), pc.metric(t, True), pc.metric_calc(t, True)]
    flat = np.array([v for lo, hi in want for v in lo + hi], np.float64)
    m = FX[f"{name}_metric"]
    assert np.array_equal(flat.view(np.uint64), m[:24].view(np.uint64))
    assert np.float64(pc.volume(*want[3])).view(np.uint64) == m[24:].view(np.uint64)[0]
    if name == "empty":
        assert not m.any()


def test_metric_cases_the_fixture_must_hold():
    one, cube = FX["one_metric"], FX["cube64_metric"]
    k = FXT["one_keys"]
    assert len(k) == 1 and np.allclose(one[15:18] - one[12:15], RES)                      # a tree of one voxel: one cell wide
    assert np.allclose(cube[15:18] - cube[12:15], 4 * RES) and tree_of("cube64").leaves(0)[1].tolist() == [14]      # the extreme leaf is a collapsed node
    differ = [n for n in TREES if not np.array_equal(FX[f"{n}_metric"][:6].view(np.uint64), FX[f"{n}_metric"][12:18].view(np.uint64))]
    assert differ, "octomap's bounds before and after prune() differ in the last bit for some tree: the tree answers the pruned ones"
    assert all(np.allclose(FX[f"{n}_metric"][:6], FX[f"{n}_metric"][12:18], rtol=0, atol=1e-9) for n in TREES)


@pytest.mark.parametrize("name", [n for n in TREES if len(FX[f"{n}_bbx_n"])])
def test_box_iterator(name):
    t = tree_of(name)
    loose = 0
    for points, lo, hi, depth, (k, d, v) in recorded_boxes(name):
        got = pc.leaves_bbx_points(t, lo, hi, depth, octomap=True) if points else pc.leaves_bbx(t, lo, hi, depth)
        assert np.array_equal(got[0], k) and np.array_equal(got[1], d) and np.array_equal(bits(got[2]), bits(v)), (name, lo, hi, depth)
        if points:
            if not pc.corners_have_keys(t, lo, hi):           # the divergence: octomap's loop visits the root once, the library nothing
                assert len(k) == (1 if t.level[0] else 0) and len(pc.leaves_bbx_points(t, lo, hi, depth)[0]) == 0
            continue
        node = pc.leaves_bbx_by_node(t, lo, hi, depth)        # a node's own test implies its ancestors'
        assert np.array_equal(node[0], k) and np.array_equal(node[1], d)
        full = t.leaves(depth)
        at = np.searchsorted(np.array([rc.morton(int(q)) for q in full[0]]), [rc.morton(int(q)) for q in k]) if len(k) else []
        assert all(full[0][i] == q for i, q in zip(at, k)), "a subsequence of leaves(max_depth), in its order"
        if (lo, hi) == ((0, 0, 0), (65535, 65535, 65535)):
            assert np.array_equal(full[0], k) and np.array_equal(full[1], d)
        if any(lo[a] > hi[a] for a in range(3)):
            assert (d < 16).all()
        loose += sum(1 for q, dd in zip(k, d) if dd < 16 and any(lo[a] == ((int(q) >> (32 - 16 * a)) & 0xFFFF) + (32768 >> int(dd)) for a in range(3)))
    if name in ("sib8", "cube64"):
        assert loose > 0, "no box visits a cube through its one-past-end key"


@pytest.mark.parametrize("name", [n for n in TREES if len(FX[f"{n}_unknown_n"])])
def test_unknown_cells(name):
    t = tree_of(name)
    for lo, hi, depth, steps, xyz in recorded_unknown(name):
        st, got, mine = pc.unknown_centers(t, lo, hi, depth)
        assert st == 0 and tuple(mine) == steps and np.array_equal(bits(got), bits(xyz)), (name, lo, hi, depth)


def test_unknown_cells_the_fixture_must_hold():
    grids, depths, drift, absent = set(), set(), 0, 0
    for name in TREES:
        t = tree_of(name)
        for lo, hi, depth, steps, xyz in recorded_unknown(name):
            grids.add(steps), depths.add(depth or 16)
            cells = steps[0] * steps[1] * steps[2]
            if len(xyz):
                d = depth or 16
                closed = np.array([[np.float32(pc.key_to_coord(pc.coord_to_key(c, d, 1.0 / RES), d, RES)) for c in p] for p in xyz])
                drift += int((bits(closed) != bits(xyz)).any())
            plo = pc.unknown_plan(RES, lo, hi, depth)[1]
            if cells and t.search(plo, depth)[0] == tc.CELL_UNKNOWN:
                assert not (bits(xyz) == bits(plo)).all(axis=1).any()
                absent += 1
    assert {(1, 1, 1), (1, 1, 65), (5, 4, 3), (12, 12, 12), (0, 0, 0)} <= grids and {16, 15, 14} <= depths
    assert any(0 in g and max(g) > 0 for g in grids) and drift and absent
    assert pc.unknown_plan(RES, [3276.85, 0, 0], [0, 0, 0], 0)[0] == pc.SIZE and pc.unknown_plan(RES, [0, 0, 0], [0, float("nan"), 0], 0)[0] == pc.SIZE
    assert pc.unknown_plan(RES, [-60, -60, -60], [60, 60, 60], 16)[0] == pc.UNSUPPORTED      # 1200^3 cells
    st, _, _, steps = pc.unknown_plan(RES, [-50, -50, -50], [50, 50, 50], 16)                 # about 1000^3 cells are accepted
    assert st == 0 and 999 ** 3 <= steps[0] * steps[1] * steps[2] <= pc.MAX_CELLS
    assert pc.unknown_plan(RES, [1, 1, 1], [0, 2, 2], 16)[3][0] == 0                           # pmax below pmin: no steps


def test_ray_entries():
    rows, found, xyz = FX["ray_cases"], FX["ray_found"], FX["ray_xyz"]
    for i, row in enumerate(rows):
        f, p = pc.ray_intersection(RES, row[:3], row[3:6], row[6:9], row[9])
        assert f == bool(found[i]) and np.array_equal(bits(p), bits(xyz[i])), (i, row)
    assert found.any() and not found.all() and np.isnan(xyz[found == 0]).all()
    d = rows[:, 3:6]
    assert (np.isnan(d).any(axis=1) & (found == 1)).any() and (np.isinf(d).any(axis=1) & (found == 1)).any()     # need no special case
    assert ((d == 0).all(axis=1) & (found == 0)).any()
    assert {0.0, 1e-3, -1e-3} <= set(rows[:, 9].tolist())
    norms = np.linalg.norm(np.where(np.isfinite(d), d, 0), axis=1)
    assert (np.abs(norms - 1) > 0.5).any()                                                   # un-normalised directions
