"""The transcription of the occupancy map's queries (tests/occupancy_query_cases.py, a literal reading of include/sbm.h,
"occupancy map: queries") against what the reference's own octomap answered for search and castRay
(tests/golden/occupancy_query.npz, tools/make_occupancy_query_fixtures.py): every recorded state, log-odds, return value and
`end`, bit for bit, over maps built by the insert transcription from the recorded scans. No GPU, no library."""
import functools
import hashlib
import json
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_query_cases as qc  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402
import occupancy_ref as occ  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "occupancy_query.npz"
FX = dict(np.load(GOLDEN))
TREES = [str(t) for t in FX["trees"]]
RES = float(FX["resolution"])


def sets_of(tree, kind):
    """The tree's query sets that hold rays / points."""
    return [f"{tree}_{s}" for s in FX[f"{tree}_sets"] if f"{tree}_{s}_{kind}" in FX]


RAY_SETS = [s for t in TREES for s in sets_of(t, "rays")]
POINT_SETS = [s for t in TREES for s in sets_of(t, "state")]


def scans_of(tree):
    n = FX[f"{tree}_npoints"]
    ends = np.cumsum(n)
    return [(FX[f"{tree}_origins"][i], float(FX[f"{tree}_scan_range"][i]), FX[f"{tree}_points"][e - k:e])
            for i, (k, e) in enumerate(zip(n, ends))]


@functools.lru_cache(maxsize=None)
def restated(tree):
    """The transcription's map of a tree, built once: the insert transcription over the recorded scans, or the key list."""
    if int(FX[f"{tree}_hits"]):
        return qc.Map(dict(zip((int(k) for k in FX[f"{tree}_keys"]), (int(c) for c in FX[f"{tree}_counts"]))), qc.HITS, 0.0, RES)
    t = rc.Tree(rc.RayParams(*[float(v) for v in FX[f"{tree}_params"]]), RES)
    for o, max_range, p in scans_of(tree):
        t.rp.max_range = max_range
        t.insert(p, o)
    return qc.Map(dict(t.v), qc.LOGODDS, FX[f"{tree}_constants"][4], RES)


def tree_of(tag):
    return max((t for t in TREES if tag.startswith(t + "_")), key=len)


def test_fixture_is_the_committed_one():
    want = GOLDEN.with_suffix(".sha256").read_text().split()[0]
    assert hashlib.sha256(GOLDEN.read_bytes()).hexdigest() == want
    cpu = json.loads((ROOT / "tests" / "golden" / "occupancy_query_cpu.json").read_text())
    assert cpu["octomap_ms_per_ray"] > 0 and cpu["rays"] == cpu["view"][0] * cpu["view"][1]


@pytest.mark.parametrize("tree", TREES)
def test_the_insert_transcription_builds_the_recorded_tree(tree):
    m = restated(tree)
    keys = np.array(sorted(m.v), np.uint64)
    assert np.array_equal(keys, FX[f"{tree}_keys"])
    if m.mode == qc.LOGODDS:
        assert np.array_equal(np.array([m.v[int(k)] for k in keys], np.float32).view(np.uint32), FX[f"{tree}_logodds"].view(np.uint32))
        assert np.array_equal(np.array(rc.constants(rc.RayParams(*[float(v) for v in FX[f"{tree}_params"]])), np.float32).view(np.uint32),
                              FX[f"{tree}_constants"].view(np.uint32))


@pytest.mark.parametrize("tag", RAY_SETS)
def test_cast_ray_equals_octomap(tag):
    m = restated(tree_of(tag))
    rays, ignore, max_range = FX[f"{tag}_rays"], FX[f"{tag}_ignore"], FX[f"{tag}_max_range"]
    status, end = np.empty(len(rays), np.int32), np.empty((len(rays), 3), np.float32)
    for i, r in enumerate(rays):
        status[i], end[i] = m.cast_ray(r[:3], r[3:], bool(ignore[i]), float(max_range[i]))
    assert np.array_equal(status == qc.RAY_HIT, FX[f"{tag}_ret"].astype(bool))           # castRay's return value
    untouched = np.isnan(FX[f"{tag}_end"]).all(axis=1)                                   # octomap left its `end` alone
    assert np.array_equal(status == qc.RAY_NONE, untouched)
    assert np.array_equal(end[~untouched].view(np.uint32), FX[f"{tag}_end"][~untouched].view(np.uint32))
    assert np.isnan(end[untouched]).all()
    assert np.array_equal(status, FX[f"{tag}_status"])


@pytest.mark.parametrize("tag", POINT_SETS)
def test_search_equals_octomap(tag):
    m = restated(tree_of(tag))
    state, value = m.search_all(FX[f"{tag}_points"])
    found = FX[f"{tag}_found"].astype(bool)
    assert np.array_equal(state > 0, found) and np.array_equal(state == qc.CELL_OCCUPIED, FX[f"{tag}_occupied"].astype(bool))
    assert np.array_equal(state, FX[f"{tag}_state"])
    if m.mode == qc.LOGODDS:
        assert np.array_equal(value[found], FX[f"{tag}_value"].view(np.uint32)[found])   # octomap's getLogOdds, bit for bit
        assert np.isnan(value[~found].view(np.float32)).all()
    else:
        assert (value[~found] == 0).all() and (value[found] > 0).all()


def test_every_status_and_state_occurs():
    status = np.concatenate([FX[f"{s}_status"] for s in RAY_SETS])
    assert set(status.tolist()) == {qc.RAY_NONE, qc.RAY_HIT, qc.RAY_RANGE, qc.RAY_UNKNOWN, qc.RAY_BOUNDS}
    state = np.concatenate([FX[f"{s}_state"] for s in POINT_SETS])
    assert set(state.tolist()) == {qc.CELL_OUT, qc.CELL_UNKNOWN, qc.CELL_FREE, qc.CELL_OCCUPIED}


def test_the_cases_say_what_they_claim():
    """What the generator asserted when it wrote the fixture, from the fixture alone."""
    assert FX["wall2_range_status"].tolist() == [qc.RAY_HIT, qc.RAY_HIT, qc.RAY_RANGE, qc.RAY_HIT, qc.RAY_HIT, qc.RAY_RANGE]
    inside, on, outside = FX["wall2_range_values"]
    assert FX["wall2_range_max_range"].tolist() == [inside, on, outside, 0.0, -1.0, 1.0]
    c = FX["wall2_origins"][0]
    e = FX["wall2_range_end"][1]
    dist = sum(float((e[j] - c[j]) * (e[j] - c[j])) for j in range(3))
    assert inside * inside > dist == on * on > outside * outside
    assert FX["gap_gap_status"].tolist() == [qc.RAY_UNKNOWN, qc.RAY_UNKNOWN, qc.RAY_HIT, qc.RAY_RANGE]
    c = FX["thres_constants"]
    assert c[3] == c[4] and (FX["thres_logodds"] == c[3]).sum() == 1                     # one voxel at the clamp = the threshold
    assert FX["thres_clamp_status"].tolist() == [qc.RAY_HIT, qc.RAY_UNKNOWN]
    above = qc.Map(restated("thres").v, qc.LOGODDS, np.nextafter(c[4], np.float32(np.inf)), RES)    # what `>` would answer
    assert above.cast_ray(*np.split(FX["thres_clamp_rays"][0], 2))[0] != qc.RAY_HIT
    origin = FX["box_origin_status"].reshape(3, 2, 2)          # start cell occupied / free / unknown x ignore x (direction, zero)
    assert (origin[0] == qc.RAY_HIT).all()
    assert origin[1].tolist() == [[qc.RAY_HIT, qc.RAY_NONE]] * 2
    assert origin[2].tolist() == [[qc.RAY_UNKNOWN, qc.RAY_UNKNOWN], [qc.RAY_HIT, qc.RAY_NONE]]
    assert (FX["box_bounds_status"][[0, 1, 3, 4]] == qc.RAY_BOUNDS).all()
    assert (FX["box_lengths_status"] == qc.RAY_HIT).all()      # three lengths of one direction: the float normalisation rounds
    assert len(np.unique(FX["box_lengths_end"][:, 0])) == 1    # differently, so the rays may part; all reach the same face
    for tree in ("scene", "scene_hits"):
        pts = FX[f"{tree}_search_points"][1::2].astype(np.float64) / RES
        assert (np.abs(pts - np.round(pts)).min(axis=1) < 1e-4).all()                    # every second point lies on a voxel face


def test_view_rays_from_the_header_formula_equal_the_recorded_sample():
    m = occ.model_from_array(FX["scene_model"])
    origins, dirs = qc.view_rays(40, 30, int(FX["scene_scale"]), m, FX["scene_poses"][0])
    for tree in ("scene", "scene_hits"):
        rec = FX[f"{tree}_view_rays"]
        assert np.array_equal(origins.view(np.uint32), rec[:, :3].view(np.uint32))
        assert np.array_equal(dirs.view(np.uint32), rec[:, 3:].view(np.uint32))
