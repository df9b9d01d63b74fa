"""The CPU restatement of buildOccupancyGridMap (oracle/occupancy_ref) against what the reference's own octomap recorded
(tests/golden/occupancy_octomap.npz, written by tools/make_occupancy_fixtures.py) and against the reprojection of the oracle."""
import hashlib
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "oracle"))
import occupancy_ref as occ  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "occupancy_octomap.npz"


@pytest.fixture(scope="module")
def fx():
    want = GOLDEN.with_suffix(".sha256").read_text().split()[0]
    assert hashlib.sha256(GOLDEN.read_bytes()).hexdigest() == want
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def restated(fx):
    """(norm, gate, key verdict, keys) of every recorded point."""
    p = occ.params(float(fx["resolution"]), float(fx["range_max"]))
    out = [occ.point(pt, o, p) for pt, o in zip(fx["points"], fx["origins"])]
    return (np.array([r[0] for r in out]), np.array([r[1] for r in out]), np.array([r[2] for r in out]),
            np.stack([r[3] for r in out]))


def accepted_keys(fx, bit):
    gate = fx["norm"] <= float(np.float32(fx["range_max"]) * np.float32(fx["range_max"]))
    take = gate & (fx["ok"] == 1) & ((fx["group"] >> bit) & 1 == 1)
    return np.unique(occ.pack(fx["keys"][take]))


def test_fixture_covers_its_cases(fx):
    ok, norm, pts = fx["ok"] == 1, fx["norm"], fx["points"]
    assert len(pts) < 5000 and ok.sum() > 3000 and (~ok).sum() > 100
    assert (norm[np.isfinite(norm)] > 25).sum() >= 10 and (norm == 25.0).any()
    near = np.abs(norm - 25.0) < 1e-4
    assert (near & (norm > 25)).any() and (near & (norm < 25)).any()
    for a in range(3):                              # zero straddled, the key range's last voxel and the one after it
        assert (pts[:, a] < 0).any() and (pts[:, a] == 0).any()
        edge = pts[:, a] == np.float32(3276.75)
        assert edge.any() and (fx["keys"][edge, a] == 65535).all() and ok[edge].all()
        assert not ok[pts[:, a] == np.float32(3276.8)].any()
    assert int(fx["leafs_blocks"]) == 1 + 1 + 7 and int(fx["size_empty"]) == 0


def test_every_norm_verdict_and_key(fx, restated):
    norm, gate, ok, keys = restated
    assert np.array_equal(norm, fx["norm"], equal_nan=True)
    assert np.array_equal(ok, fx["ok"] == 1)
    assert np.array_equal(keys[ok], fx["keys"][ok])
    assert np.array_equal(gate, fx["norm"] <= 25.0)


@pytest.mark.parametrize("name,bit", [("all", 0), ("blocks", 1), ("empty", 2)])
def test_write_binary_equals_octomap(fx, name, bit):
    keys = accepted_keys(fx, bit)
    data, nodes, leafs = occ.write_binary(keys, float(fx["resolution"]))
    assert nodes == int(fx[f"size_{name}"]) and leafs == int(fx[f"leafs_{name}"])
    assert data == fx[f"bt_{name}"].tobytes()
    # insertion order does not matter
    rng = np.random.default_rng(3)
    assert occ.write_binary(rng.permutation(keys), float(fx["resolution"]))[0] == data


def test_planes_give_the_recorded_points_and_keys(fx):
    """The fixture's planes and poses through the whole restatement: the recorded world points, and the keys octomap gave them."""
    m, scale = occ.model_from_array(fx["model"]), int(fx["scale"])
    n = fx["scene_disp"].size
    w = np.stack([occ.world(d, scale, m, pose) for d, pose in zip(fx["scene_disp"], fx["scene_poses"])])
    assert np.array_equal(w.reshape(-1, 3), fx["points"][:n], equal_nan=True)
    px = occ.pixel_keys(fx["scene_disp"], scale, m, fx["scene_poses"]).reshape(-1)
    take = (fx["ok"][:n] == 1) & (fx["norm"][:n] <= 25.0)
    assert np.array_equal(px != occ.EMPTY, take)
    assert np.array_equal(px[take], occ.pack(fx["keys"][:n][take]))
    keys, hits = occ.distinct(px)
    assert hits.sum() == take.sum() and np.all(np.diff(keys.astype(np.int64)) > 0)


def test_reprojection_equals_the_oracle(fx):
    import sbm_oracle

    rng = np.random.default_rng(5)
    disp = rng.integers(-16, 1200, (37, 53)).astype(np.int16)
    for local in (None, [0, 0, 1, 0.05, -1, 0, 0, 0, 0, -1, 0, 0.2]):
        mo = sbm_oracle.make_model(local=local)
        m = occ.model_from_array(occ.model_to_array(mo))
        for apply_local in (True, False):
            assert np.array_equal(occ.reproject(disp, 4, m, apply_local), sbm_oracle.reproject(disp, 4, mo, apply_local), equal_nan=True)
    # and the world point is that reprojection pushed through the pose in float, left to right
    mo = sbm_oracle.make_model()
    m = occ.model_from_array(occ.model_to_array(mo))
    pose = np.asarray(fx["scene_poses"][1], np.float32)
    p = sbm_oracle.reproject(disp, 4, mo, True)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    want = np.stack([pose[4 * r] * x + pose[4 * r + 1] * y + pose[4 * r + 2] * z + pose[4 * r + 3] for r in range(3)], axis=-1)
    assert want.dtype == np.float32
    assert np.array_equal(occ.world(disp, 4, m, pose), want, equal_nan=True)


def test_squared_range_quirk():
    """The reference compares the norm with range_max SQUARED: at the default 5 m a point 24 m away is kept."""
    p = occ.params()
    assert occ.point([24, 0, 0], [0, 0, 0], p)[1] and not occ.point([25.1, 0, 0], [0, 0, 0], p)[1]
    assert occ.point([3, 0, 0], [0, 0, 0], occ.params(range_max=1.5))[1] is False   # 3 > 2.25


# ---- the inputs of tests/test_gpu_occupancy_edges.py: their closed-form expectation against the restatement -----------------
import occupancy_cases as cases  # noqa: E402


def test_closed_form_at_the_range_edges():
    """-3276.8f lies below -3276.8 and is rejected; +-3276.75f are the first and the last voxel; 3276.8f is out."""
    t = np.zeros((5, 3), np.float32)
    t[:, 0] = [-3276.8, -3276.75, 3276.75, 3276.8, 0.0]
    planes, poses = cases.unit_planes(5), cases.zero_rotation_poses(t)
    px = occ.pixel_keys(planes, 1, occ.model(), poses).reshape(-1)
    assert list(px != occ.EMPTY) == [False, True, True, False, True]
    assert list(cases.unpack(px[[1, 2, 4]])[:, 0]) == [0, 65535, 32768]
    keys, hits = cases.closed_form(t)
    want = occ.distinct(px)
    assert np.array_equal(keys, want[0]) and np.array_equal(hits, want[1]) and len(keys) == 3


@pytest.mark.parametrize("n", cases.LATTICE_SIZES)
def test_lattice_case_is_what_it_claims(n):
    planes, poses, keys, hits = cases.lattice(n)
    assert len(keys) == n and np.all(np.diff(keys.astype(np.int64)) > 0) and int(keys.max()) <= cases.KEY_MAX
    assert np.array_equal(hits, 1 + np.arange(n) % 3) and planes.shape == (int(hits.sum()), 1, 1)
    for got in (occ.insert(planes, 1, occ.model(), poses), cases.closed_form(poses[:, [3, 7, 11]])):
        assert np.array_equal(got[0], keys) and np.array_equal(got[1], hits)
    if n >= 5000:
        for byte in range(6):
            assert len(np.unique((keys >> np.uint64(8 * byte)) & np.uint64(255))) >= 200, byte
    if n == cases.WITH_ENDS:
        assert keys[0] == 0 and keys[-1] == cases.KEY_MAX and keys[-1] != occ.EMPTY
    # the planes do not arrive in key order
    first = cases.closed_form(poses[:64, [3, 7, 11]])[0]
    assert n < 64 or not np.array_equal(first, keys[:len(first)])


@pytest.mark.parametrize("byte", range(6))
def test_one_byte_case_is_what_it_claims(byte):
    planes, poses, keys, hits = cases.one_byte_case(byte)
    assert len(planes) == 300 and len(keys) == 256 and sorted(np.unique(hits)) == [1, 2]
    got = occ.insert(planes, 1, occ.model(), poses)
    assert np.array_equal(got[0], keys) and np.array_equal(got[1], hits)
    for b in range(6):
        digits = np.unique((keys >> np.uint64(8 * b)) & np.uint64(255))
        assert len(digits) == (256 if b == byte else 1)


def pattern_keys(name):
    plane, pose = cases.pattern(name)
    return occ.pixel_keys(plane, 1, occ.model(), pose).reshape(-1)


def test_pattern_abab():
    k = pattern_keys("abab")
    assert len(k) == 64 and k[0] != k[1] and occ.EMPTY not in (k[0], k[1])
    assert (k[0::2] == k[0]).all() and (k[1::2] == k[1]).all()


def test_pattern_runs():
    k = pattern_keys("runs")
    assert len(k) == 128
    groups = [k[g:g + 6] for g in range(0, 126, 6)]
    for g in groups:                                           # K K - K K -
        assert g[2] == occ.EMPTY and g[5] == occ.EMPTY and g[0] != occ.EMPTY and (g[[0, 1, 3, 4]] == g[0]).all()
    assert all(a[0] != b[0] for a, b in zip(groups, groups[1:]))
    assert (k[60:62] == k[63]).all() and k[63] == k[64] and k[62] == occ.EMPTY     # a run straddles the two wavefronts
    first = [g[0] for g in groups[:10]]
    assert len(set(first)) < len(first)                        # and a key comes back later in the same wavefront


@pytest.mark.parametrize("name,w", [("tail65", 65), ("tail129", 129)])
def test_pattern_tail(name, w):
    k = pattern_keys(name)
    assert len(k) == w and w % 64 == 1 and k[-1] == k[0] != occ.EMPTY
    assert (k[1:-1] != k[0]).all() and (k != occ.EMPTY).all() and len(np.unique(k[:64])) > 8


def test_pattern_blocks():
    plane, _ = cases.pattern("blocks")
    k = pattern_keys("blocks")
    assert plane.shape == (3, 100) and (k != occ.EMPTY).all()
    wave, block = np.arange(300) // 64, np.arange(300) // 256
    spans = [(set(wave[(k == v) & (block == 0)]), set(block[k == v])) for v in np.unique(k)]
    assert any(len(w0) >= 2 and b == {0, 1} for w0, b in spans)
