"""The GPU occupancy map (u96-slam_amd/csrc/sbm_occupancy.hip) against the sequential C restatement (oracle/occupancy_ref) and
the reference's own octomap (tests/golden/occupancy_octomap.npz): sorted keys, hit counts and size are compared for exact
equality -- both sides perform the same IEEE operations in the same order without contraction, and a set has no order."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_ref as occ  # noqa: E402
from gpu_support import bm, build_callsite, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden" / "occupancy_octomap.npz"
LOCAL = [0, 0, 1, 0.05, -1, 0, 0, 0, 0, -1, 0, 0.2]


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def gpu_model(pkg, m):
    g = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(g), ctypes.byref(m), ctypes.sizeof(g))
    return g


def yaw_pose(yaw, t):
    c, s = np.cos(yaw), np.sin(yaw)
    return [c, -s, 0, t[0], s, c, 0, t[1], 0, 0, 1, t[2]]


def scene(n, h, w, seed):
    """Sloped planes with noise and invalid pixels, far rows beyond the gate; poses that turn and move."""
    rng = np.random.default_rng(seed)
    rows, cols = np.mgrid[0:h, 0:w]
    d = np.stack([10 + (900 * rows) // max(h - 1, 1) + cols // 2 + 25 * k + rng.integers(0, 4, (h, w)) for k in range(n)])
    d = d.astype(np.int16)
    d[rng.random(d.shape) < 0.05] = -16
    d[rng.random(d.shape) < 0.02] = 0
    poses = np.asarray([yaw_pose(0.4 * k - 0.3, (0.7 * k, -0.4 * k, 0.03 * k)) for k in range(n)], np.float32)
    return d, poses


def gpu_insert(pkg, bm, planes, scale, m, poses, capacity=1 << 15, calls=None, p=None):
    """The planes through a fresh map, in the given calls (lists of plane indices; default one call) -> (keys, hits, size)."""
    omap = pkg.OccupancyMap(bm, capacity, pkg.occ_params(p.resolution, p.range_max) if p else None)
    planes = np.ascontiguousarray(planes, np.int16)
    planes = planes[None] if planes.ndim == 2 else planes
    poses = occ.pose_rows(poses)
    for idx in (calls or [list(range(len(planes)))]):
        omap.insert(dev(planes[idx]), gpu_model(pkg, m), poses[idx], scale)
    keys, hits = omap.keys()
    size = omap.size()
    assert omap.overflow() == 0
    omap.close()
    return keys, hits, size


def check(pkg, bm, planes, scale, m, poses, what, **kw):
    want_k, want_h = occ.insert(planes, scale, m, poses, kw.get("p"))
    keys, hits, size = gpu_insert(pkg, bm, planes, scale, m, poses, **kw)
    assert size == len(want_k), (what, size, len(want_k))
    assert np.array_equal(keys, want_k), (what, "keys")
    assert np.array_equal(hits, want_h), (what, "hits")
    return want_k, want_h


def test_three_decimated_vga_planes(pkg, bm):
    planes, poses = scene(3, 120, 160, 1)
    k, h = check(pkg, bm, planes, 4, occ.model(local=LOCAL), poses, "vga/4")
    assert 1000 < len(k) < h.sum() < planes.size      # duplicates, and pixels that were skipped or gated out
    check(pkg, bm, planes, 4, occ.model(), poses, "vga/4 without a local transform")
    check(pkg, bm, planes, 4, occ.model(local=LOCAL), poses, "vga/4 at 5 cm, 2 m", p=occ.params(0.05, 2.0))


@pytest.mark.parametrize("h,w", [(1, 1), (5, 37), (1, 64), (3, 100)])
def test_small_and_partial_wavefronts(pkg, bm, h, w):
    planes, poses = scene(2, h, w, 2)
    planes = (np.abs(planes) + 150).astype(np.int16)           # every pixel valid and within the gate
    k, _ = check(pkg, bm, planes, 4, occ.model(local=LOCAL), poses, f"{w}x{h}")
    assert len(k) >= 1


def test_all_invalid_plane_gives_an_empty_map(pkg, bm):
    planes = np.full((2, 30, 40), -16, np.int16)
    planes[1] = 0
    keys, hits, size = gpu_insert(pkg, bm, planes, 4, occ.model(), [yaw_pose(0, (0, 0, 0))] * 2)
    assert size == 0 and len(keys) == 0 and len(hits) == 0


def test_every_pixel_in_one_voxel(pkg, bm):
    planes = np.full((1, 23, 47), 160, np.int16)
    pose = [0, 0, 0, 1.234, 0, 0, 0, -2.5, 0, 0, 0, 0.77]      # a zero rotation block: every point is the translation
    k, h = check(pkg, bm, planes, 4, occ.model(), [pose], "one voxel")
    assert len(k) == 1 and h[0] == 23 * 47


def test_64_distinct_keys_in_one_wavefront(pkg, bm):
    planes = np.full((1, 1, 64), 77, np.int16)                 # 10 m away: 8 px per column is 0.2 m
    k, h = check(pkg, bm, planes, 8, occ.model(), [yaw_pose(0, (0, 0, 0))], "64 distinct")
    assert len(k) == 64 and (h == 1).all()


def test_fixture_edge_points_as_planes(pkg, bm, fx):
    """The fixture's edge and norm cases, each a 1 x 1 plane under its pose: what octomap accepted, nothing else."""
    scale = int(fx["scale"])
    n0 = fx["scene_disp"].size
    for poses, m, first in ((fx["edge_poses"], occ.model_from_array(fx["model"]), n0),
                            (fx["norm_poses"], occ.model_from_array(fx["model_edge"]), n0 + len(fx["edge_poses"]))):
        planes = np.tile(fx["edge_disp"][None], (len(poses), 1, 1))
        keys, hits = check(pkg, bm, planes, scale, m, poses, "edge points")
        sl = slice(first, first + len(poses))
        take = (fx["ok"][sl] == 1) & (fx["norm"][sl] <= 25.0)
        want, cnt = np.unique(occ.pack(fx["keys"][sl][take]), return_counts=True)
        assert 0 < take.sum() < len(poses)
        assert np.array_equal(keys, want) and np.array_equal(hits, cnt)


def test_split_and_order_do_not_matter(pkg, bm):
    planes, poses = scene(5, 30, 40, 3)
    m = occ.model(local=LOCAL)
    one = gpu_insert(pkg, bm, planes, 4, m, poses)
    each = gpu_insert(pkg, bm, planes, 4, m, poses, calls=[[i] for i in range(5)])
    back = gpu_insert(pkg, bm, planes, 4, m, poses, calls=[[4, 3], [2], [1, 0]])
    for other in (each, back):
        assert np.array_equal(one[0], other[0]) and np.array_equal(one[1], other[1]) and one[2] == other[2]
    want = occ.insert(planes, 4, m, poses)
    assert np.array_equal(one[0], want[0]) and np.array_equal(one[1], want[1])


def test_more_planes_than_one_launch_takes(pkg, bm):
    planes, poses = scene(130, 6, 9, 4)
    check(pkg, bm, planes, 4, occ.model(local=LOCAL), poses, "130 planes")


def few_keys():
    """A 6 x 5 plane whose 30 pixels land in 30 voxels."""
    planes = np.full((1, 5, 6), 77, np.int16)
    m, pose = occ.model(), [yaw_pose(0, (0, 0, 0))]
    k, _ = occ.insert(planes, 8, m, pose)
    assert len(k) == 30
    return planes, m, pose


@pytest.mark.parametrize("capacity", [64, 16])
def test_probe_chains_in_a_small_table(pkg, bm, capacity):
    planes, m, pose = few_keys()
    check(pkg, bm, planes, 8, m, pose, f"capacity {capacity}", capacity=capacity)
    both = np.concatenate([planes, planes])
    check(pkg, bm, both, 8, m, pose * 2, f"capacity {capacity}, twice", capacity=capacity)


def test_a_table_too_small_says_so(pkg, bm):
    planes, m, pose = few_keys()
    omap = pkg.OccupancyMap(bm, 4)                              # 8 slots
    with pytest.raises(pkg.StereoBMError) as e:
        omap.insert(dev(planes), gpu_model(pkg, m), pose, 8)
    assert e.value.code == pkg.ERR_OCC_FULL
    with pytest.raises(pkg.StereoBMError):
        omap.keys()
    keys, hits = omap.keys(allow_overflow=True)
    want = occ.insert(planes, 8, m, pose)[0]
    assert omap.size() == len(keys) == 8 and np.isin(keys, want).all() and np.all(np.diff(keys.astype(np.int64)) > 0)
    assert omap.overflow() + int(hits.sum()) == 30
    # the host form reports it too, and reset clears it
    with pytest.raises(pkg.StereoBMError):
        omap.insert(planes, gpu_model(pkg, m), pose, 8)
    assert omap.overflow() + int(omap.keys(allow_overflow=True)[1].sum()) == 60
    omap.reset()
    assert omap.size() == 0 and omap.overflow() == 0
    omap.close()


def test_reset_then_reinsert(pkg, bm):
    planes, poses = scene(2, 30, 40, 5)
    other, _ = scene(2, 30, 40, 6)
    m = occ.model(local=LOCAL)
    omap = pkg.OccupancyMap(bm, 4096)
    omap.insert(dev(other), gpu_model(pkg, m), poses, 4)
    omap.reset()
    assert omap.size() == 0 and len(omap.keys()[0]) == 0
    omap.insert(dev(planes), gpu_model(pkg, m), poses, 4, sync=False)
    keys, hits = omap.keys()
    want = occ.insert(planes, 4, m, poses)
    assert np.array_equal(keys, want[0]) and np.array_equal(hits, want[1])
    dk, dh = omap.keys_device()
    assert np.array_equal(dk.cpu().numpy().view(np.uint64), want[0]) and np.array_equal(dh.cpu().numpy().view(np.uint32), want[1])
    omap.close()


def test_fetch_into_too_little_room(pkg, bm):
    planes, m, pose = few_keys()
    omap = pkg.OccupancyMap(bm, 64)
    omap.insert(planes, gpu_model(pkg, m), pose, 8)
    L = pkg.load_library()
    keys = np.zeros(10, np.uint64)
    got = ctypes.c_size_t()
    assert L.sbm_occ_fetch(omap._m, keys.ctypes.data, None, 10, ctypes.byref(got)) == -2
    assert got.value == 30 and not keys.any()
    keys = np.zeros(30, np.uint64)
    assert L.sbm_occ_fetch(omap._m, keys.ctypes.data, None, 30, ctypes.byref(got)) == 0   # counts not wanted
    assert np.array_equal(keys, occ.insert(planes, 8, m, pose)[0])
    omap.close()


def fixture_map(pkg, bm, fx, host, with_norm=True):
    """Every case of the fixture through one map, host or device form."""
    scale = int(fx["scale"])
    omap = pkg.OccupancyMap(bm, 8192, resolution=float(fx["resolution"]), range_max=float(fx["range_max"]))
    up = (lambda a: np.ascontiguousarray(a)) if host else dev
    m, me = gpu_model(pkg, occ.model_from_array(fx["model"])), gpu_model(pkg, occ.model_from_array(fx["model_edge"]))
    omap.insert(up(fx["scene_disp"]), m, fx["scene_poses"], scale)
    omap.insert(up(np.tile(fx["edge_disp"][None], (len(fx["edge_poses"]), 1, 1))), m, fx["edge_poses"], scale)
    if with_norm:
        omap.insert(up(np.tile(fx["edge_disp"][None], (len(fx["norm_poses"]), 1, 1))), me, fx["norm_poses"], scale)
    return omap


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_python_class_writes_the_fixture_stream(pkg, bm, fx, tmp_path, host):
    omap = fixture_map(pkg, bm, fx, host)
    take = (fx["ok"] == 1) & (fx["norm"] <= 25.0)
    want, cnt = np.unique(occ.pack(fx["keys"][take]), return_counts=True)
    keys, hits = omap.keys()
    assert np.array_equal(keys, want) and np.array_equal(hits, cnt)
    omap.write_binary(tmp_path / "slam.bt")
    assert (tmp_path / "slam.bt").read_bytes() == fx["bt_all"].tobytes()
    omap.close()


def test_cpp_call_site_writes_the_same_stream(pkg, bm, fx, tmp_path):
    exe, r = build_callsite(tmp_path, "occupancy_callsite_main.cpp", pkg=pkg)
    assert r.returncode == 0, r.stderr
    # one size per run: the scene's planes, then the edge cases' 1 x 1 planes into a second file
    m = occ.model_from_array(fx["model"])
    (tmp_path / "model.raw").write_bytes(bytes(m))
    for name, planes, poses in (("scene", fx["scene_disp"], fx["scene_poses"]),
                                ("edge", np.tile(fx["edge_disp"][None], (len(fx["edge_poses"]), 1, 1)), fx["edge_poses"])):
        n, h, w = planes.shape
        (tmp_path / "planes.raw").write_bytes(np.ascontiguousarray(planes, np.int16).tobytes())
        (tmp_path / "poses.raw").write_bytes(np.ascontiguousarray(poses, np.float32).tobytes())
        out = tmp_path / f"{name}.bt"
        run = subprocess.run([str(exe), str(tmp_path / "planes.raw"), str(n), str(w), str(h), str(int(fx["scale"])),
                              str(tmp_path / "poses.raw"), str(tmp_path / "model.raw"), "8192", str(out)],
                             capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stdout + run.stderr
        keys = occ.insert(planes, int(fx["scale"]), m, poses)[0]
        assert run.stdout.split() == ["size", str(len(keys)), "overflow", "0"]
        assert out.read_bytes() == occ.write_binary(keys, float(fx["resolution"]))[0]
    # the blocks alone are among the edge cases: the stream octomap wrote for them is the one the library writes
    blocks = np.unique(occ.pack(fx["keys"][(fx["group"] >> 1) & 1 == 1]))
    pkg.occ_write_binary(blocks, tmp_path / "blocks.bt")
    assert (tmp_path / "blocks.bt").read_bytes() == fx["bt_blocks"].tobytes()


def test_profile_records_stages(pkg, bm):
    planes, poses = scene(2, 30, 40, 7)
    omap = pkg.OccupancyMap(bm, 4096)
    bm.set_profiling(1)
    try:
        omap.insert(dev(planes), gpu_model(pkg, occ.model()), poses, 4)
        omap.keys()
        prof = omap.profile()
    finally:
        bm.set_profiling(0)
    assert prof["occ_insert"] > 0 and prof["occ_fetch"] > 0
    omap.close()
