"""The occupancy map's read side for planners on the GPU (u96-slam_amd/csrc/sbm_occ_planner.hip: occ_plan_*_kernel) against what
the reference's own octomap answered (tests/golden/occupancy_planner.npz): the box leaf iterator by keys and by points, the
unknown cells of a box, the metric bounds and the ray entries, device and host forms, all compared for exact equality: integers,
orders and float bits. Every map is built through the existing inserts and is the same before and after all calls."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_planner_cases as pc  # noqa: E402
import occupancy_ref as occ  # noqa: E402
import occupancy_tree_cases as tc  # noqa: E402
from gpu_support import bm, build_callsite, dev, torch_cuda  # noqa: E402,F401
from test_occupancy_planner_restatement import FX, FXQ, FXT, RES, TREES, bits, recorded_boxes, recorded_unknown, tree_of  # noqa: E402

pytestmark = pytest.mark.gpu
FAR = FX["far_origin"]
NULL, SIZE, UNSUPPORTED = -1, -2, -23
LO, ML = 0, 1
ALL = ((0, 0, 0), (65535, 65535, 65535))


def host(a):
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a)


def unpack(keys):
    return occ.unpack(np.asarray(keys, np.uint64)).astype(np.int64)


def centres(keys3):
    return ((np.asarray(keys3, np.float64) - 32768 + 0.5) * RES).astype(np.float32)


def gpu_model(pkg, m):
    g = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(g), ctypes.byref(m), ctypes.sizeof(g))
    return g


def scans_of(name):
    if name == "empty":
        return []
    if f"{name}_npoints" in FXQ:
        n = FXQ[f"{name}_npoints"]
        ends = np.cumsum(n)
        return [(FXQ[f"{name}_origins"][i], float(FXQ[f"{name}_scan_range"][i]), FXQ[f"{name}_points"][e - k:e]) for i, (k, e) in enumerate(zip(n, ends))]
    if f"{name}_scan_keys" in FXT:
        ends = np.cumsum(FXT[f"{name}_scan_n"])
        return [(FAR, -1.0, centres(FXT[f"{name}_scan_keys"][e - k:e])) for k, e in zip(FXT[f"{name}_scan_n"], ends)]
    return [(FAR, -1.0, centres(unpack(FXT[f"{name}_keys"])))]


def lay(pkg, bm, name, capacity=1 << 14):
    """The tree's map through the existing inserts and its tree under the fixture's reading -> (map, tree, stored (keys, values))"""
    omap = pkg.OccupancyMap(bm, capacity)
    if name != "empty" and int(FX[f"{name}_hits"]):
        omap.insert(dev(FXQ["scene_disp"]), gpu_model(pkg, occ.model_from_array(FXQ["scene_model"])), FXQ["scene_poses"], int(FXQ["scene_scale"]))
        stored = omap.keys()
        assert np.array_equal(stored[0], FXQ["scene_hits_keys"])
        return omap, omap.tree(ML, pkg.occ_ray_params()), stored
    params = [float(v) for v in FXT[f"{name}_params"]] if name != "empty" else []
    for o, max_range, p in scans_of(name):
        omap.insert_cloud(dev(p), o, pkg.occ_ray_params(*params, max_range=max_range))
    stored = omap.fetch_logodds() if name != "empty" else omap.keys()
    if name != "empty":
        src = FXT if f"{name}_keys" in FXT else FXQ
        assert np.array_equal(stored[0], src[f"{name}_keys"]) and np.array_equal(bits(stored[1]), bits(src[f"{name}_logodds"]))
    return omap, omap.tree(LO), stored


def unchanged(omap, name, stored):
    now = omap.keys() if name == "empty" or int(FX[f"{name}_hits"]) else omap.fetch_logodds()
    return omap.size() == len(stored[0]) and np.array_equal(now[0], stored[0]) and np.array_equal(host(now[1]).view(np.uint32), host(stored[1]).view(np.uint32))


def same_leaves(got, want, what):
    k, d, v = (host(a) for a in got)
    want = [host(a) for a in want]
    assert len(k) == len(want[0]), (what, len(k), len(want[0]))
    assert np.array_equal(k.view(np.uint64), np.asarray(want[0], np.uint64)) and np.array_equal(d, np.asarray(want[1], np.int32)), what
    assert np.array_equal(bits(v), bits(want[2])), (what, "values")


@pytest.mark.parametrize("name", TREES)
def test_every_fixture_tree_all_four_calls(pkg, bm, name):
    omap, t, stored = lay(pkg, bm, name)
    try:
        m = FX[f"{name}_metric"]
        for _ in range(2):                                       # the second answer comes from the tree
            lo, hi = t.metric_min_max()
            assert np.array_equal(lo.view(np.uint64), m[12:15].view(np.uint64)) and np.array_equal(hi.view(np.uint64), m[15:18].view(np.uint64))
        want_lo, want_hi = pc.metric(tree_of(name))
        assert np.float64(t.volume()).view(np.uint64) == np.float64(pc.volume(want_lo, want_hi)).view(np.uint64)
        assert np.array_equal(t.metric_size(), np.array(pc.metric_size(want_lo, want_hi)))
        none = (np.zeros(0, np.uint64), np.zeros(0, np.int32), np.zeros(0, np.float32))
        for points, lo, hi, depth, want in recorded_boxes(name):
            if points:
                lo, hi = np.float32(lo), np.float32(hi)
                if not pc.corners_have_keys(tree_of(name), lo, hi):
                    want = none                                  # the stated divergence: octomap's loop visits the root once
            same_leaves(t.leaves_bbx(lo, hi, depth), want, (name, lo, hi, depth, "host"))
            same_leaves(t.leaves_bbx_device(lo, hi, depth), want, (name, lo, hi, depth, "device"))
            if not points and (lo, hi) == ALL:
                same_leaves(t.leaves_bbx_device(lo, hi, depth), t.leaves_device(depth), (name, depth, "the box over everything"))
        for lo, hi, depth, steps, xyz in recorded_unknown(name):
            for got in (t.unknown_centers(lo, hi, depth), t.unknown_centers_device(lo, hi, depth)):
                assert np.array_equal(bits(host(got)).reshape(-1, 3), bits(xyz).reshape(-1, 3)), (name, lo, hi, depth, steps)
        assert unchanged(omap, name, stored)
    finally:
        t.close()
        omap.close()


def test_a_capacity_one_below_the_count_writes_nothing(pkg, bm, torch_cuda):
    torch = torch_cuda
    L = pkg.load_library()
    omap, t, _ = lay(pkg, bm, "cube63")
    try:
        lo, hi = np.array(ALL[0], np.uint16), np.array(ALL[1], np.uint16)
        want = t.leaves_device(0)
        n = len(want[0])
        assert n > 8
        k = torch.full((n + 8,), -7, dtype=torch.int64, device="cuda:0")
        d = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda:0")
        v = torch.full((n + 8,), -7, dtype=torch.int32, device="cuda:0")
        got = ctypes.c_size_t()
        args = (t._t, lo.ctypes.data, hi.ctypes.data, 0, k.data_ptr(), d.data_ptr(), v.data_ptr())
        assert L.sbm_occ_bbx_leaves_device(*args, n - 1, ctypes.byref(got)) == SIZE and got.value == n
        assert bool((k == -7).all()) and bool((d == -7).all()) and bool((v == -7).all())
        assert L.sbm_occ_bbx_leaves_device(*args, n, ctypes.byref(got)) == 0 and got.value == n
        assert np.array_equal(host(k[:n]), host(want[0])) and bool((k[n:] == -7).all()) and bool((d[n:] == -7).all()) and bool((v[n:] == -7).all())
        hk, hd = np.full(n, 5, np.uint64), np.full(n, 5, np.int32)
        assert L.sbm_occ_bbx_leaves(t._t, lo.ctypes.data, hi.ctypes.data, 0, hk.ctypes.data, hd.ctypes.data, None, n - 1, ctypes.byref(got)) == SIZE
        assert got.value == n and (hk == 5).all() and (hd == 5).all()
        box = [r for r in recorded_unknown("cube63") if r[3] == (12, 12, 12)][0]
        plo, phi = np.float32(box[0]), np.float32(box[1])
        m = len(box[4])
        assert m > 8
        x = torch.full((m + 8, 3), -7.0, dtype=torch.float32, device="cuda:0")
        args = (t._t, plo.ctypes.data, phi.ctypes.data, 16, x.data_ptr())
        assert L.sbm_occ_unknown_device(*args, m - 1, ctypes.byref(got)) == SIZE and got.value == m and bool((x == -7).all())
        assert L.sbm_occ_unknown_device(*args, m, ctypes.byref(got)) == 0 and got.value == m
        assert np.array_equal(bits(host(x[:m])), bits(box[4])) and bool((x[m:] == -7).all())
        hx = np.full((m, 3), 5, np.float32)
        assert L.sbm_occ_unknown(t._t, plo.ctypes.data, phi.ctypes.data, 16, hx.ctypes.data, m - 1, ctypes.byref(got)) == SIZE and (hx == 5).all()
    finally:
        t.close()
        omap.close()


def ray_groups():
    rows = FX["ray_cases"]
    return [(delta, np.flatnonzero(rows[:, 9] == delta)) for delta in sorted(set(rows[:, 9].tolist()))]


def test_every_recorded_ray_entry_device_and_host(pkg, bm):
    omap = pkg.OccupancyMap(bm, 1 << 10)
    try:
        rows = FX["ray_cases"][:, :9].astype(np.float32)
        for delta, at in ray_groups():
            o, d, c = (np.ascontiguousarray(rows[at, i:i + 3]) for i in (0, 3, 6))
            want_f, want_p = FX["ray_found"][at], FX["ray_xyz"][at]
            for found, xyz in (omap.ray_intersections(dev(o), dev(d), dev(c), delta), omap.ray_intersections(o, d, c, delta)):
                assert np.array_equal(host(found), want_f.astype(np.int32)), delta
                assert np.array_equal(bits(host(xyz)), bits(want_p)), delta
            for i in range(0, len(at), 37):                      # one origin for every ray: three host floats
                for found, xyz in (omap.ray_intersections(o[i], dev(d[i:i + 1]), dev(c[i:i + 1]), delta),
                                   omap.ray_intersections(o[i], d[i:i + 1], c[i:i + 1], delta)):
                    assert int(host(found)[0]) == int(want_f[i]) and np.array_equal(bits(host(xyz))[0], bits(want_p)[i])
        assert omap.size() == 0
    finally:
        omap.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wavefront_and_workgroup_edges_of_the_ray_entries(pkg, bm, torch_cuda, n):
    torch = torch_cuda
    L = pkg.load_library()
    omap = pkg.OccupancyMap(bm, 1 << 10)
    try:
        at = np.resize(np.flatnonzero(FX["ray_cases"][:, 9] == 0.0), n)
        rows = FX["ray_cases"][at, :9].astype(np.float32)
        o, d, c = (dev(np.ascontiguousarray(rows[:, i:i + 3])) for i in (0, 3, 6))
        xyz = torch.full((n + 64, 3), -7.0, dtype=torch.float32, device="cuda:0")
        found = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda:0")
        for sync in (0, 0, 1):                                   # sync = 0 calls, then a synchronous one
            assert L.sbm_occ_ray_intersections_device(omap._m, n, o.data_ptr(), 0, d.data_ptr(), c.data_ptr(), 0.0, xyz.data_ptr(), found.data_ptr(), sync) == 0
        assert np.array_equal(host(found[:n]), FX["ray_found"][at].astype(np.int32)) and np.array_equal(bits(host(xyz[:n])), bits(FX["ray_xyz"][at]))
        assert bool((xyz[n:] == -7).all()) and bool((found[n:] == -7).all())       # nothing beyond n is written
        assert L.sbm_occ_ray_intersections_device(omap._m, n, o.data_ptr(), 0, d.data_ptr(), c.data_ptr(), 0.0, xyz.data_ptr(), None, 1) == 0
    finally:
        omap.close()


def test_a_rebuilt_tree_answers_the_new_map_and_drops_the_cached_bounds(pkg, bm):
    omap, t, _ = lay(pkg, bm, "sib8")
    try:
        before = t.metric_min_max()
        lo, hi = np.array(ALL[0]), np.array(ALL[1])
        assert len(t.leaves_bbx(lo, hi)[0]) == 1
        far = np.array([[40000, 100, 65000]])
        omap.insert_cloud(centres(far), FAR)
        assert all(np.array_equal(a, b) for a, b in zip(t.metric_min_max(), before)) and len(t.leaves_bbx(lo, hi)[0]) == 1     # a snapshot
        t.build(LO)
        keys, lo_values = omap.fetch_logodds()
        want = tc.Tree(dict(zip((int(k) for k in keys), lo_values)), RES)
        got = t.metric_min_max()
        wl, wh = pc.metric(want)
        assert np.array_equal(got[0], np.array(wl)) and np.array_equal(got[1], np.array(wh)) and not np.array_equal(got[1], before[1])
        same_leaves(t.leaves_bbx(lo, hi), want.leaves(0), "rebuilt")
        same_leaves(t.leaves_bbx_device(far[0], far[0]), pc.leaves_bbx(want, tuple(far[0]), tuple(far[0])), "the new voxel")
        p = centres(far)[0]
        st, xyz, _ = pc.unknown_centers(want, p - np.float32(0.35), p + np.float32(0.3), 16)
        assert st == 0 and np.array_equal(bits(t.unknown_centers(p - np.float32(0.35), p + np.float32(0.3), 16)), bits(xyz)) and len(xyz) > 20
    finally:
        t.close()
        omap.close()


def test_a_tree_never_built_answers_as_an_empty_one(pkg, bm):
    omap = pkg.OccupancyMap(bm, 1 << 10)
    t = pkg.OccupancyTree(omap)
    try:
        assert not np.any(t.metric_min_max()) and t.volume() == 0.0
        assert len(t.leaves_bbx(ALL[0], ALL[1])[0]) == 0 and len(t.leaves_bbx_device(np.float32([0, 0, 0]), np.float32([1, 1, 1]))[0]) == 0
        box = recorded_unknown("empty")[2]
        assert np.array_equal(bits(t.unknown_centers_device(box[0], box[1], box[2]).cpu().numpy()), bits(box[4]))
    finally:
        t.close()
        omap.close()


def test_argument_checks_in_their_documented_order(pkg, bm, torch_cuda):
    torch = torch_cuda
    L = pkg.load_library()
    omap, t, _ = lay(pkg, bm, "sib8")
    try:
        n = ctypes.c_size_t(7)
        N = ctypes.byref(n)
        k = torch.zeros((64,), dtype=torch.int64, device="cuda:0")
        s = torch.zeros((64,), dtype=torch.int32, device="cuda:0")
        x = torch.zeros((64, 3), dtype=torch.float32, device="cuda:0")
        K, S, X = k.data_ptr(), s.data_ptr(), x.data_ptr()
        lo, hi = np.array(ALL[0], np.uint16), np.array(ALL[1], np.uint16)
        A, B = lo.ctypes.data, hi.ctypes.data
        # the box iterator: null, then the depth, then the alignment
        assert L.sbm_occ_bbx_leaves_device(t._t, None, B, 17, K + 4, S, None, 8, N) == NULL
        assert L.sbm_occ_bbx_leaves_device(t._t, A, B, 17, None, S, None, 8, N) == NULL
        assert L.sbm_occ_bbx_leaves_device(t._t, A, B, 17, K + 4, S, None, 8, None) == NULL
        assert L.sbm_occ_bbx_leaves_device(t._t, A, B, 17, K + 4, S, None, 8, N) == SIZE
        assert L.sbm_occ_bbx_leaves_device(t._t, A, B, -1, K, S, None, 8, N) == SIZE
        for ptrs in ((K + 4, S, None), (K, S + 2, None), (K, S, S + 1)):
            assert L.sbm_occ_bbx_leaves_device(t._t, A, B, 0, ptrs[0], ptrs[1], ptrs[2], 8, N) == UNSUPPORTED
        assert n.value == 7
        assert L.sbm_occ_bbx_leaves_device(t._t, A, B, 16, None, None, None, 0, N) == SIZE and n.value == 1       # the count
        out = np.float32([3276.85, 0, 0])
        p0, p1 = np.float32([0, 0, 0]), np.float32([1, 1, 1])
        assert L.sbm_occ_bbx_leaves_points_device(t._t, out.ctypes.data, p1.ctypes.data, 17, K, S, None, 8, N) == SIZE
        assert L.sbm_occ_bbx_leaves_points_device(t._t, out.ctypes.data, p1.ctypes.data, 0, K, S, None, 8, N) == 0 and n.value == 0
        # the unknown cells: null, the depth, a corner outside the key space, the alignment, the cell count
        n.value = 7
        P0, P1, OUT = p0.ctypes.data, p1.ctypes.data, out.ctypes.data
        big0, big1 = np.float32([-60, -60, -60]), np.float32([60, 60, 60])
        assert L.sbm_occ_unknown_device(t._t, None, P1, 17, X + 2, 8, N) == NULL
        assert L.sbm_occ_unknown_device(t._t, P0, P1, 17, None, 8, N) == NULL
        assert L.sbm_occ_unknown_device(t._t, OUT, P1, 17, X + 2, 8, N) == SIZE
        assert L.sbm_occ_unknown_device(t._t, OUT, big1.ctypes.data, 16, X + 2, 8, N) == SIZE
        assert L.sbm_occ_unknown_device(t._t, P0, np.float32([0, float("nan"), 0]).ctypes.data, 0, X, 8, N) == SIZE
        assert L.sbm_occ_unknown_device(t._t, big0.ctypes.data, big1.ctypes.data, 16, X + 2, 8, N) == UNSUPPORTED
        assert L.sbm_occ_unknown_device(t._t, P0, P1, 16, X + 2, 8, N) == UNSUPPORTED
        assert L.sbm_occ_unknown_device(t._t, big0.ctypes.data, big1.ctypes.data, 16, X, 8, N) == UNSUPPORTED
        assert L.sbm_occ_unknown(t._t, big0.ctypes.data, big1.ctypes.data, 16, None, 0, N) == UNSUPPORTED
        assert n.value == 7
        assert L.sbm_occ_unknown_device(t._t, P1, P0, 16, X, 8, N) == 0 and n.value == 0                       # pmax below pmin: no steps
        # the metric bounds
        m = np.zeros(6, np.float64)
        assert L.sbm_occ_metric(t._t, None, m.ctypes.data) == NULL and L.sbm_occ_metric(t._t, m.ctypes.data, None) == NULL and not m.any()
        # the ray entries: null, then the delta, then the count and the alignment
        nan = float("nan")
        assert L.sbm_occ_ray_intersections_device(omap._m, 8, None, 0, X, X, nan, X, None, 1) == NULL
        assert L.sbm_occ_ray_intersections_device(omap._m, 8, X, 0, X, None, nan, X, None, 1) == NULL
        assert L.sbm_occ_ray_intersections_device(omap._m, 8, X, 0, X, X, nan, None, None, 1) == NULL
        assert L.sbm_occ_ray_intersections_device(omap._m, (1 << 30) + 1, X + 2, 0, X, X, nan, X, None, 1) == SIZE
        assert L.sbm_occ_ray_intersections_device(omap._m, (1 << 30) + 1, X, 0, X, X, 0.0, X, None, 1) == UNSUPPORTED
        for ptrs in ((X + 2, X, X, X, S), (X, X + 1, X, X, S), (X, X, X + 2, X, S), (X, X, X, X + 3, S), (X, X, X, X, S + 1)):
            assert L.sbm_occ_ray_intersections_device(omap._m, 8, ptrs[0], 0, ptrs[1], ptrs[2], 0.0, ptrs[3], ptrs[4], 1) == UNSUPPORTED
        assert L.sbm_occ_ray_intersections_device(omap._m, 0, None, 0, None, None, 0.0, None, None, 1) == 0
        assert L.sbm_occ_ray_intersections(omap._m, 8, None, 1, None, None, 0.0, None, None) == NULL
        assert not bool(k.any()) and not bool(s.any()) and not bool(x.any())                                   # no refused call wrote anything
    finally:
        t.close()
        omap.close()


def test_the_calls_add_to_the_existing_profile_names(pkg):
    eng = pkg.StereoBM.create(64, 21)
    omap = pkg.OccupancyMap(eng, 1 << 12)
    t = None
    try:
        eng.set_profiling(True)
        omap.insert_cloud(dev(centres(unpack(FXT["cube63_keys"]))), FAR)
        t = omap.tree(LO)
        assert t.profile()["occ_tree_query"] == 0
        t.leaves_bbx(ALL[0], ALL[1])
        assert t.profile()["occ_tree_query"] > 0
        for call in (t.metric_min_max, lambda: t.unknown_centers(np.float32([23, -27, 13]), np.float32([23.5, -26.5, 13.5]))):
            call()
            assert t.profile()["occ_tree_query"] > 0
        o = np.float32([0, 0, 0])
        omap.ray_intersections(o, np.float32([[1, 0, 0]]), np.float32([[1.05, 0.05, 0.05]]))
        assert omap.profile()["occ_cast"] > 0
    finally:
        eng.set_profiling(False)
        if t is not None:
            t.close()
        omap.close()
        eng.close()


def test_cpp_call_site_reads_the_map_as_octomap(pkg, bm, tmp_path):
    exe, built = build_callsite(tmp_path, "occupancy_planner_callsite_main.cpp")
    assert built.returncode == 0, built.stderr
    cloud = np.concatenate([np.concatenate([np.float32([len(p)]), o, p.reshape(-1)]) for o, _, p in scans_of("cube63")]).astype(np.float32)
    cloud.tofile(tmp_path / "cloud.raw")
    box = [r for r in recorded_unknown("cube63") if r[3] == (12, 12, 12)][0]
    np.concatenate([box[0], box[1]]).astype(np.float32).tofile(tmp_path / "box.raw")
    i = int(np.flatnonzero((FX["ray_cases"][:, 9] == 1e-3) & (FX["ray_found"] == 1))[0])
    FX["ray_cases"][i, :9].astype(np.float32).tofile(tmp_path / "ray.raw")
    r = subprocess.run([str(exe), str(tmp_path / "cloud.raw"), str(len(cloud)), "-1", str(1 << 12), "0", str(tmp_path / "box.raw"), "16",
                        str(tmp_path / "ray.raw"), "1e-3", str(tmp_path / "out.raw")], capture_output=True, text=True, timeout=120)
    t = tree_of("cube63")
    kmin, kmax = (tuple(int(np.floor(10.0 * float(c))) + 32768 for c in p) for p in (box[0], box[1]))
    want = pc.leaves_bbx(t, kmin, kmax, 0)
    assert r.returncode == 0 and r.stdout.split() == ["keys", str(len(want[0])), "points", str(len(want[0])), "unknown", str(len(box[4])),
                                                       "found", "1"], r.stdout + r.stderr
    raw = (tmp_path / "out.raw").read_bytes()
    n = len(want[0])
    leaf = np.dtype([("key", "<u8"), ("depth", "<i4"), ("value", "<u4")])
    for part in (np.frombuffer(raw, leaf, n), np.frombuffer(raw, leaf, n, 16 * n)):
        assert np.array_equal(part["key"], want[0]) and np.array_equal(part["depth"], want[1]) and np.array_equal(part["value"], bits(want[2]))
    off = 32 * n
    assert np.array_equal(np.frombuffer(raw, "<u4", 3 * len(box[4]), off), bits(box[4]).reshape(-1))
    off += 12 * len(box[4])
    lo, hi = pc.metric(t)
    size = pc.metric_size(lo, hi)
    assert np.array_equal(np.frombuffer(raw, "<f8", 10, off), np.array(lo + hi + size + [size[0] * size[1] * size[2]]))
    off += 80
    assert np.frombuffer(raw, "<i4", 1, off)[0] == 1 and np.array_equal(np.frombuffer(raw, "<u4", 3, off + 4), bits(FX["ray_xyz"][i]))
    flags, many = np.frombuffer(raw, "<i4", 2, off + 16), np.frombuffer(raw, "<f4", 6, off + 24)
    assert flags.tolist() == [1, 0] and np.array_equal(bits(many[:3]), bits(FX["ray_xyz"][i])) and np.isnan(many[3:]).all()
