"""The .ot format on the GPU (u96-slam_amd/csrc/sbm_occ_ot.hip: the pre-order ranks and the body kernel of the writer; the device
parse and the expansion of the reader; sbm_occ_ot_host.hip: the host parser) against what the reference's own octomap wrote and read
(tests/golden/occupancy_ot.npz) and against the transcription tests/occupancy_ot_cases.py. Everything is compared for exact
equality: bytes of streams, sorted keys, bits of floats."""
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_load_cases as lc  # noqa: E402
import occupancy_ot_cases as oc  # noqa: E402
import occupancy_ref as occ  # noqa: E402,F401
from gpu_support import bm, build_callsite, dev, torch_cuda  # noqa: E402,F401

pytestmark = pytest.mark.gpu
FX = oc.fixture()
RAYS = dict(np.load(ROOT / "tests" / "golden" / "occupancy_rays.npz"))
NAMES = [str(n) for n in FX["names"]]
HAND = [str(n) for n in FX["hand_built"]]
LOADABLE_HAND = [n for n in HAND if n not in ("childless_root", "eight_leaves")]      # those two hold 2^48 voxels
RESUME = {str(t).split(":")[0]: int(str(t).split(":")[1]) for t in FX["resume"]}
CAPACITY = 1 << 16
LONE = (0, 1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
ENV = "SBM_OCC_OT_HOST_PARSE"


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def same(got, want, what):
    assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]), (what, "keys")
    assert np.array_equal(bits(got[1]), bits(want[1])), (what, "log-odds")


def scans(pkg, name):
    """(origin, points, sbm_occ_ray_params) of every recorded scan of a scene"""
    n = RAYS[f"{name}_npoints"]
    ends = np.cumsum(n)
    p = pkg.occ_ray_params(*[float(v) for v in RAYS[f"{name}_params"]])
    return [(RAYS[f"{name}_origins"][i], RAYS[f"{name}_points"][ends[i] - n[i]:ends[i]], p) for i in range(len(n))]


def nscans(name):
    return len(FX[f"{name}_search_found"])


def recorded_voxels(fmt):
    """octomap's recorded leaves (centre keys, depths, values; fmt names the three members) expanded to depth-16 voxels"""
    return lc.expand_centres(FX[fmt.format("key")], FX[fmt.format("depth")], FX[fmt.format("value")])


def refused(pkg, call, code):
    with pytest.raises(pkg.StereoBMError) as e:
        call()
    assert e.value.code == code, (e.value.code, code)


class host_parse:
    """SBM_OCC_OT_HOST_PARSE for the loads inside: the library reads it at every load"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get(ENV)
        os.environ[ENV] = "1" if self.on else "0"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = self.old


def load_code(pkg, omap, data):
    try:
        omap.load_ot(data)
    except pkg.StereoBMError as e:
        return e.code
    return oc.OK


# ---- 1. write ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_write_after_every_scan_equals_octomap(pkg, bm, torch_cuda, tmp_path, name):
    omap = pkg.OccupancyMap(bm, CAPACITY)
    try:
        for s, (o, pts, p) in enumerate(scans(pkg, name)):
            omap.insert_cloud(dev(pts), o, p)
            want = bytes(FX[f"{name}_ot_{s}"])
            tree = omap.tree(pkg.OCC_TREE_LOGODDS)
            assert tree.ot_body().cpu().numpy().tobytes() == want[want.index(b"data\n") + 5:], (name, s)
            tree.write_ot(tmp_path / "tree.ot")
            assert (tmp_path / "tree.ot").read_bytes() == want, (name, s, "the file, a second call of one build")
            assert tree.ot() == want, (name, s)
            tree.close()
    finally:
        omap.close()


def test_write_refusals_capacity_and_the_empty_map(pkg, bm, torch_cuda, tmp_path):
    import ctypes
    import torch
    o, pts, p = scans(pkg, "short")[0]
    omap, hits = pkg.OccupancyMap(bm, CAPACITY), pkg.OccupancyMap(bm, CAPACITY)
    try:
        empty = omap.tree(pkg.OCC_TREE_LOGODDS)
        assert empty.ot() == oc.stream(0, b"") and len(empty.ot_body()) == 0
        empty.write_ot(tmp_path / "empty.ot")
        assert (tmp_path / "empty.ot").read_bytes() == oc.stream(0, b"")
        empty.close()
        omap.insert_cloud(dev(pts), o, p)
        ml = omap.tree(pkg.OCC_TREE_MAXLIKELIHOOD, p)
        refused(pkg, ml.ot_body, oc.UNSUPPORTED)
        refused(pkg, lambda: ml.write_ot(tmp_path / "ml.ot"), oc.UNSUPPORTED)
        assert not (tmp_path / "ml.ot").exists()
        ml.close()
        hits.insert(dev(RAYS["scene_disp"][:1]), occ_model(pkg), RAYS["scene_poses"][:1], int(RAYS["scene_scale"]))
        refused(pkg, lambda: hits.tree(pkg.OCC_TREE_LOGODDS), oc.UNSUPPORTED)          # no LOGODDS tree of a hit-mode map ...
        ht = hits.tree(pkg.OCC_TREE_MAXLIKELIHOOD, p)
        refused(pkg, ht.ot_body, oc.UNSUPPORTED)                                       # ... and its other tree is not written
        ht.close()
        tree = omap.tree(pkg.OCC_TREE_LOGODDS)
        want = bytes(FX["short_ot_0"])
        n = 5 * tree.info()["nodes"]
        out = torch.full((n,), 0xA5, dtype=torch.uint8, device=torch.device("cuda", bm._device))
        got = ctypes.c_size_t()
        torch.cuda.synchronize()
        assert tree._L.sbm_occ_ot_body_device(tree._t, out.data_ptr(), n - 1, ctypes.byref(got)) == oc.SIZE
        assert got.value == n and bool((out == 0xA5).all())                            # over cap: the length, and nothing written
        assert tree._L.sbm_occ_ot_body_device(tree._t, out.data_ptr() + 1, n, ctypes.byref(got)) == oc.UNSUPPORTED     # misaligned
        assert tree._L.sbm_occ_ot_body_device(tree._t, out.data_ptr(), n, ctypes.byref(got)) == oc.OK
        assert out.cpu().numpy().tobytes() == want[want.index(b"data\n") + 5:]
        tree.close()
    finally:
        omap.close()
        hits.close()


def occ_model(pkg):
    import ctypes
    m = pkg.StereoModel()
    ref = occ.model_from_array(RAYS["scene_model"])
    ctypes.memmove(ctypes.byref(m), ctypes.byref(ref), ctypes.sizeof(m))
    return m


# ---- 2. record layout -------------------------------------------------------------------------------------------------------------
def edge_voxels(k):
    """k lone voxels low in Morton order, then a full depth-13 cube, a full depth-12 cube and one depth-15 group -- and a second
    depth-15 group equal but for one voxel one ulp apart, which must not collapse"""
    codes = np.concatenate([8 * np.arange(k), 100 * 512 + np.arange(512), 20 * 4096 + np.arange(4096), 20000 * 8 + np.arange(8),
                            20001 * 8 + np.arange(8)])
    keys = lc._unmorton_array(codes.astype(np.uint64))
    vals = np.concatenate([np.linspace(-2, 3.4, k).astype(np.float32), np.full(512, 0.75, np.float32), np.full(4096, -1.5, np.float32),
                           np.full(16, 0.4, np.float32)])
    vals[-3] = np.nextafter(np.float32(0.4), np.float32(1))
    return dict(zip(keys.tolist(), vals))


@pytest.mark.parametrize("k", LONE)
def test_record_layout_at_lane_wavefront_and_workgroup_edges(pkg, bm, torch_cuda, k):
    voxels = edge_voxels(k)
    want = oc.write(voxels, 0.1)
    p = oc.parse(want)
    assert p.leaves_at[12] == p.leaves_at[13] == 1 and p.leaves_at[15] == 1 and p.leaves_at[16] == k + 8
    omap = pkg.OccupancyMap(bm, CAPACITY)
    try:
        omap.load_ot(oc.of_records(oc.of_voxels(voxels)))          # every voxel a depth-16 record: the map holds `voxels`
        keys = sorted(voxels)
        same(omap.fetch_logodds(), (np.array(keys, np.uint64), [voxels[x] for x in keys]), k)
        tree = omap.tree(pkg.OCC_TREE_LOGODDS)
        assert tree.info()["nodes"] == p.size
        assert tree.ot() == want, k
        tree.close()
    finally:
        omap.close()


# ---- 3. load ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_fixture_stream_loaded(pkg, bm, torch_cuda, name):
    omap = pkg.OccupancyMap(bm, CAPACITY)
    points = FX["points"]
    try:
        for s in range(nscans(name)):
            data = bytes(FX[f"{name}_ot_{s}"])
            omap.load_ot(data)
            want = recorded_voxels(f"{name}_leaf_{{}}_{s}")
            assert omap.size() == len(want[0]) == pkg.occ_ot_info(data)["voxels"] and omap.overflow() == 0
            same(omap.fetch_logodds(), want, (name, s))
            tree = omap.tree(pkg.OCC_TREE_LOGODDS)
            assert tree.info()["nodes"] == int(FX[f"{name}_size_{s}"]) == int(FX[f"{name}_num_nodes_{s}"])
            assert tree.ot() == data, (name, s, "written back")
            tree.close()
            found = FX[f"{name}_search_found"][s].astype(bool)
            for got in (omap.search(dev(points), 0.0), omap.search(points, 0.0)):
                st, v = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in got)
                assert np.array_equal(st > 0, found), (name, s)
                assert np.array_equal(v.view(np.uint32)[found], FX[f"{name}_search_value"][s][found]), (name, s)
    finally:
        omap.close()


@pytest.mark.parametrize("name", LOADABLE_HAND)
def test_hand_built_streams_loaded(pkg, bm, torch_cuda, name):
    data = bytes(FX[f"hand_{name}"])
    omap = pkg.OccupancyMap(bm, CAPACITY)
    try:
        omap.load_ot(data)
        same(omap.fetch_logodds(), recorded_voxels(f"hand_{name}_leaf_{{}}"), name)          # outside_clamps: stored as they are
        found = FX[f"hand_{name}_search_found"].astype(bool)
        st, v = omap.search(FX["points"], 0.0)
        assert np.array_equal(st > 0, found) and np.array_equal(v.view(np.uint32)[found], FX[f"hand_{name}_search_value"][found])
        tree = omap.tree(pkg.OCC_TREE_LOGODDS)
        back = "inner_right" if name == "inner_wrong" else name                          # the inner values are recomputed
        assert tree.ot() == bytes(FX[f"hand_{back}"])
        tree.close()
    finally:
        omap.close()


# ---- 4. round trip and resume -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RESUME))
def test_resume_through_ot_equals_the_uninterrupted_run(pkg, bm, torch_cuda, tmp_path, name):
    k = RESUME[name]
    all_scans = scans(pkg, name)
    whole, first, second, through_bt = (pkg.OccupancyMap(bm, CAPACITY) for _ in range(4))
    try:
        for s, (o, pts, p) in enumerate(all_scans):
            whole.insert_cloud(dev(pts), o, p)
            if s <= k:
                first.insert_cloud(dev(pts), o, p)
        tree = first.tree(pkg.OCC_TREE_LOGODDS)
        tree.write_ot(tmp_path / "map.ot")
        tree.close()
        assert (tmp_path / "map.ot").read_bytes() == bytes(FX[f"{name}_ot_{k}"])
        second.load_ot(tmp_path / "map.ot")
        same(second.fetch_logodds(), first.fetch_logodds(), (name, "the round trip"))
        ml = first.tree(pkg.OCC_TREE_MAXLIKELIHOOD, all_scans[0][2])
        ml.write_binary(tmp_path / "map.bt")
        ml.close()
        through_bt.load_binary(tmp_path / "map.bt", all_scans[0][2])
        for o, pts, p in all_scans[k + 1:]:
            second.insert_cloud(dev(pts), o, p)
            through_bt.insert_cloud(dev(pts), o, p)
        want = whole.fetch_logodds()
        same(second.fetch_logodds(), want, (name, "resumed"))
        same(second.fetch_logodds(), recorded_voxels(f"{name}_resume_{{}}"), (name, "octomap's resumed tree"))
        lossy = through_bt.fetch_logodds()
        assert np.array_equal(lossy[0], want[0]) and int((bits(lossy[1]) != bits(want[1])).sum()) > 0      # what a .bt loses
    finally:
        for m in (whole, first, second, through_bt):
            m.close()


# ---- 5. device parse against host parse -------------------------------------------------------------------------------------------
def parse_streams():
    out = {f"{n}_{s}": bytes(FX[f"{n}_ot_{s}"]) for n in NAMES for s in range(nscans(n))}
    out.update({f"hand_{n}": bytes(FX[f"hand_{n}"]) for n in HAND})
    teeth = 64
    while oc.count(oc.comb(teeth)) <= 2 * oc.FAN ** 3 + 16:     # the last child of the root: more than 2 * FAN^3 records back
        teeth *= 2
    out["comb"] = oc.of_records(oc.comb(teeth))
    for n in sorted({1, oc.FAN - 1, oc.FAN, oc.FAN + 1, 2 * oc.FAN + 1, oc.FAN ** 2 - 1, oc.FAN ** 2, oc.FAN ** 2 + 1, 2 * oc.FAN ** 2 + 1,
                     oc.SCAN_TILE - 1, oc.SCAN_TILE, oc.SCAN_TILE + 1, 2 * oc.SCAN_TILE + 1}):
        tree = oc.sized(n) if n >= 17 or n == 1 else oc.chain([3] * (n - 1), 0.25, 0.25)      # below 17: a chain that ends above depth 16
        assert oc.count(tree) == n
        out[f"sized_{n}"] = oc.of_records(tree)
    return out


def wide_stream():
    """More than 256 scan tiles of records, so that every thread of the one-workgroup scan of the tile sums takes a run of tiles:
    30 000 voxels scattered over the whole key space, unpruned, each at the end of a chain of its own from about depth 5 down
    -> ((packed keys ascending, values), stream)"""
    rng = np.random.default_rng(24)
    codes = np.unique(rng.integers(0, 1 << 48, 30000, dtype=np.uint64))
    values = rng.normal(size=len(codes)).astype(np.float32)
    keys = lc._unmorton_array(codes)
    order = np.argsort(keys)
    return (keys[order], values[order]), oc.unpruned(codes, values)


PARSE = parse_streams()


def test_the_deep_tree_crosses_every_level_of_the_search():
    p = oc.parse(PARSE["comb"])
    lens = oc.search_levels(p.size)
    assert p.status == oc.OK and p.voxels < 1 << 16 and len(lens) == 5 and p.size > 2 * oc.FAN ** 3 + 16
    body = PARSE["comb"][PARSE["comb"].index(b"data\n") + 5:]
    assert bin(body[4]).count("1") == 2                        # the root's last child is 16 records from the end: its parent search
    assert max(d for _, d, _ in p.leaves) == 16                 # starts in the last tile of every level and ends at record 0


@pytest.mark.parametrize("name", sorted(PARSE))
def test_device_parse_against_host_parse(pkg, bm, torch_cuda, name):
    data = PARSE[name]
    want = oc.parse(data, 0.1)
    code = want.status if want.status != oc.OK or want.voxels <= CAPACITY else oc.OCC_FULL
    omap = pkg.OccupancyMap(bm, CAPACITY)
    try:
        got = []
        for on in (True, False):
            omap.reset()
            with host_parse(on):
                assert load_code(pkg, omap, data) == code, (name, on)
            got.append(omap.fetch_logodds() if code == oc.OK else None)
        if code == oc.OK:
            same(got[0], oc.expand(want), (name, "host parse"))
            same(got[1], got[0], (name, "device parse"))
    finally:
        omap.close()


def test_device_parse_where_the_tile_sums_take_a_run_per_thread(pkg, bm, torch_cuda):
    want, data = wide_stream()
    info = pkg.occ_ot_info(data)
    assert info["nodes"] > 256 * oc.SCAN_TILE and info["voxels"] == info["leaves"] == len(want[0]) < CAPACITY
    omap = pkg.OccupancyMap(bm, CAPACITY)
    try:
        for on in (True, False):
            omap.reset()
            with host_parse(on):
                omap.load_ot(data)
            same(omap.fetch_logodds(), want, ("host parse" if on else "device parse"))
            assert omap.overflow() == 0
    finally:
        omap.close()


@pytest.mark.parametrize("on", [True, False], ids=["host_parse", "device_parse"])
def test_staging_of_a_larger_load_is_not_read(pkg, bm, torch_cuda, on):
    """Large, small, large through one handle: the arrays of a load are placed anew in staging that only grows."""
    large = edge_voxels(257)
    streams = [large, dict(list(large.items())[:1]), dict(list(large.items())[:17]), large]
    omap = pkg.OccupancyMap(bm, CAPACITY)
    try:
        for voxels in streams:
            with host_parse(on):
                omap.load_ot(oc.of_records(oc.of_voxels(voxels)))
            keys = sorted(voxels)
            same(omap.fetch_logodds(), (np.array(keys, np.uint64), [voxels[x] for x in keys]), len(voxels))
            assert omap.overflow() == 0
    finally:
        omap.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_map_untouched_on_both_parse_paths(pkg, bm, torch_cuda, tmp_path):
    good = bytes(FX["scene_ot_0"])
    voxels = pkg.occ_ot_info(good)["voxels"]
    o, pts, p = scans(pkg, "short")[0]
    exact, small, other = pkg.OccupancyMap(bm, voxels), pkg.OccupancyMap(bm, voxels - 1), pkg.OccupancyMap(bm, CAPACITY, resolution=0.05)
    big = pkg.OccupancyMap(bm, CAPACITY)
    try:
        small.insert_cloud(dev(pts), o, p)
        before = small.fetch_logodds()
        for on in (True, False):
            with host_parse(on):
                exact.load_ot(good)
                assert exact.size() == voxels and exact.overflow() == 0                          # capacity equal to the voxel count
                refused(pkg, lambda: small.load_ot(good), oc.OCC_FULL)                           # one below it
                refused(pkg, lambda: small.load_ot(bytes(FX["hand_childless_root"])), oc.OCC_FULL)     # 2^48 voxels
                refused(pkg, lambda: small.load_ot(bytes(FX["hand_eight_leaves"])), oc.OCC_FULL)
                for name, (bad, code) in oc.malformed(good).items():
                    assert bytes(FX[f"bad_{name}"]) == bad
                    refused(pkg, lambda: small.load_ot(bad), code)
                refused(pkg, lambda: small.load_ot(tmp_path / "no-such-file.ot"), oc.UNSUPPORTED)
                refused(pkg, lambda: other.load_ot(good), oc.SIZE)                               # res 0.1 into a 0.05 map
                refused(pkg, lambda: small.load_binary(good, p), oc.UNSUPPORTED)                 # the .bt loader does not sniff
                same(small.fetch_logodds(), before, ("after the refused loads", on))
        small.insert_cloud(dev(pts), o, p)                                                       # and it is still a log-odds map
        small.load_ot(oc.stream(0, b""))                                                         # size 0: empty, no mode
        assert small.size() == 0
        big.insert(dev(RAYS["scene_disp"][:1]), occ_model(pkg), RAYS["scene_poses"][:1], int(RAYS["scene_scale"]))        # hit mode ...
        big.load_ot(bytes(FX["short_ot_0"]))                                                     # ... is replaced by a load
        same(big.fetch_logodds(), recorded_voxels("short_leaf_{}_0"), "over a hit-mode map")
    finally:
        for m in (exact, small, other, big):
            m.close()


# ---- 7. modes ---------------------------------------------------------------------------------------------------------------------
def test_async_profile_and_path_form(pkg, torch_cuda, tmp_path):
    data = bytes(FX["random_ot_0"])
    eng = pkg.StereoBM.create(64, 21)
    omap = pkg.OccupancyMap(eng, CAPACITY)
    try:
        omap.load_ot(data, sync=False)
        assert omap.size() == pkg.occ_ot_info(data)["voxels"]                  # a synchronous call follows the load in stream order
        want = omap.fetch_logodds()
        same(want, recorded_voxels("random_leaf_{}_0"), "sync=False")
        (tmp_path / "random.ot").write_bytes(data)
        omap.load_ot(str(tmp_path / "random.ot"))
        same(omap.fetch_logodds(), want, "the path form")
        omap.load_ot(np.frombuffer(data, np.uint8))
        same(omap.fetch_logodds(), want, "an array of bytes")
        eng.set_profiling(True)
        for on in (True, False):
            with host_parse(on):
                omap.load_ot(data)
            prof = omap.profile()
            assert prof["occ_load"] > 0 and prof["occ_rays_mark"] == 0 and prof["occ_fetch"] == 0, on
        omap.fetch_logodds()
        assert omap.profile()["occ_load"] == prof["occ_load"]                  # a fetch keeps the load's time
        for on in (True, False):
            with host_parse(on):
                refused(pkg, lambda: omap.load_ot(bytes(FX["bad_depth17"])), oc.SIZE)
                refused(pkg, lambda: omap.load_ot(bytes(FX["bad_color_id"])), oc.UNSUPPORTED)
            assert omap.profile()["occ_load"] == prof["occ_load"]              # and so does a refused load
        tree = omap.tree(pkg.OCC_TREE_LOGODDS)
        assert tree.ot() == data and tree.profile()["occ_tree_query"] > 0
        tree.close()
    finally:
        eng.set_profiling(False)
        omap.close()
        eng.close()


def test_cpp_call_site(pkg, torch_cuda, tmp_path):
    name, k = "scene", RESUME["scene"]
    assert [float(v) for v in RAYS["scene_params"][:5]] == [0.7, 0.4, 0.1192, 0.971, 0.5]      # the adaptor's defaults
    exe, built = build_callsite(tmp_path, "occupancy_ot_callsite_main.cpp")
    assert built.returncode == 0, built.stderr
    flat = np.concatenate([np.concatenate([np.float32([len(pts)]), o, pts.reshape(-1)]) for o, pts, _ in scans(pkg, name)]).astype(np.float32)
    flat.tofile(tmp_path / "scans.raw")
    after = lc.expand_centres(FX["scene_resume_key"], FX["scene_resume_depth"], FX["scene_resume_value"])
    r = subprocess.run([str(exe), str(tmp_path / "scans.raw"), str(len(flat)), str(k + 1), str(CAPACITY), repr(float(RAYS["scene_params"][5])),
                        str(tmp_path / "map.ot"), str(tmp_path / "out.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "map.ot").read_bytes() == bytes(FX[f"scene_ot_{k}"])
    written = pkg.occ_ot_info(bytes(FX[f"scene_ot_{k}"]))["voxels"]
    assert r.stdout.split() == ["written", str(written), "after", str(len(after[0])), "overflow", "0"], r.stdout
    tail = np.frombuffer((tmp_path / "out.raw").read_bytes(), np.dtype([("key", "<u8"), ("value", "<u4")]))
    assert np.array_equal(tail["key"], after[0]) and np.array_equal(tail["value"], bits(after[1]))
    r = subprocess.run([str(exe), str(tmp_path / "scans.raw"), str(len(flat)), "0", "16", "-1", str(tmp_path / "no-such-dir" / "x.ot"),
                        str(tmp_path / "out.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 4 and r.stdout.split() == ["error", str(oc.UNSUPPORTED)], r.stdout + r.stderr
