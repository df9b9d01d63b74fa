"""The GPU occupancy map's log-odds mode (u96-slam_amd/csrc/sbm_occ_rays.hip: occ_rays_*_kernel) against what the reference's own
octomap answered for insertPointCloud (tests/golden/occupancy_rays.npz) and, for shapes the fixture does not hold, against the
restatement tests/occupancy_ray_cases.py, which tests/test_occupancy_rays_restatement.py pins to the same fixture. Everything is
compared for exact equality: sorted keys and the bits of the float log-odds."""
import ctypes
import functools
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_ray_cases as rc  # noqa: E402
import occupancy_ref as occ  # noqa: E402
from gpu_support import bm, build_callsite, dev, torch_cuda  # noqa: E402,F401

pytestmark = pytest.mark.gpu
FX = dict(np.load(ROOT / "tests" / "golden" / "occupancy_rays.npz"))
NAMES = [str(n) for n in FX["names"]]
UNSUPPORTED, SIZE = -23, -2


def params_of(pkg, name):
    return pkg.occ_ray_params(*[float(v) for v in FX[f"{name}_params"]])


def scans_of(name):
    n = FX[f"{name}_npoints"]
    ends = np.cumsum(n)
    return [(FX[f"{name}_origins"][i], FX[f"{name}_points"][e - k:e]) for i, (k, e) in enumerate(zip(n, ends))]


def recorded(name):
    n = FX[f"{name}_nleaves"].astype(np.int64)
    ends = np.cumsum(n)
    return [(FX[f"{name}_keys"][e - k:e], FX[f"{name}_logodds"][e - k:e]) for k, e in zip(n, ends)]


def gpu_model(pkg, m):
    g = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(g), ctypes.byref(m), ctypes.sizeof(g))
    return g


def same(got, want, what):
    assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]), (what, "keys")
    assert np.array_equal(got[1].view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32)), (what, "log-odds")


@functools.lru_cache(maxsize=None)
def restated(kind, m=0):
    """Shapes beyond the fixture -> (scans [(origin, points)], RayParams, leaves), computed once."""
    rp = rc.RayParams()
    if kind == "cloud":          # the first m of 1200 points around one origin
        o, p = scans_of("random")[0]
        p = np.concatenate([p, scans_of("scene")[1][1][:176]])
        assert len(p) == 1200
        scans = [(o, p[:m])]
    elif kind == "bundle":       # 200 rays a millimetre apart: every cell near the origin is shared by all of them
        rng = np.random.default_rng(9)
        o = np.float32([0.21, -0.13, 0.07])
        scans = [(o, (o + np.float32([2.9, 1.3, 0.6]) + rng.uniform(-0.001, 0.001, (200, 3))).astype(np.float32))]
    elif kind == "planes65":     # 65 planes of 2 x 2 through 65 poses
        rng = np.random.default_rng(4)
        disp = rng.integers(150, 420, (65, 2, 2)).astype(np.int16)
        disp[7, 0, 1] = -16
        poses = np.asarray([[np.cos(0.1 * k), -np.sin(0.1 * k), 0, 0.03 * k, np.sin(0.1 * k), np.cos(0.1 * k), 0, -0.02 * k, 0, 0, 1, 0.01 * k]
                            for k in range(65)], np.float32)
        model = occ.model(local=[0, 0, 1, 0.05, -1, 0, 0, 0, 0, -1, 0, 0.2])
        rp = rc.RayParams(max_range=2.5)
        scans = [(pose[[3, 7, 11]], rc.plane_points(d, 100, model, pose)) for d, pose in zip(disp, poses)]
        t = rc.Tree(rp)
        for o, p in scans:
            t.insert(p, o)
        return (disp, poses, model, 100), rp, t.leaves()
    t = rc.Tree(rp)
    for o, p in scans:
        t.insert(p, o)
    return scans, rp, t.leaves()


@pytest.mark.parametrize("name", NAMES)
def test_every_fixture_case_through_the_cloud_form(pkg, bm, name):
    omap = pkg.OccupancyMap(bm, 1 << 16)
    try:
        rp = params_of(pkg, name)
        for s, ((o, p), want) in enumerate(zip(scans_of(name), recorded(name))):
            omap.insert_cloud(dev(p) if s % 2 == 0 else p, o, rp)       # the device form and the host form take turns
            assert omap.size() == len(want[0]), (name, s)
            same(omap.fetch_logodds(), want, (name, s))
        assert omap.overflow() == 0
    finally:
        omap.close()


@pytest.mark.parametrize("name", ["scene", "clamp"])
def test_plane_form_equals_octomap_and_the_cloud_form(pkg, bm, name):
    disp, poses, scale = FX[f"{name}_disp"], FX[f"{name}_poses"], int(FX[f"{name}_scale"])
    ref_model = occ.model_from_array(FX[f"{name}_model"])
    model = gpu_model(pkg, ref_model)
    rp = params_of(pkg, name)
    for i, (o, p) in enumerate(scans_of(name)):     # the fixture's clouds are the points the front half gives
        assert np.array_equal(p, rc.plane_points(disp[i], scale, ref_model, poses[i])) and np.array_equal(o, poses[i][[3, 7, 11]])
    omap, cloud = pkg.OccupancyMap(bm, 1 << 13), pkg.OccupancyMap(bm, 1 << 13)
    try:
        omap.insert_rays(dev(disp), model, poses, scale, rp)            # every plane in one call
        same(omap.fetch_logodds(), recorded(name)[-1], name)
        omap.reset()
        for i, want in enumerate(recorded(name)):                       # one plane per call, the host form every second time
            omap.insert_rays(dev(disp[i]) if i % 2 else disp[i], model, poses[i], scale, rp)
            cloud.insert_cloud(dev(scans_of(name)[i][1]), scans_of(name)[i][0], rp)
            got = omap.fetch_logodds()
            same(got, want, (name, i))
            same(cloud.fetch_logodds(), got, (name, i, "cloud"))
    finally:
        omap.close()
        cloud.close()


@pytest.mark.parametrize("m", [1, 63, 64, 65, 1200])
def test_cloud_sizes(pkg, bm, m):
    scans, _, want = restated("cloud", m)
    omap = pkg.OccupancyMap(bm, 1 << 16)
    try:
        omap.insert_cloud(dev(scans[0][1]), scans[0][0])
        same(omap.fetch_logodds(), want, m)
    finally:
        omap.close()


def test_many_rays_share_every_cell_near_the_origin(pkg, bm):
    scans, _, want = restated("bundle")
    shared = [set(rc.pack3(k) for k in rc.ray_keys(scans[0][0], q, 0.1)[0]) for q in scans[0][1]]
    assert len(set.intersection(*shared)) >= 20 and len(shared) >= 64
    omap = pkg.OccupancyMap(bm, 1 << 10)
    try:
        for _ in range(3):
            omap.insert_cloud(dev(scans[0][1]), scans[0][0])
        t = rc.Tree()
        for _ in range(3):
            t.insert(scans[0][1], scans[0][0])
        same(omap.fetch_logodds(), t.leaves(), "bundle")
        assert len(want[0]) == omap.size()
    finally:
        omap.close()


def test_65_planes_take_more_than_one_pose_chunk(pkg, bm):
    (disp, poses, model, scale), rp, want = restated("planes65")
    omap = pkg.OccupancyMap(bm, 1 << 12)
    try:
        omap.insert_rays(dev(disp), gpu_model(pkg, model), poses, scale, max_range=rp.max_range)
        same(omap.fetch_logodds(), want, "planes65")
    finally:
        omap.close()


def test_capacity_equal_to_the_voxel_count(pkg, bm):
    want = recorded("scene")[-1]
    omap = pkg.OccupancyMap(bm, len(want[0]))
    try:
        for o, p in scans_of("scene"):
            omap.insert_cloud(dev(p), o, params_of(pkg, "scene"))
        assert omap.overflow() == 0
        same(omap.fetch_logodds(), want, "scene at capacity")
    finally:
        omap.close()


def test_a_full_table_reports_it_and_every_stored_voxel_is_exact(pkg, bm):
    want = dict(zip((int(k) for k in recorded("scene")[-1][0]), recorded("scene")[-1][1].view(np.uint32)))
    omap = pkg.OccupancyMap(bm, 64)
    try:
        codes = []
        for o, p in scans_of("scene"):
            with pytest.raises(pkg.StereoBMError) as e:
                omap.insert_cloud(dev(p), o, params_of(pkg, "scene"))
            codes.append(e.value.code)
        assert codes == [pkg.ERR_OCC_FULL] * 3
        assert omap.overflow() > 0
        with pytest.raises(pkg.StereoBMError):
            omap.fetch_logodds()
        keys, lo = omap.fetch_logodds(allow_overflow=True)
        assert len(keys) == omap.size() == 128                      # every slot of the table
        assert np.all(np.diff(keys.astype(np.int64)) > 0)
        assert [want[int(k)] for k in keys] == list(lo.view(np.uint32))
    finally:
        omap.close()


def test_asynchronous_inserts_then_fetch(pkg, bm):
    omap = pkg.OccupancyMap(bm, 1 << 13)
    try:
        for o, p in scans_of("clamp"):
            omap.insert_cloud(dev(p), o, params_of(pkg, "clamp"), sync=False)
        same(omap.fetch_logodds(), recorded("clamp")[-1], "clamp, sync = 0")
        omap.reset()
        disp, poses = FX["scene_disp"], FX["scene_poses"]
        omap.insert_rays(dev(disp), gpu_model(pkg, occ.model_from_array(FX["scene_model"])), poses, int(FX["scene_scale"]),
                         params_of(pkg, "scene"), sync=False)
        same(omap.fetch_logodds(), recorded("scene")[-1], "scene, sync = 0")
    finally:
        omap.close()


def test_modes(pkg, bm, torch_cuda):
    """The first insert after create or reset fixes the mode; calls of the other kind are refused and change nothing."""
    torch = torch_cuda
    L = pkg.load_library()
    disp, poses, scale = FX["scene_disp"], FX["scene_poses"], int(FX["scene_scale"])
    ref_model = occ.model_from_array(FX["scene_model"])
    model = gpu_model(pkg, ref_model)
    rp = params_of(pkg, "scene")
    o, p = scans_of("scene")[0]
    hit_keys, hit_counts = occ.insert(disp, scale, ref_model, poses)
    omap = pkg.OccupancyMap(bm, 1 << 13)

    def refused(call):
        with pytest.raises(pkg.StereoBMError) as e:
            call()
        assert e.value.code == UNSUPPORTED

    try:
        assert len(omap.fetch_logodds()[0]) == 0 and len(omap.keys()[0]) == 0        # an empty map serves both
        omap.insert_cloud(dev(p), o, rp)
        refused(lambda: omap.insert(dev(disp), model, poses, scale))
        refused(lambda: omap.insert(disp, model, poses, scale))
        refused(omap.keys)
        refused(omap.keys_device)
        same(omap.fetch_logodds(), recorded("scene")[0], "after refused hit calls")
        omap.reset()
        assert omap.size() == 0
        omap.insert(dev(disp), model, poses, scale)                      # the other mode, in the same table
        refused(lambda: omap.insert_cloud(dev(p), o, rp))
        refused(lambda: omap.insert_cloud(p, o, rp))
        refused(lambda: omap.insert_rays(dev(disp), model, poses, scale, rp))
        refused(lambda: omap.insert_rays(disp, model, poses, scale, rp))
        refused(omap.fetch_logodds)
        keys, hits = omap.keys()
        assert np.array_equal(keys, hit_keys) and np.array_equal(hits, hit_counts)
        omap.reset()
        omap.insert_rays(dev(disp), model, poses, scale, rp)             # and back
        same(omap.fetch_logodds(), recorded("scene")[-1], "after reset")
        # too little room: the count is set and nothing is written
        n = omap.size()
        d_keys = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
        d_lo = torch.full((n,), -7.0, dtype=torch.float32, device="cuda:0")
        got = ctypes.c_size_t()
        assert L.sbm_occ_fetch_logodds_device(omap._m, d_keys.data_ptr(), d_lo.data_ptr(), n - 1, ctypes.byref(got)) == SIZE
        assert got.value == n and bool((d_keys == -7).all()) and bool((d_lo == -7.0).all())
        host = np.zeros(n, np.uint64)
        assert L.sbm_occ_fetch_logodds(omap._m, host.ctypes.data, None, n - 1, ctypes.byref(got)) == SIZE and not host.any()
        assert L.sbm_occ_fetch_logodds_device(omap._m, d_keys.data_ptr(), d_lo.data_ptr(), n, ctypes.byref(got)) == 0
        same((d_keys.cpu().numpy().astype(np.uint64), d_lo.cpu().numpy()), recorded("scene")[-1], "device fetch")
        # refused before anything is launched
        bad = pkg.occ_ray_params(prob_hit=0.3)
        with pytest.raises(pkg.StereoBMError) as e:
            omap.insert_cloud(dev(p), o, bad)
        assert e.value.code == SIZE
        assert L.sbm_occ_insert_cloud_device(omap._m, 4, None, o.ctypes.data, ctypes.byref(rp), 1) == -1
        assert L.sbm_occ_insert_cloud_device(omap._m, 1, dev(p).data_ptr() + 2, o.ctypes.data, ctypes.byref(rp), 1) == UNSUPPORTED
        omap.insert_cloud(p[:0], o, rp)                                  # an empty scan is a scan
        same(omap.fetch_logodds(), recorded("scene")[-1], "after refused calls")
    finally:
        omap.close()


def test_python_class_and_cpp_call_site_write_octomaps_bt(pkg, bm, tmp_path):
    disp, poses, scale = FX["scene_disp"], FX["scene_poses"], int(FX["scene_scale"])
    ref_model = occ.model_from_array(FX["scene_model"])
    rp = params_of(pkg, "scene")
    omap = pkg.OccupancyMap(bm, 1 << 13)
    try:
        omap.insert_rays(dev(disp), gpu_model(pkg, ref_model), poses, scale, rp)
        omap.write_binary_logodds(tmp_path / "py.bt")
    finally:
        omap.close()
    assert (tmp_path / "py.bt").read_bytes() == FX["scene_bt"].tobytes()
    exe, built = build_callsite(tmp_path, "occupancy_rays_callsite_main.cpp")
    assert built.returncode == 0, built.stderr
    disp.tofile(tmp_path / "planes.raw")
    poses.tofile(tmp_path / "poses.raw")
    (tmp_path / "model.raw").write_bytes(bytes(gpu_model(pkg, ref_model)))
    args = [str(exe), str(tmp_path / "planes.raw"), str(len(disp)), str(disp.shape[2]), str(disp.shape[1]), str(scale),
            str(tmp_path / "poses.raw"), str(tmp_path / "model.raw"), str(1 << 13), repr(float(rp.max_range))]
    r = subprocess.run(args + [str(tmp_path / "planes.bt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["size", str(len(recorded("scene")[-1][0])), "overflow", "0"], r.stdout + r.stderr
    assert (tmp_path / "planes.bt").read_bytes() == FX["scene_bt"].tobytes()
    cloud = np.concatenate([np.concatenate([np.float32([len(p)]), o, p.reshape(-1)]) for o, p in scans_of("scene")]).astype(np.float32)
    cloud.tofile(tmp_path / "cloud.raw")
    r = subprocess.run(args + [str(tmp_path / "cloud.bt"), str(tmp_path / "cloud.raw"), str(len(cloud))], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "cloud.bt").read_bytes() == FX["scene_bt"].tobytes()


def test_stage_names_fill(pkg):
    eng = pkg.StereoBM.create(64, 21)
    omap = pkg.OccupancyMap(eng, 1 << 13)
    try:
        eng.set_profiling(True)
        o, p = scans_of("scene")[0]
        omap.insert_cloud(dev(p), o, params_of(pkg, "scene"))
        prof = omap.profile()
        assert prof["occ_rays_mark"] > 0 and prof["occ_rays_apply"] > 0 and prof["occ_insert"] == 0 and prof["occ_fetch"] == 0
        omap.fetch_logodds()
        after = omap.profile()
        assert after["occ_fetch"] > 0 and after["occ_rays_mark"] == prof["occ_rays_mark"]      # a fetch keeps the insert's times
        disp, poses = FX["scene_disp"], FX["scene_poses"]
        omap.insert_rays(dev(disp), gpu_model(pkg, occ.model_from_array(FX["scene_model"])), poses, int(FX["scene_scale"]),
                         params_of(pkg, "scene"))
        three = omap.profile()
        assert three["occ_rays_mark"] > 0 and three["occ_rays_apply"] > 0 and three["occ_fetch"] == after["occ_fetch"]
    finally:
        eng.set_profiling(False)
        omap.close()
        eng.close()
