"""The GPU occupancy map's insert options (u96-slam_amd/csrc/sbm_occ_rays.hip: the kBox / kTrack instantiations and the dedupe
launch; sbm_occ_options.hip: the box, the change states and their fetch) against what the reference's own octomap answered
(tests/golden/occupancy_options.npz) and, for shapes the fixture does not hold, against the restatement
tests/occupancy_option_cases.py, which tests/test_occupancy_options_restatement.py pins to the same fixture. Everything is compared
for exact equality: sorted keys, the bits of the float log-odds, the changed keys and their flags."""
import ctypes
import functools
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_option_cases as oc  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402
import occupancy_ref as occ  # noqa: E402
from gpu_support import bm, build_callsite, dev, torch_cuda  # noqa: E402,F401

pytestmark = pytest.mark.gpu
FX, NAMES = oc.FX, oc.NAMES
RAYS = dict(np.load(ROOT / "tests" / "golden" / "occupancy_rays.npz"))
UNSUPPORTED, SIZE, NULL = -23, -2, -1
WHOLE = ((-3276, -3276, -3276), (3276, 3276, 3276))      # a box that holds every key the cases touch


def ray_params(pkg, case):
    rp = case["params"]
    return pkg.occ_ray_params(rp.prob_hit, rp.prob_miss, rp.clamp_min, rp.clamp_max, rp.occupancy_thres, rp.max_range)


def gpu_model(pkg, m):
    g = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(g), ctypes.byref(m), ctypes.sizeof(g))
    return g


def switches(omap, s):
    if s["box"] is not None:
        omap.set_bbx(*s["box"])
    omap.use_bbx_limit(s["use_box"])
    omap.enable_change_detection(s["detect"])
    if s["reset_changes"]:
        omap.reset_change_detection()


def state(omap):
    return omap.fetch_logodds() + omap.changes()


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "keys", len(got[0]), len(want[0]))
    assert np.array_equal(np.asarray(got[1], np.float32).view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32)), (what, "log-odds")
    if len(want) > 2:
        assert np.array_equal(got[2], want[2]), (what, "changed keys", len(got[2]), len(want[2]))
        assert np.array_equal(np.asarray(got[3], np.uint8), np.asarray(want[3], np.uint8)), (what, "created flags")


def rays_scans(name):
    n = RAYS[f"{name}_npoints"]
    ends = np.cumsum(n)
    return [(RAYS[f"{name}_origins"][i], RAYS[f"{name}_points"][e - k:e]) for i, (k, e) in enumerate(zip(n, ends))]


def rays_recorded(name):
    n = RAYS[f"{name}_nleaves"].astype(np.int64)
    ends = np.cumsum(n)
    return [(RAYS[f"{name}_keys"][e - k:e], RAYS[f"{name}_logodds"][e - k:e]) for k, e in zip(n, ends)]


@functools.lru_cache(maxsize=None)
def one_voxel(m):
    """m distinct points of one voxel three metres out, discretised under detection -> (origin, points, what the restatement holds)"""
    rng = np.random.default_rng(3)
    lo = (np.float64([30, 12, -7]) * 0.1).astype(np.float32)
    p = np.unique((lo + rng.uniform(0.001, 0.099, (2 * m, 3))).astype(np.float32), axis=0)[:m]
    assert len(p) == m and len(oc.discretize(p, 0.1)) == 1
    o = np.float32([0.02, -0.03, 0.04])
    t = oc.Tree()
    t.detect = True
    t.insert(p, o, True)
    return o, p, t.leaves() + t.changed()


@pytest.mark.parametrize("name", NAMES)
def test_every_fixture_case_through_the_device_entry_points(pkg, bm, name):
    case, want = oc.case_of(name), oc.recorded(name)
    omap = pkg.OccupancyMap(bm, 1 << 15)
    try:
        rp = ray_params(pkg, case)
        for i, s in enumerate(case["scans"]):
            switches(omap, s)
            omap.insert_cloud(dev(s["points"]), s["origin"], rp, discretize=s["discretize"])
            same(state(omap), want[i], (name, i))
            assert omap.num_changes() == len(want[i][2])
        assert omap.overflow() == 0
    finally:
        omap.close()


@pytest.mark.parametrize("name", ["toggle", "box_face", "wrap", "scene_all"])
def test_host_forms_equal_the_device_forms(pkg, bm, name):
    case, want = oc.case_of(name), oc.recorded(name)
    omap = pkg.OccupancyMap(bm, 1 << 13)
    try:
        rp = ray_params(pkg, case)
        for i, s in enumerate(case["scans"]):
            switches(omap, s)
            omap.insert_cloud(s["points"], s["origin"], rp, discretize=s["discretize"])
            same(state(omap), want[i], (name, i, "host"))
    finally:
        omap.close()


def test_plane_forms_equal_the_cloud_form_on_scene_all(pkg, bm):
    case, want = oc.case_of("scene_all"), oc.recorded("scene_all")
    disp, poses, scale = FX["scene_disp"], FX["scene_poses"], int(FX["scene_scale"])
    ref_model = occ.model_from_array(FX["scene_model"])
    model = gpu_model(pkg, ref_model)
    rp = ray_params(pkg, case)
    for i, s in enumerate(case["scans"]):
        assert np.array_equal(s["points"], rc.plane_points(disp[i], scale, ref_model, poses[i]))
    omap, host = pkg.OccupancyMap(bm, 1 << 13), pkg.OccupancyMap(bm, 1 << 13)
    try:
        for i, s in enumerate(case["scans"]):
            switches(omap, s)
            switches(host, s)
            omap.insert_rays(dev(disp[i]), model, poses[i], scale, rp, discretize=True)
            host.insert_rays(disp[i], model, poses[i], scale, rp, discretize=True)
            same(state(omap), want[i], ("planes", i))
            same(state(host), want[i], ("planes, host", i))
        omap.reset()                                         # all three planes in one call: detection is then on from the first
        omap.enable_change_detection(False)
        omap.insert_rays(dev(disp), model, poses, scale, rp, discretize=True)
        same(omap.fetch_logodds(), want[-1][:2], "planes, one call")
    finally:
        omap.close()
        host.close()


@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 1024])
def test_discretised_clouds_of_one_voxel(pkg, bm, m):
    """Partial wavefronts, several blocks, and every lane on one chain of the dedupe set: one key is claimed once."""
    o, p, want = one_voxel(m)
    omap = pkg.OccupancyMap(bm, 1 << 10)
    try:
        omap.enable_change_detection(True)
        omap.insert_cloud(dev(p), o, discretize=True)
        same(state(omap), want, m)
        assert want[3].all() and omap.num_changes() == omap.size() == len(want[0])
    finally:
        omap.close()


@pytest.mark.parametrize("name", ["scene", "random"])
def test_options_off_and_options_that_change_nothing_give_the_ray_fixture(pkg, bm, name):
    rp = pkg.occ_ray_params(*[float(v) for v in RAYS[f"{name}_params"]])
    off, on = pkg.OccupancyMap(bm, 1 << 15), pkg.OccupancyMap(bm, 1 << 15)
    try:
        off.set_bbx((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))       # a box that is set and not used; states allocated and switched off
        off.enable_change_detection(True)
        off.enable_change_detection(False)
        on.set_bbx(*WHOLE)                                     # the kBox and kTrack kernels where they may change no value
        on.use_bbx_limit(True)
        on.enable_change_detection(True)
        for i, ((o, p), want) in enumerate(zip(rays_scans(name), rays_recorded(name))):
            off.insert_cloud(dev(p), o, rp)
            on.insert_cloud(dev(p), o, rp)
            same(off.fetch_logodds(), want, (name, i, "off"))
            same(on.fetch_logodds(), want, (name, i, "on"))
        assert off.num_changes() == 0 and len(off.changes()[0]) == 0
        keys, created = on.changes()
        assert np.array_equal(keys, rays_recorded(name)[-1][0]) and created.all()     # every voxel was created under detection
    finally:
        off.close()
        on.close()


def test_change_fetch_sizes_and_device_form(pkg, bm, torch_cuda):
    torch = torch_cuda
    L = pkg.load_library()
    case, want = oc.case_of("scene_all"), oc.recorded("scene_all")
    omap = pkg.OccupancyMap(bm, 1 << 13)
    try:
        got = ctypes.c_size_t(99)
        assert L.sbm_occ_fetch_changes(omap._m, None, None, 0, ctypes.byref(got)) == 0 and got.value == 0     # never enabled
        rp = ray_params(pkg, case)
        for s in case["scans"]:
            switches(omap, s)
            omap.insert_cloud(dev(s["points"]), s["origin"], rp, discretize=True)
        before = omap.fetch_logodds()
        n = omap.num_changes()
        assert n == len(want[-1][2]) > 64
        d_keys = torch.full((n,), -7, dtype=torch.int64, device="cuda:0")
        d_flag = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
        assert L.sbm_occ_fetch_changes_device(omap._m, d_keys.data_ptr(), d_flag.data_ptr(), n - 1, ctypes.byref(got)) == SIZE
        assert got.value == n and bool((d_keys == -7).all()) and bool((d_flag == 9).all())
        host = np.zeros(n, np.uint64)
        assert L.sbm_occ_fetch_changes(omap._m, host.ctypes.data, None, n - 1, ctypes.byref(got)) == SIZE and got.value == n and not host.any()
        assert L.sbm_occ_fetch_changes_device(omap._m, d_keys.data_ptr() + 4, d_flag.data_ptr(), n, ctypes.byref(got)) == UNSUPPORTED
        assert L.sbm_occ_fetch_changes_device(omap._m, None, None, n, ctypes.byref(got)) == NULL
        assert L.sbm_occ_fetch_changes_device(omap._m, d_keys.data_ptr(), None, n, ctypes.byref(got)) == 0 and got.value == n
        assert np.array_equal(d_keys.cpu().numpy().astype(np.uint64), want[-1][2]) and bool((d_flag == 9).all())
        keys, flags = omap.changes_device()
        assert np.array_equal(keys.cpu().numpy().astype(np.uint64), want[-1][2]) and np.array_equal(flags.cpu().numpy(), want[-1][3])
        same(omap.fetch_logodds(), before, "the map after the fetches")
        assert omap.num_changes() == n
    finally:
        omap.close()


def test_reset_and_loaders_clear_the_states_and_keep_the_switches(pkg, bm, tmp_path):
    case, want = oc.case_of("toggle"), oc.recorded("toggle")
    rp = ray_params(pkg, case)
    box = (np.float32([-1.03, -2, -3]), np.float32([4, 5, 6.5]))
    omap = pkg.OccupancyMap(bm, 1 << 10)

    def first_scan():
        s = case["scans"][0]
        omap.insert_cloud(dev(s["points"]), s["origin"], rp)
        same(state(omap), want[0], "first scan")

    def kept():
        b = omap.bbx()
        assert b["enabled"] and omap.change_detection_enabled() and np.array_equal(b["min"], box[0]) and np.array_equal(b["max"], box[1])
        assert list(b["min_key"]) == [32768 - 11, 32768 - 20, 32768 - 30] and list(b["max_key"]) == [32768 + 40, 32768 + 50, 32768 + 65]

    try:
        b = omap.bbx()
        assert not b["enabled"] and not b["min"].any() and list(b["max_key"]) == [32768] * 3 and not omap.change_detection_enabled()
        omap.set_bbx(*box)
        with pytest.raises(pkg.StereoBMError) as e:
            omap.set_bbx((0, 0, 0), (0, np.nan, 0))
        assert e.value.code == SIZE
        with pytest.raises(pkg.StereoBMError):
            omap.set_bbx((0, -4000.0, 0), (1, 1, 1))
        omap.use_bbx_limit(True)
        omap.enable_change_detection(True)
        kept()
        first_scan()
        omap.write_binary_logodds(tmp_path / "map.bt")
        ot = omap.tree(pkg.OCC_TREE_LOGODDS).ot()
        leaves = omap.fetch_logodds()
        omap.reset()
        assert omap.num_changes() == 0 and omap.size() == 0
        kept()
        first_scan()                                          # the states work as before
        omap.load_ot(ot)
        assert omap.num_changes() == 0                        # cleared, and the load records nothing
        same(omap.fetch_logodds(), leaves, "after load_ot")
        kept()
        omap.reset()
        first_scan()
        omap.load_binary(tmp_path / "map.bt", rp)
        assert omap.num_changes() == 0 and omap.size() == len(leaves[0])
        kept()
        omap.enable_change_detection(False)                   # disabling keeps what is recorded
        omap.reset()
        omap.enable_change_detection(True)
        first_scan()
        omap.enable_change_detection(False)
        assert omap.num_changes() == len(want[0][2])
        omap.reset_change_detection()
        assert omap.num_changes() == 0
    finally:
        omap.close()


def test_hit_mode_refusals(pkg, bm):
    disp, poses, scale = FX["scene_disp"], FX["scene_poses"], int(FX["scene_scale"])
    ref_model = occ.model_from_array(FX["scene_model"])
    model = gpu_model(pkg, ref_model)
    hit_keys, hit_counts = occ.insert(disp, scale, ref_model, poses)
    omap = pkg.OccupancyMap(bm, 1 << 13)

    def refused(call):
        with pytest.raises(pkg.StereoBMError) as e:
            call()
        assert e.value.code == UNSUPPORTED

    try:
        omap.insert(dev(disp), model, poses, scale)
        refused(lambda: omap.use_bbx_limit(True))
        refused(lambda: omap.enable_change_detection(True))
        refused(omap.num_changes)
        refused(omap.changes)
        refused(omap.changes_device)
        omap.use_bbx_limit(False)                             # switching off is no change
        omap.enable_change_detection(False)
        omap.set_bbx((-1, -1, -1), (1, 1, 1))                 # the box itself is only two points
        assert not omap.bbx()["enabled"] and not omap.change_detection_enabled()
        keys, hits = omap.keys()
        assert np.array_equal(keys, hit_keys) and np.array_equal(hits, hit_counts)
        omap.reset()
        for enable in (omap.use_bbx_limit, omap.enable_change_detection):
            enable(True)
            refused(lambda: omap.insert(dev(disp), model, poses, scale))
            refused(lambda: omap.insert(disp, model, poses, scale))
            assert omap.size() == 0
            enable(False)
        omap.insert(disp, model, poses, scale)                # no mode was fixed by the refused calls
        keys, hits = omap.keys()
        assert np.array_equal(keys, hit_keys) and np.array_equal(hits, hit_counts)
    finally:
        omap.close()


def test_asynchronous_scans_then_one_fetch(pkg, bm):
    for name in ("toggle", "scene_all"):
        case, want = oc.case_of(name), oc.recorded(name)
        omap = pkg.OccupancyMap(bm, 1 << 13)
        try:
            rp = ray_params(pkg, case)
            for s in case["scans"]:
                switches(omap, s)
                omap.insert_cloud(dev(s["points"]), s["origin"], rp, sync=False, discretize=s["discretize"])
            same(state(omap), want[-1], (name, "sync = 0"))
        finally:
            omap.close()


def test_new_launches_are_timed_under_the_existing_names(pkg):
    eng = pkg.StereoBM.create(64, 21)
    omap = pkg.OccupancyMap(eng, 1 << 13)
    try:
        eng.set_profiling(True)
        case = oc.case_of("scene_all")
        s = case["scans"][0]
        switches(omap, s)
        omap.enable_change_detection(True)
        omap.insert_cloud(dev(s["points"]), s["origin"], ray_params(pkg, case), discretize=True)
        prof = omap.profile()
        assert set(prof) == {"occ_insert", "occ_fetch", "occ_rays_mark", "occ_rays_apply", "occ_search", "occ_cast", "occ_load"}
        assert prof["occ_rays_mark"] > 0 and prof["occ_rays_apply"] > 0 and prof["occ_fetch"] == 0 and prof["occ_insert"] == 0
        assert len(omap.changes()[0]) > 0
        after = omap.profile()
        assert after["occ_fetch"] > 0 and after["occ_rays_mark"] == prof["occ_rays_mark"]
    finally:
        eng.set_profiling(False)
        omap.close()
        eng.close()


def test_cpp_call_site(pkg, bm, tmp_path):
    case, want = oc.case_of("toggle"), oc.recorded("toggle")
    exe, built = build_callsite(tmp_path, "occupancy_options_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert built.returncode == 0, built.stderr
    cloud = np.concatenate([np.concatenate([np.float32([len(s["points"])]), s["origin"], s["points"].reshape(-1)]) for s in case["scans"]])
    cloud.astype(np.float32).tofile(tmp_path / "cloud.raw")
    r = subprocess.run([str(exe), str(tmp_path / "cloud.raw"), str(len(cloud)), "1024", "-1", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    t = oc.Tree(case["params"])
    t.detect = True
    lines = []
    for s in case["scans"]:                                   # the program resets detection before every scan
        t.reset_changes()
        t.insert(s["points"], s["origin"])
        lines.append(f"changes {len(t.changes)} created {int(t.changed()[1].sum())}")
    assert r.stdout.splitlines() == lines + [f"size {len(want[-1][0])}"], r.stdout
    r = subprocess.run([str(exe), str(tmp_path / "cloud.raw"), str(len(cloud)), "1024", "-1", "1", "1", "-1", "-1", "-1", "1", "1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "size 0", r.stdout + r.stderr     # min > max: nothing is inside
