"""The GPU occupancy map's growth (u96-slam_amd/csrc/sbm_occ_grow.hip: occ_rehash_kernel, occ_claim_kernel; the settle loops of
sbm_occ_rays.hip and sbm_occupancy.hip; the loaders' reserve). No kernel, fixture or restatement of the family depends on
which slot a key sits in, so a map that starts with ONE voxel of capacity (two slots, probe bound 2) and grows is held to what
is already committed: what the reference's own octomap recorded in tests/golden/occupancy_*.npz, and where that holds no
record (hit counts, queries, trees, written files) to the same calls on a map created large enough. Keys are compared with
array_equal, values by their uint32 views. Every growing map also meets the memory condition at its end: the policy only
doubles, and only when the size has passed the capacity or a cell was lost, so capacity <= max(created capacity, 4 * size)."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_load_cases as lc  # noqa: E402
import occupancy_option_cases as oc  # noqa: E402
import occupancy_ot_cases as otc  # noqa: E402
import occupancy_ref as occ  # noqa: E402
from gpu_support import bm, build_callsite, dev, torch_cuda  # noqa: E402,F401

pytestmark = pytest.mark.gpu
GOLDEN = ROOT / "tests" / "golden"
RAYS = dict(np.load(GOLDEN / "occupancy_rays.npz"))
HITS = dict(np.load(GOLDEN / "occupancy_octomap.npz"))
OT = otc.fixture()
LOAD, STREAMS = lc.fixture()
RAY_NAMES = [str(n) for n in RAYS["names"]]
UNSUPPORTED = -23
PROFILE_NAMES = {"occ_insert", "occ_fetch", "occ_rays_mark", "occ_rays_apply", "occ_search", "occ_cast", "occ_load"}


def bits(a):
    a = np.asarray(a)
    return a.astype(np.float32).view(np.uint32) if a.dtype.kind == "f" else a.astype(np.uint32)


def same(got, want, what):
    assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]), (what, "keys")
    assert np.array_equal(bits(got[1]), bits(np.asarray(want[1]))), (what, "values")
    if len(want) > 2:
        assert np.array_equal(got[2], want[2]), (what, "changed keys", len(got[2]), len(want[2]))
        assert np.array_equal(np.asarray(got[3], np.uint8), np.asarray(want[3], np.uint8)), (what, "created flags")


def fits(omap, created=1):
    """the memory condition, and that nothing was lost on the way"""
    g, size = omap.growth(), omap.size()
    assert g["enabled"] == 1 and g["capacity"] == omap.capacity and g["slots"] >= 2 * g["capacity"]
    assert g["capacity"] <= max(created, 4 * size), (g, size)
    assert omap.overflow() == 0
    return g


def params_of(pkg, name):
    return pkg.occ_ray_params(*[float(v) for v in RAYS[f"{name}_params"]])


def scans_of(name):
    n = RAYS[f"{name}_npoints"]
    ends = np.cumsum(n)
    return [(RAYS[f"{name}_origins"][i], RAYS[f"{name}_points"][e - k:e]) for i, (k, e) in enumerate(zip(n, ends))]


def recorded(name):
    n = RAYS[f"{name}_nleaves"].astype(np.int64)
    ends = np.cumsum(n)
    return [(RAYS[f"{name}_keys"][e - k:e], RAYS[f"{name}_logodds"][e - k:e]) for k, e in zip(n, ends)]


def gpu_model(pkg, m):
    g = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(g), ctypes.byref(m), ctypes.sizeof(g))
    return g


def planes_of(pkg, name):
    return (RAYS[f"{name}_disp"], gpu_model(pkg, occ.model_from_array(RAYS[f"{name}_model"])), RAYS[f"{name}_poses"],
            int(RAYS[f"{name}_scale"]))


# ---- log-odds inserts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RAY_NAMES)
def test_every_ray_fixture_case_from_one_voxel_of_capacity(pkg, bm, name):
    omap = pkg.OccupancyMap(bm, 1, grow=True)
    try:
        assert omap.capacity == 1 and omap.growth()["slots"] == 2
        rp = params_of(pkg, name)
        for s, ((o, p), want) in enumerate(zip(scans_of(name), recorded(name))):
            omap.insert_cloud(dev(p) if s % 2 == 0 else p, o, rp)       # the device form and the host form take turns
            assert omap.size() == len(want[0]), (name, s)
            same(omap.fetch_logodds(), want, (name, s))
            assert omap.overflow() == 0
        g = fits(omap)
        if len(recorded(name)[-1][0]) > 1:
            assert g["grown"] > 0 and g["moved"] > 0
        if name in ("scene", "clamp", "random"):                       # a first scan of a thousand voxels into two slots
            assert g["redone"] > 0
        if name == "random":
            # many steps inside one scan, past the probe bound: no step goes beyond four times the capacity, and 32 611 voxels
            # need 32 768 slots, a capacity of 4^7
            assert g["slots"] > 1024 and g["grown"] >= 7 and g["redone"] > 0
    finally:
        omap.close()


@pytest.mark.parametrize("name", ["scene", "clamp"])
def test_plane_forms_from_one_voxel_of_capacity(pkg, bm, name):
    disp, model, poses, scale = planes_of(pkg, name)
    rp = params_of(pkg, name)
    omap = pkg.OccupancyMap(bm, 1, grow=True)
    try:
        omap.insert_rays(dev(disp), model, poses, scale, rp)            # every plane in one call
        same(omap.fetch_logodds(), recorded(name)[-1], name)
        fits(omap)
        omap.close()
        omap = pkg.OccupancyMap(bm, 1, grow=True)
        for i, want in enumerate(recorded(name)):                       # one plane per call, the host form every second time
            omap.insert_rays(dev(disp[i]) if i % 2 else disp[i], model, poses[i], scale, rp)
            same(omap.fetch_logodds(), want, (name, i))
        fits(omap)
        omap.close()
        omap = pkg.OccupancyMap(bm, 1, grow=True)
        omap.insert_rays(dev(disp), model, poses, scale, rp, sync=False)
        same(omap.fetch_logodds(), recorded(name)[-1], (name, "sync = 0"))
        fits(omap)
        omap.close()
        omap = pkg.OccupancyMap(bm, 1, grow=True)
        for o, p in scans_of(name):
            omap.insert_cloud(dev(p), o, rp, sync=False)
        same(omap.fetch_logodds(), recorded(name)[-1], (name, "clouds, sync = 0"))
        fits(omap)
    finally:
        omap.close()


def test_overflow_on_a_later_scan_carries_the_flags_of_earlier_voxels(pkg, bm):
    """Created at exactly the size after scan 1: the later scans set flags on voxels of scan 1 and list their slots before
    the table has to grow, and those flags and the list ride through the rehash between MARK and APPLY."""
    first = int(RAYS["scene_nleaves"][0])
    rp = params_of(pkg, "scene")
    omap = pkg.OccupancyMap(bm, first, grow=True)
    try:
        grown = []
        for s, ((o, p), want) in enumerate(zip(scans_of("scene"), recorded("scene"))):
            omap.insert_cloud(dev(p), o, rp)
            same(omap.fetch_logodds(), want, ("scene", s))
            grown.append(omap.growth()["grown"])
        assert grown[0] == 0 and grown[-1] > 0
        fits(omap, first)
    finally:
        omap.close()


def switches(omap, s):
    if s["box"] is not None:
        omap.set_bbx(*s["box"])
    omap.use_bbx_limit(s["use_box"])
    omap.enable_change_detection(s["detect"])
    if s["reset_changes"]:
        omap.reset_change_detection()


def option_params(pkg, case):
    rp = case["params"]
    return pkg.occ_ray_params(rp.prob_hit, rp.prob_miss, rp.clamp_min, rp.clamp_max, rp.occupancy_thres, rp.max_range)


@pytest.mark.parametrize("name", oc.NAMES)
def test_every_options_fixture_case_from_one_voxel_of_capacity(pkg, bm, name):
    """The four <box, change detection> instantiations and the discretised list form; "created this scan" survives the move."""
    case, want = oc.case_of(name), oc.recorded(name)
    omap = pkg.OccupancyMap(bm, 1, grow=True)
    try:
        rp = option_params(pkg, case)
        for i, s in enumerate(case["scans"]):
            switches(omap, s)
            omap.insert_cloud(dev(s["points"]) if i % 2 == 0 else s["points"], s["origin"], rp, discretize=s["discretize"])
            same(omap.fetch_logodds() + omap.changes(), want[i], (name, i))
            assert omap.num_changes() == len(want[i][2])
        fits(omap)
    finally:
        omap.close()


def test_discretised_planes_from_one_voxel_of_capacity(pkg, bm):
    case, want = oc.case_of("scene_all"), oc.recorded("scene_all")
    disp, poses, scale = oc.FX["scene_disp"], oc.FX["scene_poses"], int(oc.FX["scene_scale"])
    model = gpu_model(pkg, occ.model_from_array(oc.FX["scene_model"]))
    rp = option_params(pkg, case)
    omap = pkg.OccupancyMap(bm, 1, grow=True)
    try:
        for i, s in enumerate(case["scans"]):
            switches(omap, s)
            omap.insert_rays(dev(disp[i]), model, poses[i], scale, rp, discretize=True)
            same(omap.fetch_logodds() + omap.changes(), want[i], ("planes", i))
        fits(omap)
    finally:
        omap.close()


# ---- hit inserts --------------------------------------------------------------------------------------------------------------
def hit_planes(pkg):
    return (HITS["scene_disp"], gpu_model(pkg, occ.model_from_array(HITS["model"])), HITS["scene_poses"], int(HITS["scale"]),
            dict(resolution=float(HITS["resolution"]), range_max=float(HITS["range_max"])))


def planes65(pkg):
    """65 planes of 2 x 2 through 65 poses, as tests/test_gpu_occupancy_rays.py builds them: more than one pose chunk"""
    rng = np.random.default_rng(4)
    disp = rng.integers(150, 420, (65, 2, 2)).astype(np.int16)
    disp[7, 0, 1] = -16
    poses = np.asarray([[np.cos(0.1 * k), -np.sin(0.1 * k), 0, 0.03 * k, np.sin(0.1 * k), np.cos(0.1 * k), 0, -0.02 * k, 0, 0, 1, 0.01 * k]
                        for k in range(65)], np.float32)
    return disp, gpu_model(pkg, occ.model(local=[0, 0, 1, 0.05, -1, 0, 0, 0, 0, -1, 0, 0.2])), poses, 100, {}


@pytest.mark.parametrize("planes", [hit_planes, planes65], ids=["fixture", "planes65"])
def test_hit_inserts_from_one_voxel_of_capacity(pkg, bm, planes):
    disp, model, poses, scale, kw = planes(pkg)
    ample = pkg.OccupancyMap(bm, 1 << 16, **kw)
    maps = [ample]
    try:
        ample.insert(dev(disp), model, poses, scale)
        want = ample.keys()
        assert len(want[0]) > 1 and ample.overflow() == 0
        for how in ("one call", "one plane per call", "sync = 0", "host"):
            omap = pkg.OccupancyMap(bm, 1, grow=True, **kw)
            maps.append(omap)
            if how == "one plane per call":
                for i in range(len(disp)):
                    omap.insert(dev(disp[i]) if i % 2 else disp[i], model, poses[i], scale)
            elif how == "host":
                omap.insert(disp, model, poses, scale)
            else:
                omap.insert(dev(disp), model, poses, scale, sync=how == "one call")
            got = omap.keys()
            same(got, want, how)
            assert int(got[1].astype(np.int64).sum()) == int(want[1].astype(np.int64).sum())
            g = fits(omap)
            assert g["grown"] > 0 and g["redone"] > 0
            omap.insert(dev(disp), model, poses, scale)                  # a second round finds every key: counts double
            again = omap.keys()
            assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], 2 * want[1])
            fits(omap)
    finally:
        for m in maps:
            m.close()


def test_hit_insert_that_fits_runs_no_claim_pass(pkg, bm):
    disp, model, poses, scale, kw = hit_planes(pkg)
    omap = pkg.OccupancyMap(bm, disp.size, grow=True, **kw)            # the host's bound: every pixel a new voxel
    try:
        omap.insert(dev(disp), model, poses, scale)
        g = omap.growth()
        assert g["grown"] == 0 and g["redone"] == 0 and g["capacity"] == disp.size and omap.overflow() == 0
    finally:
        omap.close()


# ---- reserve ------------------------------------------------------------------------------------------------------------------
def test_reserve_in_hit_mode(pkg, bm):
    disp, model, poses, scale, kw = hit_planes(pkg)
    omap, ample = pkg.OccupancyMap(bm, 2048, **kw), pkg.OccupancyMap(bm, 1 << 16, **kw)
    try:
        omap.insert(dev(disp[:2]), model, poses[:2], scale)
        before = omap.keys()
        omap.reserve(4 * 2048)
        assert omap.capacity == 4 * 2048 and omap.growth()["slots"] == 8 * 2048 and omap.growth()["grown"] == 1
        assert omap.growth()["moved"] == len(before[0]) and omap.growth()["enabled"] == 0
        same(omap.keys(), before, "after reserve")
        omap.reserve(100)                                                # smaller: nothing happens
        omap.reserve(4 * 2048)
        assert omap.capacity == 4 * 2048 and omap.growth()["grown"] == 1
        omap.insert(dev(disp[2:]), model, poses[2:], scale)
        ample.insert(dev(disp), model, poses, scale)
        same(omap.keys(), ample.keys(), "a further insert")
        with pytest.raises(pkg.StereoBMError) as e:
            omap.reserve((1 << 30) + 1)
        assert e.value.code == UNSUPPORTED
        assert omap.capacity == 4 * 2048 and omap.growth()["grown"] == 1
        same(omap.keys(), ample.keys(), "after the refused reserve")
    finally:
        omap.close()
        ample.close()


def test_reserve_in_logodds_mode_with_changes_pending(pkg, bm):
    case, want = oc.case_of("scene_all"), oc.recorded("scene_all")
    rp = option_params(pkg, case)
    omap = pkg.OccupancyMap(bm, 1 << 12)
    try:
        for i, s in enumerate(case["scans"]):
            switches(omap, s)
            omap.enable_change_detection(True)
            if i == len(case["scans"]) - 1:
                before, pending, n = omap.fetch_logodds(), omap.changes(), omap.num_changes()
                assert n > 0
                omap.reserve(4 << 12)
                assert omap.capacity == 4 << 12 and omap.num_changes() == n and omap.bbx()["enabled"] == bool(s["use_box"])
                same(omap.fetch_logodds() + omap.changes(), before + pending, "after reserve")
                assert omap.change_detection_enabled() and omap.overflow() == 0
            omap.insert_cloud(dev(s["points"]), s["origin"], rp, discretize=s["discretize"])
        ref = oc.Tree(case["params"])                                   # the record's scans with detection on from the first
        for s in case["scans"]:
            oc.apply_switches(ref, s)
            ref.detect = True
            ref.insert(s["points"], s["origin"], s["discretize"])
        same(omap.fetch_logodds() + omap.changes(), ref.leaves() + ref.changed(), "a further scan")
        same(omap.fetch_logodds(), want[-1][:2], "the record's leaves")
        with pytest.raises(pkg.StereoBMError) as e:
            omap.reserve((1 << 30) + 1)
        assert e.value.code == UNSUPPORTED and omap.capacity == 4 << 12
        same(omap.fetch_logodds(), want[-1][:2], "after the refused reserve")
    finally:
        omap.close()


# ---- after growth: queries, trees, files -----------------------------------------------------------------------------------------
def test_queries_trees_and_files_after_growth_equal_the_pre_sized_map(pkg, bm, torch_cuda, tmp_path):
    rp = params_of(pkg, "scene")
    scans = scans_of("scene")
    grown, ample = pkg.OccupancyMap(bm, 1, grow=True), pkg.OccupancyMap(bm, 1 << 14)
    early = None
    try:
        for i, (o, p) in enumerate(scans):
            grown.insert_cloud(dev(p), o, rp)
            ample.insert_cloud(dev(p), o, rp)
            if i == 0:
                early = grown.tree(pkg.OCC_TREE_LOGODDS)             # built before the later growth
                early_leaves, early_found = early.leaves(), early.search(p[:256])
                early_capacity = grown.capacity
        assert grown.capacity > early_capacity and len(early_leaves[0]) > 0
        same(grown.fetch_logodds(), ample.fetch_logodds(), "leaves")
        o, p = scans[1]
        probe = np.concatenate([p, p + np.float32(0.05), o[None]]).astype(np.float32)
        for a, b in zip(grown.search(dev(probe)), ample.search(dev(probe))):
            assert torch_cuda.equal(a, b)
        dirs = (p - o).astype(np.float32)
        for a, b in zip(grown.cast_rays(o, dev(dirs), max_range=6.0), ample.cast_rays(o, dev(dirs), max_range=6.0)):
            assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))
        tg, ta = grown.tree(pkg.OCC_TREE_LOGODDS), ample.tree(pkg.OCC_TREE_LOGODDS)
        for a, b in zip(tg.leaves(), ta.leaves()):
            assert np.array_equal(bits(a), bits(b)) and a.dtype == b.dtype
        assert tg.info() == ta.info()
        mg, ma = grown.tree(pkg.OCC_TREE_MAXLIKELIHOOD, rp), ample.tree(pkg.OCC_TREE_MAXLIKELIHOOD, rp)
        assert torch_cuda.equal(mg.binary(), ma.binary()) and len(mg.binary()) > 0
        tg.write_ot(tmp_path / "grown.ot")
        ta.write_ot(tmp_path / "ample.ot")
        assert (tmp_path / "grown.ot").read_bytes() == (tmp_path / "ample.ot").read_bytes()
        back = pkg.OccupancyMap(bm, 1, grow=True)
        try:
            back.load_ot(tmp_path / "grown.ot")
            same(back.fetch_logodds(), ample.fetch_logodds(), "write_ot, load_ot")
            assert back.capacity == back.size()
        finally:
            back.close()
        for a, b in zip(early.leaves() + early.search(scans[0][1][:256]), early_leaves + early_found):   # the snapshot answers as built
            assert np.array_equal(bits(a), bits(b))
        for t in (tg, ta, mg, ma):
            t.close()
    finally:
        if early is not None:
            early.close()
        grown.close()
        ample.close()


# ---- loaders ------------------------------------------------------------------------------------------------------------------
def test_loaders_reserve_on_a_growing_map_and_refuse_as_before_on_another(pkg, bm, torch_cuda):
    name = max((n for n in STREAMS if n != "size1"), key=lambda n: len(LOAD[f"{n}_leaf_key"]))
    data, rp = STREAMS[name]
    p = pkg.occ_ray_params(rp.prob_hit, rp.prob_miss, rp.clamp_min, rp.clamp_max, rp.occupancy_thres, -1.0)
    ot = bytes(OT["random_ot_0"])
    ample, small = pkg.OccupancyMap(bm, 1 << 16), pkg.OccupancyMap(bm, 1)
    maps = [ample, small]
    try:
        for load, stream in ((lambda m: m.load_binary(data, p), ".bt"), (lambda m: m.load_ot(ot), ".ot")):
            grown = pkg.OccupancyMap(bm, 1, grow=True)
            maps.append(grown)
            load(ample)
            want = ample.fetch_logodds()
            assert len(want[0]) > 1
            with pytest.raises(pkg.StereoBMError) as e:
                load(small)
            assert e.value.code == pkg.ERR_OCC_FULL and small.size() == 0 and small.capacity == 1
            load(grown)
            same(grown.fetch_logodds(), want, stream)
            assert grown.capacity == grown.size() == len(want[0]) and grown.growth()["grown"] == 1
            fits(grown)
        small.set_growth(True, 2)                                        # the ceiling applies: refused, and nothing is touched
        with pytest.raises(pkg.StereoBMError) as e:
            small.load_ot(ot)
        assert e.value.code == pkg.ERR_OCC_FULL and small.size() == 0 and small.capacity == 1
        with pytest.raises(pkg.StereoBMError) as e:
            grown.load_ot(bytes(OT["hand_childless_root"]))               # 2^48 voxels: above every ceiling
        assert e.value.code == pkg.ERR_OCC_FULL
        same(grown.fetch_logodds(), want, "after the refused load")
    finally:
        for m in maps:
            m.close()


# ---- the ceiling, and off by default ------------------------------------------------------------------------------------------
def test_the_ceiling_stops_growth_and_every_stored_voxel_is_exact(pkg, bm):
    want = dict(zip((int(k) for k in recorded("scene")[-1][0]), recorded("scene")[-1][1].view(np.uint32)))
    omap = pkg.OccupancyMap(bm, 1, grow=True, max_capacity=64)
    try:
        codes = []
        for o, p in scans_of("scene"):
            with pytest.raises(pkg.StereoBMError) as e:
                omap.insert_cloud(dev(p), o, params_of(pkg, "scene"))
            codes.append(e.value.code)
        assert codes == [pkg.ERR_OCC_FULL] * 3
        assert omap.overflow() > 0
        g = omap.growth()
        assert g["capacity"] == 64 == g["max_capacity"] == omap.capacity and g["slots"] == 128 and g["enabled"] == 1
        keys, lo = omap.fetch_logodds(allow_overflow=True)
        assert len(keys) == omap.size() == 128                      # every slot of the table at the ceiling
        assert np.all(np.diff(keys.astype(np.int64)) > 0)
        assert [want[int(k)] for k in keys] == list(lo.view(np.uint32))
    finally:
        omap.close()


def test_growth_is_off_by_default_and_survives_a_reset_when_on(pkg):
    eng = pkg.StereoBM.create(64, 21)
    omap = pkg.OccupancyMap(eng, 64)
    try:
        g = omap.growth()
        assert g == dict(enabled=0, capacity=64, slots=128, max_capacity=1 << 30, grown=0, moved=0, redone=0)
        eng.set_profiling(True)
        o, p = scans_of("scene")[0]
        with pytest.raises(pkg.StereoBMError) as e:
            omap.insert_cloud(dev(p), o, params_of(pkg, "scene"))
        assert e.value.code == pkg.ERR_OCC_FULL and omap.size() == 128 and omap.overflow() > 0
        assert omap.growth() == g and set(omap.profile()) == PROFILE_NAMES
        omap.reset()
        omap.set_growth(True, 1 << 12)
        omap.reset()
        assert omap.growth()["enabled"] == 1 and omap.growth()["max_capacity"] == 1 << 12
        omap.insert_cloud(dev(p), o, params_of(pkg, "scene"))
        same(omap.fetch_logodds(), recorded("scene")[0], "after enabling")
        prof = omap.profile()
        assert set(prof) == PROFILE_NAMES and prof["occ_rays_mark"] > 0 and prof["occ_insert"] == 0 and prof["occ_load"] == 0
        fits(omap, 64)
        with pytest.raises(pkg.StereoBMError) as e:
            omap.set_growth(True, (1 << 30) + 1)
        assert e.value.code == UNSUPPORTED and omap.growth()["max_capacity"] == 1 << 12
        omap.set_growth(False)
        assert omap.growth()["enabled"] == 0
    finally:
        eng.set_profiling(False)
        omap.close()
        eng.close()


# ---- the call site -----------------------------------------------------------------------------------------------------------
def test_cpp_call_site(pkg, bm, tmp_path):
    exe, built = build_callsite(tmp_path, "occupancy_growth_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert built.returncode == 0, built.stderr
    cloud = np.concatenate([np.concatenate([np.float32([len(p)]), o, p.reshape(-1)]) for o, p in scans_of("scene")]).astype(np.float32)
    cloud.tofile(tmp_path / "cloud.raw")
    rp = params_of(pkg, "scene")
    r = subprocess.run([str(exe), str(tmp_path / "cloud.raw"), str(len(cloud)), "8192", repr(float(rp.max_range))], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[:-1] == [f"scan {i} size {int(n)}" for i, n in enumerate(RAYS["scene_nleaves"])], r.stdout
    last = lines[-1].split()
    assert last[0] == "capacity" and int(last[1]) <= 4 * int(RAYS["scene_nleaves"][-1]) and int(last[3]) > 0 and int(last[5]) == 4 * 8192
