"""The GPU occupancy map edited by key (u96-slam_amd/csrc/sbm_occ_edit.hip: CLAIM, the map's radix sort, APPLY, the marking
kernels and the move behind the removal mask), held to what the reference's own octomap recorded in
tests/golden/occupancy_edit.npz after every step, and where that holds no record to the restatement
tests/occupancy_edit_cases.py. Every comparison is exact: keys with array_equal, values by their uint32 views."""
import ctypes
import functools
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_edit_cases as ec  # noqa: E402
import occupancy_ot_cases as otc  # noqa: E402
import occupancy_query_cases as qc  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402
import occupancy_ref as occ  # noqa: E402
import occupancy_tree_cases as tc  # noqa: E402
from gpu_support import bm, build_callsite, dev, torch_cuda  # noqa: E402,F401

pytestmark = pytest.mark.gpu
NULL, SIZE, UNSUPPORTED = -1, -2, -23
PROFILE_NAMES = {"occ_insert", "occ_fetch", "occ_rays_mark", "occ_rays_apply", "occ_search", "occ_cast", "occ_load"}
HITS = dict(np.load(ROOT / "tests" / "golden" / "occupancy_octomap.npz"))
DIVERGES = {(ec.LAST_VOXEL, 1), (ec.CHANGE_RECORD, 2), (ec.CHANGE_RECORD, 3)}     # (case, step) where octomap's record differs, as stated


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def same(got, want, what):
    assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]), (what, "keys")
    assert np.array_equal(bits(got[1]), bits(want[1])), (what, "values")


def same_changes(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "changed keys", len(got[0]), len(want[0]))
    assert np.array_equal(np.asarray(got[1], np.uint8), np.asarray(want[1], np.uint8)), (what, "created flags")


@functools.lru_cache(maxsize=None)
def restated(name):
    return ec.run_case(ec.case_of(name))


def d_keys(keys):
    return dev(np.ascontiguousarray(keys, np.uint64).view(np.int64))


class GpuSteps:
    """What ec.apply_step drives, on an OccupancyMap; device: the device forms, else the host forms"""

    def __init__(self, pkg, omap, rp, device):
        self.pkg, self.omap, self.rp, self.device = pkg, omap, rp, device
        lo = pkg.occ_ray_logodds(rp)
        self.hit, self.miss = lo[0], lo[1]
        self.deleted = False

    detect = property(lambda self: self.omap.change_detection_enabled(), lambda self, on: self.omap.enable_change_detection(on))

    def reset_changes(self):
        self.omap.reset_change_detection()

    def up(self, a, keys=False):
        return (d_keys(a) if keys else dev(a)) if self.device else a

    def insert(self, points, origin):
        self.omap.insert_cloud(self.up(np.ascontiguousarray(points, np.float32)), origin, self.rp)

    def edit(self, keys, ops, values):
        self.deleted |= bool((np.asarray(ops) == ec.DELETE).any())
        self.omap.edit(self.up(keys, True), self.up(np.asarray(ops, np.uint8)), self.up(np.asarray(values, np.float32)), self.rp)

    def edit_points(self, points, ops, values):
        self.deleted |= bool((np.asarray(ops) == ec.DELETE).any())
        self.omap.edit(self.up(np.ascontiguousarray(points, np.float32)), self.up(np.asarray(ops, np.uint8)),
                       self.up(np.asarray(values, np.float32)), self.rp)

    def delete(self, keys, depth):
        self.deleted = True
        self.omap.delete_nodes(self.up(keys, True), depth)

    def delete_box(self, kmin, kmax, outside):
        self.deleted = True
        self.omap.delete_box(kmin, kmax, outside)


def run_fixture_case(pkg, bm, name, device, capacity, grow=False, after_step=None):
    case = ec.case_of(name)
    rp = pkg.occ_ray_params(*[getattr(case["params"], k) for k in ("prob_hit", "prob_miss", "clamp_min", "clamp_max", "occupancy_thres",
                                                                    "max_range")])
    omap = pkg.OccupancyMap(bm, capacity, grow=grow)
    try:
        g = GpuSteps(pkg, omap, rp, device)
        for i, (s, theirs, mine) in enumerate(zip(case["steps"], ec.recorded(name), restated(name))):
            ec.apply_step(g, s)
            got, changes = omap.fetch_logodds(), omap.changes()
            assert omap.size() == len(mine[0]) and omap.overflow() == 0, (name, i)
            same(got, mine, (name, i, "restatement"))
            same_changes(changes, mine[2:], (name, i, "restatement"))
            if (name, i) not in DIVERGES:
                same(got, theirs, (name, i, "octomap"))
                same_changes(changes, theirs[2:4], (name, i, "octomap"))
            if after_step:
                after_step(omap, g, i)
        return omap
    except BaseException:
        omap.close()
        raise


# ---- 1. every fixture case, device and host forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("name", ec.NAMES)
def test_every_fixture_case_equals_octomap_after_every_step(pkg, bm, name, device):
    omap = run_fixture_case(pkg, bm, name, device, 1 << 13)
    try:
        if name == ec.LAST_VOXEL:                      # the divergence: an empty map whose search says unknown
            key = ec.case_of(name)["probes"]
            pts = np.float32([[qc.centre((int(k) >> 32, int(k) >> 16 & 0xFFFF, int(k) & 0xFFFF), 0.1)] for k in key]).reshape(-1, 3)
            state, _ = omap.search(pts)
            theirs = ec.recorded(name)[1]
            assert omap.size() == 0 and (state == qc.CELL_UNKNOWN).all() and theirs[4] and theirs[6].all()
    finally:
        omap.close()


# ---- 2. run shapes ---------------------------------------------------------------------------------------------------------------
def run_shape(n, shape, rng):
    """-> keys, ops, values of n items. The sorted order of the keys is what the shapes are about."""
    ids = np.arange(2049)
    if shape == "same":
        ids[:] = 7
    elif shape == "straddle":                          # in sorted order: a run over positions 60..67 and one over 1020..1027
        ids[60:68], ids[1020:1028] = 60, 1020
    elif shape == "long":                              # a run longer than a tile of the sort, from position 300 on
        ids[300:1500] = 300
    ids = ids[:n]
    keys = np.array([rc.pack3((32768 - 300 + int(i), 32768 + (int(i) * 7) % 11, 32768 - (int(i) % 5))) for i in ids], np.uint64)
    order = rng.permutation(n)
    keys = keys[order]
    if n >= 2 and shape != "distinct":                 # the first item of the call and the last are in the same run
        runs = [k for k in set(map(int, keys)) if (keys == k).sum() >= 2]
        if runs:
            at = np.flatnonzero(keys == runs[0])
            for src, dst in ((at[0], 0), (at[1], n - 1)):
                keys[[src, dst]] = keys[[dst, src]]
            assert keys[0] == keys[-1]
    ops = rng.choice(np.uint8([ec.UPDATE, ec.UPDATE, ec.SET, ec.DELETE]), n)
    values = rng.choice(np.float32([0.8472979, -0.4054651, 0.0, 3.0, -3.0, 1.5, -0.25]), n).astype(np.float32)
    return keys, ops, values


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_run_shapes_against_the_restatement(pkg, bm, n):
    rng = np.random.default_rng(1000 + n)
    rp = pkg.occ_ray_params()
    for shape in ("distinct", "same", "straddle", "long"):
        omap, t = pkg.OccupancyMap(bm, 1 << 13), ec.Tree()
        try:
            omap.enable_change_detection(True)
            t.detect = True
            half, _, _ = run_shape(2049, "distinct", rng)                      # every second voxel exists before the call
            omap.edit(d_keys(half[::2]), dev(np.full(len(half[::2]), ec.SET, np.uint8)), dev(np.full(len(half[::2]), 0.5, np.float32)), rp)
            t.edit(half[::2], np.full(len(half[::2]), ec.SET), np.full(len(half[::2]), 0.5, np.float32))
            keys, ops, values = run_shape(n, shape, rng)
            if n % 2:
                omap.edit(d_keys(keys), dev(ops), dev(values), rp)
            else:
                omap.edit(keys, ops, values, rp)
            t.edit(keys, ops, values)
            same(omap.fetch_logodds(), t.leaves(), (n, shape))
            same_changes(omap.changes(), t.changed(), (n, shape))
            info = omap.last_edit()
            assert info == dict(t.last, lost=0), (n, shape, info, t.last)
            assert omap.size() == len(t.v) and omap.overflow() == 0
            keys, _, values = run_shape(n, shape, rng)                          # ops NULL: all updates, no removal mask
            omap.update_nodes(d_keys(keys), dev(values), rp, sync=False)
            t.edit(keys, None, values)
            same(omap.fetch_logodds(), t.leaves(), (n, shape, "updates"))
            assert omap.last_edit() == dict(t.last, lost=0)
        finally:
            omap.close()


# ---- 3. probe chains survive a removal -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by", ["keys", "box"])
def test_probe_chains_survive_a_removal(pkg, bm, by):
    keys = np.array([rc.pack3((32768 + 10 + i, 32768 + i % 2, 32768 - 4)) for i in range(100)], np.uint64)
    values = np.linspace(-1.9, 3.4, 100).astype(np.float32)
    rp = pkg.occ_ray_params()
    omap, t = pkg.OccupancyMap(bm, 64), ec.Tree()
    try:
        assert omap.growth()["slots"] == 128
        omap.set_node_values(keys, values, rp)
        t.edit(keys, np.full(100, ec.SET), values)
        assert omap.size() == 100
        if by == "keys":
            omap.delete_nodes(d_keys(keys[1::2]))
            t.delete(keys[1::2])
        else:
            lo, hi = (32768 + 10, 32768 + 1, 32768 - 4), (32768 + 109, 32768 + 1, 32768 - 4)
            omap.delete_box(lo, hi)
            t.delete_box(lo, hi)
        assert omap.last_edit()["removed"] == 50 and omap.size() == 50 and omap.growth()["slots"] == 128 and omap.overflow() == 0
        pts = np.float32([qc.centre((int(k) >> 32, int(k) >> 16 & 0xFFFF, int(k) & 0xFFFF), 0.1) for k in keys])
        state, value = omap.search(dev(pts), float(t.thres))
        state, value = state.cpu().numpy(), value.cpu().numpy().view(np.float32)
        for i, k in enumerate(int(k) for k in keys):
            if k in t.v:
                assert state[i] == (qc.CELL_OCCUPIED if t.v[k] >= t.thres else qc.CELL_FREE) and bits(value[i]) == bits(t.v[k]), i
            else:
                assert state[i] == qc.CELL_UNKNOWN, i
        origin, points = pts[1] + np.float32([0.0, 0.0, 0.3]), pts[:6]     # six short rays: a dozen new cells, present and removed ends
        omap.insert_cloud(dev(points), origin, rp)              # a further scan claims and finds in the moved table
        t.insert(points, origin)
        same(omap.fetch_logodds(), t.leaves(), by)
        assert omap.overflow() == 0 and omap.size() == len(t.v) and 50 < len(t.v) < 100
    finally:
        omap.close()


# ---- 4. deleteNode: everything, and a hit map --------------------------------------------------------------------------------------
def test_deleting_everything_leaves_an_empty_map_that_takes_inserts(pkg, bm):
    rp = pkg.occ_ray_params()
    keys = np.array([rc.pack3((32768 + i, 32768 + 2 * i, 32768 + 3 * i)) for i in range(300)], np.uint64)
    omap, t = pkg.OccupancyMap(bm, 1024), ec.Tree()
    try:
        omap.update_nodes(keys, True, rp)
        assert omap.size() == 300 and omap.last_edit()["created"] == 300
        omap.delete_nodes(np.array([keys[0], rc.pack3((9, 9, 9))], np.uint64), 1)      # the upper half of every axis; an absent key
        assert omap.size() == 0 and omap.last_edit() == dict(items=2, skipped=0, lost=0, created=0, removed=300)
        omap.delete_nodes(keys[:5], 13)                                                # of what is not there: no error, no move
        assert omap.last_edit()["removed"] == 0
        state, _ = omap.search(np.float32([[0.05, -0.05, 0.05]]))
        assert state[0] == qc.CELL_UNKNOWN
        omap.update_nodes(d_keys(keys[:7]), dev(np.full(7, 0.25, np.float32)), rp)
        t.edit(keys[:7], None, np.full(7, 0.25, np.float32))
        same(omap.fetch_logodds(), t.leaves(), "after")
        omap.delete_nodes(np.array([keys[0] | np.uint64(1 << 50)]))                    # a bit above 47: skipped
        assert omap.last_edit() == dict(items=1, skipped=1, lost=0, created=0, removed=0) and omap.size() == 7
        with pytest.raises(pkg.StereoBMError) as e:
            omap.delete_nodes(keys[:1], 17)
        assert e.value.code == UNSUPPORTED and omap.size() == 7
    finally:
        omap.close()


def test_a_hit_map_loses_the_key_and_its_count(pkg, bm):
    disp, poses = HITS["scene_disp"], HITS["scene_poses"]
    model = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(model), ctypes.byref(occ.model_from_array(HITS["model"])), ctypes.sizeof(model))
    whole, omap = pkg.OccupancyMap(bm, 1 << 12), pkg.OccupancyMap(bm, 1 << 12)
    try:
        whole.insert(dev(disp), model, poses, 4)
        omap.insert(dev(disp), model, poses, 4)
        keys, counts = whole.keys()
        gone = keys[::3]
        bm.set_profiling(True)
        omap.delete_nodes(d_keys(gone))
        prof = omap.profile()
        bm.set_profiling(False)
        assert set(prof) == PROFILE_NAMES and prof["occ_insert"] > 0
        stay = ~np.isin(keys, gone)
        got = omap.keys()
        assert np.array_equal(got[0], keys[stay]) and np.array_equal(got[1], counts[stay]) and omap.size() == stay.sum()
        assert omap.last_edit()["removed"] == len(gone) and omap.overflow() == 0
        omap.set_growth(True)
        omap.insert(dev(disp), model, poses, 4)
        got = omap.keys()
        assert np.array_equal(got[0], keys) and np.array_equal(got[1], np.where(stay, 2 * counts, counts)) and omap.size() == len(keys)
        with pytest.raises(pkg.StereoBMError) as e:                                     # update and set belong to the log-odds mode
            omap.update_nodes(d_keys(keys[:4]), dev(np.zeros(4, np.float32)))
        assert e.value.code == UNSUPPORTED
        with pytest.raises(pkg.StereoBMError) as e:
            omap.set_node_values(keys[:4], np.zeros(4, np.float32))
        assert e.value.code == UNSUPPORTED
        again = omap.keys()
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
    finally:
        bm.set_profiling(False)
        whole.close()
        omap.close()


# ---- 5. the box delete leaves the insert's box alone ----------------------------------------------------------------------------------
def test_box_delete_does_not_touch_the_inserts_box(pkg, bm):
    omap = run_fixture_case(pkg, bm, "box_delete", True, 1 << 12)
    omap.close()
    omap = pkg.OccupancyMap(bm, 256)
    try:
        omap.set_bbx((-1.0, -2.0, -0.5), (1.5, 2.5, 0.75))
        omap.use_bbx_limit(True)
        before = omap.bbx()
        omap.update_nodes(np.array([rc.pack3((32768, 32768, 32768)), rc.pack3((32768 + 40, 32768, 32768))], np.uint64), True)
        omap.delete_box((32768 + 40, 32768, 32768), (32768 + 40, 32768, 32768))
        after = omap.bbx()
        assert omap.size() == 1 and all(np.array_equal(before[k], after[k]) for k in before) and after["enabled"]
    finally:
        omap.close()


# ---- 6. growth ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.NAMES)
def test_every_fixture_case_from_one_voxel_of_capacity(pkg, bm, name):
    def fits(omap, g, i):
        if not g.deleted:
            gr = omap.growth()
            assert gr["capacity"] <= max(1, 4 * omap.size()), (name, i, gr)

    omap = run_fixture_case(pkg, bm, name, True, 1, grow=True, after_step=fits)
    try:
        g = omap.growth()
        assert g["enabled"] == 1 and (g["grown"] > 0 or name == ec.LAST_VOXEL) and omap.overflow() == 0       # one voxel fits a capacity of one
    finally:
        omap.close()


# ---- 7. a full table with growth off -----------------------------------------------------------------------------------------------
def test_a_full_table_loses_whole_voxels_and_counts_their_items(pkg, bm):
    rng = np.random.default_rng(77)
    voxels = np.array([rc.pack3((32768 + 5 * i, 32768 - 3 * i, 32768 + i)) for i in range(40)], np.uint64)
    keys = voxels[rng.integers(0, 40, 400)]
    ops = rng.choice(np.uint8([ec.UPDATE, ec.SET]), 400)
    values = rng.uniform(-1, 1, 400).astype(np.float32)
    rp = pkg.occ_ray_params()
    omap = pkg.OccupancyMap(bm, 4)                    # eight slots
    try:
        with pytest.raises(pkg.StereoBMError) as e:
            omap.edit(d_keys(keys), dev(ops), dev(values), rp)
        assert e.value.code == pkg.ERR_OCC_FULL
        stored, _ = omap.fetch_logodds(allow_overflow=True)
        assert len(stored) == 8 and omap.size() == 8
        kept = np.isin(keys, stored)
        info = omap.last_edit()
        assert info["lost"] == (~kept).sum() and omap.overflow() == info["lost"] and info["created"] == 8 and info["skipped"] == 0
        t = ec.Tree().edit(keys[kept], ops[kept], values[kept])
        same(omap.fetch_logodds(allow_overflow=True), t.leaves(), "the stored voxels' items only")
    finally:
        omap.close()


# ---- 8. modes and the checks that need a map -----------------------------------------------------------------------------------------
def test_mode_rules_and_argument_checks(pkg, bm):
    L = pkg.load_library()
    rp = pkg.occ_ray_params()
    omap = pkg.OccupancyMap(bm, 1 << 12)
    try:
        omap.delete_nodes(np.array([rc.pack3((1, 2, 3))], np.uint64))        # accepted on a fresh map; the mode stays open
        omap.delete_box((0, 0, 0), (65535, 65535, 65535))
        assert omap.size() == 0 and omap.last_edit()["removed"] == 0
        keys, values = d_keys(np.array([rc.pack3((5, 6, 7))] * 4, np.uint64)), dev(np.zeros(4, np.float32))
        m, byref = omap._m, ctypes.byref
        assert L.sbm_occ_edit_device(m, 4, None, None, values.data_ptr(), byref(rp), 1) == NULL
        assert L.sbm_occ_edit_device(m, 4, keys.data_ptr(), None, None, byref(rp), 1) == NULL
        assert L.sbm_occ_edit_device(m, 4, keys.data_ptr(), None, values.data_ptr(), None, 1) == NULL
        bad = pkg.occ_ray_params(clamp_min=0.99)
        assert L.sbm_occ_edit_device(m, 4, keys.data_ptr(), None, values.data_ptr(), byref(bad), 1) == SIZE
        assert L.sbm_occ_edit_device(m, (1 << 30) + 1, keys.data_ptr(), None, values.data_ptr(), byref(rp), 1) == UNSUPPORTED
        assert L.sbm_occ_edit_device(m, 3, keys.data_ptr() + 4, None, values.data_ptr(), byref(rp), 1) == UNSUPPORTED
        assert L.sbm_occ_edit_device(m, 3, keys.data_ptr(), None, values.data_ptr() + 2, byref(rp), 1) == UNSUPPORTED
        assert L.sbm_occ_edit_points_device(m, 1, values.data_ptr() + 2, None, values.data_ptr(), byref(rp), 1) == UNSUPPORTED
        assert L.sbm_occ_delete_device(m, 4, None, 0) == NULL and L.sbm_occ_delete_device(m, 3, keys.data_ptr() + 4, 0) == UNSUPPORTED
        assert L.sbm_occ_delete_device(m, 4, keys.data_ptr(), -1) == UNSUPPORTED
        assert L.sbm_occ_delete_device(m, (1 << 30) + 1, keys.data_ptr(), 0) == UNSUPPORTED
        assert omap.size() == 0
        model = pkg.StereoModel()
        ctypes.memmove(ctypes.byref(model), ctypes.byref(occ.model_from_array(HITS["model"])), ctypes.sizeof(model))
        omap.insert(dev(HITS["scene_disp"][:1]), model, HITS["scene_poses"][:1], 4)      # the mode was open: a hit insert fixes it
        assert omap.size() > 0
    finally:
        omap.close()
    omap = pkg.OccupancyMap(bm, 64)
    try:
        omap.update_nodes(np.zeros(0, np.uint64), np.zeros(0, np.float32))              # no items: the mode is fixed all the same
        with pytest.raises(pkg.StereoBMError) as e:
            omap.insert(dev(HITS["scene_disp"][:1]), model, HITS["scene_poses"][:1], 4)
        assert e.value.code == UNSUPPORTED
        omap.edit(np.array([rc.pack3((5, 6, 7))] * 3, np.uint64), np.uint8([0, 9, 1]), np.float32([1, 1, 2]))      # an unknown op is skipped
        assert omap.last_edit() == dict(items=3, skipped=1, lost=0, created=1, removed=0)
        assert bits(omap.fetch_logodds()[1])[0] == bits(np.float32(2.0))
    finally:
        omap.close()


# ---- 9. an edited map through the calls that read it ---------------------------------------------------------------------------------
def test_tree_files_and_rays_of_an_edited_map(pkg, bm, torch_cuda):
    case = ec.case_of("scene_edits")
    rp = pkg.occ_ray_params(max_range=6.0)
    omap, t = pkg.OccupancyMap(bm, 1 << 13), ec.Tree(case["params"])
    try:
        g = GpuSteps(pkg, omap, rp, True)
        for s in case["steps"][:2]:                    # a scan, then a mixed edit
            ec.apply_step(g, s)
            ec.apply_step(t, s)
        omap.delete_nodes(d_keys(case["steps"][3]["keys"]), 13)
        t.delete(case["steps"][3]["keys"], 13)
        voxels = dict(t.v)
        same(omap.fetch_logodds(), t.leaves(), "edited")
        constants = pkg.occ_ray_logodds(rp)
        want = tc.Tree(voxels)
        tree = omap.tree(pkg.OCC_TREE_LOGODDS)
        info = tree.info()
        assert info["voxels"] == len(voxels) and info["nodes"] == want.size and info["leaves"] == want.num_leaves
        k, d, v = tree.leaves()
        wk, wd, wv = want.leaves()
        assert np.array_equal(k, wk) and np.array_equal(d, wd) and np.array_equal(bits(v), bits(wv))
        assert tree.ot() == otc.write(voxels)
        ml = omap.tree(pkg.OCC_TREE_MAXLIKELIHOOD, rp)
        assert ml.binary().cpu().numpy().tobytes() == tc.Tree(tc.max_likelihood(voxels, tc.LOGODDS_MODE, constants)).binary(constants[3])
        rng = np.random.default_rng(3)
        dirs = rng.normal(size=(128, 3)).astype(np.float32)
        origin = case["steps"][0]["origin"]
        m = qc.Map(voxels, qc.LOGODDS, constants[4], 0.1)
        status, end = m.cast_rays(np.repeat(origin[None], 128, 0), dirs, False, 6.0)
        s, e = omap.cast_rays(origin, dev(dirs), max_range=6.0, occupancy_thres_log=float(constants[4]))
        s, e = s.cpu().numpy(), e.cpu().numpy()
        none = status == qc.RAY_NONE
        assert np.array_equal(s, status) and np.array_equal(bits(e[~none]), bits(np.asarray(end, np.float32)[~none]))
        # a tree built earlier is a snapshot: it answers as built after a further delete
        omap.delete_box((0, 0, 0), (65535, 65535, 65535))
        assert omap.size() == 0 and tree.info()["voxels"] == len(voxels) and np.array_equal(tree.leaves()[0], wk)
    finally:
        omap.close()


# ---- 10. profiling --------------------------------------------------------------------------------------------------------------------
def test_an_edit_is_timed_under_the_names_there_are(pkg):
    eng = pkg.StereoBM.create(64, 21)
    omap = pkg.OccupancyMap(eng, 1 << 12)
    try:
        eng.set_profiling(True)
        rng = np.random.default_rng(5)
        keys = np.array([rc.pack3((32768 + int(a), 32768 + int(b), 32768)) for a, b in rng.integers(-30, 30, (2000, 2))], np.uint64)
        omap.edit(d_keys(keys), dev(rng.choice(np.uint8([0, 1, 2]), 2000)), dev(rng.uniform(-1, 1, 2000).astype(np.float32)))
        prof = omap.profile()
        assert set(prof) == PROFILE_NAMES and prof["occ_rays_mark"] > 0 and prof["occ_rays_apply"] > 0 and prof["occ_insert"] == 0
        omap.delete_box((0, 0, 0), (65535, 32768, 65535))
        prof = omap.profile()
        assert set(prof) == PROFILE_NAMES and prof["occ_rays_apply"] > 0
    finally:
        eng.set_profiling(False)
        omap.close()
        eng.close()


# ---- the C++ adaptor's two loops: the sliding window and the replay of changedKeys -------------------------------------------------------
def test_cpp_call_site(pkg, bm, tmp_path):
    case = ec.case_of("scene_edits")
    scans = [s for s in case["steps"] if s["kind"] == ec.SCAN]
    exe, built = build_callsite(tmp_path, "occupancy_edit_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert built.returncode == 0, built.stderr
    cloud = np.concatenate([np.concatenate([np.float32([len(s["points"])]), s["origin"], s["points"].reshape(-1)]) for s in scans])
    cloud.astype(np.float32).tofile(tmp_path / "cloud.raw")
    half = 25
    r = subprocess.run([str(exe), str(tmp_path / "cloud.raw"), str(len(cloud)), "8192", str(half)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    t, lines = ec.Tree(), []                             # the program's parameters are octomap's defaults, without a range limit
    for s in scans:
        t.insert(s["points"], s["origin"])
        at = rc.key3(s["origin"], 10.0)
        t.delete_box([max(k - half, 0) for k in at], [min(k + half, 65535) for k in at], True)
        lines.append(f"size {len(t.v)} removed {t.last['removed']} mirror {len(t.v)}")
    assert all(0 < int(ln.split()[3]) for ln in lines), "the window removes something after every scan"
    assert r.stdout.splitlines() == lines + [f"marked {qc.CELL_OCCUPIED} then {qc.CELL_UNKNOWN}"], r.stdout
