"""The GPU occupancy map's colours (u96-slam_amd/csrc/sbm_occ_color.hip: FIND, the map's radix sort, APPLY, the coloured search
and fetch, the tree's bottom-up colour pass, the ColorOcTree stream written by rank and loaded by expansion), held to what the
reference's own octomap (ColorOcTree) recorded in tests/golden/occupancy_color.npz after every step, and where that holds no
record to the restatement tests/occupancy_color_cases.py. Every comparison is exact: integers and bytes with array_equal, floats by
their uint32 views."""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_color_cases as cc  # noqa: E402
import occupancy_ot_cases as otc  # noqa: E402
import occupancy_ray_cases as rc  # noqa: E402
import occupancy_tree_cases as tc  # noqa: E402
from gpu_support import bm, build_callsite, dev, torch_cuda  # noqa: E402,F401

pytestmark = pytest.mark.gpu
NULL, SIZE, UNSUPPORTED, OCC_FULL = -1, -2, -23, -25
PROFILE_NAMES = {"occ_insert", "occ_fetch", "occ_rays_mark", "occ_rays_apply", "occ_search", "occ_cast", "occ_load"}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def same_voxels(got, want, what):
    assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]), (what, "keys")
    assert np.array_equal(bits(got[1]), bits(want[1])), (what, "values")
    assert np.array_equal(np.asarray(got[2], np.uint32), np.asarray(want[2], np.uint32)), (what, "colours")


def ray_params(pkg, case):
    return pkg.occ_ray_params(*[getattr(case["params"], k) for k in ("prob_hit", "prob_miss", "clamp_min", "clamp_max", "occupancy_thres", "max_range")])


def d_keys(keys):
    return dev(np.ascontiguousarray(keys, np.uint64).view(np.int64))


def d_words(words):
    return dev(np.ascontiguousarray(words, np.uint32).view(np.int32))


def color_step(omap, s, device):
    call = omap.average_colors if s["op"] == cc.AVERAGE else omap.set_colors
    items = np.ascontiguousarray(s["points"], np.float32) if s["form"] else np.ascontiguousarray(s["keys"], np.uint64)
    if device:
        call(dev(items) if s["form"] else d_keys(items), d_words(s["words"]))
    else:
        call(items, s["words"])


def check_snapshot(pkg, bm, omap, rp, theirs, what, device):
    """The tree over the map as it is: the leaf lists with colours, the stream, and what a second map holds after loading it"""
    lists, data, vox = theirs
    tree = omap.tree(params=rp)
    other = pkg.OccupancyMap(bm, 1 << 13)
    try:
        for d, want in zip(cc.DEPTHS, lists):
            got = tree.leaves_colors_device(d) if device else tree.leaves_colors(d)
            got = [g.cpu().numpy() for g in got] if device else list(got)
            assert np.array_equal(got[0].view(np.uint64), want[0]) and np.array_equal(got[1], want[1]), (what, d, "entries")
            assert np.array_equal(bits(got[2]), bits(want[2])) and np.array_equal(got[3].view(np.uint32), want[3]), (what, d, "values and colours")
        assert tree.color_ot() == data, (what, "stream")
        head = data.index(b"data\n") + 5
        assert tree.color_ot_body().cpu().numpy().tobytes() == data[head:], (what, "body on the device")
        other.load_color_ot(data)
        same_voxels(other.fetch_colors(), vox, (what, "loaded"))
        again = other.tree(params=rp)
        try:
            assert again.color_ot() == data, (what, "load, write again")
        finally:
            again.close()
    finally:
        tree.close()
        other.close()
    return data


def run_case(pkg, bm, name, device, capacity, grow=False):
    case, theirs, mine = cc.case_of(name), cc.recorded(name), restated(name)
    rp = ray_params(pkg, case)
    omap = pkg.OccupancyMap(bm, capacity, grow=grow)
    try:
        for i, s in enumerate(case["steps"]):
            what = (name, i)
            if s["kind"] == cc.SCAN:
                pts = np.ascontiguousarray(s["points"], np.float32)
                omap.insert_cloud(dev(pts) if device else pts, s["origin"], rp)
            elif s["kind"] == cc.COLOR:
                color_step(omap, s, device)
                info = omap.last_colors()
                assert info["found"] == theirs[i][3] == mine[i][3] and info == counts(name)[i], (what, info, counts(name)[i])
            elif s["kind"] == cc.SET_VALUES:
                omap.set_node_values(d_keys(s["keys"]) if device else s["keys"], dev(s["values"]) if device else s["values"], rp)
            elif s["kind"] == cc.EDIT:
                omap.edit(d_keys(s["keys"]) if device else s["keys"], dev(s["ops"]) if device else s["ops"], dev(s["values"]) if device else s["values"], rp)
            elif s["kind"] == cc.SNAPSHOT:
                assert cc.same(mine[i], theirs[i]), (what, "the restatement")
                check_snapshot(pkg, bm, omap, rp, theirs[i], what, device)
                continue
            elif s["kind"] == cc.RESUME:
                tree = omap.tree(params=rp)
                data = tree.color_ot()
                tree.close()
                omap.load_color_ot(data)
            got = omap.fetch_colors()
            assert omap.overflow() == 0, what
            same_voxels(got, mine[i], what + ("restatement",))
            same_voxels(got, theirs[i], what + ("octomap",))
        return omap
    except BaseException:
        omap.close()
        raise


_RESTATED = {}


def restated(name):
    if name not in _RESTATED:
        _RESTATED[name] = cc.run_case(cc.case_of(name))
    return _RESTATED[name]


_COUNTS = {}


def counts(name):
    if name not in _COUNTS:
        _COUNTS[name] = cc.run_counts(cc.case_of(name))
    return _COUNTS[name]


# ---- 1. every recorded case, device and host forms ---------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("name", cc.NAMES)
def test_every_recorded_case_equals_octomap_after_every_step(pkg, bm, name, device):
    run_case(pkg, bm, name, device, 1 << 13).close()


def test_the_fixture_holds_the_cases_the_issue_names():
    assert cc.NAMES == ["scans", "run300", "blocks", "reborn", "resume"]
    keys = cc.case_of("run300")["steps"][1]["keys"]
    assert (keys == keys[0]).sum() == 300, "a run that crosses a wavefront and a workgroup of items"


# ---- 2. a map created for one voxel with growth on ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.NAMES)
def test_a_growing_map_carries_the_colours(pkg, bm, name):
    omap = run_case(pkg, bm, name, True, 1, grow=True)
    try:
        g = omap.growth()
        assert g["grown"] > 0 and g["capacity"] > 1
        before = omap.fetch_colors()
        omap.reserve(4 * g["capacity"])                  # one more move, with nothing else going on
        same_voxels(omap.fetch_colors(), before, (name, "reserve"))
    finally:
        omap.close()


# ---- 3. deletes keep the survivors' colours; a voxel created again is white --------------------------------------------------------
def test_deletes_keep_the_survivors_colours_and_a_voxel_created_again_is_white(pkg, bm):
    case = cc.case_of("blocks")
    rp = ray_params(pkg, case)
    m = cc.Map(case["params"])
    omap = pkg.OccupancyMap(bm, 1 << 10)
    try:
        for s in case["steps"][:2]:
            cc.apply_step(m, s)
        omap.set_node_values(case["steps"][0]["keys"], case["steps"][0]["values"], rp)
        color_step(omap, case["steps"][1], True)
        same_voxels(omap.fetch_colors(), m.colored(), "before")
        painted = [int(k) for k in case["steps"][1]["keys"]]
        gone = painted[3:40:4]
        omap.delete_nodes(np.array(gone, np.uint64))
        m.delete(gone)
        same_voxels(omap.fetch_colors(), m.colored(), "deleteNode")
        lo, hi = (32768 + 128, 32768 + 64, 32768 + 32), (32768 + 129, 32768 + 67, 32768 + 35)
        omap.delete_box(lo, hi)
        m.delete_box(lo, hi)
        assert omap.last_edit()["removed"] > 0
        same_voxels(omap.fetch_colors(), m.colored(), "delete_box")
        assert (m.colored()[2] != cc.WHITE).sum() > 20, "survivors with colours"
        back = np.array(gone[:3], np.uint64)
        omap.set_node_values(back, np.float32([1.0, 1.0, 1.0]), rp)
        for k in back:
            m.set_node_value(int(k), 1.0)
        got = omap.fetch_colors()
        same_voxels(got, m.colored(), "created again")
        assert (got[2][np.isin(got[0], back)] == cc.WHITE).all()
        pts = np.float32([[((int(k) >> s & 0xFFFF) - 32768 + 0.5) * 0.1 for s in (32, 16, 0)] for k in back])
        st, val, col = omap.search_colors(pts)
        assert (st == tc.CELL_OCCUPIED).all() and (col == cc.WHITE).all() and np.array_equal(val, bits(np.float32([1.0] * 3)))
        omap.reset()                                      # every voxel white, the words stay allocated
        omap.set_node_values(np.array(painted[:5], np.uint64), np.float32([1.0] * 5), rp)
        assert (omap.fetch_colors()[2] == cc.WHITE).all()
    finally:
        omap.close()


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_a_voxel_deleted_and_created_again_inside_one_edit_batch_is_white(pkg, bm, device):
    """DELETE then SET / UPDATE of a coloured voxel in ONE edit call ends present, so no move drops the slot: APPLY whitens it."""
    import occupancy_edit_cases as ec
    K = lambda i: rc.pack3((32768 + i, 32768 - i, 32768 + 2 * i))                        # noqa: E731
    keys = [K(i) for i in range(1, 9)]
    m = cc.Map()
    rp = pkg.occ_ray_params()
    omap = pkg.OccupancyMap(bm, 1 << 8)
    try:
        values = np.float32([0.5 + 0.1 * i for i in range(8)])
        omap.set_node_values(d_keys(keys) if device else np.array(keys, np.uint64), dev(values) if device else values, rp)
        m.edit(keys, [ec.SET] * 8, values)
        words = np.array([cc.word(10 * i, 20 + i, 200 - i) for i in range(1, 9)], np.uint32)
        omap.set_colors(np.array(keys, np.uint64), words)
        m.color(keys, words, cc.SET)
        a, b, c, d, e, f = keys[:6]
        items = [(a, ec.DELETE, 0.0), (a, ec.SET, 1.25),                                  # delete, set: present, white
                 (b, ec.DELETE, 0.0), (b, ec.UPDATE, 0.75),                               # delete, update: created from 0, white
                 (c, ec.SET, 2.0), (c, ec.DELETE, 0.0), (c, ec.SET, -1.0),                # set, delete, set
                 (d, ec.SET, 0.25), (d, ec.UPDATE, 0.5),                                  # no delete: keeps its colour
                 (e, ec.DELETE, 0.0),                                                     # ends absent: the move drops it
                 (f, ec.UPDATE, 0.1), (a, ec.UPDATE, 0.5)]                                # a again, far from its first items
        ik, ops, vals = np.array([i[0] for i in items], np.uint64), np.array([i[1] for i in items], np.uint8), np.float32([i[2] for i in items])
        omap.edit(d_keys(ik) if device else ik, dev(ops) if device else ops, dev(vals) if device else vals, rp)
        m.edit(ik, ops, vals)
        got = omap.fetch_colors()
        same_voxels(got, m.colored(), "one batch")
        col = dict(zip(map(int, got[0]), map(int, got[2])))
        assert col[a] == col[b] == col[c] == cc.WHITE and col[d] == int(words[3]) and e not in col and col[f] == int(words[5]) and col[keys[7]] == int(words[7])
        omap.average_colors(np.array([a, e], np.uint64), np.array([0x111111, 0x222222], np.uint32))
        m.color([a, e], [0x111111, 0x222222], cc.AVERAGE)
        assert omap.last_colors() == m.last_color == dict(items=2, found=1, unknown=1, skipped=0)
        same_voxels(omap.fetch_colors(), m.colored(), "from white the colour itself")
    finally:
        omap.close()


# ---- 4. search with colours, both forms, against the restatement -------------------------------------------------------------------
def test_search_colors_equals_the_restatement(pkg, bm):
    case = cc.case_of("scans")
    rp = ray_params(pkg, case)
    m = cc.Map(case["params"])
    omap = pkg.OccupancyMap(bm, 1 << 13)
    try:
        for s in case["steps"][:2]:
            cc.apply_step(m, s)
        omap.insert_cloud(np.ascontiguousarray(case["steps"][0]["points"]), case["steps"][0]["origin"], rp)
        color_step(omap, case["steps"][1], False)
        pts = np.ascontiguousarray(case["steps"][1]["points"][600:760])          # known voxels, points outside, unknown voxels
        want = m.search_colors(pts, m.thres)
        assert {tc.CELL_OUT, tc.CELL_UNKNOWN, tc.CELL_OCCUPIED} <= set(want[0].tolist()) and (want[2] != cc.WHITE).sum() > 50
        host = omap.search_colors(pts, float(m.thres))
        device = [t.cpu().numpy() for t in omap.search_colors(dev(pts), float(m.thres))]
        for got in (host, device):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1]) and np.array_equal(got[2].view(np.uint32), want[2])
        k, lo, col = (t.cpu().numpy() for t in omap.fetch_colors_device())
        same_voxels((k.view(np.uint64), lo, col.view(np.uint32)), m.colored(), "fetch on the device")
    finally:
        omap.close()


# ---- 5. the C++ call site ---------------------------------------------------------------------------------------------------------
def test_the_cpp_call_site_equals_the_restatement(pkg, bm, tmp_path):
    exe, built = build_callsite(tmp_path, "occupancy_color_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert built.returncode == 0, built.stderr
    s = cc.case_of("resume")["steps"][0]
    pts, words = np.ascontiguousarray(s["points"], np.float32), cc.case_of("resume")["steps"][2]["words"]
    np.concatenate([np.float32([len(pts)]), s["origin"], pts.reshape(-1)]).astype(np.float32).tofile(tmp_path / "cloud.raw")
    np.ascontiguousarray(words, np.uint32).tofile(tmp_path / "colors.raw")
    probes = 6
    r = subprocess.run([str(exe), str(tmp_path / "cloud.raw"), str(4 + 3 * len(pts)), str(tmp_path / "colors.raw"), "8192", str(tmp_path / "out.ot"),
                        str(probes)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = cc.Map()                                          # the program's parameters are octomap's defaults, without a range limit
    m.insert(pts, s["origin"])
    m.color_points(pts, words, cc.AVERAGE)
    lines = ["batch found {found} unknown {unknown} skipped {skipped}".format(**m.last_color)]
    m.color_points(pts[:1], [cc.word(1, 2, 3)], cc.SET)
    a = m.last_color["found"]
    m.color_points(np.float32([[30.05, 30.05, 30.05]]), [cc.word(9, 9, 9)], cc.AVERAGE)
    b = m.last_color["found"]
    m.color([rc.pack3(rc.key3(pts[1], 10.0))], [cc.word(10, 20, 30)], cc.AVERAGE)
    lines.append(f"single {a} {b} {m.last_color['found']}")
    data = m.tree().stream()
    assert (tmp_path / "out.ot").read_bytes() == data
    back = cc.Map().load(cc.parse(data, 0.1).leaves)
    s0, s1 = m.search_colors(pts[:probes], m.thres), back.search_colors(pts[:probes], m.thres)
    for i in range(probes):
        lines.append(f"probe {s0[0][i]} {s0[1][i]:08x} {s0[2][i]:06x} back {s1[0][i]} {s1[1][i]:08x} {s1[2][i]:06x}")
    leaves = m.tree().leaves_colors(12)
    lines.append(f"leaves {len(leaves[0])} {int(np.bitwise_xor.reduce(leaves[3])):06x}")
    assert r.stdout.splitlines() == lines, r.stdout


@pytest.mark.parametrize("name", cc.NAMES)
def test_every_recorded_case_through_the_cpp_call_site(pkg, bm, name, tmp_path):
    """The program's replay mode: after every step begin_leafs(16) with colours against the restatement's tree over its map, the
    snapshots' four listings and the file writeColor wrote against octomap's record."""
    exe, built = build_callsite(tmp_path, "occupancy_color_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert built.returncode == 0, built.stderr
    case, theirs = cc.case_of(name), cc.recorded(name)
    d = rc.RayParams()
    assert all(getattr(case["params"], k) == getattr(d, k) for k in ("prob_hit", "prob_miss", "clamp_min", "clamp_max", "occupancy_thres"))
    with open(tmp_path / "steps.bin", "wb") as f:
        f.write(np.float64(case["params"].max_range).tobytes() + np.int32(len(case["steps"])).tobytes())
        for s in case["steps"]:
            f.write(np.int32([s["kind"], len(s["keys"]), s["form"], s["op"]]).tobytes() + np.float32(s["origin"]).tobytes())
            f.write(np.ascontiguousarray(s["keys"], np.uint64).tobytes() + np.ascontiguousarray(s["points"], np.float32).tobytes())
            f.write(np.ascontiguousarray(s["words"], np.uint32).tobytes() + np.ascontiguousarray(s["values"], np.float32).tobytes())
            f.write(np.ascontiguousarray(s["ops"], np.uint8).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "steps.bin"), "8192", str(tmp_path / "answers.bin"), str(tmp_path / "stream")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw, at = (tmp_path / "answers.bin").read_bytes(), [0]

    def take(dtype, n=1):
        a = np.frombuffer(raw, dtype, n, at[0])
        at[0] += a.nbytes
        return a

    def listing():
        n = int(take("<u4")[0])
        return take("<u8", n), take("<i4", n), take("<f4", n), take("<u4", n)

    def same_listing(got, want, what):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (what, "entries")
        assert np.array_equal(bits(got[2]), bits(want[2])) and np.array_equal(got[3], want[3]), (what, "values and colours")

    m = cc.Map(case["params"])
    for i, s in enumerate(case["steps"]):
        cc.apply_step(m, s)
        if s["kind"] == cc.SNAPSHOT:
            for depth, want in zip(cc.DEPTHS, theirs[i][0]):
                same_listing(listing(), want, (name, i, depth))
            assert (tmp_path / f"stream{i}").read_bytes() == theirs[i][1], (name, i, "stream")
            continue
        found = int(take("<u8")[0])
        assert found == theirs[i][3], (name, i, "found")
        same_listing(listing(), m.tree().leaves_colors(16), (name, i))
    assert at[0] == len(raw)


# ---- 6. refusals: the map stays as it was ------------------------------------------------------------------------------------------
def test_refusals_leave_the_map_as_it_was(pkg, bm):
    case = cc.case_of("blocks")
    rp = ray_params(pkg, case)
    good = cc.recorded("blocks")[2][1]
    head = good.index(b"data\n") + 5
    size = (len(good) - head) // 8
    plain = otc.write({int(k): v for k, v in zip(*cc.recorded("blocks")[0][:2])}, 0.1)
    bad = {
        "a plain OcTree stream": (plain, UNSUPPORTED),
        "cut in a record": (good[:-3], SIZE),
        "cut between records": (good[:-8], SIZE),
        "cut in the header": (good[:head - 9], SIZE),
        "size plus one": (good.replace(b"size %d\n" % size, b"size %d\n" % (size + 1)) + bytes(8), SIZE),
        "size minus one": (good.replace(b"size %d\n" % size, b"size %d\n" % (size - 1)), SIZE),
        "a root that is one leaf: 2^48 voxels": (good[:head].replace(b"size %d\n" % size, b"size 1\n") + bytes([0, 0, 0, 63, 1, 2, 3, 0]), OCC_FULL),
        "a .bt first line": (good.replace(b"# Octomap OcTree file", b"# Octomap OcTree binary file"), UNSUPPORTED),
    }
    omap = pkg.OccupancyMap(bm, 1 << 10)
    hits = pkg.OccupancyMap(bm, 1 << 10)
    try:
        omap.set_node_values(case["steps"][0]["keys"], case["steps"][0]["values"], rp)
        color_step(omap, case["steps"][1], False)
        before = omap.fetch_colors()
        for what, (data, status) in bad.items():
            with pytest.raises(pkg.StereoBMError) as e:
                omap.load_color_ot(data)
            assert e.value.code == status, (what, e.value.code)
            same_voxels(omap.fetch_colors(), before, what)
        with pytest.raises(pkg.StereoBMError) as e:       # the plain loader keeps refusing the colour stream
            omap.load_ot(good)
        assert e.value.code == UNSUPPORTED
        same_voxels(omap.fetch_colors(), before, "load_ot")
        for op in (2, -1):
            assert pkg.load_library().sbm_occ_color_keys(omap._m, 0, None, None, op) == UNSUPPORTED
        # hit mode
        fx = dict(np.load(ROOT / "tests" / "golden" / "occupancy_octomap.npz"))
        hits.insert(dev(fx["scene_disp"][:1]), _model(pkg, fx), fx["scene_poses"][:1], 4)
        assert hits.size() > 0
        for call in (lambda: hits.set_colors(np.array([1], np.uint64), np.array([5], np.uint32)), lambda: hits.average_colors(np.zeros((1, 3), np.float32), [5]),
                     lambda: hits.search_colors(np.zeros((1, 3), np.float32)), lambda: hits.fetch_colors()):
            with pytest.raises(pkg.StereoBMError) as e:
                call()
            assert e.value.code == UNSUPPORTED
    finally:
        omap.close()
        hits.close()


def _model(pkg, fx):
    import ctypes

    import occupancy_ref as occ
    ref = occ.model_from_array(fx["model"])
    m = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(m), ctypes.byref(ref), ctypes.sizeof(m))
    return m


# ---- 7. a map without colours is what it was ---------------------------------------------------------------------------------------
def test_a_colourless_map_answers_white_and_launches_what_it_launched(pkg, bm):
    case = cc.case_of("scans")
    rp = ray_params(pkg, case)
    pts = np.ascontiguousarray(case["steps"][0]["points"])
    omap = pkg.OccupancyMap(bm, 1 << 13)
    bm.set_profiling(True)
    try:
        omap.insert_cloud(pts, case["steps"][0]["origin"], rp)
        prof = omap.profile()
        assert set(prof) == PROFILE_NAMES and prof["occ_rays_mark"] > 0 and prof["occ_rays_apply"] > 0, prof
        st, val, col = omap.search_colors(pts[:64])
        plain_st, plain_val = omap.search(pts[:64])
        assert np.array_equal(st, plain_st) and np.array_equal(val, plain_val) and (col == cc.WHITE).all()
        k, lo, c = omap.fetch_colors()
        pk, plo = omap.fetch_logodds()
        assert np.array_equal(k, pk) and np.array_equal(bits(lo), bits(plo)) and (c == cc.WHITE).all()
        tree = omap.tree(params=rp)
        try:
            got = tree.leaves_colors(12)
            want = tree.leaves(12)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (got[3] == cc.WHITE).all()
            assert pkg.occ_color_ot_info(tree.color_ot())["nodes"] == tree.info()["nodes"]
        finally:
            tree.close()
        assert set(omap.profile()) == PROFILE_NAMES
    finally:
        bm.set_profiling(False)
        omap.close()
