"""The occupancy map's log-odds mode without a GPU: the Python restatement (tests/occupancy_ray_cases.py) against what the
reference's own octomap answered (tests/golden/occupancy_rays.npz, made by tools/make_occupancy_ray_fixtures.py) -- keys, float
bits, leaf counts after every recorded scan, stream bytes; the host writer sbm_occ_write_binary_logodds against the same
streams; the five log-odds constants; the parameter checks; and sbm_occ_write_binary unchanged on the hit mode's fixture."""
import ctypes
import functools
import hashlib
import math
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_ray_cases as rc  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "occupancy_rays.npz"
FX = dict(np.load(GOLDEN))
NAMES = [str(n) for n in FX["names"]]
REQUIRED = ("axes", "ties", "short", "range", "rangeneg", "bounds", "scene", "clamp", "order_ab", "order_ba", "random", "block", "mixed")
# the constants the reference's build gave for octomap's defaults
DEFAULT_CONSTANTS = ("0x1.b1d106p-1", "-0x1.9f323ep-2", "-0x1.0000eap+1", "0x1.c16974p+1", "0x0p+0")


def params_of(name):
    a = FX[f"{name}_params"]
    return rc.RayParams(*[float(v) for v in a])


def scans_of(name):
    """[(origin, points)] of a case."""
    n = FX[f"{name}_npoints"]
    ends = np.cumsum(n)
    return [(FX[f"{name}_origins"][i], FX[f"{name}_points"][e - k:e]) for i, (k, e) in enumerate(zip(n, ends))]


def recorded(name):
    """[(keys, log-odds)] after every scan of a case, as octomap gave them."""
    n = FX[f"{name}_nleaves"].astype(np.int64)
    ends = np.cumsum(n)
    return [(FX[f"{name}_keys"][e - k:e], FX[f"{name}_logodds"][e - k:e]) for k, e in zip(n, ends)]


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's leaves after every scan, and its census."""
    t = rc.Tree(params_of(name), float(FX["resolution"]))
    census, out = {}, []
    for o, p in scans_of(name):
        t.insert(p, o, census)
        out.append(t.leaves())
    return out, census


def test_fixture_is_the_committed_one_and_holds_every_case():
    want = GOLDEN.with_suffix(".sha256").read_text().split()[0]
    assert hashlib.sha256(GOLDEN.read_bytes()).hexdigest() == want
    assert set(REQUIRED) <= set(NAMES)
    assert GOLDEN.stat().st_size < (1 << 20)
    assert FX["bench_cpu_ms_5"] > 0 and FX["bench_cpu_ms_25"] > 0


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_octomap_after_every_scan(name):
    got, _ = restated(name)
    want = recorded(name)
    assert len(got) == len(want)
    for s, ((gk, gv), (wk, wv)) in enumerate(zip(got, want)):
        assert len(gk) == len(wk), (name, s)
        assert np.array_equal(gk, wk), (name, s)
        assert np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), (name, s)


@pytest.mark.parametrize("name", NAMES)
def test_restated_stream_equals_octomap(name):
    (keys, lo) = restated(name)[0][-1]
    thres = rc.constants(params_of(name))[4]
    data, nodes = rc.write_binary(keys, lo, float(FX["resolution"]), thres)
    assert nodes == int(FX[f"{name}_size"])
    assert data == FX[f"{name}_bt"].tobytes()


def test_constants(pkg):
    for name in NAMES:
        rp = params_of(name)
        want = FX[f"{name}_constants"]
        assert np.array_equal(np.array(rc.constants(rp), np.float32).view(np.uint32), want.view(np.uint32)), name
        got = pkg.occ_ray_logodds(pkg.occ_ray_params(rp.prob_hit, rp.prob_miss, rp.clamp_min, rp.clamp_max, rp.occupancy_thres))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    assert [float(v) for v in pkg.occ_ray_logodds()] == [float.fromhex(h) for h in DEFAULT_CONSTANTS]
    assert [float(v) for v in FX["scene_constants"]] == [float.fromhex(h) for h in DEFAULT_CONSTANTS]


def test_what_the_cases_claim():
    """Each case exercises what it is there for, by the restatement's census and leaves."""
    t = rc.Tree()
    _, census = restated("random")
    assert census[rc.LENGTH] >= 1 and census[rc.KEY] >= 1 and int(FX["random_length_stops"]) == census[rc.LENGTH]
    assert FX["random_npoints"][0] == 1024
    _, census = restated("short")
    assert census[rc.SAME] == 1 and census[rc.KEY] == 1 and census["steps"] == 1
    short = recorded("short")
    assert len(short[0][0]) == 1 and short[0][1][0] == t.hit                       # no free cell, one occupied
    assert len(short[1][0]) == 2 and sorted(short[1][1]) == sorted([F32(t.hit + t.miss), t.hit])   # the origin's cell alone is free
    _, census = restated("bounds")
    assert census[rc.OUT] >= 6
    v = np.concatenate([lo for _, lo in recorded("clamp")])
    assert (v == t.cmin).any() and (v == t.cmax).any()
    ab, ba = recorded("order_ab")[-1], recorded("order_ba")[-1]
    assert np.array_equal(ab[0], ba[0]) and not np.array_equal(ab[1].view(np.uint32), ba[1].view(np.uint32))
    # range: the points at and just inside 25 end their rays; those a float step beyond are cut at 25 and have no end point
    scans = scans_of("range")
    for o, p in scans[5:8]:
        _, ends = rc.scan_sets(p, o, 25.0, 0.1)
        assert (len(ends) == 1) == (rc.norm(rc.sub3(p[0], o)) <= 25.0)
    assert sorted(rc.norm(rc.sub3(p[0], o)) <= 25.0 for o, p in scans[5:8]) == [False, True, True]


def F32(v):
    return np.float32(v)


def test_ray_steps_stay_far_below_the_device_bound():
    longest = 0
    for name in NAMES:
        for o, p in scans_of(name):
            for q in p[:64]:
                ray, _ = rc.ray_keys(o, q, 0.1) if np.isfinite(q).all() else (None, None)
                longest = max(longest, len(ray or []))
    assert 0 < longest < rc.MAX_STEPS // 100


# ---- the host writer ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["scene", "clamp", "block", "mixed", "order_ab", "random"])
def test_writer_writes_octomaps_stream(pkg, tmp_path, name):
    keys, lo = recorded(name)[-1]
    thres = float(FX[f"{name}_constants"][4])
    path = tmp_path / f"{name}.bt"
    order = np.random.default_rng(3).permutation(len(keys))       # any order
    pkg.occ_write_binary_logodds(keys[order], lo[order], path, float(FX["resolution"]), thres)
    assert path.read_bytes() == FX[f"{name}_bt"].tobytes()


def test_writer_block_collapses_and_mixed_does_not(pkg, tmp_path):
    """Eight free siblings become one free leaf; with one of them occupied they stay eight leaves under an inner node."""
    base = np.uint64(32768 + 40)
    keys = np.array([rc.pack3((int(base) + i, int(base) + j, int(base) + k)) for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.uint64)
    free = np.full(8, -0.4, np.float32)
    sizes = {}
    for label, lo in (("block", free), ("mixed", np.where(np.arange(8) == 5, 0.8, free).astype(np.float32))):
        path = tmp_path / f"{label}.bt"
        pkg.occ_write_binary_logodds(keys, lo, path, 0.1, 0.0)
        data = path.read_bytes()
        want, nodes = rc.write_binary(keys, lo, 0.1, 0.0)
        assert data == want
        sizes[label] = nodes
    assert sizes["mixed"] == sizes["block"] + 8      # the inner node stays and has eight leaves below it
    assert sizes["block"] == 16                      # the root, fourteen inner nodes, one free leaf at depth 15


def test_writer_threshold_and_empty(pkg, tmp_path):
    keys = np.array([5, 9], np.uint64)
    path = tmp_path / "t.bt"
    for thres in (-1.0, 0.0, 0.5, 2.0):
        lo = np.array([0.5, -0.5], np.float32)
        pkg.occ_write_binary_logodds(keys, lo, path, 0.1, thres)
        assert path.read_bytes() == rc.write_binary(keys, lo, 0.1, thres)[0], thres
    pkg.occ_write_binary_logodds(keys[:0], np.zeros(0, np.float32), path, 0.1, 0.0)
    assert path.read_bytes() == rc.write_binary([], [], 0.1, 0.0)[0]
    hit_only = tmp_path / "h.bt"
    pkg.occ_write_binary(keys, hit_only, 0.1)
    pkg.occ_write_binary_logodds(keys, np.ones(2, np.float32), path, 0.1, 0.0)
    assert path.read_bytes() == hit_only.read_bytes()        # all occupied: the hit mode's stream


def test_writer_status_codes(pkg, tmp_path):
    L = pkg.load_library()
    pkg.occ_ray_logodds()   # binds the argument types
    k = np.array([5, 9], np.uint64)
    v = np.array([0.5, -0.5], np.float32)
    path = str(tmp_path / "x.bt").encode()
    w = L.sbm_occ_write_binary_logodds
    assert w(k.ctypes.data, v.ctypes.data, 2, 0.1, 0.0, None) == -1
    assert w(None, v.ctypes.data, 2, 0.1, 0.0, path) == -1
    assert w(k.ctypes.data, None, 2, 0.1, 0.0, path) == -1
    assert w(k.ctypes.data, v.ctypes.data, 2, 0.0, 0.0, path) == -2
    assert w(k.ctypes.data, v.ctypes.data, 2, 0.1, math.nan, path) == -2
    assert w(np.array([5, 5], np.uint64).ctypes.data, v.ctypes.data, 2, 0.1, 0.0, path) == -2      # a key given twice
    assert w(np.array([5, 1 << 48], np.uint64).ctypes.data, v.ctypes.data, 2, 0.1, 0.0, path) == -2
    assert w(k.ctypes.data, np.array([0.5, math.nan], np.float32).ctypes.data, 2, 0.1, 0.0, path) == -2
    assert w(k.ctypes.data, v.ctypes.data, 2, 0.1, 0.0, str(tmp_path / "no" / "such" / "x.bt").encode()) == -23
    assert w(k.ctypes.data, v.ctypes.data, 2, 0.1, 0.0, path) == 0


def test_hit_mode_writer_is_unchanged_on_its_fixture(pkg, tmp_path):
    old = dict(np.load(ROOT / "tests" / "golden" / "occupancy_octomap.npz"))
    keep = (old["ok"] == 1) & (old["norm"] <= float(old["range_max"]) ** 2)
    k = old["keys"].astype(np.uint64)
    packed = (k[:, 0] << np.uint64(32)) | (k[:, 1] << np.uint64(16)) | k[:, 2]
    for name, bit in (("all", 1), ("blocks", 2), ("empty", 4)):
        path = tmp_path / f"{name}.bt"
        pkg.occ_write_binary(packed[keep & ((old["group"] & bit) != 0)], path, float(old["resolution"]))
        assert path.read_bytes() == old[f"bt_{name}"].tobytes(), name


# ---- parameters ----------------------------------------------------------------------------------------------------------------
def test_ray_params_layout_and_defaults(pkg):
    p = pkg.OccRayParams()
    pkg.occ_ray_validate(pkg.occ_ray_params())   # binds the argument types
    pkg.load_library().sbm_occ_ray_params_default(p)
    assert (p.prob_hit, p.prob_miss, p.clamp_min, p.clamp_max, p.occupancy_thres, p.max_range) == (0.7, 0.4, 0.1192, 0.971, 0.5, -1.0)
    assert bytes(p) == bytes(pkg.occ_ray_params())
    assert ctypes.sizeof(p) == 48
    d = rc.RayParams()
    assert (d.prob_hit, d.prob_miss, d.clamp_min, d.clamp_max, d.occupancy_thres, d.max_range) == (0.7, 0.4, 0.1192, 0.971, 0.5, -1.0)
    pkg.load_library().sbm_occ_ray_params_default(None)   # tolerated


@pytest.mark.parametrize("change,code", [
    ({}, 0), ({"max_range": 0.0}, 0), ({"max_range": 25.0}, 0), ({"max_range": math.inf}, 0), ({"max_range": -math.inf}, 0),
    ({"max_range": math.nan}, -2),
    ({"prob_hit": 0.5}, 0), ({"prob_hit": 0.49}, -2), ({"prob_hit": 1.0}, -2), ({"prob_hit": math.nan}, -2), ({"prob_hit": 1.5}, -2),
    ({"prob_miss": 0.5}, 0), ({"prob_miss": 0.51}, -2), ({"prob_miss": 0.0}, -2), ({"prob_miss": math.nan}, -2), ({"prob_miss": -0.1}, -2),
    ({"clamp_min": 0.0}, -2), ({"clamp_min": 0.971}, -2), ({"clamp_min": 0.98}, -2), ({"clamp_min": math.nan}, -2),
    ({"clamp_max": 1.0}, -2), ({"clamp_max": 0.1}, -2), ({"clamp_max": math.nan}, -2), ({"clamp_max": 0.6}, 0),
    ({"occupancy_thres": 0.0}, -2), ({"occupancy_thres": 1.0}, -2), ({"occupancy_thres": math.nan}, -2), ({"occupancy_thres": 0.9}, 0),
])
def test_ray_params_status_codes(pkg, change, code):
    p = pkg.occ_ray_params()
    for k, v in change.items():
        setattr(p, k, v)
    assert pkg.occ_ray_validate(p) == code
    out = np.zeros(5, np.float32)
    assert pkg.load_library().sbm_occ_ray_logodds(ctypes.byref(p), out.ctypes.data) == code


def test_null_arguments(pkg):
    L = pkg.load_library()
    p = pkg.occ_ray_params()
    pkg.occ_ray_validate(p)
    m = pkg.StereoModel()
    n = ctypes.c_size_t()
    o = np.zeros(3, np.float32)
    assert L.sbm_occ_ray_params_validate(None) == -1
    assert L.sbm_occ_ray_logodds(ctypes.byref(p), None) == -1
    assert L.sbm_occ_insert_cloud_device(None, 0, None, o.ctypes.data, ctypes.byref(p), 1) == -1
    assert L.sbm_occ_insert_cloud(None, 0, None, o.ctypes.data, ctypes.byref(p)) == -1
    assert L.sbm_occ_insert_rays_device(None, 1, None, 4, 4, 1, ctypes.byref(m), None, ctypes.byref(p), 1) == -1
    assert L.sbm_occ_insert_rays(None, 1, None, 4, 4, 1, ctypes.byref(m), None, ctypes.byref(p)) == -1
    assert L.sbm_occ_fetch_logodds_device(None, None, None, 0, ctypes.byref(n)) == -1
    assert L.sbm_occ_fetch_logodds(None, None, None, 0, ctypes.byref(n)) == -1
