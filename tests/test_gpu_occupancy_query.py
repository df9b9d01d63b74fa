"""The GPU occupancy map's queries (u96-slam_amd/csrc/sbm_occ_query.hip: occ_search_kernel, occ_cast_rays_kernel,
occ_cast_view_kernel) against what the reference's own octomap answered for search and castRay
(tests/golden/occupancy_query.npz) and, for shapes the fixture does not hold, against the transcription
tests/occupancy_query_cases.py, which tests/test_occupancy_query_restatement.py pins to the same fixture. Every map is built
through the existing inserts and its fetched keys must equal the recorded list. Everything is compared for exact equality:
states, statuses and the bits of the floats."""
import ctypes
import functools
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import occupancy_query_cases as qc  # noqa: E402
import occupancy_ref as occ  # noqa: E402
from gpu_support import bm, build_callsite, dev, torch_cuda  # noqa: E402,F401

pytestmark = pytest.mark.gpu
FX = dict(np.load(ROOT / "tests" / "golden" / "occupancy_query.npz"))
TREES = [str(t) for t in FX["trees"]]
RES = float(FX["resolution"])
NULL, SIZE, UNSUPPORTED = -1, -2, -23
NAN_BITS = 0x7FC00000


def sets_of(tree, kind):
    return [str(s) for s in FX[f"{tree}_sets"] if f"{tree}_{s}_{kind}" in FX]


def is_hits(tree):
    return bool(int(FX[f"{tree}_hits"]))


def scans_of(tree):
    n = FX[f"{tree}_npoints"]
    ends = np.cumsum(n)
    return [(FX[f"{tree}_origins"][i], float(FX[f"{tree}_scan_range"][i]), FX[f"{tree}_points"][e - k:e])
            for i, (k, e) in enumerate(zip(n, ends))]


def gpu_model(pkg, m):
    g = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(g), ctypes.byref(m), ctypes.sizeof(g))
    return g


def scene_model():
    return occ.model_from_array(FX["scene_model"])


def build(pkg, bm, tree, capacity=1 << 14):
    """The tree through the existing inserts -> (map, threshold); its fetched keys equal the recorded list."""
    omap = pkg.OccupancyMap(bm, capacity)
    if is_hits(tree):
        omap.insert(dev(FX["scene_disp"]), gpu_model(pkg, scene_model()), FX["scene_poses"], int(FX["scene_scale"]))
        keys, counts = omap.keys()
        assert np.array_equal(keys, FX[f"{tree}_keys"]) and np.array_equal(counts, FX[f"{tree}_counts"])
        return omap, 0.0
    probs = [float(v) for v in FX[f"{tree}_params"]]
    for i, (o, max_range, p) in enumerate(scans_of(tree)):
        omap.insert_cloud(dev(p) if i % 2 == 0 else p, o, pkg.occ_ray_params(*probs, max_range=max_range))
    keys, lo = omap.fetch_logodds()
    assert np.array_equal(keys, FX[f"{tree}_keys"]) and np.array_equal(lo.view(np.uint32), FX[f"{tree}_logodds"].view(np.uint32))
    thres = float(pkg.occ_ray_logodds(pkg.occ_ray_params(*probs))[4])
    assert np.float32(thres) == FX[f"{tree}_constants"][4]
    return omap, thres


@functools.lru_cache(maxsize=None)
def restated(tree):
    """The transcription's map of a recorded tree, built once."""
    if is_hits(tree):
        return qc.Map(dict(zip((int(k) for k in FX[f"{tree}_keys"]), (int(c) for c in FX[f"{tree}_counts"]))), qc.HITS, 0.0, RES)
    return qc.Map(dict(zip((int(k) for k in FX[f"{tree}_keys"]), FX[f"{tree}_logodds"])), qc.LOGODDS, FX[f"{tree}_constants"][4], RES)


def same_rays(got, status, end, what):
    s, e = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in got)
    assert np.array_equal(s.reshape(-1), status), (what, "status", np.flatnonzero(s.reshape(-1) != status)[:8])
    e, none = e.reshape(-1, 3), status == qc.RAY_NONE
    assert np.array_equal(e[~none].view(np.uint32), np.asarray(end, np.float32)[~none].view(np.uint32)), (what, "end")
    assert np.isnan(e[none]).all(), (what, "end of a ray that is none")


def groups(ignore, max_range):
    """Index lists of equal (ignore_unknown, max_range): one call each."""
    out = {}
    for i, k in enumerate(zip(ignore.tolist(), max_range.tolist())):
        out.setdefault(k, []).append(i)
    return out.items()


@pytest.mark.parametrize("tree", TREES)
def test_every_fixture_case_device_and_host(pkg, bm, tree):
    omap, thres = build(pkg, bm, tree)
    try:
        for s in sets_of(tree, "rays"):
            tag = f"{tree}_{s}"
            rays, status, end = FX[f"{tag}_rays"], FX[f"{tag}_status"], FX[f"{tag}_end"]
            assert np.array_equal(status == qc.RAY_HIT, FX[f"{tag}_ret"].astype(bool))          # octomap's return value
            for (ignore, max_range), idx in groups(FX[f"{tag}_ignore"], FX[f"{tag}_max_range"]):
                q = pkg.occ_query_params(max_range, thres, ignore)
                o, d = np.ascontiguousarray(rays[idx, :3]), np.ascontiguousarray(rays[idx, 3:])
                same_rays(omap.cast_rays(dev(o), dev(d), q), status[idx], end[idx], (tag, "device", ignore, max_range))
                same_rays(omap.cast_rays(o, d, q), status[idx], end[idx], (tag, "host", ignore, max_range))
                if len({tuple(r) for r in o.view(np.uint32).tolist()}) == 1:                    # one origin for all: the shared form
                    same_rays(omap.cast_rays(o[0], dev(d), q), status[idx], end[idx], (tag, "device, one origin"))
                    same_rays(omap.cast_rays(o[0], d, q), status[idx], end[idx], (tag, "host, one origin"))
        for s in sets_of(tree, "state"):
            tag = f"{tree}_{s}"
            pts, state, value = FX[f"{tag}_points"], FX[f"{tag}_state"], FX[f"{tag}_value"]
            for got in (omap.search(dev(pts), thres), omap.search(pts, thres)):
                st, v = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in got)
                assert np.array_equal(st, state), tag
                assert np.array_equal(v.view(np.uint32), value.view(np.uint32)), tag
            if not is_hits(tree):
                found = FX[f"{tag}_found"].astype(bool)
                assert (value.view(np.uint32)[~found] == NAN_BITS).all()
        assert omap.overflow() == 0
    finally:
        omap.close()


@pytest.mark.parametrize("tree", ["scene", "scene_hits"])
def test_cast_view_equals_cast_rays_on_the_rays_of_the_header(pkg, bm, tree):
    m = scene_model()
    omap, thres = build(pkg, bm, tree)
    try:
        for pose, (w, h, scale), q in ((FX["scene_poses"][0], (40, 30, 4), pkg.occ_query_params(6.0, thres, True)),
                                       (FX["scene_poses"][1], (37, 19, 5), pkg.occ_query_params(-1.0, thres, False)),
                                       (FX["scene_poses"][2], (9, 3, 16), pkg.occ_query_params(2.5, thres, True))):
            o, d = qc.view_rays(w, h, scale, m, pose)
            want = omap.cast_rays(dev(o), dev(d), q)
            got = omap.cast_view(w, h, gpu_model(pkg, m), pose, scale, q)
            assert tuple(got[0].shape) == (h, w) and tuple(got[1].shape) == (h, w, 3)
            assert np.array_equal(got[0].cpu().numpy().reshape(-1), want[0].cpu().numpy())
            assert np.array_equal(got[1].cpu().numpy().reshape(-1, 3).view(np.uint32), want[1].cpu().numpy().view(np.uint32))
        tag = f"{tree}_view"                                     # the first view is the fixture's: octomap's answers
        got = omap.cast_view(40, 30, gpu_model(pkg, m), FX["scene_poses"][0], 4, max_range=6.0, occupancy_thres_log=thres,
                             ignore_unknown=True)
        same_rays(got, FX[f"{tag}_status"], FX[f"{tag}_end"], tag)
        plain = pkg.StereoModel()                                # without a local transform
        ctypes.memmove(ctypes.byref(plain), ctypes.byref(gpu_model(pkg, m)), ctypes.sizeof(plain))
        plain.has_local = 0
        ref = occ.model_from_array(FX["scene_model"])
        ref.has_local = 0
        o, d = qc.view_rays(13, 11, 8, ref, FX["scene_poses"][1])
        st, e = restated(tree).cast_rays(o, d, True, 6.0)
        same_rays(omap.cast_view(13, 11, plain, FX["scene_poses"][1], 8, max_range=6.0, occupancy_thres_log=thres, ignore_unknown=True),
                  st, e, "no local transform")
    finally:
        omap.close()


def test_an_empty_and_a_reset_map_answer_unknown(pkg, bm):
    rays, pts = FX["box_axes_rays"], FX["box_search_points"]
    out = np.isnan(pts).any(axis=1) | np.isinf(pts).any(axis=1) | (FX["box_search_state"] == qc.CELL_OUT)
    omap = pkg.OccupancyMap(bm, 1 << 14)
    try:
        for again in (False, True):
            st, v = omap.search(dev(pts))
            assert np.array_equal(st.cpu().numpy(), np.where(out, qc.CELL_OUT, qc.CELL_UNKNOWN)) and not v.cpu().numpy().any()
            s, e = omap.cast_rays(dev(rays[:, :3]), dev(rays[:, 3:]))
            want = qc.Map({}, qc.NONE).cast_rays(rays[:, :3], rays[:, 3:])
            assert (want[0] == qc.RAY_UNKNOWN).all()
            same_rays((s, e), *want, "empty")
            s, e = omap.cast_rays(rays[:1, :3], rays[:1, 3:], ignore_unknown=True, max_range=1.5)     # walks unknown space to the range
            want = qc.Map({}, qc.NONE).cast_rays(rays[:1, :3], rays[:1, 3:], True, 1.5)
            assert want[0][0] == qc.RAY_RANGE
            same_rays((s, e), *want, "empty, ignore")
            s, e = omap.cast_rays(dev(rays[:0, :3]), dev(rays[:0, 3:]))                               # n == 0 launches nothing
            assert tuple(s.shape) == (0,) and tuple(e.shape) == (0, 3)
            assert len(omap.search(pts[:0])[0]) == 0 and len(omap.cast_rays(rays[:0, :3], rays[:0, 3:])[0]) == 0
            if not again:
                o, max_range, p = scans_of("box")[0]
                omap.insert_cloud(dev(p), o)
                assert (omap.cast_rays(dev(rays[:, :3]), dev(rays[:, 3:]))[0].cpu().numpy() == qc.RAY_HIT).all()
                omap.reset()
    finally:
        omap.close()


def test_asynchronous_queries_then_a_synchronous_one(pkg, bm, torch_cuda):
    omap, thres = build(pkg, bm, "scene")
    try:
        tag = "scene_view"
        rays = FX[f"{tag}_rays"]
        q = pkg.occ_query_params(6.0, thres, True)
        o, d = dev(rays[:, :3]), dev(rays[:, 3:])
        first = [omap.cast_rays(o, d, q, sync=False) for _ in range(3)]
        view = omap.cast_view(40, 30, gpu_model(pkg, scene_model()), FX["scene_poses"][0], 4, q, sync=False)
        found = omap.search(dev(FX["scene_search_points"]), thres, sync=False)
        last = omap.cast_rays(o, d, q)                          # synchronous: everything before it has finished
        for got in first + [view, last]:
            same_rays(got, FX[f"{tag}_status"], FX[f"{tag}_end"], "sync = 0")
        assert np.array_equal(found[0].cpu().numpy(), FX["scene_search_state"])
    finally:
        omap.close()


@pytest.mark.parametrize("tree", ["scene", "scene_hits"])
def test_ten_thousand_queries_leave_the_map_as_it_was(pkg, bm, tree):
    omap, thres = build(pkg, bm, tree)
    try:
        before = omap.keys() if is_hits(tree) else omap.fetch_logodds()
        size = omap.size()
        rng = np.random.default_rng(3)
        rays = FX[f"{tree}_random_rays"][rng.integers(0, 1024, 10000)]
        pts = FX[f"{tree}_search_points"][rng.integers(0, 512, 10000)]
        for ignore in (False, True):
            omap.cast_rays(dev(rays[:, :3]), dev(rays[:, 3:]), max_range=6.0, occupancy_thres_log=thres, ignore_unknown=ignore)
        omap.search(dev(pts), thres)
        omap.cast_view(100, 100, gpu_model(pkg, scene_model()), FX["scene_poses"][0], 2, max_range=6.0, ignore_unknown=True)
        after = omap.keys() if is_hits(tree) else omap.fetch_logodds()
        assert omap.size() == size and omap.overflow() == 0
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
    finally:
        omap.close()


def test_host_staging_of_a_larger_query_is_not_read(pkg, bm):
    """Large, small, large through one handle: the host forms place points, states and values (directions, origins, statuses
    and ends) anew in staging that only grows, at counts whose arrays end off the staging's alignment."""
    omap, thres = build(pkg, bm, "scene")
    try:
        rays, status, end = FX["scene_view_rays"], FX["scene_view_status"], FX["scene_view_end"]
        pts, state, value = FX["scene_search_points"], FX["scene_search_state"], FX["scene_search_value"]
        q = pkg.occ_query_params(6.0, thres, True)
        for n in (257, 1, 17, 257):
            o, d = np.ascontiguousarray(rays[:n, :3]), np.ascontiguousarray(rays[:n, 3:])
            same_rays(omap.cast_rays(o, d, q), status[:n], end[:n], ("host", n))
            if len({tuple(r) for r in o.view(np.uint32).tolist()}) == 1:
                same_rays(omap.cast_rays(o[0], d, q), status[:n], end[:n], ("host, one origin", n))
            st, v = omap.search(np.ascontiguousarray(pts[:n]), thres)
            assert np.array_equal(st, state[:n]), n
            assert np.array_equal(np.asarray(v).view(np.uint32), value[:n].view(np.uint32)), n
    finally:
        omap.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wavefront_and_workgroup_edges(pkg, bm, torch_cuda, n):
    torch = torch_cuda
    omap, thres = build(pkg, bm, "scene")
    try:
        rays, status, end = FX["scene_view_rays"][:n], FX["scene_view_status"][:n], FX["scene_view_end"][:n]
        q = pkg.occ_query_params(6.0, thres, True)
        # outputs inside larger buffers: nothing beyond n is written
        d_status = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda:0")
        d_end = torch.full((n + 64, 3), -7.0, dtype=torch.float32, device="cuda:0")
        o, d = dev(rays[:, :3]), dev(rays[:, 3:])
        L = pkg.load_library()
        assert L.sbm_occ_cast_rays_device(omap._m, n, o.data_ptr(), 0, d.data_ptr(), ctypes.byref(q), d_status.data_ptr(),
                                          d_end.data_ptr(), 1) == 0
        same_rays((d_status[:n], d_end[:n]), status, end, n)
        assert bool((d_status[n:] == -7).all()) and bool((d_end[n:] == -7.0).all())
        assert L.sbm_occ_cast_rays_device(omap._m, n, o.data_ptr(), 0, d.data_ptr(), ctypes.byref(q), d_status.data_ptr(), None, 1) == 0
        pts, state, value = FX["scene_search_points"][:n], FX["scene_search_state"][:n], FX["scene_search_value"][:n]
        d_state = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda:0")
        d_value = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda:0")
        p = dev(pts)
        assert L.sbm_occ_search_device(omap._m, n, p.data_ptr(), thres, d_state.data_ptr(), d_value.data_ptr(), 1) == 0
        assert np.array_equal(d_state[:n].cpu().numpy(), state)
        assert np.array_equal(d_value[:n].cpu().numpy().view(np.uint32), value.view(np.uint32))
        assert bool((d_state[n:] == -7).all()) and bool((d_value[n:] == -7).all())
        assert L.sbm_occ_search_device(omap._m, n, p.data_ptr(), thres, d_state.data_ptr(), None, 1) == 0
        st, e = omap.cast_view(n, 1, gpu_model(pkg, scene_model()), FX["scene_poses"][0], 4, q)        # one row of n pixels
        want = restated("scene").cast_rays(*qc.view_rays(n, 1, 4, scene_model(), FX["scene_poses"][0]), True, 6.0)
        same_rays((st, e), *want, ("row", n))
        st, e = omap.cast_view(3, n, gpu_model(pkg, scene_model()), FX["scene_poses"][0], 4, q)        # and three columns of n
        want = restated("scene").cast_rays(*qc.view_rays(3, n, 4, scene_model(), FX["scene_poses"][0]), True, 6.0)
        same_rays((st, e), *want, ("columns", n))
    finally:
        omap.close()


def test_a_table_filled_to_its_capacity_answers_as_the_transcription(pkg, bm):
    """A capacity of a quarter to a half of the scene's voxels: the table has fewer slots than the scene has voxels, so it
    fills up, probe chains run to the probe bound, and some voxels find no slot. Whatever was stored answers exactly; what
    overflowed reads as unknown."""
    probs = [float(v) for v in FX["scene_params"]]
    n = len(FX["scene_keys"])
    cap = 1 << (n.bit_length() - 2)                  # slots = 2 * cap: between n / 2 and n
    omap = pkg.OccupancyMap(bm, cap)
    try:
        for o, max_range, p in scans_of("scene"):
            try:
                omap.insert_cloud(dev(p), o, pkg.occ_ray_params(*probs, max_range=max_range))
            except pkg.StereoBMError as e:
                assert e.code == pkg.ERR_OCC_FULL
        keys, lo = omap.fetch_logodds(allow_overflow=True)
        assert cap <= len(keys) <= 2 * cap < n and omap.overflow() > 0         # filled beyond its capacity
        thres = float(FX["scene_constants"][4])
        m = qc.Map(dict(zip((int(k) for k in keys), lo)), qc.LOGODDS, thres, RES)
        rays = FX["scene_random_rays"][:256]
        for ignore in (False, True):
            want = m.cast_rays(rays[:, :3], rays[:, 3:], ignore, 6.0)
            same_rays(omap.cast_rays(dev(rays[:, :3]), dev(rays[:, 3:]), max_range=6.0, occupancy_thres_log=thres, ignore_unknown=ignore),
                      *want, ("full", ignore))
        pts = FX["scene_search_points"]
        st, v = omap.search(dev(pts), thres)
        want = m.search_all(pts)
        assert np.array_equal(st.cpu().numpy(), want[0]) and np.array_equal(v.cpu().numpy().view(np.uint32), want[1])
        lost = sorted(set(int(k) for k in FX["scene_keys"]) - set(int(k) for k in keys))
        assert lost                                                            # a voxel that overflowed reads as unknown
        centre = qc.centre(((lost[0] >> 32) & 0xFFFF, (lost[0] >> 16) & 0xFFFF, lost[0] & 0xFFFF), RES)
        assert omap.search(centre[None], thres)[0][0] == qc.CELL_UNKNOWN
        after = omap.fetch_logodds(allow_overflow=True)
        assert np.array_equal(after[0], keys) and np.array_equal(after[1].view(np.uint32), lo.view(np.uint32))
    finally:
        omap.close()


def test_argument_checks_in_their_documented_order_leave_the_map_alone(pkg, bm, torch_cuda):
    torch = torch_cuda
    L = pkg.load_library()
    omap, thres = build(pkg, bm, "box")
    try:
        before = omap.fetch_logodds()
        q, nanq = pkg.occ_query_params(), pkg.occ_query_params(max_range=float("nan"))
        nant = pkg.occ_query_params(occupancy_thres_log=float("nan"))
        m = gpu_model(pkg, scene_model())
        a = torch.zeros((8, 3), dtype=torch.float32, device="cuda:0")
        s = torch.zeros((8,), dtype=torch.int32, device="cuda:0")
        h = np.zeros((8, 3), np.float32)
        hs = np.zeros(8, np.int32)
        pose = np.ascontiguousarray(FX["scene_poses"][0])
        P, S, Q, big, odd = a.data_ptr(), s.data_ptr(), ctypes.byref(q), (1 << 30) + 1, a.data_ptr() + 2
        nan = float("nan")
        # search: null, then the threshold, then the count and the alignment
        assert L.sbm_occ_search_device(omap._m, 8, None, nan, S, None, 1) == NULL
        assert L.sbm_occ_search_device(omap._m, 8, P, nan, None, None, 1) == NULL
        assert L.sbm_occ_search_device(omap._m, big, odd, nan, S, None, 1) == SIZE
        assert L.sbm_occ_search_device(omap._m, big, P, 0.0, S, None, 1) == UNSUPPORTED
        assert L.sbm_occ_search_device(omap._m, 8, odd, 0.0, S, None, 1) == UNSUPPORTED
        assert L.sbm_occ_search_device(omap._m, 8, P, 0.0, S + 2, None, 1) == UNSUPPORTED
        assert L.sbm_occ_search_device(omap._m, 8, P, 0.0, S, S + 1, 1) == UNSUPPORTED
        assert L.sbm_occ_search_device(omap._m, 0, None, 0.0, None, None, 1) == 0
        assert L.sbm_occ_search(omap._m, 8, None, nan, hs.ctypes.data, None) == NULL
        assert L.sbm_occ_search(omap._m, 8, h.ctypes.data, nan, hs.ctypes.data, None) == SIZE
        assert L.sbm_occ_search(omap._m, big, h.ctypes.data, 0.0, hs.ctypes.data, None) == UNSUPPORTED
        # cast_rays: null, then the parameters, then the count and the alignment
        assert L.sbm_occ_cast_rays_device(omap._m, 8, None, 0, P, ctypes.byref(nanq), S, None, 1) == NULL
        assert L.sbm_occ_cast_rays_device(omap._m, 8, P, 0, None, ctypes.byref(nanq), S, None, 1) == NULL
        assert L.sbm_occ_cast_rays_device(omap._m, 8, P, 0, P, None, S, None, 1) == NULL
        assert L.sbm_occ_cast_rays_device(omap._m, 8, P, 0, P, ctypes.byref(nanq), None, None, 1) == NULL
        assert L.sbm_occ_cast_rays_device(omap._m, big, odd, 0, P, ctypes.byref(nanq), S, None, 1) == SIZE
        assert L.sbm_occ_cast_rays_device(omap._m, big, odd, 0, P, ctypes.byref(nant), S, None, 1) == SIZE
        assert L.sbm_occ_cast_rays_device(omap._m, big, P, 0, P, Q, S, None, 1) == UNSUPPORTED
        assert L.sbm_occ_cast_rays_device(omap._m, 8, odd, 0, P, Q, S, None, 1) == UNSUPPORTED
        assert L.sbm_occ_cast_rays_device(omap._m, 8, P, 0, odd, Q, S, None, 1) == UNSUPPORTED
        assert L.sbm_occ_cast_rays_device(omap._m, 8, P, 0, P, Q, S + 1, None, 1) == UNSUPPORTED
        assert L.sbm_occ_cast_rays_device(omap._m, 8, P, 0, P, Q, S, P + 3, 1) == UNSUPPORTED
        assert L.sbm_occ_cast_rays_device(omap._m, 0, None, 0, None, Q, None, None, 1) == 0
        assert L.sbm_occ_cast_rays_device(omap._m, 8, h.ctypes.data, 1, P, Q, S, None, 1) == 0      # one origin in host memory
        assert L.sbm_occ_cast_rays(omap._m, 8, h.ctypes.data, 0, None, Q, hs.ctypes.data, None) == NULL
        assert L.sbm_occ_cast_rays(omap._m, 8, h.ctypes.data, 0, h.ctypes.data, ctypes.byref(nanq), hs.ctypes.data, None) == SIZE
        assert L.sbm_occ_cast_rays(omap._m, big, h.ctypes.data, 0, h.ctypes.data, Q, hs.ctypes.data, None) == UNSUPPORTED
        # cast_view: null, sizes, parameters, then what is unsupported
        view = L.sbm_occ_cast_view_device
        assert view(omap._m, 0, 4, 1, None, pose.ctypes.data, ctypes.byref(nanq), S, None, 1) == NULL
        assert view(omap._m, 0, 4, 1, ctypes.byref(m), None, ctypes.byref(nanq), S, None, 1) == NULL
        assert view(omap._m, 0, 4, 1, ctypes.byref(m), pose.ctypes.data, None, S, None, 1) == NULL
        assert view(omap._m, 0, 4, 1, ctypes.byref(m), pose.ctypes.data, ctypes.byref(nanq), None, None, 1) == NULL
        for w, hh, sc in ((0, 4, 1), (4, -1, 1), (4, 4, 0)):
            assert view(omap._m, w, hh, sc, ctypes.byref(m), pose.ctypes.data, ctypes.byref(nanq), S + 1, None, 1) == SIZE
        assert view(omap._m, 1 << 16, 1 << 16, 1, ctypes.byref(m), pose.ctypes.data, ctypes.byref(nanq), S, None, 1) == SIZE
        assert view(omap._m, 1 << 16, 1 << 16, 1, ctypes.byref(m), pose.ctypes.data, Q, S, None, 1) == UNSUPPORTED
        assert view(omap._m, 2, 2, (1 << 23) + 1, ctypes.byref(m), pose.ctypes.data, Q, S, None, 1) == UNSUPPORTED
        assert view(omap._m, 2, 2, 1, ctypes.byref(m), pose.ctypes.data, Q, S + 1, None, 1) == UNSUPPORTED
        assert view(omap._m, 2, 2, 1, ctypes.byref(m), pose.ctypes.data, Q, S, P + 2, 1) == UNSUPPORTED
        assert view(omap._m, 2, 2, 1, ctypes.byref(m), pose.ctypes.data, Q, S, None, 1) == 0
        with pytest.raises(pkg.StereoBMError) as e:
            omap.cast_rays(h, h[:3])
        assert e.value.code == SIZE
        assert not a.cpu().numpy().any()                          # no refused call wrote through a pointer
        after = omap.fetch_logodds()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
        assert omap.overflow() == 0
    finally:
        omap.close()


def test_the_two_profile_names_fill_and_leave_the_others_alone(pkg):
    eng = pkg.StereoBM.create(64, 21)
    omap = pkg.OccupancyMap(eng, 1 << 14)
    try:
        eng.set_profiling(True)
        o, max_range, p = scans_of("box")[0]
        omap.insert_cloud(dev(p), o)
        first = omap.profile()
        assert first["occ_rays_mark"] > 0 and first["occ_search"] == 0 and first["occ_cast"] == 0
        rays = FX["box_axes_rays"]
        omap.cast_rays(dev(rays[:, :3]), dev(rays[:, 3:]))
        cast = omap.profile()
        assert cast["occ_cast"] > 0 and cast["occ_search"] == 0
        omap.search(dev(FX["box_search_points"]))
        both = omap.profile()
        assert both["occ_search"] > 0 and both["occ_cast"] == cast["occ_cast"]
        omap.cast_view(8, 8, gpu_model(pkg, scene_model()), FX["scene_poses"][0], 16)
        view = omap.profile()
        assert view["occ_cast"] > 0 and view["occ_search"] == both["occ_search"]
        for k in ("occ_insert", "occ_fetch", "occ_rays_mark", "occ_rays_apply"):
            assert view[k] == first[k], k
        v = ctypes.c_float()
        for name in ("occ_searchx", "occ_cas", "occ_cast_view"):
            assert eng._L.sbm_get_profile(eng._h, name.encode(), ctypes.byref(v)) == UNSUPPORTED, name
    finally:
        eng.set_profiling(False)
        omap.close()
        eng.close()


def test_cpp_call_site_answers_as_octomap(pkg, bm, tmp_path):
    exe, built = build_callsite(tmp_path, "occupancy_query_callsite_main.cpp")
    assert built.returncode == 0, built.stderr
    cloud = np.concatenate([np.concatenate([np.float32([len(p)]), o, p.reshape(-1)]) for o, _, p in scans_of("scene")]).astype(np.float32)
    cloud.tofile(tmp_path / "cloud.raw")
    take = np.r_[0:48, 48:96:2, 49:96:2]            # the single half alternates ignore_unknown, the batch half is two batches
    rays = np.ascontiguousarray(np.concatenate([FX["scene_random_rays"][take].astype(np.float64),
                                                FX["scene_random_ignore"][take, None].astype(np.float64),
                                                FX["scene_random_max_range"][take, None]], axis=1))
    rays.tofile(tmp_path / "rays.raw")
    pts = np.ascontiguousarray(FX["scene_search_points"][:16])
    pts.tofile(tmp_path / "points.raw")
    r = subprocess.run([str(exe), str(tmp_path / "cloud.raw"), str(len(cloud)), "6.0", str(1 << 14), str(tmp_path / "rays.raw"),
                        str(len(rays)), str(tmp_path / "points.raw"), str(len(pts)), str(tmp_path / "out.raw")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split() == ["size", str(len(FX["scene_keys"])), "rays", "96", "points", "16"], r.stdout + r.stderr
    raw = (tmp_path / "out.raw").read_bytes()
    rec = np.frombuffer(raw, np.uint32, 5 * len(rays)).reshape(-1, 5)
    assert np.array_equal(rec[:, 0], FX["scene_random_ret"][take])                               # octomap's bool
    assert np.array_equal(rec[:, 1].view(np.int32), FX["scene_random_status"][take])
    assert np.array_equal(rec[:, 2:], FX["scene_random_end"][take].view(np.uint32))              # NaN where octomap left it
    found = np.frombuffer(raw, np.uint32, 2 * len(pts), 20 * len(rays)).reshape(-1, 2)
    assert np.array_equal(found[:, 0].view(np.int32), FX["scene_search_state"][:16])
    assert np.array_equal(found[:, 1], FX["scene_search_value"][:16].view(np.uint32))
