"""sbm_get_profile over every family of one handle (u96-slam_amd/csrc/sbm_handle.h: each_clock, and the stage tables in the
families' files): every documented name answers on a fresh handle, one small profiled call per family fills that family's names
and no other's, the totals are the sums the sources form, and reset, the handle pool and the block matcher's ring start at zero.
The names below are written out from include/sbm.h, not read from the library."""
import ctypes
import pathlib

import numpy as np
import pytest

import occupancy_ref
from gpu_support import dev
from lk_cases import small_pair, small_points

ROOT = pathlib.Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu
OK, UNSUPPORTED = 0, -23
W, H, N = 64, 48, 2
NAMES = {
    "bm": ("prefilter", "sad", "border", "lrcheck", "speckle", "total"),
    "sgbm": ("sgbm_cost", "sgbm_aggregate", "sgbm_select", "sgbm_median", "sgbm_speckle", "sgbm_total"),
    "gftt_select": ("gftt_select_eig", "gftt_select_select", "gftt_select_total"),
    "gftt_cv": ("gftt_cv_eig", "gftt_cv_select", "gftt_cv_total"),
    "orb": ("orb_blur", "orb_desc", "orb_total"),
    "match": ("match_knn", "match_unique", "match_project", "match_total"),
    "pnp": ("pnp_hyp", "pnp_score", "pnp_refine", "pnp_total"),
    "lk": ("lk_pyramid", "lk_track", "lk_total"),
    "occ": ("occ_insert", "occ_fetch"),
}
# what must be > 0 after the family's call, and the totals the sources form as float sums of their parts, in the sources' order
# (the block matcher's, the semi-global matcher's and gftt_select's totals are timed on their own, from the first mark to the last)
POSITIVE = {f: n[-1] for f, n in NAMES.items()}
POSITIVE["occ"] = "occ_insert"
SUMS = {
    "gftt_cv": ("gftt_cv_eig", "gftt_cv_select"),
    "orb": ("orb_blur", "orb_desc"),
    "match": ("match_knn", "match_unique", "match_project"),
    "pnp": ("pnp_hyp", "pnp_score", "pnp_refine"),
    "lk": ("lk_pyramid", "lk_track"),
}


def create(pkg):
    bm = pkg.StereoBM.create(16, 9)
    bm.setDisp12MaxDiff(1)
    bm.setSpeckleWindowSize(20)
    bm.setSpeckleRange(4)
    return bm


def pair():
    rng = np.random.default_rng(11)
    base = (np.cumsum(rng.integers(-9, 10, (N, H, W + 8)), axis=2) % 256).astype(np.uint8)
    return dev(base[:, :, 8:].copy()), dev(base[:, :, 3:3 + W].copy())


def read(bm, name):
    v = ctypes.c_float(-1.0)
    return bm._L.sbm_get_profile(bm._h, name.encode(), ctypes.byref(v)), v.value


def assert_all_zero(bm, families=tuple(NAMES)):
    for f in families:
        for name in NAMES[f]:
            assert read(bm, name) == (OK, 0.0), name


def run_bm(bm, pkg):
    bm.compute(*pair())


def run_sgbm(bm, pkg):
    bm._compute_device(bm._L.sbm_sgbm_compute_device, (ctypes.byref(pkg.sgbm_params(0, 16, 5, speckleWindowSize=20, speckleRange=2)),),
                       *pair(), None, True)


def run_gftt_select(bm, pkg):
    bm.gftt_detect(pair()[0])


def run_gftt_cv(bm, pkg):
    rng = np.random.default_rng(3003)
    bm.gftt_cv_detect(dev(rng.integers(0, 256, (N, 3, 3)).astype(np.uint8)))   # 3 x 3: the smallest of test_gpu_gftt_cv's test_sizes


def run_orb(bm, pkg):
    import torch

    pattern = np.load(ROOT / "tests" / "golden" / "orb_pattern.npz")["pattern"]
    kpts = np.tile(np.array([[32.0, 24.0], [20.0, 20.0], [40.0, 27.0]], np.float32), (N, 1, 1))
    bm.orb_describe(pair()[0], dev(kpts), torch.full((N,), 3, dtype=torch.int32, device="cuda:0"), pattern)


def run_match(bm, pkg):
    rng = np.random.default_rng(5)
    desc = rng.integers(0, 256, (24, 32), dtype=np.uint8)
    xyz = np.stack([rng.uniform(-1, 1, 24), rng.uniform(-1, 1, 24), rng.uniform(2, 4, 24)], axis=1).astype(np.float32)
    K = (60.0, 60.0, 32.0, 24.0)
    kpts = np.stack([K[0] * xyz[:, 0] / xyz[:, 2] + K[2], K[1] * xyz[:, 1] / xyz[:, 2] + K[3]], axis=1).astype(np.float32)
    T = np.eye(4, dtype=np.float32)[:3].reshape(-1)
    bm.match_guess_host(xyz, kpts, desc, desc, T, K, (W, H))   # projection and guided matching in one call


def run_pnp(bm, pkg):
    rng = np.random.default_rng(6)
    xyz = np.stack([rng.uniform(-1, 1, 40), rng.uniform(-1, 1, 40), rng.uniform(2, 4, 40)], axis=1).astype(np.float32)
    K = (60.0, 60.0, 32.0, 24.0)
    kpts = np.stack([K[0] * xyz[:, 0] / xyz[:, 2] + K[2], K[1] * xyz[:, 1] / xyz[:, 2] + K[3]], axis=1).astype(np.float32)
    pairs = np.stack([np.arange(40), np.arange(40)], axis=1).astype(np.int32)
    bm.estimate_motion_host(xyz, kpts, xyz, pairs, K)


def run_lk(bm, pkg):
    import torch

    left, right = small_pair(16, 4)   # 16 x 4: the smallest of test_gpu_lk's small frames
    pts = small_points(16, 4)
    bm.lk_stereo(dev(np.stack([left] * N)), dev(np.stack([right] * N)), dev(np.stack([pts] * N)),
                 torch.full((N,), len(pts), dtype=torch.int32, device="cuda:0"))


def run_occ(bm, pkg):
    rows, cols = np.mgrid[0:H, 0:W]
    planes = np.stack([(200 + 8 * rows + cols + 30 * k).astype(np.int16) for k in range(N)])
    poses = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(-1), (N, 1))
    m = pkg.StereoModel()
    ref = occupancy_ref.model()
    ctypes.memmove(ctypes.byref(m), ctypes.byref(ref), ctypes.sizeof(m))
    omap = pkg.OccupancyMap(bm, 1 << 15)
    try:
        omap.insert(dev(planes), m, poses, 4)
        assert len(omap.keys()[0]) > 0
    finally:
        omap.close()


RUN = {"bm": run_bm, "sgbm": run_sgbm, "gftt_select": run_gftt_select, "gftt_cv": run_gftt_cv, "orb": run_orb, "match": run_match,
       "pnp": run_pnp, "lk": run_lk, "occ": run_occ}


def test_a_fresh_handle_answers_every_name_with_zero(pkg):
    bm = create(pkg)
    try:
        assert_all_zero(bm)
        for name in ("nope", "", "total_", "sgbm_total0", "occ_fetchx", "borde"):
            assert read(bm, name)[0] == UNSUPPORTED, name
    finally:
        bm.close()


def test_each_family_fills_its_own_names_then_reset_and_pool_start_at_zero(pkg):
    bm = create(pkg)
    try:
        bm.set_profiling(1)
        families = list(NAMES)
        for i, f in enumerate(families):
            RUN[f](bm, pkg)
            t = {name: read(bm, name) for name in NAMES[f]}
            print(f, {k: v[1] for k, v in t.items()})
            assert all(st == OK and ms >= 0.0 for st, ms in t.values()), (f, t)
            assert t[POSITIVE[f]][1] > 0.0, (f, t)
            if f in SUMS:
                s = np.float32(0)
                for part in SUMS[f]:
                    s = np.float32(s + np.float32(t[part][1]))
                assert s == np.float32(t[NAMES[f][-1]][1]), (f, t)
            if f == "bm":
                assert t["border"][1] == 0.0
            assert_all_zero(bm, families[i + 1:])
        bm.set_profiling(0)
        bm.set_profiling(1)
        assert_all_zero(bm)
        RUN["bm"](bm, pkg)
        RUN["orb"](bm, pkg)
        assert read(bm, "total")[1] > 0.0 and read(bm, "orb_total")[1] > 0.0
    finally:
        bm.close()                 # parked for re-use
    bm2 = create(pkg)              # re-armed from the parked handles
    try:
        assert_all_zero(bm2)
    finally:
        bm2.close()


def test_mode_2_averages_the_ring_of_unsynchronised_calls(pkg):
    import torch

    bm = create(pkg)
    try:
        left, right = pair()
        out = torch.empty((N, H, W), dtype=torch.int16, device="cuda:0")
        bm.set_profiling(2)
        for _ in range(4):
            bm.compute_device(left, right, out, sync=False)
        t = {name: read(bm, name) for name in NAMES["bm"]}   # synchronises
        bm.synchronize()
        print(t)
        parts = [t[k][1] for k in ("prefilter", "sad", "lrcheck", "speckle")]
        assert all(st == OK for st, _ in t.values()) and all(p > 0.0 for p in parts), t
        # The four stages run from mark to mark, so they partition the total exactly. Each of the five figures is a float32
        # sum of four float32 event differences: at most five roundings of 2^-24 of itself. So the sum of the parts may pass
        # the total by ten such roundings of the total, which 2^-20 covers; nothing wider is allowed.
        assert sum(parts) <= t["total"][1] * (1 + 2.0 ** -20), t
        assert t["border"][1] == 0.0
    finally:
        bm.close()
