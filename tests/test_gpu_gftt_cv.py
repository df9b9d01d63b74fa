"""GPU generateKeypoints (u96-slam_amd/csrc/sbm_gftt_cv.hip) bit for bit against the sequential C restatement
(oracle/gftt_cv_ref): maps as uint32 views, maxima, counts and every (x, y) in order, for every frame of every batch, under
reading 0 and under each reading bit, through the device, map-level, host, asynchronous and front-end entry points. Equality is
exact: both sides perform the same IEEE operations without contraction."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
from gftt_cv_cases import PARAM_EDGES, READINGS, crafted_frames, plateau_maps, random_case  # noqa: E402
import gftt_cv_ref as ref  # noqa: E402
import orb_ref  # noqa: E402
from gpu_support import bm, build_callsite, dev  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pattern():
    return np.load(ROOT / "tests" / "golden" / "orb_pattern.npz")["pattern"]


@pytest.fixture(params=READINGS, ids=lambda r: f"reading{r}")
def reading(monkeypatch, request):
    if request.param:
        monkeypatch.setenv("SBM_CV_READING", str(request.param))
    else:
        monkeypatch.delenv("SBM_CV_READING", raising=False)
    ref.set_reading(request.param)
    yield request.param
    ref.set_reading(0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_batch(bm, imgs, mf=1500, q=0.01, md=7.0, what="", maps=True):
    """Every frame of the batch: map, maximum, count, keypoints."""
    imgs = np.stack(imgs)
    out = bm.gftt_cv_detect(dev(imgs), max_features=mf, quality_level=q, min_distance=md, maps=maps)
    kp, cn = out[0].cpu().numpy(), out[1].cpu().numpy()
    for i, im in enumerate(imgs):
        want, e, m, nc = ref.detect(im, mf, q, md)
        if maps:
            ge, gm = out[2][i].cpu().numpy(), out[3][i].cpu().numpy()
            assert np.array_equal(bits(ge), bits(e)), (what, i, "map", int((bits(ge) != bits(e)).sum()))
            assert bits(gm) == bits(m), (what, i, "max", float(gm), float(m))
        k = int(cn[i])
        assert k == len(want), (what, i, "count", k, len(want))
        assert np.array_equal(kp[i, :k], want), (what, i, "points", int((kp[i, :k] != want).any(axis=1).sum()))
    return kp, cn


def test_golden_pair(bm, golden, reading):
    kp, cn = check_batch(bm, [golden["rect_l"], golden["rect_r"]], what="golden")
    assert 100 < cn[0] < 1500 and 100 < cn[1] < 1500


def test_crafted_frames_in_one_batch(bm, reading):
    fr = crafted_frames()
    names = sorted(fr)
    check_batch(bm, [fr[k] for k in names], what=names)
    check_batch(bm, [fr[k] for k in names], -1, 0.0, 0.0, what=names)


@pytest.mark.parametrize("mf,q,md", PARAM_EDGES)
def test_param_edges(bm, mf, q, md):
    fr = crafted_frames()
    names = ["noise", "periodic", "tie_corners", "checkerboard"]
    check_batch(bm, [fr[k] for k in names], mf, q, md, what=(names, mf, q, md))


def test_64_kitti_shaped_frames(bm, pkg, reading):
    from u96_slam_amd import synth

    L, _ = synth.make_batch(0, 64, 1242, 375, 64)
    kp, cn = check_batch(bm, list(L), what="kitti")
    assert cn.min() > 0


def test_noise_frames_hit_the_cap(bm):
    rng = np.random.default_rng(1)
    imgs = [rng.integers(0, 256, (375, 1242)).astype(np.uint8) for _ in range(3)]
    kp, cn = check_batch(bm, imgs, what="noise")        # ~31 000 candidates per frame: the list is sorted in device memory
    assert (cn == 1500).all()
    check_batch(bm, imgs[:1], -1, 0.0, 0.0, what="noise uncapped")


def test_640x480(bm, reading):
    rng = np.random.default_rng(640)
    check_batch(bm, [rng.integers(0, 256, (480, 640)).astype(np.uint8),
                     np.kron(rng.integers(0, 256, (60, 80)), np.ones((8, 8), np.int64)).astype(np.uint8)], what="640x480")


@pytest.mark.parametrize("W,H", [(3, 3), (3, 2048), (2048, 3), (4, 4), (5, 3), (63, 15), (64, 16), (65, 17), (66, 18), (127, 33),
                                 (641, 479), (999, 7)])
def test_sizes(bm, W, H, reading):
    rng = np.random.default_rng(W * 1000 + H)
    imgs = [rng.integers(0, 256, (H, W)).astype(np.uint8) for _ in range(2)]
    check_batch(bm, imgs, -1, 0.001, 1.0, what=(W, H))
    check_batch(bm, imgs, 1500, 0.01, 7.0, what=(W, H), maps=False)


def test_2048x2048_frame_and_the_first_size_past_it(bm, pkg, reading):
    import torch

    rng = np.random.default_rng(2048)
    img = rng.integers(0, 256, (2048, 2048)).astype(np.uint8)
    check_batch(bm, [img], what="2048")                     # ~280 000 candidates
    check_batch(bm, [img], 20000, 0.0, 1.5, what="2048 cell 2", maps=False)
    for shape in ((10, 2049), (2049, 10)):
        with pytest.raises(pkg.StereoBMError) as e:
            bm.gftt_cv_detect(torch.zeros(shape, dtype=torch.uint8, device="cuda:0"))
        assert e.value.code == -23


def select_check(bm, e, m, mf, q, md, what):
    import torch

    kp, cn = bm.gftt_cv_select(dev(e), torch.tensor([float(m)], dtype=torch.float32), max_features=mf, quality_level=q,
                               min_distance=md)
    kp, cn = kp.cpu().numpy(), cn.cpu().numpy()
    want, nc = ref.select(e, m, mf, q, md)
    assert int(cn[0]) == len(want), (what, int(cn[0]), len(want))
    assert np.array_equal(kp[0, :len(want)], want), what
    return nc


@pytest.mark.parametrize("name", sorted(plateau_maps()))
def test_map_level_selection(bm, name):
    e, m = plateau_maps()[name]
    for mf, q, md in ((1500, 0.01, 7.0), (-1, 0.01, 0.0), (-1, 0.0, 2.5), (5, 0.5, 1.0)):
        select_check(bm, e, m, mf, q, md, (name, mf, q, md))


def test_2048x2048_plateau_worst_case_candidate_count(bm):
    """Every interior pixel a candidate: 2046 * 2046 keys, sorted in the frame's list in device memory."""
    e = np.full((2048, 2048), 0.25, np.float32)
    for mf, q, md in ((1500, 0.01, 7.0), (-1, 0.01, 7.0), (5000, 0.5, 0.0), (-1, 0.0, 30.0)):
        nc = select_check(bm, e, 0.25, mf, q, md, ("plateau", mf, q, md))
        assert nc == 2046 * 2046


def test_seeded_fuzz_300_cases(bm):
    rng = np.random.default_rng(77)
    for c in range(300):
        img, mf, q, md = random_case(rng)
        rd = int(rng.choice(READINGS))
        ref.set_reading(rd)
        import os
        os.environ["SBM_CV_READING"] = str(rd)
        try:
            check_batch(bm, [img], mf, q, md, what=f"case {c}: {img.shape} {mf} {q} {md} reading {rd}")
        finally:
            os.environ.pop("SBM_CV_READING", None)
            ref.set_reading(0)


@pytest.mark.parametrize("md", [0.0, 1.0, 3.5, 7.0, 7.4])
def test_prefix_property(bm, md):
    rng = np.random.default_rng(12)
    img = rng.integers(0, 256, (120, 160)).astype(np.uint8)
    kf, cf = bm.gftt_cv_detect(dev(img), max_features=-1, quality_level=0.001, min_distance=md, maps=False)
    full = kf[0, :int(cf[0])].cpu().numpy()
    assert np.array_equal(full, ref.detect(img, -1, 0.001, md)[0])
    for cap in (1, 63, 64, 65, 100, len(full)):
        kc, cc = bm.gftt_cv_detect(dev(img), max_features=cap, quality_level=0.001, min_distance=md, maps=False)
        assert np.array_equal(kc[0, :int(cc[0])].cpu().numpy(), full[:cap]), cap


def test_map_entry_point(bm, golden, reading):
    imgs = np.stack([golden["rect_l"], golden["rect_r"]])
    e, m = bm.gftt_cv_eig(dev(imgs))
    for i, im in enumerate(imgs):
        we, wm = ref.eig_map(im)
        assert np.array_equal(bits(e[i].cpu().numpy()), bits(we)) and bits(m[i].cpu().numpy()) == bits(wm)


def test_host_form_with_strided_input(bm, golden, reading):
    wide = np.full((480, 701), 0x33, np.uint8)
    wide[:, :640] = golden["rect_l"]
    view = wide[:, :640]
    got = bm.gftt_cv_detect_host(view)
    assert np.array_equal(got, ref.detect(golden["rect_l"])[0])
    small = np.ascontiguousarray(golden["rect_r"][100:133, 200:277])
    assert np.array_equal(bm.gftt_cv_detect_host(small, max_features=-1, min_distance=2.5), ref.detect(small, -1, 0.01, 2.5)[0])


def test_asynchronous_form_and_absent_maps(bm, golden):
    imgs = np.stack([golden["rect_r"], golden["rect_l"], golden["rect_r"]])
    kp, cn = bm.gftt_cv_detect(dev(imgs), maps=False, sync=False)
    bm.synchronize()
    kp, cn = kp.cpu().numpy(), cn.cpu().numpy()
    for i, im in enumerate(imgs):
        want = ref.detect(im)[0]
        assert int(cn[i]) == len(want) and np.array_equal(kp[i, :len(want)], want)
    kp2, cn2, e, m = bm.gftt_cv_detect(dev(imgs), sync=False)
    bm.synchronize()
    assert np.array_equal(kp2.cpu().numpy(), kp) and np.array_equal(cn2.cpu().numpy(), cn)
    assert np.array_equal(bits(e[1].cpu().numpy()), bits(ref.eig_map(imgs[1])[0]))


def test_entries_past_the_count_are_left_alone(bm, pkg, golden):
    import torch

    img = dev(golden["rect_l"][None])
    p = pkg.gftt_cv_params()
    kp = torch.full((1, 1500, 2), -7.25, dtype=torch.float32, device="cuda:0")
    cn = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    st = pkg.load_library().sbm_gftt_cv_detect_device(bm._h, 1, img.data_ptr(), 640, 480, ctypes.byref(p), None, None,
                                                       kp.data_ptr(), cn.data_ptr(), 1)
    assert st == 0
    k = int(cn[0])
    assert 0 < k < 1500 and bool((kp[0, k:] == -7.25).all()) and bool((kp[0, :k] >= 1).all())


def test_orb_features_cv_chain_and_keypoints3d(bm, pkg, oracle, golden, pattern):
    L, R = golden["rect_l"], golden["rect_r"]
    imgs = np.stack([L, R])
    d, kk, cc = bm.orb_features_cv(dev(imgs), pattern)
    dn, kn, cnn = d.cpu().numpy(), kk.cpu().numpy(), cc.cpu().numpy()
    for i, im in enumerate(imgs):
        want_k, want_d, _ = orb_ref.describe(im, ref.detect(im)[0], pattern)
        k = int(cnn[i])
        assert k == len(want_k) and k > 50
        assert np.array_equal(kn[i, :k], want_k) and np.array_equal(dn[i, :k], want_d)
    # the detector's keypoints feed keypoints3d unchanged
    disp = bm.compute(dev(L), dev(R))
    kp, cn = bm.gftt_cv_detect(dev(L), maps=False)
    k = int(cn[0])
    want = ref.detect(L)[0]
    mo = oracle.make_model()
    mg = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(mg), ctypes.byref(mo), ctypes.sizeof(mg))
    xyz = bm.keypoints3d(disp, kp[0, :k], mg, 0.0, 0.0).cpu().numpy()
    exp = oracle.keypoints3d(disp.cpu().numpy(), want, mo, 0.0, 0.0)
    assert np.isfinite(exp).all(axis=1).sum() > 20
    assert np.array_equal(np.isnan(xyz), np.isnan(exp))
    assert np.array_equal(xyz[~np.isnan(xyz)], exp[~np.isnan(exp)])


def test_profile_records_stages(bm, golden):
    bm.set_profiling(1)
    try:
        bm.gftt_cv_detect(dev(golden["rect_l"]))
        pr = bm.gftt_cv_profile()
    finally:
        bm.set_profiling(0)
    assert pr["gftt_cv_eig"] > 0 and pr["gftt_cv_select"] > 0
    assert abs(pr["gftt_cv_total"] - pr["gftt_cv_eig"] - pr["gftt_cv_select"]) < 1e-3


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_opencv"])
def test_cpp_callsite_through_the_adaptor(tmp_path, golden, mock):
    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")] if mock else []
    exe, r = build_callsite(tmp_path, "gftt_cv_callsite_main.cpp", extra, flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr
    img = golden["rect_l"]
    (tmp_path / "img.raw").write_bytes(img.tobytes())
    stride = 640 if mock else 672
    r = subprocess.run([str(exe), str(tmp_path / "img.raw"), "640", "480", str(stride), str(tmp_path / "out.raw")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / "out.raw", np.float32)
    want = ref.detect(img)[0]
    k = len(want)
    assert np.array_equal(out[:2 * k].reshape(-1, 2), want)
    if mock:
        assert out.size == 3 * k and (out[2 * k:] == 3.0).all()
    else:
        assert out.size == 2 * k


def test_engine_reproduces_the_pin_kit(bm, reading):
    kit = np.load(ROOT / "tests" / "golden" / "pin_kit_gftt_cv.npz")
    mf, q, md = int(kit["params"][0]), float(kit["params"][1]), float(kit["params"][2])
    for name in sorted({k.split("/")[0] for k in kit.files if "/" in k}):
        kp, cn, e, m = bm.gftt_cv_detect(dev(kit[f"{name}/img"]), max_features=mf, quality_level=q, min_distance=md)
        assert np.array_equal(bits(e[0].cpu().numpy()), bits(kit[f"{name}/map_r{reading}"])), name
        assert bits(m[0].cpu().numpy()) == bits(kit[f"{name}/max_r{reading}"]), name
        want = kit[f"{name}/kpts_r{reading}"]
        assert int(cn[0]) == len(want) and np.array_equal(kp[0, :len(want)].cpu().numpy(), want), name
