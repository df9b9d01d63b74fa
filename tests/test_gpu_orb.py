"""GPU ORB descriptors (u96-slam_amd/csrc/sbm_orb.hip) bit for bit against the CPU restatement of computeDescriptor (oracle/orb_ref.c):
blurred frames, kept keypoints and counts, and every descriptor byte, under both readings of the blur's rounding, through the
device, features, host and asynchronous entry points. The pattern is the reference's, from tests/golden/orb_pattern.npz."""
import ctypes
import pathlib

import numpy as np
import pytest

import gftt_select_ref as gref
import orb_ref as ref
from gpu_support import bm, build_callsite, dev  # noqa: F401

ROOT = pathlib.Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu
READINGS = [False, True]
RIDS = ["half_even", "half_up"]


@pytest.fixture(scope="module")
def pattern():
    return np.load(ROOT / "tests" / "golden" / "orb_pattern.npz")["pattern"]


@pytest.fixture
def reading(monkeypatch, request):
    half_up = request.param
    if half_up:
        monkeypatch.setenv("SBM_CV_READING", "128")
    else:
        monkeypatch.delenv("SBM_CV_READING", raising=False)
    return half_up


def slots(kp_list, cap):
    """Per-frame keypoint lists -> (n, cap, 2) float32 filled with a marker past each count, and the counts."""
    n = len(kp_list)
    out = np.full((n, cap, 2), -7.25, np.float32)
    cnt = np.zeros(n, np.int32)
    for i, k in enumerate(kp_list):
        out[i, :len(k)] = k
        cnt[i] = len(k)
    return out, cnt


def check_frame(desc, kk, cc, i, img, kpts, pattern, angle=-1.0, half_up=False, blur=None, what="", edge=19):
    want_k, want_d, want_b = ref.describe(img, kpts, pattern, angle=angle, edge=edge, half_up=half_up)
    k = int(cc[i])
    assert k == len(want_k), (what, i, k, len(want_k))
    assert np.array_equal(kk[i, :k], want_k), (what, i)
    bad = int((desc[i, :k] != want_d).sum())
    assert bad == 0, (what, i, bad)
    if blur is not None and want_b is not None:
        assert np.array_equal(blur[i], want_b), (what, i, int((blur[i] != want_b).sum()))


def run_describe(bm, imgs, kp_list, pattern, cap=None, angle=-1.0, out=None, edge=19):
    cap = cap or max(1, max(len(k) for k in kp_list))
    kp, cn = slots(kp_list, cap)
    d, kk, cc, bl = bm.orb_describe(dev(imgs), dev(kp), dev(cn), pattern, angle=angle, edge_threshold=edge, blur=True, out=out)
    return d.cpu().numpy(), kk.cpu().numpy(), cc.cpu().numpy(), bl.cpu().numpy()


def random_kpts(rng, w, h, n, frac=True):
    x = rng.uniform(-2, w + 2, n)
    y = rng.uniform(-2, h + 2, n)
    if frac:   # integral, half-integral and arbitrary
        sel = rng.integers(0, 3, n)
        x = np.where(sel == 0, np.round(x), np.where(sel == 1, np.floor(x) + 0.5, x))
        y = np.where(sel == 0, np.round(y), np.where(sel == 1, np.floor(y) + 0.5, y))
    return np.stack([x, y], 1).astype(np.float32)


@pytest.mark.parametrize("reading", READINGS, ids=RIDS, indirect=True)
def test_features_on_the_golden_frames(bm, oracle, golden, pattern, reading):
    imgs = np.stack([golden["rect_l"], golden["rect_r"]])
    d, kk, cc, bl = bm.orb_features(dev(imgs), pattern, blur=True)
    d, kk, cc, bl = d.cpu().numpy(), kk.cpu().numpy(), cc.cpu().numpy(), bl.cpu().numpy()
    for i, im in enumerate(imgs):
        e, m = oracle.gftt_eig(im)
        kpts = gref.select(e, m)
        check_frame(d, kk, cc, i, im, kpts, pattern, half_up=reading, blur=bl, what="features")
        assert cc[i] > 100 and cc[i] < len(kpts)   # some keypoints fall to the border rule


@pytest.mark.parametrize("reading", READINGS, ids=RIDS, indirect=True)
def test_random_patterns_and_angles(bm, reading):
    rng = np.random.default_rng(11 + int(reading))
    for case in range(12):
        w, h = int(rng.integers(39, 200)), int(rng.integers(39, 120))
        n = int(rng.integers(1, 4))
        imgs = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
        if case % 3 == 0:
            imgs = np.clip(imgs // 64 * 85, 0, 255).astype(np.uint8)   # flat areas: many ties in the comparisons
        pat = rng.integers(-13, 14, (512, 2))
        angle = float(rng.uniform(-360, 360)) if case % 4 else float(rng.choice([0.0, -1.0, 90.0, 45.0, -135.0]))
        kl = [random_kpts(rng, w, h, int(rng.integers(0, 300))) for _ in range(n)]
        d, kk, cc, bl = run_describe(bm, imgs, kl, pat, angle=angle)
        for i in range(n):
            check_frame(d, kk, cc, i, imgs[i], kl[i], pat, angle=angle, half_up=reading, blur=bl, what=(case, w, h, angle))


@pytest.mark.parametrize("w,h", [(39, 39), (40, 39), (41, 47), (45, 64), (61, 50), (255, 40), (257, 41), (259, 77), (300, 100),
                                 (8192, 40)])
def test_sizes(bm, pattern, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    imgs = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    fixed = np.array([[19, 19], [w - 20, h - 20], [w // 2, h // 2], [19.5, h - 20.5]], np.float32)   # (19, 19) survives even at 39 x 39
    kl = [np.concatenate([random_kpts(rng, w, h, 200), fixed]), np.concatenate([fixed, random_kpts(rng, w, h, 50)])]
    d, kk, cc, bl = run_describe(bm, imgs, kl, pattern)
    for i in range(2):
        check_frame(d, kk, cc, i, imgs[i], kl[i], pattern, blur=bl, what=(w, h))
    assert cc.sum() > 0


@pytest.mark.parametrize("w,h", [(38, 38), (38, 100), (100, 38), (1, 1), (20, 8192)])
def test_too_small_frames_keep_nothing(bm, pattern, w, h):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    kl = [random_kpts(rng, w, h, 20)]
    d, kk, cc, bl = run_describe(bm, img[None], kl, pattern)
    assert cc[0] == 0
    assert not d.any() and not bl.any()


def test_border_filter_edges(bm, pattern):
    w, h = 100, 80
    img = np.random.default_rng(3).integers(0, 256, (h, w), dtype=np.uint8)
    xs = [18.0, 18.49, 18.5, 18.51, 19.0, 19.5, 20.5, w - 20.5, w - 20.0, w - 19.51, w - 19.5, w - 19.49, w - 19.0, w - 18.5]
    ys = [18.5, 19.0, 40.0, h - 20.0, h - 19.5, h - 19.0]
    kp = np.array([(x, y) for x in xs for y in ys] + [(np.nan, 40.0), (40.0, np.inf), (-1e30, 40.0)], np.float32)
    d, kk, cc, bl = run_describe(bm, img[None], [kp], pattern)
    check_frame(d, kk, cc, 0, img, kp, pattern, blur=bl)
    kept_x = set(np.unique(kk[0, :cc[0], 0]).tolist())
    f32 = lambda vals: {float(np.float32(v)) for v in vals}   # noqa: E731
    assert f32([18.51, 19.0, 19.5, 20.5, w - 20.5, w - 20.0, w - 19.51, w - 19.5]) <= kept_x   # cvRound(x) in [19, 81)
    assert not kept_x & f32([18.0, 18.49, 18.5, w - 19.49, w - 19.0, w - 18.5])


# ---- edge thresholds other than the reference's 19 ----------------------------------------------------------------------
def corner_pattern(rng):
    """A random pattern whose first points are the four corners (+-13, +-13): at 45 degrees they turn into (+-18, 0) and
    (0, +-18), the farthest a sample can lie from its centre."""
    pat = rng.integers(-13, 14, (512, 2))
    pat[:8] = [(13, 13), (-13, -13), (13, -13), (-13, 13), (-13, 13), (13, 13), (-13, -13), (13, -13)]
    return pat


def edge_setup(edge, pattern):
    """(pattern, angle) for a threshold: at 18 the samples must reach exactly 18 pixels from the centre in x and in y."""
    if edge != 18:
        return pattern, -1.0
    pat = corner_pattern(np.random.default_rng(18))
    dx, dy = ref.offsets_np(pat, 45.0)
    assert (dx.min(), dx.max(), dy.min(), dy.max()) == (-18, 18, -18, 18)
    return pat, 45.0


@pytest.mark.parametrize("reading", READINGS, ids=RIDS, indirect=True)
@pytest.mark.parametrize("edge", [18, 19, 31])
def test_edge_thresholds(bm, pattern, edge, reading):
    w, h = 100, 80
    pat, angle = edge_setup(edge, pattern)
    rng = np.random.default_rng(edge)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    xs = [edge - 1, edge - 0.51, edge - 0.49, edge, edge + 0.49, w - edge - 1.49, w - edge - 1, w - edge - 0.51, w - edge - 0.49,
          w - edge]
    ys = [edge - 1, edge - 0.51, edge - 0.49, edge, edge + 0.49, h - edge - 1.49, h - edge - 1, h - edge - 0.51, h - edge - 0.49,
          h - edge]
    kp = np.concatenate([np.array([(x, y) for x in xs for y in ys], np.float32), random_kpts(rng, w, h, 200)])
    d, kk, cc, bl = run_describe(bm, img[None], [kp], pat, angle=angle, edge=edge)
    check_frame(d, kk, cc, 0, img, kp, pat, angle=angle, half_up=reading, blur=bl, what=edge, edge=edge)
    kept = {tuple(v) for v in kk[0, :cc[0]].tolist()}
    corners = {(float(x), float(y)) for x in (edge, w - edge - 1) for y in (edge, h - edge - 1)}
    assert corners <= kept                                  # centres whose samples reach column 0 / W - 1 and row 0 / H - 1
    rx, ry = np.rint(kk[0, :cc[0], 0]), np.rint(kk[0, :cc[0], 1])
    assert rx.min() == edge and rx.max() == w - edge - 1 and ry.min() == edge and ry.max() == h - edge - 1


@pytest.mark.parametrize("edge", [18, 19, 31])
def test_frame_with_one_centre(bm, pattern, edge):
    s = 2 * edge + 1
    pat, angle = edge_setup(edge, pattern)
    img = np.random.default_rng(100 + edge).integers(0, 256, (s, s), dtype=np.uint8)
    ys, xs = np.mgrid[0:s, 0:s]
    kp = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    d, kk, cc, bl = run_describe(bm, img[None], [kp], pat, angle=angle, edge=edge)
    check_frame(d, kk, cc, 0, img, kp, pat, angle=angle, blur=bl, what=edge, edge=edge)
    assert cc[0] == 1 and kk[0, 0].tolist() == [edge, edge]


@pytest.mark.parametrize("edge", [18, 19, 31])
def test_frame_of_twice_the_edge_keeps_nothing(bm, pattern, edge):
    pat, angle = edge_setup(edge, pattern)
    rng = np.random.default_rng(200 + edge)
    for w, h in ((2 * edge, 100), (100, 2 * edge), (2 * edge, 2 * edge)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        ys, xs = np.mgrid[0:h, 0:w]
        kp = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
        d, kk, cc, bl = run_describe(bm, img[None], [kp], pat, angle=angle, edge=edge)
        assert cc[0] == 0 and len(ref.describe(img, kp, pat, angle=angle, edge=edge)[0]) == 0
        assert not d.any() and not bl.any()


def test_edge_threshold_limits(bm, pkg, pattern):
    import torch

    assert pkg.orb_validate(pkg.orb_params(edge_threshold=17)) == -23
    assert pkg.orb_validate(pkg.orb_params(edge_threshold=4097)) == -23
    assert pkg.orb_validate(pkg.orb_params(edge_threshold=18)) == 0
    assert pkg.orb_validate(pkg.orb_params(edge_threshold=4096)) == 0
    imgs = torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda:0")
    kp = torch.full((1, 4, 2), 32.0, dtype=torch.float32, device="cuda:0")
    cn = torch.full((1,), 4, dtype=torch.int32, device="cuda:0")
    desc = torch.zeros((1, 4, 32), dtype=torch.uint8, device="cuda:0")
    assert _raw_call(bm, pkg, imgs, kp, cn, pattern, 4, desc, edge=17) == -23
    assert _raw_call(bm, pkg, imgs, kp, cn, pattern, 4, desc, edge=4097) == -23
    assert int(cn[0]) == 4                                  # a refused call writes nothing
    img = np.random.default_rng(7).integers(0, 256, (80, 100), dtype=np.uint8)
    k = random_kpts(np.random.default_rng(8), 100, 80, 50)
    d, kk, cc, bl = run_describe(bm, img[None], [k], pattern, edge=4096)
    assert cc[0] == 0 and not d.any() and not bl.any()


def _raw_call(bm, pkg, imgs, kp, cn, pattern, cap, desc, kout=None, cout=None, sync=1, edge=19):
    L = pkg.load_library()
    p = pkg.orb_params(edge_threshold=edge)
    pat = np.ascontiguousarray(pattern, dtype=np.int32).reshape(-1)
    n, h, w = imgs.shape
    kout = kp if kout is None else kout
    cout = cn if cout is None else cout
    return L.sbm_orb_describe_device(bm._h, n, imgs.data_ptr(), w, h, cap, kp.data_ptr(), cn.data_ptr(), pat.ctypes.data,
                                     ctypes.byref(p), kout.data_ptr(), cout.data_ptr(), desc.data_ptr(), None, sync)


def test_cap_beyond_count_leaves_the_tail_untouched(bm, pkg, golden, pattern):
    import torch

    img = golden["rect_l"]
    rng = np.random.default_rng(8)
    cap = 400
    kl = [random_kpts(rng, 640, 480, 150), random_kpts(rng, 640, 480, 0), random_kpts(rng, 640, 480, 399)]
    kp, cn = slots(kl, cap)
    imgs = dev(np.stack([img, golden["rect_r"], img]))
    desc = torch.full((3, cap, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
    ko = torch.full((3, cap, 2), 3.5, dtype=torch.float32, device="cuda:0")
    co = torch.full((3,), -9, dtype=torch.int32, device="cuda:0")
    assert _raw_call(bm, pkg, imgs, dev(kp), dev(cn), pattern, cap, desc, ko, co) == 0
    d, kk, cc = desc.cpu().numpy(), ko.cpu().numpy(), co.cpu().numpy()
    src = [img, golden["rect_r"], img]
    for i in range(3):
        check_frame(d, kk, cc, i, src[i], kl[i], pattern)
        assert (d[i, cc[i]:] == 0xAB).all() and (kk[i, cc[i]:] == 3.5).all()


def test_in_place_compaction(bm, golden, pattern):
    import torch

    rng = np.random.default_rng(9)
    imgs = np.stack([golden["rect_l"], golden["rect_r"]])
    kl = [random_kpts(rng, 640, 480, 1500), random_kpts(rng, 640, 480, 700)]
    kp, cn = slots(kl, 1500)
    tk, tc = dev(kp), dev(cn)
    d, kk, cc = bm.orb_describe(dev(imgs), tk, tc, pattern, out="inplace")
    assert kk.data_ptr() == tk.data_ptr() and cc.data_ptr() == tc.data_ptr()
    d, kk, cc = d.cpu().numpy(), tk.cpu().numpy(), tc.cpu().numpy()
    for i in range(2):
        check_frame(d, kk, cc, i, imgs[i], kl[i], pattern)
        assert (kk[i, cc[i]:len(kl[i])] == kp[i, cc[i]:len(kl[i])]).all()   # slots past the kept count keep what they held


def test_device_counts_without_host_sync(bm, oracle, golden, pattern):
    imgs = dev(np.stack([golden["rect_l"], golden["rect_r"]] * 3))
    kp, cn = bm.gftt_detect(imgs, sync=False)
    d, kk, cc = bm.orb_describe(imgs, kp, cn, pattern, sync=False)
    bm.synchronize()
    d, kk, cc = d.cpu().numpy(), kk.cpu().numpy(), cc.cpu().numpy()
    for i, im in enumerate([golden["rect_l"], golden["rect_r"]] * 3):
        e, m = oracle.gftt_eig(im)
        check_frame(d, kk, cc, i, im, gref.select(e, m), pattern)


def test_chunked_batch_matches_the_unchunked_one(bm, pattern):
    # 17 frames of 8192 x 2048 (16 MiB each): without d_blur the handle blurs them in chunks of 16
    rng = np.random.default_rng(12)
    n, w, h = 17, 8192, 2048
    base = rng.integers(0, 256, (h, w), dtype=np.uint8)
    imgs = np.stack([np.roll(base, 37 * i, axis=1) for i in range(n)])
    kl = [random_kpts(rng, w, h, 300) for _ in range(n)]
    kp, cn = slots(kl, 300)
    ti = dev(imgs)
    d1, k1, c1 = [t.cpu().numpy() for t in bm.orb_describe(ti, dev(kp), dev(cn), pattern)]
    d2, k2, c2, _ = bm.orb_describe(ti, dev(kp), dev(cn), pattern, blur=True)   # d_blur given: one pass
    assert np.array_equal(c1, c2.cpu().numpy()) and np.array_equal(k1, k2.cpu().numpy())
    assert np.array_equal(d1, d2.cpu().numpy())
    for i in (0, 15, 16):
        check_frame(d1, k1, c1, i, imgs[i], kl[i], pattern, what="chunk")


@pytest.mark.parametrize("reading", READINGS, ids=RIDS, indirect=True)
def test_host_form(bm, golden, pattern, reading):
    rng = np.random.default_rng(13)
    big = np.zeros((480, 700), np.uint8)
    big[:, :640] = golden["rect_l"]
    img = big[:, :640]   # strided rows
    kp = random_kpts(rng, 640, 480, 900)
    d, k = bm.orb_describe_host(img, kp, pattern)
    want_k, want_d, _ = ref.describe(np.ascontiguousarray(img), kp, pattern, half_up=reading)
    assert np.array_equal(k, want_k) and np.array_equal(d, want_d)
    d0, k0 = bm.orb_describe_host(img, np.zeros((0, 2), np.float32), pattern)
    assert d0.shape == (0, 32) and k0.shape == (0, 2)


def test_host_form_staging_of_a_larger_call_is_not_read(bm, pattern):
    """Large, small, large on one handle: points in, points out, descriptors and counts are placed anew in staging that only
    grows, at odd capacities."""
    rng = np.random.default_rng(29)
    img = rng.integers(0, 256, (80, 96), dtype=np.uint8)
    kp = np.stack([rng.uniform(15, 81, 257), rng.uniform(15, 65, 257)], 1).astype(np.float32)
    for n in (257, 1, 3, 17, 257):
        d, k = bm.orb_describe_host(img, kp[:n], pattern)
        want_k, want_d, _ = ref.describe(img, kp[:n], pattern)
        assert len(want_k) > 0 and np.array_equal(k, want_k) and np.array_equal(d, want_d), n


def test_async_features(bm, oracle, golden, pattern):
    imgs = np.stack([golden["rect_r"], golden["rect_l"]])
    d, kk, cc = bm.orb_features(dev(imgs), pattern, sync=False)
    bm.synchronize()
    d, kk, cc = d.cpu().numpy(), kk.cpu().numpy(), cc.cpu().numpy()
    for i, im in enumerate(imgs):
        e, m = oracle.gftt_eig(im)
        check_frame(d, kk, cc, i, im, gref.select(e, m), pattern)


def test_features_then_keypoints3d(bm, pkg, oracle, golden, pattern):
    L, R = golden["rect_l"], golden["rect_r"]
    disp = bm.compute(dev(L), dev(R))
    d, kk, cc = bm.orb_features(dev(L), pattern)
    k = int(cc[0])
    e, m = oracle.gftt_eig(L)
    want_k, want_d, _ = ref.describe(L, gref.select(e, m), pattern)
    assert np.array_equal(kk[0, :k].cpu().numpy(), want_k)
    mo = oracle.make_model()
    mg = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(mg), ctypes.byref(mo), ctypes.sizeof(mg))
    xyz = bm.keypoints3d(disp, kk[0, :k], mg, 0.0, 0.0).cpu().numpy()
    exp = oracle.keypoints3d(disp.cpu().numpy(), want_k, mo, 0.0, 0.0)
    assert np.isfinite(exp).all(axis=1).sum() > 20
    assert np.array_equal(np.isnan(xyz), np.isnan(exp))
    assert np.array_equal(xyz[~np.isnan(xyz)], exp[~np.isnan(exp)])


def test_profile_records_stages(bm, golden, pattern):
    bm.set_profiling(1)
    try:
        bm.orb_features(dev(np.stack([golden["rect_l"]] * 4)), pattern)
        prof = bm.orb_profile()
    finally:
        bm.set_profiling(0)
    assert prof["orb_blur"] > 0 and prof["orb_desc"] > 0
    assert prof["orb_total"] >= prof["orb_desc"]


def test_status_codes_on_the_device(bm, pkg, pattern):
    import torch

    imgs = torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda:0")
    kp = torch.zeros((1, 4, 2), dtype=torch.float32, device="cuda:0")
    cn = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    desc = torch.zeros((1, 4, 32), dtype=torch.uint8, device="cuda:0")
    assert _raw_call(bm, pkg, imgs, kp, cn, pattern, 4, desc) == 0
    bad = np.array(pattern).copy()
    bad[7, 1] = 14
    assert _raw_call(bm, pkg, imgs, kp, cn, bad, 4, desc) == -23
    assert _raw_call(bm, pkg, imgs, kp, cn, pattern, 0, desc) == -2
    with pytest.raises(pkg.StereoBMError):
        bm.orb_features(torch.zeros((1, 600, 1024), dtype=torch.uint8, device="cuda:0"), pattern)


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_opencv"])
def test_cpp_callsite_through_the_adaptor(tmp_path, oracle, golden, pattern, mock):
    import subprocess

    img = golden["rect_l"]
    e, m = oracle.gftt_eig(img)
    kpts = gref.select(e, m)
    H, W = img.shape
    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")] if mock else []
    exe, r = build_callsite(tmp_path, "orb_callsite_main.cpp", extra)
    assert r.returncode == 0, r.stderr[-3000:]
    np.ascontiguousarray(img).tofile(tmp_path / "img.raw")
    np.ascontiguousarray(kpts, np.float32).tofile(tmp_path / "kpts.raw")
    np.ascontiguousarray(pattern, np.int32).tofile(tmp_path / "pat.raw")
    r = subprocess.run([str(exe), str(tmp_path / "img.raw"), str(W), str(H), str(tmp_path / "kpts.raw"), str(tmp_path / "pat.raw"),
                        str(tmp_path / "out.raw")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = (tmp_path / "out.raw").read_bytes()
    k = int(np.frombuffer(raw[:4], np.int32)[0])
    got_k = np.frombuffer(raw[4:4 + 8 * k], np.float32).reshape(k, 2)
    got_d = np.frombuffer(raw[4 + 8 * k:], np.uint8).reshape(k, 32)
    want_k, want_d, _ = ref.describe(img, kpts, pattern)
    assert k == len(want_k) and np.array_equal(got_k, want_k) and np.array_equal(got_d, want_d)


@pytest.mark.parametrize("reading", READINGS, ids=RIDS, indirect=True)
def test_engine_reproduces_the_pin_kit(bm, reading):
    kit = np.load(ROOT / "tests" / "golden" / "pin_kit_orb.npz")
    pat = kit["pattern"]
    r = 128 if reading else 0
    for name in ("ties0", "ties1"):
        img = kit[f"{name}/img"]
        n = img.shape[0]
        ys, xs = np.mgrid[0:n, 0:n]
        kp = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
        d, kk, cc, bl = run_describe(bm, img[None], [kp], pat)
        k = int(cc[0])
        assert np.array_equal(bl[0], kit[f"{name}/blur_r{r}"])
        assert np.array_equal(kk[0, :k], kit[f"{name}/kpts"])
        assert np.array_equal(d[0, :k], kit[f"{name}/desc_r{r}"])


def test_profile_of_a_reused_handle_starts_at_zero(pkg, golden, pattern):
    pkg.trim()                                  # an empty pool: the create below re-arms the handle closed here
    bm1 = pkg.StereoBM.create(64, 21)
    bm1.set_profiling(1)
    bm1.orb_features(dev(np.stack([golden["rect_l"]] * 2)), pattern)
    assert bm1.orb_profile()["orb_total"] > 0
    bm1.close()                                 # parked for re-use
    bm2 = pkg.StereoBM.create(64, 21)           # re-armed from the parked handles
    try:
        assert bm2.orb_profile() == {"orb_blur": 0.0, "orb_desc": 0.0, "orb_total": 0.0}
    finally:
        bm2.close()
