"""GPU LK stereo (u96-slam_amd/csrc/sbm_lk.hip) bit for bit against the sequential C restatement (oracle/lk_stereo_ref): every
pyramid level and derivative plane, the tracker's right points, status and err (floats compared as uint32, no mismatch
allowed), the sparse keypoint depths, the chain behind the detector, the host form and the C++ call site. Equality is exact: both
sides perform the same IEEE operations, in the same order, without contraction."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import gftt_cv_ref  # noqa: E402
import lk_stereo_ref as ref  # noqa: E402
from gpu_support import bm, build_callsite, dev  # noqa: E402,F401
from lk_cases import PYRAMID_SIZES, bits, grid_points, noise_frame, small_pair, small_points  # noqa: E402

pytestmark = pytest.mark.gpu
KIT = ROOT / "tests" / "golden" / "pin_kit_lk.npz"


@pytest.fixture(scope="module")
def golden_ref(golden):
    """The restatement's raw and gated outputs for the grid on the golden pair, computed once."""
    pts = grid_points()
    out, st, err, info, _ = ref.track(golden["rect_l"], golden["rect_r"], pts)
    return {"pts": pts, "out": out, "st": st, "err": err, "gated": ref.gate(pts, out, st)}


def gpu_params(pkg, p):
    return pkg.lk_params(p.win_width, p.win_height, p.max_level, p.max_count, p.epsilon, p.flags, p.min_eig_threshold,
                         p.min_disparity, p.max_disparity)


def run_pair(bm, pkg, left, right, pts, p):
    import torch

    k = dev(pts[None])
    c = torch.tensor([len(pts)], dtype=torch.int32, device="cuda:0")
    rp, st, er = bm.lk_stereo(dev(left), dev(right), k, c, gpu_params(pkg, p))
    return rp[0].cpu().numpy(), st[0].cpu().numpy(), er[0].cpu().numpy()


def check_pair(bm, pkg, left, right, pts, p=None, what=""):
    p = p or ref.params()
    rp, st, er = run_pair(bm, pkg, left, right, pts, p)
    wo, ws, we = ref.correspondences(left, right, pts, p)
    assert int((bits(rp) != bits(wo)).sum()) == 0, (what, "right_pts", np.nonzero((bits(rp) != bits(wo)).any(axis=1))[0][:8])
    assert int((st != ws).sum()) == 0, (what, "status", np.nonzero(st != ws)[0][:8])
    assert int((bits(er) != bits(we)).sum()) == 0, (what, "err", np.nonzero(bits(er) != bits(we))[0][:8])
    return rp, st, er


@pytest.mark.parametrize("w,h,last", PYRAMID_SIZES)
def test_pyramid_levels_and_derivatives(bm, golden, w, h, last):
    imgs = [noise_frame(w, h, s) for s in (1, 2, 3)]
    if (w, h) == (640, 480):
        imgs[1], imgs[2] = golden["rect_l"], golden["rect_r"]
    lv, dv = bm.lk_pyramid(dev(np.stack(imgs)))
    assert len(lv) == len(dv) == last + 1
    for i, im in enumerate(imgs):
        wl, wd = ref.pyramid(im)
        for k in range(last + 1):
            assert np.array_equal(lv[k][i].cpu().numpy(), wl[k]), (i, k, "level")
            assert np.array_equal(dv[k][i].cpu().numpy(), wd[k]), (i, k, "deriv")
    lv2, dv2 = bm.lk_pyramid(dev(imgs[0]), with_deriv=False, max_level=1)
    assert dv2 == [] and len(lv2) == min(last, 1) + 1 and np.array_equal(lv2[-1][0].cpu().numpy(), ref.pyramid(imgs[0])[0][len(lv2) - 1])


def test_golden_pair_grid(bm, pkg, golden, golden_ref):
    g = golden_ref
    rp, st, er = run_pair(bm, pkg, golden["rect_l"], golden["rect_r"], g["pts"], ref.params())
    assert int((bits(rp) != bits(g["out"])).sum()) == 0 and int((bits(er) != bits(g["err"])).sum()) == 0
    assert np.array_equal(st, g["gated"]) and st.sum() >= 100
    rp2, st2, er2 = run_pair(bm, pkg, golden["rect_l"], golden["rect_r"], g["pts"], ref.params(max_disparity=-1.0))
    assert np.array_equal(st2, g["st"]) and int((bits(rp2) != bits(g["out"])).sum()) == 0   # the raw tracker status


@pytest.mark.parametrize("max_level", [0, 5])
@pytest.mark.parametrize("max_count", [1, 30])
def test_golden_pair_levels_and_counts(bm, pkg, golden, max_level, max_count):
    pts = grid_points()[::3]
    check_pair(bm, pkg, golden["rect_l"], golden["rect_r"], pts, ref.params(max_level=max_level, max_count=max_count),
               (max_level, max_count))


def test_identical_images(bm, pkg, golden):
    pts = grid_points()
    rp, st, er = check_pair(bm, pkg, golden["rect_l"], golden["rect_l"], pts, ref.params(max_disparity=-1.0), "same")
    assert st.sum() >= 100 and np.array_equal(bits(rp[st == 1]), bits(pts[st == 1]))
    assert not check_pair(bm, pkg, golden["rect_l"], golden["rect_l"], pts, what="same gated")[1].any()


def test_pin_kit(bm, pkg):
    kit = np.load(KIT)
    rp, st, er = run_pair(bm, pkg, kit["left"], kit["right"], kit["points"], ref.params(max_disparity=-1.0))
    assert np.array_equal(bits(rp), bits(kit["track/right_pts"])) and np.array_equal(st, kit["track/status"])
    assert np.array_equal(bits(er), bits(kit["track/err"]))
    assert np.array_equal(run_pair(bm, pkg, kit["left"], kit["right"], kit["points"], ref.params())[1], kit["gated/status"])
    lv, dv = bm.lk_pyramid(dev(np.stack([kit["left"], kit["right"]])))
    for k in range(int(kit["levels"]) + 1):
        assert np.array_equal(lv[k][0].cpu().numpy(), kit[f"left/level{k}"]) and np.array_equal(lv[k][1].cpu().numpy(), kit[f"right/level{k}"])
        assert np.array_equal(dv[k][0].cpu().numpy(), kit[f"left/deriv{k}"])


@pytest.mark.parametrize("w,h", [(16, 4), (37, 11)])
def test_small_frames_corners_fractions_and_outside(bm, pkg, w, h):
    left, right = small_pair(w, h)
    pts = small_points(w, h)
    for thr, gate in ((1e-4, 128.0), (1e-7, -1.0)):
        rp, st, er = check_pair(bm, pkg, left, right, pts, ref.params(min_eig_threshold=thr, max_disparity=gate), (w, h, thr))
    assert st.any() and not st.all()
    check_pair(bm, pkg, noise_frame(w, h, 5), noise_frame(w, h, 6), pts, ref.params(min_eig_threshold=0.0, max_disparity=-1.0), "noise")


def test_batch_counts_cap_zero_one_leave_the_rest_alone(bm, pkg, golden):
    import torch

    L, R = golden["rect_l"], golden["rect_r"]
    pts = grid_points()[100:164]
    cap = len(pts)
    kp = np.stack([pts, pts[::-1], pts]).astype(np.float32)
    counts = [cap, 0, 1]
    rp = torch.full((3, cap, 2), -7.25, dtype=torch.float32, device="cuda:0")
    st = torch.full((3, cap), 77, dtype=torch.uint8, device="cuda:0")
    er = torch.full((3, cap), -3.5, dtype=torch.float32, device="cuda:0")
    bm.lk_stereo(dev(np.stack([L, R, L])), dev(np.stack([R, L, R])), dev(kp), torch.tensor(counts, dtype=torch.int32, device="cuda:0"),
                 right_pts=rp, status=st, err=er)
    rp, st, er = rp.cpu().numpy(), st.cpu().numpy(), er.cpu().numpy()
    pairs = [(L, R), (R, L), (L, R)]
    for i, k in enumerate(counts):
        wo, ws, we = ref.correspondences(pairs[i][0], pairs[i][1], kp[i, :k]) if k else (np.zeros((0, 2), np.float32),) * 3
        assert np.array_equal(bits(rp[i, :k]), bits(wo).reshape(-1, 2)) and np.array_equal(st[i, :k], np.asarray(ws, np.uint8).reshape(-1))
        assert np.array_equal(bits(er[i, :k]), bits(we).reshape(-1))
        assert (rp[i, k:] == -7.25).all() and (st[i, k:] == 77).all() and (er[i, k:] == -3.5).all()


def model_pair(pkg, **kw):
    mo = ref.make_model(**kw)
    mg = pkg.StereoModel()
    ctypes.memmove(ctypes.byref(mg), ctypes.byref(mo), ctypes.sizeof(mg))
    return mo, mg


def same_with_nans(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~np.isnan(a)], bits(b)[~np.isnan(b)])


def test_keypoints3d_lk_against_the_restatement(bm, pkg, golden_ref):
    import torch

    g = golden_ref
    n = len(g["pts"])
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda:0")
    for kw, lo, hi in (({}, 0.0, 0.0), ({"local": [0, 0, 1, 0.1, -1, 0, 0, 0.2, 0, -1, 0, 0.3], "cx_r": 322.0}, 0.5, 4.0)):
        mo, mg = model_pair(pkg, **kw)
        xyz = bm.keypoints3d_lk(dev(g["pts"][None]), dev(g["out"][None]), dev(g["gated"][None]), cnt, mg, lo, hi)[0].cpu().numpy()
        want = ref.keypoints3d(g["pts"], g["out"], g["gated"], mo, lo, hi)
        assert same_with_nans(xyz, want)
        assert np.isnan(want[g["gated"] == 0]).all() and np.isfinite(want).all(axis=1).sum() >= 20
    raw = bm.keypoints3d_lk(dev(g["pts"][None]), dev(g["out"][None]), dev(g["st"][None]), cnt, mg, lo, hi)[0].cpu().numpy()
    assert same_with_nans(raw, ref.keypoints3d(g["pts"], g["out"], g["st"], mo, lo, hi))   # negative and zero disparities too


def test_keypoints3d_lk_equals_keypoints3d_on_a_constant_map(bm, pkg):
    import torch

    mo, mg = model_pair(pkg, local=[0, 0, 1, 0.1, -1, 0, 0, 0.2, 0, -1, 0, 0.3], cx_r=321.0)
    rng = np.random.default_rng(3)
    pts = np.stack([rng.integers(0, 640, 300), rng.integers(0, 480, 300)], axis=1).astype(np.float32)
    for d16 in (8, 167, 1000):
        disp = torch.full((480, 640), d16, dtype=torch.int16, device="cuda:0")
        rp = pts.copy()
        rp[:, 0] = pts[:, 0] - np.float32(d16 / 16.0)
        assert np.array_equal(pts[:, 0] - rp[:, 0], np.full(300, d16 / 16.0, np.float32))
        st = np.ones(300, np.uint8)
        a = bm.keypoints3d_lk(dev(pts[None]), dev(rp[None]), dev(st[None]), torch.tensor([300], dtype=torch.int32, device="cuda:0"), mg,
                              0.0, 0.0)[0].cpu().numpy()
        b = bm.keypoints3d(disp, dev(pts), mg, 0.0, 0.0).cpu().numpy()
        assert np.isfinite(b).all() and np.array_equal(bits(a), bits(b))


def test_chain_detect_track_depth_stays_on_the_device(bm, pkg, golden):
    L, R = golden["rect_l"], golden["rect_r"]
    dl, dr = dev(L), dev(R)
    kp, cn = bm.gftt_cv_detect(dl, maps=False)
    rp, st, er = bm.lk_stereo(dl, dr, kp, cn)
    mo, mg = model_pair(pkg)
    xyz = bm.keypoints3d_lk(kp, rp, st, cn, mg)
    want_k = gftt_cv_ref.detect(L)[0]
    k = int(cn[0])
    assert k == len(want_k) and k > 100
    wo, ws, we = ref.correspondences(L, R, want_k)
    assert np.array_equal(bits(rp[0, :k].cpu().numpy()), bits(wo)) and np.array_equal(st[0, :k].cpu().numpy(), ws)
    assert np.array_equal(bits(er[0, :k].cpu().numpy()), bits(we)) and ws.sum() > 20
    assert same_with_nans(xyz[0, :k].cpu().numpy(), ref.keypoints3d(want_k, wo, ws, mo))
    assert bool(torch_isnan_all(xyz[0, k:]))


def torch_isnan_all(t):
    import torch

    return torch.isnan(t).all()


def test_host_form_strided_and_error_codes(bm, pkg, golden, golden_ref):
    g = golden_ref
    wide_l = np.full((480, 701), 0x33, np.uint8)
    wide_r = np.full((480, 701), 0x44, np.uint8)
    wide_l[:, :640], wide_r[:, :640] = golden["rect_l"], golden["rect_r"]
    rp, st, er = bm.lk_stereo_host(wide_l[:, :640], wide_r[:, :640], g["pts"])
    assert np.array_equal(bits(rp), bits(g["out"])) and np.array_equal(st, g["gated"]) and np.array_equal(bits(er), bits(g["err"]))
    assert bm.lk_stereo_host(golden["rect_l"], golden["rect_r"], np.zeros((0, 2), np.float32))[0].shape == (0, 2)
    for kw, code in (({"flags": 0}, -23), ({"flags": 12}, -23), ({"win_width": 21}, -23), ({"win_width": 2}, -2), ({"max_level": -1}, -2)):
        with pytest.raises(pkg.StereoBMError) as e:
            bm.lk_stereo_host(golden["rect_l"], golden["rect_r"], g["pts"][:4], **kw)
        assert e.value.code == code, kw
    with pytest.raises(pkg.StereoBMError) as e:
        bm.lk_stereo_host(np.zeros((10, 2049), np.uint8), np.zeros((10, 2049), np.uint8), g["pts"][:4])
    assert e.value.code == -23
    with pytest.raises(pkg.StereoBMError) as e:
        bm.lk_stereo_host(np.zeros((1, 40), np.uint8), np.zeros((1, 40), np.uint8), g["pts"][:4])
    assert e.value.code == -2


def test_profile_records_stages(bm, golden, golden_ref):
    import torch

    bm.set_profiling(1)
    try:
        bm.lk_stereo(dev(golden["rect_l"]), dev(golden["rect_r"]), dev(golden_ref["pts"][None]),
                     torch.tensor([len(golden_ref["pts"])], dtype=torch.int32, device="cuda:0"))
        pr = bm.lk_profile()
    finally:
        bm.set_profiling(0)
    assert pr["lk_pyramid"] > 0 and pr["lk_track"] > 0 and abs(pr["lk_total"] - pr["lk_pyramid"] - pr["lk_track"]) < 1e-3


@pytest.mark.parametrize("mock", [False, True], ids=["plain", "mock_opencv"])
def test_cpp_callsite_through_the_adaptor(tmp_path, golden, golden_ref, mock):
    extra = ["-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv")] if mock else []
    exe, r = build_callsite(tmp_path, "lk_callsite_main.cpp", extra, flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr
    g = golden_ref
    (tmp_path / "l.raw").write_bytes(golden["rect_l"].tobytes())
    (tmp_path / "r.raw").write_bytes(golden["rect_r"].tobytes())
    (tmp_path / "p.raw").write_bytes(g["pts"].tobytes())
    stride = 640 if mock else 672
    r = subprocess.run([str(exe), str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), "640", "480", str(stride), str(tmp_path / "p.raw")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(g["pts"])
    got = np.array([[int(a, 16), int(b, 16)] for a, b, _ in rows], np.uint32)
    assert np.array_equal(got, bits(g["out"])) and np.array_equal(np.array([int(s) for _, _, s in rows], np.uint8), g["gated"])
    # a frame beyond the documented limit comes back as the documented code
    (tmp_path / "big.raw").write_bytes(bytes(2049 * 4))
    r = subprocess.run([str(exe), str(tmp_path / "big.raw"), str(tmp_path / "big.raw"), "2049", "4", "2049", str(tmp_path / "p.raw")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 4 and r.stdout.strip() == "error -23"
