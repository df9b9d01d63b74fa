"""The CPU restatement of the LK stereo path (oracle/lk_stereo_ref) on its own: the C pyramid against the numpy transcription of
the header's RECALLED text, bit for bit; the properties the tracker must have on identical images; and every exit of the
tracker occurring on the golden pair, often enough that a comparison against the restatement means something."""
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import lk_stereo_ref as ref  # noqa: E402
from lk_cases import PYRAMID_SIZES, bits, grid_points, noise_frame, small_pair, small_points  # noqa: E402


@pytest.mark.parametrize("w,h,last", PYRAMID_SIZES)
def test_c_pyramid_equals_numpy_pyramid(w, h, last, golden):
    img = golden["rect_l"] if (w, h) == (640, 480) else noise_frame(w, h)
    lv, dv = ref.pyramid(img)
    nlv, ndv = ref.pyramid_np(img)
    assert len(lv) - 1 == last == ref.levels(w, h) and len(nlv) == len(lv) == len(dv) == len(ndv)
    for k in range(len(lv)):
        assert lv[k].shape == nlv[k].shape and np.array_equal(lv[k], nlv[k]), k
        assert dv[k].dtype == np.int16 and np.array_equal(dv[k], ndv[k]), k
    assert np.array_equal(lv[0], img)
    if (w, h) == (640, 480):
        assert lv[-1].shape == (15, 20)
    assert ref.pyramid(img, with_deriv=False)[1] == []


def test_max_level_caps_the_count():
    img = noise_frame(160, 120)
    for ml, last in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 3), (9, 3)):
        assert len(ref.pyramid(img, ref.params(max_level=ml))[0]) - 1 == last
        assert len(ref.pyramid_np(img, ref.params(max_level=ml))[0]) - 1 == last


def test_identical_images(golden):
    L = golden["rect_l"]
    pts = grid_points()
    out, st, err, info, _ = ref.track(L, L, pts)
    passed = info[:, 0] != ref.MIN_EIG
    inside = info[:, 0] != ref.PREV_OUT
    ok = passed & inside
    assert ok.sum() >= 100 and (~passed).sum() >= 50
    assert (st[ok] == 1).all() and (st[~ok] == 0).all()
    assert np.array_equal(bits(out[ok]), bits(pts[ok]))              # right == left exactly
    assert (info[ok, 0] == ref.CONVERGED).all() and (info[ok, 1] == 1).all()
    out2, st2, err2 = ref.correspondences(L, L, pts)                 # d = 0 <= 0.5: the gate clears everything
    assert not st2.any() and np.array_equal(bits(out2), bits(out)) and np.array_equal(bits(err2), bits(err))


def test_every_exit_occurs_on_the_golden_pair(golden):
    L, R = golden["rect_l"], golden["rect_r"]
    pts = grid_points()
    out, st, err, info, hist = ref.track(L, R, pts)
    why, iters = info[:, 0], info[:, 1]
    n = {k: int((why == k).sum()) for k in range(6)}
    tracked = int(st.sum())
    print("exits", n, "tracked", tracked)
    assert tracked == n[ref.CONVERGED] + n[ref.MAX_COUNT] + n[ref.OSCILLATION]
    assert tracked >= 100 and n[ref.MIN_EIG] >= 50 and n[ref.NEXT_OUT] >= 50
    assert n[ref.PREV_OUT] == 4 and (why[-4:] == ref.PREV_OUT).all() and (err[-4:] == 0).all()
    assert n[ref.MAX_COUNT] >= 1 and (iters[why == ref.MAX_COUNT] == 30).all()
    assert n[ref.OSCILLATION] >= 1 and (iters[why == ref.OSCILLATION] >= 2).all()
    assert n[ref.CONVERGED] >= 1
    assert hist.shape[0] == 6 and hist[0].sum() == len(pts) - n[ref.PREV_OUT] - n[ref.MIN_EIG]
    d = pts[:, 0] - out[:, 0]
    gated = ref.gate(pts, out, st)
    assert np.array_equal(gated, (st == 1) & (d > 0.5) & (d <= 128))
    assert 100 <= gated.sum() < tracked and 30 < np.median(d[gated == 1]) < 80
    out2, st2, err2 = ref.correspondences(L, R, pts)
    assert np.array_equal(st2, gated) and np.array_equal(bits(out2), bits(out)) and np.array_equal(bits(err2), bits(err))
    raw = ref.correspondences(L, R, pts, ref.params(max_disparity=-1.0))[1]
    assert np.array_equal(raw, st)


def test_clamps_of_max_count_and_epsilon(golden):
    L, R = golden["rect_l"], golden["rect_r"]
    pts = grid_points()[:200]
    o0 = ref.track(L, R, pts, ref.params(max_count=-3))
    o1 = ref.track(L, R, pts, ref.params(max_count=0))
    assert np.array_equal(bits(o0[0]), bits(o1[0])) and (o1[3][:, 1] == 0).all()
    a = ref.track(L, R, pts, ref.params(max_count=100))
    b = ref.track(L, R, pts, ref.params(max_count=1000))
    assert np.array_equal(bits(a[0]), bits(b[0])) and a[3][:, 1].max() == 100
    c = ref.track(L, R, pts, ref.params(epsilon=10.0))
    d = ref.track(L, R, pts, ref.params(epsilon=99.0))
    assert np.array_equal(bits(c[0]), bits(d[0]))


@pytest.mark.parametrize("w,h", [(16, 4), (37, 11)])
def test_small_frames_run_every_border_rule(w, h):
    left, right = small_pair(w, h)
    pts = small_points(w, h)
    out, st, err, info, _ = ref.track(left, right, pts, ref.params(min_eig_threshold=1e-7))
    assert (info[:, 0] == ref.PREV_OUT).sum() >= 6 and (info[:, 0] != ref.PREV_OUT).sum() >= 20
    assert np.isfinite(out).all() and st.any()


def test_keypoints3d_branches():
    m = ref.make_model(local=[1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 2.0])
    pts = np.array([(100, 50), (200, 60), (300, 70), (310, 80), (320, 90)], np.float32)
    rp = pts - np.array([(10, 0), (0, 0), (-3, 0), (2.5, 0), (40, 0)], np.float32)
    st = np.array([1, 1, 1, 0, 1], np.uint8)
    xyz = ref.keypoints3d(pts, rp, st, m)
    assert np.isfinite(xyz[0]).all() and np.isfinite(xyz[4]).all()
    assert np.isnan(xyz[1]).all() and np.isnan(xyz[2]).all() and np.isnan(xyz[3]).all()   # d = 0, d < 0, status 0
    z = 700.0 * 0.12 / 10.0
    assert abs(xyz[0, 2] - (z + 2.0)) < 1e-4
    assert np.isnan(ref.keypoints3d(pts, rp, st, m, 0.0, 5.0)[0]).all()                       # beyond max_depth
