"""The CPU restatement of the LK tracker (oracle/lk_stereo_ref.c, written from the text of include/sbm.h) against the reference's
OWN tracker, executed: calcOpticalFlowPyrLKStereo compiled from the reference tree into oracle/_ref/liblk_reference.so
(oracle/Makefile, oracle/lk_reference.py). Right points, status and err bit for bit -- floats compared as uint32, no mismatch
allowed. Both sides get the same pyramid (lk_stereo_ref.pyramid; it stays RECALLED), so this pins the tracker given the pyramid:
the cvRound tie rule, iw11 by subtraction, the 9- and 14-bit descales, the output written before a level is skipped, the
oscillation break, the clamps of the criteria -- and, because the reference reads real padded planes where the restatement
applies the border rule at the read, that the two are the same thing.

Where the library is missing AND there is no reference tree to build it from, the tests skip with that reason; with the tree
present a missing library is a failure."""
import pathlib
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import lk_reference  # noqa: E402
import lk_stereo_ref as ref  # noqa: E402
from lk_cases import (DEEP_SIZES, bits, bound_points, deep_pair, edge_points, grid_points, noise_frame, small_pair,  # noqa: E402
                      small_points, tie_points, weight_ties)

KIT = ROOT / "tests" / "golden" / "pin_kit_lk.npz"


@pytest.fixture(scope="module")
def reference():
    ok, why = lk_reference.available()
    if not ok:
        pytest.skip(why)
    lk_reference.lib()          # with a reference tree present, a library that cannot be built fails here
    return lk_reference


def same(reference, left, right, pts, p=None, what="", **kw):
    """The restatement's raw tracker outputs equal the reference's; returns the restatement's (out, status, err, info)."""
    p = p or ref.params()
    out, st, err, info, _ = ref.track(left, right, pts, p)
    wo, ws, we = reference.track(left, right, pts, p, **kw)
    bad = (bits(out) != bits(wo)).any(axis=1) | (st != ws) | (bits(err) != bits(we))
    assert not bad.any(), (what, int(bad.sum()), "of", len(bad), "points differ; first", np.nonzero(bad)[0][:8],
                           out[bad][:4], wo[bad][:4], st[bad][:4], ws[bad][:4], err[bad][:4], we[bad][:4])
    return out, st, err, info


def test_golden_pair_default_parameters_every_exit(reference, golden):
    out, st, err, info = same(reference, golden["rect_l"], golden["rect_r"], grid_points(), what="golden")
    assert sorted(set(info[:, 0].tolist())) == list(range(6)) and st.sum() >= 100       # all six exit classes were compared


@pytest.mark.parametrize("max_level", [0, 5])
@pytest.mark.parametrize("max_count", [1, 30])
def test_golden_pair_levels_and_counts(reference, golden, max_level, max_count):
    same(reference, golden["rect_l"], golden["rect_r"], grid_points(), ref.params(max_level=max_level, max_count=max_count),
         (max_level, max_count))


def test_identical_images(reference, golden):
    pts = grid_points()
    out, st, err, info = same(reference, golden["rect_l"], golden["rect_l"], pts, what="same")
    assert st.sum() >= 100 and np.array_equal(bits(out[st == 1]), bits(pts[st == 1]))


@pytest.mark.parametrize("w,h", [(16, 4), (37, 11)])
def test_small_frames_corners_fractions_and_outside(reference, w, h):
    left, right = small_pair(w, h)
    pts = small_points(w, h)
    for thr in (1e-4, 1e-7):
        out, st, err, info = same(reference, left, right, pts, ref.params(min_eig_threshold=thr), (w, h, thr))
    assert st.any() and not st.all()
    same(reference, noise_frame(w, h, 5), noise_frame(w, h, 6), pts, ref.params(min_eig_threshold=0.0), "noise")


def test_pin_kit_crop(reference):
    kit = np.load(KIT)
    out, st, err, info = same(reference, kit["left"], kit["right"], kit["points"], what="pin kit")
    assert np.array_equal(bits(out), bits(kit["track/right_pts"])) and np.array_equal(st, kit["track/status"])


@pytest.mark.parametrize("w,h,last", [(2048, 40, 3), (2048, 512, 7)])
def test_deep_pyramid(reference, w, h, last):
    """max_level 9 on 2048 columns: 40 rows end the pyramid at level 3, 512 rows keep level 7 (16 x 4)."""
    assert (w, h, last) in DEEP_SIZES
    left, right = deep_pair(w, h)
    p = ref.params(max_level=9)
    sizes = ref.level_sizes(w, h, p)
    assert len(sizes) - 1 == last == ref.levels(w, h, p) and (last != 7 or sizes[-1] == (16, 4))
    pts = np.concatenate([edge_points(w, h, last), bound_points(w, h, last), grid_points()[::7] * np.float32(w / 640.0)])
    pts[:, 1] = np.where(pts[:, 1] > 2 * h, pts[:, 1] * np.float32(h / 480.0), pts[:, 1])
    out, st, err, info = same(reference, left, right, pts, p, (w, h))
    assert st.sum() >= 10 and (st == 0).sum() >= 4
    good = st == 1
    assert (np.abs((pts[good, 0] - out[good, 0]) - 11.0) < 1.0).sum() >= 5       # the 11-column shift is found from the top down


@pytest.mark.parametrize("case", ["golden", "small", "noise"])
def test_window_start_exactly_on_each_bound(reference, golden, case):
    if case == "golden":
        left, right, w, h, last = golden["rect_l"], golden["rect_r"], 640, 480, 5
    elif case == "small":
        (left, right), w, h, last = small_pair(37, 11), 37, 11, 1
    else:
        left, right, w, h, last = noise_frame(160, 120, 8), noise_frame(160, 120, 9), 160, 120, 3
    assert ref.levels(w, h) == last
    pts = bound_points(w, h, last)
    out, st, err, info = same(reference, left, right, pts, ref.params(min_eig_threshold=0.0), case)
    # level 0's eight bounds: the kept side tracks or fails later, the skipped side is PREV_OUT (status 0, err 0)
    lvl0 = info[:16, 0].reshape(8, 2)
    assert (lvl0[[1, 3, 5, 7]] == ref.PREV_OUT).all() and (lvl0[[0, 2, 4, 6]] != ref.PREV_OUT).all()


def test_weight_ties_round_half_to_even(reference, golden):
    pts = tie_points()
    ties0 = weight_ties(pts, 0)
    assert ties0 >= 3 * (len(pts) - 9) and weight_ties(pts, 5) > ties0       # every grid point ties at level 0, some above it too
    out, st, err, info = same(reference, golden["rect_l"], golden["rect_r"], pts, ref.params(min_eig_threshold=0.0), "ties")
    assert st.sum() >= 100
    same(reference, noise_frame(640, 480, 21), noise_frame(640, 480, 22), pts, ref.params(min_eig_threshold=0.0, max_level=0), "ties noise")


@pytest.mark.parametrize("max_count", [-3, 0, 100, 1000])
def test_clamp_of_max_count(reference, golden, max_count):
    pts = grid_points()[:200]
    out, st, err, info = same(reference, golden["rect_l"], golden["rect_r"], pts, ref.params(max_count=max_count), max_count,
                              criteria_type=lk_reference.COUNT | lk_reference.EPS)
    assert info[:, 1].max() == min(max(max_count, 0), 100)


@pytest.mark.parametrize("epsilon", [10.0, 99.0])
def test_clamp_of_epsilon(reference, golden, epsilon):
    pts = grid_points()[:200]
    out, st, err, info = same(reference, golden["rect_l"], golden["rect_r"], pts, ref.params(epsilon=epsilon), epsilon,
                              criteria_type=lk_reference.COUNT | lk_reference.EPS)
    assert (info[:, 0] == ref.CONVERGED).sum() >= 50       # |delta| <= 10 ends nearly every point in its first iterations
