"""The CPU restatement of computeDescriptor (oracle/orb_ref.c) held to its literal numpy transcription (orb_ref.py), and the
facts the restatement rests on: the derived taps, the rotated pattern's distance from every rounding boundary at -1 degree, the
border rule's edges."""
import math
import pathlib

import numpy as np
import pytest

import orb_ref as ref

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def pattern():
    return np.load(ROOT / "tests" / "golden" / "orb_pattern.npz")["pattern"]


def test_taps_are_derived_not_typed():
    k = ref.taps_np()
    assert k.tolist() == [18, 34, 49, 55, 49, 34, 18] and k.sum() == 257
    assert ref.taps().tolist() == k.tolist()
    # the row pass fits 16 bits exactly: 55 * 255 + (49 + 34 + 18) * 510
    assert 55 * 255 + (49 + 34 + 18) * 510 == 65535 == k.sum() * 255


def test_pattern_fixture(pattern):
    import hashlib

    assert pattern.shape == (512, 2) and pattern.dtype == np.int32
    assert pattern.min() >= -13 and pattern.max() <= 13
    want = (ROOT / "tests" / "golden" / "orb_pattern.sha256").read_text().split()[0]
    assert hashlib.sha256(pattern.tobytes()).hexdigest() == want


def test_fused_and_unfused_offsets_agree_at_minus_one_degree(pattern):
    ang = np.float32(-1.0) * np.float32(math.pi / 180.0)
    a, b = np.float32(math.cos(float(ang))), np.float32(math.sin(float(ang)))
    assert (a, b) == (np.float32(0.9998477), np.float32(-0.017452406))
    p = pattern.astype(np.float64)
    # unfused: each product rounded to float, then the difference; fused: one rounding of the exact expression (either order)
    xu = (pattern[:, 0].astype(np.float32) * a - pattern[:, 1].astype(np.float32) * b)
    yu = (pattern[:, 0].astype(np.float32) * b + pattern[:, 1].astype(np.float32) * a)
    xf1 = (p[:, 0] * float(a) - np.float32(pattern[:, 1].astype(np.float32) * b)).astype(np.float32)
    xf2 = (np.float32(pattern[:, 0].astype(np.float32) * a) - p[:, 1] * float(b)).astype(np.float32)
    yf1 = (p[:, 0] * float(b) + np.float32(pattern[:, 1].astype(np.float32) * a)).astype(np.float32)
    yf2 = (np.float32(pattern[:, 0].astype(np.float32) * b) + p[:, 1] * float(a)).astype(np.float32)
    exact_x, exact_y = p[:, 0] * float(a) - p[:, 1] * float(b), p[:, 0] * float(b) + p[:, 1] * float(a)
    margin = min(np.abs(np.abs(exact_x - np.floor(exact_x)) - 0.5).min(), np.abs(np.abs(exact_y - np.floor(exact_y)) - 0.5).min())
    assert margin > 0.27
    for x in (xf1, xf2):
        assert np.array_equal(np.rint(x), np.rint(xu))
    for y in (yf1, yf2):
        assert np.array_equal(np.rint(y), np.rint(yu))
    dx, dy = ref.offsets_np(pattern, -1.0)
    assert np.array_equal(dx, np.rint(xu)) and np.array_equal(dy, np.rint(yu))
    assert np.abs(dx).max() <= 18 and np.abs(dy).max() <= 18


def test_any_angle_keeps_samples_within_18_pixels():
    corners = np.array([[13, 13], [-13, 13], [13, -13], [-13, -13]] * 128, np.int32)
    for ang in np.linspace(-360, 360, 721):
        dx, dy = ref.offsets_np(corners, float(ang))
        assert np.abs(dx).max() <= 18 and np.abs(dy).max() <= 18


def _frames(rng):
    yield rng.integers(0, 256, (50, 61), dtype=np.uint8)
    yield np.full((40, 40), 255, np.uint8)                                  # saturation: 257 * 255 / 256 > 255
    yield (rng.integers(0, 2, (45, 70)) * 255).astype(np.uint8)              # hard edges
    yield np.tile(np.arange(77, dtype=np.uint8) * 3, (39, 1))               # ramps
    yield rng.integers(100, 104, (64, 64), dtype=np.uint8)                  # nearly flat: many equal comparisons


@pytest.mark.parametrize("half_up", [False, True], ids=["half_even", "half_up"])
def test_c_restatement_matches_numpy_transcription(pattern, half_up):
    rng = np.random.default_rng(1 + int(half_up))
    for img in _frames(rng):
        h, w = img.shape
        assert np.array_equal(ref.blur(img, half_up), ref.blur_np(img, half_up))
        for ang in (-1.0, 0.0, 33.3, -170.0):
            kp = np.stack([rng.uniform(-3, w + 3, 120), rng.uniform(-3, h + 3, 120)], 1).astype(np.float32)
            kp[::3] = np.round(kp[::3] * 2) / 2
            c = ref.describe(img, kp, pattern, angle=ang, half_up=half_up)
            n = ref.describe_np(img, kp, pattern, angle=ang, half_up=half_up)
            assert np.array_equal(c[0], n[0]) and np.array_equal(c[1], n[1]) and np.array_equal(c[2], n[2])


def test_readings_differ_only_on_odd_ties():
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (300, 300), dtype=np.uint8)
    a, b = ref.blur(img, False), ref.blur(img, True)
    diff = a != b
    assert (b[diff].astype(int) - a[diff].astype(int) == 1).all()
    assert ((a[diff] & 1) == 0).all()   # a tie q + 1/2 with q even: half to even stays on q, half up goes to q + 1


@pytest.mark.parametrize("w,h,x,y,kept", [
    (100, 80, 18.5, 40, False), (100, 80, 18.51, 40, True), (100, 80, 19, 40, True), (100, 80, 19.5, 40, True),
    (100, 80, 80, 40, True), (100, 80, 80.5, 40, True), (100, 80, 80.51, 40, False), (100, 80, 81, 40, False),
    (100, 80, 40, 18.5, False), (100, 80, 40, 60.5, True), (100, 80, 40, 61, False),
    (38, 80, 19, 40, False), (100, 38, 40, 19, False), (39, 39, 19, 19, True), (39, 39, 19.5, 19.5, False),
    (39, 39, 20, 19, False),
])
def test_border_rule_edges(pattern, w, h, x, y, kept):
    img = np.random.default_rng(0).integers(0, 256, (h, w), dtype=np.uint8)
    k, d, _ = ref.describe(img, np.array([[x, y]], np.float32), pattern)
    kn, dn, _ = ref.describe_np(img, np.array([[x, y]], np.float32), pattern)
    assert len(k) == int(kept) and np.array_equal(k, kn) and np.array_equal(d, dn)
