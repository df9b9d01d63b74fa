"""The sequential C restatement of generateKeypoints (oracle/gftt_cv_ref.c) against the independent numpy transcription
of include/sbm.h's text, bit for bit: maps as uint32 views, maxima, candidate counts and every keypoint in order, under reading 0
and under each reading bit. No GPU."""
import numpy as np
import pytest

from gftt_cv_cases import PARAM_EDGES, READINGS, crafted_frames, plateau_maps, random_case
import gftt_cv_ref as ref


@pytest.fixture(params=READINGS, ids=lambda r: f"reading{r}")
def reading(request):
    ref.set_reading(request.param)
    yield request.param
    ref.set_reading(0)


def same(img, mf=1500, q=0.01, md=7.0, what=""):
    pc, ec, mc, nc = ref.detect(img, mf, q, md)
    pn, en, mn, nn = ref.detect_np(img, mf, q, md)
    assert np.array_equal(ec.view(np.uint32), en.view(np.uint32)), (what, int((ec.view(np.uint32) != en.view(np.uint32)).sum()))
    assert np.float32(mc).view(np.uint32) == np.float32(mn).view(np.uint32), (what, mc, mn)
    assert nc == nn, (what, nc, nn)
    assert pc.shape == pn.shape and np.array_equal(pc, pn), (what, pc.shape, pn.shape)
    return pc, ec, mc, nc


def test_golden_frames(reading, golden):
    for k in ("rect_l", "rect_r"):
        p, e, m, nc = same(golden[k], what=k)
        print(k, reading, "candidates", nc, "keypoints", len(p), "max", m)
        assert 100 < len(p) < 1500 and nc > len(p)      # the trim works, the cap does not


def test_golden_frames_strided(reading, golden):
    wide = np.zeros((480, 700), np.uint8)
    wide[:, :640] = golden["rect_l"]
    p, e, m, nc = ref.detect(wide[:, :640])
    p2, e2, m2, nc2 = ref.detect(golden["rect_l"])
    assert np.array_equal(p, p2) and np.array_equal(e.view(np.uint32), e2.view(np.uint32))


@pytest.mark.parametrize("name", sorted(crafted_frames()))
def test_crafted_frames(reading, name):
    img = crafted_frames()[name]
    p, e, m, nc = same(img, what=name)
    if name == "constant":
        assert nc == 0 and len(p) == 0 and not e.any()
    if name == "tie_corners":
        srt = np.sort(e.ravel())[::-1]
        assert srt[0] == srt[1] and len(p) >= 2      # the two strongest responses tie exactly
        assert int(p[0, 0]) > int(p[1, 0]) and p[0, 1] == p[1, 1]   # the higher raster index first
    same(img, -1, 0.0, 0.0, name)
    same(img, 3, 0.5, 2.5, name)


@pytest.mark.parametrize("shape", [(3, 3), (3, 17), (17, 3), (3, 64), (4, 5)])
def test_small_frames(reading, shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for _ in range(5):
        img = rng.integers(0, 256, shape).astype(np.uint8)
        same(img, -1, 0.0, 0.0, shape)
        same(img, 1500, 0.01, 1.0, shape)


@pytest.mark.parametrize("mf,q,md", PARAM_EDGES)
def test_param_edges(reading, mf, q, md):
    frames = crafted_frames()
    for name in ("noise", "periodic", "tie_corners"):
        same(frames[name], mf, q, md, (name, mf, q, md))


def test_seeded_random_frames(reading):
    rng = np.random.default_rng(2024 + reading)
    for c in range(150):
        img, mf, q, md = random_case(rng)
        same(img, mf, q, md, f"case {c}: {img.shape} {mf} {q} {md}")


def test_noise_frame_hits_the_cap(reading):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (375, 1242)).astype(np.uint8)
    p, e, m, nc = ref.detect(img)
    assert len(p) == 1500 and nc > 10000


@pytest.mark.parametrize("name", sorted(plateau_maps()))
def test_map_level_selection(name):
    e, m = plateau_maps()[name]
    H, W = e.shape
    for mf, q, md in ((1500, 0.01, 7.0), (-1, 0.01, 0.0), (-1, 0.0, 2.5), (5, 0.5, 1.0)):
        pc, nc = ref.select(e, m, mf, q, md)
        pn, nn = ref.select_np(e, m, mf, q, md)
        assert nc == nn and np.array_equal(pc, pn), (name, mf, q, md)
        if name == "plateau":
            assert nc == (H - 2) * (W - 2)          # every interior pixel is a candidate
            if md == 0.0:
                assert len(pc) == nc and tuple(pc[0]) == (W - 2, H - 2) and tuple(pc[-1]) == (1, 1)
        if name == "zeros":
            assert nc == 0


@pytest.mark.parametrize("bit", [b for b in READINGS if b])
def test_every_reading_bit_changes_a_map(bit):
    """A bit that does nothing cannot pass: under each bit at least one crafted frame's map differs from reading 0's."""
    frames = crafted_frames()
    changed = []
    for name, img in frames.items():
        ref.set_reading(0)
        e0, _ = ref.eig_map(img)
        ref.set_reading(bit)
        e1, _ = ref.eig_map(img)
        ref.set_reading(0)
        if not np.array_equal(e0.view(np.uint32), e1.view(np.uint32)):
            changed.append(name)
    print(bit, changed)
    assert "noise" in changed


@pytest.mark.parametrize("md", [0.0, 1.0, 3.5, 7.0, 7.4])
def test_prefix_property(md):
    rng = np.random.default_rng(12)
    img = rng.integers(0, 256, (120, 160)).astype(np.uint8)
    full = ref.detect(img, -1, 0.001, md)[0]
    assert len(full) > 100
    for cap in (1, 63, 64, 65, 100, len(full)):
        assert np.array_equal(ref.detect(img, cap, 0.001, md)[0], full[:cap]), cap


def test_host_sqrtf_is_correctly_rounded():
    rng = np.random.default_rng(9)
    x = np.concatenate([rng.random(20000).astype(np.float32) ** 4,
                        np.abs(rng.integers(0, 1 << 31, 20000)).astype(np.uint32).view(np.float32),
                        np.array([0.0, 1e-45, 1.1754944e-38, 1.0, 2.0, 3.4e38, 0.25, 1.0 / 9.0], np.float32)])
    x = x[np.isfinite(x) & (x >= 0)]
    want = np.sqrt(x.astype(np.float64)).astype(np.float32)   # double's square root rounded to float is correctly rounded
    assert np.array_equal(np.sqrt(x).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ref.sqrtf(x).view(np.uint32), want.view(np.uint32))
