"""Holds the restatements of tests/frontend_cases.py to the C oracle on every input that tests/test_gpu_frontend_edges.py then
runs through the HIP kernels: bit for bit, NaN at the same places. The restatements are written from the reference's sources in
numpy and Python integers, the oracle in C by other hands at another time: where both agree on inputs chosen for what they do
to the arithmetic, the GPU tests have a reference that is not the oracle alone. Also asserts what the inputs are FOR: that the
disparity plane and the camera models reach a zero and a negative denominator, subnormal and overflowing conversions; that
the rectifier calibrations reach lw < 0 and lw == 0 and never leave int64; that the GFTT images reach every regime listed in
frontend_cases.GFTT_REGIMES."""
import functools

import numpy as np
import pytest

import frontend_cases as fc
from test_frontend import py_rect_point

MODELS = fc.models()
PLANES = fc.disparity_planes()


def omodel(oracle, m):
    return fc.fill_model(oracle.StereoModel(), m)


def assert_same(got, ref, what, behind=None):
    if not fc.same_floats(got, ref):
        d = fc.first_diffs(got, ref)
        pytest.fail(f"{what}: first differences at {d}" + (f", inputs {[behind(i) for i in d]}" if behind else ""))


# ---------------------------------------------------------------------------------------------------------- consumers ---------
def test_disparity_plane_layout():
    p = PLANES[0]
    assert np.array_equal(np.sort(p.ravel()), np.arange(-32768, 32768))
    assert (p[0] > 0).all() and (p[-1] > 0).all() and (p[:, 0] > 0).all() and (p[:, -1] > 0).all() and (p[:4, :4] > 0).all()
    for i in (1, 2):
        assert np.array_equal(np.sort(PLANES[i].ravel()), np.arange(-32768, 32768)) and not np.array_equal(PLANES[i], p)


@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("scale", fc.REPROJECT_SCALES)
def test_reproject_equals_oracle(oracle, name, scale):
    m = MODELS[name]
    for apply_local in ((True, False) if m["local"] is not None else (True,)):
        for i in range(3 if scale == 1 else 1):
            ref = oracle.reproject(PLANES[i], scale, omodel(oracle, m), apply_local)
            got = fc.reproject(PLANES[i], scale, m, apply_local)
            assert_same(got, ref, f"{name} scale {scale} local {apply_local} plane {i}", lambda j: int(PLANES[i][j[0], j[1]]))


def test_models_reach_their_regimes():
    """The figures the models were chosen for, from the restatement (plane 0, scale 1)."""
    p = PLANES[0]
    tiny = float(np.finfo(np.float32).tiny)
    sub = fc.reproject(p, 1, MODELS["subnormal"])
    nsub = int(((np.abs(sub) < tiny) & (sub != 0)).sum())
    assert nsub > 60000, nsub                                           # Wx, Wy, z of every positive disparity: subnormal
    over = fc.reproject(p, 1, MODELS["overflow_1e38"])
    share = np.isfinite(over[..., 2]).mean()
    assert 0.40 < share < 0.49, share                                   # part of the positive disparities overflow, part do not
    big = fc.reproject(p, 1, MODELS["overflow_1e36+local"])              # fx Wx overflows below 2.2 px only; the transform's
    assert np.isfinite(big[p >= 64]).all() and np.abs(big[p >= 64]).max() > 1e36     # sums stay finite above that
    ex = fc.reproject(p, 1, MODELS["cxr_lt_exact"])
    assert np.isnan(ex[p == 100]).all()                                 # disp + c == 0: W infinite, dropped
    assert (ex[(p > 0) & (p < 100)][:, 2] < 0).all() and (ex[p > 100][:, 2] > 0).all()   # negative below it
    assert (fc.reproject(p, 1, MODELS["baseline0"])[p > 0][:, 2] == 0).all()


@pytest.mark.parametrize("name", list(MODELS))
def test_keypoints3d_equals_oracle(oracle, name):
    m, kp, disp = MODELS[name], fc.keypoints(), PLANES[0]
    gates = fc.depth_gates(disp, kp, m)
    assert len(gates) == 6 or name.startswith("baseline0")
    for lo, hi in gates:
        for nk in fc.KEYPOINT_COUNTS:
            ref = oracle.keypoints3d(disp, kp[:nk], omodel(oracle, m), lo, hi)
            got = fc.keypoints3d(disp, kp[:nk], m, lo, hi)
            assert got.shape == (nk, 3)
            assert_same(got, ref, f"{name} gates ({lo}, {hi}) nk {nk}", lambda j: kp[j[0]].tolist())


def test_keypoint_edges_and_exact_gates():
    m, kp, disp = MODELS["kitti"], fc.keypoints(), PLANES[0]
    out = fc.keypoints3d(disp, kp, m)
    fin = np.isfinite(out).all(1)
    # (-0.5, y), (-0.999, -0.999): column / row 0 by truncation; (-1, y), (W, y), (x, H), every non-finite or huge one: NaN
    assert fin[0] and fin[1] and not fin[2] and fin[3] and not fin[4] and not fin[5] and not fin[6:20].any() and fin[20] and fin[21]
    (_, zmax), (_, zbelow), (zmin, _) = fc.depth_gates(disp, kp, m)[3:]
    z = fc.keypoints3d(disp, kp, m)[:, 2]
    hit = z == np.float32(zmax)
    assert hit.any()
    assert np.isfinite(fc.keypoints3d(disp, kp, m, 0.0, zmax)[hit]).all()          # z <= max_depth keeps an equal z
    assert np.isnan(fc.keypoints3d(disp, kp, m, 0.0, zbelow)[hit]).all()
    assert np.isnan(fc.keypoints3d(disp, kp, m, zmin, 0.0)[hit]).all()             # z > min_depth drops it


@pytest.mark.parametrize("scale", fc.DECIMATE_SCALES)
def test_decimate_equals_oracle(oracle, scale):
    for planes in fc.decimate_planes():
        got = fc.decimate(planes, scale)
        assert got.shape == (3, planes.shape[1] // scale, planes.shape[2] // scale)
        for i in range(3):
            assert np.array_equal(got[i], oracle.decimate(planes[i], scale))


def test_to_float_expectation_is_exact():
    """float32(float64(v) / 16) is v / 16 exactly: 16 bits of integer scaled by a power of two."""
    for d in fc.to_float_inputs():
        f = fc.to_float(d)
        assert f.dtype == np.float32 and np.array_equal(f.astype(np.float64) * 16, d.astype(np.float64))
    sizes = [d.size for d in fc.to_float_inputs()]
    assert sizes == [65536, 65537, 1, 2, 3]


# ---------------------------------------------------------------------------------------------------------- rectifier ---------
@functools.lru_cache(maxsize=None)
def rect_ref(name):
    return fc.rect_map(fc.rect_cams()[name])


@pytest.mark.parametrize("name", list(fc.rect_cams()))
def test_rect_map_equals_oracle(oracle, name):
    cam = fc.rect_cams()[name]
    m, lw, over = rect_ref(name)
    assert not over.any(), f"{name}: {int(over.sum())} pixels leave int64 (undefined in the firmware's C)"
    assert np.array_equal(m, oracle.rect_map(oracle.make_rect_cam(**cam), fc.RW, fc.RH))
    for y in range(0, fc.RH, 4):
        for x in range(fc.RW):
            assert list(m[y, x]) == py_rect_point(cam, x, y)


def test_rect_cams_reach_negative_and_zero_lw():
    cams = fc.rect_cams()
    assert len(cams) == 32
    lw = {n: rect_ref(n)[1] for n in cams}
    neg = {n: int((v < 0).sum()) for n, v in lw.items()}
    npix = fc.RW * fc.RH
    assert (lw["lw_zero"] == 0).all() and (lw["lw_minus1"] == -1).all()
    assert 0 < neg["rotx89"] < npix and 0 < neg["roty90"] < npix and 0 < neg["lw_is_xn"] < npix
    assert neg["rotx120"] == npix and neg["rotx180"] == npix and neg["roty180"] == npix and 0 < neg["roty120"] < npix
    assert neg["rotx0"] == neg["rotz180"] == neg["rotx60"] == 0
    row = lw["lw_is_xn"][0]
    assert row[0] < 0 < row[-1]
    # the undefined one stays out: rot[2][2] = 1 overflows on every pixel
    bad = dict(cams["lw_minus1"], rot=[[1 << 24, 0, 0], [0, 1 << 24, 0], [0, 0, 1]])
    assert fc.rect_map(bad)[2].all()


# ---------------------------------------------------------------------------------------------------------- resampler ---------
def test_remap_maps_cover_the_fast_path_boundary():
    maps = fc.remap_maps(40, 30)
    ent = {(int(x), int(y)) for m in maps for x, y in m.reshape(-1, 2)}
    for xi in (-2, -1, 0, 38, 39, 40):
        for yi in (-2, -1, 0, 28, 29, 30):
            for f in (0, 1, 31):
                assert (xi * 32 + f, yi * 32 + 31 - f) in ent
    assert (-32768, 32767) in ent and (32767, 0) in ent and (0, -32768) in ent
    assert len(fc.remap_maps(192, 192)) == 2 and fc.remap_maps(192, 192)[0].shape == (192, 192, 2)


@pytest.mark.parametrize("name", list(fc.remap_cases()))
def test_rect_remap_equals_oracle(oracle, name):
    src, maps = fc.remap_cases()[name]
    h, w = src.shape[-2:]
    for k, m in enumerate(maps):
        got = fc.rect_remap(src, m)
        for i, s in enumerate(src if src.ndim == 3 else [src]):
            g = got[i] if src.ndim == 3 else got
            assert np.array_equal(g, oracle.rect_remap(s, m)), (name, k, i)
            if k % 8 == 0 and i == 0:
                assert np.array_equal(g, fc.rect_remap_points(s, m)), (name, k)
        if name.endswith("all255"):
            assert (got[fc.fully_inside(m, w, h)] == 255).all()                    # the weights sum to 1024


# ---------------------------------------------------------------------------------------------------------- GFTT --------------
def test_gftt_eig_equals_oracle_and_reaches_every_regime(oracle):
    seen = {k: [] for k in fc.GFTT_REGIMES}
    count = 0
    for W, H in fc.GFTT_SIZES:
        for name, im in fc.gftt_images(W, H).items():
            g = fc.gftt_eig(im)
            ref, rmax = oracle.gftt_eig(im)
            assert np.array_equal(g["eig"], ref) and g["max"] == rmax, (W, H, name)
            count += 1
            for k, v in fc.gftt_regimes(g).items():
                if v and k in seen:
                    seen[k].append((W, H, name, v))
    assert count >= 19 * len(fc.GFTT_SIZES)
    distinct = {n for v in seen['float32 sqrt(s) * 32 truncates above the root, showing'] for n in v[2:3]}
    assert len(distinct) >= 4, distinct
    missing = [k for k, v in seen.items() if not v]
    assert not missing, missing
    # the images the module's docstring names for the two searched regimes
    assert any(n == "diag_blobs" for _, _, n, _ in seen["b at its limiter"])
    assert any(n == "step75_noise4" for _, _, n, _ in seen["a + c - r < 0"])
    # and what the issue measured: ramps are perfect squares below 1024, the 2 x 2 checkerboard sits at the cap
    g = fc.gftt_regimes(fc.gftt_eig(fc.gftt_images(130, 60)["ramp_x"]))
    assert g["s a non-zero perfect square"] + g["s == 0"] > 0.9 * 128 * 56
    g = fc.gftt_regimes(fc.gftt_eig(fc.gftt_images(130, 60)["checker2"]))
    assert g["s == 0x3fffff"] > 0.9 * 128 * 56


@pytest.mark.parametrize("W,H", fc.GFTT_NARROW)
def test_gftt_narrow_equals_oracle(oracle, W, H):
    rng = np.random.default_rng(W * 10 + H)
    for im in (rng.integers(0, 256, (H, W), dtype=np.uint8), (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8)):
        g = fc.gftt_eig(im)
        ref, rmax = oracle.gftt_eig(im)
        assert np.array_equal(g["eig"], ref) and g["max"] == rmax


@pytest.mark.parametrize("W,H,n,seg", fc.GFTT_BATCHES)
def test_gftt_batches_reach_their_segment_length(oracle, W, H, n, seg):
    assert fc.gftt_launch_seg(W, H, n) == seg and fc.gftt_launch_seg(W, H, 8) == 64
    assert W * H * n <= 20 * 1000 * 1000
    for im in fc.gftt_batch_frames(W, H):
        g = fc.gftt_eig(im)
        ref, rmax = oracle.gftt_eig(im)
        assert np.array_equal(g["eig"], ref) and g["max"] == rmax
