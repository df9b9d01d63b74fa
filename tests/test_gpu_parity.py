"""GPU parity: the HIP engine, called through its C-ABI (include/sbm.h), against the CPU oracle on the same
inputs. Bit-exact (int16 disparity, uint8 prefilter, int32 cost) -- integer path, tolerance 0.

The oracle is the checker only; nothing here routes the product through it."""
import pathlib

import numpy as np
import pytest

from gpu_support import build_callsite, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]


def run_engine(pkg, oracle, params_kw, L, R, stages=True):
    """Runs engine (host entry point) + oracle, returns (engine dict, oracle dict)."""
    bm = pkg.StereoBM.create(params_kw.get("num_disparities", 64), params_kw.get("block_size", 21))
    setters = dict(prefilter_cap=bm.setPreFilterCap, min_disparity=bm.setMinDisparity,
                   texture_threshold=bm.setTextureThreshold, uniqueness_ratio=bm.setUniquenessRatio,
                   speckle_window_size=bm.setSpeckleWindowSize, speckle_range=bm.setSpeckleRange,
                   disp12_max_diff=bm.setDisp12MaxDiff, roi1=bm.setROI1, roi2=bm.setROI2,
                   prefilter_type=bm.setPreFilterType, prefilter_size=bm.setPreFilterSize)
    for k, v in params_kw.items():
        if k in setters:
            setters[k](v)
    disp = bm.compute(L, R)
    h, w = L.shape[-2:]
    n = 1 if L.ndim == 2 else L.shape[0]
    eng = dict(disp=disp)
    if stages:
        eng["pf_l"] = bm.debug_fetch(0, n, h, w)
        eng["pf_r"] = bm.debug_fetch(1, n, h, w)
        eng["pre_lr"] = bm.debug_fetch(3, n, h, w)
        if params_kw.get("disp12_max_diff", -1) >= 0:
            eng["cost"] = bm.debug_fetch(2, n, h, w)
    p = oracle.make_params(**params_kw)
    refs = []
    L3 = L[None] if L.ndim == 2 else L
    R3 = R[None] if R.ndim == 2 else R
    for i in range(n):
        st, ref = oracle.compute(p, L3[i], R3[i], stages=True)
        assert st == 0
        refs.append(ref)
    ref = {k: np.stack([r[k] for r in refs]) for k in refs[0]}
    return eng, ref


def run_engine_device(pkg, oracle, params_kw, L, R):
    """The same through ONE device call (sbm_compute_device): the host entry point pipelines batches of 16 pairs or more in
    chunks, and the per-stage planes then belong to the last chunk only."""
    import torch

    bm = pkg.StereoBM.create(params_kw.get("num_disparities", 64), params_kw.get("block_size", 21))
    setters = dict(prefilter_cap=bm.setPreFilterCap, min_disparity=bm.setMinDisparity, texture_threshold=bm.setTextureThreshold,
                   uniqueness_ratio=bm.setUniquenessRatio, speckle_window_size=bm.setSpeckleWindowSize,
                   speckle_range=bm.setSpeckleRange, disp12_max_diff=bm.setDisp12MaxDiff, roi1=bm.setROI1, roi2=bm.setROI2)
    for k, v in params_kw.items():
        if k in setters:
            setters[k](v)
    n, h, w = L.shape
    dd = bm.compute_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    eng = dict(disp=dd.cpu().numpy(), pf_l=bm.debug_fetch(0, n, h, w), pf_r=bm.debug_fetch(1, n, h, w), pre_lr=bm.debug_fetch(3, n, h, w))
    if params_kw.get("disp12_max_diff", -1) >= 0:
        eng["cost"] = bm.debug_fetch(2, n, h, w)
    p = oracle.make_params(**params_kw)
    refs = [oracle.compute(p, L[i], R[i], stages=True)[1] for i in range(n)]
    return eng, {k: np.stack([r[k] for r in refs]) for k in refs[0]}


def assert_stages_equal(eng, ref, params_kw):
    n, h, w = ref["disp"].shape
    filtered = (params_kw.get("min_disparity", 0) - 1) * 16
    if "pf_l" in eng and ref["pre_lr"].max() > filtered:   # prefilter only runs when anything is computable
        assert np.array_equal(eng["pf_l"], ref["pf_l"]), "prefiltered left differs"
        assert np.array_equal(eng["pf_r"], ref["pf_r"]), "prefiltered right differs"
    if "pre_lr" in eng:
        e, r = eng["pre_lr"].copy(), ref["pre_lr"].copy()
        if params_kw.get("disp12_max_diff", -1) < 0:
            # without the LR check the clamped-window border columns cannot influence the output and the engine
            # does not compute them: compare the valid-ROI columns only
            import sbm_oracle
            full = (0, 0, w, h)
            r1 = params_kw.get("roi1", full); r2 = params_kw.get("roi2", full)
            x0, _, rw, _ = sbm_oracle.valid_roi(r1 if r1[2] > 0 else full, r2 if r2[2] > 0 else full,
                                                params_kw.get("min_disparity", 0), params_kw.get("num_disparities", 64),
                                                params_kw.get("block_size", 21))
            keep = np.zeros(w, bool)
            keep[max(x0, 0):max(x0 + rw, 0)] = True
            e[..., ~keep] = filtered
            r[..., ~keep] = filtered
        bad = np.argwhere(e != r)
        assert bad.size == 0, f"pre-LR disparity differs at {bad[:5].tolist()} ({len(bad)} px)"
    if "cost" in eng:
        valid = ref["pre_lr"] != filtered
        assert np.array_equal(eng["cost"][valid], ref["cost"][valid]), "WTA cost differs"
    d = eng["disp"].reshape(ref["disp"].shape)
    bad = np.argwhere(d != ref["disp"])
    assert bad.size == 0, f"final disparity differs at {bad[:5].tolist()} ({len(bad)} px)"


def rand_pair(rng, h, w, shift=5, noise=3):
    from scipy import ndimage

    base = rng.integers(0, 256, (h, w + 64), dtype=np.uint8)
    base = ndimage.uniform_filter(base.astype(np.float32), 3).astype(np.uint8)
    L = base[:, 32:32 + w]
    R = np.clip(base[:, 32 + shift:32 + shift + w].astype(int) + rng.integers(-noise, noise + 1, (h, w)), 0, 255)
    return np.ascontiguousarray(L), np.ascontiguousarray(R.astype(np.uint8))


SMALL_CASES = [
    # h, w, params
    (40, 64, dict(num_disparities=16, block_size=5, texture_threshold=10, uniqueness_ratio=15)),
    (37, 71, dict(num_disparities=32, block_size=9, texture_threshold=0, uniqueness_ratio=0)),
    (48, 80, dict(num_disparities=16, block_size=15, prefilter_cap=15, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1)),
    (33, 70, dict(num_disparities=16, block_size=7, min_disparity=-8, texture_threshold=5, uniqueness_ratio=10, disp12_max_diff=0)),
    (33, 70, dict(num_disparities=16, block_size=7, min_disparity=4, prefilter_cap=63, texture_threshold=5, uniqueness_ratio=10, disp12_max_diff=2)),
    (30, 90, dict(num_disparities=48, block_size=11, min_disparity=-60, texture_threshold=0, uniqueness_ratio=5, disp12_max_diff=1)),
    (45, 60, dict(num_disparities=32, block_size=21, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1,
                  speckle_window_size=20, speckle_range=16)),
    (64, 200, dict(num_disparities=64, block_size=9, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1,
                   speckle_window_size=50, speckle_range=32)),
    (75, 333, dict(num_disparities=128, block_size=15, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1,
                   speckle_window_size=50, speckle_range=32)),
    (61, 131, dict(num_disparities=48, block_size=13, texture_threshold=3, uniqueness_ratio=20, disp12_max_diff=1)),
    (50, 100, dict(num_disparities=16, block_size=33, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1)),
    (60, 120, dict(num_disparities=32, block_size=9, roi1=(10, 5, 100, 50), roi2=(4, 2, 110, 55), disp12_max_diff=1)),
    # fast-kernel envelope corners: disparity counts below the template size, minDisparity != 0, cap 63, windows 9..27
    (50, 150, dict(num_disparities=16, block_size=15, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1)),
    (47, 160, dict(num_disparities=48, block_size=9, texture_threshold=10, uniqueness_ratio=15, disp12_max_diff=1,
                   speckle_window_size=30, speckle_range=16)),
    (70, 260, dict(num_disparities=96, block_size=21, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1)),
    (80, 300, dict(num_disparities=112, block_size=27, texture_threshold=20, uniqueness_ratio=5, disp12_max_diff=2)),
    (55, 140, dict(num_disparities=32, block_size=9, min_disparity=-8, texture_threshold=5, uniqueness_ratio=10, disp12_max_diff=1)),
    (55, 140, dict(num_disparities=32, block_size=15, min_disparity=4, texture_threshold=5, uniqueness_ratio=10, disp12_max_diff=1)),
    (64, 180, dict(num_disparities=64, block_size=21, prefilter_cap=63, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1)),
    (64, 180, dict(num_disparities=64, block_size=15, prefilter_cap=5, texture_threshold=0, uniqueness_ratio=60, disp12_max_diff=1)),
    (64, 180, dict(num_disparities=64, block_size=15, texture_threshold=0, uniqueness_ratio=0, disp12_max_diff=0)),
    (40, 400, dict(num_disparities=128, block_size=9, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1)),
    # more than 128 disparities: four cooperating wavefronts per column strip (exact and masked disparity counts)
    (48, 520, dict(num_disparities=256, block_size=15, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1,
                   speckle_window_size=50, speckle_range=32)),
    (44, 430, dict(num_disparities=160, block_size=9, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1)),
    (70, 500, dict(num_disparities=208, block_size=21, min_disparity=-16, texture_threshold=10, uniqueness_ratio=15, disp12_max_diff=1)),
    (90, 470, dict(num_disparities=144, block_size=27, texture_threshold=0, uniqueness_ratio=0, disp12_max_diff=1)),
    (40, 330, dict(num_disparities=80, block_size=15, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1)),
    # windows that are not multiples of 3: 1-column vertical sums, w partners in the horizontal exchange
    (40, 200, dict(num_disparities=64, block_size=5, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1)),
    (44, 210, dict(num_disparities=32, block_size=7, texture_threshold=10, uniqueness_ratio=15, disp12_max_diff=1,
                   speckle_window_size=30, speckle_range=16)),
    (50, 300, dict(num_disparities=128, block_size=11, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1)),
    (52, 310, dict(num_disparities=96, block_size=13, min_disparity=-5, texture_threshold=5, uniqueness_ratio=10, disp12_max_diff=2)),
    (60, 420, dict(num_disparities=192, block_size=17, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1)),
    (66, 330, dict(num_disparities=64, block_size=19, prefilter_cap=63, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1)),
    (70, 350, dict(num_disparities=48, block_size=23, texture_threshold=0, uniqueness_ratio=0, disp12_max_diff=1)),
    (80, 560, dict(num_disparities=256, block_size=25, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1,
                   speckle_window_size=50, speckle_range=32)),
]


@pytest.mark.parametrize("h,w,kw", SMALL_CASES)
def test_small_random_cases(torch_cuda, pkg, oracle, h, w, kw):
    rng = np.random.default_rng(h * 131 + w)
    L, R = rand_pair(rng, h, w, shift=int(rng.integers(1, 9)))
    eng, ref = run_engine(pkg, oracle, kw, L, R)
    assert_stages_equal(eng, ref, kw)


@pytest.mark.parametrize("wsz", [9, 21])
def test_reference_pair_bit_exact(torch_cuda, pkg, oracle, golden, wsz):
    """data/ref_rect_{l,r} with the call-site parameters of src/slam/src/core/main.cpp:201-212 (blockSize 21) and
    BASELINE.json's configs[0] window (9)."""
    kw = dict(num_disparities=64, block_size=wsz, prefilter_cap=31, texture_threshold=10, uniqueness_ratio=10,
              speckle_window_size=50, speckle_range=32, disp12_max_diff=1)
    eng, ref = run_engine(pkg, oracle, kw, golden["rect_l"], golden["rect_r"])
    assert_stages_equal(eng, ref, kw)
    if wsz == 21:
        assert int((eng["disp"] >= 0).sum()) == 124940
        # the engine's prefilter also satisfies the RTL-golden identity directly (reference-produced vector)
        assert np.array_equal(eng["pf_l"][0][1:-1, 1:-1], np.maximum(golden["xsbl_l"][1:-1, 1:-1].astype(int) - 1, 0))
        assert np.array_equal(eng["pf_r"][0][1:-1, 1:-1], np.maximum(golden["xsbl_r"][1:-1, 1:-1].astype(int) - 1, 0))


def test_kitti_shape_batch_bit_exact(torch_cuda, pkg, oracle):
    """BASELINE configs[1]: 1242x375, ndisp 128, 15x15, full post-filter chain, 3 synthetic pairs in one batch."""
    from u96_slam_amd import synth

    L, R = synth.make_batch(0, 3, 1242, 375, 128)
    kw = dict(num_disparities=128, block_size=15, prefilter_cap=31, texture_threshold=10, uniqueness_ratio=10,
              speckle_window_size=50, speckle_range=32, disp12_max_diff=1)
    eng, ref = run_engine(pkg, oracle, kw, L, R)
    assert_stages_equal(eng, ref, kw)
    assert (eng["disp"] >= 0).mean() > 0.3   # the synthetic scene is matchable


def test_full_hd_nd256_bit_exact(torch_cuda, pkg, oracle):
    """BASELINE configs[2] shape: 1920x1080, ndisp 256 (one pair; the oracle needs a few seconds)."""
    from u96_slam_amd import synth

    L, R = synth.make_pair(7, 1920, 1080, 256)
    kw = dict(num_disparities=256, block_size=21, prefilter_cap=31, texture_threshold=10, uniqueness_ratio=10,
              speckle_window_size=50, speckle_range=32, disp12_max_diff=1)
    eng, ref = run_engine(pkg, oracle, kw, L, R, stages=False)
    assert_stages_equal(eng, ref, kw)


@pytest.mark.parametrize("levels,wsz,nd", [(2, 15, 64), (3, 9, 32), (4, 21, 128), (2, 27, 64), (3, 15, 256), (2, 9, 176)])
def test_tie_heavy_images(torch_cuda, pkg, oracle, levels, wsz, nd):
    """Few grey levels and no texture/uniqueness rejection: SAD ties everywhere, so the 'first index wins' rule, the
    mirrored sub-pixel neighbours at d = 0 / nd-1 and the uniqueness bookkeeping are all exercised."""
    rng = np.random.default_rng(levels * 100 + wsz)
    h, w = 3 * wsz + 11, nd + 4 * wsz + 37
    L = (rng.integers(0, levels, (h, w)) * (255 // max(levels - 1, 1))).astype(np.uint8)
    L = np.repeat(np.repeat(L[::4, ::4], 4, 0), 4, 1)[:h, :w].copy()      # blocky: large exactly-equal regions
    R = np.roll(L, -3, axis=1)
    for uniq, tex in ((0, 0), (10, 0), (0, 10)):
        kw = dict(num_disparities=nd, block_size=wsz, texture_threshold=tex, uniqueness_ratio=uniq, disp12_max_diff=1,
                  speckle_window_size=10, speckle_range=8)
        eng, ref = run_engine(pkg, oracle, kw, L, R)
        assert_stages_equal(eng, ref, kw)


def test_device_entry_point_matches_host_entry_point(torch_cuda, pkg, oracle):
    torch = torch_cuda
    from u96_slam_amd import synth

    L, R = synth.make_batch(3, 4, 640, 200, 64)
    bm = pkg.StereoBM.create(64, 9)
    bm.setDisp12MaxDiff(1)
    bm.setSpeckleWindowSize(50)
    bm.setSpeckleRange(32)
    host = bm.compute(L, R)
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    dev = bm.compute(dl, dr)
    assert dev.is_cuda and dev.dtype == torch.int16
    assert np.array_equal(dev.cpu().numpy(), host)
    # strided host input (cv::Mat::step larger than the row)
    big = np.zeros((200, 700), np.uint8)
    big[:, :640] = L[0]
    one = bm.compute(big[:, :640], np.ascontiguousarray(R[0]))
    assert np.array_equal(one, host[0])
    # strided output (a cv::Mat ROI view): rows land at the caller's step, the padding is untouched
    obig = np.full((200, 700), 1234, np.int16)
    bm.compute(L[0], R[0], obig[:, 30:670])
    assert np.array_equal(obig[:, 30:670], host[0]) and (obig[:, :30] == 1234).all() and (obig[:, 670:] == 1234).all()
    # a dense batch large enough for the pipelined host path (chunks over copy / compute / copy streams), ragged last chunk
    L3, R3 = synth.make_batch(20, 5, 320, 96, 32)
    L3, R3 = np.concatenate([L3] * 4)[:19], np.concatenate([R3] * 4)[:19]
    bm3 = pkg.StereoBM.create(32, 9)
    bm3.setDisp12MaxDiff(1); bm3.setSpeckleWindowSize(30); bm3.setSpeckleRange(16)
    h3 = bm3.compute(L3, R3)
    d3 = bm3.compute(torch.from_numpy(L3).cuda(), torch.from_numpy(R3).cuda()).cpu().numpy()
    assert np.array_equal(h3, d3)
    for i in range(5, 19):
        assert np.array_equal(h3[i], h3[i % 5])
    # odd width (1-D copies of rows that are not multiples of 4 bytes), dense batch
    L2, R2 = synth.make_batch(9, 2, 333, 64, 32)
    bm2 = pkg.StereoBM.create(32, 9)
    h2 = bm2.compute(L2, R2)
    assert np.array_equal(h2, bm2.compute(torch.from_numpy(L2).cuda(), torch.from_numpy(R2).cuda()).cpu().numpy())


def test_degenerate_and_error_behaviour(torch_cuda, pkg, oracle):
    img = np.zeros((32, 40), np.uint8)
    bm = pkg.StereoBM.create(48, 5)          # disparity range does not fit: whole map FILTERED
    assert (bm.compute(img, img) == -16).all()
    bm = pkg.StereoBM.create(16, 9)
    flat = np.full((40, 64), 100, np.uint8)
    assert (bm.compute(flat, flat) == -16).all()     # textureless
    bm.setTextureThreshold(0)
    bm.setUniquenessRatio(0)
    d = bm.compute(flat, flat)                        # every SAD ties at 0 -> largest disparity wins
    assert (d[4:-4, 19:-4] == 15 * 16).all()
    for setter, val, code in (("setNumDisparities", 20, -7), ("setBlockSize", 4, -6), ("setBlockSize", 41, -6),
                              ("setPreFilterCap", 64, -5), ("setTextureThreshold", -1, -8),
                              ("setUniquenessRatio", -1, -9), ("setPreFilterType", 2, -3), ("setPreFilterSize", 8, -4)):
        bm2 = pkg.StereoBM.create(16, 9)
        getattr(bm2, setter)(val)
        with pytest.raises(pkg.StereoBMError) as e:
            bm2.compute(flat, flat)
        assert e.value.code == code
        assert oracle.compute_status(oracle.make_params(**{"num_disparities": 16, "block_size": 9,
                                                           {"setNumDisparities": "num_disparities", "setBlockSize": "block_size",
                                                            "setPreFilterCap": "prefilter_cap", "setTextureThreshold": "texture_threshold",
                                                            "setUniquenessRatio": "uniqueness_ratio", "setPreFilterType": "prefilter_type",
                                                            "setPreFilterSize": "prefilter_size"}[setter]: val}),
                                     64, 40) == code
    with pytest.raises(pkg.StereoBMError):
        bm.compute(flat, flat[:, :60])


def test_idempotent_and_deterministic(torch_cuda, pkg):
    """Size-independent properties at a bench-sized batch: same inputs -> same outputs across calls and across
    batch positions (pairs are independent)."""
    from u96_slam_amd import synth

    L, R = synth.make_batch(0, 2, 1242, 375, 128)
    L8 = np.concatenate([L, L, L, L])
    R8 = np.concatenate([R, R, R, R])
    bm = pkg.StereoBM.create(128, 15)
    bm.setDisp12MaxDiff(1)
    bm.setSpeckleWindowSize(50)
    bm.setSpeckleRange(32)
    a = bm.compute(L8, R8)
    b = bm.compute(L8, R8)
    assert np.array_equal(a, b)
    for i in range(2, 8):
        assert np.array_equal(a[i], a[i % 2])


def _same_floats(a, b):
    """bit-identical float32 arrays (NaN payloads aside: NaN must be at the same places)."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def test_float_disparity_is_exact_sixteenth(torch_cuda, pkg):
    """CV_32F output = int16 / 16 exactly (cv convertTo(CV_32F, 1./16)); odd element counts take the scalar tail."""
    torch = torch_cuda
    rng = np.random.default_rng(4)
    for shape in ((3, 37, 53), (61, 35), (2, 8, 16)):
        d = rng.integers(-32768, 32768, shape).astype(np.int16)
        bm = pkg.StereoBM.create(16, 9)
        got = bm.to_float(torch.from_numpy(d).cuda()).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, (d.astype(np.float64) / 16.0).astype(np.float32))


def test_map_consumers_bit_exact(torch_cuda, pkg, oracle):
    """decimation (SensorData.cpp:50-58), reprojection (Stereo.cpp:157-199, main.cpp:522-553) and
    keypoint depth (Stereo.cpp:53-117) on the device vs the restatement of the reference's own C++ expressions.
    Floating point: tolerance 0 (same operation order and types, no FMA contraction)."""
    torch = torch_cuda
    from u96_slam_amd import synth

    L, R = synth.make_batch(0, 2, 1242, 375, 128)
    bm = pkg.StereoBM.create(128, 15)
    bm.setDisp12MaxDiff(1)
    bm.setSpeckleWindowSize(50)
    bm.setSpeckleRange(32)
    disp = bm.compute(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    hd = disp.cpu().numpy()
    local = [0, 0, 1, 0.1, -1, 0, 0, 0.2, 0, -1, 0, 0.3]
    for mk in (dict(), dict(cx_r=600.5, local=local)):
        mo = oracle.make_model(**mk)
        mg = pkg.StereoModel()
        import ctypes
        ctypes.memmove(ctypes.byref(mg), ctypes.byref(mo), ctypes.sizeof(mg))
        dec = bm.decimate(disp, 4)
        assert dec.shape == (2, 93, 310)
        for i in range(2):
            assert np.array_equal(dec[i].cpu().numpy(), oracle.decimate(hd[i], 4))
        xyz = bm.reproject(dec, mg, scale=4).cpu().numpy()
        full = bm.reproject(disp[0], mg, scale=1, apply_local=False).cpu().numpy()
        for i in range(2):
            assert _same_floats(xyz[i], oracle.reproject(dec[i].cpu().numpy(), 4, mo))
        assert _same_floats(full, oracle.reproject(hd[0], 1, mo, apply_local=False))
        assert np.isfinite(full[..., 2]).mean() > 0.3 and np.nanmin(full[..., 2]) > 0
        rng = np.random.default_rng(4)
        kp = np.stack([rng.uniform(-3, 1245, 500), rng.uniform(-3, 378, 500)], 1).astype(np.float32)
        for mind, maxd in ((0.0, 0.0), (2.0, 30.0), (-1.0, 8.0)):
            got = bm.keypoints3d(disp[1], torch.from_numpy(kp).cuda(), mg, mind, maxd).cpu().numpy()
            assert _same_floats(got, oracle.keypoints3d(hd[1], kp, mo, mind, maxd))


def test_randomised_parameter_sweep(torch_cuda, pkg, oracle):
    """Seeded fuzz over the parameter space (fast, border and generic kernels; all post-filter combinations):
    every stage bit-exact against the oracle."""
    rng = np.random.default_rng(20261002)
    for it in range(40):
        wsz = int(rng.choice([5, 7, 9, 9, 11, 15, 15, 21, 21, 27]))
        nd = int(rng.choice([16, 32, 48, 64, 96, 128, 160, 256]))
        mind = int(rng.choice([0, 0, 0, -16, 5, -nd // 2]))
        h = int(rng.integers(wsz + 8, wsz + 60))
        w = int(rng.integers(max(nd + abs(mind), 0) + 2 * wsz + 8, max(nd + abs(mind), 0) + 2 * wsz + 220))
        kw = dict(num_disparities=nd, block_size=wsz, min_disparity=mind, prefilter_cap=int(rng.choice([31, 31, 15, 63, 1])),
                  texture_threshold=int(rng.choice([0, 10, 10, 200])), uniqueness_ratio=int(rng.choice([0, 5, 10, 15, 40])),
                  disp12_max_diff=int(rng.choice([-1, 0, 1, 1, 3])))
        if rng.random() < 0.6:
            kw.update(speckle_window_size=int(rng.choice([1, 10, 50, 200])), speckle_range=int(rng.choice([0, 4, 16, 32])))
        L, R = rand_pair(rng, h, w, shift=int(rng.integers(0, 12)), noise=int(rng.integers(0, 6)))
        if rng.random() < 0.3:   # coarse grey levels: many exact ties
            L = (L // 64 * 64).astype(np.uint8)
            R = (R // 64 * 64).astype(np.uint8)
        eng, ref = run_engine(pkg, oracle, kw, L, R)
        try:
            assert_stages_equal(eng, ref, kw)
        except AssertionError as e:
            raise AssertionError(f"iteration {it}: {h}x{w} {kw}: {e}")


def test_matcher_recreated_every_frame(torch_cuda, pkg, oracle):
    """The reference builds a new matcher per frame (main.cpp:201): destroyed handles are parked and re-armed, so changing
    parameters and sizes between incarnations must give the same results as fresh handles, and trim() must free them."""
    from u96_slam_amd import synth

    cases = [(320, 96, 32, 9), (320, 96, 32, 9), (333, 77, 64, 15), (320, 96, 48, 21), (640, 200, 64, 9), (320, 96, 32, 9)]
    for i, (W, H, nd, wsz) in enumerate(cases):
        L, R = synth.make_pair(40 + i, W, H, nd)
        bm = pkg.StereoBM.create(16, 9)
        bm.setBlockSize(wsz); bm.setNumDisparities(nd); bm.setTextureThreshold(10); bm.setUniquenessRatio(10)
        bm.setDisp12MaxDiff(1); bm.setSpeckleWindowSize(30); bm.setSpeckleRange(16)
        got = bm.compute(L, R)
        del bm
        p = oracle.make_params(num_disparities=nd, block_size=wsz, texture_threshold=10, uniqueness_ratio=10,
                               disp12_max_diff=1, speckle_window_size=30, speckle_range=16)
        assert np.array_equal(got, oracle.compute(p, L, R)), f"incarnation {i}"
        if i == 3:
            pkg.trim()
    pkg.trim()


def test_two_handles_interleaved_without_sync(torch_cuda, pkg, oracle):
    """Distinct handles own distinct streams and scratch: asynchronous launches on two of them, interleaved, must not
    disturb each other (include/sbm.h: 'distinct handles may be used concurrently')."""
    torch = torch_cuda
    from u96_slam_amd import synth

    cfgs = [(640, 200, 64, 9), (333, 120, 32, 15)]
    hs, ins, outs, refs = [], [], [], []
    for i, (W, H, nd, wsz) in enumerate(cfgs):
        L, R = synth.make_batch(60 + 4 * i, 4, W, H, nd)
        bm = pkg.StereoBM.create(nd, wsz)
        bm.setTextureThreshold(10); bm.setUniquenessRatio(10); bm.setDisp12MaxDiff(1)
        bm.setSpeckleWindowSize(30); bm.setSpeckleRange(16)
        dL, dR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
        hs.append(bm); ins.append((dL, dR)); outs.append(torch.empty((4, H, W), dtype=torch.int16, device="cuda"))
        p = oracle.make_params(num_disparities=nd, block_size=wsz, texture_threshold=10, uniqueness_ratio=10,
                               disp12_max_diff=1, speckle_window_size=30, speckle_range=16)
        refs.append(oracle.compute_batch(p, L, R))
    torch.cuda.synchronize()
    for _ in range(10):
        for bm, (dL, dR), o in zip(hs, ins, outs):
            bm.compute_device(dL, dR, o, sync=False)
    for bm in hs:
        bm.synchronize()
    for o, r in zip(outs, refs):
        assert np.array_equal(o.cpu().numpy(), r)


@pytest.mark.parametrize("h,w,kw", [
    (60, 150, dict(num_disparities=32, block_size=9, prefilter_type=0, prefilter_size=9, prefilter_cap=31, texture_threshold=10,
                   uniqueness_ratio=10, disp12_max_diff=1)),
    (47, 131, dict(num_disparities=16, block_size=15, prefilter_type=0, prefilter_size=5, prefilter_cap=63, texture_threshold=0,
                   uniqueness_ratio=5, disp12_max_diff=1, speckle_window_size=20, speckle_range=16)),
    (80, 260, dict(num_disparities=64, block_size=21, prefilter_type=0, prefilter_size=21, prefilter_cap=15, texture_threshold=10,
                   uniqueness_ratio=10, disp12_max_diff=1)),
    (33, 90, dict(num_disparities=16, block_size=7, prefilter_type=0, prefilter_size=41, prefilter_cap=31)),
    (40, 300, dict(num_disparities=128, block_size=11, prefilter_type=0, prefilter_size=255, prefilter_cap=31, disp12_max_diff=0)),
])
def test_normalized_response_prefilter(torch_cuda, pkg, oracle, h, w, kw):
    """PREFILTER_NORMALIZED_RESPONSE (cv prefilterNorm): every stage bit-exact against the oracle, batches included."""
    rng = np.random.default_rng(h * 1000 + w)
    pairs = [rand_pair(rng, h, w, shift=4, noise=3) for _ in range(3)]
    L = np.stack([p[0] for p in pairs]); R = np.stack([p[1] for p in pairs])
    bm = pkg.StereoBM.create(kw["num_disparities"], kw["block_size"])
    bm.setPreFilterType(pkg.PREFILTER_NORMALIZED_RESPONSE)
    bm.setPreFilterSize(kw["prefilter_size"])
    setters = dict(prefilter_cap=bm.setPreFilterCap, texture_threshold=bm.setTextureThreshold, uniqueness_ratio=bm.setUniquenessRatio,
                   speckle_window_size=bm.setSpeckleWindowSize, speckle_range=bm.setSpeckleRange, disp12_max_diff=bm.setDisp12MaxDiff)
    for k, v in kw.items():
        if k in setters:
            setters[k](v)
    got = bm.compute(L, R)
    pf_l, pf_r = bm.debug_fetch(0, 3, h, w), bm.debug_fetch(1, 3, h, w)
    p = oracle.make_params(**kw)
    for i in range(3):
        assert np.array_equal(pf_l[i], oracle.prefilter_norm(L[i], kw["prefilter_size"], kw["prefilter_cap"]))
        assert np.array_equal(pf_r[i], oracle.prefilter_norm(R[i], kw["prefilter_size"], kw["prefilter_cap"]))
        assert np.array_equal(got[i], oracle.compute(p, L[i], R[i]))


# ---- the C++ boundary, exercised the way the reference calls it -----------------------------------
def _build_callsite(tmp_path, pkg, extra=()):
    return build_callsite(tmp_path, "callsite_main.cpp", extra, exe="callsite_main", pkg=pkg)


@pytest.mark.gpu
def test_cpp_call_site_three_frames_matches_oracle(tmp_path, pkg, oracle, golden):
    """A C++ program with the main.cpp:197-217 shape (matcher re-created per frame, 11 setters, compute on host
    images) built against include/sbm_stereobm.hpp + libsbm_hip.so; its maps must equal the oracle's bit for bit."""
    import subprocess

    exe, r = _build_callsite(tmp_path, pkg)
    assert r.returncode == 0, r.stderr
    L0, R0 = golden["rect_l"], golden["rect_r"]
    frames_l = np.stack([L0, L0[::-1].copy(), np.roll(L0, 3, axis=1)])
    frames_r = np.stack([R0, R0[::-1].copy(), np.roll(R0, 3, axis=1)])
    (tmp_path / "l.raw").write_bytes(frames_l.tobytes())
    (tmp_path / "r.raw").write_bytes(frames_r.tobytes())
    run = subprocess.run([str(exe), "640", "480", "3", str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(tmp_path / "d.raw")],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    got = np.frombuffer((tmp_path / "d.raw").read_bytes(), np.int16).reshape(3, 480, 640)
    p = oracle.make_params(64, 21, 31, 0, 10, 10, 50, 32, 1)      # the parameters of main.cpp:204-212
    for i in range(3):
        ref = oracle.compute(p, frames_l[i], frames_r[i])
        assert np.array_equal(got[i], ref), (i, int((got[i] != ref).sum()))
    assert (got[0] >= 0).mean() > 0.3


@pytest.mark.gpu
def test_cpp_compute_async_two_frames_in_flight(tmp_path, pkg, oracle, golden):
    """The adaptor's opt-in computeAsync() / wait() pair (one matcher, two frames in flight, the destructor drains the rest):
    five frames, every map equal to the oracle's."""
    import subprocess

    exe, r = _build_callsite(tmp_path, pkg)
    assert r.returncode == 0, r.stderr
    L0, R0 = golden["rect_l"], golden["rect_r"]
    frames_l = np.stack([np.roll(L0, k, axis=1) for k in range(5)])
    frames_r = np.stack([np.roll(R0, k, axis=1) for k in range(5)])
    (tmp_path / "l.raw").write_bytes(frames_l.tobytes())
    (tmp_path / "r.raw").write_bytes(frames_r.tobytes())
    run = subprocess.run([str(exe), "640", "480", "5", str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(tmp_path / "d.raw"), "async"],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    got = np.frombuffer((tmp_path / "d.raw").read_bytes(), np.int16).reshape(5, 480, 640)
    p = oracle.make_params(64, 21, 31, 0, 10, 10, 50, 32, 1)
    for i in range(5):
        assert np.array_equal(got[i], oracle.compute(p, frames_l[i], frames_r[i])), i


@pytest.mark.gpu
def test_cpp_inputarray_overload_compiles_and_runs(tmp_path, pkg, oracle, golden):
    """The cv::InputArray / cv::OutputArray overload of sbm::StereoBM::compute -- what the INTEGRATION.md diff at
    main.cpp:201-215 relies on -- compiled and run: against the real OpenCV headers where a box has them, otherwise against
    tests/cpp/mock_opencv (a from-scratch mock of the few names involved; it proves that the adaptor's text compiles and
    works, it pins nothing about cv::StereoBM's arithmetic). Three frames through bm->compute(cv::Mat, cv::Mat, cv::Mat), a
    fixed-CV_32F destination, and parameter / size errors surfacing as cv::Exception; maps compared with the oracle."""
    import subprocess

    probe = subprocess.run(["g++", "-x", "c++", "-E", "-"], input="#include <opencv2/core.hpp>\n", capture_output=True, text=True)
    if probe.returncode == 0:
        extra = ("-DSBM_TEST_WITH_OPENCV", "-lopencv_core")
    else:
        extra = ("-DSBM_TEST_WITH_OPENCV", "-I", str(ROOT / "tests" / "cpp" / "mock_opencv"))
    exe, r = _build_callsite(tmp_path, pkg, extra=extra)
    assert r.returncode == 0, r.stderr
    L0, R0 = golden["rect_l"], golden["rect_r"]
    frames_l = np.stack([L0, L0[::-1].copy(), np.roll(L0, 3, axis=1)])
    frames_r = np.stack([R0, R0[::-1].copy(), np.roll(R0, 3, axis=1)])
    (tmp_path / "l.raw").write_bytes(frames_l.tobytes())
    (tmp_path / "r.raw").write_bytes(frames_r.tobytes())
    run = subprocess.run([str(exe), "640", "480", "3", str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(tmp_path / "d.raw")],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    got = np.frombuffer((tmp_path / "d.raw").read_bytes(), np.int16).reshape(3, 480, 640)
    p = oracle.make_params(64, 21, 31, 0, 10, 10, 50, 32, 1)
    for i in range(3):
        assert np.array_equal(got[i], oracle.compute(p, frames_l[i], frames_r[i])), i


@pytest.mark.gpu
def test_output_buffer_validation(pkg, torch_cuda):
    """A caller-supplied disparity buffer reaches the C-ABI as a raw pointer: wrong dtype / shape / device / layout must
    be refused before that."""
    torch = torch_cuda
    bm = pkg.StereoBM.create(32, 9)
    L = torch.zeros((2, 64, 160), dtype=torch.uint8, device="cuda:0")
    good = torch.empty((2, 64, 160), dtype=torch.int16, device="cuda:0")
    assert bm.compute_device(L, L, good) is good
    for bad in (torch.empty((2, 64, 160), dtype=torch.int32, device="cuda:0"), torch.empty((2, 64, 159), dtype=torch.int16, device="cuda:0"),
                torch.empty((2, 64, 160), dtype=torch.int16), torch.empty((2, 64, 320), dtype=torch.int16, device="cuda:0")[:, :, ::2]):
        with pytest.raises(pkg.StereoBMError):
            bm.compute_device(L, L, bad)
    Ln = np.zeros((64, 160), np.uint8)
    for bad in (np.empty((64, 160), np.int32), np.empty((63, 160), np.int16), np.empty((64, 320), np.int16)[:, ::2]):
        with pytest.raises(pkg.StereoBMError):
            bm.compute(Ln, Ln, bad)
    with pytest.raises(pkg.StereoBMError):
        bm.compute(Ln[::-1], Ln, None)          # negative row stride
    d = bm.compute_device(L, L, sync=False)      # async: the wrapper keeps the buffers alive until synchronize()
    bm.synchronize()
    assert d.shape == L.shape


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [(40, 4200, 64, 9, 2), (33, 5000, 128, 15, 1), (60, 4097, 32, 5, 3), (48, 4096, 64, 21, 2)])
def test_rows_wider_than_4096(pkg, oracle, cfg):
    """Rows at and beyond the 4096-column limit of the 16-bit LR kernel (the generic LR kernel takes over, with the 16-bit cost
    plane of the fast SAD kernels), with every post-filter on."""
    h, w, nd, wsz, n = cfg
    rng = np.random.default_rng(5)
    pairs = [rand_pair(rng, h, w, shift=7, noise=3) for _ in range(n)]
    L = np.stack([p[0] for p in pairs]); R = np.stack([p[1] for p in pairs])
    kw = dict(num_disparities=nd, block_size=wsz, texture_threshold=10, uniqueness_ratio=10, speckle_window_size=50,
              speckle_range=32, disp12_max_diff=1)
    eng, ref = run_engine(pkg, oracle, kw, L, R)
    assert_stages_equal(eng, ref, kw)
    assert (eng["disp"] >= 0).mean() > 0.3


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [
    # (H, W, nd, window, minDisparity, disp12MaxDiff, roi?): widths either side of the LR kernel's layout rules (two pixels per
    # thread up to 1280 columns in blocks of 64 / 128 threads and 1..5 iterations, four pixels beyond), tolerances from 0 to "passes
    # everything", both signs of minDisparity, ROIs that cut the checked column range
    (24, 129, 32, 9, 0, 1, False), (24, 639, 64, 9, 0, 0, False), (20, 640, 32, 15, -8, 1, False), (20, 641, 32, 9, 5, 3, True),
    (16, 1279, 48, 9, 0, 1, True), (16, 1280, 32, 9, -16, 2, False), (16, 1281, 32, 9, 0, 1, False), (26, 1537, 64, 15, 4, 0, True),
    (12, 2049, 32, 9, 0, 2000, False), (12, 3073, 32, 9, -4, 1, True), (12, 4096, 48, 9, 0, 1, False), (30, 322, 16, 5, 0, 100000, False),
])
def test_lr_check_layouts(pkg, oracle, cfg):
    """The left-right check on its own terms: pre-LR map, cost plane and final map against the oracle (speckle filter off, so the
    final map is the LR kernel's output) over the widths where its thread layout changes. Filtered pixels take part in the claim
    pass with the 0xffff cost the SAD kernels store for them: textureless bands make plenty of those."""
    h, w, nd, wsz, mind, tol, roi = cfg
    rng = np.random.default_rng(w * 7 + nd)
    L, R = rand_pair(rng, h, w, shift=max(3, min(nd - 4, 9)) + min(mind, 0), noise=4)
    L = L.copy(); R = R.copy()
    L[:, w // 3:w // 3 + 40] = 90; R[:, w // 3:w // 3 + 40] = 90      # a textureless band: filtered pixels inside checked ranges
    kw = dict(num_disparities=nd, block_size=wsz, min_disparity=mind, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=tol)
    if roi:
        kw["roi1"] = (w // 8, 1, w - w // 4, h - 2); kw["roi2"] = (w // 10, 0, w - w // 5, h - 1)
    eng, ref = run_engine_device(pkg, oracle, kw, L[None], R[None])
    assert_stages_equal(eng, ref, kw)
    assert (ref["pre_lr"] != (mind - 1) * 16).mean() > 0.1     # (the case exercises the check at all)
    assert tol >= 2000 or (ref["disp"] != ref["pre_lr"]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("cs3", ["1", "0"])
@pytest.mark.parametrize("cfg", [
    # (nd, window, H, interior columns, pairs): interior columns = W - nd - (window - 1) around the tiling of the interior
    # kernel -- triples of column-stride-3 strips cover 3 * (65 - window / 3) columns, plain strips 67 - window each
    (64, 15, 60, 180, 2), (64, 15, 60, 181, 1), (64, 15, 60, 179, 1), (64, 15, 60, 232, 1), (64, 15, 60, 233, 1),
    (64, 15, 60, 285, 1), (64, 15, 60, 360, 1), (64, 15, 60, 52, 1), (64, 15, 60, 1, 1), (128, 15, 50, 465, 2),
    (64, 21, 70, 174, 1), (64, 21, 70, 175, 1), (64, 21, 70, 267, 1), (32, 9, 40, 186, 2), (32, 9, 40, 187, 1),
    (64, 27, 80, 168, 1), (64, 27, 80, 250, 1), (96, 15, 48, 200, 1), (176, 9, 40, 400, 1), (256, 21, 70, 350, 1),
])
def test_interior_strip_tilings(pkg, oracle, cs3, cfg, monkeypatch):
    """Interior kernel on widths that put the end of the interior columns on, just before and just behind the boundaries of its
    strip tiling (column-stride-3 triples + plain remainder strips; SBM_FAST_CS3=0: plain strips only), windows 9 / 15 / 21 / 27,
    one and several cooperating disparity wavefronts, a masked disparity count: every stage against the oracle."""
    from u96_slam_amd import synth

    monkeypatch.setenv("SBM_FAST_CS3", cs3)
    nd, wsz, H, ncols, n = cfg
    W = ncols + nd + wsz - 1
    L, R = synth.make_batch(77, n, W, H, min(nd, 64))
    kw = dict(num_disparities=nd, block_size=wsz, texture_threshold=10, uniqueness_ratio=10, speckle_window_size=50,
              speckle_range=32, disp12_max_diff=1)
    eng, ref = run_engine(pkg, oracle, kw, L, R)
    assert_stages_equal(eng, ref, kw)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [
    # (nd, window, H, W, pairs, minDisparity): every lane layout of a border wavefront (sbm_sad_border_wave.h) --
    # 4 jobs of 16 lanes (nd <= 64), 2 of 32 (<= 128), 1 of 64 (<= 256); disparity counts that leave quads of a job idle;
    # batches that are not multiples of 8 x jobs pairs (partly filled and empty wavefronts, pair stride 8); both clamp
    # patterns of the window columns (minDisparity of either sign moves the left and the right clamp apart); windows from
    # 5 to 27; heights that give one short and many border row segments
    (64, 21, 480, 640, 2, 0), (64, 15, 133, 300, 3, 0), (32, 9, 97, 200, 3, 0), (32, 11, 64, 180, 1, 0),
    (48, 13, 77, 260, 2, 0), (16, 5, 50, 120, 4, 0), (64, 21, 90, 300, 37, 0), (128, 15, 70, 400, 19, 0),
    (256, 21, 66, 520, 9, 0), (192, 9, 48, 420, 11, 0), (112, 27, 88, 330, 5, 0), (80, 19, 60, 290, 33, 0),
    (144, 7, 45, 380, 3, 0), (64, 15, 61, 310, 9, -24), (64, 15, 61, 310, 9, 20), (128, 21, 72, 420, 4, -150),
    (32, 25, 75, 200, 17, 7), (16, 23, 70, 150, 70, -3),
])
def test_border_columns_inside_the_interior_launch(pkg, oracle, cfg):
    """The w/2 clamped-window columns on each side, computed by extra wavefronts of the interior SAD launch: pre-LR disparity
    and cost of those columns, and everything downstream (they only matter through the LR check), against the oracle."""
    from u96_slam_amd import synth

    nd, wsz, H, W, n, mind = cfg
    L, R = synth.make_batch(31, n, W, H, min(nd, 64))
    kw = dict(num_disparities=nd, block_size=wsz, min_disparity=mind, texture_threshold=10, uniqueness_ratio=10, speckle_window_size=50,
              speckle_range=32, disp12_max_diff=1)
    eng, ref = run_engine_device(pkg, oracle, kw, L, R)
    assert_stages_equal(eng, ref, kw)
    # the border columns themselves were compared: the oracle produces them, and some of them found a match
    filtered = (mind - 1) * 16
    lofs = max(nd - 1 + mind, 0)
    assert (ref["pre_lr"][..., lofs:lofs + wsz // 2] != filtered).any()


@pytest.mark.gpu
@pytest.mark.parametrize("band,seg", [("0", "0"), ("2", "1"), ("2", "2"), ("2", "4"), ("4", "1"), ("4", "2"), ("4", "4"), ("-1", "0")])
@pytest.mark.parametrize("shape", [(37, 70, 1), (130, 300, 2), (64, 257, 3), (375, 1242, 2), (201, 515, 40), (50, 64, 2), (61, 128, 3),
                                   (33, 1280, 1), (45, 320, 2), (30, 321, 2)])
def test_speckle_band_walk_variants(pkg, oracle, band, seg, shape, monkeypatch):
    """The speckle filter's band walk (runs + merge of 2/4 rows by the wavefronts of a workgroup, one column segment each;
    seam contacts unioned by a second kernel) against the oracle: every band height and segment count (and the automatic
    choice), heights that are not multiples of the band, widths that are not multiples of a chunk or a load group and widths
    that are (a run that reaches a segment's last column then ends behind the walk), widths that leave the last segment
    empty, components that cross many seams and segment edges, and a batch large enough for every automatic choice."""
    from u96_slam_amd import synth

    monkeypatch.setenv("SBM_SPECKLE_BAND", band)
    monkeypatch.setenv("SBM_SPECKLE_SEG", seg)
    H, W, n = shape
    nd = 32 if W < 400 else 64
    L, R = synth.make_batch(11, n, W, H, nd)
    kw = dict(num_disparities=nd, block_size=9, texture_threshold=10, uniqueness_ratio=5, speckle_window_size=60,
              speckle_range=16, disp12_max_diff=1)
    if n > 8:   # oracle on a few pairs of the batch only
        bm = pkg.StereoBM.create(nd, 9)
        bm.setTextureThreshold(10); bm.setUniquenessRatio(5); bm.setSpeckleWindowSize(60); bm.setSpeckleRange(16)
        bm.setDisp12MaxDiff(1)
        disp = bm.compute(L, R)
        p = oracle.make_params(**kw)
        for i in (0, n // 2, n - 1):
            assert np.array_equal(disp[i], oracle.compute(p, L[i], R[i])), f"pair {i}"
        return
    eng, ref = run_engine(pkg, oracle, kw, L, R)
    assert_stages_equal(eng, ref, kw)
    assert (eng["disp"] != eng["pre_lr"]).any()   # the post-filters removed something


@pytest.mark.gpu
@pytest.mark.parametrize("band,seg", [("2", "2"), ("2", "4"), ("4", "2"), ("4", "4"), ("4", "1")])
def test_speckle_band_walk_overflows_its_lds_table_with_segments(pkg, oracle, band, seg, monkeypatch):
    """More runs in a row of a column segment than the band walk's LDS table holds (128 at 4 rows per band, 256 at 2): the
    band is walked again with its records in memory, by every wavefront of the band, and the runs that cross a segment edge are
    joined by L2 atomics instead of LDS ones. speckleRange 0 on noise 1 100 columns wide: segments of 320 / 576 columns with a
    run per pixel nearly everywhere, next to rows that are cleared to one long invalid stretch (bands that do NOT overflow in
    the same workgroups)."""
    monkeypatch.setenv("SBM_SPECKLE_BAND", band)
    monkeypatch.setenv("SBM_SPECKLE_SEG", seg)
    rng = np.random.default_rng(7)
    L = rng.integers(0, 256, (2, 70, 1100), dtype=np.uint8)
    R = rng.integers(0, 256, (2, 70, 1100), dtype=np.uint8)
    L[:, 20:32] = 128; R[:, 20:32] = 128          # textureless rows: everything filtered, bands without a single run
    kw = dict(num_disparities=64, block_size=5, texture_threshold=5, uniqueness_ratio=0, speckle_window_size=4, speckle_range=0,
              disp12_max_diff=-1)
    eng, ref = run_engine(pkg, oracle, kw, L, R)
    assert_stages_equal(eng, ref, kw)
    runs = (eng["pre_lr"][0] >= 0).sum(axis=1)
    assert runs.max() > 4 * 256 * 0.5 and runs.min() == 0     # rows far beyond every table size, and rows without runs


@pytest.mark.gpu
@pytest.mark.parametrize("spw", [2047, 2048, 2049, 6000])
@pytest.mark.parametrize("wsz", [9, 21])
def test_speckle_windows_around_the_band_walk_limit(pkg, oracle, golden, spw, wsz):
    """maxSpeckleSize up to 2048 runs the band walk (its size marks need that bound, include/sbm.h), beyond it the row-walking
    kernels: components of thousands of pixels erased or kept exactly like the oracle on the reference's pair, five calls each
    (the size sums of a component that spans many bands are racing atomic adds)."""
    kw = dict(num_disparities=64, block_size=wsz, prefilter_cap=31, texture_threshold=10, uniqueness_ratio=10,
              speckle_window_size=spw, speckle_range=32, disp12_max_diff=1)
    p = oracle.make_params(**kw)
    ref = oracle.compute(p, golden["rect_l"], golden["rect_r"])
    pre = oracle.compute(oracle.make_params(**dict(kw, speckle_window_size=0)), golden["rect_l"], golden["rect_r"])
    assert int(((pre >= 0) & (ref < 0)).sum()) > spw      # the filter erased more than one window's worth: large components took part
    bm = pkg.StereoBM.create(64, wsz)
    bm.setTextureThreshold(10); bm.setUniquenessRatio(10); bm.setSpeckleWindowSize(spw); bm.setSpeckleRange(32); bm.setDisp12MaxDiff(1)
    for rep in range(5):
        got = bm.compute(golden["rect_l"], golden["rect_r"])
        assert np.array_equal(got, ref), (rep, int((got != ref).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("seg", ["1", "4"])
@pytest.mark.parametrize("lists,band", [("1", "-1"), ("1", "0"), ("1", "2"), ("1", "4"), ("0", "-1")])
def test_speckle_with_one_run_per_pixel(pkg, oracle, lists, band, seg, monkeypatch):
    """speckleRange 0 on a noisy map: adjacent valid pixels rarely agree, so nearly every pixel is its own run -- the
    worst case for the compact run-head lists of the speckle filter (up to W heads per row), in every kernel variant."""
    monkeypatch.setenv("SBM_SPECKLE_LISTS", lists)
    monkeypatch.setenv("SBM_SPECKLE_BAND", band)   # band walk (2/4 rows per wavefront), 0 = separate runs + merge kernels
    monkeypatch.setenv("SBM_SPECKLE_SEG", seg)     # column segments per band
    rng = np.random.default_rng(42)
    L = rng.integers(0, 256, (3, 96, 400), dtype=np.uint8)      # no correlation between the images: disparities are noise
    R = rng.integers(0, 256, (3, 96, 400), dtype=np.uint8)
    kw = dict(num_disparities=64, block_size=5, texture_threshold=0, uniqueness_ratio=0, speckle_window_size=3, speckle_range=0,
              disp12_max_diff=-1)
    eng, ref = run_engine(pkg, oracle, kw, L, R)
    assert_stages_equal(eng, ref, kw)
    valid = eng["disp"] >= 0
    assert valid.mean() > 0.01 and (eng["pre_lr"] >= 0).mean() > 0.3   # the filter had work and left something to compare
