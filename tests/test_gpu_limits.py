"""The engine at and beyond every limit include/sbm.h documents ("Limits"), against the CPU oracle, bit-exact: rows wider than
the LR check's LDS claim table (8192 columns) under every LR reading and both cost-plane widths, the speckle filter's band walk
at its column limit (16-bit run indices) and its image-size limit ((W + 288) * H < 2^27) and the row-walking kernels just past
them, the height limit, the per-column SAD kernel up to 4096 disparities, the batch limit and block size 255. One step past each
limit the engine must answer SBM_ERR_UNSUPPORTED (-23) before any launch -- never a HIP error, never a wrong map."""
import pathlib
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
from gpu_support import torch_cuda  # noqa: E402,F401

UNSUPPORTED = -23


def smooth_pair(rng, h, w, shift, noise=3):
    """rand_pair (test_gpu_parity) without scipy: 3x3 box-smoothed random texture, right view shifted by `shift` columns plus
    per-pixel noise. Cheap enough for 10^8 pixels."""
    from u96_slam_amd import synth

    base = synth.box3(rng.integers(0, 256, (h, w + 64), dtype=np.uint8))
    L = np.ascontiguousarray(base[:, 32:32 + w])
    R = base[:, 32 + shift:32 + shift + w].astype(np.int16) + rng.integers(-noise, noise + 1, (h, w), dtype=np.int16)
    return L, np.clip(R, 0, 255).astype(np.uint8)


def with_flat_band(L, R, x0, width=40):
    """a textureless band: filtered pixels (cost 0xffff in the 16-bit plane) inside the checked column range"""
    L = L.copy(); R = R.copy()
    L[..., x0:x0 + width] = 90; R[..., x0:x0 + width] = 90
    return L, R


def engine(pkg, kw):
    bm = pkg.StereoBM.create(kw.get("num_disparities", 64), kw.get("block_size", 21))
    setters = dict(prefilter_cap=bm.setPreFilterCap, min_disparity=bm.setMinDisparity, texture_threshold=bm.setTextureThreshold,
                   uniqueness_ratio=bm.setUniquenessRatio, speckle_window_size=bm.setSpeckleWindowSize,
                   speckle_range=bm.setSpeckleRange, disp12_max_diff=bm.setDisp12MaxDiff)
    for k, v in kw.items():
        if k in setters:
            setters[k](v)
    return bm


def staged(pkg, oracle, kw, L, R):
    """run_engine_device (one sbm_compute_device call, every stage fetched) with the oracle on its SIMD path where that holds"""
    from test_gpu_parity import run_engine_device

    with oracle.simd(oracle.simd_ok(oracle.make_params(**kw))):
        return run_engine_device(pkg, oracle, kw, L, R)


def final_map(torch, pkg, kw, L, R):
    bm = engine(pkg, kw)
    out = bm.compute_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()).cpu().numpy()
    return out, bm


def oracle_map(oracle, kw, L, R):
    p = oracle.make_params(**kw)
    with oracle.simd(oracle.simd_ok(p)):
        return oracle.compute(p, L, R)


def assert_map_equal(got, ref, what=""):
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{what}final disparity differs at {bad[:5].tolist()} ({len(bad)} px); first: engine " \
                          f"{int(got[tuple(bad[0])])}, oracle {int(ref[tuple(bad[0])])}"


def assert_status(torch, pkg, kw, n, h, w, want):
    from u96_slam_amd.stereobm import StereoBMError

    z = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(StereoBMError) as e:
        engine(pkg, kw).compute_device(z, z)
    assert e.value.code == want, str(e.value)


# ---- the generic LR kernel on rows wider than its LDS claim table (8192 columns x 8 B = 64 KiB) --------------------------------
WIDE = [8192, 8193, 12000, 16384, 20480, 20481, 32768, 65535]


@pytest.mark.parametrize("w", WIDE)
def test_lr_check_wide_rows(torch_cuda, pkg, oracle, w):
    """Pre-LR map, cost plane and final map against the oracle, LR check on (speckle off: the final map is the LR kernel's)."""
    k = WIDE.index(w)
    h, nd, wsz, tol = 24 + 2 * k, (32, 64)[k % 2], (5, 9)[(k // 2) % 2], (k + k // 4) % 2
    rng = np.random.default_rng(w)
    L, R = with_flat_band(*smooth_pair(rng, h, w, shift=7, noise=4), w // 3)
    kw = dict(num_disparities=nd, block_size=wsz, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=tol)
    eng, ref = staged(pkg, oracle, kw, L[None], R[None])
    from test_gpu_parity import assert_stages_equal

    assert_stages_equal(eng, ref, kw)
    assert (ref["pre_lr"] != -16).mean() > 0.3 and (ref["disp"] != ref["pre_lr"]).any()   # (the check has work to do)


@pytest.mark.parametrize("w", [8193, 20481, 65535])
@pytest.mark.parametrize("variant", ["cost_short", "tie_later", "cost32"])
def test_lr_check_wide_rows_readings(torch_cuda, pkg, oracle, variant, w, monkeypatch):
    """The same beyond 8192 columns under SBM_CV_READING=2 (cost plane read as `short`) and =16 (the key stores W-1-x; equal costs
    -> the later x wins), each against the oracle under the same reading, and with block size 33 (sliding-sum SAD kernel: 32-bit
    cost plane)."""
    from test_gpu_parity import assert_stages_equal

    mask = dict(cost_short=2, tie_later=16, cost32=0)[variant]
    h = 28
    rng = np.random.default_rng(w + mask)
    L, R = with_flat_band(*smooth_pair(rng, h if variant != "cost32" else 48, w, shift=6, noise=4), w // 2)
    kw = dict(num_disparities=32, block_size=33 if variant == "cost32" else 9, texture_threshold=10, uniqueness_ratio=10,
              disp12_max_diff=1)
    monkeypatch.setenv("SBM_CV_READING", str(mask))
    with oracle.reading(mask):
        eng, ref = staged(pkg, oracle, kw, L[None], R[None])
    assert_stages_equal(eng, ref, kw)
    assert (ref["disp"] != ref["pre_lr"]).any()
    bm = engine(pkg, kw)
    bm.compute(L[:48], R[:48])
    assert bm.last_kernel().startswith("sad_wide_kernel" if variant == "cost32" else "sad_fast_kernel<"), bm.last_kernel()


# ---- speckle filter: band walk up to 65 535 columns (16-bit run indices), row-walking kernels beyond ------------------------------
@pytest.mark.parametrize("w", [65535, 65536, 70000])
@pytest.mark.parametrize("content", ["smooth", "noise"])
def test_speckle_column_limit(torch_cuda, pkg, oracle, content, w, monkeypatch):
    """Speckle and LR on, whole map against the oracle, with the default dispatch and with the row-walking kernels forced
    (SBM_SPECKLE_BAND=0). `noise`: uncorrelated images, speckleRange 0, window 3 -- about one run per pixel, so a row of 65 535
    columns fills the 16-bit run indices."""
    from u96_slam_amd import synth

    if content == "smooth":
        h = 48
        L, R = synth.make_batch(300, 1, w, h, 32)
        kw = dict(num_disparities=32, block_size=9, texture_threshold=10, uniqueness_ratio=10, speckle_window_size=50,
                  speckle_range=32, disp12_max_diff=1)
    else:
        h = 32
        rng = np.random.default_rng(w)
        L = rng.integers(0, 256, (1, h, w), dtype=np.uint8)
        R = rng.integers(0, 256, (1, h, w), dtype=np.uint8)
        kw = dict(num_disparities=32, block_size=5, texture_threshold=0, uniqueness_ratio=0, speckle_window_size=3,
                  speckle_range=0, disp12_max_diff=1)
    ref = oracle_map(oracle, kw, L[0], R[0])
    for band in (None, "0"):
        if band is None:
            monkeypatch.delenv("SBM_SPECKLE_BAND", raising=False)
        else:
            monkeypatch.setenv("SBM_SPECKLE_BAND", band)
        got, _ = final_map(torch_cuda, pkg, kw, L, R)
        assert_map_equal(got[0], ref, f"SBM_SPECKLE_BAND={band}: ")
    nosp = oracle_map(oracle, dict(kw, speckle_window_size=0, speckle_range=0), L[0], R[0])
    assert (nosp != ref).sum() > (100 if content == "smooth" else w)   # (the filter removes something; noise: many speckles)


# ---- speckle band walk while (W + 288) * H < 2^27, and the height limit ------------------------------------------------------
@pytest.mark.parametrize("w", [1760, 1761])
def test_tallest_images(torch_cuda, pkg, oracle, w):
    """65 535 rows: (1760 + 288) * 65535 is just below 2^27 (band walk), 1761 just above (row-walking kernels). Speckle and LR on,
    whole map against the oracle; the lower half of the right view is noisy, so speckles exist."""
    h = 65535
    rng = np.random.default_rng(w)
    L, R = smooth_pair(rng, h, w, shift=5, noise=2)
    R[h // 2:] = np.clip(R[h // 2:].astype(np.int16) + rng.integers(-40, 41, (h - h // 2, w), dtype=np.int16), 0, 255).astype(np.uint8)
    kw = dict(num_disparities=16, block_size=5, texture_threshold=10, uniqueness_ratio=10, speckle_window_size=50,
              speckle_range=32, disp12_max_diff=1)
    got, _ = final_map(torch_cuda, pkg, kw, L[None], R[None])
    ref = oracle_map(oracle, kw, L, R)
    assert_map_equal(got[0], ref)
    assert (ref >= 0).mean() > 0.3


def test_height_limit(torch_cuda, pkg, oracle):
    kw = dict(num_disparities=16, block_size=5)
    assert oracle.compute_status(oracle.make_params(**kw), 64, 65536) == 0   # cv::StereoBM accepts it; this engine does not
    assert_status(torch_cuda, pkg, kw, 1, 65536, 64, UNSUPPORTED)


# ---- beyond the sliding-sum kernel's 2048 disparities: the per-column kernel, up to 4096 --------------------------------------
@pytest.mark.parametrize("lr", [-1, 1])
@pytest.mark.parametrize("nd,w", [(2064, 2300), (4096, 4200)])
def test_per_column_kernel_disparity_limit(torch_cuda, pkg, oracle, nd, w, lr):
    from test_gpu_parity import assert_stages_equal

    rng = np.random.default_rng(nd)
    L, R = with_flat_band(*smooth_pair(rng, 24, w, shift=7, noise=3), nd + 20, 30)
    kw = dict(num_disparities=nd, block_size=7, texture_threshold=10, uniqueness_ratio=10, speckle_window_size=20,
              speckle_range=16, disp12_max_diff=lr)
    eng, ref = staged(pkg, oracle, kw, L[None], R[None])
    assert_stages_equal(eng, ref, kw)
    assert (ref["disp"] >= 0).sum() > 200
    bm = engine(pkg, kw)
    bm.compute(L, R)
    assert bm.last_kernel() == "sad_generic_kernel", bm.last_kernel()


def test_disparity_count_limit(torch_cuda, pkg, oracle):
    kw = dict(num_disparities=4112, block_size=7)
    assert oracle.compute_status(oracle.make_params(**kw), 4300, 24) == 0
    assert_status(torch_cuda, pkg, kw, 1, 24, 4300, UNSUPPORTED)


# ---- 32 767 pairs per call -----------------------------------------------------------------------------------------------------
def test_batch_limit(torch_cuda, pkg, oracle):
    """32 767 distinct 64x16 pairs in one sbm_compute_device call, every post-filter on, each map against the oracle (speckle
    scratch ~3.5 GB at this frame size)."""
    torch = torch_cuda
    from u96_slam_amd import synth

    n, h, w = 32767, 16, 64
    rng = np.random.default_rng(32767)
    T = synth.box3(rng.integers(0, 256, (n * h, w + 32), dtype=np.uint8)).reshape(n, h, w + 32)
    shift = 2 + np.arange(n) % 11                     # disparity of pair i: 2..12, so a pair computed from a neighbour's data shows
    L = np.ascontiguousarray(T[:, :, 16:16 + w])
    cols = 16 + shift[:, None, None] + np.arange(w)[None, None, :]
    R = np.take_along_axis(T, np.broadcast_to(cols, (n, h, w)), axis=2).astype(np.int16)
    R = np.clip(R + rng.integers(-3, 4, R.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    kw = dict(num_disparities=16, block_size=5, texture_threshold=10, uniqueness_ratio=10, speckle_window_size=8,
              speckle_range=16, disp12_max_diff=1)
    got, _ = final_map(torch, pkg, kw, L, R)
    p = oracle.make_params(**kw)
    with oracle.simd(oracle.simd_ok(p)):
        ref = oracle.compute_batch(p, L, R)
    assert_map_equal(got, ref)
    assert (ref >= 0).mean() > 0.2
    del got
    assert_status(torch, pkg, kw, 32768, h, w, UNSUPPORTED)


# ---- block size 255 ------------------------------------------------------------------------------------------------------------
def test_block_size_255(torch_cuda, pkg, oracle):
    from test_gpu_parity import assert_stages_equal

    rng = np.random.default_rng(255)
    L, R = with_flat_band(*smooth_pair(rng, 300, 700, shift=9, noise=6), 300, 60)
    kw = dict(num_disparities=64, block_size=255, prefilter_cap=63, texture_threshold=10, uniqueness_ratio=5,
              speckle_window_size=50, speckle_range=32, disp12_max_diff=1)
    eng, ref = staged(pkg, oracle, kw, L[None], R[None])
    assert_stages_equal(eng, ref, kw)
    assert (ref["disp"] >= 0).sum() > 1000
    bm = engine(pkg, kw)
    bm.compute(L, R)
    assert bm.last_kernel() == "sad_wide_kernel", bm.last_kernel()
    # blockSize < min(W, H): accepted at min = 256 (computed exactly), SBM_ERR_BLOCK_SIZE at 255 -- as the oracle says
    p = oracle.make_params(**kw)
    assert oracle.compute_status(p, 700, 256) == 0
    eng, ref = staged(pkg, oracle, kw, L[None, :256], R[None, :256])
    assert_stages_equal(eng, ref, kw)
    assert oracle.compute_status(p, 700, 255) == -6
    assert_status(torch_cuda, pkg, kw, 1, 255, 700, -6)
