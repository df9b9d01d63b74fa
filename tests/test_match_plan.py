"""The keypoint matcher's launch plan (sbm_match_plan, include/sbm.h) without a device: for every store capacity and the job
counts either side of each launch split, the slices tile the store, the launches tile the jobs, and one launch's scratch stays
within the 256 MiB the header promises with the full min(m, 64) jobs per launch -- which is why match_plan (sbm_match.hip) has
no scratch-budget clamp. The shapes tests/test_gpu_match_paths.py aims at are pinned here, so a retuned constant fails loudly
instead of silently moving those tests off their path."""
import ctypes

import numpy as np
import pytest

MS = list(range(1, 65)) + [65, 128, 129, 4097, 65535]
CAPS = 65535
FIELDS = ("qtiles", "nslice", "slice_rows", "jobs_per_launch", "launches", "proj_jobs_per_launch", "proj_launches", "pad")


@pytest.mark.parametrize("m", MS)
def test_every_capacity(pkg, m):
    L = pkg.load_library()
    plans = (pkg.MatchPlanInfo * CAPS)()
    size = ctypes.sizeof(pkg.MatchPlanInfo)
    assert size == 40
    call, base = L.sbm_match_plan, ctypes.addressof(plans)
    bad = [cap for cap in range(1, CAPS + 1) if call(cap, m, base + (cap - 1) * size, size) != 0]
    assert not bad, bad[:5]
    words = np.frombuffer(plans, np.int32).reshape(CAPS, 10)
    f = {k: words[:, i].astype(np.int64) for i, k in enumerate(FIELDS)}
    scratch = np.frombuffer(plans, np.int64).reshape(CAPS, 5)[:, 4]
    cap = np.arange(1, CAPS + 1, dtype=np.int64)
    assert np.all(f["qtiles"] == (cap + 63) // 64)
    assert np.all(f["slice_rows"] % 64 == 0) and np.all(f["slice_rows"] > 0)
    assert np.all((f["nslice"] - 1) * f["slice_rows"] < cap) and np.all(cap <= f["nslice"] * f["slice_rows"])
    assert np.all(f["nslice"] >= 1) and np.all(f["nslice"] <= 32)
    assert np.all(f["jobs_per_launch"] == min(m, 64))
    assert np.all(f["launches"] == -(-m // min(m, 64)))
    assert np.all(f["proj_jobs_per_launch"] == min(m, 32))
    assert np.all(f["proj_launches"] == -(-m // 32))
    assert np.all(scratch == f["jobs_per_launch"] * cap * (16 * f["nslice"] + 8))
    assert scratch.max() <= 256 << 20


def test_status_codes(pkg):
    L = pkg.load_library()
    pl = pkg.MatchPlanInfo()
    size = ctypes.sizeof(pl)
    call = lambda cap, m: L.sbm_match_plan(cap, m, ctypes.byref(pl), size)   # noqa: E731
    assert call(1, 1) == 0 and call(65535, 65535) == 0
    assert call(0, 1) == -2 and call(65536, 1) == -2 and call(-1, 1) == -2          # SBM_ERR_SIZE, as match_check
    assert call(1, 0) == -24 and call(1, -3) == -24                                  # SBM_ERR_BATCH
    assert call(1, 65536) == -23                                                     # SBM_ERR_UNSUPPORTED
    assert call(0, 0) == -24 and call(0, 65536) == -2                                # in match_check's order
    with pytest.raises(pkg.StereoBMError):
        pkg.match_plan(0, 1)
    with pytest.raises(pkg.StereoBMError):
        pkg.match_plan(1, 65536)


# (cap, m) -> (nslice, slice_rows): what tests/test_gpu_match_paths.py relies on
PINS = {(64, 1): (1, 64), (65, 1): (2, 64), (129, 1): (3, 64), (300, 1): (5, 64), (300, 65): (5, 64), (200, 130): (4, 64),
        (1500, 64): (6, 256), (2100, 1): (17, 128), (4096, 1): (32, 128), (65535, 1): (8, 8192), (65535, 30): (1, 65536)}


@pytest.mark.parametrize("shape", list(PINS), ids=[f"{c}x{m}" for c, m in PINS])
def test_pinned_shapes(pkg, shape):
    pl = pkg.match_plan(*shape)
    assert (pl.nslice, pl.slice_rows) == PINS[shape]


def test_the_largest_scratch_is_96_mib(pkg):
    pl = pkg.match_plan(65535, 64)
    assert (pl.nslice, pl.jobs_per_launch, pl.scratch_bytes) == (1, 64, 64 * 65535 * 24)
    assert pl.scratch_bytes <= 96 << 20
