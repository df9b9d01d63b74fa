"""What runs is what was planned: for a handful of tiny calls that between them reach the interior kernel's layouts <32,1>, <32,2>
(split), <64,1>, <128,2>, <64,3>, <128,3> (border columns from the sliding-sum kernel), a 1-column-sum window and the sliding-sum
kernel itself, one device call with the LR check and the speckle filter on equals the oracle's map, and the kernel it reports is
the one sbm_debug_plan names for the same parameters. The plan's own invariants are tests/test_bm_plan.py's (CPU)."""
import numpy as np
import pytest

import test_bm_plan as plan

# (W, H, nd, w, n) -> what the plan must say the call runs (checked: a tuning change that moves a case is told to move it back)
CASES = [
    ((96, 48, 16, 5, 1), "sad_fast_kernel<32,1,5,1,"),       # one wavefront, 1-column sums
    ((160, 48, 64, 21, 1), "sad_fast_kernel<32,2,7,3,"),     # split
    ((400, 128, 64, 21, 24), "sad_fast_kernel<64,1,7,3,"),
    ((400, 80, 160, 15, 32), "sad_fast_kernel<128,2,5,3,"),
    ((400, 40, 192, 15, 2), "sad_fast_kernel<64,3,5,3,"),
    ((640, 40, 272, 9, 1), "sad_fast_kernel<128,3,3,3,"),    # beyond 256 disparities: separate wide launches for the borders
    ((200, 80, 32, 33, 3), "sad_wide_kernel"),               # outside the envelope
]


@pytest.fixture(scope="module")
def ctx(pkg, oracle):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return pkg, oracle


@pytest.mark.gpu
@pytest.mark.parametrize("shape,want", CASES, ids=[w.split("kernel")[1] or "wide" for _, w in CASES])
def test_planned_kernel_runs_and_matches_the_oracle(ctx, shape, want):
    import torch

    from u96_slam_amd import synth

    pkg, oracle = ctx
    W, H, nd, w, n = shape
    c = dict(W=W, H=H, n=n, nd=nd, w=w, mind=0, roi=None, inplace=1, env={}, cap=31, uniq=10, tex=10, d12=1, spk_win=50, spk_range=32)
    st, pl = plan.query(pkg, c)
    assert st == 0
    plan.check_plan(c, pl)
    name = pl.kernel.decode()
    assert name.startswith(want), (name, want)
    if "<128,3," in want:
        assert pl.wide_borders and not pl.border
    if n >= 24:
        assert not pl.f.split

    L, R = synth.make_batch(0, min(n, 4), W, H, nd)
    L, R = np.concatenate([L] * (n // len(L))), np.concatenate([R] * (n // len(R)))
    assert len(L) == n
    bm = pkg.StereoBM.create(nd, w, device=0)
    bm.setPreFilterCap(31); bm.setTextureThreshold(10); bm.setUniquenessRatio(10)
    bm.setDisp12MaxDiff(1); bm.setSpeckleWindowSize(50); bm.setSpeckleRange(32)
    disp = bm.compute_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()).cpu().numpy()
    assert bm.last_kernel() == name
    p = oracle.make_params(nd, w, 31, 0, 10, 10, 50, 32, 1)
    for i in range(min(n, 4)):       # (the batch repeats its first four pairs)
        ref = oracle.compute(p, L[i], R[i])
        for j in range(i, n, 4):
            assert np.array_equal(disp[j], ref), (shape, j, int((disp[j] != ref).sum()))
