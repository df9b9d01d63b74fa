"""The linked row-segment plan of the interior SAD kernel on the device (fast_linked_plan, csrc/sbm_sad_fast.hip): lengths that
fall towards the end of the launch, more and shorter segments, hand-off slots for the linked segments only. In every mode of
SBM_FAST_HANDOFF the map, the map before the LR check and the cost plane are bit-exact against the CPU oracle AND against mode 0
of the same engine; mode 2 takes every hand-off; two consecutive calls give equal maps. The images and the oracle's stages are
tests/test_gpu_sad_handoff.py's; the oracle runs once per case."""
import math

import numpy as np
import pytest

import test_bm_plan as plan
import test_gpu_sad_handoff as ho

# name -> (W, H, n, distinct pairs, nd, w, image kind)
CASES = {
    "x48_w15_nd128": (330, 96, 48, 4, 128, 15, "synth"),       # the existing hand-off shapes: ten / nine segments of 8 to 11 rows
    "x48_w21_nd64": (330, 96, 48, 4, 64, 21, "synth"),
    "reordered_nd128": (330, 280, 64, 4, 128, 15, "synth"),    # stride 13 < segments: the default mode links and reorders
    "reordered_ties_nd128": (330, 280, 64, 4, 128, 15, "ties"),   # the winner-search tags ride in the sums that are handed over
    "taper_to_zero": (330, 527, 48, 4, 128, 15, "synth"),      # the last position's share of the rows rounds to none: it drops out
}
LINKED = ("reordered_nd128", "reordered_ties_nd128", "taper_to_zero")


@pytest.fixture(scope="module")
def ctx(pkg, oracle):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dict(pkg=pkg, oracle=oracle, parity=ho._parity(), refs={})


def run(ctx, monkeypatch, mode, L, R, nd, w):
    """One engine: a call in mode 0, then two calls in `mode` (the second meets the first one's slots and flags)."""
    import torch

    bm = ctx["pkg"].StereoBM.create(nd, w, device=0)
    bm.setPreFilterCap(31); bm.setTextureThreshold(10); bm.setUniquenessRatio(10)
    bm.setDisp12MaxDiff(1); bm.setSpeckleWindowSize(50); bm.setSpeckleRange(32)
    n, h, wd = L.shape
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    outs = []
    for m in (0, mode, mode):
        monkeypatch.setenv("SBM_FAST_HANDOFF", str(m))
        d = bm.compute_device(dl, dr).cpu().numpy()
        outs.append(dict(disp=d, pre_lr=bm.debug_fetch(3, n, h, wd), cost=bm.debug_fetch(2, n, h, wd), counts=bm.debug_fetch(7).tolist()))
    return outs[0], outs[1:], bm.last_kernel()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_every_mode_matches_the_oracle_and_mode_0(ctx, monkeypatch, name, mode):
    W, H, n, distinct, nd, w, kind = CASES[name]
    monkeypatch.setenv("SBM_FAST_HANDOFF", str(mode))
    st, pl = plan.query(ctx["pkg"], ho.case_dict(W, H, n, nd, w))
    assert st == 0 and pl.fast and pl.f.NWAVES == 1 and pl.f.exact
    f = pl.f
    per_seg = n * f.strips
    rows = [f.segrow[k + 1] - f.segrow[k] for k in range(f.nseg)]
    assert min(rows) > 0 and sum(rows) == pl.g.row1 - pl.g.row0
    stride = -(-(4096 if nd <= 64 else 3072) // per_seg) + 1
    L, R, ref = ho.reference(ctx, name, W, H, n, nd, w, kind, distinct)
    base, outs, ran = run(ctx, monkeypatch, mode, L, R, nd, w)
    assert base["counts"] == [0, 0]
    assert ran == pl.kernel.decode()
    for o in outs:
        ctx["parity"].assert_stages_equal(o, ref, dict(ho.KW, num_disparities=nd, block_size=w))
        taken, could = o["counts"]
        print(f"{name} mode {mode}: nseg {f.nseg} stride {stride} rows {rows} took over {taken} of {could}")
        if mode == 0:
            assert (taken, could) == (0, 0)
        elif mode == 2:
            assert taken == could == (f.nseg - 1) * per_seg            # every hand-off is taken
        elif name in LINKED:
            assert stride < f.nseg and could == (f.nseg - stride) * per_seg and 0 <= taken <= could
        else:
            assert stride >= f.nseg and (taken, could) == (0, 0)
    for k in ("disp", "pre_lr", "cost"):
        assert np.array_equal(outs[0][k], outs[1][k]), k                  # two consecutive calls
    for k in ("disp", "pre_lr", "cost"):
        assert np.array_equal(outs[0][k], base[k]), k                     # mode 0 of the same engine
    if name == "taper_to_zero" and mode == 1:
        # the count of the documented model (kSegCLinked = 0.12, kHandoffRows = 0.7), less the position that got no row
        want = int(math.sqrt(0.12 * 3072 * sum(rows) / (per_seg * 0.7)) + 0.5)
        assert f.nseg == want - 1, (f.nseg, want)
