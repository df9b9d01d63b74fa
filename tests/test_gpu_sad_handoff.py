"""The interior SAD kernel hands its vertical sums from one row segment of a (pair, strip) to the next (sbm_sad_fast_strip.h):
the later segment loads what the earlier one left instead of recomputing it from w - 1 priming rows -- if it is there when the
segment starts; it never waits. Both ways give the same integers, so nothing here may depend on which one was taken.

SBM_FAST_HANDOFF (read per call) selects: 1 the default, opportunistic; 0 every segment primes; 2 the segments are launches of
their own, top to bottom, so that EVERY hand-off is taken -- the mode that tests the inherit path without relying on timing.
For each mode the map, the map before the LR check and the cost plane are bit-exact against the CPU oracle; sbm_debug_fetch(7)
reports (segments x pairs x strips that took their sums over, those that could have): all of them in mode 2, none in mode 0.
The oracle's maps are computed once per case and shared by the modes."""
import importlib.util
import pathlib

import numpy as np
import pytest

import test_bm_plan as plan

ROOT = pathlib.Path(__file__).resolve().parents[1]

# name -> (W, H, n, distinct pairs, nd, w, image kind, layout the plan must choose, takes part in the hand-off: the lone wavefronts
# of the exact kernels). Three pairs of 330 x 96 are a launch that does not fill the chip: it is split over cooperating
# wavefronts (except at 32 disparities), which always prime; 48 pairs (four different ones, repeated) reach the lone wavefronts.
CASES = {
    "w15_nd128": (330, 96, 3, 3, 128, 15, "synth", "sad_fast_kernel<64,2,5,3,true,", False),    # one stride-3 triple + a plain strip
    "w15_nd32": (330, 96, 3, 3, 32, 15, "synth", "sad_fast_kernel<32,1,5,3,true,", True),
    "w15_nd64": (330, 96, 3, 3, 64, 15, "synth", "sad_fast_kernel<32,2,5,3,true,", False),
    "w21_nd64": (330, 96, 3, 3, 64, 21, "synth", "sad_fast_kernel<32,2,7,3,true,", False),
    "masked_nd96": (330, 96, 3, 3, 96, 15, "synth", "sad_fast_kernel<64,2,5,3,false,", False),
    "cooperating_nd256": (400, 96, 3, 3, 256, 15, "synth", "sad_fast_kernel<64,4,5,3,false,", False),
    "split_one_pair": (330, 96, 1, 1, 64, 15, "synth", "sad_fast_kernel<32,2,5,3,true,", False),
    "ties_nd32": (330, 96, 3, 3, 32, 15, "ties", "sad_fast_kernel<32,1,5,3,true,", True),
    "x48_w15_nd128": (330, 96, 48, 4, 128, 15, "synth", "sad_fast_kernel<128,1,5,3,true,", True),
    "x48_w15_nd64": (330, 96, 48, 4, 64, 15, "synth", "sad_fast_kernel<64,1,5,3,true,", True),
    "x48_w21_nd64": (330, 96, 48, 4, 64, 21, "synth", "sad_fast_kernel<64,1,7,3,true,", True),
    "x48_masked_nd96": (330, 96, 48, 4, 96, 15, "synth", "sad_fast_kernel<128,1,5,3,false,", False),
    "x48_ties_nd128": (330, 96, 48, 4, 128, 15, "ties", "sad_fast_kernel<128,1,5,3,true,", True),
    "x48_w9_nd128": (300, 96, 48, 4, 128, 9, "synth", "sad_fast_kernel<128,1,3,3,true,", True),
    "x48_w11_nd64": (300, 96, 48, 4, 64, 11, "synth", "sad_fast_kernel<64,1,11,1,true,", True),      # 1-column sums: plain strips only
}
# a launch that fills the chip often enough for the default mode to reorder its segments: 4 strips x 64 pairs = 256 workgroups per
# segment set against 3 072 slots -> stride 13, and more segments than that
BIG = (330, 280, 64, 4, 128, 15)


def _parity():
    spec = importlib.util.spec_from_file_location("_handoff_parity", ROOT / "tests" / "test_gpu_parity.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def images(kind, W, H, n, nd):
    from u96_slam_amd import synth

    if kind == "ties":
        # constant images plus a few pixels: nearly every window sum ties, and the winner is decided by the tags the carrier
        # lanes hold in their vertical sums -- a tag lost in the hand-off moves it
        rng = np.random.default_rng(7)
        L = np.full((n, H, W), 100, np.uint8)
        R = L.copy()
        for img in (L, R):
            for i in range(n):
                ys, xs = rng.integers(0, H, 12), rng.integers(0, W, 12)
                img[i, ys, xs] = rng.integers(0, 256, 12)
        return L, R
    return synth.make_batch(0, n, W, H, nd)


def case_dict(W, H, n, nd, w):
    return dict(W=W, H=H, n=n, nd=nd, w=w, mind=0, roi=None, inplace=1, env={}, cap=31, uniq=10, tex=10, d12=1, spk_win=50, spk_range=32)


KW = dict(prefilter_cap=31, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1, speckle_window_size=50, speckle_range=32)


@pytest.fixture(scope="module")
def ctx(pkg, oracle):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dict(pkg=pkg, oracle=oracle, parity=_parity(), refs={})


def reference(ctx, name, W, H, n, nd, w, kind, distinct):
    """Images of the case and the oracle's stages, computed once: `distinct` different pairs, repeated up to n."""
    if name not in ctx["refs"]:
        L, R = images(kind, W, H, distinct, nd)
        p = ctx["oracle"].make_params(num_disparities=nd, block_size=w, **KW)
        refs = [ctx["oracle"].compute(p, L[i], R[i], stages=True)[1] for i in range(distinct)]
        ref = {k: np.stack([refs[i % distinct][k] for i in range(n)]) for k in refs[0]}
        reps = n // distinct
        ctx["refs"][name] = (np.concatenate([L] * reps), np.concatenate([R] * reps), ref)
    return ctx["refs"][name]


def run(ctx, L, R, nd, w):
    """One device call; the stages, the kernel's name and the hand-off counts."""
    import torch

    bm = ctx["pkg"].StereoBM.create(nd, w, device=0)
    bm.setPreFilterCap(31); bm.setTextureThreshold(10); bm.setUniquenessRatio(10)
    bm.setDisp12MaxDiff(1); bm.setSpeckleWindowSize(50); bm.setSpeckleRange(32)
    n, h, wd = L.shape
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    outs = []
    for _ in range(2):           # twice on the same engine: the second call meets the first one's slots and flags
        d = bm.compute_device(dl, dr).cpu().numpy()
        outs.append(dict(disp=d, pre_lr=bm.debug_fetch(3, n, h, wd), cost=bm.debug_fetch(2, n, h, wd), counts=bm.debug_fetch(7).tolist()))
    return outs, bm.last_kernel()


def check(ctx, monkeypatch, mode, name, W, H, n, distinct, nd, w, kind, want, lone):
    monkeypatch.setenv("SBM_FAST_HANDOFF", str(mode))
    st, pl = plan.query(ctx["pkg"], case_dict(W, H, n, nd, w))
    assert st == 0 and pl.fast
    kernel = pl.kernel.decode()
    assert kernel.startswith(want), (kernel, want)
    assert pl.f.nseg >= 3, pl.f.nseg
    if nd == 128 and w == 15:
        assert 0 < pl.f.strips3 < pl.f.strips, (pl.f.strips3, pl.f.strips)     # both strip kinds: a stride-3 triple and a plain strip
    assert (pl.f.NWAVES == 1 and bool(pl.f.exact)) == lone
    later = (pl.f.nseg - 1) * n * pl.f.strips
    L, R, ref = reference(ctx, name, W, H, n, nd, w, kind, distinct)
    outs, ran = run(ctx, L, R, nd, w)
    assert ran == kernel
    for o in outs:
        ctx["parity"].assert_stages_equal(o, ref, dict(KW, num_disparities=nd, block_size=w))
        taken, could = o["counts"]
        print(f"{name} mode {mode}: nseg {pl.f.nseg} strips {pl.f.strips} took over {taken} of {could} possible, {later} later segments")
        if mode == 0 or not lone:
            assert (taken, could) == (0, 0)
        elif mode == 2:
            assert (taken, could) == (later, later)
        else:
            assert 0 <= taken <= could <= later
    for k in ("disp", "pre_lr", "cost"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    return pl, outs


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", list(CASES))
def test_every_mode_matches_the_oracle(ctx, monkeypatch, name, mode):
    check(ctx, monkeypatch, mode, name, *CASES[name])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0, 2])
def test_a_launch_that_reorders_its_segments(ctx, monkeypatch, mode):
    """64 pairs (four different ones, repeated): in the default mode the segments are dispatched out of their natural order and
    the later ones of every chain may take over; how many do is timing, the maps are not."""
    n = BIG[2]
    pl, outs = check(ctx, monkeypatch, mode, "big", *BIG, "synth", "sad_fast_kernel<128,1,5,3,true,", True)
    per_seg = n * pl.f.strips
    if mode == 1:
        stride = -(-3072 // per_seg) + 1
        assert stride < pl.f.nseg, (stride, pl.f.nseg)                     # the order is not the identity
        assert outs[0]["counts"][1] == (pl.f.nseg - stride) * per_seg      # the positions behind the first `stride` may take over
        rows = [pl.f.segrow[k + 1] - pl.f.segrow[k] for k in range(pl.f.nseg)]
        assert sum(rows) == pl.g.row1 - pl.g.row0 and min(rows) > 0


@pytest.mark.gpu
def test_changing_shapes_on_one_engine(ctx, monkeypatch):
    """The slots and their flags are laid out per plan: calls of different shapes on one engine, back and forth, stay exact
    (a flag word of one layout must never read as this launch's number in another)."""
    import torch

    monkeypatch.setenv("SBM_FAST_HANDOFF", "2")
    bm = ctx["pkg"].StereoBM.create(128, 15, device=0)
    bm.setPreFilterCap(31); bm.setTextureThreshold(10); bm.setUniquenessRatio(10)
    bm.setDisp12MaxDiff(1); bm.setSpeckleWindowSize(50); bm.setSpeckleRange(32)
    for name in ("x48_w15_nd128", "x48_ties_nd128", "x48_w15_nd128"):
        W, H, n, distinct, nd, w, kind = CASES[name][:7]
        for m in (n, n - 3, n):                     # fewer pairs: fewer slots, the flags end earlier
            L, R, ref = reference(ctx, name, W, H, n, nd, w, kind, distinct)
            d = bm.compute_device(torch.from_numpy(L[:m]).cuda(), torch.from_numpy(R[:m]).cuda()).cpu().numpy()
            assert np.array_equal(d, ref["disp"][:m]), (name, m)
            taken, could = bm.debug_fetch(7).tolist()
            assert taken == could and (m < n or could > 0)


@pytest.mark.gpu
def test_a_full_chip_under_load_agrees_with_priming(ctx, monkeypatch):
    """The flagship shape, 64 KITTI-sized pairs, where the default mode takes thousands of hand-offs per call between workgroups
    on different CUs and XCDs while the chip is busy: 40 calls back to back, every map and cost plane equal to the ones the
    priming mode gives (a stale or torn slot would show as a changed pixel)."""
    import torch

    from u96_slam_amd import synth

    W, H, n, nd, w = 1242, 375, 64, 128, 15
    L, R = synth.make_batch(0, 4, W, H, nd)
    dl, dr = torch.from_numpy(np.concatenate([L] * 16)).cuda(), torch.from_numpy(np.concatenate([R] * 16)).cuda()
    bm = ctx["pkg"].StereoBM.create(nd, w, device=0)
    bm.setPreFilterCap(31); bm.setTextureThreshold(10); bm.setUniquenessRatio(10)
    bm.setDisp12MaxDiff(1); bm.setSpeckleWindowSize(50); bm.setSpeckleRange(32)
    monkeypatch.setenv("SBM_FAST_HANDOFF", "0")
    want = bm.compute_device(dl, dr).clone()
    want_cost = bm.debug_fetch(2, n, H, W)
    assert bm.debug_fetch(7).tolist() == [0, 0]
    monkeypatch.setenv("SBM_FAST_HANDOFF", "1")
    outs = [torch.empty_like(want) for _ in range(40)]
    for o in outs:
        bm.compute_device(dl, dr, o, sync=False)
    torch.cuda.synchronize()
    taken, could = bm.debug_fetch(7).tolist()
    print(f"KITTI x 64: took over {taken} of {could} possible")
    assert could > 0 and 0 <= taken <= could
    assert np.array_equal(bm.debug_fetch(2, n, H, W), want_cost)
    for i, o in enumerate(outs):
        assert torch.equal(o, want), i
