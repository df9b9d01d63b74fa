"""The folded leftover strip of the interior SAD kernel (csrc/sbm_sad_fast_fold.h): the last plain strip of a 128-disparity,
window-15 launch with at most 22 columns runs with the wavefront folded over its two disparity halves. Same integers as the plain
strip, so every case here is held twice: bit-exact against the CPU oracle (map, map before the LR check, cost plane -- with
disp12MaxDiff 1 the cost plane also goes through the LR stage) and byte-equal against SBM_FAST_FOLD=0 on the same engine.

Shapes: W = 141 + R with R in {1, 21, 22}, where the folded strip is the launch's only strip, and W = 342, one stride-3 triple
plus R = 21; H = 28 gives one row segment, H = 96 ten (down to two rows). That many small pairs (a few different ones, repeated)
because fewer are split over cooperating wavefronts, which do not fold. SBM_FAST_HANDOFF 0 and 2: every segment primes / every
later segment takes its sums over (sbm_debug_fetch(7) counts them). The oracle's maps are computed once per case and shared."""
import importlib.util
import pathlib

import numpy as np
import pytest

import test_bm_plan as plan
import test_bm_plan_fold as foldplan

ROOT = pathlib.Path(__file__).resolve().parents[1]
ND, WSZ = 128, 15
KW = dict(prefilter_cap=31, texture_threshold=10, uniqueness_ratio=10, disp12_max_diff=1, speckle_window_size=50, speckle_range=32)

# name -> (W, H, pairs, R, row segments: one or several)
SHAPES = {
    "r1": (142, 96, 192, 1, False), "r21": (162, 96, 192, 21, False), "r22": (163, 96, 192, 22, False),
    "triple_r21": (342, 96, 48, 21, False),
    "r1_one_segment": (142, 28, 1800, 1, True), "r21_one_segment": (162, 28, 1800, 21, True),
    "r22_one_segment": (163, 28, 1800, 22, True), "triple_r21_one_segment": (342, 28, 450, 21, True),
}
# buffer index d <-> disparity ND - 1 - d: winners at the ends of the range (the neighbours mirror) and around the half boundary
# (the neighbours come from the other half)
SHIFT_INDEX = (0, 62, 63, 64, 65, 127)
# name -> (image kind, different pairs, parameter overrides)
CONTENT = {
    "constant": ("constant", 1, dict(texture_threshold=0, uniqueness_ratio=0)),   # all 128 sums tie: index 0 must win across the halves
    "ties": ("ties", 4, dict(texture_threshold=0, uniqueness_ratio=0)),          # nearly all tie, nothing is filtered: every winner shows
    "ties_filtered": ("ties", 4, {}),
    "shifts": ("shifts", len(SHIFT_INDEX), {}),
    "uniq60": ("synth", 4, dict(uniqueness_ratio=60)),                          # deficit sums beyond 16 bits: the saturating adds
}


def _parity():
    spec = importlib.util.spec_from_file_location("_fold_parity", ROOT / "tests" / "test_gpu_parity.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def images(kind, W, H, distinct):
    from u96_slam_amd import synth

    if kind == "constant":
        L = np.full((distinct, H, W), 100, np.uint8)
        return L, L.copy()
    if kind == "ties":        # constant plus a few pixels: nearly every sum ties, the tags of the carrier lanes decide
        rng = np.random.default_rng(7)
        L = np.full((distinct, H, W), 100, np.uint8)
        R = L.copy()
        for img in (L, R):
            for i in range(distinct):
                ys, xs = rng.integers(0, H, 12), rng.integers(0, W, 12)
                img[i, ys, xs] = rng.integers(0, 256, 12)
        return L, R
    if kind == "shifts":      # pair i: the right image is the left one moved by ND - 1 - SHIFT_INDEX[i] columns
        rng = np.random.default_rng(11)
        T = synth.box3(rng.integers(0, 256, (H, W + 2 * ND), dtype=np.uint8))
        L = np.stack([T[:, ND:ND + W]] * distinct)
        R = np.stack([T[:, ND + (ND - 1 - k):ND + (ND - 1 - k) + W] for k in SHIFT_INDEX[:distinct]])
        return np.ascontiguousarray(L), np.ascontiguousarray(R)
    return synth.make_batch(0, distinct, W, H, ND)


@pytest.fixture(scope="module")
def ctx(pkg, oracle):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return dict(pkg=pkg, oracle=oracle, parity=_parity(), refs={})


def reference(ctx, key, W, H, n, kind, distinct, kw):
    """Images of the case (`distinct` different pairs, repeated up to n) and the oracle's stages, computed once."""
    if key not in ctx["refs"]:
        L, R = images(kind, W, H, distinct)
        p = ctx["oracle"].make_params(num_disparities=ND, block_size=WSZ, **kw)
        refs = [ctx["oracle"].compute(p, L[i], R[i], stages=True)[1] for i in range(distinct)]
        pick = np.arange(n) % distinct
        ref = {k: np.stack([refs[i][k] for i in range(distinct)])[pick] for k in refs[0]}
        ctx["refs"][key] = (np.ascontiguousarray(L[pick]), np.ascontiguousarray(R[pick]), ref)
    return ctx["refs"][key]


def check(ctx, monkeypatch, mode, key, W, H, n, R, one_segment, kind="synth", distinct=4, override={}):
    import torch

    kw = dict(KW, **override)
    monkeypatch.setenv("SBM_FAST_HANDOFF", str(mode))
    c = dict(foldplan.case(W, H, n, ND, WSZ), uniq=kw["uniqueness_ratio"], tex=kw["texture_threshold"])
    st, pl = plan.query(ctx["pkg"], c)
    assert st == plan.OK and pl.fast
    kernel = pl.kernel.decode()
    assert kernel.startswith("sad_fast_kernel<128,1,5,3,true,true>"), kernel
    assert pl.f.strips == pl.f.strips3 + 1 and pl.f.strips3 == (3 if W > 300 else 0)
    assert (pl.f.nseg == 1) if one_segment else (pl.f.nseg >= 3), pl.f.nseg
    assert pl.f.uniq_plain == (kw["uniqueness_ratio"] <= 10)
    assert foldplan.fold_cols(ctx["pkg"], monkeypatch, c) == R
    later = (pl.f.nseg - 1) * n * pl.f.strips

    L, Rt, ref = reference(ctx, key, W, H, n, kind, distinct, kw)
    bm = ctx["pkg"].StereoBM.create(ND, WSZ, device=0)
    bm.setPreFilterCap(kw["prefilter_cap"]); bm.setTextureThreshold(kw["texture_threshold"]); bm.setUniquenessRatio(kw["uniqueness_ratio"])
    bm.setDisp12MaxDiff(kw["disp12_max_diff"]); bm.setSpeckleWindowSize(kw["speckle_window_size"]); bm.setSpeckleRange(kw["speckle_range"])
    dl, dr = torch.from_numpy(L).cuda(), torch.from_numpy(Rt).cuda()
    outs = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("SBM_FAST_FOLD", fold)
        d = bm.compute_device(dl, dr).cpu().numpy()
        assert bm.last_kernel() == kernel
        outs[fold] = dict(disp=d, pre_lr=bm.debug_fetch(3, n, H, W), cost=bm.debug_fetch(2, n, H, W))
        taken, could = bm.debug_fetch(7).tolist()
        print(f"{key} hand-off mode {mode} fold {fold}: nseg {pl.f.nseg} strips {pl.f.strips} took over {taken} of {could}, {later} later segments")
        assert (taken, could) == ((0, 0) if mode == 0 else (later, later))
    ctx["parity"].assert_stages_equal(outs["1"], ref, dict(kw, num_disparities=ND, block_size=WSZ))
    for k in ("disp", "pre_lr", "cost"):
        assert outs["1"][k].tobytes() == outs["0"][k].tobytes(), k
    return pl, ref


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_shape_matches_the_oracle_and_the_plain_strip(ctx, monkeypatch, name, mode):
    check(ctx, monkeypatch, mode, name, *SHAPES[name])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("shape", ["r21", "triple_r21"])
@pytest.mark.parametrize("content", list(CONTENT))
def test_content_that_crosses_the_halves(ctx, monkeypatch, content, shape, mode):
    kind, distinct, override = CONTENT[content]
    W, H, n, R, one = SHAPES[shape]
    pl, ref = check(ctx, monkeypatch, mode, f"{shape}_{content}", W, H, n, R, one, kind, distinct, override)
    # the folded strip's columns of the map before the LR check (image columns lofs + xc0 + cbase ...)
    x0 = pl.g.lofs + pl.f.xc1 - R
    cols = ref["pre_lr"][:, pl.g.row0:pl.g.row1, x0:x0 + R]
    if content == "constant":     # every sum is 0: the first buffer index, disparity ND - 1, everywhere
        assert (cols == (ND - 1) * 16).all()
    if content == "shifts":       # the case is what it says: pair i's winner sits at SHIFT_INDEX[i] (the sub-pixel step moves it by at most 8 / 16)
        for i, k in enumerate(SHIFT_INDEX):
            at_k = np.abs(cols[i].astype(int) - (ND - 1 - k) * 16) <= 8
            assert at_k.mean() > 0.9, (k, float(at_k.mean()))
