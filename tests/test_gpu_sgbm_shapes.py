"""The semi-global matcher on the GPU against the CPU restatement (oracle/sgbm_ref.c), bit for bit, where the kernels' layout can go
wrong: every lane layout of sgbm_path_kernel / sgbm_select_kernel (NV = 1/2/4/8 disparities per lane, fully and partly masked)
with winners placed on purpose in lane 0, in the last active lane and on both sides of a lane boundary; path grids of 1-5 rows and
63/64/65 columns with every chain count mod 4; whole frames at camera sizes (the reference call on a 640 x 480 batch, KITTI,
1080p); and the chunking of batches, up to one pair whose C and S volumes each hold more than 2^31 elements.

Every case compares the whole final map with sgbm_ref.compute under the same parameters and reading; where the batch is one
chunk it also compares C, S and the map before the median (debug_fetch 4 / 5 / 6)."""
import concurrent.futures

import numpy as np
import pytest

import sgbm_ref

pytestmark = pytest.mark.gpu
HH, SG = sgbm_ref.MODE_HH, sgbm_ref.MODE_SGBM
# main.cpp:219-230, positionally
REF_ARGS = (-64, 128, 11, 100, 1000, 32, 0, 15, 1000, 16, HH)
REF_CHUNK = 15   # pairs per chunk at the reference call on 640 x 480


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available()
    return t


def _device(torch, sg, Ls, Rs, **kw):
    dl = torch.from_numpy(np.ascontiguousarray(np.stack(Ls))).cuda()
    dr = torch.from_numpy(np.ascontiguousarray(np.stack(Rs))).cuda()
    return sg.compute(dl, dr, **kw)


def _nv(D):
    return 1 if D <= 64 else 2 if D <= 128 else 4 if D <= 256 else 8


def _args(p):
    return [getattr(p, f) for f, _ in sgbm_ref.SgbmParams._fields_]


def _texture(rng, H, W):
    """Smoothed noise stretched to the full grey range: distinct at every shift, smooth enough for sub-pixel steps."""
    t = rng.integers(0, 256, (H, W), dtype=np.uint8)
    p = np.pad(t.astype(np.int32), 1, mode="edge")
    box = sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) // 9
    return np.clip((box - 128) * 3 + 128, 0, 255).astype(np.uint8)


def _banded_pair(rng, H, W, disps, T=None):
    """L(x) = R(x - d) with one whole-pixel disparity d per row band (bands of equal height, top to bottom)."""
    pad = max(abs(d) for d in disps) + 4
    if T is None:
        T = _texture(rng, H, W + 2 * pad)
    nb = len(disps)
    band = -(-H // nb)
    which = np.minimum(np.arange(H) // band, nb - 1)
    cols = np.arange(W)[None, :] + pad + np.asarray(disps)[which][:, None]
    L = np.ascontiguousarray(T[:, pad:pad + W])
    R = np.ascontiguousarray(np.take_along_axis(T, cols, axis=1))
    return L, R, which


def _stripes(rng, H, W):
    """Vertical stripes 20-80 px wide on four grey levels: S ties exactly across many disparities."""
    widths = rng.integers(20, 81, W // 20 + 1)
    levels = rng.integers(0, 4, len(widths)) * 85
    return np.broadcast_to(np.repeat(levels, widths)[:W].astype(np.uint8), (H, W)).copy()


def _compare_stages(sg, p, Ls, Rs, got, reading=0, label=""):
    """Whole maps, and C, S, pre against the restatement (the batch is one chunk). Returns the restatement's stages."""
    H, W = Ls[0].shape
    w1 = sgbm_ref.width1(p, W)
    n = len(Ls)
    sts = []
    for k in range(n):
        want, st = sgbm_ref.compute(p, Ls[k], Rs[k], reading=reading, stages=True)
        assert np.array_equal(got[k], want), (label, k, "map", int((got[k] != want).sum()))
        sts.append(st)
    pre = sg.debug_fetch(6, (n, H, W))
    if w1 >= 1:
        C = sg.debug_fetch(4, (n, H, w1, p.num_disparities))
        S = sg.debug_fetch(5, (n, H, w1, p.num_disparities))
    for k in range(n):
        assert np.array_equal(pre[k], sts[k]["pre"]), (label, k, "pre", int((pre[k] != sts[k]["pre"]).sum()))
        if w1 >= 1:
            assert np.array_equal(C[k], sts[k]["C"]), (label, k, "C", int((C[k] != sts[k]["C"]).sum()))
            assert np.array_equal(S[k], sts[k]["S"]), (label, k, "S", int((S[k] != sts[k]["S"]).sum()))
    return sts


# ---- 1. lane layouts -------------------------------------------------------------------------------------------------------
LANE_DS = (16, 48, 64, 80, 112, 128, 144, 208, 256, 272, 400, 496, 512)


def _spread(rng, values, n):
    """n picks that use every value at least once, in a seeded order."""
    out = [values[i % len(values)] for i in range(n)]
    rng.shuffle(out)
    return out


def _lane_cases():
    keys = [(D, mode) for D in LANE_DS for mode in (HH, SG)]
    n = len(keys)
    rng = np.random.default_rng(2027)
    minDs = _spread(rng, ["neg", "zero", "pos"], n)
    bss = _spread(rng, [1, 3, 5, 11], n)
    explicit = _spread(rng, [False, True], n)
    caps = _spread(rng, [0, 31], n)
    uniqs = _spread(rng, [0, 15], n)
    d12s = _spread(rng, [0, -1, 4, 32], n)     # <= 0 means 1, as in OpenCV
    speckles = _spread(rng, [False, True], n)
    readings = _spread(rng, [0, 96], n)
    cases = []
    for i, (D, mode) in enumerate(keys):
        minD = {"neg": -(D // 4) - 3, "zero": 0, "pos": 5}[minDs[i]]
        bs = bss[i]
        P1, P2 = (8 * bs * bs, 32 * bs * bs) if explicit[i] else (0, 0)
        sws, sr = (20, 2) if speckles[i] else (0, 0)
        p = sgbm_ref.make_params(minD, D, bs, P1, P2, d12s[i], caps[i], uniqs[i], sws, sr, mode)
        assert sgbm_ref.envelope(p) <= 32767
        cases.append((p, readings[i]))
    return cases


LANE_CASES = _lane_cases()


def _lane_targets(D):
    """Disparity indices to land the winner on: lane 0, both sides of a lane boundary in the middle of the active lanes, the
    last active lane's last slot and the slot before it (whose sub-pixel neighbour is D - 1)."""
    NV = _nv(D)
    m = (D // NV) // 2
    return [0, m * NV - 1, m * NV, D - 2, D - 1]


def _lane_pairs(p, seed):
    """Two pairs with one target per row band (the second in another band order), and a pair of coarse grey stripes shifted by
    the boundary target, whose S ties exactly between lanes."""
    D, minD = p.num_disparities, p.min_disparity
    bands = _lane_targets(D)
    band_h = 8 if p.block_size >= 9 else 6
    H = band_h * len(bands)
    W = 72 + max(minD + D, 0) - min(minD, 0)
    rng = np.random.default_rng(seed)
    Ls, Rs = [], []
    for order in (bands, bands[2:] + bands[:2]):
        L, R, which = _banded_pair(rng, H, W, [minD + b for b in order])
        Ls.append(L)
        Rs.append(R)
    pad = abs(minD + bands[1]) + 4
    L, R, _w = _banded_pair(rng, H, W, [minD + bands[1]], T=_stripes(rng, H, W + 2 * pad))
    Ls.append(L)
    Rs.append(R)
    return Ls, Rs, which, bands


def test_lane_cases_cover_the_matrix():
    ps = [p for p, _ in LANE_CASES]
    for D in LANE_DS:
        assert {p.mode for p in ps if p.num_disparities == D} == {HH, SG}
    assert {np.sign(p.min_disparity) for p in ps} == {-1, 0, 1}
    assert {p.block_size for p in ps} == {1, 3, 5, 11}
    assert {p.p2 > 0 for p in ps} == {False, True}
    assert {p.uniqueness_ratio for p in ps} == {0, 15}
    assert {p.disp12_max_diff for p in ps} >= {0, 4, 32}
    assert {p.speckle_window_size > 0 for p in ps} == {False, True}
    assert {r for _, r in LANE_CASES} == {0, 96}
    # every NV, fully and partly masked
    assert {(_nv(D), D == 64 * _nv(D)) for D in LANE_DS} == {(nv, full) for nv in (1, 2, 4, 8) for full in (False, True)}


@pytest.mark.parametrize("case", range(len(LANE_CASES)),
                         ids=[f"D{p.num_disparities}-{'HH' if p.mode == HH else 'SG'}" for p, _ in LANE_CASES])
def test_lane_layouts(pkg, torch, monkeypatch, case):
    p, reading = LANE_CASES[case]
    D = p.num_disparities
    Ls, Rs, which, bands = _lane_pairs(p, 100 + case)
    monkeypatch.setenv("SBM_CV_READING", str(reading))
    sg = pkg.StereoSGBM.create(*_args(p))
    got = _device(torch, sg, Ls, Rs).cpu().numpy()
    sts = _compare_stages(sg, p, Ls, Rs, got, reading, f"D{D} mode {p.mode}")
    sg.close()
    # the content does what it is for: each target is the winner (lowest S) of pixels in its band
    best = sts[0]["S"].argmin(axis=2)
    for b, t in enumerate(bands):
        assert (best[which == b] == t).mean() > 0.3, (D, b, t, float((best[which == b] == t).mean()))
    assert (got[0] > (p.min_disparity - 1) * 16).mean() > 0.05


def _lane_ties(S, D):
    """Fraction of pixels whose lowest S is reached in more than one lane."""
    at_min = S == S.min(axis=2, keepdims=True)
    lanes = np.arange(D) // _nv(D)
    return float((np.where(at_min, lanes, 1 << 20).min(axis=2) < np.where(at_min, lanes, -1).max(axis=2)).mean())


def test_lane_stripes_tie_between_lanes():
    # SGM breaks most ties along its paths; the stripe pairs of the matrix still hold exact ties between lanes at the lowest S in
    # a good part of it, at every NV
    tied = set()
    for case, (p, reading) in enumerate(LANE_CASES):
        Ls, Rs, _w, _b = _lane_pairs(p, 100 + case)
        _, st = sgbm_ref.compute(p, Ls[2], Rs[2], reading=reading, stages=True)
        if _lane_ties(st["S"], p.num_disparities) > 0.5:
            tied.add(case)
    assert len(tied) >= len(LANE_CASES) // 4, sorted(tied)
    assert {_nv(LANE_CASES[c][0].num_disparities) for c in tied} == {1, 2, 4, 8}


# ---- 2. path geometry ------------------------------------------------------------------------------------------------------
GEOM_BS = 9                                   # SW2 = 4: H = 4 and 5 are SW2 and SW2 + 1
GEOM_SHAPES = [(H, w1) for H in (1, 2, 3, 4, 5) for w1 in (1, 2, 63, 64, 65)] + [(3, 301), (2, 700), (301, 3), (700, 2),
                                                                                   (130, 65)]
GEOM_MODES = {HH: (-5, 32), SG: (3, 96)}      # (minD, D): NV 1 and NV 2, both partly masked


def test_geometry_covers_every_chain_count_mod_4():
    for f in (lambda H, w1: H, lambda H, w1: w1, lambda H, w1: w1 + H - 1):
        assert {f(H, w1) % 4 for H, w1 in GEOM_SHAPES} == {0, 1, 2, 3}
    assert any(w1 > 50 * H for H, w1 in GEOM_SHAPES) and any(H > 50 * w1 for H, w1 in GEOM_SHAPES)


@pytest.mark.parametrize("mode", [HH, SG], ids=["HH", "SG"])
def test_path_geometry(pkg, torch, mode):
    minD, D = GEOM_MODES[mode]
    p = sgbm_ref.make_params(minD, D, GEOM_BS, 20, 300, 2, 0, 5, 0, 0, mode)
    sg = pkg.StereoSGBM.create(*_args(p))
    rng = np.random.default_rng(60 + mode)
    for H, w1 in GEOM_SHAPES:
        W = w1 + max(minD + D, 0) - min(minD, 0)
        assert sgbm_ref.width1(p, W) == w1
        Ls, Rs = [], []
        for _ in range(2):
            L, R, _w = _banded_pair(rng, H, W, [minD + int(rng.integers(0, D)) for _ in range(min(H, 3))])
            Ls.append(L)
            Rs.append(R)
        got = _device(torch, sg, Ls, Rs).cpu().numpy()
        _compare_stages(sg, p, Ls, Rs, got, 0, f"H {H} width1 {w1}")
    sg.close()


# ---- 3. frame sizes and 4. chunk edges -------------------------------------------------------------------------------------
def _noisy(rng, img, sigma):
    return np.clip(img.astype(np.float64) + rng.normal(0, sigma, img.shape), 0, 255).astype(np.uint8)


def _ref_pairs():
    """Three unique 640 x 480 pairs for the reference call (disparities 8..63 inside its -64..63); the last with heavy noise."""
    from u96_slam_amd import synth

    pairs = [synth.make_pair(200 + i, 640, 480, 72) for i in range(3)]
    rng = np.random.default_rng(77)
    L, R = pairs[2]
    pairs[2] = (_noisy(rng, L, 12), _noisy(rng, R, 12))
    return pairs


FRAMES = {
    # name: (params, width, height, synth field width)
    "kitti": (sgbm_ref.make_params(0, 128, 5, 200, 800, 1, 31, 10, 100, 2, HH), 1242, 375, 128),
    "1080p-HH": (sgbm_ref.make_params(0, 256, 3, 72, 288, 1, 0, 10, 100, 2, HH), 1920, 1080, 256),
    "1080p-SG": (sgbm_ref.make_params(0, 256, 3, 72, 288, 1, 0, 10, 100, 2, SG), 1920, 1080, 256),
}
BIG = (sgbm_ref.make_params(0, 512, 3, 0, 0, 1, 0, 10, 100, 2, SG), 8192, 560)


@pytest.fixture(scope="module")
def frames():
    """Inputs and restatement maps of every frame-sized pair, computed once, in parallel (ctypes releases the GIL)."""
    from u96_slam_amd import synth

    sgbm_ref.lib()
    sgbm_ref.sbm_oracle.lib()
    inputs = {f"ref{i}": (sgbm_ref.make_params(*REF_ARGS),) + pr for i, pr in enumerate(_ref_pairs())}
    for name, (p, W, H, nd) in FRAMES.items():
        inputs[name] = (p,) + synth.make_pair(300 + len(inputs), W, H, nd)
    p, W, H = BIG
    inputs["big"] = (p,) + synth.make_pair(400, W, H, 512)
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(inputs)) as ex:
        futs = {k: ex.submit(sgbm_ref.compute, p, L, R, pre_only=True) for k, (p, L, R) in inputs.items()}
        return {k: inputs[k] + futs[k].result() for k in inputs}   # (params, L, R, map, pre)


def _variant(p, **kw):
    a = dict(zip([f for f, _ in sgbm_ref.SgbmParams._fields_], _args(p)))
    a.update(kw)
    return [a[f] for f, _ in sgbm_ref.SgbmParams._fields_]


def _not_vacuous(pkg, torch, p, Ls, Rs, got, floor):
    """The map is real, and the uniqueness test, the LR check and the speckle filter each change it."""
    inv = (p.min_disparity - 1) * 16
    valid = (got > inv).sum()
    assert valid / got.size > floor, float(valid / got.size)
    for kw in (dict(uniqueness_ratio=0), dict(disp12_max_diff=4096), dict(speckle_window_size=0, speckle_range=0)):
        sg = pkg.StereoSGBM.create(*_variant(p, **kw))
        alt = _device(torch, sg, Ls, Rs).cpu().numpy()
        sg.close()
        assert (alt > inv).sum() > valid, (kw, int((alt > inv).sum()), int(valid))


def test_reference_call_batch_properties(pkg, torch, frames):
    # 16 pairs = two chunks (15 + 1) of 3 unique pairs; the last unique pair is noisy
    uniq = [frames[f"ref{i}"] for i in range(3)]
    p = uniq[0][0]
    idx = [i % 3 for i in range(16)]
    Ls, Rs = [uniq[i][1] for i in idx], [uniq[i][2] for i in idx]
    sg = pkg.StereoSGBM.create(*REF_ARGS)
    got = _device(torch, sg, Ls, Rs).cpu().numpy()
    for k, i in enumerate(idx):
        assert np.array_equal(got[k], uniq[i][3]), (k, int((got[k] != uniq[i][3]).sum()))   # duplicates equal, and the oracle
    for i in range(3):
        alone = _device(torch, sg, [uniq[i][1]], [uniq[i][2]]).cpu().numpy()[0]
        assert np.array_equal(alone, got[i]) and np.array_equal(alone, got[i + 12])
    sg.close()
    _not_vacuous(pkg, torch, p, [u[1] for u in uniq], [u[2] for u in uniq], got[:3], 0.3)
    assert (got[2] > (p.min_disparity - 1) * 16).mean() < (got[0] > (p.min_disparity - 1) * 16).mean()   # the noise bites


@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_size(pkg, torch, frames, name):
    p, L, R, want, pre = frames[name]
    sg = pkg.StereoSGBM.create(*_args(p))
    got = _device(torch, sg, [L], [R]).cpu().numpy()
    assert np.array_equal(got[0], want), int((got[0] != want).sum())
    assert np.array_equal(sg.debug_fetch(6, (1,) + L.shape)[0], pre)
    sg.close()
    _not_vacuous(pkg, torch, p, [L], [R], got, 0.4)


@pytest.mark.parametrize("n", [REF_CHUNK, REF_CHUNK + 1, 2 * REF_CHUNK + 1])
def test_chunk_edges_at_the_reference_call(pkg, torch, frames, n):
    uniq = [frames[f"ref{i}"] for i in range(3)]
    idx = [i % 3 for i in range(n)]
    Ls, Rs = [uniq[i][1] for i in idx], [uniq[i][2] for i in idx]
    sg = pkg.StereoSGBM.create(*REF_ARGS)
    got = _device(torch, sg, Ls, Rs).cpu().numpy()
    for c0 in range(0, n, REF_CHUNK):
        for k in {c0, min(c0 + REF_CHUNK, n) - 1}:
            assert np.array_equal(got[k], uniq[idx[k]][3]), (n, k)
    H, W = Ls[0].shape
    if n <= REF_CHUNK:
        pre = sg.debug_fetch(6, (n, H, W))
        for k in (0, n - 1):
            assert np.array_equal(pre[k], uniq[idx[k]][4]), (n, k)
    else:
        for which, shape in ((4, (n, H, 512, 128)), (5, (n, H, 512, 128)), (6, (n, H, W))):
            with pytest.raises(pkg.StereoBMError):
                sg.debug_fetch(which, shape)
    sg.close()


def test_pair_above_the_chunk_budget(pkg, torch, frames):
    # width1 = 7680: C and S hold 7680 * 560 * 512 = 2.2e9 int16 elements each (4.4 GB), more than 2^31; the pair runs alone
    p, L, R, want, pre = frames["big"]
    H, W = L.shape
    assert sgbm_ref.width1(p, W) * H * p.num_disparities > 2 ** 31
    sg = pkg.StereoSGBM.create(*_args(p))
    got = _device(torch, sg, [L], [R]).cpu().numpy()[0]
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(sg.debug_fetch(6, (1, H, W))[0], pre)
    assert (got > (p.min_disparity - 1) * 16).mean() > 0.4
    # two copies: two chunks of one pair each, equal to each other; the stages of more than one chunk are not kept
    two = _device(torch, sg, [L, L], [R, R]).cpu().numpy()
    assert np.array_equal(two[0], want) and np.array_equal(two[1], want)
    with pytest.raises(pkg.StereoBMError):
        sg.debug_fetch(6, (2, H, W))
    sg.close()
