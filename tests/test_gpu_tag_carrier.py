"""The interior SAD kernel's window sums arrive at the winner search already tagged: carrier lanes start their vertical sums
at the register tag (sbm_sad_fast_core.h, FastTag). Everything here is bit-exact against the CPU oracle and aimed at what that
can break: ties across tag-group boundaries, sums at the envelope maximum, a uniqueness rival in another tag group exactly at
and one above the threshold, the mirrored neighbours at both ends of the range, every wavefront layout, plain strips only, and
the untagged start (SBM_FAST_PFSHIFT=0 / =1, read once per process: those run this file as a child process).

Coverage condition: except under SBM_FAST_PFSHIFT=0 / =1 every case must have run a tagged search -- asserted through the
`pfshift=` field of the kernel name, so that the file cannot pass by never reaching the tagged sums."""
import importlib.util
import json
import os
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _parity():
    spec = importlib.util.spec_from_file_location("_tag_carrier_parity", ROOT / "tests" / "test_gpu_parity.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _env():
    sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "oracle"))
    import torch

    import _pkg
    import sbm_oracle

    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    sbm_oracle.lib()
    return _pkg.load(), sbm_oracle


def tag_bits(wsz, cap=31):
    """pfshift sad_fast_pfshift() chooses at uniqueness 10 or below: the window's tag width where (maxS << bits) + tag fits 16 bits."""
    bits = 2 if wsz <= 15 else 1
    f = 1 << bits
    maxs = wsz * wsz * 2 * cap
    return bits if (f * 2 * cap + 1 <= 255 and f * maxs + f - 1 <= 65535) else 0


def run_case(pkg, oracle, kw, L, R):
    """One device call on the batch (n, H, W); returns (engine stages, oracle stages, kernel name)."""
    import torch

    bm = pkg.StereoBM.create(kw["num_disparities"], kw["block_size"])
    setters = dict(prefilter_cap=bm.setPreFilterCap, min_disparity=bm.setMinDisparity, texture_threshold=bm.setTextureThreshold,
                   uniqueness_ratio=bm.setUniquenessRatio, speckle_window_size=bm.setSpeckleWindowSize,
                   speckle_range=bm.setSpeckleRange, disp12_max_diff=bm.setDisp12MaxDiff)
    for k, v in kw.items():
        if k in setters:
            setters[k](v)
    n, h, w = L.shape
    dd = bm.compute_device(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())
    eng = dict(disp=dd.cpu().numpy(), pf_l=bm.debug_fetch(0, n, h, w), pf_r=bm.debug_fetch(1, n, h, w), pre_lr=bm.debug_fetch(3, n, h, w))
    if kw.get("disp12_max_diff", -1) >= 0:
        eng["cost"] = bm.debug_fetch(2, n, h, w)
    name = bm.last_kernel()
    p = oracle.make_params(**kw)
    refs = [oracle.compute(p, L[i], R[i], stages=True)[1] for i in range(n)]
    return eng, {k: np.stack([r[k] for r in refs]) for k in refs[0]}, name


def check_case(pkg, oracle, par, kw, L, R, want_pfshift=None):
    """Every stage against the oracle, and the search that ran: the window's tagged one unless `want_pfshift` says otherwise."""
    eng, ref, name = run_case(pkg, oracle, kw, L, R)
    par.assert_stages_equal(eng, ref, kw)
    want = tag_bits(kw["block_size"], kw.get("prefilter_cap", 31)) if want_pfshift is None else want_pfshift
    assert name.startswith("sad_fast_kernel<") and name.endswith(f"pfshift={want}"), (name, want)
    return eng, ref, name


def layout(name):
    m = re.match(r"sad_fast_kernel<(\d+),(\d+),(\d+),(\d+),(true|false)", name)
    return int(m.group(1)), int(m.group(2)), m.group(5) == "true"


def size_for(nd, wsz):
    return 2 * wsz + 9, nd + 4 * wsz + 70       # H, W: a few output rows, interior columns beyond one strip


def flat_pair(nd, wsz, n=1):
    h, w = size_for(nd, wsz)
    L = np.full((n, h, w), 100, np.uint8)
    return L, L.copy()


def two_level_pair(nd, wsz, n=1):
    """Blocky two-level images, the right one a shifted copy: large regions where every sum ties."""
    h, w = size_for(nd, wsz)
    rng = np.random.default_rng(nd * 31 + wsz)
    L = (rng.integers(0, 2, (n, h, w)) * 255).astype(np.uint8)
    L = np.repeat(np.repeat(L[:, ::8, ::8], 8, 1), 8, 2)[:, :h, :w].copy()
    return L, np.roll(L, -3, axis=2).copy()


def envelope_pair(nd, wsz, n=1):
    """Alternating 0 / 255 column pairs against their inverse (single alternating columns have no x-gradient: p[x+1] - p[x-1]
    is 0): the prefiltered planes are 0, 2 cap, 2 cap, 0, ... and the complement, so every absolute difference at the disparities
    that are multiples of 4 is 2 cap and the window sums there are the envelope maximum w * w * 2 cap."""
    h, w = size_for(nd, wsz)
    col = ((np.arange(w) >> 1) & 1) * 255
    L = np.broadcast_to(col.astype(np.uint8), (n, h, w)).copy()
    R = np.broadcast_to((255 - col).astype(np.uint8), (n, h, w)).copy()
    return L, R


def textured_pair(nd, wsz, shift, n=1, seed=0):
    h, w = size_for(nd, wsz)
    rng = np.random.default_rng(seed + nd + wsz)
    base = rng.integers(0, 256, (n, h, w + nd + 8), dtype=np.uint8)
    return base[:, :, :w].copy(), base[:, :, shift:shift + w].copy()


KW = dict(prefilter_cap=31, texture_threshold=0, uniqueness_ratio=0, disp12_max_diff=1)
LAYOUT_ND = [32, 64, 128, 192, 256, 384, 512, 96, 160]


def sad_volume(pfl, pfr, nd, wsz, mind=0):
    """Window sums of one pair in numpy, [buffer index][row][centre column] over the interior (unclamped) columns only, as int64;
    NaN-free: columns outside get -1. Buffer index b is disparity nd - 1 - b + mind."""
    h, w = pfl.shape
    w2 = wsz // 2
    vol = np.full((nd, h, w), -1, np.int64)
    a = pfl.astype(np.int64)
    b = pfr.astype(np.int64)
    for bi in range(nd):
        d = nd - 1 - bi + mind
        diff = np.zeros((h, w), np.int64)
        if d >= 0:
            diff[:, d:] = np.abs(a[:, d:] - b[:, :w - d])
        ii = np.zeros((h + 1, w + 1), np.int64)
        ii[1:, 1:] = diff.cumsum(0).cumsum(1)
        s = ii[wsz:, wsz:] - ii[:-wsz, wsz:] - ii[wsz:, :-wsz] + ii[:-wsz, :-wsz]      # (h - wsz + 1, w - wsz + 1)
        x0 = nd - 1 + mind + w2                                                        # first centre column with every window inside
        vol[bi, w2:h - w2, x0:w - w2] = s[:, x0 - w2:]
    return vol


# --------------------------------------------------------------------------------------------------------------------------
# the cases; each returns the kernel name it ran. `tagged`: False under SBM_FAST_PFSHIFT=0 / =1 (the child process)
# --------------------------------------------------------------------------------------------------------------------------

def case_ties(pkg, oracle, par, nd, wsz, want):
    """Flat and two-level images, every sum ties: the winner stays the first index across the tag-group boundaries."""
    names = []
    for mk in (flat_pair, two_level_pair):
        for uniq in (0, 10):
            L, R = mk(nd, wsz, n=2)
            kw = dict(KW, num_disparities=nd, block_size=wsz, uniqueness_ratio=uniq)
            eng, ref, name = check_case(pkg, oracle, par, kw, L, R, want)
            names.append(name)
            if mk is flat_pair and uniq == 0:
                # all sums are 0: buffer index 0 wins everywhere = disparity nd - 1
                h, w = L.shape[1:]
                inner = ref["pre_lr"][:, wsz:h - wsz, nd + wsz:w - wsz]
                assert inner.size and (inner >> 4 == nd - 1).all()
    return names


def case_envelope(pkg, oracle, par, nd, wsz, want, uniq=10):
    L, R = envelope_pair(nd, wsz, n=2)
    kw = dict(KW, num_disparities=nd, block_size=wsz, uniqueness_ratio=uniq)
    eng, ref, name = check_case(pkg, oracle, par, kw, L, R, want)
    # the construction reaches the envelope maximum (on the oracle's own prefiltered planes)
    vol = sad_volume(ref["pf_l"][0], ref["pf_r"][0], nd, wsz)
    assert vol.max() == wsz * wsz * 2 * 31, (int(vol.max()), wsz * wsz * 2 * 31)
    return [name]


def case_rival(pkg, oracle, par, want):
    """A periodic texture (period 40 columns at 128 disparities: three near-equal minima, each in another tag group of 32 buffer
    indices) under small noise: among ~10^4 pixels some have their only rival -- outside mind +- 1 and in another tag group than
    the winner -- exactly at thresh (rejected) and exactly at thresh + 1 (accepted). Both must occur; the maps must be equal."""
    nd, wsz, uniq = 128, 15, 10
    h, w = 70, nd + 330
    rng = np.random.default_rng(4242)
    tile = rng.integers(0, 256, (h, 40), dtype=np.uint8)
    base = np.tile(tile, (1, (w + nd) // 40 + 2))
    Ls, Rs = [], []
    for i in range(4):
        Ls.append(np.clip(base[:, 45:45 + w].astype(int) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8))
        Rs.append(np.clip(base[:, 50:50 + w].astype(int) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8))
    L, R = np.stack(Ls), np.stack(Rs)
    kw = dict(KW, num_disparities=nd, block_size=wsz, uniqueness_ratio=uniq)
    eng, ref, name = check_case(pkg, oracle, par, kw, L, R, want)
    at, above = 0, 0
    for i in range(L.shape[0]):
        vol = sad_volume(ref["pf_l"][i], ref["pf_r"][i], nd, wsz)
        ok = vol[0] >= 0
        big = np.where(vol < 0, np.int64(1) << 40, vol)
        mind = big.argmin(0)                                  # first index attaining the minimum
        ms = big.min(0)
        thresh = ms + ms * uniq // 100
        idx = np.arange(nd)[:, None, None]
        outside = np.abs(idx - mind[None]) > 1
        rivals = np.where(outside, big, np.int64(1) << 40)
        r1 = rivals.argmin(0)
        r1v = rivals.min(0)
        rivals2 = np.where(idx == r1[None], np.int64(1) << 40, rivals)
        single = rivals2.min(0) > thresh + 1                  # the only rival near the threshold
        other = (r1 // (nd // 4)) != (mind // (nd // 4))
        sel = ok & single & other & (ms > 0)
        at += int((sel & (r1v == thresh)).sum())
        above += int((sel & (r1v == thresh + 1)).sum())
    assert at > 0 and above > 0, (at, above)
    return [name]


def case_ends(pkg, oracle, par, nd, wsz, want):
    """The minimum at buffer index 0 and at nd - 1: mirrored sub-pixel neighbours."""
    names = []
    for shift in (nd - 1, 0):
        L, R = textured_pair(nd, wsz, shift, n=2, seed=shift)
        kw = dict(KW, num_disparities=nd, block_size=wsz, uniqueness_ratio=10, texture_threshold=10)
        eng, ref, name = check_case(pkg, oracle, par, kw, L, R, want)
        names.append(name)
        valid = ref["pre_lr"][ref["pre_lr"] >= 0]
        assert valid.size and ((valid + 8) >> 4 == shift).mean() > 0.9, shift
    return names


def case_filled_chip(pkg, oracle, par, nd, wsz, want, n=32):
    """Enough pairs and rows for the layouts of a launch that fills the chip (one wavefront up to 128 disparities, two beyond):
    3 strips x 32 pairs x ~32 row segments of 8 rows are beyond the 1 800 workgroups under which launch_sad_fast() splits."""
    Lt, Rt = two_level_pair(nd, wsz, n=n // 2)
    Lx, Rx = textured_pair(nd, wsz, 7, n=n // 2)
    h, w = 280, Lt.shape[2]
    L = np.concatenate([np.tile(Lt, (1, 10, 1))[:, :h], np.tile(Lx, (1, 10, 1))[:, :h]])
    R = np.concatenate([np.tile(Rt, (1, 10, 1))[:, :h], np.tile(Rx, (1, 10, 1))[:, :h]])
    kw = dict(KW, num_disparities=nd, block_size=wsz, uniqueness_ratio=10)
    eng, ref, name = check_case(pkg, oracle, par, kw, L, R, want)
    return [name]


def untagged_cases(pkg, oracle, par, want15, want21):
    """What the child process runs under SBM_FAST_PFSHIFT=0 / =1: the same images through the untagged start."""
    names = []
    names += case_ties(pkg, oracle, par, 128, 15, want15)
    names += case_ties(pkg, oracle, par, 64, 21, want21)
    names += case_envelope(pkg, oracle, par, 128, 15, want15)
    names += case_envelope(pkg, oracle, par, 64, 21, want21)
    names += case_ends(pkg, oracle, par, 64, 15, want15)
    names += case_rival(pkg, oracle, par, want15)
    return names


# --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    pkg, oracle = _env()
    return pkg, oracle, _parity()


@pytest.mark.gpu
@pytest.mark.parametrize("wsz", [15, 21])
@pytest.mark.parametrize("nd", LAYOUT_ND)
def test_ties_in_every_layout(ctx, nd, wsz):
    """One-pair-sized launches: the `split` layouts (two to four narrower wavefronts) and three / four 128-disparity wavefronts."""
    names = case_ties(*ctx, nd, wsz, None)
    ndw, nw, exact = layout(names[0])
    assert ndw * nw >= nd and exact == (ndw * nw == nd and (ndw, nw) != (64, 4)), names[0]


@pytest.mark.gpu
@pytest.mark.parametrize("nd,wsz,lay", [(32, 15, (32, 1)), (64, 15, (64, 1)), (128, 15, (128, 1)), (96, 15, (128, 1)), (256, 15, (128, 2)),
                                        (160, 21, (128, 2)), (64, 21, (64, 1)), (128, 21, (128, 1))])
def test_ties_in_the_layouts_of_a_filled_chip(ctx, nd, wsz, lay):
    names = case_filled_chip(*ctx, nd, wsz, None)
    assert layout(names[0])[:2] == lay, names[0]


@pytest.mark.gpu
@pytest.mark.parametrize("nd,wsz", [(128, 15), (64, 15), (256, 15), (128, 21), (64, 21), (192, 21), (64, 9), (160, 9), (64, 19), (128, 19)])
@pytest.mark.parametrize("uniq", [10, 40])
def test_sums_at_the_envelope_maximum(ctx, nd, wsz, uniq):
    """cap 31: w 15 and 9 carry two tag bits, 21 and 19 one; (maxS << bits) + tag is within 3 % of 65535 at w 15 / 21."""
    case_envelope(*ctx, nd, wsz, None, uniq=uniq)


@pytest.mark.gpu
def test_window_23_runs_untagged_and_stays_exact(ctx):
    """2 * maxS + 1 does not fit 16 bits at w 23, cap 31: no pre-scaled planes, plain keys, accumulators start at 0."""
    assert tag_bits(23) == 0
    case_envelope(*ctx, 64, 23, 0)
    case_ties(*ctx, 128, 23, 0)


@pytest.mark.gpu
def test_rival_in_another_tag_group_at_the_threshold(ctx):
    case_rival(*ctx, None)


@pytest.mark.gpu
@pytest.mark.parametrize("nd,wsz", [(32, 15), (64, 15), (128, 15), (256, 15), (96, 15), (64, 21), (128, 21), (384, 21), (128, 9), (64, 19)])
def test_minimum_at_both_ends_of_the_range(ctx, nd, wsz):
    case_ends(*ctx, nd, wsz, None)


@pytest.mark.gpu
@pytest.mark.parametrize("nd,wsz", [(128, 15), (64, 21), (160, 15), (256, 21)])
def test_plain_strips_only(ctx, nd, wsz, monkeypatch):
    """SBM_FAST_CS3=0 (read per call): lane distance 3 between the partners of a window, carriers in runs of three lanes."""
    monkeypatch.setenv("SBM_FAST_CS3", "0")
    case_ties(*ctx, nd, wsz, None)
    case_envelope(*ctx, nd, wsz, None)
    case_ends(*ctx, nd, wsz, None)


@pytest.mark.gpu
@pytest.mark.parametrize("pfshift,want15,want21", [("0", 0, 0), ("1", 0, 1)])
def test_untagged_start(pfshift, want15, want21):
    """SBM_FAST_PFSHIFT=0: unscaled planes everywhere. =1: w 15 holds the two-bit variant only and runs untagged, w 21 keeps its
    one tag bit. The switch is read once per process, hence the child."""
    env = dict(os.environ, SBM_FAST_PFSHIFT=pfshift)
    r = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve()), str(want15), str(want21)], capture_output=True, text=True,
                       timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    names = json.loads([l for l in r.stdout.splitlines() if l.startswith("[")][-1])
    assert names and all(n.endswith("pfshift=0") for n in names if ",5,3," in n), names
    assert any(n.endswith(f"pfshift={want21}") for n in names if ",7,3," in n), names


if __name__ == "__main__":
    pkg_, oracle_ = _env()
    print(json.dumps(untagged_cases(pkg_, oracle_, _parity(), int(sys.argv[1]), int(sys.argv[2]))))
