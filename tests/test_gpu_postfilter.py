"""The device post-filters (sbm_lrcheck.hip, sbm_speckle.hip) on the designed maps of tests/postfilter_cases.py, handed to them by
sbm_debug_postfilter: every speckle case under every kernel variant, every LR case at the widths that reach every instantiation
of launch_lrcheck, both stages together, repeated runs of the racing cases, stale scratch, the cost invariant the entry otherwise
supplies itself, and the alternative readings. SBM_FAST_INPLACE is read once per process, so everything that wants the int32
cost plane on the interior kernel's envelope runs in one child process (this file run as a script). Every comparison is bit for bit against the CPU oracle, and against the cases' own
closed forms where they have one; `info` must name the kernel each test was written for."""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import postfilter_cases as pc  # noqa: E402
from gpu_support import torch_cuda  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SPECKLE = pc.speckle_cases()
SPK_BY = {c["name"]: c for c in SPECKLE}
LR_FAST = pc.lr_cases_fast()
LR_GENERIC = pc.lr_cases_generic()
LR_INT32 = pc.lr_cases_int32()
VARIANTS = [(1, 2, 1), (1, 2, 2), (1, 2, 4), (1, 4, 1), (1, 4, 2), (1, 4, 4), (1, -1, 0), (0, -1, 0)]   # SBM_SPECKLE_LISTS, _BAND, _SEG
SOME_VARIANTS = [(1, 2, 4), (1, 4, 2), (1, -1, 0), (0, -1, 0)]
_WANT = {}


def vid(v):
    return "lists%d_band%d_seg%d" % v


def set_variant(monkeypatch, v):
    for name, val in zip(("SBM_SPECKLE_LISTS", "SBM_SPECKLE_BAND", "SBM_SPECKLE_SEG"), v):
        monkeypatch.setenv(name, str(val))


def spk_engine(pkg, case):
    bm = pkg.StereoBM.create(pc.SPK_ND, 5)
    bm.setMinDisparity(pc.SPK_MIND)
    bm.setSpeckleWindowSize(case["max_size"])
    bm.setSpeckleRange(case["max_diff"])
    return bm


def spk_want(oracle, case):
    """The oracle's result, computed once per case and left alone."""
    if case["name"] not in _WANT:
        w = np.stack([oracle.filter_speckles(m, case["newval"], case["max_size"], case["max_diff"]) for m in case["maps"]])
        w.setflags(write=False)
        _WANT[case["name"]] = w
    return _WANT[case["name"]]


def spk_plan(variant, case):
    """lists, G, S, SW as speckle_plan chooses them for this variant and map: S falls back on maps of fewer chunks than segments."""
    lists, band, seg = variant
    n, H, W = case["maps"].shape
    if not lists or case["max_size"] > 2048:
        return dict(lists=0, G=0, S=0, SW=0)
    G = band if band in (2, 4) else 2
    S = seg if seg in (1, 2, 4) else 4
    chunks = (W + 63) // 64
    while S > 1 and chunks < S:
        S //= 2
    return dict(lists=1, G=G, S=S, SW=64 * ((chunks + S - 1) // S))


def run_speckle(bm, oracle, case, variant):
    got, info = bm.debug_postfilter(case["maps"], None, stages=2)
    assert info["stages"] == 2 and info["speckle"] == 1 and info["lr_kernel"] == -1
    assert {k: info[k] for k in ("lists", "G", "S", "SW")} == spk_plan(variant, case)
    assert info["max_diff"] == min(case["max_diff"], 1 << 17)
    assert np.array_equal(got, spk_want(oracle, case)), int((got != spk_want(oracle, case)).sum())
    if case["keep"] is not None:
        assert np.array_equal(got, pc.spk_expected(case))
    return got, info


@pytest.mark.parametrize("case", SPECKLE, ids=[c["name"] for c in SPECKLE])
@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
def test_speckle_case(torch_cuda, pkg, oracle, monkeypatch, variant, case):
    set_variant(monkeypatch, variant)
    run_speckle(spk_engine(pkg, case), oracle, case, variant)


@pytest.mark.parametrize("name", pc.RACE_CASES)
@pytest.mark.parametrize("variant", SOME_VARIANTS, ids=vid)
def test_racing_cases_repeat(torch_cuda, pkg, oracle, monkeypatch, variant, name):
    """Size sums that race at max_size / max_size + 1 and seam unions that race along a chain: five runs on one handle."""
    set_variant(monkeypatch, variant)
    bm = spk_engine(pkg, SPK_BY[name])
    for _ in range(5):
        run_speckle(bm, oracle, SPK_BY[name], variant)


@pytest.mark.parametrize("variant", SOME_VARIANTS, ids=vid)
def test_nothing_stale_is_read_from_the_scratch(torch_cuda, pkg, oracle, monkeypatch, variant):
    """Most runs and seam contacts, then a few islands, then the stripes again, on one handle: each equals what a handle without any
    scratch gives (the pool of parked handles is emptied first), so no record, run count or seam list of the call before is read."""
    set_variant(monkeypatch, variant)
    a, b = (SPK_BY[n] for n in pc.STALE_PAIR)
    fresh = {}
    for c in (a, b):
        pkg.trim()
        fresh[c["name"]] = run_speckle(spk_engine(pkg, c), oracle, c, variant)[0]
    pkg.trim()
    bm = spk_engine(pkg, a)
    for c in (a, b, a):
        bm.setSpeckleWindowSize(c["max_size"])
        got, _ = run_speckle(bm, oracle, c, variant)
        assert np.array_equal(got, fresh[c["name"]])


# ---- LR check -----------------------------------------------------------------------------------------------------------------
def lr_engine(pkg, case, speckle=None):
    bm = pkg.StereoBM.create(case["nd"], pc.LR_BLOCK)
    bm.setMinDisparity(case["mind"])
    bm.setDisp12MaxDiff(case["d12"])
    if speckle:
        bm.setSpeckleWindowSize(speckle[0])
        bm.setSpeckleRange(speckle[1])
    return bm


def run_lr(bm, oracle, case, validate=None):
    got, info = bm.debug_postfilter(case["pre"], case["cost"], stages=1)
    assert info["stages"] == 1 and info["speckle"] == 0
    assert (info["row0"], info["row1"]) == (2, pc.LR_H - 2) and info["col1"] > info["col0"]
    want = pc.lr_device_expected(validate or oracle.validate_disparity, case, info)
    assert np.array_equal(got, want), int((got != want).sum())
    if validate is None:
        # the closed forms, where the valid ROI and the computed columns leave the designed pixels alone
        lo, hi = max(info["col0"], info["lofs"]), min(info["col1"], info["lofs"] + info["xend"])
        for r, (m, y) in zip(case["rows"], case["where"]):
            if r["designed"]:
                assert np.array_equal(got[m, y, lo:hi], pc.lr_row_expected(r, case["mind"])[lo:hi]), r["name"]
    return info


FAST_KERNEL = dict(pc.LR_FAST_WIDTHS)


@pytest.mark.parametrize("case", LR_FAST, ids=[c["name"] for c in LR_FAST])
def test_lr_case(torch_cuda, pkg, oracle, case):
    info = run_lr(lr_engine(pkg, case), oracle, case)
    assert info["cost16"] == 1 and info["lr_kernel"] == pkg.StereoBM.LR_FAST16
    assert (info["nit"], info["px"]) == FAST_KERNEL.get(case["W"], (5, 2))      # (1100 columns, the clamp cases: 5 x 2)
    assert info["bs"] % 64 == 0 and info["bs"] * info["nit"] * info["px"] >= case["W"]


@pytest.mark.parametrize("case", LR_GENERIC, ids=[c["name"] for c in LR_GENERIC])
def test_lr_case_on_the_generic_kernels(torch_cuda, pkg, oracle, case):
    info = run_lr(lr_engine(pkg, case), oracle, case)
    assert info["lr_kernel"] == (pkg.StereoBM.LR_GENERIC_GLOBAL if case["W"] > 8192 else pkg.StereoBM.LR_GENERIC_LDS)
    assert info["cost16"] == (0 if case["nd"] > 512 else 1)


# ---- both stages --------------------------------------------------------------------------------------------------------------
def cut_band_case(W=200, H=14, mind=0, nd=16, d12=1):
    """A band of one disparity over the whole map, cut by the LR check: at every cut column x a cheaper pixel three columns on claims
    the right-view column of x with a disparity 48 away, so x dies, the claimant stays as a one-pixel column of another value, and
    the two columns between them become a strip of their own. Cuts 5 columns apart leave pieces of 1 or 2 columns (erased at
    max_size 60: 10 matched rows), cuts 40 apart leave pieces the speckle filter keeps."""
    k = 4
    pre = np.full((2, H, W), 16 * k, np.int16)
    cost = np.full((2, H, W), 10, np.int32)
    cuts = [30, 35, 40, 45, 90, 130, 135, 170]
    for x in cuts:
        pre[:, :, x + 3] = 16 * (k + 3)
        cost[:, :, x + 3] = 5
    pre[1, :, :] = (mind - 1) * 16      # the second map: nothing at all
    return dict(name="cut_band", W=W, mind=mind, nd=nd, d12=d12, pre=pre, cost=cost, cuts=cuts, k=k)


def check_cut_band(pkg, oracle, inplace):
    case = cut_band_case()
    bm = lr_engine(pkg, case, speckle=(60, 32))
    after_lr, _ = bm.debug_postfilter(case["pre"], case["cost"], stages=1)
    got, info = bm.debug_postfilter(case["pre"], case["cost"], stages=3)
    assert info["stages"] == 3 and info["speckle"] == 1 and info["lr_kernel"] == (1 if inplace else 2) and info["cost16"] == inplace
    inv = np.int16(-16)
    lr = pc.lr_device_expected(oracle.validate_disparity, case, info)
    assert np.array_equal(after_lr, lr)
    want = np.stack([oracle.filter_speckles(m, int(inv), 60, 32) for m in lr])
    assert np.array_equal(got, want), int((got != want).sum())
    # closed form: the cut columns die in the LR check; claimant columns and pieces of at most 6 columns go in the speckle filter
    rows = slice(info["row0"], info["row1"])
    for x in case["cuts"]:
        assert (after_lr[0, rows, x] == inv).all() and (after_lr[0, rows, x + 1:x + 4] != inv).all()
        assert (got[0, rows, x:x + 4] == inv).all()
    assert (after_lr[0, rows, 41:45] != inv).all() and (got[0, rows, 31:49] == inv).all()
    assert (got[0, rows, 49:90] == 16 * case["k"]).all() and (got[0, rows, 94:130] == 16 * case["k"]).all()
    assert (got[1] == inv).all()


@pytest.mark.parametrize("variant", SOME_VARIANTS, ids=vid)
def test_lr_erasures_cut_components_the_speckle_filter_removes(torch_cuda, pkg, oracle, monkeypatch, variant):
    set_variant(monkeypatch, variant)
    check_cut_band(pkg, oracle, 1)


# ---- the int32 cost plane on the interior kernel's envelope: one child process ------------------------------------------------------
def int32_plane_sweep(pkg, oracle):
    """Runs under SBM_FAST_INPLACE=0: every fast-path LR case again (same input, int32 plane, generic kernel), costs beyond 16 bits,
    the 8193-column row with int32 costs, and both stages under the speckle variants. Returns what `info` named."""
    seen = set()
    for case in LR_FAST + LR_INT32 + LR_GENERIC[:2]:
        info = run_lr(lr_engine(pkg, case), oracle, case)
        assert info["cost16"] == 0 and info["nit"] == 0
        assert info["lr_kernel"] == (pkg.StereoBM.LR_GENERIC_GLOBAL if case["W"] > 8192 else pkg.StereoBM.LR_GENERIC_LDS)
        seen.add(info["lr_kernel"])
    for v in SOME_VARIANTS:
        for name, val in zip(("SBM_SPECKLE_LISTS", "SBM_SPECKLE_BAND", "SBM_SPECKLE_SEG"), v):
            os.environ[name] = str(val)
        check_cut_band(pkg, oracle, 0)
    return dict(cases=len(LR_FAST + LR_INT32) + 2, kernels=sorted(seen))


def test_int32_cost_plane_on_the_same_inputs(torch_cuda):
    env = dict(os.environ, SBM_FAST_INPLACE="0")
    r = subprocess.run([sys.executable, str(pathlib.Path(__file__).resolve())], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    res = json.loads([line for line in r.stdout.splitlines() if line.startswith("{")][-1])
    assert res == dict(cases=len(LR_FAST) + len(LR_INT32) + 2, kernels=[2, 3])


# ---- the invariant the entry supplies itself: SAD stores cost 0xffff with every filtered pixel --------------------------------------
def test_sad_kernels_store_cost_ffff_with_every_filtered_pixel(torch_cuda, pkg):
    """lrcheck16_kernel's inner wavefronts let filtered pixels take part in the claims because their cost reads 0xffff. On a small
    pair of the fast path: debug_fetch(2) reads 65535 wherever debug_fetch(3) reports a filtered pixel, over the matched rows and the
    computed columns."""
    from u96_slam_amd import synth

    n, W, H, nd = 2, 320, 96, 64
    L, R = synth.make_batch(3, n, W, H, nd)
    bm = pkg.StereoBM.create(nd, 15)
    bm.setUniquenessRatio(10)
    bm.setDisp12MaxDiff(1)
    _, info = bm.debug_postfilter(np.full((n, H, W), -16, np.int16), np.zeros((n, H, W), np.int32), stages=1)
    assert info["cost16"] == 1 and info["lr_kernel"] == 1
    bm.compute(torch_cuda.from_numpy(L).to("cuda:0"), torch_cuda.from_numpy(R).to("cuda:0"))
    cost, pre = bm.debug_fetch(2, n, H, W), bm.debug_fetch(3, n, H, W)
    reg = (slice(None), slice(info["row0"], info["row1"]), slice(info["lofs"], info["lofs"] + info["xend"]))
    filtered = pre[reg] == -16
    assert filtered.any() and (~filtered).any()
    assert (cost[reg][filtered] == 65535).all(), int((cost[reg][filtered] != 65535).sum())
    assert (cost[reg][~filtered] <= 65534).all()


# ---- alternative readings ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [(1, -1, 0), (0, -1, 0)], ids=vid)
def test_reading_speckle_range_times_16(torch_cuda, pkg, oracle, monkeypatch, variant):
    """SBM_CV_READING=4: neighbours 100 apart join at speckleRange 8 (x 16 = 128), and do not without the reading."""
    set_variant(monkeypatch, variant)
    case = pc.ramp(10, 257, 100, 8, 50)
    bm = spk_engine(pkg, case)
    got, info = bm.debug_postfilter(case["maps"], None, stages=2)
    assert info["max_diff"] == 8 and (got == case["newval"]).all()
    monkeypatch.setenv("SBM_CV_READING", "4")
    got, info = bm.debug_postfilter(case["maps"], None, stages=2)
    assert info["max_diff"] == 128
    # (the oracle's reading lives in its compute(), which scales the range it hands to filter_speckles: the same call here)
    want = oracle.filter_speckles(case["maps"][0], case["newval"], 50, 8 * 16)
    assert np.array_equal(got[0], want) and np.array_equal(got, case["maps"])


def test_reading_lr_tie_goes_to_the_later_pixel(torch_cuda, pkg, oracle, monkeypatch):
    """SBM_CV_READING=16: on equal cost the later x takes the column -- the generic kernel, against the oracle under the same reading."""
    case = pc.lr_case(386, 0, 16, 1)
    monkeypatch.setenv("SBM_CV_READING", "16")

    def validate(*a):
        with oracle.reading(oracle.READ_LR_TIE_LATER):
            return oracle.validate_disparity(*a)

    info = run_lr(lr_engine(pkg, case), oracle, case, validate)
    assert info["lr_kernel"] == pkg.StereoBM.LR_GENERIC_LDS
    got, _ = lr_engine(pkg, case).debug_postfilter(case["pre"], case["cost"], stages=1)
    monkeypatch.delenv("SBM_CV_READING")
    plain, _ = lr_engine(pkg, case).debug_postfilter(case["pre"], case["cost"], stages=1)
    assert not np.array_equal(got, plain)      # the designed ties make the two readings differ


# ---- the entry itself ------------------------------------------------------------------------------------------------------------
def test_entry_refuses_what_the_sad_kernels_cannot_produce(torch_cuda, pkg):
    case = LR_FAST[0]
    bm = lr_engine(pkg, case)
    pre, cost = case["pre"].copy(), case["cost"].copy()
    top = (case["mind"] + case["nd"] - 1) * 16

    def code(p, c, stages=1):
        with pytest.raises(pkg.StereoBMError) as e:
            bm.debug_postfilter(p, c, stages)
        return e.value.code

    bad = pre.copy(); bad[0, 2, 50] = top + 1
    assert code(bad, cost) == -23
    bad = pre.copy(); bad[0, 0, 0] = case["mind"] * 16 - 1 if case["mind"] * 16 - 1 != (case["mind"] - 1) * 16 else case["mind"] * 16 - 2
    assert code(bad, cost) == -23
    valid = np.argwhere(pre != (case["mind"] - 1) * 16)[0]
    bad = cost.copy(); bad[tuple(valid)] = 65535
    assert code(pre, bad) == -23                         # a valid pixel's cost beyond 65534 on the 16-bit plane
    bad = cost.copy(); bad[tuple(valid)] = -1
    assert code(pre, bad) == -23
    assert code(pre, None) == -1                         # the LR check reads the costs
    assert code(pre, cost, stages=2) == -23              # this matcher has no speckle filter
    assert code(pre, cost, stages=0) == -23
    filt = np.argwhere(pre == (case["mind"] - 1) * 16)[0]
    ok = cost.copy(); ok[tuple(filt)] = 1 << 20          # a filtered pixel's cost is the entry's business
    got, _ = bm.debug_postfilter(pre, ok, 1)
    assert np.array_equal(got, bm.debug_postfilter(pre, cost, 1)[0])


def test_every_kernel_the_post_filters_have_ran(torch_cuda, pkg, oracle, monkeypatch):
    """One small case per speckle variant and one per LR width, collected from `info`: the eight speckle variants, the eight
    lrcheck16 instantiations, both generic LR kernels and the row-walking speckle kernels beyond 2048 all ran, and on these inputs."""
    seen_spk, seen_lr = set(), set()
    case = SPK_BY["islands_18x320_max9"]
    for v in VARIANTS:
        set_variant(monkeypatch, v)
        _, info = run_speckle(spk_engine(pkg, case), oracle, case, v)
        seen_spk.add((info["lists"], info["G"], info["S"], info["SW"]))
    assert seen_spk == {(1, 2, 1, 320), (1, 2, 2, 192), (1, 2, 4, 128), (1, 4, 1, 320), (1, 4, 2, 192), (1, 4, 4, 128), (0, 0, 0, 0)}
    set_variant(monkeypatch, (1, -1, 0))
    beyond = SPK_BY["snake_18x257_max2049_size2050"]      # maxSpeckleSize beyond 2048: the row-walking kernels whatever the switches
    _, info = run_speckle(spk_engine(pkg, beyond), oracle, beyond, (1, -1, 0))
    assert info["lists"] == 0
    done = set()
    for c in LR_FAST:
        if c["W"] in FAST_KERNEL and c["W"] not in done:
            done.add(c["W"])
            info = run_lr(lr_engine(pkg, c), oracle, c)
            seen_lr.add((info["lr_kernel"], info["nit"], info["px"]))
    for c in LR_GENERIC[:2]:
        info = run_lr(lr_engine(pkg, c), oracle, c)
        seen_lr.add((info["lr_kernel"], info["nit"], info["px"]))
    assert seen_lr == {(1, n, 2) for n in (1, 2, 3, 4, 5)} | {(1, n, 4) for n in (2, 3, 4)} | {(2, 0, 0), (3, 0, 0)}


if __name__ == "__main__":     # the child of test_int32_cost_plane_on_the_same_inputs
    ROOT = pathlib.Path(__file__).resolve().parents[1]
    sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "oracle"))
    import _pkg
    import sbm_oracle

    assert os.environ.get("SBM_FAST_INPLACE") == "0"
    print(json.dumps(int32_plane_sweep(_pkg.load(), sbm_oracle)))
