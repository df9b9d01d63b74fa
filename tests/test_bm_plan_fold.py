"""Which launches run their last strip folded over its disparity halves (sad_fast_fold_cols, csrc/sbm_sad_fast.hip;
the strip: csrc/sbm_sad_fast_fold.h), through the debug query sbm_debug_fold; no device.

The last plain strip folds when it has R <= 22 columns, the window is 15, the count exactly 128 and the layout the lone
wavefront. At 128 disparities and window 15 a pair of width W has W - 141 interior columns; a stride-3 triple takes 180 of
them, a plain strip 52."""
import ctypes

import pytest

import test_bm_plan as plan


def case(W, H, n, nd, w, **env):
    return dict(W=W, H=H, n=n, nd=nd, w=w, mind=0, roi=None, inplace=1, env=env, cap=31, uniq=10, tex=10, d12=1, spk_win=50, spk_range=32)


def fold_cols(pkg, monkeypatch, c, fold=None):
    """sbm_debug_fold of a case: the columns of its folded strip, 0 where nothing folds. fold: SBM_FAST_FOLD, None = unset."""
    if fold is None:
        monkeypatch.delenv("SBM_FAST_FOLD", raising=False)
    else:
        monkeypatch.setenv("SBM_FAST_FOLD", str(fold))
    for k, v in c["env"].items():
        monkeypatch.setenv(k, str(v))
    fn = pkg.load_library().sbm_debug_fold
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    out = (ctypes.c_int * 1)(-1)
    assert fn(ctypes.byref(plan.make_params(pkg, c)), c["n"], c["W"], c["H"], c["inplace"], out) == plan.OK
    return int(out[0])


def test_kitti_folds_its_21_columns(pkg, monkeypatch):
    c = case(1242, 375, 64, 128, 15)
    st, pl = plan.query(pkg, c)
    assert st == plan.OK and pl.fast
    assert (pl.f.strips3, pl.f.strips, pl.f.NDW, pl.f.NWAVES, pl.f.exact) == (18, 19, 128, 1, 1)
    assert pl.kernel.decode().startswith("sad_fast_kernel<128,1,5,3,true,true>")
    assert fold_cols(pkg, monkeypatch, c) == 21
    assert fold_cols(pkg, monkeypatch, c, fold=1) == 21


# (W, H, pairs) that reach the lone 128-disparity wavefront: R columns alone, and behind one stride-3 triple
@pytest.mark.parametrize("base, n", [(141, 64), (141 + 180, 64), (141 + 6 * 180, 64)])
@pytest.mark.parametrize("R, folds", [(1, True), (21, True), (22, True), (23, False), (52, False)])
def test_the_remainder_decides(pkg, monkeypatch, base, n, R, folds):
    c = case(base + R, 526, n, 128, 15)
    st, pl = plan.query(pkg, c)
    assert st == plan.OK and pl.fast and pl.f.NWAVES == 1 and pl.f.exact and pl.f.strips == pl.f.strips3 + 1
    assert pl.f.xc1 - pl.f.xc0 == base - 141 + R
    assert fold_cols(pkg, monkeypatch, c) == (R if folds else 0)
    assert fold_cols(pkg, monkeypatch, c, fold=0) == 0


def test_only_the_last_plain_strip_counts(pkg, monkeypatch):
    """Plain strips only (SBM_FAST_CS3=0): 52 columns each, the last one folds on its own remainder."""
    assert fold_cols(pkg, monkeypatch, case(141 + 3 * 52 + 9, 526, 64, 128, 15, SBM_FAST_CS3=0)) == 9
    assert fold_cols(pkg, monkeypatch, case(141 + 3 * 52 + 30, 526, 64, 128, 15, SBM_FAST_CS3=0)) == 0
    # two remainders' worth of columns become one more triple: no plain strip, nothing to fold
    c = case(141 + 180 + 110, 526, 64, 128, 15)
    st, pl = plan.query(pkg, c)
    assert pl.f.strips == pl.f.strips3 == 6
    assert fold_cols(pkg, monkeypatch, c) == 0


@pytest.mark.parametrize("what, c", [
    ("a masked count", case(1242, 375, 64, 112, 15)),
    ("64 disparities", case(1242, 375, 64, 64, 15)),
    ("256 disparities", case(1242, 375, 64, 256, 15)),
    ("window 21", case(1242 - 12, 375, 64, 128, 21)),
    ("window 9", case(1242, 375, 64, 128, 9)),
    ("cooperating wavefronts (one pair: split)", case(1242, 375, 1, 128, 15)),
    ("no in-place accumulate", dict(case(1242, 375, 64, 128, 15), inplace=0)),
])
def test_nothing_else_folds(pkg, monkeypatch, what, c):
    st, pl = plan.query(pkg, c)
    assert st == plan.OK
    assert fold_cols(pkg, monkeypatch, c) == 0, what
    assert fold_cols(pkg, monkeypatch, c, fold=0) == 0, what


def test_the_switch_leaves_the_plan_alone(pkg, monkeypatch):
    """SBM_FAST_FOLD changes which body the last strip runs, nothing the plan holds: grid, LDS, segments, hand-off slots."""
    c = case(1242, 375, 64, 128, 15)
    plans = []
    for v in ("0", "1"):
        monkeypatch.setenv("SBM_FAST_FOLD", v)
        st, pl = plan.query(pkg, c)
        assert st == plan.OK
        plans.append(bytes(pl))
    assert plans[0] == plans[1]
