"""The designed post-filter maps of tests/postfilter_cases.py are what they claim (no GPU): for every case the oracle, the numpy
restatement and the case's own closed form agree, the case keeps its promises (component sizes, runs per row, contacts per seam,
gadget counts), it erases something and keeps something unless it is one-sided on purpose, and it meets the input contract of
sbm_debug_postfilter."""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import postfilter_cases as pc  # noqa: E402

SPECKLE = pc.speckle_cases()
LR = pc.lr_cases_fast() + pc.lr_cases_generic() + pc.lr_cases_int32()


@pytest.mark.parametrize("case", SPECKLE, ids=[c["name"] for c in SPECKLE])
def test_speckle_case(oracle, case):
    nv, ms, md = case["newval"], case["max_size"], case["max_diff"]
    assert 0 < ms and (ms <= 2048 or "max2049" in case["name"])
    assert pc.contract_ok(case["maps"], pc.SPK_MIND, pc.SPK_ND)
    erased = kept = False
    for i, img in enumerate(case["maps"]):
        want = oracle.filter_speckles(img, nv, ms, md)
        assert np.array_equal(want, pc.np_speckles(img, nv, ms, md))
        if case["keep"] is not None:
            assert np.array_equal(want, pc.spk_expected(case)[i])
        valid = img != nv
        erased |= bool((valid & (want == nv)).any())
        kept |= bool((want != nv).any())
        if case["ids"] is not None:
            # the shapes are the components, and their arithmetic sizes are their pixel counts
            ids, lab = case["ids"][i], pc.np_components(img, nv, md)
            assert np.array_equal(ids != 0, valid)
            counts = np.bincount(ids.ravel(), minlength=len(case["sizes"][i]) + 1)[1:]
            assert counts.tolist() == [case["sizes"][i][k] for k in sorted(case["sizes"][i])]
            pairs = np.unique(np.stack([ids[valid], lab[valid]]), axis=1)
            assert pairs.shape[1] == len(case["sizes"][i]) == np.unique(pairs[1]).size
    if not (case["maps"] != nv).any():
        assert case["one_sided"] and not erased and not kept
    else:
        assert (erased and kept) == (not case["one_sided"]), (erased, kept)
    pr, img = case["promises"], case["maps"][0]
    H = img.shape[0]
    live = [y for y in range(H) if (img[y] != nv).any()]
    if "runs_per_row" in pr:
        assert all(pc.count_runs(img[y], nv, md) == pr["runs_per_row"] for y in live)
    if "contacts_per_seam" in pr:
        assert all(pc.count_contacts(img[y], img[y + 1], nv, md) == pr["contacts_per_seam"] for y in live[:-1])
        # 64 per pair of rows and chunk: what fills the band walk's contact list until it is flushed mid-walk
        W = img.shape[1]
        assert all(pc.count_contacts(img[0, c:c + 64], img[1, c:c + 64], nv, md) == min(64, W - c) for c in range(0, W, 64))
    if "component_size" in pr:
        assert pr["component_size"] in case["sizes"][0].values()
    if "components" in pr:
        lab = pc.np_components(img, nv, md)
        assert np.unique(lab[img != nv]).size == pr["components"]
    if "loose" in pr:
        assert sum(s == pr["loose"] for s in case["sizes"][0].values()) >= 2 and pr["loose"] <= ms
    if "sizes" in pr:
        assert set(case["sizes"][0].values()) == pr["sizes"]
    if "neighbour_step" in pr:
        v = img.astype(int)
        assert (np.abs(np.diff(v, axis=0)) == pr["neighbour_step"]).all() and (np.abs(np.diff(v, axis=1)) == pr["neighbour_step"]).all()


def test_speckle_cases_cover_what_they_were_designed_for():
    by = {c["name"]: c for c in SPECKLE}
    for name in pc.RACE_CASES + pc.STALE_PAIR:
        assert name in by
    assert by[pc.STALE_PAIR[0]]["maps"].shape == by[pc.STALE_PAIR[1]]["maps"].shape
    shapes = {c["maps"].shape[1:] for c in SPECKLE}
    assert {h for h, _ in shapes} == {5, 9, 10, 11, 18} and {w for _, w in shapes} == {64, 65, 130, 256, 257, 320, 1100}
    # thin-backed comb: no piece inside a band of two or four rows exceeds max_size, the whole does
    c = by["thincomb_18x130_x50_back1x30_max100"]
    whole = c["promises"]["component_size"]
    assert whole > c["max_size"]
    for G in (2, 4):
        for y0 in range(0, 18, G):
            band = c["maps"][0, y0:y0 + G]
            lab = pc.np_components(band, c["newval"], c["max_diff"])
            assert np.bincount(lab[band != c["newval"]]).max() <= c["max_size"]
    assert by["thincomb_18x130_x50_back1x30_exact"]["max_size"] == whole and by["thincomb_18x130_x50_back1x30_minus1"]["max_size"] == whole - 1
    # a comb's back is large inside its own band, and its teeth run through at least three further bands
    c = by["comb_18x130_x40_back4x60_max50"]
    assert 2 * 60 > c["max_size"] and (18 - 4) // 4 >= 3
    # islands sit across every boundary column the band walk knows, at every row offset mod 4 (18 rows)
    c = by["islands_18x1100_max9"]
    ids = c["ids"][0]
    for col in pc.seg_boundaries(1100):
        both = [y for y in range(18) if ids[y, col - 1] and ids[y, col - 1] == ids[y, col]]
        starts = {y for y in both if y - 1 not in both}
        assert {y % 4 for y in starts} == {0, 1, 2, 3}, col
    assert pc.seg_boundaries(1100) == [64, 256, 320, 576, 640, 960] and pc.seg_boundaries(320) == [64, 128, 192, 256]
    for corner in (ids[0, 0], ids[0, -1], ids[-1, 0], ids[-1, -1]):
        assert corner


@pytest.mark.parametrize("case", LR, ids=[c["name"] for c in LR])
def test_lr_case(oracle, case):
    mind, nd, d12 = case["mind"], case["nd"], case["d12"]
    assert pc.contract_ok(case["pre"], mind, nd, case["cost"], cost16=case["cost_hi"] <= 65534)
    slow = case["W"] > 1500    # the restatement is a Python loop: the widest rows get it on the designed rows' first case only
    for r in case["rows"]:
        d, c = r["d"][None], r["c"][None]
        want = oracle.validate_disparity(d, c, mind, nd, d12)
        if not slow or r["name"] in ("fans_tie_on_min", "range_edges"):
            assert np.array_equal(want, pc.np_validate(d, c, mind, nd, d12)), r["name"]
        if r["designed"]:
            assert np.array_equal(want[0], pc.lr_row_expected(r, mind)), r["name"]
    by = {r["name"]: r for r in case["rows"]}
    inv = (mind - 1) * 16
    standard = nd - 1 > d12 + 4
    for name in ("fans_unique_min", "fans_tie_on_min", "fans_all_equal", "fans_top_of_16_bits"):
        assert by[name]["gadgets"] >= 3
        valid = by[name]["d"] != inv
        if d12 < min(nd, 12) - 1:
            assert (valid & ~by[name]["keep"]).any() and by[name]["keep"].any()     # a fan wider than the tolerance loses pixels
    assert by["fans_top_of_16_bits"]["c"].max() == case["cost_hi"]
    if standard:
        assert by["subpixel_targets"]["gadgets"] >= 18 and by["tolerance_edges"]["gadgets"] >= 4   # every combination is there
        for name in ("subpixel_targets", "tolerance_edges"):
            valid = by[name]["d"] != inv
            assert (valid & ~by[name]["keep"]).any() and by[name]["keep"].any()
    r = by["range_edges"]
    minX1, maxX1 = max(mind + nd, 0), case["W"] + min(mind, 0)
    assert r["d"][minX1] != inv and r["d"][maxX1 - 1] != inv
    assert maxX1 - 1 - ((r["d"][maxX1 - 1] + 8) >> 4) == case["W"] - 1 - max(mind, 0)       # the highest column a claim reaches
    assert minX1 - ((r["d"][minX1] + 8) >> 4) == 1                                         # and the lowest
    if standard:
        assert r["d"][minX1 - 1] != inv and r["keep"][minX1 - 1]
        assert mind >= 0 or (r["d"][maxX1] != inv and r["keep"][maxX1])


def test_lr_widths_hit_every_instantiation():
    """The (NIT, PX) each width is listed with is what launch_lrcheck's arithmetic gives, and the list holds all eight."""
    for W, (nit, px) in pc.LR_FAST_WIDTHS:
        p = 2 if W <= 1280 else 4
        bsmax = 256 if p == 4 else (64 if W <= 640 else 128)
        groups = -(-W // p)
        assert (-(-groups // bsmax), p) == (nit, px), W
    assert {k for _, k in pc.LR_FAST_WIDTHS} == {(1, 2), (2, 2), (3, 2), (4, 2), (5, 2), (2, 4), (3, 4), (4, 4)}
    ws = [w for w, _ in pc.LR_FAST_WIDTHS]
    assert {w % 4 for w in ws} == {0, 1, 2, 3} and {640, 641, 1280, 1281, 4096} <= set(ws)
    assert {(c["mind"], c["d12"]) for c in LR} >= {(-8, 0), (0, 1), (5, 2), (0, 64)}


@pytest.mark.parametrize("mind", [-8, 0, 5])
def test_contract_is_what_find_correspondence_produces(oracle, mind):
    """The range sbm_debug_postfilter holds its input to is the one the correspondence stage produces: noise pairs (every disparity
    wins somewhere, both ends of the range among them) with the texture and uniqueness tests off."""
    rng = np.random.default_rng(40 + mind)
    nd, H, W = 16, 40, 160
    L, R = (rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(2))
    p = oracle.make_params(nd, 5, 31, mind, 0, 0, 0, 0, 1)
    st, s = oracle.compute(p, L, R, stages=True)
    assert st == 0 and pc.contract_ok(s["pre_lr"], mind, nd, s["cost"], cost16=True)
    valid = s["pre_lr"][s["pre_lr"] != (mind - 1) * 16]
    assert valid.min() == mind * 16 and valid.max() == (mind + nd - 1) * 16 and (valid % 16 != 0).any()
