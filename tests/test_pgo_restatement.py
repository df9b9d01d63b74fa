"""Holds the numpy restatement of the pose-graph optimiser (tests/pgo_cases.py) to what the reference's own code recorded in
tests/golden/pgo_reference.npz (tools/make_pgo_fixtures.py). lambda, chi2, the return value and the poses within 4 * E0, E0 the
largest relative difference measured on the file's first six cases when it was written (2.8e-13, in its metadata; Eigen
eliminates in another order and a second machine's libm and LAPACK may round differently); a later case, shaped as the
reference's mapper shapes its graphs, within 4 * max(E0, its own measured E); the discrete outcomes exactly: which links are
removed in which order, which vertices are reached, and which reading of the lower-triangle and of the max_diag question the reference's code shows."""
import pathlib

import numpy as np
import pytest

import pgo_cases as pc

ROOT = pathlib.Path(__file__).resolve().parents[1]
REC = np.load(ROOT / "tests" / "golden" / "pgo_reference.npz")
E0 = float(REC["meta/E0"])
NAMES = [str(n) for n in REC["meta/names"]]


def recorded(name):
    c = {k: REC[f"{name}/{k}"] for k in ("ids", "poses", "frm", "to", "meas", "info")}
    rec = {k: REC[f"{name}/{k}"] for k in ("lam", "chi", "out_ids", "out_poses", "removed", "edgechi", "err")}
    return c, rec, int(REC[f"{name}/num"]), bool(REC[f"{name}/robust"])


def test_tolerance_is_the_measured_one():
    assert 0 < E0 <= 1e-6 and set(NAMES) == set(pc.recorded_cases())


@pytest.mark.parametrize("name", NAMES)
def test_inputs_are_the_builders(name):
    c, _, num, robust = recorded(name)
    b, bnum, brobust = pc.recorded_cases()[name]
    assert (num, robust) == (bnum, brobust)
    for k in c:
        assert np.array_equal(c[k], b[k]), k


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_recording(name):
    c, rec, num, robust = recorded(name)
    got = pc.restated(c, num, robust)
    assert np.array_equal(got["out_ids"], rec["out_ids"])
    assert np.array_equal(got["removed"], rec["removed"])
    d = pc.difference(rec, got, robust)
    allowed = pc.tolerance(REC, name, 4)                     # 4 E0; a case later than the first six, 4 max(E0, its own E)
    print(name, "difference", d, "allowed", allowed)
    assert d <= allowed


def recorded_rounds(name):
    """The recording's "roundchi": one (from, to, chi2) per robust round, as the reference's own code printed them."""
    off = REC[f"{name}/round_off"]
    return [tuple(REC[f"{name}/round_{k}"][off[r]:off[r + 1]] for k in ("from", "to", "chi")) for r in range(len(off) - 1)]


@pytest.mark.parametrize("name", pc.ROBUST_CASES)
def test_robust_cases_decide_by_a_factor_of_two(name):
    """The chi2 values that decide a round sit a factor of 2 from the threshold and from each other: in every removing round the
    winner is at least 2 THR and twice the runner-up among the links the id rule lets the loop remove, in the stopping round
    every such link is at most THR / 2. Conditions on the inputs, met by the choice of seed and outlier sizes; they hold on the
    restatement's numbers and on the ones the reference's own code recorded."""
    c, rec, num, robust = recorded(name)
    assert robust
    rounds = []
    _, _, _, removed = pc.run_optimize_robust(*pc.args(c), num, rounds=rounds)
    theirs = recorded_rounds(name)
    assert len(rounds) == len(theirs) == len(removed) + 1 == len(rec["removed"]) + 1
    for mine, ref in zip(rounds, theirs):                     # the same links in the same order, round by round
        assert np.array_equal(mine[0], ref[0]) and np.array_equal(mine[1], ref[1])
    for who, r in (("restatement", rounds), ("recording", theirs)):
        m = pc.round_margins(r)
        print(name, who, [(round(w, 2), round(u, 2)) for w, u in m])
        for w, u in m[:-1]:
            assert w >= 2 * pc.THR and w >= 2 * u, (who, w, u)  # the winner, from the threshold and from the runner-up
        assert m[-1][0] <= pc.THR / 2, (who, m[-1])            # the round that stops
        assert pc.decided_by_a_factor_of_two(r)


def test_robust60_removes_its_one_outlier():
    assert REC["robust60/removed"].tolist() == REC["robust60_bidir/removed"].tolist() == [[27, 41]]


@pytest.mark.parametrize("name", [n for n in pc.ROBUST_CASES if n.startswith("multi48")])
def test_multi_outlier_cases_remove_at_least_three(name):
    """... and the bidirectional forms remove a link the builder listed as good: getConnectedGraph keeps one link per vertex
    pair in the direction its walk met first, about half of them from the larger id to the smaller, and under the reference's
    lower-triangle reading those couple nothing, so five iterations leave a good closure with a chi2 far above the threshold.
    In the gapped bidirectional form an odometry link whose ids a gap separates goes first: the id rule takes it for a closure."""
    removed = [tuple(r) for r in REC[f"{name}/removed"].tolist()]
    assert len(removed) >= 3
    f = pc.gapped if "gaps" in name else (lambda v: v)
    label = lambda pairs: {(f(a), f(b)) for a, b in pairs} | {(f(b), f(a)) for a, b in pairs}  # noqa: E731
    bad, good = label(pc.MULTI_BAD), label(pc.MULTI_GOOD)
    assert len(set(removed) & bad) == 3                        # every outlier goes, in either direction
    if name == "multi48_bidir":
        assert set(removed) & good                             # a good closure
    elif name == "multi48_bidir_gaps":
        assert set(removed) - bad                              # a good odometry link, below
    else:
        assert set(removed) <= bad
    if name == "multi48_bidir_gaps":
        a, b = removed[0]
        assert (a, b) not in bad | good and abs(a - b) == 3 and f(10) == a and f(9) == b     # the odometry link 10 -> 9, relabelled


def test_identity_case_keeps_iterating():
    """The recorded case that takes oplus' identity branch in its first update: the reference's chi2 goes on changing after it
    (a recording frozen after the branch would show one value from then on), and so does the restatement's, whose every
    iteration applies its update."""
    c, rec, num, _ = recorded("identity16")
    assert num == pc.IDENTITY_NUM >= 5 and len(rec["chi"]) == num
    tr = {}
    pc.run_optimize(*pc.args(c), num, trace=tr)
    first = tr["ident_its"].index(True)
    assert first == 0
    steps = np.abs(np.diff(rec["chi"][first + 1:])) / rec["chi"][first + 1:-1]
    print("identity16 chi", rec["chi"].tolist(), "relative steps after the branch", steps.tolist())
    assert len(steps) >= 3 and (steps > 0.05).all()


def test_the_readings_the_recording_shows():
    """Lower triangle: on the ring closed new -> old the reference's numbers are the REFERENCE reading's, far from SYMMETRIC's.
    max_diag: lambda0 is tau times the LAST edge's largest diagonal entry, not the matrix's."""
    c, rec, num, _ = recorded("ring8_new_old")
    sym = pc.restated(c, num, False, coupling=pc.SYMMETRIC)
    assert abs(sym["err"] - rec["err"]) > 0.5 * rec["err"]
    c, rec, num, _ = recorded("iter40")
    g = pc.Graph(*pc.args(c))
    A, _, last = g.build(g.linearise())
    assert abs(rec["lam"][0] - pc.TAU * last) <= 4 * E0 * rec["lam"][0]
    assert abs(rec["lam"][0] - pc.TAU * np.abs(np.diag(A)).max()) > 1e-3 * rec["lam"][0]    # not the matrix's largest entry


def test_unreachable_vertex_drops_out():
    c, rec, _, _ = recorded("unreachable")
    assert 9 in c["ids"] and 9 not in rec["out_ids"]
