"""Holds the numpy restatement of the pose-graph optimiser (tests/pgo_cases.py) to what the reference's own code recorded in
tests/golden/pgo_reference.npz (tools/make_pgo_fixtures.py). lambda, chi2, the return value and the poses within 4 * E0, E0 the
largest relative difference measured when the file was written (2.8e-13, in its metadata; Eigen eliminates in another order and a
second machine's libm and LAPACK may round differently); the discrete outcomes exactly: which links are removed in which order,
which vertices are reached, and which reading of the lower-triangle and of the max_diag question the reference's code shows."""
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
    print(name, "difference", d, "allowed", 4 * E0)
    assert d <= 4 * E0


def test_robust_cases_decide_by_a_factor_of_two():
    """The chi2 values that decide a round sit a factor of 2 from the threshold and from each other (restatement alone)."""
    c = pc.robust_case()
    alive = np.arange(len(c["frm"]))
    rounds = []
    while True:
        oid, op, kept = pc.connected_graph(1, c["ids"], c["poses"], c["frm"][alive], c["to"][alive], c["meas"][alive])
        sel = alive[kept]
        g = pc.Graph(oid, op, c["frm"][sel], c["to"][sel], c["meas"][sel], c["info"][sel])
        pc.optimize(g, 5)
        chi = g.errors()[1][np.abs(g.frm - g.to) != 1]
        rounds.append(np.sort(chi)[::-1])
        if chi.max() < pc.THR:
            break
        k = int(np.argmax(g.errors()[1] * (np.abs(g.frm - g.to) != 1)))
        alive = np.array([j for j in sel if (c["frm"][j], c["to"][j]) != (g.frm[k], g.to[k])])
    assert len(rounds) == 2
    assert rounds[0][0] >= 2 * pc.THR and rounds[0][0] >= 2 * rounds[0][1]     # the winner, from the threshold and the runner-up
    assert rounds[1][0] <= pc.THR / 2                                          # the round that stops


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
