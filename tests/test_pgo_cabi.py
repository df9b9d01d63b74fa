"""The pose-graph optimiser's C-ABI without a GPU: structure layout and defaults, every refusal of sbm_pgo_params_check with its
code, and the invariants of sbm_pgo_plan on the shapes of tests/pgo_cases.py under both coupling readings."""
import ctypes
import pathlib

import numpy as np
import pytest

import pgo_cases as pc
from gpu_support import build_callsite

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_struct_layout_and_defaults(pkg):
    p = pkg.PgoParams()
    pkg.load_library().sbm_pgo_params_default(p)
    assert (p.num, p.fixed_id, p.coupling, p.run_max) == (20, 1, pkg.PGO_COUPLING_REFERENCE, 64)
    assert bytes(p) == bytes(pkg.pgo_params()) and ctypes.sizeof(p) == 16
    assert ctypes.sizeof(pkg.PgoPlanInfo) == 32
    assert (pkg.PGO_COUPLING_REFERENCE, pkg.PGO_COUPLING_SYMMETRIC, pkg.PGO_EDGE_RECORD) == (pc.REFERENCE, pc.SYMMETRIC, 200)
    pkg.load_library().sbm_pgo_params_default(None)   # tolerated


def bad(c, **kw):
    c = {k: np.array(v) for k, v in c.items()}
    for k, (idx, val) in kw.items():
        c[k][idx] = val
    return c


BASE = pc.chain_graph(5, [(4, 2)], seed=2)
REFUSALS = [
    ("ok", {}, BASE, 0),
    ("num_negative", {"num": -1}, BASE, -2),
    ("pose_nan", {}, bad(BASE, poses=((2, 1, 3), np.nan)), -23),
    ("pose_inf", {}, bad(BASE, poses=((0, 0, 0), np.inf)), -23),
    ("meas_nan", {}, bad(BASE, meas=((1, 2, 2), np.nan)), -23),
    ("info_inf", {}, bad(BASE, info=((3, 5, 5), -np.inf)), -23),
    ("edge_absent_from", {}, bad(BASE, frm=(0, 77)), -2),
    ("edge_absent_to", {}, bad(BASE, to=(2, 0)), -2),
    ("fixed_absent", {"fixed_id": 9}, BASE, -2),
    ("self_edge", {}, bad(BASE, to=(1, int(BASE["frm"][1]))), -23),
    ("duplicate_id", {}, bad(BASE, ids=(4, 4)), -2),
    ("coupling_unknown", {"coupling": 2}, BASE, -23),
    ("run_max_zero", {"run_max": 0}, BASE, -23),
]


@pytest.mark.parametrize("name,change,c,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_check_status_codes(pkg, name, change, c, code):
    assert pkg.pgo_check(pkg.pgo_params(**change), *pc.args(c)) == code


def test_empty_graph_and_nulls(pkg):
    L = pkg.load_library()
    p = pkg.pgo_params()
    empty = pkg.PgoGraph()
    assert L.sbm_pgo_params_check(ctypes.byref(p), ctypes.byref(empty)) == -2          # an empty graph
    assert L.sbm_pgo_params_check(None, ctypes.byref(empty)) == -1 and L.sbm_pgo_params_check(ctypes.byref(p), None) == -1
    assert L.sbm_pgo_plan(ctypes.byref(p), ctypes.byref(empty), None, None, None, None) == -1
    err = ctypes.c_double()
    assert L.sbm_pgo_optimize(None, ctypes.byref(p), ctypes.byref(empty), None, ctypes.byref(err)) == -1
    assert L.sbm_pgo_debug_fetch(None, 0, None, 0) == -1 and L.sbm_pgo_last_plan(None, None, None, None) == -1


def test_only_the_fixed_vertex_is_ok(pkg):
    info, vrun, rc, cp = pkg.pgo_plan(pkg.pgo_params(), [1], pc.pose()[None], [], [], np.zeros((0, 3, 4)), np.zeros((0, 6, 6)))
    assert (info.n_free, info.n_runs, info.n_junctions) == (0, 0, 0)


SHAPES = pc.shape_cases()
SHAPES["iter40"], SHAPES["robust60"] = pc.iteration_case(), pc.robust_case()


@pytest.mark.parametrize("coupling", [pc.REFERENCE, pc.SYMMETRIC], ids=["reference", "symmetric"])
@pytest.mark.parametrize("run_max", [1, 4, 64])
@pytest.mark.parametrize("name", list(SHAPES))
def test_plan_invariants(pkg, name, run_max, coupling):
    c = SHAPES[name]
    info, vrun, rc, couples = pkg.pgo_plan(pkg.pgo_params(coupling=coupling, run_max=run_max, fixed_id=pc.fixed(c)), *pc.args(c))
    g = pc.Graph(*pc.args(c), fixed_id=pc.fixed(c), coupling=coupling)
    assert info.n_free == g.nfree == len(vrun) and info.schur_size == 6 * info.n_junctions
    assert np.array_equal(couples, g.couples()) and info.n_coupling == couples.sum()
    # every free vertex lies in exactly one run or is a junction; runs are stretches of consecutive indices, numbered in order
    assert ((vrun >= -1) & (vrun < info.n_runs)).all() and (vrun == -1).sum() == info.n_junctions
    runs = vrun[vrun >= 0]
    assert np.array_equal(np.unique(runs), np.arange(info.n_runs)) and (np.diff(runs) >= 0).all()
    for r in range(info.n_runs):
        idx = np.flatnonzero(vrun == r)
        assert (np.diff(idx) == 1).all() and len(idx) <= run_max            # no run is longer than run_max
    if info.n_runs:
        assert info.longest_run == np.bincount(runs).max()
    # every coupling edge joins run neighbours or ends on junctions; the slots are the distinct coupled pairs
    hi, hj = g.hidx[g.vi][couples], g.hidx[g.vj][couples]
    pairs = {(max(a, b), min(a, b)) for a, b in zip(hi.tolist(), hj.tolist())}
    assert pairs == {tuple(p) for p in rc.tolist()} and len(rc) == info.n_slots
    for r, c_ in rc.tolist():
        assert r > c_
        assert r - c_ == 1 or (vrun[r] == -1 and vrun[c_] == -1)


def plan_of(pkg, name, coupling, run_max=64):
    c = SHAPES[name]
    return c, pkg.pgo_plan(pkg.pgo_params(coupling=coupling, run_max=run_max, fixed_id=pc.fixed(c)), *pc.args(c))


@pytest.mark.parametrize("name", ["reversed_chain", "reversed_chain_all"])
def test_reversed_chain_couples_nothing_under_the_reference_reading(pkg, name):
    """Every link runs to the smaller Hessian index (or touches the fixed vertex): the lower triangle holds no block, the
    system is block diagonal, no slot, no junction. The symmetric reading has the chain's n - 2 sub-diagonal slots."""
    c, (info, vrun, rc, couples) = plan_of(pkg, name, pc.REFERENCE)
    n = len(c["ids"])
    assert (info.n_free, info.n_slots, info.n_junctions, info.n_coupling) == (n - 1, 0, 0, 0) and not couples.any() and len(rc) == 0
    c, (info, vrun, rc, couples) = plan_of(pkg, name, pc.SYMMETRIC)
    assert info.n_slots == n - 2 == info.n_coupling and info.n_junctions == 0
    assert rc.tolist() == [[k + 1, k] for k in range(n - 2)]


def test_opposite_pair_feeds_one_slot_from_two_edges(pkg):
    """Closures (2, 5) and (5, 2): under the symmetric reading both couple Hessian indices 0 and 3, one as m^T and one as m, and
    the plan has ONE slot for the pair; under the reference reading only (2, 5) couples."""
    c, (info, vrun, rc, couples) = plan_of(pkg, "opposite_pair", pc.SYMMETRIC)
    g = pc.Graph(*pc.args(c), coupling=pc.SYMMETRIC)
    both = np.flatnonzero(((c["frm"] == 2) & (c["to"] == 5)) | ((c["frm"] == 5) & (c["to"] == 2)))
    assert len(both) == 2 and couples[both].all()
    assert sorted(g.hidx[g.vi][both].tolist()) == [0, 3] and rc.tolist().count([3, 0]) == 1      # ids 2 and 5, vertex 1 fixed
    assert info.n_slots == (len(c["ids"]) - 2) + 1 and info.n_coupling == info.n_slots + 1      # two edges, one slot
    c, (info, vrun, rc, couples) = plan_of(pkg, "opposite_pair", pc.REFERENCE)
    assert couples[both].tolist() == [True, False] and c["frm"][both[0]] == 2 and rc.tolist().count([3, 0]) == 1


@pytest.mark.parametrize("coupling", [pc.REFERENCE, pc.SYMMETRIC], ids=["reference", "symmetric"])
@pytest.mark.parametrize("name", ["fixed_mid", "fixed_last"])
def test_fixed_vertex_elsewhere_splits_the_chain(pkg, name, coupling):
    """The fixed vertex has no Hessian index: the odometry links on either side of it couple nothing, so the Hessian
    neighbours across it (fixed_mid) share no sub-diagonal slot, although their indices differ by 1."""
    c, (info, vrun, rc, couples) = plan_of(pkg, name, coupling)
    g = pc.Graph(*pc.args(c), fixed_id=pc.fixed(c), coupling=coupling)
    fixed_pos = int(np.flatnonzero(g.ids == pc.fixed(c))[0])
    assert g.hidx[fixed_pos] == -1 and info.n_free == len(c["ids"]) - 1
    touching = (c["frm"] == pc.fixed(c)) | (c["to"] == pc.fixed(c))
    assert touching.sum() >= 1 and not couples[touching].any()
    if name == "fixed_mid":
        below = int(g.hidx[fixed_pos - 1])
        assert g.hidx[fixed_pos + 1] == below + 1 and [below + 1, below] not in rc.tolist()
        assert any(r > below >= c_ for r, c_ in rc.tolist())             # the closures do span it


def test_junction_cap_is_reported(pkg):
    """More than 1024 junctions: SBM_ERR_UNSUPPORTED from the plan, without a device."""
    n = 2200
    c = pc.chain_graph(n, [], seed=1)
    with pytest.raises(pkg.StereoBMError) as e:
        pkg.pgo_plan(pkg.pgo_params(run_max=1), *pc.args(c))
    assert e.value.code == -23


def test_cpp_adaptor_compiles_against_stand_in_map_types(tmp_path):
    """include/sbm_pgo.hpp with the host compiler against stand-ins for the caller's Transform and Link (tests/cpp/
    pgo_callsite_main.cpp): main.cpp:328 with a one-line swap. Compile and link only."""
    _, r = build_callsite(tmp_path, "pgo_callsite_main.cpp", flags=("-Wall", "-Werror"))
    assert r.returncode == 0, r.stderr


def test_header_states_the_readings():
    text = (ROOT / "include" / "sbm.h").read_text()
    for phrase in ('"pgo_linearise"', '"pgo_solve"', "SBM_PGO_COUPLING_SYMMETRIC", "LAST edge", "lower triangle", "no step rejection",
                   "negative triplet", "1024 junctions", "sbm_pgo_optimize_device", "Not guarded"):
        assert phrase in text, phrase
