"""The pose-graph optimiser on the device against the numpy restatement of tests/pgo_cases.py (itself held to the reference's
recording by tests/test_pgo_restatement.py).

Edge kernel: with contraction off the device and the restatement perform the same operations in the same order. Error, chi2,
the translation rows of both Jacobians and everything else without sqrt or pow upstream must be EQUAL. The rotation blocks of the
Jacobians are sums dq M with dq linear in 1 / qw and 1 / pow(qw, 3), qw from a sqrt: 2 ulp in sqrt and 2 ulp in pow move every dq
entry by at most (3 * 2 + 2) eps relative, so |dJ| <= 8 eps |dq| |M| entry by entry -- on the scale of the terms, not of the sum,
which near 180 degrees cancels by three orders of magnitude. Blocks and vectors built from J carry that bound through
|dJ|^T |O| |J| + |J|^T |O| |dJ| (+ the second-order term); where the carried bound is 0 equality is demanded. Largest difference seen: 8.5e-14 in Ji of the 179 degree edge
about (1, 0.2, -0.1) (Ji's largest entry 1.1, terms of 1.6e3: one ulp of pow), 0.11 of its bound; seven of nine edges are equal
in every entry.
Solve: backward error eta = |b - (A + lambda I) x| / (|A + lambda I| |x| + |b|) on the exported system, at most 16 x the eta of
numpy.linalg.solve on the same system (a direct fp64 solve is backward stable; the factor covers the other elimination order).
The engine takes one step of iterative refinement with the residual in twice the working precision; without it the two-vertex
graph sat at 16.3 times numpy's eta (8.09e-17 against 4.96e-18), with it at 2.6 times.
Iterations: lambda, chi2 and poses against the restatement within TOL = 4 * E0 * 4: the CPU test's tolerance (what two CPU
eliminations of the same systems differ by) widened by the engine-to-restatement difference measured on the solve test, where
the engine's eta is between 0.19 and 3.6 times numpy's (all below 3.9e-17); 4 is that 3.6 rounded up, the only headroom. The
iterates differ from the restatement by 5e-13 relative at most (chi2 after one symmetric iteration), TOL is 4.4e-12. Recorded in
DESIGN.md section 17. The identity
branch case of test_quirk_identity_branch_of_oplus sits next to the singularity of dq/dR on purpose and is compared to 1e-6.
Cases recorded after the first six (graphs shaped as the reference's mapper shapes them: links in both directions, ids with
gaps, several outliers, the identity branch early in a longer run) carry their own measured restatement-to-recording difference
E; they are held to 16 * max(E0, E), the same two factors of 4 on the same grounds (pgo_cases.tolerance). The discrete outcomes
of the robust loop, the removed links in order and the reached ids, are the recording's exactly. A fixed vertex that is not the
smallest id (fixed_mid, fixed_last) and a free `from` with a fixed `to` (reversed_chain_all, bidir_chain_all) the reference
cannot run, so those shapes are held to the restatement alone."""
import ctypes
import math
import pathlib

import numpy as np
import pytest

import pgo_cases as pc
from gpu_support import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]
REC = np.load(ROOT / "tests" / "golden" / "pgo_reference.npz")
E0 = float(REC["meta/E0"])
TOL = 4 * E0 * 4
RUN_MAX = 4


@pytest.fixture(scope="module")
def engine(pkg):
    bm = pkg.StereoBM.create(16, 9)
    yield bm
    bm.close()


def dense(dbg, rc, nfree, lam):
    """The exported system as SimplicialLDLT reads it: the lower triangle mirrored, plus lambda I."""
    A = np.zeros((6 * nfree, 6 * nfree))
    for h in range(nfree):
        A[6 * h:6 * h + 6, 6 * h:6 * h + 6] = dbg["D"][h]
    for s, (r, c) in enumerate(rc.tolist()):
        A[6 * r:6 * r + 6, 6 * c:6 * c + 6] = dbg["E"][s]
    A = np.tril(A)
    return A + np.tril(A, -1).T + lam * np.eye(6 * nfree)


def eta(S, x, b):
    return np.linalg.norm(b - S @ x) / (np.linalg.norm(S, 2) * np.linalg.norm(x) + np.linalg.norm(b))


def test_edge_kernel_against_the_restatement(pkg, engine):
    c = pc.edge_cases()
    g = pkg.PoseGraph(engine, num=1, coupling=pc.SYMMETRIC)
    g.optimize(*pc.args(c))
    dbg = g.debug(len(c["frm"]))
    G = pc.Graph(*pc.args(c), coupling=pc.SYMMETRIC)
    lin = G.linearise()
    Rz, tz = pc.split(G.meas)
    R, t = pc.split(G.poses)
    _, _, Bi, Bj = pc.edge_jacobians(Rz, tz, R[G.vi], t[G.vi], R[G.vj], t[G.vj], with_bound=True)
    eps = np.finfo(float).eps
    O = np.abs(G.info)
    dJ = {"Ji": 8 * eps * Bi, "Jj": 8 * eps * Bj}
    aJ = {"Ji": np.abs(lin["Ji"]), "Jj": np.abs(lin["Jj"])}
    awe = np.abs(pc.mat6_vec(G.info, lin["e"]))
    T = lambda M: np.swapaxes(M, 1, 2)  # noqa: E731

    def carried(a, b):   # bound of Ja^T O Jb
        P = T(dJ[a]) @ O @ aJ[b] + T(aJ[a]) @ O @ dJ[b] + T(dJ[a]) @ O @ dJ[b]
        return P

    def carried_b(a):
        return np.einsum("eri,er->ei", dJ[a], awe)

    tol = {"e": 0.0, "chi": 0.0, "Ji": dJ["Ji"], "Jj": dJ["Jj"], "mii": carried("Ji", "Ji"), "mjj": carried("Jj", "Jj"),
           "mij": carried("Ji", "Jj"), "bi": carried_b("Ji"), "bj": carried_b("Jj")}
    for k, allowed in tol.items():
        diff = np.abs(dbg[k] - lin[k])
        allowed = np.broadcast_to(allowed, diff.shape)
        nz = allowed > 0
        print(k, "largest difference", float(diff.max()), "largest share of its bound", float((diff[nz] / allowed[nz]).max()) if nz.any() else 0.0,
              "entries that must be equal", int((~nz).sum()))
        assert np.array_equal(dbg[k][~nz], lin[k][~nz]), k
        assert (diff <= allowed).all(), k


SHAPES = pc.shape_cases(RUN_MAX)


def solve_and_first_step(pkg, engine, name, c, coupling, run_max):
    fixed = pc.fixed(c)
    g = pkg.PoseGraph(engine, num=1, coupling=coupling, run_max=run_max, fixed_id=fixed)
    err, ids, poses = g.optimize(*pc.args(c))
    info, lam, its = g.last_plan()
    want_info, _, rc, _ = pkg.pgo_plan(g.params, *pc.args(c))
    assert bytes(info) == bytes(want_info) and its == 1                      # the plan agrees with what the call launched
    dbg = g.debug(len(c["frm"]))
    # ... and with what it exported: one diagonal block, b and x per free vertex, one lower block per coupled pair
    assert (len(dbg["D"]), len(dbg["b"]), len(dbg["x"]), len(dbg["E"])) == (want_info.n_free,) * 3 + (want_info.n_slots,)
    tr = {}
    werr, wids, wposes = pc.run_optimize(*pc.args(c), 1, fixed_id=fixed, coupling=coupling, trace=tr)
    S = dense(dbg, rc, info.n_free, lam)
    b, x = dbg["b"].reshape(-1), dbg["x"].reshape(-1)
    Sw = tr["A"] + np.tril(tr["A"], -1).T + tr["lam"][0] * np.eye(len(b))
    assert np.abs(S - Sw).max() <= 1e-12 * np.abs(Sw).max() and np.abs(b - tr["b"]).max() <= 1e-12 * max(np.abs(tr["b"]).max(), 1e-300)
    e_dev, e_np = eta(S, x, b), eta(S, np.linalg.solve(S, b), b)
    print(name, coupling, "run_max", run_max, "fixed", fixed, "junctions", info.n_junctions, "runs", info.n_runs, "slots", info.n_slots,
          "eta device", e_dev, "eta numpy", e_np, "first step share of TOL", np.abs(poses - wposes).max() / np.abs(wposes).max() / TOL)
    assert e_dev <= 16 * e_np
    assert abs(lam - tr["lam"][0]) <= TOL * tr["lam"][0]
    assert np.array_equal(ids, wids) and np.abs(poses - wposes).max() <= TOL * np.abs(wposes).max()
    return info


@pytest.mark.parametrize("coupling", [pc.REFERENCE, pc.SYMMETRIC], ids=["reference", "symmetric"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_solve_backward_error_and_first_step(pkg, engine, name, coupling):
    info = solve_and_first_step(pkg, engine, name, SHAPES[name], coupling, RUN_MAX)
    if name.startswith("reversed_chain") and coupling == pc.REFERENCE:        # a block-diagonal system: nothing couples
        assert (info.n_slots, info.n_coupling) == (0, 0)


@pytest.mark.parametrize("coupling", [pc.REFERENCE, pc.SYMMETRIC], ids=["reference", "symmetric"])
@pytest.mark.parametrize("run_max", [1, 2, 64])
@pytest.mark.parametrize("name", ["star5", "bidir_chain", "fixed_mid", "reversed_chain"])
def test_solve_at_other_run_lengths(pkg, engine, name, run_max, coupling):
    """run_max 1: every vertex a junction, the dense path alone; 2: runs of one or two between promoted junctions; 64: one run
    per stretch (reversed_chain under the reference reading then has no junction and no slot at all)."""
    info = solve_and_first_step(pkg, engine, name, pc.shape_cases(run_max)[name], coupling, run_max)
    assert info.longest_run <= run_max
    if name == "reversed_chain" and coupling == pc.REFERENCE and run_max == 64:
        assert (info.n_slots, info.n_junctions) == (0, 0)


@pytest.mark.parametrize("num", [1, 5])
def test_iterations_on_a_chain_with_closures(pkg, engine, num):
    c = pc.iteration_case()
    for coupling in (pc.REFERENCE, pc.SYMMETRIC):
        g = pkg.PoseGraph(engine, num=num, coupling=coupling, run_max=RUN_MAX)
        err, ids, poses = g.optimize(*pc.args(c))
        tr = {}
        werr, wids, wposes = pc.run_optimize(*pc.args(c), num, coupling=coupling, trace=tr)
        _, lam, its = g.last_plan()
        print(num, coupling, "err", err, werr, "lambda", lam, tr["lam"][-1], "pose diff", np.abs(poses - wposes).max())
        assert its == num and abs(lam - tr["lam"][-1]) <= TOL * tr["lam"][-1]
        assert abs(err - werr) <= TOL * werr and np.abs(poses - wposes).max() <= TOL * np.abs(wposes).max()
    if num == 5:   # and the recording itself, REFERENCE reading
        g = pkg.PoseGraph(engine, num=5, run_max=RUN_MAX)
        err, _, poses = g.optimize(*pc.args(c))
        assert abs(err - float(REC["iter40/err"])) <= TOL * err and np.abs(poses - REC["iter40/out_poses"]).max() <= TOL * np.abs(poses).max()


def test_quirk_identity_branch_of_oplus(pkg, engine):
    """An update with |v| > 1 takes the identity rotation; the translation still applies."""
    c = pc.chain_graph(3, seed=51, info=np.eye(6))
    c["poses"][2] = pc.mul(c["poses"][2], pc.pose(pc.rot([0, 0, 1], 179.9), [0.5, 0, 0]))   # dq/dR blows up near 180 degrees
    tr = {}
    werr, _, wposes = pc.run_optimize(*pc.args(c), 1, trace=tr)
    assert tr["identity"]
    g = pkg.PoseGraph(engine, num=1)
    err, _, poses = g.optimize(*pc.args(c))
    x = g.debug(len(c["frm"]))["x"]
    assert (np.sum(x[:, 3:] ** 2, axis=1) > 1).any()
    assert np.abs(poses - wposes).max() <= 1e-6 * np.abs(wposes).max()


def test_identity_branch_early_then_more_iterations(pkg, engine):
    """identity16: the first update takes oplus' identity branch at some vertex and five more iterations follow. Run with num =
    0 .. 6 the device returns, as err, the chi2 the next iteration would start from: every entry of the recording's chi, then its
    err; lambda and the poses after every iteration against the restatement."""
    c = pc.identity_case()
    num = pc.IDENTITY_NUM
    tol = pc.tolerance(REC, "identity16", 16)
    rchi, worst = REC["identity16/chi"], 0.0
    full = {}
    pc.run_optimize(*pc.args(c), num, trace=full)
    first = full["ident_its"].index(True)
    assert first == 0 and num - first >= 5
    before = None
    for k in range(num + 1):
        g = pkg.PoseGraph(engine, num=k, run_max=RUN_MAX)
        err, ids, poses = g.optimize(*pc.args(c))
        tr = {}
        werr, wids, wposes = pc.run_optimize(*pc.args(c), k, trace=tr)
        want = float(rchi[k]) if k < num else float(REC["identity16/err"])
        d = max(abs(err - werr) / werr, abs(err - want) / want, np.abs(poses - wposes).max() / np.abs(wposes).max())
        _, lam, its = g.last_plan()
        assert its == k
        if k:
            d = max(d, abs(lam - tr["lam"][-1]) / tr["lam"][-1], abs(lam - float(REC["identity16/lam"][k - 1])) / lam)
        if k == first + 1:                                  # the branch iteration: some rotation update has |v| > 1
            x = g.debug(len(c["frm"]))["x"]
            assert (np.sum(x[:, 3:] ** 2, axis=1) > 1).any()
        if k > first + 1:                                   # ... and the poses keep moving afterwards
            assert np.abs(poses - before).max() > 1e-3 * np.abs(poses).max()
        before = poses
        worst = max(worst, d)
        print("identity16 after", k, "iterations: err", err, "restatement", werr, "recording", want, "difference", d)
        assert np.array_equal(ids, wids) and d <= tol
    assert np.abs(before - REC["identity16/out_poses"]).max() <= tol * np.abs(before).max()
    print("identity16 largest difference", worst, "share of its tolerance", worst / tol)


@pytest.mark.parametrize("name", ["reversed_chain", "bidir_chain", "opposite_pair"])
def test_recorded_mapper_shapes(pkg, engine, name):
    """Three iterations on the recorded plain shapes against the recording (REFERENCE) and the restatement (both readings).
    Under the symmetric reading the two chains converge: after three iterations chi2 is 1e-15 and less, a sum of squares of
    residuals of 1e-8 that are themselves differences of pose entries of order 1, so its rounding error is relative to the
    residuals' scale, not to itself; there the chi2 difference is taken against the chi2 the run started from."""
    c, num, tol = SHAPES[name], int(REC[f"{name}/num"]), pc.tolerance(REC, name, 16)
    worst = 0.0
    for coupling in (pc.REFERENCE, pc.SYMMETRIC):
        err, ids, poses = pkg.PoseGraph(engine, num=num, coupling=coupling, run_max=RUN_MAX).optimize(*pc.args(c))
        tr = {}
        werr, wids, wposes = pc.run_optimize(*pc.args(c), num, coupling=coupling, trace=tr)
        scale = werr if coupling == pc.REFERENCE else tr["chi"][0]
        d = max(abs(err - werr) / scale, np.abs(poses - wposes).max() / np.abs(wposes).max())
        if coupling == pc.REFERENCE:
            rerr, rposes = float(REC[f"{name}/err"]), REC[f"{name}/out_poses"]
            d = max(d, abs(err - rerr) / rerr, np.abs(poses - rposes).max() / np.abs(rposes).max())
        worst = max(worst, d)
        assert np.array_equal(ids, wids) and d <= tol, (coupling, d, tol)
    print(name, "largest difference", worst, "share of its tolerance", worst / tol)


@pytest.mark.parametrize("name", ["iter40", "identity16", "multi48_bidir_gaps"])
def test_no_iteration_returns_the_input(pkg, engine, name):
    """num = 0: the poses come back as they went in (ascending id), err is the chi2 at those poses, no iteration is reported.
    Every edge's chi2 equals the restatement's bit for bit (the edge test demands that), so err differs from their exact sum by
    the rounding of one summation of ne non-negative terms, whatever its order: at most ne eps times the sum."""
    c = {k: REC[f"{name}/{k}"] for k in ("ids", "poses", "frm", "to", "meas", "info")}
    g = pkg.PoseGraph(engine, num=0, run_max=RUN_MAX)
    err, ids, poses = g.optimize(*pc.args(c))
    G = pc.Graph(*pc.args(c))
    want = math.fsum(G.errors()[1].tolist())
    _, lam, its = g.last_plan()
    print(name, "err", err, "restatement", want, "difference / bound", abs(err - want) / (len(c["frm"]) * np.finfo(float).eps * want))
    assert its == 0 and np.array_equal(ids, G.ids) and np.array_equal(poses, G.poses)
    assert abs(err - want) <= len(c["frm"]) * np.finfo(float).eps * want


def test_quirk_max_diag_is_the_last_edges(pkg, engine):
    c = pc.iteration_case()
    g = pkg.PoseGraph(engine, num=1, run_max=RUN_MAX)
    lams = []
    for order in (np.arange(len(c["frm"])), np.arange(len(c["frm"]))[::-1]):
        d = dict(c, frm=c["frm"][order], to=c["to"][order], meas=c["meas"][order], info=c["info"][order])
        g.optimize(*pc.args(d))
        tr = {}
        pc.run_optimize(*pc.args(d), 1, trace=tr)
        lams.append(g.last_plan()[1])
        assert abs(lams[-1] - tr["lam"][0]) <= TOL * tr["lam"][0]
    assert abs(lams[0] - lams[1]) > 1e-3 * lams[0]


def c_graph(pkg, c):
    """(sbm_pgo_graph over c's arrays, the arrays to keep alive)."""
    keep = [np.ascontiguousarray(c["ids"], np.int32), np.ascontiguousarray(np.asarray(c["poses"], np.float64).reshape(-1, 12)),
            np.ascontiguousarray(c["frm"], np.int32), np.ascontiguousarray(c["to"], np.int32),
            np.ascontiguousarray(np.asarray(c["meas"], np.float64).reshape(-1, 12)),
            np.ascontiguousarray(np.asarray(c["info"], np.float64).reshape(-1, 36))]
    ids, poses, frm, to, meas, info = (a.ctypes.data for a in keep)
    return pkg.PgoGraph(len(keep[0]), ids, poses, len(keep[2]), frm, to, meas, info), keep


@pytest.mark.parametrize("name", pc.ROBUST_CASES)
def test_robust_loop_equals_the_recording(pkg, engine, torch_cuda, name):
    """Removed links, in order, and reached ids exactly the recording's; err and poses within the case's tolerance. The
    bidirectional cases are what the reference's mapper hands over: getConnectedGraph keeps one link per pair, about half of
    them towards the smaller id, which couple nothing under the reference's reading, so good links go too."""
    c = {k: REC[f"{name}/{k}"] for k in ("ids", "poses", "frm", "to", "meas", "info")}
    tol = pc.tolerance(REC, name, 16)
    want_removed = [tuple(r) for r in REC[f"{name}/removed"].tolist()]
    g = pkg.PoseGraph(engine, num=int(REC[f"{name}/num"]), run_max=RUN_MAX)
    err, ids, poses, removed = g.optimize_robust(*pc.args(c))
    assert removed == want_removed
    if name == "robust60":
        assert removed == [(27, 41)]
    assert np.array_equal(ids, REC[f"{name}/out_ids"])
    rerr, rposes = float(REC[f"{name}/err"]), REC[f"{name}/out_poses"]
    d = max(abs(err - rerr) / err, np.abs(poses - rposes).max() / np.abs(poses).max())
    print(name, "removed", removed, "err", err, rerr, "largest difference", d, "share of its tolerance", d / tol)
    assert abs(err - rerr) <= tol * err
    assert np.abs(poses - rposes).max() <= tol * np.abs(poses).max()
    if name != "multi48_bidir":
        return
    # the device form, bit for bit
    up = lambda a: torch_cuda.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda:0")  # noqa: E731
    derr, doid, dout, dremoved = g.optimize_robust_device(c["ids"], up(c["poses"]), c["frm"], c["to"], up(c["meas"]), up(c["info"]))
    assert derr == err and np.array_equal(doid, ids) and dremoved == removed and np.array_equal(dout.cpu().numpy(), poses)
    # removed_cap below the number removed, through the C ABI: n_removed counts all, only removed_cap pairs are written
    assert len(removed) == 4
    cg, keep = c_graph(pkg, c)
    n, nrem, cerr = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
    oid, out = np.empty(len(c["ids"]), np.int32), np.empty((len(c["ids"]), 12), np.float64)
    for cap in (2, 0):
        rem = np.full((len(removed), 2), -7, np.int32)
        st = engine._L.sbm_pgo_optimize_robust(engine._h, ctypes.byref(g.params), ctypes.byref(cg), ctypes.byref(n), oid.ctypes.data,
                                               out.ctypes.data, ctypes.byref(cerr), rem.ctypes.data if cap else None, cap,
                                               ctypes.byref(nrem))
        assert st == 0 and nrem.value == len(removed) and n.value == len(ids) and cerr.value == err
        assert [tuple(r) for r in rem[:cap].tolist()] == removed[:cap] and (rem[cap:] == -7).all()
        assert np.array_equal(out[:n.value].reshape(-1, 3, 4), poses)


def test_robust_loop_drops_an_unreachable_vertex(pkg, engine):
    c = pc.unreachable_case()
    err, ids, poses, removed = pkg.PoseGraph(engine, num=4).optimize_robust(*pc.args(c))
    assert removed == [] and np.array_equal(ids, REC["unreachable/out_ids"]) and 9 not in ids
    assert np.abs(poses - REC["unreachable/out_poses"]).max() <= TOL * np.abs(poses).max()


def test_device_form_equals_the_host_form_bit_for_bit(pkg, engine, torch_cuda):
    torch = torch_cuda
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to("cuda:0")  # noqa: E731
    c = pc.iteration_case()
    perm = np.random.default_rng(5).permutation(len(c["ids"]))          # vertices in no particular order
    ids, poses = c["ids"][perm], c["poses"][perm]
    for coupling in (pc.REFERENCE, pc.SYMMETRIC):
        g = pkg.PoseGraph(engine, num=3, coupling=coupling, run_max=RUN_MAX)
        err, oid, out = g.optimize(ids, poses, c["frm"], c["to"], c["meas"], c["info"])
        derr, doid, dout = g.optimize_device(ids, up(poses), c["frm"], c["to"], up(c["meas"]), up(c["info"]))
        assert derr == err and np.array_equal(doid, oid) and np.array_equal(dout.cpu().numpy(), out)
    c = pc.robust_case()
    g = pkg.PoseGraph(engine, num=20, run_max=RUN_MAX)
    err, oid, out, removed = g.optimize_robust(*pc.args(c))
    derr, doid, dout, dremoved = g.optimize_robust_device(c["ids"], up(c["poses"]), c["frm"], c["to"], up(c["meas"]), up(c["info"]))
    assert derr == err and np.array_equal(doid, oid) and dremoved == removed and np.array_equal(dout.cpu().numpy(), out)


def test_no_free_vertex_and_default_run_length(pkg, engine):
    err, ids, poses = pkg.PoseGraph(engine, num=3).optimize([1], pc.pose()[None], [], [], np.zeros((0, 3, 4)), np.zeros((0, 6, 6)))
    assert err == 0.0 and np.array_equal(poses[0], pc.pose())
    c = pc.chain_graph(150, [(120, 10), (20, 140)], seed=61, noise=3e-3)       # runs of 64 and the Schur part together
    g = pkg.PoseGraph(engine, num=3, coupling=pc.SYMMETRIC)
    err, ids, poses = g.optimize(*pc.args(c))
    werr, _, wposes = pc.run_optimize(*pc.args(c), 3, coupling=pc.SYMMETRIC)
    assert g.last_plan()[0].longest_run <= 64
    assert abs(err - werr) <= TOL * werr and np.abs(poses - wposes).max() <= TOL * np.abs(wposes).max()


def test_stage_names_answer(pkg, engine):
    import ctypes
    names = ("pgo_linearise", "pgo_assemble", "pgo_solve", "pgo_update", "pgo_total")

    def read(name):
        v = ctypes.c_float(-1.0)
        return engine._L.sbm_get_profile(engine._h, name.encode(), ctypes.byref(v)), v.value

    engine.set_profiling(1)
    try:
        for n in names:
            assert read(n) == (0, 0.0)
        g = pkg.PoseGraph(engine, num=2, run_max=RUN_MAX)
        g.optimize(*pc.args(pc.iteration_case()))
        t = {n: read(n) for n in names}
        print(t)
        assert all(st == 0 and ms > 0.0 for st, ms in t.values()), t
        assert g.profile().keys() == set(names) and read("pgo")[0] == -23
    finally:
        engine.set_profiling(0)
