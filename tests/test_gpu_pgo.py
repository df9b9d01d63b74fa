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
branch case sits next to the singularity of dq/dR on purpose and is compared to 1e-6."""
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


@pytest.mark.parametrize("coupling", [pc.REFERENCE, pc.SYMMETRIC], ids=["reference", "symmetric"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_solve_backward_error_and_first_step(pkg, engine, name, coupling):
    c = SHAPES[name]
    g = pkg.PoseGraph(engine, num=1, coupling=coupling, run_max=RUN_MAX)
    err, ids, poses = g.optimize(*pc.args(c))
    info, lam, its = g.last_plan()
    want_info, _, rc, _ = pkg.pgo_plan(g.params, *pc.args(c))
    assert bytes(info) == bytes(want_info) and its == 1                      # the plan agrees with what the call launched
    dbg = g.debug(len(c["frm"]))
    # ... and with what it exported: one diagonal block, b and x per free vertex, one lower block per coupled pair
    assert (len(dbg["D"]), len(dbg["b"]), len(dbg["x"]), len(dbg["E"])) == (want_info.n_free,) * 3 + (want_info.n_slots,)
    tr = {}
    werr, wids, wposes = pc.run_optimize(*pc.args(c), 1, coupling=coupling, trace=tr)
    S = dense(dbg, rc, info.n_free, lam)
    b, x = dbg["b"].reshape(-1), dbg["x"].reshape(-1)
    Sw = tr["A"] + np.tril(tr["A"], -1).T + tr["lam"][0] * np.eye(len(b))
    assert np.abs(S - Sw).max() <= 1e-12 * np.abs(Sw).max() and np.abs(b - tr["b"]).max() <= 1e-12 * max(np.abs(tr["b"]).max(), 1e-300)
    e_dev, e_np = eta(S, x, b), eta(S, np.linalg.solve(S, b), b)
    print(name, coupling, "junctions", info.n_junctions, "runs", info.n_runs, "eta device", e_dev, "eta numpy", e_np)
    assert e_dev <= 16 * e_np
    assert abs(lam - tr["lam"][0]) <= TOL * tr["lam"][0]
    assert np.array_equal(ids, wids) and np.abs(poses - wposes).max() <= TOL * np.abs(wposes).max()


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


def test_robust_loop_equals_the_recording(pkg, engine):
    c = pc.robust_case()
    g = pkg.PoseGraph(engine, num=20, run_max=RUN_MAX)
    err, ids, poses, removed = g.optimize_robust(*pc.args(c))
    assert removed == [tuple(r) for r in REC["robust60/removed"].tolist()] == [(27, 41)]
    assert np.array_equal(ids, REC["robust60/out_ids"])
    print("robust err", err, float(REC["robust60/err"]))
    assert abs(err - float(REC["robust60/err"])) <= TOL * err
    assert np.abs(poses - REC["robust60/out_poses"]).max() <= TOL * np.abs(poses).max()


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
