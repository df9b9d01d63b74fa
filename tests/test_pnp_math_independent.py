"""The arithmetic of u96-slam_amd/csrc/sbm_pnp_math.h, through the one-line exports of oracle/pnp_ref, against the independent
statement in tests/pnp_independent.py (expm, mpmath.diff, numpy.linalg, scipy's LM). The parity tests compile this header on both
sides and cannot see an error in it; these can. No GPU.

Tolerances. Where the number formats give a bound it is derived in the test's docstring. Where they do not (the Jacobi SVD's
accuracy, dR/dr where 1 - cos cancels, the logarithm next to pi, LM stopped by its FLT_EPSILON rule) the header's largest
deviation over the listed inputs was measured on the CPU and stands in MEASURED; hold() asserts 8 times that (other seeds, other
libm builds). DESIGN.md section 12 has the table. None of these figures comes from the device."""
import math

import numpy as np
import pytest

import pnp_independent as ind
import pnp_ref
from test_gpu_pnp import LOCAL, K, Store

EPS = np.finfo(np.float64).eps
EPS32 = float(np.finfo(np.float32).eps)

MEASURED = {
    "svd values / s_max": 1.7e-15,
    "svd U W Vt - A / s_max": 1.0e-15,
    "svd Vt Vt^T - I": 3.2e-15,
    "svd_solve - lstsq, relative": 5.8e-15,
    "svd_solve minimum norm, relative": 5.2e-15,
    "qr_solve - lstsq, relative": 1.3e-15,
    "dRdr theta 0": 0.0e+00,
    "dRdr theta 1e-300": 5.0e-301,
    "dRdr theta 1e-17": 1.0e-17,
    "dRdr theta 3e-16": 1.5e-16,
    "dRdr theta 1e-08": 5.0e-09,
    "dRdr theta 0.001": 7.8e-15,
    "dRdr theta 1": 1.1e-16,
    "dRdr theta pi-1e-6": 2.8e-16,
    "dRdr theta pi": 1.1e-16,
    "dRdr theta 3.5": 3.3e-16,
    "dRdr theta 2pi": 1.8e-16,
    "log R(rv) - R, pi-1e-3": 8.2e-14,
    "log R(rv) - R, pi-1e-7": 2.2e-07,
    "log R(rv) - R, pi-1e-11": 1.0e-11,
    "log R(rv) - R, pi": 2.8e-16,
    "log vector, pi-1e-3": 1.3e-13,
    "log vector, pi-1e-7": 1.6e-07,
    "log vector, pi-1e-11": 1.0e-11,
    "log vector, pi": 4.4e-16,
    "lm_point e": 1.8e-13,
    "lm_point J / |J|": 1.4e-15,
    "lm_point JtJ / |JtJ|": 1.5e-15,
    "lm_point Jte / |Jte|": 1.1e-12,
    "lm_point ete, relative": 3.8e-13,
    "lm_step lambda 0.001, relative": 1.2e-13,
    "lm_step lambda 1, relative": 5.2e-14,
    "lm_step lambda 1e+16, relative": 1.6e-14,
    "refine rvec - minimum": 1.8e-09,
    "refine tvec - minimum": 2.7e-08,
    "refine |Jte| at pose / at RANSAC pose": 2.0e-09,
    "tf_inverse general / |inv|": 1.7e-07,
}
SEEN = {}


def hold(name, value):
    """value (a deviation measured now) against 8 x the figure recorded in MEASURED."""
    value = float(value)
    SEEN[name] = max(SEEN.get(name, 0.0), value)
    print(f"measured {name!r}: {value:.3e} (recorded {MEASURED[name]:.3e})")
    assert value <= 8 * MEASURED[name], (name, value, MEASURED[name])


def unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


# ---- SVD and the solvers -------------------------------------------------------------------------------------------------
def svd_cases():
    """(name, A): the shapes of the header's call sites -- 12 x 12 M^T M and 3 x 3 (pnp_epnp6, pnp_compute_R_and_t), 6 x 6
    (pnp_lm_step), 6 x 3 / 6 x 4 / 6 x 5 (the betas), 4 x 4 -- a dozen random ones each, and the degenerate ones."""
    rng = np.random.default_rng(1)
    out = []
    for k in range(12):
        M = rng.normal(size=(12, 12))
        out.append((f"MtM {k}", M.T @ M))
        for m, n in ((6, 6), (3, 3), (4, 4), (6, 3), (6, 4), (6, 5)):
            out.append((f"{m}x{n} {k}", rng.normal(size=(m, n)) * 10.0 ** rng.integers(-3, 4)))
    B, C = rng.integers(-4, 5, (6, 5)).astype(float), rng.integers(-4, 5, (5, 6)).astype(float)
    out.append(("rank 5 of 6", B @ C))
    out.append(("zero", np.zeros((6, 6))))
    Q1, Q2 = np.linalg.qr(rng.normal(size=(6, 6)))[0], np.linalg.qr(rng.normal(size=(6, 6)))[0]
    out.append(("two equal singular values", Q1 @ np.diag([5.0, 3.0, 3.0, 2.0, 1.0, 0.5]) @ Q2))
    A = rng.normal(size=(6, 6))
    A[:, 2] *= 1e-12
    out.append(("a column scaled by 1e-12", A))
    M = rng.normal(size=(12, 12))
    M[6:] = 0                                  # EPnP's M has rank below 12: several zero singular values of M^T M
    out.append(("MtM of rank 6", M.T @ M))
    return out


def test_jacobi_svd():
    for name, A in svd_cases():
        U, W, Vt = pnp_ref.jacobi_svd(A)
        s = ind.svd(A)[1]
        top = max(s[0], 1e-300)
        assert np.all(np.diff(W) <= 0) and np.all(W >= 0), name
        hold("svd values / s_max", np.abs(W - s).max() / top)
        hold("svd U W Vt - A / s_max", np.abs((U * W) @ Vt - A).max() / top)
        hold("svd Vt Vt^T - I", np.abs(Vt @ Vt.T - np.eye(A.shape[1])).max())


def test_svd_solve_and_qr_solve_are_least_squares():
    rng = np.random.default_rng(2)
    for m, n in ((6, 3), (6, 4), (6, 5), (6, 6)) * 12:
        A, b = rng.normal(size=(m, n)), rng.normal(size=m)
        want = ind.lstsq(A, b)
        hold("svd_solve - lstsq, relative", np.abs(pnp_ref.svd_solve(A, b) - want).max() / np.abs(want).max())
        if (m, n) == (6, 4):
            hold("qr_solve - lstsq, relative", np.abs(pnp_ref.qr_solve(A, b) - want).max() / np.abs(want).max())


def test_svd_solve_minimum_norm_on_rank_deficient_input():
    rng = np.random.default_rng(3)
    for trial in range(12):
        n = (3, 4, 5, 6)[trial % 4]
        A = (rng.integers(-4, 5, (6, n - 1)) @ rng.integers(-4, 5, (n - 1, n))).astype(float)   # rank n - 1, exactly
        assert np.linalg.matrix_rank(A) == n - 1
        b = rng.normal(size=6)
        want = ind.lstsq(A, b)
        got = pnp_ref.svd_solve(A, b)
        hold("svd_solve minimum norm, relative", np.abs(got - want).max() / np.abs(want).max())
    assert np.array_equal(pnp_ref.svd_solve(np.zeros((6, 4)), np.ones(6)), np.zeros(4))


def test_qr_solve_zero_column_keeps_x():
    A = np.random.default_rng(4).normal(size=(6, 4))
    A[:, 1] = 0
    assert np.array_equal(pnp_ref.qr_solve(A, np.ones(6), x0=[1, 2, 3, 4]), [1, 2, 3, 4])


# ---- Rodrigues -----------------------------------------------------------------------------------------------------------
THETAS = [("0", 0.0), ("1e-300", 1e-300), ("1e-17", 1e-17), ("3e-16", 3e-16), ("1e-08", 1e-8), ("0.001", 1e-3), ("1", 1.0),
          ("pi-1e-6", math.pi - 1e-6), ("pi", math.pi), ("3.5", 3.5), ("2pi", 2 * math.pi)]
AXES = [np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0]), unit([0.3, -0.5, 0.8]), unit([-0.7, 0.6, 0.2])]


@pytest.mark.parametrize("name,theta", THETAS, ids=[t[0] for t in THETAS])
def test_rodrigues_and_its_derivative(name, theta):
    """R against expm at 50 digits: theta carries about 2 eps relative (three squares, two sums, a square root), which moves cos
    and sin by up to 2 theta eps; the unit axis carries 2 eps more per component, its products 4, and c I + c1 rr^T + s [r]x
    adds three roundings: (4 max(theta, 1) + 8) eps in all. dRdr against mpmath.diff of expm: measured (1 - cos cancels)."""
    worst = 0.0
    for ax in AXES:
        rv = ax * theta
        R, d = pnp_ref.rodrigues_d(rv)
        assert np.abs(R - ind.rot_mp(rv)).max() <= (4 * max(theta, 1.0) + 8) * EPS, (name, ax)
        worst = max(worst, np.abs(d - ind.drot(rv)).max())
    hold(f"dRdr theta {name}", worst)


# ---- Rodrigues, inverse --------------------------------------------------------------------------------------------------
LOG_AXES = [np.array(a, float) for a in ([1, 0, 0], [0, 1, 0], [0, 0, 1])] + \
           [unit([sx * 0.5, sy * 0.3, sz * 0.8]) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)] + \
           [unit([sx * 0.1, sy * 0.7, sz * 0.6]) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)] + \
           [unit([0, 0.6, 0.8]), unit([0, -0.6, 0.8]), unit([0, 0.6, -0.8]), unit([0, -0.6, -0.8])]
LOG_ANGLES = [("pi-1e-3", 1e-3), ("pi-1e-7", 1e-7), ("pi-1e-11", 1e-11), ("pi", 0.0)]


def rotation_about(ax, below_pi):
    """R of angle pi - below_pi about ax, from 50 digits (pi itself is not a float64), and the rotation vector."""
    import mpmath as mp

    with mp.workdps(ind.DPS):
        a = [mp.mpf(float(v)) for v in ax]
        n = mp.sqrt(sum(v * v for v in a))
        ang = mp.pi - mp.mpf(below_pi)
        rv = [v / n * ang for v in a]
        return ind.rot_mp(rv), np.array([float(v) for v in rv])


@pytest.mark.parametrize("name,below", LOG_ANGLES, ids=[a[0] for a in LOG_ANGLES])
def test_rodrigues_inverse_next_to_pi(name, below):
    """As a rotation: R(rv_out) against R. As a vector: against the rotation vector R was built from; from 1e-5 below pi on the
    header answers with OpenCV's rule for angle pi (x >= 0 and so on), so there r and -r count as one. Both measured."""
    worst_r = worst_v = 0.0
    for ax in LOG_AXES:
        R, want = rotation_about(ax, below)
        rv = pnp_ref.rodrigues_inv(R)
        assert np.linalg.norm(rv) <= math.pi + 4 * EPS
        worst_r = max(worst_r, np.abs(ind.rot_mp(rv) - R).max())
        dv = np.abs(rv - want).max()
        if below <= 1e-5:
            dv = min(dv, np.abs(rv + want).max())
        worst_v = max(worst_v, dv)
        mine = ind.log_rot(R)                    # the independent logarithm agrees with the construction
        assert min(np.abs(mine - want).max(), np.abs(mine + want).max() if below == 0 else math.inf) < 1e-13, (name, ax)
    hold(f"log R(rv) - R, {name}", worst_r)
    hold(f"log vector, {name}", worst_v)


def test_rodrigues_inverse_generic_angles():
    """Away from 0 and pi the logarithm is well conditioned: rv back to 64 eps / sin(angle) (the axis is the axial vector of
    R - R^T, of length 2 sin, known to a few eps absolute)."""
    rng = np.random.default_rng(5)
    for _ in range(50):
        rv = unit(rng.normal(size=3)) * rng.uniform(0.05, 3.0)
        got = pnp_ref.rodrigues_inv(ind.rot_mp(rv))
        assert np.abs(got - rv).max() <= 64 * EPS / math.sin(np.linalg.norm(rv)), rv
        assert np.abs(ind.log_rot(ind.rot_mp(rv)) - rv).max() <= 64 * EPS / math.sin(np.linalg.norm(rv)), rv


# ---- LM point ------------------------------------------------------------------------------------------------------------
def lm_cases():
    """77 (pose, point, observation): |r| up to 3, depth 0.5 to 40 in the camera, the observation within a pixel or so of the
    projection (float32). The first twelve walk the corners (|r|, depth); the other 65 share one pose, for the packing test."""
    rng = np.random.default_rng(6)
    out = []
    shared = np.r_[unit(rng.normal(size=3)) * 1.3, rng.normal(0, 0.3, 3)]
    grid = [(a, z) for a in (0.0, 0.01, 1.0, 3.0) for z in (0.5, 5.0, 40.0)]
    for i in range(77):
        if i < 12:
            x = np.r_[unit(rng.normal(size=3)) * grid[i][0], rng.normal(0, 0.3, 3)]
            z = grid[i][1]
        else:
            x, z = shared, rng.uniform(0.5, 40)
        Xc = np.array([rng.uniform(-0.4, 0.4) * z, rng.uniform(-0.15, 0.15) * z, z])
        p = (ind.rot(x[:3]).T @ (Xc - x[3:])).astype(np.float32)
        m = (ind.project(x[:3], x[3:], p, K)[0] + rng.uniform(-1, 1, 2)).astype(np.float32)
        out.append((x, p, m))
    return out


@pytest.fixture(scope="module")
def lm_terms():
    """The independent e and J of every case, computed once."""
    cases = lm_cases()
    return cases, [ind.residual_jacobian(x, p, m, K) for x, p, m in cases]


def header_acc(x, P, M, with_j=1):
    R, d = pnp_ref.rodrigues_d(x[:3])
    return pnp_ref.lm_points(R, d, x[3:], P, M, K, with_j)


def unpack(acc):
    JtJ = np.zeros((6, 6))
    JtJ[np.triu_indices(6)] = acc[:21]           # the upper triangle, row by row
    return JtJ + np.triu(JtJ, 1).T, acc[21:27], acc[27]


def test_lm_point_residual_and_jacobian(lm_terms):
    """J itself, not only J^T J: J^T e is linear in e, so moving the observation by one pixel in u (exact in float32 below 4096)
    changes acc[21..26] by J's first row, and likewise in v. e from e^T e and J^T e needs no such trick: it is compared through
    them below."""
    cases, terms = lm_terms
    for (x, p, m), (e, J) in zip(cases[:24], terms[:24]):
        a0 = header_acc(x, p, m)
        rows = [a0[21:27] - header_acc(x, p, m + np.array(d, np.float32))[21:27] for d in ((1, 0), (0, 1))]
        hold("lm_point J / |J|", np.abs(np.array(rows) - J).max() / np.abs(J).max())
        JtJ, Jte, ete = unpack(a0)
        hold("lm_point e", abs(math.sqrt(ete) - np.linalg.norm(e)))
        hold("lm_point JtJ / |JtJ|", np.abs(JtJ - J.T @ J).max() / np.abs(J.T @ J).max())
        hold("lm_point Jte / |Jte|", np.abs(Jte - J.T @ e).max() / np.abs(J.T @ e).max())


@pytest.mark.parametrize("n", [1, 2, 65])
def test_lm_point_packs_28_accumulators(lm_terms, n):
    cases, terms = lm_terms
    sel = list(range(12, 12 + n))   # one pose
    x = cases[12][0]
    P, M = np.array([cases[i][1] for i in sel]), np.array([cases[i][2] for i in sel])
    JtJ, Jte, ete = unpack(header_acc(x, P, M))
    wJ = sum(terms[i][1].T @ terms[i][1] for i in sel)
    we = sum(terms[i][1].T @ terms[i][0] for i in sel)
    wee = sum(float(terms[i][0] @ terms[i][0]) for i in sel)
    hold("lm_point JtJ / |JtJ|", np.abs(JtJ - wJ).max() / np.abs(wJ).max())
    hold("lm_point Jte / |Jte|", np.abs(Jte - we).max() / np.abs(we).max())
    hold("lm_point ete, relative", abs(ete - wee) / wee)
    only_e = header_acc(x, P, M, with_j=0)
    assert np.all(only_e[:27] == 0) and only_e[27] == ete


def test_lm_point_at_z_zero_is_not_divided():
    """R = I, t_z = -Z: the camera z is exactly 0 and x, y stay undivided (z = Z ? 1 / Z : 1). The residual only."""
    x = np.array([0, 0, 0, 0.5, 0.25, -3.0])
    p, m = np.array([1, 2, 3], np.float32), np.array([1700.5, 1800.25], np.float32)
    e = ind.residual(x, p, m, K)[0]
    assert np.allclose(e, [K[0] * 1.5 + K[2] - 1700.5, K[1] * 2.25 + K[3] - 1800.25], rtol=0, atol=1e-12)
    got = header_acc(x, p, m, with_j=0)[27]
    assert abs(got - e @ e) <= 8 * EPS * (e @ e)


# ---- LM step -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [1e-3, 1.0, 1e16])
def test_lm_step_is_the_damped_solve(lm_terms, lam):
    cases, _ = lm_terms
    x = cases[12][0]
    acc = header_acc(x, np.array([c[1] for c in cases[12:]]), np.array([c[2] for c in cases[12:]]))
    JtJ, Jte, _ = unpack(acc)
    want = ind.damped_step(JtJ, Jte, lam)
    got = x - pnp_ref.lm_step(acc, lam, x)
    assert np.abs(want).max() > 0
    if lam < 1e10:
        hold(f"lm_step lambda {lam:g}, relative", np.abs(got - want).max() / np.abs(want).max())
    else:   # the step is 1e-16 of the pose: x - (x - delta) cannot show it; compare the pose, and the step from a zero pose
        assert np.abs(pnp_ref.lm_step(acc, lam, x) - (x - want)).max() <= 2 * EPS * np.abs(x).max()
        got0 = -pnp_ref.lm_step(acc, lam, np.zeros(6))
        hold(f"lm_step lambda {lam:g}, relative", np.abs(got0 - want).max() / np.abs(want).max())


def test_lm_converged_is_the_relative_step_below_flt_epsilon():
    p = np.array([0.1, -0.2, 0.3, 1.0, 2.0, -3.0])
    n = np.linalg.norm(p)
    d = np.array([1.0, 0, 0, 0, 0, 0])
    assert pnp_ref.lm_converged(p + d * n * EPS32 * 0.99, p) and not pnp_ref.lm_converged(p + d * n * EPS32 * 1.01, p)
    assert pnp_ref.lm_converged(p, p) and not pnp_ref.lm_converged(d, np.zeros(6))


# ---- the refine as a whole -----------------------------------------------------------------------------------------------
def refine_scene(n, rounds):
    rng = np.random.default_rng(1000 + 10 * n + rounds)
    st = Store(rng, [n], n, outliers=0.3, noise=float(rng.uniform(0.5, 0.8)))
    pairs = np.c_[np.arange(n), np.arange(n)].astype(np.int32)
    return st, pairs


def estimate(st, pairs, rounds, local=None, xyz_to=None):
    p = pnp_ref.pnp_params(min_inliers=6, refine_iterations=rounds)
    n = st.count[0]
    return pnp_ref.estimate(st.xyz[0, :n], st.kpts[1, :n], st.xyz[1, :n] if xyz_to is None else xyz_to, pairs, K, local, p)


@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("n", [20, 63, 64, 65, 129, 400])
def test_refined_pose_is_the_lm_minimum(n, rounds):
    """The returned pose against scipy's minimum over the set the last solve ran on, started where that solve started (the pose
    of the same job with one solve fewer). After a normal exit or a break on an unchanged set the returned list is that set;
    these scenes never break on too few inliers. Measured: the FLT_EPSILON stop rule decides how far from the minimum LM ends."""
    st, pairs = refine_scene(n, rounds)
    r, inl, ran, _, ex = estimate(st, pairs, rounds)
    assert r["status"] == 0 and r["refine_exit"] in (0, 2) and r["refine_solves"] >= 1
    before = estimate(st, pairs, int(r["refine_solves"]) - 1)[0]
    ransac = estimate(st, pairs, 0)[0]
    if r["refine_solves"] == 1:
        assert np.array_equal(inl, ex["matches"][ran]) or r["refine_exit"] == 2
    P, uv = st.xyz[0, inl], st.kpts[1, inl]      # pairs are the identity: a from-index is the point's index
    x0 = np.r_[before["rvec"], before["tvec"]]
    got = np.r_[r["rvec"], r["tvec"]]
    best = ind.lm_minimum(x0, P, uv, K)
    assert np.sum(ind.residual(best, P, uv, K) ** 2) <= np.sum(ind.residual(got, P, uv, K) ** 2) * (1 + 1e-12)
    hold("refine rvec - minimum", np.abs(got[:3] - best[:3]).max())
    hold("refine tvec - minimum", np.abs(got[3:] - best[3:]).max())
    g_ransac = ind.gradient(np.r_[ransac["rvec"], ransac["tvec"]], P, uv, K)
    hold("refine |Jte| at pose / at RANSAC pose", np.linalg.norm(ind.gradient(got, P, uv, K)) / np.linalg.norm(g_ransac))
    assert np.abs(r["R"].reshape(3, 3) - ind.rot_mp(r["rvec"])).max() <= 12 * EPS


# ---- reprojection error --------------------------------------------------------------------------------------------------
def test_reproj_err_against_float64():
    """The header rounds the projection to float32 (half an ulp of a coordinate up to 2048: 2^-13 / 2... by np.spacing), takes
    the difference in float32 (half an ulp of the difference) and rounds the norm to float32 (half an ulp of it). So
    |err - err64| <= sqrt(2) (ulp32(coordinate) + ulp32(difference)) / 2 + ulp32(err) / 2, plus 1e-9 for the double part."""
    rng = np.random.default_rng(7)
    Kw = np.array([1400.0, 1400.0, 1024.0, 1024.0])
    for _ in range(300):
        rv, t = rng.normal(0, 0.3, 3), rng.normal(0, 0.3, 3)
        z = rng.uniform(0.5, 40)
        Xc = np.array([rng.uniform(-0.7, 0.7) * z, rng.uniform(-0.7, 0.7) * z, z])
        p = (ind.rot(rv).T @ (Xc - t)).astype(np.float32)
        uv64 = ind.project(rv, t, p, Kw)[0]
        m = (uv64 + rng.choice([0.0, 1.0, 100.0]) * rng.normal(0, 1, 2)).astype(np.float32)
        R = ind.rot_mp(rv)
        want = float(np.linalg.norm(uv64 - m.astype(np.float64)))
        sp = lambda v: float(np.spacing(np.float32(abs(v))))
        bound = math.sqrt(2) * (sp(np.abs(uv64).max()) + sp(np.abs(uv64 - m).max())) / 2 + sp(want) / 2 + 1e-9
        assert abs(float(pnp_ref.reproj_err(R, t, p, m, Kw)) - want) <= bound, (rv, t, p, m)
    # camera z exactly 0: not divided
    got = pnp_ref.reproj_err(np.eye(3), [0.5, 0.25, -3.0], np.array([1, 2, 3], np.float32), np.array([1700, 1800], np.float32), K)
    want = np.linalg.norm(ind.project(np.eye(3), [0.5, 0.25, -3.0], [[1, 2, 3]], K)[0] - [1700, 1800])
    assert abs(float(got) - want) <= 2e-4


# ---- transform -----------------------------------------------------------------------------------------------------------
def about(axis, a):
    return ind.rot_mp(np.eye(3)[axis] * a)


LOCALS = {
    "identity": np.c_[np.eye(3), [0.0, 0, 0]],                       # trace > 0
    "3 rad about x": np.c_[about(0, 3.0), [0.1, 0.05, 1.2]],         # trace < 0, m00 the largest
    "3 rad about y": np.c_[about(1, 3.0), [0.1, 0.05, 1.2]],         # m11
    "3 rad about z": np.c_[about(2, 3.0), [0.1, 0.05, 1.2]],         # m22
    "trace 0": np.asarray(LOCAL, float).reshape(3, 4),              # trace exactly 0 with the identity pose: not > 0
}


def poses():
    rng = np.random.default_rng(8)
    return [(np.eye(3), np.zeros(3))] + [(ind.rot_mp(rng.normal(0, 0.05, 3)), rng.normal(0, 0.3, 3)) for _ in range(6)]


def ulps4(M):
    return 4 * max(1.0, float(np.abs(M).max())) * EPS32


@pytest.mark.parametrize("name", list(LOCALS))
def test_tf_mul_is_the_product(name):
    """The project's own bound: 4 float ulps of the largest entry (at least 1). Orthonormality: R R^T = |q|^4 I for the matrix
    of a quaternion q; the normalised q has |q|^2 within 3 eps32 of 1 (a square root, a division, four squares), so 6 eps32, and
    each entry of R carries about 2 eps32 of rounding (two or three products and a sum), which moves an entry of R R^T by up to
    2 sqrt(3) 2 eps32 = 7 eps32: 16 eps32 bounds both."""
    lo = LOCALS[name].astype(np.float32)
    for R, t in poses():
        B = np.c_[R, t].astype(np.float32)
        C = pnp_ref.tf_mul(lo, B)
        want = (ind._h(lo) @ ind._h(B))[:3]
        assert np.abs(C - want).max() <= ulps4(want), (name, np.abs(C - want).max())
        Rc = C[:, :3].astype(np.float64)
        assert np.abs(Rc @ Rc.T - np.eye(3)).max() <= 16 * EPS32 and abs(np.linalg.det(Rc) - 1) <= 16 * EPS32


@pytest.mark.parametrize("name", [None] + list(LOCALS))
def test_transform_is_the_inverse_of_local_times_pnp(name):
    lo = None if name is None else LOCALS[name].astype(np.float32)
    for R, t in poses():
        got = pnp_ref.transform(R, t, lo)
        want = ind.transform(R, t, lo)
        assert np.abs(got - want).max() <= ulps4(want), (name, np.abs(got - want).max())


def test_tf_inverse():
    """Rotations and near-rotations: 4 float ulps of the largest entry. A general affine map (scale, shear): measured."""
    rng = np.random.default_rng(9)
    for _ in range(20):
        A = np.c_[ind.rot_mp(unit(rng.normal(size=3)) * rng.uniform(0, 3.1)), rng.normal(0, 2, 3)].astype(np.float32)
        want = np.linalg.inv(ind._h(A))[:3]
        assert np.abs(pnp_ref.tf_inverse(A) - want).max() <= ulps4(want)
    for _ in range(20):
        A = np.c_[ind.rot_mp(rng.normal(size=3)) @ np.diag(rng.uniform(0.5, 3, 3)) @ (np.eye(3) + np.triu(rng.normal(0, 0.3, (3, 3)), 1)),
                  rng.normal(0, 2, 3)].astype(np.float32)
        want = np.linalg.inv(ind._h(A))[:3]
        hold("tf_inverse general / |inv|", np.abs(pnp_ref.tf_inverse(A) - want).max() / np.abs(want).max())


# ---- covariance ----------------------------------------------------------------------------------------------------------
def cov_bounds(obj, to, T):
    """Float32 against float64. T * to: each coordinate is a sum of four terms, at most 4 roundings of the running magnitude
    S = sum |T_ij| |to_j| + |T_i3|: d = 4 eps32 S per coordinate, and as much again for obj - (T * to) and for the vectors from
    T's origin, so 2 d. Squared distance: 2 |diff| sqrt(3) 2d + 3 (2d)^2, and 4 eps32 of it for its own three products and sums.
    Cosine: each unit vector carries 2d / |v| plus 3 eps32 from the normalisation, the dot product 3 eps32, and the angle's
    rounding to float32 moves its cosine by at most pi eps32 / 2."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    S = float((np.abs(T[:, :3]) @ np.abs(to) + np.abs(T[:, 3])).max() + np.abs(obj).max())
    d = 2 * 4 * EPS32 * S
    dist, cosang, ang = ind.cov_terms(obj, to, T)
    v1, v2 = np.linalg.norm(obj - T[:, 3]), np.linalg.norm(T[:, :3] @ to)
    return (2 * math.sqrt(3 * dist) * d + 3 * d * d + 4 * EPS32 * dist, d / v1 + d / v2 + 9 * EPS32 + math.pi * EPS32 / 2)


def test_cov_terms():
    rng = np.random.default_rng(10)
    for i in range(200):
        R, t = ind.rot_mp(rng.normal(0, 0.3, 3)), rng.normal(0, 1, 3)
        T = ind.transform(R, t, LOCALS["3 rad about y"] if i % 2 else None).astype(np.float32)
        to = np.array([rng.uniform(-8, 8), rng.uniform(-3, 3), rng.uniform(4, 40)], np.float32)
        obj = (T[:, :3].astype(np.float64) @ to + T[:, 3] + rng.normal(0, [0.0, 1e-3, 0.1, 2.0][i % 4], 3)).astype(np.float32)
        dist, ang = pnp_ref.cov_terms(obj, to, T)
        wd, wc, _ = ind.cov_terms(obj.astype(np.float64), to.astype(np.float64), T)
        bd, bc = cov_bounds(obj.astype(np.float64), to.astype(np.float64), T)
        assert abs(float(dist) - wd) <= bd, (i, dist, wd, bd)
        assert abs(math.cos(float(ang)) - wc) <= bc, (i, ang, wc, bc)


COV_CASES = {"odd": 5, "even": 4, "none finite": 0, "clamped": -1}


def cov_scene(kind, local):
    """A 65-point job whose to-points are the from-points in the to-camera moved by 0.1 m (exact, and in a scene without pixel
    noise, for "clamped": the pose is then the true one and the distances are float32 roundings), finite for 5, 4 or none of the
    job's inliers. Returns what estimate() takes and the inlier list (which the to-points do not move)."""
    rng = np.random.default_rng(50)
    st = Store(rng, [65], 65, outliers=0.3, noise=0.0 if kind == "clamped" else 0.3)
    pairs = np.c_[np.arange(65), np.arange(65)].astype(np.int32)
    inl = estimate(st, pairs, 1, local)[1]
    to = st.xyz[1, :65].copy()
    if kind != "clamped":
        to += rng.normal(0, 0.1, to.shape).astype(np.float32)
        to[inl[COV_CASES[kind]:]] = np.nan
    return st, pairs, to, inl


@pytest.mark.parametrize("local", [None, "3 rad about y"])
@pytest.mark.parametrize("kind", list(COV_CASES))
def test_covariance_scales_are_the_upper_medians(kind, local):
    """cov_dist and cov_angle of a whole job against sorted[n >> 1] of the independent terms under the independent transform.
    A median moves by no more than its elements do, so the bound is the largest of cov_bounds; the angle through its cosine."""
    lo = None if local is None else LOCALS[local].astype(np.float32)
    st, pairs, to, inl = cov_scene(kind, lo)
    r, inl2, _, _, _ = estimate(st, pairs, 1, lo, xyz_to=to)
    assert np.array_equal(inl, inl2)
    check_cov(r, inl2, st, to, lo, kind, local)


def check_cov(r, inl, st, to, lo, kind, local):
    assert r["status"] == 0
    T = ind.transform(r["R"].reshape(3, 3), r["tvec"], lo)
    fin = [i for i in inl if np.isfinite(to[i]).all()]
    terms = [ind.cov_terms(st.xyz[0, i], to[i], T) for i in fin]
    bounds = [cov_bounds(st.xyz[0, i].astype(np.float64), to[i].astype(np.float64), T) for i in fin]
    if kind == "none finite":
        assert not fin and r["cov_dist"] == 1.0 and r["cov_angle"] == 1.0
        return
    assert len(fin) == (COV_CASES[kind] if kind != "clamped" else len(inl))
    wd = ind.median_scale([t[0] for t in terms])
    wa = ind.median_scale([t[2] for t in terms])
    if kind == "clamped" and local is None:   # (with a localTransform the reference's formula compares two different frames)
        assert wd == 1e-4 and r["cov_dist"] == 1e-4 and wa == 1e-4
    assert abs(r["cov_dist"] - wd) <= max(b[0] for b in bounds) + 4 * EPS32 * wd
    assert abs(math.cos(r["cov_angle"]) - math.cos(wa)) <= max(b[1] for b in bounds)
    if kind in ("odd", "even"):   # the rank matters here: the neighbours in sorted order lie farther away than the bound
        d = np.sort([t[0] for t in terms])
        assert d[(len(d) >> 1)] - d[(len(d) >> 1) - 1] > 4 * max(b[0] for b in bounds)


# ---- variance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 1500])
def test_variance(n):
    """Float32 sums in order: the mean carries n eps32 max|v|, each of the n squares (v - mean)^2 moves by 2 |v - mean| times
    that, and their sum carries n eps32 of itself: |var - var64| <= n eps32 (var64 + 2 max|v| mean|v - mean| n / (n - 1))."""
    v = np.random.default_rng(11).uniform(0, 2, n).astype(np.float32)
    got = float(pnp_ref.variance(v))
    want = ind.variance(v)
    if n < 2:
        assert got == 0.0 and want == 0.0
        return
    v64 = v.astype(np.float64)
    bound = n * EPS32 * (want + 2 * v64.max() * np.abs(v64 - v64.mean()).mean() * n / (n - 1))
    assert abs(got - want) <= bound, (got, want, bound)
    assert bound < want / 3          # n against n - 1 differ by var / n at least... at n = 2 by a factor 2


# ---- the scenes and checks tests/test_gpu_pnp_independent.py runs on the device, here on the restatement ---------------------
# The checks read result and hypothesis records only, so the same functions hold the restatement (below, no GPU) and the
# device. The seeds are chosen so that the restatement needs no exemption at the gate; the device is expected to need none too.
SIZES = [20, 63, 64, 65, 129, 200]     # the finish kernel strides points over 64 lanes
ITERATIONS = [1, 64, 300]
GATE_PX = 1e-3                         # a point this close to the gate may be decided either way
AXIS_ANGLES = [0.0, 0.5, math.pi - 1e-3, 3.1]
SEEDS = {("clean", 1): 301, ("clean", 64): 2364, ("clean", 300): 1600, ("noisy", 1): 401, ("noisy", 64): 2464, ("noisy", 300): 2700,
         ("axis", 0): 500}


def set_pose(st, k, R, t):
    """Job k of the store seen under (R, t) instead of its own pose: exact projections, rounded to float32 once."""
    n = st.count[2 * k]
    Xc = st.xyz[2 * k, :n].astype(np.float64) @ R.T + t
    st.kpts[2 * k + 1, :n] = np.c_[K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]].astype(np.float32)
    st.xyz[2 * k + 1, :n] = Xc.astype(np.float32)
    st.poses[k] = (R, t)


def device_store(kind, iterations=0):
    """"clean": no noise, no outliers; eight jobs of one hypothesis, six of 64, one of 300. "noisy": 0.5 px and 30 % outliers, six
    jobs (three of 300 hypotheses). "axis": clean, the poses turned about the optical axis by AXIS_ANGLES. Pairs are the identity, so compacted index =
    point index. Six float32 points can be a poorly conditioned subset, whose EPnP pose misses 1e-5 in t by a small factor
    (about one subset in 1 500 here): the clean seeds are those for which no subset of the restatement's does."""
    rng = np.random.default_rng(SEEDS[kind, iterations])
    if kind == "axis":
        st = Store(rng, [200] * len(AXIS_ANGLES), 200, outliers=0.0)
        for k, a in enumerate(AXIS_ANGLES):
            set_pose(st, k, ind.rot_mp([0, 0, a]), np.array([0.1, -0.05, 0.2]))
    else:
        sizes = {1: SIZES + [64, 129], 64: SIZES, 300: [65] if kind == "clean" else [20, 65, 129]}[iterations]
        sizes = sizes[:6] if kind == "noisy" else sizes
        st = Store(rng, sizes, 200, outliers=0.0 if kind == "clean" else 0.3, noise=0.0 if kind == "clean" else 0.5)
    jobs = [(2 * k, 2 * k + 1) for k in range(len(st.poses))]
    pairs, npairs = st.pairs_for(jobs, rng, shuffle=False)
    return st, jobs, pairs, npairs


def restatement_records(st, jobs, pairs, npairs, params, local=None):
    out = [pnp_ref.estimate(st.xyz[f, :st.count[f]], st.kpts[t, :st.count[t]], st.xyz[t, :st.count[t]], pairs[j, :npairs[j]], K,
                            local, params) for j, (f, t) in enumerate(jobs)]
    inl = np.full((len(jobs), st.cap), -1, np.int32)
    for j, o in enumerate(out):
        inl[j, :len(o[1])] = o[1]
    return np.array([o[0] for o in out]), inl, np.array([o[3] for o in out])


ORTHO = 2 * 8 * MEASURED["svd Vt Vt^T - I"] + 16 * EPS   # R = U V^T of two factors, each orthonormal to 8 x the measured figure


def check_clean_hypotheses(hy, st):
    """Every hypothesis of a noise-free job: a rotation (orthonormal, determinant +1) and the true pose to the EPnP tolerance
    of tests/test_pnp_restatement.py (1e-6 in R, 1e-5 in t: the float32 inputs set that floor)."""
    for j, (Rt, tt) in enumerate(st.poses):
        for i, h in enumerate(hy[j]):
            R = h["R"].reshape(3, 3)
            assert np.abs(R @ R.T - np.eye(3)).max() <= ORTHO and np.linalg.det(R) > 0.5, (j, i)
            assert np.abs(R - Rt).max() < 1e-6 and np.abs(h["t"] - tt).max() < 1e-5, (j, i, np.abs(R - Rt).max(), h["t"] - tt)


def check_counts(hy, st, gate=4.0):
    """Every count against the independent inlier count at the RANSAC gate (the norm against reprojection_error^2 = 4 px).
    Returns the (hypothesis, point) pairs within GATE_PX of the gate; a count may differ by those and by nothing else."""
    near_total = pairs_total = 0
    for j in range(len(st.poses)):
        n = st.count[2 * j]
        X, U = st.xyz[2 * j, :n], st.kpts[2 * j + 1, :n]
        for i, h in enumerate(hy[j]):
            if not np.isfinite(h["R"]).all() or not np.isfinite(h["t"]).all():
                assert h["count"] == 0, (j, i)
                continue
            R = h["R"].reshape(3, 3)
            assert np.abs(R @ R.T - np.eye(3)).max() <= ORTHO and np.linalg.det(R) > 0.5, (j, i)
            mask, margin = ind.inliers(R, h["t"], X, U, K, gate)
            near = margin < GATE_PX
            assert (mask & ~near).sum() <= h["count"] <= (mask | near).sum(), (j, i, h["count"], mask.sum())
            near_total += int(near.sum())
            pairs_total += n
    assert near_total <= 0.01 * pairs_total
    return near_total


def check_inlier_lists(recs, inl, hy, st):
    """One refine round, with a normal exit or a break on an unchanged set, returns the RANSAC set: the best hypothesis' inliers
    at the gate, in order."""
    near_total = 0
    for j in range(len(st.poses)):
        r = recs[j]
        assert r["status"] == 0 and r["refine_exit"] in (0, 2) and r["refine_solves"] == 1, (j, r)
        n = st.count[2 * j]
        h = hy[j][r["best_iteration"]]
        mask, margin = ind.inliers(h["R"].reshape(3, 3), h["t"], st.xyz[2 * j, :n], st.kpts[2 * j + 1, :n], K, 4.0)
        near = margin < GATE_PX
        got = inl[j, :r["num_inliers"]]
        assert np.all(np.diff(got) > 0) and np.all(inl[j, r["num_inliers"]:] == -1), j
        assert set(np.flatnonzero(mask & ~near)) <= set(got.tolist()) <= set(np.flatnonzero(mask | near)), j
        near_total += int(near.sum())
    assert near_total <= 0.01 * sum(st.count[::2])
    return near_total


def check_refined_poses(recs, inl, hy, st):
    """rvec / tvec against scipy's minimum over the returned list (one round, normal exit or unchanged set: the set the solve ran on), started
    from the best hypothesis; R against expm(rvec). The bounds are those of the CPU tests above."""
    for j in range(len(st.poses)):
        r = recs[j]
        assert r["status"] == 0 and r["refine_exit"] in (0, 2) and r["refine_solves"] == 1, (j, r)
        got = inl[j, :r["num_inliers"]]
        P, uv = st.xyz[2 * j, got], st.kpts[2 * j + 1, got]
        h = hy[j][r["best_iteration"]]
        best = ind.lm_minimum(np.r_[ind.log_rot(h["R"].reshape(3, 3)), h["t"]], P, uv, K)
        assert np.abs(r["rvec"] - best[:3]).max() <= 8 * MEASURED["refine rvec - minimum"], (j, r["rvec"], best)
        assert np.abs(r["tvec"] - best[3:]).max() <= 8 * MEASURED["refine tvec - minimum"], (j, r["tvec"], best)
        th = float(np.linalg.norm(r["rvec"]))
        assert np.abs(r["R"].reshape(3, 3) - ind.rot_mp(r["rvec"])).max() <= (4 * max(th, 1.0) + 8) * EPS, j


def check_true_poses(recs, st):
    for j, (Rt, tt) in enumerate(st.poses):
        r = recs[j]
        assert r["status"] == 0 and r["num_inliers"] == st.count[2 * j], (j, r)
        assert np.abs(r["R"].reshape(3, 3) - Rt).max() < 1e-6 and np.abs(r["tvec"] - tt).max() < 1e-5, (j, r)
        assert np.abs(ind.rot_mp(r["rvec"]) - Rt).max() < 1e-6, (j, r["rvec"])


def check_transform(r, lo):
    want = ind.transform(r["R"].reshape(3, 3), r["tvec"], lo)
    assert r["status"] == 0 and np.abs(r["transform"].reshape(3, 4) - want).max() <= ulps4(want), (r["transform"], want)


def params_for(iterations=300, rounds=1):
    return pnp_ref.pnp_params(min_inliers=6, refine_iterations=rounds, iterations=iterations)


@pytest.mark.parametrize("iterations", ITERATIONS)
def test_device_scenes_on_the_restatement(iterations):
    p = params_for(iterations)
    st, jobs, pairs, npairs = device_store("clean", iterations)
    check_clean_hypotheses(restatement_records(st, jobs, pairs, npairs, p)[2], st)
    st, jobs, pairs, npairs = device_store("noisy", iterations)
    recs, inl, hy = restatement_records(st, jobs, pairs, npairs, p)
    assert check_counts(hy, st) == 0
    if iterations == 300:
        assert check_inlier_lists(recs, inl, hy, st) == 0
        check_refined_poses(recs, inl, hy, st)


def test_device_axis_scenes_on_the_restatement():
    st, jobs, pairs, npairs = device_store("axis")
    check_true_poses(restatement_records(st, jobs, pairs, npairs, params_for())[0], st)


def test_zz_print_measured():
    """Not a check: the figures this run measured, for the table in DESIGN.md."""
    for k, v in SEEN.items():
        print(f"    {k!r}: {v:.1e},")
