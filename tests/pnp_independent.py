"""An independent statement of the motion-estimation arithmetic, written from the mathematical definitions in float64 numpy /
scipy and, where float64 is itself in doubt, mpmath at 50 digits. TEST INFRASTRUCTURE ONLY.

Nothing here follows u96-slam_amd/csrc/sbm_pnp_math.h: no shared operation order, no float32 staging, no closed-form Rodrigues.
The rotation is the matrix exponential of the skew matrix, every derivative is mpmath.diff of that definition, the solvers are
numpy.linalg's, the LM minimum is scipy's. The header and the device are held to this file by tests/test_pnp_math_independent.py
and tests/test_gpu_pnp_independent.py.

    skew(r), rot(r), rot_mp(r)                       R = expm([r]x): float64 through scipy, 50 digits through mpmath
    drot(r)                                          dR / dr_j, (3, 3, 3), mpmath.diff of expm
    log_rot(R)                                       the rotation vector of angle <= pi (at pi the sign of the axis is free)
    project(r_or_R, t, P, K)                         pinhole projection in pixels, (n, 2)
    residual(x, P, uv, K)                            projection - observation at x = (r, t), (n, 2)
    residual_jacobian(x, p, uv, K)                   e (2,) and de / d(r, t) (2, 6) of one point, mpmath.diff
    normal_equations(x, P, uv, K)                    J^T J (6, 6), J^T e (6,), e^T e, with J from mpmath.diff
    damped_step(JtJ, Jte, lam)                       solve(JtJ + lam diag(JtJ), Jte)
    lm_minimum(x0, P, uv, K)                         scipy least_squares(method="lm") at machine-precision tolerances
    svd(A), lstsq(A, b)                              numpy.linalg
    transform(R, t, local)                           inv(local @ [R t]) as 3 x 4 float64 (local None: inv([R t]))
    cov_terms(obj, to, T)                            squared distance, cosine and angle of the covariance terms
    variance(v)                                      var(ddof=1), 0 below two values
    median_scale(values)                             sorted[n >> 1], at least 1e-4; 1 when there is no value
    inliers(R, t, P, uv, K, thr)                     mask of float64 reprojection error <= thr, and each |error - thr|
"""
import mpmath as mp
import numpy as np
import scipy.linalg
import scipy.optimize

DPS = 50


def skew(r):
    x, y, z = (float(v) for v in r)
    return np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])


def _skew_mp(r):
    x, y, z = r
    return mp.matrix([[0, -z, y], [z, 0, -x], [-y, x, 0]])


def rot(r):
    return scipy.linalg.expm(skew(r))


def rot_mp(r):
    """expm([r]x) at 50 digits, rounded to float64 once. r: floats or mpf."""
    with mp.workdps(DPS):
        E = mp.expm(_skew_mp([mp.mpf(v) for v in r]))
        return np.array([[float(E[i, j]) for j in range(3)] for i in range(3)])


def _diff_all(f, x, nout):
    """d f_k / d x_j for a vector function of a vector, by mpmath.diff on every (k, j); f's values are shared between the
    outputs k (mpmath.diff evaluates each of them at the same abscissae)."""
    out = np.zeros((nout, len(x)))
    for j in range(len(x)):
        memo = {}

        def g(v, j=j, memo=memo):
            if v not in memo:
                y = list(x)
                y[j] = v
                memo[v] = f(y)
            return memo[v]

        for k in range(nout):
            out[k, j] = float(mp.diff(lambda v, k=k: g(v)[k], x[j]))
    return out


def drot(r):
    """dR / dr: out[j] = dR / dr_j (3 x 3)."""
    with mp.workdps(DPS):
        x = [mp.mpf(float(v)) for v in r]
        d = _diff_all(lambda y: list(mp.expm(_skew_mp(y))), x, 9)   # a matrix iterates row-major
        return d.T.reshape(3, 3, 3)


def log_rot(R):
    """The rotation vector of angle in [0, pi]: angle = atan2(|a|, (tr R - 1) / 2) with a the axial vector of (R - R^T) / 2
    (= sin(angle) n); the axis is the unit eigenvector of (R + R^T) / 2 (= cos I + (1 - cos) n n^T) for its largest eigenvalue,
    signed by a. At angle pi a vanishes and n, -n describe the same rotation: the eigenvector's own sign is returned."""
    R = np.asarray(R, float)
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.linalg.norm(a)), 0.5 * (np.trace(R) - 1.0)
    ang = float(np.arctan2(s, c))
    if ang == 0.0:
        return np.zeros(3)
    if c > 0.5:          # the symmetric part is close to I: the axial vector is the well-conditioned source
        return a / s * ang
    w, V = np.linalg.eigh(0.5 * (R + R.T))
    n = V[:, np.argmax(w)]
    if np.dot(n, a) < 0:
        n = -n
    return n * ang


def _project_mp(x, p, K):
    E = mp.expm(_skew_mp(x[:3]))
    X = [E[i, 0] * p[0] + E[i, 1] * p[1] + E[i, 2] * p[2] + x[3 + i] for i in range(3)]
    return [K[0] * X[0] / X[2] + K[2], K[1] * X[1] / X[2] + K[3]]


def project(rot_or_rvec, t, P, K):
    """Pixels of the points P (n, 3) under (R or r, t). A point with camera z exactly 0 is not divided (the reference's reading
    of cvProjectPoints2: z = Z ? 1 / Z : 1)."""
    A = np.asarray(rot_or_rvec, float)
    Rm = A if A.shape == (3, 3) else rot(A)
    X = np.asarray(P, np.float64).reshape(-1, 3) @ Rm.T + np.asarray(t, float)
    z = np.where(X[:, 2] != 0, X[:, 2], 1.0)
    return np.c_[K[0] * X[:, 0] / z + K[2], K[1] * X[:, 1] / z + K[3]]


def residual(x, P, uv, K):
    x = np.asarray(x, float)
    return project(x[:3], x[3:], P, K) - np.asarray(uv, np.float64).reshape(-1, 2)


def residual_jacobian(x, p, uv, K):
    """One point: e (2,) and J = de / d(r, t) (2, 6)."""
    with mp.workdps(DPS):
        xm = [mp.mpf(float(v)) for v in x]
        pm = [mp.mpf(float(v)) for v in p]
        Km = [mp.mpf(float(v)) for v in K]
        e = _project_mp(xm, pm, Km)
        J = _diff_all(lambda y: _project_mp(y, pm, Km), xm, 2)
        return np.array([float(e[0] - mp.mpf(float(uv[0]))), float(e[1] - mp.mpf(float(uv[1])))]), J


def normal_equations(x, P, uv, K):
    P, uv = np.asarray(P).reshape(-1, 3), np.asarray(uv).reshape(-1, 2)
    JtJ, Jte, ete = np.zeros((6, 6)), np.zeros(6), 0.0
    for p, m in zip(P, uv):
        e, J = residual_jacobian(x, p, m, K)
        JtJ += J.T @ J
        Jte += J.T @ e
        ete += float(e @ e)
    return JtJ, Jte, ete


def gradient(x, P, uv, K):
    """J^T e over many points, where mpmath.diff is too slow: J by central differences of the float64 residual (h = 1e-6:
    truncation about 1e-12, rounding about 1e-10 of J's scale)."""
    x = np.asarray(x, float)
    e = residual(x, P, uv, K).ravel()
    J = np.zeros((e.size, 6))
    for j in range(6):
        h = 1e-6 * max(1.0, abs(x[j]))
        a, b = x.copy(), x.copy()
        a[j] += h
        b[j] -= h
        J[:, j] = (residual(a, P, uv, K).ravel() - residual(b, P, uv, K).ravel()) / (2 * h)
    return J.T @ e


def damped_step(JtJ, Jte, lam):
    return np.linalg.solve(JtJ + lam * np.diag(np.diag(JtJ)), Jte)


def lm_minimum(x0, P, uv, K):
    """The minimum of the sum of squared residuals next to x0."""
    eps = np.finfo(float).eps
    r = scipy.optimize.least_squares(lambda x: residual(x, P, uv, K).ravel(), np.asarray(x0, float), jac="2-point", method="lm",
                                     xtol=4 * eps, ftol=4 * eps, gtol=4 * eps, max_nfev=4000)
    return r.x


def svd(A):
    return np.linalg.svd(np.asarray(A, float), full_matrices=False)


def lstsq(A, b):
    """The minimum-norm least-squares solution."""
    return np.linalg.lstsq(np.asarray(A, float), np.asarray(b, float), rcond=None)[0]


def _h(T):
    return np.vstack([np.asarray(T, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])


def transform(R, t, local=None):
    M = _h(np.c_[np.asarray(R, float).reshape(3, 3), np.asarray(t, float).reshape(3)])
    if local is not None:
        M = _h(local) @ M
    return np.linalg.inv(M)[:3]


def cov_terms(obj, to, T):
    """(squared distance of obj from T * to, cosine and angle between obj and T * to as seen from T's origin)."""
    T = np.asarray(T, np.float64).reshape(3, 4)
    obj, to = np.asarray(obj, np.float64), np.asarray(to, np.float64)
    new = T[:, :3] @ to + T[:, 3]
    v1, v2 = obj - T[:, 3], new - T[:, 3]
    cosang = float(np.clip(v1 @ v2 / (np.linalg.norm(v1) * np.linalg.norm(v2)), -1.0, 1.0))
    return float(np.sum((obj - new) ** 2)), cosang, float(np.arccos(cosang))


def variance(v):
    v = np.asarray(v, np.float64)
    return float(np.var(v, ddof=1)) if v.size > 1 else 0.0


def median_scale(values):
    v = np.sort(np.asarray(values, np.float64))
    return 1.0 if v.size == 0 else max(float(v[v.size >> 1]), 1e-4)


def inliers(rot_or_rvec, t, P, uv, K, thr):
    err = np.linalg.norm(project(rot_or_rvec, t, P, K) - np.asarray(uv, np.float64).reshape(-1, 2), axis=1)
    return err <= thr, np.abs(err - thr)
