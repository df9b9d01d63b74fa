"""The pose-graph optimiser restated in numpy, and the graphs the pgo tests share.

A literal transcription of the reference's HyperGraph / Edge / Vertex / computeEdgeSE3Gradient / runOptimize / runOptimizeRobust /
getConnectedGraph, vectorised over edges only: every scalar operation is written out in the order the device kernels use, so that
with contraction off the per-edge quantities agree bit for bit wherever no library call (sqrt, pow) is involved. The matrix is
dense, the solve is numpy.linalg.solve on the lower triangle mirrored (what SimplicialLDLT reads), both `coupling` readings are
here, and so is the host loop of runOptimizeRobust. include/sbm.h describes the same arithmetic in words."""
import numpy as np

REFERENCE, SYMMETRIC = 0, 1
TAU = 1e-5
THR = 10.0


# ---- rigid transforms as (R (E,3,3), t (E,3)), products summed left to right ---------------------------------------------------
def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def mul33(A, B):
    out = np.empty(np.broadcast_shapes(A.shape, B.shape))
    for i in range(3):
        for j in range(3):
            out[..., i, j] = _dot3(A[..., i, 0], A[..., i, 1], A[..., i, 2], B[..., 0, j], B[..., 1, j], B[..., 2, j])
    return out


def mul3v(A, v):
    out = np.empty(np.broadcast_shapes(A.shape[:-1], v.shape))
    for i in range(3):
        out[..., i] = _dot3(A[..., i, 0], A[..., i, 1], A[..., i, 2], v[..., 0], v[..., 1], v[..., 2])
    return out


def split(P):
    P = np.asarray(P, np.float64).reshape(-1, 3, 4)
    return P[:, :, :3].copy(), P[:, :, 3].copy()


def join(R, t):
    return np.concatenate([R, t[..., None]], axis=-1)


def inverse(R, t):
    Rt = np.swapaxes(R, -1, -2).copy()
    return Rt, -mul3v(Rt, t)


def compose(Ra, ta, Rb, tb):
    return mul33(Ra, Rb), mul3v(Ra, tb) + ta


def quat_from_matrix(m):
    """Eigen's Quaternion(Matrix3): (x, y, z, w), the trace-positive branch and the largest-diagonal branch."""
    E = m.shape[0]
    q = np.empty((E, 4))
    tr = (m[:, 0, 0] + m[:, 1, 1]) + m[:, 2, 2]
    for e in range(E):
        a = m[e]
        if tr[e] > 0:
            t = np.sqrt(tr[e] + 1.0)
            q[e, 3] = 0.5 * t
            t = 0.5 / t
            q[e, 0] = (a[2, 1] - a[1, 2]) * t
            q[e, 1] = (a[0, 2] - a[2, 0]) * t
            q[e, 2] = (a[1, 0] - a[0, 1]) * t
        else:
            i = 0
            if a[1, 1] > a[0, 0]:
                i = 1
            if a[2, 2] > a[i, i]:
                i = 2
            j = (i + 1) % 3
            k = (j + 1) % 3
            t = np.sqrt(a[i, i] - a[j, j] - a[k, k] + 1.0)
            q[e, i] = 0.5 * t
            t = 0.5 / t
            q[e, 3] = (a[k, j] - a[j, k]) * t
            q[e, j] = (a[j, i] + a[i, j]) * t
            q[e, k] = (a[k, i] + a[i, k]) * t
    return q, tr > 0


def edge_error(Rzi, tzi, Ri, ti, Rj, tj):
    """delta = (Z^-1 * Xi^-1) * Xj; e = (translation, vector of the normalised quaternion with w >= 0)."""
    Rii, tii = inverse(Ri, ti)
    R1, t1 = compose(Rzi, tzi, Rii, tii)
    Rd, td = compose(R1, t1, Rj, tj)
    q, _ = quat_from_matrix(Rd)
    n = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    q = q / n[:, None]
    q = np.where(q[:, 3:4] < 0, -q, q)
    return np.concatenate([td, q[:, :3]], axis=1)


def mat6_vec(M, v):
    out = np.zeros(v.shape)
    for i in range(6):
        s = M[:, i, 0] * v[:, 0]
        for j in range(1, 6):
            s = s + M[:, i, j] * v[:, j]
        out[:, i] = s
    return out


def dot6(a, b):
    s = a[:, 0] * b[:, 0]
    for j in range(1, 6):
        s = s + a[:, j] * b[:, j]
    return s


def matT_mat(A, B):
    """A^T B for stacks of 6x6, summed over the row index 0..5 in order."""
    out = np.empty(A.shape)
    for i in range(6):
        for j in range(6):
            s = A[:, 0, i] * B[:, 0, j]
            for r in range(1, 6):
                s = s + A[:, r, i] * B[:, r, j]
            out[:, i, j] = s
    return out


def mat_mat(A, B):
    out = np.empty(A.shape)
    for i in range(6):
        for j in range(6):
            s = A[:, i, 0] * B[:, 0, j]
            for r in range(1, 6):
                s = s + A[:, i, r] * B[:, r, j]
            out[:, i, j] = s
    return out


def edge_jacobians(Rz, tz, Ri, ti, Rj, tj, with_bound=False):
    """computeEdgeSE3Gradient as written: A = Z^-1, B = Xi^-1 Xj, E = A B, dq/dR through qw = sqrt(tr + 1) / 2 and 1 / pow(qw, 3).
    with_bound: also |dq| |M| for both rotation blocks (zero elsewhere), the scale on which a rounding difference in sqrt or pow
    shows: the sums dq M cancel heavily near 180 degrees."""
    E = Rz.shape[0]
    Ra, ta = inverse(Rz, tz)
    Rii, tii = inverse(Ri, ti)
    Rb, tb = compose(Rii, tii, Rj, tj)
    Re, _ = compose(Ra, ta, Rb, tb)
    tr = (Re[:, 0, 0] + Re[:, 1, 1]) + Re[:, 2, 2]
    S = np.sqrt(tr + 1.0) * 2
    qw = S * .25
    a1 = 1 / np.power(qw, 3.0)
    a2 = -0.03125 * (Re[:, 2, 1] - Re[:, 1, 2]) * a1
    a3 = 1 / qw
    a4 = 0.25 * a3
    a5 = -0.25 * a3
    a6 = 0.03125 * (Re[:, 2, 0] - Re[:, 0, 2]) * a1
    a7 = -0.03125 * (Re[:, 1, 0] - Re[:, 0, 1]) * a1
    z = np.zeros(E)
    dq = np.stack([np.stack([a2, z, z, z, a2, a4, z, a5, a2], 1), np.stack([a6, z, a5, z, a6, z, a4, z, a6], 1),
                   np.stack([a7, a4, z, a5, a7, z, z, z, a7], 1)], 1)          # (E, 3, 9)
    Ji = np.zeros((E, 6, 6))
    Jj = np.zeros((E, 6, 6))
    Ji[:, :3, :3] = -Ra
    Jj[:, :3, :3] = Re
    x, y, zz = 2 * tb[:, 0], 2 * tb[:, 1], 2 * tb[:, 2]
    Sk = np.zeros((E, 3, 3))
    Sk[:, 0, 1], Sk[:, 0, 2], Sk[:, 1, 0], Sk[:, 1, 2], Sk[:, 2, 0], Sk[:, 2, 1] = -zz, y, zz, -x, -y, x
    Ji[:, :3, 3:] = mul33(Ra, Sk)

    def skew2(R, transposed):
        r = 2 * R
        Sx, Sy, Sz = np.zeros((E, 3, 3)), np.zeros((E, 3, 3)), np.zeros((E, 3, 3))
        sg = 1.0 if transposed else -1.0
        Sx[:, 1, :], Sx[:, 2, :] = sg * r[:, 2, :], -sg * r[:, 1, :]
        Sy[:, 0, :], Sy[:, 2, :] = -sg * r[:, 2, :], sg * r[:, 0, :]
        Sz[:, 0, :], Sz[:, 1, :] = sg * r[:, 1, :], -sg * r[:, 0, :]
        return Sx, Sy, Sz

    def dq_times(L, Ss):
        M = np.empty((E, 9, 3))
        for c, Sc in enumerate(Ss):
            P = mul33(L, Sc)
            for cc in range(3):
                for r in range(3):
                    M[:, r + 3 * cc, c] = P[:, r, cc]      # a column-major 3x3 is one column of M
        out = np.empty((E, 3, 3))
        for i in range(3):
            for j in range(3):
                s = dq[:, i, 0] * M[:, 0, j]
                for k in range(1, 9):
                    s = s + dq[:, i, k] * M[:, k, j]
                out[:, i, j] = s
        return out, np.einsum("eik,ekj->eij", np.abs(dq), np.abs(M))

    Ji[:, 3:, 3:], ai = dq_times(Ra, skew2(Rb, True))
    Jj[:, 3:, 3:], aj = dq_times(Re, skew2(np.broadcast_to(np.eye(3), (E, 3, 3)), False))
    if with_bound:
        Bi, Bj = np.zeros((E, 6, 6)), np.zeros((E, 6, 6))
        Bi[:, 3:, 3:], Bj[:, 3:, 3:] = ai, aj
        return Ji, Jj, Bi, Bj
    return Ji, Jj


def rotation_from_compact(v):
    """fromCompactQuaternion: the identity when 1 - |v|^2 < 0, else Quaternion(sqrt(w), v).toRotationMatrix()."""
    n = v.shape[0]
    w = 1 - ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    ident = w < 0
    w = np.sqrt(np.where(ident, 0.0, w))
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty((n, 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - (tyy + tzz), txy - twz, txz + twy
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = txy + twz, 1 - (txx + tzz), tyz - twx
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = txz - twy, tyz + twx, 1 - (txx + tyy)
    R[ident] = np.eye(3)
    return R, ident


# ---- the graph ------------------------------------------------------------------------------------------------------------------
class Graph:
    """ids (n,) ascending, poses (n, 3, 4), frm / to (E,) vertex ids, meas (E, 3, 4), info (E, 6, 6)."""

    def __init__(self, ids, poses, frm, to, meas, info, fixed_id=1, coupling=REFERENCE):
        order = np.argsort(np.asarray(ids, np.int64), kind="stable")
        self.ids = np.asarray(ids, np.int64)[order]
        self.poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)[order].copy()
        self.frm, self.to = np.asarray(frm, np.int64), np.asarray(to, np.int64)
        self.meas = np.asarray(meas, np.float64).reshape(-1, 3, 4)
        self.info = np.asarray(info, np.float64).reshape(-1, 6, 6)
        self.fixed_id, self.coupling = fixed_id, coupling
        pos = {int(v): k for k, v in enumerate(self.ids)}
        self.vi = np.array([pos[int(v)] for v in self.frm], np.int64)
        self.vj = np.array([pos[int(v)] for v in self.to], np.int64)
        self.hidx = np.full(len(self.ids), -1, np.int64)      # Hessian index: ascending id, the fixed vertex left out
        free = self.ids != fixed_id
        self.hidx[free] = np.arange(free.sum())
        self.nfree = int(free.sum())

    def couples(self):
        """Per edge: does it contribute an off-diagonal block (both ends free; under REFERENCE only when `to` has the larger
        Hessian index, the lower triangle SimplicialLDLT reads)."""
        hi, hj = self.hidx[self.vi], self.hidx[self.vj]
        both = (hi >= 0) & (hj >= 0)
        return both & (hj > hi) if self.coupling == REFERENCE else both

    def errors(self):
        Rz, tz = split(self.meas)
        Rzi, tzi = inverse(Rz, tz)
        R, t = split(self.poses)
        e = edge_error(Rzi, tzi, R[self.vi], t[self.vi], R[self.vj], t[self.vj])
        chi = dot6(e, mat6_vec(self.info, e))
        return e, chi

    def linearise(self):
        """Per edge: error, chi2, Ji, Jj, the blocks m_ii = Ji^T O Ji, m_jj, m_ij = Ji^T O Jj and the vectors Ji^T(-Oe), Jj^T(-Oe)."""
        e, chi = self.errors()
        Rz, tz = split(self.meas)
        R, t = split(self.poses)
        Ji, Jj = edge_jacobians(Rz, tz, R[self.vi], t[self.vi], R[self.vj], t[self.vj])
        we = -mat6_vec(self.info, e)
        bi = mat6_vec(np.swapaxes(Ji, 1, 2), we)
        bj = mat6_vec(np.swapaxes(Jj, 1, 2), we)
        JiO, JjO = matT_mat(Ji, self.info), matT_mat(Jj, self.info)
        return dict(e=e, chi=chi, Ji=Ji, Jj=Jj, bi=bi, bj=bj, mii=mat_mat(JiO, Ji), mjj=mat_mat(JjO, Jj), mij=mat_mat(JiO, Jj))

    def build(self, lin):
        """The lower triangle of A (dense, the upper left zero), b, and max_diag as the LAST edge leaves it."""
        n6 = 6 * self.nfree
        A, b = np.zeros((n6, n6)), np.zeros(n6)
        hi, hj = self.hidx[self.vi], self.hidx[self.vj]
        cp = self.couples()
        max_diag = 0.0
        for k in range(len(self.frm)):
            max_diag = 0.0
            for h, bb, m in ((hi[k], lin["bi"][k], lin["mii"][k]), (hj[k], lin["bj"][k], lin["mjj"][k])):
                if h < 0:
                    continue
                b[6 * h:6 * h + 6] += bb
                A[6 * h:6 * h + 6, 6 * h:6 * h + 6] += m.T        # triplet (h6 + j, h6 + i, m(i, j))
                max_diag = max(max_diag, float(np.abs(np.diag(m)).max()))
            if cp[k]:
                r, c, m = hj[k], hi[k], lin["mij"][k].T             # block (to, from) = m^T
                if r < c:                                          # SYMMETRIC: mirrored into the lower triangle
                    r, c, m = c, r, m.T
                A[6 * r:6 * r + 6, 6 * c:6 * c + 6] += m
        return np.tril(A), b, max_diag

    def apply(self, x):
        R, t = split(self.poses)
        free = np.flatnonzero(self.hidx >= 0)
        xs = x.reshape(-1, 6)
        Rinc, ident = rotation_from_compact(xs[:, 3:])
        Rn, tn = compose(R[free], t[free], Rinc, xs[:, :3].copy())
        self.poses[free] = join(Rn, tn)
        return ident


def solve_lower(A, b, lam):
    """(A + lam I) x = b with A's lower triangle mirrored."""
    S = A + np.tril(A, -1).T + lam * np.eye(len(b))
    return np.linalg.solve(S, b)


def scale_lambda(dot, chi_before, chi_after):
    rho = (chi_before - chi_after) / (dot + 1e-3)
    alpha = 1. - (2 * rho - 1) ** 3
    alpha = min(alpha, 2. / 3.)
    return max(1. / 3., alpha)


def optimize(g, num, trace=None):
    """HyperGraph::optimize: num iterations on g.poses in place; returns the final chi2. trace (a dict) receives per-iteration
    lists 'lam', 'chi' and the last iteration's A, b, x, lin, and whether any update took oplus' identity branch."""
    lam = 0.0
    tr = dict(lam=[], chi=[], identity=False) if trace is None else trace
    tr.setdefault("lam", []), tr.setdefault("chi", []), tr.setdefault("identity", False)
    for it in range(num):
        if g.nfree == 0:
            break
        lin = g.linearise()
        chi = float(np.sum(lin["chi"]))
        A, b, max_diag = g.build(lin)
        if it == 0:
            lam = TAU * max_diag
        x = solve_lower(A, b, lam)
        tr["lam"].append(lam), tr["chi"].append(chi)
        tr.update(A=A, b=b, x=x, lin=lin)
        ident = bool(g.apply(x).any())                     # every iteration applies its update, whatever the earlier ones took
        tr.setdefault("ident_its", []).append(ident)
        tr["identity"] = bool(tr["identity"] or ident)
        dot = float(np.sum(x * (lam * x + b)))
        lam *= scale_lambda(dot, chi, float(np.sum(g.errors()[1])))
    return float(np.sum(g.errors()[1]))


def run_optimize(ids, poses, frm, to, meas, info, num, fixed_id=1, coupling=REFERENCE, trace=None):
    g = Graph(ids, poses, frm, to, meas, info, fixed_id, coupling)
    err = optimize(g, num, trace)
    return err, g.ids, g.poses


def connected_graph(from_id, ids, poses, frm, to, meas):
    """getConnectedGraph as written, on links in the caller's multimap order (keyed by `from`). Returns the reached ids
    (ascending), their propagated poses, and the indices of the kept links in the order the out-multimap holds them (by `from`,
    insertion order among equals). Propagation is in double: pose[to] = pose[cur] * T or * T^-1."""
    ids = [int(v) for v in ids]
    P = {v: np.asarray(poses[k], np.float64).reshape(3, 4) for k, v in enumerate(ids)}
    bi = {}
    for k in range(len(frm)):
        bi.setdefault(int(frm[k]), []).append(int(to[k]))
        bi.setdefault(int(to[k]), []).append(int(frm[k]))

    def find(cands, a, b):
        for k in cands:
            if frm[k] == a and to[k] == b:
                return k
        for k in cands:
            if frm[k] == b and to[k] == a:
                return k
        return -1

    all_links = list(range(len(frm)))
    out, kept, pending = {}, [], {from_id}
    while pending:
        cur = max(pending)
        pending.discard(cur)
        if not out:
            out[cur] = P[cur]
        for nb in bi.get(cur, []):
            k = find(all_links, cur, nb)
            if nb in pending:
                continue
            if nb not in out:
                Rc, tc = split(out[cur])
                Rm, tm = split(meas[k])
                if frm[k] != cur:
                    Rm, tm = inverse(Rm, tm)
                Rn, tn = compose(Rc, tc, Rm, tm)
                out[nb] = join(Rn, tn)[0]
                pending.add(nb)
            if find(kept, cur, nb) < 0:
                kept.append(k)
    kept = sorted(kept, key=lambda k: int(frm[k]))          # stable: insertion order among equal keys
    oid = sorted(out)
    return np.array(oid, np.int64), np.stack([out[v] for v in oid]), np.array(kept, np.int64)


def run_optimize_robust(ids, poses, frm, to, meas, info, num, fixed_id=1, coupling=REFERENCE, rounds=None):
    """runOptimizeRobust. Returns (err, ids, poses, removed) with removed the (from, to) pairs in the order they were dropped.
    rounds (a list) receives one (from, to, chi2) triple of arrays per round: every link of that round's graph after its five
    iterations, the numbers the round decides on."""
    frm, to = np.asarray(frm, np.int64), np.asarray(to, np.int64)
    meas, info = np.asarray(meas, np.float64).reshape(-1, 3, 4), np.asarray(info, np.float64).reshape(-1, 6, 6)
    alive = np.arange(len(frm))
    removed = []
    while True:
        oid, oposes, kept = connected_graph(fixed_id, ids, poses, frm[alive], to[alive], meas[alive])
        sel = alive[kept]
        g = Graph(oid, oposes, frm[sel], to[sel], meas[sel], info[sel], fixed_id, coupling)
        optimize(g, 5)
        chi = g.errors()[1]
        if rounds is not None:
            rounds.append((frm[sel].copy(), to[sel].copy(), chi.copy()))
        worst, werr = -1, 0.0
        for k in range(len(sel)):
            a, b = int(frm[sel[k]]), int(to[sel[k]])
            if a != b + 1 and b != a + 1 and chi[k] >= THR and chi[k] > werr:
                worst, werr = k, float(chi[k])
        if worst < 0:
            err, rid, rposes = run_optimize(oid, oposes, frm[sel], to[sel], meas[sel], info[sel], num, fixed_id, coupling)
            return err, rid, rposes, removed
        a, b = int(frm[sel[worst]]), int(to[sel[worst]])
        removed.append((a, b))
        alive = np.array([k for k in sel if not (frm[k] == a and to[k] == b)], np.int64)


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def pose(R=None, t=(0, 0, 0)):
    return np.concatenate([np.eye(3) if R is None else R, np.asarray(t, np.float64).reshape(3, 1)], axis=1)


def mul(a, b):
    A, B = np.vstack([a, [0, 0, 0, 1]]), np.vstack([b, [0, 0, 0, 1]])
    return (A @ B)[:3]


def inv(a):
    return np.linalg.inv(np.vstack([a, [0, 0, 0, 1]]))[:3]


def spd_info(seed):
    r = np.random.default_rng(seed)
    M = r.normal(size=(6, 6))
    return M @ M.T + 6 * np.eye(6)


def trajectory(n, seed, step=0.8, turn=4.0):
    """n poses, ids 1..n: a gently turning walk."""
    r = np.random.default_rng(seed)
    P = [pose()]
    for _ in range(n - 1):
        d = pose(rot(r.normal(size=3) + [0, 0, 3], turn * (0.5 + r.random())), [step, 0.05 * r.normal(), 0.02 * r.normal()])
        P.append(mul(P[-1], d))
    return np.arange(1, n + 1), np.stack(P)


def chain_graph(n, closures=(), seed=0, noise=2e-3, float_noise=False, outliers=(), info=None, perturb=0.0, odo_info=None):
    """A chain of n vertices (ids 1..n) whose odometry edges k -> k+1 measure the true motion plus noise, plus closure edges
    (from, to) measuring the true relative pose plus noise; closures listed in `outliers` measure something grossly wrong. The
    initial poses are the odometry integrated. Links are in multimap order (by `from`, stable)."""
    r = np.random.default_rng(seed + 1000)
    ids, T = trajectory(n, seed)
    links = [(k, k + 1) for k in range(1, n)] + list(closures)
    meas = []
    for a, b in links:
        d = mul(inv(T[a - 1]), T[b - 1])
        if (a, b) in outliers:
            d = mul(d, pose(rot([0.3, 1, 0.2], 25.0), [3.0, -2.0, 1.0]))
        else:
            d = mul(d, pose(rot(r.normal(size=3), noise * 57.3 * r.normal()), noise * r.normal(size=3)))
        if float_noise:
            d = d.astype(np.float32).astype(np.float64)
        meas.append(d)
    order = sorted(range(len(links)), key=lambda k: links[k][0])
    links = [links[k] for k in order]
    meas = np.stack([meas[k] for k in order])
    P = [pose()]
    od = {a: m for (a, b), m in zip(links, meas) if b == a + 1}
    for k in range(1, n):
        P.append(mul(P[-1], od[k]))
    if perturb:                       # the initial poses off the odometry, so that a chain has something to solve
        P = [P[0]] + [mul(p, pose(rot(r.normal(size=3), perturb * 57.3), perturb * r.normal(size=3))) for p in P[1:]]
    frm, to = np.array([a for a, _ in links]), np.array([b for _, b in links])
    O = np.broadcast_to(np.eye(6) if info is None else info, (len(links), 6, 6)).copy()
    if odo_info is not None:
        O[to == frm + 1] = odo_info
    return dict(ids=ids, poses=np.stack(P), frm=frm, to=to, meas=meas, info=O)


def args(c):
    return c["ids"], c["poses"], c["frm"], c["to"], c["meas"], c["info"]


def fixed(c):
    """The fixed vertex a graph asks for: its own `fixed_id` where it carries one, else 1."""
    return int(c.get("fixed_id", 1))


# ---- builders over a graph: each returns a new graph with its links in multimap order (by `from`, stable) ----------------------
def _with_links(c, frm, to, meas, info):
    frm, to = np.asarray(frm, np.int64), np.asarray(to, np.int64)
    order = np.argsort(frm, kind="stable")
    out = dict(c, ids=np.array(c["ids"]), poses=np.array(c["poses"]), frm=frm[order], to=to[order],
               meas=np.asarray(meas, np.float64)[order].copy(), info=np.asarray(info, np.float64)[order].copy())
    return out


def _inverse_meas(meas):
    return join(*inverse(*split(meas)))


def bidirectional(c):
    """Every link also reversed, with the inverse measurement and the same information, as the reference's mapper stores them
    (link_forward and link_reverse of the odometry path; addLink's inverse at the other node)."""
    return _with_links(c, np.concatenate([c["frm"], c["to"]]), np.concatenate([c["to"], c["frm"]]),
                       np.concatenate([c["meas"], _inverse_meas(c["meas"])]), np.concatenate([c["info"], c["info"]]))


def reverse(c, which):
    """The links chosen by the boolean mask `which` turned round, their measurements inverted."""
    which = np.asarray(which, bool)
    meas = np.array(c["meas"], np.float64)
    meas[which] = _inverse_meas(meas[which])
    return _with_links(c, np.where(which, c["to"], c["frm"]), np.where(which, c["frm"], c["to"]), meas, c["info"])


def relabel(c, f):
    """Ids mapped through f, which must be strictly increasing and keep 1 (the order of vertices and links stays)."""
    new = np.array([f(int(v)) for v in c["ids"]], np.int64)
    assert f(1) == 1 and (np.diff(new[np.argsort(c["ids"])]) > 0).all()
    m = dict(zip((int(v) for v in c["ids"]), new.tolist()))
    out = _with_links(c, [m[int(v)] for v in c["frm"]], [m[int(v)] for v in c["to"]], c["meas"], c["info"])
    out["ids"] = new
    if "fixed_id" in c:
        out["fixed_id"] = m[int(c["fixed_id"])]
    return out


def gapped(v):
    """The id map of the gapped forms: 1..3 stay, then every group of three ids starts 2 further on (4 5 6 -> 6 7 8,
    7 8 9 -> 11 12 13, ...), so that every third odometry link joins ids that are not neighbours: a sub-diagonal block for the
    plan, a removable loop closure for the robust loop's id rule."""
    return v + 2 * ((v - 1) // 3)


def with_outliers(c, sizes):
    """The links (from, to) of `sizes` measure something wrong by a chosen size s: 25 s degrees and s (3, -2, 1) off."""
    meas = np.array(c["meas"], np.float64)
    for (a, b), s in sizes.items():
        k = np.flatnonzero((c["frm"] == a) & (c["to"] == b))
        assert len(k) == 1
        meas[k[0]] = mul(meas[k[0]], pose(rot([0.3, 1, 0.2], 25.0 * s), s * np.array([3.0, -2.0, 1.0])))
    return dict(c, meas=meas)


def edge_cases():
    """Single edges 1 -> 2 with a chosen error rotation: identity; 1, 90 and 179 degrees (both branches of Quaternion(R)); an
    error whose quaternion has w < 0 before the flip; each with a non-diagonal SPD information matrix. One graph, one edge each,
    gathered into one graph of disjoint pairs so one launch sees them all (vertex 1 is fixed, the rest are free)."""
    errs = [pose(), pose(rot([1, 2, 3], 1.0), [0.1, -0.2, 0.3]), pose(rot([0, 0, 1], 90.0), [1, 0, 0]),
            pose(rot([1, 0.2, -0.1], 179.0), [0, 0.5, 0]), pose(rot([0, 1, 0], 179.0)), pose(rot([0.1, 0.2, 1], 179.0)),
            pose(rot([1, 1, 0], 120.0), [0.3, 0.3, 0.3]), pose(rot([0, 0, 1], 181.0)), pose(rot([2, -1, 0.5], 200.0), [1, 2, 3])]
    ids, poses, frm, to, meas, info = [], [], [], [], [], []
    base = pose(rot([0.2, -0.4, 1], 33.0), [1.5, -0.5, 0.25])
    for k, E in enumerate(errs):
        a, b = 2 * k + 1, 2 * k + 2
        Z = pose(rot([1, -1, 0.5], 12.0 * (k + 1)), [0.4, 0.1 * k, -0.2])
        Xi = mul(base, pose(rot([0, 1, 1], 7.0 * k), [k, 0, 0]))
        ids += [a, b]
        poses += [Xi, mul(mul(Xi, Z), E)]
        frm.append(a), to.append(b), meas.append(Z), info.append(spd_info(k))
    return dict(ids=np.array(ids), poses=np.stack(poses), frm=np.array(frm), to=np.array(to), meas=np.stack(meas),
                info=np.stack(info))


def shape_cases(run_max=4):
    """name -> graph: the shapes that hit each elimination path."""
    out = {"pair": chain_graph(2, seed=1, perturb=2e-2)}
    for n in (3, max(run_max - 1, 1), run_max, run_max + 1, 2 * run_max + 1):   # a chain has an edge: run_max 1 has no chain0
        out[f"chain{n}"] = chain_graph(n + 1, seed=10 + n, noise=2e-2, perturb=2e-2)
    out["ring8_new_old"] = chain_graph(8, [(8, 2)], seed=3, noise=2e-2)
    out["ring8_old_new"] = chain_graph(8, [(2, 8)], seed=3, noise=2e-2)
    out["closure_to_fixed"] = chain_graph(7, [(6, 1)], seed=4, noise=2e-2)
    out["closure_from_fixed"] = chain_graph(7, [(1, 6)], seed=4, noise=2e-2)
    out["shared_vertex"] = chain_graph(12, [(9, 3), (11, 3)], seed=5, noise=2e-2)
    out["star5"] = chain_graph(14, [(4, 7), (9, 7), (11, 7), (13, 7)], seed=6, noise=2e-2)
    out["double_link"] = chain_graph(6, [(2, 3), (5, 2), (5, 2)], seed=8, noise=2e-2)
    for n in (65, 257):
        out[f"fan{n}"] = chain_graph(n + 1, [(k, 2) for k in range(4, n + 2)][:n - 2], seed=7, noise=1e-2)
    # the shapes the reference's mapper hands over: links from the larger id to the smaller, both directions, ids with gaps,
    # and a fixed vertex that is not the smallest id. 8 to 16 vertices each, whatever run_max is.
    c = chain_graph(10, seed=71, noise=2e-2, perturb=2e-2)
    # REFERENCE: no slot, no junction, a block-diagonal system. reversed_chain keeps the link at the fixed vertex as 1 -> 2, as
    # getConnectedGraph's walk from vertex 1 always meets it, and is recorded; reversed_chain_all turns that one round too, a
    # free `from` with a fixed `to`, on which the reference forms a negative triplet index and Eigen asserts: restatement alone.
    out["reversed_chain"] = reverse(c, c["frm"] != 1)
    out["reversed_chain_all"] = reverse(c, np.ones(len(c["frm"]), bool))
    c = bidirectional(chain_graph(9, seed=72, noise=2e-2, perturb=2e-2))
    keep = c["to"] != 1                                   # the same split: without the link 2 -> 1 the reference runs it
    out["bidir_chain"] = dict(c, frm=c["frm"][keep], to=c["to"][keep], meas=c["meas"][keep], info=c["info"][keep])
    out["bidir_chain_all"] = c
    out["opposite_pair"] = chain_graph(8, [(2, 5), (5, 2)], seed=73, noise=2e-2)  # SYMMETRIC: m and m^T into the slot of (2, 5)
    out["gaps"] = relabel(chain_graph(10, [(8, 3)], seed=74, noise=2e-2), gapped)
    # the reference cannot run these two: with a fixed vertex that is not the smallest id it forms a negative triplet index and
    # Eigen asserts. They are held to the restatement alone.
    out["fixed_mid"] = dict(chain_graph(11, [(3, 9), (10, 2)], seed=75, noise=2e-2), fixed_id=6)
    out["fixed_last"] = dict(chain_graph(11, [(11, 4), (2, 8)], seed=76, noise=2e-2), fixed_id=11)
    return out


def iteration_case():
    return chain_graph(40, [(30, 5), (38, 12), (25, 14)], seed=21, noise=3e-3, float_noise=True)


def robust_case():
    good = [(4, 25), (11, 37), (20, 48), (33, 58)]
    bad = (27, 41)
    return chain_graph(60, good + [bad], seed=31, noise=1e-3, outliers={bad}, info=100.0 * np.eye(6), odo_info=1e4 * np.eye(6))


MULTI_GOOD = [(37, 19), (21, 34), (40, 2), (27, 13)]
MULTI_BAD = {(14, 36): 1.0, (20, 11): 0.7, (10, 44): 0.3}


def multi_outlier_case():
    """48 vertices, four good closures and three outliers of sizes 1, 0.7 and 0.3, closures in both directions of id. Seed and
    sizes are chosen so that in this form, in bidirectional(), in relabel(, gapped) and in both together every round of the
    robust loop decides by a factor of two (test_pgo_restatement.py checks that, on the reference's numbers too)."""
    c = chain_graph(48, MULTI_GOOD + list(MULTI_BAD), seed=893, noise=1e-3, info=100.0 * np.eye(6), odo_info=1e4 * np.eye(6))
    return with_outliers(c, MULTI_BAD)


def first_round(c, from_id=1):
    """The graph the robust loop's first round optimises: what getConnectedGraph reaches from from_id, one link per vertex
    pair in the direction its walk met first, the poses propagated along the links."""
    oid, op, kept = connected_graph(from_id, c["ids"], c["poses"], c["frm"], c["to"], c["meas"])
    return dict(ids=oid, poses=op, frm=c["frm"][kept], to=c["to"][kept], meas=c["meas"][kept], info=c["info"][kept])


IDENTITY_NUM = 6


def identity_case():
    """A plain (non-robust) graph whose FIRST update takes oplus' identity branch (|v| > 1 at some vertex) and which is then
    iterated five times more: 16 vertices, every link in both directions, one closure (15, 2) wrong by 75 degrees and 10 units,
    as the robust loop's first round sees it. Under the REFERENCE reading half the couplings are missing, the iteration does not
    converge and chi2 keeps moving between 2.7e5 and 9.5e5."""
    c = chain_graph(16, [(15, 2)], seed=81, noise=1e-3, info=100.0 * np.eye(6), odo_info=1e4 * np.eye(6))
    return first_round(bidirectional(with_outliers(c, {(15, 2): 3.0})))


def round_margins(rounds):
    """Per robust round (from, to, chi2): (the two largest chi2 among the links the id rule lets the loop remove, largest
    first; 0 where there is none). A round removes when the largest reaches THR."""
    out = []
    for frm, to, chi in rounds:
        cand = np.sort(np.asarray(chi, np.float64)[np.abs(np.asarray(frm, np.int64) - np.asarray(to, np.int64)) != 1])[::-1]
        out.append(tuple(np.concatenate([cand[:2], np.zeros(2)])[:2].tolist()))
    return out


def decided_by_a_factor_of_two(rounds):
    """Every removing round's winner is at least 2 THR and twice the runner-up; the stopping round's candidates are at most
    THR / 2; the last round and no other is the stopping one."""
    m = round_margins(rounds)
    removing = all(w >= 2 * THR and w >= 2 * r for w, r in m[:-1])
    return bool(removing and m[-1][0] <= THR / 2)


def unreachable_case():
    """Vertex 9 has no link: it drops out."""
    c = chain_graph(8, [(7, 2)], seed=41, noise=1e-3)
    c["ids"] = np.append(c["ids"], 9)
    c["poses"] = np.concatenate([c["poses"], pose(t=(9, 9, 9))[None]])
    return c


def recorded_cases():
    """name -> (graph, num, coupling is REFERENCE there) for tools/make_pgo_fixtures.py and the restatement test."""
    out = {"iter40": (iteration_case(), 5, False), "ring8_new_old": (shape_cases()["ring8_new_old"], 3, False),
           "ring8_old_new": (shape_cases()["ring8_old_new"], 3, False), "edges": (edge_cases(), 0, False),
           "robust60": (robust_case(), 20, True), "unreachable": (unreachable_case(), 4, True)}
    assert tuple(out) == ORIGINAL_CASES
    # graphs shaped as the reference's mapper builds them; each is held to its own measured difference (name/E in the file)
    m, sh = multi_outlier_case(), shape_cases()
    out.update({"robust60_bidir": (bidirectional(robust_case()), 20, True), "multi48": (m, 20, True),
                "multi48_bidir": (bidirectional(m), 20, True), "multi48_gaps": (relabel(m, gapped), 20, True),
                "multi48_bidir_gaps": (relabel(bidirectional(m), gapped), 20, True),
                "identity16": (identity_case(), IDENTITY_NUM, False), "reversed_chain": (sh["reversed_chain"], 3, False),
                "bidir_chain": (sh["bidir_chain"], 3, False), "opposite_pair": (sh["opposite_pair"], 3, False)})
    return out


ORIGINAL_CASES = ("iter40", "ring8_new_old", "ring8_old_new", "edges", "robust60", "unreachable")   # meta/E0 is measured on these
ROBUST_CASES = ("robust60", "robust60_bidir", "multi48", "multi48_bidir", "multi48_gaps", "multi48_bidir_gaps")


def tolerance(rec, name, factor):
    """factor * E0 for the six original cases, factor * max(E0, the case's own measured E) for every later one."""
    e0 = float(rec["meta/E0"])
    return factor * (e0 if name in ORIGINAL_CASES else max(e0, float(rec[f"{name}/E"])))


# ---- comparison with the recording (tests/test_pgo_restatement.py, tools/make_pgo_fixtures.py) --------------------------------------
def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def restated(c, num, robust, coupling=REFERENCE):
    """What the restatement gives for one recorded case, in the shape tools/make_pgo_fixtures.py records."""
    if robust:
        err, ids, poses, removed = run_optimize_robust(*args(c), num, coupling=coupling)
        return dict(lam=np.zeros(0), chi=np.zeros(0), out_ids=ids, out_poses=poses, err=err,
                    removed=np.array(removed, np.int64).reshape(-1, 2))
    tr = {}
    err, ids, poses = run_optimize(*args(c), num, coupling=coupling, trace=tr)
    return dict(lam=np.array(tr["lam"]), chi=np.array(tr["chi"]), out_ids=ids, out_poses=poses, err=err,
                removed=np.zeros((0, 2), np.int64), edgechi=Graph(*args(c)).errors()[1])


def difference(rec, got, robust):
    """Largest relative difference of one case: lambda, chi2 and the return value entry by entry, the poses by their scale."""
    d = [rel(got["err"], rec["err"]), float(np.abs(got["out_poses"] - rec["out_poses"]).max() / np.abs(rec["out_poses"]).max())]
    if not robust:
        d += [rel(got["lam"], rec["lam"]), rel(got["chi"], rec["chi"]),
              float(np.abs(got["edgechi"] - rec["edgechi"]).max() / max(np.abs(rec["edgechi"]).max(), 1e-300))]
    return max(d)
