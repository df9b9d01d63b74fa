"""The sequential CPU restatement of estimateMotion3DTo2D (oracle/libpnp_ref.so) through ctypes, and a literal
transcription of the reference's loops that the C file is held to. TEST INFRASTRUCTURE ONLY.

    estimate(xyz_from, kpts_to, xyz_to, pairs, K, local=None, params=None, hyp=True)
        -> (result record, inliers, RANSAC set, hypotheses or None, extra: {"matches", "xyz", "uv", "gate_margin"})
    draw(n, iterations) / draw_np(n, iterations)                             -> (iterations, 6) subsets
    replay(counts, n, conf) / replay_np(...)                                 -> (best iteration, niters, best count)
    refine_walk(ransac, sets, rounds, min_inliers) / refine_walk_np(...)     -> (final list, solves, exit)
    update_num_iters(p, ep, mp, max_iters)                                   -> RANSACUpdateNumIters
    epnp6(pw, uv, K) -> (R (3, 3), t (3,)); rodrigues(rvec) -> R; rodrigues_inv(R) -> rvec
    The header's blocks one by one (for tests/pnp_independent.py's comparisons): jacobi_svd(A) -> (U, W, Vt); svd_solve(A, b);
    qr_solve(A, b); rodrigues_d(rvec) -> (R, dRdr (3, 3, 3)); lm_points(R, dRdr, t, p, m, K, with_j) -> 28 accumulators;
    lm_step(acc, lam, prev); lm_converged(param, prev); reproj_err(R, t, p, m, K); variance(v); tf_mul(A, B); tf_inverse(A);
    transform(R, t, local); cov_terms(obj, to, T) -> (dist, angle)

The *_np functions transcribe CvSolvePnP.cpp (RNG::uniform, getSubset, RANSACPointSetRegistrator::run) and
MotionEstimation.cpp (solvePnPRansac's refine loop with its two std::swap calls) line by line in Python.
"""
import ctypes
import math
import pathlib
import sys

import numpy as np

import oracle_lib

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[0]))
from _pkg import load as _load_pkg  # noqa: E402

_pkg = _load_pkg()
PNP_RESULT_DTYPE, PNP_HYP_DTYPE, PnpParams, pnp_params = _pkg.PNP_RESULT_DTYPE, _pkg.PNP_HYP_DTYPE, _pkg.PnpParams, _pkg.pnp_params
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = oracle_lib.load("libpnp_ref.so")
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.pnp_ref_update_num_iters.argtypes = [cd, cd, ci, ci]
        L.pnp_ref_draw.argtypes = [ci, ci, vp]
        L.pnp_ref_draw.restype = None
        L.pnp_ref_epnp6.argtypes = [vp, vp, vp, vp, vp]
        L.pnp_ref_epnp6.restype = None
        L.pnp_ref_rodrigues.argtypes = [vp, vp]
        L.pnp_ref_rodrigues.restype = None
        L.pnp_ref_rodrigues_inv.argtypes = [vp, vp]
        L.pnp_ref_rodrigues_inv.restype = None
        L.pnp_ref_replay.argtypes = [vp, ci, ci, cd, vp, vp, vp]
        L.pnp_ref_replay.restype = None
        L.pnp_ref_refine_walk.argtypes = [vp, ci, vp, vp, ci, ci, ci, vp, vp, vp]
        L.pnp_ref_estimate.argtypes = [vp, ci, vp, vp, ci, vp, ci, vp, vp, ctypes.POINTER(PnpParams), vp, vp, vp, vp, vp, vp, vp, vp,
                                       vp]
        cf = ctypes.c_float
        for name, args, res in (("jacobi_svd", [vp, vp, vp, ci, ci], None), ("svd_solve", [vp, ci, ci, vp, vp], None),
                                ("qr_solve", [vp, vp, vp], None), ("rodrigues_d", [vp, vp, vp], None),
                                ("lm_points", [vp, vp, vp, vp, vp, ci, vp, ci, vp], None), ("lm_step", [vp, cd, vp, vp], None),
                                ("lm_converged", [vp, vp], ci), ("reproj_err", [vp, vp, vp, vp, vp], cf),
                                ("variance", [vp, ci], cf), ("tf_mul", [vp, vp, vp], None), ("tf_inverse", [vp, vp], None),
                                ("transform", [vp, vp, vp, vp], None), ("cov_terms", [vp, vp, vp, vp, vp], None), ("ld", [], ci)):
            f = getattr(L, "pnp_ref_" + name)
            f.argtypes, f.restype = args, res
        _LIB = L
    return _LIB


def _a(x, dt):
    return np.ascontiguousarray(np.asarray(x, dt))


# ---- the C restatement -------------------------------------------------------------------------------------------------
def update_num_iters(p, ep, model_points, max_iters):
    return lib().pnp_ref_update_num_iters(p, ep, model_points, max_iters)


def draw(n, iterations):
    out = np.zeros((iterations, 6), np.int32)
    lib().pnp_ref_draw(n, iterations, out.ctypes.data)
    return out


def epnp6(pw, uv, K):
    pw, uv, Kd = _a(pw, np.float32).reshape(6, 3), _a(uv, np.float32).reshape(6, 2), _a(K, np.float64)
    R, t = np.zeros(9), np.zeros(3)
    lib().pnp_ref_epnp6(pw.ctypes.data, uv.ctypes.data, Kd.ctypes.data, R.ctypes.data, t.ctypes.data)
    return R.reshape(3, 3), t


def rodrigues(rv):
    rv, R = _a(rv, np.float64), np.zeros(9)
    lib().pnp_ref_rodrigues(rv.ctypes.data, R.ctypes.data)
    return R.reshape(3, 3)


def rodrigues_inv(R):
    R, rv = _a(R, np.float64).reshape(9), np.zeros(3)
    lib().pnp_ref_rodrigues_inv(R.ctypes.data, rv.ctypes.data)
    return rv


def jacobi_svd(A):
    """pnp_jacobi_svd of A (m x n, m >= n) -> (U (m, n), W (n,), Vt (n, n)): the header takes A's columns as rows of stride LD."""
    A = _a(A, np.float64)
    m, n = A.shape
    ld = lib().pnp_ref_ld()
    At, Vt, W = np.zeros((ld, ld)), np.zeros((ld, ld)), np.zeros(ld)
    At[:n, :m] = A.T
    lib().pnp_ref_jacobi_svd(At.ctypes.data, W.ctypes.data, Vt.ctypes.data, m, n)
    return At[:n, :m].T.copy(), W[:n].copy(), Vt[:n, :n].copy()


def svd_solve(A, b):
    A, b = _a(A, np.float64), _a(b, np.float64)
    x = np.zeros(A.shape[1])
    lib().pnp_ref_svd_solve(A.ctypes.data, A.shape[0], A.shape[1], b.ctypes.data, x.ctypes.data)
    return x


def qr_solve(A, b, x0=None):
    """epnp::qr_solve on a 6 x 4 system (copies; the header overwrites A and b). x0: what X holds before the call."""
    A, b = _a(A, np.float64).reshape(6, 4).copy(), _a(b, np.float64).reshape(6).copy()
    x = np.zeros(4) if x0 is None else _a(x0, np.float64).copy()
    lib().pnp_ref_qr_solve(A.ctypes.data, b.ctypes.data, x.ctypes.data)
    return x


def rodrigues_d(rv):
    """(R (3, 3), dRdr (3, 3, 3): dRdr[j] = dR / dr_j)."""
    rv, R, d = _a(rv, np.float64), np.zeros(9), np.zeros(27)
    lib().pnp_ref_rodrigues_d(rv.ctypes.data, R.ctypes.data, d.ctypes.data)
    return R.reshape(3, 3), d.reshape(3, 3, 3)


def lm_points(R, dRdr, t, p, m, K, with_j=1):
    """The 28 accumulators of pnp_lm_point over the points p (n, 3) float32 and observations m (n, 2) float32, in order."""
    R, d, t, Kd = _a(R, np.float64).reshape(9), _a(dRdr, np.float64).reshape(27), _a(t, np.float64), _a(K, np.float64)
    p, m = _a(p, np.float32).reshape(-1, 3), _a(m, np.float32).reshape(-1, 2)
    acc = np.zeros(28)
    lib().pnp_ref_lm_points(R.ctypes.data, d.ctypes.data, t.ctypes.data, p.ctypes.data, m.ctypes.data, p.shape[0], Kd.ctypes.data,
                            int(with_j), acc.ctypes.data)
    return acc


def lm_step(acc, lam, prev):
    acc, prev, out = _a(acc, np.float64), _a(prev, np.float64), np.zeros(6)
    lib().pnp_ref_lm_step(acc.ctypes.data, float(lam), prev.ctypes.data, out.ctypes.data)
    return out


def lm_converged(param, prev):
    param, prev = _a(param, np.float64), _a(prev, np.float64)
    return bool(lib().pnp_ref_lm_converged(param.ctypes.data, prev.ctypes.data))


def reproj_err(R, t, p, m, K):
    R, t, Kd = _a(R, np.float64).reshape(9), _a(t, np.float64), _a(K, np.float64)
    p, m = _a(p, np.float32), _a(m, np.float32)
    return np.float32(lib().pnp_ref_reproj_err(R.ctypes.data, t.ctypes.data, p.ctypes.data, m.ctypes.data, Kd.ctypes.data))


def variance(v):
    v = _a(v, np.float32)
    return np.float32(lib().pnp_ref_variance(v.ctypes.data, v.size))


def tf_mul(A, B):
    A, B, C = _a(A, np.float32).reshape(12), _a(B, np.float32).reshape(12), np.zeros(12, np.float32)
    lib().pnp_ref_tf_mul(A.ctypes.data, B.ctypes.data, C.ctypes.data)
    return C.reshape(3, 4)


def tf_inverse(A):
    A, C = _a(A, np.float32).reshape(12), np.zeros(12, np.float32)
    lib().pnp_ref_tf_inverse(A.ctypes.data, C.ctypes.data)
    return C.reshape(3, 4)


def transform(R, t, local=None):
    R, t, out = _a(R, np.float64).reshape(9), _a(t, np.float64), np.zeros(12, np.float32)
    lo = None if local is None else _a(local, np.float32).reshape(12)
    lib().pnp_ref_transform(R.ctypes.data, t.ctypes.data, None if lo is None else lo.ctypes.data, out.ctypes.data)
    return out.reshape(3, 4)


def cov_terms(obj, to, T):
    obj, to, T = _a(obj, np.float32), _a(to, np.float32), _a(T, np.float32).reshape(12)
    out = np.zeros(2, np.float32)
    lib().pnp_ref_cov_terms(obj.ctypes.data, to.ctypes.data, T.ctypes.data, out.ctypes.data, out.ctypes.data + 4)
    return out[0], out[1]


def replay(counts, n, confidence=0.99):
    c = _a(counts, np.int32)
    out = np.zeros(3, np.int32)
    o = out.ctypes.data
    lib().pnp_ref_replay(c.ctypes.data, c.size, n, confidence, o, o + 4, o + 8)
    return int(out[0]), int(out[1]), int(out[2])


def refine_walk(ransac, sets, rounds, min_inliers):
    cap = max([len(ransac)] + [len(s) for s in sets] + [1])
    S = np.zeros((max(len(sets), 1), cap), np.int32)
    lens = np.zeros(max(len(sets), 1), np.int32)
    for r, s in enumerate(sets):
        S[r, :len(s)] = s
        lens[r] = len(s)
    ra = _a(ransac, np.int32) if len(ransac) else np.zeros(1, np.int32)
    out = np.zeros(cap + 1, np.int32)
    aux = np.zeros(2, np.int32)
    k = lib().pnp_ref_refine_walk(ra.ctypes.data, len(ransac), S.ctypes.data, lens.ctypes.data, cap, rounds, min_inliers,
                                  out.ctypes.data, aux.ctypes.data, aux.ctypes.data + 4)
    return list(out[:k]), int(aux[0]), int(aux[1])


def estimate(xyz_from, kpts_to, xyz_to, pairs, K, local=None, params=None, hyp=True):
    """One job. Returns (result record, inliers (from-indices), RANSAC inlier set (compacted indices), hypotheses (iterations,)
    or None with hyp=False, extra): extra holds the compacted from-indices ("matches"), points ("xyz", "uv") and "gate_margin",
    the least |residual - threshold| over every refine round's reprojection (inf when no refine ran). hyp=False does only the
    work the reference does (no hypotheses beyond the ones the RANSAC loop reaches)."""
    p = params if params is not None else pnp_params()
    x = _a(xyz_from, np.float32).reshape(-1, 3)
    kp = _a(kpts_to, np.float32).reshape(-1, 2)
    xt = _a(xyz_to, np.float32).reshape(-1, 3)
    pr = _a(pairs, np.int32).reshape(-1, 2)
    Kd = _a(K, np.float64)
    lo = None if local is None else _a(local, np.float32).reshape(12)
    res = np.zeros(1, PNP_RESULT_DTYPE)
    k = max(pr.shape[0], 1)
    inl, ran, nran = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(1, np.int32)
    cx, cu, cm = np.zeros((k, 3), np.float32), np.zeros((k, 2), np.float32), np.zeros(k, np.int32)
    hy = np.zeros(p.iterations, PNP_HYP_DTYPE) if hyp else None
    margin = np.zeros(1)
    lib().pnp_ref_estimate(x.ctypes.data, x.shape[0], kp.ctypes.data, xt.ctypes.data, kp.shape[0], pr.ctypes.data, pr.shape[0],
                           Kd.ctypes.data, None if lo is None else lo.ctypes.data, ctypes.byref(p), res.ctypes.data,
                           inl.ctypes.data, cx.ctypes.data, cu.ctypes.data, cm.ctypes.data, ran.ctypes.data, nran.ctypes.data,
                           None if hy is None else hy.ctypes.data, margin.ctypes.data)
    r = res[0]
    n = int(r["num_matches"])
    extra = {"matches": cm[:n].copy(), "xyz": cx[:n].copy(), "uv": cu[:n].copy(), "gate_margin": float(margin[0])}
    return r, inl[:r["num_inliers"]].copy(), ran[:nran[0]].copy(), hy, extra


# ---- literal transcriptions ----------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1


class RNG:
    """cv::RNG: state = (uint64)(unsigned)state * CV_RNG_COEFF + (unsigned)(state >> 32); uniform(a, b) = next() % (b - a) + a."""

    def __init__(self, state):
        self.state = state if state else 0xffffffff

    def next(self):
        self.state = ((self.state & 0xffffffff) * 4164903690 + ((self.state >> 32) & 0xffffffff)) & M64
        return self.state & 0xffffffff

    def uniform(self, a, b):
        return a if a == b else self.next() % (b - a) + a


def get_subset(rng, count, model_points=6):
    """RANSACPointSetRegistrator::getSubset with checkPartialSubsets = false and the default checkSubset (always true)."""
    idx = [0] * model_points
    i = 0
    while i < model_points:
        while True:
            idx_i = idx[i] = rng.uniform(0, count)
            j = 0
            while j < i:
                if idx_i == idx[j]:
                    break
                j += 1
            if j == i:
                break
        i += 1
    return idx


def draw_np(n, iterations):
    rng = RNG(M64)   # RNG rng((uint64)-1)
    return np.array([get_subset(rng, n) for _ in range(iterations)], np.int32).reshape(-1, 6)


def update_num_iters_np(p, ep, model_points, max_iters):
    """RANSACUpdateNumIters with Python's libm; returns (value, num / denom or None)."""
    p, ep = min(max(p, 0.), 1.), min(max(ep, 0.), 1.)
    num = max(1. - p, sys.float_info.min)
    denom = 1. - math.pow(1. - ep, model_points)
    if denom < sys.float_info.min:
        return 0, None
    num, denom = math.log(num), math.log(denom)
    if denom >= 0 or -num >= max_iters * (-denom):
        return max_iters, num / denom
    r = num / denom
    return int(np.rint(r)), r


def replay_np(counts, n, confidence=0.99, model_points=6):
    """RANSACPointSetRegistrator::run's loop over given findInliers counts."""
    niters = max(len(counts), 1)
    max_good = 0
    best = -1
    it = 0
    while it < niters:
        good = counts[it]
        if good > max(max_good, model_points - 1):
            best = it
            max_good = good
            niters = update_num_iters_np(confidence, (n - good) / n, model_points, niters)[0]
        it += 1
    return best, niters, max_good


def refine_walk_np(ransac, sets, rounds, min_inliers):
    """solvePnPRansac's refine loop (MotionEstimation.cpp:291-373) with round r's computeReprojErrors producing sets[r]."""
    inliers = list(ransac)
    new_inliers = []
    prev_inliers = list(inliers)
    refine_count = 0
    solves = 0
    exit_code = 0
    while refine_count < rounds:
        solves += 1                                      # cv::solvePnP on prev_inliers
        new_inliers = list(sets[refine_count])           # computeReprojErrors
        if len(new_inliers) < min_inliers:
            exit_code = 1
            break
        if new_inliers == prev_inliers:                  # std::equal over both ranges
            exit_code = 2
            break
        new_inliers, prev_inliers = prev_inliers, new_inliers   # std::swap(new_inliers, prev_inliers)
        refine_count += 1
    new_inliers, inliers = inliers, new_inliers          # std::swap(new_inliers, inliers)
    return inliers, solves, exit_code
