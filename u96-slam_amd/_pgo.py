"""The pose-graph optimiser of the reference's main loop: runOptimize and runOptimizeRobust (src/slam/src/core/Optimizer.cpp,
HyperGraph.cpp, GraphEdge.cpp, GraphVertex.cpp, g2o/SE3Gradient.cpp, getConnectedGraph of Mapper.cpp:195-255) with the
Levenberg-Marquardt iteration on the device. include/sbm.h states the arithmetic and the readings."""
import ctypes

import numpy as np

from ._abi import (PGO_COUPLING_REFERENCE, PGO_COUPLING_SYMMETRIC, PGO_EDGE_RECORD, PgoGraph, PgoParams, PgoPlanInfo,  # noqa: F401
                   StereoBMError, _check, _torch, load_library)

_FIELDS = (("e", 0, (6,)), ("chi", 6, ()), ("Ji", 8, (6, 6)), ("Jj", 44, (6, 6)), ("mii", 80, (6, 6)), ("mjj", 116, (6, 6)),
           ("mij", 152, (6, 6)), ("bi", 188, (6,)), ("bj", 194, (6,)))


def pgo_params(num=20, fixed_id=1, coupling=PGO_COUPLING_REFERENCE, run_max=64):
    """The reference's values by default: 20 iterations, vertex 1 fixed, the lower-triangle reading of the coupling."""
    return PgoParams(int(num), int(fixed_id), int(coupling), int(run_max))


class _Arrays:
    """The caller's arrays as the C structure sees them; keeps them alive."""

    def __init__(self, ids, poses, frm, to, meas, info):
        self.ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
        self.poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 12))
        self.frm = np.ascontiguousarray(np.asarray(frm, np.int32).reshape(-1))
        self.to = np.ascontiguousarray(np.asarray(to, np.int32).reshape(-1))
        self.meas = np.ascontiguousarray(np.asarray(meas, np.float64).reshape(-1, 12))
        self.info = np.ascontiguousarray(np.asarray(info, np.float64).reshape(-1, 36))
        if len(self.poses) != len(self.ids) or not (len(self.frm) == len(self.to) == len(self.meas) == len(self.info)):
            raise StereoBMError(-2, "ids / poses and from / to / meas / info must have matching lengths")
        ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        self.c = PgoGraph(len(self.ids), ptr(self.ids), ptr(self.poses), len(self.frm), ptr(self.frm), ptr(self.to), ptr(self.meas),
                          ptr(self.info))


def pgo_check(params, ids, poses, frm, to, meas, info):
    """Status code of sbm_pgo_params_check (0 = ok). Needs no GPU."""
    a = _Arrays(ids, poses, frm, to, meas, info)
    return load_library().sbm_pgo_params_check(ctypes.byref(params), ctypes.byref(a.c))


def pgo_plan(params, ids, poses, frm, to, meas, info):
    """The partition of one graph, computed on the host: (PgoPlanInfo, vertex_run int32 (n_free,): run or -1 for a junction,
    slot_rc int32 (n_slots, 2): the coupled pairs as (row, column) Hessian indices, edge_couples bool (n_edges,)). Raises for a
    refused graph; a graph over the junction cap raises StereoBMError(-23)."""
    a = _Arrays(ids, poses, frm, to, meas, info)
    info_ = PgoPlanInfo()
    vrun = np.full(max(len(a.ids), 1), -2, np.int32)
    rc = np.zeros((max(len(a.frm), 1), 2), np.int32)
    cp = np.zeros(max(len(a.frm), 1), np.uint8)
    _check(load_library().sbm_pgo_plan(ctypes.byref(params), ctypes.byref(a.c), ctypes.byref(info_), vrun.ctypes.data, rc.ctypes.data,
                                       cp.ctypes.data))
    return info_, vrun[:info_.n_free], rc[:info_.n_slots], cp[:len(a.frm)].astype(bool)


class PoseGraph:
    """runOptimize / runOptimizeRobust on the device of `engine` (a StereoBM or StereoSGBM), which must outlive it: the optimiser
    uses the engine's handle, stream and scratch. Not thread-safe."""

    def __init__(self, engine, params=None, **kw):
        if params is not None and kw:
            raise TypeError("pass either a PgoParams or keyword parameters")
        self.params = params if params is not None else pgo_params(**kw)
        self._engine = engine
        self._L = engine._L

    def optimize(self, ids, poses, frm, to, meas, info):
        """runOptimize: returns (err, ids ascending int32, poses float64 (n, 3, 4))."""
        a = _Arrays(ids, poses, frm, to, meas, info)
        out = np.empty((max(len(a.ids), 1), 12), np.float64)
        err = ctypes.c_double()
        _check(self._L.sbm_pgo_optimize(self._engine._h, ctypes.byref(self.params), ctypes.byref(a.c), out.ctypes.data,
                                        ctypes.byref(err)), self._engine._h)
        return err.value, np.sort(a.ids), out[:len(a.ids)].reshape(-1, 3, 4)

    def optimize_robust(self, ids, poses, frm, to, meas, info):
        """runOptimizeRobust: returns (err, ids of the reached vertices, their poses, the removed (from, to) links in order)."""
        a = _Arrays(ids, poses, frm, to, meas, info)
        n, nrem, err = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        oid = np.empty(max(len(a.ids), 1), np.int32)
        out = np.empty((max(len(a.ids), 1), 12), np.float64)
        rem = np.empty((max(len(a.frm), 1), 2), np.int32)
        _check(self._L.sbm_pgo_optimize_robust(self._engine._h, ctypes.byref(self.params), ctypes.byref(a.c), ctypes.byref(n),
                                               oid.ctypes.data, out.ctypes.data, ctypes.byref(err), rem.ctypes.data, len(rem),
                                               ctypes.byref(nrem)), self._engine._h)
        return err.value, oid[:n.value].copy(), out[:n.value].reshape(-1, 3, 4), [tuple(int(v) for v in r) for r in rem[:nrem.value]]

    def _device_graph(self, ids, poses, frm, to, meas, info):
        """The C structure over torch CUDA float64 tensors poses (n, 3, 4), meas (E, 3, 4), info (E, 6, 6) and host id arrays."""
        torch = _torch()
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
        frm = np.ascontiguousarray(np.asarray(frm, np.int32).reshape(-1))
        to = np.ascontiguousarray(np.asarray(to, np.int32).reshape(-1))
        for t, rows, width in ((poses, len(ids), 12), (meas, len(frm), 12), (info, len(frm), 36)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or not t.is_cuda or not t.is_contiguous() or \
                    t.numel() != rows * width or t.device.index != self._engine._device:
                raise StereoBMError(-2, "poses / meas / info must be contiguous float64 CUDA tensors on the engine's device")
        if len(frm) != len(to):
            raise StereoBMError(-2, "from / to must have matching lengths")
        torch.cuda.current_stream(poses.device).synchronize()
        ptr = lambda a: a.ctypes.data if a.size else None  # noqa: E731
        dptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
        return (ids, frm, to), PgoGraph(len(ids), ptr(ids), dptr(poses), len(frm), ptr(frm), ptr(to), dptr(meas), dptr(info))

    def optimize_device(self, ids, poses, frm, to, meas, info):
        """runOptimize on device arrays (torch CUDA float64; ids / from / to host): returns (err, ids ascending, poses as a CUDA
        tensor (n, 3, 4)), bit for bit what optimize returns."""
        torch = _torch()
        keep, g = self._device_graph(ids, poses, frm, to, meas, info)
        out = torch.empty((len(keep[0]), 3, 4), dtype=torch.float64, device=poses.device)
        err = ctypes.c_double()
        _check(self._L.sbm_pgo_optimize_device(self._engine._h, ctypes.byref(self.params), ctypes.byref(g), out.data_ptr(),
                                               ctypes.byref(err)), self._engine._h)
        return err.value, np.sort(keep[0]), out

    def optimize_robust_device(self, ids, poses, frm, to, meas, info):
        """runOptimizeRobust on device arrays: (err, reached ids, their poses as a CUDA tensor, the removed links)."""
        torch = _torch()
        keep, g = self._device_graph(ids, poses, frm, to, meas, info)
        n, nrem, err = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_double()
        oid = np.empty(max(len(keep[0]), 1), np.int32)
        out = torch.empty((max(len(keep[0]), 1), 3, 4), dtype=torch.float64, device=poses.device)
        rem = np.empty((max(len(keep[1]), 1), 2), np.int32)
        _check(self._L.sbm_pgo_optimize_robust_device(self._engine._h, ctypes.byref(self.params), ctypes.byref(g), ctypes.byref(n),
                                                      oid.ctypes.data, out.data_ptr(), ctypes.byref(err), rem.ctypes.data, len(rem),
                                                      ctypes.byref(nrem)), self._engine._h)
        return err.value, oid[:n.value].copy(), out[:n.value], [tuple(int(v) for v in r) for r in rem[:nrem.value]]

    def last_plan(self):
        """(PgoPlanInfo, lambda of the last iteration, iterations run) of the last optimisation on this engine."""
        info_, lam, it = PgoPlanInfo(), ctypes.c_double(), ctypes.c_int32()
        _check(self._L.sbm_pgo_last_plan(self._engine._h, ctypes.byref(info_), ctypes.byref(lam), ctypes.byref(it)), self._engine._h)
        return info_, lam.value, it.value

    def debug(self, n_edges):
        """The last iteration of the last optimisation: dict of per-edge e, chi, Ji, Jj, mii, mjj, mij, bi, bj, and the system D
        (n_free, 6, 6), E (n_slots, 6, 6), b, x (n_free, 6), lam."""
        info_, lam, _ = self.last_plan()

        def fetch(which, shape):
            buf = np.empty(shape, np.float64)
            _check(self._L.sbm_pgo_debug_fetch(self._engine._h, which, buf.ctypes.data, buf.nbytes), self._engine._h)
            return buf

        rec = fetch(0, (n_edges, PGO_EDGE_RECORD))
        out = {k: rec[:, o:o + int(np.prod(s, dtype=int))].reshape((n_edges,) + s).copy() for k, o, s in _FIELDS}
        out.update(D=fetch(1, (info_.n_free, 6, 6)), E=fetch(2, (info_.n_slots, 6, 6)), b=fetch(3, (info_.n_free, 6)),
                   x=fetch(4, (info_.n_free, 6)), lam=lam)
        return out

    def profile(self):
        return self._engine._profile(("pgo_linearise", "pgo_assemble", "pgo_solve", "pgo_update", "pgo_total"))
