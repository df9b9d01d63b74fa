"""Keypoint matching of computeTransform (src/slam/src/core/Registration.cpp): matchingNoGuess, matchingGuess and its
projection, over a store of per-frame descriptors in sbm_orb_describe_device's layout or on host rows."""
import ctypes

import numpy as np

from ._abi import MatchParams, MatchPlanInfo, StereoBMError, _check, _torch, load_library
from ._engine import _count_values, _jobs_array


def match_params(nndr=0.8, radius=40.0):
    """The reference's values by default."""
    return MatchParams(float(nndr), float(radius))


def match_validate(params):
    """Status code of sbm_match_params_validate (0 = ok)."""
    return load_library().sbm_match_params_validate(ctypes.byref(params))


def match_plan(cap, m=1):
    """The launch plan of a matching / projection call over m jobs on a store of capacity cap (sbm_match_plan: no handle, no
    device). Raises StereoBMError for a cap or m the calls refuse."""
    pl = MatchPlanInfo()
    _check(load_library().sbm_match_plan(int(cap), int(m), ctypes.byref(pl), ctypes.sizeof(pl)))
    return pl


def _desc_rows(d):
    d = np.asarray(d, dtype=np.uint8).reshape(-1, 32)
    if d.strides[1] != 1:
        d = np.ascontiguousarray(d)
    return d


class Match:
    def _match(self, fn, desc, count, jobs, guess, params, knn, sync):
        """Either matching, fn(handle, n, m, jobs, desc, count, cap, *guess tensors, params, pairs, npairs, knn, sync)."""
        torch = _torch()
        if desc.dtype != torch.uint8 or desc.dim() != 3 or desc.shape[2] != 32 or not desc.is_contiguous() or not desc.is_cuda:
            raise StereoBMError(-2, "desc must be a contiguous uint8 CUDA tensor (n, cap, 32)")
        n, cap = desc.shape[0], desc.shape[1]
        c1 = _count_values(count, n, "count must be a contiguous int32 CUDA tensor of n values")
        j = _jobs_array(jobs)
        m = j.shape[0]
        for t, shape in zip(guess, ((n, cap, 2), (m, cap, 2))):
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise StereoBMError(-2, f"expected a contiguous float32 CUDA tensor {shape}")
        p = params if params is not None else match_params()
        pairs = torch.full((m, cap, 2), -1, dtype=torch.int32, device=desc.device)
        npairs = torch.zeros((m,), dtype=torch.int32, device=desc.device)
        rec = torch.zeros((m, cap, 4), dtype=torch.int32, device=desc.device) if knn else None
        self._device_call(fn, (n, m, j.ctypes.data, desc.data_ptr(), c1.data_ptr(), cap) + tuple(t.data_ptr() for t in guess)
                          + (ctypes.byref(p), pairs.data_ptr(), npairs.data_ptr(), rec.data_ptr() if knn else None),
                          (desc, c1) + tuple(guess) + (pairs, npairs, rec), sync)
        return (pairs, npairs, rec) if knn else (pairs, npairs)

    def match(self, desc, count, jobs, params=None, knn=False, sync=True):
        """matchingNoGuess for every (from, to) job over a store in sbm_orb_describe_device's layout: desc uint8 (n, cap, 32),
        count int32 (n,) on the device. Returns (pairs int32 (m, cap, 2), npairs int32 (m,)) [+ records int32 (m, cap, 4)
        with knn=True]; pair slots past npairs hold -1."""
        return self._match(self._L.sbm_match_device, desc, count, jobs, (), params, knn, sync)

    def match_guess(self, desc, count, kpts, proj, jobs, params=None, knn=False, sync=True):
        """matchingGuess's matching: kpts float32 (n, cap, 2) the frames' keypoints, proj float32 (m, cap, 2) each job's projected
        from-points (project_points; NaN = not a query). Returns as match()."""
        return self._match(self._L.sbm_match_guess_device, desc, count, jobs, (kpts, proj), params, knn, sync)

    def project_points(self, xyz, count, from_frames, T, K, size, sync=True):
        """matchingGuess_Projection for m jobs: xyz float32 (n, cap, 3) and count int32 (n,) on the device, from_frames (m,) ints,
        T (m, 12) float32 (guessCameraRef per job), K = (fx, fy, cx, cy), size = (W, H). Returns float32 (m, cap, 2), NaN where
        a point is not valid."""
        torch = _torch()
        if xyz.dtype != torch.float32 or xyz.dim() != 3 or xyz.shape[2] != 3 or not xyz.is_contiguous() or not xyz.is_cuda:
            raise StereoBMError(-2, "xyz must be a contiguous float32 CUDA tensor (n, cap, 3)")
        n, cap = xyz.shape[0], xyz.shape[1]
        c1 = _count_values(count, n, "count must be a contiguous int32 CUDA tensor of n values")
        fr = np.ascontiguousarray(np.asarray(from_frames, np.int32).reshape(-1))
        m = fr.shape[0]
        Tm = np.ascontiguousarray(np.asarray(T, np.float32).reshape(m, 12))
        Kd = np.ascontiguousarray(np.asarray(K, np.float64).reshape(4))
        proj = torch.zeros((max(m, 1), cap, 2), dtype=torch.float32, device=xyz.device)
        self._device_call(self._L.sbm_project_points_device, (n, m, fr.ctypes.data, xyz.data_ptr(), c1.data_ptr(), cap, Tm.ctypes.data,
                                                              Kd.ctypes.data, int(size[0]), int(size[1]), proj.data_ptr()),
                          (xyz, c1, proj), sync)
        return proj

    def match_host(self, desc_from, desc_to, params=None):
        """matchingNoGuess(descriptorsFrom, descriptorsTo) on (k, 32) uint8 host rows (row stride may exceed 32): (k, 2) int32
        (from, to) pairs in increasing from."""
        a, b = _desc_rows(desc_from), _desc_rows(desc_to)
        p = params if params is not None else match_params()
        out = np.zeros((max(a.shape[0], 1), 2), np.int32)
        k = ctypes.c_int()
        _check(self._L.sbm_match(self._h, a.ctypes.data, a.strides[0], a.shape[0], b.ctypes.data, b.strides[0], b.shape[0],
                                 ctypes.byref(p), out.ctypes.data, ctypes.byref(k)), self._h)
        return out[:k.value].copy()

    def match_guess_host(self, xyz_from, kpts_to, desc_from, desc_to, T, K, size, params=None):
        """matchingGuess on host arrays: xyz_from (nf, 3) float32, kpts_to (nt, 2) float32, both descriptor sets, T (12,)
        float32 guessCameraRef, K = (fx, fy, cx, cy), size = (W, H). Returns (k, 2) int32 pairs."""
        a, b = _desc_rows(desc_from), _desc_rows(desc_to)
        x = np.ascontiguousarray(np.asarray(xyz_from, np.float32).reshape(-1, 3))
        kp = np.ascontiguousarray(np.asarray(kpts_to, np.float32).reshape(-1, 2))
        if x.shape[0] != a.shape[0] or kp.shape[0] != b.shape[0]:
            raise StereoBMError(-2, "one 3-D point per from-row and one keypoint per to-row")
        x1 = x if x.shape[0] else np.zeros((1, 3), np.float32)
        k1 = kp if kp.shape[0] else np.zeros((1, 2), np.float32)
        Tm = np.ascontiguousarray(np.asarray(T, np.float32).reshape(12))
        Kd = np.ascontiguousarray(np.asarray(K, np.float64).reshape(4))
        p = params if params is not None else match_params()
        out = np.zeros((max(a.shape[0], 1), 2), np.int32)
        k = ctypes.c_int()
        _check(self._L.sbm_match_guess(self._h, x1.ctypes.data, k1.ctypes.data, a.ctypes.data, a.strides[0], a.shape[0],
                                       b.ctypes.data, b.strides[0], b.shape[0], Tm.ctypes.data, Kd.ctypes.data, int(size[0]),
                                       int(size[1]), ctypes.byref(p), out.ctypes.data, ctypes.byref(k)), self._h)
        return out[:k.value].copy()

    def match_profile(self):
        return self._profile(("match_knn", "match_unique", "match_total", "match_project"))
