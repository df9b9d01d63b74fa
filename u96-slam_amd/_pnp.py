"""Motion estimation of computeTransform (Registration.cpp:337-397): estimateMotion's PnP-RANSAC and refinement."""
import ctypes

import numpy as np

from ._abi import PNP_HYP_DTYPE, PNP_RESULT_DTYPE, PnpParams, StereoBMError, _check, _torch, load_library
from ._engine import _count_values, _jobs_array


def pnp_params(min_inliers=20, refine_iterations=1, iterations=300, reprojection_error=2.0, refine_sigma=3.0, confidence=0.99):
    """The reference's values by default."""
    return PnpParams(int(min_inliers), int(refine_iterations), int(iterations), float(reprojection_error), float(refine_sigma), 0,
                     float(confidence))


def pnp_validate(params):
    """Status code of sbm_pnp_params_validate (0 = ok)."""
    return load_library().sbm_pnp_params_validate(ctypes.byref(params))


def pnp_records(t, dtype=None):
    """Device or host bytes of sbm_pnp_result (or, with dtype=PNP_HYP_DTYPE, sbm_pnp_hypothesis) records -> numpy records."""
    dtype = PNP_RESULT_DTYPE if dtype is None else dtype
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=dtype).reshape(a.shape[:-1])


class Pnp:
    def estimate_motion(self, xyz, kpts, count, pairs, npairs, jobs, K, model=None, params=None, hyp=False, sync=True):
        """estimateMotion for every (from, to) job over a store: xyz float32 (n, cap, 3) (keypoints3d per frame), kpts float32
        (n, cap, 2), count int32 (n,), pairs int32 (m, cap, 2) and npairs int32 (m,) as match() returns them, all on the device;
        K = (fx, fy, cx, cy); model: a StereoModel whose localTransform applies, or None. Returns (results uint8 (m, 216): one
        sbm_pnp_result per job, decode with pnp_records; inliers int32 (m, cap) from-indices) [+ hypotheses uint8
        (m, iterations, 128) with hyp=True]."""
        torch = _torch()
        for t, d, last in ((xyz, torch.float32, 3), (kpts, torch.float32, 2), (pairs, torch.int32, 2)):
            if t.dtype != d or t.dim() != 3 or t.shape[2] != last or not t.is_contiguous() or not t.is_cuda:
                raise StereoBMError(-2, f"expected a contiguous {d} CUDA tensor (., cap, {last})")
        n, cap = xyz.shape[0], xyz.shape[1]
        if tuple(kpts.shape[:2]) != (n, cap) or pairs.shape[1] != cap:
            raise StereoBMError(-2, "xyz, kpts and pairs must share cap; xyz and kpts the frame count")
        c1 = _count_values(count, n, "count / npairs must be contiguous int32 CUDA tensors")
        np1 = _count_values(npairs, pairs.shape[0], "count / npairs must be contiguous int32 CUDA tensors")
        j = _jobs_array(jobs)
        m = j.shape[0]
        if pairs.shape[0] < m:
            raise StereoBMError(-2, "one pair list per job")
        p = params if params is not None else pnp_params()
        Kd = np.ascontiguousarray(np.asarray(K, np.float64).reshape(4))
        res = torch.zeros((m, PNP_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=xyz.device)
        inl = torch.full((m, cap), -1, dtype=torch.int32, device=xyz.device)
        hy = torch.zeros((m, max(p.iterations, 1), PNP_HYP_DTYPE.itemsize), dtype=torch.uint8, device=xyz.device) if hyp else None
        self._device_call(self._L.sbm_estimate_motion_device,
                          (n, m, j.ctypes.data, xyz.data_ptr(), kpts.data_ptr(), c1.data_ptr(), cap, pairs.data_ptr(), np1.data_ptr(),
                           Kd.ctypes.data, None if model is None else ctypes.byref(model), ctypes.byref(p), res.data_ptr(),
                           inl.data_ptr(), hy.data_ptr() if hyp else None), (xyz, kpts, c1, pairs, np1, res, inl, hy), sync)
        return (res, inl, hy) if hyp else (res, inl)

    def estimate_motion_host(self, xyz_from, kpts_to, xyz_to, pairs, K, model=None, params=None):
        """estimateMotion on host arrays: xyz_from (nf, 3), kpts_to (nt, 2), xyz_to (nt, 3) float32, pairs (k, 2) int32
        (from, to). Returns (the sbm_pnp_result record as a numpy record, inliers int32 from-indices)."""
        x = np.ascontiguousarray(np.asarray(xyz_from, np.float32).reshape(-1, 3))
        kp = np.ascontiguousarray(np.asarray(kpts_to, np.float32).reshape(-1, 2))
        xt = np.ascontiguousarray(np.asarray(xyz_to, np.float32).reshape(-1, 3))
        pr = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        if kp.shape[0] != xt.shape[0]:
            raise StereoBMError(-2, "one 3-D point per to-keypoint")
        p = params if params is not None else pnp_params()
        Kd = np.ascontiguousarray(np.asarray(K, np.float64).reshape(4))
        res = np.zeros(1, PNP_RESULT_DTYPE)
        inl = np.zeros(max(pr.shape[0], 1), np.int32)
        _check(self._L.sbm_estimate_motion(self._h, x.ctypes.data if x.size else None, x.shape[0], kp.ctypes.data if kp.size else None,
                                           xt.ctypes.data if xt.size else None, kp.shape[0], pr.ctypes.data if pr.size else None,
                                           pr.shape[0], Kd.ctypes.data, None if model is None else ctypes.byref(model),
                                           ctypes.byref(p), res.ctypes.data, inl.ctypes.data), self._h)
        return res[0], inl[:res[0]["num_inliers"]].copy()

    def pnp_profile(self):
        return self._profile(("pnp_hyp", "pnp_score", "pnp_refine", "pnp_total"))
