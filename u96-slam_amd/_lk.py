"""Pyramidal LK stereo, the reference's DEPTH_METHOD_CV_LK: computeCorrespondences (src/slam/src/core/Stereo.cpp:9-51) over
calcOpticalFlowPyrLKStereo (src/slam/src/opencv/CvLKStereo.cpp), its pyramid on its own, and the sparse branch of
generateKeypoints3DStereo (Stereo.cpp:53-117)."""
import ctypes

import numpy as np

from ._abi import LK_GET_MIN_EIGENVALS, LkParams, StereoBMError, _check, _torch, load_library
from ._engine import _count_values


def lk_params(win_width=15, win_height=3, max_level=5, max_count=30, epsilon=0.01, flags=LK_GET_MIN_EIGENVALS,
              min_eig_threshold=1e-4, min_disparity=0.5, max_disparity=128.0):
    """The reference's constants by default; a negative max_disparity switches the disparity gate off."""
    return LkParams(int(win_width), int(win_height), int(max_level), int(max_count), float(epsilon), int(flags),
                    float(min_eig_threshold), float(min_disparity), float(max_disparity))


def lk_validate(params, width, height):
    """Status code of sbm_lk_params_validate (0 = ok)."""
    return load_library().sbm_lk_params_validate(ctypes.byref(params), width, height)


def lk_level_sizes(params, width, height):
    """[(w_l, h_l)] of the levels cv::buildOpticalFlowPyramid keeps (include/sbm.h, "count")."""
    out = [(width, height)]
    while len(out) <= params.max_level:
        width, height = (width + 1) // 2, (height + 1) // 2
        if width <= params.win_width or height <= params.win_height:
            break
        out.append((width, height))
    return out


def _lk(params, kw):
    if params is None:
        return lk_params(**kw)
    if kw:
        raise TypeError("pass either an LkParams or keyword parameters")
    return params


def _pairs(t, n, name):
    """(n, cap, 2) or (cap, 2) float32 CUDA points -> a contiguous (n, cap, 2) tensor."""
    torch = _torch()
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() not in (2, 3) or t.shape[-1] != 2:
        raise StereoBMError(-2, f"{name} must be a float32 CUDA (n, cap, 2) or (cap, 2) tensor")
    t3 = (t if t.dim() == 3 else t[None]).contiguous()
    if t3.shape[0] != n or t3.shape[1] < 1:
        raise StereoBMError(-2, f"{name} holds {t3.shape[0]} frames of {t3.shape[1]} slots for {n} frames")
    return t3


class Lk:
    def lk_pyramid(self, img, params=None, with_deriv=True, **kw):
        """cv::buildOpticalFlowPyramid of torch CUDA uint8 frames (n,H,W) or (H,W) as include/sbm.h states it:
        ([uint8 (n, h_l, w_l) per level], [int16 (n, h_l, w_l, 2) per level]); the second list is empty without with_deriv."""
        torch = _torch()
        p = _lk(params, kw)
        self._check_device_images(img)
        i3, n, h, w = self._as3d(img)
        _check(self._L.sbm_lk_params_validate(ctypes.byref(p), w, h), self._h)
        sizes = lk_level_sizes(p, w, h)
        total = n * sum(a * b for a, b in sizes)
        lev = torch.empty((total,), dtype=torch.uint8, device=i3.device)
        der = torch.empty((total * 2,), dtype=torch.int16, device=i3.device) if with_deriv else None
        last = ctypes.c_int(-1)
        torch.cuda.current_stream(i3.device).synchronize()
        _check(self._L.sbm_lk_pyramid_device(self._h, n, i3.data_ptr(), w, h, 1 if with_deriv else 0, ctypes.byref(p), lev.data_ptr(),
                                             der.data_ptr() if with_deriv else None, ctypes.byref(last)), self._h)
        if last.value != len(sizes) - 1:
            raise StereoBMError(-23, f"the engine kept {last.value + 1} levels, the mirror expected {len(sizes)}")
        planes, ders, off = [], [], 0
        for lw, lh in sizes:
            planes.append(lev[off:off + n * lw * lh].view(n, lh, lw))
            if with_deriv:
                ders.append(der[2 * off:2 * (off + n * lw * lh)].view(n, lh, lw, 2))
            off += n * lw * lh
        return planes, ders

    def lk_stereo(self, left, right, kpts, count, params=None, right_pts=None, status=None, err=None, sync=True, **kw):
        """computeCorrespondences on torch CUDA uint8 pairs (n,H,W) or (H,W). kpts float32 (n, cap, 2) and count int32 (n,) as the
        detectors return them. Returns (right_pts float32 (n, cap, 2), status uint8 (n, cap), err float32 (n, cap)); entries past a
        frame's count keep what the tensors held (zeros when they are allocated here)."""
        torch = _torch()
        p = _lk(params, kw)
        self._check_device_images(left, right)
        if left.shape != right.shape:
            raise StereoBMError(-2, "All the images must have the same size")
        l3, n, h, w = self._as3d(left)
        r3 = self._as3d(right)[0]
        k3 = _pairs(kpts, n, "kpts")
        cap = k3.shape[1]
        c1 = _count_values(count, n, "count must be an int32 CUDA tensor with one value per frame")

        def out(t, shape, dtype, name):
            if t is None:
                return torch.zeros(shape, dtype=dtype, device=l3.device)
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or \
                    t.device != l3.device:
                raise StereoBMError(-2, f"{name} must be a contiguous {dtype} CUDA tensor of shape {shape}")
            return t

        right_pts = out(right_pts, (n, cap, 2), torch.float32, "right_pts")
        status = out(status, (n, cap), torch.uint8, "status")
        err = out(err, (n, cap), torch.float32, "err")
        self._device_call(self._L.sbm_lk_stereo_device, (n, l3.data_ptr(), r3.data_ptr(), w, h, k3.data_ptr(), c1.data_ptr(), cap,
                                                         ctypes.byref(p), right_pts.data_ptr(), status.data_ptr(), err.data_ptr()),
                          (l3, r3, k3, c1, right_pts, status, err), sync)
        return right_pts, status, err

    def keypoints3d_lk(self, kpts, right_pts, status, count, model, min_depth=0.0, max_depth=0.0, sync=True):
        """The sparse branch of generateKeypoints3DStereo on lk_stereo's outputs: float32 (n, cap, 3), NaN where the status is 0;
        entries past a frame's count are NaN too (the tensor starts as NaN)."""
        torch = _torch()
        c1 = count.reshape(-1)
        n = c1.numel()
        k3 = _pairs(kpts, n, "kpts")
        r3 = _pairs(right_pts, n, "right_pts")
        cap = k3.shape[1]
        c1 = _count_values(count, n, "count must be an int32 CUDA tensor with one value per frame")
        s2 = status.reshape(n, -1).contiguous()
        if s2.dtype != torch.uint8 or not s2.is_cuda or s2.shape[1] != cap or r3.shape[1] != cap:
            raise StereoBMError(-2, "right_pts (n, cap, 2) and status uint8 (n, cap) must match kpts")
        xyz = torch.full((n, cap, 3), float("nan"), dtype=torch.float32, device=k3.device)
        self._device_call(self._L.sbm_keypoints3d_lk_device, (n, k3.data_ptr(), r3.data_ptr(), s2.data_ptr(), c1.data_ptr(), cap,
                                                              ctypes.byref(model), min_depth, max_depth, xyz.data_ptr()),
                          (k3, r3, s2, c1, xyz), sync)
        return xyz

    def lk_stereo_host(self, left, right, pts, params=None, **kw):
        """numpy uint8 (H,W) images (rows may be strided) + float32 (k, 2) points -> (right_pts (k, 2), status uint8 (k,), err
        float32 (k,)), as computeCorrespondences(left, right, leftCorners, status) returns and fills them."""
        p = _lk(params, kw)
        for a in (left, right):
            if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 2 or a.strides[1] != 1 or a.strides[0] < a.shape[1]:
                raise StereoBMError(-2, "images must be (H,W) uint8 arrays with dense rows")
        if left.shape != right.shape:
            raise StereoBMError(-2, "All the images must have the same size")
        pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 2))
        k = len(pts)
        h, w = left.shape
        rp, st, er = np.zeros((k, 2), np.float32), np.zeros((k,), np.uint8), np.zeros((k,), np.float32)
        _check(self._L.sbm_lk_stereo(self._h, left.ctypes.data, left.strides[0], right.ctypes.data, right.strides[0], w, h,
                                     pts.ctypes.data, k, ctypes.byref(p), rp.ctypes.data, st.ctypes.data, er.ctypes.data), self._h)
        return rp, st, er

    def lk_profile(self):
        return self._profile(("lk_pyramid", "lk_track", "lk_total"))
