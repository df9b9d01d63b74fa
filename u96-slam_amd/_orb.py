"""ORB descriptors of computeDescriptor (src/slam/src/opencv/CvORB.cpp), alone or behind either GFTT selection in one call."""
import ctypes

import numpy as np

from ._abi import OrbParams, StereoBMError, _check, _torch, load_library
from ._engine import _count_values
from ._gftt import _cv_params, _kpts_out, _select_params


def orb_params(edge_threshold=19, angle=-1.0, blur_ksize=7, blur_sigma=2.0):
    """The reference's values by default."""
    return OrbParams(int(edge_threshold), float(angle), int(blur_ksize), float(blur_sigma))


def orb_validate(params):
    """Status code of sbm_orb_params_validate (0 = ok)."""
    return load_library().sbm_orb_params_validate(ctypes.byref(params))


def orb_pattern_array(pattern):
    """512 (x, y) points as a contiguous int32 array of 1024 values (ctypes pointer + keep-alive)."""
    p = np.ascontiguousarray(np.asarray(pattern, dtype=np.int32).reshape(-1))
    if p.size != 1024:
        raise StereoBMError(-2, f"the pattern holds {p.size} values, not 1024 (512 points)")
    return p


def _params(params, angle, edge_threshold):
    return params if params is not None else orb_params(edge_threshold=edge_threshold, angle=angle)


def _desc_out(n, cap, h, w, blur, device):
    """Zeroed descriptors (n, cap, 32) and, with blur, the blurred frames (n, H, W); (desc, bl, bl's address or None)."""
    torch = _torch()
    desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device=device)
    bl = torch.zeros((n, h, w), dtype=torch.uint8, device=device) if blur else None
    return desc, bl, None if bl is None else bl.data_ptr()


class Orb:
    def orb_describe(self, img, kpts, count, pattern, angle=-1.0, edge_threshold=19, params=None, out=None, blur=False,
                     sync=True):
        """computeDescriptor on torch CUDA uint8 frames (n,H,W) or (H,W) with keypoints in sbm_gftt_select_device's layout:
        kpts float32 (n, cap, 2), count int32 (n,) on the device. Returns (desc uint8 (n, cap, 32), kpts_kept (n, cap, 2),
        count_kept (n,)), plus the blurred frames (n, H, W) when blur=True. out="inplace" compacts into kpts / count themselves;
        otherwise new tensors (copies of kpts, so slots past the kept count keep their old values). Descriptor rows past the
        kept count are zero here (the C-ABI leaves them as they were)."""
        torch = _torch()
        p = _params(params, angle, edge_threshold)
        pat = orb_pattern_array(pattern)
        self._check_device_images(img)
        i3, n, h, w = self._as3d(img)
        k3 = kpts if kpts.dim() == 3 else kpts[None]
        if k3.dtype != torch.float32 or k3.shape[0] != n or k3.shape[2] != 2 or not k3.is_contiguous() or not k3.is_cuda:
            raise StereoBMError(-2, "kpts must be a contiguous float32 CUDA tensor (n, cap, 2)")
        c1 = _count_values(count, n, "count must be an int32 CUDA tensor of n values", dense=False)
        cap = k3.shape[1]
        ko, co = (k3, c1) if out == "inplace" else (k3.clone(), torch.zeros_like(c1))
        desc, bl, d_bl = _desc_out(n, cap, h, w, blur, i3.device)
        self._device_call(self._L.sbm_orb_describe_device,
                          (n, i3.data_ptr(), w, h, cap, k3.data_ptr(), c1.data_ptr(), pat.ctypes.data, ctypes.byref(p), ko.data_ptr(),
                           co.data_ptr(), desc.data_ptr(), d_bl), (i3, k3, c1, ko, co, desc, bl), sync)
        return (desc, ko, co, bl) if blur else (desc, ko, co)

    def orb_describe_host(self, img, kpts, pattern, angle=-1.0, edge_threshold=19, params=None):
        """numpy uint8 (H,W) frame (rows may be strided) + float32 (k, 2) keypoints -> (desc uint8 (m, 32), kept (m, 2)), as
        computeDescriptor(image, noArray(), kpts, true, desc) leaves desc and kpts."""
        p = _params(params, angle, edge_threshold)
        pat = orb_pattern_array(pattern)
        if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1:
            raise StereoBMError(-2, "img must be an (H,W) uint8 array with dense rows")
        h, w = img.shape
        kp = np.ascontiguousarray(np.asarray(kpts, dtype=np.float32).reshape(-1, 2))
        k = kp.shape[0]
        kept = np.zeros((max(k, 1), 2), np.float32)
        desc = np.zeros((max(k, 1), 32), np.uint8)
        m = ctypes.c_int()
        _check(self._L.sbm_orb_describe(self._h, img.ctypes.data, img.strides[0], w, h, kp.ctypes.data, k, pat.ctypes.data,
                                        ctypes.byref(p), kept.ctypes.data, ctypes.byref(m), desc.ctypes.data), self._h)
        return desc[:m.value].copy(), kept[:m.value].copy()

    def _features(self, fn, gp, maps, img, pattern, p, blur, sync):
        """A detector and computeDescriptor in one call: fn(handle, n, img, w, h, gftt params, pattern, orb params, d_eig,
        d_max, kpts, count, desc, blur, sync); maps: hand the PL's int16 map and int32 maxima out of the scratch."""
        torch = _torch()
        pat = orb_pattern_array(pattern)
        self._check_device_images(img)
        i3, n, h, w = self._as3d(img)
        eig = torch.empty((n, h, w), dtype=torch.int16, device=i3.device) if maps else None
        mx = torch.empty((n,), dtype=torch.int32, device=i3.device) if maps else None
        kpts, count = _kpts_out(gp, n, h, w, i3.device)
        desc, bl, d_bl = _desc_out(n, kpts.shape[1], h, w, blur, i3.device)
        self._device_call(fn, (n, i3.data_ptr(), w, h, ctypes.byref(gp), pat.ctypes.data, ctypes.byref(p),
                               eig.data_ptr() if maps else None, mx.data_ptr() if maps else None, kpts.data_ptr(),
                               count.data_ptr(), desc.data_ptr(), d_bl), (i3, eig, mx, kpts, count, desc, bl), sync)
        return (desc, kpts, count, bl) if blur else (desc, kpts, count)

    def orb_features(self, img, pattern, gftt=None, angle=-1.0, edge_threshold=19, params=None, blur=False, sync=True, **kw):
        """The KPTS_METHOD_FPGA_GFTT + desc front end on torch CUDA uint8 frames (n,H,W) or (H,W): eigenvalue map,
        generateKeypoints2, computeDescriptor, in one call. gftt: a GfttSelectParams (or keyword parameters of
        gftt_select_params). Returns (desc (n, cap, 32), kpts (n, cap, 2), count (n,)) [+ blurred frames]."""
        return self._features(self._L.sbm_orb_features_device, _select_params(gftt, kw), True, img, pattern,
                              _params(params, angle, edge_threshold), blur, sync)

    def orb_features_cv(self, img, pattern, gftt=None, angle=-1.0, edge_threshold=19, params=None, blur=False, sync=True, **kw):
        """The KPTS_METHOD_CV_GFTT + desc front end (SLAM_BATCH's) on torch CUDA uint8 frames (n,H,W) or (H,W): generateKeypoints,
        computeDescriptor, in one call. gftt: a GfttCvParams (or keyword parameters of gftt_cv_params). Returns (desc (n, cap,
        32), kpts (n, cap, 2), count (n,)) [+ blurred frames]."""
        return self._features(self._L.sbm_orb_features_cv_device, _cv_params(gftt, kw), False, img, pattern,
                              _params(params, angle, edge_threshold), blur, sync)

    def orb_profile(self):
        return self._profile(("orb_blur", "orb_desc", "orb_total"))
