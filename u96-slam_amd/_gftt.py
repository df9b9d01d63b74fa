"""GFTT keypoints in the reference's two forms: generateKeypoints2 on the PL's uint16 map (src/slam/src/core/GFTT.cpp:41-170)
and OpenCV's detector, generateKeypoints (GFTT.cpp:11-25). Both return (kpts float32 (n, cap, 2), count int32 (n,))."""
import ctypes

import numpy as np

from ._abi import GfttCvParams, GfttSelectParams, StereoBMError, _check, _torch, load_library


def gftt_select_params(max_features=1500, quality_level=0.01, min_distance=7.0, block_size=3):
    """The reference's constants by default."""
    return GfttSelectParams(int(max_features), float(quality_level), float(min_distance), int(block_size))


def gftt_select_validate(params, width, height):
    """Status code of sbm_gftt_select_params_validate (0 = ok)."""
    return load_library().sbm_gftt_select_params_validate(ctypes.byref(params), width, height)


def gftt_select_capacity(params, width, height):
    """Points per image slot: max_features, or every interior pixel when max_features <= 0."""
    return params.max_features if params.max_features > 0 else (width - 2) * (height - 2)


def gftt_cv_params(max_features=1500, quality_level=0.01, min_distance=7.0, block_size=3, use_harris=False, k=0.04):
    """The reference's constants by default."""
    return GfttCvParams(int(max_features), float(quality_level), float(min_distance), int(block_size), int(bool(use_harris)),
                        float(k))


def gftt_cv_validate(params, width, height):
    """Status code of sbm_gftt_cv_params_validate (0 = ok)."""
    return load_library().sbm_gftt_cv_params_validate(ctypes.byref(params), width, height)


def _params(params, kw, make, kind):
    """A parameter struct handed over as such, or made from keyword parameters (either selection's)."""
    if params is None:
        return make(**kw)
    if kw:
        raise TypeError(f"pass either a {kind.__name__} or keyword parameters")
    return params


def _select_params(params, kw):
    return _params(params, kw, gftt_select_params, GfttSelectParams)


def _cv_params(params, kw):
    return _params(params, kw, gftt_cv_params, GfttCvParams)


def _kpts_out(p, n, h, w, device):
    """The output pair of every selection: zeroed kpts (n, cap, 2) and count (n,)."""
    torch = _torch()
    cap = max(gftt_select_capacity(p, w, h), 1)
    return (torch.zeros((n, cap, 2), dtype=torch.float32, device=device), torch.zeros((n,), dtype=torch.int32, device=device))


def _maxima(mx, n, dtype, device):
    m1 = mx.reshape(-1).to(device=device, dtype=dtype).contiguous()
    if m1.numel() != n:
        raise StereoBMError(-2, f"mx holds {m1.numel()} values for {n} maps")
    return m1


class Gftt:
    def gftt_select(self, eig, mx=None, params=None, sync=True, **kw):
        """generateKeypoints2 on torch CUDA maps (n,H,W) or (H,W) -- uint16 payload as int16 (what sbm_gftt_eig_device writes), or
        int32 holding 0..65535 (what gftt_eig returns) -- and their Max words mx (n,) int32, or None: each map's maximum.
        Returns (kpts float32 (n, cap, 2), count int32 (n,)); map i's points are kpts[i, :count[i]], in acceptance order.
        sync=False leaves the call running on the engine's stream (call synchronize() before reading the results)."""
        torch = _torch()
        p = _select_params(params, kw)
        if eig.dim() not in (2, 3) or not eig.is_cuda:
            raise StereoBMError(-2, "eig must be a torch CUDA (n,H,W) or (H,W) tensor")
        if eig.dtype in (torch.int32, torch.int64):
            eig = torch.where(eig > 32767, eig - 65536, eig).to(torch.int16)
        elif eig.dtype != torch.int16 and str(eig.dtype) != "torch.uint16":
            raise StereoBMError(-2, "eig must hold uint16 values (int16, uint16 or int32 tensor)")
        e3, n, h, w = self._as3d(eig)
        kpts, count = _kpts_out(p, n, h, w, e3.device)
        mp = None if mx is None else _maxima(mx, n, torch.int32, e3.device)
        self._device_call(self._L.sbm_gftt_select_device, (n, e3.data_ptr(), None if mp is None else mp.data_ptr(), w, h,
                                                           ctypes.byref(p), kpts.data_ptr(), count.data_ptr()),
                          (e3, mp, kpts, count), sync)
        return kpts, count

    def gftt_detect(self, img, params=None, sync=True, **kw):
        """The KPTS_METHOD_FPGA_GFTT front end on torch CUDA uint8 frames (n,H,W) or (H,W): eigenvalue map, then
        generateKeypoints2, in one call. Returns (kpts float32 (n, cap, 2), count int32 (n,))."""
        torch = _torch()
        p = _select_params(params, kw)
        self._check_device_images(img)
        i3, n, h, w = self._as3d(img)
        eig = torch.empty((n, h, w), dtype=torch.int16, device=i3.device)
        mx = torch.empty((n,), dtype=torch.int32, device=i3.device)
        kpts, count = _kpts_out(p, n, h, w, i3.device)
        self._device_call(self._L.sbm_gftt_detect_device, (n, i3.data_ptr(), w, h, ctypes.byref(p), eig.data_ptr(), mx.data_ptr(),
                                                           kpts.data_ptr(), count.data_ptr()), (i3, eig, mx, kpts, count), sync)
        return kpts, count

    def _points_host(self, fn, a, dtype, name, p, lead=()):
        """A host selection fn(handle, map, stride, w, h, *lead, params, out, cap, count) -> the accepted points (k, 2)."""
        if not isinstance(a, np.ndarray) or a.dtype != dtype or a.ndim != 2 or a.strides[1] != a.itemsize or \
                a.strides[0] < a.itemsize * a.shape[1]:
            raise StereoBMError(-2, f"{name} must be an (H,W) {np.dtype(dtype).name} array with dense rows")
        h, w = a.shape
        cap = gftt_select_capacity(p, w, h)
        out = np.zeros((max(cap, 1), 2), np.float32)
        k = ctypes.c_int()
        _check(fn(self._h, a.ctypes.data, a.strides[0], w, h, *lead, ctypes.byref(p), out.ctypes.data, max(cap, 0), ctypes.byref(k)),
               self._h)
        return out[:k.value].copy()

    def gftt_select_host(self, eig, max_eig, params=None, **kw):
        """numpy uint16 (H,W) map (rows may be strided) + the Max register -> numpy float32 (k, 2) points, as
        generateKeypoints2(eig, max, kpts2d) fills kpts2d."""
        return self._points_host(self._L.sbm_gftt_select, eig, np.uint16, "eig", _select_params(params, kw), (int(max_eig) & 0xffff,))

    def gftt_cv_eig(self, img, sync=True):
        """cv::cornerMinEigenVal (block 3, aperture 3) of torch CUDA uint8 frames (n,H,W) or (H,W), as include/sbm.h states it:
        (float32 maps (n,H,W), float32 maxima (n,))."""
        torch = _torch()
        self._check_device_images(img)
        i3, n, h, w = self._as3d(img)
        eig = torch.empty((n, h, w), dtype=torch.float32, device=i3.device)
        mx = torch.empty((n,), dtype=torch.float32, device=i3.device)
        self._device_call(self._L.sbm_gftt_cv_eig_device, (n, i3.data_ptr(), w, h, eig.data_ptr(), mx.data_ptr()), (i3, eig, mx), sync)
        return eig, mx

    def gftt_cv_detect(self, img, params=None, maps=True, sync=True, **kw):
        """generateKeypoints on torch CUDA uint8 frames (n,H,W) or (H,W). Returns (kpts float32 (n, cap, 2), count int32 (n,)) in
        gftt_select's layout, plus (maps (n,H,W) float32, maxima (n,) float32) when maps=True; maps=False passes no d_eig /
        d_max (the maps then live in the engine's scratch only)."""
        torch = _torch()
        p = _cv_params(params, kw)
        self._check_device_images(img)
        i3, n, h, w = self._as3d(img)
        eig = torch.empty((n, h, w), dtype=torch.float32, device=i3.device) if maps else None
        mx = torch.empty((n,), dtype=torch.float32, device=i3.device) if maps else None
        kpts, count = _kpts_out(p, n, h, w, i3.device)
        self._device_call(self._L.sbm_gftt_cv_detect_device, (n, i3.data_ptr(), w, h, ctypes.byref(p), eig.data_ptr() if maps else None,
                                                              mx.data_ptr() if maps else None, kpts.data_ptr(), count.data_ptr()),
                          (i3, eig, mx, kpts, count), sync)
        return (kpts, count, eig, mx) if maps else (kpts, count)

    def gftt_cv_select(self, eig, mx, params=None, sync=True, **kw):
        """The selection of generateKeypoints on float32 torch CUDA maps (n,H,W) or (H,W) and their maxima mx (n,) float32."""
        torch = _torch()
        p = _cv_params(params, kw)
        if eig.dim() not in (2, 3) or not eig.is_cuda or eig.dtype != torch.float32:
            raise StereoBMError(-2, "eig must be a float32 torch CUDA (n,H,W) or (H,W) tensor")
        e3, n, h, w = self._as3d(eig)
        m1 = _maxima(mx, n, torch.float32, e3.device)
        kpts, count = _kpts_out(p, n, h, w, e3.device)
        self._device_call(self._L.sbm_gftt_cv_select_device, (n, e3.data_ptr(), m1.data_ptr(), w, h, ctypes.byref(p), kpts.data_ptr(),
                                                              count.data_ptr()), (e3, m1, kpts, count), sync)
        return kpts, count

    def gftt_cv_detect_host(self, img, params=None, **kw):
        """numpy uint8 (H,W) frame (rows may be strided) -> numpy float32 (k, 2) points, as generateKeypoints(img, kpts2d) fills
        kpts2d."""
        return self._points_host(self._L.sbm_gftt_cv_detect, img, np.uint8, "img", _cv_params(params, kw))

    def gftt_profile(self):
        return self._profile(("gftt_select_eig", "gftt_select_select", "gftt_select_total"))

    def gftt_cv_profile(self):
        return self._profile(("gftt_cv_eig", "gftt_cv_select", "gftt_cv_total"))
