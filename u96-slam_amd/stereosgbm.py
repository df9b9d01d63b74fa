"""Host-side mirror of the cv::StereoSGBM interface over the C-ABI (include/sbm.h, sbm_sgbm_*): MODE_HH and MODE_SGBM on
8-bit single-channel pairs, int16 maps in 1/16 px. Like StereoBM, there is no CPU fallback: without the HIP library or a GPU,
construction raises."""
import ctypes

import numpy as np

from .stereobm import StereoBMError, SbmParams, _check, load_library

MODE_SGBM, MODE_HH, MODE_SGBM_3WAY, MODE_HH4 = 0, 1, 2, 3


class SgbmParams(ctypes.Structure):
    """Mirror of `sbm_sgbm_params` (include/sbm.h), in cv::StereoSGBM::create argument order."""

    _fields_ = [(n, ctypes.c_int32) for n in ("min_disparity", "num_disparities", "block_size", "p1", "p2", "disp12_max_diff",
                                                "prefilter_cap", "uniqueness_ratio", "speckle_window_size", "speckle_range", "mode")]


def _bind(L):
    if getattr(L, "_sgbm_bound", False):
        return L
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    sp = ctypes.POINTER(SgbmParams)
    L.sbm_sgbm_params_default.argtypes = [sp, ci, ci, ci]
    L.sbm_sgbm_params_default.restype = None
    L.sbm_sgbm_params_validate.argtypes = [sp, ci, ci]
    L.sbm_sgbm_compute.argtypes = [vp, sp, vp, sz, vp, sz, ci, ci, vp, sz]
    L.sbm_sgbm_compute_device.argtypes = [vp, sp, ci, vp, vp, ci, ci, vp, ci]
    L._sgbm_bound = True
    return L


def sgbm_params(minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0, uniquenessRatio=0,
                speckleWindowSize=0, speckleRange=0, mode=MODE_SGBM):
    return SgbmParams(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio,
                      speckleWindowSize, speckleRange, mode)


def sgbm_validate(params, width, height):
    """sbm_sgbm_params_validate: 0 or a negative status code."""
    return _bind(load_library()).sbm_sgbm_params_validate(ctypes.byref(params), width, height)


class StereoSGBM:
    """cv::StereoSGBM look-alike. One instance owns one device handle (stream + scratch); not thread-safe."""

    def __init__(self, minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0,
                 uniquenessRatio=0, speckleWindowSize=0, speckleRange=0, mode=MODE_SGBM, device=0):
        L = _bind(load_library())
        self._L = L
        self._p = SgbmParams()
        L.sbm_sgbm_params_default(ctypes.byref(self._p), minDisparity, numDisparities, blockSize)
        for name, v in (("p1", P1), ("p2", P2), ("disp12_max_diff", disp12MaxDiff), ("prefilter_cap", preFilterCap),
                        ("uniqueness_ratio", uniquenessRatio), ("speckle_window_size", speckleWindowSize),
                        ("speckle_range", speckleRange), ("mode", mode)):
            setattr(self._p, name, int(v))
        bm = SbmParams()
        L.sbm_params_default(ctypes.byref(bm), 0, 0)   # the handle's block-matcher parameters are not used here
        self._h = ctypes.c_void_p()
        self._device = device
        self._inflight = []
        _check(L.sbm_create(ctypes.byref(self._h), ctypes.byref(bm), device))

    @staticmethod
    def create(minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0, uniquenessRatio=0,
               speckleWindowSize=0, speckleRange=0, mode=MODE_SGBM, device=0):
        return StereoSGBM(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio,
                          speckleWindowSize, speckleRange, mode, device)

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            if self._inflight:
                self._L.sbm_synchronize(h)
                self._inflight.clear()
            self._L.sbm_destroy(h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def params(self):
        return self._p

    @property
    def handle(self):
        return self._h

    # ---- the cv::StereoSGBM / cv::StereoMatcher setters and getters --------------------------------------------------------
    def setMinDisparity(self, v): self._p.min_disparity = int(v)
    def setNumDisparities(self, v): self._p.num_disparities = int(v)
    def setBlockSize(self, v): self._p.block_size = int(v)
    def setP1(self, v): self._p.p1 = int(v)
    def setP2(self, v): self._p.p2 = int(v)
    def setDisp12MaxDiff(self, v): self._p.disp12_max_diff = int(v)
    def setPreFilterCap(self, v): self._p.prefilter_cap = int(v)
    def setUniquenessRatio(self, v): self._p.uniqueness_ratio = int(v)
    def setSpeckleWindowSize(self, v): self._p.speckle_window_size = int(v)
    def setSpeckleRange(self, v): self._p.speckle_range = int(v)
    def setMode(self, v): self._p.mode = int(v)

    def getMinDisparity(self): return self._p.min_disparity
    def getNumDisparities(self): return self._p.num_disparities
    def getBlockSize(self): return self._p.block_size
    def getP1(self): return self._p.p1
    def getP2(self): return self._p.p2
    def getDisp12MaxDiff(self): return self._p.disp12_max_diff
    def getPreFilterCap(self): return self._p.prefilter_cap
    def getUniquenessRatio(self): return self._p.uniqueness_ratio
    def getSpeckleWindowSize(self): return self._p.speckle_window_size
    def getSpeckleRange(self): return self._p.speckle_range
    def getMode(self): return self._p.mode

    def compute(self, left, right, disparity=None, sync=True):
        """cv::StereoSGBM::compute. numpy (H,W) uint8 -> numpy int16 (host entry point, one pair); torch CUDA uint8 (H,W) or
        (n,H,W) -> torch CUDA int16 (device entry point)."""
        if isinstance(left, np.ndarray):
            return self._compute_host(left, right, disparity)
        return self.compute_device(left, right, disparity, sync)

    def _compute_host(self, left, right, disparity):
        if not isinstance(right, np.ndarray) or left.shape != right.shape:
            raise StereoBMError(-2, "All the images must have the same size")
        if left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim != 2:
            raise StereoBMError(-2, "Both input images must be (H,W) CV_8UC1")
        h, w = left.shape
        left = left if left.strides[-1] == 1 and left.strides[0] >= w else np.ascontiguousarray(left)
        right = right if right.strides[-1] == 1 and right.strides[0] >= w else np.ascontiguousarray(right)
        out = disparity if disparity is not None else np.empty((h, w), np.int16)
        if (not isinstance(out, np.ndarray) or out.dtype != np.int16 or out.shape != (h, w) or not out.flags.writeable
                or out.strides[-1] != 2 or out.strides[0] < 2 * w):
            raise StereoBMError(-2, f"disparity must be a writable int16 array of shape {(h, w)} with dense rows")
        _check(self._L.sbm_sgbm_compute(self._h, ctypes.byref(self._p), left.ctypes.data, left.strides[0], right.ctypes.data,
                                        right.strides[0], w, h, out.ctypes.data, out.strides[0]), self._h)
        return out

    def compute_device(self, left, right, disparity=None, sync=True):
        import torch

        if left.shape != right.shape:
            raise StereoBMError(-2, "All the images must have the same size")
        if left.dtype != torch.uint8 or right.dtype != torch.uint8 or not left.is_cuda or not right.is_cuda:
            raise StereoBMError(-2, "Both input images must be CUDA uint8 tensors")
        if left.device.index != self._device or right.device.index != self._device:
            raise StereoBMError(-20, f"tensor on cuda:{left.device.index}, engine on device {self._device}")
        if left.dim() not in (2, 3):
            raise StereoBMError(-2, "expected (H,W) or (n,H,W) images")
        left, right = left.contiguous(), right.contiguous()
        shape = left.shape
        n = 1 if left.dim() == 2 else shape[0]
        h, w = shape[-2], shape[-1]
        if disparity is None:
            disparity = torch.empty(shape, dtype=torch.int16, device=left.device)
        elif (not isinstance(disparity, torch.Tensor) or disparity.dtype != torch.int16 or disparity.device != left.device
              or tuple(disparity.shape) != tuple(shape) or not disparity.is_contiguous()):
            raise StereoBMError(-2, f"disparity must be a contiguous CUDA int16 tensor of shape {tuple(shape)} on {left.device}")
        torch.cuda.current_stream(left.device).synchronize()   # the engine's stream does not order behind torch's
        _check(self._L.sbm_sgbm_compute_device(self._h, ctypes.byref(self._p), n, left.data_ptr(), right.data_ptr(), w, h,
                                               disparity.data_ptr(), 1 if sync else 0), self._h)
        if sync:
            self._inflight.clear()
        else:
            self._inflight.append((left, right, disparity))
        return disparity

    def synchronize(self):
        _check(self._L.sbm_synchronize(self._h), self._h)
        self._inflight.clear()

    def debug_fetch(self, which, shape, dtype=np.int16):
        out = np.empty(shape, dtype)
        _check(self._L.sbm_debug_fetch(self._h, which, out.ctypes.data, out.nbytes), self._h)
        return out

    def set_profiling(self, enabled):
        _check(self._L.sbm_set_profiling(self._h, enabled), self._h)

    def profile(self, name):
        ms = ctypes.c_float()
        _check(self._L.sbm_get_profile(self._h, name.encode(), ctypes.byref(ms)), self._h)
        return ms.value
