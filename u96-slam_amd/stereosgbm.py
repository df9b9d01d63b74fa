"""Host-side mirror of the cv::StereoSGBM interface over the C-ABI (include/sbm.h, sbm_sgbm_*): MODE_HH and MODE_SGBM on
8-bit single-channel pairs, int16 maps in 1/16 px. Like StereoBM, there is no CPU fallback: without the HIP library or a GPU,
construction raises."""
import ctypes

import numpy as np

from . import _engine
from ._abi import SgbmParams
from .stereobm import StereoBMError, SbmParams, _check, load_library

MODE_SGBM, MODE_HH, MODE_SGBM_3WAY, MODE_HH4 = 0, 1, 2, 3


def sgbm_params(minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0, uniquenessRatio=0,
                speckleWindowSize=0, speckleRange=0, mode=MODE_SGBM):
    return SgbmParams(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio,
                      speckleWindowSize, speckleRange, mode)


def sgbm_validate(params, width, height):
    """sbm_sgbm_params_validate: 0 or a negative status code."""
    return load_library().sbm_sgbm_params_validate(ctypes.byref(params), width, height)


class StereoSGBM(_engine.Engine):
    """cv::StereoSGBM look-alike. One instance owns one device handle (stream + scratch); not thread-safe."""

    def __init__(self, minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0,
                 uniquenessRatio=0, speckleWindowSize=0, speckleRange=0, mode=MODE_SGBM, device=0):
        L = load_library()
        self._p = SgbmParams()
        L.sbm_sgbm_params_default(ctypes.byref(self._p), minDisparity, numDisparities, blockSize)
        for name, v in (("p1", P1), ("p2", P2), ("disp12_max_diff", disp12MaxDiff), ("prefilter_cap", preFilterCap),
                        ("uniqueness_ratio", uniquenessRatio), ("speckle_window_size", speckleWindowSize),
                        ("speckle_range", speckleRange), ("mode", mode)):
            setattr(self._p, name, int(v))
        bm = SbmParams()
        L.sbm_params_default(ctypes.byref(bm), 0, 0)   # the handle's block-matcher parameters are not used here
        self._open(L, bm, device)

    @staticmethod
    def create(minDisparity=0, numDisparities=16, blockSize=3, P1=0, P2=0, disp12MaxDiff=0, preFilterCap=0, uniquenessRatio=0,
               speckleWindowSize=0, speckleRange=0, mode=MODE_SGBM, device=0):
        return StereoSGBM(minDisparity, numDisparities, blockSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio,
                          speckleWindowSize, speckleRange, mode, device)

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
        return self._compute_device(self._L.sbm_sgbm_compute_device, (ctypes.byref(self._p),), left, right, disparity, sync)

    def debug_fetch(self, which, shape, dtype=np.int16):
        out = np.empty(shape, dtype)
        _check(self._L.sbm_debug_fetch(self._h, which, out.ctypes.data, out.nbytes), self._h)
        return out

    def set_profiling(self, enabled):
        _engine.Engine.set_profiling(self, enabled)

    def profile(self, name):
        return self._profile((name,))[name]
