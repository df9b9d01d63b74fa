"""Host-side mirror of cv::StereoBM over the C-ABI of lib/libsbm_hip.so (include/sbm.h).

Same names, argument meaning and error behaviour as the interface used at
src/slam/src/core/main.cpp:201-215 of the reference:

    bm = StereoBM.create(16, 9); bm.setPreFilterCap(31); bm.setBlockSize(21); ...; disp = bm.compute(left, right)

`compute` accepts numpy uint8 images (host path, sbm_compute / sbm_compute_batch) or torch CUDA uint8 tensors
(device path, sbm_compute_device; torch is used for device memory only). Parameter errors raise StereoBMError
with the status code and OpenCV's message, where cv::StereoBM::compute would throw cv::Error.

The C-ABI's structures and loader are in _abi.py, the handle and the one path to its device entry points in _engine.py, and
each family beside the dense path in a module of its own (_frontend, _fpga, _gftt, _orb, _match, _pnp, _lk); StereoBM joins them,
and every name is offered from here as before.
"""
import ctypes

import numpy as np

from . import _engine, _fpga, _frontend, _gftt, _lk, _match, _orb, _pnp
from ._abi import (PNP_FEW_MATCHES, PNP_FEW_RANSAC_INLIERS, PNP_FEW_REFINED_INLIERS, PNP_HYP_DTYPE, PNP_NO_MODEL, PNP_OK,  # noqa: F401
                   PNP_RESULT_DTYPE, PREFILTER_FLAVOUR_CV, PREFILTER_FLAVOUR_RTL, PREFILTER_NORMALIZED_RESPONSE, PREFILTER_XSOBEL,
                   FpgaParams, FpgaPlan, GfttCvParams, GfttSelectParams, LK_GET_MIN_EIGENVALS, LK_USE_INITIAL_FLOW, LkParams, MatchParams, MatchPlanInfo, OrbParams, PnpParams, RectCam, SbmParams, StereoBMError,
                   StereoModel, _check, library_path, load_library, loaded_library_name)
from ._fpga import fpga_params, fpga_params_from_regs, fpga_plan, fpga_sad_size_reg, fpga_validate  # noqa: F401
from ._frontend import make_rect_cam  # noqa: F401
from ._gftt import gftt_cv_params, gftt_cv_validate, gftt_select_capacity, gftt_select_params, gftt_select_validate  # noqa: F401
from ._lk import lk_level_sizes, lk_params, lk_validate  # noqa: F401
from ._match import match_params, match_plan, match_validate  # noqa: F401
from ._orb import orb_params, orb_pattern_array, orb_validate  # noqa: F401
from ._pnp import pnp_params, pnp_records, pnp_validate  # noqa: F401


class StereoBM(_engine.Engine, _frontend.FrontEnd, _fpga.FpgaMatcher, _gftt.Gftt, _orb.Orb, _match.Match, _pnp.Pnp, _lk.Lk):
    """cv::StereoBM look-alike. One instance owns one device handle (stream + scratch); not thread-safe."""

    def __init__(self, numDisparities=0, blockSize=21, device=0):
        L = load_library()
        self._p = SbmParams()
        L.sbm_params_default(ctypes.byref(self._p), numDisparities, blockSize)
        self._open(L, self._p, device)

    @staticmethod
    def create(numDisparities=0, blockSize=21, device=0):
        return StereoBM(numDisparities, blockSize, device)

    # ---- the cv::StereoBM / cv::StereoMatcher setters and getters -------------------------------------------
    def _set(self, name, v):
        setattr(self._p, name, int(v))
        _check(self._L.sbm_set_params(self._h, ctypes.byref(self._p)), self._h)

    def setPreFilterType(self, v): self._set("prefilter_type", v)
    def setPreFilterSize(self, v): self._set("prefilter_size", v)
    def setPreFilterCap(self, v): self._set("prefilter_cap", v)
    def setBlockSize(self, v): self._set("block_size", v)
    def setMinDisparity(self, v): self._set("min_disparity", v)
    def setNumDisparities(self, v): self._set("num_disparities", v)
    def setTextureThreshold(self, v): self._set("texture_threshold", v)
    def setUniquenessRatio(self, v): self._set("uniqueness_ratio", v)
    def setSpeckleWindowSize(self, v): self._set("speckle_window_size", v)
    def setSpeckleRange(self, v): self._set("speckle_range", v)
    def setDisp12MaxDiff(self, v): self._set("disp12_max_diff", v)

    def setROI1(self, rect):
        self._p.roi1[:] = [int(v) for v in rect]
        _check(self._L.sbm_set_params(self._h, ctypes.byref(self._p)), self._h)

    def setROI2(self, rect):
        self._p.roi2[:] = [int(v) for v in rect]
        _check(self._L.sbm_set_params(self._h, ctypes.byref(self._p)), self._h)

    def getPreFilterType(self): return self._p.prefilter_type
    def getPreFilterSize(self): return self._p.prefilter_size
    def getPreFilterCap(self): return self._p.prefilter_cap
    def getBlockSize(self): return self._p.block_size
    def getMinDisparity(self): return self._p.min_disparity
    def getNumDisparities(self): return self._p.num_disparities
    def getTextureThreshold(self): return self._p.texture_threshold
    def getUniquenessRatio(self): return self._p.uniqueness_ratio
    def getSpeckleWindowSize(self): return self._p.speckle_window_size
    def getSpeckleRange(self): return self._p.speckle_range
    def getDisp12MaxDiff(self): return self._p.disp12_max_diff
    def getROI1(self): return tuple(self._p.roi1)
    def getROI2(self): return tuple(self._p.roi2)

    def params(self):
        q = SbmParams()
        ctypes.memmove(ctypes.byref(q), ctypes.byref(self._p), ctypes.sizeof(SbmParams))
        return q

    # ---- compute ----------------------------------------------------------------------------------------------
    def compute(self, left, right, disparity=None):
        """cv::StereoBM::compute. numpy (H,W) or (n,H,W) uint8 -> numpy int16; torch CUDA uint8 -> torch CUDA int16."""
        if isinstance(left, np.ndarray):
            return self._compute_host(left, right, disparity)
        return self.compute_device(left, right, disparity)

    def _compute_host(self, left, right, disparity):
        if left.shape != right.shape:
            raise StereoBMError(-2, "All the images must have the same size")
        if left.dtype != np.uint8 or right.dtype != np.uint8:
            raise StereoBMError(-2, "Both input images must have CV_8UC1")
        single = left.ndim == 2
        L3 = left[None] if single else left
        R3 = right[None] if single else right
        if L3.ndim != 3:
            raise StereoBMError(-2, "expected (H,W) or (n,H,W) images")
        n, h, w = L3.shape
        # honour arbitrary row strides like cv::Mat::step, but rows themselves must be dense
        def rows(a):
            if a.strides[-1] != 1:
                a = np.ascontiguousarray(a)
            return a
        L3, R3 = rows(L3), rows(R3)
        out = disparity if disparity is not None else np.empty(L3.shape, np.int16)
        if not isinstance(out, np.ndarray) or out.dtype != np.int16:
            raise StereoBMError(-2, "disparity must be a numpy int16 array")
        out3 = out[None] if out.ndim == 2 else out
        if out3.shape != L3.shape or not out.flags.writeable:
            raise StereoBMError(-2, f"disparity has shape {out.shape}, the images {left.shape}")
        # strides travel to C as size_t: rows must be dense and every row stride positive and at least one row long
        for a, item in ((L3, 1), (R3, 1), (out3, 2)):
            if a.strides[-1] != item or a.strides[-2] < a.shape[-1] * item or (a.ndim == 3 and a.shape[0] > 1 and a.strides[0] <= 0):
                raise StereoBMError(-2, "rows must be dense with a positive row stride (negative or overlapping strides are not supported)")
        vp = ctypes.c_void_p
        lp = (vp * n)(*[L3[i].ctypes.data for i in range(n)])
        rp = (vp * n)(*[R3[i].ctypes.data for i in range(n)])
        dp = (vp * n)(*[out3[i].ctypes.data for i in range(n)])
        _check(self._L.sbm_compute_batch(self._h, n, lp, L3.strides[-2], rp, R3.strides[-2], w, h, dp, out3.strides[-2]),
               self._h)
        return out[0] if (single and disparity is None) else out

    def submit_host(self, left, right, disparity):
        """sbm_submit_dense: queue one dense (n,H,W) uint8 batch in (pinned) host memory; `disparity` (n,H,W) int16 is filled
        when the matching wait_host() returns. At most three submissions are in flight. Dropping the engine with submissions
        outstanding drains them first (close()); the bare C call sbm_destroy() would drop the newest submission's maps."""
        for a, dt in ((left, np.uint8), (right, np.uint8), (disparity, np.int16)):
            if not isinstance(a, np.ndarray) or a.dtype != dt or a.ndim != 3 or not a.flags.c_contiguous:
                raise StereoBMError(-2, "submit_host takes C-contiguous (n,H,W) arrays: uint8 images, int16 disparity")
        if left.shape != right.shape or left.shape != disparity.shape:
            raise StereoBMError(-2, "All the images must have the same size")
        n, h, w = left.shape
        # The engine drains to at most two outstanding submissions INSIDE this call, before it queues the new one: only once
        # it has returned are the oldest submissions' copies known to be complete, so their arrays are released afterwards.
        _check(self._L.sbm_submit_dense(self._h, n, left.ctypes.data, right.ctypes.data, w, h, disparity.ctypes.data), self._h)
        while len(self._host_inflight) > 2:
            self._host_inflight.popleft()
        self._host_inflight.append((left, right, disparity))

    def wait_host(self):
        """sbm_wait_oldest: block until the oldest outstanding submit_host() has delivered its maps."""
        _check(self._L.sbm_wait_oldest(self._h), self._h)
        if self._host_inflight:
            self._host_inflight.popleft()     # its arrays are the caller's again

    def compute_device(self, left, right, disparity=None, sync=True):
        """Device-resident batch: torch CUDA uint8 tensors (n,H,W) or (H,W), contiguous. Returns a torch int16 tensor."""
        return self._compute_device(self._L.sbm_compute_device, (), left, right, disparity, sync)

    def launch_raw(self, n, d_left, d_right, w, h, d_disp, sync=False):
        """Thin call of sbm_compute_device on raw device addresses (used by bench.py's timed loop)."""
        _check(self._L.sbm_compute_device(self._h, n, d_left, d_right, w, h, d_disp, 1 if sync else 0), self._h)

    def stream(self):
        return self._L.sbm_stream(self._h)

    def last_kernel(self):
        """Template instantiation of the SAD kernel the last compute call launched (sbm_last_kernel_name)."""
        buf = ctypes.create_string_buffer(128)
        _check(self._L.sbm_last_kernel_name(self._h, buf, 128), self._h)
        return buf.value.decode()

    def profile(self):
        return self._profile(("prefilter", "sad", "lrcheck", "speckle", "total"))

    def debug_fetch(self, which, n=0, h=0, w=0):
        """Planes of the last device call: 0 / 1 the prefiltered images, 2 the cost plane, 3 the map before the LR check, each
        (n, h, w); 7 the hand-off of the interior SAD kernel's vertical sums: int32 (row segments x pairs x strips that took
        their sums over, those that could have)."""
        dt = {0: np.uint8, 1: np.uint8, 2: np.int32, 3: np.int16, 7: np.int32}[which]
        a = np.empty((2,) if which == 7 else (n, h, w), dt)
        _check(self._L.sbm_debug_fetch(self._h, which, a.ctypes.data, a.nbytes), self._h)
        return a

    POSTFILTER_INFO = ("stages", "lr_kernel", "nit", "px", "bs", "cost16", "speckle", "lists", "G", "S", "SW", "max_diff",
                       "row0", "row1", "col0", "col1", "lofs", "xend")
    LR_COPY, LR_FAST16, LR_GENERIC_LDS, LR_GENERIC_GLOBAL = 0, 1, 2, 3

    def debug_postfilter(self, pre, cost=None, stages=3):
        """sbm_debug_postfilter (for the tests): this matcher's post-filters on the caller's (n,H,W) or (H,W) int16 map and int32
        costs (None where nothing reads them), planned as compute() plans them. stages: 1 = LR check + valid-ROI fill,
        2 = speckle filter on the whole map, 3 = both. Returns (map, info) with info a dict over POSTFILTER_INFO."""
        pre = np.ascontiguousarray(pre, np.int16)
        single = pre.ndim == 2
        p3 = pre[None] if single else pre
        if p3.ndim != 3:
            raise StereoBMError(-2, "expected an (H,W) or (n,H,W) map")
        if cost is not None:
            cost = np.ascontiguousarray(cost, np.int32)
            if cost.size != p3.size:
                raise StereoBMError(-2, "the cost plane must have the map's size")
        n, h, w = p3.shape
        out = np.empty_like(p3)
        info = np.zeros(len(self.POSTFILTER_INFO), np.int32)
        _check(self._L.sbm_debug_postfilter(self._h, n, w, h, p3.ctypes.data, None if cost is None else cost.ctypes.data, int(stages),
                                            out.ctypes.data, info.ctypes.data, info.size), self._h)
        return (out[0] if single else out), dict(zip(self.POSTFILTER_INFO, info.tolist()))


def compute_multi(engines, left, right, disparity):
    """sbm_compute_batch_multi: one dense (n,H,W) uint8 host batch over several StereoBM engines (normally one per GPU),
    contiguous pair blocks, maps delivered into `disparity` (n,H,W) int16 in place. Host memory should be pinned."""
    for a, dt in ((left, np.uint8), (right, np.uint8), (disparity, np.int16)):
        if not isinstance(a, np.ndarray) or a.dtype != dt or a.ndim != 3 or not a.flags.c_contiguous:
            raise StereoBMError(-2, "compute_multi takes C-contiguous (n,H,W) arrays: uint8 images, int16 disparity")
    if left.shape != right.shape or left.shape != disparity.shape:
        raise StereoBMError(-2, "All the images must have the same size")
    if not engines:
        raise StereoBMError(-24, "compute_multi needs at least one engine")
    n, h, w = left.shape
    L = load_library()
    hs = (ctypes.c_void_p * len(engines))(*[e._h for e in engines])
    _check(L.sbm_compute_batch_multi(hs, len(engines), n, left.ctypes.data, right.ctypes.data, w, h, disparity.ctypes.data), engines[0]._h)
    return disparity


def trim():
    """Free the handles parked by destroyed matchers (see sbm_trim in include/sbm.h)."""
    load_library().sbm_trim()


def validate(params, width, height):
    """Status code of cv::StereoBM::compute's parameter checks (0 = ok)."""
    return load_library().sbm_params_validate(ctypes.byref(params), width, height)
