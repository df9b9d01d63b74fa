"""Host-side mirror of cv::StereoBM over the C-ABI of lib/libsbm_hip.so (include/sbm.h).

Same names, argument meaning and error behaviour as the interface used at
src/slam/src/core/main.cpp:201-215 of the reference:

    bm = StereoBM.create(16, 9); bm.setPreFilterCap(31); bm.setBlockSize(21); ...; disp = bm.compute(left, right)

`compute` accepts numpy uint8 images (host path, sbm_compute / sbm_compute_batch) or torch CUDA uint8 tensors
(device path, sbm_compute_device; torch is used for device memory only). Parameter errors raise StereoBMError
with the status code and OpenCV's message, where cv::StereoBM::compute would throw cv::Error.
"""
import collections
import ctypes
import os
import pathlib

import numpy as np

PREFILTER_NORMALIZED_RESPONSE = 0
PREFILTER_XSOBEL = 1

_HERE = pathlib.Path(__file__).resolve().parent
_LIB = None


class SbmParams(ctypes.Structure):
    """`sbm_params` of include/sbm.h."""

    _fields_ = [
        ("prefilter_type", ctypes.c_int32), ("prefilter_size", ctypes.c_int32), ("prefilter_cap", ctypes.c_int32),
        ("block_size", ctypes.c_int32), ("min_disparity", ctypes.c_int32), ("num_disparities", ctypes.c_int32),
        ("texture_threshold", ctypes.c_int32), ("uniqueness_ratio", ctypes.c_int32),
        ("speckle_window_size", ctypes.c_int32), ("speckle_range", ctypes.c_int32), ("disp12_max_diff", ctypes.c_int32),
        ("roi1", ctypes.c_int32 * 4), ("roi2", ctypes.c_int32 * 4),
    ]


class StereoModel(ctypes.Structure):
    """`sbm_stereo_model` of include/sbm.h: the StereoCameraModel entries the reference's reprojection reads
    (include/core/StereoCameraModel.h:25-34) plus the optional local transform."""

    _fields_ = [(k, ctypes.c_double) for k in ("fx_l", "fy_l", "cx_l", "cy_l", "Tx_l", "fx_r", "fy_r", "cx_r", "Tx_r")] + [
        ("local", ctypes.c_float * 12), ("has_local", ctypes.c_int32)]


class RectCam(ctypes.Structure):
    """`sbm_rect_cam` of include/sbm.h = struct RECT_PARAM_CH (src/StereoBM/src/fpga.h:250-256), one camera."""

    _fields_ = [("f", ctypes.c_int32 * 2), ("c", ctypes.c_int32 * 2), ("f2inv", ctypes.c_int32 * 2),
                ("c2_f2", ctypes.c_int32 * 2), ("rot", (ctypes.c_int32 * 3) * 3)]


def make_rect_cam(f, c, f2inv, c2_f2, rot):
    cam = RectCam()
    cam.f[:] = [int(v) for v in f]
    cam.c[:] = [int(v) for v in c]
    cam.f2inv[:] = [int(v) for v in f2inv]
    cam.c2_f2[:] = [int(v) for v in c2_f2]
    for r in range(3):
        for k in range(3):
            cam.rot[r][k] = int(rot[r][k])
    return cam


PREFILTER_FLAVOUR_CV = 0
PREFILTER_FLAVOUR_RTL = 1


class FpgaParams(ctypes.Structure):
    """`sbm_fpga_params` of include/sbm.h: the fields of the BM register block (struct FPGA_REG_BM,
    src/StereoBM/src/fpga.h:154-169) as decoded by src/dvp/rtl/bm.v:172-193."""

    _fields_ = [(k, ctypes.c_int32) for k in ("width", "height", "block_size", "num_disparities", "uni_enable", "uni_mode",
                                              "uni_threshold")]


def fpga_params(width, height, block_size=21, num_disparities=64, uni_enable=0, uni_mode=0, uni_threshold=0):
    return FpgaParams(width, height, block_size, num_disparities, uni_enable, uni_mode, uni_threshold)


def fpga_params_from_regs(image_size, bm_setting, uni_filt_ctrl=0):
    """ImageSize [1708h], BmSetting [170Ch], UniFiltCtrl [1728h] -> FpgaParams (firmware: fpga.c:155,158)."""
    q = FpgaParams()
    _check(load_library().sbm_fpga_params_from_regs(image_size, bm_setting, uni_filt_ctrl, ctypes.byref(q)))
    return q


def fpga_sad_size_reg(params):
    """Read-back value of SAD_Size [1724h] (bm.v:208)."""
    return int(load_library().sbm_fpga_sad_size_reg(ctypes.byref(params)))


def fpga_validate(params):
    return int(load_library().sbm_fpga_params_validate(ctypes.byref(params)))


class GfttSelectParams(ctypes.Structure):
    """`sbm_gftt_select_params` of include/sbm.h: generateKeypoints2's constants (src/slam/src/core/GFTT.cpp:50-53)."""

    _fields_ = [("max_features", ctypes.c_int32), ("quality_level", ctypes.c_double), ("min_distance", ctypes.c_double),
                ("block_size", ctypes.c_int32)]


def gftt_select_params(max_features=1500, quality_level=0.01, min_distance=7.0, block_size=3):
    """The reference's constants by default."""
    return GfttSelectParams(int(max_features), float(quality_level), float(min_distance), int(block_size))


def gftt_select_validate(params, width, height):
    """Status code of sbm_gftt_select_params_validate (0 = ok)."""
    return load_library().sbm_gftt_select_params_validate(ctypes.byref(params), width, height)


def gftt_select_capacity(params, width, height):
    """Points per image slot: max_features, or every interior pixel when max_features <= 0."""
    return params.max_features if params.max_features > 0 else (width - 2) * (height - 2)


class GfttCvParams(ctypes.Structure):
    """`sbm_gftt_cv_params` of include/sbm.h: cv::GFTTDetector::create's arguments (src/slam/src/core/GFTT.cpp:13-24)."""

    _fields_ = [("max_features", ctypes.c_int32), ("quality_level", ctypes.c_double), ("min_distance", ctypes.c_double),
                ("block_size", ctypes.c_int32), ("use_harris", ctypes.c_int32), ("k", ctypes.c_double)]


def gftt_cv_params(max_features=1500, quality_level=0.01, min_distance=7.0, block_size=3, use_harris=False, k=0.04):
    """The reference's constants by default."""
    return GfttCvParams(int(max_features), float(quality_level), float(min_distance), int(block_size), int(bool(use_harris)),
                        float(k))


def gftt_cv_validate(params, width, height):
    """Status code of sbm_gftt_cv_params_validate (0 = ok)."""
    return load_library().sbm_gftt_cv_params_validate(ctypes.byref(params), width, height)


class OrbParams(ctypes.Structure):
    """`sbm_orb_params` of include/sbm.h: computeDescriptor's constants (src/slam/src/opencv/CvORB.cpp) and the keypoints' angle."""

    _fields_ = [("edge_threshold", ctypes.c_int32), ("angle", ctypes.c_float), ("blur_ksize", ctypes.c_int32),
                ("blur_sigma", ctypes.c_double)]


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


class MatchParams(ctypes.Structure):
    """`sbm_match_params` of include/sbm.h: the NNDR ratio and guided radius of computeTransform's matching (Registration.cpp)."""

    _fields_ = [("nndr", ctypes.c_float), ("radius", ctypes.c_float)]


def match_params(nndr=0.8, radius=40.0):
    """The reference's values by default."""
    return MatchParams(float(nndr), float(radius))


def match_validate(params):
    """Status code of sbm_match_params_validate (0 = ok)."""
    return load_library().sbm_match_params_validate(ctypes.byref(params))


class PnpParams(ctypes.Structure):
    """`sbm_pnp_params` of include/sbm.h: estimateMotion's minInliers, refineIterations and solvePnPRansac's constants."""

    _fields_ = [("min_inliers", ctypes.c_int32), ("refine_iterations", ctypes.c_int32), ("iterations", ctypes.c_int32),
                ("reprojection_error", ctypes.c_float), ("refine_sigma", ctypes.c_float), ("pad", ctypes.c_int32),
                ("confidence", ctypes.c_double)]


def pnp_params(min_inliers=20, refine_iterations=1, iterations=300, reprojection_error=2.0, refine_sigma=3.0, confidence=0.99):
    """The reference's values by default."""
    return PnpParams(int(min_inliers), int(refine_iterations), int(iterations), float(reprojection_error), float(refine_sigma), 0,
                     float(confidence))


def pnp_validate(params):
    """Status code of sbm_pnp_params_validate (0 = ok)."""
    return load_library().sbm_pnp_params_validate(ctypes.byref(params))


# `sbm_pnp_result` (216 bytes) and `sbm_pnp_hypothesis` (128 bytes) as numpy record types
PNP_RESULT_DTYPE = np.dtype([("status", "<i4"), ("num_matches", "<i4"), ("num_inliers", "<i4"), ("ransac_inliers", "<i4"),
                             ("best_iteration", "<i4"), ("niters", "<i4"), ("refine_solves", "<i4"), ("refine_exit", "<i4"),
                             ("rvec", "<f8", 3), ("tvec", "<f8", 3), ("R", "<f8", 9), ("cov_dist", "<f8"), ("cov_angle", "<f8"),
                             ("transform", "<f4", 12)])
PNP_HYP_DTYPE = np.dtype([("subset", "<i4", 6), ("count", "<i4"), ("pad", "<i4"), ("R", "<f8", 9), ("t", "<f8", 3)])
PNP_OK, PNP_FEW_MATCHES, PNP_NO_MODEL, PNP_FEW_RANSAC_INLIERS, PNP_FEW_REFINED_INLIERS = 0, 1, 2, 3, 4


def pnp_records(t, dtype=None):
    """Device or host bytes of sbm_pnp_result (or, with dtype=PNP_HYP_DTYPE, sbm_pnp_hypothesis) records -> numpy records."""
    dtype = PNP_RESULT_DTYPE if dtype is None else dtype
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=dtype).reshape(a.shape[:-1])


def _jobs_array(jobs):
    j = np.ascontiguousarray(np.asarray(jobs, dtype=np.int32).reshape(-1, 2))
    if j.shape[0] == 0:
        raise StereoBMError(-24, "no jobs")
    return j


class StereoBMError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"sbm status {code}: {message}")
        self.code = code


def library_path():
    """lib/libsbm_hip.so, or -- SBM_LIB_AB=<file name> -- another build of the same HIP engine inside lib/ for kernel A/B
    runs. Only a bare libsbm_hip*.so name is accepted and the file must exist: never a fallback, never a path."""
    name = os.environ.get("SBM_LIB_AB", "libsbm_hip.so")
    if name != os.path.basename(name) or not (name.startswith("libsbm_hip") and name.endswith(".so")):
        raise ImportError(f"SBM_LIB_AB={name!r}: expected the bare name of a libsbm_hip*.so inside {_HERE / 'lib'}")
    return _HERE / "lib" / name


def loaded_library_name():
    """File name of the engine library this process uses (bench.py prints it)."""
    return library_path().name


def load_library():
    """Load lib/libsbm_hip.so. Fails loudly when it has not been built (no fallback of any kind)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch ships its own HIP runtime; when both live in one process it must be the first one loaded so that
    # libsbm_hip.so binds to the same runtime (device memory and streams are shared with torch).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = library_path()
    if not path.exists():
        raise ImportError(f"{path} is missing: build it with `make` (or __graft_entry__.build()); "
                          "this package has no CPU fallback")
    L = ctypes.CDLL(str(path))
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    pp = ctypes.POINTER(SbmParams)
    L.sbm_params_default.argtypes = [pp, ci, ci]
    L.sbm_params_default.restype = None
    L.sbm_params_validate.argtypes = [pp, ci, ci]
    L.sbm_create.argtypes = [ctypes.POINTER(vp), pp, ci]
    L.sbm_destroy.argtypes = [vp]
    L.sbm_destroy.restype = None
    L.sbm_set_params.argtypes = [vp, pp]
    L.sbm_get_params.argtypes = [vp, pp]
    L.sbm_compute.argtypes = [vp, vp, sz, vp, sz, ci, ci, vp, sz]
    L.sbm_compute_batch.argtypes = [vp, ci, ctypes.POINTER(vp), sz, ctypes.POINTER(vp), sz, ci, ci, ctypes.POINTER(vp), sz]
    L.sbm_compute_device.argtypes = [vp, ci, vp, vp, ci, ci, vp, ci]
    L.sbm_synchronize.argtypes = [vp]
    L.sbm_submit_dense.argtypes = [vp, ci, vp, vp, ci, ci, vp]
    L.sbm_wait_oldest.argtypes = [vp]
    L.sbm_compute_batch_multi.argtypes = [ctypes.POINTER(vp), ci, ci, vp, vp, ci, ci, vp]
    L.sbm_debug_fetch.argtypes = [vp, ci, vp, sz]
    L.sbm_set_profiling.argtypes = [vp, ci]
    L.sbm_get_profile.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_float)]
    L.sbm_last_kernel_name.argtypes = [vp, ctypes.c_char_p, sz]
    mp = ctypes.POINTER(StereoModel)
    L.sbm_disparity_to_float_device.argtypes = [vp, ci, vp, ci, ci, vp, ci]
    L.sbm_decimate_device.argtypes = [vp, ci, vp, ci, ci, ci, vp, ci]
    L.sbm_reproject_device.argtypes = [vp, ci, vp, ci, ci, ci, mp, ci, vp, ci]
    L.sbm_keypoints3d_device.argtypes = [vp, vp, ci, ci, vp, ci, mp, ctypes.c_float, ctypes.c_float, vp, ci]
    L.sbm_rect_map_device.argtypes = [vp, ctypes.POINTER(RectCam), ci, ci, vp, ci]
    L.sbm_rect_remap_device.argtypes = [vp, ci, vp, vp, ci, ci, vp, ci]
    L.sbm_prefilter_device.argtypes = [vp, ci, vp, ci, ci, ci, ci, vp, ci]
    fp = ctypes.POINTER(FpgaParams)
    u32 = ctypes.c_uint32
    L.sbm_fpga_params_from_regs.argtypes = [u32, u32, u32, fp]
    L.sbm_fpga_sad_size_reg.argtypes = [fp]
    L.sbm_fpga_sad_size_reg.restype = u32
    L.sbm_fpga_params_validate.argtypes = [fp]
    L.sbm_fpga_bm_device.argtypes = [vp, ci, vp, vp, fp, vp, ci]
    L.sbm_fpga_compute_device.argtypes = [vp, ci, vp, vp, fp, vp, ci]
    L.sbm_gftt_eig_device.argtypes = [vp, ci, vp, ci, ci, vp, vp, ci]
    L.sbm_fpga_compute.argtypes = [vp, vp, sz, vp, sz, fp, vp, sz]
    L.sbm_gftt_eig.argtypes = [vp, vp, sz, ci, ci, vp, sz, ctypes.POINTER(u32)]
    gp = ctypes.POINTER(GfttSelectParams)
    L.sbm_gftt_select_params_default.argtypes = [gp]
    L.sbm_gftt_select_params_default.restype = None
    L.sbm_gftt_select_params_validate.argtypes = [gp, ci, ci]
    L.sbm_gftt_select_device.argtypes = [vp, ci, vp, vp, ci, ci, gp, vp, vp, ci]
    L.sbm_gftt_select.argtypes = [vp, vp, sz, ci, ci, ctypes.c_uint16, gp, vp, sz, ctypes.POINTER(ctypes.c_int)]
    L.sbm_gftt_detect_device.argtypes = [vp, ci, vp, ci, ci, gp, vp, vp, vp, vp, ci]
    gcp = ctypes.POINTER(GfttCvParams)
    L.sbm_gftt_cv_params_default.argtypes = [gcp]
    L.sbm_gftt_cv_params_default.restype = None
    L.sbm_gftt_cv_params_validate.argtypes = [gcp, ci, ci]
    L.sbm_gftt_cv_eig_device.argtypes = [vp, ci, vp, ci, ci, vp, vp, ci]
    L.sbm_gftt_cv_detect_device.argtypes = [vp, ci, vp, ci, ci, gcp, vp, vp, vp, vp, ci]
    L.sbm_gftt_cv_select_device.argtypes = [vp, ci, vp, vp, ci, ci, gcp, vp, vp, ci]
    L.sbm_gftt_cv_detect.argtypes = [vp, vp, sz, ci, ci, gcp, vp, sz, ctypes.POINTER(ctypes.c_int)]
    op = ctypes.POINTER(OrbParams)
    L.sbm_orb_params_default.argtypes = [op]
    L.sbm_orb_params_default.restype = None
    L.sbm_orb_params_validate.argtypes = [op]
    L.sbm_orb_describe_device.argtypes = [vp, ci, vp, ci, ci, ci, vp, vp, vp, op, vp, vp, vp, vp, ci]
    L.sbm_orb_describe.argtypes = [vp, vp, sz, ci, ci, vp, ci, vp, op, vp, ctypes.POINTER(ctypes.c_int), vp]
    L.sbm_orb_features_device.argtypes = [vp, ci, vp, ci, ci, gp, vp, op, vp, vp, vp, vp, vp, vp, ci]
    L.sbm_orb_features_cv_device.argtypes = [vp, ci, vp, ci, ci, gcp, vp, op, vp, vp, vp, vp, vp, vp, ci]
    mp_ = ctypes.POINTER(MatchParams)
    L.sbm_match_params_default.argtypes = [mp_]
    L.sbm_match_params_default.restype = None
    L.sbm_match_params_validate.argtypes = [mp_]
    L.sbm_match_device.argtypes = [vp, ci, ci, vp, vp, vp, ci, mp_, vp, vp, vp, ci]
    L.sbm_match_guess_device.argtypes = [vp, ci, ci, vp, vp, vp, ci, vp, vp, mp_, vp, vp, vp, ci]
    L.sbm_project_points_device.argtypes = [vp, ci, ci, vp, vp, vp, ci, vp, vp, ci, ci, vp, ci]
    L.sbm_match.argtypes = [vp, vp, sz, ci, vp, sz, ci, mp_, vp, ctypes.POINTER(ci)]
    L.sbm_match_guess.argtypes = [vp, vp, vp, vp, sz, ci, vp, sz, ci, vp, vp, ci, ci, mp_, vp, ctypes.POINTER(ci)]
    pp_ = ctypes.POINTER(PnpParams)
    L.sbm_pnp_params_default.argtypes = [pp_]
    L.sbm_pnp_params_default.restype = None
    L.sbm_pnp_params_validate.argtypes = [pp_]
    L.sbm_estimate_motion_device.argtypes = [vp, ci, ci, vp, vp, vp, vp, ci, vp, vp, vp, mp, pp_, vp, vp, vp, ci]
    L.sbm_estimate_motion.argtypes = [vp, vp, ci, vp, vp, ci, vp, ci, vp, mp, pp_, vp, vp]
    L.sbm_stream.argtypes = [vp]
    L.sbm_stream.restype = vp
    L.sbm_strerror.argtypes = [ci]
    L.sbm_strerror.restype = ctypes.c_char_p
    L.sbm_last_hip_error.argtypes = [vp]
    L.sbm_version.restype = ci
    _LIB = L
    return L


def _check(code, handle=None):
    if code != 0:
        L = load_library()
        msg = L.sbm_strerror(code).decode()
        if code == -21 and handle:
            msg += f" (hipError {L.sbm_last_hip_error(handle)})"
        raise StereoBMError(code, msg)


class StereoBM:
    """cv::StereoBM look-alike. One instance owns one device handle (stream + scratch); not thread-safe."""

    def __init__(self, numDisparities=0, blockSize=21, device=0):
        L = load_library()
        self._L = L
        self._p = SbmParams()
        L.sbm_params_default(ctypes.byref(self._p), numDisparities, blockSize)
        self._h = ctypes.c_void_p()
        self._device = device
        self._inflight = []                   # buffers of asynchronous compute_device calls, until synchronize()
        self._host_inflight = collections.deque()   # (left, right, disparity) of submit_host, oldest first
        _check(L.sbm_create(ctypes.byref(self._h), ctypes.byref(self._p), device))

    @staticmethod
    def create(numDisparities=0, blockSize=21, device=0):
        return StereoBM(numDisparities, blockSize, device)

    def close(self):
        """Release the engine. Outstanding submit_host() submissions are drained first (sbm_synchronize) while their arrays are
        still referenced here, so every submitted `disparity` array is filled -- sbm_destroy on its own would let the queued
        copies finish and DROP the maps of the newest submission (include/sbm.h, "sbm_destroy() and the asynchronous feed")."""
        h = getattr(self, "_h", None)
        if h:
            if getattr(self, "_host_inflight", None):
                self._L.sbm_synchronize(h)
                self._host_inflight.clear()
            self._L.sbm_destroy(h)
            self._h = None

    def __del__(self):
        self.close()

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
        import torch

        if left.shape != right.shape:
            raise StereoBMError(-2, "All the images must have the same size")
        if left.dtype != torch.uint8 or right.dtype != torch.uint8 or not left.is_cuda or not right.is_cuda:
            raise StereoBMError(-2, "Both input images must be CUDA uint8 tensors")
        if left.device.index != self._device:
            raise StereoBMError(-20, f"tensor on cuda:{left.device.index}, engine on device {self._device}")
        if left.dim() not in (2, 3):
            raise StereoBMError(-2, "expected (H,W) or (n,H,W) images")
        left, right = left.contiguous(), right.contiguous()
        shape = left.shape
        n = 1 if left.dim() == 2 else shape[0]
        h, w = shape[-2], shape[-1]
        if disparity is None:
            disparity = torch.empty(shape, dtype=torch.int16, device=left.device)
        elif (not isinstance(disparity, torch.Tensor) or disparity.dtype != torch.int16 or not disparity.is_cuda
              or disparity.device != left.device or tuple(disparity.shape) != tuple(shape) or not disparity.is_contiguous()):
            # the C-ABI writes n*h*w int16 through the raw pointer: anything else would be an out-of-bounds / strided-wrong write
            raise StereoBMError(-2, f"disparity must be a contiguous CUDA int16 tensor of shape {tuple(shape)} on {left.device}")
        # the engine runs on its own (non-blocking) stream: order it behind whatever produced the inputs
        torch.cuda.current_stream(left.device).synchronize()
        _check(self._L.sbm_compute_device(self._h, n, left.data_ptr(), right.data_ptr(), w, h, disparity.data_ptr(),
                                          1 if sync else 0), self._h)
        if not sync:
            # torch's caching allocator only knows its own streams: without this the .contiguous() temporaries and a
            # freshly allocated output could be handed out again while the engine's kernels still use them
            # (a list: back-to-back asynchronous calls each keep their buffers until the next synchronize())
            self._inflight.append((left, right, disparity))
        else:
            # a synchronous call drains the engine's compute stream: earlier asynchronous DEVICE calls are done too
            # (host submissions keep their arrays: their maps may still be on the way home on the copy stream)
            self._inflight.clear()
        return disparity

    def _check_device_images(self, *tensors):
        """Every image handed to the engine as a raw pointer: CUDA uint8, on the handle's device, (H,W) or (n,H,W)."""
        import torch

        for t in tensors:
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or not t.is_cuda:
                raise StereoBMError(-2, "images must be CUDA uint8 tensors")
            if t.device.index != self._device:
                raise StereoBMError(-20, f"tensor on cuda:{t.device.index}, engine on device {self._device}")
            if t.dim() not in (2, 3):
                raise StereoBMError(-2, "expected (H,W) or (n,H,W) images")

    def launch_raw(self, n, d_left, d_right, w, h, d_disp, sync=False):
        """Thin call of sbm_compute_device on raw device addresses (used by bench.py's timed loop)."""
        _check(self._L.sbm_compute_device(self._h, n, d_left, d_right, w, h, d_disp, 1 if sync else 0), self._h)

    # ---- consumers of the map (SensorData.cpp:50-58, Stereo.cpp:53-117,157-199, main.cpp:522-553) ----------------
    def to_float(self, disp):
        """CV_32F form of a torch CUDA int16 disparity tensor: disp / 16 as float32 (cv convertTo(CV_32F, 1/16))."""
        import torch

        disp = disp.contiguous()
        h, w = disp.shape[-2], disp.shape[-1]
        n = 1 if disp.dim() == 2 else disp.shape[0]
        out = torch.empty(disp.shape, dtype=torch.float32, device=disp.device)
        torch.cuda.current_stream(disp.device).synchronize()
        _check(self._L.sbm_disparity_to_float_device(self._h, n, disp.data_ptr(), w, h, out.data_ptr(), 1), self._h)
        return out

    def decimate(self, disp, scale=4):
        """torch CUDA int16 (n,H,W) or (H,W) -> every scale-th pixel, on the device."""
        import torch

        d3 = disp if disp.dim() == 3 else disp[None]
        d3 = d3.contiguous()
        n, h, w = d3.shape
        out = torch.empty((n, h // scale, w // scale), dtype=torch.int16, device=d3.device)
        torch.cuda.current_stream(d3.device).synchronize()
        _check(self._L.sbm_decimate_device(self._h, n, d3.data_ptr(), w, h, scale, out.data_ptr(), 1), self._h)
        return out if disp.dim() == 3 else out[0]

    def reproject(self, disp, model, scale=1, apply_local=True):
        """torch CUDA int16 map(s) -> float32 (..., H, W, 3) points, NaN where invalid."""
        import torch

        d3 = disp if disp.dim() == 3 else disp[None]
        d3 = d3.contiguous()
        n, h, w = d3.shape
        xyz = torch.empty((n, h, w, 3), dtype=torch.float32, device=d3.device)
        torch.cuda.current_stream(d3.device).synchronize()
        _check(self._L.sbm_reproject_device(self._h, n, d3.data_ptr(), w, h, scale, ctypes.byref(model),
                                            1 if apply_local else 0, xyz.data_ptr(), 1), self._h)
        return xyz if disp.dim() == 3 else xyz[0]

    def keypoints3d(self, disp, kpts, model, min_depth=0.0, max_depth=0.0):
        """One full-resolution torch CUDA int16 map + float32 (nk,2) keypoints (x,y) -> float32 (nk,3)."""
        import torch

        disp = disp.contiguous()
        kpts = kpts.contiguous()
        h, w = disp.shape
        xyz = torch.empty((kpts.shape[0], 3), dtype=torch.float32, device=disp.device)
        torch.cuda.current_stream(disp.device).synchronize()
        _check(self._L.sbm_keypoints3d_device(self._h, disp.data_ptr(), w, h, kpts.data_ptr(), kpts.shape[0],
                                              ctypes.byref(model), min_depth, max_depth, xyz.data_ptr(), 1), self._h)
        return xyz

    # ---- producers in front of the path (fpga.c:303-366, rect_intp.v:285-404, xsbl2.v:661-874) --------------------
    def rect_map(self, cam, width, height):
        """Inverse rectification map of one camera: torch CUDA int16 (H, W, 2), (x, y) in 1/32 source pixels."""
        import torch

        m = torch.empty((height, width, 2), dtype=torch.int16, device=f"cuda:{self._device}")
        _check(self._L.sbm_rect_map_device(self._h, ctypes.byref(cam), width, height, m.data_ptr(), 1), self._h)
        return m

    def rect_remap(self, src, rmap):
        """torch CUDA uint8 (n,H,W) or (H,W) raw frames + a map from rect_map -> rectified frames, on the device."""
        import torch

        src, rmap = src.contiguous(), rmap.contiguous()
        h, w = src.shape[-2], src.shape[-1]
        if tuple(rmap.shape) != (h, w, 2) or rmap.dtype != torch.int16 or src.dtype != torch.uint8:
            raise StereoBMError(-2, "map must be int16 (H,W,2) and frames uint8 (..,H,W)")
        n = 1 if src.dim() == 2 else src.shape[0]
        out = torch.empty_like(src)
        torch.cuda.current_stream(src.device).synchronize()
        _check(self._L.sbm_rect_remap_device(self._h, n, src.data_ptr(), rmap.data_ptr(), w, h, out.data_ptr(), 1), self._h)
        return out

    def prefilter(self, src, flavour=PREFILTER_FLAVOUR_CV, cap=None):
        """Stand-alone x-Sobel prefilter of torch CUDA uint8 (n,H,W) or (H,W) frames, cv or RTL flavour."""
        import torch

        self._check_device_images(src)
        src = src.contiguous()
        h, w = src.shape[-2], src.shape[-1]
        n = 1 if src.dim() == 2 else src.shape[0]
        out = torch.empty_like(src)
        torch.cuda.current_stream(src.device).synchronize()
        _check(self._L.sbm_prefilter_device(self._h, n, src.data_ptr(), w, h, flavour,
                                            self._p.prefilter_cap if cap is None else cap, out.data_ptr(), 1), self._h)
        return out

    # ---- the reference's own matcher: FPGA flavour (src/dvp/rtl/bm*.v; FPGA.cpp:270-279 consumers) ---------------------
    def _fpga(self, fn, a, b, params):
        import torch

        self._check_device_images(a, b)
        if a.shape != b.shape:
            raise StereoBMError(-2, "both inputs must be CUDA uint8 tensors of the same shape")
        a, b = a.contiguous(), b.contiguous()
        h, w = a.shape[-2], a.shape[-1]
        if (w, h) != (params.width, params.height):
            raise StereoBMError(-2, f"images are {w}x{h}, ImageSize says {params.width}x{params.height}")
        n = 1 if a.dim() == 2 else a.shape[0]
        out = torch.empty(a.shape, dtype=torch.int16, device=a.device)
        torch.cuda.current_stream(a.device).synchronize()
        _check(fn(self._h, n, a.data_ptr(), b.data_ptr(), ctypes.byref(params), out.data_ptr(), 1), self._h)
        return out

    def fpga_bm(self, xsbl_l, xsbl_r, params):
        """RTL block matcher on x-Sobel planes (torch CUDA uint8, (n,H,W) or (H,W)) -> int16 s11.4, -1 = none."""
        return self._fpga(self._L.sbm_fpga_bm_device, xsbl_l, xsbl_r, params)

    def fpga_compute(self, left, right, params):
        """xsbl2.v prefilter + RTL block matcher on rectified frames: the PL pipeline behind Fpga::receiveDepthMap."""
        return self._fpga(self._L.sbm_fpga_compute_device, left, right, params)

    def fpga_compute_host(self, left, right, params):
        """numpy uint8 (H,W) rectified pair -> numpy int16 (H,W): the frame Fpga::receiveDepthMap would hand out."""
        if left.shape != right.shape or left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim != 2:
            raise StereoBMError(-2, "both inputs must be (H,W) uint8 arrays of the same shape")
        if left.strides[1] != 1 or right.strides[1] != 1 or left.strides[0] < left.shape[1] or right.strides[0] < right.shape[1]:
            raise StereoBMError(-2, "rows must be dense with a positive row stride")
        out = np.empty(left.shape, np.int16)
        _check(self._L.sbm_fpga_compute(self._h, left.ctypes.data, left.strides[0], right.ctypes.data, right.strides[0],
                                        ctypes.byref(params), out.ctypes.data, out.strides[0]), self._h)
        return out

    def gftt_eig_host(self, img):
        """numpy uint8 (H,W) -> (numpy uint16 map, Max register value), as FPGA.cpp:283-291 assembles them."""
        if img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1 or img.strides[0] < img.shape[1]:
            raise StereoBMError(-2, "image must be an (H,W) uint8 array with dense rows")
        out = np.empty(img.shape, np.uint16)
        mx = ctypes.c_uint32()
        _check(self._L.sbm_gftt_eig(self._h, img.ctypes.data, img.strides[0], img.shape[1], img.shape[0], out.ctypes.data,
                                    out.strides[0], ctypes.byref(mx)), self._h)
        return out, int(mx.value)

    def gftt_eig(self, img):
        """PL GFTT min-eigenvalue map of torch CUDA uint8 frames (n,H,W) or (H,W): (int16-viewed uint16 map as torch.int32,
        per-image maximum) -- the inputs of generateKeypoints2 (src/slam/src/core/GFTT.cpp:41)."""
        import torch

        self._check_device_images(img)
        img = img.contiguous()
        h, w = img.shape[-2], img.shape[-1]
        n = 1 if img.dim() == 2 else img.shape[0]
        eig = torch.empty(img.shape, dtype=torch.int16, device=img.device)     # uint16 payload (torch has no uint16 math)
        mx = torch.empty((n,), dtype=torch.int32, device=img.device)
        torch.cuda.current_stream(img.device).synchronize()
        _check(self._L.sbm_gftt_eig_device(self._h, n, img.data_ptr(), w, h, eig.data_ptr(), mx.data_ptr(), 1), self._h)
        return eig.to(torch.int32) & 0xffff, mx

    # ---- keypoint selection of generateKeypoints2 (src/slam/src/core/GFTT.cpp:41-170) ------------------------------------------
    @staticmethod
    def _gftt_params(params, kw):
        if params is None:
            return gftt_select_params(**kw)
        if kw:
            raise TypeError("pass either a GfttSelectParams or keyword parameters")
        return params

    def gftt_select(self, eig, mx=None, params=None, sync=True, **kw):
        """generateKeypoints2 on torch CUDA maps (n,H,W) or (H,W) -- uint16 payload as int16 (what sbm_gftt_eig_device writes), or
        int32 holding 0..65535 (what gftt_eig returns) -- and their Max words mx (n,) int32, or None: each map's maximum.
        Returns (kpts float32 (n, cap, 2), count int32 (n,)); map i's points are kpts[i, :count[i]], in acceptance order.
        sync=False leaves the call running on the engine's stream (call synchronize() before reading the results)."""
        import torch

        p = self._gftt_params(params, kw)
        e3 = eig if eig.dim() == 3 else eig[None]
        if e3.dim() != 3 or not e3.is_cuda:
            raise StereoBMError(-2, "eig must be a torch CUDA (n,H,W) or (H,W) tensor")
        if e3.dtype in (torch.int32, torch.int64):
            e3 = torch.where(e3 > 32767, e3 - 65536, e3).to(torch.int16)
        elif e3.dtype != torch.int16 and str(e3.dtype) != "torch.uint16":
            raise StereoBMError(-2, "eig must hold uint16 values (int16, uint16 or int32 tensor)")
        e3 = e3.contiguous()
        n, h, w = e3.shape
        cap = gftt_select_capacity(p, w, h)
        kpts = torch.zeros((n, max(cap, 1), 2), dtype=torch.float32, device=e3.device)
        count = torch.zeros((n,), dtype=torch.int32, device=e3.device)
        mp = None
        if mx is not None:
            mp = mx.reshape(-1).to(device=e3.device, dtype=torch.int32).contiguous()
            if mp.numel() != n:
                raise StereoBMError(-2, f"mx holds {mp.numel()} values for {n} maps")
        torch.cuda.current_stream(e3.device).synchronize()
        _check(self._L.sbm_gftt_select_device(self._h, n, e3.data_ptr(), None if mp is None else mp.data_ptr(), w, h,
                                               ctypes.byref(p), kpts.data_ptr(), count.data_ptr(), 1 if sync else 0), self._h)
        if not sync:
            self._inflight.append((e3, mp, kpts, count))
        return kpts, count

    def gftt_detect(self, img, params=None, sync=True, **kw):
        """The KPTS_METHOD_FPGA_GFTT front end on torch CUDA uint8 frames (n,H,W) or (H,W): eigenvalue map, then
        generateKeypoints2, in one call. Returns (kpts float32 (n, cap, 2), count int32 (n,))."""
        import torch

        p = self._gftt_params(params, kw)
        self._check_device_images(img)
        i3 = (img if img.dim() == 3 else img[None]).contiguous()
        n, h, w = i3.shape
        cap = gftt_select_capacity(p, w, h)
        eig = torch.empty((n, h, w), dtype=torch.int16, device=i3.device)
        mx = torch.empty((n,), dtype=torch.int32, device=i3.device)
        kpts = torch.zeros((n, max(cap, 1), 2), dtype=torch.float32, device=i3.device)
        count = torch.zeros((n,), dtype=torch.int32, device=i3.device)
        torch.cuda.current_stream(i3.device).synchronize()
        _check(self._L.sbm_gftt_detect_device(self._h, n, i3.data_ptr(), w, h, ctypes.byref(p), eig.data_ptr(), mx.data_ptr(),
                                               kpts.data_ptr(), count.data_ptr(), 1 if sync else 0), self._h)
        if not sync:
            self._inflight.append((i3, eig, mx, kpts, count))
        return kpts, count

    def gftt_select_host(self, eig, max_eig, params=None, **kw):
        """numpy uint16 (H,W) map (rows may be strided) + the Max register -> numpy float32 (k, 2) points, as
        generateKeypoints2(eig, max, kpts2d) fills kpts2d."""
        p = self._gftt_params(params, kw)
        if not isinstance(eig, np.ndarray) or eig.dtype != np.uint16 or eig.ndim != 2 or eig.strides[1] != 2 or \
                eig.strides[0] < 2 * eig.shape[1]:
            raise StereoBMError(-2, "eig must be an (H,W) uint16 array with dense rows")
        h, w = eig.shape
        cap = gftt_select_capacity(p, w, h)
        out = np.zeros((max(cap, 1), 2), np.float32)
        k = ctypes.c_int()
        _check(self._L.sbm_gftt_select(self._h, eig.ctypes.data, eig.strides[0], w, h, int(max_eig) & 0xffff, ctypes.byref(p),
                                       out.ctypes.data, max(cap, 0), ctypes.byref(k)), self._h)
        return out[:k.value].copy()

    # ---- OpenCV's detector: generateKeypoints (src/slam/src/core/GFTT.cpp:11-25) ------------------------------------------------
    @staticmethod
    def _gftt_cv_params(params, kw):
        if params is None:
            return gftt_cv_params(**kw)
        if kw:
            raise TypeError("pass either a GfttCvParams or keyword parameters")
        return params

    def gftt_cv_eig(self, img, sync=True):
        """cv::cornerMinEigenVal (block 3, aperture 3) of torch CUDA uint8 frames (n,H,W) or (H,W), as include/sbm.h states it:
        (float32 maps (n,H,W), float32 maxima (n,))."""
        import torch

        self._check_device_images(img)
        i3 = (img if img.dim() == 3 else img[None]).contiguous()
        n, h, w = i3.shape
        eig = torch.empty((n, h, w), dtype=torch.float32, device=i3.device)
        mx = torch.empty((n,), dtype=torch.float32, device=i3.device)
        torch.cuda.current_stream(i3.device).synchronize()
        _check(self._L.sbm_gftt_cv_eig_device(self._h, n, i3.data_ptr(), w, h, eig.data_ptr(), mx.data_ptr(), 1 if sync else 0),
               self._h)
        if not sync:
            self._inflight.append((i3, eig, mx))
        return eig, mx

    def gftt_cv_detect(self, img, params=None, maps=True, sync=True, **kw):
        """generateKeypoints on torch CUDA uint8 frames (n,H,W) or (H,W). Returns (kpts float32 (n, cap, 2), count int32 (n,)) in
        gftt_select's layout, plus (maps (n,H,W) float32, maxima (n,) float32) when maps=True; maps=False passes no d_eig /
        d_max (the maps then live in the engine's scratch only)."""
        import torch

        p = self._gftt_cv_params(params, kw)
        self._check_device_images(img)
        i3 = (img if img.dim() == 3 else img[None]).contiguous()
        n, h, w = i3.shape
        cap = gftt_select_capacity(p, w, h)
        eig = torch.empty((n, h, w), dtype=torch.float32, device=i3.device) if maps else None
        mx = torch.empty((n,), dtype=torch.float32, device=i3.device) if maps else None
        kpts = torch.zeros((n, max(cap, 1), 2), dtype=torch.float32, device=i3.device)
        count = torch.zeros((n,), dtype=torch.int32, device=i3.device)
        torch.cuda.current_stream(i3.device).synchronize()
        _check(self._L.sbm_gftt_cv_detect_device(self._h, n, i3.data_ptr(), w, h, ctypes.byref(p),
                                                  eig.data_ptr() if maps else None, mx.data_ptr() if maps else None,
                                                  kpts.data_ptr(), count.data_ptr(), 1 if sync else 0), self._h)
        if not sync:
            self._inflight.append((i3, eig, mx, kpts, count))
        return (kpts, count, eig, mx) if maps else (kpts, count)

    def gftt_cv_select(self, eig, mx, params=None, sync=True, **kw):
        """The selection of generateKeypoints on float32 torch CUDA maps (n,H,W) or (H,W) and their maxima mx (n,) float32."""
        import torch

        p = self._gftt_cv_params(params, kw)
        e3 = eig if eig.dim() == 3 else eig[None]
        if e3.dim() != 3 or not e3.is_cuda or e3.dtype != torch.float32:
            raise StereoBMError(-2, "eig must be a float32 torch CUDA (n,H,W) or (H,W) tensor")
        e3 = e3.contiguous()
        n, h, w = e3.shape
        m1 = mx.reshape(-1).to(device=e3.device, dtype=torch.float32).contiguous()
        if m1.numel() != n:
            raise StereoBMError(-2, f"mx holds {m1.numel()} values for {n} maps")
        cap = gftt_select_capacity(p, w, h)
        kpts = torch.zeros((n, max(cap, 1), 2), dtype=torch.float32, device=e3.device)
        count = torch.zeros((n,), dtype=torch.int32, device=e3.device)
        torch.cuda.current_stream(e3.device).synchronize()
        _check(self._L.sbm_gftt_cv_select_device(self._h, n, e3.data_ptr(), m1.data_ptr(), w, h, ctypes.byref(p), kpts.data_ptr(),
                                                  count.data_ptr(), 1 if sync else 0), self._h)
        if not sync:
            self._inflight.append((e3, m1, kpts, count))
        return kpts, count

    def gftt_cv_detect_host(self, img, params=None, **kw):
        """numpy uint8 (H,W) frame (rows may be strided) -> numpy float32 (k, 2) points, as generateKeypoints(img, kpts2d) fills
        kpts2d."""
        p = self._gftt_cv_params(params, kw)
        if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1 or \
                img.strides[0] < img.shape[1]:
            raise StereoBMError(-2, "img must be an (H,W) uint8 array with dense rows")
        h, w = img.shape
        cap = gftt_select_capacity(p, w, h)
        out = np.zeros((max(cap, 1), 2), np.float32)
        k = ctypes.c_int()
        _check(self._L.sbm_gftt_cv_detect(self._h, img.ctypes.data, img.strides[0], w, h, ctypes.byref(p), out.ctypes.data,
                                          max(cap, 0), ctypes.byref(k)), self._h)
        return out[:k.value].copy()

    def orb_features_cv(self, img, pattern, gftt=None, angle=-1.0, edge_threshold=19, params=None, blur=False, sync=True, **kw):
        """The KPTS_METHOD_CV_GFTT + desc front end (SLAM_BATCH's) on torch CUDA uint8 frames (n,H,W) or (H,W): generateKeypoints,
        computeDescriptor, in one call. gftt: a GfttCvParams (or keyword parameters of gftt_cv_params). Returns (desc (n, cap,
        32), kpts (n, cap, 2), count (n,)) [+ blurred frames]."""
        import torch

        gp = self._gftt_cv_params(gftt, kw)
        p = self._orb_params(params, angle, edge_threshold)
        pat = orb_pattern_array(pattern)
        self._check_device_images(img)
        i3 = (img if img.dim() == 3 else img[None]).contiguous()
        n, h, w = i3.shape
        cap = max(gftt_select_capacity(gp, w, h), 1)
        kpts = torch.zeros((n, cap, 2), dtype=torch.float32, device=i3.device)
        count = torch.zeros((n,), dtype=torch.int32, device=i3.device)
        desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device=i3.device)
        bl = torch.zeros((n, h, w), dtype=torch.uint8, device=i3.device) if blur else None
        torch.cuda.current_stream(i3.device).synchronize()
        _check(self._L.sbm_orb_features_cv_device(self._h, n, i3.data_ptr(), w, h, ctypes.byref(gp), pat.ctypes.data,
                                                   ctypes.byref(p), None, None, kpts.data_ptr(), count.data_ptr(), desc.data_ptr(),
                                                   None if bl is None else bl.data_ptr(), 1 if sync else 0), self._h)
        if not sync:
            self._inflight.append((i3, kpts, count, desc, bl))
        return (desc, kpts, count, bl) if blur else (desc, kpts, count)

    def gftt_cv_profile(self):
        out = {}
        for k in ("gftt_cv_eig", "gftt_cv_select", "gftt_cv_total"):
            v = ctypes.c_float()
            _check(self._L.sbm_get_profile(self._h, k.encode(), ctypes.byref(v)), self._h)
            out[k] = v.value
        return out

    # ---- ORB descriptors of computeDescriptor (src/slam/src/opencv/CvORB.cpp) -------------------------------------------------
    @staticmethod
    def _orb_params(params, angle, edge_threshold):
        return params if params is not None else orb_params(edge_threshold=edge_threshold, angle=angle)

    def orb_describe(self, img, kpts, count, pattern, angle=-1.0, edge_threshold=19, params=None, out=None, blur=False,
                     sync=True):
        """computeDescriptor on torch CUDA uint8 frames (n,H,W) or (H,W) with keypoints in sbm_gftt_select_device's layout:
        kpts float32 (n, cap, 2), count int32 (n,) on the device. Returns (desc uint8 (n, cap, 32), kpts_kept (n, cap, 2),
        count_kept (n,)), plus the blurred frames (n, H, W) when blur=True. out="inplace" compacts into kpts / count themselves;
        otherwise new tensors (copies of kpts, so slots past the kept count keep their old values). Descriptor rows past the
        kept count are zero here (the C-ABI leaves them as they were)."""
        import torch

        p = self._orb_params(params, angle, edge_threshold)
        pat = orb_pattern_array(pattern)
        self._check_device_images(img)
        i3 = (img if img.dim() == 3 else img[None]).contiguous()
        n, h, w = i3.shape
        k3 = kpts if kpts.dim() == 3 else kpts[None]
        if k3.dtype != torch.float32 or k3.shape[0] != n or k3.shape[2] != 2 or not k3.is_contiguous() or not k3.is_cuda:
            raise StereoBMError(-2, "kpts must be a contiguous float32 CUDA tensor (n, cap, 2)")
        c1 = count.reshape(-1)
        if c1.dtype != torch.int32 or c1.numel() != n or not c1.is_cuda:
            raise StereoBMError(-2, "count must be an int32 CUDA tensor of n values")
        c1 = c1.contiguous()
        cap = k3.shape[1]
        if out == "inplace":
            ko, co = k3, c1
        else:
            ko, co = k3.clone(), torch.zeros_like(c1)
        desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device=i3.device)
        bl = torch.zeros((n, h, w), dtype=torch.uint8, device=i3.device) if blur else None
        torch.cuda.current_stream(i3.device).synchronize()
        _check(self._L.sbm_orb_describe_device(self._h, n, i3.data_ptr(), w, h, cap, k3.data_ptr(), c1.data_ptr(),
                                                pat.ctypes.data, ctypes.byref(p), ko.data_ptr(), co.data_ptr(), desc.data_ptr(),
                                                None if bl is None else bl.data_ptr(), 1 if sync else 0), self._h)
        if not sync:
            self._inflight.append((i3, k3, c1, ko, co, desc, bl))
        return (desc, ko, co, bl) if blur else (desc, ko, co)

    def orb_describe_host(self, img, kpts, pattern, angle=-1.0, edge_threshold=19, params=None):
        """numpy uint8 (H,W) frame (rows may be strided) + float32 (k, 2) keypoints -> (desc uint8 (m, 32), kept (m, 2)), as
        computeDescriptor(image, noArray(), kpts, true, desc) leaves desc and kpts."""
        p = self._orb_params(params, angle, edge_threshold)
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

    def orb_features(self, img, pattern, gftt=None, angle=-1.0, edge_threshold=19, params=None, blur=False, sync=True, **kw):
        """The KPTS_METHOD_FPGA_GFTT + desc front end on torch CUDA uint8 frames (n,H,W) or (H,W): eigenvalue map,
        generateKeypoints2, computeDescriptor, in one call. gftt: a GfttSelectParams (or keyword parameters of
        gftt_select_params). Returns (desc (n, cap, 32), kpts (n, cap, 2), count (n,)) [+ blurred frames]."""
        import torch

        gp = self._gftt_params(gftt, kw)
        p = self._orb_params(params, angle, edge_threshold)
        pat = orb_pattern_array(pattern)
        self._check_device_images(img)
        i3 = (img if img.dim() == 3 else img[None]).contiguous()
        n, h, w = i3.shape
        cap = max(gftt_select_capacity(gp, w, h), 1)
        eig = torch.empty((n, h, w), dtype=torch.int16, device=i3.device)
        mx = torch.empty((n,), dtype=torch.int32, device=i3.device)
        kpts = torch.zeros((n, cap, 2), dtype=torch.float32, device=i3.device)
        count = torch.zeros((n,), dtype=torch.int32, device=i3.device)
        desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device=i3.device)
        bl = torch.zeros((n, h, w), dtype=torch.uint8, device=i3.device) if blur else None
        torch.cuda.current_stream(i3.device).synchronize()
        _check(self._L.sbm_orb_features_device(self._h, n, i3.data_ptr(), w, h, ctypes.byref(gp), pat.ctypes.data, ctypes.byref(p),
                                                eig.data_ptr(), mx.data_ptr(), kpts.data_ptr(), count.data_ptr(), desc.data_ptr(),
                                                None if bl is None else bl.data_ptr(), 1 if sync else 0), self._h)
        if not sync:
            self._inflight.append((i3, eig, mx, kpts, count, desc, bl))
        return (desc, kpts, count, bl) if blur else (desc, kpts, count)

    # ---- keypoint matching of computeTransform (src/slam/src/core/Registration.cpp) ---------------------------------------
    def _match_store(self, desc, count):
        import torch

        if desc.dtype != torch.uint8 or desc.dim() != 3 or desc.shape[2] != 32 or not desc.is_contiguous() or not desc.is_cuda:
            raise StereoBMError(-2, "desc must be a contiguous uint8 CUDA tensor (n, cap, 32)")
        c1 = count.reshape(-1)
        if c1.dtype != torch.int32 or c1.numel() != desc.shape[0] or not c1.is_cuda or not c1.is_contiguous():
            raise StereoBMError(-2, "count must be a contiguous int32 CUDA tensor of n values")
        return desc.shape[0], desc.shape[1], c1

    def _match_out(self, m, cap, knn, dev):
        import torch

        pairs = torch.full((m, cap, 2), -1, dtype=torch.int32, device=dev)
        npairs = torch.zeros((m,), dtype=torch.int32, device=dev)
        rec = torch.zeros((m, cap, 4), dtype=torch.int32, device=dev) if knn else None
        return pairs, npairs, rec

    def match(self, desc, count, jobs, params=None, knn=False, sync=True):
        """matchingNoGuess for every (from, to) job over a store in sbm_orb_describe_device's layout: desc uint8 (n, cap, 32),
        count int32 (n,) on the device. Returns (pairs int32 (m, cap, 2), npairs int32 (m,)) [+ records int32 (m, cap, 4)
        with knn=True]; pair slots past npairs hold -1."""
        import torch

        n, cap, c1 = self._match_store(desc, count)
        j = _jobs_array(jobs)
        p = params if params is not None else match_params()
        pairs, npairs, rec = self._match_out(j.shape[0], cap, knn, desc.device)
        torch.cuda.current_stream(desc.device).synchronize()
        _check(self._L.sbm_match_device(self._h, n, j.shape[0], j.ctypes.data, desc.data_ptr(), c1.data_ptr(), cap, ctypes.byref(p),
                                        pairs.data_ptr(), npairs.data_ptr(), None if rec is None else rec.data_ptr(),
                                        1 if sync else 0), self._h)
        if not sync:
            self._inflight.append((desc, c1, pairs, npairs, rec))
        return (pairs, npairs, rec) if knn else (pairs, npairs)

    def match_guess(self, desc, count, kpts, proj, jobs, params=None, knn=False, sync=True):
        """matchingGuess's matching: kpts float32 (n, cap, 2) the frames' keypoints, proj float32 (m, cap, 2) each job's projected
        from-points (project_points; NaN = not a query). Returns as match()."""
        import torch

        n, cap, c1 = self._match_store(desc, count)
        j = _jobs_array(jobs)
        for t, shape in ((kpts, (n, cap, 2)), (proj, (j.shape[0], cap, 2))):
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise StereoBMError(-2, f"expected a contiguous float32 CUDA tensor {shape}")
        p = params if params is not None else match_params()
        pairs, npairs, rec = self._match_out(j.shape[0], cap, knn, desc.device)
        torch.cuda.current_stream(desc.device).synchronize()
        _check(self._L.sbm_match_guess_device(self._h, n, j.shape[0], j.ctypes.data, desc.data_ptr(), c1.data_ptr(), cap,
                                              kpts.data_ptr(), proj.data_ptr(), ctypes.byref(p), pairs.data_ptr(),
                                              npairs.data_ptr(), None if rec is None else rec.data_ptr(), 1 if sync else 0),
               self._h)
        if not sync:
            self._inflight.append((desc, c1, kpts, proj, pairs, npairs, rec))
        return (pairs, npairs, rec) if knn else (pairs, npairs)

    def project_points(self, xyz, count, from_frames, T, K, size, sync=True):
        """matchingGuess_Projection for m jobs: xyz float32 (n, cap, 3) and count int32 (n,) on the device, from_frames (m,) ints,
        T (m, 12) float32 (guessCameraRef per job), K = (fx, fy, cx, cy), size = (W, H). Returns float32 (m, cap, 2), NaN where
        a point is not valid."""
        import torch

        if xyz.dtype != torch.float32 or xyz.dim() != 3 or xyz.shape[2] != 3 or not xyz.is_contiguous() or not xyz.is_cuda:
            raise StereoBMError(-2, "xyz must be a contiguous float32 CUDA tensor (n, cap, 3)")
        n, cap = xyz.shape[0], xyz.shape[1]
        c1 = count.reshape(-1)
        if c1.dtype != torch.int32 or c1.numel() != n or not c1.is_cuda or not c1.is_contiguous():
            raise StereoBMError(-2, "count must be a contiguous int32 CUDA tensor of n values")
        fr = np.ascontiguousarray(np.asarray(from_frames, np.int32).reshape(-1))
        m = fr.shape[0]
        Tm = np.ascontiguousarray(np.asarray(T, np.float32).reshape(m, 12))
        Kd = np.ascontiguousarray(np.asarray(K, np.float64).reshape(4))
        proj = torch.zeros((max(m, 1), cap, 2), dtype=torch.float32, device=xyz.device)
        torch.cuda.current_stream(xyz.device).synchronize()
        _check(self._L.sbm_project_points_device(self._h, n, m, fr.ctypes.data, xyz.data_ptr(), c1.data_ptr(), cap, Tm.ctypes.data,
                                                 Kd.ctypes.data, int(size[0]), int(size[1]), proj.data_ptr(), 1 if sync else 0),
               self._h)
        if not sync:
            self._inflight.append((xyz, c1, proj))
        return proj

    @staticmethod
    def _desc_rows(d):
        d = np.asarray(d, dtype=np.uint8).reshape(-1, 32)
        if d.strides[1] != 1:
            d = np.ascontiguousarray(d)
        return d

    def match_host(self, desc_from, desc_to, params=None):
        """matchingNoGuess(descriptorsFrom, descriptorsTo) on (k, 32) uint8 host rows (row stride may exceed 32): (k, 2) int32
        (from, to) pairs in increasing from."""
        a, b = self._desc_rows(desc_from), self._desc_rows(desc_to)
        p = params if params is not None else match_params()
        out = np.zeros((max(a.shape[0], 1), 2), np.int32)
        k = ctypes.c_int()
        _check(self._L.sbm_match(self._h, a.ctypes.data, a.strides[0], a.shape[0], b.ctypes.data, b.strides[0], b.shape[0],
                                 ctypes.byref(p), out.ctypes.data, ctypes.byref(k)), self._h)
        return out[:k.value].copy()

    def match_guess_host(self, xyz_from, kpts_to, desc_from, desc_to, T, K, size, params=None):
        """matchingGuess on host arrays: xyz_from (nf, 3) float32, kpts_to (nt, 2) float32, both descriptor sets, T (12,)
        float32 guessCameraRef, K = (fx, fy, cx, cy), size = (W, H). Returns (k, 2) int32 pairs."""
        a, b = self._desc_rows(desc_from), self._desc_rows(desc_to)
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

    # ---- motion estimation of computeTransform (Registration.cpp:337-397) -------------------------------------------------
    @staticmethod
    def _pnp_K(K):
        return np.ascontiguousarray(np.asarray(K, np.float64).reshape(4))

    def estimate_motion(self, xyz, kpts, count, pairs, npairs, jobs, K, model=None, params=None, hyp=False, sync=True):
        """estimateMotion for every (from, to) job over a store: xyz float32 (n, cap, 3) (keypoints3d per frame), kpts float32
        (n, cap, 2), count int32 (n,), pairs int32 (m, cap, 2) and npairs int32 (m,) as match() returns them, all on the device;
        K = (fx, fy, cx, cy); model: a StereoModel whose localTransform applies, or None. Returns (results uint8 (m, 216): one
        sbm_pnp_result per job, decode with pnp_records; inliers int32 (m, cap) from-indices) [+ hypotheses uint8
        (m, iterations, 128) with hyp=True]."""
        import torch

        for t, d, last in ((xyz, torch.float32, 3), (kpts, torch.float32, 2), (pairs, torch.int32, 2)):
            if t.dtype != d or t.dim() != 3 or t.shape[2] != last or not t.is_contiguous() or not t.is_cuda:
                raise StereoBMError(-2, f"expected a contiguous {d} CUDA tensor (., cap, {last})")
        n, cap = xyz.shape[0], xyz.shape[1]
        if tuple(kpts.shape[:2]) != (n, cap) or pairs.shape[1] != cap:
            raise StereoBMError(-2, "xyz, kpts and pairs must share cap; xyz and kpts the frame count")
        c1, np1 = count.reshape(-1), npairs.reshape(-1)
        for t, k in ((c1, n), (np1, pairs.shape[0])):
            if t.dtype != torch.int32 or t.numel() != k or not t.is_cuda or not t.is_contiguous():
                raise StereoBMError(-2, "count / npairs must be contiguous int32 CUDA tensors")
        j = _jobs_array(jobs)
        m = j.shape[0]
        if pairs.shape[0] < m:
            raise StereoBMError(-2, "one pair list per job")
        p = params if params is not None else pnp_params()
        Kd = self._pnp_K(K)
        res = torch.zeros((m, PNP_RESULT_DTYPE.itemsize), dtype=torch.uint8, device=xyz.device)
        inl = torch.full((m, cap), -1, dtype=torch.int32, device=xyz.device)
        hy = torch.zeros((m, max(p.iterations, 1), PNP_HYP_DTYPE.itemsize), dtype=torch.uint8, device=xyz.device) if hyp else None
        torch.cuda.current_stream(xyz.device).synchronize()
        _check(self._L.sbm_estimate_motion_device(self._h, n, m, j.ctypes.data, xyz.data_ptr(), kpts.data_ptr(), c1.data_ptr(), cap,
                                                  pairs.data_ptr(), np1.data_ptr(), Kd.ctypes.data,
                                                  None if model is None else ctypes.byref(model), ctypes.byref(p), res.data_ptr(),
                                                  inl.data_ptr(), None if hy is None else hy.data_ptr(), 1 if sync else 0), self._h)
        if not sync:
            self._inflight.append((xyz, kpts, c1, pairs, np1, res, inl, hy))
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
        Kd = self._pnp_K(K)
        res = np.zeros(1, PNP_RESULT_DTYPE)
        inl = np.zeros(max(pr.shape[0], 1), np.int32)
        _check(self._L.sbm_estimate_motion(self._h, x.ctypes.data if x.size else None, x.shape[0], kp.ctypes.data if kp.size else None,
                                           xt.ctypes.data if xt.size else None, kp.shape[0], pr.ctypes.data if pr.size else None,
                                           pr.shape[0], Kd.ctypes.data, None if model is None else ctypes.byref(model),
                                           ctypes.byref(p), res.ctypes.data, inl.ctypes.data), self._h)
        return res[0], inl[:res[0]["num_inliers"]].copy()

    def pnp_profile(self):
        out = {}
        for k in ("pnp_hyp", "pnp_score", "pnp_refine", "pnp_total"):
            v = ctypes.c_float()
            _check(self._L.sbm_get_profile(self._h, k.encode(), ctypes.byref(v)), self._h)
            out[k] = v.value
        return out

    def match_profile(self):
        out = {}
        for k in ("match_knn", "match_unique", "match_total", "match_project"):
            v = ctypes.c_float()
            _check(self._L.sbm_get_profile(self._h, k.encode(), ctypes.byref(v)), self._h)
            out[k] = v.value
        return out

    def orb_profile(self):
        out = {}
        for k in ("orb_blur", "orb_desc", "orb_total"):
            v = ctypes.c_float()
            _check(self._L.sbm_get_profile(self._h, k.encode(), ctypes.byref(v)), self._h)
            out[k] = v.value
        return out

    def gftt_profile(self):
        out = {}
        for k in ("gftt_select_eig", "gftt_select_select", "gftt_select_total"):
            v = ctypes.c_float()
            _check(self._L.sbm_get_profile(self._h, k.encode(), ctypes.byref(v)), self._h)
            out[k] = v.value
        return out

    def synchronize(self):
        _check(self._L.sbm_synchronize(self._h), self._h)
        self._inflight.clear()   # buffers of asynchronous compute_device calls may be released now
        self._host_inflight.clear()

    def stream(self):
        return self._L.sbm_stream(self._h)

    def set_profiling(self, on):
        # 0 = off, 1 = sync after every call, 2 = stage events only (no host sync; up to 64 calls per profile() read),
        # 3 = as 2 on every 4th call only
        _check(self._L.sbm_set_profiling(self._h, int(on)), self._h)

    def last_kernel(self):
        """Template instantiation of the SAD kernel the last compute call launched (sbm_last_kernel_name)."""
        buf = ctypes.create_string_buffer(128)
        _check(self._L.sbm_last_kernel_name(self._h, buf, 128), self._h)
        return buf.value.decode()

    def profile(self):
        out = {}
        for k in ("prefilter", "sad", "lrcheck", "speckle", "total"):
            v = ctypes.c_float()
            _check(self._L.sbm_get_profile(self._h, k.encode(), ctypes.byref(v)), self._h)
            out[k] = v.value
        return out

    def debug_fetch(self, which, n, h, w):
        dt = {0: np.uint8, 1: np.uint8, 2: np.int32, 3: np.int16}[which]
        a = np.empty((n, h, w), dt)
        _check(self._L.sbm_debug_fetch(self._h, which, a.ctypes.data, a.nbytes), self._h)
        return a


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
