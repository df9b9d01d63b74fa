"""ctypes mirror of include/sbm.h: every structure and constant of the C-ABI, the loader of lib/libsbm_hip.so with the one
table of argument types, and the status check. Nothing here owns a handle; the classes over it are in _engine.py."""
import ctypes
import os
import pathlib

import numpy as np

PREFILTER_NORMALIZED_RESPONSE = 0
PREFILTER_XSOBEL = 1
PREFILTER_FLAVOUR_CV = 0
PREFILTER_FLAVOUR_RTL = 1

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


class SgbmParams(ctypes.Structure):
    """Mirror of `sbm_sgbm_params` (include/sbm.h), in cv::StereoSGBM::create argument order."""

    _fields_ = [(n, ctypes.c_int32) for n in ("min_disparity", "num_disparities", "block_size", "p1", "p2", "disp12_max_diff",
                                                "prefilter_cap", "uniqueness_ratio", "speckle_window_size", "speckle_range", "mode")]


class StereoModel(ctypes.Structure):
    """`sbm_stereo_model` of include/sbm.h: the StereoCameraModel entries the reference's reprojection reads
    (include/core/StereoCameraModel.h:25-34) plus the optional local transform."""

    _fields_ = [(k, ctypes.c_double) for k in ("fx_l", "fy_l", "cx_l", "cy_l", "Tx_l", "fx_r", "fy_r", "cx_r", "Tx_r")] + [
        ("local", ctypes.c_float * 12), ("has_local", ctypes.c_int32)]


class RectCam(ctypes.Structure):
    """`sbm_rect_cam` of include/sbm.h = struct RECT_PARAM_CH (src/StereoBM/src/fpga.h:250-256), one camera."""

    _fields_ = [("f", ctypes.c_int32 * 2), ("c", ctypes.c_int32 * 2), ("f2inv", ctypes.c_int32 * 2),
                ("c2_f2", ctypes.c_int32 * 2), ("rot", (ctypes.c_int32 * 3) * 3)]


class FpgaParams(ctypes.Structure):
    """`sbm_fpga_params` of include/sbm.h: the fields of the BM register block (struct FPGA_REG_BM,
    src/StereoBM/src/fpga.h:154-169) as decoded by src/dvp/rtl/bm.v:172-193."""

    _fields_ = [(k, ctypes.c_int32) for k in ("width", "height", "block_size", "num_disparities", "uni_enable", "uni_mode",
                                              "uni_threshold")]


class FpgaLaunch(ctypes.Structure):
    """One launch of `FpgaPlan`: its first 32-disparity phase, how many it holds (1, 2 or 4), the lean instantiation."""

    _fields_ = [(k, ctypes.c_int32) for k in ("phase0", "nph", "lean")]


class FpgaPlan(ctypes.Structure):
    """`FpgaPlan` of csrc/sbm_fpga.hip, as sbm_fpga_debug_plan copies it out: what the host decides before the matcher's launches."""

    _fields_ = [(k, ctypes.c_int32) for k in ("hwsz", "hsad_wdt", "sad_wdt", "sad_hgt", "nv", "strips", "nphase", "nseg", "seg",
                                              "grid_y", "track_sat", "exact", "xs", "lds", "nlaunch")] + [("launch", FpgaLaunch * 8)]

    @property
    def groups(self):
        return [self.launch[i].nph for i in range(self.nlaunch)]


class GfttSelectParams(ctypes.Structure):
    """`sbm_gftt_select_params` of include/sbm.h: generateKeypoints2's constants (src/slam/src/core/GFTT.cpp:50-53)."""

    _fields_ = [("max_features", ctypes.c_int32), ("quality_level", ctypes.c_double), ("min_distance", ctypes.c_double),
                ("block_size", ctypes.c_int32)]


class GfttCvParams(ctypes.Structure):
    """`sbm_gftt_cv_params` of include/sbm.h: cv::GFTTDetector::create's arguments (src/slam/src/core/GFTT.cpp:13-24)."""

    _fields_ = [("max_features", ctypes.c_int32), ("quality_level", ctypes.c_double), ("min_distance", ctypes.c_double),
                ("block_size", ctypes.c_int32), ("use_harris", ctypes.c_int32), ("k", ctypes.c_double)]


class OrbParams(ctypes.Structure):
    """`sbm_orb_params` of include/sbm.h: computeDescriptor's constants (src/slam/src/opencv/CvORB.cpp) and the keypoints' angle."""

    _fields_ = [("edge_threshold", ctypes.c_int32), ("angle", ctypes.c_float), ("blur_ksize", ctypes.c_int32),
                ("blur_sigma", ctypes.c_double)]


class MatchParams(ctypes.Structure):
    """`sbm_match_params` of include/sbm.h: the NNDR ratio and guided radius of computeTransform's matching (Registration.cpp)."""

    _fields_ = [("nndr", ctypes.c_float), ("radius", ctypes.c_float)]


class MatchPlanInfo(ctypes.Structure):
    """`sbm_match_plan_info` of include/sbm.h: the launch plan of a matching / projection call, a function of (cap, m)."""

    _fields_ = [(k, ctypes.c_int32) for k in ("qtiles", "nslice", "slice_rows", "jobs_per_launch", "launches",
                                              "proj_jobs_per_launch", "proj_launches", "pad")] + [("scratch_bytes", ctypes.c_int64)]


class PnpParams(ctypes.Structure):
    """`sbm_pnp_params` of include/sbm.h: estimateMotion's minInliers, refineIterations and solvePnPRansac's constants."""

    _fields_ = [("min_inliers", ctypes.c_int32), ("refine_iterations", ctypes.c_int32), ("iterations", ctypes.c_int32),
                ("reprojection_error", ctypes.c_float), ("refine_sigma", ctypes.c_float), ("pad", ctypes.c_int32),
                ("confidence", ctypes.c_double)]


class LkParams(ctypes.Structure):
    """`sbm_lk_params` of include/sbm.h: computeCorrespondences' constants (src/slam/src/core/Stereo.cpp:16-37)."""

    _fields_ = [("win_width", ctypes.c_int32), ("win_height", ctypes.c_int32), ("max_level", ctypes.c_int32),
                ("max_count", ctypes.c_int32), ("epsilon", ctypes.c_float), ("flags", ctypes.c_int32),
                ("min_eig_threshold", ctypes.c_double), ("min_disparity", ctypes.c_float), ("max_disparity", ctypes.c_float)]


class OccParams(ctypes.Structure):
    """`sbm_occ_params` of include/sbm.h: buildOccupancyGridMap's constants (src/slam/src/core/main.cpp:499-501)."""

    _fields_ = [("resolution", ctypes.c_double), ("range_max", ctypes.c_float), ("tree_depth", ctypes.c_int32)]


class OccRayParams(ctypes.Structure):
    """`sbm_occ_ray_params` of include/sbm.h: the probabilities of octomap's insertPointCloud and its maxrange (< 0: no limit)."""

    _fields_ = [("prob_hit", ctypes.c_double), ("prob_miss", ctypes.c_double), ("clamp_min", ctypes.c_double),
                ("clamp_max", ctypes.c_double), ("occupancy_thres", ctypes.c_double), ("max_range", ctypes.c_double)]


class OccQueryParams(ctypes.Structure):
    """`sbm_occ_query_params` of include/sbm.h: castRay's maxRange (<= 0: no limit), the log-odds threshold of isNodeOccupied and
    ignoreUnknownCells."""

    _fields_ = [("max_range", ctypes.c_double), ("occupancy_thres_log", ctypes.c_float), ("ignore_unknown", ctypes.c_int32)]


class OccTreeCounts(ctypes.Structure):
    """`sbm_occ_tree_counts` of include/sbm.h: what sbm_occ_tree_info reports of the last build."""

    _fields_ = [("voxels", ctypes.c_uint64), ("nodes", ctypes.c_uint64), ("leaves", ctypes.c_uint64),
                ("nodes_at", ctypes.c_uint64 * 17), ("leaves_at", ctypes.c_uint64 * 17), ("key_min", ctypes.c_uint16 * 3),
                ("key_max", ctypes.c_uint16 * 3), ("pad", ctypes.c_uint32)]


class OccBinaryHeader(ctypes.Structure):
    """`sbm_occ_binary_header` of include/sbm.h: what sbm_occ_binary_info reports of a .bt stream."""

    _fields_ = [("resolution", ctypes.c_double), ("size", ctypes.c_uint64), ("nodes", ctypes.c_uint64), ("leaves", ctypes.c_uint64),
                ("occupied", ctypes.c_uint64), ("voxels", ctypes.c_uint64), ("leaves_at", ctypes.c_uint64 * 17),
                ("key_min", ctypes.c_uint16 * 3), ("key_max", ctypes.c_uint16 * 3), ("pad", ctypes.c_uint32)]


class OccOtHeader(ctypes.Structure):
    """`sbm_occ_ot_header` of include/sbm.h: what sbm_occ_ot_info reports of an .ot stream."""

    _fields_ = [("resolution", ctypes.c_double), ("size", ctypes.c_uint64), ("nodes", ctypes.c_uint64), ("leaves", ctypes.c_uint64),
                ("voxels", ctypes.c_uint64), ("leaves_at", ctypes.c_uint64 * 17), ("value_min", ctypes.c_float),
                ("value_max", ctypes.c_float), ("key_min", ctypes.c_uint16 * 3), ("key_max", ctypes.c_uint16 * 3), ("pad", ctypes.c_uint32)]


class OccGrowthInfo(ctypes.Structure):
    """`sbm_occ_growth_info` of include/sbm.h: what sbm_occ_get_growth reports of a map's table and its growth so far."""

    _fields_ = [("enabled", ctypes.c_int32), ("reserved", ctypes.c_int32), ("capacity", ctypes.c_uint64), ("slots", ctypes.c_uint64),
                ("max_capacity", ctypes.c_uint64), ("grown", ctypes.c_uint64), ("moved", ctypes.c_uint64), ("redone", ctypes.c_uint64)]


class OccEditInfo(ctypes.Structure):
    """`sbm_occ_edit_info` of include/sbm.h: what sbm_occ_last_edit reports of the last edit or delete call."""

    _fields_ = [("items", ctypes.c_uint64), ("skipped", ctypes.c_uint64), ("lost", ctypes.c_uint64), ("created", ctypes.c_uint64),
                ("removed", ctypes.c_uint64)]


class OccColorInfo(ctypes.Structure):
    """`sbm_occ_color_info` of include/sbm.h: what sbm_occ_color_last reports of the last colour batch."""

    _fields_ = [("items", ctypes.c_uint64), ("found", ctypes.c_uint64), ("unknown", ctypes.c_uint64), ("skipped", ctypes.c_uint64)]


OCC_COLOR_SET, OCC_COLOR_AVERAGE = 0, 1      # SBM_OCC_COLOR_*: the op of a colour batch
OCC_COLOR_WHITE = 0x00FFFFFF                 # SBM_OCC_COLOR_WHITE: the colour word of a voxel without a colour
OCC_EDIT_UPDATE, OCC_EDIT_SET, OCC_EDIT_DELETE = 0, 1, 2      # SBM_OCC_EDIT_*: the op of an item
OCC_EDIT_CHUNK = 2097152                                     # SBM_OCC_EDIT_CHUNK: items per chunk of a large batch
OCC_OT_FAN, OCC_OT_SCAN_TILE = 16, 1024      # SBM_OCC_OT_FAN, SBM_OCC_OT_SCAN_TILE: the tile constants of the .ot device parse


class VwdParams(ctypes.Structure):
    """`sbm_vwd_params` of include/sbm.h: addNewWords' metric and NNDR ratio (VWDictionary.cpp:43), and the search's slice count."""

    _fields_ = [("metric", ctypes.c_int32), ("nndr", ctypes.c_float), ("slices", ctypes.c_int32)]


class PgoParams(ctypes.Structure):
    """`sbm_pgo_params` of include/sbm.h: runOptimize's iteration count, the fixed vertex, the coupling reading, the run length."""

    _fields_ = [("num", ctypes.c_int32), ("fixed_id", ctypes.c_int32), ("coupling", ctypes.c_int32), ("run_max", ctypes.c_int32)]


class PgoGraph(ctypes.Structure):
    """`sbm_pgo_graph`: pointers to the caller's vertex and edge arrays."""

    _fields_ = [("n_vertices", ctypes.c_int32), ("ids", ctypes.c_void_p), ("poses", ctypes.c_void_p), ("n_edges", ctypes.c_int32),
                ("frm", ctypes.c_void_p), ("to", ctypes.c_void_p), ("meas", ctypes.c_void_p), ("info", ctypes.c_void_p)]


class PgoPlanInfo(ctypes.Structure):
    """`sbm_pgo_plan_info`: the partition of one graph into runs and junctions."""

    _fields_ = [(n, ctypes.c_int32) for n in ("n_free", "n_runs", "n_junctions", "schur_size", "n_coupling", "longest_run",
                                              "n_slots", "max_junctions")]


PGO_COUPLING_REFERENCE, PGO_COUPLING_SYMMETRIC = 0, 1
PGO_EDGE_RECORD = 200
ERR_OCC_FULL = -25
ERR_VWD_FULL = -26
OCC_CELL_OUT, OCC_CELL_UNKNOWN, OCC_CELL_FREE, OCC_CELL_OCCUPIED = -1, 0, 1, 2
OCC_RAY_NONE, OCC_RAY_HIT, OCC_RAY_RANGE, OCC_RAY_UNKNOWN, OCC_RAY_BOUNDS = 0, 1, 2, 3, 4
OCC_TREE_LOGODDS, OCC_TREE_MAXLIKELIHOOD = 0, 1
VWD_L1, VWD_L2 = 0, 1
VWD_NONE = 2147483647
LK_USE_INITIAL_FLOW = 4
LK_GET_MIN_EIGENVALS = 8

# `sbm_pnp_result` (216 bytes) and `sbm_pnp_hypothesis` (128 bytes) as numpy record types
PNP_RESULT_DTYPE = np.dtype([("status", "<i4"), ("num_matches", "<i4"), ("num_inliers", "<i4"), ("ransac_inliers", "<i4"),
                             ("best_iteration", "<i4"), ("niters", "<i4"), ("refine_solves", "<i4"), ("refine_exit", "<i4"),
                             ("rvec", "<f8", 3), ("tvec", "<f8", 3), ("R", "<f8", 9), ("cov_dist", "<f8"), ("cov_angle", "<f8"),
                             ("transform", "<f4", 12)])
PNP_HYP_DTYPE = np.dtype([("subset", "<i4", 6), ("count", "<i4"), ("pad", "<i4"), ("R", "<f8", 9), ("t", "<f8", 3)])
PNP_OK, PNP_FEW_MATCHES, PNP_NO_MODEL, PNP_FEW_RANSAC_INLIERS, PNP_FEW_REFINED_INLIERS = 0, 1, 2, 3, 4


class StereoBMError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"sbm status {code}: {message}")
        self.code = code


def _torch():
    """torch, imported on first use and nowhere else: importing the package must not import it, and the numpy-only host entry
    points work without it."""
    import torch
    return torch


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
        _torch()
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
    L.sbm_debug_postfilter.argtypes = [vp, ci, ci, ci, vp, vp, ci, vp, vp, sz]   # for the tests: not in include/sbm.h
    L.sbm_set_profiling.argtypes = [vp, ci]
    L.sbm_get_profile.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_float)]
    L.sbm_last_kernel_name.argtypes = [vp, ctypes.c_char_p, sz]
    sp = ctypes.POINTER(SgbmParams)
    L.sbm_sgbm_params_default.argtypes = [sp, ci, ci, ci]
    L.sbm_sgbm_params_default.restype = None
    L.sbm_sgbm_params_validate.argtypes = [sp, ci, ci]
    L.sbm_sgbm_compute.argtypes = [vp, sp, vp, sz, vp, sz, ci, ci, vp, sz]
    L.sbm_sgbm_compute_device.argtypes = [vp, sp, ci, vp, vp, ci, ci, vp, ci]
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
    L.sbm_fpga_debug_plan.argtypes = [fp, ci, vp, sz]
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
    L.sbm_match_plan.argtypes = [ci, ci, vp, sz]
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
    lp = ctypes.POINTER(LkParams)
    L.sbm_lk_params_default.argtypes = [lp]
    L.sbm_lk_params_default.restype = None
    L.sbm_lk_params_validate.argtypes = [lp, ci, ci]
    L.sbm_lk_pyramid_device.argtypes = [vp, ci, vp, ci, ci, ci, lp, vp, vp, ctypes.POINTER(ci)]
    L.sbm_lk_stereo_device.argtypes = [vp, ci, vp, vp, ci, ci, vp, vp, ci, lp, vp, vp, vp, ci]
    L.sbm_lk_stereo.argtypes = [vp, vp, sz, vp, sz, ci, ci, vp, ci, lp, vp, vp, vp]
    L.sbm_keypoints3d_lk_device.argtypes = [vp, ci, vp, vp, vp, vp, ci, mp, ctypes.c_float, ctypes.c_float, vp, ci]
    ocp = ctypes.POINTER(OccParams)
    L.sbm_occ_params_default.argtypes = [ocp]
    L.sbm_occ_params_default.restype = None
    L.sbm_occ_params_validate.argtypes = [ocp]
    L.sbm_occ_create.argtypes = [vp, ocp, sz, ctypes.POINTER(vp)]
    L.sbm_occ_destroy.argtypes = [vp]
    L.sbm_occ_destroy.restype = None
    L.sbm_occ_reset.argtypes = [vp]
    L.sbm_occ_insert_device.argtypes = [vp, ci, vp, ci, ci, ci, mp, vp, ci]
    L.sbm_occ_insert.argtypes = [vp, ci, vp, ci, ci, ci, mp, vp]
    L.sbm_occ_size.argtypes = [vp, ctypes.POINTER(sz)]
    L.sbm_occ_overflow.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.sbm_occ_fetch_device.argtypes = [vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_fetch.argtypes = [vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_write_binary.argtypes = [vp, sz, ctypes.c_double, ctypes.c_char_p]
    orp = ctypes.POINTER(OccRayParams)
    L.sbm_occ_ray_params_default.argtypes = [orp]
    L.sbm_occ_ray_params_default.restype = None
    L.sbm_occ_ray_params_validate.argtypes = [orp]
    L.sbm_occ_ray_logodds.argtypes = [orp, vp]
    L.sbm_occ_insert_cloud_device.argtypes = [vp, sz, vp, vp, orp, ci]
    L.sbm_occ_insert_cloud.argtypes = [vp, sz, vp, vp, orp]
    L.sbm_occ_insert_rays_device.argtypes = [vp, ci, vp, ci, ci, ci, mp, vp, orp, ci]
    L.sbm_occ_insert_rays.argtypes = [vp, ci, vp, ci, ci, ci, mp, vp, orp]
    L.sbm_occ_fetch_logodds_device.argtypes = [vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_fetch_logodds.argtypes = [vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_write_binary_logodds.argtypes = [vp, vp, sz, ctypes.c_double, ctypes.c_float, ctypes.c_char_p]
    oqp = ctypes.POINTER(OccQueryParams)
    L.sbm_occ_query_params_default.argtypes = [oqp]
    L.sbm_occ_query_params_default.restype = None
    L.sbm_occ_query_params_validate.argtypes = [oqp]
    L.sbm_occ_search_device.argtypes = [vp, sz, vp, ctypes.c_float, vp, vp, ci]
    L.sbm_occ_search.argtypes = [vp, sz, vp, ctypes.c_float, vp, vp]
    L.sbm_occ_cast_rays_device.argtypes = [vp, sz, vp, ci, vp, oqp, vp, vp, ci]
    L.sbm_occ_cast_rays.argtypes = [vp, sz, vp, ci, vp, oqp, vp, vp]
    L.sbm_occ_cast_view_device.argtypes = [vp, ci, ci, ci, mp, vp, oqp, vp, vp, ci]
    L.sbm_occ_tree_create.argtypes = [vp, ctypes.POINTER(vp)]
    L.sbm_occ_tree_destroy.argtypes = [vp]
    L.sbm_occ_tree_destroy.restype = None
    L.sbm_occ_tree_build.argtypes = [vp, ci, orp, ci]
    L.sbm_occ_tree_info.argtypes = [vp, ctypes.POINTER(OccTreeCounts)]
    L.sbm_occ_tree_search_device.argtypes = [vp, sz, vp, ci, ctypes.c_float, vp, vp, vp, ci]
    L.sbm_occ_tree_search.argtypes = [vp, sz, vp, ci, ctypes.c_float, vp, vp, vp]
    L.sbm_occ_tree_leaves_device.argtypes = [vp, ci, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_tree_leaves.argtypes = [vp, ci, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_tree_binary_device.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_tree_write_binary.argtypes = [vp, ctypes.c_char_p]
    L.sbm_occ_binary_info.argtypes = [vp, sz, ctypes.POINTER(OccBinaryHeader)]
    L.sbm_occ_binary_leaves.argtypes = [vp, sz, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_load_binary.argtypes = [vp, vp, sz, orp, ci]
    L.sbm_occ_read_binary.argtypes = [vp, ctypes.c_char_p, orp, ci]
    L.sbm_occ_ot_body_device.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_ot_write.argtypes = [vp, ctypes.c_char_p]
    L.sbm_occ_ot_info.argtypes = [vp, sz, ctypes.POINTER(OccOtHeader)]
    L.sbm_occ_ot_leaves.argtypes = [vp, sz, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_ot_load.argtypes = [vp, vp, sz, ci]
    L.sbm_occ_ot_read.argtypes = [vp, ctypes.c_char_p, ci]
    # occupancy map: insert options
    L.sbm_occ_set_bbx.argtypes = [vp, vp, vp]
    L.sbm_occ_use_bbx_limit.argtypes = [vp, ci]
    L.sbm_occ_get_bbx.argtypes = [vp, vp, vp, vp, vp, ctypes.POINTER(ci)]
    L.sbm_occ_enable_change_detection.argtypes = [vp, ci]
    L.sbm_occ_change_detection_enabled.argtypes = [vp, ctypes.POINTER(ci)]
    L.sbm_occ_reset_change_detection.argtypes = [vp]
    L.sbm_occ_num_changes.argtypes = [vp, ctypes.POINTER(sz)]
    L.sbm_occ_fetch_changes_device.argtypes = [vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_fetch_changes.argtypes = [vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_insert_cloud_discrete_device.argtypes = L.sbm_occ_insert_cloud_device.argtypes
    L.sbm_occ_insert_cloud_discrete.argtypes = L.sbm_occ_insert_cloud.argtypes
    L.sbm_occ_insert_rays_discrete_device.argtypes = L.sbm_occ_insert_rays_device.argtypes
    L.sbm_occ_insert_rays_discrete.argtypes = L.sbm_occ_insert_rays.argtypes
    L.sbm_occ_capacity.argtypes = [vp, ctypes.POINTER(sz)]
    L.sbm_occ_reserve.argtypes = [vp, sz]
    L.sbm_occ_set_growth.argtypes = [vp, ci, sz]
    L.sbm_occ_get_growth.argtypes = [vp, ctypes.POINTER(OccGrowthInfo)]
    L.sbm_occ_growth_step.argtypes = [sz, sz, sz, ctypes.POINTER(sz)]
    # edits by key: items (keys or points, ops, values) in device or host memory
    L.sbm_occ_edit_device.argtypes = [vp, sz, vp, vp, vp, orp, ci]
    L.sbm_occ_edit.argtypes = [vp, sz, vp, vp, vp, orp]
    L.sbm_occ_edit_points_device.argtypes = L.sbm_occ_edit_device.argtypes
    L.sbm_occ_edit_points.argtypes = L.sbm_occ_edit.argtypes
    L.sbm_occ_delete_device.argtypes = [vp, sz, vp, ci]
    L.sbm_occ_delete.argtypes = [vp, sz, vp, ci]
    L.sbm_occ_delete_box.argtypes = [vp, vp, vp, ci]
    L.sbm_occ_last_edit.argtypes = [vp, ctypes.POINTER(OccEditInfo)]
    # colour per voxel: batches (keys or points, colour words), the coloured search and fetch
    L.sbm_occ_color_keys_device.argtypes = [vp, sz, vp, vp, ci, ci]
    L.sbm_occ_color_keys.argtypes = [vp, sz, vp, vp, ci]
    L.sbm_occ_color_points_device.argtypes = L.sbm_occ_color_keys_device.argtypes
    L.sbm_occ_color_points.argtypes = L.sbm_occ_color_keys.argtypes
    L.sbm_occ_color_last.argtypes = [vp, ctypes.POINTER(OccColorInfo)]
    L.sbm_occ_color_search_device.argtypes = [vp, sz, vp, ctypes.c_float, vp, vp, vp, ci]
    L.sbm_occ_color_search.argtypes = [vp, sz, vp, ctypes.c_float, vp, vp, vp]
    L.sbm_occ_color_fetch_device.argtypes = [vp, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_color_fetch.argtypes = [vp, vp, vp, vp, sz, ctypes.POINTER(sz)]
    # ... on a tree's nodes, and the ColorOcTree stream
    L.sbm_occ_color_leaves_device.argtypes = [vp, ci, vp, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_color_leaves.argtypes = [vp, ci, vp, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_color_ot_body_device.argtypes = [vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_color_ot_write.argtypes = [vp, ctypes.c_char_p]
    L.sbm_occ_color_ot_info.argtypes = [vp, sz, ctypes.POINTER(OccOtHeader)]
    L.sbm_occ_color_ot_leaves.argtypes = [vp, sz, vp, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_color_ot_load.argtypes = [vp, vp, sz, ci]
    L.sbm_occ_color_ot_read.argtypes = [vp, ctypes.c_char_p, ci]
    # time stamps per voxel: the map's clock, the degrade, forgetting by age, the stamped search and fetch
    u32 = ctypes.c_uint32
    L.sbm_occ_stamp_enable.argtypes = [vp]
    L.sbm_occ_stamp_enabled.argtypes = [vp, ctypes.POINTER(ci)]
    L.sbm_occ_stamp_set_time.argtypes = [vp, u32]
    L.sbm_occ_stamp_time.argtypes = [vp, ctypes.POINTER(u32)]
    L.sbm_occ_stamp_degrade.argtypes = [vp, u32, vp, ctypes.POINTER(ctypes.c_uint64)]
    L.sbm_occ_stamp_forget.argtypes = [vp, u32, ctypes.POINTER(ctypes.c_uint64)]
    L.sbm_occ_stamp_search_device.argtypes = [vp, sz, vp, ctypes.c_float, vp, vp, vp, ci]
    L.sbm_occ_stamp_search.argtypes = [vp, sz, vp, ctypes.c_float, vp, vp, vp]
    L.sbm_occ_stamp_fetch_device.argtypes = [vp, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_stamp_fetch.argtypes = [vp, vp, vp, vp, sz, ctypes.POINTER(sz)]
    # ... on a tree's nodes, and the OcTreeStamped stream
    L.sbm_occ_stamp_leaves_device.argtypes = [vp, ci, vp, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_stamp_leaves.argtypes = [vp, ci, vp, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_stamp_root.argtypes = [vp, ctypes.POINTER(u32)]
    L.sbm_occ_stamp_ot_write.argtypes = [vp, ctypes.c_char_p]
    L.sbm_occ_stamp_ot_info.argtypes = [vp, sz, ctypes.POINTER(OccOtHeader)]
    L.sbm_occ_stamp_ot_leaves.argtypes = [vp, sz, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_stamp_ot_load.argtypes = [vp, vp, sz, ci]
    L.sbm_occ_stamp_ot_read.argtypes = [vp, ctypes.c_char_p, ci]
    # the read side for planners: a box's corners and a ray's shared origin are host memory
    L.sbm_occ_bbx_leaves_device.argtypes = [vp, vp, vp, ci, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_bbx_leaves.argtypes = L.sbm_occ_bbx_leaves_device.argtypes
    L.sbm_occ_bbx_leaves_points_device.argtypes = L.sbm_occ_bbx_leaves_device.argtypes
    L.sbm_occ_bbx_leaves_points.argtypes = L.sbm_occ_bbx_leaves_device.argtypes
    L.sbm_occ_unknown_device.argtypes = [vp, vp, vp, ci, vp, sz, ctypes.POINTER(sz)]
    L.sbm_occ_unknown.argtypes = L.sbm_occ_unknown_device.argtypes
    L.sbm_occ_metric.argtypes = [vp, vp, vp]
    L.sbm_occ_ray_intersections_device.argtypes = [vp, sz, vp, ci, vp, vp, ctypes.c_double, vp, vp, ci]
    L.sbm_occ_ray_intersections.argtypes = [vp, sz, vp, ci, vp, vp, ctypes.c_double, vp, vp]
    wp = ctypes.POINTER(VwdParams)
    pi = ctypes.POINTER(ci)
    L.sbm_vwd_params_default.argtypes = [wp]
    L.sbm_vwd_params_default.restype = None
    L.sbm_vwd_params_validate.argtypes = [wp]
    L.sbm_vwd_create.argtypes = [vp, sz, wp, ctypes.POINTER(vp)]
    L.sbm_vwd_destroy.argtypes = [vp]
    L.sbm_vwd_destroy.restype = None
    L.sbm_vwd_reset.argtypes = [vp]
    L.sbm_vwd_size.argtypes = [vp, ctypes.POINTER(sz)]
    L.sbm_vwd_overflow.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.sbm_vwd_add_words_device.argtypes = [vp, vp, ci, ci, ci, vp]
    L.sbm_vwd_add_words.argtypes = [vp, vp, sz, ci, ci, ci, vp]
    L.sbm_vwd_search_device.argtypes = [vp, vp, ci, vp, ci]
    L.sbm_vwd_fetch_words.argtypes = [vp, sz, sz, vp]
    L.sbm_vwd_references.argtypes = [vp, ci, vp, vp, ci, pi]
    L.sbm_vwd_likelihood.argtypes = [vp, ci, vp, ci, ci, vp, pi, ctypes.POINTER(ctypes.c_float)]
    L.sbm_vwd_limit_keypoints.argtypes = [vp, ci, ci, vp]
    gp, qp, ip = ctypes.POINTER(PgoParams), ctypes.POINTER(PgoGraph), ctypes.POINTER(PgoPlanInfo)
    L.sbm_pgo_params_default.argtypes = [gp]
    L.sbm_pgo_params_default.restype = None
    L.sbm_pgo_params_check.argtypes = [gp, qp]
    L.sbm_pgo_plan.argtypes = [gp, qp, ip, vp, vp, vp]
    L.sbm_pgo_optimize.argtypes = [vp, gp, qp, vp, ctypes.POINTER(ctypes.c_double)]
    L.sbm_pgo_optimize_robust.argtypes = [vp, gp, qp, ctypes.POINTER(ctypes.c_int32), vp, vp, ctypes.POINTER(ctypes.c_double), vp,
                                          ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    L.sbm_pgo_optimize_device.argtypes = [vp, gp, qp, vp, ctypes.POINTER(ctypes.c_double)]
    L.sbm_pgo_optimize_robust_device.argtypes = [vp, gp, qp, ctypes.POINTER(ctypes.c_int32), vp, vp, ctypes.POINTER(ctypes.c_double),
                                                 vp, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    L.sbm_pgo_last_plan.argtypes = [vp, ip, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)]
    L.sbm_pgo_debug_fetch.argtypes = [vp, ci, vp, sz]
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
