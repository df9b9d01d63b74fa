"""MI355X-native stereo block-matching disparity engine (drop-in for the cv::StereoBM call of
sdoira/U96-SLAM, src/slam/src/core/main.cpp:197-217).

Layout
  csrc/         hand-written HIP kernels (gfx950) + the C-ABI (include/sbm.h)  -> lib/libsbm_hip.so
  _abi.py       ctypes mirror of include/sbm.h: structures, loader with the one argtypes table, status check
  _engine.py    the base of both classes: one handle, its in-flight buffers, the one call path to the device entry points
  _frontend.py _fpga.py _gftt.py _orb.py _match.py _pnp.py _lk.py   one family of entry points each, as mixins of StereoBM
  _occupancy.py OccupancyMap: the voxel map of buildOccupancyGridMap, made from a StereoBM / StereoSGBM's handle
  _vwd.py       VWDictionary: the visual-word dictionary and loop-closure likelihood, made from such a handle too
  _pgo.py       PoseGraph: the pose-graph optimiser (runOptimize / runOptimizeRobust), made from such a handle too
  stereobm.py   host-side mirror of the cv::StereoBM interface (the dense path) and every public name of the above
  stereosgbm.py the same for cv::StereoSGBM (MODE_HH / MODE_SGBM)
  synth.py      deterministic synthetic stereo frames
  shard.py      one-process-per-GPU sharding of pair batches (torch.distributed; RCCL on GPU, gloo on CPU)

There is no CPU fallback in this package: constructing a StereoBM without the built HIP library or without a
GPU raises. The CPU oracle lives in /oracle and is only used by the tests and by bench.py's cpu_baseline leg.
"""
from .stereobm import (StereoBM, StereoBMError, SbmParams, StereoModel, library_path, load_library, PREFILTER_XSOBEL,  # noqa: F401
                       PREFILTER_NORMALIZED_RESPONSE, RectCam, make_rect_cam, PREFILTER_FLAVOUR_CV, PREFILTER_FLAVOUR_RTL, trim,
                       FpgaParams, fpga_params, fpga_params_from_regs, fpga_sad_size_reg, fpga_validate, compute_multi,
                       FpgaPlan, fpga_plan,
                       GfttSelectParams, gftt_select_params, gftt_select_validate, gftt_select_capacity,
                       GfttCvParams, gftt_cv_params, gftt_cv_validate,
                       OrbParams, orb_params, orb_validate, MatchParams, MatchPlanInfo, match_params, match_plan, match_validate,
                       PnpParams, pnp_params, pnp_validate, pnp_records, PNP_RESULT_DTYPE, PNP_HYP_DTYPE,
                       LkParams, lk_params, lk_validate, lk_level_sizes, LK_GET_MIN_EIGENVALS, LK_USE_INITIAL_FLOW)
from .stereosgbm import StereoSGBM, SgbmParams, sgbm_params, sgbm_validate  # noqa: F401
from ._occupancy import OccupancyMap, OccParams, occ_params, occ_validate, occ_write_binary, ERR_OCC_FULL  # noqa: F401
from ._occupancy import OccRayParams, occ_ray_params, occ_ray_validate, occ_ray_logodds, occ_write_binary_logodds  # noqa: F401
from ._occupancy import (OccQueryParams, occ_query_params, occ_query_validate, OCC_CELL_OUT, OCC_CELL_UNKNOWN,  # noqa: F401
                         OCC_CELL_FREE, OCC_CELL_OCCUPIED, OCC_RAY_NONE, OCC_RAY_HIT, OCC_RAY_RANGE, OCC_RAY_UNKNOWN, OCC_RAY_BOUNDS)
from ._occupancy import OccupancyTree, OccTreeCounts, OCC_TREE_LOGODDS, OCC_TREE_MAXLIKELIHOOD  # noqa: F401
from ._occupancy import OccBinaryHeader, occ_binary_info, occ_binary_leaves  # noqa: F401
from ._occupancy import OccOtHeader, occ_ot_info, occ_ot_leaves  # noqa: F401
from ._occupancy import OccGrowthInfo, occ_growth_step  # noqa: F401
from ._occupancy import occ_stamped_ot_info, occ_stamped_ot_leaves  # noqa: F401
from ._occupancy import OccColorInfo, OCC_COLOR_AVERAGE, OCC_COLOR_SET, OCC_COLOR_WHITE, occ_color_ot_info, occ_color_ot_leaves, occ_color_rgb, occ_color_words  # noqa: F401
from ._occupancy import OccEditInfo, OCC_EDIT_CHUNK, OCC_EDIT_DELETE, OCC_EDIT_SET, OCC_EDIT_UPDATE  # noqa: F401
from ._vwd import (VWDictionary, VwdParams, vwd_params, vwd_validate, limit_keypoints, ERR_VWD_FULL, VWD_L1, VWD_L2,  # noqa: F401
                   VWD_NONE)
from ._pgo import (PoseGraph, PgoParams, PgoPlanInfo, PgoGraph, pgo_params, pgo_check, pgo_plan, PGO_COUPLING_REFERENCE,  # noqa: F401
                   PGO_COUPLING_SYMMETRIC, PGO_EDGE_RECORD)

__all__ = ["StereoBM", "StereoBMError", "SbmParams", "StereoModel", "library_path", "load_library", "PREFILTER_XSOBEL",
           "PREFILTER_NORMALIZED_RESPONSE", "RectCam", "make_rect_cam", "PREFILTER_FLAVOUR_CV", "PREFILTER_FLAVOUR_RTL", "trim",
           "FpgaParams", "fpga_params", "fpga_params_from_regs", "fpga_sad_size_reg", "fpga_validate", "compute_multi",
           "FpgaPlan", "fpga_plan",
           "StereoSGBM", "SgbmParams", "sgbm_params", "sgbm_validate", "GfttSelectParams", "gftt_select_params",
           "gftt_select_validate", "gftt_select_capacity", "OrbParams", "orb_params", "orb_validate", "MatchParams",
           "match_params", "match_plan", "MatchPlanInfo", "match_validate", "PnpParams", "pnp_params", "pnp_validate", "pnp_records", "PNP_RESULT_DTYPE",
           "PNP_HYP_DTYPE", "GfttCvParams", "gftt_cv_params", "gftt_cv_validate", "LkParams", "lk_params", "lk_validate",
           "lk_level_sizes", "LK_GET_MIN_EIGENVALS", "LK_USE_INITIAL_FLOW", "OccupancyMap", "OccParams", "occ_params", "occ_validate",
           "occ_write_binary", "ERR_OCC_FULL", "OccRayParams", "occ_ray_params", "occ_ray_validate", "occ_ray_logodds",
           "occ_write_binary_logodds", "OccQueryParams", "occ_query_params", "occ_query_validate", "OCC_CELL_OUT", "OCC_CELL_UNKNOWN",
           "OCC_CELL_FREE", "OCC_CELL_OCCUPIED", "OCC_RAY_NONE", "OCC_RAY_HIT", "OCC_RAY_RANGE", "OCC_RAY_UNKNOWN", "OCC_RAY_BOUNDS",
           "OccupancyTree", "OccTreeCounts", "OccBinaryHeader", "occ_binary_info", "occ_binary_leaves", "OccOtHeader", "occ_ot_info", "occ_ot_leaves", "OccGrowthInfo", "occ_growth_step", "occ_stamped_ot_info", "occ_stamped_ot_leaves", "OccColorInfo", "OCC_COLOR_AVERAGE", "OCC_COLOR_SET", "OCC_COLOR_WHITE", "occ_color_ot_info", "occ_color_ot_leaves", "occ_color_rgb", "occ_color_words", "OccEditInfo", "OCC_EDIT_CHUNK", "OCC_EDIT_DELETE", "OCC_EDIT_SET", "OCC_EDIT_UPDATE", "OCC_TREE_LOGODDS", "OCC_TREE_MAXLIKELIHOOD", "VWDictionary", "VwdParams", "vwd_params", "vwd_validate", "limit_keypoints",
           "ERR_VWD_FULL", "VWD_L1", "VWD_L2", "VWD_NONE", "PoseGraph", "PgoParams", "PgoPlanInfo", "PgoGraph", "pgo_params", "pgo_check",
           "pgo_plan", "PGO_COUPLING_REFERENCE", "PGO_COUPLING_SYMMETRIC", "PGO_EDGE_RECORD"]
