/*
 * sbm.h -- C-ABI of the MI355X stereo block-matching disparity engine (libsbm_hip.so).
 *
 * This is the drop-in boundary for the dense-disparity provider of sdoira/U96-SLAM:
 *
 *   reference call site               src/slam/src/core/main.cpp:197-217
 *       cv::Ptr<cv::StereoBM> bm = cv::StereoBM::create(16, 9);     (main.cpp:201)
 *       bm->setROI1 ... bm->setDisp12MaxDiff(1);                    (main.cpp:202-212)
 *       bm->compute(left, right, disp);                             (main.cpp:215)
 *   alternative provider, same output  src/slam/src/core/FPGA.cpp:270-279 (receiveDepthMap)
 *   consumers of the output contract   src/slam/src/core/Stereo.cpp:79-83, SensorData.cpp:50-58,
 *                                      main.cpp:529-530
 *
 * Output contract (identical to cv::StereoBM with a CV_16SC1 destination): int16, value =
 * 16 * disparity (4 fractional bits); every rejected / uncomputable pixel holds
 * (minDisparity - 1) * 16.
 *
 * All entry points are plain C: pointers, sizes, int status codes. No exceptions, no aborts,
 * no spinning (contrast the reference's Logger.cpp:52-55). The C++ adaptor that restores the
 * cv::StereoBM spelling (create / 11 setters / compute) is include/sbm_stereobm.hpp.
 *
 * There is NO CPU backend behind this ABI: if no HIP device is usable sbm_create() fails with
 * SBM_ERR_NO_DEVICE. The CPU restatement used by the tests lives in oracle/ and is never linked here.
 *
 * Exactness. Every parameter set cv::StereoBM accepts is computed (block sizes 5..255, any minDisparity / ROI, any multiple of 16
 * disparities up to the limits below); sets inside the fast envelope -- odd block size 5..31, numDisparities <= 512, blockSize^2
 * * 2 * preFilterCap <= 65534 -- run the hand-tuned kernels (4 T pixel-disparities/s), everything else a sliding-sum kernel with
 * 32-bit sums (0.15-0.5 T, same results; up to 2048 disparities, beyond that a per-column kernel ~10x slower again).
 * Bit-exactness against cv::StereoBM is CLAIMED for blockSize^2 * 2 * preFilterCap <= 32767 only (the reference's 21 x 21
 * at cap 31 is 27 342): OpenCV keeps its block-matching cost plane as `short`, so beyond that bound its left-right check
 * would see a wrapped cost where this engine (and its oracle) keep the true one.
 *
 * Limits (SBM_ERR_UNSUPPORTED beyond them; cv::StereoBM itself has none of these): numDisparities <= 4096, at most 32 767 pairs
 * per call, image height <= 65 535. There is no width limit: the left-right check keeps a row's claim table in LDS up to 8192
 * columns and in device scratch beyond. The speckle filter's band walk serves images up to 65 535 columns and
 * (W + 288) * H < 2^27 and speckleWindowSize up to 2048; larger images or windows take its row-walking kernels (same results,
 * ~3x the stage time). tests/test_gpu_limits.py computes each of these edges and the first value past it. Disparities of 2048
 * and more do not fit the int16 map: 16 * d wraps, as cv::StereoBM's (short) cast does, and the LR check ignores a claim that
 * such a value points outside the row.
 * Device scratch per pixel of a call (n * W * H), held by the handle until the size changes: ~4 B (prefiltered planes with their
 * padding + the pre-check map), + 4 B with the LR check on (cost plane), + 8 B more when that check meets rows wider than 8192
 * columns (its claim table), + 16 * (W + 288) / W + ~2 B with the speckle filter on (run records, seam lists), + 4 B for
 * PREFILTER_NORMALIZED_RESPONSE. Every pixel of a host-memory call adds 4 B of staging. The interior SAD kernel of a batch that
 * fills the chip more than once hands its vertical sums from one row segment to the next through scratch as well: per pair,
 * column strip and row segment that can take its sums over (the segments behind the first D dispatch positions, D = the sets of
 * pairs x strips workgroups the chip holds at once, rounded up, + 1), 128 * numDisparities + 256 B (+ 8 B of flags) -- 16.25 KB at
 * 128 disparities, 174 MB for 64 KITTI pairs (19 strips, 13 segments, 9 of them linked), 72 MB for 64 pairs of 640 x 480 at 64 disparities (10 strips, 22
 * segments, 14 linked). The segment count is held to what fits 1 GiB of slots; a call whose slots would still exceed that recomputes
 * the sums instead.
 *
 * The hand-tuned kernels accumulate in place with v_mqsad_pk_u16_u8 (vdst == src2), which the hardware does right and the
 * compiler's register model forbids; a device self-test (once per device and process, on the stream of the first call that would
 * take the interior SAD kernel: pseudo-random operands, single instructions and dependent chains, at 1 / 4 / 8 wavefronts per SIMD)
 * guards it. What the self-test does NOT cover is a device that miscomputes only in instruction mixes it does not generate. If it
 * fails, or with SBM_FAST_INPLACE=0, the sliding-sum kernel takes every configuration of the interior kernel's envelope: same
 * results, 8-25x slower SAD stage; the kernel name, sbm_last_kernel_name(), then reads
 * "sad_wide_kernel [in-place accumulate unavailable]". If the self-test cannot run (one of its HIP calls fails), that call
 * returns SBM_ERR_HIP (SBM_ERR_NOMEM if its 8-byte allocation fails) with the error in sbm_last_hip_error(), nothing is
 * remembered, and the next call runs the self-test again.
 *
 * Environment. The library reads these thirteen variables (nothing else); an integrator never needs to set any of them:
 *   variable            default  read      who sets it, and what for
 *   SBM_FAST_INPLACE    1        once      0 = run the sliding-sum SAD kernel instead of the interior one (the fallback that
 *                                          is taken automatically when the device self-test of the in-place v_mqsad
 *                                          accumulate fails); set by the GPU tests to check that fallback
 *   SBM_FAST_PFSHIFT    2        once      0 = unscaled prefiltered planes (plain winner search), 1 = at most one tag bit;
 *                                          GPU tests
 *   SBM_FAST_CS3        1        per call  0 = plain column strips only (no column-stride-3 strips); GPU tests
 *   SBM_FAST_HANDOFF    1        per call  0 = every row segment of the interior SAD kernel recomputes its vertical sums from w - 1
 *                                          priming rows; 1 = a segment takes the sums its predecessor left, where they are there
 *                                          when it starts (same results either way); 2 = the segments are launches of their own,
 *                                          so that every hand-off is taken; GPU tests / A-B measurements
 *   SBM_FAST_FOLD       1        per call  0 = the last plain strip of a 128-disparity, window-15 launch runs as a plain strip even
 *                                          where it has at most 22 columns (1 = folded over its disparity halves: same results);
 *                                          GPU tests / A-B measurements
 *   SBM_FAST_NBR        1        per call  0 = the lone wavefronts of the interior SAD kernel select the winner's two neighbour sums in
 *                                          the full tree over all disparities on every row (1 = only in the groups of 32 disparities
 *                                          that a row's winners touch, the tree where they touch more than half: same results);
 *                                          GPU tests / A-B measurements
 *   SBM_SPECKLE_LISTS   1        per call  0 = the speckle filter's row-walking kernels (one wavefront per row, per-pixel labels)
 *                                          instead of the band walk + run records; GPU tests
 *   SBM_SPECKLE_BAND    auto     per call  2 / 4 = band height of the speckle filter's band walk, 0 = row-walking kernels;
 *                                          GPU tests
 *   SBM_SPECKLE_SEG     auto     per call  1 / 2 / 4 = column segments per band of the band walk (wavefronts of one workgroup that
 *                                          walk a band together; automatic: 4 for one-pair calls, 1 for frame batches); GPU tests
 *   SBM_HOST_ZEROCOPY   1        per call  0 = small host-buffer calls (sbm_compute / sbm_compute_batch up to 8 MB of maps) into
 *                                          pageable memory return their maps through a D2H copy + stream synchronisation instead of
 *                                          the copy kernel that writes pinned host memory and raises a flag the host polls; GPU
 *                                          tests / A-B measurements
 *   SBM_WIDE            1        per call  0 = configurations outside the fast envelope run the per-column kernel
 *                                          (sbm_sad_generic.hip) instead of the sliding-sum one (sbm_sad_wide.hip); GPU tests
 *   SBM_CV_READING      0        per call  bit mask of ALTERNATIVE readings of cv::StereoBM behaviours that this engine restates from
 *                                          memory and nothing in the reference can pin: 1 = getValidDisparityROI
 *                                          subtracts minDisparity from roi2's right edge (2.4 lineage), 2 = the LR check reads the cost
 *                                          plane as `short`, 4 = speckleRange * 16, 8 = the last row of an odd-height image is
 *                                          prefiltered instead of filled with preFilterCap, 16 = LR check: equal cost -> the later x
 *                                          wins. The oracle has the same bits; tests/golden/pin_kit.npz holds this engine's outputs
 *                                          under both readings of each, and tools/verify_with_opencv.py (numpy + cv2 only) names the
 *                                          reading a given OpenCV implements -- adopting it is a default flip here, not a rewrite;
 *                                          bits 32 and 64 belong to the semi-global matcher (see sbm_sgbm_params below),
 *                                          bit 128 to the ORB descriptor's blur (see sbm_orb_params below),
 *                                          bit 256 to the keypoint matcher's radius test (see sbm_match_params below),
 *                                          bit 512 to cv::goodFeaturesToTrack's float sums (see sbm_gftt_cv_params below)
 *   SBM_OCC_OT_HOST_PARSE 0      per call  1 = sbm_occ_ot_load / sbm_occ_ot_read parse the records with the one-pass host parser of
 *                                          sbm_occ_ot_info instead of on the device (same maps, same codes); GPU tests / A-B
 *                                          measurements
 * The Python mirror adds SBM_LIB_AB (file name of another build of this library inside u96-slam_amd/lib/, A-B measurements
 * only); bench.py reads SBM_BENCH_BACKEND / SBM_BENCH_FEED / SBM_BENCH_SG_FAULT (tests of its multi-process control flow).
 */
#ifndef SBM_H_
#define SBM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBM_VERSION_MAJOR 0
#define SBM_VERSION_MINOR 1

/* status codes (0 = ok). The negative "parameter" codes map 1:1 onto the CV_Error() checks at the
 * top of cv::StereoBM::compute (OpenCV calib3d, stereobm.cpp). */
enum {
  SBM_OK = 0,
  SBM_ERR_NULL = -1,             /* null handle / pointer argument                                   */
  SBM_ERR_SIZE = -2,             /* width/height <= 0, stride < width, left/right size mismatch       */
  SBM_ERR_PREFILTER_TYPE = -3,   /* preFilterType must be NORMALIZED_RESPONSE or XSOBEL               */
  SBM_ERR_PREFILTER_SIZE = -4,   /* preFilterSize must be odd and within 5..255                       */
  SBM_ERR_PREFILTER_CAP = -5,    /* preFilterCap must be within 1..63                                 */
  SBM_ERR_BLOCK_SIZE = -6,       /* blockSize must be odd, within 5..255 and < min(width,height)      */
  SBM_ERR_NUM_DISPARITIES = -7,  /* numDisparities must be > 0 and divisible by 16                    */
  SBM_ERR_TEXTURE = -8,          /* textureThreshold must be >= 0                                     */
  SBM_ERR_UNIQUENESS = -9,       /* uniquenessRatio must be >= 0                                      */
  SBM_ERR_NO_DEVICE = -20,       /* no usable HIP device / device index out of range                  */
  SBM_ERR_HIP = -21,             /* a HIP runtime call failed (see sbm_last_hip_error)                */
  SBM_ERR_NOMEM = -22,           /* device or host allocation failed                                  */
  SBM_ERR_UNSUPPORTED = -23,     /* valid OpenCV parameters this build cannot run (documented limits) */
  SBM_ERR_BATCH = -24,           /* batch count <= 0                                                  */
  SBM_ERR_OCC_FULL = -25,        /* occupancy map: points found the table full (see sbm_occ_overflow) */
  SBM_ERR_VWD_FULL = -26         /* visual-word dictionary: a call's new words did not fit (sbm_vwd_overflow) */
};

#define SBM_PREFILTER_NORMALIZED_RESPONSE 0
#define SBM_PREFILTER_XSOBEL 1

/* Parameter block: one field per cv::StereoBM setter used at main.cpp:202-212 plus the ones left at
 * their OpenCV defaults there (preFilterType, preFilterSize). roi = {x, y, width, height}; a roi with
 * width <= 0 or height <= 0 is "empty" (cv::Rect()) and means "whole image", as at main.cpp:200-203. */
typedef struct sbm_params {
  int32_t prefilter_type;      /* setPreFilterType      default SBM_PREFILTER_XSOBEL                  */
  int32_t prefilter_size;      /* setPreFilterSize      default 9 (unused by XSOBEL)                  */
  int32_t prefilter_cap;       /* setPreFilterCap       default 31                                    */
  int32_t block_size;          /* setBlockSize          default 21  (SADWindowSize)                   */
  int32_t min_disparity;       /* setMinDisparity       default 0                                     */
  int32_t num_disparities;     /* setNumDisparities     default 64                                    */
  int32_t texture_threshold;   /* setTextureThreshold   default 10                                    */
  int32_t uniqueness_ratio;    /* setUniquenessRatio    default 15                                    */
  int32_t speckle_window_size; /* setSpeckleWindowSize  default 0 (off)                               */
  int32_t speckle_range;       /* setSpeckleRange       default 0                                     */
  int32_t disp12_max_diff;     /* setDisp12MaxDiff      default -1 (off)                              */
  int32_t roi1[4];             /* setROI1                                                             */
  int32_t roi2[4];             /* setROI2                                                             */
} sbm_params;

typedef struct sbm_handle sbm_handle; /* opaque; owns a HIP stream and lazily sized device scratch */

/* Fill *p with cv::StereoBM::create(numDisparities, blockSize) defaults (0 -> 64 resp. 21). */
void sbm_params_default(sbm_params* p, int num_disparities, int block_size);

/* Check p against an image size exactly as cv::StereoBM::compute does before doing any work. */
int sbm_params_validate(const sbm_params* p, int width, int height);

/* Create an engine on HIP device `device` (>= 0). Parameters are copied. */
int sbm_create(sbm_handle** out, const sbm_params* p, int device);
void sbm_destroy(sbm_handle* h);

/* Destroyed handles are parked (streams, events and up to 512 MB of device scratch each, at most 4) so that the
 * reference's pattern -- a new matcher per frame, src/slam/src/core/main.cpp:201 -- does not pay ~2 ms of set-up per
 * frame. sbm_trim() frees everything that is parked (e.g. before the process hands the GPU to someone else). */
void sbm_trim(void);

/* Replace the parameter block (the cv::StereoBM setters). Cheap; scratch is re-sized lazily. */
int sbm_set_params(sbm_handle* h, const sbm_params* p);
int sbm_get_params(const sbm_handle* h, sbm_params* p);

/* cv::StereoBM::compute() for one pair in HOST memory (the main.cpp:215 shape): strided, row-major
 * 8-bit inputs (cv::Mat::data / cv::Mat::step), strided int16 output. Strides are in BYTES.
 * Synchronous: on return `disp` is filled. */
int sbm_compute(sbm_handle* h, const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride,
                int width, int height, int16_t* disp, size_t disp_stride);

/* Same for n independent pairs in host memory (array-of-pointers, common size and strides). */
int sbm_compute_batch(sbm_handle* h, int n, const uint8_t* const* left, size_t left_stride,
                      const uint8_t* const* right, size_t right_stride, int width, int height,
                      int16_t* const* disp, size_t disp_stride);

/* n pairs already resident in DEVICE memory, densely packed: left/right = n*height*width bytes,
 * disp = n*height*width int16. Asynchronous on the handle's stream unless `sync` is non-zero.
 * This is the entry point bench.py times (inputs resident in HBM when the timed region starts).
 * Ordering: the handle's stream is a hipStreamNonBlocking stream -- it does NOT order behind the null stream or any
 * other stream of the caller. The inputs must be complete before the call (synchronise the producing stream, or make
 * sbm_stream() wait on an event of the producer with hipStreamWaitEvent), and with sync == 0 the buffers must stay
 * alive and untouched until sbm_synchronize() or an event recorded on sbm_stream() after the call has completed.
 * Every kernel of the call runs on the handle's stream (one SAD launch: the clamped border columns are extra wavefronts
 * of it). */
int sbm_compute_device(sbm_handle* h, int n, const void* d_left, const void* d_right, int width, int height,
                       void* d_disp, int sync);

/* Asynchronous dense feed (what a per-GPU feeder thread of a multi-GPU job uses; bench.py --feed host): sbm_submit_dense
 * queues one dense batch -- left/right: n*height*width bytes each, disp: n*height*width int16, all in HOST memory that
 * should be pinned -- and returns at once; at most three submissions are in flight (a fourth call first waits for the oldest).
 * Inputs cross PCIe on an H2D stream, the kernels run on the handle's stream, the maps return on a D2H stream, so batch k+1
 * arrives while batch k computes and batch k-1 leaves (two device staging sets, re-used through stream dependencies). sbm_wait_oldest blocks until the oldest outstanding submission's maps
 * are in `disp` (returns SBM_OK at once when nothing is outstanding). The buffers of a submission must stay untouched until
 * it has been waited for. The reference's call is synchronous (main.cpp:215); this pair exists because a feeder that keeps
 * the GPU busy across calls needs it. */
int sbm_submit_dense(sbm_handle* h, int n, const uint8_t* left, const uint8_t* right, int width, int height, int16_t* disp);
int sbm_wait_oldest(sbm_handle* h);

/* Block until everything queued on the handle's stream has finished and every outstanding submission of the asynchronous
 * feed has delivered its maps. */
int sbm_synchronize(sbm_handle* h);

/* sbm_destroy() and the asynchronous feed: copies that are already queued finish first (so the `disp` buffer of every
 * submission that was followed by another submission or by a wait must still exist when the handle is destroyed); the maps of
 * the NEWEST submission, whose trip home is only queued by the next submission or by a wait, are dropped -- destroy never
 * starts a write into caller memory. Callers that want those maps call sbm_synchronize() first. */

/* One dense host batch spread over several engines -- normally one handle per GPU of the node, created with
 * sbm_create(&h[k], &params, k) ("pair batches shard embarrassingly across the GPUs"; the reference's
 * caller is a single C++ thread, src/slam/src/core/main.cpp:149-216). left / right: n*height*width bytes, disp:
 * n*height*width int16, HOST memory that should be pinned (pageable memory works, but the runtime then stages every copy
 * synchronously and the devices run one after the other). Handle k computes the contiguous block of pairs
 * [n*k/K, n*(k+1)/K) through its asynchronous feed (two submissions per block); all blocks are queued before any is waited
 * for. Blocking: on return every map is in `disp`. The handles must be distinct (SBM_ERR_BATCH otherwise), may sit on the same
 * or on different devices and keep their own parameter blocks; results equal sbm_compute_batch() of each block on its handle.
 * Every handle is drained even when one of them fails; the first failure is returned. */
int sbm_compute_batch_multi(sbm_handle* const* handles, int n_handles, int n, const uint8_t* left, const uint8_t* right,
                            int width, int height, int16_t* disp);

/* Intermediate planes of the LAST sbm_compute_device call, for stage-by-stage parity tests.
 * which: 0 = prefiltered left (u8), 1 = prefiltered right (u8), 2 = WTA cost plane (int32, valid only
 * where the pre-LR disparity is valid and disp12_max_diff >= 0), 3 = disparity before LR/speckle (int16).
 * Copies n*height*width elements into host memory `dst`. */
int sbm_debug_fetch(sbm_handle* h, int which, void* dst, size_t dst_bytes);

/* Per-stage device time in ms, measured with HIP events recorded on the handle's stream around each stage.
 * enabled = 1: every sbm_compute_device call synchronises and sbm_get_profile returns the LAST call's times;
 * enabled = 2: events are recorded without synchronising (use inside a timed region) and sbm_get_profile
 *              (which synchronises) returns the average over the calls made since enabling (last 64 at most).
 * enabled = 3: as 2, but only every 4th call is instrumented (the five event records cost ~20 us per call at the bench size;
 *              sampling keeps a timed region close to the un-instrumented rate).
 * names: "prefilter", "sad" (the SAD/WTA kernels of the call: the interior kernel -- plus, beyond 256 disparities, the two
 * launches for its clamped border columns -- or the sliding-sum / per-column kernel when the fast path is off;
 * sbm_last_kernel_name() says which), "lrcheck", "speckle", "total"; "border" is still accepted and reads 0 (up to 256
 * disparities the clamped border columns have been wavefronts of the SAD launch since round 4: no second kernel to time). */
int sbm_set_profiling(sbm_handle* h, int enabled);
int sbm_get_profile(sbm_handle* h, const char* name, float* ms);

/* Which SAD kernel the LAST sbm_compute_device call launched, as text: the template instantiation of the interior
 * kernel ("sad_fast_kernel<128,1,5,3,true> pfshift=2"), or "sad_wide_kernel" / "sad_generic_kernel" when the configuration
 * is outside the fast envelope ("sad_wide_kernel [in-place accumulate unavailable]" when it is inside but the device self-test
 * above failed or SBM_FAST_INPLACE=0). bench.py compares it with the kernel the committed counter profile was taken on, so
 * that stale counters are never attached to a different kernel. */
int sbm_last_kernel_name(sbm_handle* h, char* dst, size_t dst_bytes);

/* ---- consumers of the disparity map --------------------------------------------
 * Device-side versions of what the reference does with the map right after compute(), so that only the small
 * results have to cross PCIe:
 *   decimation      SensorData::setFeatures, src/slam/src/core/SensorData.cpp:50-58  (keeps every scale-th pixel)
 *   reprojection    projectDisparityTo3D, src/slam/src/core/Stereo.cpp:157-182, as used on the decimated map by
 *                   buildOccupancyGridMap, src/slam/src/core/main.cpp:522-553 (pt2d = (col*scale, row*scale))
 *   keypoint depth  generateKeypoints3DStereo (dense-map branch), src/slam/src/core/Stereo.cpp:53-117
 * Arithmetic follows the C++ source operation by operation (float / double exactly where the reference uses them,
 * no fused multiply-add), so results are bit-identical to the reference's expressions. Invalid points are NaN. */
typedef struct sbm_stereo_model {
  double fx_l, fy_l, cx_l, cy_l, Tx_l;  /* StereoCameraModel P[0] entries (include/core/StereoCameraModel.h:25-29) */
  double fx_r, fy_r, cx_r, Tx_r;        /* P[1] entries (:30-34)                                                   */
  float local[12];                      /* localTransform r11 r12 r13 o14 / r21.. / r31.. (Transform.h:38-41)       */
  int32_t has_local;                    /* 0 = localTransform().isNull()                                            */
} sbm_stereo_model;

/* The CV_32F form of the result (cv::StereoBM::compute into a CV_32F destination: disp16.convertTo(dst, CV_32F, 1./16)):
 * out = disp / 16 as float, exact; FILTERED pixels become (minDisparity - 1). n*height*width floats. */
int sbm_disparity_to_float_device(sbm_handle* h, int n, const void* d_disp, int width, int height, void* d_out, int sync);

/* out[p][r][c] = disp[p][r*scale][c*scale]; out planes are (height/scale) x (width/scale), densely packed. */
int sbm_decimate_device(sbm_handle* h, int n, const void* d_disp, int width, int height, int scale, void* d_out, int sync);

/* xyz[p][r][c] = projectDisparityTo3D((c*scale, r*scale), disp[p][r][c]/16.0f, model), then localTransform if
 * apply_local != 0 and the model has one; NaN triple where the disparity is <= 0 or the point is not finite.
 * width/height are those of the (possibly decimated) map; d_xyz holds n*height*width*3 floats. */
int sbm_reproject_device(sbm_handle* h, int n, const void* d_disp, int width, int height, int scale,
                         const sbm_stereo_model* model, int apply_local, void* d_xyz, int sync);

/* 3-D points of nk keypoints of ONE full-resolution disparity plane: for keypoint (x,y) the disparity is
 * disp[(int)y][(int)x]/16.0f (negative -> 0 -> invalid), range-checked with min_depth / max_depth exactly as
 * generateKeypoints3DStereo does, then localTransform. d_kpts: nk*2 floats (x,y); d_xyz: nk*3 floats. */
int sbm_keypoints3d_device(sbm_handle* h, const void* d_disp, int width, int height, const void* d_kpts, int nk,
                           const sbm_stereo_model* model, float min_depth, float max_depth, void* d_xyz, int sync);

/* ---- producers in front of the path (SURVEY.md 8f rank 2 and the prefilter half of rank 3) -------------------------
 * Device-resident versions of the two stages the reference's FPGA flavour runs before block matching, so raw camera
 * frames can enter the engine without a host round trip:
 *   rectification   inverse map: rect_remap(), src/StereoBM/src/fpga.c:303-366 (s1.24 fixed point; the RTL twin is
 *                   src/dvp/rtl/rect_rmp.v:339-572); bilinear resampling with 5-bit fractions:
 *                   src/dvp/rtl/rect_intp.v:285-404
 *   x-Sobel         stand-alone prefilter of dense images, either flavour: cv prefilterXSobel (what sbm_compute runs
 *                   internally) or the RTL's src/dvp/rtl/xsbl2.v:185-198,661-874 (clip to [-32,31], +32; rows 0 and
 *                   H-1 unwritten = 0) -- the flavour data/ref_xsbl_{l,r} was produced with.
 * Integer arithmetic throughout; results are bit-identical to the reference's C / RTL expressions. */
typedef struct sbm_rect_cam {   /* struct RECT_PARAM_CH, src/StereoBM/src/fpga.h:250-256 (one camera)                  */
  int32_t f[2];                 /* focal length x, y of the source camera, u10.16                                      */
  int32_t c[2];                 /* principal point x, y of the source camera, integer pixels                           */
  int32_t f2inv[2];             /* 1 / f2 of the rectified camera, u-8.32                                              */
  int32_t c2_f2[2];             /* c2 / f2 of the rectified camera, u0.24                                              */
  int32_t rot[3][3];            /* inverted rotation, s0.24, indexed as the firmware does (rot[row][col])              */
} sbm_rect_cam;

/* d_map: height*width*2 int16, (x, y) interleaved, source coordinates in 1/32 px (what rect_remap() stores in
 * MAT2S.data[0] / data[1]). Depends on the camera only: build once, reuse for every frame. */
int sbm_rect_map_device(sbm_handle* h, const sbm_rect_cam* cam, int width, int height, void* d_map, int sync);

/* dst[i] = bilinear(src[i], map) for n dense u8 images sharing one map:
 *   ((UL*(32-xf)*(32-yf) + UR*xf*(32-yf) + DL*(32-xf)*yf + DR*xf*yf) >> 9) + 1) >> 1, taps at (x>>5, y>>5) and +1.
 * Taps outside the source image read as 0 (the RTL reads stale line-buffer contents there; calibrated rigs keep the
 * valid region inside). */
int sbm_rect_remap_device(sbm_handle* h, int n, const void* d_src, const void* d_map, int width, int height, void* d_dst,
                          int sync);

#define SBM_PREFILTER_FLAVOUR_CV 0  /* clip(s,-cap,cap)+cap, reflect-101 rows, odd H: last row = cap */
#define SBM_PREFILTER_FLAVOUR_RTL 1 /* clip(s,-32,31)+32, rows 0 and H-1 = 0 (cap ignored)           */
/* n dense u8 images -> n dense u8 planes. */
int sbm_prefilter_device(sbm_handle* h, int n, const void* d_src, int width, int height, int flavour, int cap,
                         void* d_dst, int sync);

/* ---- the reference's own matcher: FPGA flavour (SURVEY.md 8f rank 3 + 8a row a8) -------------------------------------
 * Bit-level restatement of the block matcher the reference runs in programmable logic (src/dvp/rtl/bm*.v, fed by
 * xsbl2.v), for consumers of DEPTH_METHOD_FPGA_BM (src/slam/src/core/FPGA.cpp:270-279): 6-bit x-Sobel inputs, 10-bit
 * saturating column sums, 32-disparity phases, tournament minimum, divider-based sub-pixel fraction, optional min1/min2
 * ratio filter, int16 s11.4 output with -1 (0xFFFF) for "no disparity" and for the never-computed borders
 * (hwsz rows top and bottom, ndisp + hwsz + 1 columns left, hwsz columns right). It differs from cv::StereoBM in every
 * stage; no texture threshold, LR check or speckle filter exists in this flavour.
 * Parameters are the fields of the BM register block, struct FPGA_REG_BM (src/StereoBM/src/fpga.h:154-169) as decoded by
 * src/dvp/rtl/bm.v:172-193; the firmware programs ImageSize = 480 << 16 | 640, BmSetting = 0x00150040 (window 21,
 * 64 disparities) and leaves UniFiltCtrl at 0 (src/StereoBM/src/fpga.c:150-160). */
typedef struct sbm_fpga_params {
  int32_t width;            /* ImageSize [9:0]    */
  int32_t height;           /* ImageSize [24:16]  */
  int32_t block_size;       /* BmSetting [20:16]  wsz: odd, 3..31 */
  int32_t num_disparities;  /* BmSetting [8:0]    ndisp: multiple of 32, 32..256 (whole disparity phases) */
  int32_t uni_enable;       /* UniFiltCtrl [31]   */
  int32_t uni_mode;         /* UniFiltCtrl [16]   0: rejected pixels read 0xFFFF, 1: they read disparity 255 + 255/256 */
  int32_t uni_threshold;    /* UniFiltCtrl [9:0]  reject when min1/min2 (u0.10) > threshold */
} sbm_fpga_params;

/* Register words -> parameters, exactly the bit fields of bm.v:172-193 (no validation). */
int sbm_fpga_params_from_regs(uint32_t image_size, uint32_t bm_setting, uint32_t uni_filt_ctrl, sbm_fpga_params* out);
/* Read-back value of SAD_Size [1724h] = sad_hgt << 16 | sad_wdt (bm.v:208,249-255). */
uint32_t sbm_fpga_sad_size_reg(const sbm_fpga_params* p);
/* Limits of the RTL as status codes: field widths (width <= 1023, height <= 511), odd window 3..31, ndisp a positive
 * multiple of 32 up to 256, at least one output pixel; SBM_ERR_UNSUPPORTED for (ndisp + hwsz + 1) % 32 == 0, where the
 * RTL's output sequencer (bm_obuf2.v:239) never leaves its fill state. */
int sbm_fpga_params_validate(const sbm_fpga_params* p);
/* The matcher on n dense pairs of x-Sobel planes (what data/ref_xsbl_{l,r} are: xsbl2.v output, 0..63) resident in
 * device memory; d_disp = n*height*width int16. Asynchronous on the handle's stream unless sync != 0. */
int sbm_fpga_bm_device(sbm_handle* h, int n, const void* d_xsbl_l, const void* d_xsbl_r, const sbm_fpga_params* p,
                       void* d_disp, int sync);
/* xsbl2.v prefilter (SBM_PREFILTER_FLAVOUR_RTL) of n dense rectified pairs followed by the matcher: the whole PL
 * pipeline behind Fpga::receiveDepthMap. */
int sbm_fpga_compute_device(sbm_handle* h, int n, const void* d_left, const void* d_right, const sbm_fpga_params* p,
                            void* d_disp, int sync);

/* Host-memory form of sbm_fpga_compute_device for ONE pair, shaped like the frame Fpga::receiveDepthMap hands out
 * (src/slam/src/core/FPGA.cpp:270-279: a dense height x width CV_16SC1 image): strided 8-bit rectified inputs, strided int16
 * output, strides in bytes. Synchronous. */
int sbm_fpga_compute(sbm_handle* h, const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride,
                     const sbm_fpga_params* p, int16_t* disp, size_t disp_stride);

/* ---- GFTT minimum-eigenvalue map of the PL ----------------------------------------------------------
 * The dense half of the reference's FPGA feature detector (src/dvp/rtl/gftt_sbl.v, gftt_box.v, gftt_eig.v, gftt_obuf.v):
 * per image a height*width uint16 map of (a + c) - sqrt((a - c)^2 + 4 b^2) over 3x3 boxes of the Sobel products, rows
 * 0, 1, H-2, H-1 and columns 0, W-1 = 0, plus the maximum of the map (the GFTT `Max` register) -- exactly what
 * generateKeypoints2() consumes (src/slam/src/core/GFTT.cpp:41-170, fed by FPGA.cpp:283-291). Fixed-point steps and
 * limiters follow the RTL; its CORDIC square root is specified to +-1 LSB, this engine returns the exact floor.
 * d_img: n dense u8 images (the rectified left frames already on the device); d_eig: n*height*width uint16;
 * d_max: n uint32. width 3..1023, height 5..511 (the RTL's field widths). */
int sbm_gftt_eig_device(sbm_handle* h, int n, const void* d_img, int width, int height, void* d_eig, void* d_max, int sync);
/* Host-memory form for one image (what FPGA.cpp:283-291 builds: a CV_16UC1 map and the Max register). Synchronous. */
int sbm_gftt_eig(sbm_handle* h, const uint8_t* img, size_t img_stride, int width, int height, uint16_t* eig, size_t eig_stride,
                 uint32_t* max_out);

/* ---- GFTT keypoint selection: generateKeypoints2 (src/slam/src/core/GFTT.cpp:41-170) --------------------------------------
 * The CPU half of the reference's KPTS_METHOD_FPGA_GFTT path (main.cpp:238-243), on the device, so that the keypoints of
 * frames on the GPU go straight from sbm_gftt_eig_device to sbm_keypoints3d_device. Per map, exactly as the reference:
 *   threshold  thr = (double)(max & 0xffff) * quality_level; the candidates are the pixels with (float)eig[y][x] >= thr,
 *              1 <= y < height - 1, 1 <= x < width - 1 (max = 0: every interior pixel, zeros included);
 *   order      value descending, ties by the higher raster index y * width + x first (greaterThanPtr on a dense map);
 *   trim       min_distance >= 1: cells of cvRound(min_distance) (half to even) pixels; a candidate is rejected by an accepted
 *              point of the 3x3 cells around its own one with dx^2 + dy^2 < min_distance^2 (points two cells away are not
 *              looked at when the cell is smaller than min_distance, as in the reference); min_distance < 1: no trim;
 *   stop       after max_features accepted points when max_features > 0.
 * Output: points (x, y) as float, in acceptance order. The result with a cap is the prefix of the result without one.
 * Limits: width and height 3..2048 (SBM_ERR_SIZE below 3, SBM_ERR_UNSUPPORTED above 2048), at most 65 535 maps per call,
 * quality_level finite and >= 0, min_distance finite and in [0, 255] (SBM_ERR_UNSUPPORTED otherwise). block_size is carried
 * for the C++ adaptor (cv::KeyPoint size) only.
 * Kernels: one workgroup of 1024 threads per map; the accepted points live in a cell table of 16 B per
 * cell, ceil(width / cell) * ceil(height / cell) cells. When that table fits in LDS next to the sort keys (at 640 x 480 every
 * min_distance >= 5.5, i.e. cells of 6 and more) there is no device scratch; otherwise the tables live in device scratch held by
 * the handle, worked through in chunks of maps whose tables stay within 2 GiB (64 MiB per 2048 x 2048 map at cell 1).
 * sbm_get_profile: while profiling is enabled (any mode) these calls synchronise and record "gftt_select_eig" (the map of
 * sbm_gftt_detect_device, else 0), "gftt_select_select" and "gftt_select_total" (ms of the last call). */
typedef struct sbm_gftt_select_params {  /* generateKeypoints2's constants (GFTT.cpp:50-53) */
  int32_t max_features;     /* nfeatures, default 1500; <= 0: no limit                      */
  double quality_level;     /* qualityLevel, default 0.01                                   */
  double min_distance;      /* minDistance, default 7.0                                     */
  int32_t block_size;       /* blockSize, default 3: the size of the adaptor's cv::KeyPoint */
} sbm_gftt_select_params;

/* Fill *p with the reference's constants: 1500, 0.01, 7.0, 3. */
void sbm_gftt_select_params_default(sbm_gftt_select_params* p);
/* SBM_ERR_NULL, SBM_ERR_SIZE (width or height < 3), SBM_ERR_UNSUPPORTED (above 2048, or a parameter outside the limits above),
 * else SBM_OK. */
int sbm_gftt_select_params_validate(const sbm_gftt_select_params* p, int width, int height);
/* n dense uint16 maps in DEVICE memory (d_eig: n * height * width), d_max: n uint32 as sbm_gftt_eig_device writes them (the low
 * 16 bits are the reference's unsigned short) or NULL: each map's own maximum. cap = max_features > 0 ? max_features :
 * (width - 2) * (height - 2); d_kpts: n * cap float pairs (x, y), map i's points from i * cap * 2 on -- a slice
 * sbm_keypoints3d_device takes directly; entries past the count are left as they were; d_count: n int32. Asynchronous on the
 * handle's stream unless sync != 0. */
int sbm_gftt_select_device(sbm_handle* h, int n, const void* d_eig, const void* d_max, int width, int height,
                           const sbm_gftt_select_params* p, void* d_kpts, void* d_count, int sync);
/* Host form for ONE map, shaped like generateKeypoints2(eig, max, kpts2d): eig strided (eig_stride in bytes), max_eig the
 * register value, kpts at least cap float pairs (capacity counts pairs; SBM_ERR_SIZE below cap). *count receives the number of
 * points. Synchronous. */
int sbm_gftt_select(sbm_handle* h, const uint16_t* eig, size_t eig_stride, int width, int height, uint16_t max_eig,
                    const sbm_gftt_select_params* p, float* kpts, size_t capacity, int* count);
/* The whole KPTS_METHOD_FPGA_GFTT front end on n dense u8 frames: sbm_gftt_eig_device into d_eig / d_max (both required), then
 * sbm_gftt_select_device on them, in one call on the handle's stream. The map's limits apply: width 3..1023, height 5..511
 * (SBM_ERR_SIZE outside). */
int sbm_gftt_detect_device(sbm_handle* h, int n, const void* d_img, int width, int height, const sbm_gftt_select_params* p,
                           void* d_eig, void* d_max, void* d_kpts, void* d_count, int sync);

/* ---- GFTT keypoints of OpenCV: generateKeypoints (src/slam/src/core/GFTT.cpp:11-25; main.cpp:239) ---------------------------
 * The detector of the reference's KPTS_METHOD_CV_GFTT modes (SLAM_BATCH among them, Parameters.cpp:163-168):
 * cv::GFTTDetector::create(1500, 0.01, 7.0, 3, false, 0.04)->detect(img, kpts) (GFTT.cpp:13-24 holds those six constants), i.e.
 * cv::goodFeaturesToTrack on the 8-bit frame without a mask. OpenCV is not part of the reference tree: every step below is
 * RECALLED from OpenCV's imgproc (cornerMinEigenVal, Sobel / sepFilter2D, boxFilter, goodFeaturesToTrack), NOT pinned by anything
 * here, unless it says otherwise. The engine, oracle/gftt_cv_ref (sequential C and a numpy transcription of this text) and
 * tests/golden/pin_kit_gftt_cv.npz implement exactly this text; all arithmetic is IEEE binary32 / binary64 without contraction.
 *   scale     s = (float)(1.0 / (4 * 3 * 255.0)): 1 / (2^(aperture - 1) * blockSize * 255) in double, aperture 3, blockSize 3,
 *             rounded to float with the Sobel kernel it multiplies; f1 = s, f0 = 2 * s (exact).
 *   image     p[y][x] with BORDER_REFLECT_101 outside the frame (p[-1] = p[1], p[n] = p[n - 2]).
 *   tap       the scaled symmetric three-tap: tap(c, q) = f1 * q + f0 * c, both products and the sum rounded to float; q is the
 *             sum of the two outer samples. Bit 512 of SBM_CV_READING: tap(c, q) = fmaf(f1, q, f0 * c), what a contracting
 *             build makes of OpenCV's `s0 = f0 * c; s0 += f1 * (a + b)` (the precedent is bit 256).
 *   Dx        rows first, taps [-1, 0, 1] on the pixels: d[y][x] = p[y][x + 1] - p[y][x - 1], an exact integer; then columns:
 *             dx = tap(d[y][x], d[y - 1][x] + d[y + 1][x]) (the integer sum is exact in float).
 *   Dy        rows first: r[y][x] = tap(p[y][x], p[y][x - 1] + p[y][x + 1]) (integers, exact in float); then columns, taps
 *             [-1, 0, 1]: dy = r[y + 1][x] - r[y - 1][x], rounded to float.
 *   products  xx = dx * dx, xy = dx * dy, yy = dy * dy, each rounded to float, at every pixel of the frame.
 *   box       unnormalised 3 x 3 sum of each product plane, BORDER_REFLECT_101 OF THE PRODUCT PLANE (the product at column -1 is
 *             the product at column 1; it is not recomputed from the reflected image, whose dx changes sign there). For a float
 *             source OpenCV's box filter accumulates in double and rounds once: here, per row the three products are added
 *             left to right in double, the three row sums top to bottom in double, and the result is rounded to float. OpenCV
 *             slides its row and column sums (add the entering value, subtract the leaving one); the two agree wherever every
 *             partial sum is exact in 53 bits. That holds for the dx products (|dx| is 0 or at least about s, at most 1 / 3: 24-bit
 *             values whose exponents span about 20 bits) but is NOT shown for dy, which is a rounded difference of rounded
 *             floats and can be a tiny non-zero value where the exact difference is 0; there the last bit of the double sum --
 *             29 bits below the float result's -- could depend on the order. The order above is the contract. The alternative
 *             reading "float sums" was judged not live (createBoxFilter picks a double sum type for every float source) and has
 *             no bit; bit 1024 stays free.
 *   eig       a = xx * 0.5f; b = xy; c = yy * 0.5f; eig = (a + c) - sqrtf((a - c) * (a - c) + b * b), all float, the square
 *             root correctly rounded. Bit 512: the radicand is fmaf(a - c, a - c, b * b). Rounding can leave eig a few ulps
 *             below zero (or -0); no value is NaN.
 *   maximum   over the whole map, borders included, in the total order "numeric, -0 below +0" (the order of the float's bit
 *             pattern after the usual flip: bits ^ 0x80000000 for a clear sign bit, ~bits for a set one; the engine reduces
 *             with atomicMax on that key, so negative values order correctly too). d_max receives it as a float.
 *   threshold thr = (float)((double)maximum * quality_level); t = v > thr ? v : 0.0f (THRESH_TOZERO).
 *   candidate 1 <= y < H - 1, 1 <= x < W - 1, t != 0 and t equal to the maximum of t over the pixel's 3 x 3 neighbourhood (the
 *             dilation; every neighbour of an interior pixel is inside the frame). Each pixel of a plateau is a candidate.
 *   order     value descending (float comparison; candidates are never +-0 or NaN, so that is the order of the flipped bit
 *             pattern), ties by the HIGHER raster index y * W + x first: the deterministic greaterThanPtr the reference's
 *             own copy carries (GFTT.cpp:31-39). (A stock OpenCV that sorts by value alone leaves ties to std::sort.)
 *   trim      the cell table, the 3 x 3 cell test, the cap and the prefix property exactly as stated for generateKeypoints2 above
 *             (min_distance >= 1: cells of cvRound(min_distance); min_distance < 1: no trim; stop after max_features > 0).
 *   output    points (x, y) as float in acceptance order; the adaptor makes cv::KeyPoint(pt, (float)block_size).
 * Out of scope: the Harris response (use_harris != 0 -> SBM_ERR_UNSUPPORTED; k is carried only), masks, block_size other than
 * 3 (SBM_ERR_UNSUPPORTED), apertures other than 3, colour input, sub-pixel refinement.
 * Limits: width and height 3..2048 (SBM_ERR_SIZE below 3, SBM_ERR_UNSUPPORTED above 2048), at most 65 535 frames per call,
 * quality_level finite and >= 0, min_distance finite and in [0, 255] (SBM_ERR_UNSUPPORTED otherwise); d_eig 4-byte aligned.
 * Kernels: a tiled map kernel (frame tile with a 2-pixel halo in LDS -> products with a 1-pixel halo ->
 * box, eigenvalue, one atomicMax per workgroup), a candidate kernel that appends 64-bit keys (flipped value << 32 | raster
 * index) to a per-frame list, and one workgroup of 1024 threads per frame that sorts the list (in LDS up to 8192 keys, in the
 * list itself beyond) and runs the trim shared with generateKeypoints2. Device scratch, held by the handle: per frame of a
 * chunk 8 B times the next power of two >= (W - 2) * (H - 2) for the list (32 MiB at 2048 x 2048: every interior pixel can be a
 * candidate), 4 B per pixel when d_eig is absent, and the cell table as above; a call works through its frames in chunks whose
 * lists and maps stay within 256 MiB each (one frame at a time when a single frame is larger).
 * sbm_get_profile: while profiling is enabled (any mode) these calls synchronise and record "gftt_cv_eig" (map and maximum),
 * "gftt_cv_select" (candidates, order, trim) and "gftt_cv_total" (ms of the last call, summed over its chunks). */
typedef struct sbm_gftt_cv_params {  /* cv::GFTTDetector::create's arguments, in its order (GFTT.cpp:13-24) */
  int32_t max_features;     /* maxCorners, default 1500; <= 0: no limit                          */
  double quality_level;     /* qualityLevel, default 0.01                                        */
  double min_distance;      /* minDistance, default 7.0                                          */
  int32_t block_size;       /* blockSize, default 3 (nothing else is supported)                  */
  int32_t use_harris;       /* useHarrisDetector, default 0 (nothing else is supported)          */
  double k;                 /* Harris k, default 0.04; carried, unused                           */
} sbm_gftt_cv_params;

/* Fill *p with the reference's constants: 1500, 0.01, 7.0, 3, 0, 0.04. */
void sbm_gftt_cv_params_default(sbm_gftt_cv_params* p);
/* SBM_ERR_NULL, SBM_ERR_SIZE (width or height < 3), SBM_ERR_UNSUPPORTED (above 2048, block_size != 3, use_harris != 0, or a
 * parameter outside the limits above), else SBM_OK. */
int sbm_gftt_cv_params_validate(const sbm_gftt_cv_params* p, int width, int height);
/* The map alone: n dense u8 frames in DEVICE memory -> d_eig n * height * width float, d_max n float (NULL: not wanted).
 * Asynchronous on the handle's stream unless sync != 0. */
int sbm_gftt_cv_eig_device(sbm_handle* h, int n, const void* d_img, int width, int height, void* d_eig, void* d_max, int sync);
/* generateKeypoints on n dense u8 frames in DEVICE memory. d_kpts / d_count exactly as sbm_gftt_select_device writes them (cap =
 * max_features > 0 ? max_features : (width - 2) * (height - 2); frame i's float pairs from i * cap * 2; entries past the count are
 * left as they were), so sbm_orb_describe_device and sbm_keypoints3d_device take them as they are. d_eig (n * height * width
 * float) and d_max (n float) are optional outputs: NULL = not wanted. Asynchronous on the handle's stream unless sync != 0. */
int sbm_gftt_cv_detect_device(sbm_handle* h, int n, const void* d_img, int width, int height, const sbm_gftt_cv_params* p,
                              void* d_eig, void* d_max, void* d_kpts, void* d_count, int sync);
/* The selection alone, on maps the caller already has: d_eig n * height * width float and d_max n float (both required, read
 * only; a d_max that is not the map's maximum moves the threshold, nothing else). Values must not be NaN. The sibling of
 * sbm_gftt_select_device; it is also how a map of equal values -- every interior pixel a candidate, which no frame produces
 * through the map above, whose reflected border forces dx = 0 in column 0 -- reaches the ordering and the trim. */
int sbm_gftt_cv_select_device(sbm_handle* h, int n, const void* d_eig, const void* d_max, int width, int height,
                              const sbm_gftt_cv_params* p, void* d_kpts, void* d_count, int sync);
/* Host form for ONE frame, shaped like generateKeypoints(img, kpts2d): img strided (img_stride in bytes), kpts at least cap float
 * pairs (capacity counts pairs; SBM_ERR_SIZE below cap), *count receives the number of points. Synchronous. */
int sbm_gftt_cv_detect(sbm_handle* h, const uint8_t* img, size_t img_stride, int width, int height, const sbm_gftt_cv_params* p,
                       float* kpts, size_t capacity, int* count);
/* sbm_orb_features_cv_device, this detector followed by the descriptors in one call, is declared with the ORB entry points. */

/* ---- ORB descriptors: computeDescriptor (src/slam/src/opencv/CvORB.cpp; main.cpp:246-248) ----------------------------------
 * The reference's descriptor step for the keypoints generateKeypoints2 produces (cv::KeyPoint(pt, blockSize): angle -1, octave
 * 0), on the device, so that a frame's keypoints, descriptors and depth stay there. What the reference computes at level 0:
 *   blur      GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) of the image-sized ROI of the frame's reflect-101 bordered copy. The
 *             ROI is a sub-matrix without BORDER_ISOLATED, so (recalled, not pinned) OpenCV takes sepFilter2D's 8-bit path:
 *             taps cvRound(256 g) of getGaussianKernel(7, 2) = [18, 34, 49, 55, 49, 34, 18] (they sum to 257), exact integer
 *             row sums r, column sums S = sum k_j r_j, out = min(255, round(S / 2^16)); the pixels around the ROI are the
 *             unblurred frame's reflect-101 copy. Rounding of S / 2^16 ties: half to even (the vectorised column filter, every
 *             column at width 640), or half up with bit 128 of SBM_CV_READING (the scalar tail's (S + 32768) >> 16).
 *   border    runByImageBorder(kpts, size, edge_threshold): the points outside Rect(Point(e, e), Point(W - e, H - e)) are
 *             erased, keeping the order; all of them when W <= 2e or H <= 2e. Rect::contains receives the point converted to
 *             Point by saturate_cast, i.e. cvRound (half to even) -- recalled, not pinned; GFTT's integral points do not care.
 *   describe  a = (float)cos(angle * (float)(CV_PI / 180.f)), b = (float)sin(...) (in double); per pattern point p, in float
 *             without contraction, dx = cvRound(p.x * a - p.y * b), dy = cvRound(p.x * b + p.y * a); byte i of a descriptor
 *             holds in bit k blur[c + d(16i + 2k)] < blur[c + d(16i + 2k + 1)], c = (cvRound(y), cvRound(x)).
 * The pattern is the caller's: 512 points (x, y) as 1024 ints, pairs of consecutive points compared -- the reference passes
 * bit_pattern_31_2 from its CvORB.h. Coordinates in [-13, 13] (SBM_ERR_UNSUPPORTED outside), so that every sample lies within 18
 * pixels of its centre. Scope: level 0, one angle per call, WTA_K 2, 32-byte descriptors, no mask.
 * Limits (status codes): width and height 1..8192 (SBM_ERR_SIZE outside; at or below 2 * edge_threshold every keypoint is
 * erased and nothing is blurred -- count 0, not an error), at most 65 535 frames per call (SBM_ERR_UNSUPPORTED), cap >= 1
 * (SBM_ERR_SIZE); device pointers d_kpts / d_kpts_out 8-byte and d_desc 4-byte aligned (SBM_ERR_UNSUPPORTED).
 * Kernels: a tiled blur of every frame, a per-frame compaction, and the descriptors over all (frame,
 * keypoint) slots. Without d_blur the blurred frames go to handle-owned scratch, in chunks of frames of at most 256 MiB.
 * sbm_get_profile: while profiling is enabled (any mode) these calls synchronise and record "orb_blur", "orb_desc" (compaction
 * and descriptors) and "orb_total" (ms of the last call; sbm_orb_features_device's keypoint detection is not in them). */
typedef struct sbm_orb_params {
  int32_t edge_threshold;   /* edgeThreshold, default 19; 18..4096 (samples reach 18 pixels from the centre)       */
  float angle;              /* the keypoints' shared cv::KeyPoint::angle in degrees, default -1; finite          */
  int32_t blur_ksize;       /* GaussianBlur's kernel size: 7, the reference's (nothing else is supported)        */
  double blur_sigma;        /* GaussianBlur's sigma: 2.0, the reference's (nothing else is supported)            */
} sbm_orb_params;

/* Fill *p with the reference's values: 19, -1, 7, 2.0. */
void sbm_orb_params_default(sbm_orb_params* p);
/* SBM_ERR_NULL, SBM_ERR_UNSUPPORTED (a field outside the limits above), else SBM_OK. */
int sbm_orb_params_validate(const sbm_orb_params* p);
/* n dense u8 frames in DEVICE memory (d_img: n * height * width); keypoints in the layout sbm_gftt_select_device writes: frame
 * i's float (x, y) pairs from d_kpts + i * cap * 2, d_count n int32 read on the device (clamped to [0, cap]). Writes the kept
 * keypoints (stable order, same layout; d_kpts_out == d_kpts is allowed), the kept counts d_count_out (n int32; may be
 * d_count), and the descriptors d_desc (n * cap * 32 bytes, row j of frame i at (i * cap + j) * 32; rows past the kept count
 * are left as they were). d_blur: NULL, or n * height * width bytes that receive the blurred frames (untouched when width or
 * height <= 2 * edge_threshold). pattern: 1024 host ints. Asynchronous on the handle's stream unless sync != 0. */
int sbm_orb_describe_device(sbm_handle* h, int n, const void* d_img, int width, int height, int cap, const void* d_kpts,
                            const void* d_count, const int* pattern, const sbm_orb_params* p, void* d_kpts_out, void* d_count_out,
                            void* d_desc, void* d_blur, int sync);
/* Host form for ONE frame, shaped like computeDescriptor(image, noArray(), kpts, true, desc): img strided (img_stride in
 * bytes), count float (x, y) pairs in kpts; the kept pairs go to kpts_out (count entries; may be kpts), their number to
 * *count_out, their descriptors to desc (32 bytes each). Synchronous. */
int sbm_orb_describe(sbm_handle* h, const uint8_t* img, size_t img_stride, int width, int height, const float* kpts, int count,
                     const int* pattern, const sbm_orb_params* p, float* kpts_out, int* count_out, uint8_t* desc);
/* The whole KPTS_METHOD_FPGA_GFTT + desc front end on n dense u8 frames: sbm_gftt_detect_device (d_eig, d_max, d_kpts, d_count
 * as there; cap = the selection's), then sbm_orb_describe_device on its output with the keypoints compacted in place, in one
 * call on the handle's stream. The eigenvalue map's limits apply: width 3..1023, height 5..511 (SBM_ERR_SIZE outside). */
int sbm_orb_features_device(sbm_handle* h, int n, const void* d_img, int width, int height, const sbm_gftt_select_params* gp,
                            const int* pattern, const sbm_orb_params* p, void* d_eig, void* d_max, void* d_kpts, void* d_count,
                            void* d_desc, void* d_blur, int sync);

/* The whole KPTS_METHOD_CV_GFTT + desc front end (SLAM_BATCH's) on n dense u8 frames: sbm_gftt_cv_detect_device (d_eig, d_max
 * optional as there), then sbm_orb_describe_device on its output with the keypoints compacted in place, in one call on the
 * handle's stream. The detector's limits apply. */
int sbm_orb_features_cv_device(sbm_handle* h, int n, const void* d_img, int width, int height, const sbm_gftt_cv_params* gp,
                               const int* pattern, const sbm_orb_params* p, void* d_eig, void* d_max, void* d_kpts, void* d_count,
                               void* d_desc, void* d_blur, int sync);

/* ---- keypoint matching: computeTransform's matchingNoGuess / matchingGuess (src/slam/src/core/Registration.cpp) --------------
 * What the reference does with a frame's descriptors first: match the current frame against the key frame, brute force on the
 * first frame and after a failed guess (matchingNoGuess, Registration.cpp:311-335), else guided by the motion guess
 * (matchingGuess, :250-303). Restated bit for bit, for 32-byte descriptor rows; Hamming distance = popcount(a XOR b), 0..256.
 *   k-NN-2    over a query's candidate set, in increasing train index, as batchDistance inserts: a candidate enters only on a
 *             strictly smaller distance, so on equal distances the lower index ranks first. Result: best (index, d0), second d1.
 *   NNDR      accept when (float)d0 < nndr * (float)d1, in float (nndr = 0.8f). For every d0, d1 in 0..256 this equals
 *             5 * d0 < 4 * d1: a tie between the two best is always rejected, so the tie order never changes an output.
 *   no-guess  queries: from-rows 0..nf-1; candidates: all nt to-rows; a query matches its best row when NNDR passes. nt == 0: no
 *             pairs. nt == 1: the reference reads matches[i][1] out of range (undefined); defined here as NO pairs.
 *   guided    queries: the from-points whose projection is valid (see projection), in increasing from-index; a to-keypoint is a
 *             candidate when sqrtf(dx * dx + dy * dy) < radius (radius = 40.0f; float, each product rounded, the sum unfused, the
 *             square root correctly rounded, a strict <) -- recalled from OpenCV's radiusMatch / normL2Sqr, not pinned; bit 256 of
 *             SBM_CV_READING reads the sum as fmaf(dy, dy, dx * dx) (an aarch64 OpenCV build may contract). The engine compares
 *             the sum with the least float whose rounded square root reaches the radius (just below 1600 for 40: NOT d2 < 1600).
 *             0 candidates: no match; exactly 1: that candidate, WITHOUT NNDR (:207-210); 2 or more: k-NN-2 + NNDR over them.
 *   unique    (both modes) a match (q -> t) is kept iff q is the smallest query index whose accepted match is t: the std::set
 *             rule, a rejected duplicate does not fall back to its second best. Pairs (from, to) as int32, increasing from.
 *   project   (matchingGuess_Projection, :36-74) T = guessCameraRef as a 3x4 float matrix (computed by the caller), K = fx, fy,
 *             cx, cy (double), W x H the camera model's image size. Per point p (float x, y, z; NaN = no depth): zc = T's third
 *             row applied to p in float, unfused, left to right (transformPoint, Stereo.cpp:189-198); X = R p + t in double with
 *             R, t promoted from T; inv = Z != 0 ? 1.0 / Z : 1.0; u = (float)(X * inv * fx + cx), v likewise; valid iff
 *             0 < u < W - 1 && 0 < v < H - 1 && zc > 0; invalid points are written as (NaN, NaN), so a NaN point is never valid.
 *             NOT reproduced: OpenCV's Rodrigues round trip (R -> rvec -> R, through an SVD) and its zero-distortion terms, so
 *             projected coordinates can differ from cv::projectPoints in the last bits; that can only matter within rounding of
 *             the 40 px radius or of the image-border bounds. The guided matcher is exact given its projected points (a caller with
 *             OpenCV may pass cv::projectPoints' output to sbm_match_guess_device instead).
 * Store layout: descriptors and counts exactly as sbm_orb_describe_device writes them -- frame i's rows from d_desc + i * cap * 32,
 * d_count n int32 read on the device and clamped to [0, cap]. A job is a (from frame, to frame) pair of frames in [0, n);
 * from == to and repeated frames are allowed. Job j's pairs go to d_pairs + j * cap (int32 pairs), their number to d_npairs[j].
 * d_knn (NULL, or m * cap records of 4 int32, for tests and diagnostics): per query slot (best index, d0, d1, candidate count)
 * over its candidate set; best = -1 and d0 / d1 = 257 where there are fewer candidates; slots past the from-count hold
 * (-1, 257, 257, 0).
 * Limits (status codes): n, m >= 1 (SBM_ERR_BATCH), m <= 65 535 (SBM_ERR_UNSUPPORTED), cap 1..65 535 (SBM_ERR_SIZE), every frame
 * index in [0, n) (SBM_ERR_SIZE); d_desc and d_knn 16-byte, d_pairs, d_kpts and d_proj 8-byte, d_count, d_npairs and d_xyz
 * 4-byte aligned (SBM_ERR_UNSUPPORTED).
 * Kernels: k-NN over (job, 64-query tile, train slice) with partial records, a claim kernel (merge, NNDR,
 * atomicMin of the query into its train row's owner slot), and one workgroup per job that emits the owners' pairs. Up to 64
 * jobs per launch sequence; handle scratch for one launch stays within 256 MiB. Everything is enqueued on the handle's stream;
 * nothing synchronises the host unless sync != 0 (the counts stay on the device).
 * sbm_get_profile: while profiling is enabled (any mode) these calls synchronise and record "match_knn", "match_unique" (claim +
 * emit), "match_project" and "match_total" (ms of the last call). */
typedef struct sbm_match_params {
  float nndr;     /* NNDR ratio, default 0.8f; finite, in (0, 1]        */
  float radius;   /* guided search radius in pixels, default 40.0f; > 0 */
} sbm_match_params;

/* Fill *p with the reference's values: 0.8f, 40.0f. */
void sbm_match_params_default(sbm_match_params* p);
/* SBM_ERR_NULL, SBM_ERR_UNSUPPORTED (a field outside the limits above), else SBM_OK. */
int sbm_match_params_validate(const sbm_match_params* p);
/* The launch plan of a matching or projection call over m jobs on a store of capacity cap, as the calls below compute and
 * execute it; depends on (cap, m) alone. No handle, no device: tests ask it which path a shape takes.
 *   k-NN      grid (qtiles, nslice, jobs of the launch): query tiles of 64 slots, train slices of slice_rows rows (a multiple of
 *             64; (nslice - 1) * slice_rows < cap <= nslice * slice_rows, 1 <= nslice <= 32). A job reads the first
 *             ceil(nt / slice_rows) slices' partial records.
 *   launches  jobs_per_launch = min(m, 64) jobs per k-NN / claim / emit sequence, launches = ceil(m / jobs_per_launch) of them;
 *             sbm_project_points_device: proj_jobs_per_launch = min(m, 32), proj_launches = ceil(m / 32).
 *   scratch   scratch_bytes = jobs_per_launch * cap * (16 * nslice + 8) of handle scratch, at most 256 MiB.
 * sbm_match_plan: SBM_ERR_NULL (out), SBM_ERR_SIZE (out_bytes != sizeof(sbm_match_plan_info)), then the limits above in the calls'
 * order: m < 1 SBM_ERR_BATCH, cap outside 1..65 535 SBM_ERR_SIZE, m > 65 535 SBM_ERR_UNSUPPORTED (*out zeroed). */
typedef struct sbm_match_plan_info {
  int32_t qtiles, nslice, slice_rows;
  int32_t jobs_per_launch, launches;
  int32_t proj_jobs_per_launch, proj_launches;
  int32_t pad;
  int64_t scratch_bytes;
} sbm_match_plan_info;
int sbm_match_plan(int cap, int m, sbm_match_plan_info* out, size_t out_bytes);
/* matchingNoGuess for m jobs over a store of n frames (jobs: 2 * m host ints, copied with the call). */
int sbm_match_device(sbm_handle* h, int n, int m, const int* jobs, const void* d_desc, const void* d_count, int cap,
                     const sbm_match_params* p, void* d_pairs, void* d_npairs, void* d_knn, int sync);
/* matchingGuess's matching for m jobs: d_kpts holds the frames' keypoints in the layout sbm_orb_describe_device leaves its kept
 * keypoints in (frame i's float (x, y) pairs from i * cap * 2; the to-frames' are read), d_proj job j's cap projected float pairs
 * from j * cap * 2 as sbm_project_points_device writes them (a NaN coordinate has no candidates). */
int sbm_match_guess_device(sbm_handle* h, int n, int m, const int* jobs, const void* d_desc, const void* d_count, int cap,
                           const void* d_kpts, const void* d_proj, const sbm_match_params* p, void* d_pairs, void* d_npairs,
                           void* d_knn, int sync);
/* matchingGuess_Projection for m jobs: job j projects frame from[j]'s points (d_xyz: frame i's float (x, y, z) from i * cap * 3,
 * each slice as sbm_keypoints3d_device writes it; count d_count[from[j]]) with its own T (T + 12 j, host), into d_proj + j * cap * 2;
 * slots past the count are written as NaN. K: fx, fy, cx, cy (host). Limits as above, width and height >= 1 (SBM_ERR_SIZE). */
int sbm_project_points_device(sbm_handle* h, int n, int m, const int* from, const void* d_xyz, const void* d_count, int cap,
                              const float* T, const double* K, int width, int height, void* d_proj, int sync);
/* Host forms for ONE job, shaped like the reference's calls, synchronous: descriptor rows strided (strides in bytes, >= 32),
 * pairs receives up to nf int32 pairs, *npairs their number. nf or nt may be 0; max(nf, nt) <= 65 535 (SBM_ERR_SIZE). */
int sbm_match(sbm_handle* h, const uint8_t* desc_from, size_t stride_from, int nf, const uint8_t* desc_to, size_t stride_to, int nt,
              const sbm_match_params* p, int* pairs, int* npairs);
/* matchingGuess: xyz_from nf float (x, y, z) points, kpts_to nt float (x, y) keypoints, both descriptor sets, T (12 floats), K
 * (4 doubles), the image size; projection included. */
int sbm_match_guess(sbm_handle* h, const float* xyz_from, const float* kpts_to, const uint8_t* desc_from, size_t stride_from, int nf,
                    const uint8_t* desc_to, size_t stride_to, int nt, const float* T, const double* K, int width, int height,
                    const sbm_match_params* p, int* pairs, int* npairs);

/* ---- motion estimation: computeTransform's estimateMotion (src/slam/src/core/Registration.cpp:337-397) -----------------------
 * What the reference does with the matcher's pairs: estimateMotion3DTo2D (MotionEstimation.cpp:59-241) -> its solvePnPRansac
 * (:243-374, refineIterations 1, minInliers 20, refineSigma 3) -> cv3::solvePnPRansac / RANSACPointSetRegistrator
 * (src/slam/src/opencv/CvSolvePnP.cpp). Restated as follows, per job (from frame f, to frame t, the matcher's pairs):
 *   gather    (MotionEstimation.cpp:85-118, Registration.cpp:337-365) over the pairs in increasing from-index (std::map order,
 *             the matcher's output order): object point xyz_from[f], image point kpts_to[t]; a pair whose 3-D point is not finite
 *             in all three coordinates is dropped (and so is a pair with an index outside [0, min(count, cap))). N = what remains,
 *             the reference's num_matches; matches = their from-indices. The motion guess has NO effect on the output (EPnP ignores
 *             useExtrinsicGuess, the refine starts from the RANSAC model, and the guess is echoed only when RANSAC fails, which
 *             returns a null transform), so no guess is taken. N < min_inliers: SBM_PNP_FEW_MATCHES.
 *   RANSAC    (CvSolvePnP.cpp:112-210, 216-236, 326-419) six-point EPnP hypotheses, at most `iterations`, confidence 0.99.
 *             cv::RNG((uint64)-1) re-seeded per job; uniform(0, N) = the multiply-with-carry step state = (uint64)(unsigned)state *
 *             4164903690 + (state >> 32), draw (unsigned)state % N; getSubset redraws duplicates; no partial-subset checks and the
 *             default checkSubset, so the subsets depend on N alone. Inlier test: computeError returns the NORM of the residual
 *             and findInliers compares it with threshold * threshold: err <= 4.0f px for reprojection_error 2. A hypothesis
 *             becomes the best iff its count > max(best, 5) (the earliest wins a tie), and then niters = RANSACUpdateNumIters(0.99,
 *             (N - count) / N, 6, niters). N == 6: one EPnP on all six, every point an inlier, no scoring. The final EPnP over
 *             all inliers (:180-184) is dead (its pose is overwritten by the best model; EPnP always succeeds): not run. P3P
 *             (N == 4) cannot be reached. No hypothesis scores above 5: SBM_PNP_NO_MODEL (no inliers).
 *   refine    (MotionEstimation.cpp:291-373) when the RANSAC inliers number >= min_inliers and refine_iterations > 0: per round,
 *             cv::solvePnP(ITERATIVE, useExtrinsicGuess) on the current inlier set (Levenberg-Marquardt, at most 20 iterations),
 *             then computeReprojErrors over all N points (e = (float)norm(residual) <= threshold, no squaring here), the float
 *             variance and threshold = min(reprojection_error, refine_sigma * sqrt(variance)); the loop breaks when the new set
 *             has fewer than min_inliers points or equals the current one. The std::swap pair at the end: on a normal exit the
 *             inlier list is the set the last solve RAN ON (for one round: the RANSAC set), on a break the set the last
 *             reprojection PRODUCED. The pose is always the refined one (new_rvec shares rvec's data).
 *   result    (MotionEstimation.cpp:120-241) final inliers < min_inliers: SBM_PNP_FEW_RANSAC_INLIERS (no refine ran) or
 *             SBM_PNP_FEW_REFINED_INLIERS, null transform. Else SBM_PNP_OK: R = Rodrigues(rvec), transform =
 *             (localTransform * pnp).inverse() in the reference's float Transform arithmetic, and the covariance scales: medians
 *             (element size >> 1 after sorting) of the squared 3-D distances and of the acos angles over the inliers whose
 *             xyz_to[t] is finite, each clamped below at 1e-4 (1 when there is no such inlier: covariance = identity). The inlier
 *             list (from-indices) is written whatever the status, as the reference returns it.
 * Deviations and readings (recalled from OpenCV code that is not vendored, NOT pinned -- as the radius test of the matcher):
 * EPnP's control points (PCA of the points), barycentric coordinates (cvInvert by SVD), M^T M and its SVD, the betas
 * (cvSolve by SVD) and epnp::qr_solve's Gauss-Newton; cv::SVD as a one-sided Jacobi SVD with hypot read as sqrt(p*p + b*b);
 * undistortPoints' float normalisation of the image points; projectPoints' zero-distortion arithmetic; Rodrigues both ways
 * (R -> rvec without OpenCV's SVD re-orthonormalisation); CvLevMarq's step schedule (lambda 10^-3, x10 on a worse error up to
 * 10^16, /10 otherwise, stop at 20 iterations or a relative step < FLT_EPSILON) and its 6 x 6 solve by SVD; the Eigen float
 * product, quaternion renormalisation and 4 x 4 inverse of Transform. RANSAC scores each hypothesis with R, t as EPnP
 * produced them (OpenCV round-trips through rvec; that moves the pose by ulps). With has_local == 0 (or no model) the
 * localTransform product is skipped.
 * Of these, what is mathematics is now held to an independent statement (tests/pnp_independent.py: expm, mpmath derivatives,
 * numpy.linalg, scipy's LM; DESIGN.md section 12 lists blocks, inputs and bounds): the SVD and both solvers, Rodrigues with
 * dR/dr and its inverse, the LM residual, Jacobian, accumulators and damped step, the refined pose as a minimum, the projection
 * gate, the float variance, the Transform product / inverse and the covariance terms and medians. What stays a reading, seen
 * and kept: the SVD's cut-off, the lambda schedule, z == 0 left undivided, no rvec round trip, and Rodrigues' inverse within
 * 1e-5 of pi, which answers with the rule for pi itself (x >= 0, the signs of y and z from R01 and R02): the vector is then off
 * by up to 2 (pi - angle) as a rotation, and is -r where the axis has x < 0 (2.2e-7 measured at pi - 1e-7).
 * Parity contract (GPU vs the sequential C restatement, oracle/pnp_ref): bit for bit -- N, every subset, every hypothesis' R, t
 * and count, the best iteration, the final niters and the RANSAC inliers. Refined pose (rvec, tvec, R): 1e-9 relative (the
 * transcendental functions of Rodrigues differ between host and device libraries by ulps); transform and covariance scales:
 * float ulps (4 ulps relative to the largest entry); status, num_matches, num_inliers and the inlier list exact except for a
 * point whose residual lies within 1e-6 px of the refine threshold. A degenerate job whose refine runs the translation off
 * towards infinity (|t| >= 1e6, e.g. every image point alike) amplifies those ulps without bound: only its exact fields are
 * compared. RANSACUpdateNumIters' log / pow differ between libraries
 * too: for every N <= 4096 and every count, num / denom lies farther than 1e-9 from a multiple of 0.5, so the rounding, and
 * with it niters, cannot differ (tests/test_pnp_restatement.py walks it). That argument is shown for N <= 4 096 only; above it
 * (up to the cap, 65 535) bit-for-bit niters and best iteration are expected but not proven.
 * Store layout: d_xyz frame i's float (x, y, z) from i * cap * 3 (sbm_keypoints3d_device per frame), d_kpts frame i's float
 * (x, y) from i * cap * 2 (sbm_orb_describe_device's kept keypoints), d_count n int32 clamped to [0, cap]; job j = (from, to)
 * frames in [0, n) reads the pairs d_pairs + j * cap (int32 pairs) and d_npairs[j] (clamped to [0, cap]) as sbm_match*_device
 * writes them. Out: d_result m records; d_inliers m * cap int32, job j's list from j * cap (slots past num_inliers untouched);
 * d_hyp NULL, or m * iterations sbm_pnp_hypothesis (for tests: every hypothesis, whether or not the RANSAC loop reached it;
 * jobs without RANSAC hold subset -1, count -1, R = t = 0; N == 6: record 0 is the one solve, count 6).
 * Limits (status codes): n, m >= 1 (SBM_ERR_BATCH), m <= 65 535 (SBM_ERR_UNSUPPORTED), cap 1..65 535 (SBM_ERR_SIZE), every
 * frame index in [0, n) (SBM_ERR_SIZE), K finite with fx, fy != 0 (SBM_ERR_UNSUPPORTED); d_xyz, d_count, d_npairs, d_inliers
 * 4-byte, d_kpts, d_pairs, d_result and d_hyp 8-byte aligned (SBM_ERR_UNSUPPORTED).
 * Kernels: gather + draw (one workgroup per job), hypotheses (one lane per (job, iteration)), score (one
 * wavefront per (job, iteration)), finish (one wavefront per job: the RANSAC replay, the refine with wavefront reductions, the
 * transform and the covariance medians). Up to 64 jobs per launch sequence; handle scratch stays within 256 MiB. Everything is
 * enqueued on the handle's stream; nothing synchronises the host unless sync != 0.
 * sbm_get_profile: while profiling is enabled these calls synchronise and record "pnp_hyp" (gather, draw, hypotheses),
 * "pnp_score", "pnp_refine" (replay, refine, result) and "pnp_total" (ms of the last call). */
enum {
  SBM_PNP_OK = 0,
  SBM_PNP_FEW_MATCHES = 1,          /* N < min_inliers                                */
  SBM_PNP_NO_MODEL = 2,             /* RANSAC found no model                          */
  SBM_PNP_FEW_RANSAC_INLIERS = 3,   /* RANSAC's inliers < min_inliers (no refine ran) */
  SBM_PNP_FEW_REFINED_INLIERS = 4   /* the refine left < min_inliers                  */
};

typedef struct sbm_pnp_params {
  int32_t min_inliers;        /* minInliers, default 20; 6..65 535                                     */
  int32_t refine_iterations;  /* refineIterations, default 1; 0..100                                   */
  int32_t iterations;         /* RANSAC's iterationsCount, default 300; 1..1000                        */
  float reprojection_error;   /* default 2.0f; finite, > 0 (RANSAC gates at its square)                */
  float refine_sigma;         /* default 3.0f; finite, >= 0                                            */
  int32_t pad;
  double confidence;          /* default 0.99; in (0, 1)                                               */
} sbm_pnp_params;

/* One job's result: 216 bytes. */
typedef struct sbm_pnp_result {
  int32_t status;            /* SBM_PNP_*                                                               */
  int32_t num_matches;       /* N                                                                       */
  int32_t num_inliers;       /* length of the job's inlier list                                        */
  int32_t ransac_inliers;    /* the best hypothesis' count (0 without a model)                         */
  int32_t best_iteration;    /* the RANSAC iteration of the model, -1 without one                      */
  int32_t niters;            /* RANSAC's final niters (0 when RANSAC did not run)                      */
  int32_t refine_solves;     /* LM solves the refine ran                                               */
  int32_t refine_exit;       /* -1 not run, 0 normal exit, 1 break: too few, 2 break: unchanged        */
  double rvec[3];            /* the PnP pose (camera from object): rotation vector, translation, R    */
  double tvec[3];
  double R[9];
  double cov_dist;           /* covariance scales: the 3 x 3 blocks of the identity are multiplied by */
  double cov_angle;
  float transform[12];       /* (localTransform * pnp).inverse(), 3 x 4 row-major; zeros unless OK    */
} sbm_pnp_result;

/* One RANSAC hypothesis (d_hyp): 128 bytes. */
typedef struct sbm_pnp_hypothesis {
  int32_t subset[6];
  int32_t count;             /* inliers at err <= reprojection_error^2                                  */
  int32_t pad;
  double R[9];
  double t[3];
} sbm_pnp_hypothesis;

/* Fill *p with the reference's values: 20, 1, 300, 2.0f, 3.0f, 0.99. */
void sbm_pnp_params_default(sbm_pnp_params* p);
/* SBM_ERR_NULL, SBM_ERR_UNSUPPORTED (a field outside the limits above), else SBM_OK. */
int sbm_pnp_params_validate(const sbm_pnp_params* p);
/* estimateMotion for m jobs (jobs: 2 * m host ints (from, to), copied with the call). K: fx, fy, cx, cy of the left camera (host
 * doubles); model: NULL or the camera model whose localTransform (local, has_local) applies. */
int sbm_estimate_motion_device(sbm_handle* h, int n, int m, const int* jobs, const void* d_xyz, const void* d_kpts, const void* d_count,
                               int cap, const void* d_pairs, const void* d_npairs, const double* K, const sbm_stereo_model* model,
                               const sbm_pnp_params* p, void* d_result, void* d_inliers, void* d_hyp, int sync);
/* Host form for ONE job, shaped like estimateMotion: xyz_from nf float (x, y, z), kpts_to and xyz_to nt float pairs / triples,
 * npairs (from, to) int32 pairs; inliers receives up to npairs from-indices. Synchronous. max(nf, nt, npairs) <= 65 535. */
int sbm_estimate_motion(sbm_handle* h, const float* xyz_from, int nf, const float* kpts_to, const float* xyz_to, int nt,
                        const int* pairs, int npairs, const double* K, const sbm_stereo_model* model, const sbm_pnp_params* p,
                        sbm_pnp_result* result, int* inliers);

/* ---- semi-global matcher: cv::StereoSGBM (the reference's DEPTH_METHOD_CV_SGBM, main.cpp:218-234) -------------------------
 * Restatement of cv::StereoSGBM::compute() for 8-bit single-channel pairs in MODE_HH (two passes, 8 paths: the reference's
 * mode, main.cpp:219-230) and MODE_SGBM (OpenCV's default: one pass, 5 paths). Output contract as for the block matcher:
 * int16, 1/16 px, invalid pixels hold (minDisparity - 1) * 16. Stages: Birchfield-Tomasi costs on the clipped x-Sobel and on
 * the raw image (that one >> 2), summed over the block with clamped borders -> C (int16, biased by P2 as OpenCV keeps it) over
 * the width1 = maxX1 - minX1 computable columns -> path sweeps summed into S -> winner-take-all, uniqueness, parabolic sub-pixel
 * and SGBM's own left-right check through its claim table -> 3x3 median (replicated border) -> speckle filter with
 * 16 * speckleRange. Parameters are passed per call and run on an existing handle (its stream and device).
 *
 * Exactness envelope. With blockSize_eff = 2 * (blockSize / 2) + 1 (blockSize <= 0 -> 5), ftzero = max(preFilterCap, 15) | 1
 * and P2_eff = max(P2 > 0 ? P2 : 5, P1_eff + 1), every call with blockSize_eff^2 * (2 * ftzero + 63) + P2_eff <= 32767 is
 * computed; inside it every path cost lies in [C - P2_eff, C] and is non-negative, so OpenCV's two saturating int16 sums equal
 * min(32767, sum of all path costs) in any order, which is what the engine computes. Outside it OpenCV's int16 casts wrap; such
 * calls return SBM_ERR_UNSUPPORTED (the reference's call is at 12 253). Other limits (SBM_ERR_UNSUPPORTED beyond them):
 * numDisparities <= 512, width <= 8192, height <= 65 535, preFilterCap <= 63, uniquenessRatio <= 65 535, minDisparity >= -2047
 * and minDisparity + numDisparities <= 2047 (every disparity * 16 fits the int16 map), speckleRange >= 0 when the speckle filter
 * is on, at most 32 767 pairs per call. tests/test_gpu_sgbm.py computes each edge and the first value past it.
 * Device scratch: a call works through its pairs in chunks, every stage (median and speckle filter included) chunk by chunk, so
 * that the scratch of one chunk stays within 2 GiB (one pair at a time when a single pair is larger): per pair, C and S at 4 B
 * per cell (width1 * height * numDisparities), the map before the median at 2 B per pixel, and with speckleWindowSize > 0 the
 * speckle filter's scratch, 16 * (W + 288) / W + ~2 B per pixel. Every pixel of a host-memory call adds 4 B of staging.
 * Readings nobody could pin (bits of SBM_CV_READING above the block matcher's, which ignores them): 32 = no medianBlur stage,
 * 64 = the bottom rows (y + blockSize/2 >= height, y > 0) sum a clamped window instead of keeping what OpenCV's incremental
 * box sum leaves there (the P2 bias alone in MODE_HH, the previous row's C in MODE_SGBM). */
#define SBM_SGBM_MODE_SGBM 0
#define SBM_SGBM_MODE_HH 1
#define SBM_SGBM_MODE_SGBM_3WAY 2
#define SBM_SGBM_MODE_HH4 3

typedef struct sbm_sgbm_params {  /* one field per cv::StereoSGBM::create argument, in its order */
  int32_t min_disparity;           /* default 0                                                   */
  int32_t num_disparities;         /* default 16; > 0 and divisible by 16                         */
  int32_t block_size;              /* default 3; <= 0 -> 5                                        */
  int32_t p1;                      /* default 0 -> 2                                              */
  int32_t p2;                      /* default 0 -> max(5, P1 + 1)                                 */
  int32_t disp12_max_diff;         /* default 0; <= 0 -> 1 (the LR check is always on)            */
  int32_t prefilter_cap;           /* default 0; ftzero = max(cap, 15) | 1                        */
  int32_t uniqueness_ratio;        /* default 0; < 0 -> 10                                        */
  int32_t speckle_window_size;     /* default 0 (off)                                             */
  int32_t speckle_range;           /* default 0; the filter gets 16 * speckleRange                */
  int32_t mode;                    /* default SBM_SGBM_MODE_SGBM                                  */
} sbm_sgbm_params;

/* Fill *p with cv::StereoSGBM::create(minDisparity, numDisparities, blockSize) and the defaults of the other arguments. */
void sbm_sgbm_params_default(sbm_sgbm_params* p, int min_disparity, int num_disparities, int block_size);
/* SBM_ERR_SIZE (width/height <= 0), SBM_ERR_NUM_DISPARITIES (<= 0 or not divisible by 16), SBM_ERR_UNSUPPORTED (MODE_HH4,
 * MODE_SGBM_3WAY, an unknown mode, outside the exactness envelope or the limits above), else SBM_OK. */
int sbm_sgbm_params_validate(const sbm_sgbm_params* p, int width, int height);
/* One pair in HOST memory (the main.cpp:233 shape): strided 8-bit inputs, strided int16 output, strides in bytes. Synchronous. */
int sbm_sgbm_compute(sbm_handle* h, const sbm_sgbm_params* p, const uint8_t* left, size_t left_stride, const uint8_t* right,
                     size_t right_stride, int width, int height, int16_t* disp, size_t disp_stride);
/* n dense pairs resident in DEVICE memory; disp = n*height*width int16. Asynchronous on the handle's stream unless sync != 0,
 * with the ordering rules of sbm_compute_device. */
int sbm_sgbm_compute_device(sbm_handle* h, const sbm_sgbm_params* p, int n, const void* d_left, const void* d_right, int width,
                            int height, void* d_disp, int sync);
/* sbm_debug_fetch `which` values for the LAST sbm_sgbm_compute_device call: 4 = C, 5 = S (int16, n * height * width1 *
 * numDisparities, [pair][y][x - minX1][d - minDisparity]; SBM_ERR_UNSUPPORTED when width1 < 1), 6 = the map before the median
 * (int16, n*height*width); all three only when the call's pairs fitted one chunk, else SBM_ERR_UNSUPPORTED.
 * sbm_get_profile: while profiling is enabled (any mode) SGBM calls synchronise after each chunk and record "sgbm_cost",
 * "sgbm_aggregate", "sgbm_select", "sgbm_median", "sgbm_speckle", "sgbm_total" (ms of the last call, summed over its chunks). */

/* ---- pyramidal LK stereo: computeCorrespondences (src/slam/src/core/Stereo.cpp:9-51; DEPTH_METHOD_CV_LK) --------------------
 * The reference's sparse depth provider: generateKeypoints3D (Stereo.cpp:119-155) calls computeCorrespondences, which tracks
 * every left keypoint into the right image with calcOpticalFlowPyrLKStereo (src/slam/src/opencv/CvLKStereo.cpp: OpenCV's
 * pyramidal LK with the y update forced to 0) -- window 15 x 3, 5 pyramid levels, 30 iterations, eps 0.01,
 * OPTFLOW_LK_GET_MIN_EIGENVALS, threshold 1e-4 -- and gates the result on 0.5 < d <= 128; generateKeypoints3DStereo then takes
 * disparity = left.x - right.x under the status mask (Stereo.cpp:85-87). Each step below is marked REF (pinned by the reference's
 * own source) or RECALLED (OpenCV, not part of the reference tree, pinned by nothing here). The engine, oracle/lk_stereo_ref
 * (sequential C, and a numpy transcription of the RECALLED half) and tests/golden/pin_kit_lk.npz implement exactly this text.
 * All arithmetic is IEEE binary32 / binary64 WITHOUT contraction: an aarch64 build of the reference may fuse some of the
 * multiply-adds below (A11 * A22 - A12 * A12, the radicand, A12 * b2 - A22 * b1); the uncontracted reading is the contract, and
 * no SBM_CV_READING bit is spent on the other.
 *  Pyramid (RECALLED: cv::buildOpticalFlowPyramid(img, pyr, winSize, maxLevel, withDerivatives)):
 *   level 0   the frame. Level k = pyrDown of level k - 1: size ((w + 1) / 2, (h + 1) / 2); out(x, y) = (s + 128) >> 8 with s the
 *             separable [1 4 6 4 1] x [1 4 6 4 1] integer sum around (2x, 2y), BORDER_REFLECT_101.
 *   count     after level k is built the next size is computed; building stops, and k is the last level, when that size has
 *             width <= win_width or height <= win_height, or when k = max_level. The left pyramid is built first and the right
 *             one with the left's count (equal sizes: the same count).
 *   padding   every level is padded by the window size with BORDER_REFLECT_101 (p[-1] = p[1], p[n] = p[n - 2], repeated when
 *             the level is narrower than the padding); the derivative plane is padded with zeros (BORDER_CONSTANT).
 *   deriv     left only, Scharr on the UNPADDED level, reflect-101 at both borders, int16 (dx, dy) interleaved:
 *             dx = 3 (p[y-1][x+1] - p[y-1][x-1]) + 10 (p[y][x+1] - p[y][x-1]) + 3 (p[y+1][x+1] - p[y+1][x-1]), dy transposed.
 *   The engine stores no padding: it applies the two border rules when it reads.
 *  Tracker (REF: CvLKStereo.cpp:147-361), per point, levels from the last down to 0, nothing shared between points:
 *   point     prev = pt * (float)(1. / (1 << level)); next = prev at the last level, else next = (previous level's next) * 2.f;
 *             the output is set to next before anything can skip the level.
 *   window    halfWin = ((w - 1) * 0.5f, (h - 1) * 0.5f); prev -= halfWin; iprev = cvFloor(prev); the level is skipped when
 *             iprev.x is outside [-w, cols) or iprev.y outside [-h, rows) (at level 0: status 0, err 0).
 *   weights   a = prev.x - iprev.x, b = prev.y - iprev.y; iw00 = cvRound((1.f - a) * (1.f - b) * 16384) (float products left to
 *             right, cvRound = round half to even), iw01 from a * (1.f - b), iw10 from (1.f - a) * b, iw11 = 16384 - the others.
 *   patch     over the window in raster order: I = (bilinear sum of the 4 pixels + 256) >> 9; Ix, Iy = (bilinear sum of the 4
 *             derivatives + 8192) >> 14 (arithmetic shift); iA11 += (float)(Ix * Ix), iA12 += (float)(Ix * Iy), iA22 +=
 *             (float)(Iy * Iy): float accumulators, int products, every addition rounded. That order is the contract.
 *   matrix    A = iA * 2^-20; D = A11 * A22 - A12 * A12; minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 *
 *             A12)) / (2 * w * h), all float, square root and division correctly rounded. err = minEig. The level is skipped
 *             (at level 0: status 0) when (double)minEig < min_eig_threshold or D < FLT_EPSILON. D = 1.f / D.
 *   iterate   next -= halfWin; at most max_count times (clamped to 0..100): inext = cvFloor(next); out of the same range ->
 *             stop (at level 0: status 0). Weights as above from next; over the window in raster order diff = ((bilinear sum
 *             of the right image + 256) >> 9) - I; ib1 += (float)(diff * Ix), ib2 += (float)(diff * Iy) (the products pass
 *             2^24: conversion and sums both round); b = ib * 2^-20; delta = ((A12 * b2 - A22 * b1) * D, 0) -- the reference's
 *             one change to OpenCV; next += delta; output = next + halfWin; stop when (double)dx * dx + (double)dy * dy <=
 *             eps^2 (epsilon clamped to 0..10 and squared in double); stop with output -= delta * 0.5f when this is not the
 *             first iteration and |delta.x + previous delta.x| < 0.01 (and the same for y).
 *   status    1 unless cleared at level 0; err = level 0's minEig, or 0 where the point is outside at level 0.
 *  Gate (REF: Stereo.cpp:41-48): where status is set, d = left.x - right.x; status = 0 when d <= min_disparity or d >
 *   max_disparity. A NEGATIVE max_disparity switches the gate off: the outputs are calcOpticalFlowPyrLKStereo's own.
 *  Out of scope (SBM_ERR_UNSUPPORTED): OPTFLOW_USE_INITIAL_FLOW, flags without OPTFLOW_LK_GET_MIN_EIGENVALS (the L1 patch
 *   error), any other flag bit, any window other than 15 x 3; not expressible: caller-supplied pyramids, colour input.
 *  Limits: width and height 2..2048 (SBM_ERR_SIZE below 2 and for the reference's assertions win > 2, max_level >= 0;
 *   SBM_ERR_UNSUPPORTED above 2048), at most 65 535 pairs per call, cap >= 1; pointers to floats and counts 4-byte aligned.
 *   Coordinates must be finite and within +-2^30 at every level (cvFloor of anything else is undefined in the reference too).
 *  Kernels: per level one pyrDown launch over both images of every pair of a chunk and one Scharr launch
 *   over its left images, then ONE tracker launch, one wavefront per keypoint, that walks the levels. Device scratch, held by the
 *   handle: per pair of a chunk the levels above 0 of both images (1 B per pixel each) and the derivatives of every left level
 *   (4 B per pixel), ~6.7 B per frame pixel; a call works through its pairs in chunks of at most 256 MiB of it, and of at most
 *   32 767 pairs where a level above 0 exists (one pyrDown launch holds both images of every pair of a chunk).
 *  sbm_get_profile: while profiling is enabled (any mode) sbm_lk_stereo_device synchronises and records "lk_pyramid", "lk_track"
 *   and "lk_total" (ms of the last call, summed over its chunks). */
#define SBM_LK_USE_INITIAL_FLOW 4    /* cv::OPTFLOW_USE_INITIAL_FLOW: unsupported                     */
#define SBM_LK_GET_MIN_EIGENVALS 8   /* cv::OPTFLOW_LK_GET_MIN_EIGENVALS: required                    */

typedef struct sbm_lk_params {  /* computeCorrespondences' constants (Stereo.cpp:16-37) */
  int32_t win_width;         /* winSize.width, 15 (nothing else is supported)                         */
  int32_t win_height;        /* winSize.height, 3 (nothing else is supported)                         */
  int32_t max_level;         /* maxLevel, 5                                                           */
  int32_t max_count;         /* TermCriteria maxCount, 30; clamped to 0..100                          */
  float epsilon;             /* TermCriteria epsilon, 0.01f; clamped to 0..10                         */
  int32_t flags;             /* SBM_LK_GET_MIN_EIGENVALS                                              */
  double min_eig_threshold;  /* minEigThreshold, 1e-4                                                 */
  float min_disparity;       /* 0.5f                                                                  */
  float max_disparity;       /* 128.f; negative: no gate                                              */
} sbm_lk_params;

/* Fill *p with the reference's constants: 15, 3, 5, 30, 0.01f, GET_MIN_EIGENVALS, 1e-4, 0.5f, 128.f. */
void sbm_lk_params_default(sbm_lk_params* p);
/* SBM_ERR_NULL, SBM_ERR_SIZE, SBM_ERR_UNSUPPORTED as listed above, else SBM_OK. */
int sbm_lk_params_validate(const sbm_lk_params* p, int width, int height);
/* The pyramid alone, of n dense u8 frames in DEVICE memory, so that each level can be checked and used on its own. Layout, level
 * major: level l (size w_l x h_l, w_0 = width, w_l = (w_{l-1} + 1) / 2) starts n * (sum of w_k * h_k over k < l) bytes into
 * d_levels and holds the n frames' planes back to back; d_deriv (required when with_deriv != 0) has the same layout counted in
 * (dx, dy) int16 pairs. Both must hold every level the count rule above keeps (at most n * 4 / 3 * width * height + n elements).
 * *levels_out (host memory, may be NULL) receives the index of the last level. Synchronous. */
int sbm_lk_pyramid_device(sbm_handle* h, int n, const void* d_img, int width, int height, int with_deriv, const sbm_lk_params* p,
                          void* d_levels, void* d_deriv, int* levels_out);
/* computeCorrespondences on n dense pairs in DEVICE memory. d_kpts / d_count exactly as sbm_gftt_cv_detect_device and
 * sbm_gftt_select_device write them: n * cap float pairs, n int32 read on the device (a count above cap reads as cap). Outputs:
 * d_right_pts n * cap float pairs, d_status n * cap bytes, d_err n * cap floats (NULL: not wanted); entries past a frame's count
 * are left as they were. Asynchronous on the handle's stream unless sync != 0, with the ordering rules of sbm_compute_device. */
int sbm_lk_stereo_device(sbm_handle* h, int n, const void* d_left, const void* d_right, int width, int height, const void* d_kpts,
                         const void* d_count, int cap, const sbm_lk_params* p, void* d_right_pts, void* d_status, void* d_err,
                         int sync);
/* Host form for ONE pair, shaped like computeCorrespondences(left, right, leftCorners, status): strided 8-bit images (strides in
 * bytes), npts (x, y) pairs; right_pts npts pairs, status npts bytes, err npts floats or NULL. npts == 0 returns SBM_OK and
 * touches nothing. Synchronous. */
int sbm_lk_stereo(sbm_handle* h, const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride, int width,
                  int height, const float* pts, int npts, const sbm_lk_params* p, float* right_pts, uint8_t* status, float* err);
/* The sparse branch of generateKeypoints3DStereo (Stereo.cpp:53-117) on what sbm_lk_stereo_device wrote: per slot below the
 * frame's count a NaN triple where the status is 0, else projectDisparityTo3D(left, left.x - right.x, model), the depth range
 * check and localTransform -- the same device function as sbm_keypoints3d_device, so the two agree bit for bit on equal
 * disparities. d_xyz: n * cap * 3 floats; entries past a frame's count are left as they were. */
int sbm_keypoints3d_lk_device(sbm_handle* h, int n, const void* d_kpts, const void* d_right_pts, const void* d_status,
                              const void* d_count, int cap, const sbm_stereo_model* model, float min_depth, float max_depth,
                              void* d_xyz, int sync);

/* ---- occupancy map: buildOccupancyGridMap (src/slam/src/core/main.cpp:495-561) ----------------------------------------------
 * The reference's last dense consumer of the disparity maps: for every key frame it reprojects every pixel of the decimated map,
 * moves the point through the camera's local transform and the optimised pose, gates it on range, turns it into an octomap key
 * (coordToKeyChecked) and calls tree.updateNode(key, true) -- one octree descent per point -- and at the end writes the tree with
 * writeBinary("slam.bt"). Every update is a hit, so after writeBinary's toMaxLikelihood() + prune() the file depends only on the
 * SET of distinct voxel keys. Here the per-pixel work and a concurrent set insert run on the device, only the distinct voxels
 * cross PCIe, and the host writes the .bt stream from them. oracle/occupancy_ref (sequential C) implements exactly this text, and
 * tests/golden/occupancy_octomap.npz holds what the reference's own octomap (vendored under src/slam/src/octomap) answered for
 * the norm, the key and the stream on a few thousand points.
 *  Per plane p (with its pose, 12 floats r11 r12 r13 o14 / r21 .. / r31 .., the layout of sbm_stereo_model.local) and pixel
 *  (row, col) of the (possibly decimated) int16 map, IEEE binary32 / binary64 without contraction:
 *   disparity  d = (float)(disp / 16.0f) (main.cpp:529); the pixel is skipped unless d > 0.
 *   reproject  pt = projectDisparityTo3D((col * scale, row * scale), d, model), exactly as sbm_reproject_device; skipped unless
 *              all three coordinates are finite (main.cpp:533-536).
 *   transform  pt = transformPoint(pt, model.local) when model.has_local, then pt = transformPoint(pt, pose): per row
 *              r1 * x + r2 * y + r3 * z + o in float, left to right (Stereo.cpp:189-198; main.cpp:538-539).
 *   gate       v = pt - origin in float, origin = (o14, o24, o34) of the pose; norm = sqrt((double)(v.x * v.x + v.y * v.y +
 *              v.z * v.z)) with the sum in FLOAT (octomap's Vector3::norm); kept iff norm <= (double)(range_max * range_max),
 *              the product in float. QUIRK, restated on purpose: the reference compares the norm, not its square, with the
 *              SQUARED range (main.cpp:501, 544), so its 5 m gate keeps everything within 25 m.
 *   key        per axis s = (int)floor(resolution_factor * (double)coord) + 32768, resolution_factor = 1. / resolution in double
 *              (OcTreeBaseImpl.hxx:158, 310-321); kept iff 0 <= s < 65536 on all three axes. A coordinate that is not finite or
 *              whose floor fits no int rejects the point (what x86 gives for the reference's cast). The reference does not look
 *              at coordToKeyChecked's verdict and would update the tree with a half-written key; a rejected point is dropped here.
 *   packed     k0 << 32 | k1 << 16 | k2 in a uint64_t (axis 0 = x); the all-ones word is the empty slot.
 *  The reference takes the pose by ORDINAL, optimized_poses[i] with i counting from 1, not by node id; the engine uses the pose
 *  the caller passes.
 *  Map. sbm_occ_map is created from a handle with a capacity in voxels and uses that handle's stream, scratch and stage clock; it
 *  must be destroyed before the handle, and like the handle it serves one thread at a time. Device state: an open-addressing
 *  table of 64-bit keys, linear probing, with the smallest power of two of slots >= 2 * capacity (load factor <= 1/2 up to the
 *  capacity); a uint32 hit count per slot (wraps at 2^32); a 64-bit overflow counter. 12 B per slot.
 *  Insert, ONE launch from pixel to table (no n * h * w intermediate): a wavefront reduces its 64 keys to distinct leaders with
 *  lane counts, and only the leaders do a 64-bit compare-and-swap on the key slot and an atomic add of the lane count. A key
 *  that finds no free slot within min(slots, 1024) probes adds its lane count to the overflow counter and the entry point returns
 *  SBM_ERR_OCC_FULL (with sync == 0 nothing is known yet: SBM_OK, and the next synchronous insert, sbm_occ_overflow or a fetch
 *  reports it). Nothing is dropped silently: stored hits + overflow = accepted points. Key set and hit counts do not depend on
 *  insertion order or on how planes are split across calls (as long as nothing overflowed). Up to the capacity no probe chain
 *  comes near the bound; a map filled past it keeps storing, with longer chains, while a free slot lies within the probe bound
 *  of the key's hash -- in a table of more than 1024 slots a key can overflow while slots further on are still free. A stored
 *  key carries all its hits: its chain is full behind it, so a later point of that voxel finds it or nothing.
 *  Fetch compacts the occupied slots and sorts them ascending by packed key, counts as payload, with an LSD radix sort over the
 *  48 key bits (6 passes of 8 bits), all on the device.
 *  sbm_get_profile: while profiling is enabled (any mode) inserts and fetches synchronise and record "occ_insert" / "occ_fetch"
 *  (ms of the last call). */
typedef struct sbm_occ_params {
  double resolution;   /* octomap::OcTree(0.1): edge of a voxel, finite and > 0                  */
  float range_max;     /* rangeMax_ 5.0f; squared in float and compared with the NORM (see gate) */
  int32_t tree_depth;  /* 16 (octomap's fixed depth; nothing else is supported)                  */
} sbm_occ_params;
typedef struct sbm_occ_map sbm_occ_map; /* opaque */

/* Fill *p with the reference's constants: 0.1, 5.0f, 16. */
void sbm_occ_params_default(sbm_occ_params* p);
/* SBM_ERR_NULL; SBM_ERR_SIZE for a resolution that is not finite and > 0 or a range_max that is NaN or negative;
 * SBM_ERR_UNSUPPORTED for tree_depth != 16; else SBM_OK. */
int sbm_occ_params_validate(const sbm_occ_params* p);
/* A map for up to `capacity` voxels (1 .. 2^30) on the handle's device, empty. The codes of sbm_occ_params_validate;
 * SBM_ERR_SIZE for capacity 0, SBM_ERR_UNSUPPORTED above 2^30, both before anything is allocated; *out is NULL on failure. */
int sbm_occ_create(sbm_handle* h, const sbm_occ_params* p, size_t capacity, sbm_occ_map** out);
void sbm_occ_destroy(sbm_occ_map* map);
/* Empties the table and the overflow counter without reallocating. Asynchronous on the handle's stream. */
int sbm_occ_reset(sbm_occ_map* map);
/* n planes of width x height int16 in DEVICE memory, densely packed; poses in HOST memory, n * 12 floats, read before the call
 * returns. Asynchronous on the handle's stream unless sync != 0, with the ordering rules of sbm_compute_device.
 * Checked in this order, before anything is read or launched: SBM_ERR_NULL; SBM_ERR_BATCH for n <= 0; SBM_ERR_SIZE for a
 * width, height or scale <= 0; SBM_ERR_UNSUPPORTED for a plane of more than 2^30 pixels, for width * scale or height * scale
 * above 2^24, and for a d_disp that is not 2-byte aligned. The map is left as it was. */
int sbm_occ_insert_device(sbm_occ_map* map, int n, const void* d_disp, int width, int height, int scale,
                          const sbm_stereo_model* model, const float* poses, int sync);
/* The same from planes in HOST memory (n * height * width int16, dense). Synchronous. */
int sbm_occ_insert(sbm_occ_map* map, int n, const int16_t* disp, int width, int height, int scale, const sbm_stereo_model* model,
                   const float* poses);
/* Distinct voxels stored / points that found the table full, so far. Both synchronise the handle's stream. */
int sbm_occ_size(sbm_occ_map* map, size_t* size);
int sbm_occ_overflow(sbm_occ_map* map, uint64_t* overflow);
/* The stored voxels ascending by packed key into DEVICE memory: d_keys cap uint64 (8-byte aligned), d_hits cap uint32 (may be
 * NULL); *count = sbm_occ_size. SBM_ERR_SIZE, with *count set and nothing written, when cap < count; SBM_ERR_OCC_FULL, with the
 * outputs complete, when points overflowed. SBM_ERR_NULL for cap > 0 without d_keys, then SBM_ERR_UNSUPPORTED for a d_keys
 * that is not 8-byte or a d_hits that is not 4-byte aligned, both before anything is launched. Without d_hits the counts are
 * sorted along in scratch and dropped. Synchronous; the map is left as it was. */
int sbm_occ_fetch_device(sbm_occ_map* map, void* d_keys, void* d_hits, size_t cap, size_t* count);
/* The same into HOST memory. */
int sbm_occ_fetch(sbm_occ_map* map, uint64_t* keys, uint32_t* hits, size_t cap, size_t* count);
/* Plain host code, no GPU: writes to `path` the octomap binary stream (.bt) that OcTree::writeBinary produces for a tree of
 * depth 16 holding exactly these n packed keys (any order, duplicates allowed) as occupied leaves: the header lines ("size" =
 * node count after prune()), then depth first per inner node 2 bits per child (01 occupied leaf, 11 inner, 00 none; children
 * 0-3 in the first byte, 4-7 in the second; child index = bit of x + 2 * bit of y + 4 * bit of z as computeChildIdx), eight
 * sibling leaves collapsed into their parent as prune() does, built by one pass over the keys in Morton order.
 * SBM_ERR_NULL, SBM_ERR_SIZE (resolution, or a key above 48 bits), SBM_ERR_NOMEM, SBM_ERR_UNSUPPORTED (the file cannot be
 * written). */
int sbm_occ_write_binary(const uint64_t* keys, size_t n, double resolution, const char* path);

/* ---- occupancy map: ray-cast free space, insertPointCloud (OccupancyOcTreeBase.hxx:86-102, computeUpdate :169-270) -----------
 * buildOccupancyGridMap computes a sensorOrigin per key frame (main.cpp:520) and never uses it: its map has occupied voxels and
 * nothing else, so unknown and free space cannot be told apart. The second mode of sbm_occ_map is what octomap offers for that:
 * the voxel state is a float log-odds, updated scan by scan exactly as insertPointCloud(scan, origin, maxrange, lazy_eval =
 * false, discretize = false) without a bounding box updates the depth-16 leaves of an octomap::OcTree (pruning and expansion
 * inside the tree never change a leaf's value, so the contract is per voxel). tests/occupancy_ray_cases.py is a literal
 * transcription of this text, and tests/golden/occupancy_rays.npz holds what the reference's own octomap answered, bit for bit.
 * IEEE binary32 / binary64 as written, no contraction, correctly rounded sqrt and division:
 *  constants  logodds(p) = (float)log(p / (1 - p)), formed on the host at call time, for the five probabilities of
 *             sbm_occ_ray_params (octomap's defaults, AbstractOccupancyOcTree.cpp:42-47).
 *  scan       an origin and a list of points. A point that is not finite contributes nothing.
 *  gate       v = p - origin in float; norm = sqrt((double)(v.x * v.x + v.y * v.y + v.z * v.z)), the sum in float; the point is
 *             within range iff max_range < 0 or norm <= max_range (doubles). THIS gate is octomap's: the hit mode's
 *             norm-against-squared-range quirk is not applied here.
 *  within     ray cells: computeRayKeys(origin, p); p's voxel is occupied if coordToKeyChecked(p) passes (the key of the hit mode).
 *  beyond     ray cells: computeRayKeys(origin, origin + dir * (float)max_range), dir = v / (float)norm per component when
 *             norm > 0, all in float; no end point.
 *  ray        computeRayKeys (OcTreeBaseImpl.hxx:542-648): nothing when either end has no key; nothing when both keys are equal;
 *             else the origin's cell, then the 3-D DDA: d = end - origin in float, length = (float)norm(d), d /= length; per
 *             axis step = sign(d) and, where step != 0, tMax = (keyToCoord(key) + (float)(step * resolution * 0.5) - origin) /
 *             d and tDelta = resolution / |d| in double, else both the largest double. Each step advances the axis with the
 *             smallest tMax (strict <: x only if below y and z, else y only if below z, else z), then stops if the key equals
 *             the end's key, then stops if min(tMax) > length, else adds the cell. The end's cell is not part of the ray.
 *             On the device the loop is also bounded by 3 * 65536 steps, which no ray between two keys reaches.
 *  sets       free = union of the rays, occupied = union of the end points, free -= occupied.
 *  update     every voxel of either set gets exactly ONE update per scan, u = miss or u = hit: an absent voxel starts at 0;
 *             v += u in float; v = cmin if v < cmin, else cmax if v > cmax (updateNodeLogOdds; updateNode's early return for a
 *             leaf at its clamp gives the same value).
 *  order      scans are applied in call order and plane order; through the clamps the result depends on it.
 *  Not provided: insertPointCloudRays (per-ray updates whose result depends on thread order); the other switches are below, under "insert options".
 *  Mode. A map's mode is fixed by its first accepted insert after create or reset: hits (sbm_occ_insert*) or log-odds
 *  (sbm_occ_insert_cloud*, sbm_occ_insert_rays*). An insert or a fetch of the other kind returns SBM_ERR_UNSUPPORTED and changes
 *  nothing; a fetch of either kind serves an empty map. sbm_occ_size, sbm_occ_overflow and sbm_occ_reset serve both.
 *  State. The log-odds of a slot lives in the slot's 32-bit count word; the first log-odds insert allocates 8 B per slot more (a
 *  flag word and an entry of the scan's touched list), which reset keeps. The hit mode's 12 B per slot are unchanged.
 *  Per scan two launches in stream order, no n * h * w intermediate: MARK, one lane per ray, walks the DDA in registers and for
 *  every cell finds or claims the slot (the hit mode's compare-and-swap) and ORs "free" or "occupied this scan" into its flag
 *  word, reading the word first so that the thousands of rays that share their first cells issue no atomic for a bit already
 *  set; the lane whose OR found the word clear appends the slot to the touched list (one atomic per wavefront). APPLY runs over
 *  the touched list: occupied wins, the update above, the flags are cleared. No float atomics, no spin waits, no grid barriers;
 *  nothing depends on scheduling.
 *  Overflow. A cell that finds no slot within the probe bound raises the overflow counter (once per ray that reaches it), and
 *  the call, or with sync == 0 the next synchronous one, returns SBM_ERR_OCC_FULL. The table never frees a slot -- the one
 *  exception is a delete ("occupancy map: edit voxels by key"), which moves the map into a fresh table --, so a stored
 *  voxel has received every one of its updates and its value is exact; what is missing is whole voxels.
 *  sbm_get_profile: "occ_rays_mark" / "occ_rays_apply", ms of the last log-odds insert summed over its scans. */
typedef struct sbm_occ_ray_params {
  double prob_hit;         /* 0.7    */
  double prob_miss;        /* 0.4    */
  double clamp_min;        /* 0.1192 */
  double clamp_max;        /* 0.971  */
  double occupancy_thres;  /* 0.5: a leaf is occupied iff its log-odds >= logodds(occupancy_thres) (the writer)   */
  double max_range;        /* insertPointCloud's maxrange in metres; negative (the default, -1) means no limit    */
} sbm_occ_ray_params;

/* Fill *p with octomap's defaults. */
void sbm_occ_ray_params_default(sbm_occ_ray_params* p);
/* SBM_ERR_NULL; SBM_ERR_SIZE for a probability that is NaN or outside (0, 1), prob_hit < 0.5, prob_miss > 0.5, clamp_min >=
 * clamp_max, or a max_range that is NaN; else SBM_OK. */
int sbm_occ_ray_params_validate(const sbm_occ_ray_params* p);
/* The five log-odds the inserts and the writer use, in the struct's order: hit, miss, clamp min, clamp max, threshold. Host
 * code. The codes of sbm_occ_ray_params_validate, SBM_ERR_NULL without `logodds`. */
int sbm_occ_ray_logodds(const sbm_occ_ray_params* p, float logodds[5]);
/* One scan, octomap's own signature: n_points float triples in DEVICE memory (4-byte aligned), origin[3] and params in HOST
 * memory, read before the call returns. Asynchronous on the handle's stream unless sync != 0. Checked before anything is
 * launched: SBM_ERR_NULL (d_xyz may be NULL only for n_points == 0, an empty scan, which is accepted), the codes of
 * sbm_occ_ray_params_validate, SBM_ERR_UNSUPPORTED for more than 2^30 points, a misaligned d_xyz or a map in hit mode;
 * SBM_ERR_OCC_FULL as described above. */
int sbm_occ_insert_cloud_device(sbm_occ_map* map, size_t n_points, const void* d_xyz, const float* origin,
                                const sbm_occ_ray_params* params, int sync);
/* The same from points in HOST memory. Synchronous. */
int sbm_occ_insert_cloud(sbm_occ_map* map, size_t n_points, const float* xyz, const float* origin, const sbm_occ_ray_params* params);
/* n scans from n disparity planes: plane i's points are the pixels sbm_occ_insert_device reprojects and transforms (d > 0, a
 * finite reprojection, the local transform, then pose i; the same device function), its origin is (o14, o24, o34) of pose i
 * (main.cpp:520). Arguments and their checks as sbm_occ_insert_device, then those of params. */
int sbm_occ_insert_rays_device(sbm_occ_map* map, int n, const void* d_disp, int width, int height, int scale,
                               const sbm_stereo_model* model, const float* poses, const sbm_occ_ray_params* params, int sync);
/* The same from planes in HOST memory. Synchronous. */
int sbm_occ_insert_rays(sbm_occ_map* map, int n, const int16_t* disp, int width, int height, int scale, const sbm_stereo_model* model,
                        const float* poses, const sbm_occ_ray_params* params);
/* sbm_occ_fetch_device / sbm_occ_fetch for a log-odds map: the stored voxels ascending by packed key with their float log-odds
 * (the radix sort's 32-bit payload is the float's bits). Same arguments, checks and codes; SBM_ERR_UNSUPPORTED for a map in
 * hit mode. */
int sbm_occ_fetch_logodds_device(sbm_occ_map* map, void* d_keys, void* d_logodds, size_t cap, size_t* count);
int sbm_occ_fetch_logodds(sbm_occ_map* map, uint64_t* keys, float* logodds, size_t cap, size_t* count);
/* Plain host code, no GPU: what OcTree::writeBinary writes for a tree whose depth-16 leaves are exactly these n voxels (any
 * order, each key once). First toMaxLikelihood: a leaf is occupied iff logodds >= occupancy_thres_log (the fifth value of
 * sbm_occ_ray_logodds). Then prune(): eight sibling leaves of the same kind collapse, recursively. Then the stream of
 * writeBinaryNode (OccupancyOcTreeBase.hxx:1031-1090) under sbm_occ_write_binary's header: per inner node 2 bits per child,
 * 01 occupied leaf, 10 free leaf, 11 inner, 00 none; "size" is the node count after pruning. SBM_ERR_NULL, SBM_ERR_SIZE
 * (resolution, a key above 48 bits, a key given twice, a NaN), SBM_ERR_NOMEM, SBM_ERR_UNSUPPORTED (the file cannot be written). */
int sbm_occ_write_binary_logodds(const uint64_t* keys, const float* logodds, size_t n, double resolution, float occupancy_thres_log,
                                 const char* path);

/* ---- occupancy map: queries, search and castRay (OcTreeBaseImpl.hxx:408-470, OccupancyOcTreeBase.hxx:645-765) -----------------
 * The read side of sbm_occ_map: "what is at this point?" and "what does this ray hit?", answered on the device for batches of
 * points, rays, or the pixels of a virtual camera, from the table the inserts left in device memory. Both are stated per
 * depth-16 voxel, as the inserts are: pruning and expansion inside octomap never change a depth-16 value, so search(point) and
 * castRay on octomap's tree answer exactly this. tests/occupancy_query_cases.py is a literal transcription of this text, and
 * tests/golden/occupancy_query.npz holds what the reference's own octomap answered, bit for bit. The calls never change the map
 * and never return SBM_ERR_OCC_FULL. IEEE binary32 / binary64 as written, no contraction, correctly rounded sqrt and division:
 *  voxel      log-odds mode: a stored voxel is OCCUPIED iff logodds >= occupancy_thres_log (isNodeOccupied), else FREE; a key
 *             that is not stored is UNKNOWN. Hit mode: a stored voxel is OCCUPIED, the threshold is ignored; a key that is not
 *             stored is UNKNOWN. A map without a mode (empty since create or reset): every key is UNKNOWN. A voxel that
 *             overflowed out of the table (sbm_occ_overflow) is not stored and reads as UNKNOWN.
 *  key        coordToKeyChecked per axis as the inserts state it: (int)floor(factor * (double)coord) + 32768 with factor = 1. /
 *             resolution, kept iff 0 <= . < 65536; a coordinate that is not finite has no key.
 *  centre     keyToCoord(k) = (float)(((double)(k - 32768) + 0.5) * resolution) per axis.
 *  search     per point: SBM_OCC_CELL_OUT when the point has no key, else the voxel's state; with it a 4-byte value: in log-odds
 *             mode the float log-odds, NaN (0x7FC00000) where nothing is stored or the point has no key; in hit mode the uint32
 *             hit count, 0 there; without a mode 0.
 *  castRay(origin, directionP, end, ignore_unknown, max_range), in the order of the source:
 *   1 origin  key = coordToKeyChecked(origin); none: SBM_OCC_RAY_NONE.
 *   2 start   the origin's voxel, BEFORE the direction is looked at: OCCUPIED -> SBM_OCC_RAY_HIT, end = centre(key), even for a
 *             zero direction; UNKNOWN and ignore_unknown == 0 -> SBM_OCC_RAY_UNKNOWN, end = centre(key).
 *   3 normal  direction = directionP.normalized(): len = sqrt((double)(x * x + y * y + z * z)), the sum in FLOAT left to right;
 *             when len > 0 each component is divided by (float)len in float (Vector3.h:260-282).
 *   4 steps   per axis step = 1 if direction > 0, -1 if direction < 0, else 0 (zero and NaN give 0). Where step != 0:
 *             border = ((double)(key - 32768) + 0.5) * resolution, border += (double)step * resolution * 0.5 -- a DOUBLE
 *             increment, where computeRayKeys of the insert casts that term to float --, tMax = (border - (double)origin) /
 *             (double)direction, tDelta = resolution / |(double)direction|; else both the largest double. All three steps 0
 *             (a zero, NaN or infinite directionP: inf / inf is NaN, finite / inf is 0): SBM_OCC_RAY_NONE.
 *   5 loop    dim = the axis with the smallest tMax by the insert's strict < (x only if below y and z, else y only if below z,
 *             else z). If step[dim] < 0 and key[dim] == 0, or step[dim] > 0 and key[dim] == 65535: SBM_OCC_RAY_BOUNDS, end =
 *             centre(key), tested BEFORE the advance. Else key[dim] += step[dim], tMax[dim] += tDelta[dim], end = centre(key).
 *             Only when max_range > 0 (0 means no limit, like any negative value): dist = 0.0; dist += (double)((end.x -
 *             origin.x) * (end.x - origin.x)), then y, then z -- float differences, float products, a double sum (:741-749);
 *             dist > max_range * max_range (double): SBM_OCC_RAY_RANGE. Then the voxel of key: OCCUPIED -> SBM_OCC_RAY_HIT;
 *             UNKNOWN and ignore_unknown == 0 -> SBM_OCC_RAY_UNKNOWN; else the next step. On the device the loop is also
 *             bounded by 3 * 65536 steps, which no ray reaches: each step moves one key one cell towards its limit.
 *  One status per ray (int32) and one end (three floats):
 *   SBM_OCC_RAY_HIT      the only case where octomap returns true; end = centre of the occupied cell.
 *   SBM_OCC_RAY_RANGE    the ray left max_range; end = centre of the cell that left it.
 *   SBM_OCC_RAY_UNKNOWN  the ray met an unknown cell with ignore_unknown == 0; end = its centre (the origin's cell included).
 *   SBM_OCC_RAY_BOUNDS   the ray reached the edge of the key space; end = centre of the last cell inside it.
 *   SBM_OCC_RAY_NONE     no key for the origin, or no direction; end = three NaN (octomap leaves its `end` untouched there).
 *  view       sbm_occ_cast_view_device casts one ray per pixel (row, col) of a width x height virtual camera: q = ((float)
 *             (((double)(col * scale) - cx_l) / fx_l), (float)(((double)(row * scale) - cy_l) / fy_l), 1.0f); T(p) =
 *             transformPoint(transformPoint(p, model.local) when model.has_local, pose), the transform of the inserts; origin
 *             o = T((0, 0, 0)), direction T(q) - o per component in float; ray row * width + col. The call is EXACTLY
 *             sbm_occ_cast_rays on those rays and has no other contract.
 *  Device. One lane per point, ray or pixel; the DDA state (three keys, three steps, six doubles) stays in registers and a
 *  lane that has its answer leaves its loop. A lookup is a plain probe: the key's hash, then a linear walk to the key, an empty
 *  slot or min(slots, 1024) probes, with ordinary cached loads and no atomics -- queries are stream-ordered after the inserts
 *  and write nothing but their outputs. The view kernel maps each wavefront to an 8 x 8 pixel tile, so that its 64 rays stay in
 *  neighbouring voxels.
 *  sbm_get_profile: "occ_search" / "occ_cast", ms of the last search / cast call. */
enum { SBM_OCC_CELL_OUT = -1, SBM_OCC_CELL_UNKNOWN = 0, SBM_OCC_CELL_FREE = 1, SBM_OCC_CELL_OCCUPIED = 2 };
enum { SBM_OCC_RAY_NONE = 0, SBM_OCC_RAY_HIT = 1, SBM_OCC_RAY_RANGE = 2, SBM_OCC_RAY_UNKNOWN = 3, SBM_OCC_RAY_BOUNDS = 4 };
typedef struct sbm_occ_query_params {
  double max_range;           /* castRay's maxRange in metres; <= 0 (the default, -1) means no limit                     */
  float occupancy_thres_log;  /* 0.0f: the fifth value of sbm_occ_ray_logodds; a voxel is occupied iff logodds >= this  */
  int32_t ignore_unknown;     /* 0: an unknown cell ends the ray (castRay's ignoreUnknownCells = false)                  */
} sbm_occ_query_params;

/* Fill *p with castRay's defaults: -1, 0.0f, 0. */
void sbm_occ_query_params_default(sbm_occ_query_params* p);
/* SBM_ERR_NULL; SBM_ERR_SIZE for a max_range or a threshold that is NaN; else SBM_OK. */
int sbm_occ_query_params_validate(const sbm_occ_query_params* p);
/* search on n points: d_xyz n float triples, d_state n int32 (SBM_OCC_CELL_*), d_value n 4-byte values (may be NULL), all in
 * DEVICE memory, 4-byte aligned. Asynchronous on the handle's stream unless sync != 0. Checked in this order before anything is
 * launched: SBM_ERR_NULL (d_xyz and d_state may be NULL only for n == 0, which is accepted and launches nothing); SBM_ERR_SIZE
 * for a NaN threshold; SBM_ERR_UNSUPPORTED for more than 2^30 points or a misaligned pointer. */
int sbm_occ_search_device(sbm_occ_map* map, size_t n, const void* d_xyz, float occupancy_thres_log, void* d_state, void* d_value,
                          int sync);
/* The same on HOST memory. Synchronous. */
int sbm_occ_search(sbm_occ_map* map, size_t n, const float* xyz, float occupancy_thres_log, int32_t* state, void* value);
/* castRay on n rays: d_dirs n float triples, d_status n int32 (SBM_OCC_RAY_*), d_end n float triples (may be NULL), in DEVICE
 * memory, 4-byte aligned. With shared_origin == 0 `origins` is n float triples in DEVICE memory; with shared_origin != 0 it is
 * ONE origin, three floats in HOST memory, read before the call returns, that every ray starts from. params in HOST memory.
 * Asynchronous on the handle's stream unless sync != 0. Checked in this order before anything is launched: SBM_ERR_NULL
 * (origins, d_dirs and d_status may be NULL only for n == 0, which is accepted and launches nothing); the codes of
 * sbm_occ_query_params_validate; SBM_ERR_UNSUPPORTED for more than 2^30 rays or a misaligned device pointer. */
int sbm_occ_cast_rays_device(sbm_occ_map* map, size_t n, const void* origins, int shared_origin, const void* d_dirs,
                             const sbm_occ_query_params* params, void* d_status, void* d_end, int sync);
/* The same with every array in HOST memory (origins: n triples, or one with shared_origin != 0). Synchronous. */
int sbm_occ_cast_rays(sbm_occ_map* map, size_t n, const float* origins, int shared_origin, const float* dirs,
                      const sbm_occ_query_params* params, int32_t* status, float* end);
/* One ray per pixel of a virtual camera (see "view"): d_status width * height int32, d_end as many float triples (may be NULL),
 * DEVICE memory; model, pose (12 floats) and params in HOST memory, read before the call returns. Checked in this order:
 * SBM_ERR_NULL; SBM_ERR_SIZE for a width, height or scale <= 0; the codes of sbm_occ_query_params_validate;
 * SBM_ERR_UNSUPPORTED for more than 2^30 pixels, for width * scale or height * scale above 2^24, and for a misaligned pointer. */
int sbm_occ_cast_view_device(sbm_occ_map* map, int width, int height, int scale, const sbm_stereo_model* model, const float* pose,
                             const sbm_occ_query_params* params, void* d_status, void* d_end, int sync);

/* ---- occupancy map: the octree above the voxels (OcTreeBaseImpl.hxx, OccupancyOcTreeBase.hxx: updateInnerOccupancy, prune,
 * search(point, depth), begin_leafs(maxDepth), calcNumNodes, writeBinary) --------------------------------------------------------
 * sbm_occ_tree is a SNAPSHOT of an sbm_occ_map with the sixteen levels octomap keeps above the depth-16 voxels, built and queried
 * on the device. The map and every entry point above stay as they are: a build only reads the table. After non-lazy inserts an
 * inner node's value in octomap is the maximum of its children (updateOccupancyChildren) and prune() collapses eight equal
 * childless siblings; both are pure functions of the set of voxels and their values, so everything here is exact: integers,
 * orders, float bits and bytes. tests/occupancy_tree_cases.py is a literal transcription of this text, and
 * tests/golden/occupancy_tree.npz holds what the reference's own octomap answered.
 *  leaves     the stored voxels of the map at build time, under one of two readings of their value:
 *             SBM_OCC_TREE_LOGODDS (log-odds maps only; a hit-mode map: SBM_ERR_UNSUPPORTED): the stored float.
 *             SBM_OCC_TREE_MAXLIKELIHOOD (both modes), toMaxLikelihood() as writeBinary applies it, with the constants of
 *             sbm_occ_ray_logodds(params): a log-odds voxel with logodds >= threshold becomes the clamp-max log-odds, any other
 *             log-odds voxel the clamp-min log-odds; every stored voxel of a hit-mode map becomes clamp-max.
 *  nodes      for a depth d in 0..16 and a key prefix (key >> (16 - d) per axis) the node exists iff some stored voxel lies below
 *             it; its value is the float maximum over those voxels. An empty map has no nodes, not even a root.
 *  collapsed  a node at depth d < 16 is collapsed iff all 8^(16 - d) voxels below it are stored and their values compare equal
 *             with float == (isNodeCollapsible applied bottom-up).
 *  pruned     the pruned tree holds the nodes that have no collapsed proper ancestor. A leaf of it is a depth-16 node or a
 *             collapsed node. The tree's size is its number of nodes: calcNumNodes after prune(), the `size` line of a .bt.
 *  children   everywhere the child index is (x bit) | (y bit) << 1 | (z bit) << 2, from the top key bit down (computeChildIdx).
 *  node key   octomap's centre key, adjustKeyAtDepth: at depth 16 the key itself; above, per axis, ((k >> l) << l) | (1 << (l - 1))
 *             with l = 16 - d; packed as the map's 48-bit key.
 *  search(point, depth)   OcTreeBaseImpl.hxx:408-471. depth 0 means 16. SBM_OCC_CELL_OUT for a point without a key;
 *             SBM_OCC_CELL_UNKNOWN where no node of that depth covers the key; else occupied or free by value >=
 *             occupancy_thres_log. The value is the node's float, NaN (0x7FC00000) for out and unknown. The found depth is that
 *             of the node octomap returns: the shallowest collapsed node at or above the asked depth if there is one (it holds
 *             the same value), else the asked depth; -1 for out and unknown.
 *  leaves(max_depth)      begin_leafs(maxDepth). 0 means 16. Every leaf of the pruned tree at depth <= max_depth and every other
 *             node of it at exactly max_depth, in octomap's iteration order, which is Morton order of the covered cubes; per
 *             entry the centre key, the depth (int32) and the value.
 *  binary     the body of writeBinaryNode (OccupancyOcTreeBase.hxx:1031-1090) of a MAXLIKELIHOOD tree: every non-leaf node of the
 *             pruned tree contributes two bytes, in depth-first pre-order, per child two bits as sbm_occ_write_binary_logodds
 *             states them; a leaf is occupied iff it holds clamp max, which is its voxels' own >= threshold. With the header of
 *             sbm_occ_write_binary and `size` the node count the file equals, byte for byte, what sbm_occ_write_binary /
 *             sbm_occ_write_binary_logodds write for the fetched voxels.
 *  Elsewhere: getMetricMin / getMetricMax / volume, the bounding-box leaf iterator and getUnknownLeafCenters read a tree through the
 *  section "the read side for planners" below (octomap forms the metric bounds in double from the leaves' centre keys and depths,
 *  which the snapshot holds). Not here: incremental update (a rebuild is the update). The .ot format of a tree has a section of its
 *  own below ("the .ot format": sbm_occ_ot_body_device, sbm_occ_ot_write).
 *  Device. The compacted table is sorted by 48-bit Morton code with the map's radix sort; siblings are then
 *  neighbours, and sixteen bottom-up passes (heads per tile, a scan, one write per head) make each level from the one below;
 *  one top-down pass per depth marks what lies under a collapsed node and ranks the non-leaf nodes in pre-order, so that the .bt
 *  body is one store per node. No spin waits, no grid barriers, and no atomics other than integer counts. A tree holds 20 bytes per
 *  stored voxel and 32 per node above them.
 *  sbm_get_profile: "occ_tree_build" / "occ_tree_query", ms of the last build / of the last search, leaves or binary call. */
typedef struct sbm_occ_tree sbm_occ_tree;
enum { SBM_OCC_TREE_LOGODDS = 0, SBM_OCC_TREE_MAXLIKELIHOOD = 1 };
typedef struct sbm_occ_tree_counts {
  uint64_t voxels;          /* stored voxels at build time                                                  */
  uint64_t nodes, leaves;   /* of the pruned tree: calcNumNodes, getNumLeafNodes                            */
  uint64_t nodes_at[17];    /* nodes of the pruned tree per depth 0..16                                     */
  uint64_t leaves_at[17];   /* leaves of the pruned tree per depth                                          */
  uint16_t key_min[3];      /* per axis over the stored voxels; an empty tree reports 65535 ...             */
  uint16_t key_max[3];      /* ... and 0                                                                    */
  uint32_t pad;
} sbm_occ_tree_counts;

/* A tree over `map`, empty until built. It uses the map's handle, which must outlive it; the map itself is read by
 * sbm_occ_tree_build only and may be destroyed once no further build follows. SBM_ERR_NULL, SBM_ERR_NOMEM. */
int sbm_occ_tree_create(sbm_occ_map* map, sbm_occ_tree** tree);
void sbm_occ_tree_destroy(sbm_occ_tree* tree);
/* Take a new snapshot of the map under `reading`, reusing the tree's buffers; later inserts do not change a built tree. params
 * (host memory) gives the constants of SBM_OCC_TREE_MAXLIKELIHOOD and may be NULL only for SBM_OCC_TREE_LOGODDS. A map whose table
 * overflowed builds the tree of what is stored and returns SBM_OK (the inserts reported the overflow). The call waits for the
 * stream twice (the voxel count, the level sizes); what follows is asynchronous unless sync != 0. Checked in this order before
 * anything is launched: SBM_ERR_NULL; SBM_ERR_SIZE for a reading that is neither, then the codes of sbm_occ_ray_params_validate
 * where params is given; SBM_ERR_UNSUPPORTED for SBM_OCC_TREE_LOGODDS on a hit-mode map. After the voxel count is known:
 * SBM_ERR_UNSUPPORTED for a map with 2^31 or more nodes above its voxels. A build that fails leaves an empty tree. */
int sbm_occ_tree_build(sbm_occ_tree* tree, int reading, const sbm_occ_ray_params* params, int sync);
/* The counts of the last build. A tree that was never built answers as an empty one, here and below. Waits for the stream. */
int sbm_occ_tree_info(sbm_occ_tree* tree, sbm_occ_tree_counts* info);
/* search(point, depth) on n points: d_xyz n float triples, d_state n int32 (SBM_OCC_CELL_*), d_value n 4-byte values (may be
 * NULL), d_found_depth n int32 (may be NULL), DEVICE memory, 4-byte aligned. Asynchronous unless sync != 0. Checked in this order
 * before anything is launched: SBM_ERR_NULL (d_xyz and d_state may be NULL only for n == 0, which is accepted and launches
 * nothing); SBM_ERR_SIZE for a depth outside 0..16 or a NaN threshold; SBM_ERR_UNSUPPORTED for more than 2^30 points or a
 * misaligned pointer. */
int sbm_occ_tree_search_device(sbm_occ_tree* tree, size_t n, const void* d_xyz, int depth, float occupancy_thres_log, void* d_state,
                               void* d_value, void* d_found_depth, int sync);
/* The same on HOST memory. Synchronous. */
int sbm_occ_tree_search(sbm_occ_tree* tree, size_t n, const float* xyz, int depth, float occupancy_thres_log, int32_t* state,
                        void* value, int32_t* found_depth);
/* leaves(max_depth) into d_keys (uint64, 8-byte aligned), d_depth (int32) and d_value (float, may be NULL), cap entries each, DEVICE
 * memory. *count receives the number of entries; when it exceeds cap nothing is written and the call returns SBM_ERR_SIZE, as
 * sbm_occ_fetch_device does. Synchronous. SBM_ERR_NULL (d_keys and d_depth may be NULL only for cap == 0); SBM_ERR_SIZE for a
 * max_depth outside 0..16; SBM_ERR_UNSUPPORTED for a misaligned pointer. */
int sbm_occ_tree_leaves_device(sbm_occ_tree* tree, int max_depth, void* d_keys, void* d_depth, void* d_value, size_t cap, size_t* count);
/* The same into HOST memory. */
int sbm_occ_tree_leaves(sbm_occ_tree* tree, int max_depth, uint64_t* keys, int32_t* depth, float* value, size_t cap, size_t* count);
/* The .bt body into d_bytes (DEVICE memory, cap bytes); *nbytes receives its length, twice the number of non-leaf nodes; when it
 * exceeds cap nothing is written and the call returns SBM_ERR_SIZE. Synchronous. SBM_ERR_NULL; SBM_ERR_UNSUPPORTED for a tree
 * built with SBM_OCC_TREE_LOGODDS. */
int sbm_occ_tree_binary_device(sbm_occ_tree* tree, void* d_bytes, size_t cap, size_t* nbytes);
/* tree.writeBinary(path): the header with the tree's size and resolution, then that body. SBM_ERR_NULL; SBM_ERR_UNSUPPORTED for a
 * tree built with SBM_OCC_TREE_LOGODDS or a file that cannot be written; SBM_ERR_NOMEM. */
int sbm_occ_tree_write_binary(sbm_occ_tree* tree, const char* path);

/* ---- occupancy map: load a .bt stream, readBinary (AbstractOccupancyOcTree.cpp:126-178, readHeader, readBinaryData /
 * readBinaryNode at OccupancyOcTreeBase.hxx:937-1028) ---------------------------------------------------------------------------
 * The other half of the writers above: a .bt stream becomes the log-odds map it describes, so that search, castRay, the tree and
 * further insertPointCloud scans start from a saved map, as they do in octomap after readBinary. The pruned tree is parsed on the
 * host in one pass (two bytes per inner node); the expansion of its leaves to depth-16 voxels, the work that grows with the map,
 * runs on the device. tests/occupancy_load_cases.py is a literal transcription of this text, and tests/golden/occupancy_load.npz
 * holds what the reference's own octomap read from the same streams.
 *  header     the first line starts with "# Octomap OcTree binary file". Then whitespace-separated tokens up to the token `data`,
 *             whose line ends the header: a token that begins with # skips its line; `id`, `size` and `res` take the next token
 *             (size an unsigned decimal below 2^32, res as strtod reads it), in any order, the last one given counting; any
 *             other keyword skips its line. id must be OcTree (or the "1" octomap itself renames to it), res must be > 0.
 *  body       only when size > 0. One two-byte record per node that has children, the root's first: two bits per child, children
 *             0-3 in the first byte and 4-7 in the second, child c in bits (2c, 2c + 1) of the 16-bit little-endian word, the
 *             first of the pair lower: 01 an occupied leaf, 10 a free leaf, 11 a child whose own record follows, 00 no child.
 *             The records of the 11 children follow in child order, depth first. The child index is computeChildIdx's, so
 *             pre-order is Morton order of the cubes. An occupied leaf holds the clamp-max log-odds and a free leaf the
 *             clamp-min log-odds: the fourth and third floats of sbm_occ_ray_logodds for the caller's sbm_occ_ray_params. A
 *             record whose eight codes are all 00 leaves a childless node at clamp max, as readBinaryNode does: an occupied
 *             leaf of that depth. Bytes after the last record are ignored, as octomap ignores them.
 *  nodes      the root, plus one per child code other than 00. The stream is accepted iff this equals the header's size
 *             (calcNumNodes() against size, AbstractOccupancyOcTree.cpp:172).
 *  result     per depth-16 voxel below every leaf, that leaf's value -- the per-voxel reading of every section above: pruning
 *             and expansion never change a depth-16 value. A leaf of depth d with Morton prefix c covers the 8^(16-d) voxels
 *             whose codes are c << 3(16-d) | 0 .. 8^(16-d) - 1; its first key is the de-interleaved c << 3(16-d).
 *  status     SBM_ERR_UNSUPPORTED: the first line is something else (the legacy binary header, tree type 3, is not provided),
 *             another id or none, a file that cannot be opened or read. SBM_ERR_SIZE: the stream ends inside the header or
 *             inside the tree, a number that does not parse, res not greater than 0, a 11 child of a depth-15 record (depth
 *             17), size different from the nodes read. SBM_ERR_NOMEM. octomap itself does not look at the id of a stream it
 *             reads into an OcTree and does not bound the depth; those two verdicts are this library's.
 *  resolution the header carries `res` with 6 significant digits (%g). A load requires the file's res to EQUAL what this library's
 *             own writers print for the map's resolution, parsed back (SBM_ERR_SIZE otherwise). The key set of a loaded map is
 *             exact; its metric coordinates agree with the tree that was written to that precision, as octomap's do.
 *  load       sbm_occ_load_binary / sbm_occ_read_binary, in this order before anything is launched or changed -- on any error
 *             the map is exactly as it was: SBM_ERR_NULL; the codes of sbm_occ_ray_params_validate; the codes above; the
 *             resolution; SBM_ERR_OCC_FULL when the expanded voxel count exceeds the map's capacity. Then, as readBinary does
 *             clear() first, the map is reset whatever its mode was, put in log-odds mode with the flag words and the touched
 *             list the first log-odds insert allocates (later sbm_occ_insert_cloud* / sbm_occ_insert_rays* scans continue on
 *             the loaded map), the leaves are uploaded and expanded. size 0 leaves an empty map with no mode.
 *  Device. Per leaf the host uploads a word (first Morton code << 8 | depth << 1 | occupied) and the exclusive prefix of the leaf
 *  volumes (at most 2^30 voxels, 32 bits). One launch, one output voxel per lane: a binary search of the prefix array for the
 *  leaf that holds the lane's index, the code as the leaf's first code OR'd with the offset, the packed key by de-interleaving
 *  (the inverse of the tree build's five shift-and-mask steps), then the inserts' find-or-claim probe (the key's hash, a linear
 *  walk, min(slots, 1024) probes) and a plain store of the float: the voxels of one load are distinct, so a slot has one writer.
 *  The only atomics are the key's compare-and-swap and the size and overflow counters (one add per wavefront); no spin waits, no
 *  grid barriers. The call returns once the leaves are uploaded; the reset and the expansion are asynchronous on the handle's
 *  stream unless sync != 0 or profiling is on. A voxel that finds no slot within the probe bound counts as overflow and the call,
 *  or with sync == 0 the next synchronous one, returns SBM_ERR_OCC_FULL, as for the inserts.
 *  Not provided: the legacy header, a resolution other than the map's, trees of another depth than 16. An .ot stream is refused
 *  here and read by sbm_occ_ot_load / sbm_occ_ot_read ("the .ot format" below).
 *  sbm_get_profile: "occ_load", ms of the last load's reset and expansion on the device. */
typedef struct sbm_occ_binary_header {
  double resolution;        /* res as parsed                                                                    */
  uint64_t size;            /* the header's size                                                                */
  uint64_t nodes;           /* nodes read: calcNumNodes() of the tree octomap would hold                        */
  uint64_t leaves;          /* leaves of the pruned tree, childless nodes among them                            */
  uint64_t occupied;        /* leaves that hold clamp max                                                       */
  uint64_t voxels;          /* depth-16 voxels below the leaves: up to 2^48                                     */
  uint64_t leaves_at[17];   /* leaves per depth 0..16                                                           */
  uint16_t key_min[3];      /* per axis over those voxels; a stream without leaves reports 65535 ...            */
  uint16_t key_max[3];      /* ... and 0                                                                        */
  uint32_t pad;
} sbm_occ_binary_header;

/* Plain host code, no GPU: parse n bytes of a .bt stream and report its counts. On an error *out holds what was read up to it
 * (for a size mismatch everything). SBM_ERR_NULL (bytes may be NULL only for n == 0), then the codes under "status". */
int sbm_occ_binary_info(const void* bytes, size_t n, sbm_occ_binary_header* out);
/* Plain host code, no GPU: the leaves in stream order, which is Morton order -- the packed key of the cube's lowest voxel, the
 * depth, and 1 for occupied, 0 for free -- into arrays of cap entries. *count receives their number; when it exceeds cap nothing is
 * written and the call returns SBM_ERR_SIZE. SBM_ERR_NULL (the arrays may be NULL only for cap == 0), then the codes under
 * "status", which leave *count as it was. */
int sbm_occ_binary_leaves(const void* bytes, size_t n, uint64_t* first_key, int32_t* depth, uint8_t* occupied, size_t cap, size_t* count);
/* tree.readBinary(stream) from n bytes in HOST memory, read before the call returns; params (host) gives the two clamp log-odds.
 * See "load" for the checks and their order and "Device" for what is asynchronous. */
int sbm_occ_load_binary(sbm_occ_map* map, const void* bytes, size_t n, const sbm_occ_ray_params* params, int sync);
/* tree.readBinary(filename): the same from a file; SBM_ERR_UNSUPPORTED when it cannot be opened or read. */
int sbm_occ_read_binary(sbm_occ_map* map, const char* path, const sbm_occ_ray_params* params, int sync);

/* ---- occupancy map: the .ot format, AbstractOcTree::write / read (AbstractOcTree.cpp:45-182, writeNodesRecurs / readNodesRecurs
 * at OcTreeBaseImpl.hxx:763-844, OcTreeDataNode<float>::writeData / readData) -------------------------------------------------------
 * The format that keeps the probabilities: a .bt thresholds every voxel to one of the two clamp values, so a map that went through
 * a .bt continues from saturated values; an .ot holds every node's float. Scans, sbm_occ_ot_write, later sbm_occ_ot_read and
 * more scans give the keys and float bits of the uninterrupted run. tests/occupancy_ot_cases.py is a literal transcription of
 * this text, and tests/golden/occupancy_ot.npz holds what the reference's own octomap wrote and read.
 *  header     written: "# Octomap OcTree file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n
 *             id OcTree\nsize <nodes>\nres <resolution>\ndata\n", the resolution as the .bt writers print it (%g). Read: the first
 *             line starts with "# Octomap OcTree file"; then the tokens of readHeader exactly as the .bt load section above states
 *             them (comments, id / size / res in any order, unknown keywords skipped, the line of `data` ends the header). id must
 *             be OcTree (or "1"), res > 0, and for a load res must EQUAL what this library prints for the map's resolution, parsed
 *             back -- the .bt rule.
 *  body       written for a tree built with SBM_OCC_TREE_LOGODDS (a SBM_OCC_TREE_MAXLIKELIHOOD tree, and with it every tree of a
 *             hit-mode map: SBM_ERR_UNSUPPORTED -- the mirror image of `binary`, which refuses LOGODDS). Every node of the pruned
 *             tree, in depth-first pre-order, contributes 5 bytes: its value as little-endian binary32 (the float maximum the
 *             tree holds) and one byte whose bit c is set iff child c exists (computeChildIdx order). A leaf of the pruned tree
 *             writes mask 0. `size` is the node count; an empty tree writes `size 0` and no body.
 *             Read only when size > 0: `size` records of 5 bytes, the root's first; the children of a record follow in ascending
 *             child index, depth first; a record with mask 0 is a leaf of its depth. The value of a record with children is not
 *             kept: the map has no inner nodes, and a tree built afterwards recomputes them. Bytes after record `size` are ignored.
 *  result     per depth-16 voxel below every leaf, that leaf's float, bits unchanged. Nothing is clamped (a load takes no
 *             sbm_occ_ray_params): a leaf value outside the clamps of later scans is stored as it is. A scan after a load is exact
 *             against octomap only for values inside the clamp interval of that scan's parameters: beyond the clamps octomap's
 *             early return for a saturated node and the apply kernel's clamp(v + update) differ.
 *  status     SBM_ERR_UNSUPPORTED: another first line (the .bt header included; nothing sniffs the format, and the .bt entry
 *             points keep refusing an .ot header), another id or none, a leaf value that is not finite, a file that cannot be
 *             opened or read. SBM_ERR_SIZE: the stream ends in the header, a number does not parse, res <= 0 or not the map's,
 *             5 * size exceeds the body's bytes, the first `size` records are not exactly one complete tree (it completes
 *             earlier, or is still open after them), a record at depth 16 has a child bit. SBM_ERR_OCC_FULL: the expanded voxel
 *             count exceeds the map's capacity. SBM_ERR_NOMEM. In this order after SBM_ERR_NULL: first line, header tokens, id,
 *             res, the map's resolution, 5 * size, the shape of the tree, the leaf values, the capacity. octomap's read() never
 *             compares `size` with the nodes it read and reads past a short stream; those verdicts are this library's, and the
 *             fixture records octomap's beside them.
 *  load       everything is checked before the map is touched: a refused load leaves the map exactly as it was. A successful
 *             load resets the map whatever its mode was, puts it in log-odds mode with what the first log-odds insert allocates,
 *             and expands the leaves. size 0 leaves an empty map with no mode.
 *  Device. Write: the first .ot call after a build ranks every node of the pruned tree in pre-order (a
 *  bottom-up pass of subtree node counts, a top-down pass of ranks that also notes the node at every rank; 8 bytes per node above
 *  the voxels and 4 per node, kept until the next build; a build that is never written as .ot costs what it did). The body is
 *  mapped by rank, one node per lane; a workgroup's 1280 bytes are put together in LDS and stored as whole dwords, no atomics.
 *  Load: every record is 5 bytes at 5 i, so the host parses only the header and uploads the first `size` records raw. With
 *  c[i] = popcount(mask[i]): D[0] = 1, D[i + 1] = D[i] + c[i] - 1 is a device-wide scan (tiles of SBM_OCC_OT_SCAN_TILE records),
 *  and the stream is one complete tree iff D[i] >= 1 for i < size and D[size] = 0; parent(i) is the largest j < i with
 *  D[j] <= D[i], found through minima of D per SBM_OCC_OT_FAN records, minima of those per SBM_OCC_OT_FAN, and so on; i is child
 *  number D[p] + c[p] - 1 - D[i] of its parent p, which with mask[p] gives its child index; each leaf walks up at most 16 parents
 *  for its depth and Morton prefix (a 17th step: malformed); the leaves are compacted in record order, which is Morton order,
 *  and their volumes 8^(16 - d) are scanned (64 bits, saturating) into the prefix array of the expansion. One read-back (flags,
 *  leaf count, voxel total) is the load's only wait besides the upload. Every loop there has a bound that does not depend on the
 *  stream. The expansion is the .bt loader's with the leaf's float as the stored word. Streams of more than 2^28 records, and
 *  every stream with SBM_OCC_OT_HOST_PARSE=1, take the one-pass host parser of sbm_occ_ot_info instead: same maps, same codes.
 *  Not provided: OcTreeStamped streams, the legacy headers, an .ot of a MAXLIKELIHOOD tree. A ColorOcTree stream is refused by
 *  these calls and written and read by sbm_occ_color_ot_* ("colour per voxel" below).
 *  sbm_get_profile: "occ_tree_query", ms of the last body call (the ranking included when it ran); "occ_load", ms of the last
 *  load on the device: the parse (where it ran there, its upload included), the reset and the expansion; a refused load leaves
 *  the time of the last one. */
#define SBM_OCC_OT_FAN 16          /* entries per tile of the parent search's minima hierarchy     */
#define SBM_OCC_OT_SCAN_TILE 1024  /* records per workgroup of the device parse's scans            */
typedef struct sbm_occ_ot_header {
  double resolution;        /* res as parsed                                                                    */
  uint64_t size;            /* the header's size                                                                */
  uint64_t nodes;           /* records read                                                                     */
  uint64_t leaves;          /* records with mask 0                                                              */
  uint64_t voxels;          /* depth-16 voxels below the leaves: up to 2^48, counted and never expanded here    */
  uint64_t leaves_at[17];   /* leaves per depth 0..16                                                           */
  float value_min;          /* over the finite leaf values; a stream without one reports 0 ...                  */
  float value_max;          /* ... and 0                                                                        */
  uint16_t key_min[3];      /* per axis over those voxels; a stream without leaves reports 65535 ...            */
  uint16_t key_max[3];      /* ... and 0                                                                        */
  uint32_t pad;
} sbm_occ_ot_header;

/* The .ot body of a LOGODDS tree into d_bytes (DEVICE memory, 4-byte aligned, cap bytes); *nbytes receives its length, 5 * nodes;
 * when it exceeds cap nothing is written and the call returns SBM_ERR_SIZE. Synchronous. SBM_ERR_NULL; SBM_ERR_UNSUPPORTED for a
 * tree built with SBM_OCC_TREE_MAXLIKELIHOOD or a misaligned pointer. A tree that was never built answers as an empty one. */
int sbm_occ_ot_body_device(sbm_occ_tree* tree, void* d_bytes, size_t cap, size_t* nbytes);
/* tree.write(path): the header with the tree's size and resolution, then that body. SBM_ERR_NULL; SBM_ERR_UNSUPPORTED for a tree
 * built with SBM_OCC_TREE_MAXLIKELIHOOD or a file that cannot be written; SBM_ERR_NOMEM. */
int sbm_occ_ot_write(sbm_occ_tree* tree, const char* path);
/* Plain host code, no GPU: parse n bytes of an .ot stream and report its counts. On an error *out holds what was read up to it.
 * SBM_ERR_NULL (bytes may be NULL only for n == 0), then the codes under "status" but the map's. */
int sbm_occ_ot_info(const void* bytes, size_t n, sbm_occ_ot_header* out);
/* Plain host code, no GPU: the leaves in stream order, which is Morton order -- the packed key of the cube's lowest voxel, the
 * depth and the value -- into arrays of cap entries. *count receives their number; when it exceeds cap nothing is written and the
 * call returns SBM_ERR_SIZE. SBM_ERR_NULL (the arrays may be NULL only for cap == 0), then the codes under "status", which leave
 * *count as it was. */
int sbm_occ_ot_leaves(const void* bytes, size_t n, uint64_t* first_key, int32_t* depth, float* value, size_t cap, size_t* count);
/* AbstractOcTree::read from n bytes in HOST memory, read before the call returns. No ray parameters: nothing is clamped. See
 * "load" and "status"; the reset and the expansion are asynchronous on the handle's stream unless sync != 0 or profiling is on,
 * and a voxel that finds no slot within the probe bound counts as overflow, as for sbm_occ_load_binary. */
int sbm_occ_ot_load(sbm_occ_map* map, const void* bytes, size_t n, int sync);
/* The same from a file; SBM_ERR_UNSUPPORTED when it cannot be opened or read. */
int sbm_occ_ot_read(sbm_occ_map* map, const char* path, int sync);

/* ---- occupancy map: insert options, discretize, the bounding box and change detection (OccupancyOcTreeBase.hxx:148-165,
 * 222-259, 415-427, 891-918) ------------------------------------------------------------------------------------------------------
 * The three switches of insertPointCloud that a long-running mapper needs, for the log-odds mode above ("occupancy map: ray-cast
 * free space"), whose every statement stays true when all three are off. All three are per-voxel contracts.
 * tests/occupancy_option_cases.py is a literal transcription of this text, and tests/golden/occupancy_options.npz holds what the
 * reference's own octomap answered: after every scan the leaves and the changed keys, bit for bit.
 *  discretize computeDiscreteUpdate: per point and per axis k = (uint16)((int)floor(factor * (double)coord) + 32768), the
 *             UNCHECKED coordToKey. QUIRK, restated on purpose: a coordinate outside +-3276.8 m whose floor still fits an int
 *             wraps modulo 65536 and lands inside the map (x = 3300 gives key 232, centre -3253.55). A point with a coordinate
 *             that is not finite, or whose floor fits no int, is dropped (the reference's cast is undefined there). The
 *             distinct keys of the scan each give ONE point, keyToCoord(k) per axis = (float)(((double)((int)k - 32768) + 0.5)
 *             * resolution), and that list goes through the scan unchanged: the range gate, the truncation and the box tests
 *             see the voxel centre, not the original point. The result is a set; it does not depend on which duplicate wins.
 *  box        two float points, min and max, with their keys from coordToKeyChecked; a new map holds (0, 0, 0) twice. Setting a
 *             point that has no key (NaN included) returns SBM_ERR_SIZE and leaves the box as it was (octomap logs an error and
 *             keeps a half-written key). min > max on an axis is accepted: nothing is inside such a box. With the limit on, per
 *             point p: its voxel is occupied iff inBBX(p) in FLOAT (>= min and <= max per axis, both inclusive) and p is within
 *             range and coordToKeyChecked(p) passes, whether or not a ray exists; the ray runs to p, or to the truncated end when
 *             p is beyond max_range; its cells are taken in order while inBBX(key) holds (by KEY, inclusive), and the first cell
 *             outside ENDS THE RAY. An origin outside the box therefore frees nothing, even when the ray crosses the box later.
 *             free -= occupied as before.
 *  changes    per voxel one of three states: none, created (octomap's true), flipped (octomap's false). While detection is on,
 *             the one update a voxel gets per scan makes a voxel that was absent before the scan `created`; otherwise, if
 *             isNodeOccupied (logodds >= logodds(occupancy_thres)) differs before and after the update: none -> flipped, flipped
 *             -> none (octomap erases the entry), created stays. sbm_occ_reset_change_detection clears every state; disabling
 *             stops recording and keeps what is recorded. A voxel lost to overflow records nothing.
 *             DIVERGENCE: sbm_occ_reset and the .bt / .ot loaders clear the states (octomap's clear() keeps keys of nodes that
 *             no longer exist). The two switches and the box survive a reset. The loaders record nothing, as readBinary / read
 *             record nothing.
 *  lazy_eval  only defers octomap's inner nodes; the depth-16 values are identical. The C++ adaptor accepts the flag and ignores it.
 *  Mode. The box, detection and discretize belong to the log-odds mode. SBM_ERR_UNSUPPORTED, and nothing changes: enabling the
 *  box or detection on a map in hit mode; a hit insert (sbm_occ_insert*) on a map with either switch on; a change fetch or count
 *  on a map in hit mode.
 *  Device. The switches select instantiations of the MARK and APPLY kernels; with both off the launches
 *  are the ones of the section above. Box: MARK tests every cell, the origin's included, against the key box before it marks it,
 *  and the end point against the float box. Changes: one byte per slot, allocated by the first enable; the lane whose
 *  compare-and-swap claimed a slot ORs "created this scan" into the flag word with its bit, and APPLY, which visits a touched slot
 *  once, steps the state without an atomic. Discretize: a launch before MARK, one lane per point, claims the wrapped key in a
 *  per-scan scratch set (64-bit compare-and-swap, open addressing over at least twice the points, cleared per scan in stream
 *  order); the claiming lane appends the key to a list, and MARK runs one lane per list entry. No float atomics, no spin waits,
 *  no grid barriers. sbm_get_profile: no new names; the dedupe counts under "occ_rays_mark", the change fetch under "occ_fetch". */
/* The box's two points (HOST memory). SBM_ERR_NULL; SBM_ERR_SIZE when a coordinate of either has no key: the box is then as it
 * was. Host code: serves a map in either mode. */
int sbm_occ_set_bbx(sbm_occ_map* map, const float min[3], const float max[3]);
/* useBBXLimit(enable != 0) for the inserts that follow. SBM_ERR_NULL; SBM_ERR_UNSUPPORTED to enable on a map in hit mode. */
int sbm_occ_use_bbx_limit(sbm_occ_map* map, int enable);
/* The box as it is: its points, their keys and the switch; every output may be NULL. SBM_ERR_NULL without a map. */
int sbm_occ_get_bbx(sbm_occ_map* map, float min[3], float max[3], uint16_t min_key[3], uint16_t max_key[3], int* enabled);
/* enableChangeDetection(enable != 0) for the inserts that follow. The first enable allocates one byte per slot. SBM_ERR_NULL;
 * SBM_ERR_UNSUPPORTED to enable on a map in hit mode. */
int sbm_occ_enable_change_detection(sbm_occ_map* map, int enable);
/* isChangeDetectionEnabled into *enabled. SBM_ERR_NULL. */
int sbm_occ_change_detection_enabled(sbm_occ_map* map, int* enabled);
/* resetChangeDetection: every state becomes none, in stream order. SBM_ERR_NULL. */
int sbm_occ_reset_change_detection(sbm_occ_map* map);
/* numChangesDetected into *count. Synchronous. SBM_ERR_NULL; SBM_ERR_UNSUPPORTED for a map in hit mode. */
int sbm_occ_num_changes(sbm_occ_map* map, size_t* count);
/* changedKeys, as sbm_occ_fetch_logodds_device fetches: the changed voxels ascending by packed key (octomap's KeyBoolMap has no
 * order of its own) through the map's radix sort, with one byte per key in d_created (may be NULL): 1 created, 0 flipped. d_keys
 * (8-byte aligned) and d_created hold cap entries in DEVICE memory; *count receives the number of changes, and when it exceeds
 * cap nothing is written and the call returns SBM_ERR_SIZE. Synchronous; the map is left as it was. SBM_ERR_NULL (d_keys may be
 * NULL only for cap == 0); SBM_ERR_UNSUPPORTED for a misaligned d_keys or a map in hit mode. */
int sbm_occ_fetch_changes_device(sbm_occ_map* map, void* d_keys, void* d_created, size_t cap, size_t* count);
/* The same into HOST memory. */
int sbm_occ_fetch_changes(sbm_occ_map* map, uint64_t* keys, uint8_t* created, size_t cap, size_t* count);
/* insertPointCloud(scan, origin, maxrange, lazy_eval, discretize = true): the arguments, checks and codes of
 * sbm_occ_insert_cloud_device / sbm_occ_insert_cloud, the scan discretised as stated above. */
int sbm_occ_insert_cloud_discrete_device(sbm_occ_map* map, size_t n_points, const void* d_xyz, const float* origin,
                                         const sbm_occ_ray_params* params, int sync);
int sbm_occ_insert_cloud_discrete(sbm_occ_map* map, size_t n_points, const float* xyz, const float* origin,
                                  const sbm_occ_ray_params* params);
/* The arguments, checks and codes of sbm_occ_insert_rays_device / sbm_occ_insert_rays; every plane is one discretised scan of the
 * points sbm_occ_insert_rays_device gives it (the pixels the hit insert reprojects and transforms). */
int sbm_occ_insert_rays_discrete_device(sbm_occ_map* map, int n, const void* d_disp, int width, int height, int scale,
                                        const sbm_stereo_model* model, const float* poses, const sbm_occ_ray_params* params, int sync);
int sbm_occ_insert_rays_discrete(sbm_occ_map* map, int n, const int16_t* disp, int width, int height, int scale,
                                 const sbm_stereo_model* model, const float* poses, const sbm_occ_ray_params* params);

/* ---- occupancy map: growth, a table that rehashes itself into a larger one on the device ---------------------------------------
 * octomap has no full map: updateNode and insertPointCloud never refuse a voxel. sbm_occ_create fixes a capacity, and a voxel
 * that finds no slot is counted (SBM_ERR_OCC_FULL, sbm_occ_overflow) and lost. A mapper that cannot know its voxel count in
 * advance either reserves more by hand (sbm_occ_reserve) or lets the map grow (sbm_occ_set_growth). No statement of the sections
 * above depends on which slot a key sits in, so the contract is one sentence: a map that grew is, bit for bit, what the same
 * calls produce on a map created large enough -- keys, hit counts or log-odds bits, change states, every fetch, query, tree and
 * written file. tests/test_gpu_occupancy_growth.py holds it to the octomap fixtures from a capacity of 1.
 *  Off by default. Growth is a switch, off in a new map; a map that never enables it and never reserves behaves as stated above
 *  and its calls launch what they launched before this section existed: growth-off maps launch the same kernels, and none of
 *  this section's.
 *  Policy, stated once in sbm_occ_growth_step: a step doubles the capacity, reaches at least what is needed -- the size the
 *  counters report, twice that size where a cell found no slot, the voxel count of a load --, and clamps to the ceiling
 *  (max_capacity; 0 is the create limit of 2^30 voxels). The slots follow as sbm_occ_create rounds them: the
 *  power of two >= 2 * capacity. A step begins only when a cell found no slot or the size has passed the nominal capacity, so the
 *  load stays at or below one half and the capacity at or below max(the created capacity, 4 * size).
 *  Log-odds inserts (cloud, planes, discretised; every box / change-detection instantiation). The host reads the counters
 *  between MARK and APPLY. MARK is idempotent: it claims keys and ORs bits, and a slot enters the touched list only when its flag
 *  word was clear. If cells were lost the table is rehashed -- flag words, "created this scan" among them, move with their
 *  keys, and the touched list is rebuilt from them --, the overflow counter goes back to its value before the scan, and the same
 *  MARK runs again, until nothing is lost or the ceiling stops it; then APPLY runs once.
 *  Hit inserts add counts and cannot run twice. The host keeps an upper bound on the size (launched pixels add up; every counter
 *  read makes it exact). A launch whose pixels, added to that bound, exceed the capacity is preceded by a claim pass: the
 *  insert's own front half, which claims keys, counts the ones that found no slot and adds no hit. It is redone after a rehash;
 *  after it the unchanged insert kernel finds every key.
 *  Loaders. sbm_occ_load_binary / sbm_occ_read_binary and sbm_occ_ot_load / sbm_occ_ot_read know the voxel count before they
 *  touch the map; with growth on they reserve it where they returned SBM_ERR_OCC_FULL (a count above the ceiling still does).
 *  Stopped. Where the ceiling or a refused allocation stops a step, the call finishes exactly as a growth-off call on the table
 *  it has: lost cells are counted, the call returns SBM_ERR_OCC_FULL, and sbm_last_hip_error holds the allocation's error.
 *  Synchronisation. With growth on, every insert and load waits for its own launches to read the counters: sync == 0 calls may
 *  synchronise internally and are NOT capturable in a graph. With growth off nothing changes. A rehash allocates the new table
 *  beside the old one (12 B per slot, 20 B in log-odds mode, 21 B with change states) and frees the old one after the move.
 *  DIVERGENCE from a pre-sized map, none in content: the order of slots, and therefore nothing a caller can see. A tree built
 *  before a growth answers as built (it is a snapshot). The probe bound (1024 slots) is unchanged; a key that finds no slot
 *  within it in the larger table -- not seen at a load of one half -- is counted as lost.
 *  Device. One lane per old slot; a stored key takes its place through the table's 64-bit
 *  compare-and-swap (keys are distinct: every swap on an empty slot claims), plain vector stores carry its words, and the lanes
 *  with a set flag word append their new slot to the touched list with one atomic per wavefront. No float atomics, no spin
 *  waits, no grid barriers. sbm_get_profile: no new names; growth inside a call counts under that call's stage ("occ_rays_mark",
 *  "occ_insert", "occ_load"), and an explicit sbm_occ_reserve records nothing. */
typedef struct sbm_occ_growth_info {
  int32_t enabled;        /* the switch */
  int32_t reserved;
  uint64_t capacity;      /* nominal, in voxels */
  uint64_t slots;         /* of the table: the power of two >= 2 * capacity */
  uint64_t max_capacity;  /* the ceiling in voxels (2^30 where none was given) */
  uint64_t grown;         /* tables moved into a larger one so far, reserves and loads included */
  uint64_t moved;         /* slots those moves carried */
  uint64_t redone;        /* MARK launches and claim passes run again after a move */
} sbm_occ_growth_info;
/* The nominal capacity into *capacity. Host code. SBM_ERR_NULL; *capacity is written only on SBM_OK. */
int sbm_occ_capacity(sbm_occ_map* map, size_t* capacity);
/* Moves the map into a table for at least `capacity` voxels, on the device, in stream order behind earlier asynchronous calls;
 * synchronous. Independent of the switch. It never shrinks: a value at or below the current capacity is SBM_OK and does
 * nothing. Everything the map holds is the same afterwards: keys, hit counts or log-odds bits, change states, the overflow
 * counter, mode, scan parity, the switches and the box. SBM_ERR_NULL; SBM_ERR_UNSUPPORTED above 2^30; SBM_ERR_NOMEM when an
 * allocation is refused (SBM_ERR_HIP for another error): in all of these the map stays exactly as it was. */
int sbm_occ_reserve(sbm_occ_map* map, size_t capacity);
/* The switch (enable != 0) for the inserts and loads that follow, and its ceiling: max_capacity voxels, 0 meaning the create
 * limit of 2^30. Survives sbm_occ_reset, as the other switches do. Host code: serves a map in either mode. SBM_ERR_NULL;
 * SBM_ERR_UNSUPPORTED for a ceiling above 2^30, and nothing changes. A ceiling below the current capacity stops every step. */
int sbm_occ_set_growth(sbm_occ_map* map, int enable, size_t max_capacity);
/* The switch, the table and the counts so far into *out. Host code. SBM_ERR_NULL; *out is written only on SBM_OK. */
int sbm_occ_get_growth(sbm_occ_map* map, sbm_occ_growth_info* out);
/* The policy, plain host code: the capacity a growth step goes to from `capacity` when `need` voxels are known, under the
 * ceiling max_capacity (0 or above 2^30: 2^30). *next = min(max(2 * capacity, need, 1), ceiling). SBM_ERR_NULL;
 * SBM_ERR_OCC_FULL when capacity is already at or above the ceiling, and *next is left alone. */
int sbm_occ_growth_step(size_t capacity, size_t need, size_t max_capacity, size_t* next);

/* ---- occupancy map: edit voxels by key, updateNode, setNodeValue and deleteNode (OccupancyOcTreeBase.hxx:273-285, 307-327,
 * 373-433, 1097-1107; OcTreeBaseImpl.hxx:501-509, 681-716) --------------------------------------------------------------------------
 * A scan is not the only way to write a map: a caller marks or clears single voxels, seeds a prior, replays the keys that
 * sbm_occ_fetch_changes of another map produced, and forgets voxels, which is how a map at its ceiling keeps a sliding window
 * around the robot. Everything is stated per depth-16 voxel, as the inserts are; arithmetic is IEEE binary32 as written, with
 * no contraction. tests/occupancy_edit_cases.py is a literal transcription of this text, and tests/golden/occupancy_edit.npz
 * holds what the reference's own octomap answered after every step, bit for bit.
 *  Items. An item is (key or point, op, value); cmin, cmax and thres are the log-odds of the call's clamp_min, clamp_max and
 *  occupancy_thres (sbm_occ_ray_logodds); v is the voxel's log-odds.
 *   SBM_OCC_EDIT_UPDATE  updateNode(key, float u). EARLY ABORT: if the voxel exists and (u >= 0 && v >= cmax) or (u <= 0 && v <=
 *             cmin), nothing happens at all, and no change record is made either. Otherwise an absent voxel is created at 0;
 *             then v = v + u; v = cmin if v < cmin, else cmax if v > cmax (a NaN passes both tests and stays).
 *             updateNode(key, bool) is this with u = the hit or the miss log-odds; the adaptors form it on the host from
 *             sbm_occ_ray_params, as sbm_occ_ray_logodds does. The C-ABI takes floats only.
 *   SBM_OCC_EDIT_SET     setNodeValue(key, float x). x = min(max(x, cmin), cmax) with the two std:: comparisons as written,
 *             max(a, b) = a < b ? b : a and min(a, b) = b < a ? b : a, so a NaN stays NaN. An absent voxel is created. v = x.
 *   SBM_OCC_EDIT_DELETE  deleteNode(key, depth 16): the voxel is removed with all it holds, its log-odds and its change state.
 *             The value is not read. Deleting what is not there is not an error.
 *  deleteNode(key, depth d) of sbm_occ_delete: d 0 means 16; d outside 0..16 gives SBM_ERR_UNSUPPORTED. Every stored voxel whose
 *  three key components agree with the given key in their top d bits is removed with all it holds: log-odds or hit count, and the
 *  change state. The rest of the map is untouched.
 *  Change detection steps as octomap's leaf code does, per item, while detection is on: a voxel created by the item gets
 *  `created`; else, where v >= thres differs before and after the item: none -> flipped, flipped -> none, and created stays.
 *  Point forms. The key is coordToKeyChecked per axis (floor(factor * (double)coord) + 32768 within 0..65535). An item whose point
 *  has no key is skipped, where octomap returns NULL or false.
 *  Key forms. Keys are the packed k0 << 32 | k1 << 16 | k2. An item with a bit above 47 set is skipped. An op outside the three
 *  values cannot be checked on the host for device arrays: such an item is skipped too. Skipped items are counted.
 *  ORDER. Items of one call that name the same voxel take effect in item order: the clamps, setNodeValue and deletes in between
 *  make the result depend on it (set then update differs from update then set; delete then update creates again from 0). Items
 *  of different voxels do not interact. Calls take effect in call order.
 *  DIVERGENCE, deleting the last voxel: it leaves an empty map here, and search says unknown. octomap keeps a childless root,
 *  which its search then returns for every key.
 *  DIVERGENCE, a deleted voxel's change record: it goes with the voxel here. octomap keeps the key in changed_keys, and its
 *  std::map::insert then does not overwrite it when the voxel is created again.
 *  Modes. Update and set belong to the log-odds mode: they fix the mode of a fresh map, as sbm_occ_insert_cloud does, and on a hit
 *  map they return SBM_ERR_UNSUPPORTED and leave the map as it was (so does any sbm_occ_edit* call on a hit map, whatever its
 *  items). Deletes (sbm_occ_delete*, sbm_occ_delete_box) serve both modes and leave the mode of a fresh map open: a hit map loses
 *  the key and its count.
 *  Large batches. n is up to 2^30. A batch is worked through in chunks of SBM_OCC_EDIT_CHUNK = 2097152 items, in item order, so
 *  that scratch stays bounded: 28 B per item of a chunk (sorted keys, indices, the sort's second buffers, one slot per item).
 *  Full table. With growth off an update or set item whose voxel finds no slot within the probe bound raises the overflow
 *  counter once and is counted as lost; the call returns SBM_ERR_OCC_FULL; that voxel gets none of its items, every other voxel
 *  gets all of its own. With growth on the claim pass is idempotent and is settled as MARK is ("occupancy map: growth"): the
 *  table is rehashed and the same claims run again until nothing is lost or the ceiling stops it.
 *  Deletes and the table. A call that removes something moves the map into a fresh table of the same capacity without the
 *  removed slots -- it never shrinks --, so lookups, inserts, fetches and queries stay exactly as they are: there are no
 *  tombstones. The move's buffers are allocated before anything is applied (per chunk; a batch of up to one chunk is applied
 *  whole or not at all): a refused allocation returns SBM_ERR_NOMEM, with the error in sbm_last_hip_error, and the map is exactly
 *  as it was. A call that may remove -- sbm_occ_delete*, sbm_occ_delete_box, and sbm_occ_edit* given ops -- synchronises whatever
 *  `sync` says (the host counts the delete items, and reads what was removed), and cannot be captured in a graph; sbm_occ_edit*
 *  with ops == NULL on a map that does not grow is asynchronous as the inserts are. Afterwards the size counter, and the hit
 *  mode's host-side bound on it, are right; the overflow counter is unchanged; a tree built earlier is a snapshot and answers as
 *  built. The insert's bounding box and its switch are not touched by sbm_occ_delete_box.
 *  Device. CLAIM: one lane per item finds or claims the slot (the table's 64-bit compare-and-swap; delete
 *  items only look) and counts claims, losses and skips. ORDER: the map's LSD radix sort orders (packed key, item index) pairs; it
 *  is stable, so item order inside a voxel's run survives. APPLY: one lane per run head -- found from the sorted keys, not from
 *  lane position -- walks its run with the rules above from the slot's current word to its final one, steps the change byte and
 *  marks the slot in a removal mask if the voxel ends the batch absent. REMOVE: range and box deletes mark by predicate, one lane
 *  per slot; the move is the growth section's, with the mask. Per-slot values are written with plain vector stores. No float
 *  atomics, no spin waits, no grid barriers. sbm_get_profile: no new names; CLAIM counts under "occ_rays_mark"; ORDER, APPLY and
 *  the move under "occ_rays_apply"; a delete on a hit map under "occ_insert". */
enum { SBM_OCC_EDIT_UPDATE = 0, SBM_OCC_EDIT_SET = 1, SBM_OCC_EDIT_DELETE = 2 };
#define SBM_OCC_EDIT_CHUNK 2097152
typedef struct sbm_occ_edit_info {
  uint64_t items;         /* of the last edit or delete call (sbm_occ_delete_box: 0) */
  uint64_t skipped;       /* items without a key, with a key above bit 47 or with an unknown op */
  uint64_t lost;          /* update and set items whose voxel found no slot */
  uint64_t created;       /* voxels that were absent when the call began and were given a slot */
  uint64_t removed;       /* voxels taken out of the table */
} sbm_occ_edit_info;
/* n mixed items in item order: d_keys n packed keys (8-byte aligned), d_ops n bytes (SBM_OCC_EDIT_*; NULL means all updates),
 * d_values n floats (4-byte aligned), all in DEVICE memory; params (HOST memory) gives the clamps and the threshold. Asynchronous
 * on the handle's stream unless sync != 0, profiling is on, growth is on or d_ops is given (see "Deletes and the table").
 * SBM_ERR_NULL (d_keys and d_values may be NULL only for n == 0); SBM_ERR_SIZE for params sbm_occ_ray_params_validate rejects;
 * SBM_ERR_UNSUPPORTED for n above 2^30, a misaligned array or a map in hit mode; SBM_ERR_NOMEM; SBM_ERR_OCC_FULL. */
int sbm_occ_edit_device(sbm_occ_map* map, size_t n, const void* d_keys, const void* d_ops, const void* d_values,
                        const sbm_occ_ray_params* params, int sync);
/* The same from HOST memory, read before the call returns. Synchronous. */
int sbm_occ_edit(sbm_occ_map* map, size_t n, const uint64_t* keys, const uint8_t* ops, const float* values,
                 const sbm_occ_ray_params* params);
/* The same with n float triples (4-byte aligned, DEVICE memory) in place of the keys. */
int sbm_occ_edit_points_device(sbm_occ_map* map, size_t n, const void* d_xyz, const void* d_ops, const void* d_values,
                               const sbm_occ_ray_params* params, int sync);
int sbm_occ_edit_points(sbm_occ_map* map, size_t n, const float* xyz, const uint8_t* ops, const float* values,
                        const sbm_occ_ray_params* params);
/* deleteNode(key, depth) for n packed keys in DEVICE memory (8-byte aligned). Synchronous; either mode. SBM_ERR_NULL (d_keys may
 * be NULL only for n == 0); SBM_ERR_UNSUPPORTED for a depth outside 0..16, n above 2^30 or a misaligned array; SBM_ERR_NOMEM. */
int sbm_occ_delete_device(sbm_occ_map* map, size_t n, const void* d_keys, int depth);
/* The same from HOST memory. */
int sbm_occ_delete(sbm_occ_map* map, size_t n, const uint64_t* keys, int depth);
/* Removes every voxel inside (outside != 0: outside) the key box, inclusive on both ends: inBBX(key) of "insert options" with
 * these bounds, the loop octomap's users write (collect the depth-16 keys that pass the test, then deleteNode each). min > max on
 * an axis is the empty box: nothing is inside it. Synchronous; either mode. SBM_ERR_NULL; SBM_ERR_NOMEM. */
int sbm_occ_delete_box(sbm_occ_map* map, const uint16_t min_key[3], const uint16_t max_key[3], int outside);
/* Synchronises and returns the counts of the last edit or delete call. SBM_ERR_NULL; *out is written only on SBM_OK. */
int sbm_occ_last_edit(sbm_occ_map* map, sbm_occ_edit_info* out);

/* ---- occupancy map: the read side for planners (begin_leafs_bbx, OcTreeIterator.hxx:335-460; getUnknownLeafCenters and getMetricMin /
 * getMetricMax / volume, OcTreeBaseImpl.hxx:872-1116; getRayIntersection, OccupancyOcTreeBase.hxx:768-853) ---------------------------
 * How a planner or an explorer reads an octomap, on the device and without fetching the voxels: the leaves inside a box, the cells
 * of a box that are still unknown, the metric bounds of the map, and where a ray enters the voxel it hit. Each is octomap's own
 * function restated operation by operation; tests/occupancy_planner_cases.py is a literal transcription of this text and
 * tests/golden/occupancy_planner.npz holds what the reference's own octomap answered, which the device equals bit for bit. The
 * first three read an sbm_occ_tree SNAPSHOT (a tree that was never built answers as an empty one), the fourth needs the map's
 * resolution only. All are read-only: the map, the tree and every entry point above stay as they are, and a tree or map that
 * never calls these launches what it launched before. The names do not begin with sbm_occ_tree_ although three take a tree: that
 * prefix is the closed set of the section "the octree above the voxels".
 *  leaves in a key box   begin_leafs_bbx(min, max, maxDepth). Output layout, order, the cap / *count / SBM_ERR_SIZE rule and the
 *             max_depth rule (0 means 16) are those of sbm_occ_tree_leaves_device; the entries are the subsequence of
 *             leaves(max_depth) that the iterator visits. singleIncrement pushes a child at depth d with centre key c and
 *             off = 32768 >> d iff, on every axis, min <= c + off && max >= c - off, in int. The test is LOOSE BY ONE KEY at the
 *             upper side of a cube (a cube covers c - off .. c + off - 1): a box whose minimum equals a cube's one-past-end key
 *             still visits that cube. The root itself is never tested. A node's own test implies its ancestors' tests -- the
 *             interval [c - off, c + off] of a child lies inside its parent's, on either side and at depth 16 as well, where off
 *             is 0 and the child's key is c or c - 1 of its parent -- so one lane per node decides for itself, and the visited set
 *             is: every entry of leaves(max_depth) that passes its own test. A box with min > max on an axis visits no depth-16
 *             voxel (off is 0 there); a node above them whose loose interval holds both bounds is still visited, as octomap does.
 *             The point form applies coordToKeyChecked to both corners; if either has no key it returns SBM_OK with a count of 0.
 *             DIVERGENCE: octomap's constructor says "set to end iterator" there, but it leaves the root on the stack and its loop
 *             visits the root once; the fixture records that entry, the library returns none.
 *  unknown cells in a box   getUnknownLeafCenters(centres, pmin, pmax, depth), literally: depth 0 means 16; each corner is clamped
 *             to keyToCoord(coordToKey(p, depth), depth) as floats; step_size is the float of resolution * pow(2, 16 - depth);
 *             steps[i] = floor(diff[i] / step_size) with diff the float difference of the clamped corners; each coordinate is a
 *             running float sum from the clamped pmin, incremented BEFORE the query, so the cell at pmin itself is never asked and
 *             the reported floats are not keyToCoord centres; a centre is reported iff search(p, depth) is NULL, which covers a
 *             point without a key. Output: float triples in octomap's push order, x outermost and z innermost. Each axis resets
 *             to the clamped pmin, so the three running sums are independent: the host forms three tables of at most 65 536
 *             floats, sequentially, and one lane per cell of the steps[0] x steps[1] x steps[2] grid does the lookup of search at
 *             the asked level. DIVERGENCES: coordToKey is unchecked in octomap and wraps its 16-bit cast for a corner outside the
 *             key space; such a corner (a NaN among them) is refused with SBM_ERR_SIZE. A step count that is negative (pmax below
 *             pmin on an axis), which octomap casts to unsigned with no defined result, is 0 steps: nothing is reported.
 *  metric bounds   getMetricMin / getMetricMax, the const forms: over every leaf of the pruned tree the minimum of
 *             keyToCoord(centre key, depth) - getNodeSize(depth) / 2.0 and the maximum of the same centre plus half the size, all
 *             in double, with keyToCoord's three cases (depth 0: 0.0; depth 16: (key - 32768 + 0.5) * resolution; between:
 *             (floor((key - 32768) / 2^(16 - depth)) + 0.5) * getNodeSize(depth)). An empty tree answers six zeros. At a fixed
 *             depth these are non-decreasing functions of the key, so the device reduces the smallest and largest centre key per
 *             axis and depth with integer minima / maxima (no float atomics) and the host forms at most 17 x 6 doubles; the result
 *             is cached in the tree until the next build. Size is max - min and volume is x * y * z of the size. The bounds of
 *             the pruned tree and of its expanded voxels may differ in the last bit, as they do in octomap (the fixture records
 *             both); octomap's non-const calcMinMax forms the maximum as (centre - half) + size, which may differ likewise (the
 *             fixture records it, the library does not provide it).
 *  ray entry   getRayIntersection(origin, direction, center, intersection, delta), literally: the half cell is
 *             float(resolution / 2.0); Vector3::dot multiplies and adds in float and returns double; operator- and
 *             direction * float(d) + origin are float; per axis whose normal . direction != 0.0 the two planes are met at
 *             d = (point - origin) . normal / (normal . direction) in double, and a meeting point passes unless one of its two
 *             other coordinates is below the lower plane - 1e-6 or above the upper plane + 1e-6, compared in double; outD is the
 *             minimum of d over the planes that pass; the result is direction * float(outD + delta) + origin. The direction is
 *             NOT normalised here, and a negative d counts (an origin inside the voxel, a voxel behind the origin). found 0
 *             leaves a NaN triple (0x7FC00000) where octomap leaves `intersection` untouched, the convention of SBM_OCC_RAY_NONE.
 *             A zero direction meets no plane: not found. A NaN or infinite direction needs no special case: normal . direction
 *             is NaN (x * 0 of an infinite x) or the value itself, != 0.0 holds, and every comparison with a NaN meeting point
 *             is false, so the plane passes: found is 1. std::min(outD, d) leaves outD where d is NaN, and the result carries NaN
 *             in the coordinates where the float arithmetic gives it (0 * inf, anything * NaN), exactly as octomap. getNormals is NOT provided: it needs octomap's marching-cubes tables.
 *  Device. One launch per step, integer counters per wavefront, kernel boundaries only. The box iterator
 *  runs a count pass, reads the count, then selects, sorts and gathers as sbm_occ_tree_leaves_device does. The unknown cells count
 *  per tile of 1024 cells, scan the tile counts and write in linear cell order. No kernel contracts a multiply-add.
 *  sbm_get_profile: the tree calls add to "occ_tree_query", the ray entries to "occ_cast". */
/* begin_leafs_bbx by keys into d_keys (uint64, 8-byte aligned), d_depth (int32) and d_value (float, may be NULL), cap entries each,
 * DEVICE memory; min_key / max_key are HOST memory. *count receives the number of entries; when it exceeds cap nothing is written
 * and the call returns SBM_ERR_SIZE. Synchronous; waits for the stream twice. Checked in this order before anything is launched:
 * SBM_ERR_NULL (d_keys and d_depth may be NULL only for cap == 0); SBM_ERR_SIZE for a max_depth outside 0..16;
 * SBM_ERR_UNSUPPORTED for a misaligned pointer. */
int sbm_occ_bbx_leaves_device(sbm_occ_tree* tree, const uint16_t min_key[3], const uint16_t max_key[3], int max_depth, void* d_keys,
                              void* d_depth, void* d_value, size_t cap, size_t* count);
/* The same into HOST memory. */
int sbm_occ_bbx_leaves(sbm_occ_tree* tree, const uint16_t min_key[3], const uint16_t max_key[3], int max_depth, uint64_t* keys,
                       int32_t* depth, float* value, size_t cap, size_t* count);
/* begin_leafs_bbx by points (HOST memory): the same checks, then coordToKeyChecked of both corners; a corner without a key gives
 * SBM_OK and a count of 0. */
int sbm_occ_bbx_leaves_points_device(sbm_occ_tree* tree, const float min[3], const float max[3], int max_depth, void* d_keys, void* d_depth,
                                     void* d_value, size_t cap, size_t* count);
int sbm_occ_bbx_leaves_points(sbm_occ_tree* tree, const float min[3], const float max[3], int max_depth, uint64_t* keys, int32_t* depth,
                              float* value, size_t cap, size_t* count);
/* getUnknownLeafCenters into d_xyz (cap float triples, DEVICE memory, 4-byte aligned); pmin / pmax are HOST memory. *count receives
 * the number of centres; when it exceeds cap nothing is written and the call returns SBM_ERR_SIZE. Synchronous. Checked in this
 * order before anything is launched: SBM_ERR_NULL (d_xyz may be NULL only for cap == 0); SBM_ERR_SIZE for a depth outside 0..16,
 * then for a corner outside the key space; SBM_ERR_UNSUPPORTED for a misaligned pointer, then for more than 2^30 cells. */
int sbm_occ_unknown_device(sbm_occ_tree* tree, const float pmin[3], const float pmax[3], int depth, void* d_xyz, size_t cap, size_t* count);
/* The same into HOST memory. */
int sbm_occ_unknown(sbm_occ_tree* tree, const float pmin[3], const float pmax[3], int depth, float* xyz, size_t cap, size_t* count);
/* getMetricMin and getMetricMax of the tree. The first call after a build reduces on the device and waits for the stream; later
 * calls answer from the tree. SBM_ERR_NULL. */
int sbm_occ_metric(sbm_occ_tree* tree, double min[3], double max[3]);
/* getRayIntersection on n rays: d_dirs, d_centres and d_xyz n float triples, d_found n int32 (may be NULL), DEVICE memory, 4-byte
 * aligned. Origins follow sbm_occ_cast_rays_device: n triples in DEVICE memory, or with shared_origin != 0 three floats in HOST
 * memory that every ray starts from. Read-only, one lane per ray. Asynchronous unless sync != 0. Checked in this order before
 * anything is launched: SBM_ERR_NULL (the arrays may be NULL only for n == 0, which is accepted and launches nothing);
 * SBM_ERR_SIZE for a NaN delta; SBM_ERR_UNSUPPORTED for more than 2^30 rays or a misaligned pointer. */
int sbm_occ_ray_intersections_device(sbm_occ_map* map, size_t n, const void* origins, int shared_origin, const void* d_dirs,
                                     const void* d_centres, double delta, void* d_xyz, void* d_found, int sync);
/* The same on HOST memory. Synchronous. */
int sbm_occ_ray_intersections(sbm_occ_map* map, size_t n, const float* origins, int shared_origin, const float* dirs, const float* centres,
                              double delta, float* xyz, int32_t* found);

/* ---- occupancy map: colour per voxel (ColorOcTree::setNodeColor, averageNodeColor; ColorOcTree.cpp:96-105, 146-161) -----------
 * A colour beside the log-odds of every voxel, as octomap's ColorOcTree keeps one per node: the coloured map a camera builds.
 * tests/occupancy_color_cases.py is a literal transcription of this text and tests/golden/occupancy_color.npz holds what the
 * reference's own octomap answered, which the device equals in every integer.
 *  Storage. One 32-bit word per slot, r | g << 8 | b << 16 (the top byte is zero). "Not set" is octomap's own convention: white
 *  (255, 255, 255) is isColorSet() == false, and there is no separate flag, so white given as a colour UNSETS the voxel. Colour
 *  exists in the log-odds mode only: every call below answers SBM_ERR_UNSUPPORTED on a hit map. The words are allocated at the
 *  first call that writes colours (sbm_occ_color_keys* / sbm_occ_color_points*), as the change bytes are at the first enable;
 *  such a call fixes the mode of a fresh map to log-odds, as an edit does, so that a hit insert after it is refused; a
 *  map that never makes such a call allocates nothing and launches exactly what it launched before, and the reads below answer
 *  white for every voxel of it.
 *  What moves or drops a slot carries or drops its colour: growth and the deletes' move carry the word with the key;
 *  sbm_occ_reset and the .bt / .ot loaders leave every voxel white; a voxel created by an insert or an edit is white, and so is
 *  one that was deleted and created again, also inside ONE edit batch (delete then set of a coloured voxel: the edit's APPLY
 *  stores white where a run passes through a delete and ends present, since no move drops that slot).
 *  The batch. Item i is (key or point, rgb word; the word's top byte is ignored). Both ops search(key) first: an item whose
 *  voxel is unknown does nothing. A packed key with a bit above 47 set, and a point outside the key space (coordToKeyChecked
 *  fails; a NaN among them), is skipped.
 *   SBM_OCC_COLOR_SET      setNodeColor: the voxel's colour is the item's.
 *   SBM_OCC_COLOR_AVERAGE  averageNodeColor: if the voxel is white the item's colour, else per channel (prev + new) / 2 in int
 *                          (truncating). The result depends on the order, and a chain that passes through white starts over.
 *  The op is per call. The items of one voxel take effect in item order, calls in call order; items of different voxels do not
 *  interact. n is up to 2^30, worked through in chunks of SBM_OCC_EDIT_CHUNK items in item order.
 *  Device. One lane per item looks its slot up (a look-up, never a claim); the map's stable radix sort of (key, item index)
 *  brings each voxel's items together in item order; one lane per run head -- found from the sorted keys, not from lane position
 *  -- walks its run sequentially from the slot's word to its final one, whatever the run's length (no closed form: the white
 *  restart breaks it), and stores it with a plain vector store. No atomics on colour words.
 *  DIVERGENCE, pruning during inserts. octomap with lazy_eval = false prunes and re-expands while it inserts; pruneNode and
 *  expandNode smear colours through copyData, and which transient prunes happen depends on the iteration order of an
 *  unordered_set. Here a colour belongs to ONE depth-16 voxel and is never smeared: the recordings drive octomap with lazy_eval =
 *  true inserts (no pruning during inserts) and colour by key on the unpruned tree. For the same reason, after octomap reads a
 *  pruned stream a colour call there colours a whole pruned leaf where this map colours one voxel, unless expand() is called first.
 *  Not provided: integrateNodeColor. It needs a double exp per voxel, and (uint8_t)(prev * p + r * (0.99 - p)) with prev == r
 *  sits on an integer boundary; whether the device's exp equals glibc's in every bit has not been measured and cannot be
 *  assumed. Not provided either: colour in hit mode, writeColorHistogram, and a colour argument on the insert
 *  calls: the caller colours after inserting, as octomap's users do. OcTreeStamped's stamps are a section of their own ("occupancy
 *  map: time stamps per voxel"); a map holds colours or stamps, not both.
 *  The tree. ColorOcTree::isNodeCollapsible ignores colour, so the pruned tree has the structure of the plain tree ("the octree
 *  above the voxels"); an sbm_occ_tree built over a map that has colours gets a colour word per node, octomap's after prune();
 *  updateInnerOccupancy(), in one bottom-up pass over the levels the build has. getAverageChildColor() is int sums of r, g, b over
 *  the children whose colour is SET, each divided by their count (truncating), or white if none is set. A node that is not
 *  collapsed takes it (updateColorChildren). A collapsed node takes child 0's colour (copyData) and, if that is set, replaces it
 *  by getAverageChildColor(): so a collapsed node whose child 0 is white is white even if its siblings are coloured. Bottom-up, a
 *  node over collapsed children uses their collapsed colours. The pass runs only when the map has colours: the build over a
 *  colourless map is unchanged, and its nodes answer white. sbm_occ_color_leaves* is sbm_occ_tree_leaves* with the colour word of
 *  every entry, in the same order, for both readings; the colour of an entry is found by a binary search over its depth's codes.
 *  The stream. AbstractOcTree::write with `id ColorOcTree`: the .ot header with that id line, then eight bytes per node of the
 *  pruned LOGODDS tree in pre-order -- the float value, r, g, b, the child mask (0 for a leaf) -- written on the device by the
 *  ranks of the plain .ot writer as two dwords per node. Loading (AbstractOcTree::read) parses on the host in one pass, as the
 *  .bt loader does, and expands on the device: every voxel of a leaf's cube takes the leaf's float, unclamped, and the leaf's
 *  colour. Status and refusals are those of "the .ot format" with eight bytes per record; a stream whose id is not ColorOcTree
 *  (a plain OcTree among them) is SBM_ERR_UNSUPPORTED, as sbm_occ_ot_* keep refusing `id ColorOcTree`; a refused stream leaves
 *  the map as it was. An inner node's colour in a stream is read and dropped, as its value is.
 *  sbm_get_profile: no new names. The batch is timed under "occ_rays_apply", the search under "occ_search", the fetch under
 *  "occ_fetch" (DESIGN.md section 29). */
enum { SBM_OCC_COLOR_SET = 0, SBM_OCC_COLOR_AVERAGE = 1 };
#define SBM_OCC_COLOR_WHITE 0x00FFFFFFu
typedef struct sbm_occ_color_info {
  uint64_t items;    /* of the last colour batch                                              */
  uint64_t found;    /* items whose voxel exists: they took effect                            */
  uint64_t unknown;  /* items with a valid key whose voxel is unknown: no-ops                 */
  uint64_t skipped;  /* items without a key: a bit above 47, or a point outside the key space */
} sbm_occ_color_info;
/* n items in item order: d_keys n packed keys (8-byte aligned), d_rgb n colour words (4-byte aligned), in DEVICE memory. op is
 * SBM_OCC_COLOR_*. Asynchronous on the handle's stream unless sync != 0. Checked in this order before anything is launched:
 * SBM_ERR_NULL (the arrays may be NULL only for n == 0); SBM_ERR_UNSUPPORTED for another op, more than 2^30 items, a hit map or a
 * misaligned pointer. SBM_ERR_NOMEM where the colour words cannot be allocated: the map is as it was. */
int sbm_occ_color_keys_device(sbm_occ_map* map, size_t n, const void* d_keys, const void* d_rgb, int op, int sync);
/* The same on HOST memory. Synchronous. */
int sbm_occ_color_keys(sbm_occ_map* map, size_t n, const uint64_t* keys, const uint32_t* rgb, int op);
/* The same by points: d_xyz n float triples (4-byte aligned); a point's key is coordToKeyChecked's. */
int sbm_occ_color_points_device(sbm_occ_map* map, size_t n, const void* d_xyz, const void* d_rgb, int op, int sync);
int sbm_occ_color_points(sbm_occ_map* map, size_t n, const float* xyz, const uint32_t* rgb, int op);
/* Synchronises and returns the counts of the last colour batch (zeros before the first). SBM_ERR_NULL; *out is written only on
 * SBM_OK. */
int sbm_occ_color_last(sbm_occ_map* map, sbm_occ_color_info* out);
/* sbm_occ_search_device with a colour: d_color n colour words (may be NULL, as d_value may). An unknown voxel and a point
 * outside the key space answer SBM_OCC_COLOR_WHITE and the quiet NaN 0x7FC00000. Read-only; it allocates nothing. The checks are
 * sbm_occ_search_device's, and SBM_ERR_UNSUPPORTED on a hit map. */
int sbm_occ_color_search_device(sbm_occ_map* map, size_t n, const void* d_xyz, float occupancy_thres_log, void* d_state, void* d_value,
                                void* d_color, int sync);
/* The same on HOST memory. Synchronous. */
int sbm_occ_color_search(sbm_occ_map* map, size_t n, const float* xyz, float occupancy_thres_log, int32_t* state, void* value,
                         uint32_t* color);
/* sbm_occ_fetch_logodds_device with the colours: the voxels in ascending order of their packed keys, d_logodds and d_colors cap
 * 4-byte words each (either may be NULL). Same cap / *count / SBM_ERR_SIZE / SBM_ERR_OCC_FULL rule. Read-only. */
int sbm_occ_color_fetch_device(sbm_occ_map* map, void* d_keys, void* d_logodds, void* d_colors, size_t cap, size_t* count);
int sbm_occ_color_fetch(sbm_occ_map* map, uint64_t* keys, float* logodds, uint32_t* colors, size_t cap, size_t* count);
/* sbm_occ_tree_leaves_device with d_color, cap colour words in DEVICE memory, 4-byte aligned (NULL: exactly that call). Same
 * entries, order, checks and cap / *count rule. Synchronous. */
int sbm_occ_color_leaves_device(sbm_occ_tree* tree, int max_depth, void* d_keys, void* d_depth, void* d_value, void* d_color, size_t cap,
                                size_t* count);
/* The same on HOST memory; value may be NULL, color not. */
int sbm_occ_color_leaves(sbm_occ_tree* tree, int max_depth, uint64_t* keys, int32_t* depth, float* value, uint32_t* color, size_t cap,
                         size_t* count);
/* The ColorOcTree body of a LOGODDS tree into d_bytes (DEVICE memory, 4-byte aligned, cap bytes); *nbytes receives its length,
 * 8 * nodes; the rules of sbm_occ_ot_body_device. */
int sbm_occ_color_ot_body_device(sbm_occ_tree* tree, void* d_bytes, size_t cap, size_t* nbytes);
/* tree.write(path) of a ColorOcTree: the header, then that body. The codes of sbm_occ_ot_write. */
int sbm_occ_color_ot_write(sbm_occ_tree* tree, const char* path);
/* Plain host code, no GPU: sbm_occ_ot_info and sbm_occ_ot_leaves for a ColorOcTree stream, the leaves with their colour words. */
int sbm_occ_color_ot_info(const void* bytes, size_t n, sbm_occ_ot_header* out);
int sbm_occ_color_ot_leaves(const void* bytes, size_t n, uint64_t* first_key, int32_t* depth, float* value, uint32_t* color, size_t cap,
                            size_t* count);
/* AbstractOcTree::read of a ColorOcTree stream from n bytes in HOST memory, read before the call returns: the map's content is
 * replaced by the stream's voxels and their colours. Synchronous whatever `sync` says (the parse is the host's). The codes of
 * sbm_occ_ot_load. */
int sbm_occ_color_ot_load(sbm_occ_map* map, const void* bytes, size_t n, int sync);
/* The same from a file; SBM_ERR_UNSUPPORTED when it cannot be opened or read. */
int sbm_occ_color_ot_read(sbm_occ_map* map, const char* path, int sync);

/* ---- occupancy map: time stamps per voxel (OcTreeStamped.h, OcTreeStamped.cpp:43-68) -----------------------------------------
 * When a voxel was last observed, beside its log-odds, as octomap's OcTreeStamped keeps one per node: what a long-running mapper
 * needs to forget what it has not seen for a while. tests/occupancy_stamped_cases.py is a literal transcription of this text and
 * tests/golden/occupancy_stamped.npz holds what the reference's own octomap answered, which the device equals in every integer.
 *  Storage and the clock. One uint32 per slot. The time is the MAP'S CLOCK, a uint32 the caller sets (sbm_occ_stamp_set_time;
 *  0 after create): the library never reads the wall clock, and nothing requires the clock to be monotone. Every stamping call
 *  uses the clock as it is at the time of the call. sbm_occ_stamp_enable allocates the words, zeroed: existing voxels have stamp
 *  0, as after a load. It fixes the mode of a fresh map to log-odds, as a colour call or an edit does; a hit map is refused with
 *  SBM_ERR_UNSUPPORTED, and so is a map that already holds colour words: a map is one octomap class. For the same reason a
 *  stamped map refuses every colour write (sbm_occ_color_keys*, sbm_occ_color_points*, sbm_occ_color_ot_load / _read) with
 *  SBM_ERR_UNSUPPORTED and is as it was. A map that holds stamp words stays a log-odds map: sbm_occ_reset empties it and keeps the
 *  words and the clock, and sbm_occ_insert* (the hit insert) answers SBM_ERR_UNSUPPORTED on it, before and after a reset. A map that never enables stamps allocates nothing and launches exactly what it launched
 *  before; the reads below answer stamp 0 for every voxel of it, and the degrade and the forget refuse it.
 *  Stamping. Every per-voxel updateNode with a log-odds update stamps the voxel with the clock (OcTreeStamped::updateNodeLogOdds:
 *  the plain update, then updateTimestamp()) UNLESS updateNode's early return applies (OccupancyOcTreeBase.hxx:307-317), which
 *  comes before updateNodeLogOdds: the voxel exists, and (update >= 0 and value >= clamp max) or (update <= 0 and value <= clamp
 *  min). An update of exactly 0 tests both. So a wall hit ten times at clocks 1000..1009 saturates at the fifth hit and keeps stamp
 *  1004, and the degrade below degrades it although it was seen a second ago; after that it is below the clamp and the next hit
 *  stamps it again. This is octomap's behaviour, restated, not repaired. It covers the scan inserts (sbm_occ_insert_cloud*,
 *  sbm_occ_insert_rays*, their _discrete forms, with and without the bounding box and change detection: each touched voxel gets
 *  its one update, occupied before free) and the UPDATE items of the edit batches, where a voxel's items take effect in item
 *  order: the voxel's stamp after the batch is the clock if any UPDATE item passed the early-return test at its turn, else the
 *  stamp it had. setNodeValue (SBM_OCC_EDIT_SET) never stamps, and a voxel it creates has stamp 0. A deleted voxel goes with its
 *  stamp: created again, also inside ONE edit batch, it starts from stamp 0.
 *  Carry. Growth and the deletes' move carry the word with the key; sbm_occ_reset and every loader (.bt, .ot) leave stamp 0
 *  everywhere (octomap's streams carry no stamps: OcTreeNodeStamped does not override writeData / readData). The clock stays.
 *  sbm_occ_stamp_degrade is degradeOutdatedNodes(time_thres): every voxel with logodds >= the occupancy threshold and
 *  (uint32)(clock - stamp) > time_thres gets one miss update, clamped (integrateMissNoTime: v + miss, then below clamp min ->
 *  clamp min, above clamp max -> clamp max). The subtraction wraps in 32 bits as octomap's unsigned int does: a clock below a
 *  stamp makes a huge age. The stamp is untouched and change detection is untouched. One lane per slot, plain stores.
 *  sbm_occ_stamp_forget is an extension, not octomap: every voxel with (uint32)(clock - stamp) > time_thres is deleted, whatever
 *  its value, through the delete family's move into a fresh table; its counts are those of a delete (sbm_occ_last_edit). In
 *  octomap's terms: a leaf loop that collects those keys, then deleteNode of each.
 *  Device. The stamp is a template switch of the scan's APPLY and of the edit's APPLY (one device function each, instantiated as
 *  the kernel a map without stamps launches, unchanged in name, arguments and registers, and as a stamped kernel that takes the
 *  words and the clock as two more arguments; the host picks beside kBox / kTrack): a plain vector store by the
 *  lane that owns the slot (a slot is in the touched list once, and a run has one walker), no atomics on stamp words. On a
 *  stamped map the scan's MARK always notes "created this scan", which the early-return test needs.
 *  DIVERGENCE, pruning during inserts: as for colour, a stamp belongs to ONE depth-16 voxel; the recordings drive octomap with
 *  lazy_eval = true, so that it never prunes while it inserts (pruneNode would smear stamps through copyData).
 *  The tree. sbm_occ_tree_build over a map that holds stamp words builds octomap's STAMPED pruned tree, in both readings:
 *  OcTreeNodeStamped's operator== compares value AND stamp, so isNodeCollapsible is "all eight present, all leaves, equal value,
 *  equal stamp", applied bottom-up: eight siblings of equal value and equal stamps are 16 nodes and 1 leaf, with one stamp
 *  different 24 nodes and 8 leaves. The pruned tree of a stamped map is therefore NOT the plain tree's wherever such stamps
 *  differ: node counts, leaf order and the .bt and .ot bytes follow the stamped structure. A collapsed node has its children's
 *  common stamp (copyData); every other inner node has the map's clock at build time (updateInnerOccupancy()); the root's stamp
 *  is getLastUpdateTime() (sbm_occ_stamp_root). The stamp is gathered per voxel by key and the test is a template switch of the
 *  level kernel; all other tree calls (info, search, leaves, the .bt body, the planner calls, sbm_occ_ot_body_device) work on that
 *  structure unchanged. sbm_occ_stamp_leaves* is sbm_occ_tree_leaves* with the stamp of every entry, in the same order. A snapshot
 *  of a map without stamps is built exactly as before, and its entries answer stamp 0.
 *  The stream. AbstractOcTree::write with `id OcTreeStamped`: OcTreeNodeStamped does not override writeData, so the records are
 *  the plain five bytes per node, over the stamped structure, under the other id line; sbm_occ_stamp_ot_info / _leaves / _load /
 *  _read are the plain .ot parsers (on the device for the load) with the other id test, and a tree read back has stamp 0
 *  everywhere. sbm_occ_ot_* and sbm_occ_color_ot_* keep refusing `id OcTreeStamped`, sbm_occ_stamp_ot_* refuse every other id; a
 *  refused stream leaves the map as it was. writeBinary of an OcTreeStamped names the class in its header too; sbm_occ_tree_
 *  write_binary writes `id OcTree` over the same body. integrateNodeColor, insertPointCloudRays and getNormals stay out as before.
 *  sbm_get_profile: no new names. The degrade is timed under "occ_rays_apply", as the edits' APPLY is; the forget as a delete; the
 *  search under "occ_search", the fetch under "occ_fetch" (DESIGN.md section 30). */
/* Allocates the stamp words of a log-odds map, zeroed; a second call does nothing. SBM_ERR_NULL; SBM_ERR_UNSUPPORTED for a hit
 * map and for a map that holds colour words; SBM_ERR_NOMEM where the words cannot be allocated: the map is as it was. */
int sbm_occ_stamp_enable(sbm_occ_map* map);
/* *enabled: 1 if the map holds stamp words, else 0. SBM_ERR_NULL. Host only. */
int sbm_occ_stamp_enabled(const sbm_occ_map* map, int* enabled);
/* The map's clock: set, and read back. SBM_ERR_NULL. Host only: no launch, and they work whether stamps are enabled or not. */
int sbm_occ_stamp_set_time(sbm_occ_map* map, uint32_t clock);
int sbm_occ_stamp_time(const sbm_occ_map* map, uint32_t* clock);
/* degradeOutdatedNodes(time_thres) with the miss, the clamps and the occupancy threshold of params. *degraded: how many voxels
 * got the miss update. Synchronous. Checked in this order before anything is launched: SBM_ERR_NULL; the codes of
 * sbm_occ_ray_params_validate; SBM_ERR_UNSUPPORTED for a map without stamps. */
int sbm_occ_stamp_degrade(sbm_occ_map* map, uint32_t time_thres, const sbm_occ_ray_params* params, uint64_t* degraded);
/* Deletes every voxel with (uint32)(clock - stamp) > time_thres. removed (may be NULL): how many. Synchronous. SBM_ERR_NULL;
 * SBM_ERR_UNSUPPORTED for a map without stamps; SBM_ERR_NOMEM where the move's table cannot be allocated: the map is as it was. */
int sbm_occ_stamp_forget(sbm_occ_map* map, uint32_t time_thres, uint64_t* removed);
/* sbm_occ_search_device with the stamp: d_stamp n uint32 (may be NULL, as d_value may). An unknown voxel and a point outside
 * the key space answer stamp 0 and the quiet NaN 0x7FC00000. Read-only; it allocates nothing. The checks are
 * sbm_occ_search_device's, and SBM_ERR_UNSUPPORTED on a hit map. */
int sbm_occ_stamp_search_device(sbm_occ_map* map, size_t n, const void* d_xyz, float occupancy_thres_log, void* d_state, void* d_value,
                                void* d_stamp, int sync);
/* The same on HOST memory. Synchronous. */
int sbm_occ_stamp_search(sbm_occ_map* map, size_t n, const float* xyz, float occupancy_thres_log, int32_t* state, void* value,
                         uint32_t* stamp);
/* sbm_occ_fetch_logodds_device with the stamps, through the map's radix sort: the voxels in ascending order of their packed keys,
 * d_logodds and d_stamps cap 4-byte words each (either may be NULL). Same cap / *count / SBM_ERR_SIZE / SBM_ERR_OCC_FULL rule.
 * Read-only. */
int sbm_occ_stamp_fetch_device(sbm_occ_map* map, void* d_keys, void* d_logodds, void* d_stamps, size_t cap, size_t* count);
int sbm_occ_stamp_fetch(sbm_occ_map* map, uint64_t* keys, float* logodds, uint32_t* stamps, size_t cap, size_t* count);
/* sbm_occ_tree_leaves_device with d_stamp, cap uint32 in DEVICE memory, 4-byte aligned (NULL: exactly that call): the stamp of
 * every entry, in the same order. Same entries, order, checks and cap / *count rule. 0 for every entry of a snapshot of a map
 * without stamps. Synchronous. */
int sbm_occ_stamp_leaves_device(sbm_occ_tree* tree, int max_depth, void* d_keys, void* d_depth, void* d_value, void* d_stamp, size_t cap,
                                size_t* count);
/* The same on HOST memory; value may be NULL, stamp not. */
int sbm_occ_stamp_leaves(sbm_occ_tree* tree, int max_depth, uint64_t* keys, int32_t* depth, float* value, uint32_t* stamp, size_t cap,
                         size_t* count);
/* getLastUpdateTime(): the root's stamp, 0 for a snapshot without stamps or without a voxel. SBM_ERR_NULL. Synchronous. */
int sbm_occ_stamp_root(sbm_occ_tree* tree, uint32_t* stamp);
/* tree.write(path) of an OcTreeStamped: the .ot header with `id OcTreeStamped`, then the plain body (sbm_occ_ot_body_device) of
 * the stamped snapshot. The codes of sbm_occ_ot_write; SBM_ERR_UNSUPPORTED for a snapshot of a map without stamps. */
int sbm_occ_stamp_ot_write(sbm_occ_tree* tree, const char* path);
/* sbm_occ_ot_info / _leaves / _load / _read for a stream whose id is OcTreeStamped: the same parsers (on the device for the load),
 * the same codes; any other id, a plain OcTree among them, is SBM_ERR_UNSUPPORTED, and a refused stream leaves the map as it
 * was. The loaded map has stamp 0 everywhere. */
int sbm_occ_stamp_ot_info(const void* bytes, size_t n, sbm_occ_ot_header* out);
int sbm_occ_stamp_ot_leaves(const void* bytes, size_t n, uint64_t* first_key, int32_t* depth, float* value, size_t cap, size_t* count);
int sbm_occ_stamp_ot_load(sbm_occ_map* map, const void* bytes, size_t n, int sync);
int sbm_occ_stamp_ot_read(sbm_occ_map* map, const char* path, int sync);

/* ---- visual-word dictionary: addNewWords, computeLikelihood, limitKeypoints ---------------------------------------------------
 * The reference's loop-closure thread, started by Mapper::process for each key frame: addWordIds -> VWDictionary::addNewWords
 * (src/slam/src/core/Mapper.cpp:413-484, VWDictionary.cpp:40-115) and detectLoopClosure -> computeLikelihood
 * (Mapper.cpp:536-677). The only stage whose cost grows with the run: up to 750 descriptors per key frame are searched against
 * a dictionary that gains up to 750 words per key frame.
 *  EXACT WHERE THE REFERENCE APPROXIMATES. The reference searches with FLANN, four randomised kd-trees and 32 checks; the answer
 *  depends on its random trees and is not reproduced. The search here is exhaustive: every query is compared with every word.
 *  That is the answer FLANN's converges to as its checks grow. No comparison against FLANN is made.
 *  addNewWords(descriptors, nodeId), as defined here:
 *   1 all n rows are searched, 2-NN, against the dictionary as it was BEFORE the call; words added by earlier rows of the same
 *     call are not seen by later rows;
 *   2 row i is unique if fewer than two neighbours came back, or if (float)d0 > nndr * (float)d1 -- one float multiply, one float
 *     compare, not contracted;
 *   3 a unique row becomes a new word; its id is the next integer, counting from 0, in row order (the id is the word's index in
 *     the store); it gets one reference (nodeId, 1);
 *   4 a row that is not unique calls addRef(nodeId) on its nearest word: that word's count for this node is incremented, or
 *     (nodeId, 1) inserted;
 *   5 the word id of every row is returned, in row order.
 *  The metric. FlannIndex builds flann::Index<flann::L1<float>> over the bytes converted to float and searches through a pointer
 *  cast to Index<L2<float>> (FlannIndex.cpp:51,92); the object that answers is the L1 one. SBM_VWD_L1, the default, is the sum of
 *  absolute byte differences (<= 8160); SBM_VWD_L2 is the sum of squared byte differences (<= 2 080 800). Both are exact in float;
 *  they are computed in integers and converted once for the NNDR test.
 *  Defined where the reference is not: neighbours are ordered by (distance, dictionary index), so of two equally distant words
 *  the older one ranks first and a row that is not unique goes to that word; a dictionary of one word gives every row fewer
 *  than two neighbours, so every row is unique (the reference reads an unset index there); node_id < 1 is an invalid value
 *  (SBM_ERR_UNSUPPORTED): the reference's VisualWord constructor silently adds no reference for node 0.
 *  Store. sbm_vwd is created from a handle with a fixed capacity in words (1 .. 2^26) and uses that handle's stream, scratch and
 *  stage clock; it must be destroyed before the handle and serves one thread at a time. Device state: 32 bytes and one squared
 *  norm per word, the size, a counter of refused calls. A call whose new words would pass the capacity adds NOTHING (no word, no
 *  reference, no node), returns SBM_ERR_VWD_FULL and raises sbm_vwd_overflow by one. Host state: per word its references
 *  (node -> count), per node its word ids in row order and ni, its keypoint count including the ones cut by the limit
 *  (n_keypoints_total >= n). Calls that name the same node again extend its word list and add to its ni.
 *  Kernels. Search: one wavefront per (64-query tile, dictionary slice); slices = params.slices, or with 0 as many as give the
 *  launch about 4096 wavefronts; slice s covers words [s * R, (s + 1) * R) with R = 64 * ceil(ceil(N / 64) / slices), and empty
 *  slices are dropped. Decide: merges the slices in dictionary order and takes the uniqueness decision. Append: a prefix scan
 *  over the unique flags in row order places row i at size + rank. Searches read rows < size, the append writes rows >= size.
 *  2-NN record: four int32 (i0, d0, i1, d1), i = -1 and d = SBM_VWD_NONE where there is no such neighbour.
 *  computeLikelihood, reproduced as written: the distinct word ids of the query node are walked in ascending order; ids <= 0 are
 *  skipped (the very first word, id 0; the reference's negative ids of cut keypoints never reach the store and count only in
 *  ni); logNnw = log10f(N / nw), N = (float)n_nodes the caller's total node count, nw the number of nodes that reference the
 *  word; a zero logNnw is skipped; for each referencing node that is in the candidate list, score += (nwi * logNnw) / ni in
 *  float, nwi that node's count, ni its keypoint count. The best hypothesis is the first strictly greatest score walking the
 *  candidates in ascending id order, among ids > 0, starting from (0, 0.0f) (detectLoopClosure, Mapper.cpp:568-573).
 *  limitKeypoints (SensorData.cpp:109-133): when max > 0 and n > max, keep the max highest fabs(response); among equal
 *  responses the HIGHER index wins (reverse iteration of a multimap, which keeps insertion order among equal keys). Otherwise
 *  every keypoint is kept.
 *  sbm_get_profile: while profiling is enabled (any mode) searches and additions synchronise and record "vwd_search",
 *  "vwd_append" (decide + append) and "vwd_total" (their float sum), ms of the last call. */
enum { SBM_VWD_L1 = 0, SBM_VWD_L2 = 1 };
#define SBM_VWD_NONE 2147483647
typedef struct sbm_vwd_params {
  int32_t metric;  /* SBM_VWD_L1 (what the reference's index answers with) or SBM_VWD_L2                   */
  float nndr;      /* nndrRatio 0.8f; in (0, 1]                                                            */
  int32_t slices;  /* dictionary slices per query tile, 0 = automatic; 0 .. 65 535                         */
} sbm_vwd_params;
typedef struct sbm_vwd sbm_vwd; /* opaque */

/* The reference's constants: L1, 0.8f, automatic slices. */
void sbm_vwd_params_default(sbm_vwd_params* p);
/* SBM_ERR_NULL; SBM_ERR_UNSUPPORTED for an unknown metric, an nndr that is NaN, <= 0 or > 1, or slices outside 0 .. 65 535. */
int sbm_vwd_params_validate(const sbm_vwd_params* p);
/* An empty dictionary for up to `capacity` words on the handle's device. The codes of sbm_vwd_params_validate; SBM_ERR_SIZE for
 * capacity 0, SBM_ERR_UNSUPPORTED above 2^26, both before anything is allocated; *out is NULL on failure. */
int sbm_vwd_create(sbm_handle* h, size_t capacity, const sbm_vwd_params* p, sbm_vwd** out);
void sbm_vwd_destroy(sbm_vwd* vwd);
/* Forget every word, reference and node (and the overflow count); the store is kept. */
int sbm_vwd_reset(sbm_vwd* vwd);
int sbm_vwd_size(sbm_vwd* vwd, size_t* size);
/* Calls refused so far because their new words did not fit. */
int sbm_vwd_overflow(sbm_vwd* vwd, uint64_t* overflow);
/* addNewWords on n rows of 32 bytes in DEVICE memory, dense, in the layout sbm_orb_describe_device writes (a frame's rows;
 * 16-byte aligned, SBM_ERR_UNSUPPORTED otherwise). word_ids (host, n ints, may be NULL) receives the word id of every row.
 * n 0 .. 65 535 and n_keypoints_total >= n (SBM_ERR_SIZE), node_id >= 1 (SBM_ERR_UNSUPPORTED). Synchronous: the ids come back
 * to the host, which keeps the references. SBM_ERR_VWD_FULL as above. */
int sbm_vwd_add_words_device(sbm_vwd* vwd, const void* d_desc, int n, int node_id, int n_keypoints_total, int* word_ids);
/* The same on host rows, `stride` bytes apart (>= 32). */
int sbm_vwd_add_words(sbm_vwd* vwd, const uint8_t* desc, size_t stride, int n, int node_id, int n_keypoints_total, int* word_ids);
/* The 2-NN records of n device rows against the dictionary as it is, nothing added: d_knn receives n records (16-byte aligned). */
int sbm_vwd_search_device(sbm_vwd* vwd, const void* d_desc, int n, void* d_knn, int sync);
/* Words first .. first + count - 1 of the store, 32 bytes each, into host memory; SBM_ERR_SIZE beyond the size. */
int sbm_vwd_fetch_words(sbm_vwd* vwd, size_t first, size_t count, uint8_t* rows);
/* The references of one word, ascending by node: *count pairs into nodes / counts (cap entries each; SBM_ERR_SIZE with *count
 * set when cap is too small, or for a word id outside the dictionary). */
int sbm_vwd_references(sbm_vwd* vwd, int word_id, int* nodes, int* counts, int cap, int* count);
/* computeLikelihood of node_id against n candidate node ids (any order; a repeated id is one candidate) with n_nodes the
 * caller's total node count: scores[i] is candidates[i]'s score; *best_id / *best_score the highest hypothesis, (0, 0.0f) when
 * none is positive. Host code. SBM_ERR_UNSUPPORTED for node_id < 1, SBM_ERR_SIZE for a node the dictionary has not seen or a
 * negative n or n_nodes. */
int sbm_vwd_likelihood(sbm_vwd* vwd, int node_id, const int* candidates, int n, int n_nodes, float* scores, int* best_id,
                       float* best_score);
/* limitKeypoints: keep_flags[i] = 1 for the keypoints kept, else 0. Pure host code, no handle. SBM_ERR_NULL, SBM_ERR_SIZE
 * (n < 0), SBM_ERR_UNSUPPORTED for a NaN response (the reference's multimap has no order for it). */
int sbm_vwd_limit_keypoints(const float* responses, int n, int max, uint8_t* keep_flags);

/* ---- pose-graph optimiser: runOptimize, runOptimizeRobust ------------------------------------------------------------------------
 * The reference's last stage between its motion estimates and its map (main.cpp:328, Optimizer.cpp, HyperGraph.cpp,
 * GraphEdge.cpp, GraphVertex.cpp, g2o/SE3Gradient.cpp, getConnectedGraph of Mapper.cpp:195-255): Levenberg-Marquardt over SE3-SE3
 * edges. All device arithmetic is fp64 and nothing is contracted. tests/pgo_cases.py restates every step in numpy;
 * tests/golden/pgo_reference.npz records what the reference's own code computes (tools/make_pgo_fixtures.py).
 *  Vertices are ordered by ascending id; that order, the fixed vertex left out, is the Hessian index. One vertex is fixed
 *  (fixed_id, the reference's 1). Poses and measurements are 3 x 4 row-major doubles; the float-to-double conversion of addVertices
 *  is the caller's. Edges are taken in the caller's order, which is the reference's multimap order (keyed by `from`).
 *  Error. delta = (Z^-1 Xi^-1) Xj; e = (delta's translation, the vector part of Quaternion(R) normalised and negated when w < 0),
 *  Quaternion(R) being Eigen's conversion with its trace-positive and its largest-diagonal branch; chi2 = e^T O e.
 *  Jacobians. computeEdgeSE3Gradient as written, with A = Z^-1, B = Xi^-1 Xj, E = A B and dq/dR through S = 2 sqrt(tr + 1),
 *  qw = S / 4, 1 / pow(qw, 3). That form is singular at a 180 degree error and is not repaired.
 *  Quadratic form. b receives Jn^T(-O e) for each free end, the diagonal blocks Jn^T O Jn; there is ONE off-diagonal block, at
 *  (row to, column from), inserted only when `from` is free.
 *  coupling. SBM_PGO_COUPLING_REFERENCE (default): SimplicialLDLT reads the lower triangle only, so an edge whose `to` has the
 *  SMALLER Hessian index keeps its diagonal blocks and its b but couples nothing -- the reference's loop closures are
 *  Link(new id, old id), so this is its usual case. SBM_PGO_COUPLING_SYMMETRIC: every edge between two free vertices couples
 *  them; what a caller who wants a correct optimiser passes. The recording shows the first reading.
 *  Initial lambda. lambda0 = tau * max_diag, tau = 1e-5; constructQuadraticForm resets max_diag to 0 for EVERY edge, so max_diag
 *  is the largest absolute diagonal entry of the LAST edge's free blocks, not of the matrix. Restated on purpose; reorder the edges
 *  and lambda0 changes.
 *  Iteration. Solve (A + lambda I) x = b, oplus on every free vertex, lambda *= scaleLambda: scale = sum x (lambda x + b) + 1e-3,
 *  rho = (chi2 before - chi2 after) / scale, alpha = 1 - (2 rho - 1)^3 clamped to [1/3, 2/3]. There is no step rejection: a step
 *  that raises chi2 is kept. oplus: fromCompactQuaternion returns the identity rotation when 1 - |v|^2 < 0 (the translation still
 *  applies), else Quaternion(sqrt(w), v).toRotationMatrix(); estimate = estimate * increment.
 *  sbm_pgo_optimize = runOptimize: num iterations, then computeActiveErrors; poses come back in ascending id order.
 *  sbm_pgo_optimize_robust = runOptimizeRobust, the loop on the host: 1 getConnectedGraph(fixed_id) as written (the largest pending
 *  id first, poses propagated through forward or inverted links, unique links kept, unreached vertices drop out); 2 five
 *  iterations on the device, then the per-edge chi2; 3 among edges with |id1 - id2| != 1 and chi2 >= 10 the strictly greatest (the
 *  first in link order among equals); 4 none: runOptimize(num) from the RE-PROPAGATED poses, not from the five-iteration result,
 *  and stop; 5 else every link with that (from, to) is removed, and again. The removed links are reported in order.
 *  Defined where the reference is not: where `to` is the fixed vertex and `from` is free the reference forms a negative triplet
 *  index; here that coupling is dropped, the mathematically right answer. The reference erases links while iterating over them;
 *  here "every link with that (from, to)". Propagation in getConnectedGraph is in double, pose[to] = pose[cur] * T or * T^-1,
 *  without the float quaternion renormalisation of Transform::operator*; the caller's float map rounds at the end.
 *  Elimination. Exact, not iterative. A free vertex is a JUNCTION when it touches a coupling between Hessian indices that are not
 *  neighbours, or is promoted so that no stretch is longer than run_max; the stretches between junctions are RUNS, block
 *  tridiagonal and independent. Every run is eliminated by block Thomas (16 lanes per run, one right-hand column each: b, 6 towards
 *  the left junction, 6 towards the right); the Schur complement on the junctions is dense, factorised by block Cholesky, and
 *  substituted back. One step of iterative refinement follows: the residual b - (A + lambda I) x is accumulated in twice the
 *  working precision and solved against the same factors, and the correction is added to x. More than 1024 junctions
 *  (plan.max_junctions) is SBM_ERR_UNSUPPORTED. No atomics anywhere: a result does not depend on scheduling.
 *  Not guarded: a 6 x 6 pivot that is not positive -- from the singular dq/dR near 180 degrees, or from an information matrix
 *  that is not positive definite, which sbm_pgo_params_check does not test -- makes sqrt return NaN; the call then returns
 *  SBM_OK with NaN in *err and in the poses. The reference's LDLT goes on in the same situation (it logs a warning).
 *  sbm_pgo_params_check: SBM_ERR_NULL for a null pointer; SBM_ERR_SIZE for num < 0, an empty graph (no vertex), a vertex id given
 *  twice, an absent fixed_id, an edge naming an absent vertex; SBM_ERR_UNSUPPORTED for from == to, a non-finite pose, measurement
 *  or information matrix, an unknown coupling, run_max outside 1 .. 65 536. No free vertices is SBM_OK with the poses unchanged.
 *  sbm_get_profile: while profiling is enabled the LAST iteration of a call records "pgo_linearise", "pgo_assemble", "pgo_solve",
 *  "pgo_update" and "pgo_total" (their float sum), ms. */
enum { SBM_PGO_COUPLING_REFERENCE = 0, SBM_PGO_COUPLING_SYMMETRIC = 1 };
enum { SBM_PGO_DEBUG_EDGES = 0, SBM_PGO_DEBUG_DIAG = 1, SBM_PGO_DEBUG_OFFDIAG = 2, SBM_PGO_DEBUG_B = 3, SBM_PGO_DEBUG_X = 4 };
#define SBM_PGO_EDGE_RECORD 200 /* doubles per edge: e 6, chi2 1, pad 1, Ji 36, Jj 36, Ji^T O Ji 36, Jj^T O Jj 36, Ji^T O Jj 36, bi 6, bj 6 */
typedef struct sbm_pgo_params {
  int32_t num;       /* iterations of the final runOptimize; the reference passes 20; >= 0          */
  int32_t fixed_id;  /* the vertex that stays; the reference fixes id 1                                */
  int32_t coupling;  /* SBM_PGO_COUPLING_REFERENCE or SBM_PGO_COUPLING_SYMMETRIC                      */
  int32_t run_max;   /* the longest run of the elimination, 1 .. 65 536; default 64                   */
} sbm_pgo_params;
typedef struct sbm_pgo_graph {
  int32_t n_vertices;
  const int32_t* ids;    /* n_vertices distinct ids, any order                                         */
  const double* poses;   /* n_vertices x 12                                                            */
  int32_t n_edges;
  const int32_t* from;   /* n_edges vertex ids                                                         */
  const int32_t* to;
  const double* meas;    /* n_edges x 12                                                               */
  const double* info;    /* n_edges x 36, row-major                                                    */
} sbm_pgo_graph;
typedef struct sbm_pgo_plan_info {
  int32_t n_free, n_runs, n_junctions, schur_size /* 6 * n_junctions */, n_coupling /* edges with an off-diagonal block */,
      longest_run, n_slots /* distinct coupled vertex pairs */, max_junctions;
} sbm_pgo_plan_info;

/* The reference's constants: 20 iterations, vertex 1 fixed, the lower-triangle reading, runs of up to 64. */
void sbm_pgo_params_default(sbm_pgo_params* p);
int sbm_pgo_params_check(const sbm_pgo_params* p, const sbm_pgo_graph* g);
/* The partition, computed on the host without a device. vertex_run (n_free ints, may be NULL): per Hessian index its run, or -1
 * for a junction. slot_rc (2 * n_slots ints, may be NULL; size it 2 * n_edges): (row, column) Hessian indices of every coupled
 * pair, row > column, in the order of SBM_PGO_DEBUG_OFFDIAG. edge_couples (n_edges bytes, may be NULL). The codes of
 * sbm_pgo_params_check; SBM_ERR_UNSUPPORTED with everything filled in when the junctions pass max_junctions. */
int sbm_pgo_plan(const sbm_pgo_params* p, const sbm_pgo_graph* g, sbm_pgo_plan_info* info, int32_t* vertex_run, int32_t* slot_rc,
                 uint8_t* edge_couples);
/* runOptimize on host arrays: poses_out (n_vertices x 12, ascending id order), *err the final chi2. Synchronous. */
int sbm_pgo_optimize(sbm_handle* h, const sbm_pgo_params* p, const sbm_pgo_graph* g, double* poses_out, double* err);
/* runOptimizeRobust: *n_out vertices were reached; ids_out / poses_out (room for n_vertices) in ascending id order; removed
 * receives up to removed_cap (from, to) pairs, *n_removed how many links were dropped. */
int sbm_pgo_optimize_robust(sbm_handle* h, const sbm_pgo_params* p, const sbm_pgo_graph* g, int32_t* n_out, int32_t* ids_out,
                            double* poses_out, double* err, int32_t* removed, int32_t removed_cap, int32_t* n_removed);
/* The device forms: g->poses, g->meas and g->info are DEVICE memory (same layouts, poses in the order of g->ids), d_poses_out
 * device memory for n_vertices x 12 doubles (ascending id order); ids, from and to stay host memory, since the partition is
 * host code. The work runs on the handle's stream, which the call synchronises before it returns (chi2 comes home every
 * iteration). Ids and topology are checked as in sbm_pgo_params_check; the values on the device are not read by the host, so
 * non-finite ones are not refused. The results equal the host forms' bit for bit. The robust device form brings poses and
 * measurements home once, because getConnectedGraph propagates on the host, and runs the host form. */
int sbm_pgo_optimize_device(sbm_handle* h, const sbm_pgo_params* p, const sbm_pgo_graph* g, void* d_poses_out, double* err);
int sbm_pgo_optimize_robust_device(sbm_handle* h, const sbm_pgo_params* p, const sbm_pgo_graph* g, int32_t* n_out, int32_t* ids_out,
                                   void* d_poses_out, double* err, int32_t* removed, int32_t removed_cap, int32_t* n_removed);
/* What the last optimisation on this handle launched: its partition, the lambda of its last iteration, its iteration count. */
int sbm_pgo_last_plan(sbm_handle* h, sbm_pgo_plan_info* info, double* lambda, int32_t* iterations);
/* The last iteration of the last optimisation (meant after a call of one iteration): SBM_PGO_DEBUG_EDGES n_edges records of
 * SBM_PGO_EDGE_RECORD doubles; _DIAG n_free diagonal blocks of A (36 doubles, row-major; the lower triangle is what is read);
 * _OFFDIAG n_slots lower blocks; _B and _X n_free x 6. SBM_ERR_SIZE when dst_bytes is too small, SBM_ERR_UNSUPPORTED before a
 * call. */
int sbm_pgo_debug_fetch(sbm_handle* h, int which, void* dst, size_t dst_bytes);

/* The raw HIP stream (hipStream_t) as void*, so callers can order their own work behind ours (record an event on it
 * after sbm_compute_device(..., sync = 0)) or ours behind theirs (hipStreamWaitEvent on it before the call). Every entry
 * point selects the handle's device for the duration of the call and restores the caller's current device on return. */
void* sbm_stream(sbm_handle* h);

const char* sbm_strerror(int code);
int sbm_last_hip_error(const sbm_handle* h); /* hipError_t of the last failing runtime call, else 0 */
int sbm_version(void);                        /* major * 1000 + minor */

#ifdef __cplusplus
}
#endif
#endif /* SBM_H_ */
