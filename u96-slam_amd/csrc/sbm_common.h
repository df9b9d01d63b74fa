// sbm_common.h -- shared declarations of the HIP stereo block-matching engine (internal, gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sbm.h"
#include "sbm_carve.h"

#include <stdlib.h>

namespace sbm {

// Environment switches of the library -- the complete list, documented for integrators in include/sbm.h ("Environment").
// They select a tested fallback or a code path that the GPU tests compare with the default one: SBM_FAST_INPLACE (0: the
// sliding-sum kernel in place of the interior one), SBM_FAST_PFSHIFT, SBM_FAST_CS3, SBM_FAST_HANDOFF, SBM_FAST_FOLD, SBM_FAST_NBR, SBM_SPECKLE_LISTS, SBM_SPECKLE_BAND,
// SBM_SPECKLE_SEG, SBM_HOST_ZEROCOPY, SBM_WIDE, SBM_CV_READING, SBM_OCC_OT_HOST_PARSE.
inline int env_switch(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// Geometry of one launch, derived on the host from sbm_params and the image size. Naming follows
// cv::StereoBM (calib3d stereobm.cpp): lofs/rofs/width1, buffer index d <-> true disparity nd-1-d+mindisp.
struct Geom {
  int W, H;            // image size
  int n;               // pairs in the batch
  int pitch;           // byte pitch of the padded prefiltered planes
  int padl;            // bytes of left padding in front of column 0 of a prefiltered row
  int plane;           // bytes per prefiltered plane (pitch * H)
  int nd, mindisp, wsz, w2, cap;
  int lofs, rofs, width1, xend;  // xend = min(width1, W - lofs): computed columns are X = lofs + x, x in [0,xend)
  int tex, uniq;
  int filtered;        // (mindisp - 1) * 16
  int row0, row1;      // valid-ROI rows [row0,row1)
  int col0, col1;      // valid-ROI columns [col0,col1)
  int want_cost;       // disp12_max_diff >= 0
  int cost16;          // the cost plane holds uint16 (fast + border kernels: sums <= 65534) instead of int32
  int pfshift;         // the prefiltered planes hold (value << pfshift) + 1 (0 unless the fast path asks for it)
  int reading;         // SBM_CV_READING: alternative readings of cv::StereoBM behaviours nobody could pin (kRead* bits; 0 = default)
};

// The bits of SBM_CV_READING (include/sbm.h): every behaviour of cv::StereoBM that this engine restates from
// memory and that the reference's data cannot pin has its alternative reading behind one bit here AND in the CPU oracle
// (sbmo_set_reading), so that the day somebody runs tools/verify_with_opencv.py the fix is a default flip.
constexpr int kReadRoiMinusMinD = 1;      // getValidDisparityROI: xmax = min(roi1 right edge, roi2 right edge - minDisparity) - w/2 (2.4 lineage)
constexpr int kReadCostShort = 2;         // validateDisparity sees the block-matching cost plane as `short` (wraps beyond 32767)
constexpr int kReadSpeckleX16 = 4;        // filterSpeckles receives speckleRange * 16 (StereoSGBM's convention)
constexpr int kReadOddRowComputed = 8;    // prefilterXSobel: the last row of an odd-height image is computed, not filled with cap
constexpr int kReadLrTieLater = 16;       // validateDisparity: on equal cost the LATER x takes the slot

// Prefiltered planes store value+1 (range 1..2*cap+1 <= 127) so that 0 can act as the "masked byte" of
// v_mqsad_pk_u16_u8; padding bytes are 0. sbm_debug_fetch() removes the bias again.
// With Geom::pfshift = 2 the planes store 4*value+1 (<= 253): every absolute difference, hence every SAD, is a multiple
// of 4, which leaves the two low bits of the packed 16-bit sums free for a register tag in the interior kernel's
// winner search (sbm_sad_fast.hip; chosen by sad_fast_pfshift() when 4*maxS still fits 16 bits; pfshift = 1: 2*value+1,
// one tag bit, where only 2*maxS fits). The tag is carried by the sums themselves: one lane of every window starts its
// vertical accumulators at the tag (FastTag, sbm_sad_fast_core.h). The border wavefronts of the same launch work on the scaled sums too; only the
// uniqueness threshold and the stored cost go back to the unscaled sum.
constexpr int kPfBias = 1;

hipError_t launch_prefilter(const uint8_t* d_left, const uint8_t* d_right, uint8_t* pf_l, uint8_t* pf_r,
                            const Geom& g, hipStream_t s);

// PREFILTER_NORMALIZED_RESPONSE (cv prefilterNorm); vsum = 2*n*W*H uint16 scratch (column sums).
hipError_t launch_prefilter_norm(const uint8_t* d_left, const uint8_t* d_right, uint8_t* pf_l, uint8_t* pf_r, uint16_t* vsum,
                                 const Geom& g, int winsize, hipStream_t s);

// Generic SAD/WTA for output columns x in [xa,xb) (x relative to lofs) and rows [row0,row1): any block size,
// any disparity count, clamped border windows. Used for the border columns and as the fallback path.
hipError_t launch_sad_generic(const uint8_t* pf_l, const uint8_t* pf_r, int16_t* disp, int32_t* cost, const Geom& g,
                              int xa, int xb, hipStream_t s);

// The same definition and outputs with sliding sums in both directions (sbm_sad_wide.hip): the fallback outside the fast
// envelope for up to 2048 disparities; SBM_WIDE=0 selects the per-column kernel above instead.
bool sad_wide_supported(const Geom& g);
hipError_t launch_sad_wide(const uint8_t* pf_l, const uint8_t* pf_r, int16_t* disp, int32_t* cost, const Geom& g, int xa, int xb,
                           hipStream_t s);

// The plan of one sbm_compute_device call: everything the host decides before it launches anything, as plain data (no pointers,
// no HIP types, no constructors), computed once per call by bm_plan() without a HIP call. The launchers execute it and recompute
// nothing. sbm_debug_plan() (sbm_api.hip; not in include/sbm.h) copies it out as it stands, so the layout below IS that export's:
// int32 words in declaration order (Geom's 26 first), the four scratch sizes as int64 (two words each, 8-byte aligned), the name
// last. tests/test_bm_plan.py mirrors it with ctypes; the export refuses a mirror of another size.
enum SadKernel { kSadNone = 0, kSadFast = 1, kSadWide = 2, kSadGeneric = 3 };
struct FastPlan {            // the interior kernel's launch (sad_fast_plan, sbm_sad_fast.hip); zero unless BmPlan::fast
  int xc0, xc1;              // interior centre columns [xc0,xc1) (relative to lofs); xc0 = w/2
  int strips, strips3, nseg; // as FastArgs (sbm_sad_fast_core.h)
  int segrow[66];
  int split;                 // the disparities are spread over more, narrower wavefronts (launch_nd)
  int uniq_plain;
  int NDW, NWAVES, NTERM, PW, exact, dual;   // the instantiation sad_fast_kernel<NDW, NWAVES, NTERM, PW, exact, dual>
  int bord, bnw, bseg, nbseg;                // the border jobs of the same launch, as FastArgs
  int grid, block, lds;      // 1-D grid, threads per workgroup, dynamic LDS bytes
};
struct SpkPlan {             // the speckle filter's launches (speckle_plan, sbm_speckle.hip)
  int lists;                 // band walk + record-driven kernels (else the four row-walking kernels; G, S, SW, nbands are 0 then)
  int G, S, SW, nbands;      // rows per band, column segments per band and their width, bands per image
  int max_diff;              // the effective maxDiff
  int grid[4][2];            // x, y of the four launches in stream order (band / seam / count / apply, or runs / merge / count / apply)
};
struct BmPlan {
  Geom g;
  int any_rows;              // there is something to match (else every stage but the LR fill is skipped)
  int in_envelope;           // any_rows and sad_fast_supported(): the call the in-place self-test is run for
  int fast;                  // in_envelope and the in-place accumulate is available: the interior kernel runs
  int border;                // the clamped border columns ride in the interior launch (visible, and up to 256 disparities)
  int speckle;
  int sad;                   // SadKernel
  int wide_borders;          // beyond 256 disparities: the visible border columns [wide_l) and [wide_r) from launch_sad_wide
  int wide_l[2], wide_r[2];
  FastPlan f;
  SpkPlan spk;
  int spk_pad_;              // (keeps spk_bytes 8-byte aligned)
  long long spk_bytes[4];    // SpeckleScratch::bytes: runs, nheads, seam, nseam (0 without the speckle filter)
  char kernel[96];           // the SAD kernel's name as sbm_last_kernel_name reports it ("" when nothing is matched)
};
// Status codes of sbm_compute_device behind its null and batch checks, in its order; Geom, any_rows and in_envelope.
int bm_plan_geom(const sbm_params& p, int n, int W, int H, BmPlan* pl);
// The rest, once the result of mqsad_inplace_ok is known (it is only asked for calls in the envelope).
void bm_plan_launches(const sbm_params& p, bool inplace_ok, BmPlan* pl);
inline int bm_plan(const sbm_params& p, int n, int W, int H, bool inplace_ok, BmPlan* pl) {
  const int st = bm_plan_geom(p, n, W, H, pl);
  if (st == SBM_OK) bm_plan_launches(p, inplace_ok, pl);
  return st;
}

// Fast path (interior columns, odd block sizes 5..31, up to 512 disparities, 16-bit sums: sad_fast_supported()).
bool sad_fast_supported(const Geom& g);
// device self-test behind the in-place v_mqsad accumulate, on stream s: *ok once it ran (cached per device); a HIP error when it
// could not run (nothing cached)
hipError_t mqsad_inplace_ok(hipStream_t s, bool* ok);
constexpr int kFastNdMax = 512;   // disparities the interior kernel takes (four cooperating 128-disparity wavefronts)
bool sad_fast_borders_in_launch(const Geom& g);   // the clamped border columns ride in the interior launch (up to 256 disparities)
int sad_fast_pfshift(const Geom& g);   // 2 or 1 when the interior kernel wants pre-scaled planes (see kPfBias), else 0
// pl->f and the kernel's name for a call with pl->fast (g, border set): strips, row segments, layout, border jobs, grid and LDS
void sad_fast_plan(BmPlan* pl);
// Columns of the launch's last strip if it runs folded over its disparity halves (sbm_sad_fast_fold.h), else 0: a function of
// the plan and SBM_FAST_FOLD alone.
int sad_fast_fold_cols(const BmPlan& pl);
// The planned launch. With pl.border the w/2 clamped columns on each side of [xc0,xc1) are computed by extra wavefronts of the
// same launch (sbm_sad_border_wave.h); without it the launch leaves them untouched.
// handoff / epoch / links: the scratch through which a row segment leaves its vertical sums to the next one (sad_fast_handoff_bytes()
// of it, the first *flag_bytes zero or written by earlier launches with smaller epochs; 0 bytes: this call hands nothing over),
// this launch's number, and how many (segment, pair, strip) may take their sums over.
size_t sad_fast_handoff_bytes(const BmPlan& pl, size_t* flag_bytes);
hipError_t launch_sad_fast(const uint8_t* pf_l, const uint8_t* pf_r, int16_t* disp, int32_t* cost, BmPlan& pl, void* handoff,
                           unsigned epoch, long* links, hipStream_t s);

// Left-right consistency (cv validateDisparity) + invalid rows/columns fill. Reads disp_pre/cost, writes disp_out.
// Rows wider than kLrLdsCols keep their claim table in global memory: keys = n * H * W 64-bit words (lr_keys_bytes; null
// when the LR check is off or every row fits LDS).
constexpr int kLrLdsCols = 8192;   // 8 B per column: 64 KiB of LDS, the most a kernel gets without asking
inline size_t lr_keys_bytes(int n, int W, int H, bool do_lr) {
  return do_lr && W > kLrLdsCols ? (size_t)n * H * W * sizeof(unsigned long long) : 0;
}
hipError_t launch_lrcheck(const int16_t* disp_pre, const int32_t* cost, int16_t* disp_out, unsigned long long* keys,
                          const Geom& g, int disp12_max_diff, hipStream_t s);
// The kernel launch_lrcheck picks (host only; sbm_debug_postfilter reports it): the fill alone when the check is off, lrcheck16_kernel
// <nit, px> in blocks of bs threads, or the generic kernel with its claim table in LDS or in global memory (nit, px, bs are 0 then).
enum LrKernel { kLrCopy = 0, kLrFast16 = 1, kLrGenericLds = 2, kLrGenericGlobal = 3 };
struct LrChoice { int kernel, nit, px, bs; };
LrChoice lr_choice(const Geom& g, int disp12_max_diff);

// Speckle filter: launch_speckle and its scratch are in sbm_handle.h.
constexpr int kSpkMaxSeg = 4, kSpkRecordPad = 288, kSpkSeamPad = 512;
// The filter's launches for n maps of W x H (g.n, g.W, g.H; g.reading), cv's maxSpeckleSize and maxDiff.
void speckle_plan(const Geom& g, int max_size, int max_diff, SpkPlan* k);

// Stand-alone prefilter of dense images (either flavour) and the rectifier in front of it (sbm_rectify.hip).
hipError_t launch_prefilter_dense(const uint8_t* d_src, uint8_t* d_dst, int n, int W, int H, int rtl, int cap,
                                  hipStream_t s);
hipError_t launch_rect_map(const sbm_rect_cam& cam, int W, int H, int16_t* d_map, hipStream_t s);
hipError_t launch_rect_remap(const uint8_t* d_src, const int16_t* d_map, uint8_t* d_dst, int n, int W, int H,
                             hipStream_t s);

// GFTT minimum-eigenvalue map of the PL (sbm_gftt.hip): eig = n*H*W uint16, maxv = n uint32 (`Max` register per image).
hipError_t launch_gftt_eig(const uint8_t* img, uint16_t* eig, unsigned* maxv, int n, int W, int H, hipStream_t s);

// Consumers of the map (sbm_consume.hip): decimation, reprojection, keypoint depth.
hipError_t launch_disp_to_float(const int16_t* disp, float* out, size_t count, hipStream_t s);
hipError_t launch_decimate(const int16_t* disp, int16_t* out, int n, int W, int H, int scale, hipStream_t s);
hipError_t launch_reproject(const int16_t* disp, float* xyz, int n, int W, int H, int scale, const sbm_stereo_model& m,
                            int apply_local, hipStream_t s);
hipError_t launch_keypoints3d(const int16_t* disp, const float* kp, float* xyz, int W, int H, int nk,
                              const sbm_stereo_model& m, float min_depth, float max_depth, hipStream_t s);
// The sparse branch of the same function: disparity = left.x - right.x under the status mask, n frames of cap slots each.
hipError_t launch_keypoints3d_lk(const float* kp, const float* rp, const uint8_t* status, const int* count, int n, int cap,
                                 const sbm_stereo_model& m, float min_depth, float max_depth, float* xyz, hipStream_t s);

// Semi-global matcher (sbm_sgbm.hip). Naming follows cv::StereoSGBM (calib3d stereosgbm.cpp): computable columns
// X = minX1 + x, x in [0, W1); buffer index d <-> disparity minD + d; P1, P2, d12 and uniq are the effective values.
// C, S, hsum: n * H * W1 * D int16 ([pair][y][x][d]).
struct SgbmGeom {
  int W, H, n;
  int minD, D, minX1, maxX1, W1;
  int SW2, P1, P2, ftzero, uniq, d12;
  int fullDP;          // MODE_HH: 8 paths
  int reading;
};

}  // namespace sbm
