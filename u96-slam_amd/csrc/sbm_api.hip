// sbm_api.hip -- C-ABI of libsbm_hip.so (declared in include/sbm.h): parameters, the handle's life and its pool, the block
// matcher on device buffers, profiling and debug dispatch, and the thin rectify / prefilter / consumer entry points. The other
// families' entry points sit with their kernels (sbm_fpga, sbm_sgbm, sbm_gftt, sbm_gftt_select, sbm_orb, sbm_match, sbm_pnp, sbm_lk, sbm_occupancy and sbm_occ_*); the block
// matcher's host-buffer paths are in sbm_host.hip. Replaces cv::StereoBM::compute at src/slam/src/core/main.cpp:201-216.
//
// Stage order (same as cv::StereoBM::compute): prefilter both images -> SAD/WTA on the valid-ROI rows
// (fast kernel: interior columns + the clamped border columns as extra wavefronts of the same launch; generic kernel otherwise) -> LR check + invalid
// row/column fill -> speckle filter.  Everything is enqueued on the handle's stream; no host sync inside.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>

#include "sbm_handle.h"

using namespace sbm;

// The block matcher's stages as sbm_get_profile names them, and the marks sbm_compute_device records into one slot of the
// handle's ring. "border" is never timed and reads 0: up to 256 disparities the clamped columns ride in the SAD launch.
enum BmStage { kBmPrefilter, kBmSad, kBmBorder, kBmLr, kBmSpeckle, kBmTotal, kBmStageCount };
enum BmMark { kBmBegin, kBmPrefiltered, kBmMatched, kBmChecked, kBmEnd, kBmMarkCount };
static const char* const kBmNames[] = {"prefilter", "sad", "border", "lrcheck", "speckle", "total"};
StageTable sbm::bm_stages() { return stage_table<kBmStageCount, 0>(kBmNames); }   // no marks of the clock's own: the ring has them
static_assert(kBmMarkCount == sbm_handle::kMarks, "the ring holds one event per mark");

extern "C" {

void sbm_params_default(sbm_params* p, int num_disparities, int block_size) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->prefilter_type = SBM_PREFILTER_XSOBEL;
  p->prefilter_size = 9;
  p->prefilter_cap = 31;
  p->block_size = block_size > 0 ? block_size : 21;
  p->min_disparity = 0;
  p->num_disparities = num_disparities > 0 ? num_disparities : 64;
  p->texture_threshold = 10;
  p->uniqueness_ratio = 15;
  p->speckle_window_size = 0;
  p->speckle_range = 0;
  p->disp12_max_diff = -1;
}

int sbm_params_validate(const sbm_params* p, int width, int height) {
  if (!p) return SBM_ERR_NULL;
  if (width <= 0 || height <= 0) return SBM_ERR_SIZE;
  if (p->prefilter_type != SBM_PREFILTER_NORMALIZED_RESPONSE && p->prefilter_type != SBM_PREFILTER_XSOBEL)
    return SBM_ERR_PREFILTER_TYPE;
  if (p->prefilter_size < 5 || p->prefilter_size > 255 || p->prefilter_size % 2 == 0) return SBM_ERR_PREFILTER_SIZE;
  if (p->prefilter_cap < 1 || p->prefilter_cap > 63) return SBM_ERR_PREFILTER_CAP;
  if (p->block_size < 5 || p->block_size > 255 || p->block_size % 2 == 0 || p->block_size >= std::min(width, height))
    return SBM_ERR_BLOCK_SIZE;
  if (p->num_disparities <= 0 || p->num_disparities % 16 != 0) return SBM_ERR_NUM_DISPARITIES;
  if (p->texture_threshold < 0) return SBM_ERR_TEXTURE;
  if (p->uniqueness_ratio < 0) return SBM_ERR_UNIQUENESS;
  return SBM_OK;
}

const char* sbm_strerror(int code) {
  switch (code) {
    case SBM_OK: return "ok";
    case SBM_ERR_NULL: return "null argument";
    case SBM_ERR_SIZE: return "bad image size or stride (all the images must have the same size)";
    case SBM_ERR_PREFILTER_TYPE: return "preFilterType must be PREFILTER_NORMALIZED_RESPONSE or PREFILTER_XSOBEL";
    case SBM_ERR_PREFILTER_SIZE: return "preFilterSize must be odd and be within 5..255";
    case SBM_ERR_PREFILTER_CAP: return "preFilterCap must be within 1..63";
    case SBM_ERR_BLOCK_SIZE: return "SADWindowSize must be odd, be within 5..255 and be not larger than image width or height";
    case SBM_ERR_NUM_DISPARITIES: return "numDisparities must be positive and divisible by 16";
    case SBM_ERR_TEXTURE: return "texture threshold must be non-negative";
    case SBM_ERR_UNIQUENESS: return "uniqueness ratio must be non-negative";
    case SBM_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU backend)";
    case SBM_ERR_HIP: return "HIP runtime error (see sbm_last_hip_error)";
    case SBM_ERR_NOMEM: return "out of memory";
    case SBM_ERR_UNSUPPORTED: return "configuration outside this build's limits";
    case SBM_ERR_BATCH: return "batch count must be positive";
    case SBM_ERR_OCC_FULL: return "occupancy map full: points were counted as overflow, not stored (see sbm_occ_overflow)";
    case SBM_ERR_VWD_FULL: return "visual-word dictionary full: the call's new words did not fit and nothing was added (see sbm_vwd_overflow)";
    default: return "unknown status";
  }
}

int sbm_version(void) { return SBM_VERSION_MAJOR * 1000 + SBM_VERSION_MINOR; }

// Every device buffer and pinned staging buffer of the handle; streams and events stay.
static void free_buffers(sbm_handle* h) {
  h->each_set([](auto& s) { release_all(s); });
  // What goes with some sets' buffers (releasing those again is a no-op). bm, fp and fq are keyed on their shape and lose the key
  // too. fq, the asynchronous feed's sets, may have submissions outstanding while a synchronous host entry point resizes ITS
  // staging: free_staging leaves them alone, and only the feed's own realloc path (drained first) and this function free them.
  release_set(h->bm); release_set(h->fp); release_set(h->fq);
  free_staging(h);   // the host entry points' staging: its key, and the pinned host memory that mirrors it
  h->sg.have_last = false;   // nothing of the last semi-global call is left for sbm_debug_fetch
}

// The reference re-creates its matcher for every frame (cv::StereoBM::create inside the loop, main.cpp:201). Streams,
// ~400 events and the device scratch make a cold handle cost ~2 ms -- ten times the frame itself -- so destroyed handles
// are parked (a few, with at most kPoolScratch bytes of scratch each) and sbm_create re-arms one for the same device.
static std::mutex g_pool_mu;
static constexpr int kPool = 4;
static constexpr size_t kPoolScratch = (size_t)512 << 20;
static sbm_handle* g_pool[kPool];
static int g_pool_n = 0;

static size_t scratch_bytes(sbm_handle* h) {
  size_t n = h->pin_bytes;
  h->each_set([&](auto& s) { n += bytes_held(s); });
  return n;
}

// Stage times: every family's, the block matcher's among them, start at zero.
static void reset_profile(sbm_handle* h, int enabled) {
  h->profiling = enabled;
  h->calls = h->ncall = 0;
  h->instr = false;
  h->each_clock([](StageClock& c, const StageTable&) { c.reset(); });
}

static void destroy_now(sbm_handle* h);

void sbm_trim(void) {
  std::lock_guard<std::mutex> lock(g_pool_mu);
  for (int i = 0; i < g_pool_n; i++) destroy_now(g_pool[i]);
  g_pool_n = 0;
}

int sbm_create(sbm_handle** out, const sbm_params* p, int device) {
  if (!out || !p) return SBM_ERR_NULL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return SBM_ERR_NO_DEVICE;
  {
    std::lock_guard<std::mutex> lock(g_pool_mu);
    for (int i = 0; i < g_pool_n; i++)
      if (g_pool[i]->device == device) {
        sbm_handle* h = g_pool[i];
        g_pool[i] = g_pool[--g_pool_n];
        h->p = *p;
        h->last_hip = 0;
        h->have_last = h->sg.have_last = false;
        reset_profile(h, 0);
        *out = h;
        return SBM_OK;
      }
  }
  sbm_handle* h = new (std::nothrow) sbm_handle();
  if (!h) return SBM_ERR_NOMEM;
  memset(h, 0, sizeof(*h));
  h->p = *p;
  h->device = device;
  DeviceScope dscope(device);
  if (dscope.enter() != hipSuccess) {
    delete h;
    return SBM_ERR_NO_DEVICE;
  }
  // every failure below goes through destroy_now(), which tolerates the members that were never created (null)
  bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess;
  if (!ok) {
    destroy_now(h);
    return SBM_ERR_HIP;
  }
  h->ev_ok = true;
  for (int r = 0; r < sbm_handle::kRing; r++)
    for (int i = 0; i < sbm_handle::kMarks; i++) h->ev_ok &= hipEventCreate(&h->ev[r][i]) == hipSuccess;
  *out = h;
  return SBM_OK;
}

static void sync_all_streams(sbm_handle* h) {
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->stream_in) hipStreamSynchronize(h->stream_in);
  if (h->stream_out) hipStreamSynchronize(h->stream_out);
}

void sbm_destroy(sbm_handle* h) {
  if (!h) return;
  DeviceScope dscope(h->device);
  dscope.enter();
  // submissions of the asynchronous feed nobody waited for: the copies that are already queued finish (their destination
  // must still exist, as for any submission that has not been waited for); the newest submission's maps, whose trip home is
  // only queued by a wait or by the next submission, are DROPPED -- destroy never starts a write into caller memory
  h->fq_pending_dst = nullptr;
  h->fq_waited = h->fq_submitted;
  sync_all_streams(h);
  {
    std::lock_guard<std::mutex> lock(g_pool_mu);
    if (g_pool_n < kPool) {
      if (scratch_bytes(h) > kPoolScratch) {
        free_buffers(h);
      }
      g_pool[g_pool_n++] = h;
      return;
    }
  }
  destroy_now(h);
}

// Frees whatever the handle owns; members that were never created are null (the handle is zero-initialised), so this is
// also the failure path of sbm_create. Restores the caller's current device.
static void destroy_now(sbm_handle* h) {
  DeviceScope dscope(h->device);
  dscope.enter();
  sync_all_streams(h);
  free_buffers(h);
  h->each_clock([](StageClock& c, const StageTable&) { c.release(); });
  for (int r = 0; r < sbm_handle::kRing; r++)
    for (int i = 0; i < sbm_handle::kMarks; i++)
      if (h->ev[r][i]) hipEventDestroy(h->ev[r][i]);
  for (int i = 0; i < sbm_handle::kChunks; i++) {
    if (h->ev_in[i]) hipEventDestroy(h->ev_in[i]);
    if (h->ev_done[i]) hipEventDestroy(h->ev_done[i]);
  }
  for (int k = 0; k < 4; k++) {
    if (h->ev_fq_in[k]) hipEventDestroy(h->ev_fq_in[k]);
    if (h->ev_fq_done[k]) hipEventDestroy(h->ev_fq_done[k]);
    if (h->ev_fq_out[k]) hipEventDestroy(h->ev_fq_out[k]);
  }
  if (h->stream_in) hipStreamDestroy(h->stream_in);
  if (h->stream_out) hipStreamDestroy(h->stream_out);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
}

int sbm_set_params(sbm_handle* h, const sbm_params* p) {
  if (!h || !p) return SBM_ERR_NULL;
  h->p = *p;
  return SBM_OK;
}

int sbm_get_params(const sbm_handle* h, sbm_params* p) {
  if (!h || !p) return SBM_ERR_NULL;
  *p = h->p;
  return SBM_OK;
}

void* sbm_stream(sbm_handle* h) { return h ? (void*)h->stream : nullptr; }
int sbm_last_hip_error(const sbm_handle* h) { return h ? h->last_hip : 0; }

int sbm_synchronize(sbm_handle* h) {
  if (!h) return SBM_ERR_NULL;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  while (h->fq_waited != h->fq_submitted) {   // submissions of the asynchronous feed count as pending work too
    const int st = sbm_wait_oldest(h);
    if (st != SBM_OK) return st;
  }
  return SBM_OK;
}

int sbm_set_profiling(sbm_handle* h, int enabled) {
  if (!h) return SBM_ERR_NULL;
  reset_profile(h, enabled);
  return SBM_OK;
}

}  // extern "C"

// cv getValidDisparityROI (calib3d stereosgbm.cpp) with cv::StereoBM's "empty rect = whole image" substitution.
static void valid_roi(const sbm_params& p, int W, int H, int reading, int roi[4]) {
  int full[4] = {0, 0, W, H};
  const int* r1 = (p.roi1[2] > 0 && p.roi1[3] > 0) ? p.roi1 : full;
  const int* r2 = (p.roi2[2] > 0 && p.roi2[3] > 0) ? p.roi2 : full;
  const int sw2 = p.block_size / 2, maxd = p.min_disparity + p.num_disparities - 1;
  const int xmin = std::max(r1[0], r2[0] + maxd) + sw2;
  const int xmax = std::min(r1[0] + r1[2], r2[0] + r2[2] - ((reading & kReadRoiMinusMinD) ? p.min_disparity : 0)) - sw2;
  const int ymin = std::max(r1[1], r2[1]) + sw2;
  const int ymax = std::min(r1[1] + r1[3], r2[1] + r2[3]) - sw2;
  if (xmax - xmin > 0 && ymax - ymin > 0) {
    roi[0] = xmin; roi[1] = ymin; roi[2] = xmax - xmin; roi[3] = ymax - ymin;
  } else {
    roi[0] = roi[1] = roi[2] = roi[3] = 0;
  }
}

int sbm::bm_plan_geom(const sbm_params& p, int n, int width, int height, BmPlan* pl) {
  const int st = sbm_params_validate(&p, width, height);
  if (st != SBM_OK) return st;
  if (n > 32767 || height > 65535) return SBM_ERR_UNSUPPORTED;
  if (p.num_disparities > 4096) return SBM_ERR_UNSUPPORTED;
  memset(pl, 0, sizeof(*pl));
  Geom& g = pl->g;
  g.W = width; g.H = height; g.n = n;
  g.nd = p.num_disparities; g.mindisp = p.min_disparity; g.wsz = p.block_size; g.w2 = p.block_size / 2;
  g.cap = p.prefilter_cap; g.tex = p.texture_threshold; g.uniq = p.uniqueness_ratio;
  g.filtered = (p.min_disparity - 1) * 16;
  g.lofs = std::max(g.nd - 1 + g.mindisp, 0);
  g.rofs = -std::min(g.nd - 1 + g.mindisp, 0);
  g.width1 = width - g.rofs - g.nd + 1;
  g.xend = std::min(g.width1, width - g.lofs);
  g.want_cost = p.disp12_max_diff >= 0;
  // padded prefiltered planes: the fast kernel stages 16-byte pieces that may start up to nd+64 bytes left of
  // column 0 and end up to 96 bytes right of column W-1
  g.padl = ((g.nd + 64 + 63) / 64) * 64;
  g.pitch = ((g.padl + width + 128 + 63) / 64) * 64;
  g.plane = g.pitch * height;

  int roi[4];
  g.reading = env_switch("SBM_CV_READING", 0);
  valid_roi(p, width, height, g.reading, roi);
  g.row0 = std::max(roi[1], 0); g.row1 = std::min(roi[1] + roi[3], height);
  g.col0 = std::max(std::min(roi[0], width), 0); g.col1 = std::max(std::min(roi[0] + roi[2], width), 0);
  const bool range_fits = !(g.lofs >= width || g.rofs >= width || g.width1 < 1);
  pl->any_rows = range_fits && roi[2] > 0 && roi[3] > 0 && g.row1 > g.row0;
  if (!pl->any_rows) { g.row0 = g.row1 = 0; }
  pl->in_envelope = pl->any_rows && sad_fast_supported(g);
  return SBM_OK;
}

void sbm::bm_plan_launches(const sbm_params& p, bool inplace_ok, BmPlan* pl) {
  Geom& g = pl->g;
  pl->fast = pl->in_envelope && inplace_ok;
  if (pl->fast) {
    // 16-bit cost plane when every producer is a 16-bit-sum kernel (fast interior + border kernels, w/2 clamped columns on
    // each side); the generic kernel needs int32
    g.cost16 = 1;
    g.pfshift = sad_fast_pfshift(g);   // pre-scaled planes for the interior kernel's tagged winner search
    const int xhi = std::min(g.W - g.lofs - 1, g.W - g.rofs - g.nd);
    const int fa = g.w2, fb = xhi - g.w2 + 1;   // the interior range the launch covers; xend - fb == w/2 by construction
    // columns left and right of the fast range: clamped windows. They only matter if they can influence the output:
    // through the LR check or when inside the valid ROI.
    const bool borders_visible = g.want_cost || g.col0 < g.lofs + fa || g.col1 > g.lofs + fb;
    // ... and then they ride in the interior launch as extra wavefronts (sbm_sad_border_wave.h): one SAD launch, one stream;
    // beyond 256 disparities they come from the sliding-sum kernel in launches of their own
    pl->border = borders_visible && sad_fast_borders_in_launch(g);
    pl->wide_borders = borders_visible && !pl->border;
    pl->sad = kSadFast;
    sad_fast_plan(pl);
    if (pl->wide_borders) { pl->wide_l[0] = 0; pl->wide_l[1] = pl->f.xc0; pl->wide_r[0] = pl->f.xc1; pl->wide_r[1] = g.xend; }
  } else if (pl->any_rows) {
    // (say so when the interior kernel was left out only because the in-place accumulate is off or its device self-test
    // failed: 8-25x slower, see include/sbm.h)
    const bool wide = sad_wide_supported(g) && env_switch("SBM_WIDE", 1);
    pl->sad = wide ? kSadWide : kSadGeneric;
    snprintf(pl->kernel, sizeof(pl->kernel), "%s",
             !wide ? "sad_generic_kernel" : (pl->in_envelope ? "sad_wide_kernel [in-place accumulate unavailable]" : "sad_wide_kernel"));
  }
  pl->speckle = p.speckle_range >= 0 && p.speckle_window_size > 0;
  if (pl->speckle) {
    speckle_plan(g, p.speckle_window_size, p.speckle_range, &pl->spk);
    size_t part[4];
    SpeckleScratch::bytes(g.n, g.W, g.H, part);
    for (int i = 0; i < 4; i++) pl->spk_bytes[i] = (long long)part[i];
  }
}

extern "C" {

// ho_bytes / ho_flags: sad_fast_handoff_bytes() of the call's plan (0: nothing is handed over)
static int ensure_scratch(sbm_handle* h, int n, int W, int H, int pitch, bool need_cost, bool need_speckle, size_t ho_bytes,
                          size_t ho_flags) {
  auto& s = h->bm;
  const bool fits = n <= s.n && W == s.W && H == s.H && pitch == s.pitch && s.pf_l.p;
  if (!fits) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    release_set(s);
    const size_t npix = (size_t)n * W * H, pfbytes = (size_t)n * pitch * H + 4096;
    HIPCHK(h, s.pf_l.grow(pfbytes, h->stream));
    HIPCHK(h, s.pf_r.grow(pfbytes, h->stream));
    HIPCHK(h, s.disp_pre.grow(npix * sizeof(int16_t), h->stream));
    // padding bytes must read as 0 (the masked value of the fast kernel); the prefilter never writes them
    HIPCHK(h, hipMemsetAsync(s.pf_l.p, 0, pfbytes, h->stream));
    HIPCHK(h, hipMemsetAsync(s.pf_r.p, 0, pfbytes, h->stream));
    s.n = n; s.W = W; s.H = H; s.pitch = pitch;
  }
  const size_t npix = (size_t)s.n * W * H;
  if (need_cost) HIPCHK(h, s.cost.grow(npix * sizeof(int32_t), h->stream));
  HIPCHK(h, s.lr_keys.grow(lr_keys_bytes(s.n, W, H, need_cost), h->stream));
  if (need_speckle) HIPCHK(h, s.spk.ensure(s.n, W, H, h->stream));
  if (ho_bytes) {
    // The flag words in front of the slots must never hold a number a later launch will use: they are cleared when the buffer is
    // new, when another plan moves the boundary between flags and slots, and when the launch counter wraps.
    const bool fresh = ho_bytes > s.handoff.bytes;
    HIPCHK(h, s.handoff.grow(ho_bytes, h->stream));
    if (fresh || ho_flags != s.ho_flags || s.ho_epoch == 0xffffffffu) {
      HIPCHK(h, hipMemsetAsync(s.handoff.p, 0, ho_flags, h->stream));
      s.ho_flags = ho_flags;
      s.ho_epoch = 0;
    }
  }
  return SBM_OK;
}

static inline void mark(sbm_handle* h, BmMark i) {
  if (h->instr) hipEventRecord(h->ev[h->calls % sbm_handle::kRing][i], h->stream);
}

// mode 2: average stage times over the recorded calls (at most the last kRing); mode 1: the last call only.
// The stream must be idle.
static void collect_profile(sbm_handle* h) {
  unsigned nrec = std::min<unsigned>(h->calls, sbm_handle::kRing), first = 0;
  if (h->profiling == 1 && h->calls > 0) { first = (h->calls - 1) % sbm_handle::kRing; nrec = 1; }
  static const BmStage kStage[kBmMarkCount - 1] = {kBmPrefilter, kBmSad, kBmLr, kBmSpeckle};   // stage i: from mark i to mark i + 1
  float acc[kBmMarkCount - 1] = {}, tot = 0.f;
  for (unsigned r = first; r < first + nrec; r++) {
    for (int i = 0; i < kBmMarkCount - 1; i++) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, h->ev[r][i], h->ev[r][i + 1]) == hipSuccess) acc[i] += ms;
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev[r][kBmBegin], h->ev[r][kBmEnd]) == hipSuccess) tot += ms;
  }
  const float inv = nrec ? 1.f / nrec : 0.f;
  for (int i = 0; i < kBmMarkCount - 1; i++) h->bm.clock.ms[kStage[i]] = acc[i] * inv;
  h->bm.clock.ms[kBmTotal] = tot * inv;
}

// The tail of a call, behind the SAD kernels: LR check + valid-ROI fill from disp_pre / cost into out (stages & 1), then the
// speckle filter on out where the plan has one (stages & 2). sbm_compute_device runs both; sbm_debug_postfilter runs the same
// code on a caller's map.
static int post_filters(sbm_handle* h, const BmPlan& pl, const int16_t* disp_pre, const int32_t* cost, int16_t* out, int stages) {
  const sbm_params& p = h->p;
  if (stages & 1) {
    HIPCHK(h, launch_lrcheck(disp_pre, cost, out, h->bm.lr_keys.as<unsigned long long>(), pl.g, p.disp12_max_diff, h->stream));
    mark(h, kBmChecked);
  }
  if ((stages & 2) && pl.speckle) HIPCHK(h, launch_speckle(out, h->bm.spk, pl.g, pl.spk, p.speckle_window_size, h->stream));
  return SBM_OK;
}

int sbm_compute_device(sbm_handle* h, int n, const void* d_left, const void* d_right, int width, int height,
                       void* d_disp, int sync) {
  if (!h || !d_left || !d_right || !d_disp) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  const sbm_params& p = h->p;
  BmPlan pl;
  const int st = bm_plan_geom(p, n, width, height, &pl);
  if (st != SBM_OK) return st;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  // The interior kernel needs the in-place v_mqsad accumulate: its device self-test runs on this handle's stream, once per
  // device (a check that could not run fails this call with its HIP error and runs again on the next one). Without it the
  // sliding-sum kernel takes the whole envelope.
  bool inplace = false;
  if (pl.in_envelope) HIPCHK(h, mqsad_inplace_ok(h->stream, &inplace));
  bm_plan_launches(p, inplace, &pl);
  const Geom& g = pl.g;
  size_t ho_flags = 0;
  const size_t ho_bytes = sad_fast_handoff_bytes(pl, &ho_flags);
  const int st2 = ensure_scratch(h, n, width, height, g.pitch, g.want_cost, pl.speckle, ho_bytes, ho_flags);
  if (st2 != SBM_OK) return st2;
  h->last = g; h->have_last = true;
  h->bm.ho_links = 0;
  if (pl.any_rows) snprintf(h->last_kernel, sizeof(h->last_kernel), "%s", pl.kernel);

  // Stages run one after the other on the main stream. Overlapping LR + speckle of one sub-batch with the SAD kernel of
  // the next was built and measured in round 2 (profiles/r02_subbatch_pipeline.md; the code is in the history at commit
  // "Engine: device guard ..."): 1.47 ms -> 1.54 / 1.73 ms with 2 / 4 sub-batches, because four 126-VGPR wavefronts per
  // SIMD leave no registers for a guest wavefront -- the post-filters only overlap once the SAD kernel runs at 3
  // wavefronts per SIMD, which costs it 27 %.
  const uint8_t* dl = (const uint8_t*)d_left;
  const uint8_t* dr = (const uint8_t*)d_right;
  uint8_t *pf_l = h->bm.pf_l.as<uint8_t>(), *pf_r = h->bm.pf_r.as<uint8_t>();
  int16_t* disp_pre = h->bm.disp_pre.as<int16_t>();
  int32_t* cost = h->bm.cost.as<int32_t>();
  int16_t* out = (int16_t*)d_disp;

  h->instr = h->profiling && h->ev_ok && (h->profiling != 3 || (h->ncall & 3u) == 0);
  mark(h, kBmBegin);
  if (pl.any_rows) {
    if (p.prefilter_type == SBM_PREFILTER_XSOBEL) {
      HIPCHK(h, launch_prefilter(dl, dr, pf_l, pf_r, g, h->stream));
    } else {
      HIPCHK(h, h->bm.vsum.grow((size_t)2 * h->bm.n * width * height * sizeof(uint16_t), h->stream));
      HIPCHK(h, launch_prefilter_norm(dl, dr, pf_l, pf_r, h->bm.vsum.as<uint16_t>(), g, p.prefilter_size, h->stream));
    }
  }
  mark(h, kBmPrefiltered);
  if (pl.sad == kSadFast) {
    HIPCHK(h, launch_sad_fast(pf_l, pf_r, disp_pre, cost, pl, ho_bytes ? h->bm.handoff.p : nullptr, ho_bytes ? ++h->bm.ho_epoch : 0u,
                              &h->bm.ho_links, h->stream));
    h->bm.ho_slots = (size_t)h->bm.ho_links;   // one slot per (linked segment, pair, strip)
    if (pl.wide_borders) {   // beyond 256 disparities: the clamped columns from the sliding-sum kernel
      HIPCHK(h, launch_sad_wide(pf_l, pf_r, disp_pre, cost, g, pl.wide_l[0], pl.wide_l[1], h->stream));
      HIPCHK(h, launch_sad_wide(pf_l, pf_r, disp_pre, cost, g, pl.wide_r[0], pl.wide_r[1], h->stream));
    }
  } else if (pl.sad == kSadWide) {
    HIPCHK(h, launch_sad_wide(pf_l, pf_r, disp_pre, cost, g, 0, g.xend, h->stream));
  } else if (pl.sad == kSadGeneric) {
    HIPCHK(h, launch_sad_generic(pf_l, pf_r, disp_pre, cost, g, 0, g.xend, h->stream));
  }
  mark(h, kBmMatched);
  const int st3 = post_filters(h, pl, disp_pre, cost, out, 3);
  if (st3 != SBM_OK) return st3;
  mark(h, kBmEnd);
  if (h->instr) h->calls++;
  h->ncall++;
  if (sync || h->profiling == 1) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

// The plan of a call as sbm_compute_device would compute it for these parameters, given the in-place self-test's result: a copy
// of BmPlan (sbm_common.h has the layout). No handle, no device. Not part of the public header: for the tests.
int sbm_debug_plan(const sbm_params* p, int n, int width, int height, int inplace_ok, void* out, size_t out_bytes) {
  if (!p || !out) return SBM_ERR_NULL;
  if (out_bytes != sizeof(BmPlan)) return SBM_ERR_SIZE;
  if (n <= 0) return SBM_ERR_BATCH;
  BmPlan pl;
  const int st = bm_plan(*p, n, width, height, inplace_ok != 0, &pl);
  if (st == SBM_OK) memcpy(out, &pl, sizeof(pl));
  return st;
}

// The hand-off scratch of that plan under the current SBM_FAST_HANDOFF: out[0] = sad_fast_handoff_bytes() (0: the call hands nothing
// over), out[1] = the flag words in front of the slots. As sbm_debug_plan: for the tests, not part of the public header.
int sbm_debug_handoff_bytes(const sbm_params* p, int n, int width, int height, int inplace_ok, uint64_t* out) {
  if (!p || !out) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  BmPlan pl;
  const int st = bm_plan(*p, n, width, height, inplace_ok != 0, &pl);
  if (st != SBM_OK) return st;
  size_t flags = 0;
  out[0] = sad_fast_handoff_bytes(pl, &flags);
  out[1] = flags;
  return SBM_OK;
}

// Whether that plan's last strip runs folded over its disparity halves under the current SBM_FAST_FOLD: out[0] = its columns
// (sad_fast_fold_cols; 0: it does not fold). As sbm_debug_plan: for the tests, not part of the public header.
int sbm_debug_fold(const sbm_params* p, int n, int width, int height, int inplace_ok, int* out) {
  if (!p || !out) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  BmPlan pl;
  const int st = bm_plan(*p, n, width, height, inplace_ok != 0, &pl);
  if (st != SBM_OK) return st;
  out[0] = sad_fast_fold_cols(pl);
  return SBM_OK;
}

// The post-filters of sbm_compute_device on a caller's map: the call is planned as sbm_compute_device plans it for the handle's
// parameters and n maps of width x height (same environment switches, same self-test, same scratch), the prefilter and the SAD
// kernels are skipped, disp_pre / cost (host, n * height * width each) take the place of what they would have left in the handle's
// planes, and post_filters() runs: stages 1 = LR check + valid-ROI fill, 2 = speckle filter, 3 = both; disp (host) receives the
// map. With stages == 2 the map goes to the filter as it is and every pixel of it counts (no ROI fill); the handle's parameters
// must switch the filter on, and the block size is not held against the image then (the filter reads no window), so maps of
// fewer rows than the smallest block can be filtered.
// The input must be what the SAD kernels produce (SBM_ERR_UNSUPPORTED otherwise; lrcheck16_kernel's inner wavefronts test no range):
// a pixel is (minDisparity - 1) * 16 or within [minDisparity * 16, (minDisparity + numDisparities - 1) * 16]; costs are
// non-negative, and where the plan's cost plane is 16 bits (Geom::cost16) at most 65534 at valid pixels -- the int32 costs are
// narrowed and every filtered pixel gets 0xffff, as the SAD kernels store it. cost may be null when nothing reads it (stages == 2,
// disp12MaxDiff < 0).
// info (info_count >= kPostInfoCount int32) says what ran: [0] stages, [1] LrKernel or -1, [2] nit, [3] px, [4] block size, [5] cost16,
// [6] the speckle filter ran, [7] SpkPlan::lists, [8] G, [9] S, [10] SW, [11] max_diff, [12..15] row0, row1, col0, col1 of the valid
// ROI, [16] lofs, [17] xend. As sbm_debug_plan: for the tests, not part of the public header.
constexpr size_t kPostInfoCount = 18;
int sbm_debug_postfilter(sbm_handle* h, int n, int width, int height, const int16_t* disp_pre, const int32_t* cost, int stages,
                         int16_t* disp, int32_t* info, size_t info_count) {
  if (!disp_pre || !disp || !info) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (width <= 0 || height <= 0) return SBM_ERR_SIZE;
  if (info_count < kPostInfoCount) return SBM_ERR_SIZE;
  if (stages < 1 || stages > 3) return SBM_ERR_UNSUPPORTED;
  if (!h) return SBM_ERR_NULL;   // (last of the argument checks: the others can be tested without a device)
  const sbm_params& p = h->p;
  BmPlan pl;
  int st = bm_plan_geom(p, n, width, height, &pl);
  if (st == SBM_ERR_BLOCK_SIZE && stages == 2 && n <= 32767 && height <= 65535) {
    sbm_params q = p;
    q.block_size = 5;
    if (sbm_params_validate(&q, 64, 64) == SBM_OK && p.num_disparities <= 4096) {   // nothing but the block against the image
      memset(&pl, 0, sizeof(pl));
      pl.g.W = width; pl.g.H = height; pl.g.n = n;
      pl.g.nd = p.num_disparities; pl.g.mindisp = p.min_disparity; pl.g.filtered = (p.min_disparity - 1) * 16;
      pl.g.reading = env_switch("SBM_CV_READING", 0);
      st = SBM_OK;
    }
  }
  if (st != SBM_OK) return st;
  const bool lr_reads_cost = (stages & 1) && p.disp12_max_diff >= 0;
  if (lr_reads_cost && !cost) return SBM_ERR_NULL;
  if (stages == 2 && !(p.speckle_range >= 0 && p.speckle_window_size > 0)) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  bool inplace = false;
  if (pl.in_envelope) HIPCHK(h, mqsad_inplace_ok(h->stream, &inplace));
  bm_plan_launches(p, inplace, &pl);
  const Geom& g = pl.g;

  // the input contract, and the cost plane as the plan's SAD kernels would have stored it
  const size_t npix = (size_t)n * width * height;
  const int lo = g.mindisp * 16, hi = (g.mindisp + g.nd - 1) * 16;
  for (size_t i = 0; i < npix; i++)
    if (disp_pre[i] != g.filtered && (disp_pre[i] < lo || disp_pre[i] > hi)) return SBM_ERR_UNSUPPORTED;
  uint16_t* c16 = nullptr;
  if (lr_reads_cost) {
    for (size_t i = 0; i < npix; i++)
      if (cost[i] < 0 || (g.cost16 && disp_pre[i] != g.filtered && cost[i] > 65534)) return SBM_ERR_UNSUPPORTED;
    if (g.cost16) {
      c16 = (uint16_t*)malloc(npix * sizeof(uint16_t));
      if (!c16) return SBM_ERR_NOMEM;
      for (size_t i = 0; i < npix; i++) c16[i] = disp_pre[i] == g.filtered ? (uint16_t)0xffff : (uint16_t)cost[i];
    }
  }
  struct Tmp {   // the narrowed plane and the device map, whichever way the entry is left
    uint16_t* c16;
    void* out = nullptr;
    ~Tmp() { free(c16); if (out) hipFree(out); }
  } tmp{c16};

  size_t ho_flags = 0;
  const size_t ho_bytes = sad_fast_handoff_bytes(pl, &ho_flags);
  st = ensure_scratch(h, n, width, height, g.pitch, g.want_cost, pl.speckle, ho_bytes, ho_flags);
  if (st != SBM_OK) return st;
  h->have_last = false;   // the planes no longer hold a call's stages
  h->instr = false;       // and this is no call for the stage clock
  HIPCHK(h, hipMalloc(&tmp.out, npix * sizeof(int16_t)));
  int16_t* out = (int16_t*)tmp.out;
  if (stages & 1) {
    HIPCHK(h, hipMemcpyAsync(h->bm.disp_pre.p, disp_pre, npix * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
    if (lr_reads_cost)
      HIPCHK(h, hipMemcpyAsync(h->bm.cost.p, g.cost16 ? (const void*)c16 : (const void*)cost,
                               npix * (g.cost16 ? sizeof(uint16_t) : sizeof(int32_t)), hipMemcpyHostToDevice, h->stream));
  } else {
    HIPCHK(h, hipMemcpyAsync(out, disp_pre, npix * sizeof(int16_t), hipMemcpyHostToDevice, h->stream));
  }
  st = post_filters(h, pl, h->bm.disp_pre.as<int16_t>(), h->bm.cost.as<int32_t>(), out, stages);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpyAsync(disp, out, npix * sizeof(int16_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));

  const LrChoice lc = lr_choice(g, p.disp12_max_diff);
  const bool lr = (stages & 1) != 0, spk = (stages & 2) && pl.speckle;
  const int32_t rep[kPostInfoCount] = {stages, lr ? lc.kernel : -1, lr ? lc.nit : 0, lr ? lc.px : 0, lr ? lc.bs : 0, g.cost16,
                                       spk, spk ? pl.spk.lists : 0, spk ? pl.spk.G : 0, spk ? pl.spk.S : 0, spk ? pl.spk.SW : 0,
                                       spk ? pl.spk.max_diff : 0, g.row0, g.row1, g.col0, g.col1, g.lofs, g.xend};
  memcpy(info, rep, sizeof(rep));
  return SBM_OK;
}

int sbm_rect_map_device(sbm_handle* h, const sbm_rect_cam* cam, int width, int height, void* d_map, int sync) {
  if (!h || !cam || !d_map) return SBM_ERR_NULL;
  if (width <= 0 || height <= 0 || width > 32767 || height > 32767) return SBM_ERR_SIZE;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, launch_rect_map(*cam, width, height, (int16_t*)d_map, h->stream));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_rect_remap_device(sbm_handle* h, int n, const void* d_src, const void* d_map, int width, int height, void* d_dst,
                          int sync) {
  if (!h || !d_src || !d_map || !d_dst) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (width <= 0 || height <= 0 || width > 32767 || height > 32767) return SBM_ERR_SIZE;
  if (((size_t)width * height + 1023) / 1024 > 65535) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, launch_rect_remap((const uint8_t*)d_src, (const int16_t*)d_map, (uint8_t*)d_dst, n, width, height, h->stream));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_prefilter_device(sbm_handle* h, int n, const void* d_src, int width, int height, int flavour, int cap,
                         void* d_dst, int sync) {
  if (!h || !d_src || !d_dst) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (width <= 0 || height <= 0) return SBM_ERR_SIZE;
  if (flavour != SBM_PREFILTER_FLAVOUR_CV && flavour != SBM_PREFILTER_FLAVOUR_RTL) return SBM_ERR_PREFILTER_TYPE;
  if (flavour == SBM_PREFILTER_FLAVOUR_CV && (cap < 1 || cap > 63)) return SBM_ERR_PREFILTER_CAP;
  if (n > 65534 || height > 65535 * 4) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, launch_prefilter_dense((const uint8_t*)d_src, (uint8_t*)d_dst, n, width, height,
                                   flavour == SBM_PREFILTER_FLAVOUR_RTL, cap, h->stream));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_disparity_to_float_device(sbm_handle* h, int n, const void* d_disp, int width, int height, void* d_out, int sync) {
  if (!h || !d_disp || !d_out) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (width <= 0 || height <= 0) return SBM_ERR_SIZE;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, launch_disp_to_float((const int16_t*)d_disp, (float*)d_out, (size_t)n * width * height, h->stream));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_decimate_device(sbm_handle* h, int n, const void* d_disp, int width, int height, int scale, void* d_out, int sync) {
  if (!h || !d_disp || !d_out) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (width <= 0 || height <= 0 || scale <= 0) return SBM_ERR_SIZE;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, launch_decimate((const int16_t*)d_disp, (int16_t*)d_out, n, width, height, scale, h->stream));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_reproject_device(sbm_handle* h, int n, const void* d_disp, int width, int height, int scale,
                         const sbm_stereo_model* model, int apply_local, void* d_xyz, int sync) {
  if (!h || !d_disp || !d_xyz || !model) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (width <= 0 || height <= 0 || scale <= 0) return SBM_ERR_SIZE;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, launch_reproject((const int16_t*)d_disp, (float*)d_xyz, n, width, height, scale, *model, apply_local, h->stream));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_keypoints3d_device(sbm_handle* h, const void* d_disp, int width, int height, const void* d_kpts, int nk,
                           const sbm_stereo_model* model, float min_depth, float max_depth, void* d_xyz, int sync) {
  if (!h || !d_disp || !model || (nk > 0 && (!d_kpts || !d_xyz))) return SBM_ERR_NULL;
  if (width <= 0 || height <= 0 || nk < 0) return SBM_ERR_SIZE;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, launch_keypoints3d((const int16_t*)d_disp, (const float*)d_kpts, (float*)d_xyz, width, height, nk, *model,
                               min_depth, max_depth, h->stream));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_get_profile(sbm_handle* h, const char* name, float* ms) {
  if (!h || !name || !ms) return SBM_ERR_NULL;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->profiling && h->ev_ok) collect_profile(h);
  const float* t = nullptr;
  h->each_clock([&](StageClock& c, const StageTable& tab) {
    for (int i = 0; i < tab.nstage; i++)
      if (!strcmp(name, tab.names[i])) t = &c.ms[i];
  });
  if (!t) return SBM_ERR_UNSUPPORTED;
  *ms = *t;
  return SBM_OK;
}

int sbm_last_kernel_name(sbm_handle* h, char* dst, size_t dst_bytes) {
  if (!h || !dst || dst_bytes == 0) return SBM_ERR_NULL;
  snprintf(dst, dst_bytes, "%s", h->last_kernel);
  return SBM_OK;
}

int sbm_debug_fetch(sbm_handle* h, int which, void* dst, size_t dst_bytes) {
  if (!h || !dst) return SBM_ERR_NULL;
  if (which >= 4 && which <= 6) return sgbm_debug_fetch(h, which, dst, dst_bytes);   // the last semi-global matcher call
  if (!h->have_last) return SBM_ERR_UNSUPPORTED;
  const Geom& g = h->last;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const size_t npix = (size_t)g.n * g.W * g.H;
  if (which == 0 || which == 1) {
    if (dst_bytes < npix) return SBM_ERR_SIZE;
    const uint8_t* src = (which == 0 ? h->bm.pf_l : h->bm.pf_r).as<uint8_t>();
    HIPCHK(h, hipMemcpy2D(dst, g.W, src + g.padl, g.pitch, g.W, (size_t)g.n * g.H, hipMemcpyDeviceToHost));
    uint8_t* d = (uint8_t*)dst;
    for (size_t i = 0; i < npix; i++) d[i] = (uint8_t)((d[i] - kPfBias) >> g.pfshift);
    return SBM_OK;
  }
  if (which == 2) {
    if (!h->bm.cost.p) return SBM_ERR_UNSUPPORTED;
    if (dst_bytes < npix * sizeof(int32_t)) return SBM_ERR_SIZE;
    if (g.cost16) {
      uint16_t* tmp = (uint16_t*)malloc(npix * sizeof(uint16_t));
      if (!tmp) return SBM_ERR_NOMEM;
      hipError_t e = hipMemcpy(tmp, h->bm.cost.p, npix * sizeof(uint16_t), hipMemcpyDeviceToHost);
      if (e == hipSuccess)
        for (size_t i = 0; i < npix; i++) ((int32_t*)dst)[i] = tmp[i];
      free(tmp);
      HIPCHK(h, e);
      return SBM_OK;
    }
    HIPCHK(h, hipMemcpy(dst, h->bm.cost.p, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SBM_OK;
  }
  if (which == 3) {
    if (dst_bytes < npix * sizeof(int16_t)) return SBM_ERR_SIZE;
    HIPCHK(h, hipMemcpy(dst, h->bm.disp_pre.p, npix * sizeof(int16_t), hipMemcpyDeviceToHost));
    // rows outside the valid ROI and the never-matchable column bands are not produced on the device
    int16_t* d = (int16_t*)dst;
    for (int i = 0; i < g.n; i++)
      for (int y = 0; y < g.H; y++) {
        int16_t* row = d + ((size_t)i * g.H + y) * g.W;
        const bool live = y >= g.row0 && y < g.row1;
        for (int x = 0; x < g.W; x++)
          if (!live || x < g.lofs || x >= g.lofs + g.xend) row[x] = (int16_t)g.filtered;
      }
    return SBM_OK;
  }
  if (which == 7) {
    // the hand-off of the interior kernel's vertical sums in the last call: int32 { (segment, pair, strip) that took their sums
    // over, those that could have }
    if (dst_bytes < 2 * sizeof(int32_t)) return SBM_ERR_SIZE;
    int32_t* d = (int32_t*)dst;
    d[0] = 0;
    d[1] = (int32_t)h->bm.ho_links;
    if (!h->bm.ho_links) return SBM_OK;
    // [slots] ready words, [slots] taken words: a slot that was taken holds the call's number in its taken word
    const size_t slots = h->bm.ho_slots;
    uint32_t* tmp = (uint32_t*)malloc(slots * sizeof(uint32_t));
    if (!tmp) return SBM_ERR_NOMEM;
    const hipError_t e = hipMemcpy(tmp, h->bm.handoff.as<uint32_t>() + slots, slots * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess)
      for (size_t i = 0; i < slots; i++) d[0] += tmp[i] == h->bm.ho_epoch;
    free(tmp);
    HIPCHK(h, e);
    return SBM_OK;
  }
  return SBM_ERR_UNSUPPORTED;
}

}  // extern "C"
