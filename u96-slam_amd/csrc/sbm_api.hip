// sbm_api.hip -- C-ABI of libsbm_hip.so (declared in include/sbm.h): parameter checks, device scratch,
// kernel orchestration.  Replaces cv::StereoBM::compute at src/slam/src/core/main.cpp:201-216.
//
// Stage order (same as cv::StereoBM::compute): prefilter both images -> SAD/WTA on the valid-ROI rows
// (fast kernel: interior columns + the clamped border columns as extra wavefronts of the same launch; generic kernel otherwise) -> LR check + invalid
// row/column fill -> speckle filter.  Everything is enqueued on the handle's stream; no host sync inside.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <chrono>
#include <mutex>
#include <new>
#include <thread>

#include "sbm_common.h"

using namespace sbm;
namespace sbm { thread_local char g_sad_kernel_name[96] = ""; }

struct sbm_handle {
  sbm_params p;
  int device;
  hipStream_t stream;
  int last_hip;
  // scratch, sized for (cap_n, cap_W, cap_H, cap pitch)
  int cap_n, cap_W, cap_H, cap_pitch;
  uint8_t *pf_l, *pf_r;
  int16_t* disp_pre;
  int32_t* cost;
  unsigned long long* lr_keys;   // claim table of the LR check for rows wider than kLrLdsCols (lr_keys_bytes), else null
  size_t lr_keys_bytes;
  void* spk_runs;        // speckle filter: 16 bytes per pixel (run records of the band walk / labels + sizes of the row-walking kernels)
  int32_t* spk_nheads;   // cap_n * H (runs per row)
  uint32_t* spk_seam;    // contacts across band seams (band walk of the speckle filter): cap_n * ceil(H/2) * W entries
  int32_t* spk_nseam;    // cap_n * ceil(H/2)
  uint16_t* vsum;      // column sums of PREFILTER_NORMALIZED_RESPONSE (2 * cap_n * W * H), allocated on first use
  // FPGA-flavour matcher scratch (allocated on first use, sized for fp_n pairs of fp_W x fp_H)
  int fp_n, fp_W, fp_H;
  uint8_t *fp_xs_l, *fp_xs_r;
  int fp_gen;              // call counter of the FPGA-flavour matcher: generation stamp of its saturation flags
  void* fp_rec;
  int* fp_flag;
  // staging for the host-buffer entry points
  int st_n, st_W, st_H;
  uint8_t *st_l, *st_r;
  int16_t* st_d;
  uint8_t* pin;        // pinned host staging for strided caller images (rows packed / unpacked on the CPU)
  size_t pin_bytes;
  // small host-buffer calls (the reference's one pair per call): the maps leave through a copy kernel that writes pinned,
  // device-mapped host memory and raises a flag there; the host polls the flag instead of synchronising the stream
  int16_t* zc_out;     // pinned + mapped host staging of the maps
  size_t zc_bytes;
  unsigned* zc_flag;   // pinned + mapped: sequence number of the last call whose maps are complete in zc_out
  unsigned* zc_cnt;    // device: workgroups of the copy kernel that have finished (the last one raises the flag and clears it)
  unsigned zc_seq;
  // copy streams + per-chunk events of the pipelined host batch path (created on first use)
  hipStream_t stream_in, stream_out;
  // asynchronous dense feed (sbm_submit_dense / sbm_wait_oldest): two device staging sets, up to three submissions in
  // flight (one arriving, one computing, one leaving); events are indexed by submission number & 3
  uint8_t *fq_l[2], *fq_r[2];
  int16_t* fq_d[2];
  int fq_n, fq_W, fq_H;
  hipEvent_t ev_fq_in[4], ev_fq_done[4], ev_fq_out[4];
  bool fq_ok;
  unsigned fq_submitted, fq_waited;
  int16_t* fq_pending_dst;     // maps of the newest submission not yet queued for their trip home (see sbm_submit_dense)
  size_t fq_pending_bytes;
  static constexpr int kChunks = 64;
  hipEvent_t ev_in[kChunks], ev_done[kChunks];
  bool pipe_ok;
  char last_kernel[128];   // SAD kernel of the last sbm_compute_device call (sbm_last_kernel_name)
  // last launch (for sbm_debug_fetch)
  Geom last;
  bool have_last;
  // profiling: mode 1 = sync after every call and keep that call's stage times; mode 2 = record stage events of
  // every call into a ring WITHOUT syncing (bench.py's timed region); sbm_get_profile then averages the ring.
  // mode 3 = mode 2 on every 4th call only (six event records cost ~25 us per call: sampling keeps the timed region honest)
  int profiling;
  unsigned ncall;      // calls since profiling was (re)enabled
  bool instr;          // this call records events
  static constexpr int kRing = 64, kMarks = 6;
  hipEvent_t ev[kRing][kMarks];
  bool ev_ok;
  unsigned calls;  // calls recorded since profiling was (re)enabled
  float ms_prefilter, ms_sad, ms_border, ms_lr, ms_speckle, ms_total;
  // semi-global matcher (allocated on first use): C and S for sg_chunk pairs, the map before the median for sg_n pairs, the
  // speckle filter's scratch for sg_n pairs; the geometry of the last call for sbm_debug_fetch
  int16_t *sg_C, *sg_S;
  size_t sg_cs_bytes;
  int16_t* sg_pre;
  size_t sg_pre_bytes;
  int sg_spk_n, sg_spk_W, sg_spk_H;
  void* sg_spk_runs;
  int32_t *sg_spk_nheads, *sg_spk_nseam;
  uint32_t* sg_spk_seam;
  SgbmGeom sg_last;
  bool sg_have_last, sg_last_one_chunk;
  hipEvent_t sg_ev[6];
  float sg_ms[6];   // cost, aggregate, select, median, speckle, total
  // keypoint selection (allocated on first use): the cell tables of the global-table kernel for one chunk of images; the
  // points and counts of the host-memory entry point
  unsigned* gs_tab;
  size_t gs_tab_bytes;
  void* gs_out;
  size_t gs_out_bytes;
  hipEvent_t gs_ev[3];
  float gs_ms[3];   // eig, select, total
  // ORB descriptors (allocated on first use): blurred frames of one chunk; the keypoints, counts and descriptors of the
  // host-memory entry point
  uint8_t* or_blur;
  size_t or_blur_bytes;
  void* or_io;
  size_t or_io_bytes;
  hipEvent_t or_ev[3];
  float or_ms[3];   // blur, desc, total
};

// Entry points select the handle's device and put the caller's current device back on return.
struct DeviceScope {
  int prev, dev;
  bool have;
  explicit DeviceScope(int d) : prev(-1), dev(d), have(false) { have = hipGetDevice(&prev) == hipSuccess; }
  hipError_t enter() { return (have && prev == dev) ? hipSuccess : hipSetDevice(dev); }
  ~DeviceScope() {
    if (have && prev != dev) hipSetDevice(prev);
  }
};

#ifdef SBM_DEV   // development builds: wall-clock stamps of the host-buffer entry point's phases (tools/exp/r05_host_attrib.py)
static double g_hp_acc[8];
static unsigned long long g_hp_calls;
struct HostProf {
  std::chrono::steady_clock::time_point t;
  HostProf() : t(std::chrono::steady_clock::now()) {}
  void stamp(int i) {
    const auto n = std::chrono::steady_clock::now();
    g_hp_acc[i] += std::chrono::duration<double, std::micro>(n - t).count();
    t = n;
  }
};
#define HP_BEGIN() HostProf hp_; g_hp_calls++
#define HP(i) hp_.stamp(i)
extern "C" int sbm_dev_host_prof(double* out8, unsigned long long* calls) {
  for (int i = 0; i < 8; i++) { out8[i] = g_hp_acc[i]; g_hp_acc[i] = 0; }
  *calls = g_hp_calls; g_hp_calls = 0;
  return 0;
}
#else
#define HP_BEGIN() do { } while (0)
#define HP(i) do { } while (0)
#endif

static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield");
#else
  std::this_thread::yield();
#endif
}

#define HIPCHK(h, call)                         \
  do {                                          \
    hipError_t e_ = (call);                     \
    if (e_ != hipSuccess) {                     \
      (h)->last_hip = (int)e_;                  \
      return e_ == hipErrorOutOfMemory ? SBM_ERR_NOMEM : SBM_ERR_HIP; \
    }                                           \
  } while (0)

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
    default: return "unknown status";
  }
}

int sbm_version(void) { return SBM_VERSION_MAJOR * 1000 + SBM_VERSION_MINOR; }

static void free_scratch(sbm_handle* h) {
  hipFree(h->pf_l); hipFree(h->pf_r); hipFree(h->disp_pre); hipFree(h->cost);
  hipFree(h->lr_keys);
  h->lr_keys = nullptr; h->lr_keys_bytes = 0;
  hipFree(h->spk_runs); hipFree(h->spk_nheads); hipFree(h->spk_seam); hipFree(h->spk_nseam);
  h->spk_runs = nullptr; h->spk_nheads = nullptr; h->spk_seam = nullptr; h->spk_nseam = nullptr;
  hipFree(h->vsum);
  h->vsum = nullptr;
  h->pf_l = h->pf_r = nullptr; h->disp_pre = nullptr; h->cost = nullptr;
  h->cap_n = h->cap_W = h->cap_H = h->cap_pitch = 0;
}

static void free_sgbm(sbm_handle* h) {
  hipFree(h->sg_C); hipFree(h->sg_S); hipFree(h->sg_pre);
  h->sg_C = h->sg_S = h->sg_pre = nullptr; h->sg_cs_bytes = h->sg_pre_bytes = 0;
  hipFree(h->sg_spk_runs); hipFree(h->sg_spk_nheads); hipFree(h->sg_spk_seam); hipFree(h->sg_spk_nseam);
  h->sg_spk_runs = nullptr; h->sg_spk_nheads = h->sg_spk_nseam = nullptr; h->sg_spk_seam = nullptr;
  h->sg_spk_n = h->sg_spk_W = h->sg_spk_H = 0;
  h->sg_have_last = false;
}

static void free_gftt_sel(sbm_handle* h) {
  hipFree(h->gs_tab); hipFree(h->gs_out);
  h->gs_tab = nullptr; h->gs_out = nullptr; h->gs_tab_bytes = h->gs_out_bytes = 0;
}

static void free_orb(sbm_handle* h) {
  hipFree(h->or_blur); hipFree(h->or_io);
  h->or_blur = nullptr; h->or_io = nullptr; h->or_blur_bytes = h->or_io_bytes = 0;
}

static void free_fpga(sbm_handle* h) {
  hipFree(h->fp_xs_l); hipFree(h->fp_xs_r); hipFree(h->fp_rec); hipFree(h->fp_flag);
  h->fp_xs_l = h->fp_xs_r = nullptr; h->fp_rec = nullptr; h->fp_flag = nullptr;
  h->fp_n = h->fp_W = h->fp_H = 0;
}

// The device sets of the asynchronous dense feed have their own life: submissions may be outstanding (the newest one's
// trip home not even queued yet) while a synchronous host entry point resizes ITS staging, so only the feed's own realloc
// path (drained first) and the handle's end of life free them.
static void free_feed(sbm_handle* h) {
  for (int k = 0; k < 2; k++) { hipFree(h->fq_l[k]); hipFree(h->fq_r[k]); hipFree(h->fq_d[k]); h->fq_l[k] = h->fq_r[k] = nullptr; h->fq_d[k] = nullptr; }
  h->fq_n = h->fq_W = h->fq_H = 0;
}

static void free_staging(sbm_handle* h) {
  hipFree(h->st_l); hipFree(h->st_r); hipFree(h->st_d);
  if (h->pin) hipHostFree(h->pin);
  h->pin = nullptr; h->pin_bytes = 0;
  if (h->zc_out) hipHostFree(h->zc_out);
  if (h->zc_flag) hipHostFree(h->zc_flag);
  hipFree(h->zc_cnt);
  h->zc_out = nullptr; h->zc_flag = nullptr; h->zc_cnt = nullptr; h->zc_bytes = 0;
  h->st_l = h->st_r = nullptr; h->st_d = nullptr; h->st_n = h->st_W = h->st_H = 0;
}

// The reference re-creates its matcher for every frame (cv::StereoBM::create inside the loop, main.cpp:201). Streams,
// ~400 events and the device scratch make a cold handle cost ~2 ms -- ten times the frame itself -- so destroyed handles
// are parked (a few, with at most kPoolScratch bytes of scratch each) and sbm_create re-arms one for the same device.
static std::mutex g_pool_mu;
static constexpr int kPool = 4;
static constexpr size_t kPoolScratch = (size_t)512 << 20;
static sbm_handle* g_pool[kPool];
static int g_pool_n = 0;

static size_t scratch_bytes(const sbm_handle* h) {
  const size_t npix = (size_t)h->cap_n * h->cap_W * h->cap_H, plane = (size_t)h->cap_n * h->cap_pitch * h->cap_H;
  size_t b = 2 * plane + npix * 2;
  if (h->cost) b += npix * 4;
  b += h->lr_keys_bytes;
  if (h->spk_runs) b += (size_t)h->cap_n * h->cap_H * (16 * ((size_t)h->cap_W + kSpkRecordPad) + 2 * ((size_t)h->cap_W + kSpkSeamPad) + 24);   // run records, seam lists, run / contact counts
  if (h->vsum) b += 2 * npix * sizeof(uint16_t);
  b += (size_t)h->st_n * h->st_W * h->st_H * 4 + h->pin_bytes;
  b += (size_t)h->fq_n * h->fq_W * h->fq_H * 8;
  b += (size_t)h->fp_n * h->fp_W * h->fp_H * 10;
  b += 2 * h->sg_cs_bytes + h->sg_pre_bytes;
  b += h->or_blur_bytes + h->or_io_bytes;
  if (h->sg_spk_runs) b += (size_t)h->sg_spk_n * h->sg_spk_H * (16 * ((size_t)h->sg_spk_W + kSpkRecordPad) + 4 * ((size_t)h->sg_spk_W + kSpkSeamPad) + 24);
  return b;
}

static void destroy_now(sbm_handle* h);

void sbm_trim(void) {
  std::lock_guard<std::mutex> lk(g_pool_mu);
  for (int i = 0; i < g_pool_n; i++) destroy_now(g_pool[i]);
  g_pool_n = 0;
}

int sbm_create(sbm_handle** out, const sbm_params* p, int device) {
  if (!out || !p) return SBM_ERR_NULL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return SBM_ERR_NO_DEVICE;
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    for (int i = 0; i < g_pool_n; i++)
      if (g_pool[i]->device == device) {
        sbm_handle* h = g_pool[i];
        g_pool[i] = g_pool[--g_pool_n];
        h->p = *p;
        h->last_hip = 0;
        h->have_last = false;
        h->sg_have_last = false;
        h->profiling = 0;
        h->calls = 0;
        h->ms_prefilter = h->ms_sad = h->ms_border = h->ms_lr = h->ms_speckle = h->ms_total = 0.f;
        for (float& t : h->sg_ms) t = 0.f;
        for (float& t : h->gs_ms) t = 0.f;
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
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (g_pool_n < kPool) {
      if (scratch_bytes(h) > kPoolScratch) {
        free_scratch(h);
        free_staging(h);
        free_feed(h);
        free_fpga(h);
        free_sgbm(h);
        free_gftt_sel(h);
        free_orb(h);
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
  free_scratch(h);
  free_staging(h);
  free_feed(h);
  free_fpga(h);
  free_sgbm(h);
  free_gftt_sel(h);
  free_orb(h);
  for (int i = 0; i < 6; i++)
    if (h->sg_ev[i]) hipEventDestroy(h->sg_ev[i]);
  for (int i = 0; i < 3; i++)
    if (h->gs_ev[i]) hipEventDestroy(h->gs_ev[i]);
  for (int i = 0; i < 3; i++)
    if (h->or_ev[i]) hipEventDestroy(h->or_ev[i]);
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
  h->profiling = enabled;
  h->calls = 0;
  h->ncall = 0;
  h->instr = false;
  h->ms_prefilter = h->ms_sad = h->ms_border = h->ms_lr = h->ms_speckle = h->ms_total = 0.f;
  for (float& t : h->sg_ms) t = 0.f;
  for (float& t : h->gs_ms) t = 0.f;
  for (float& t : h->or_ms) t = 0.f;
  return SBM_OK;
}

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

static int ensure_scratch(sbm_handle* h, int n, int W, int H, int pitch, bool need_cost, bool need_speckle) {
  const bool fits = n <= h->cap_n && W == h->cap_W && H == h->cap_H && pitch == h->cap_pitch && h->pf_l;
  if (!fits) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    free_scratch(h);
    const size_t npix = (size_t)n * W * H, pfbytes = (size_t)n * pitch * H + 4096;
    HIPCHK(h, hipMalloc((void**)&h->pf_l, pfbytes));
    HIPCHK(h, hipMalloc((void**)&h->pf_r, pfbytes));
    HIPCHK(h, hipMalloc((void**)&h->disp_pre, npix * sizeof(int16_t)));
    // padding bytes must read as 0 (the masked value of the fast kernel); the prefilter never writes them
    HIPCHK(h, hipMemsetAsync(h->pf_l, 0, pfbytes, h->stream));
    HIPCHK(h, hipMemsetAsync(h->pf_r, 0, pfbytes, h->stream));
    h->cap_n = n; h->cap_W = W; h->cap_H = H; h->cap_pitch = pitch;
  }
  const size_t npix = (size_t)h->cap_n * W * H;
  if (need_cost && !h->cost) HIPCHK(h, hipMalloc((void**)&h->cost, npix * sizeof(int32_t)));
  const size_t keys = lr_keys_bytes(h->cap_n, W, H, need_cost);
  if (keys > h->lr_keys_bytes) {
    hipFree(h->lr_keys);
    h->lr_keys = nullptr; h->lr_keys_bytes = 0;
    HIPCHK(h, hipMalloc((void**)&h->lr_keys, keys));
    h->lr_keys_bytes = keys;
  }
  if (need_speckle && !h->spk_nseam) {   // keyed on the LAST buffer of the set: an attempt that failed half way is redone
    hipFree(h->spk_runs); hipFree(h->spk_nheads); hipFree(h->spk_seam);
    h->spk_runs = nullptr; h->spk_nheads = nullptr; h->spk_seam = nullptr;
    // sizes: launch_speckle (sbm_common.h)
    HIPCHK(h, hipMalloc(&h->spk_runs, (size_t)h->cap_n * H * ((size_t)W + kSpkRecordPad) * 16));
    HIPCHK(h, hipMalloc((void**)&h->spk_nheads, (size_t)h->cap_n * H * kSpkMaxSeg * sizeof(int32_t)));
    const size_t seams = (size_t)h->cap_n * ((H + 1) / 2);
    HIPCHK(h, hipMalloc((void**)&h->spk_seam, seams * ((size_t)W + kSpkSeamPad) * sizeof(uint32_t)));
    HIPCHK(h, hipMalloc((void**)&h->spk_nseam, seams * kSpkMaxSeg * sizeof(int32_t)));
  }
  return SBM_OK;
}

static inline void mark(sbm_handle* h, int i) {
  if (h->instr) hipEventRecord(h->ev[h->calls % sbm_handle::kRing][i], h->stream);
}

// mode 2: average stage times over the recorded calls (at most the last kRing); mode 1: the last call only.
// The stream must be idle.
static void collect_profile(sbm_handle* h) {
  unsigned nrec = std::min<unsigned>(h->calls, sbm_handle::kRing), first = 0;
  if (h->profiling == 1 && h->calls > 0) { first = (h->calls - 1) % sbm_handle::kRing; nrec = 1; }
  // events 0..5 with 3 unused (it used to close the border kernel's side stream; one launch carries those columns now)
  static const int kFrom[4] = {0, 1, 2, 4}, kTo[4] = {1, 2, 4, 5};
  float acc[4] = {0, 0, 0, 0}, tot = 0.f;
  for (unsigned r = first; r < first + nrec; r++) {
    for (int i = 0; i < 4; i++) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, h->ev[r][kFrom[i]], h->ev[r][kTo[i]]) == hipSuccess) acc[i] += ms;
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->ev[r][0], h->ev[r][5]) == hipSuccess) tot += ms;
  }
  const float inv = nrec ? 1.f / nrec : 0.f;
  h->ms_prefilter = acc[0] * inv; h->ms_sad = acc[1] * inv; h->ms_border = 0.f; h->ms_lr = acc[2] * inv;
  h->ms_speckle = acc[3] * inv; h->ms_total = tot * inv;
}

int sbm_compute_device(sbm_handle* h, int n, const void* d_left, const void* d_right, int width, int height,
                       void* d_disp, int sync) {
  if (!h || !d_left || !d_right || !d_disp) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  int st = sbm_params_validate(&h->p, width, height);
  if (st != SBM_OK) return st;
  if (n > 32767 || height > 65535) return SBM_ERR_UNSUPPORTED;
  const sbm_params& p = h->p;
  if (p.num_disparities > 4096) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());

  Geom g;
  memset(&g, 0, sizeof(g));
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
  int16_t* out = (int16_t*)d_disp;

  int roi[4];
  g.reading = env_switch("SBM_CV_READING", 0);
  valid_roi(p, width, height, g.reading, roi);
  g.row0 = std::max(roi[1], 0); g.row1 = std::min(roi[1] + roi[3], height);
  g.col0 = std::max(std::min(roi[0], width), 0); g.col1 = std::max(std::min(roi[0] + roi[2], width), 0);
  const bool range_fits = !(g.lofs >= width || g.rofs >= width || g.width1 < 1);
  const bool any_rows = range_fits && roi[2] > 0 && roi[3] > 0 && g.row1 > g.row0;
  if (!any_rows) { g.row0 = g.row1 = 0; }
  const bool speckle = p.speckle_range >= 0 && p.speckle_window_size > 0;

  st = ensure_scratch(h, n, width, height, g.pitch, g.want_cost, speckle);
  if (st != SBM_OK) return st;
  h->last = g; h->have_last = true;

  // The interior kernel needs the in-place v_mqsad accumulate: its device self-test runs on this handle's stream, once per
  // device (a check that could not run fails this call with its HIP error and runs again on the next one). Without it the
  // sliding-sum kernel takes the whole envelope.
  const bool in_envelope = any_rows && sad_fast_supported(g);
  bool inplace = false;
  if (in_envelope) HIPCHK(h, mqsad_inplace_ok(h->stream, &inplace));
  const bool fast = in_envelope && inplace;
  // 16-bit cost plane when every producer is a 16-bit-sum kernel (fast interior + border kernels, w/2 clamped columns on
  // each side); the generic kernel needs int32
  int fa = 0, fb = 0;
  if (fast) {
    const int xhi = std::min(g.W - g.lofs - 1, g.W - g.rofs - g.nd);
    fa = g.w2; fb = xhi - g.w2 + 1;   // the interior range launch_sad_fast covers; xend - fb == w/2 by construction
    g.cost16 = 1;
    g.pfshift = sad_fast_pfshift(g);   // pre-scaled planes for the interior kernel's tagged winner search
  }
  h->last = g;
  // columns left and right of the fast range: clamped windows. They only matter if they can influence the output:
  // through the LR check or when inside the valid ROI.
  const bool borders_visible = g.want_cost || g.col0 < g.lofs + fa || g.col1 > g.lofs + fb;
  // ... and then they ride in the interior launch as extra wavefronts (sbm_sad_border_wave.h): one SAD launch, one stream
  const bool border = fast && borders_visible;
  // Stages run one after the other on the main stream. Overlapping LR + speckle of one sub-batch with the SAD kernel of
  // the next was built and measured in round 2 (profiles/r02_subbatch_pipeline.md; the code is in the history at commit
  // "Engine: device guard ..."): 1.47 ms -> 1.54 / 1.73 ms with 2 / 4 sub-batches, because four 126-VGPR wavefronts per
  // SIMD leave no registers for a guest wavefront -- the post-filters only overlap once the SAD kernel runs at 3
  // wavefronts per SIMD, which costs it 27 %.
  const uint8_t* dl = (const uint8_t*)d_left;
  const uint8_t* dr = (const uint8_t*)d_right;

  h->instr = h->profiling && h->ev_ok && (h->profiling != 3 || (h->ncall & 3u) == 0);
  mark(h, 0);
  if (any_rows) {
    if (p.prefilter_type == SBM_PREFILTER_XSOBEL) {
      HIPCHK(h, launch_prefilter(dl, dr, h->pf_l, h->pf_r, g, h->stream));
    } else {
      if (!h->vsum) HIPCHK(h, hipMalloc((void**)&h->vsum, (size_t)2 * h->cap_n * width * height * sizeof(uint16_t)));
      HIPCHK(h, launch_prefilter_norm(dl, dr, h->pf_l, h->pf_r, h->vsum, g, p.prefilter_size, h->stream));
    }
  }
  mark(h, 1);
  if (any_rows) {
    if (fast) {
      int xa = 0, xb = 0;
      HIPCHK(h, launch_sad_fast(h->pf_l, h->pf_r, h->disp_pre, h->cost, g, &xa, &xb, border, h->stream));
      snprintf(h->last_kernel, sizeof(h->last_kernel), "%s", g_sad_kernel_name);
      if (border && !sad_fast_borders_in_launch(g)) {   // beyond 256 disparities: the clamped columns from the sliding-sum kernel
        HIPCHK(h, launch_sad_wide(h->pf_l, h->pf_r, h->disp_pre, h->cost, g, 0, xa, h->stream));
        HIPCHK(h, launch_sad_wide(h->pf_l, h->pf_r, h->disp_pre, h->cost, g, xb, g.xend, h->stream));
      }
    } else if (sad_wide_supported(g) && env_switch("SBM_WIDE", 1)) {
      HIPCHK(h, launch_sad_wide(h->pf_l, h->pf_r, h->disp_pre, h->cost, g, 0, g.xend, h->stream));
      // (say so when the interior kernel was left out only because the in-place accumulate is off or its device self-test
      // failed: 8-25x slower, see include/sbm.h)
      snprintf(h->last_kernel, sizeof(h->last_kernel), in_envelope ? "sad_wide_kernel [in-place accumulate unavailable]" : "sad_wide_kernel");
    } else {
      HIPCHK(h, launch_sad_generic(h->pf_l, h->pf_r, h->disp_pre, h->cost, g, 0, g.xend, h->stream));
      snprintf(h->last_kernel, sizeof(h->last_kernel), "sad_generic_kernel");
    }
  }
  mark(h, 2);
  HIPCHK(h, launch_lrcheck(h->disp_pre, h->cost, out, h->lr_keys, g, p.disp12_max_diff, h->stream));
  mark(h, 4);
  if (speckle)
    HIPCHK(h, launch_speckle(out, h->spk_runs, h->spk_nheads, h->spk_seam, h->spk_nseam, g, p.speckle_window_size, p.speckle_range, h->stream));
  mark(h, 5);
  if (h->instr) h->calls++;
  h->ncall++;
  if (sync || h->profiling == 1) HIPCHK(h, hipStreamSynchronize(h->stream));
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

// ---- FPGA flavour: register decode (bm.v:172-193), limits, entry points -----------------------------------------------------
int sbm_fpga_params_from_regs(uint32_t image_size, uint32_t bm_setting, uint32_t uni_filt_ctrl, sbm_fpga_params* out) {
  if (!out) return SBM_ERR_NULL;
  out->width = (int32_t)(image_size & 0x3ffu);
  out->height = (int32_t)((image_size >> 16) & 0x1ffu);
  out->block_size = (int32_t)((bm_setting >> 16) & 0x1fu);
  out->num_disparities = (int32_t)(bm_setting & 0x1ffu);
  out->uni_enable = (int32_t)((uni_filt_ctrl >> 31) & 1u);
  out->uni_mode = (int32_t)((uni_filt_ctrl >> 16) & 1u);
  out->uni_threshold = (int32_t)(uni_filt_ctrl & 0x3ffu);
  return SBM_OK;
}

uint32_t sbm_fpga_sad_size_reg(const sbm_fpga_params* p) {
  if (!p) return 0;
  const uint32_t hwsz = ((uint32_t)p->block_size >> 1) & 0xfu;
  const uint32_t hsad_wdt = ((uint32_t)p->width - (uint32_t)p->num_disparities - 1u) & 0x3ffu;   // bm.v:249
  const uint32_t sad_wdt = (hsad_wdt - 2u * hwsz) & 0x3ffu;                                        // bm.v:252
  const uint32_t sad_hgt = ((uint32_t)p->height - 2u * hwsz) & 0x1ffu;                             // bm.v:255
  return (sad_hgt << 16) | sad_wdt;
}

int sbm_fpga_params_validate(const sbm_fpga_params* p) {
  if (!p) return SBM_ERR_NULL;
  if (p->width <= 0 || p->height <= 0 || p->width > 1023 || p->height > 511) return SBM_ERR_SIZE;
  if (p->block_size < 3 || p->block_size > 31 || (p->block_size & 1) == 0) return SBM_ERR_BLOCK_SIZE;
  if (p->num_disparities < 32 || p->num_disparities > 256 || (p->num_disparities & 31)) return SBM_ERR_NUM_DISPARITIES;
  const int hwsz = p->block_size >> 1;
  if (p->width - p->num_disparities - 1 - 2 * hwsz < 1 || p->height - 2 * hwsz < 1) return SBM_ERR_SIZE;
  if (((p->num_disparities + hwsz + 1) & 31) == 0) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

static int ensure_fpga(sbm_handle* h, int n, int W, int H, bool need_xs) {
  const bool fits = n <= h->fp_n && W == h->fp_W && H == h->fp_H && h->fp_flag;
  if (!fits) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    free_fpga(h);
    const size_t npix = (size_t)n * W * H;
    HIPCHK(h, hipMalloc(&h->fp_rec, npix * 8));
    HIPCHK(h, hipMalloc((void**)&h->fp_flag, (size_t)n * sizeof(int)));
    HIPCHK(h, hipMemsetAsync(h->fp_flag, 0, (size_t)n * sizeof(int), h->stream));   // generation stamps: 0 = never saturated
    h->fp_gen = 0;
    h->fp_n = n; h->fp_W = W; h->fp_H = H;
  }
  if (need_xs && !h->fp_xs_l) {
    const size_t npix = (size_t)h->fp_n * W * H;
    HIPCHK(h, hipMalloc((void**)&h->fp_xs_l, npix + 64));
    HIPCHK(h, hipMalloc((void**)&h->fp_xs_r, npix + 64));
  }
  return SBM_OK;
}

int sbm_fpga_bm_device(sbm_handle* h, int n, const void* d_xsbl_l, const void* d_xsbl_r, const sbm_fpga_params* p,
                       void* d_disp, int sync) {
  if (!h || !d_xsbl_l || !d_xsbl_r || !p || !d_disp) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  int st = sbm_fpga_params_validate(p);
  if (st != SBM_OK) return st;
  if (n > 65535) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = ensure_fpga(h, n, p->width, p->height, false);
  if (st != SBM_OK) return st;
  HIPCHK(h, launch_fpga_bm((const uint8_t*)d_xsbl_l, (const uint8_t*)d_xsbl_r, h->fp_rec, h->fp_flag, ++h->fp_gen, (int16_t*)d_disp, n, *p,
                           h->stream));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_fpga_compute_device(sbm_handle* h, int n, const void* d_left, const void* d_right, const sbm_fpga_params* p,
                            void* d_disp, int sync) {
  if (!h || !d_left || !d_right || !p || !d_disp) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  int st = sbm_fpga_params_validate(p);
  if (st != SBM_OK) return st;
  if (n > 65534) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = ensure_fpga(h, n, p->width, p->height, true);
  if (st != SBM_OK) return st;
  HIPCHK(h, launch_prefilter_dense((const uint8_t*)d_left, h->fp_xs_l, n, p->width, p->height, 1, 31, h->stream));
  HIPCHK(h, launch_prefilter_dense((const uint8_t*)d_right, h->fp_xs_r, n, p->width, p->height, 1, 31, h->stream));
  HIPCHK(h, launch_fpga_bm(h->fp_xs_l, h->fp_xs_r, h->fp_rec, h->fp_flag, ++h->fp_gen, (int16_t*)d_disp, n, *p, h->stream));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

static int ensure_staging(sbm_handle* h, int n, int W, int H);

// host-memory forms of the PL blocks for one frame: staged through the handle's device staging buffers (2-D copies
// take care of the caller's strides)
int sbm_fpga_compute(sbm_handle* h, const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride,
                     const sbm_fpga_params* p, int16_t* disp, size_t disp_stride) {
  if (!h || !left || !right || !p || !disp) return SBM_ERR_NULL;
  int st = sbm_fpga_params_validate(p);
  if (st != SBM_OK) return st;
  const int W = p->width, H = p->height;
  if (left_stride < (size_t)W || right_stride < (size_t)W || disp_stride < (size_t)W * 2) return SBM_ERR_SIZE;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = ensure_staging(h, 1, W, H);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpy2DAsync(h->st_l, W, left, left_stride, W, H, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpy2DAsync(h->st_r, W, right, right_stride, W, H, hipMemcpyHostToDevice, h->stream));
  st = sbm_fpga_compute_device(h, 1, h->st_l, h->st_r, p, h->st_d, 0);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpy2DAsync(disp, disp_stride, h->st_d, (size_t)W * 2, (size_t)W * 2, H, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

// ---- semi-global matcher (cv::StereoSGBM, MODE_HH / MODE_SGBM) ---------------------------------------------------------------
void sbm_sgbm_params_default(sbm_sgbm_params* p, int min_disparity, int num_disparities, int block_size) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->min_disparity = min_disparity;
  p->num_disparities = num_disparities;
  p->block_size = block_size;
  p->mode = SBM_SGBM_MODE_SGBM;
}

static void sgbm_effective(const sbm_sgbm_params& p, int& bs, int& ftzero, int& P1, int& P2) {
  bs = 2 * ((p.block_size > 0 ? p.block_size : 5) / 2) + 1;
  ftzero = std::max(p.prefilter_cap, 15) | 1;
  P1 = p.p1 > 0 ? p.p1 : 2;
  P2 = std::max(p.p2 > 0 ? p.p2 : 5, P1 + 1);
}

int sbm_sgbm_params_validate(const sbm_sgbm_params* p, int width, int height) {
  if (!p) return SBM_ERR_NULL;
  if (width <= 0 || height <= 0) return SBM_ERR_SIZE;
  if (p->num_disparities <= 0 || p->num_disparities % 16 != 0) return SBM_ERR_NUM_DISPARITIES;
  if (p->mode != SBM_SGBM_MODE_SGBM && p->mode != SBM_SGBM_MODE_HH) return SBM_ERR_UNSUPPORTED;
  if (p->num_disparities > kSgbmNdMax || width > kSgbmWMax || height > 65535 || p->prefilter_cap > 63 ||
      p->uniqueness_ratio > 65535 || (p->speckle_window_size > 0 && p->speckle_range < 0))
    return SBM_ERR_UNSUPPORTED;
  // (every disparity * 16 of the map, (minDisparity - 1) * 16 included, must fit int16)
  if (p->min_disparity < -2047 || (long)p->min_disparity + p->num_disparities > 2047) return SBM_ERR_UNSUPPORTED;
  int bs, ftzero, P1, P2;
  sgbm_effective(*p, bs, ftzero, P1, P2);
  if ((long)bs * bs * (2 * ftzero + 63) + P2 > 32767) return SBM_ERR_UNSUPPORTED;   // the exactness envelope
  return SBM_OK;
}

static int ensure_sgbm(sbm_handle* h, size_t cs_bytes, size_t pre_bytes, int n, int W, int H, bool speckle) {
  if (cs_bytes > h->sg_cs_bytes || pre_bytes > h->sg_pre_bytes) HIPCHK(h, hipStreamSynchronize(h->stream));
  if (cs_bytes > h->sg_cs_bytes) {
    hipFree(h->sg_C); hipFree(h->sg_S);
    h->sg_C = h->sg_S = nullptr; h->sg_cs_bytes = 0;
    HIPCHK(h, hipMalloc((void**)&h->sg_C, cs_bytes));
    HIPCHK(h, hipMalloc((void**)&h->sg_S, cs_bytes));
    h->sg_cs_bytes = cs_bytes;
  }
  if (pre_bytes > h->sg_pre_bytes) {
    hipFree(h->sg_pre);
    h->sg_pre = nullptr; h->sg_pre_bytes = 0;
    HIPCHK(h, hipMalloc((void**)&h->sg_pre, pre_bytes));
    h->sg_pre_bytes = pre_bytes;
  }
  if (speckle && !(h->sg_spk_nseam && n <= h->sg_spk_n && W == h->sg_spk_W && H == h->sg_spk_H)) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    hipFree(h->sg_spk_runs); hipFree(h->sg_spk_nheads); hipFree(h->sg_spk_seam); hipFree(h->sg_spk_nseam);
    h->sg_spk_runs = nullptr; h->sg_spk_nheads = h->sg_spk_nseam = nullptr; h->sg_spk_seam = nullptr;
    h->sg_spk_n = h->sg_spk_W = h->sg_spk_H = 0;
    // sizes: launch_speckle (sbm_common.h)
    HIPCHK(h, hipMalloc(&h->sg_spk_runs, (size_t)n * H * ((size_t)W + kSpkRecordPad) * 16));
    HIPCHK(h, hipMalloc((void**)&h->sg_spk_nheads, (size_t)n * H * kSpkMaxSeg * sizeof(int32_t)));
    const size_t seams = (size_t)n * ((H + 1) / 2);
    HIPCHK(h, hipMalloc((void**)&h->sg_spk_seam, seams * ((size_t)W + kSpkSeamPad) * sizeof(uint32_t)));
    HIPCHK(h, hipMalloc((void**)&h->sg_spk_nseam, seams * kSpkMaxSeg * sizeof(int32_t)));
    h->sg_spk_n = n; h->sg_spk_W = W; h->sg_spk_H = H;
  }
  return SBM_OK;
}

// Device scratch of one chunk of pairs -- C, S, the map before the median and (speckle filter on) its scratch -- stays within
// kSgbmChunkBytes; a single pair larger than that runs alone.
static constexpr size_t kSgbmChunkBytes = (size_t)2 << 30;

static size_t sgbm_speckle_bytes_per_pair(int W, int H) {   // sizes: launch_speckle (sbm_common.h), as allocated by ensure_sgbm
  const size_t seams = (size_t)(H + 1) / 2;
  return (size_t)H * ((size_t)W + kSpkRecordPad) * 16 + (size_t)H * kSpkMaxSeg * sizeof(int32_t) +
         seams * (((size_t)W + kSpkSeamPad) * sizeof(uint32_t) + kSpkMaxSeg * sizeof(int32_t));
}

int sbm_sgbm_compute_device(sbm_handle* h, const sbm_sgbm_params* p, int n, const void* d_left, const void* d_right, int width,
                            int height, void* d_disp, int sync) {
  if (!h || !p || !d_left || !d_right || !d_disp) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  int st = sbm_sgbm_params_validate(p, width, height);
  if (st != SBM_OK) return st;
  if (n > 32767) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());

  SgbmGeom g;
  memset(&g, 0, sizeof(g));
  int bs, ftzero, P1, P2;
  sgbm_effective(*p, bs, ftzero, P1, P2);
  g.W = width; g.H = height;
  g.minD = p->min_disparity; g.D = p->num_disparities;
  g.minX1 = std::max(g.minD + g.D, 0); g.maxX1 = width + std::min(g.minD, 0); g.W1 = g.maxX1 - g.minX1;
  g.SW2 = bs / 2; g.P1 = P1; g.P2 = P2; g.ftzero = ftzero;
  g.uniq = p->uniqueness_ratio >= 0 ? p->uniqueness_ratio : 10;
  g.d12 = p->disp12_max_diff > 0 ? p->disp12_max_diff : 1;
  g.fullDP = p->mode == SBM_SGBM_MODE_HH;
  g.reading = env_switch("SBM_CV_READING", 0);
  const bool speckle = p->speckle_window_size > 0;
  const size_t npix = (size_t)width * height;
  const size_t pair_cs = g.W1 >= 1 ? (size_t)g.W1 * height * g.D * sizeof(int16_t) : 0;
  const size_t pair_bytes = 2 * pair_cs + npix * sizeof(int16_t) + (speckle ? sgbm_speckle_bytes_per_pair(width, height) : 0);
  const int chunk = (int)std::min<size_t>(n, std::max<size_t>(1, kSgbmChunkBytes / pair_bytes));
  st = ensure_sgbm(h, pair_cs * chunk, (size_t)chunk * npix * sizeof(int16_t), chunk, width, height, speckle);
  if (st != SBM_OK) return st;
  g.n = n;
  h->sg_last = g;
  h->sg_have_last = true;
  h->sg_last_one_chunk = chunk == n;

  const bool prof = h->profiling != 0;
  if (prof) {
    for (int i = 0; i < 6; i++)
      if (!h->sg_ev[i]) HIPCHK(h, hipEventCreate(&h->sg_ev[i]));
    for (int i = 0; i < 6; i++) h->sg_ms[i] = 0.f;
  }
  auto mark = [&](int i) -> hipError_t { return prof ? hipEventRecord(h->sg_ev[i], h->stream) : hipSuccess; };
  auto lap = [&](int a, int b, int slot) -> hipError_t {
    float ms = 0.f;
    hipError_t e = hipEventSynchronize(h->sg_ev[b]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, h->sg_ev[a], h->sg_ev[b]);
    h->sg_ms[slot] += ms;
    return e;
  };
  const uint8_t* dl = (const uint8_t*)d_left;
  const uint8_t* dr = (const uint8_t*)d_right;
  const int inv = (g.minD - 1) * 16;
  const int max_diff = (int)std::min<long>(16L * p->speckle_range, 1L << 17);
  // every stage, the median and the speckle filter included, runs chunk by chunk
  for (int c0 = 0; c0 < n; c0 += chunk) {
    SgbmGeom gc = g;
    gc.n = std::min(chunk, n - c0);
    int16_t* out = (int16_t*)d_disp + (size_t)c0 * npix;
    HIPCHK(h, mark(0));
    if (pair_cs) {
      HIPCHK(h, launch_sgbm_cost(dl + (size_t)c0 * npix, dr + (size_t)c0 * npix, h->sg_S, h->sg_C, gc, h->stream));
      HIPCHK(h, mark(1));
      HIPCHK(h, launch_sgbm_paths(h->sg_C, h->sg_S, gc, h->stream));
      HIPCHK(h, mark(2));
      HIPCHK(h, launch_sgbm_select(h->sg_S, h->sg_pre, gc, h->stream));
    } else {   // no computable column: every pixel is invalid (the median and the speckle filter keep it so)
      HIPCHK(h, mark(1));
      HIPCHK(h, mark(2));
      HIPCHK(h, launch_sgbm_fill(h->sg_pre, (size_t)gc.n * npix, inv, h->stream));
    }
    HIPCHK(h, mark(3));
    if (g.reading & kReadSgbmNoMedian)
      HIPCHK(h, hipMemcpyAsync(out, h->sg_pre, (size_t)gc.n * npix * sizeof(int16_t), hipMemcpyDeviceToDevice, h->stream));
    else
      HIPCHK(h, launch_sgbm_median(h->sg_pre, out, gc.n, width, height, h->stream));
    HIPCHK(h, mark(4));
    if (speckle) {
      // the block matcher's filter, with cv::StereoSGBM's arguments: newVal = (minD - 1) * 16, maxDiff = 16 * speckleRange (the
      // block matcher's own x16 reading bit does not apply here)
      Geom sg;
      memset(&sg, 0, sizeof(sg));
      sg.W = width; sg.H = height; sg.n = gc.n; sg.filtered = inv; sg.reading = 0;
      HIPCHK(h, launch_speckle(out, h->sg_spk_runs, h->sg_spk_nheads, h->sg_spk_seam, h->sg_spk_nseam, sg, p->speckle_window_size,
                               max_diff, h->stream));
    }
    HIPCHK(h, mark(5));
    if (prof) {
      HIPCHK(h, lap(0, 1, 0)); HIPCHK(h, lap(1, 2, 1)); HIPCHK(h, lap(2, 3, 2)); HIPCHK(h, lap(3, 4, 3)); HIPCHK(h, lap(4, 5, 4));
      HIPCHK(h, lap(0, 5, 5));
    }
  }
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_sgbm_compute(sbm_handle* h, const sbm_sgbm_params* p, const uint8_t* left, size_t left_stride, const uint8_t* right,
                     size_t right_stride, int width, int height, int16_t* disp, size_t disp_stride) {
  if (!h || !p || !left || !right || !disp) return SBM_ERR_NULL;
  int st = sbm_sgbm_params_validate(p, width, height);
  if (st != SBM_OK) return st;
  if (left_stride < (size_t)width || right_stride < (size_t)width || disp_stride < (size_t)width * 2) return SBM_ERR_SIZE;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = ensure_staging(h, 1, width, height);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpy2DAsync(h->st_l, width, left, left_stride, width, height, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpy2DAsync(h->st_r, width, right, right_stride, width, height, hipMemcpyHostToDevice, h->stream));
  st = sbm_sgbm_compute_device(h, p, 1, h->st_l, h->st_r, width, height, h->st_d, 0);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpy2DAsync(disp, disp_stride, h->st_d, (size_t)width * 2, (size_t)width * 2, height, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_gftt_eig(sbm_handle* h, const uint8_t* img, size_t img_stride, int width, int height, uint16_t* eig, size_t eig_stride,
                 uint32_t* max_out) {
  if (!h || !img || !eig) return SBM_ERR_NULL;
  if (width < 3 || height < 5 || width > 1023 || height > 511) return SBM_ERR_SIZE;
  if (img_stride < (size_t)width || eig_stride < (size_t)width * 2) return SBM_ERR_SIZE;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  int st = ensure_staging(h, 1, width, height);
  if (st != SBM_OK) return st;
  // st_l: image, st_d: map, st_r: the Max word
  HIPCHK(h, hipMemcpy2DAsync(h->st_l, width, img, img_stride, width, height, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, launch_gftt_eig(h->st_l, reinterpret_cast<uint16_t*>(h->st_d), reinterpret_cast<unsigned*>(h->st_r), 1, width, height, h->stream));
  HIPCHK(h, hipMemcpy2DAsync(eig, eig_stride, h->st_d, (size_t)width * 2, (size_t)width * 2, height, hipMemcpyDeviceToHost, h->stream));
  uint32_t mx = 0;
  HIPCHK(h, hipMemcpyAsync(&mx, h->st_r, sizeof(mx), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (max_out) *max_out = mx;
  return SBM_OK;
}

int sbm_gftt_eig_device(sbm_handle* h, int n, const void* d_img, int width, int height, void* d_eig, void* d_max, int sync) {
  if (!h || !d_img || !d_eig || !d_max) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (width < 3 || height < 5 || width > 1023 || height > 511) return SBM_ERR_SIZE;
  if (n > 65535) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, launch_gftt_eig((const uint8_t*)d_img, (uint16_t*)d_eig, (unsigned*)d_max, n, width, height, h->stream));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

// ---- keypoint selection of generateKeypoints2 (GFTT.cpp:41-170) ---------------------------------------------------------------
void sbm_gftt_select_params_default(sbm_gftt_select_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->max_features = 1500;
  p->quality_level = 0.01;
  p->min_distance = 7.0;
  p->block_size = 3;
}

int sbm_gftt_select_params_validate(const sbm_gftt_select_params* p, int width, int height) {
  if (!p) return SBM_ERR_NULL;
  if (width < 3 || height < 3) return SBM_ERR_SIZE;
  if (width > kGftSelWMax || height > kGftSelWMax) return SBM_ERR_UNSUPPORTED;
  if (!std::isfinite(p->quality_level) || p->quality_level < 0) return SBM_ERR_UNSUPPORTED;
  if (!std::isfinite(p->min_distance) || p->min_distance < 0 || p->min_distance > 255) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

// Enqueues the selection of n dense maps; with tm (profiling) the eig event tm[0] is already recorded by the caller.
static int gftt_select_enqueue(sbm_handle* h, int n, const void* d_eig, const void* d_max, int width, int height,
                               const sbm_gftt_select_params* p, void* d_kpts, void* d_count) {
  const GftSelPlan pl = gftt_select_plan(width, height, p->max_features, p->quality_level, p->min_distance);
  // the global-table kernel works through the images in chunks whose tables stay within 2 GiB
  int chunk = n;
  if (pl.global_table) {
    chunk = (int)std::min<size_t>(n, std::max<size_t>(1, ((size_t)2 << 30) / pl.table_bytes_per_image));
    const size_t bytes = pl.table_bytes_per_image * chunk;
    if (bytes > h->gs_tab_bytes) {
      HIPCHK(h, hipStreamSynchronize(h->stream));
      hipFree(h->gs_tab);
      h->gs_tab = nullptr; h->gs_tab_bytes = 0;
      HIPCHK(h, hipMalloc((void**)&h->gs_tab, bytes));
      h->gs_tab_bytes = bytes;
    }
  }
  for (int c0 = 0; c0 < n; c0 += chunk)
    HIPCHK(h, launch_gftt_select((const uint16_t*)d_eig, (const unsigned*)d_max, (float*)d_kpts, (int*)d_count, h->gs_tab, pl, c0,
                                 std::min(chunk, n - c0), h->stream));
  return SBM_OK;
}

static int gftt_select_run(sbm_handle* h, int n, const void* d_img, const void* d_eig, const void* d_max, int width, int height,
                           const sbm_gftt_select_params* p, void* d_kpts, void* d_count, int sync) {
  const bool prof = h->profiling != 0;
  if (prof) {
    for (int i = 0; i < 3; i++)
      if (!h->gs_ev[i]) HIPCHK(h, hipEventCreate(&h->gs_ev[i]));
    HIPCHK(h, hipEventRecord(h->gs_ev[0], h->stream));
  }
  if (d_img)
    HIPCHK(h, launch_gftt_eig((const uint8_t*)d_img, (uint16_t*)d_eig, (unsigned*)d_max, n, width, height, h->stream));
  if (prof) HIPCHK(h, hipEventRecord(h->gs_ev[1], h->stream));
  const int st = gftt_select_enqueue(h, n, d_eig, d_max, width, height, p, d_kpts, d_count);
  if (st != SBM_OK) return st;
  if (prof) {
    HIPCHK(h, hipEventRecord(h->gs_ev[2], h->stream));
    HIPCHK(h, hipEventSynchronize(h->gs_ev[2]));
    HIPCHK(h, hipEventElapsedTime(&h->gs_ms[0], h->gs_ev[0], h->gs_ev[1]));
    HIPCHK(h, hipEventElapsedTime(&h->gs_ms[1], h->gs_ev[1], h->gs_ev[2]));
    HIPCHK(h, hipEventElapsedTime(&h->gs_ms[2], h->gs_ev[0], h->gs_ev[2]));
  }
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_gftt_select_device(sbm_handle* h, int n, const void* d_eig, const void* d_max, int width, int height,
                           const sbm_gftt_select_params* p, void* d_kpts, void* d_count, int sync) {
  if (!h || !p || !d_eig || !d_kpts || !d_count) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  const int st = sbm_gftt_select_params_validate(p, width, height);
  if (st != SBM_OK) return st;
  if (n > 65535) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  return gftt_select_run(h, n, nullptr, d_eig, d_max, width, height, p, d_kpts, d_count, sync);
}

int sbm_gftt_detect_device(sbm_handle* h, int n, const void* d_img, int width, int height, const sbm_gftt_select_params* p,
                           void* d_eig, void* d_max, void* d_kpts, void* d_count, int sync) {
  if (!h || !p || !d_img || !d_eig || !d_max || !d_kpts || !d_count) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (width < 3 || height < 5 || width > 1023 || height > 511) return SBM_ERR_SIZE;   // the eigenvalue map's limits
  const int st = sbm_gftt_select_params_validate(p, width, height);
  if (st != SBM_OK) return st;
  if (n > 65535) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  return gftt_select_run(h, n, d_img, d_eig, d_max, width, height, p, d_kpts, d_count, sync);
}

int sbm_gftt_select(sbm_handle* h, const uint16_t* eig, size_t eig_stride, int width, int height, uint16_t max_eig,
                    const sbm_gftt_select_params* p, float* kpts, size_t capacity, int* count) {
  if (!h || !p || !eig || !kpts || !count) return SBM_ERR_NULL;
  int st = sbm_gftt_select_params_validate(p, width, height);
  if (st != SBM_OK) return st;
  const size_t cap = p->max_features > 0 ? (size_t)p->max_features : (size_t)(width - 2) * (height - 2);
  if (eig_stride < (size_t)width * 2 || capacity < cap) return SBM_ERR_SIZE;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = ensure_staging(h, 1, width, height);
  if (st != SBM_OK) return st;
  const size_t out_bytes = cap * 2 * sizeof(float) + 16;   // points, then the count
  if (out_bytes > h->gs_out_bytes) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    hipFree(h->gs_out);
    h->gs_out = nullptr; h->gs_out_bytes = 0;
    HIPCHK(h, hipMalloc(&h->gs_out, out_bytes));
    h->gs_out_bytes = out_bytes;
  }
  // st_d: the map, st_r: the Max word
  const uint32_t mx = max_eig;
  HIPCHK(h, hipMemcpy2DAsync(h->st_d, (size_t)width * 2, eig, eig_stride, (size_t)width * 2, height, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->st_r, &mx, sizeof(mx), hipMemcpyHostToDevice, h->stream));
  float* d_k = (float*)h->gs_out;
  int* d_n = (int*)((char*)h->gs_out + cap * 2 * sizeof(float));
  st = gftt_select_run(h, 1, nullptr, h->st_d, h->st_r, width, height, p, d_k, d_n, 0);
  if (st != SBM_OK) {
    hipStreamSynchronize(h->stream);   // `mx` is read by an enqueued copy
    return st;
  }
  int k = 0;
  HIPCHK(h, hipMemcpyAsync(&k, d_n, sizeof(k), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (k > 0) HIPCHK(h, hipMemcpy(kpts, d_k, (size_t)k * 2 * sizeof(float), hipMemcpyDeviceToHost));
  *count = k;
  return SBM_OK;
}

// ---- ORB descriptors of computeDescriptor (CvORB.cpp) --------------------------------------------------------------------------
void sbm_orb_params_default(sbm_orb_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->edge_threshold = 19;
  p->angle = -1.f;
  p->blur_ksize = 7;
  p->blur_sigma = 2.0;
}

int sbm_orb_params_validate(const sbm_orb_params* p) {
  if (!p) return SBM_ERR_NULL;
  if (p->edge_threshold < 18 || p->edge_threshold > 4096) return SBM_ERR_UNSUPPORTED;
  if (!std::isfinite(p->angle)) return SBM_ERR_UNSUPPORTED;
  if (p->blur_ksize != 7 || p->blur_sigma != 2.0) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

// The 512 sample offsets of computeOrbDescriptors' GET_VALUE, as the reference evaluates them: float products and differences
// without contraction (hipcc contracts by default), cvRound half to even.
static int orb_offsets(const int* pattern, float angle_deg, int W, OrbOffsets* o) {
#pragma clang fp contract(off)
  for (int i = 0; i < 1024; i++)
    if (pattern[i] < -13 || pattern[i] > 13) return SBM_ERR_UNSUPPORTED;
  const float angle = angle_deg * (float)(3.14159265358979323846 / 180.f);
  const float a = (float)cos((double)angle), b = (float)sin((double)angle);
  for (int i = 0; i < 512; i++) {
    const float px = (float)pattern[2 * i], py = (float)pattern[2 * i + 1];
    const float x = px * a - py * b, y = px * b + py * a;
    o->off[i] = (int)std::nearbyint(y) * W + (int)std::nearbyint(x);
  }
  return SBM_OK;
}

static int orb_check(int n, int width, int height, int cap, const void* d_kpts, const void* d_kpts_out, const void* d_desc) {
  if (n <= 0) return SBM_ERR_BATCH;
  if (width < 1 || height < 1 || width > 8192 || height > 8192 || cap < 1) return SBM_ERR_SIZE;
  if (n > 65535) return SBM_ERR_UNSUPPORTED;
  if (((uintptr_t)d_kpts & 7) || ((uintptr_t)d_kpts_out & 7) || ((uintptr_t)d_desc & 3)) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

// Enqueues compaction, blur and descriptors; with profiling, synchronises on its own events (tm[0..2] of the call).
static int orb_run(sbm_handle* h, int n, const void* d_img, int width, int height, int cap, const void* d_kpts, const void* d_count,
                   const OrbOffsets& offs, const sbm_orb_params* p, void* d_kpts_out, void* d_count_out, void* d_desc,
                   void* d_blur, int sync) {
  const bool prof = h->profiling != 0;
  float ms[3] = {0.f, 0.f, 0.f};
  if (prof)
    for (int i = 0; i < 3; i++)
      if (!h->or_ev[i]) HIPCHK(h, hipEventCreate(&h->or_ev[i]));
  auto lap = [&](int i, int j, float* acc) -> int {   // acc += elapsed(or_ev[i], or_ev[j]) once or_ev[j] is reached
    HIPCHK(h, hipEventSynchronize(h->or_ev[j]));
    float t = 0.f;
    HIPCHK(h, hipEventElapsedTime(&t, h->or_ev[i], h->or_ev[j]));
    *acc += t;
    return SBM_OK;
  };
  const int edge = p->edge_threshold;
  if (prof) HIPCHK(h, hipEventRecord(h->or_ev[0], h->stream));
  HIPCHK(h, launch_orb_compact((const float*)d_kpts, (const int*)d_count, (float*)d_kpts_out, (int*)d_count_out, n, cap, width,
                               height, edge, h->stream));
  if (prof) {
    HIPCHK(h, hipEventRecord(h->or_ev[1], h->stream));
    const int st = lap(0, 1, &ms[1]);
    if (st != SBM_OK) return st;
  }
  if (width > 2 * edge && height > 2 * edge) {   // else every keypoint is gone and nothing needs the blur
    const int reading = env_switch("SBM_CV_READING", 0);
    const size_t plane = (size_t)width * height;
    int chunk = n;
    uint8_t* blur = (uint8_t*)d_blur;
    if (!blur) {
      chunk = (int)std::min<size_t>(n, std::max<size_t>(1, ((size_t)256 << 20) / plane));
      const size_t bytes = plane * chunk;
      if (bytes > h->or_blur_bytes) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        hipFree(h->or_blur);
        h->or_blur = nullptr; h->or_blur_bytes = 0;
        HIPCHK(h, hipMalloc((void**)&h->or_blur, bytes));
        h->or_blur_bytes = bytes;
      }
    }
    for (int c0 = 0; c0 < n; c0 += chunk) {
      const int m = std::min(chunk, n - c0);
      uint8_t* bc = d_blur ? blur + plane * c0 : h->or_blur;
      if (prof) HIPCHK(h, hipEventRecord(h->or_ev[0], h->stream));
      HIPCHK(h, launch_orb_blur((const uint8_t*)d_img + plane * c0, bc, m, width, height, (reading & kReadOrbHalfUp) ? 1 : 0,
                                h->stream));
      if (prof) HIPCHK(h, hipEventRecord(h->or_ev[1], h->stream));
      HIPCHK(h, launch_orb_desc(bc, (const float*)d_kpts_out, (const int*)d_count_out, (uint8_t*)d_desc, c0, m, cap, width, height,
                                offs, h->stream));
      if (prof) {
        HIPCHK(h, hipEventRecord(h->or_ev[2], h->stream));
        int st = lap(0, 1, &ms[0]);
        if (st == SBM_OK) st = lap(1, 2, &ms[1]);
        if (st != SBM_OK) return st;
      }
    }
  }
  if (prof) {
    ms[2] = ms[0] + ms[1];
    for (int i = 0; i < 3; i++) h->or_ms[i] = ms[i];
  }
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_orb_describe_device(sbm_handle* h, int n, const void* d_img, int width, int height, int cap, const void* d_kpts,
                            const void* d_count, const int* pattern, const sbm_orb_params* p, void* d_kpts_out, void* d_count_out,
                            void* d_desc, void* d_blur, int sync) {
  if (!h || !d_img || !d_kpts || !d_count || !pattern || !p || !d_kpts_out || !d_count_out || !d_desc) return SBM_ERR_NULL;
  int st = sbm_orb_params_validate(p);
  if (st == SBM_OK) st = orb_check(n, width, height, cap, d_kpts, d_kpts_out, d_desc);
  if (st != SBM_OK) return st;
  OrbOffsets offs;
  st = orb_offsets(pattern, p->angle, width, &offs);
  if (st != SBM_OK) return st;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  return orb_run(h, n, d_img, width, height, cap, d_kpts, d_count, offs, p, d_kpts_out, d_count_out, d_desc, d_blur, sync);
}

int sbm_orb_features_device(sbm_handle* h, int n, const void* d_img, int width, int height, const sbm_gftt_select_params* gp,
                            const int* pattern, const sbm_orb_params* p, void* d_eig, void* d_max, void* d_kpts, void* d_count,
                            void* d_desc, void* d_blur, int sync) {
  if (!h || !gp || !d_img || !d_eig || !d_max || !d_kpts || !d_count || !pattern || !p || !d_desc) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (width < 3 || height < 5 || width > 1023 || height > 511) return SBM_ERR_SIZE;   // the eigenvalue map's limits
  int st = sbm_gftt_select_params_validate(gp, width, height);
  if (st == SBM_OK) st = sbm_orb_params_validate(p);
  const int cap = gp->max_features > 0 ? gp->max_features : (width - 2) * (height - 2);
  if (st == SBM_OK) st = orb_check(n, width, height, cap, d_kpts, d_kpts, d_desc);
  if (st != SBM_OK) return st;
  OrbOffsets offs;
  st = orb_offsets(pattern, p->angle, width, &offs);
  if (st != SBM_OK) return st;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = gftt_select_run(h, n, d_img, d_eig, d_max, width, height, gp, d_kpts, d_count, 0);
  if (st != SBM_OK) return st;
  return orb_run(h, n, d_img, width, height, cap, d_kpts, d_count, offs, p, d_kpts, d_count, d_desc, d_blur, sync);
}

int sbm_orb_describe(sbm_handle* h, const uint8_t* img, size_t img_stride, int width, int height, const float* kpts, int count,
                     const int* pattern, const sbm_orb_params* p, float* kpts_out, int* count_out, uint8_t* desc) {
  if (!h || !img || !pattern || !p || !count_out || (count > 0 && (!kpts || !kpts_out || !desc))) return SBM_ERR_NULL;
  if (count < 0 || img_stride < (size_t)width) return SBM_ERR_SIZE;
  const int cap = std::max(count, 1);
  int st = sbm_orb_params_validate(p);
  if (st == SBM_OK) st = orb_check(1, width, height, cap, nullptr, nullptr, nullptr);
  if (st != SBM_OK) return st;
  OrbOffsets offs;
  st = orb_offsets(pattern, p->angle, width, &offs);
  if (st != SBM_OK) return st;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = ensure_staging(h, 1, width, height);
  if (st != SBM_OK) return st;
  const size_t kb = (size_t)cap * 8, out_bytes = 2 * kb + (size_t)cap * 32 + 16;   // points in, points out, descriptors, counts
  if (out_bytes > h->or_io_bytes) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    hipFree(h->or_io);
    h->or_io = nullptr; h->or_io_bytes = 0;
    HIPCHK(h, hipMalloc(&h->or_io, out_bytes));
    h->or_io_bytes = out_bytes;
  }
  char* io = (char*)h->or_io;
  float* d_ki = (float*)io;
  float* d_ko = (float*)(io + kb);
  uint8_t* d_de = (uint8_t*)(io + 2 * kb);
  int* d_n = (int*)(io + 2 * kb + (size_t)cap * 32);
  HIPCHK(h, hipMemcpy2DAsync(h->st_l, width, img, img_stride, width, height, hipMemcpyHostToDevice, h->stream));
  if (count > 0) HIPCHK(h, hipMemcpyAsync(d_ki, kpts, (size_t)count * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_n, &count, sizeof(int), hipMemcpyHostToDevice, h->stream));
  st = orb_run(h, 1, h->st_l, width, height, cap, d_ki, d_n, offs, p, d_ko, d_n + 1, d_de, nullptr, 0);
  if (st != SBM_OK) {
    hipStreamSynchronize(h->stream);   // `count` is read by an enqueued copy
    return st;
  }
  int k = 0;
  HIPCHK(h, hipMemcpyAsync(&k, d_n + 1, sizeof(k), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (k > 0) {
    HIPCHK(h, hipMemcpy(kpts_out, d_ko, (size_t)k * 8, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(desc, d_de, (size_t)k * 32, hipMemcpyDeviceToHost));
  }
  *count_out = k;
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
  if (!strcmp(name, "prefilter")) *ms = h->ms_prefilter;
  else if (!strcmp(name, "sad")) *ms = h->ms_sad;
  else if (!strcmp(name, "border")) *ms = h->ms_border;
  else if (!strcmp(name, "lrcheck")) *ms = h->ms_lr;
  else if (!strcmp(name, "speckle")) *ms = h->ms_speckle;
  else if (!strcmp(name, "total")) *ms = h->ms_total;
  else if (!strncmp(name, "sgbm_", 5)) {
    static const char* const kSg[6] = {"sgbm_cost", "sgbm_aggregate", "sgbm_select", "sgbm_median", "sgbm_speckle", "sgbm_total"};
    int i = 0;
    while (i < 6 && strcmp(name, kSg[i])) i++;
    if (i == 6) return SBM_ERR_UNSUPPORTED;
    *ms = h->sg_ms[i];
  }
  else if (!strncmp(name, "gftt_select_", 12)) {
    static const char* const kGs[3] = {"gftt_select_eig", "gftt_select_select", "gftt_select_total"};
    int i = 0;
    while (i < 3 && strcmp(name, kGs[i])) i++;
    if (i == 3) return SBM_ERR_UNSUPPORTED;
    *ms = h->gs_ms[i];
  }
  else if (!strncmp(name, "orb_", 4)) {
    static const char* const kOr[3] = {"orb_blur", "orb_desc", "orb_total"};
    int i = 0;
    while (i < 3 && strcmp(name, kOr[i])) i++;
    if (i == 3) return SBM_ERR_UNSUPPORTED;
    *ms = h->or_ms[i];
  }
  else return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

int sbm_last_kernel_name(sbm_handle* h, char* dst, size_t dst_bytes) {
  if (!h || !dst || dst_bytes == 0) return SBM_ERR_NULL;
  snprintf(dst, dst_bytes, "%s", h->last_kernel);
  return SBM_OK;
}

int sbm_debug_fetch(sbm_handle* h, int which, void* dst, size_t dst_bytes) {
  if (!h || !dst) return SBM_ERR_NULL;
  if (which >= 4 && which <= 6) {   // the last semi-global matcher call
    if (!h->sg_have_last) return SBM_ERR_UNSUPPORTED;
    const SgbmGeom& g = h->sg_last;
    DeviceScope dscope(h->device);
    HIPCHK(h, dscope.enter());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!h->sg_last_one_chunk) return SBM_ERR_UNSUPPORTED;
    if (which == 6) {
      const size_t bytes = (size_t)g.n * g.W * g.H * sizeof(int16_t);
      if (dst_bytes < bytes) return SBM_ERR_SIZE;
      HIPCHK(h, hipMemcpy(dst, h->sg_pre, bytes, hipMemcpyDeviceToHost));
      return SBM_OK;
    }
    if (g.W1 < 1) return SBM_ERR_UNSUPPORTED;
    const size_t bytes = (size_t)g.n * g.H * g.W1 * g.D * sizeof(int16_t);
    if (dst_bytes < bytes) return SBM_ERR_SIZE;
    HIPCHK(h, hipMemcpy(dst, which == 4 ? h->sg_C : h->sg_S, bytes, hipMemcpyDeviceToHost));
    return SBM_OK;
  }
  if (!h->have_last) return SBM_ERR_UNSUPPORTED;
  const Geom& g = h->last;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const size_t npix = (size_t)g.n * g.W * g.H;
  if (which == 0 || which == 1) {
    if (dst_bytes < npix) return SBM_ERR_SIZE;
    const uint8_t* src = which == 0 ? h->pf_l : h->pf_r;
    HIPCHK(h, hipMemcpy2D(dst, g.W, src + g.padl, g.pitch, g.W, (size_t)g.n * g.H, hipMemcpyDeviceToHost));
    uint8_t* d = (uint8_t*)dst;
    for (size_t i = 0; i < npix; i++) d[i] = (uint8_t)((d[i] - kPfBias) >> g.pfshift);
    return SBM_OK;
  }
  if (which == 2) {
    if (!h->cost) return SBM_ERR_UNSUPPORTED;
    if (dst_bytes < npix * sizeof(int32_t)) return SBM_ERR_SIZE;
    if (g.cost16) {
      uint16_t* tmp = (uint16_t*)malloc(npix * sizeof(uint16_t));
      if (!tmp) return SBM_ERR_NOMEM;
      hipError_t e = hipMemcpy(tmp, h->cost, npix * sizeof(uint16_t), hipMemcpyDeviceToHost);
      if (e == hipSuccess)
        for (size_t i = 0; i < npix; i++) ((int32_t*)dst)[i] = tmp[i];
      free(tmp);
      HIPCHK(h, e);
      return SBM_OK;
    }
    HIPCHK(h, hipMemcpy(dst, h->cost, npix * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SBM_OK;
  }
  if (which == 3) {
    if (dst_bytes < npix * sizeof(int16_t)) return SBM_ERR_SIZE;
    HIPCHK(h, hipMemcpy(dst, h->disp_pre, npix * sizeof(int16_t), hipMemcpyDeviceToHost));
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
  return SBM_ERR_UNSUPPORTED;
}

static int ensure_staging(sbm_handle* h, int n, int W, int H) {
  if (n <= h->st_n && W == h->st_W && H == h->st_H && h->st_l) return SBM_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  free_staging(h);
  const size_t npix = (size_t)n * W * H;
  HIPCHK(h, hipMalloc((void**)&h->st_l, npix + 64));
  HIPCHK(h, hipMalloc((void**)&h->st_r, npix + 64));
  HIPCHK(h, hipMalloc((void**)&h->st_d, npix * sizeof(int16_t)));
  h->st_n = n; h->st_W = W; h->st_H = H;
  return SBM_OK;
}

static int ensure_pipe(sbm_handle* h) {
  if (h->pipe_ok) return SBM_OK;
  HIPCHK(h, hipStreamCreateWithFlags(&h->stream_in, hipStreamNonBlocking));
  HIPCHK(h, hipStreamCreateWithFlags(&h->stream_out, hipStreamNonBlocking));
  for (int i = 0; i < sbm_handle::kChunks; i++) {
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_in[i], hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&h->ev_done[i], hipEventDisableTiming));
  }
  h->pipe_ok = true;
  return SBM_OK;
}

// Large dense host batches: chunks of pairs flow through three streams -- H2D copies, compute, D2H copies -- so the GPU
// works on chunk k while chunk k+1 arrives and chunk k-1 leaves. With pageable caller memory the copies themselves still
// run one after the other on the calling thread (the runtime stages them), but the compute disappears behind them; with
// pinned (hipHostMalloc / hipHostRegister) caller memory the two copy directions overlap as well.
// maps [i0, i1) device -> caller, one transfer per run of maps that are contiguous in the caller's memory
static hipError_t copy_out_runs(sbm_handle* h, int16_t* const* disp, int i0, int i1, size_t npix1) {
  for (int i = i0; i < i1;) {
    int j = i + 1;
    while (j < i1 && disp[j] == disp[j - 1] + npix1) j++;
    const hipError_t e = hipMemcpyAsync(disp[i], h->st_d + i * npix1, (size_t)(j - i) * npix1 * 2, hipMemcpyDeviceToHost, h->stream_out);
    if (e != hipSuccess) return e;
    i = j;
  }
  return hipSuccess;
}

static int pipelined_enqueue(sbm_handle* h, int n, const uint8_t* const* left, const uint8_t* const* right, int width,
                             int height, int16_t* const* disp) {
  const size_t npix1 = (size_t)width * height;
  // Chunk plan. Small chunks overlap more of the transfers but run the kernels on part-filled launches (8 KITTI pairs cost
  // 0.36 ms on the device, 64 pairs 1.2 ms), so: a small FIRST chunk (the computation starts after one short transfer), a
  // small LAST one (only its computation and its maps are left when the inputs have arrived) and large ones in between.
  // Measured on 64 KITTI pairs from pinned memory (profiles/r03_host_feed.json). SBM_HOST_CHUNK=<pairs>: uniform chunks.
  static const int chunk_env = SBM_TUNE("SBM_HOST_CHUNK", 0);
  int start[sbm_handle::kChunks + 1];
  int nch = 0;
  start[0] = 0;
  if (chunk_env > 0 || n < 32) {
    int chunk = chunk_env > 0 ? chunk_env : 8;
    while ((n + chunk - 1) / chunk > sbm_handle::kChunks) chunk *= 2;
    for (int i = 0; i < n; i += chunk) start[++nch] = std::min(n, i + chunk);
  } else {
    const int edge = 8, mid = n - 2 * edge;
    int nmid = std::max(1, (mid + 23) / 24);                     // middle chunks of at most 24 pairs
    nmid = std::min(nmid, sbm_handle::kChunks - 2);
    start[++nch] = edge;
    for (int k = 1; k <= nmid; k++) start[++nch] = edge + (int)((long)mid * k / nmid);
    start[++nch] = n;
  }
  for (int k = 0; k < nch; k++) {
    const int i0 = start[k], cnt = start[k + 1] - i0;
    // images that follow each other in the caller's memory (one (n,H,W) array) travel as one transfer per run
    for (int i = i0; i < i0 + cnt;) {
      int j = i + 1;
      while (j < i0 + cnt && left[j] == left[j - 1] + npix1) j++;
      HIPCHK(h, hipMemcpyAsync(h->st_l + i * npix1, left[i], (size_t)(j - i) * npix1, hipMemcpyHostToDevice, h->stream_in));
      i = j;
    }
    for (int i = i0; i < i0 + cnt;) {
      int j = i + 1;
      while (j < i0 + cnt && right[j] == right[j - 1] + npix1) j++;
      HIPCHK(h, hipMemcpyAsync(h->st_r + i * npix1, right[i], (size_t)(j - i) * npix1, hipMemcpyHostToDevice, h->stream_in));
      i = j;
    }
    HIPCHK(h, hipEventRecord(h->ev_in[k], h->stream_in));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_in[k], 0));
    const int st = sbm_compute_device(h, cnt, h->st_l + i0 * npix1, h->st_r + i0 * npix1, width, height, h->st_d + i0 * npix1, 0);
    if (st != SBM_OK) return st;
    HIPCHK(h, hipEventRecord(h->ev_done[k], h->stream));
    if (k > 0) {   // the previous chunk leaves while this one computes
      HIPCHK(h, hipStreamWaitEvent(h->stream_out, h->ev_done[k - 1], 0));
      HIPCHK(h, copy_out_runs(h, disp, start[k - 1], start[k], npix1));
    }
  }
  HIPCHK(h, hipStreamWaitEvent(h->stream_out, h->ev_done[nch - 1], 0));
  HIPCHK(h, copy_out_runs(h, disp, start[nch - 1], n, npix1));
  return SBM_OK;
}

static int compute_batch_pipelined(sbm_handle* h, int n, const uint8_t* const* left, const uint8_t* const* right, int width,
                                   int height, int16_t* const* disp) {
  int st = ensure_pipe(h);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipStreamSynchronize(h->stream));   // staging buffers of an earlier call are free
  st = pipelined_enqueue(h, n, left, right, width, height, disp);
  // success or not: nothing may still be reading or writing the caller's buffers when this returns
  const hipError_t e1 = hipStreamSynchronize(h->stream_in), e2 = hipStreamSynchronize(h->stream),
                   e3 = hipStreamSynchronize(h->stream_out);
  if (st != SBM_OK) return st;
  HIPCHK(h, e1);
  HIPCHK(h, e2);
  HIPCHK(h, e3);
  return SBM_OK;
}

// ---- asynchronous dense feed -------------------------------------------------------------------------------------
// What a per-GPU feeder thread uses: batch k+1 is submitted (its inputs start crossing PCIe on the H2D stream) while batch k
// computes and batch k-1's maps travel back on the D2H stream. Whole batches, no chunking: the kernels run on full launches
// and in steady state a step costs its slowest leg (profiles/r03_host_feed.json). Caller buffers should be pinned
// (hipHostMalloc / hipHostRegister) -- pageable memory works but the runtime then copies synchronously.
// The runtime executes the copies of all streams in the order they were queued (measured: an H2D transfer queued behind a
// D2H one does not start before it, whatever their streams -- profiles/r03_host_feed.json), and a D2H copy can only run when
// its batch has been computed. So the maps of submission k are queued for their trip home only AFTER the inputs of
// submission k+1 (or when somebody waits for k): the inputs of k+1 then cross PCIe while k computes.
static int fq_flush_pending(sbm_handle* h) {
  if (!h->fq_pending_dst) return SBM_OK;
  const unsigned k = h->fq_submitted - 1u, slot = k & 1u, e = k & 3u;
  HIPCHK(h, hipStreamWaitEvent(h->stream_out, h->ev_fq_done[e], 0));
  HIPCHK(h, hipMemcpyAsync(h->fq_pending_dst, h->fq_d[slot], h->fq_pending_bytes, hipMemcpyDeviceToHost, h->stream_out));
  HIPCHK(h, hipEventRecord(h->ev_fq_out[e], h->stream_out));
  h->fq_pending_dst = nullptr;
  return SBM_OK;
}

int sbm_wait_oldest(sbm_handle* h) {
  if (!h) return SBM_ERR_NULL;
  if (h->fq_waited == h->fq_submitted) return SBM_OK;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  if (h->fq_waited + 1u == h->fq_submitted) {   // the newest submission: its maps may not have been queued yet
    const int st = fq_flush_pending(h);
    if (st != SBM_OK) return st;
  }
  HIPCHK(h, hipEventSynchronize(h->ev_fq_out[h->fq_waited & 3u]));
  h->fq_waited++;
  return SBM_OK;
}

int sbm_submit_dense(sbm_handle* h, int n, const uint8_t* left, const uint8_t* right, int width, int height, int16_t* disp) {
  if (!h || !left || !right || !disp) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  int st = sbm_params_validate(&h->p, width, height);
  if (st != SBM_OK) return st;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = ensure_pipe(h);
  if (st != SBM_OK) return st;
  if (!h->fq_ok) {
    for (int k = 0; k < 4; k++) {
      HIPCHK(h, hipEventCreateWithFlags(&h->ev_fq_in[k], hipEventDisableTiming));
      HIPCHK(h, hipEventCreateWithFlags(&h->ev_fq_done[k], hipEventDisableTiming));
      HIPCHK(h, hipEventCreateWithFlags(&h->ev_fq_out[k], hipEventDisableTiming));
    }
    h->fq_ok = true;
  }
  while (h->fq_submitted - h->fq_waited >= 3u) {   // queue depth: one batch arriving, one computing, one leaving
    st = sbm_wait_oldest(h);
    if (st != SBM_OK) return st;
  }
  const size_t npix = (size_t)n * width * height;
  if (!(n <= h->fq_n && width == h->fq_W && height == h->fq_H && h->fq_l[0])) {
    while (h->fq_waited != h->fq_submitted) {
      st = sbm_wait_oldest(h);
      if (st != SBM_OK) return st;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    free_feed(h);
    for (int k = 0; k < 2; k++) {
      HIPCHK(h, hipMalloc((void**)&h->fq_l[k], npix + 64));
      HIPCHK(h, hipMalloc((void**)&h->fq_r[k], npix + 64));
      HIPCHK(h, hipMalloc((void**)&h->fq_d[k], npix * sizeof(int16_t)));
    }
    h->fq_n = n; h->fq_W = width; h->fq_H = height;
  }
  // submission k uses device staging set k & 1. The set's previous user is submission k-2: its inputs are free once k-2 has
  // computed, its map buffer once k-2's maps have left -- both are stream dependencies, the host never blocks on them.
  const unsigned k = h->fq_submitted, slot = k & 1u, e = k & 3u;
  if (k >= 2 && k - 2 >= h->fq_waited) {
    HIPCHK(h, hipStreamWaitEvent(h->stream_in, h->ev_fq_done[(k - 2) & 3u], 0));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_fq_out[(k - 2) & 3u], 0));
  }
  HIPCHK(h, hipMemcpyAsync(h->fq_l[slot], left, npix, hipMemcpyHostToDevice, h->stream_in));
  HIPCHK(h, hipMemcpyAsync(h->fq_r[slot], right, npix, hipMemcpyHostToDevice, h->stream_in));
  HIPCHK(h, hipEventRecord(h->ev_fq_in[e], h->stream_in));
  st = fq_flush_pending(h);                      // the previous submission's maps: queued behind this one's inputs
  if (st != SBM_OK) return st;
  HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_fq_in[e], 0));
  st = sbm_compute_device(h, n, h->fq_l[slot], h->fq_r[slot], width, height, h->fq_d[slot], 0);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipEventRecord(h->ev_fq_done[e], h->stream));
  h->fq_pending_dst = disp;
  h->fq_pending_bytes = npix * sizeof(int16_t);
  h->fq_submitted++;
  return SBM_OK;
}

// Maps of a small host-buffer call on their way out (the reference's pattern: one 640x480 pair per call, main.cpp:201-216).
// A D2H copy into pageable memory costs the call ~70 us after the last kernel (the runtime stages it: DMA + CPU copy) and the
// stream synchronisation behind it another ~15 (profiles/r05_host_attrib.txt). Instead the last kernel of the call copies the
// maps into pinned, device-mapped host memory and raises a sequence flag there (last workgroup done, system-scope release);
// the host spins on the flag and copies the rows to the caller itself.
// The maps leave in up to kZcChunks contiguous chunks, each with its own arrival counter and flag: the host copies chunk k to
// the caller while the chunks behind it are still crossing PCIe (round 6: the 25 us CPU copy of a 640x480 map used to START
// when the last byte had landed).
constexpr int kZcChunks = 8;
__global__ void __launch_bounds__(256) maps_out_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16, size_t per_chunk, int bpc,
                                                       const int16_t* __restrict__ src_tail, int16_t* __restrict__ dst_tail, int ntail, unsigned* cnt,
                                                       unsigned* flag, unsigned seq) {
  const int c = blockIdx.x / bpc, bi = blockIdx.x - c * bpc;   // chunk, block within the chunk
  const size_t lo = (size_t)c * per_chunk, hi = lo + per_chunk < n16 ? lo + per_chunk : n16;
  for (size_t i = lo + (size_t)bi * 256 + threadIdx.x; i < hi; i += (size_t)bpc * 256) {
    const uint4 v = src[i];
    __builtin_nontemporal_store(v.x, &dst[i].x); __builtin_nontemporal_store(v.y, &dst[i].y);
    __builtin_nontemporal_store(v.z, &dst[i].z); __builtin_nontemporal_store(v.w, &dst[i].w);
  }
  if (blockIdx.x == gridDim.x - 1 && (int)threadIdx.x < ntail) dst_tail[threadIdx.x] = src_tail[threadIdx.x];   // (the last chunk's last block)
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned done = __hip_atomic_fetch_add(cnt + c, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1u;
    if (done == (unsigned)bpc) {
      __hip_atomic_store(cnt + c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence_system();
      __hip_atomic_store(flag + c, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

static int ensure_zc(sbm_handle* h, size_t bytes) {
  if (h->zc_out && h->zc_flag && h->zc_cnt && h->zc_bytes >= bytes) return SBM_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // flag and counter first, the staging last: zc_bytes only ever describes a complete set (a failure half way leaves a state
  // the next call simply completes)
  if (!h->zc_flag) {
    HIPCHK(h, hipHostMalloc((void**)&h->zc_flag, 64, hipHostMallocMapped | hipHostMallocCoherent));
    for (int k = 0; k < kZcChunks; k++) h->zc_flag[k] = 0u;
    h->zc_seq = 0u;
  }
  if (!h->zc_cnt) {
    unsigned* cnt = nullptr;
    HIPCHK(h, hipMalloc((void**)&cnt, 64));
    const hipError_t e = hipMemsetAsync(cnt, 0, 64, h->stream);
    if (e != hipSuccess) {
      hipFree(cnt);
      HIPCHK(h, e);
    }
    h->zc_cnt = cnt;
  }
  if (!(h->zc_out && h->zc_bytes >= bytes)) {
    if (h->zc_out) hipHostFree(h->zc_out);
    h->zc_out = nullptr; h->zc_bytes = 0;
    HIPCHK(h, hipHostMalloc((void**)&h->zc_out, bytes + 64, hipHostMallocMapped | hipHostMallocCoherent));
    h->zc_bytes = bytes;
  }
  return SBM_OK;
}

// queue the copy kernel behind the call's kernels; the maps arrive in h->zc_out chunk by chunk and go to the caller (n dense maps
// of npix1 pixels at disp[i]) as they arrive
static int maps_out_to_caller(sbm_handle* h, const int16_t* d_src, int n, size_t npix1, int16_t* const* disp) {
  const size_t count = (size_t)n * npix1, bytes = count * sizeof(int16_t);
  int st = ensure_zc(h, bytes);
  if (st != SBM_OK) return st;
  const size_t n16 = bytes / 16;
  const int ntail = (int)((bytes - n16 * 16) / 2);
  const unsigned seq = ++h->zc_seq == 0u ? ++h->zc_seq : h->zc_seq;   // (0 is "nothing yet")
  const int nch = (int)std::min<size_t>(kZcChunks, std::max<size_t>(1, bytes >> 16));        // chunks of at least 64 KB
  const size_t per_chunk = (n16 + nch - 1) / nch;
  const int bpc = (int)std::min<size_t>(256 / nch, std::max<size_t>(1, (per_chunk + 511) / 512));   // blocks per chunk
  hipLaunchKernelGGL(maps_out_kernel, dim3(nch * bpc), dim3(256), 0, h->stream, reinterpret_cast<const uint4*>(d_src), reinterpret_cast<uint4*>(h->zc_out), n16,
                     per_chunk, bpc, d_src + n16 * 8, h->zc_out + n16 * 8, ntail, h->zc_cnt, h->zc_flag, seq);
  HIPCHK(h, hipGetLastError());
  // Poll the chunk flags in order: a short pure spin (a one-pair call ends within tens of microseconds of the launch), then spin
  // with yields so that a loaded host or many engines driven from many threads do not burn a core each, and after 2 ms the
  // runtime's own wait -- also the way out when the stream has failed and the flags will never be raised.
  const auto t0 = std::chrono::steady_clock::now();
  bool synced = false;
  size_t done = 0;   // int16 elements already with the caller
  for (int c = 0; c < nch; c++) {
    unsigned spins = 0;
    while (!synced && __atomic_load_n(h->zc_flag + c, __ATOMIC_ACQUIRE) != seq) {
      cpu_relax();
      if ((++spins & 0xffu) == 0u) {
        const auto dt = std::chrono::steady_clock::now() - t0;
        if (dt > std::chrono::milliseconds(2)) {
          HIPCHK(h, hipStreamSynchronize(h->stream));
          synced = true;
        } else if (dt > std::chrono::microseconds(150)) {
          std::this_thread::yield();
        }
      }
    }
    // elements [done, end) have landed: hand them to the maps they belong to
    const size_t end = c == nch - 1 ? count : std::min(count, (size_t)(c + 1) * per_chunk * 8);
    while (done < end) {
      const size_t i = done / npix1, off = done - i * npix1, len = std::min(end - done, npix1 - off);
      memcpy(disp[i] + off, h->zc_out + done, len * sizeof(int16_t));
      done += len;
    }
  }
  return SBM_OK;
}

// One dense host batch over several engines -- the C++ caller's form of "pair batches shard across the GPUs of a node"
// (one process, one stream set per device): handle k takes the contiguous block of pairs
// [n k / K, n (k + 1) / K), cut into at most two submissions of its asynchronous feed so that the second half's inputs cross
// PCIe while the first half computes; every device's submissions are queued before anything is waited for, so the devices run
// side by side from ONE host thread. Pairs are independent: no data-path collective, the blocks' maps land in `disp` in place.
int sbm_compute_batch_multi(sbm_handle* const* handles, int n_handles, int n, const uint8_t* left, const uint8_t* right,
                            int width, int height, int16_t* disp) {
  if (!handles || !left || !right || !disp) return SBM_ERR_NULL;
  if (n_handles <= 0 || n <= 0) return SBM_ERR_BATCH;
  for (int k = 0; k < n_handles; k++) {
    if (!handles[k]) return SBM_ERR_NULL;
    for (int j = 0; j < k; j++)
      if (handles[j] == handles[k]) return SBM_ERR_BATCH;   // a handle owns one feed: the same one twice would interleave its staging sets
  }
  const size_t npix1 = (size_t)width * height;
  int first_err = SBM_OK;
  for (int part = 0; part < 2 && first_err == SBM_OK; part++)
    for (int k = 0; k < n_handles && first_err == SBM_OK; k++) {
      const long b0 = (long)n * k / n_handles, b1 = (long)n * (k + 1) / n_handles;   // this engine's block
      const long half = (b1 - b0 + 1) / 2;
      const long c0 = part == 0 ? b0 : b0 + half, c1 = part == 0 ? b0 + half : b1;
      if (c1 <= c0) continue;
      first_err = sbm_submit_dense(handles[k], (int)(c1 - c0), left + c0 * npix1, right + c0 * npix1, width, height, disp + c0 * npix1);
    }
  // drain every engine even after a failure: what was queued writes into `disp`, which the caller may free on return
  for (int k = 0; k < n_handles; k++) {
    const int st = sbm_synchronize(handles[k]);
    if (first_err == SBM_OK) first_err = st;
  }
  return first_err;
}

int sbm_compute_batch(sbm_handle* h, int n, const uint8_t* const* left, size_t left_stride, const uint8_t* const* right,
                      size_t right_stride, int width, int height, int16_t* const* disp, size_t disp_stride) {
  if (!h || !left || !right || !disp) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  int st = sbm_params_validate(&h->p, width, height);
  if (st != SBM_OK) return st;
  if (left_stride < (size_t)width || right_stride < (size_t)width || disp_stride < (size_t)width * 2) return SBM_ERR_SIZE;
  for (int i = 0; i < n; i++)
    if (!left[i] || !right[i] || !disp[i]) return SBM_ERR_NULL;
  HP_BEGIN();
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = ensure_staging(h, n, width, height);
  if (st != SBM_OK) return st;
  HP(0);
  const size_t npix1 = (size_t)width * height;
  // Dense caller images (stride == width, what cv::Mat::isContinuous() gives) go through plain 1-D copies. Strided ones
  // are packed row by row into pinned staging on the CPU: a 2-D copy from pageable memory degenerates into one small
  // transfer per row (measured 5.6 ms per 1242x375 pair against 0.2 ms packed).
  const bool in_dense = left_stride == (size_t)width && right_stride == (size_t)width;
  const bool out_dense = disp_stride == (size_t)width * 2;
  static const int pipe_env = SBM_TUNE("SBM_HOST_PIPELINE", 1);
  if (in_dense && out_dense && n >= 16 && pipe_env && !h->profiling)
    return compute_batch_pipelined(h, n, left, right, width, height, disp);
  if (!in_dense || !out_dense) {
    const size_t need = (size_t)n * npix1 * 4;
    if (need > h->pin_bytes) {
      HIPCHK(h, hipStreamSynchronize(h->stream));
      if (h->pin) hipHostFree(h->pin);
      h->pin = nullptr; h->pin_bytes = 0;
      HIPCHK(h, hipHostMalloc((void**)&h->pin, need, hipHostMallocDefault));
      h->pin_bytes = need;
    }
  }
  uint8_t* pin_l = h->pin;
  uint8_t* pin_r = h->pin ? h->pin + (size_t)n * npix1 : nullptr;
  uint8_t* pin_d = h->pin ? h->pin + (size_t)n * npix1 * 2 : nullptr;
  if (in_dense) {
    for (int i = 0; i < n; i++) {
      HIPCHK(h, hipMemcpyAsync(h->st_l + i * npix1, left[i], npix1, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(h->st_r + i * npix1, right[i], npix1, hipMemcpyHostToDevice, h->stream));
    }
  } else {
    for (int i = 0; i < n; i++)
      for (int y = 0; y < height; y++) {
        memcpy(pin_l + i * npix1 + (size_t)y * width, left[i] + (size_t)y * left_stride, width);
        memcpy(pin_r + i * npix1 + (size_t)y * width, right[i] + (size_t)y * right_stride, width);
      }
    HIPCHK(h, hipMemcpyAsync(h->st_l, pin_l, (size_t)n * npix1, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->st_r, pin_r, (size_t)n * npix1, hipMemcpyHostToDevice, h->stream));
  }
  HP(1);
  st = sbm_compute_device(h, n, h->st_l, h->st_r, width, height, h->st_d, 0);
  if (st != SBM_OK) return st;
  HP(2);
  // Small calls into PAGEABLE caller memory (what a cv::Mat is): copy kernel into pinned host memory + flag, then the rows go to
  // the caller from there (see maps_out_kernel; 640x480: 0.199 -> 0.187 ms per call). Pinned caller memory takes the D2H copy
  // below: the DMA engine writes it directly and nothing is left for the CPU to copy (0.158 against 0.180 ms through the kernel).
  bool zero_copy = false;
  if (out_dense && (size_t)n * npix1 * 2 <= ((size_t)8 << 20) && !h->profiling && env_switch("SBM_HOST_ZEROCOPY", 1)) {
    hipPointerAttribute_t attr;
    const hipError_t pe = hipPointerGetAttributes(&attr, disp[0]);
    if (pe != hipSuccess) (void)hipGetLastError();   // (pageable memory is unknown to the runtime: that is the answer, not an error)
    zero_copy = !(pe == hipSuccess && (attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeManaged || attr.type == hipMemoryTypeDevice));
  }
  if (zero_copy) {
    st = maps_out_to_caller(h, h->st_d, n, npix1, disp);
    if (st != SBM_OK) return st;
    HP(4);
  } else if (out_dense) {
    for (int i = 0; i < n; i++)
      HIPCHK(h, hipMemcpyAsync(disp[i], h->st_d + i * npix1, npix1 * 2, hipMemcpyDeviceToHost, h->stream));
    HP(3);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HP(4);
  } else {
    HIPCHK(h, hipMemcpyAsync(pin_d, h->st_d, (size_t)n * npix1 * 2, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; i++)
      for (int y = 0; y < height; y++)
        memcpy((uint8_t*)disp[i] + (size_t)y * disp_stride, pin_d + (i * npix1 + (size_t)y * width) * 2, (size_t)width * 2);
  }
  return SBM_OK;
}

int sbm_compute(sbm_handle* h, const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride, int width,
                int height, int16_t* disp, size_t disp_stride) {
  const uint8_t* l[1] = {left};
  const uint8_t* r[1] = {right};
  int16_t* d[1] = {disp};
  if (!left || !right || !disp) return SBM_ERR_NULL;
  return sbm_compute_batch(h, 1, l, left_stride, r, right_stride, width, height, d, disp_stride);
}

}  // extern "C"
