// sbm_handle.h -- the engine handle and the host-side helpers its entry points share across files (internal, gfx950 only).
//
// No constructors or destructors anywhere in here: sbm_create zero-fills a handle with memset, destroyed handles are parked
// for reuse, and destroy_now frees every member explicitly once the device is selected and the streams are idle.
#pragma once
#include <string.h>

#include "sbm_common.h"

#define HIPCHK(h, call)                         \
  do {                                          \
    hipError_t e_ = (call);                     \
    if (e_ != hipSuccess) {                     \
      (h)->last_hip = (int)e_;                  \
      return e_ == hipErrorOutOfMemory ? SBM_ERR_NOMEM : SBM_ERR_HIP; \
    }                                           \
  } while (0)

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

namespace sbm {

// Grow-only device memory: a pointer and its capacity in bytes.
struct DevBuf {
  void* p;
  size_t bytes;
  template <class T> T* as() const { return static_cast<T*>(p); }
  // At least `need` bytes. A buffer that is too small is replaced, contents lost, once the stream no longer uses it.
  hipError_t grow(size_t need, hipStream_t s) {
    if (need <= bytes) return hipSuccess;
    hipError_t e = p ? hipStreamSynchronize(s) : hipSuccess;
    if (e != hipSuccess) return e;
    release();
    e = hipMalloc(&p, need);
    if (e != hipSuccess) { p = nullptr; return e; }
    bytes = need;
    return hipSuccess;
  }
  void release() { hipFree(p); p = nullptr; bytes = 0; }
};

// A buffer grown to a layout (sbm_carve.h) and the layout placed in it: the counting pass sizes it, the second pass places.
template <class Layout> hipError_t carve(DevBuf& b, hipStream_t s, Layout layout, size_t align = 16) {
  const hipError_t e = b.grow(carve_bytes(layout, align), s);
  Carve place{b.as<char>(), 0, align};
  if (e == hipSuccess) layout(place);
  return e;
}

// The sets below list their buffers through each(f); these walk them.
template <class Set> void release_all(Set& s) { s.each([](DevBuf& b) { b.release(); }); }
template <class Set> size_t bytes_held(Set& s) {
  size_t n = 0;
  s.each([&](DevBuf& b) { n += b.bytes; });
  return n;
}
// A set keyed on its shape (n, W, H) is released with its key: a set whose reallocation failed half way never fits a later
// call (n >= 1 never fits n = 0), so that call redoes the whole set.
template <class Set> void release_set(Set& s) {
  release_all(s);
  s.n = s.W = s.H = 0;
}

// Scratch of the speckle filter for up to n pairs of W x H, replaced as a whole when it does not fit.
struct SpeckleScratch {
  int n, W, H;
  DevBuf runs, nheads, seam, nseam;
  template <class F> void each(F f) { f(runs); f(nheads); f(seam); f(nseam); }
  // sizes launch_speckle expects (sbm_speckle.hip): returns the total; part (may be null) receives runs, nheads, seam, nseam
  static size_t bytes(int n, int W, int H, size_t* part);
  hipError_t ensure(int n_, int W_, int H_, hipStream_t s) {
    if (nseam.p && n_ <= n && W_ == W && H_ == H) return hipSuccess;   // keyed on the LAST buffer: a half-failed attempt is redone
    hipError_t e = bytes_held(*this) ? hipStreamSynchronize(s) : hipSuccess;
    if (e != hipSuccess) return e;
    release_set(*this);
    size_t part[4];
    bytes(n_, W_, H_, part);
    DevBuf* b[4] = {&runs, &nheads, &seam, &nseam};
    for (int i = 0; i < 4 && e == hipSuccess; i++) e = b[i]->grow(part[i], s);
    if (e == hipSuccess) { n = n_; W = W_; H = H_; }
    return e;
  }
};

// cv filterSpeckles as parallel connected components (union-find) on n maps of W x H (g.n, g.W, g.H), sc sized for them: the
// launches of speckle_plan(g, max_size, ...).
hipError_t launch_speckle(int16_t* disp, const SpeckleScratch& sc, const Geom& g, const SpkPlan& k, int max_size, hipStream_t s);

// The stages of one family: the names sbm_get_profile answers, and how many marks one call records. Each family's file (the
// block matcher's is sbm_api.hip) has the names, next to the enums that index its stages and marks and the code that times them.
struct StageTable { const char* const* names; int nstage, nmark; };
StageTable bm_stages(), sgbm_stages(), gftt_select_stages(), gftt_cv_stages(), orb_stages(), match_stages(), pnp_stages(), lk_stages(), occ_stages(), vwd_stages(), pgo_stages();

// Stage times of one family's last call while profiling is on: one event per mark, created on the first profiled call, and per
// stage the milliseconds of the last call summed over its chunks. All zero is a valid clock. A family whose stages run back to
// back has one enum for both: mark s is recorded as stage s begins, the total's mark at the end.
struct StageClock {
  static constexpr int kMax = 12;
  bool on;   // this call is timed
  hipEvent_t ev[kMax];
  float ms[kMax];
  // a call begins: with profiling, its times start at 0
  hipError_t start(const StageTable& t, bool profiling) {
    on = profiling;
    hipError_t e = hipSuccess;
    for (int i = 0; on && i < t.nmark && e == hipSuccess; i++)
      if (!ev[i]) e = hipEventCreate(&ev[i]);
    if (on) reset();
    return e;
  }
  hipError_t mark(int i, hipStream_t s) { return on ? hipEventRecord(ev[i], s) : hipSuccess; }
  // stage += time from mark a to mark b, once b is reached
  hipError_t add(int stage, int a, int b) {
    if (!on) return hipSuccess;
    float t = 0.f;
    hipError_t e = hipEventSynchronize(ev[b]);
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ev[a], ev[b]);
    ms[stage] += t;
    return e;
  }
  void reset() { for (float& t : ms) t = 0.f; }
  void release() {
    for (hipEvent_t& e : ev)
      if (e) { hipEventDestroy(e); e = nullptr; }
  }
};
// A family's table from the counts its enums end in: a name table and an enum of different lengths do not build.
template <int NStage, int NMark, int N> constexpr StageTable stage_table(const char* const (&names)[N]) {
  static_assert(N == NStage && NStage <= StageClock::kMax && NMark <= StageClock::kMax, "stages and marks must fit StageClock::kMax");
  return {names, NStage, NMark};
}

// The pose-graph optimiser's last call, for sbm_pgo_last_plan and sbm_pgo_debug_fetch: its sizes, the lambda of its last
// iteration, and where that iteration's records lie in the handle's buffers (null until a call has finished). One record, so
// that a call resets all of it in one statement before it replaces any buffer.
struct PgoDebug { const double *rec, *D, *Eoff, *bv, *x; };
struct PgoLast { int ne, nfree, nslots, nj, nruns, iterations; double lambda; PgoDebug dev; };

}  // namespace sbm

struct sbm_handle {
  sbm_params p;
  int device;
  hipStream_t stream;
  int last_hip;
  struct {   // block matcher scratch, sized for (n, W, H, pitch)
    int n, W, H, pitch;
    sbm::DevBuf pf_l, pf_r;   // padded prefiltered planes (+4096 bytes); the padding must read as 0
    sbm::DevBuf disp_pre;
    sbm::DevBuf cost;         // allocated once the LR check is on
    sbm::DevBuf lr_keys;      // claim table of the LR check for rows wider than kLrLdsCols (lr_keys_bytes)
    sbm::DevBuf vsum;         // column sums of PREFILTER_NORMALIZED_RESPONSE (2 * n * W * H uint16), allocated on first use
    sbm::DevBuf handoff;      // vertical sums between the interior kernel's row segments (sad_fast_handoff_bytes), on first use
    size_t ho_flags;          // bytes at its start that hold ready / taken words: zero, or epochs of earlier launches
    unsigned ho_epoch;        // number of the last interior launch that used it
    size_t ho_slots;          // slots of the last call: linked row segments * pairs * strips
    long ho_links;            // (segment, pair, strip) that could take their sums over in the last call, for sbm_debug_fetch(7)
    sbm::SpeckleScratch spk;
    sbm::StageClock clock;    // stage times only: the marks are the handle's ring below (bm_stages() has no marks of its own)
    template <class F> void each(F f) { f(pf_l); f(pf_r); f(disp_pre); f(cost); f(lr_keys); f(vsum); f(handoff); spk.each(f); }
  } bm;
  struct {   // FPGA-flavour matcher, sized for n pairs of W x H
    int n, W, H;
    int gen;                  // call counter: generation stamp of the saturation flags
    sbm::DevBuf rec, flag, xs_l, xs_r;
    template <class F> void each(F f) { f(rec); f(flag); f(xs_l); f(xs_r); }
  } fp;
  struct {   // device staging of the host-buffer entry points, sized for n pairs of W x H
    int n, W, H;
    sbm::DevBuf l, r, d;      // left and right images (+64 bytes), maps
    sbm::DevBuf zc_cnt;       // workgroups of the maps-out copy kernel that have finished (the last one raises the flag)
    template <class F> void each(F f) { f(l); f(r); f(d); f(zc_cnt); }
  } st;
  uint8_t* pin;        // pinned host staging for strided caller images (rows packed / unpacked on the CPU)
  size_t pin_bytes;
  // small host-buffer calls (the reference's one pair per call): the maps leave through a copy kernel that writes pinned,
  // device-mapped host memory and raises a flag there; the host polls the flag instead of synchronising the stream
  int16_t* zc_out;     // pinned + mapped host staging of the maps
  size_t zc_bytes;
  unsigned* zc_flag;   // pinned + mapped: sequence number of the last call whose maps are complete in zc_out
  unsigned zc_seq;
  // copy streams + per-chunk events of the pipelined host batch path (created on first use)
  hipStream_t stream_in, stream_out;
  static constexpr int kChunks = 64;
  hipEvent_t ev_in[kChunks], ev_done[kChunks];
  bool pipe_ok;
  // asynchronous dense feed (sbm_submit_dense / sbm_wait_oldest): two device staging sets, up to three submissions in
  // flight (one arriving, one computing, one leaving); events are indexed by submission number & 3
  struct {
    int n, W, H;
    sbm::DevBuf l[2], r[2], d[2];
    template <class F> void each(F f) {
      for (int k = 0; k < 2; k++) { f(l[k]); f(r[k]); f(d[k]); }
    }
  } fq;
  hipEvent_t ev_fq_in[4], ev_fq_done[4], ev_fq_out[4];
  bool fq_ok;
  unsigned fq_submitted, fq_waited;
  int16_t* fq_pending_dst;     // maps of the newest submission not yet queued for their trip home (see sbm_submit_dense)
  size_t fq_pending_bytes;
  char last_kernel[128];   // SAD kernel of the last sbm_compute_device call (sbm_last_kernel_name)
  // last launch (for sbm_debug_fetch)
  sbm::Geom last;
  bool have_last;
  // profiling: mode 1 = sync after every call and keep that call's stage times; mode 2 = record stage events of
  // every call into a ring WITHOUT syncing (bench.py's timed region); sbm_get_profile then averages the ring.
  // mode 3 = mode 2 on every 4th call only (five event records cost ~20 us per call: sampling keeps the timed region honest)
  int profiling;
  unsigned ncall;      // calls since profiling was (re)enabled
  bool instr;          // this call records events
  static constexpr int kRing = 64, kMarks = 5;   // the marks of sbm_compute_device (BmMark in sbm_api.hip)
  hipEvent_t ev[kRing][kMarks];
  bool ev_ok;
  unsigned calls;  // calls recorded since profiling was (re)enabled
  struct {   // semi-global matcher: C and S for a chunk of pairs, the map before the median, the speckle filter's scratch
    sbm::DevBuf C, S, pre;
    sbm::SpeckleScratch spk;
    sbm::SgbmGeom last;       // the geometry of the last call, for sbm_debug_fetch
    bool have_last, last_one_chunk;
    sbm::StageClock clock;
    template <class F> void each(F f) { f(C); f(S); f(pre); spk.each(f); }
  } sg;
  struct {   // keypoint selection: the cell tables of the global-table kernel for one chunk of images; the points and count of
             // the host-memory entry point
    sbm::DevBuf tab, out;
    sbm::StageClock clock;
    template <class F> void each(F f) { f(tab); f(out); }
  } gs;
  struct {   // OpenCV-flavour keypoint detection: key lists, maxima and counts (and the maps nobody asked for) of one chunk of
             // frames; the cell tables of the global-table kernel; the points and count of the host-memory entry point
    sbm::DevBuf keys, small, eig, tab, out;
    sbm::StageClock clock;
    template <class F> void each(F f) { f(keys); f(small); f(eig); f(tab); f(out); }
  } gc;
  struct {   // ORB descriptors: blurred frames of one chunk; the keypoints, counts and descriptors of the host-memory entry point
    sbm::DevBuf blur, io;
    sbm::StageClock clock;
    template <class F> void each(F f) { f(blur); f(io); }
  } orb;
  struct {   // keypoint matching: partial k-NN records, owner and accepted tables of one launch; the host forms' staging
    sbm::DevBuf scratch, io;
    sbm::StageClock clock;
    template <class F> void each(F f) { f(scratch); f(io); }
  } mt;
  struct {   // motion estimation: compacted points, subsets, hypotheses, counts and refine lists of one launch; host-form staging
    sbm::DevBuf scratch, io;
    sbm::StageClock clock;
    template <class F> void each(F f) { f(scratch); f(io); }
  } pnp;
  struct {   // LK stereo: levels 1.. of both images and the left derivatives of one chunk of pairs; the host form's staging
    sbm::DevBuf pyr, deriv, io;
    sbm::StageClock clock;
    template <class F> void each(F f) { f(pyr); f(deriv); f(io); }
  } lk;
  struct {   // occupancy maps made from this handle: the radix sort's second key / count arrays and its digit counts; the host
             // forms' staging (planes in, keys and counts out). The tables themselves belong to each sbm_occ_map (sbm_occ.h).
    sbm::DevBuf sort, hist, io;
    sbm::StageClock clock;
    template <class F> void each(F f) { f(sort); f(hist); f(io); }
  } occ;
  struct {   // visual-word dictionaries made from this handle: partial 2-NN records of every slice, merged records and flags; the
             // word ids of one call; the host form's descriptor rows. The stores themselves belong to each sbm_vwd.
    sbm::DevBuf scratch, ids, io;
    sbm::StageClock clock;
    template <class F> void each(F f) { f(scratch); f(ids); f(io); }
  } vwd;
  struct {   // pose-graph optimiser: the graph (index lists, poses, measurements, information); the per-edge records and chi2;
             // the block system, the runs' factors and columns, x; the dense Schur complement and its factor
    sbm::DevBuf graph, edge, sys, schur;
    sbm::StageClock clock;
    sbm::PgoLast last;
    sbm_pgo_plan_info plan;
    template <class F> void each(F f) { f(graph); f(edge); f(sys); f(schur); }
  } pgo;
  // The two lists a new family joins: f(set) for every set that owns DevBufs, f(clock, table) for every family with stage times.
  template <class F> void each_set(F f) { f(bm); f(fp); f(st); f(fq); f(sg); f(gs); f(gc); f(orb); f(mt); f(pnp); f(lk); f(occ); f(vwd); f(pgo); }
  template <class F> void each_clock(F f) {
    using namespace sbm;
    f(bm.clock, bm_stages()); f(sg.clock, sgbm_stages()); f(gs.clock, gftt_select_stages()); f(gc.clock, gftt_cv_stages()); f(orb.clock, orb_stages());
    f(mt.clock, match_stages()); f(pnp.clock, pnp_stages()); f(lk.clock, lk_stages()); f(occ.clock, occ_stages()); f(vwd.clock, vwd_stages()); f(pgo.clock, pgo_stages());
  }
};

namespace sbm {

// Frees the device staging set of the host-buffer entry points, and with it the pinned host staging.
void free_staging(sbm_handle* h);
// Device staging for n pairs of W x H (sbm_host.hip); drops the pinned host staging when it reallocates.
int ensure_staging(sbm_handle* h, int n, int W, int H);
// Keypoint selection of n maps on the handle's stream, the eigenvalue maps first when d_img is given (sbm_gftt_select.hip).
int gftt_select_run(sbm_handle* h, int n, const void* d_img, const void* d_eig, const void* d_max, int width, int height,
                    const sbm_gftt_select_params* p, void* d_kpts, void* d_count, int sync);
// cv::goodFeaturesToTrack on n dense frames on the handle's stream (sbm_gftt_cv.hip); d_eig, d_max and d_kpts / d_count may be
// null (not wanted; without d_kpts only the maps are computed).
int gftt_cv_run(sbm_handle* h, int n, const void* d_img, int width, int height, const sbm_gftt_cv_params* p, void* d_eig, void* d_max,
                void* d_kpts, void* d_count, int sync);
// sbm_debug_fetch of the last semi-global matcher call: which = 4 (C), 5 (S), 6 (the map before the median) (sbm_sgbm.hip).
int sgbm_debug_fetch(sbm_handle* h, int which, void* dst, size_t dst_bytes);

}  // namespace sbm
