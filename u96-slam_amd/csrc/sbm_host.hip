// sbm_host.hip -- the block matcher's host-buffer entry points: device staging, the pipelined batch, the asynchronous dense
// feed, the zero-copy maps-out kernel, sbm_compute_batch_multi, sbm_compute_batch and sbm_compute. They feed
// sbm_compute_device (sbm_api.hip) from and to caller memory.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <thread>

#include "sbm_handle.h"

using namespace sbm;

static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield");
#else
  std::this_thread::yield();
#endif
}

// The pinned host staging goes with the device set: both are sized for the last batch shape.
void sbm::free_staging(sbm_handle* h) {
  release_set(h->st);
  if (h->pin) hipHostFree(h->pin);
  h->pin = nullptr; h->pin_bytes = 0;
  if (h->zc_out) hipHostFree(h->zc_out);
  if (h->zc_flag) hipHostFree(h->zc_flag);
  h->zc_out = nullptr; h->zc_flag = nullptr; h->zc_bytes = 0;
}

int sbm::ensure_staging(sbm_handle* h, int n, int W, int H) {
  auto& s = h->st;
  if (n <= s.n && W == s.W && H == s.H && s.l.p) return SBM_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  free_staging(h);
  const size_t npix = (size_t)n * W * H;
  HIPCHK(h, s.l.grow(npix + 64, h->stream));
  HIPCHK(h, s.r.grow(npix + 64, h->stream));
  HIPCHK(h, s.d.grow(npix * sizeof(int16_t), h->stream));
  s.n = n; s.W = W; s.H = H;
  return SBM_OK;
}

extern "C" {

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
  const int16_t* st_d = h->st.d.as<int16_t>();
  for (int i = i0; i < i1;) {
    int j = i + 1;
    while (j < i1 && disp[j] == disp[j - 1] + npix1) j++;
    const hipError_t e = hipMemcpyAsync(disp[i], st_d + i * npix1, (size_t)(j - i) * npix1 * 2, hipMemcpyDeviceToHost, h->stream_out);
    if (e != hipSuccess) return e;
    i = j;
  }
  return hipSuccess;
}

static int pipelined_enqueue(sbm_handle* h, int n, const uint8_t* const* left, const uint8_t* const* right, int width,
                             int height, int16_t* const* disp) {
  const size_t npix1 = (size_t)width * height;
  uint8_t *st_l = h->st.l.as<uint8_t>(), *st_r = h->st.r.as<uint8_t>();
  int16_t* st_d = h->st.d.as<int16_t>();
  // Chunk plan. Small chunks overlap more of the transfers but run the kernels on part-filled launches (8 KITTI pairs cost
  // 0.36 ms on the device, 64 pairs 1.2 ms), so: a small FIRST chunk (the computation starts after one short transfer), a
  // small LAST one (only its computation and its maps are left when the inputs have arrived) and large ones in between.
  // Measured on 64 KITTI pairs from pinned memory (profiles/r03_host_feed.json). Fewer than 32 pairs: chunks of 8.
  int start[sbm_handle::kChunks + 1];
  int nch = 0;
  start[0] = 0;
  if (n < 32) {
    for (int i = 0; i < n; i += 8) start[++nch] = std::min(n, i + 8);
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
      HIPCHK(h, hipMemcpyAsync(st_l + i * npix1, left[i], (size_t)(j - i) * npix1, hipMemcpyHostToDevice, h->stream_in));
      i = j;
    }
    for (int i = i0; i < i0 + cnt;) {
      int j = i + 1;
      while (j < i0 + cnt && right[j] == right[j - 1] + npix1) j++;
      HIPCHK(h, hipMemcpyAsync(st_r + i * npix1, right[i], (size_t)(j - i) * npix1, hipMemcpyHostToDevice, h->stream_in));
      i = j;
    }
    HIPCHK(h, hipEventRecord(h->ev_in[k], h->stream_in));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_in[k], 0));
    const int st = sbm_compute_device(h, cnt, st_l + i0 * npix1, st_r + i0 * npix1, width, height, st_d + i0 * npix1, 0);
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
  HIPCHK(h, hipMemcpyAsync(h->fq_pending_dst, h->fq.d[slot].p, h->fq_pending_bytes, hipMemcpyDeviceToHost, h->stream_out));
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
  auto& fq = h->fq;
  if (!(n <= fq.n && width == fq.W && height == fq.H && fq.l[0].p)) {
    while (h->fq_waited != h->fq_submitted) {
      st = sbm_wait_oldest(h);
      if (st != SBM_OK) return st;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    release_set(fq);
    for (int k = 0; k < 2; k++) {
      HIPCHK(h, fq.l[k].grow(npix + 64, h->stream));
      HIPCHK(h, fq.r[k].grow(npix + 64, h->stream));
      HIPCHK(h, fq.d[k].grow(npix * sizeof(int16_t), h->stream));
    }
    fq.n = n; fq.W = width; fq.H = height;
  }
  // submission k uses device staging set k & 1. The set's previous user is submission k-2: its inputs are free once k-2 has
  // computed, its map buffer once k-2's maps have left -- both are stream dependencies, the host never blocks on them.
  const unsigned k = h->fq_submitted, slot = k & 1u, e = k & 3u;
  if (k >= 2 && k - 2 >= h->fq_waited) {
    HIPCHK(h, hipStreamWaitEvent(h->stream_in, h->ev_fq_done[(k - 2) & 3u], 0));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_fq_out[(k - 2) & 3u], 0));
  }
  HIPCHK(h, hipMemcpyAsync(fq.l[slot].p, left, npix, hipMemcpyHostToDevice, h->stream_in));
  HIPCHK(h, hipMemcpyAsync(fq.r[slot].p, right, npix, hipMemcpyHostToDevice, h->stream_in));
  HIPCHK(h, hipEventRecord(h->ev_fq_in[e], h->stream_in));
  st = fq_flush_pending(h);                      // the previous submission's maps: queued behind this one's inputs
  if (st != SBM_OK) return st;
  HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_fq_in[e], 0));
  st = sbm_compute_device(h, n, fq.l[slot].p, fq.r[slot].p, width, height, fq.d[slot].p, 0);
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
  if (h->zc_out && h->zc_flag && h->st.zc_cnt.p && h->zc_bytes >= bytes) return SBM_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // flag and counter first, the staging last: zc_bytes only ever describes a complete set (a failure half way leaves a state
  // the next call simply completes)
  if (!h->zc_flag) {
    HIPCHK(h, hipHostMalloc((void**)&h->zc_flag, 64, hipHostMallocMapped | hipHostMallocCoherent));
    for (int k = 0; k < kZcChunks; k++) h->zc_flag[k] = 0u;
    h->zc_seq = 0u;
  }
  if (!h->st.zc_cnt.p) {
    HIPCHK(h, h->st.zc_cnt.grow(64, h->stream));
    const hipError_t e = hipMemsetAsync(h->st.zc_cnt.p, 0, 64, h->stream);
    if (e != hipSuccess) {
      h->st.zc_cnt.release();
      HIPCHK(h, e);
    }
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
                     per_chunk, bpc, d_src + n16 * 8, h->zc_out + n16 * 8, ntail, h->st.zc_cnt.as<unsigned>(), h->zc_flag, seq);
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
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = ensure_staging(h, n, width, height);
  if (st != SBM_OK) return st;
  uint8_t *st_l = h->st.l.as<uint8_t>(), *st_r = h->st.r.as<uint8_t>();
  int16_t* st_d = h->st.d.as<int16_t>();
  const size_t npix1 = (size_t)width * height;
  // Dense caller images (stride == width, what cv::Mat::isContinuous() gives) go through plain 1-D copies. Strided ones
  // are packed row by row into pinned staging on the CPU: a 2-D copy from pageable memory degenerates into one small
  // transfer per row (measured 5.6 ms per 1242x375 pair against 0.2 ms packed).
  const bool in_dense = left_stride == (size_t)width && right_stride == (size_t)width;
  const bool out_dense = disp_stride == (size_t)width * 2;
  if (in_dense && out_dense && n >= 16 && !h->profiling)
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
      HIPCHK(h, hipMemcpyAsync(st_l + i * npix1, left[i], npix1, hipMemcpyHostToDevice, h->stream));
      HIPCHK(h, hipMemcpyAsync(st_r + i * npix1, right[i], npix1, hipMemcpyHostToDevice, h->stream));
    }
  } else {
    for (int i = 0; i < n; i++)
      for (int y = 0; y < height; y++) {
        memcpy(pin_l + i * npix1 + (size_t)y * width, left[i] + (size_t)y * left_stride, width);
        memcpy(pin_r + i * npix1 + (size_t)y * width, right[i] + (size_t)y * right_stride, width);
      }
    HIPCHK(h, hipMemcpyAsync(st_l, pin_l, (size_t)n * npix1, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(st_r, pin_r, (size_t)n * npix1, hipMemcpyHostToDevice, h->stream));
  }
  st = sbm_compute_device(h, n, st_l, st_r, width, height, st_d, 0);
  if (st != SBM_OK) return st;
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
    st = maps_out_to_caller(h, st_d, n, npix1, disp);
    if (st != SBM_OK) return st;
  } else if (out_dense) {
    for (int i = 0; i < n; i++)
      HIPCHK(h, hipMemcpyAsync(disp[i], st_d + i * npix1, npix1 * 2, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  } else {
    HIPCHK(h, hipMemcpyAsync(pin_d, st_d, (size_t)n * npix1 * 2, hipMemcpyDeviceToHost, h->stream));
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
