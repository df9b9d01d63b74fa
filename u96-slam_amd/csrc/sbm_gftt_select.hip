// sbm_gftt_select.hip -- keypoint selection of the reference's FPGA feature path, generateKeypoints2()
// (src/slam/src/core/GFTT.cpp:41-170), on gfx950: threshold, order (value descending, ties by the higher raster index first),
// greedy minimum-distance trim on a grid of cvRound(minDistance) cells, stop at nfeatures.
//
// One workgroup of 1024 threads per image works through the candidates in value windows, from the top:
//   1. window: a 256-bin histogram of the high byte of the values still to be taken, then one of the low byte inside the bin
//      where the running count from the top reaches the key capacity B, give the lowest value `lo` of the window: fewer than B
//      candidates lie in (lo, hi);
//   2. those are gathered into LDS as 64-bit keys (value << 32 | index) and sorted, descending, by a bitonic network;
//   3. the candidates equal to `lo` either fit behind them (same sort) or, when `lo` is a large plateau, are streamed in
//      descending raster order, 1024 pixels at a time, by an ordered compaction: no sort is needed inside one value;
//   4. wavefront 0 trims each ordered run, 64 candidates per step (gftt_trim), until nfeatures are accepted.
// Only the prefix that is consumed gets ordered; a plateau (an all-zero map with max = 0) costs one pass per 1024 pixels it
// scans, never a sort.
//
// The accepted points live in a cell table of 4 words per cell: a count and up to three packed points (x | y << 16). Points of
// one cell are at least minDistance >= cell - 0.5 apart inside a square of side cell - 1, so a cell never holds four. The table
// sits in LDS when it fits next to the keys (gftt_select_kernel<false>), else in device scratch (<true>; small cells on large
// images). Both are exact: the candidate test, the in-batch conflicts and the acceptance order are the same code.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "sbm_handle.h"
#include "sbm_gftt_trim.h"

namespace sbm {

template <bool GT>
__global__ void __launch_bounds__(GS_THREADS) gftt_select_kernel(const uint16_t* __restrict__ eig, const unsigned* __restrict__ maxv,
                                                                 float* __restrict__ kpts, int* __restrict__ count,
                                                                 unsigned* __restrict__ gtab, GftSelGeom g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gs_lds[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(gs_lds);
  GsShared* sh = reinterpret_cast<GsShared*>(gs_lds + (size_t)g.nkeys * 8);
  unsigned* tab = GT ? gtab + (size_t)blockIdx.x * 4 * g.gw * g.gh
                     : reinterpret_cast<unsigned*>(gs_lds + (size_t)g.nkeys * 8 + GS_FIXED_LDS);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t img = (size_t)g.img0 + blockIdx.x;
  const uint16_t* map = eig + img * g.W * g.H;
  float* out = kpts + img * (size_t)g.cap * 2;
  const int npix = g.W * g.H;
  const int p0 = g.W + 1, p1 = (g.H - 1) * g.W - 1;   // rows 1..H-2 (columns 0 and W-1 are skipped by the x test)

  if (tid == 0) { sh->acc = 0; sh->hi = 65536; sh->mx = 0; }
  if (!GT && g.trim)
    for (int c = tid; c < g.gw * g.gh; c += GS_THREADS) tab[4 * c] = 0u;
  __syncthreads();
  // the Max register: the caller's low 16 bits, or the map's maximum
  if (maxv) {
    if (tid == 0) sh->mx = (int)(maxv[img] & 0xffffu);
  } else {
    unsigned m = 0;
    for (int p = tid; p < npix; p += GS_THREADS) m = max(m, (unsigned)map[p]);
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if (lane == 0) atomicMax(&sh->mx, (int)m);
  }
  __syncthreads();
  if (tid == 0) {
    const double thr = (double)sh->mx * g.q;   // (float)value >= thr, value an integer: value >= ceil(thr)
    sh->tmin = thr <= 0.0 ? 0 : (thr > 65535.0 ? 65536 : (int)ceil(thr));
  }
  __syncthreads();
  const int tmin = sh->tmin;
  const unsigned B = (unsigned)g.nkeys;

  while (true) {
    const int hi = sh->hi;
    if (tmin >= hi || sh->acc >= g.cap) break;
    // 1. the window: high-byte histogram of the values in [tmin, hi)
    for (int k = tid; k < 256; k += GS_THREADS) sh->hist[k] = 0;
    __syncthreads();
    {
      int cb = -1, cc = 0;   // runs of one bin are counted in a register (plateaus would serialise the LDS atomics)
#pragma unroll 4
      for (int p = p0 + tid; p < p1; p += GS_THREADS) {
        int x, y;
        gs_xy((unsigned)p, g, x, y);
        const int v = map[p];
        if (x >= 1 && x <= g.W - 2 && v >= tmin && v < hi) {
          const int b = v >> 8;
          if (b != cb) { if (cc) atomicAdd(&sh->hist[cb], (unsigned)cc); cb = b; cc = 0; }
          cc++;
        }
      }
      if (cc) atomicAdd(&sh->hist[cb], (unsigned)cc);
    }
    __syncthreads();
    if (wave == 0) gs_cut(sh, B + 1);   // more than B candidates left?
    __syncthreads();
    if (sh->cut_bin < 0) {   // all of them fit: one sorted run
      if (tid == 0) { sh->lo = tmin; sh->inc = 1; }
    } else {
      const int b1 = sh->cut_bin;
      const unsigned above1 = (unsigned)sh->cut_above;
      __syncthreads();
      for (int k = tid; k < 256; k += GS_THREADS) sh->hist[k] = 0;
      __syncthreads();
      const int va = max(tmin, b1 << 8), vb = min(hi, (b1 << 8) + 256);
      int cb = -1, cc = 0;
#pragma unroll 4
      for (int p = p0 + tid; p < p1; p += GS_THREADS) {
        int x, y;
        gs_xy((unsigned)p, g, x, y);
        const int v = map[p];
        if (x >= 1 && x <= g.W - 2 && v >= va && v < vb) {
          const int b = v & 255;
          if (b != cb) { if (cc) atomicAdd(&sh->hist[cb], (unsigned)cc); cb = b; cc = 0; }
          cc++;
        }
      }
      if (cc) atomicAdd(&sh->hist[cb], (unsigned)cc);
      __syncthreads();
      if (wave == 0) gs_cut(sh, B - above1);   // >= 1; the bin holds more than that
      __syncthreads();
      if (tid == 0) {
        const int b2 = sh->cut_bin;
        const int gt = (int)above1 + sh->cut_above, eq = (int)sh->hist[b2];
        sh->lo = (b1 << 8) + b2;
        sh->cnt_gt = gt;
        sh->cnt_eq = eq;
        sh->inc = (unsigned)(gt + eq) <= B;
      }
    }
    if (tid == 0) sh->nk = 0;
    __syncthreads();
    const int lo = sh->lo, inc = sh->inc;
    // 2. gather (lo, hi) -- and lo itself when it fits -- and sort
    {
      const int vlo = inc ? lo : lo + 1;
      for (int pb = p0; pb < p1; pb += GS_THREADS) {
        const int p = pb + tid;
        int x = 0, y = 0;
        bool f = false;
        unsigned v = 0;
        if (p < p1) {
          gs_xy((unsigned)p, g, x, y);
          v = map[p];
          f = x >= 1 && x <= g.W - 2 && (int)v >= vlo && (int)v < hi;
        }
        const unsigned long long m = __ballot(f);
        if (m) {
          int base = 0;
          if (lane == __builtin_ctzll(m)) base = atomicAdd(&sh->nk, __popcll(m));
          base = __shfl(base, __builtin_ctzll(m), 64);
          if (f) keys[base + __popcll(m & ((1ull << lane) - 1ull))] = ((unsigned long long)v << 32) | (unsigned)p;
        }
      }
    }
    __syncthreads();
    const int nk = sh->nk;
    if (nk > 1) {
      int P = 1;
      while (P < nk) P <<= 1;
      for (int k = nk + tid; k < P; k += GS_THREADS) keys[k] = 0ull;   // real keys are > 0 (index >= W + 1)
      __syncthreads();
      for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int i = tid; i < P; i += GS_THREADS) {
            const int ixj = i ^ j;
            if (ixj > i) {
              const unsigned long long a = keys[i], b = keys[ixj];
              if (((i & k) == 0) ? (a < b) : (a > b)) { keys[i] = b; keys[ixj] = a; }
            }
          }
          __syncthreads();
        }
    }
    if (wave == 0 && nk > 0) gftt_trim<GT>(keys, nk, sh, tab, out, g);
    __syncthreads();
    // 3. a plateau at lo that did not fit: descending raster order, 1024 pixels at a time
    if (!inc) {
      int left = sh->cnt_eq;
      for (int pb = p1 - 1; pb >= p0 && left > 0 && sh->acc < g.cap; pb -= GS_THREADS) {
        const int p = pb - tid;
        bool f = false;
        if (p >= p0) {
          int x, y;
          gs_xy((unsigned)p, g, x, y);
          f = x >= 1 && x <= g.W - 2 && (int)map[p] == lo;
        }
        const unsigned long long m = __ballot(f);
        if (lane == 0) sh->wsum[wave] = __popcll(m);
        __syncthreads();
        int base = 0, tot = 0;
        for (int w = 0; w < GS_WAVES; w++) {
          const int c = sh->wsum[w];
          base += w < wave ? c : 0;
          tot += c;
        }
        if (f) keys[base + __popcll(m & ((1ull << lane) - 1ull))] = ((unsigned long long)lo << 32) | (unsigned)p;
        __syncthreads();
        if (wave == 0 && tot > 0) gftt_trim<GT>(keys, tot, sh, tab, out, g);
        left -= tot;
        __syncthreads();
      }
    }
    if (tid == 0) sh->hi = lo;
    __syncthreads();
  }
  if (tid == 0) count[img] = sh->acc;
}

// eig: dense uint16 maps, maxv: their Max words (null: each map's maximum); images [img0, img0 + n) of the batch
static hipError_t launch_gftt_select(const uint16_t* eig, const unsigned* maxv, float* kpts, int* count, unsigned* gtab, const GftSelPlan& pl,
                                     int img0, int n, hipStream_t s) {
  GftSelGeom g = pl.g;
  g.img0 = img0;
  if (pl.global_table) {
    hipError_t e = hipMemsetAsync(gtab, 0, pl.table_bytes_per_image * n, s);
    if (e != hipSuccess) return e;
  }
  auto kern = pl.global_table ? gftt_select_kernel<true> : gftt_select_kernel<false>;
  // (more than 64 KB of dynamic LDS has to be granted per kernel; idempotent, so unsynchronised repeats are harmless)
  if (pl.lds_bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)kGftSelLds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kern, dim3(n), dim3(GS_THREADS), pl.lds_bytes, s, eig, maxv, kpts, count, gtab, g);
  return hipGetLastError();
}

}  // namespace sbm

// ---- entry points --------------------------------------------------------------------------------------------------------
using namespace sbm;

extern "C" {

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
  float* d_k;
  int* d_n;   // points on 8-byte boundaries, then the count
  HIPCHK(h, carve(h->gs.out, h->stream, [&](Carve& c) { d_k = c.take<float>(cap * 2); d_n = c.take<int>(4); }, 8));
  // st.d: the map, st.r: the Max word
  const uint32_t mx = max_eig;
  HIPCHK(h, hipMemcpy2DAsync(h->st.d.p, (size_t)width * 2, eig, eig_stride, (size_t)width * 2, height, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->st.r.p, &mx, sizeof(mx), hipMemcpyHostToDevice, h->stream));
  st = gftt_select_run(h, 1, nullptr, h->st.d.p, h->st.r.p, width, height, p, d_k, d_n, 0);
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

}  // extern "C"

enum GfttSelectStage { kGsEig, kGsSelect, kGsTotal, kGsStageCount };
static const char* const kGfttSelectNames[] = {"gftt_select_eig", "gftt_select_select", "gftt_select_total"};
StageTable sbm::gftt_select_stages() { return stage_table<kGsStageCount, kGsStageCount>(kGfttSelectNames); }

// Enqueues the eigenvalue maps (d_img given) and the selection of n dense maps; profiling times the two.
int sbm::gftt_select_run(sbm_handle* h, int n, const void* d_img, const void* d_eig, const void* d_max, int width, int height,
                         const sbm_gftt_select_params* p, void* d_kpts, void* d_count, int sync) {
  StageClock& clk = h->gs.clock;
  HIPCHK(h, clk.start(gftt_select_stages(), h->profiling != 0));
  HIPCHK(h, clk.mark(kGsEig, h->stream));
  if (d_img)
    HIPCHK(h, launch_gftt_eig((const uint8_t*)d_img, (uint16_t*)d_eig, (unsigned*)d_max, n, width, height, h->stream));
  HIPCHK(h, clk.mark(kGsSelect, h->stream));
  const GftSelPlan pl = gftt_select_plan(width, height, p->max_features, p->quality_level, p->min_distance);
  // the global-table kernel works through the images in chunks whose tables stay within 2 GiB
  int chunk = n;
  if (pl.global_table) {
    chunk = (int)std::min<size_t>(n, std::max<size_t>(1, ((size_t)2 << 30) / pl.table_bytes_per_image));
    HIPCHK(h, h->gs.tab.grow(pl.table_bytes_per_image * chunk, h->stream));
  }
  for (int c0 = 0; c0 < n; c0 += chunk)
    HIPCHK(h, launch_gftt_select((const uint16_t*)d_eig, (const unsigned*)d_max, (float*)d_kpts, (int*)d_count, h->gs.tab.as<unsigned>(),
                                 pl, c0, std::min(chunk, n - c0), h->stream));
  HIPCHK(h, clk.mark(kGsTotal, h->stream));
  if (d_img) HIPCHK(h, clk.add(kGsEig, kGsEig, kGsSelect));
  HIPCHK(h, clk.add(kGsSelect, kGsSelect, kGsTotal));
  HIPCHK(h, clk.add(kGsTotal, kGsEig, kGsTotal));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}
