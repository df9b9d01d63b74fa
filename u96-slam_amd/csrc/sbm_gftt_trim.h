// sbm_gftt_trim.h -- the greedy minimum-distance trim of cv::goodFeaturesToTrack and of the reference's copy of it
// (generateKeypoints2, src/slam/src/core/GFTT.cpp:104-170), shared by the two keypoint selections (sbm_gftt_select.hip: uint16
// maps of the PL; sbm_gftt_cv.hip: float maps of OpenCV's detector): the launch geometry and its plan (where the cell table
// lives), the raster index -> (x, y) split, and gftt_trim: wave 0 of a workgroup walks an ordered key list 64 candidates per
// step, tests them against the cell table and against each other (64 x 64 conflict mask, resolved in order), and appends the
// accepted points. Internal, gfx950 only.
#pragma once
#include <math.h>
#include <string.h>

#include "sbm_common.h"

namespace sbm {

// One workgroup per image. The cell table of the minimum-distance trim (16 B per cell, ceil(W/cell) * ceil(H/cell) cells) sits in
// LDS next to the sort keys when it fits (global_table = false), else in device scratch of table_bytes_per_image per image,
// zeroed by the launch.
constexpr size_t kGftSelLds = 160 * 1024;     // LDS of one workgroup
constexpr int kGftSelKeysMax = 8192;          // keys sorted per value window (64 KiB)
constexpr int kGftSelWMax = 2048;             // width and height limit: (x, y) pack into 16 bits each, indices into 22 bits
struct GftSelGeom {
  int W, H, img0;
  int cap;                  // points per image slot: max_features > 0 ? max_features : (W - 2) * (H - 2)
  int trim;                 // min_distance >= 1
  int cell, gw, gh, lim;    // cvRound(min_distance), grid size, ceil(min_distance^2)
  int nkeys;                // key capacity of a value window (a power of two)
  double q;                 // quality_level
  unsigned long long magic; // floor(2^40 / W) + 1: y = (p * magic) >> 40
};
struct GftSelPlan {
  GftSelGeom g;
  bool global_table;
  size_t lds_bytes, table_bytes_per_image;
};

constexpr int GS_THREADS = 1024, GS_WAVES = GS_THREADS / 64;
constexpr int GS_FIXED_LDS = 1280;   // 256 words of hist, 16 wave sums, 16 scalars, rounded to 16 B

struct GsShared {
  unsigned hist[256];
  int wsum[GS_WAVES];
  int acc, hi, lo, inc, cnt_gt, cnt_eq, nk, mx, cut_bin, cut_above, tmin, pad_[5];
};
static_assert(sizeof(GsShared) <= GS_FIXED_LDS, "fixed LDS");

__device__ __forceinline__ void gs_xy(unsigned p, const GftSelGeom& g, int& x, int& y) {
  y = (int)(((unsigned long long)p * g.magic) >> 40);   // exact for p < 2^22, W <= 2048
  x = (int)p - y * g.W;
}

// Wave 0: the largest bin b with sum(hist[b..255]) >= need, and sum(hist[b+1..255]); b = -1 when the total is below need.
__device__ void gs_cut(GsShared* sh, unsigned need) {
  const int lane = threadIdx.x & 63;
  const unsigned h0 = sh->hist[4 * lane], h1 = sh->hist[4 * lane + 1], h2 = sh->hist[4 * lane + 2], h3 = sh->hist[4 * lane + 3];
  const unsigned s = h0 + h1 + h2 + h3;
  unsigned suf = s;   // inclusive suffix sum over lanes >= lane
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_down(suf, o, 64);
    if (lane + o < 64) suf += t;
  }
  const unsigned long long m = __ballot(suf >= need);
  if (m == 0) {
    if (lane == 0) { sh->cut_bin = -1; sh->cut_above = 0; }
    return;
  }
  const int L = 63 - __builtin_clzll(m);
  if (lane == L) {
    unsigned above = suf - s;   // lanes > L
    int b = 4 * L + 3;
    const unsigned hv[4] = {h0, h1, h2, h3};
    for (int k = 3; k >= 0; k--) {
      b = 4 * L + k;
      if (above + hv[k] >= need) break;
      above += hv[k];
    }
    sh->cut_bin = b;
    sh->cut_above = (int)above;
  }
}

// Wave 0: trim the ordered keys [0, nk) against the table, 64 per step, and append the accepted points to `out`.
template <bool GT>
__device__ void gftt_trim(const unsigned long long* keys, int nk, GsShared* sh, unsigned* tab, float* out, const GftSelGeom& g) {
  const int lane = threadIdx.x & 63;
  int acc = sh->acc;
  for (int b0 = 0; b0 < nk && acc < g.cap; b0 += 64) {
    const int i = b0 + lane;
    const bool live = i < nk;
    const unsigned idx = live ? (unsigned)keys[i] : 0u;
    int x = 0, y = 0;
    gs_xy(idx, g, x, y);
    bool good = live;
    unsigned long long conf = 0;   // earlier lanes of this batch within minDistance in the 3x3 cells
    int cx = 0, cy = 0;
    if (g.trim) {
      cx = x / g.cell; cy = y / g.cell;
      if (live) {
        const int x1 = max(cx - 1, 0), x2 = min(cx + 1, g.gw - 1), y1 = max(cy - 1, 0), y2 = min(cy + 1, g.gh - 1);
        for (int yy = y1; yy <= y2 && good; yy++)
          for (int xx = x1; xx <= x2 && good; xx++) {
            const unsigned* c = tab + 4 * ((size_t)yy * g.gw + xx);
            unsigned w[4];
            if constexpr (GT) {
              for (int k = 0; k < 4; k++) w[k] = __hip_atomic_load(c + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
              const uint4 v = *reinterpret_cast<const uint4*>(c);
              w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            }
            const int nc = min((int)w[0], 3);
            for (int s = 0; s < nc; s++) {
              const int dx = x - (int)(w[1 + s] & 0xffffu), dy = y - (int)(w[1 + s] >> 16);
              if (dx * dx + dy * dy < g.lim) good = false;
            }
          }
      }
      const int last = min(nk - b0, 64);
      for (int j = 0; j < last - 1; j++) {
        const int xj = __shfl(x, j, 64), yj = __shfl(y, j, 64), cxj = __shfl(cx, j, 64), cyj = __shfl(cy, j, 64);
        const int dx = x - xj, dy = y - yj;
        if (j < lane && abs(cx - cxj) <= 1 && abs(cy - cyj) <= 1 && dx * dx + dy * dy < g.lim) conf |= 1ull << j;
      }
    }
    const unsigned long long G = __ballot(good);
    unsigned long long A = G;
    if (g.trim && __ballot(good && (conf & G) != 0)) {   // some good lane meets an earlier good one: resolve in order
      A = 0;
      unsigned long long rest = G;
      while (rest) {
        const int j = __builtin_ctzll(rest);
        rest &= rest - 1;
        const unsigned long long cj = ((unsigned long long)(unsigned)__shfl((int)(conf >> 32), j, 64) << 32) |
                                      (unsigned)__shfl((int)(unsigned)conf, j, 64);
        if (!(cj & A)) A |= 1ull << j;
      }
    }
    int room = g.cap - acc, na = __popcll(A);
    while (na > room) { A &= ~(1ull << (63 - __builtin_clzll(A))); na--; }   // acceptance is in order: keep the first `room`
    if ((A >> lane) & 1ull) {
      const int r = acc + __popcll(A & ((1ull << lane) - 1ull));
      out[2 * (size_t)r] = (float)x;
      out[2 * (size_t)r + 1] = (float)y;
      if (g.trim) {
        unsigned* c = tab + 4 * ((size_t)cy * g.gw + cx);
        const unsigned slot = atomicAdd(c, 1u);
        if (slot < 3) {
          if constexpr (GT) __hip_atomic_store(c + 1 + slot, (unsigned)x | ((unsigned)y << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          else c[1 + slot] = (unsigned)x | ((unsigned)y << 16);
        }
      }
    }
    if constexpr (GT) __threadfence();
    acc += na;
  }
  if (lane == 0) sh->acc = acc;
}

static inline GftSelPlan gftt_select_plan(int W, int H, int max_features, double quality, double min_distance) {
  GftSelPlan pl;
  memset(&pl, 0, sizeof(pl));
  GftSelGeom& g = pl.g;
  g.W = W; g.H = H;
  g.cap = max_features > 0 ? max_features : (W - 2) * (H - 2);
  g.q = quality;
  g.trim = min_distance >= 1.0;
  g.magic = ((1ull << 40) / (unsigned long long)W) + 1ull;
  if (g.trim) {
    g.cell = (int)lrint(min_distance);   // cvRound: half to even
    g.gw = (W + g.cell - 1) / g.cell;
    g.gh = (H + g.cell - 1) / g.cell;
    g.lim = (int)ceil(min_distance * min_distance);   // integer d2 < md^2 (double)  <=>  d2 < ceil(md^2)
  }
  const size_t table = g.trim ? (size_t)16 * g.gw * g.gh : 0;
  const size_t room = kGftSelLds - GS_FIXED_LDS;
  if (table + (size_t)8 * 1024 <= room) {
    size_t B = 1024;
    while (2 * B <= kGftSelKeysMax && 2 * B * 8 + table <= room) B *= 2;
    g.nkeys = (int)B;
    pl.global_table = false;
    pl.lds_bytes = (size_t)B * 8 + GS_FIXED_LDS + table;
  } else {
    g.nkeys = kGftSelKeysMax;
    pl.global_table = true;
    pl.lds_bytes = (size_t)kGftSelKeysMax * 8 + GS_FIXED_LDS;
    pl.table_bytes_per_image = table;
  }
  return pl;
}

}  // namespace sbm
