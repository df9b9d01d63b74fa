// sbm_lk.hip -- pyramidal LK stereo, the reference's DEPTH_METHOD_CV_LK (include/sbm.h, "pyramidal LK stereo"). gfx950.
//
// Reference: computeCorrespondences, src/slam/src/core/Stereo.cpp:9-51, over calcOpticalFlowPyrLKStereo,
// src/slam/src/opencv/CvLKStereo.cpp (the tracker: REF), and cv::buildOpticalFlowPyramid (the pyramid: RECALLED).
// Three kernels: pyrDown of every frame of a level in one launch, Scharr derivatives of the left frames of a level in one
// launch, and ONE tracker launch that walks the levels top down per point: one wavefront per keypoint, lanes 0..44 own the 45
// pixels of the 15 x 3 window and keep I, Ix, Iy in registers across the iterations. The float sums are part of the contract
// (raster order of the window, every partial sum rounded): each lane's term is read back lane by lane (v_readlane) and added
// by one chain, identically in every lane, so every decision after it is uniform across the wavefront. Nothing is stored
// padded: the image is read with BORDER_REFLECT_101 and the derivative with zeros outside the level.
// Everything is IEEE binary32 / binary64 without contraction (the Makefile adds -ffp-contract=off; the pragma says so too).
#include <algorithm>
#include <cmath>

#include "sbm_handle.h"

namespace sbm {

#pragma clang fp contract(off)

constexpr int kLkWinW = 15, kLkWinH = 3, kLkWin = kLkWinW * kLkWinH;   // the one supported window
constexpr int kLkMaxLevels = 8;                                         // 2048 -> 16 columns at level 7, the last one kept
constexpr int kLkMaxDim = 2048;
constexpr size_t kLkChunkBytes = (size_t)256 << 20;
constexpr size_t kLkMaxGridZ = 65535;                                   // frames of one launch (gridDim.z, and gridDim.y of the tracker)
constexpr int kLkFlagInitialFlow = 4, kLkFlagMinEig = 8;                // cv::OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_LK_GET_MIN_EIGENVALS
constexpr int kLkWaves = 4;                                             // keypoints per workgroup of the tracker

// BORDER_REFLECT_101 of i into [0, n), as often as it takes (n >= 2)
__host__ __device__ __forceinline__ int lk_reflect(int i, int n) {
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

struct LkLevel {
  const uint8_t* I;   // left frames of the chunk at this level, w * h each
  const uint8_t* J;   // right frames
  const short* d;     // (dx, dy) of the left frames
  int w, h;
};
struct LkGeom {
  LkLevel lv[kLkMaxLevels];
  int L;              // index of the last level
  int cap, max_count, gate;
  double eps2, min_eig;
  float min_disp, max_disp;
};

// dst frame f of the launch <- pyrDown(src frame f); frames [0, nA) come from srcA, the rest from srcB (level 1 reads the
// caller's two buffers, every later level the scratch where right follows left)
__global__ void __launch_bounds__(256) lk_pyrdown_kernel(const uint8_t* __restrict__ srcA, const uint8_t* __restrict__ srcB, int nA,
                                                          uint8_t* __restrict__ dst, int w, int h, int dw, int dh) {
  const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5), f = blockIdx.z;
  if (x >= dw || y >= dh) return;
  const uint8_t* src = f < nA ? srcA + (size_t)f * w * h : srcB + (size_t)(f - nA) * w * h;
  const int k[5] = {1, 4, 6, 4, 1};
  int xi[5];
#pragma unroll
  for (int i = 0; i < 5; i++) xi[i] = lk_reflect(2 * x + i - 2, w);
  int s = 0;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const uint8_t* row = src + (size_t)lk_reflect(2 * y + j - 2, h) * w;
    int r = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) r += k[i] * row[xi[i]];
    s += k[j] * r;
  }
  dst[(size_t)f * dw * dh + (size_t)y * dw + x] = (uint8_t)((s + 128) >> 8);
}

// Scharr (3, 10, 3) x (-1, 0, 1) of frame f of the level, reflect-101, (dx, dy) int16 interleaved
__global__ void __launch_bounds__(256) lk_scharr_kernel(const uint8_t* __restrict__ img, short* __restrict__ d, int w, int h) {
  const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5), f = blockIdx.z;
  if (x >= w || y >= h) return;
  const uint8_t* src = img + (size_t)f * w * h;
  const uint8_t* r0 = src + (size_t)lk_reflect(y - 1, h) * w;
  const uint8_t* r1 = src + (size_t)y * w;
  const uint8_t* r2 = src + (size_t)lk_reflect(y + 1, h) * w;
  const int xl = lk_reflect(x - 1, w), xr = lk_reflect(x + 1, w);
  const int dx = 3 * (r0[xr] - r0[xl]) + 10 * (r1[xr] - r1[xl]) + 3 * (r2[xr] - r2[xl]);
  const int dy = 3 * (r2[xl] - r0[xl]) + 10 * (r2[x] - r0[x]) + 3 * (r2[xr] - r0[xr]);
  short2 o;
  o.x = (short)dx;
  o.y = (short)dy;
  reinterpret_cast<short2*>(d)[(size_t)f * w * h + (size_t)y * w + x] = o;
}

// sum of term over lanes 0..44 in lane order, one rounded addition after the other, the same value in every lane
__device__ __forceinline__ float lk_ordered_sum(float term) {
#pragma clang fp contract(off)
  const int bits = __float_as_int(term);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kLkWin; i++) s = s + __int_as_float(__builtin_amdgcn_readlane(bits, i));
  return s;
}

struct LkWeights { int w00, w01, w10, w11; };
__device__ __forceinline__ LkWeights lk_weights(float a, float b) {
#pragma clang fp contract(off)
  const float a1 = 1.f - a, b1 = 1.f - b;
  LkWeights q;
  float t = a1 * b1;
  q.w00 = __float2int_rn(t * 16384.f);
  t = a * b1;
  q.w01 = __float2int_rn(t * 16384.f);
  t = a1 * b;
  q.w10 = __float2int_rn(t * 16384.f);
  q.w11 = 16384 - q.w00 - q.w01 - q.w10;
  return q;
}

__device__ __forceinline__ int lk_patch(const uint8_t* p, int w, int h, int X, int Y, const LkWeights& q) {
  const int x0 = lk_reflect(X, w), x1 = lk_reflect(X + 1, w);
  const uint8_t* r0 = p + (size_t)lk_reflect(Y, h) * w;
  const uint8_t* r1 = p + (size_t)lk_reflect(Y + 1, h) * w;
  return (r0[x0] * q.w00 + r0[x1] * q.w01 + r1[x0] * q.w10 + r1[x1] * q.w11 + 256) >> 9;
}
__device__ __forceinline__ short2 lk_der(const short* d, int w, int h, int x, int y) {
  short2 z;
  z.x = z.y = 0;
  return (x < 0 || x >= w || y < 0 || y >= h) ? z : reinterpret_cast<const short2*>(d)[(size_t)y * w + x];
}

// One wavefront per (frame, keypoint) slot below the frame's count. Every exit below is taken by the whole wavefront.
__global__ void __launch_bounds__(64 * kLkWaves) lk_track_kernel(LkGeom g, const float* __restrict__ kpts, const int* __restrict__ count,
                                                                  float* __restrict__ right_pts, uint8_t* __restrict__ status,
                                                                  float* __restrict__ err, int frame0) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int idx = blockIdx.x * kLkWaves + (threadIdx.x >> 6), f = blockIdx.y;
  const int cnt = min(count[frame0 + f], g.cap);
  if (idx >= cnt) return;
  const size_t slot = (size_t)(frame0 + f) * g.cap + idx;
  const float ptx = kpts[2 * slot], pty = kpts[2 * slot + 1];
  const bool own = lane < kLkWin;
  const int wy = own ? lane / kLkWinW : 0, wx = own ? lane % kLkWinW : 0;
  const float half_x = (kLkWinW - 1) * 0.5f, half_y = (kLkWinH - 1) * 0.5f;
  const float FLT_SCALE = 1.f / (1 << 20);
  float outx = 0.f, outy = 0.f, e = 0.f;
  int st = 1;

  for (int level = g.L; level >= 0; level--) {
    const LkLevel v = g.lv[level];
    const size_t plane = (size_t)v.w * v.h;
    const uint8_t* I = v.I + plane * f;
    const uint8_t* J = v.J + plane * f;
    const short* dI = v.d + plane * f * 2;
    const float scale = (float)(1. / (1 << level));
    float px = ptx * scale, py = pty * scale;
    float nx, ny;
    if (level == g.L) { nx = px; ny = py; } else { nx = outx * 2.f; ny = outy * 2.f; }
    outx = nx;
    outy = ny;
    px = px - half_x;
    py = py - half_y;
    const int ipx = (int)floorf(px), ipy = (int)floorf(py);
    if (ipx < -kLkWinW || ipx >= v.w || ipy < -kLkWinH || ipy >= v.h) {
      if (level == 0) { st = 0; e = 0.f; }
      continue;
    }
    LkWeights q = lk_weights(px - (float)ipx, py - (float)ipy);
    int ival = 0, ixval = 0, iyval = 0;
    if (own) {
      const int X = ipx + wx, Y = ipy + wy;
      ival = lk_patch(I, v.w, v.h, X, Y, q);
      const short2 d00 = lk_der(dI, v.w, v.h, X, Y), d01 = lk_der(dI, v.w, v.h, X + 1, Y), d10 = lk_der(dI, v.w, v.h, X, Y + 1),
                   d11 = lk_der(dI, v.w, v.h, X + 1, Y + 1);
      ixval = (d00.x * q.w00 + d01.x * q.w01 + d10.x * q.w10 + d11.x * q.w11 + 8192) >> 14;
      iyval = (d00.y * q.w00 + d01.y * q.w01 + d10.y * q.w10 + d11.y * q.w11 + 8192) >> 14;
    }
    const float iA11 = lk_ordered_sum((float)(ixval * ixval));
    const float iA12 = lk_ordered_sum((float)(ixval * iyval));
    const float iA22 = lk_ordered_sum((float)(iyval * iyval));
    const float A11 = iA11 * FLT_SCALE, A12 = iA12 * FLT_SCALE, A22 = iA22 * FLT_SCALE;
    const float t1 = A11 * A22, t2 = A12 * A12;
    float D = t1 - t2;
    const float dA = A11 - A22;
    const float r1 = dA * dA;
    float r2 = 4.f * A12;
    r2 = r2 * A12;
    const float sq = sqrtf(r1 + r2);   // correctly rounded (the bare instruction, __fsqrt_rn, is not)
    float num = A22 + A11;
    num = num - sq;
    const float minEig = num / (float)(2 * kLkWinW * kLkWinH);
    e = minEig;
    if ((double)minEig < g.min_eig || D < 1.1920928955078125e-7f) {
      if (level == 0) st = 0;
      continue;
    }
    D = 1.f / D;
    nx = nx - half_x;
    ny = ny - half_y;
    float pdx = 0.f;
    for (int j = 0; j < g.max_count; j++) {
      const int inx = (int)floorf(nx), iny = (int)floorf(ny);
      if (inx < -kLkWinW || inx >= v.w || iny < -kLkWinH || iny >= v.h) {
        if (level == 0) st = 0;
        break;
      }
      q = lk_weights(nx - (float)inx, ny - (float)iny);
      int diff = 0;
      if (own) diff = lk_patch(J, v.w, v.h, inx + wx, iny + wy, q) - ival;
      const float ib1 = lk_ordered_sum((float)(diff * ixval));
      const float ib2 = lk_ordered_sum((float)(diff * iyval));
      const float b1 = ib1 * FLT_SCALE, b2 = ib2 * FLT_SCALE;
      const float m1 = A12 * b2, m2 = A22 * b1;
      float dx = m1 - m2;
      dx = dx * D;
      const float dy = 0.f;
      nx = nx + dx;
      ny = ny + dy;
      outx = nx + half_x;
      outy = ny + half_y;
      if ((double)dx * (double)dx + (double)dy * (double)dy <= g.eps2) break;
      if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + 0.f) < 0.01) {
        outx = outx - dx * 0.5f;
        outy = outy - dy * 0.5f;
        break;
      }
      pdx = dx;
    }
  }
  if (g.gate && st) {   // Stereo.cpp:41-48
    const float d = ptx - outx;
    if (d <= g.min_disp || d > g.max_disp) st = 0;
  }
  if (lane == 0) {
    right_pts[2 * slot] = outx;
    right_pts[2 * slot + 1] = outy;
    status[slot] = (uint8_t)st;
    if (err) err[slot] = e;
  }
}

// index of the last level buildOpticalFlowPyramid keeps, and every level's size
static int lk_plan_levels(int w, int h, int max_level, int lw[kLkMaxLevels], int lh[kLkMaxLevels]) {
  int level = 0;
  lw[0] = w;
  lh[0] = h;
  for (; level < max_level && level < kLkMaxLevels - 1; level++) {
    w = (w + 1) / 2;
    h = (h + 1) / 2;
    if (w <= kLkWinW || h <= kLkWinH) break;
    lw[level + 1] = w;
    lh[level + 1] = h;
  }
  return level;
}

static inline dim3 lk_grid(int w, int h, int frames) { return dim3((w + 31) / 32, (h + 7) / 8, frames); }

static int lk_check(const sbm_lk_params* p, int n, int width, int height) {
  const int st = sbm_lk_params_validate(p, width, height);
  if (st != SBM_OK) return st;
  return (size_t)n > kLkMaxGridZ ? SBM_ERR_UNSUPPORTED : SBM_OK;
}

enum LkStage { kLkPyramid, kLkTrack, kLkTotal, kLkStageCount };
static const char* const kLkNames[] = {"lk_pyramid", "lk_track", "lk_total"};
StageTable lk_stages() { return stage_table<kLkStageCount, kLkStageCount>(kLkNames); }

// Pyramids and tracker of n pairs on the handle's stream, chunk by chunk; profiling times them.
static int lk_run(sbm_handle* h, int n, const uint8_t* d_left, const uint8_t* d_right, int W, int H, const float* d_kpts,
                  const int* d_count, int cap, const sbm_lk_params* p, float* d_right_pts, uint8_t* d_status, float* d_err, int sync) {
  StageClock& clk = h->lk.clock;
  HIPCHK(h, clk.start(lk_stages(), h->profiling != 0));
  int lw[kLkMaxLevels], lh[kLkMaxLevels];
  const int L = lk_plan_levels(W, H, p->max_level, lw, lh);
  size_t upper = 0, all = 0;   // pixels per frame of levels 1..L, of levels 0..L
  for (int l = 0; l <= L; l++) {
    all += (size_t)lw[l] * lh[l];
    if (l) upper += (size_t)lw[l] * lh[l];
  }
  const size_t per_pair = 2 * upper + 4 * all;   // both images' upper levels, the left's derivatives
  // a chunk also has to fit one launch: pyrDown takes BOTH images of every pair of the chunk in gridDim.z (2 C frames <= 65 535)
  const size_t fit = std::min<size_t>(std::max<size_t>(1, kLkChunkBytes / per_pair), L > 0 ? kLkMaxGridZ / 2 : kLkMaxGridZ);
  const int C = (int)std::min<size_t>(n, fit);
  // pyr: level l >= 1 of m pairs is 2 m frames (left, then right), the levels packed to the byte, and 256 bytes behind the last;
  // deriv: level l of the m left frames, a pair of shorts per pixel. Sized for a whole chunk, placed for each chunk's pairs.
  uint8_t* lev[kLkMaxLevels];
  short* der[kLkMaxLevels];
  int m = C;
  const auto pyr_layout = [&](Carve& c) {
    for (int l = 1; l <= L; l++) lev[l] = c.take<uint8_t>((size_t)lw[l] * lh[l] * 2 * m);
    c.take<uint8_t>(256);
  };
  const auto deriv_layout = [&](Carve& c) { for (int l = 0; l <= L; l++) der[l] = c.take<short>((size_t)lw[l] * lh[l] * 2 * m); };
  HIPCHK(h, carve(h->lk.pyr, h->stream, pyr_layout, 1));
  HIPCHK(h, carve(h->lk.deriv, h->stream, deriv_layout, 4));
  LkGeom g;
  memset(&g, 0, sizeof(g));
  g.L = L;
  g.cap = cap;
  g.max_count = std::min(std::max(p->max_count, 0), 100);
  double eps = std::min(std::max((double)p->epsilon, 0.), 10.);
  g.eps2 = eps * eps;
  g.min_eig = p->min_eig_threshold;
  g.gate = p->max_disparity >= 0.f;
  g.min_disp = p->min_disparity;
  g.max_disp = p->max_disparity;
  const size_t plane0 = (size_t)W * H;
  for (int c0 = 0; c0 < n; c0 += C) {
    m = std::min(C, n - c0);
    Carve pc{h->lk.pyr.as<char>(), 0, 1}, dc{h->lk.deriv.as<char>(), 0, 4};
    pyr_layout(pc), deriv_layout(dc);
    HIPCHK(h, clk.mark(kLkPyramid, h->stream));
    for (int l = 0; l <= L; l++) {
      const size_t plane = (size_t)lw[l] * lh[l];
      LkLevel& v = g.lv[l];
      v.w = lw[l];
      v.h = lh[l];
      if (l == 0) {
        v.I = d_left + plane0 * c0;
        v.J = d_right + plane0 * c0;
      } else {
        uint8_t* dst = lev[l];
        hipLaunchKernelGGL(lk_pyrdown_kernel, lk_grid(lw[l], lh[l], 2 * m), dim3(256), 0, h->stream, g.lv[l - 1].I, g.lv[l - 1].J, m, dst,
                           lw[l - 1], lh[l - 1], lw[l], lh[l]);
        HIPCHK(h, hipGetLastError());
        v.I = dst;
        v.J = dst + plane * m;
      }
      short* dd = der[l];
      hipLaunchKernelGGL(lk_scharr_kernel, lk_grid(lw[l], lh[l], m), dim3(256), 0, h->stream, v.I, dd, lw[l], lh[l]);
      HIPCHK(h, hipGetLastError());
      v.d = dd;
    }
    HIPCHK(h, clk.mark(kLkTrack, h->stream));
    hipLaunchKernelGGL(lk_track_kernel, dim3((cap + kLkWaves - 1) / kLkWaves, m), dim3(64 * kLkWaves), 0, h->stream, g, d_kpts, d_count,
                       d_right_pts, d_status, d_err, c0);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, clk.mark(kLkTotal, h->stream));
    for (int s = kLkPyramid; s < kLkTotal; s++) HIPCHK(h, clk.add(s, s, s + 1));
  }
  if (clk.on) clk.ms[kLkTotal] = clk.ms[kLkPyramid] + clk.ms[kLkTrack];
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

}  // namespace sbm

// ---- entry points --------------------------------------------------------------------------------------------------------
using namespace sbm;

extern "C" {

void sbm_lk_params_default(sbm_lk_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->win_width = kLkWinW;
  p->win_height = kLkWinH;
  p->max_level = 5;
  p->max_count = 30;
  p->epsilon = 0.01f;
  p->flags = SBM_LK_GET_MIN_EIGENVALS;
  p->min_eig_threshold = 1e-4;
  p->min_disparity = 0.5f;
  p->max_disparity = 128.f;
}

int sbm_lk_params_validate(const sbm_lk_params* p, int width, int height) {
  if (!p) return SBM_ERR_NULL;
  if (width < 2 || height < 2) return SBM_ERR_SIZE;
  if (p->win_width <= 2 || p->win_height <= 2 || p->max_level < 0) return SBM_ERR_SIZE;   // the reference's CV_Assert
  if (width > kLkMaxDim || height > kLkMaxDim) return SBM_ERR_UNSUPPORTED;
  if (p->win_width != kLkWinW || p->win_height != kLkWinH) return SBM_ERR_UNSUPPORTED;
  if ((p->flags & kLkFlagInitialFlow) || !(p->flags & kLkFlagMinEig) || (p->flags & ~(kLkFlagInitialFlow | kLkFlagMinEig)))
    return SBM_ERR_UNSUPPORTED;
  if (!std::isfinite(p->epsilon) || !std::isfinite(p->min_eig_threshold) || std::isnan(p->min_disparity) ||
      std::isnan(p->max_disparity))
    return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

int sbm_lk_pyramid_device(sbm_handle* h, int n, const void* d_img, int width, int height, int with_deriv, const sbm_lk_params* p,
                          void* d_levels, void* d_deriv, int* levels_out) {
  if (!h || !p || !d_img || !d_levels || (with_deriv && !d_deriv)) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  const int st = lk_check(p, n, width, height);
  if (st != SBM_OK) return st;
  if (with_deriv && ((uintptr_t)d_deriv & 3)) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  int lw[kLkMaxLevels], lh[kLkMaxLevels];
  const int L = lk_plan_levels(width, height, p->max_level, lw, lh);
  uint8_t* lev = (uint8_t*)d_levels;
  short* der = (short*)d_deriv;
  size_t off = 0;
  const uint8_t* prev = nullptr;
  for (int l = 0; l <= L; l++) {
    const size_t plane = (size_t)lw[l] * lh[l];
    uint8_t* dst = lev + off;
    if (l == 0) {
      HIPCHK(h, hipMemcpyAsync(dst, d_img, plane * n, hipMemcpyDeviceToDevice, h->stream));   // level 0 is the frame
    } else {
      hipLaunchKernelGGL(lk_pyrdown_kernel, lk_grid(lw[l], lh[l], n), dim3(256), 0, h->stream, prev, prev, n, dst, lw[l - 1], lh[l - 1],
                         lw[l], lh[l]);
    }
    HIPCHK(h, hipGetLastError());
    if (with_deriv) {
      hipLaunchKernelGGL(lk_scharr_kernel, lk_grid(lw[l], lh[l], n), dim3(256), 0, h->stream, dst, der + 2 * off, lw[l], lh[l]);
      HIPCHK(h, hipGetLastError());
    }
    prev = dst;
    off += plane * n;
  }
  if (levels_out) *levels_out = L;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_lk_stereo_device(sbm_handle* h, int n, const void* d_left, const void* d_right, int width, int height, const void* d_kpts,
                         const void* d_count, int cap, const sbm_lk_params* p, void* d_right_pts, void* d_status, void* d_err,
                         int sync) {
  if (!h || !p || !d_left || !d_right || !d_kpts || !d_count || !d_right_pts || !d_status) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  const int st = lk_check(p, n, width, height);
  if (st != SBM_OK) return st;
  if (cap < 1) return SBM_ERR_SIZE;
  if (((uintptr_t)d_kpts & 3) || ((uintptr_t)d_right_pts & 3) || ((uintptr_t)d_err & 3) || ((uintptr_t)d_count & 3))
    return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  return lk_run(h, n, (const uint8_t*)d_left, (const uint8_t*)d_right, width, height, (const float*)d_kpts, (const int*)d_count, cap, p,
                (float*)d_right_pts, (uint8_t*)d_status, (float*)d_err, sync);
}

int sbm_lk_stereo(sbm_handle* h, const uint8_t* left, size_t left_stride, const uint8_t* right, size_t right_stride, int width,
                  int height, const float* pts, int npts, const sbm_lk_params* p, float* right_pts, uint8_t* status, float* err) {
  if (!h || !p || !left || !right || (npts > 0 && (!pts || !right_pts || !status))) return SBM_ERR_NULL;
  int st = lk_check(p, 1, width, height);
  if (st != SBM_OK) return st;
  if (npts < 0 || left_stride < (size_t)width || right_stride < (size_t)width) return SBM_ERR_SIZE;
  if (npts == 0) return SBM_OK;   // the reference releases its outputs and returns
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = ensure_staging(h, 1, width, height);
  if (st != SBM_OK) return st;
  const size_t np = (size_t)npts;
  float *d_p = nullptr, *d_r = nullptr, *d_e = nullptr;
  int* d_n = nullptr;
  uint8_t* d_s = nullptr;
  HIPCHK(h, carve(h->lk.io, h->stream, [&](Carve& c) {
    d_p = c.take<float>(2 * np);   // points
    d_r = c.take<float>(2 * np);   // right points
    d_e = c.take<float>(np);       // errors
    d_n = c.take<int>(4);          // count (16 bytes)
    d_s = c.take<uint8_t>(np);     // status
  }));
  HIPCHK(h, hipMemcpy2DAsync(h->st.l.p, width, left, left_stride, width, height, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpy2DAsync(h->st.r.p, width, right, right_stride, width, height, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_p, pts, np * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_n, &npts, sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // npts lives on this frame
  st = lk_run(h, 1, h->st.l.as<uint8_t>(), h->st.r.as<uint8_t>(), width, height, d_p, d_n, npts, p, d_r, d_s, d_e, 0);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpyAsync(right_pts, d_r, np * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(status, d_s, np, hipMemcpyDeviceToHost, h->stream));
  if (err) HIPCHK(h, hipMemcpyAsync(err, d_e, np * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

int sbm_keypoints3d_lk_device(sbm_handle* h, int n, const void* d_kpts, const void* d_right_pts, const void* d_status,
                              const void* d_count, int cap, const sbm_stereo_model* model, float min_depth, float max_depth,
                              void* d_xyz, int sync) {
  if (!h || !d_kpts || !d_right_pts || !d_status || !d_count || !model || !d_xyz) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (cap < 1) return SBM_ERR_SIZE;
  if (n > 65535 || ((uintptr_t)d_kpts & 3) || ((uintptr_t)d_right_pts & 3) || ((uintptr_t)d_xyz & 3) || ((uintptr_t)d_count & 3))
    return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, launch_keypoints3d_lk((const float*)d_kpts, (const float*)d_right_pts, (const uint8_t*)d_status, (const int*)d_count, n, cap,
                                  *model, min_depth, max_depth, (float*)d_xyz, h->stream));
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

}  // extern "C"
