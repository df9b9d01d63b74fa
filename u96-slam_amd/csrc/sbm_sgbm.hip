// sbm_sgbm.hip -- kernels of the semi-global matcher (cv::StereoSGBM, MODE_HH / MODE_SGBM; include/sbm.h).
//
// Stages, one launch each, all on the handle's stream:
//   cost    sgbm_hsum_kernel: per row, the two Birchfield-Tomasi channels (clipped x-Sobel, raw >> 2) and their horizontal
//           box sum over the width1 computable columns (clamped) -> hsum (int16, in the S buffer);
//           sgbm_vsum_kernel: per (column, disparity) the vertical box sum walked down the rows, + P2 -> C (int16), with
//           OpenCV's incremental-sum behaviour at the bottom rows.
//   paths   sgbm_path_kernel: one wavefront per path (a row, a column or a diagonal of the width1 x H grid), the disparities
//           across the lanes (NV contiguous ones per lane), the steps of the path in order. Inside the exactness envelope every
//           path cost is non-negative, so S = min(32767, sum over paths) is accumulated with a saturating add in any order;
//           the first path writes S, the others read-add-write it.
//   select  sgbm_select_kernel: one workgroup per row: winner, uniqueness, sub-pixel, claims (an LDS table of
//           (cost << 16 | 0xffff - x) keys: lowest cost wins, among equal costs the highest x -- what OpenCV's descending
//           x loop with a strict `>` leaves), then the LR check -> the map before the median.
//   median  sgbm_median_kernel: 3x3, replicated border.
// The speckle filter is the block matcher's (launch_speckle).
#include <algorithm>

#include "sbm_handle.h"

namespace sbm {

constexpr int kReadSgbmNoMedian = 32;        // SBM_CV_READING: no medianBlur stage
constexpr int kReadSgbmBottomClamped = 64;   // SBM_CV_READING: rows with y + SH2 >= H (y > 0) sum a clamped window
constexpr int kSgbmNdMax = 512, kSgbmWMax = 8192;

namespace {

constexpr int kMaxCost = 32767;

__device__ inline int bt_cost(const uint8_t* __restrict__ a, int X, const uint8_t* __restrict__ b, int X2, int W) {
  const int u = a[X];
  const int ul = X > 0 ? (u + a[X - 1]) >> 1 : u, ur = X < W - 1 ? (u + a[X + 1]) >> 1 : u;
  const int u0 = min(min(ul, ur), u), u1 = max(max(ul, ur), u);
  const int v = b[X2];
  const int vl = X2 > 0 ? (v + b[X2 - 1]) >> 1 : v, vr = X2 < W - 1 ? (v + b[X2 + 1]) >> 1 : v;
  const int v0 = min(min(vl, vr), v), v1 = max(max(vl, vr), v);
  const int c0 = max(max(0, u - v1), v0 - u), c1 = max(max(0, v - u1), u0 - v);
  return min(c0, c1);
}

// one block per (row, pair); LDS: the two channels of both images (4 * W bytes)
constexpr int kHsumSeg = 64;   // output columns per sliding window
__global__ void __launch_bounds__(256) sgbm_hsum_kernel(const uint8_t* __restrict__ left, const uint8_t* __restrict__ right,
                                                        int16_t* __restrict__ hsum, const SgbmGeom g) {
  extern __shared__ uint8_t sh[];
  const int W = g.W, H = g.H, y = blockIdx.x, p = blockIdx.y;
  uint8_t* ch = sh;   // [0]: sobel L, [W]: raw L, [2W]: sobel R, [3W]: raw R
  for (int side = 0; side < 2; side++) {
    const uint8_t* r = (side ? right : left) + ((size_t)p * H + y) * W;
    const uint8_t* ru = y > 0 ? r - W : r;
    const uint8_t* rd = y < H - 1 ? r + W : r;
    uint8_t* sob = ch + 2 * side * W;
    uint8_t* raw = sob + W;
    for (int X = threadIdx.x; X < W; X += blockDim.x) {
      if (X == 0 || X == W - 1) {
        sob[X] = raw[X] = (uint8_t)g.ftzero;
      } else {
        const int s = (r[X + 1] - r[X - 1]) * 2 + ru[X + 1] - ru[X - 1] + rd[X + 1] - rd[X - 1];
        sob[X] = (uint8_t)(min(max(s, -g.ftzero), g.ftzero) + g.ftzero);
        raw[X] = r[X];
      }
    }
  }
  __syncthreads();
  const int D = g.D, W1 = g.W1, r2 = g.SW2;
  const int nseg = (W1 + kHsumSeg - 1) / kHsumSeg;
  int16_t* out = hsum + ((size_t)p * H + y) * W1 * D;
  for (int task = threadIdx.x; task < D * nseg; task += blockDim.x) {
    const int d = task % D, seg = task / D;
    const int x0 = seg * kHsumSeg, x1 = min(x0 + kHsumSeg, W1);
    const int shift = g.minX1 - g.minD - d;   // X2 = X - disparity = x + minX1 - minD - d
    auto pix = [&](int x) {
      x = min(max(x, 0), W1 - 1);
      const int X = g.minX1 + x, X2 = x + shift;
      return bt_cost(ch, X, ch + 2 * W, X2, W) + (bt_cost(ch + W, X, ch + 3 * W, X2, W) >> 2);
    };
    int sum = 0;
    for (int j = -r2; j <= r2; j++) sum += pix(x0 + j);
    out[(size_t)x0 * D + d] = (int16_t)sum;
    for (int x = x0 + 1; x < x1; x++) {
      sum += pix(x + r2) - pix(x - r2 - 1);
      out[(size_t)x * D + d] = (int16_t)sum;
    }
  }
}

// one thread per (column, disparity) of a pair, walking the rows
__global__ void __launch_bounds__(256) sgbm_vsum_kernel(const int16_t* __restrict__ hsum, int16_t* __restrict__ C, const SgbmGeom g) {
  const int plane = g.W1 * g.D;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= plane) return;
  const int H = g.H, r2 = g.SW2;
  const size_t base = (size_t)blockIdx.y * H * plane + i;
  const int16_t* h = hsum + base;
  int16_t* c = C + base;
  auto hr = [&](int k) { return (int)h[(size_t)k * plane]; };
  int sum = (r2 + 1) * hr(0);
  for (int k = 1; k <= r2; k++) sum += hr(min(k, H - 1));
  c[0] = (int16_t)(g.P2 + sum);
  const bool clamped = (g.reading & kReadSgbmBottomClamped) != 0;
  for (int y = 1; y < H; y++) {
    if (y + r2 < H || clamped) {
      sum += hr(min(y + r2, H - 1)) - hr(max(y - r2 - 1, 0));
      c[(size_t)y * plane] = (int16_t)(g.P2 + sum);
    } else {
      // OpenCV's incremental box sum stops at the last row: MODE_HH keeps the row's initial P2, MODE_SGBM's single C row
      // keeps the previous row's costs
      c[(size_t)y * plane] = (int16_t)(g.fullDP ? g.P2 : g.P2 + sum);
    }
  }
}

__device__ inline int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

template <int NV>
struct VecOf;
template <> struct VecOf<1> { typedef short T __attribute__((ext_vector_type(1))); };
template <> struct VecOf<2> { typedef short T __attribute__((ext_vector_type(2))); };
template <> struct VecOf<4> { typedef short T __attribute__((ext_vector_type(4))); };
template <> struct VecOf<8> { typedef short T __attribute__((ext_vector_type(8))); };

// One wavefront per path. Paths of direction (sx, sy) -- a step from the previous pixel (x - sx, y - sy) to (x, y) -- start
// where that previous pixel is outside the width1 x H grid, with L = 0 and min L = 0 (OpenCV's cleared borders).
template <int NV>
__global__ void __launch_bounds__(256) sgbm_path_kernel(const int16_t* __restrict__ C, int16_t* __restrict__ S, const SgbmGeom g,
                                                        int sx, int sy, int first) {
  typedef typename VecOf<NV>::T V;
  constexpr int PF = 4;   // steps loaded ahead
  const int lane = threadIdx.x & 63;
  const int chain = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  const int W1 = g.W1, H = g.H, D = g.D;
  int x, y, len;
  if (sy == 0) {
    if (chain >= H) return;
    y = chain; x = sx > 0 ? 0 : W1 - 1; len = W1;
  } else if (sx == 0) {
    if (chain >= W1) return;
    x = chain; y = sy > 0 ? 0 : H - 1; len = H;
  } else {
    if (chain >= W1 + H - 1) return;
    const int y0 = sy > 0 ? 0 : H - 1, x0 = sx > 0 ? 0 : W1 - 1;
    if (chain < W1) { x = chain; y = y0; }
    else { x = x0; y = y0 + sy * (chain - W1 + 1); }
    len = min(sx > 0 ? W1 - x : x + 1, sy > 0 ? H - y : y + 1);
  }
  const long step = ((long)sy * W1 + sx) * D;
  const int dlo = lane * NV;
  const bool active = dlo < D;
  const size_t off0 = ((size_t)blockIdx.y * H + y) * W1 * D + (size_t)x * D + (active ? dlo : 0);
  const V* Cp = reinterpret_cast<const V*>(C + off0);
  V* Sp = reinterpret_cast<V*>(S + off0);
  const long vstep = step / NV;   // D is a multiple of NV
  const int P1 = g.P1, P2 = g.P2;

  V cbuf[PF], sbuf[PF];
#pragma unroll
  for (int j = 0; j < PF; j++)
    if (j < len && active) {
      cbuf[j] = Cp[j * vstep];
      if (!first) sbuf[j] = Sp[j * vstep];
    }
  int Lp[NV];
#pragma unroll
  for (int k = 0; k < NV; k++) Lp[k] = 0;
  int minLp = 0;
  for (int t0 = 0; t0 < len; t0 += PF) {
#pragma unroll
    for (int j = 0; j < PF; j++) {
      const int t = t0 + j;
      if (t >= len) break;
      const V c = cbuf[j];
      const V s = sbuf[j];
      if (t + PF < len && active) {
        cbuf[j] = Cp[(t + PF) * vstep];
        if (!first) sbuf[j] = Sp[(t + PF) * vstep];
      }
      const int left = __shfl_up(Lp[NV - 1], 1);
      const int right = __shfl_down(Lp[0], 1);
      const int delta = minLp + P2;
      int L[NV];
      int m = kMaxCost;
#pragma unroll
      for (int k = 0; k < NV; k++) {
        const int lv = k > 0 ? Lp[k - 1] : (dlo == 0 ? kMaxCost : left);
        const int rv = k < NV - 1 ? Lp[k + 1] : (dlo + NV >= D ? kMaxCost : right);
        L[k] = (int)c[k] + min(Lp[k], min(lv + P1, min(rv + P1, delta))) - delta;
        m = min(m, L[k]);
      }
      minLp = wave_min(active ? m : kMaxCost);
      if (active) {
        V o;
#pragma unroll
        for (int k = 0; k < NV; k++) o[k] = (short)(first ? L[k] : min(kMaxCost, (int)s[k] + L[k]));
        Sp[t * vstep] = o;
      }
#pragma unroll
      for (int k = 0; k < NV; k++) Lp[k] = L[k];
    }
  }
}

// one workgroup per (row, pair); LDS: W claim keys + W map entries
constexpr unsigned kNoClaim = 0x7fffffffu;
template <int NV>
__global__ void __launch_bounds__(256) sgbm_select_kernel(const int16_t* __restrict__ S, int16_t* __restrict__ pre, const SgbmGeom g) {
  extern __shared__ unsigned char smem[];
  const int W = g.W, H = g.H, D = g.D, W1 = g.W1, y = blockIdx.x, p = blockIdx.y;
  unsigned* keys = reinterpret_cast<unsigned*>(smem);
  int16_t* row = reinterpret_cast<int16_t*>(keys + W);
  const int inv = (g.minD - 1) * 16;
  for (int X = threadIdx.x; X < W; X += blockDim.x) { keys[X] = kNoClaim; row[X] = (int16_t)inv; }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dlo = lane * NV;
  const bool active = dlo < D;
  const int16_t* Srow = S + ((size_t)p * H + y) * W1 * D;
  for (int x = wave; x < W1; x += (int)(blockDim.x >> 6)) {
    int s[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) s[k] = active ? Srow[(size_t)x * D + dlo + k] : kMaxCost;
    int key = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < NV; k++) key = min(key, (s[k] << 16) | (dlo + k));   // lowest S, then lowest d
    key = wave_min(key);
    const int minS = key >> 16, best = key & 0xffff;
    // S saturated at every disparity: OpenCV's winner loop (strict `<` against a start of MAX_COST) keeps bestDisp = -1. Such a
    // pixel is rejected by uniqueness or written as -16 + minD * 16 = invalid, and its claim (cost MAX_COST) can never be taken:
    // either way it stays invalid and claims nothing
    if (minS == kMaxCost) continue;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const int d = dlo + k;
      bad |= active && s[k] * (100 - g.uniq) < minS * 100 && abs(best - d) > 1;
    }
    if (__any(bad)) continue;
    // S[best - 1] and S[best + 1] from the lanes that hold them
    const int bm = max(best - 1, 0), bp = min(best + 1, D - 1);
    int vm = 0, vp = 0;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      if (k == bm % NV) vm = s[k];
      if (k == bp % NV) vp = s[k];
    }
    vm = __shfl(vm, bm / NV);
    vp = __shfl(vp, bp / NV);
    if (lane == 0) {
      const int x2 = x + g.minX1 - best - g.minD;
      atomicMin(&keys[x2], ((unsigned)minS << 16) | (unsigned)(0xffff - x));
      int d;
      if (0 < best && best < D - 1) {
        const int denom2 = max(vm + vp - 2 * minS, 1);
        d = best * 16 + ((vm - vp) * 16 + denom2) / (denom2 * 2);
      } else {
        d = best * 16;
      }
      row[x + g.minX1] = (int16_t)(d + g.minD * 16);
    }
  }
  __syncthreads();
  int16_t* out = pre + ((size_t)p * H + y) * W;
  for (int X = threadIdx.x; X < W; X += blockDim.x) {
    int v = row[X];
    if (v != inv && X >= g.minX1 && X < g.maxX1) {
      const int d_lo = v >> 4, d_hi = (v + 15) >> 4;
      const int xa = X - d_lo, xb = X - d_hi;
      auto disp2 = [&](int xt) {
        const unsigned k = keys[xt];
        return k == kNoClaim ? inv : (int)(0xffff - (k & 0xffff)) + g.minX1 - xt;
      };
      if (0 <= xa && xa < W && 0 <= xb && xb < W) {
        const int da = disp2(xa), db = disp2(xb);
        if (da >= g.minD && abs(da - d_lo) > g.d12 && db >= g.minD && abs(db - d_hi) > g.d12) v = inv;
      }
    }
    out[X] = (int16_t)v;
  }
}

#define SGBM_OP(a, b) { const int t_ = min(a, b); b = max(a, b); a = t_; }
__global__ void __launch_bounds__(256) sgbm_median_kernel(const int16_t* __restrict__ src, int16_t* __restrict__ dst, int W, int H) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (X >= W) return;
  const int16_t* s = src + ((size_t)blockIdx.z * H) * W;
  const int xl = max(X - 1, 0), xr = min(X + 1, W - 1);
  const int16_t* r0 = s + (size_t)max(y - 1, 0) * W;
  const int16_t* r1 = s + (size_t)y * W;
  const int16_t* r2 = s + (size_t)min(y + 1, H - 1) * W;
  int p0 = r0[xl], p1 = r0[X], p2 = r0[xr], p3 = r1[xl], p4 = r1[X], p5 = r1[xr], p6 = r2[xl], p7 = r2[X], p8 = r2[xr];
  SGBM_OP(p1, p2); SGBM_OP(p4, p5); SGBM_OP(p7, p8); SGBM_OP(p0, p1); SGBM_OP(p3, p4); SGBM_OP(p6, p7); SGBM_OP(p1, p2);
  SGBM_OP(p4, p5); SGBM_OP(p7, p8); SGBM_OP(p0, p3); SGBM_OP(p5, p8); SGBM_OP(p4, p7); SGBM_OP(p3, p6); SGBM_OP(p1, p4);
  SGBM_OP(p2, p5); SGBM_OP(p4, p7); SGBM_OP(p4, p2); SGBM_OP(p6, p4); SGBM_OP(p4, p2);
  dst[((size_t)blockIdx.z * H + y) * W + X] = (int16_t)p4;
}
#undef SGBM_OP

__global__ void __launch_bounds__(256) sgbm_fill_kernel(int16_t* __restrict__ dst, size_t count, int v) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) dst[i] = (int16_t)v;
}

template <typename F>
hipError_t with_nv(int D, F f) {
  if (D <= 64) return f(std::integral_constant<int, 1>{});
  if (D <= 128) return f(std::integral_constant<int, 2>{});
  if (D <= 256) return f(std::integral_constant<int, 4>{});
  return f(std::integral_constant<int, 8>{});
}

}  // namespace

static hipError_t launch_sgbm_cost(const uint8_t* left, const uint8_t* right, int16_t* hsum, int16_t* C, const SgbmGeom& g, hipStream_t s) {
  hipLaunchKernelGGL(sgbm_hsum_kernel, dim3(g.H, g.n), dim3(256), (size_t)4 * g.W, s, left, right, hsum, g);
  const int plane = g.W1 * g.D;
  hipLaunchKernelGGL(sgbm_vsum_kernel, dim3((plane + 255) / 256, g.n), dim3(256), 0, s, hsum, C, g);
  return hipGetLastError();
}

static hipError_t launch_sgbm_paths(const int16_t* C, int16_t* S, const SgbmGeom& g, hipStream_t s) {
  // the pass-1 directions of OpenCV's sweep, then pass 2 (MODE_HH) or the fifth path (MODE_SGBM)
  static const int kDirs[8][2] = {{1, 0}, {1, 1}, {0, 1}, {-1, 1}, {-1, 0}, {-1, -1}, {0, -1}, {1, -1}};
  const int ndir = g.fullDP ? 8 : 5;
  for (int i = 0; i < ndir; i++) {
    const int sx = kDirs[i][0], sy = kDirs[i][1];
    const int nchains = sy == 0 ? g.H : (sx == 0 ? g.W1 : g.W1 + g.H - 1);
    const dim3 grid((nchains + 3) / 4, g.n);
    hipError_t e = with_nv(g.D, [&](auto nv) {
      constexpr int NV = decltype(nv)::value;
      hipLaunchKernelGGL(sgbm_path_kernel<NV>, grid, dim3(256), 0, s, C, S, g, sx, sy, i == 0 ? 1 : 0);
      return hipGetLastError();
    });
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

static hipError_t launch_sgbm_select(const int16_t* S, int16_t* pre, const SgbmGeom& g, hipStream_t s) {
  return with_nv(g.D, [&](auto nv) {
    constexpr int NV = decltype(nv)::value;
    hipLaunchKernelGGL(sgbm_select_kernel<NV>, dim3(g.H, g.n), dim3(256), (size_t)6 * g.W, s, S, pre, g);
    return hipGetLastError();
  });
}

static hipError_t launch_sgbm_median(const int16_t* src, int16_t* dst, int n, int W, int H, hipStream_t s) {
  hipLaunchKernelGGL(sgbm_median_kernel, dim3((W + 255) / 256, H, n), dim3(256), 0, s, src, dst, W, H);
  return hipGetLastError();
}

static hipError_t launch_sgbm_fill(int16_t* dst, size_t count, int v, hipStream_t s) {
  const size_t blocks = std::min<size_t>((count + 255) / 256, 65535);
  hipLaunchKernelGGL(sgbm_fill_kernel, dim3((unsigned)std::max<size_t>(blocks, 1)), dim3(256), 0, s, dst, count, v);
  return hipGetLastError();
}

}  // namespace sbm

// ---- entry points --------------------------------------------------------------------------------------------------------
using namespace sbm;

enum SgbmStage { kSgCost, kSgAggregate, kSgSelect, kSgMedian, kSgSpeckle, kSgTotal, kSgStageCount };
static const char* const kSgbmNames[] = {"sgbm_cost", "sgbm_aggregate", "sgbm_select", "sgbm_median", "sgbm_speckle", "sgbm_total"};
StageTable sbm::sgbm_stages() { return stage_table<kSgStageCount, kSgStageCount>(kSgbmNames); }

extern "C" {

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

// Device scratch of one chunk of pairs -- C, S, the map before the median and (speckle filter on) its scratch -- stays within
// kSgbmChunkBytes; a single pair larger than that runs alone.
static constexpr size_t kSgbmChunkBytes = (size_t)2 << 30;

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
  const size_t pair_bytes = 2 * pair_cs + npix * sizeof(int16_t) + (speckle ? SpeckleScratch::bytes(1, width, height, nullptr) : 0);
  const int chunk = (int)std::min<size_t>(n, std::max<size_t>(1, kSgbmChunkBytes / pair_bytes));
  auto& sgs = h->sg;
  HIPCHK(h, sgs.C.grow(pair_cs * chunk, h->stream));
  HIPCHK(h, sgs.S.grow(pair_cs * chunk, h->stream));
  HIPCHK(h, sgs.pre.grow((size_t)chunk * npix * sizeof(int16_t), h->stream));
  if (speckle) HIPCHK(h, sgs.spk.ensure(chunk, width, height, h->stream));
  g.n = n;
  sgs.last = g;
  sgs.have_last = true;
  sgs.last_one_chunk = chunk == n;
  int16_t *C = sgs.C.as<int16_t>(), *S = sgs.S.as<int16_t>(), *pre = sgs.pre.as<int16_t>();

  StageClock& clk = sgs.clock;
  HIPCHK(h, clk.start(sgbm_stages(), h->profiling != 0));
  const uint8_t* dl = (const uint8_t*)d_left;
  const uint8_t* dr = (const uint8_t*)d_right;
  const int inv = (g.minD - 1) * 16;
  const int max_diff = (int)std::min<long>(16L * p->speckle_range, 1L << 17);
  // every stage, the median and the speckle filter included, runs chunk by chunk
  for (int c0 = 0; c0 < n; c0 += chunk) {
    SgbmGeom gc = g;
    gc.n = std::min(chunk, n - c0);
    int16_t* out = (int16_t*)d_disp + (size_t)c0 * npix;
    HIPCHK(h, clk.mark(kSgCost, h->stream));
    if (pair_cs) {
      HIPCHK(h, launch_sgbm_cost(dl + (size_t)c0 * npix, dr + (size_t)c0 * npix, S, C, gc, h->stream));
      HIPCHK(h, clk.mark(kSgAggregate, h->stream));
      HIPCHK(h, launch_sgbm_paths(C, S, gc, h->stream));
      HIPCHK(h, clk.mark(kSgSelect, h->stream));
      HIPCHK(h, launch_sgbm_select(S, pre, gc, h->stream));
    } else {   // no computable column: every pixel is invalid (the median and the speckle filter keep it so)
      HIPCHK(h, clk.mark(kSgAggregate, h->stream));
      HIPCHK(h, clk.mark(kSgSelect, h->stream));
      HIPCHK(h, launch_sgbm_fill(pre, (size_t)gc.n * npix, inv, h->stream));
    }
    HIPCHK(h, clk.mark(kSgMedian, h->stream));
    if (g.reading & kReadSgbmNoMedian)
      HIPCHK(h, hipMemcpyAsync(out, pre, (size_t)gc.n * npix * sizeof(int16_t), hipMemcpyDeviceToDevice, h->stream));
    else
      HIPCHK(h, launch_sgbm_median(pre, out, gc.n, width, height, h->stream));
    HIPCHK(h, clk.mark(kSgSpeckle, h->stream));
    if (speckle) {
      // the block matcher's filter, with cv::StereoSGBM's arguments: newVal = (minD - 1) * 16, maxDiff = 16 * speckleRange (the
      // block matcher's own x16 reading bit does not apply here)
      Geom sg;
      memset(&sg, 0, sizeof(sg));
      sg.W = width; sg.H = height; sg.n = gc.n; sg.filtered = inv; sg.reading = 0;
      SpkPlan k;
      speckle_plan(sg, p->speckle_window_size, max_diff, &k);
      HIPCHK(h, launch_speckle(out, sgs.spk, sg, k, p->speckle_window_size, h->stream));
    }
    HIPCHK(h, clk.mark(kSgTotal, h->stream));
    for (int s = kSgCost; s < kSgTotal; s++) HIPCHK(h, clk.add(s, s, s + 1));
    HIPCHK(h, clk.add(kSgTotal, kSgCost, kSgTotal));
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
  HIPCHK(h, hipMemcpy2DAsync(h->st.l.as<uint8_t>(), width, left, left_stride, width, height, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpy2DAsync(h->st.r.as<uint8_t>(), width, right, right_stride, width, height, hipMemcpyHostToDevice, h->stream));
  st = sbm_sgbm_compute_device(h, p, 1, h->st.l.as<uint8_t>(), h->st.r.as<uint8_t>(), width, height, h->st.d.as<int16_t>(), 0);
  if (st != SBM_OK) return st;
  HIPCHK(h, hipMemcpy2DAsync(disp, disp_stride, h->st.d.as<int16_t>(), (size_t)width * 2, (size_t)width * 2, height, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}

}  // extern "C"

// sbm_debug_fetch of the last call: which = 4 (C), 5 (S), 6 (the map before the median); one chunk only
int sbm::sgbm_debug_fetch(sbm_handle* h, int which, void* dst, size_t dst_bytes) {
  if (!h->sg.have_last) return SBM_ERR_UNSUPPORTED;
  const SgbmGeom& g = h->sg.last;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (!h->sg.last_one_chunk) return SBM_ERR_UNSUPPORTED;
  if (which == 6) {
    const size_t bytes = (size_t)g.n * g.W * g.H * sizeof(int16_t);
    if (dst_bytes < bytes) return SBM_ERR_SIZE;
    HIPCHK(h, hipMemcpy(dst, h->sg.pre.p, bytes, hipMemcpyDeviceToHost));
    return SBM_OK;
  }
  if (g.W1 < 1) return SBM_ERR_UNSUPPORTED;
  const size_t bytes = (size_t)g.n * g.H * g.W1 * g.D * sizeof(int16_t);
  if (dst_bytes < bytes) return SBM_ERR_SIZE;
  HIPCHK(h, hipMemcpy(dst, which == 4 ? h->sg.C.p : h->sg.S.p, bytes, hipMemcpyDeviceToHost));
  return SBM_OK;
}
