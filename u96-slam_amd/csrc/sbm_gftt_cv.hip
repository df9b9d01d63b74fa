// sbm_gftt_cv.hip -- the reference's generateKeypoints() (src/slam/src/core/GFTT.cpp:11-25: cv::GFTTDetector, i.e.
// cv::goodFeaturesToTrack) on gfx950. The arithmetic is the text of include/sbm.h ("GFTT keypoints of OpenCV"); this file is
// compiled with -ffp-contract=off, and every fused multiply-add that bit 512 of SBM_CV_READING asks for is spelled fmaf.
//
//   gftt_cv_map_kernel     256 threads per 64 x 16 tile of a frame: the tile with a 2-pixel halo (reflect-101) goes to LDS as
//                          bytes, the three derivative products of the tile plus a 1-pixel halo (reflect-101 of the PRODUCT
//                          plane) to LDS as floats, then every thread sums the 3 x 3 boxes of four neighbouring pixels in double,
//                          takes the eigenvalue, stores 16 bytes and joins a wavefront-then-workgroup maximum that ends in one
//                          atomicMax per workgroup on the order-preserving key of the float. 1 B read and 4 B written per pixel.
//   gftt_cv_max_kernel     key -> float, for the caller's d_max.
//   gftt_cv_cand_kernel    threshold + 3 x 3 local maximum on the float map; a candidate appends (key << 32 | raster index) to
//                          its frame's list (one atomicAdd per workgroup of 4096 pixels). The thresholded map is never stored.
//   gftt_cv_select_kernel  one workgroup of 1024 threads per frame: bitonic sort of the list, descending (in LDS when it fits
//                          the key window, else in place in device memory: every interior pixel of a 2048 x 2048 frame can be a
//                          candidate), then the trim of sbm_gftt_trim.h by wave 0.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "sbm_handle.h"
#include "sbm_gftt_trim.h"

namespace sbm {

constexpr int kReadGfttCvFused = 512;   // SBM_CV_READING: the scaled three-tap and the radicand are fused multiply-adds

constexpr int GC_TW = 64, GC_TH = 16;                   // output tile
constexpr int GC_IW = GC_TW + 4, GC_IH = GC_TH + 4;     // image tile (2-pixel halo)
constexpr int GC_IP = 72;                               // its pitch in bytes
constexpr int GC_PW = GC_TW + 2, GC_PH = GC_TH + 2;     // product tile (1-pixel halo)
constexpr int GC_PP = 67;                               // its pitch in floats (odd: rows of a wavefront spread over the banks)
constexpr size_t kGcChunkBytes = (size_t)256 << 20;     // key lists (and maps) of one chunk of frames

// BORDER_REFLECT_101, then clamped: positions more than one pixel outside the frame never reach a result.
__device__ __forceinline__ int gc_reflect(int p, int n) {
  if (p < 0) p = -p;
  if (p >= n) p = 2 * (n - 1) - p;
  return min(max(p, 0), n - 1);
}

// The order-preserving key of a float (numeric order, -0 below +0) and back.
__device__ __forceinline__ unsigned gc_key(float v) {
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ float gc_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

template <bool FUSED>
__device__ __forceinline__ float gc_tap(float c, float q, float f0, float f1) {
  if constexpr (FUSED) return fmaf(f1, q, f0 * c);
  else return f1 * q + f0 * c;
}

template <bool FUSED>
__global__ void __launch_bounds__(256) gftt_cv_map_kernel(const uint8_t* __restrict__ img, float* __restrict__ eig,
                                                          unsigned* __restrict__ keymax, int W, int H, int tx, float f1, int vec) {
  __shared__ uint8_t im[GC_IH][GC_IP];
  __shared__ float pr[3][GC_PH][GC_PP];
  __shared__ unsigned wmax[4];
  const int tid = threadIdx.x;
  const int x0 = (int)(blockIdx.x % (unsigned)tx) * GC_TW, y0 = (int)(blockIdx.x / (unsigned)tx) * GC_TH;
  const size_t plane = (size_t)W * H;
  const uint8_t* src = img + blockIdx.y * plane;
  float* dst = eig + blockIdx.y * plane;
  const float f0 = 2.f * f1;

  for (int i = tid; i < GC_IH * GC_IW; i += 256) {
    const int ly = i / GC_IW, lx = i - ly * GC_IW;
    im[ly][lx] = src[(size_t)gc_reflect(y0 - 2 + ly, H) * W + gc_reflect(x0 - 2 + lx, W)];
  }
  __syncthreads();
  for (int i = tid; i < GC_PH * GC_PW; i += 256) {
    const int py = i / GC_PW, px = i - py * GC_PW;
    const int gx = x0 - 1 + px, gy = y0 - 1 + py;
    float xx = 0.f, xy = 0.f, yy = 0.f;
    if (gx <= W && gy <= H) {
      // the product at a position one outside the frame is the product AT the reflected position
      const int cx = gc_reflect(gx, W) - x0 + 2, cy = gc_reflect(gy, H) - y0 + 2;
      const int a0 = im[cy - 1][cx - 1], a1 = im[cy - 1][cx], a2 = im[cy - 1][cx + 1];
      const int b0 = im[cy][cx - 1], b2 = im[cy][cx + 1];
      const int c0 = im[cy + 1][cx - 1], c1 = im[cy + 1][cx], c2 = im[cy + 1][cx + 1];
      const float dx = gc_tap<FUSED>((float)(b2 - b0), (float)((a2 - a0) + (c2 - c0)), f0, f1);
      const float ra = gc_tap<FUSED>((float)a1, (float)(a0 + a2), f0, f1);
      const float rc = gc_tap<FUSED>((float)c1, (float)(c0 + c2), f0, f1);
      const float dy = rc - ra;
      xx = dx * dx; xy = dx * dy; yy = dy * dy;
    }
    pr[0][py][px] = xx; pr[1][py][px] = xy; pr[2][py][px] = yy;
  }
  __syncthreads();

  const int ly = tid >> 4, lx = (tid & 15) * 4;
  const int gy = y0 + ly, gx = x0 + lx;
  float box[3][4];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double t[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 3; r++) {
      float v[6];
#pragma unroll
      for (int c = 0; c < 6; c++) v[c] = pr[k][ly + r][lx + c];
#pragma unroll
      for (int o = 0; o < 4; o++) {
        const double rs = ((double)v[o] + (double)v[o + 1]) + (double)v[o + 2];
        t[o] = r == 0 ? rs : t[o] + rs;
      }
    }
#pragma unroll
    for (int o = 0; o < 4; o++) box[k][o] = (float)t[o];
  }
  float e[4];
  unsigned m = 0;
#pragma unroll
  for (int o = 0; o < 4; o++) {
    const float a = box[0][o] * 0.5f, b = box[1][o], c = box[2][o] * 0.5f;
    const float d = a - c;
    const float rad = FUSED ? fmaf(d, d, b * b) : d * d + b * b;
    e[o] = (a + c) - sqrtf(rad);   // correctly rounded (v_sqrt_f32 plus the compiler's fix-up; __fsqrt_rn is the bare instruction)
    if (gy < H && gx + o < W) m = max(m, gc_key(e[o]));
  }
  if (gy < H) {
    float* q = dst + (size_t)gy * W + gx;
    if (vec && gx + 3 < W) {
      *reinterpret_cast<float4*>(q) = make_float4(e[0], e[1], e[2], e[3]);
    } else {
#pragma unroll
      for (int o = 0; o < 4; o++)
        if (gx + o < W) q[o] = e[o];
    }
  }
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  if ((tid & 63) == 0) wmax[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) atomicMax(&keymax[blockIdx.y], max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])));
}

__global__ void gftt_cv_max_kernel(const unsigned* __restrict__ keymax, float* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = gc_unkey(keymax[i]);
}

__global__ void gftt_cv_key_kernel(const float* __restrict__ mx, unsigned* __restrict__ keymax, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keymax[i] = gc_key(mx[i]);
}

// 256 threads take GC_CPT * 256 consecutive raster positions of one frame, thread t the positions t, t + 256, ...; the block's
// candidates are counted in LDS and reserved with ONE atomicAdd on the frame's counter (thousands of returning atomics on one
// address from as many wavefronts serialise in L2: 4.8 ms per 64 KITTI-sized noise-like frames when every wavefront had its own).
constexpr int GC_CPT = 16;
__global__ void __launch_bounds__(256) gftt_cv_cand_kernel(const float* __restrict__ eig, const unsigned* __restrict__ keymax,
                                                           unsigned long long* __restrict__ keys, int* __restrict__ ncand,
                                                           size_t kstride, int W, int H, double q) {
  __shared__ int blk_cnt, blk_base;
  const int f = blockIdx.y;
  const float* map = eig + (size_t)f * W * H;
  const int p0 = blockIdx.x * (256 * GC_CPT) + threadIdx.x;
  const float thr = (float)((double)gc_unkey(keymax[f]) * q);
  if (threadIdx.x == 0) blk_cnt = 0;
  __syncthreads();
  float val[GC_CPT];
  unsigned mask = 0;
#pragma unroll
  for (int k = 0; k < GC_CPT; k++) {
    const int p = p0 + k * 256;
    val[k] = 0.f;
    if (p < W * H) {
      const int y = p / W, x = p - y * W;
      if (y >= 1 && y < H - 1 && x >= 1 && x < W - 1) {
        const float v = map[p];
        const float t = v > thr ? v : 0.f;
        if (t != 0.f) {
          float mx = t;
#pragma unroll
          for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
              const float w = map[p + dy * W + dx];
              const float tw = w > thr ? w : 0.f;
              mx = tw > mx ? tw : mx;
            }
          if (t == mx) { mask |= 1u << k; val[k] = v; }
        }
      }
    }
  }
  const int mine = __popc(mask);
  int at = mine ? atomicAdd(&blk_cnt, mine) : 0;
  __syncthreads();
  if (threadIdx.x == 0) blk_base = blk_cnt ? atomicAdd(&ncand[f], blk_cnt) : 0;
  __syncthreads();
  unsigned long long* dst = keys + (size_t)f * kstride + blk_base;
#pragma unroll
  for (int k = 0; k < GC_CPT; k++)
    if ((mask >> k) & 1u) dst[at++] = ((unsigned long long)gc_key(val[k]) << 32) | (unsigned)(p0 + k * 256);
}

// Bitonic network over P = 2^k keys, descending, by all threads of the workgroup (LDS or device memory alike).
__device__ void gc_bitonic(unsigned long long* keys, int P) {
  const int tid = threadIdx.x;
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

template <bool GT>
__global__ void __launch_bounds__(GS_THREADS) gftt_cv_select_kernel(unsigned long long* gkeys, const int* __restrict__ ncand,
                                                                    size_t kstride, float* __restrict__ kpts, int* __restrict__ count,
                                                                    unsigned* gtab, GftSelGeom g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gc_lds[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(gc_lds);
  GsShared* sh = reinterpret_cast<GsShared*>(gc_lds + (size_t)g.nkeys * 8);
  unsigned* tab = GT ? gtab + (size_t)blockIdx.x * 4 * g.gw * g.gh
                     : reinterpret_cast<unsigned*>(gc_lds + (size_t)g.nkeys * 8 + GS_FIXED_LDS);
  const int tid = threadIdx.x, wave = tid >> 6;
  const size_t img = (size_t)g.img0 + blockIdx.x;
  unsigned long long* list = gkeys + (size_t)blockIdx.x * kstride;
  float* out = kpts + img * (size_t)g.cap * 2;
  const int nk = (int)min((size_t)max(ncand[blockIdx.x], 0), kstride);

  if (tid == 0) sh->acc = 0;
  if (!GT && g.trim)
    for (int c = tid; c < g.gw * g.gh; c += GS_THREADS) tab[4 * c] = 0u;
  int P = 1;
  while (P < nk) P <<= 1;
  // real keys are > 0 (the key of a positive or negative non-zero float is never 0), so zero padding sorts last
  unsigned long long* sorted = list;
  if (nk <= g.nkeys) {
    sorted = keys;
    for (int k = tid; k < P; k += GS_THREADS) keys[k] = k < nk ? list[k] : 0ull;
  } else {
    for (int k = nk + tid; k < P; k += GS_THREADS) list[k] = 0ull;   // P <= kstride, a power of two
  }
  __syncthreads();
  if (nk > 1) gc_bitonic(sorted, P);
  if (wave == 0 && nk > 0) gftt_trim<GT>(sorted, nk, sh, tab, out, g);
  __syncthreads();
  if (tid == 0) count[img] = sh->acc;
}

static size_t gc_pow2(size_t v) {
  size_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

}  // namespace sbm

// ---- entry points --------------------------------------------------------------------------------------------------------
using namespace sbm;

extern "C" {

void sbm_gftt_cv_params_default(sbm_gftt_cv_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->max_features = 1500;
  p->quality_level = 0.01;
  p->min_distance = 7.0;
  p->block_size = 3;
  p->use_harris = 0;
  p->k = 0.04;
}

int sbm_gftt_cv_params_validate(const sbm_gftt_cv_params* p, int width, int height) {
  if (!p) return SBM_ERR_NULL;
  if (width < 3 || height < 3) return SBM_ERR_SIZE;
  if (width > kGftSelWMax || height > kGftSelWMax) return SBM_ERR_UNSUPPORTED;
  if (!std::isfinite(p->quality_level) || p->quality_level < 0) return SBM_ERR_UNSUPPORTED;
  if (!std::isfinite(p->min_distance) || p->min_distance < 0 || p->min_distance > 255) return SBM_ERR_UNSUPPORTED;
  if (p->block_size != 3 || p->use_harris != 0) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

int sbm_gftt_cv_eig_device(sbm_handle* h, int n, const void* d_img, int width, int height, void* d_eig, void* d_max, int sync) {
  if (!h || !d_img || !d_eig) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  if (width < 3 || height < 3) return SBM_ERR_SIZE;
  if (width > kGftSelWMax || height > kGftSelWMax || n > 65535 || ((uintptr_t)d_eig & 3) || ((uintptr_t)d_max & 3))
    return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  return gftt_cv_run(h, n, d_img, width, height, nullptr, d_eig, d_max, nullptr, nullptr, sync);
}

int sbm_gftt_cv_detect_device(sbm_handle* h, int n, const void* d_img, int width, int height, const sbm_gftt_cv_params* p,
                              void* d_eig, void* d_max, void* d_kpts, void* d_count, int sync) {
  if (!h || !p || !d_img || !d_kpts || !d_count) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  const int st = sbm_gftt_cv_params_validate(p, width, height);
  if (st != SBM_OK) return st;
  if (n > 65535 || ((uintptr_t)d_eig & 3) || ((uintptr_t)d_max & 3)) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  return gftt_cv_run(h, n, d_img, width, height, p, d_eig, d_max, d_kpts, d_count, sync);
}

int sbm_gftt_cv_select_device(sbm_handle* h, int n, const void* d_eig, const void* d_max, int width, int height,
                              const sbm_gftt_cv_params* p, void* d_kpts, void* d_count, int sync) {
  if (!h || !p || !d_eig || !d_max || !d_kpts || !d_count) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  const int st = sbm_gftt_cv_params_validate(p, width, height);
  if (st != SBM_OK) return st;
  if (n > 65535 || ((uintptr_t)d_eig & 3) || ((uintptr_t)d_max & 3)) return SBM_ERR_UNSUPPORTED;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  return gftt_cv_run(h, n, nullptr, width, height, p, const_cast<void*>(d_eig), const_cast<void*>(d_max), d_kpts, d_count, sync);
}

int sbm_gftt_cv_detect(sbm_handle* h, const uint8_t* img, size_t img_stride, int width, int height, const sbm_gftt_cv_params* p,
                       float* kpts, size_t capacity, int* count) {
  if (!h || !p || !img || !kpts || !count) return SBM_ERR_NULL;
  int st = sbm_gftt_cv_params_validate(p, width, height);
  if (st != SBM_OK) return st;
  const size_t cap = p->max_features > 0 ? (size_t)p->max_features : (size_t)(width - 2) * (height - 2);
  if (img_stride < (size_t)width || capacity < cap) return SBM_ERR_SIZE;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = ensure_staging(h, 1, width, height);
  if (st != SBM_OK) return st;
  float* d_k;
  int* d_n;   // points on 8-byte boundaries, then the count
  HIPCHK(h, carve(h->gc.out, h->stream, [&](Carve& c) { d_k = c.take<float>(cap * 2); d_n = c.take<int>(4); }, 8));
  HIPCHK(h, hipMemcpy2DAsync(h->st.l.p, width, img, img_stride, width, height, hipMemcpyHostToDevice, h->stream));
  st = gftt_cv_run(h, 1, h->st.l.p, width, height, p, nullptr, nullptr, d_k, d_n, 0);
  if (st != SBM_OK) return st;
  int k = 0;
  HIPCHK(h, hipMemcpyAsync(&k, d_n, sizeof(k), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (k > 0) HIPCHK(h, hipMemcpy(kpts, d_k, (size_t)k * 2 * sizeof(float), hipMemcpyDeviceToHost));
  *count = k;
  return SBM_OK;
}

}  // extern "C"

enum GfttCvStage { kGcEig, kGcSelect, kGcTotal, kGcStageCount };
static const char* const kGfttCvNames[] = {"gftt_cv_eig", "gftt_cv_select", "gftt_cv_total"};
StageTable sbm::gftt_cv_stages() { return stage_table<kGcStageCount, kGcStageCount>(kGfttCvNames); }

// Enqueues maps and maxima (with d_img; without it d_eig and d_max are the caller's, read only) and (with d_kpts) candidates, order and trim of n dense frames, chunk by chunk; profiling times them.
int sbm::gftt_cv_run(sbm_handle* h, int n, const void* d_img, int width, int height, const sbm_gftt_cv_params* p, void* d_eig,
                     void* d_max, void* d_kpts, void* d_count, int sync) {
  StageClock& clk = h->gc.clock;
  HIPCHK(h, clk.start(gftt_cv_stages(), h->profiling != 0));
  const int W = width, H = height;
  const size_t plane = (size_t)W * H;
  const bool select = d_kpts != nullptr;
  const int fused = (env_switch("SBM_CV_READING", 0) & kReadGfttCvFused) ? 1 : 0;
  const float f1 = (float)(1.0 / (4.0 * 3.0 * 255.0));
  GftSelPlan pl;
  memset(&pl, 0, sizeof(pl));
  size_t kstride = 0;
  if (select) {
    pl = gftt_select_plan(W, H, p->max_features, p->quality_level, p->min_distance);
    kstride = gc_pow2((size_t)(W - 2) * (H - 2));
  }
  // frames per chunk: key lists and (when the caller keeps no maps) maps within kGcChunkBytes each, cell tables within 2 GiB
  size_t chunk = n;
  if (select) chunk = std::min(chunk, std::max<size_t>(1, kGcChunkBytes / (kstride * 8)));
  if (!d_eig) chunk = std::min(chunk, std::max<size_t>(1, kGcChunkBytes / (plane * 4)));
  if (select && pl.global_table) chunk = std::min(chunk, std::max<size_t>(1, ((size_t)2 << 30) / pl.table_bytes_per_image));
  const int C = (int)chunk;
  unsigned* keymax;
  int* ncand;   // n keys of the maxima, then n candidate counts, on 4-byte boundaries
  HIPCHK(h, carve(h->gc.small, h->stream, [&](Carve& c) { keymax = c.take<unsigned>(n); ncand = c.take<int>(n); }, 4));
  if (select) HIPCHK(h, h->gc.keys.grow(kstride * 8 * C, h->stream));
  if (!d_eig) HIPCHK(h, h->gc.eig.grow(plane * 4 * C + 16, h->stream));
  if (select && pl.global_table) HIPCHK(h, h->gc.tab.grow(pl.table_bytes_per_image * C, h->stream));
  HIPCHK(h, hipMemsetAsync(keymax, 0, (char*)(ncand + n) - (char*)keymax, h->stream));   // both pieces
  if (!d_img) {   // the caller's maps and maxima
    hipLaunchKernelGGL(gftt_cv_key_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, (const float*)d_max, keymax, n);
    HIPCHK(h, hipGetLastError());
  }
  const int tx = (W + GC_TW - 1) / GC_TW, ty = (H + GC_TH - 1) / GC_TH;
  auto mapk = fused ? gftt_cv_map_kernel<true> : gftt_cv_map_kernel<false>;
  auto selk = pl.global_table ? gftt_cv_select_kernel<true> : gftt_cv_select_kernel<false>;
  if (select && pl.lds_bytes > 64 * 1024)
    HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(selk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGftSelLds));
  for (int c0 = 0; c0 < n; c0 += C) {
    const int m = std::min(C, n - c0);
    float* eig = d_eig ? (float*)d_eig + plane * c0 : h->gc.eig.as<float>();
    const int vec = (W % 4 == 0 && ((uintptr_t)eig & 15) == 0) ? 1 : 0;
    HIPCHK(h, clk.mark(kGcEig, h->stream));
    if (d_img) {
      hipLaunchKernelGGL(mapk, dim3(tx * ty, m), dim3(256), 0, h->stream, (const uint8_t*)d_img + plane * c0, eig, keymax + c0, W, H,
                         tx, f1, vec);
      HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, clk.mark(kGcSelect, h->stream));
    if (select) {
      hipLaunchKernelGGL(gftt_cv_cand_kernel, dim3((unsigned)((plane + 256 * GC_CPT - 1) / (256 * GC_CPT)), m), dim3(256), 0, h->stream, eig, keymax + c0,
                         h->gc.keys.as<unsigned long long>(), ncand + c0, kstride, W, H, p->quality_level);
      HIPCHK(h, hipGetLastError());
      if (pl.global_table) HIPCHK(h, hipMemsetAsync(h->gc.tab.p, 0, pl.table_bytes_per_image * m, h->stream));
      GftSelGeom g = pl.g;
      g.img0 = c0;
      hipLaunchKernelGGL(selk, dim3(m), dim3(GS_THREADS), pl.lds_bytes, h->stream, h->gc.keys.as<unsigned long long>(), ncand + c0,
                         kstride, (float*)d_kpts, (int*)d_count, h->gc.tab.as<unsigned>(), g);
      HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, clk.mark(kGcTotal, h->stream));
    for (int s = kGcEig; s < kGcTotal; s++) HIPCHK(h, clk.add(s, s, s + 1));
  }
  if (d_max && d_img) {
    hipLaunchKernelGGL(gftt_cv_max_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, keymax, (float*)d_max, n);
    HIPCHK(h, hipGetLastError());
  }
  if (clk.on) clk.ms[kGcTotal] = clk.ms[kGcEig] + clk.ms[kGcSelect];
  if (sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return SBM_OK;
}
