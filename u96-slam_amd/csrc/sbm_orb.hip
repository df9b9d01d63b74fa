// ORB descriptors of the reference's computeDescriptor (src/slam/src/opencv/CvORB.cpp) at pyramid level 0 with one shared
// angle: the 7x7 sigma-2 Gaussian blur of the frame (cv::GaussianBlur on a sub-matrix of the reflect-101 bordered copy, i.e.
// sepFilter2D's 8-bit fixed-point path), runByImageBorder's stable erase of the keypoints near the border, and the 256 intensity
// comparisons of computeOrbDescriptors per kept keypoint. DESIGN.md section 10.
//
//   blur      r = sum_i k_i p(x + i - 3) per row (exact, <= 65535: u16, two pixels per packed 16-bit multiply-add), then
//             S = sum_j k_j r(y + j - 3) per column (u32), out = min(255, round(S / 65536)); taps k = cvRound(256 g) of
//             getGaussianKernel(7, 2) = [18, 34, 49, 55, 49, 34, 18] (sum 257); reflect-101 at the image edges. Rounding:
//             half to even (OpenCV's vectorised column filter), or half up with kReadOrbHalfUp.
//   compact   one workgroup per frame keeps the points with cvRound(x) in [e, W - e) and cvRound(y) in [e, H - e), in order.
//   describe  eight lanes per kept keypoint, four descriptor bytes per lane; the 512 sample offsets dy * W + dx come from the
//             host (orb_offsets below) as a kernel argument and are copied to LDS.
#include <algorithm>
#include <cmath>

#include "sbm_handle.h"

namespace sbm {

// Launches. blur: n dense u8 frames -> n dense u8 frames (W, H >= 4);
// compact: runByImageBorder per frame (one workgroup each; in place allowed); desc: frames [f0, f0 + n) of the batch, `blur`
// holding exactly those n frames, 32 bytes per kept keypoint at (f * cap + j) * 32.
constexpr int kReadOrbHalfUp = 128;   // SBM_CV_READING: the blur's column filter rounds half up instead of half to even
struct OrbOffsets {
  int off[512];   // dy * W + dx of the 512 rotated pattern points, in pattern order
};

namespace {

constexpr int kBlurTW = 256;          // tile columns: 64 lanes x 4 pixels
constexpr int kBlurTH = 16;           // tile rows: 4 row groups x 4 rows
constexpr int kBlurSrcW = kBlurTW + 8;   // staged source columns x0 - 4 .. x0 + TW + 3
constexpr int kBlurSrcH = kBlurTH + 6;   // staged source rows y0 - 3 .. y0 + TH + 2

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);   // only tile cells whose outputs are never stored can still be outside
}

__global__ void __launch_bounds__(256) orb_blur_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W, int H,
                                                       int tiles_x, int half_up) {
  __shared__ __attribute__((aligned(16))) uint8_t s_src[kBlurSrcH][kBlurSrcW];
  __shared__ __attribute__((aligned(16))) unsigned s_row[kBlurSrcH][kBlurTW / 2];   // u16 pairs of the row pass
  const int tid = threadIdx.x, lx = tid & 63, ly = tid >> 6;
  const int x0 = (blockIdx.x % tiles_x) * kBlurTW, y0 = (blockIdx.x / tiles_x) * kBlurTH;
  const size_t plane = (size_t)W * H;
  const uint8_t* img = src + blockIdx.y * plane;
  uint8_t* out = dst + blockIdx.y * plane;

  for (int k = tid; k < kBlurSrcH * kBlurSrcW; k += 256) {
    const int r = k / kBlurSrcW, c = k - r * kBlurSrcW;
    const int yy = reflect101(y0 - 3 + r, H), xx = reflect101(x0 - 4 + c, W);
    s_src[r][c] = img[(size_t)yy * W + xx];
  }
  __syncthreads();

  // row pass: outputs x0 + 4lx .. +3 read staged columns 4lx + 1 .. 4lx + 10
  const u16x2 k0 = {18, 18}, k1 = {34, 34}, k2 = {49, 49}, k3 = {55, 55};
  for (int r = ly; r < kBlurSrcH; r += 4) {
    const unsigned* w = (const unsigned*)&s_src[r][4 * lx];
    const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
    uint8_t p[12];
#pragma unroll
    for (int b = 0; b < 4; b++) {
      p[b] = (w0 >> (8 * b)) & 255; p[4 + b] = (w1 >> (8 * b)) & 255; p[8 + b] = (w2 >> (8 * b)) & 255;
    }
    u16x2 acc[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {   // pixels (2q, 2q + 1) of the four; pixel c has taps at staged 4lx + 1 + c .. + 7 + c
      const int c = 2 * q + 1;
      const u16x2 a0 = {p[c], p[c + 1]}, a1 = {p[c + 1], p[c + 2]}, a2 = {p[c + 2], p[c + 3]}, a3 = {p[c + 3], p[c + 4]};
      const u16x2 a4 = {p[c + 4], p[c + 5]}, a5 = {p[c + 5], p[c + 6]}, a6 = {p[c + 6], p[c + 7]};
      acc[q] = (a0 + a6) * k0 + (a1 + a5) * k1 + (a2 + a4) * k2 + a3 * k3;   // (a0 + a6) <= 510: no partial sum wraps
    }
    uint2 v;
    v.x = (unsigned)acc[0].x | ((unsigned)acc[0].y << 16);
    v.y = (unsigned)acc[1].x | ((unsigned)acc[1].y << 16);
    *(uint2*)&s_row[r][2 * lx] = v;
  }
  __syncthreads();

  // column pass: rows y0 + 4ly .. +3, columns x0 + 4lx .. +3
  const int x = x0 + 4 * lx;
  if (x >= W) return;
  const bool vec = (W & 3) == 0 && x + 4 <= W;
#pragma unroll
  for (int rr = 0; rr < 4; rr++) {
    const int y = y0 + 4 * ly + rr;
    if (y >= H) break;
    unsigned s[4] = {0, 0, 0, 0};
    const unsigned kt[7] = {18, 34, 49, 55, 49, 34, 18};
#pragma unroll
    for (int j = 0; j < 7; j++) {
      const uint2 v = *(const uint2*)&s_row[4 * ly + rr + j][2 * lx];
      s[0] += kt[j] * (v.x & 0xffff); s[1] += kt[j] * (v.x >> 16);
      s[2] += kt[j] * (v.y & 0xffff); s[3] += kt[j] * (v.y >> 16);
    }
    unsigned o = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      unsigned q = s[b] >> 16;
      const unsigned rem = s[b] & 0xffff;
      q += half_up ? (rem >= 0x8000u) : (rem > 0x8000u || (rem == 0x8000u && (q & 1)));
      o |= min(q, 255u) << (8 * b);
    }
    uint8_t* po = out + (size_t)y * W + x;
    if (vec) {
      *(unsigned*)po = o;
    } else {
      for (int b = 0; b < 4 && x + b < W; b++) po[b] = (o >> (8 * b)) & 255;
    }
  }
}

// runByImageBorder(kpts, size, e) as a stable compaction, one workgroup of 256 per frame. In place is allowed: block b reads
// slots [256b, 256b + 256) before it writes any slot below 256b + 256.
__global__ void __launch_bounds__(256) orb_compact_kernel(const float* kin, const int* cin, float* kout, int* cout, int cap, int W,
                                                          int H, int edge) {
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t f = blockIdx.x;
  const float2* in = (const float2*)kin + f * cap;
  float2* out = (float2*)kout + f * cap;
  const int n = min(max(cin[f], 0), cap);
  const bool any = W > 2 * edge && H > 2 * edge;
  const float xl = (float)edge, xh = (float)(W - edge), yl = (float)edge, yh = (float)(H - edge);
  int kept = 0;
  __syncthreads();   // every lane has read the count before thread 0 may overwrite it (in place)
  for (int base = 0; any && base < n; base += 256) {
    const int j = base + tid;
    float2 p = make_float2(0.f, 0.f);
    bool keep = false;
    if (j < n) {
      p = in[j];
      const float rx = rintf(p.x), ry = rintf(p.y);   // cvRound through Point_<int>'s saturate_cast, half to even
      keep = rx >= xl && rx < xh && ry >= yl && ry < yh;
    }
    const unsigned long long m = __ballot(keep);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int off = kept;
    for (int w = 0; w < wv; w++) off += s_wave[w];
    const int tot = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (keep) out[off + below] = p;
    kept += tot;
    __syncthreads();
  }
  if (tid == 0) cout[f] = kept;
}

// One kept keypoint per 8 lanes, four descriptor bytes per lane; 32 keypoints per workgroup. Samples lie within 18 pixels of a
// centre at least `edge` >= 18 pixels inside the frame.
__global__ void __launch_bounds__(256) orb_desc_kernel(const uint8_t* __restrict__ blur, const float* __restrict__ kpts,
                                                       const int* __restrict__ count, uint8_t* __restrict__ desc, int cap, int W,
                                                       int H, int f0, OrbOffsets offs) {
  __shared__ int s_off[512];
  const int tid = threadIdx.x;
  s_off[tid] = offs.off[tid];
  s_off[tid + 256] = offs.off[tid + 256];
  __syncthreads();
  const int f = f0 + blockIdx.y;
  const int j = blockIdx.x * 32 + (tid >> 3), q = tid & 7;
  if (j >= count[f]) return;
  const float2 p = ((const float2*)kpts)[(size_t)f * cap + j];
  const int cx = (int)rintf(p.x), cy = (int)rintf(p.y);
  const uint8_t* c = blur + (size_t)blockIdx.y * W * H + (size_t)cy * W + cx;
  unsigned v = 0;
#pragma unroll
  for (int b = 0; b < 4; b++) {
    const int* o = s_off + 16 * (4 * q + b);
    unsigned byte = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) byte |= (unsigned)(c[o[2 * k]] < c[o[2 * k + 1]]) << k;
    v |= byte << (8 * b);
  }
  ((unsigned*)(desc + ((size_t)f * cap + j) * 32))[q] = v;
}

}  // namespace

static hipError_t launch_orb_blur(const uint8_t* src, uint8_t* dst, int n, int W, int H, int half_up, hipStream_t s) {
  const int tx = (W + kBlurTW - 1) / kBlurTW, ty = (H + kBlurTH - 1) / kBlurTH;
  hipLaunchKernelGGL(orb_blur_kernel, dim3(tx * ty, n), dim3(256), 0, s, src, dst, W, H, tx, half_up);
  return hipGetLastError();
}

static hipError_t launch_orb_compact(const float* kin, const int* cin, float* kout, int* cout, int n, int cap, int W, int H, int edge,
                                     hipStream_t s) {
  hipLaunchKernelGGL(orb_compact_kernel, dim3(n), dim3(256), 0, s, kin, cin, kout, cout, cap, W, H, edge);
  return hipGetLastError();
}

static hipError_t launch_orb_desc(const uint8_t* blur, const float* kpts, const int* count, uint8_t* desc, int f0, int n, int cap, int W,
                                  int H, const OrbOffsets& offs, hipStream_t s) {
  hipLaunchKernelGGL(orb_desc_kernel, dim3((cap + 31) / 32, n), dim3(256), 0, s, blur, kpts, count, desc, cap, W, H, f0, offs);
  return hipGetLastError();
}

}  // namespace sbm

// ---- entry points --------------------------------------------------------------------------------------------------------
using namespace sbm;

// The marks: kOrbBegin and kOrbMid around the compaction (it counts as descriptors), then per chunk before the blur, after it, after the descriptors.
enum OrbStage { kOrbBlur, kOrbDesc, kOrbTotal, kOrbStageCount };
enum OrbMark { kOrbBegin, kOrbMid, kOrbEnd, kOrbMarkCount };
static const char* const kOrbNames[] = {"orb_blur", "orb_desc", "orb_total"};
StageTable sbm::orb_stages() { return stage_table<kOrbStageCount, kOrbMarkCount>(kOrbNames); }

extern "C" {

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

// Enqueues compaction, blur and descriptors; profiling times them, the compaction as part of the descriptors.
static int orb_run(sbm_handle* h, int n, const void* d_img, int width, int height, int cap, const void* d_kpts, const void* d_count,
                   const OrbOffsets& offs, const sbm_orb_params* p, void* d_kpts_out, void* d_count_out, void* d_desc,
                   void* d_blur, int sync) {
  StageClock& clk = h->orb.clock;
  HIPCHK(h, clk.start(orb_stages(), h->profiling != 0));
  const int edge = p->edge_threshold;
  HIPCHK(h, clk.mark(kOrbBegin, h->stream));
  HIPCHK(h, launch_orb_compact((const float*)d_kpts, (const int*)d_count, (float*)d_kpts_out, (int*)d_count_out, n, cap, width,
                               height, edge, h->stream));
  HIPCHK(h, clk.mark(kOrbMid, h->stream));
  HIPCHK(h, clk.add(kOrbDesc, kOrbBegin, kOrbMid));
  if (width > 2 * edge && height > 2 * edge) {   // else every keypoint is gone and nothing needs the blur
    const int reading = env_switch("SBM_CV_READING", 0);
    const size_t plane = (size_t)width * height;
    int chunk = n;
    if (!d_blur) {
      chunk = (int)std::min<size_t>(n, std::max<size_t>(1, ((size_t)256 << 20) / plane));
      HIPCHK(h, h->orb.blur.grow(plane * chunk, h->stream));
    }
    for (int c0 = 0; c0 < n; c0 += chunk) {
      const int m = std::min(chunk, n - c0);
      uint8_t* bc = d_blur ? (uint8_t*)d_blur + plane * c0 : h->orb.blur.as<uint8_t>();
      HIPCHK(h, clk.mark(kOrbBegin, h->stream));
      HIPCHK(h, launch_orb_blur((const uint8_t*)d_img + plane * c0, bc, m, width, height, (reading & kReadOrbHalfUp) ? 1 : 0,
                                h->stream));
      HIPCHK(h, clk.mark(kOrbMid, h->stream));
      HIPCHK(h, launch_orb_desc(bc, (const float*)d_kpts_out, (const int*)d_count_out, (uint8_t*)d_desc, c0, m, cap, width, height,
                                offs, h->stream));
      HIPCHK(h, clk.mark(kOrbEnd, h->stream));
      HIPCHK(h, clk.add(kOrbBlur, kOrbBegin, kOrbMid));
      HIPCHK(h, clk.add(kOrbDesc, kOrbMid, kOrbEnd));
    }
  }
  if (clk.on) clk.ms[kOrbTotal] = clk.ms[kOrbBlur] + clk.ms[kOrbDesc];
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

int sbm_orb_features_cv_device(sbm_handle* h, int n, const void* d_img, int width, int height, const sbm_gftt_cv_params* gp,
                               const int* pattern, const sbm_orb_params* p, void* d_eig, void* d_max, void* d_kpts, void* d_count,
                               void* d_desc, void* d_blur, int sync) {
  if (!h || !gp || !d_img || !d_kpts || !d_count || !pattern || !p || !d_desc) return SBM_ERR_NULL;
  if (n <= 0) return SBM_ERR_BATCH;
  int st = sbm_gftt_cv_params_validate(gp, width, height);
  if (st == SBM_OK) st = sbm_orb_params_validate(p);
  const int cap = gp->max_features > 0 ? gp->max_features : (width - 2) * (height - 2);
  if (st == SBM_OK) st = orb_check(n, width, height, cap, d_kpts, d_kpts, d_desc);
  if (st == SBM_OK && (((uintptr_t)d_eig & 3) || ((uintptr_t)d_max & 3))) st = SBM_ERR_UNSUPPORTED;
  if (st != SBM_OK) return st;
  OrbOffsets offs;
  st = orb_offsets(pattern, p->angle, width, &offs);
  if (st != SBM_OK) return st;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  st = gftt_cv_run(h, n, d_img, width, height, gp, d_eig, d_max, d_kpts, d_count, 0);
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
  float *d_ki, *d_ko;
  uint8_t* d_de;
  int* d_n;
  HIPCHK(h, carve(h->orb.io, h->stream, [&](Carve& c) {   // on 8-byte boundaries: two point lists before them keep the descriptors on 16
    d_ki = c.take<float>((size_t)cap * 2); d_ko = c.take<float>((size_t)cap * 2);
    d_de = c.take<uint8_t>((size_t)cap * 32); d_n = c.take<int>(4);   // count in, count out
  }, 8));
  HIPCHK(h, hipMemcpy2DAsync(h->st.l.p, width, img, img_stride, width, height, hipMemcpyHostToDevice, h->stream));
  if (count > 0) HIPCHK(h, hipMemcpyAsync(d_ki, kpts, (size_t)count * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_n, &count, sizeof(int), hipMemcpyHostToDevice, h->stream));
  st = orb_run(h, 1, h->st.l.p, width, height, cap, d_ki, d_n, offs, p, d_ko, d_n + 1, d_de, nullptr, 0);
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

}  // extern "C"
