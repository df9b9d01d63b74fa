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
//             host (sbm_api.hip) as a kernel argument and are copied to LDS.
#include "sbm_common.h"

namespace sbm {

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

hipError_t launch_orb_blur(const uint8_t* src, uint8_t* dst, int n, int W, int H, int half_up, hipStream_t s) {
  const int tx = (W + kBlurTW - 1) / kBlurTW, ty = (H + kBlurTH - 1) / kBlurTH;
  hipLaunchKernelGGL(orb_blur_kernel, dim3(tx * ty, n), dim3(256), 0, s, src, dst, W, H, tx, half_up);
  return hipGetLastError();
}

hipError_t launch_orb_compact(const float* kin, const int* cin, float* kout, int* cout, int n, int cap, int W, int H, int edge,
                              hipStream_t s) {
  hipLaunchKernelGGL(orb_compact_kernel, dim3(n), dim3(256), 0, s, kin, cin, kout, cout, cap, W, H, edge);
  return hipGetLastError();
}

hipError_t launch_orb_desc(const uint8_t* blur, const float* kpts, const int* count, uint8_t* desc, int f0, int n, int cap, int W,
                           int H, const OrbOffsets& offs, hipStream_t s) {
  hipLaunchKernelGGL(orb_desc_kernel, dim3((cap + 31) / 32, n), dim3(256), 0, s, blur, kpts, count, desc, cap, W, H, f0, offs);
  return hipGetLastError();
}

}  // namespace sbm
