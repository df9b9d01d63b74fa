/* orb_ref.c -- CPU restatement of the reference's descriptor step, computeDescriptor() (src/slam/src/opencv/CvORB.cpp), for the
 * keypoints generateKeypoints2 produces: pyramid level 0, one shared angle, WTA_K 2, 32-byte descriptors, no mask. TEST
 * INFRASTRUCTURE ONLY. Written from the semantics stated in include/sbm.h (sbm_orb_params), step by step as the reference runs:
 *
 *   1. copyMakeBorder(image, ext, 23, 23, 23, 23, BORDER_REFLECT_101) into a buffer of (W + 46) x (H + 46);
 *   2. GaussianBlur of the image-sized ROI of ext in place, as sepFilter2D's 8-bit path: integer taps cvRound(256 g) of
 *      getGaussianKernel(7, 2) (derived here, not typed in), exact row sums over the ROI's rows -3 .. H + 2 read from ext (the
 *      unblurred border), column sums S, out = min(255, round(S / 65536)) -- ties half to even, or half up (`half_up`);
 *   3. runByImageBorder(kpts, size, edge): stable erase of the points whose cvRound(x), cvRound(y) lie outside
 *      [edge, W - edge) x [edge, H - edge); all of them when W <= 2 edge or H <= 2 edge;
 *   4. computeOrbDescriptors: centre = ext + (cvRound(y) + 23) * step + cvRound(x) + 23, GET_VALUE offsets iy * step + ix with
 *      ix = cvRound(p.x * a - p.y * b), iy = cvRound(p.x * b + p.y * a) in float (this file is built with -ffp-contract=off).
 *
 * orb_taps(k)                 the seven integer taps
 * orb_blur(img, stride, W, H, half_up, out)   steps 1-2 on one frame (W, H >= 24), out dense W x H; 0, or -1 out of memory
 * orb_describe(img, stride, W, H, kpts, count, pattern, angle, edge, half_up, kpts_out, desc, blur_out) -> kept count (or -1);
 *                             kpts_out (may be kpts) and desc (32 bytes per kept point) receive the result; blur_out (dense
 *                             W x H, may be NULL) the blurred frame when W, H > 2 edge. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ORB_BORDER 23

static int round_even(float v) { return (int)nearbyintf(v); }   /* cvRound: half to even in the default rounding mode */

/* getGaussianKernel(7, 2.0, CV_32F): exp(-(i - 3)^2 / (2 sigma^2)) computed in double, scaled to sum 1, stored as float; then
 * cvRound(256 * k) as sepFilter2D's 8-bit path does. */
void orb_taps(int* k) {
  double g[7], sum = 0.0;
  const double scale2x = -0.5 / (2.0 * 2.0);
  for (int i = 0; i < 7; i++) {
    const double x = i - 3;
    g[i] = exp(scale2x * x * x);
    sum += g[i];
  }
  for (int i = 0; i < 7; i++) {
    const float f = (float)(g[i] / sum);
    k[i] = (int)nearbyint((double)f * 256.0);
  }
}

static int reflect101(int i, int n) {
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

/* steps 1 and 2 into ext (pitch ew); returns the ext buffer or NULL */
static uint8_t* border_and_blur(const uint8_t* img, size_t stride, int W, int H, int half_up, int* ew_out) {
  const int ew = W + 2 * ORB_BORDER, eh = H + 2 * ORB_BORDER;
  uint8_t* ext = (uint8_t*)malloc((size_t)ew * eh);
  uint32_t* rows = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)W * (H + 6));
  if (!ext || !rows) { free(ext); free(rows); return NULL; }
  for (int y = 0; y < eh; y++)
    for (int x = 0; x < ew; x++)
      ext[(size_t)y * ew + x] = img[(size_t)reflect101(y - ORB_BORDER, H) * stride + reflect101(x - ORB_BORDER, W)];
  int k[7];
  orb_taps(k);
  /* row filter of ROI rows -3 .. H + 2, every value read from ext before anything is written back */
  for (int r = 0; r < H + 6; r++) {
    const uint8_t* src = ext + (size_t)(r - 3 + ORB_BORDER) * ew + ORB_BORDER;
    for (int x = 0; x < W; x++) {
      uint32_t s = 0;
      for (int i = 0; i < 7; i++) s += (uint32_t)k[i] * src[x + i - 3];
      rows[(size_t)r * W + x] = s;
    }
  }
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      uint64_t S = 0;
      for (int j = 0; j < 7; j++) S += (uint64_t)k[j] * rows[(size_t)(y + j) * W + x];
      uint64_t q = S >> 16;
      const uint64_t rem = S & 0xffff;
      if (half_up) q += rem >= 0x8000;
      else q += rem > 0x8000 || (rem == 0x8000 && (q & 1));
      ext[(size_t)(y + ORB_BORDER) * ew + x + ORB_BORDER] = (uint8_t)(q > 255 ? 255 : q);
    }
  free(rows);
  *ew_out = ew;
  return ext;
}

int orb_blur(const uint8_t* img, size_t stride, int W, int H, int half_up, uint8_t* out) {
  int ew = 0;
  uint8_t* ext = border_and_blur(img, stride, W, H, half_up, &ew);
  if (!ext) return -1;
  for (int y = 0; y < H; y++) memcpy(out + (size_t)y * W, ext + (size_t)(y + ORB_BORDER) * ew + ORB_BORDER, (size_t)W);
  free(ext);
  return 0;
}

int orb_describe(const uint8_t* img, size_t stride, int W, int H, const float* kpts, int count, const int* pattern, float angle_deg,
                 int edge, int half_up, float* kpts_out, uint8_t* desc, uint8_t* blur_out) {
  /* runByImageBorder */
  int kept = 0;
  if (W > 2 * edge && H > 2 * edge) {
    for (int j = 0; j < count; j++) {
      const float x = kpts[2 * j], y = kpts[2 * j + 1];
      if (!(x == x) || !(y == y) || fabsf(x) > 1e9f || fabsf(y) > 1e9f) continue;   /* saturate_cast lands far outside */
      const int ix = round_even(x), iy = round_even(y);
      if (ix >= edge && ix < W - edge && iy >= edge && iy < H - edge) {
        kpts_out[2 * kept] = x;
        kpts_out[2 * kept + 1] = y;
        kept++;
      }
    }
  }
  if (kept == 0 && !(W > 2 * edge && H > 2 * edge)) return 0;
  int ew = 0;
  uint8_t* ext = border_and_blur(img, stride, W, H, half_up, &ew);
  if (!ext) return -1;
  if (blur_out)
    for (int y = 0; y < H; y++) memcpy(blur_out + (size_t)y * W, ext + (size_t)(y + ORB_BORDER) * ew + ORB_BORDER, (size_t)W);
  /* computeOrbDescriptors, level 0: scale 1 */
  float angle = angle_deg;
  angle *= (float)(3.14159265358979323846 / 180.f);
  const float a = (float)cos(angle), b = (float)sin(angle);
  for (int j = 0; j < kept; j++) {
    const uint8_t* center = ext + (size_t)(round_even(kpts_out[2 * j + 1]) + ORB_BORDER) * ew + round_even(kpts_out[2 * j]) + ORB_BORDER;
    const int* pat = pattern;
    for (int i = 0; i < 32; i++, pat += 32) {
      int val = 0;
      for (int k = 0; k < 8; k++) {
        int t[2];
        for (int e = 0; e < 2; e++) {
          const float px = (float)pat[2 * (2 * k + e)], py = (float)pat[2 * (2 * k + e) + 1];
          const float x = px * a - py * b, y = px * b + py * a;
          t[e] = center[round_even(y) * ew + round_even(x)];
        }
        val |= (t[0] < t[1]) << k;
      }
      desc[(size_t)j * 32 + i] = (uint8_t)val;
    }
  }
  free(ext);
  return kept;
}
