/* gftt_cv_ref.c -- sequential CPU restatement of the reference's generateKeypoints() (src/slam/src/core/GFTT.cpp:11-25:
 * cv::GFTTDetector, i.e. cv::goodFeaturesToTrack with the minimum-eigenvalue response), step by step as include/sbm.h states
 * it ("GFTT keypoints of OpenCV"). TEST INFRASTRUCTURE ONLY. Built without contraction; the fused multiply-adds of reading bit
 * 512 are spelled fmaf.
 *
 * gftt_cv_ref_set_reading(bits)                                    the SBM_CV_READING bits this file knows: 512
 * gftt_cv_ref_map(img, stride, W, H, eig, &max)                    eig: dense W * H floats; 0, or -1 when out of memory
 * gftt_cv_ref_detect(img, stride, W, H, nfeatures, quality, min_distance, eig or NULL, &max, &candidates, out_xy, out_cap)
 *                                                                  -> number of points (at most out_cap are written), -1 when
 *                                                                  out of memory
 * gftt_cv_ref_select(eig, max, W, H, nfeatures, quality, min_distance, &candidates, out_xy, out_cap)
 *                                                                  the same from a dense float map and its maximum
 * gftt_cv_ref_sqrtf(x)                                             the square root the map uses */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int g_reading = 0;
#define READ_FUSED 512

void gftt_cv_ref_set_reading(int bits) { g_reading = bits; }
float gftt_cv_ref_sqrtf(float x) { return sqrtf(x); }

static int reflect101(int p, int n) {
  if (p < 0) p = -p;
  if (p >= n) p = 2 * (n - 1) - p;
  return p;
}

static float tap(float c, float q, float f0, float f1) {
  if (g_reading & READ_FUSED) return fmaf(f1, q, f0 * c);
  const float a = f1 * q, b = f0 * c;
  return a + b;
}

/* the order of the maximum and of the sort: numeric, -0 below +0 */
static uint32_t key_of(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}

int gftt_cv_ref_map(const uint8_t* img, size_t stride, int W, int H, float* eig, float* max_out) {
  const size_t n = (size_t)W * H;
  float* xx = (float*)malloc(3 * n * sizeof(float));
  if (!xx) return -1;
  float* xy = xx + n;
  float* yy = xy + n;
  const float f1 = (float)(1.0 / (4.0 * 3.0 * 255.0)), f0 = 2.f * f1;
#define P(y, x) ((int)img[(size_t)reflect101((y), H) * stride + reflect101((x), W)])
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      const int d0 = P(y - 1, x + 1) - P(y - 1, x - 1), d1 = P(y, x + 1) - P(y, x - 1), d2 = P(y + 1, x + 1) - P(y + 1, x - 1);
      const float dx = tap((float)d1, (float)(d0 + d2), f0, f1);
      const float ra = tap((float)P(y - 1, x), (float)(P(y - 1, x - 1) + P(y - 1, x + 1)), f0, f1);
      const float rc = tap((float)P(y + 1, x), (float)(P(y + 1, x - 1) + P(y + 1, x + 1)), f0, f1);
      const float dy = rc - ra;
      xx[(size_t)y * W + x] = dx * dx;
      xy[(size_t)y * W + x] = dx * dy;
      yy[(size_t)y * W + x] = dy * dy;
    }
#undef P
  uint32_t best = 0;
  for (int y = 0; y < H; y++)
    for (int x = 0; x < W; x++) {
      float box[3];
      const float* pl[3] = {xx, xy, yy};
      for (int k = 0; k < 3; k++) {
        double t = 0.0;
        for (int r = -1; r <= 1; r++) {
          const float* row = pl[k] + (size_t)reflect101(y + r, H) * W;
          const double rs = ((double)row[reflect101(x - 1, W)] + (double)row[x]) + (double)row[reflect101(x + 1, W)];
          t = r == -1 ? rs : t + rs;
        }
        box[k] = (float)t;
      }
      const float a = box[0] * 0.5f, b = box[1], c = box[2] * 0.5f;
      const float d = a - c;
      float rad;
      if (g_reading & READ_FUSED) rad = fmaf(d, d, b * b);
      else { const float dd = d * d, bb = b * b; rad = dd + bb; }
      const float tr = a + c;
      const float e = tr - sqrtf(rad);
      eig[(size_t)y * W + x] = e;
      if (key_of(e) > best || (y == 0 && x == 0)) best = key_of(e);
    }
  free(xx);
  {
    const uint32_t b = (best & 0x80000000u) ? (best ^ 0x80000000u) : ~best;
    memcpy(max_out, &b, 4);
  }
  return 0;
}

typedef struct { uint32_t key; uint32_t idx; } cand;

/* value descending, then raster index descending */
static int cand_before(const void* pa, const void* pb) {
  const cand* a = (const cand*)pa;
  const cand* b = (const cand*)pb;
  if (a->key != b->key) return a->key > b->key ? -1 : 1;
  return a->idx > b->idx ? -1 : (a->idx < b->idx ? 1 : 0);
}

typedef struct { int* v; int n, cap; } cell;   /* accepted points of one cell, as raster indices */

/* the selection on a dense map and its maximum */
long gftt_cv_ref_select(const float* eig, float mx, int W, int H, int nfeatures, double quality, double min_distance,
                        long* ncand_out, float* out_xy, long out_cap) {
  const size_t n = (size_t)W * H;
  float* thr_map = (float*)malloc(n * sizeof(float));
  cand* cs = (cand*)malloc(n * sizeof(cand));
  long result = -1;
  cell* grid = NULL;
  size_t ncell = 0;
  if (!thr_map || !cs) goto done;
  const float thr = (float)((double)mx * quality);
  for (size_t i = 0; i < n; i++) thr_map[i] = eig[i] > thr ? eig[i] : 0.0f;
  size_t total = 0;
  for (int y = 1; y < H - 1; y++)
    for (int x = 1; x < W - 1; x++) {
      const float v = thr_map[(size_t)y * W + x];
      if (v == 0.0f) continue;
      float dil = v;
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
          const float w = thr_map[(size_t)(y + dy) * W + (x + dx)];
          if (w > dil) dil = w;
        }
      if (v == dil) { cs[total].key = key_of(v); cs[total].idx = (uint32_t)(y * W + x); total++; }
    }
  if (ncand_out) *ncand_out = (long)total;
  qsort(cs, total, sizeof(cand), cand_before);
  long ncorners = 0;
  if (min_distance >= 1) {
    const int cell_size = (int)lrint(min_distance);   /* cvRound: half to even */
    const int gw = (W + cell_size - 1) / cell_size, gh = (H + cell_size - 1) / cell_size;
    ncell = (size_t)gw * gh;
    grid = (cell*)calloc(ncell, sizeof(cell));
    if (!grid) goto done;
    const double md2 = min_distance * min_distance;
    for (size_t i = 0; i < total; i++) {
      const int y = (int)(cs[i].idx / (uint32_t)W), x = (int)(cs[i].idx % (uint32_t)W);
      const int xc = x / cell_size, yc = y / cell_size;
      const int x1 = xc > 0 ? xc - 1 : 0, y1 = yc > 0 ? yc - 1 : 0;
      const int x2 = xc + 1 < gw ? xc + 1 : gw - 1, y2 = yc + 1 < gh ? yc + 1 : gh - 1;
      int good = 1;
      for (int yy = y1; yy <= y2 && good; yy++)
        for (int xx = x1; xx <= x2 && good; xx++) {
          const cell* m = &grid[(size_t)yy * gw + xx];
          for (int j = 0; j < m->n; j++) {
            const float dx = (float)(x - m->v[j] % W), dy = (float)(y - m->v[j] / W);
            if (dx * dx + dy * dy < md2) { good = 0; break; }
          }
        }
      if (!good) continue;
      cell* m = &grid[(size_t)yc * gw + xc];
      if (m->n == m->cap) {
        const int c = m->cap ? 2 * m->cap : 4;
        int* v = (int*)realloc(m->v, (size_t)c * sizeof(int));
        if (!v) goto done;
        m->v = v; m->cap = c;
      }
      m->v[m->n++] = (int)cs[i].idx;
      if (ncorners < out_cap) { out_xy[2 * ncorners] = (float)x; out_xy[2 * ncorners + 1] = (float)y; }
      ncorners++;
      if (nfeatures > 0 && ncorners == nfeatures) break;
    }
  } else {
    for (size_t i = 0; i < total; i++) {
      const int y = (int)(cs[i].idx / (uint32_t)W), x = (int)(cs[i].idx % (uint32_t)W);
      if (ncorners < out_cap) { out_xy[2 * ncorners] = (float)x; out_xy[2 * ncorners + 1] = (float)y; }
      ncorners++;
      if (nfeatures > 0 && ncorners == nfeatures) break;
    }
  }
  result = ncorners;
done:
  if (grid) {
    for (size_t k = 0; k < ncell; k++) free(grid[k].v);
    free(grid);
  }
  free(cs);
  free(thr_map);
  return result;
}

long gftt_cv_ref_detect(const uint8_t* img, size_t stride, int W, int H, int nfeatures, double quality, double min_distance,
                        float* eig_out, float* max_out, long* ncand_out, float* out_xy, long out_cap) {
  float* eig = eig_out ? eig_out : (float*)malloc((size_t)W * H * sizeof(float));
  long result = -1;
  if (eig && gftt_cv_ref_map(img, stride, W, H, eig, max_out) == 0)
    result = gftt_cv_ref_select(eig, *max_out, W, H, nfeatures, quality, min_distance, ncand_out, out_xy, out_cap);
  if (!eig_out) free(eig);
  return result;
}
