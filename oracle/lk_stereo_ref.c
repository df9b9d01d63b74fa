/* lk_stereo_ref.c -- sequential CPU restatement of the reference's DEPTH_METHOD_CV_LK path as include/sbm.h states it
 * (section "pyramidal LK stereo"): the pyramid of cv::buildOpticalFlowPyramid (RECALLED), the x-only tracker of
 * calcOpticalFlowPyrLKStereo (REF), computeCorrespondences' disparity gate and the sparse branch of generateKeypoints3DStereo.
 * Written from the header's text, one operation per line where rounding matters. TEST INFRASTRUCTURE ONLY.
 * Build: oracle/Makefile, liblk_stereo_ref.so (REF_CFLAGS: -O2 -std=c11 -fPIC -ffp-contract=off). */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define LK_MAX_LEVELS 16

/* exits of a point at level 0 (info[2 * i]); info[2 * i + 1] = iterations run at level 0 */
enum { LK_CONVERGED = 0, LK_PREV_OUT = 1, LK_MIN_EIG = 2, LK_NEXT_OUT = 3, LK_MAX_COUNT = 4, LK_OSCILLATION = 5 };

typedef struct lk_ref_params {
  int32_t win_width, win_height, max_level, max_count;
  float epsilon;
  int32_t flags;
  double min_eig_threshold;
  float min_disparity, max_disparity;
} lk_ref_params;

typedef struct lk_ref_model {
  double fx_l, fy_l, cx_l, cy_l, Tx_l, fx_r, fy_r, cx_r, Tx_r;
  float local[12];
  int32_t has_local;
} lk_ref_model;

/* BORDER_REFLECT_101 of index i into [0, n), as often as it takes (n >= 2; n == 1 -> 0) */
static int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

/* levels beyond 0: building stops at the first level whose successor is not larger than the window in both directions */
int lk_ref_levels(int w, int h, int ww, int wh, int max_level) {
  int level = 0;
  for (; level < max_level && level < LK_MAX_LEVELS - 1; level++) {
    w = (w + 1) / 2;
    h = (h + 1) / 2;
    if (w <= ww || h <= wh) break;
  }
  return level;
}

/* pyrDown: separable [1 4 6 4 1] at the even samples, reflect-101, (s + 128) >> 8 */
static void pyr_down(const uint8_t* src, int w, int h, uint8_t* dst, int dw, int dh) {
  static const int k[5] = {1, 4, 6, 4, 1};
  for (int y = 0; y < dh; y++)
    for (int x = 0; x < dw; x++) {
      int s = 0;
      for (int j = 0; j < 5; j++) {
        const uint8_t* row = src + (size_t)reflect101(2 * y + j - 2, h) * w;
        int r = 0;
        for (int i = 0; i < 5; i++) r += k[i] * row[reflect101(2 * x + i - 2, w)];
        s += k[j] * r;
      }
      dst[(size_t)y * dw + x] = (uint8_t)((s + 128) >> 8);
    }
}

/* Scharr derivatives of the unpadded level: smoothing (3, 10, 3) across, difference (-1, 0, 1) along; reflect-101 */
static void scharr(const uint8_t* src, int w, int h, int16_t* d) {
  for (int y = 0; y < h; y++) {
    const uint8_t* r0 = src + (size_t)reflect101(y - 1, h) * w;
    const uint8_t* r1 = src + (size_t)y * w;
    const uint8_t* r2 = src + (size_t)reflect101(y + 1, h) * w;
    for (int x = 0; x < w; x++) {
      const int xl = reflect101(x - 1, w), xr = reflect101(x + 1, w);
      const int dx = 3 * (r0[xr] - r0[xl]) + 10 * (r1[xr] - r1[xl]) + 3 * (r2[xr] - r2[xl]);
      const int dy = 3 * (r2[xl] - r0[xl]) + 10 * (r2[x] - r0[x]) + 3 * (r2[xr] - r0[xr]);
      d[((size_t)y * w + x) * 2] = (int16_t)dx;
      d[((size_t)y * w + x) * 2 + 1] = (int16_t)dy;
    }
  }
}

/* One frame. levels: the unpadded planes back to back, level 0 first (sum of w_l * h_l bytes); deriv (may be NULL): the same
 * order, (dx, dy) int16 pairs. Returns the index of the last level. */
int lk_ref_pyramid(const uint8_t* img, int w, int h, int ww, int wh, int max_level, uint8_t* levels, int16_t* deriv) {
  const int L = lk_ref_levels(w, h, ww, wh, max_level);
  memcpy(levels, img, (size_t)w * h);
  const uint8_t* prev = levels;
  size_t off = 0;
  for (int l = 0;; l++) {
    if (deriv) scharr(prev, w, h, deriv + 2 * off);
    if (l == L) break;
    off += (size_t)w * h;
    const int dw = (w + 1) / 2, dh = (h + 1) / 2;
    pyr_down(prev, w, h, levels + off, dw, dh);
    prev = levels + off;
    w = dw;
    h = dh;
  }
  return L;
}

typedef struct {
  const uint8_t *I, *J;
  const int16_t* d;
  int w, h;
} lk_level;

static int pix(const uint8_t* p, int w, int h, int x, int y) { return p[(size_t)reflect101(y, h) * w + reflect101(x, w)]; }
static int der(const int16_t* d, int w, int h, int x, int y, int c) {
  return (x < 0 || x >= w || y < 0 || y >= h) ? 0 : d[((size_t)y * w + x) * 2 + c];
}
static int cv_floor(float v) { return (int)floorf(v); }
static int cv_round(float v) { return (int)lrintf(v); } /* half to even in the default rounding mode */

static void weights(float a, float b, int* w00, int* w01, int* w10, int* w11) {
  const float a1 = 1.f - a, b1 = 1.f - b;
  float t = a1 * b1;
  t = t * 16384.f;
  *w00 = cv_round(t);
  t = a * b1;
  t = t * 16384.f;
  *w01 = cv_round(t);
  t = a1 * b;
  t = t * 16384.f;
  *w10 = cv_round(t);
  *w11 = 16384 - *w00 - *w01 - *w10;
}

/* The tracker on one pair. pts / out: n (x, y) pairs; status n bytes; err n floats or NULL; info 2 n ints or NULL; hist
 * (LK_MAX_LEVELS x 102 ints, or NULL) counts [level][iterations]. No gate. Returns the last level, or -1 (out of memory). */
int lk_ref_track(const uint8_t* left, const uint8_t* right, int w, int h, const float* pts, int n, const lk_ref_params* p,
                 float* out, uint8_t* status, float* err, int32_t* info, int32_t* hist) {
  const int ww = p->win_width, wh = p->win_height;
  size_t total = 0;
  {
    int lw = w, lh = h;
    const int L0 = lk_ref_levels(w, h, ww, wh, p->max_level);
    for (int l = 0; l <= L0; l++) { total += (size_t)lw * lh; lw = (lw + 1) / 2; lh = (lh + 1) / 2; }
  }
  uint8_t* pl = (uint8_t*)malloc(total);
  uint8_t* pr = (uint8_t*)malloc(total);
  int16_t* pd = (int16_t*)malloc(total * 4);
  short* Iw = (short*)malloc((size_t)ww * wh * 3 * sizeof(short));
  if (!pl || !pr || !pd || !Iw) { free(pl); free(pr); free(pd); free(Iw); return -1; }
  const int L = lk_ref_pyramid(left, w, h, ww, wh, p->max_level, pl, pd);
  lk_ref_pyramid(right, w, h, ww, wh, L, pr, NULL);
  lk_level lv[LK_MAX_LEVELS];
  {
    size_t off = 0;
    int lw = w, lh = h;
    for (int l = 0; l <= L; l++) {
      lv[l].I = pl + off; lv[l].J = pr + off; lv[l].d = pd + 2 * off; lv[l].w = lw; lv[l].h = lh;
      off += (size_t)lw * lh; lw = (lw + 1) / 2; lh = (lh + 1) / 2;
    }
  }
  int max_count = p->max_count < 0 ? 0 : (p->max_count > 100 ? 100 : p->max_count);
  double eps = (double)p->epsilon;
  eps = eps < 0. ? 0. : (eps > 10. ? 10. : eps);
  eps *= eps;
  const float half_x = (ww - 1) * 0.5f, half_y = (wh - 1) * 0.5f;
  const float FLT_SCALE = 1.f / (1 << 20);
  short* dIw = Iw + (size_t)ww * wh;
  for (int i = 0; i < n; i++) status[i] = 1;
  if (hist) memset(hist, 0, sizeof(int32_t) * LK_MAX_LEVELS * 102);

  for (int level = L; level >= 0; level--) {
    const lk_level* v = &lv[level];
    const float scale = (float)(1. / (1 << level));
    for (int i = 0; i < n; i++) {
      float px = pts[2 * i] * scale, py = pts[2 * i + 1] * scale;
      float nx, ny;
      if (level == L) { nx = px; ny = py; } else { nx = out[2 * i] * 2.f; ny = out[2 * i + 1] * 2.f; }
      out[2 * i] = nx;
      out[2 * i + 1] = ny;
      px = px - half_x;
      py = py - half_y;
      const int ipx = cv_floor(px), ipy = cv_floor(py);
      if (ipx < -ww || ipx >= v->w || ipy < -wh || ipy >= v->h) {
        if (level == 0) {
          status[i] = 0;
          if (err) err[i] = 0.f;
          if (info) { info[2 * i] = LK_PREV_OUT; info[2 * i + 1] = 0; }
        }
        continue;
      }
      float a = px - (float)ipx, b = py - (float)ipy;
      int w00, w01, w10, w11;
      weights(a, b, &w00, &w01, &w10, &w11);
      float iA11 = 0.f, iA12 = 0.f, iA22 = 0.f;
      for (int y = 0; y < wh; y++)
        for (int x = 0; x < ww; x++) {
          const int X = ipx + x, Y = ipy + y;
          const int ival = (pix(v->I, v->w, v->h, X, Y) * w00 + pix(v->I, v->w, v->h, X + 1, Y) * w01 +
                            pix(v->I, v->w, v->h, X, Y + 1) * w10 + pix(v->I, v->w, v->h, X + 1, Y + 1) * w11 + 256) >> 9;
          const int ixval = (der(v->d, v->w, v->h, X, Y, 0) * w00 + der(v->d, v->w, v->h, X + 1, Y, 0) * w01 +
                             der(v->d, v->w, v->h, X, Y + 1, 0) * w10 + der(v->d, v->w, v->h, X + 1, Y + 1, 0) * w11 + 8192) >> 14;
          const int iyval = (der(v->d, v->w, v->h, X, Y, 1) * w00 + der(v->d, v->w, v->h, X + 1, Y, 1) * w01 +
                             der(v->d, v->w, v->h, X, Y + 1, 1) * w10 + der(v->d, v->w, v->h, X + 1, Y + 1, 1) * w11 + 8192) >> 14;
          Iw[y * ww + x] = (short)ival;
          dIw[(y * ww + x) * 2] = (short)ixval;
          dIw[(y * ww + x) * 2 + 1] = (short)iyval;
          iA11 += (float)(ixval * ixval);
          iA12 += (float)(ixval * iyval);
          iA22 += (float)(iyval * iyval);
        }
      const float A11 = iA11 * FLT_SCALE, A12 = iA12 * FLT_SCALE, A22 = iA22 * FLT_SCALE;
      const float t1 = A11 * A22, t2 = A12 * A12;
      float D = t1 - t2;
      const float dA = A11 - A22;
      const float r1 = dA * dA;
      float r2 = 4.f * A12;
      r2 = r2 * A12;
      const float rad = r1 + r2;
      const float sq = sqrtf(rad);
      float num = A22 + A11;
      num = num - sq;
      const float minEig = num / (float)(2 * ww * wh);
      if (err) err[i] = minEig;
      if ((double)minEig < p->min_eig_threshold || D < FLT_EPSILON) {
        if (level == 0) {
          status[i] = 0;
          if (info) { info[2 * i] = LK_MIN_EIG; info[2 * i + 1] = 0; }
        }
        continue;
      }
      D = 1.f / D;
      nx = nx - half_x;
      ny = ny - half_y;
      float pdx = 0.f;
      int j, why = LK_MAX_COUNT;
      for (j = 0; j < max_count; j++) {
        const int inx = cv_floor(nx), iny = cv_floor(ny);
        if (inx < -ww || inx >= v->w || iny < -wh || iny >= v->h) {
          if (level == 0) status[i] = 0;
          why = LK_NEXT_OUT;
          break;
        }
        a = nx - (float)inx;
        b = ny - (float)iny;
        weights(a, b, &w00, &w01, &w10, &w11);
        float ib1 = 0.f, ib2 = 0.f;
        for (int y = 0; y < wh; y++)
          for (int x = 0; x < ww; x++) {
            const int X = inx + x, Y = iny + y;
            const int diff = ((pix(v->J, v->w, v->h, X, Y) * w00 + pix(v->J, v->w, v->h, X + 1, Y) * w01 +
                               pix(v->J, v->w, v->h, X, Y + 1) * w10 + pix(v->J, v->w, v->h, X + 1, Y + 1) * w11 + 256) >> 9) -
                             Iw[y * ww + x];
            ib1 += (float)(diff * dIw[(y * ww + x) * 2]);
            ib2 += (float)(diff * dIw[(y * ww + x) * 2 + 1]);
          }
        const float b1 = ib1 * FLT_SCALE, b2 = ib2 * FLT_SCALE;
        const float m1 = A12 * b2, m2 = A22 * b1;
        float dx = m1 - m2;
        dx = dx * D;
        const float dy = 0.f;
        nx = nx + dx;
        ny = ny + dy;
        out[2 * i] = nx + half_x;
        out[2 * i + 1] = ny + half_y;
        if ((double)dx * (double)dx + (double)dy * (double)dy <= eps) { why = LK_CONVERGED; j++; break; }
        if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + 0.f) < 0.01) {
          out[2 * i] = out[2 * i] - dx * 0.5f;
          out[2 * i + 1] = out[2 * i + 1] - dy * 0.5f;
          why = LK_OSCILLATION;
          j++;
          break;
        }
        pdx = dx;
      }
      if (hist) hist[level * 102 + j]++;
      if (level == 0 && info) { info[2 * i] = why; info[2 * i + 1] = j; }
    }
  }
  free(pl); free(pr); free(pd); free(Iw);
  return L;
}

/* computeCorrespondences' validity check (Stereo.cpp:41-48); a negative max_disparity leaves the tracker's status */
void lk_ref_gate(const float* pts, const float* out, uint8_t* status, int n, float min_disparity, float max_disparity) {
  if (max_disparity < 0.f) return;
  for (int i = 0; i < n; i++)
    if (status[i]) {
      const float d = pts[2 * i] - out[2 * i];
      if (d <= min_disparity || d > max_disparity) status[i] = 0;
    }
}

int lk_ref_correspondences(const uint8_t* left, const uint8_t* right, int w, int h, const float* pts, int n,
                           const lk_ref_params* p, float* out, uint8_t* status, float* err) {
  const int L = lk_ref_track(left, right, w, h, pts, n, p, out, status, err, NULL, NULL);
  if (L >= 0) lk_ref_gate(pts, out, status, n, p->min_disparity, p->max_disparity);
  return L;
}

/* generateKeypoints3DStereo, the branch disparity = left.x - right.x under the status mask (Stereo.cpp:53-117,157-199) */
void lk_ref_keypoints3d(const float* pts, const float* rpts, const uint8_t* status, int n, const lk_ref_model* m, float min_depth,
                        float max_depth, float* xyz) {
  const float q = nanf("");
  for (int i = 0; i < n; i++) {
    float X = q, Y = q, Z = q;
    if (status[i]) {
      const float disp = pts[2 * i] - rpts[2 * i];
      if (disp != 0.0f && disp > 0.0f) {
        const float c = (float)(m->cx_r - m->cx_l);
        const float dc = disp + c;
        const float Wx = (float)((m->Tx_l / m->fx_l - m->Tx_r / m->fx_r) / (double)dc);
        const float Wy = (float)((m->Tx_l / m->fy_l - m->Tx_r / m->fy_r) / (double)dc);
        const float tx = (float)(((double)pts[2 * i] - m->cx_l) * (double)Wx);
        const float ty = (float)(((double)pts[2 * i + 1] - m->cy_l) * (double)Wy);
        const float tz = (float)(m->fx_l * (double)Wx);
        if (isfinite(tx) && isfinite(ty) && isfinite(tz) && (min_depth < 0.0f || tz > min_depth) &&
            (max_depth <= 0.0f || tz <= max_depth)) {
          X = tx; Y = ty; Z = tz;
          if (m->has_local) {
            const float* t = m->local;
            float s;
            s = t[0] * tx; s = s + t[1] * ty; s = s + t[2] * tz; X = s + t[3];
            s = t[4] * tx; s = s + t[5] * ty; s = s + t[6] * tz; Y = s + t[7];
            s = t[8] * tx; s = s + t[9] * ty; s = s + t[10] * tz; Z = s + t[11];
          }
        }
      }
    }
    xyz[3 * i] = X; xyz[3 * i + 1] = Y; xyz[3 * i + 2] = Z;
  }
}
