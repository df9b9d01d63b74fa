/* gftt_select_ref.c -- CPU restatement of the reference's keypoint selection, generateKeypoints2()
 * (src/slam/src/core/GFTT.cpp:41-170), with its four constants made parameters. TEST INFRASTRUCTURE ONLY.
 *
 * Statement for statement: the threshold loop collects the addresses of the interior pixels whose value, as float, is >= the
 * double threshold; std::sort with greaterThanPtr (value descending, then address descending) orders them; the grid of
 * cvRound(minDistance)-sized cells holds the accepted points, and a candidate is rejected by any accepted point of the 3x3 cells
 * around its own one (clamped at the grid edge) with dx*dx + dy*dy < minDistance^2 (float on the left, double on the right).
 * Addresses become indices into the strided map: address order is raster order, whatever the stride.
 *
 * gfsr_select(eig, stride_elems, W, H, max, nfeatures, quality, min_distance, out_xy, out_cap) -> number of points, or -1 when
 * out of memory; at most out_cap points (x, y) are written, in acceptance order. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { const uint16_t* p; } corner;   /* a pointer into the map, as tmpCorners holds them */
typedef struct { float x, y; } point2f;
typedef struct { point2f* v; size_t n, cap; } pvec;   /* std::vector<cv::Point2f> */

/* greaterThanPtr: *a > *b, ties by the address, a > b. qsort wants "a before b" as negative. */
static int greater_than_ptr(const void* pa, const void* pb) {
  const uint16_t* a = ((const corner*)pa)->p;
  const uint16_t* b = ((const corner*)pb)->p;
  if (*a != *b) return *a > *b ? -1 : 1;
  return a > b ? -1 : (a < b ? 1 : 0);
}

static int push(pvec* m, point2f q) {
  if (m->n == m->cap) {
    size_t c = m->cap ? 2 * m->cap : 4;
    point2f* v = (point2f*)realloc(m->v, c * sizeof(point2f));
    if (!v) return -1;
    m->v = v; m->cap = c;
  }
  m->v[m->n++] = q;
  return 0;
}

/* cvRound for the non-negative values used here: round half to even (lrint in the default rounding mode) */
static int cv_round(double v) { return (int)lrint(v); }

long gfsr_select(const uint16_t* eig, size_t stride, int W, int H, unsigned max, int nfeatures, double qualityLevel,
                 double minDistance, float* out_xy, long out_cap) {
  /* Thresholding */
  double thr = (unsigned short)max * qualityLevel;
  size_t total = 0, cap = 16;
  corner* tmpCorners = (corner*)malloc(cap * sizeof(corner));
  if (!tmpCorners) return -1;
  for (int y = 1; y < H - 1; y++) {
    const uint16_t* eig_data = eig + (size_t)y * stride;
    for (int x = 1; x < W - 1; x++) {
      float val = eig_data[x];
      if (val >= thr) {
        if (total == cap) {
          corner* t = (corner*)realloc(tmpCorners, 2 * cap * sizeof(corner));
          if (!t) { free(tmpCorners); return -1; }
          tmpCorners = t; cap *= 2;
        }
        tmpCorners[total++].p = eig_data + x;
      }
    }
  }
  /* sort in descending order (greaterThanPtr is a total order, so any correct sort gives the same sequence) */
  qsort(tmpCorners, total, sizeof(corner), greater_than_ptr);

  /* Trim Neighbor */
  long ncorners = 0;
  if (minDistance >= 1) {
    const int w = W, h = H;
    const int cell_size = cv_round(minDistance);
    const int grid_width = (w + cell_size - 1) / cell_size;
    const int grid_height = (h + cell_size - 1) / cell_size;
    pvec* grid = (pvec*)calloc((size_t)grid_width * grid_height, sizeof(pvec));
    if (!grid) { free(tmpCorners); return -1; }
    minDistance *= minDistance;
    for (size_t i = 0; i < total; i++) {
      const size_t ofs = (size_t)(tmpCorners[i].p - eig);
      const int y = (int)(ofs / stride);
      const int x = (int)(ofs - (size_t)y * stride);
      int good = 1;
      const int x_cell = x / cell_size;
      const int y_cell = y / cell_size;
      int x1 = x_cell - 1, y1 = y_cell - 1, x2 = x_cell + 1, y2 = y_cell + 1;
      /* boundary check */
      if (x1 < 0) x1 = 0;
      if (y1 < 0) y1 = 0;
      if (x2 > grid_width - 1) x2 = grid_width - 1;
      if (y2 > grid_height - 1) y2 = grid_height - 1;
      for (int yy = y1; yy <= y2 && good; yy++) {
        for (int xx = x1; xx <= x2 && good; xx++) {
          const pvec* m = &grid[(size_t)yy * grid_width + xx];
          for (size_t j = 0; j < m->n; j++) {
            float dx = x - m->v[j].x;
            float dy = y - m->v[j].y;
            if (dx * dx + dy * dy < minDistance) { good = 0; break; }
          }
        }
      }
      if (good) {
        const point2f q = {(float)x, (float)y};
        if (push(&grid[(size_t)y_cell * grid_width + x_cell], q)) { ncorners = -1; break; }
        if (ncorners < out_cap) { out_xy[2 * ncorners] = q.x; out_xy[2 * ncorners + 1] = q.y; }
        ++ncorners;
        if (nfeatures > 0 && ncorners == nfeatures) break;
      }
    }
    for (size_t k = 0; k < (size_t)grid_width * grid_height; k++) free(grid[k].v);
    free(grid);
  } else {
    /* no trimming */
    for (size_t i = 0; i < total; i++) {
      const size_t ofs = (size_t)(tmpCorners[i].p - eig);
      const int y = (int)(ofs / stride);
      const int x = (int)(ofs - (size_t)y * stride);
      if (ncorners < out_cap) { out_xy[2 * ncorners] = (float)x; out_xy[2 * ncorners + 1] = (float)y; }
      ++ncorners;
      if (nfeatures > 0 && ncorners == nfeatures) break;
    }
  }
  free(tmpCorners);
  return ncorners;
}

/* The number of candidates (interior pixels with (float)value >= max * qualityLevel). */
long gfsr_candidates(const uint16_t* eig, size_t stride, int W, int H, unsigned max, double qualityLevel) {
  double thr = (unsigned short)max * qualityLevel;
  long total = 0;
  for (int y = 1; y < H - 1; y++)
    for (int x = 1; x < W - 1; x++) {
      float val = eig[(size_t)y * stride + x];
      if (val >= thr) total++;
    }
  return total;
}
