/* match_ref.c -- CPU restatement of the reference's keypoint matching, computeTransform's matchingNoGuess and matchingGuess
 * (src/slam/src/core/Registration.cpp), for 32-byte descriptor rows. TEST INFRASTRUCTURE ONLY. Written from the semantics
 * stated in include/sbm.h (sbm_match_params), loop by loop as the reference runs them:
 *
 *   no-guess  knnMatch(from, to, k = 2): per from-row the distances to every to-row in order, batchDistance's insertion (a
 *             candidate enters only on a strictly smaller distance); then NNDR and the std::set of taken to-indices.
 *   guided    matchingGuess_Projection (transformPoint's z in float, the pinhole projection in double, the border and depth
 *             test), radiusMatch's gate sqrtf(dx * dx + dy * dy) < radius per to-keypoint (this file is built with
 *             -ffp-contract=off; `fused` reads the sum as fmaf(dy, dy, dx * dx)), matchingGuess_search per projected point,
 *             then the std::set.
 *
 * match_ref_hamming(a, b)                       popcount of a XOR b over 32 bytes
 * match_ref_project(xyz, n, T, K, W, H, proj)   proj: n (u, v) float pairs, NaN where the point is not valid
 * match_ref_match(a, nf, b, nt, proj, kpts, radius, nndr, fused, rec, pairs) -> pair count; proj == NULL: no-guess.
 *             rec: nf records (best, d0, d1, candidates) over the candidates in increasing to-index (-1, 257, 257, 0 without
 *             candidates); pairs: (from, to) int32 pairs in increasing from. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NONE 257

int match_ref_hamming(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}

void match_ref_project(const float* xyz, int n, const float* T, const double* K, int W, int H, float* proj) {
  for (int i = 0; i < n; i++) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const float zc = T[8] * x + T[9] * y + T[10] * z + T[11];
    const double X = x, Y = y, Z = z;
    const double xc = (double)T[0] * X + (double)T[1] * Y + (double)T[2] * Z + (double)T[3];
    const double yc = (double)T[4] * X + (double)T[5] * Y + (double)T[6] * Z + (double)T[7];
    const double wc = (double)T[8] * X + (double)T[9] * Y + (double)T[10] * Z + (double)T[11];
    const double inv = wc != 0.0 ? 1.0 / wc : 1.0;
    const double xn = xc * inv, yn = yc * inv;
    const float u = (float)(xn * K[0] + K[2]), v = (float)(yn * K[1] + K[3]);
    if ((0.0f < u) && (u < W - 1) && (0.0f < v) && (v < H - 1) && (zc > 0.0)) {
      proj[2 * i] = u;
      proj[2 * i + 1] = v;
    } else {
      proj[2 * i] = NAN;
      proj[2 * i + 1] = NAN;
    }
  }
}

/* k-NN-2 of one query over the listed candidates, in list order */
static void knn2(const uint8_t* q, const uint8_t* b, const int* list, int nc, int* rec) {
  int best = -1, d0 = NONE, d1 = NONE;
  for (int c = 0; c < nc; c++) {
    const int d = match_ref_hamming(q, b + (size_t)list[c] * 32);
    if (d < d0) {
      d1 = d0;
      d0 = d;
      best = list[c];
    } else if (d < d1) {
      d1 = d;
    }
  }
  rec[0] = best;
  rec[1] = d0;
  rec[2] = d1;
  rec[3] = nc;
}

int match_ref_match(const uint8_t* a, int nf, const uint8_t* b, int nt, const float* proj, const float* kpts, float radius, float nndr,
                    int fused, int* rec, int* pairs) {
  int* list = (int*)malloc(sizeof(int) * (size_t)(nt > 0 ? nt : 1));
  uint8_t* added = (uint8_t*)calloc((size_t)(nt > 0 ? nt : 1), 1);   /* the std::set of taken to-indices */
  if (!list || !added) {
    free(list);
    free(added);
    return -1;
  }
  int np = 0;
  for (int i = 0; i < nf; i++) {
    int* r = rec + 4 * i;
    int nc = 0;
    if (!proj) {
      for (int j = 0; j < nt; j++) list[nc++] = j;
    } else {
      const float px = proj[2 * i], py = proj[2 * i + 1];
      if (!isnan(px) && !isnan(py)) {   /* projectedIndex holds only the valid points */
        for (int j = 0; j < nt; j++) {
          const float dx = px - kpts[2 * j], dy = py - kpts[2 * j + 1];
          const float d2 = fused ? fmaf(dy, dy, dx * dx) : dx * dx + dy * dy;
          if (sqrtf(d2) < radius) list[nc++] = j;
        }
      }
    }
    knn2(a + (size_t)i * 32, b, list, nc, r);
    int to = -1;
    if (!proj) {
      if (nt >= 2 && (float)r[1] < nndr * (float)r[2]) to = r[0];   /* nt == 1: defined as no match */
    } else if (nc == 1) {
      to = list[0];
    } else if (nc >= 2 && (float)r[1] < nndr * (float)r[2]) {
      to = r[0];
    }
    if (to >= 0 && !added[to]) {
      added[to] = 1;
      pairs[2 * np] = i;
      pairs[2 * np + 1] = to;
      np++;
    }
  }
  free(list);
  free(added);
  return np;
}
