/* sgbm_ref.c -- CPU restatement of cv::StereoSGBM::compute() (calib3d stereosgbm.cpp, computeDisparitySGBM, as recalled) for
 * 8-bit single-channel pairs in MODE_HH and MODE_SGBM. TEST INFRASTRUCTURE ONLY: the engine (libsbm_hip.so) never links it.
 *
 * Written statement for statement after OpenCV's single-threaded implementation, loop order included (the selection loop runs
 * x descending, which decides ties of the claim table): per-row calcPixelCostBT, the incremental box sum over hsumBuf rows,
 * C biased by P2, the 4-direction Lr sweep per pass (x ascending then descending), the fifth path of MODE_SGBM inside the
 * selection loop, winner/uniqueness/sub-pixel, the disp2 claim table and the LR check, then medianBlur(3). The speckle stage
 * is the block matcher's restatement, called from sgbm_ref.py.
 *
 * Everything is computed in `int` and stored as `short` exactly where OpenCV stores CostType; inside the exactness envelope
 * (include/sbm.h) none of those stores wraps. Callers check the envelope first (sgbm_ref.py). */
#include <limits.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/sbm.h"

typedef short CostType;
typedef short DispType;
typedef unsigned char PixType;

#define SGBMR_READ_NO_MEDIAN 32
#define SGBMR_READ_BOTTOM_CLAMPED 64

enum { NR = 16, NR2 = NR / 2, DISP_SHIFT = 4, DISP_SCALE = 1 << DISP_SHIFT };

static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }

/* calcPixelCostBT for one row y, cn == 1: cost[x*D + d] for x in [0, width1), d in [0, D) (d = disparity - minD). */
static void calc_pixel_cost_bt(const uint8_t* img1, size_t step1, const uint8_t* img2, size_t step2, int width, int height, int y,
                               int minD, int maxD, CostType* cost, PixType* buffer, const PixType* tab) {
  int x, c;
  const int minX1 = imax(maxD, 0), maxX1 = width + imin(minD, 0);
  const int D = maxD - minD, width1 = maxX1 - minX1;
  const int minX2 = imax(minX1 - maxD, 0), maxX2 = imin(maxX1 - minD, width);
  const int width2 = maxX2 - minX2;
  const PixType *row1 = img1 + (size_t)y * step1, *row2 = img2 + (size_t)y * step2;
  PixType *prow1 = buffer + width2 * 2, *prow2 = prow1 + width * 2;

  for (c = 0; c < 2; c++) prow1[width * c] = prow1[width * c + width - 1] = prow2[width * c] = prow2[width * c + width - 1] = tab[0];

  const long n1 = y > 0 ? -(long)step1 : 0, s1 = y < height - 1 ? (long)step1 : 0;
  const long n2 = y > 0 ? -(long)step2 : 0, s2 = y < height - 1 ? (long)step2 : 0;

  int minX_cmn = imin(minX1, minX2) - 1;
  int maxX_cmn = imax(maxX1, maxX2) + 1;
  minX_cmn = imax(minX_cmn, 1);
  maxX_cmn = imin(maxX_cmn, width - 1);
  for (x = minX_cmn; x < maxX_cmn; x++) {
    prow1[x] = tab[(row1[x + 1] - row1[x - 1]) * 2 + row1[x + n1 + 1] - row1[x + n1 - 1] + row1[x + s1 + 1] - row1[x + s1 - 1]];
    prow2[width - 1 - x] = tab[(row2[x + 1] - row2[x - 1]) * 2 + row2[x + n2 + 1] - row2[x + n2 - 1] + row2[x + s2 + 1] - row2[x + s2 - 1]];
    prow1[x + width] = row1[x];
    prow2[width - 1 - x + width] = row2[x];
  }

  memset(cost, 0, (size_t)width1 * D * sizeof(cost[0]));
  buffer -= width - 1 - maxX2;
  cost -= minX1 * D + minD;   /* simplify the cost indices inside the loop */

  for (c = 0; c < 2; c++, prow1 += width, prow2 += width) {
    const int diff_scale = c < 1 ? 0 : 2;
    /* v0 = min(row2[x-1/2], row2[x], row2[x+1/2]) and v1 = max(...) */
    for (x = width - 1 - maxX2; x < width - 1 - minX2; x++) {
      int v = prow2[x];
      int vl = x > 0 ? (v + prow2[x - 1]) / 2 : v;
      int vr = x < width - 1 ? (v + prow2[x + 1]) / 2 : v;
      int v0 = imin(vl, vr); v0 = imin(v0, v);
      int v1 = imax(vl, vr); v1 = imax(v1, v);
      buffer[x] = (PixType)v0;
      buffer[x + width2] = (PixType)v1;
    }
    for (x = minX1; x < maxX1; x++) {
      int u = prow1[x];
      int ul = x > 0 ? (u + prow1[x - 1]) / 2 : u;
      int ur = x < width - 1 ? (u + prow1[x + 1]) / 2 : u;
      int u0 = imin(ul, ur); u0 = imin(u0, u);
      int u1 = imax(ul, ur); u1 = imax(u1, u);
      for (int d = minD; d < maxD; d++) {
        int v = prow2[width - x - 1 + d];
        int v0 = buffer[width - x - 1 + d];
        int v1 = buffer[width - x - 1 + d + width2];
        int c0 = imax(0, u - v1); c0 = imax(c0, v0 - u);
        int c1 = imax(0, v - u1); c1 = imax(c1, u0 - v);
        cost[x * D + d] = (CostType)(cost[x * D + d] + (imin(c0, c1) >> diff_scale));
      }
    }
  }
}

static void median3x3(const int16_t* src, int16_t* dst, int width, int height) {
  for (int y = 0; y < height; y++)
    for (int x = 0; x < width; x++) {
      int v[9], k = 0;
      for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
          const int yy = imin(imax(y + dy, 0), height - 1), xx = imin(imax(x + dx, 0), width - 1);
          v[k++] = src[(size_t)yy * width + xx];
        }
      for (int i = 1; i < 9; i++)   /* insertion sort: the median of nine */
        for (int j = i; j > 0 && v[j - 1] > v[j]; j--) { int t = v[j]; v[j] = v[j - 1]; v[j - 1] = t; }
      dst[(size_t)y * width + x] = (int16_t)v[4];
    }
}

/* disp: height*width (dense). Optional outputs: C_out / S_out = height * width1 * D (C as OpenCV keeps it, biased by P2; S after
 * all paths), pre_out = height*width (the map before the median). Returns 0, or -1 when a buffer cannot be allocated. */
int sgbmr_compute(const sbm_sgbm_params* params, const uint8_t* img1, size_t step1, const uint8_t* img2, size_t step2, int width,
                  int height, int16_t* disp, int16_t* C_out, int16_t* S_out, int16_t* pre_out, int reading) {
  const CostType MAX_COST = SHRT_MAX;
  const int minD = params->min_disparity, maxD = minD + params->num_disparities;
  const int SADWindowSize = params->block_size > 0 ? params->block_size : 5;
  const int ftzero = imax(params->prefilter_cap, 15) | 1;
  const int uniquenessRatio = params->uniqueness_ratio >= 0 ? params->uniqueness_ratio : 10;
  const int disp12MaxDiff = params->disp12_max_diff > 0 ? params->disp12_max_diff : 1;
  const int P1 = params->p1 > 0 ? params->p1 : 2, P2 = imax(params->p2 > 0 ? params->p2 : 5, P1 + 1);
  const int minX1 = imax(maxD, 0), maxX1 = width + imin(minD, 0);
  const int D = maxD - minD, width1 = maxX1 - minX1;
  const int INVALID_DISP = minD - 1, INVALID_DISP_SCALED = INVALID_DISP * DISP_SCALE;
  const int SW2 = SADWindowSize / 2, SH2 = SADWindowSize / 2;
  const int fullDP = params->mode == SBM_SGBM_MODE_HH;
  const int npasses = fullDP ? 2 : 1;
  enum { TAB_OFS = 256 * 4, TAB_SIZE = 256 + TAB_OFS * 2 };
  PixType clipTab[TAB_SIZE];
  int k;
  int16_t* disp1 = pre_out ? pre_out : (int16_t*)malloc((size_t)width * height * sizeof(int16_t));
  if (!disp1) return -1;

  for (k = 0; k < TAB_SIZE; k++) clipTab[k] = (PixType)(imin(imax(k - TAB_OFS, -ftzero), ftzero) + ftzero);

  if (minX1 >= maxX1) {
    for (size_t i = 0; i < (size_t)width * height; i++) disp1[i] = (int16_t)INVALID_DISP_SCALED;
  } else {
    const int D2 = D + 16, NRD2 = NR2 * D2;
    const int NLR = 2, LrBorder = NLR - 1;
    const size_t costBufSize = (size_t)width1 * D;
    const size_t CSBufSize = costBufSize * (fullDP ? height : 1);
    const size_t minLrSize = (size_t)(width1 + LrBorder * 2) * NR2, LrSize = minLrSize * D2;
    const int hsumBufNRows = SH2 * 2 + 2;
    CostType* Cbuf = (CostType*)malloc(CSBufSize * sizeof(CostType));
    CostType* Sbuf = (CostType*)malloc(CSBufSize * sizeof(CostType));
    CostType* hsumBuf = (CostType*)malloc(costBufSize * hsumBufNRows * sizeof(CostType));
    CostType* pixDiff = (CostType*)malloc(costBufSize * sizeof(CostType));
    CostType* LrBuf = (CostType*)malloc((LrSize * NLR + 16) * sizeof(CostType));
    CostType* minLrBuf = (CostType*)malloc(minLrSize * NLR * sizeof(CostType));
    CostType* disp2cost = (CostType*)malloc((size_t)width * sizeof(CostType));
    DispType* disp2ptr = (DispType*)malloc((size_t)width * sizeof(DispType));
    PixType* tempBuf = (PixType*)malloc((size_t)width * 16);
    if (!Cbuf || !Sbuf || !hsumBuf || !pixDiff || !LrBuf || !minLrBuf || !disp2cost || !disp2ptr || !tempBuf) {
      free(Cbuf); free(Sbuf); free(hsumBuf); free(pixDiff); free(LrBuf); free(minLrBuf); free(disp2cost); free(disp2ptr); free(tempBuf);
      if (!pre_out) free(disp1);
      return -1;
    }

    /* add P2 to every C(x,y). it saves a few operations in the inner loops */
    for (k = 0; k < (int)CSBufSize; k++) Cbuf[k] = (CostType)P2;

    for (int pass = 1; pass <= npasses; pass++) {
      int x1, y1, x2, y2, dx, dy;
      if (pass == 1) { y1 = 0; y2 = height; dy = 1; x1 = 0; x2 = width1; dx = 1; }
      else { y1 = height - 1; y2 = -1; dy = -1; x1 = width1 - 1; x2 = -1; dx = -1; }

      CostType *Lr[2], *minLr[2];
      for (k = 0; k < NLR; k++) {
        Lr[k] = LrBuf + LrSize * k + NRD2 * LrBorder + 8;
        memset(Lr[k] - LrBorder * NRD2 - 8, 0, LrSize * sizeof(CostType));
        minLr[k] = minLrBuf + minLrSize * k + NR2 * LrBorder;
        memset(minLr[k] - LrBorder * NR2, 0, minLrSize * sizeof(CostType));
      }

      for (int y = y1; y != y2; y += dy) {
        int x, d;
        DispType* disp1ptr = disp1 + (size_t)y * width;
        CostType* C = Cbuf + (!fullDP ? 0 : (size_t)y * costBufSize);
        CostType* S = Sbuf + (!fullDP ? 0 : (size_t)y * costBufSize);

        if (pass == 1) {   /* compute C on the first pass, and reuse it on the second pass, if any */
          int dy1 = y == 0 ? 0 : y + SH2, dy2 = y == 0 ? SH2 : dy1;
          for (k = dy1; k <= dy2; k++) {
            CostType* hsumAdd = hsumBuf + (size_t)(imin(k, height - 1) % hsumBufNRows) * costBufSize;
            /* reading 64: rows past the bottom re-add the last row (a clamped window) instead of leaving C as it is */
            const int kk = (k >= height && y > 0 && (reading & SGBMR_READ_BOTTOM_CLAMPED)) ? height - 1 : k;
            if (kk < height) {
              if (kk == k) {
                calc_pixel_cost_bt(img1, step1, img2, step2, width, height, k, minD, maxD, pixDiff, tempBuf, clipTab + TAB_OFS);
                memset(hsumAdd, 0, D * sizeof(CostType));
                for (d = 0; d < D; d++) {
                  hsumAdd[d] = (CostType)(pixDiff[d] * (SW2 + 1));
                  for (x = 1; x <= SW2; x++) hsumAdd[d] = (CostType)(hsumAdd[d] + pixDiff[(size_t)imin(x, width1 - 1) * D + d]);
                }
              }
              if (y > 0) {
                const CostType* hsumSub = hsumBuf + (size_t)(imax(y - SH2 - 1, 0) % hsumBufNRows) * costBufSize;
                const CostType* Cprev = !fullDP || y == 0 ? C : C - costBufSize;
                for (d = 0; d < D; d++) C[d] = (CostType)(Cprev[d] + hsumAdd[d] - hsumSub[d]);
                for (x = D; x < (int)(width1 * D); x += D) {
                  const CostType* pixAdd = pixDiff + imin(x + SW2 * D, (width1 - 1) * D);
                  const CostType* pixSub = pixDiff + imax(x - (SW2 + 1) * D, 0);
                  for (d = 0; d < D; d++) {
                    int hv = kk == k ? (hsumAdd[x + d] = (CostType)(hsumAdd[x - D + d] + pixAdd[d] - pixSub[d])) : hsumAdd[x + d];
                    C[x + d] = (CostType)(Cprev[x + d] + hv - hsumSub[x + d]);
                  }
                }
              } else {
                for (x = D; x < (int)(width1 * D); x += D) {
                  const CostType* pixAdd = pixDiff + imin(x + SW2 * D, (width1 - 1) * D);
                  const CostType* pixSub = pixDiff + imax(x - (SW2 + 1) * D, 0);
                  for (d = 0; d < D; d++) hsumAdd[x + d] = (CostType)(hsumAdd[x - D + d] + pixAdd[d] - pixSub[d]);
                }
              }
            }
            if (y == 0) {
              int scale = k == 0 ? SH2 + 1 : 1;
              for (x = 0; x < (int)(width1 * D); x++) C[x] = (CostType)(C[x] + hsumAdd[x] * scale);
            }
          }
          /* also, clear the S buffer */
          for (k = 0; k < (int)(width1 * D); k++) S[k] = 0;
          if (C_out) memcpy(C_out + (size_t)y * costBufSize, C, costBufSize * sizeof(CostType));
        }

        /* clear the left and the right borders */
        memset(Lr[0] - NRD2 * LrBorder - 8, 0, NRD2 * LrBorder * sizeof(CostType));
        memset(Lr[0] + width1 * NRD2 - 8, 0, NRD2 * LrBorder * sizeof(CostType));
        memset(minLr[0] - NR2 * LrBorder, 0, NR2 * LrBorder * sizeof(CostType));
        memset(minLr[0] + width1 * NR2, 0, NR2 * LrBorder * sizeof(CostType));

        /* L_r(p,d) = C(p,d) + min(L_r(p-r,d), L_r(p-r,d-1) + P1, L_r(p-r,d+1) + P1, min_k L_r(p-r,k) + P2) - min_k L_r(p-r,k)
         * directions of this pass: 0: r=(-dx,0), 1: r=(-1,-dy), 2: r=(0,-dy), 3: r=(1,-dy) */
        for (x = x1; x != x2; x += dx) {
          int xm = x * NR2, xd = xm * D2;
          int delta0 = minLr[0][xm - dx * NR2] + P2, delta1 = minLr[1][xm - NR2 + 1] + P2;
          int delta2 = minLr[1][xm + 2] + P2, delta3 = minLr[1][xm + NR2 + 3] + P2;
          CostType* Lr_p0 = Lr[0] + xd - dx * NRD2;
          CostType* Lr_p1 = Lr[1] + xd - NRD2 + D2;
          CostType* Lr_p2 = Lr[1] + xd + D2 * 2;
          CostType* Lr_p3 = Lr[1] + xd + NRD2 + D2 * 3;
          Lr_p0[-1] = Lr_p0[D] = Lr_p1[-1] = Lr_p1[D] = Lr_p2[-1] = Lr_p2[D] = Lr_p3[-1] = Lr_p3[D] = MAX_COST;
          CostType* Lr_p = Lr[0] + xd;
          const CostType* Cp = C + (size_t)x * D;
          CostType* Sp = S + (size_t)x * D;
          int minL0 = MAX_COST, minL1 = MAX_COST, minL2 = MAX_COST, minL3 = MAX_COST;
          for (d = 0; d < D; d++) {
            int Cpd = Cp[d], L0, L1, L2, L3;
            L0 = Cpd + imin((int)Lr_p0[d], imin(Lr_p0[d - 1] + P1, imin(Lr_p0[d + 1] + P1, delta0))) - delta0;
            L1 = Cpd + imin((int)Lr_p1[d], imin(Lr_p1[d - 1] + P1, imin(Lr_p1[d + 1] + P1, delta1))) - delta1;
            L2 = Cpd + imin((int)Lr_p2[d], imin(Lr_p2[d - 1] + P1, imin(Lr_p2[d + 1] + P1, delta2))) - delta2;
            L3 = Cpd + imin((int)Lr_p3[d], imin(Lr_p3[d - 1] + P1, imin(Lr_p3[d + 1] + P1, delta3))) - delta3;
            Lr_p[d] = (CostType)L0; minL0 = imin(minL0, L0);
            Lr_p[d + D2] = (CostType)L1; minL1 = imin(minL1, L1);
            Lr_p[d + D2 * 2] = (CostType)L2; minL2 = imin(minL2, L2);
            Lr_p[d + D2 * 3] = (CostType)L3; minL3 = imin(minL3, L3);
            int s = Sp[d] + L0 + L1 + L2 + L3;   /* saturate_cast<CostType> */
            Sp[d] = (CostType)(s > SHRT_MAX ? SHRT_MAX : s < SHRT_MIN ? SHRT_MIN : s);
          }
          minLr[0][xm] = (CostType)minL0;
          minLr[0][xm + 1] = (CostType)minL1;
          minLr[0][xm + 2] = (CostType)minL2;
          minLr[0][xm + 3] = (CostType)minL3;
        }

        if (pass == npasses) {
          for (x = 0; x < width; x++) {
            disp1ptr[x] = disp2ptr[x] = (DispType)INVALID_DISP_SCALED;
            disp2cost[x] = MAX_COST;
          }
          for (x = width1 - 1; x >= 0; x--) {
            CostType* Sp = S + (size_t)x * D;
            int minS = MAX_COST, bestDisp = -1;
            if (npasses == 1) {
              int xm = x * NR2, xd = xm * D2;
              int minL0 = MAX_COST;
              int delta0 = minLr[0][xm + NR2] + P2;
              CostType* Lr_p0 = Lr[0] + xd + NRD2;
              Lr_p0[-1] = Lr_p0[D] = MAX_COST;
              CostType* Lr_p = Lr[0] + xd;
              const CostType* Cp = C + (size_t)x * D;
              for (d = 0; d < D; d++) {
                int L0 = Cp[d] + imin((int)Lr_p0[d], imin(Lr_p0[d - 1] + P1, imin(Lr_p0[d + 1] + P1, delta0))) - delta0;
                Lr_p[d] = (CostType)L0;
                minL0 = imin(minL0, L0);
                int s = Sp[d] + L0;
                int Sval = Sp[d] = (CostType)(s > SHRT_MAX ? SHRT_MAX : s < SHRT_MIN ? SHRT_MIN : s);
                if (Sval < minS) { minS = Sval; bestDisp = d; }
              }
              minLr[0][xm] = (CostType)minL0;
            } else {
              for (d = 0; d < D; d++) {
                int Sval = Sp[d];
                if (Sval < minS) { minS = Sval; bestDisp = d; }
              }
            }
            for (d = 0; d < D; d++)
              if (Sp[d] * (100 - uniquenessRatio) < minS * 100 && abs(bestDisp - d) > 1) break;
            if (d < D) continue;
            d = bestDisp;
            int _x2 = x + minX1 - d - minD;
            /* (with every S saturated, d is still -1 here and _x2 may be one past the row; OpenCV reads that element, but a
             * short is never > MAX_COST, so the claim cannot be taken: the restatement does not read it) */
            if (minS < MAX_COST && disp2cost[_x2] > minS) {
              disp2cost[_x2] = (CostType)minS;
              disp2ptr[_x2] = (DispType)(d + minD);
            }
            if (0 < d && d < D - 1) {
              /* subpixel quadratic interpolation through (d-1, Sp[d-1]), (d, Sp[d]), (d+1, Sp[d+1]) */
              int denom2 = imax(Sp[d - 1] + Sp[d + 1] - 2 * Sp[d], 1);
              d = d * DISP_SCALE + ((Sp[d - 1] - Sp[d + 1]) * DISP_SCALE + denom2) / (denom2 * 2);
            } else {
              d *= DISP_SCALE;
            }
            disp1ptr[x + minX1] = (DispType)(d + minD * DISP_SCALE);
          }
          for (x = minX1; x < maxX1; x++) {
            /* round the computed disparity both towards -inf and +inf and check whether either is consistent in disp2 */
            int d1 = disp1ptr[x];
            if (d1 == INVALID_DISP_SCALED) continue;
            int _d = d1 >> DISP_SHIFT;
            int d_ = (d1 + DISP_SCALE - 1) >> DISP_SHIFT;
            int _x = x - _d, x_ = x - d_;
            if (0 <= _x && _x < width && disp2ptr[_x] >= minD && abs(disp2ptr[_x] - _d) > disp12MaxDiff && 0 <= x_ && x_ < width &&
                disp2ptr[x_] >= minD && abs(disp2ptr[x_] - d_) > disp12MaxDiff)
              disp1ptr[x] = (DispType)INVALID_DISP_SCALED;
          }
          if (S_out) memcpy(S_out + (size_t)y * costBufSize, S, costBufSize * sizeof(CostType));
        }
        /* now shift the cyclic buffers */
        { CostType* t = Lr[0]; Lr[0] = Lr[1]; Lr[1] = t; }
        { CostType* t = minLr[0]; minLr[0] = minLr[1]; minLr[1] = t; }
      }
    }
    free(Cbuf); free(Sbuf); free(hsumBuf); free(pixDiff); free(LrBuf); free(minLrBuf); free(disp2cost); free(disp2ptr); free(tempBuf);
  }

  if (reading & SGBMR_READ_NO_MEDIAN) memcpy(disp, disp1, (size_t)width * height * sizeof(int16_t));
  else median3x3(disp1, disp, width, height);
  if (!pre_out) free(disp1);
  return 0;
}
