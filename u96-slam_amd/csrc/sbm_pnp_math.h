/* sbm_pnp_math.h -- the double-precision arithmetic of estimateMotion3DTo2D (include/sbm.h), written once
 * and compiled twice: as HIP device code in sbm_pnp.hip (with contraction off) and as C11 in the tests' sequential restatement,
 * pnp_ref.c (-ffp-contract=off). Only + - * / and sqrt reach the bits that must agree; the transcendental calls (acos, cos,
 * sin in Rodrigues; acos in the covariance angles) are the places where libm and the device library may differ in the last ulp.
 * Plain C on purpose: no templates, no references, fixed-size arrays, every loop bounded. */
#ifndef SBM_PNP_MATH_H_
#define SBM_PNP_MATH_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define PNP_FN __host__ __device__ static inline
#else
#define PNP_FN static inline
#endif
#ifdef __clang__
#pragma clang fp contract(off)
#endif

#define PNP_LANES 64          /* the refine's reductions: lane s sums points s, s + 64, ...; then the 64 partials in lane order */
#define PNP_LD 12             /* row stride of the Jacobi SVD's matrices (at most 12 x 12) */
#define PNP_DBL_EPS 2.2204460492503131e-16
#define PNP_DBL_MIN 2.2250738585072014e-308
#define PNP_FLT_EPS 1.1920928955078125e-07

/* ---- cv::RNG((uint64)-1) and RANSACPointSetRegistrator::getSubset (no partial-subset checks) ------------------------------ */
PNP_FN unsigned pnp_rng_next(uint64_t* s) {
  *s = (uint64_t)(unsigned)*s * 4164903690u + (*s >> 32);
  return (unsigned)*s;
}

PNP_FN void pnp_draw_subset(uint64_t* s, int n, int* idx) {
  for (int i = 0; i < 6; i++) {
    for (;;) {
      int v = (int)(pnp_rng_next(s) % (unsigned)n), j;
      for (j = 0; j < i; j++)
        if (idx[j] == v) break;
      idx[i] = v;
      if (j == i) break;
    }
  }
}

/* RANSACUpdateNumIters (CvSolvePnP.cpp:216-236); cvRound = round half to even. */
PNP_FN int pnp_update_num_iters(double p, double ep, int model_points, int max_iters) {
  p = p > 0. ? p : 0.;
  p = p < 1. ? p : 1.;
  ep = ep > 0. ? ep : 0.;
  ep = ep < 1. ? ep : 1.;
  double num = 1. - p > PNP_DBL_MIN ? 1. - p : PNP_DBL_MIN;
  double denom = 1. - pow(1. - ep, model_points);
  if (denom < PNP_DBL_MIN) return 0;
  num = log(num);
  denom = log(denom);
  return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)rint(num / denom);
}

/* ---- one-sided Jacobi SVD (cv::SVD::compute's JacobiSVDImpl_, recalled) -------------------------------------------------
 * At: n rows of length m (the columns of A, m >= n), row stride PNP_LD. On return W holds the singular values in descending
 * order, At's rows the left singular vectors (scaled by 1 / W; a zero singular value leaves its row as it is -- OpenCV completes
 * it with a random orthogonal vector), Vt's rows the right singular vectors. Pairs (i, j) in row-major cyclic order; a sweep
 * without a rotation ends it, at most max(m, 30) sweeps, so a degenerate or NaN input ends in a bounded number of steps. */
PNP_FN void pnp_jacobi_svd(double* At, double* W, double* Vt, int m, int n) {
  const double eps = PNP_DBL_EPS * 10;
  const int max_iter = m > 30 ? m : 30;
  for (int i = 0; i < n; i++) {
    double sd = 0;
    for (int k = 0; k < m; k++) sd += At[i * PNP_LD + k] * At[i * PNP_LD + k];
    W[i] = sd;
    for (int k = 0; k < n; k++) Vt[i * PNP_LD + k] = 0;
    Vt[i * PNP_LD + i] = 1;
  }
  for (int iter = 0; iter < max_iter; iter++) {
    int changed = 0;
    for (int i = 0; i < n - 1; i++)
      for (int j = i + 1; j < n; j++) {
        double* Ai = At + i * PNP_LD;
        double* Aj = At + j * PNP_LD;
        double a = W[i], p = 0, b = W[j];
        for (int k = 0; k < m; k++) p += Ai[k] * Aj[k];
        if (fabs(p) <= eps * sqrt(a * b)) continue;
        p *= 2;
        double beta = a - b, gamma = sqrt(p * p + beta * beta), c, s;   /* hypot in OpenCV: not pinned */
        if (beta < 0) {
          double delta = (gamma - beta) * 0.5;
          s = sqrt(delta / gamma);
          c = p / (gamma * s * 2);
        } else {
          c = sqrt((gamma + beta) / (gamma * 2));
          s = p / (gamma * c * 2);
        }
        a = b = 0;
        for (int k = 0; k < m; k++) {
          double t0 = c * Ai[k] + s * Aj[k];
          double t1 = -s * Ai[k] + c * Aj[k];
          Ai[k] = t0;
          Aj[k] = t1;
          a += t0 * t0;
          b += t1 * t1;
        }
        W[i] = a;
        W[j] = b;
        changed = 1;
        double* Vi = Vt + i * PNP_LD;
        double* Vj = Vt + j * PNP_LD;
        for (int k = 0; k < n; k++) {
          double t0 = c * Vi[k] + s * Vj[k];
          double t1 = -s * Vi[k] + c * Vj[k];
          Vi[k] = t0;
          Vj[k] = t1;
        }
      }
    if (!changed) break;
  }
  for (int i = 0; i < n; i++) {
    double sd = 0;
    for (int k = 0; k < m; k++) sd += At[i * PNP_LD + k] * At[i * PNP_LD + k];
    W[i] = sqrt(sd);
  }
  for (int i = 0; i < n - 1; i++) {
    int j = i;
    for (int k = i + 1; k < n; k++)
      if (W[j] < W[k]) j = k;
    if (i != j) {
      double t = W[i];
      W[i] = W[j];
      W[j] = t;
      for (int k = 0; k < m; k++) {
        t = At[i * PNP_LD + k];
        At[i * PNP_LD + k] = At[j * PNP_LD + k];
        At[j * PNP_LD + k] = t;
      }
      for (int k = 0; k < n; k++) {
        t = Vt[i * PNP_LD + k];
        Vt[i * PNP_LD + k] = Vt[j * PNP_LD + k];
        Vt[j * PNP_LD + k] = t;
      }
    }
  }
  for (int i = 0; i < n; i++)
    if (W[i] > PNP_DBL_MIN) {
      double sd = 1. / W[i];
      for (int k = 0; k < m; k++) At[i * PNP_LD + k] *= sd;
    }
}

/* x = pinv(A) b for A m x n (row-major, stride n; m >= n), as cv::solve(DECOMP_SVD): singular values at or below
 * 2 DBL_EPSILON times their sum are dropped (the back-substitution's order: recalled, not pinned). */
PNP_FN void pnp_svd_solve(const double* A, int m, int n, const double* b, double* x) {
  double At[PNP_LD * PNP_LD], Vt[PNP_LD * PNP_LD], W[PNP_LD];
  for (int i = 0; i < n; i++)
    for (int k = 0; k < m; k++) At[i * PNP_LD + k] = A[k * n + i];
  pnp_jacobi_svd(At, W, Vt, m, n);
  double thr = 0;
  for (int i = 0; i < n; i++) thr += W[i];
  thr *= PNP_DBL_EPS * 2;
  for (int j = 0; j < n; j++) x[j] = 0;
  for (int i = 0; i < n; i++) {
    if (fabs(W[i]) <= thr) continue;
    double s = 0;
    for (int k = 0; k < m; k++) s += At[i * PNP_LD + k] * b[k];
    s *= 1. / W[i];
    for (int j = 0; j < n; j++) x[j] += s * Vt[i * PNP_LD + j];
  }
}

/* ---- EPnP on six points (OpenCV's epnp class, recalled) -------------------------------------------------------------------
 * pw: 6 float (x, y, z); uv: 6 float (u, v) pixels; K: fx, fy, cx, cy. The image points pass through solvePnP's undistortPoints
 * (zero distortion): normalised (float)(((double)u - cx) * (1 / fx)), then epnp::init_points' u * fx + cx, in double. */
PNP_FN double pnp_dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

PNP_FN double pnp_dist2(const double* a, const double* b) {
  return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

/* epnp::qr_solve on the 6 x 4 Gauss-Newton system; A and b are overwritten. On a zero column it returns early and x keeps its
 * previous value, as OpenCV's does. */
PNP_FN void pnp_qr_solve(double* A, double* b, double* X) {
  const int nr = 6, nc = 4;
  double A1[4], A2[4];
  double* pA = A;
  double* ppAkk = pA;
  for (int k = 0; k < nc; k++) {
    double* ppAik1 = ppAkk;
    double eta = fabs(*ppAik1);
    for (int i = k + 1; i < nr; i++) {
      double elt = fabs(*ppAik1);
      if (eta < elt) eta = elt;
      ppAik1 += nc;
    }
    if (eta == 0) {
      A1[k] = A2[k] = 0.0;
      return;
    }
    double* ppAik2 = ppAkk;
    double sum2 = 0.0, inv_eta = 1. / eta;
    for (int i = k; i < nr; i++) {
      *ppAik2 *= inv_eta;
      sum2 += *ppAik2 * *ppAik2;
      ppAik2 += nc;
    }
    double sigma = sqrt(sum2);
    if (*ppAkk < 0) sigma = -sigma;
    *ppAkk += sigma;
    A1[k] = sigma * *ppAkk;
    A2[k] = -eta * sigma;
    for (int j = k + 1; j < nc; j++) {
      double* ppAik = ppAkk;
      double sum = 0;
      for (int i = k; i < nr; i++) {
        sum += *ppAik * ppAik[j - k];
        ppAik += nc;
      }
      double tau = sum / A1[k];
      ppAik = ppAkk;
      for (int i = k; i < nr; i++) {
        ppAik[j - k] -= tau * *ppAik;
        ppAik += nc;
      }
    }
    ppAkk += nc + 1;
  }
  double* ppAjj = pA;
  double* pb = b;
  for (int j = 0; j < nc; j++) {
    double* ppAij = ppAjj;
    double tau = 0;
    for (int i = j; i < nr; i++) {
      tau += *ppAij * pb[i];
      ppAij += nc;
    }
    tau /= A1[j];
    ppAij = ppAjj;
    for (int i = j; i < nr; i++) {
      pb[i] -= tau * *ppAij;
      ppAij += nc;
    }
    ppAjj += nc + 1;
  }
  X[nc - 1] = pb[nc - 1] / A2[nc - 1];
  for (int i = nc - 2; i >= 0; i--) {
    double* ppAij = pA + i * nc + (i + 1);
    double sum = 0;
    for (int j = i + 1; j < nc; j++) {
      sum += *ppAij * X[j];
      ppAij++;
    }
    X[i] = (pb[i] - sum) / A2[i];
  }
}

PNP_FN void pnp_gauss_newton(const double* L, const double* rho, double* betas) {
  double A[24], b[6], x[4] = {0, 0, 0, 0};
  for (int k = 0; k < 5; k++) {
    for (int i = 0; i < 6; i++) {
      const double* rowL = L + i * 10;
      double* rowA = A + i * 4;
      rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
      rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
      rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
      rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
      b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] +
                       rowL[3] * betas[0] * betas[2] + rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                       rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] + rowL[8] * betas[2] * betas[3] +
                       rowL[9] * betas[3] * betas[3]);
    }
    pnp_qr_solve(A, b, x);
    for (int i = 0; i < 4; i++) betas[i] += x[i];
  }
}

/* compute_R_and_t: control points in the camera frame from the betas, the points, sign, Procrustes (3 x 3 SVD), mean
 * reprojection error. */
PNP_FN double pnp_compute_R_and_t(const double* ut, const double* betas, const double* alphas, const double* pws,
                                  const double* us, const double* Kd, double* R, double* t) {
  double ccs[4][3], pcs[18];
  for (int i = 0; i < 4; i++) ccs[i][0] = ccs[i][1] = ccs[i][2] = 0.0;
  for (int i = 0; i < 4; i++) {
    const double* v = ut + 12 * (11 - i);
    for (int j = 0; j < 4; j++)
      for (int k = 0; k < 3; k++) ccs[j][k] += betas[i] * v[3 * j + k];
  }
  for (int i = 0; i < 6; i++) {
    const double* a = alphas + 4 * i;
    for (int j = 0; j < 3; j++) pcs[3 * i + j] = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
  }
  if (pcs[2] < 0.0)
    for (int i = 0; i < 18; i++) pcs[i] = -pcs[i];   /* solve_for_sign (ccs are not used past this point) */
  double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 3; j++) {
      pc0[j] += pcs[3 * i + j];
      pw0[j] += pws[3 * i + j];
    }
  for (int j = 0; j < 3; j++) {
    pc0[j] /= 6;
    pw0[j] /= 6;
  }
  double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 6; i++) {
    const double* pc = pcs + 3 * i;
    const double* pw = pws + 3 * i;
    for (int j = 0; j < 3; j++) {
      abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - pw0[0]);
      abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1]);
      abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2]);
    }
  }
  /* cvSVD(ABt, D, U, V): U's columns are At's rows, V's columns Vt's rows; R = U V^T */
  double At[PNP_LD * PNP_LD], Vt[PNP_LD * PNP_LD], W[PNP_LD];
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) At[i * PNP_LD + k] = abt[k * 3 + i];
  pnp_jacobi_svd(At, W, Vt, 3, 3);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      R[3 * i + j] = At[0 * PNP_LD + i] * Vt[0 * PNP_LD + j] + At[1 * PNP_LD + i] * Vt[1 * PNP_LD + j] +
                     At[2 * PNP_LD + i] * Vt[2 * PNP_LD + j];
  const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] -
                     R[0] * R[5] * R[7];
  if (det < 0) {
    R[6] = -R[6];
    R[7] = -R[7];
    R[8] = -R[8];
  }
  t[0] = pc0[0] - pnp_dot3(R + 0, pw0);
  t[1] = pc0[1] - pnp_dot3(R + 3, pw0);
  t[2] = pc0[2] - pnp_dot3(R + 6, pw0);
  double sum2 = 0.0;
  for (int i = 0; i < 6; i++) {
    const double* pw = pws + 3 * i;
    double Xc = pnp_dot3(R + 0, pw) + t[0];
    double Yc = pnp_dot3(R + 3, pw) + t[1];
    double inv_Zc = 1.0 / (pnp_dot3(R + 6, pw) + t[2]);
    double ue = Kd[2] + Kd[0] * Xc * inv_Zc;
    double ve = Kd[3] + Kd[1] * Yc * inv_Zc;
    double u = us[2 * i], v = us[2 * i + 1];
    sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
  }
  return sum2 / 6;
}

/* epnp::compute_pose for six correspondences: R (row-major 3 x 3) and t. */
PNP_FN void pnp_epnp6(const float* pwf, const float* uvf, const double* K, double* R, double* t) {
  const double fu = K[0], fv = K[1], uc = K[2], vc = K[3];
  const double ifx = 1. / fu, ify = 1. / fv;
  double pws[18], us[12], alphas[24], cws[4][3];
  for (int i = 0; i < 6; i++) {
    pws[3 * i] = pwf[3 * i];
    pws[3 * i + 1] = pwf[3 * i + 1];
    pws[3 * i + 2] = pwf[3 * i + 2];
    float xn = (float)(((double)uvf[2 * i] - uc) * ifx);
    float yn = (float)(((double)uvf[2 * i + 1] - vc) * ify);
    us[2 * i] = xn * fu + uc;
    us[2 * i + 1] = yn * fv + vc;
  }
  /* choose_control_points: the centroid and the principal axes of the points */
  cws[0][0] = cws[0][1] = cws[0][2] = 0;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 3; j++) cws[0][j] += pws[3 * i + j];
  for (int j = 0; j < 3; j++) cws[0][j] /= 6;
  double pw0[18];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 3; j++) pw0[3 * i + j] = pws[3 * i + j] - cws[0][j];
  double At[PNP_LD * PNP_LD], Vt[PNP_LD * PNP_LD], W[PNP_LD];
  for (int i = 0; i < 3; i++)          /* PW0^T PW0 (cvMulTransposed, k in order), symmetric: At = its transpose = itself */
    for (int j = 0; j < 3; j++) {
      double s = 0;
      for (int k = 0; k < 6; k++) s += pw0[3 * k + i] * pw0[3 * k + j];
      At[i * PNP_LD + j] = s;
    }
  pnp_jacobi_svd(At, W, Vt, 3, 3);     /* dc = W, uct rows = At rows */
  for (int i = 1; i < 4; i++) {
    double k = sqrt(W[i - 1] / 6);
    for (int j = 0; j < 3; j++) cws[i][j] = cws[0][j] + k * At[(i - 1) * PNP_LD + j];
  }
  /* compute_barycentric_coordinates: cvInvert(CC, CV_SVD) */
  double cc[9], ci[9];
  for (int i = 0; i < 3; i++)
    for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[j][i] - cws[0][i];
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) At[i * PNP_LD + k] = cc[k * 3 + i];
  pnp_jacobi_svd(At, W, Vt, 3, 3);
  {
    double thr = (W[0] + W[1] + W[2]) * (PNP_DBL_EPS * 2);
    for (int r = 0; r < 9; r++) ci[r] = 0;
    for (int i = 0; i < 3; i++) {
      if (fabs(W[i]) <= thr) continue;
      double wi = 1. / W[i];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) ci[3 * r + c] += Vt[i * PNP_LD + r] * wi * At[i * PNP_LD + c];
    }
  }
  for (int i = 0; i < 6; i++) {
    const double* pi = pws + 3 * i;
    double* a = alphas + 4 * i;
    for (int j = 0; j < 3; j++)
      a[1 + j] = ci[3 * j] * (pi[0] - cws[0][0]) + ci[3 * j + 1] * (pi[1] - cws[0][1]) + ci[3 * j + 2] * (pi[2] - cws[0][2]);
    a[0] = 1.0f - a[1] - a[2] - a[3];
  }
  /* M (12 x 12), M^T M, its SVD; ut rows = At rows */
  double M[144];
  for (int i = 0; i < 6; i++) {
    double* M1 = M + 24 * i;
    double* M2 = M1 + 12;
    const double* as = alphas + 4 * i;
    const double u = us[2 * i], v = us[2 * i + 1];
    for (int k = 0; k < 4; k++) {
      M1[3 * k] = as[k] * fu;
      M1[3 * k + 1] = 0.0;
      M1[3 * k + 2] = as[k] * (uc - u);
      M2[3 * k] = 0.0;
      M2[3 * k + 1] = as[k] * fv;
      M2[3 * k + 2] = as[k] * (vc - v);
    }
  }
  for (int i = 0; i < 12; i++)
    for (int j = 0; j < 12; j++) {
      double s = 0;
      for (int k = 0; k < 12; k++) s += M[12 * k + i] * M[12 * k + j];
      At[i * PNP_LD + j] = s;
    }
  pnp_jacobi_svd(At, W, Vt, 12, 12);
  double ut[144];
  for (int i = 0; i < 12; i++)
    for (int k = 0; k < 12; k++) ut[12 * i + k] = At[i * PNP_LD + k];
  /* compute_L_6x10, compute_rho */
  double L[60], rho[6], dv[4][6][3];
  for (int i = 0; i < 4; i++) {
    const double* v = ut + 12 * (11 - i);
    int a = 0, b = 1;
    for (int j = 0; j < 6; j++) {
      dv[i][j][0] = v[3 * a] - v[3 * b];
      dv[i][j][1] = v[3 * a + 1] - v[3 * b + 1];
      dv[i][j][2] = v[3 * a + 2] - v[3 * b + 2];
      b++;
      if (b > 3) {
        a++;
        b = a + 1;
      }
    }
  }
  for (int i = 0; i < 6; i++) {
    double* row = L + 10 * i;
    row[0] = pnp_dot3(dv[0][i], dv[0][i]);
    row[1] = 2.0f * pnp_dot3(dv[0][i], dv[1][i]);
    row[2] = pnp_dot3(dv[1][i], dv[1][i]);
    row[3] = 2.0f * pnp_dot3(dv[0][i], dv[2][i]);
    row[4] = 2.0f * pnp_dot3(dv[1][i], dv[2][i]);
    row[5] = pnp_dot3(dv[2][i], dv[2][i]);
    row[6] = 2.0f * pnp_dot3(dv[0][i], dv[3][i]);
    row[7] = 2.0f * pnp_dot3(dv[1][i], dv[3][i]);
    row[8] = 2.0f * pnp_dot3(dv[2][i], dv[3][i]);
    row[9] = pnp_dot3(dv[3][i], dv[3][i]);
  }
  rho[0] = pnp_dist2(cws[0], cws[1]);
  rho[1] = pnp_dist2(cws[0], cws[2]);
  rho[2] = pnp_dist2(cws[0], cws[3]);
  rho[3] = pnp_dist2(cws[1], cws[2]);
  rho[4] = pnp_dist2(cws[1], cws[3]);
  rho[5] = pnp_dist2(cws[2], cws[3]);
  double Betas[4][4], rep[4], Rs[4][9], ts[4][3], Ls[30], b5[5];
  /* find_betas_approx_1: [B11 B12 B13 B14] */
  for (int i = 0; i < 6; i++) {
    Ls[4 * i] = L[10 * i];
    Ls[4 * i + 1] = L[10 * i + 1];
    Ls[4 * i + 2] = L[10 * i + 3];
    Ls[4 * i + 3] = L[10 * i + 6];
  }
  pnp_svd_solve(Ls, 6, 4, rho, b5);
  if (b5[0] < 0) {
    Betas[1][0] = sqrt(-b5[0]);
    Betas[1][1] = -b5[1] / Betas[1][0];
    Betas[1][2] = -b5[2] / Betas[1][0];
    Betas[1][3] = -b5[3] / Betas[1][0];
  } else {
    Betas[1][0] = sqrt(b5[0]);
    Betas[1][1] = b5[1] / Betas[1][0];
    Betas[1][2] = b5[2] / Betas[1][0];
    Betas[1][3] = b5[3] / Betas[1][0];
  }
  pnp_gauss_newton(L, rho, Betas[1]);
  rep[1] = pnp_compute_R_and_t(ut, Betas[1], alphas, pws, us, K, Rs[1], ts[1]);
  /* find_betas_approx_2: [B11 B12 B22] */
  for (int i = 0; i < 6; i++) {
    Ls[3 * i] = L[10 * i];
    Ls[3 * i + 1] = L[10 * i + 1];
    Ls[3 * i + 2] = L[10 * i + 2];
  }
  pnp_svd_solve(Ls, 6, 3, rho, b5);
  if (b5[0] < 0) {
    Betas[2][0] = sqrt(-b5[0]);
    Betas[2][1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
  } else {
    Betas[2][0] = sqrt(b5[0]);
    Betas[2][1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
  }
  if (b5[1] < 0) Betas[2][0] = -Betas[2][0];
  Betas[2][2] = 0.0;
  Betas[2][3] = 0.0;
  pnp_gauss_newton(L, rho, Betas[2]);
  rep[2] = pnp_compute_R_and_t(ut, Betas[2], alphas, pws, us, K, Rs[2], ts[2]);
  /* find_betas_approx_3: [B11 B12 B22 B13 B23] */
  for (int i = 0; i < 6; i++)
    for (int k = 0; k < 5; k++) Ls[5 * i + k] = L[10 * i + k];
  pnp_svd_solve(Ls, 6, 5, rho, b5);
  if (b5[0] < 0) {
    Betas[3][0] = sqrt(-b5[0]);
    Betas[3][1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
  } else {
    Betas[3][0] = sqrt(b5[0]);
    Betas[3][1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
  }
  if (b5[1] < 0) Betas[3][0] = -Betas[3][0];
  Betas[3][2] = b5[3] / Betas[3][0];
  Betas[3][3] = 0.0;
  pnp_gauss_newton(L, rho, Betas[3]);
  rep[3] = pnp_compute_R_and_t(ut, Betas[3], alphas, pws, us, K, Rs[3], ts[3]);
  int N = 1;
  if (rep[2] < rep[1]) N = 2;
  if (rep[3] < rep[N]) N = 3;
  for (int i = 0; i < 9; i++) R[i] = Rs[N][i];
  for (int i = 0; i < 3; i++) t[i] = ts[N][i];
}

/* ---- projection and the two reprojection gates ------------------------------------------------------------------------------
 * cvProjectPoints2 with zero distortion (recalled): X = R p + t left to right, z = Z ? 1 / Z : 1, u = x * z * fx + cx, in double;
 * projectPoints' float output; the residual ipoint - projpoint in float; (float)cv::norm = sqrt((double)dx * dx + (double)dy * dy).
 * RANSAC scores hypotheses with (R, t) as EPnP produced them (no Rodrigues round trip). */
PNP_FN float pnp_reproj_err(const double* R, const double* t, const float* p, const float* m, const double* K) {
  const double X = p[0], Y = p[1], Z = p[2];
  double x = R[0] * X + R[1] * Y + R[2] * Z + t[0];
  double y = R[3] * X + R[4] * Y + R[5] * Z + t[1];
  double z = R[6] * X + R[7] * Y + R[8] * Z + t[2];
  z = z != 0 ? 1. / z : 1;
  x *= z;
  y *= z;
  const float pu = (float)(x * K[0] + K[2]), pv = (float)(y * K[1] + K[3]);
  const float dx = m[0] - pu, dy = m[1] - pv;
  return (float)sqrt((double)dx * dx + (double)dy * dy);
}

/* ---- Rodrigues (cv::Rodrigues, recalled) ------------------------------------------------------------------------------------ */
/* rvec -> R and dR/dr (3 x 9: row j = dR / dr_j, R row-major). */
PNP_FN void pnp_rodrigues(const double* rv, double* R, double* dRdr) {
  double rx = rv[0], ry = rv[1], rz = rv[2];
  double theta = sqrt(rx * rx + ry * ry + rz * rz);
  if (theta < PNP_DBL_EPS) {
    for (int i = 0; i < 9; i++) R[i] = (i % 4) == 0 ? 1 : 0;
    for (int i = 0; i < 27; i++) dRdr[i] = 0;
    dRdr[5] = dRdr[15] = dRdr[19] = -1;
    dRdr[7] = dRdr[11] = dRdr[21] = 1;
    return;
  }
  double c = cos(theta), s = sin(theta), c1 = 1. - c;
  double itheta = theta ? 1. / theta : 0.;
  rx *= itheta;
  ry *= itheta;
  rz *= itheta;
  const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
  const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int k = 0; k < 9; k++) R[k] = c * I[k] + c1 * rrt[k] + s * r_x[k];
  const double drrt[27] = {rx + rx, ry, rz, ry, 0, 0, rz, 0, 0, 0, rx, 0, rx, ry + ry, rz, 0, rz, 0, 0, 0, rx, 0, 0, ry, rx, ry, rz + rz};
  const double d_r_x_[27] = {0, 0, 0, 0, 0, -1, 0, 1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 1, 0, 0, 0, 0, 0};
  for (int i = 0; i < 3; i++) {
    double ri = i == 0 ? rx : i == 1 ? ry : rz;
    double a0 = -s * ri, a1 = (s - 2 * c1 * itheta) * ri, a2 = c1 * itheta;
    double a3 = (c - s * itheta) * ri, a4 = s * itheta;
    for (int k = 0; k < 9; k++)
      dRdr[i * 9 + k] = a0 * I[k] + a1 * rrt[k] + a2 * drrt[i * 9 + k] + a3 * r_x[k] + a4 * d_r_x_[i * 9 + k];
  }
}

/* R -> rvec, without OpenCV's SVD re-orthonormalisation of R (EPnP's R is already U V^T). */
PNP_FN void pnp_rodrigues_inv(const double* R, double* rv) {
  double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
  double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
  double c = (R[0] + R[4] + R[8] - 1) * 0.5;
  c = c > 1. ? 1. : c < -1. ? -1. : c;
  double theta = acos(c);
  if (s < 1e-5) {
    if (c > 0) {
      rx = ry = rz = 0;
    } else {
      double t = (R[0] + 1) * 0.5;
      rx = sqrt(t > 0. ? t : 0.);
      t = (R[4] + 1) * 0.5;
      ry = sqrt(t > 0. ? t : 0.) * (R[1] < 0 ? -1. : 1.);
      t = (R[8] + 1) * 0.5;
      rz = sqrt(t > 0. ? t : 0.) * (R[2] < 0 ? -1. : 1.);
      if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
      theta /= sqrt(rx * rx + ry * ry + rz * rz);
      rx *= theta;
      ry *= theta;
      rz *= theta;
    }
  } else {
    double vth = 1 / (2 * s);
    vth *= theta;
    rx *= vth;
    ry *= vth;
    rz *= vth;
  }
  rv[0] = rx;
  rv[1] = ry;
  rv[2] = rz;
}

/* ---- the refine's Levenberg-Marquardt (cvFindExtrinsicCameraParams2 + CvLevMarq, recalled) ----------------------------------
 * Per point: the residual e = projection - observation (pixels, double) and its 2 x 6 Jacobian over (r, t); accumulated into
 * acc[0..20] = J^T J (upper triangle, row-major), acc[21..26] = J^T e, acc[27] = e^T e. */
#define PNP_ACC 28
PNP_FN void pnp_lm_point(const double* R, const double* dRdr, const double* t, const float* p, const float* m, const double* K,
                         int with_j, double* acc) {
  const double X = p[0], Y = p[1], Z = p[2];
  double x = R[0] * X + R[1] * Y + R[2] * Z + t[0];
  double y = R[3] * X + R[4] * Y + R[5] * Z + t[1];
  double z = R[6] * X + R[7] * Y + R[8] * Z + t[2];
  z = z != 0 ? 1. / z : 1;
  x *= z;
  y *= z;
  const double e0 = (x * K[0] + K[2]) - (double)m[0], e1 = (y * K[1] + K[3]) - (double)m[1];
  acc[27] += e0 * e0 + e1 * e1;
  if (!with_j) return;
  double J0[6], J1[6];
  for (int j = 0; j < 3; j++) {
    double dx0 = X * dRdr[j * 9] + Y * dRdr[j * 9 + 1] + Z * dRdr[j * 9 + 2];
    double dy0 = X * dRdr[j * 9 + 3] + Y * dRdr[j * 9 + 4] + Z * dRdr[j * 9 + 5];
    double dz0 = X * dRdr[j * 9 + 6] + Y * dRdr[j * 9 + 7] + Z * dRdr[j * 9 + 8];
    J0[j] = K[0] * (z * (dx0 - x * dz0));
    J1[j] = K[1] * (z * (dy0 - y * dz0));
  }
  J0[3] = K[0] * z;
  J0[4] = 0;
  J0[5] = K[0] * (-x * z);
  J1[3] = 0;
  J1[4] = K[1] * z;
  J1[5] = K[1] * (-y * z);
  int q = 0;
  for (int a = 0; a < 6; a++)
    for (int b = a; b < 6; b++) acc[q++] += J0[a] * J0[b] + J1[a] * J1[b];
  for (int a = 0; a < 6; a++) acc[21 + a] += J0[a] * e0 + J1[a] * e1;
}

/* CvLevMarq::step: JtJ's diagonal times (1 + lambda), solve by SVD, param = prev - delta. */
PNP_FN void pnp_lm_step(const double* acc, double lambda, const double* prev, double* param) {
  double A[36], x[6];
  int q = 0;
  for (int a = 0; a < 6; a++)
    for (int b = a; b < 6; b++) {
      A[a * 6 + b] = acc[q];
      A[b * 6 + a] = acc[q];
      q++;
    }
  for (int a = 0; a < 6; a++) A[a * 7] *= 1. + lambda;
  pnp_svd_solve(A, 6, 6, acc + 21, x);
  for (int a = 0; a < 6; a++) param[a] = prev[a] - x[a];
}

/* cvNorm(param, prevParam, CV_RELATIVE_L2) < FLT_EPSILON */
PNP_FN int pnp_lm_converged(const double* param, const double* prev) {
  double d = 0, p = 0;
  for (int a = 0; a < 6; a++) {
    d += (param[a] - prev[a]) * (param[a] - prev[a]);
    p += prev[a] * prev[a];
  }
  return sqrt(d) / (sqrt(p) + PNP_DBL_EPS) < PNP_FLT_EPS;
}

/* calcVariance (MotionEstimation.cpp:14-36), float, in order. */
PNP_FN float pnp_variance(const float* v, int n) {
  float mean = 0;
  if (n) {
    for (int i = 0; i < n; i++) mean += v[i];
    mean /= n;
  }
  float var = 0;
  if (n > 1) {
    float sum = 0;
    for (int i = 0; i < n; i++) sum += (v[i] - mean) * (v[i] - mean);
    var = sum / (n - 1);
  }
  return var;
}

/* ---- the reference's float Transform (Transform.cpp, Eigen; recalled, not pinned) ------------------------------------------ */
/* C = A * B as 4 x 4 floats, then the rotation through Eigen::Quaternionf(...).normalized().toRotationMatrix(). */
PNP_FN void pnp_tf_mul(const float* A, const float* B, float* C) {
  float m[12];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) m[4 * i + j] = A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j] + A[4 * i + 2] * B[8 + j] + (j == 3 ? A[4 * i + 3] : 0.0f);
  float q[4];   /* w, x, y, z */
  float tr = m[0] + m[5] + m[10];
  if (tr > 0.0f) {
    float t = sqrtf(tr + 1.0f);
    q[0] = 0.5f * t;
    t = 0.5f / t;
    q[1] = (m[9] - m[6]) * t;
    q[2] = (m[2] - m[8]) * t;
    q[3] = (m[4] - m[1]) * t;
  } else {
    int i = 0;
    if (m[5] > m[0]) i = 1;
    if (m[10] > m[4 * i + i]) i = 2;
    int j = (i + 1) % 3, k = (j + 1) % 3;
    float t = sqrtf(m[4 * i + i] - m[4 * j + j] - m[4 * k + k] + 1.0f);
    q[1 + i] = 0.5f * t;
    t = 0.5f / t;
    q[0] = (m[4 * k + j] - m[4 * j + k]) * t;
    q[1 + j] = (m[4 * j + i] + m[4 * i + j]) * t;
    q[1 + k] = (m[4 * k + i] + m[4 * i + k]) * t;
  }
  float n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (n2 > 0.0f) {
    float n = sqrtf(n2);
    for (int i = 0; i < 4; i++) q[i] = q[i] / n;
  }
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y,
              tzz = tz * z;
  C[0] = 1.0f - (tyy + tzz);
  C[1] = txy - twz;
  C[2] = txz + twy;
  C[4] = txy + twz;
  C[5] = 1.0f - (txx + tzz);
  C[6] = tyz - twx;
  C[8] = txz - twy;
  C[9] = tyz + twx;
  C[10] = 1.0f - (txx + tyy);
  C[3] = m[3];
  C[7] = m[7];
  C[11] = m[11];
}

/* The 4 x 4 inverse of [A; 0 0 0 1] by cofactors, in float. */
PNP_FN void pnp_tf_inverse(const float* A, float* C) {
  const float a = A[0], b = A[1], c = A[2], d = A[3], e = A[4], f = A[5], g = A[6], h = A[7], i = A[8], j = A[9], k = A[10],
              l = A[11];
  const float c00 = f * k - g * j, c01 = g * i - e * k, c02 = e * j - f * i;
  const float det = a * c00 + b * c01 + c * c02;
  const float id = 1.0f / det;
  float R[9];
  R[0] = c00 * id;
  R[1] = (c * j - b * k) * id;
  R[2] = (b * g - c * f) * id;
  R[3] = c01 * id;
  R[4] = (a * k - c * i) * id;
  R[5] = (c * e - a * g) * id;
  R[6] = c02 * id;
  R[7] = (b * i - a * j) * id;
  R[8] = (a * f - b * e) * id;
  for (int r = 0; r < 3; r++) {
    C[4 * r] = R[3 * r];
    C[4 * r + 1] = R[3 * r + 1];
    C[4 * r + 2] = R[3 * r + 2];
    C[4 * r + 3] = -(R[3 * r] * d + R[3 * r + 1] * h + R[3 * r + 2] * l);
  }
}

/* transform = (localTransform * pnp).inverse(); local NULL = no localTransform (the product is skipped). */
PNP_FN void pnp_transform(const double* R, const double* t, const float* local, float* out) {
  float pnp[12];
  for (int r = 0; r < 3; r++) {
    pnp[4 * r] = (float)R[3 * r];
    pnp[4 * r + 1] = (float)R[3 * r + 1];
    pnp[4 * r + 2] = (float)R[3 * r + 2];
    pnp[4 * r + 3] = (float)t[r];
  }
  if (local) {
    float lp[12];
    pnp_tf_mul(local, pnp, lp);
    pnp_tf_inverse(lp, out);
  } else {
    pnp_tf_inverse(pnp, out);
  }
}

/* Covariance terms of one inlier (MotionEstimation.cpp:165-187): obj the from-point, to the to-frame's 3-D point (finite). */
PNP_FN void pnp_cov_terms(const float* obj, const float* to, const float* T, float* dist, float* ang) {
  float nx = T[0] * to[0] + T[1] * to[1] + T[2] * to[2] + T[3];
  float ny = T[4] * to[0] + T[5] * to[1] + T[6] * to[2] + T[7];
  float nz = T[8] * to[0] + T[9] * to[1] + T[10] * to[2] + T[11];
  float dx = obj[0] - nx, dy = obj[1] - ny, dz = obj[2] - nz;
  *dist = dx * dx + dy * dy + dz * dz;
  float v1[3] = {obj[0] - T[3], obj[1] - T[7], obj[2] - T[11]}, v2[3] = {nx - T[3], ny - T[7], nz - T[11]};
  float n1 = v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2], n2 = v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2];
  if (n1 > 0.0f) {
    float s = sqrtf(n1);
    v1[0] = v1[0] / s;
    v1[1] = v1[1] / s;
    v1[2] = v1[2] / s;
  }
  if (n2 > 0.0f) {
    float s = sqrtf(n2);
    v2[0] = v2[0] / s;
    v2[1] = v2[1] / s;
    v2[2] = v2[2] / s;
  }
  double rad = (double)(v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]);
  rad = rad < -1.0 ? -1.0 : rad > 1.0 ? 1.0 : rad;
  *ang = (float)acos(rad);
}

PNP_FN int pnp_finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

#endif /* SBM_PNP_MATH_H_ */
