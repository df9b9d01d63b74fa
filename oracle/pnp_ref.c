/* pnp_ref.c -- the sequential CPU restatement of estimateMotion3DTo2D (include/sbm.h, "motion estimation"). TEST
 * INFRASTRUCTURE ONLY; built with -O2 -ffp-contract=off (oracle/Makefile).
 *
 * The arithmetic comes from u96-slam_amd/csrc/sbm_pnp_math.h, the same file the kernels compile. What this file restates is the
 * control flow of the reference in its own order: gather, then the RANSAC loop with draw, solve, score and update interleaved
 * (CvSolvePnP.cpp:326-419), the refine loop with its swap pair (MotionEstimation.cpp:291-373), and the result
 * (MotionEstimation.cpp:120-241). The kernels restate the same loop as all-solve / all-score / replay; pnp_ref.py holds this file
 * to the reference's loops. The refine's sums run in PNP_LANES strided partials, summed in lane order, as the kernel's
 * wavefront reduction does. */
#include <stdlib.h>
#include <string.h>

#include "../include/sbm.h"
#include "../u96-slam_amd/csrc/sbm_pnp_math.h"

/* CvLevMarq's lambda = exp(lambdaLg10 * log(10)), lambdaLg10 in -16..16: computed on the host, passed to the kernels. */
void pnp_ref_lambda_table(double* tab) {
  const double LOG10 = log(10.);
  for (int k = -16; k <= 16; k++) tab[k + 16] = exp(k * LOG10);
}

int pnp_ref_update_num_iters(double p, double ep, int model_points, int max_iters) {
  return pnp_update_num_iters(p, ep, model_points, max_iters);
}

/* The subsets the RANSAC loop of a job with n points draws, for `iterations` iterations: 6 * iterations ints. */
void pnp_ref_draw(int n, int iterations, int* out) {
  uint64_t s = (uint64_t)-1;
  for (int i = 0; i < iterations; i++) pnp_draw_subset(&s, n, out + 6 * i);
}

void pnp_ref_epnp6(const float* pw, const float* uv, const double* K, double* R, double* t) { pnp_epnp6(pw, uv, K, R, t); }

void pnp_ref_rodrigues(const double* rv, double* R) {
  double d[27];
  pnp_rodrigues(rv, R, d);
}

void pnp_ref_rodrigues_inv(const double* R, double* rv) { pnp_rodrigues_inv(R, rv); }

/* The header's blocks one by one, for tests that hold them to an independent statement (tests/pnp_independent.py). The
 * matrices of the SVD are the header's own: rows of stride PNP_LD. */
int pnp_ref_ld(void) { return PNP_LD; }
void pnp_ref_jacobi_svd(double* At, double* W, double* Vt, int m, int n) { pnp_jacobi_svd(At, W, Vt, m, n); }
void pnp_ref_svd_solve(const double* A, int m, int n, const double* b, double* x) { pnp_svd_solve(A, m, n, b, x); }
void pnp_ref_qr_solve(double* A, double* b, double* X) { pnp_qr_solve(A, b, X); }
void pnp_ref_rodrigues_d(const double* rv, double* R, double* dRdr) { pnp_rodrigues(rv, R, dRdr); }
void pnp_ref_lm_points(const double* R, const double* dRdr, const double* t, const float* p, const float* m, int n, const double* K,
                       int with_j, double* acc) {
  for (int i = 0; i < n; i++) pnp_lm_point(R, dRdr, t, p + 3 * i, m + 2 * i, K, with_j, acc);
}
void pnp_ref_lm_step(const double* acc, double lambda, const double* prev, double* param) { pnp_lm_step(acc, lambda, prev, param); }
int pnp_ref_lm_converged(const double* param, const double* prev) { return pnp_lm_converged(param, prev); }
float pnp_ref_reproj_err(const double* R, const double* t, const float* p, const float* m, const double* K) {
  return pnp_reproj_err(R, t, p, m, K);
}
float pnp_ref_variance(const float* v, int n) { return pnp_variance(v, n); }
void pnp_ref_tf_mul(const float* A, const float* B, float* C) { pnp_tf_mul(A, B, C); }
void pnp_ref_tf_inverse(const float* A, float* C) { pnp_tf_inverse(A, C); }
void pnp_ref_transform(const double* R, const double* t, const float* local, float* out) { pnp_transform(R, t, local, out); }
void pnp_ref_cov_terms(const float* obj, const float* to, const float* T, float* dist, float* ang) {
  pnp_cov_terms(obj, to, T, dist, ang);
}

/* The RANSAC loop over given counts (what findInliers would return per iteration): best iteration, final niters, best count. */
void pnp_ref_replay(const int* counts, int iterations, int n, double confidence, int* best, int* niters_out, int* maxgood) {
  int niters = iterations > 1 ? iterations : 1, good = 0, b = -1;
  for (int iter = 0; iter < niters; iter++) {
    const int c = counts[iter];
    if (c > (good > 5 ? good : 5)) {
      b = iter;
      good = c;
      niters = pnp_update_num_iters(confidence, (double)(n - c) / n, 6, niters);
    }
  }
  *best = b;
  *niters_out = niters;
  *maxgood = good;
}

typedef struct Job {
  const float* xyz;   /* compacted object points, N * 3 */
  const float* uv;    /* compacted image points, N * 2  */
  int n;
  const double* K;
  const double* lam;
  double rv[3], tv[3];
} Job;

/* cv::solvePnP(ITERATIVE, useExtrinsicGuess = true) on the points `set` (len of them), from and into (rv, tv). */
static void lm_refine(Job* jb, const int* set, int len) {
  double param[6] = {jb->rv[0], jb->rv[1], jb->rv[2], jb->tv[0], jb->tv[1], jb->tv[2]}, prev[6], acc[PNP_ACC];
  double part[PNP_LANES][PNP_ACC];
  int lg = -3, iters = 0;
#define LM_EVAL(with_j)                                                                                  \
  do {                                                                                                   \
    double R[9], dR[27];                                                                                 \
    pnp_rodrigues(param, R, dR);                                                                         \
    memset(part, 0, sizeof(part));                                                                       \
    for (int s = 0; s < PNP_LANES; s++)                                                                  \
      for (int i = s; i < len; i += PNP_LANES)                                                           \
        pnp_lm_point(R, dR, param + 3, jb->xyz + 3 * set[i], jb->uv + 2 * set[i], jb->K, with_j, part[s]); \
    memset(acc, 0, sizeof(acc));                                                                         \
    for (int s = 0; s < PNP_LANES; s++)                                                                  \
      for (int q = 0; q < PNP_ACC; q++) acc[q] += part[s][q];                                            \
  } while (0)
  LM_EVAL(1);
  double JtJ[PNP_ACC];
  memcpy(JtJ, acc, sizeof(acc));
  double prev_norm = sqrt(acc[27]);
  for (;;) {
    memcpy(prev, param, sizeof(prev));
    pnp_lm_step(JtJ, jb->lam[lg + 16], prev, param);
    double err_norm;
    for (;;) {
      LM_EVAL(0);
      err_norm = sqrt(acc[27]);
      if (err_norm > prev_norm && ++lg <= 16) {
        pnp_lm_step(JtJ, jb->lam[lg + 16], prev, param);
        continue;
      }
      break;
    }
    lg = lg - 1 > -16 ? lg - 1 : -16;
    if (++iters >= 20 || pnp_lm_converged(param, prev)) break;
    prev_norm = err_norm;
    LM_EVAL(1);
    memcpy(JtJ, acc, sizeof(acc));
  }
#undef LM_EVAL
  for (int a = 0; a < 3; a++) {
    jb->rv[a] = param[a];
    jb->tv[a] = param[3 + a];
  }
}

/* computeReprojErrors over all N points at (rv, tv): the set and its errors; returns its length. *margin keeps the least
 * |e - thr| seen, the distance of the closest point to the gate of this round. */
static int reproject(const Job* jb, float thr, int* set, float* err, double* margin) {
  double R[9], dR[27];
  pnp_rodrigues(jb->rv, R, dR);
  int k = 0;
  for (int i = 0; i < jb->n; i++) {
    float e = pnp_reproj_err(R, jb->tv, jb->xyz + 3 * i, jb->uv + 2 * i, jb->K);
    const double d = fabs((double)e - (double)thr);
    if (d < *margin) *margin = d;
    if (e <= thr) {
      set[k] = i;
      err[k] = e;
      k++;
    }
  }
  return k;
}

/* The refine loop's control flow (MotionEstimation.cpp:291-373) over a step that solves on `prev` and produces `next`:
 * returns the final list's length (in *out), the solves run and the exit (0 normal, 1 too few, 2 unchanged). */
typedef int (*refine_step_fn)(void* ctx, const int* prev, int prev_len, int round, int* next);

static int refine_loop(void* ctx, refine_step_fn step, const int* ransac, int ransac_len, int rounds, int min_inliers, int cap,
                       int* out, int* solves, int* exit_code) {
  int* prev = (int*)malloc(sizeof(int) * (cap + 1));
  int* next = (int*)malloc(sizeof(int) * (cap + 1));
  memcpy(prev, ransac, sizeof(int) * ransac_len);
  int prev_len = ransac_len, next_len = 0, count = 0;
  *exit_code = 0;
  *solves = 0;
  while (count < rounds) {
    next_len = step(ctx, prev, prev_len, count, next);
    (*solves)++;
    if (next_len < min_inliers) {
      *exit_code = 1;
      break;
    }
    if (next_len == prev_len && !memcmp(next, prev, sizeof(int) * next_len)) {
      *exit_code = 2;
      break;
    }
    int* t = next;   /* std::swap(new_inliers, prev_inliers) */
    next = prev;
    prev = t;
    int tl = next_len;
    next_len = prev_len;
    prev_len = tl;
    count++;
  }
  /* std::swap(new_inliers, inliers): on a normal exit `next` holds the set the last solve ran on */
  memcpy(out, next, sizeof(int) * next_len);
  free(prev);
  free(next);
  return next_len;
}

/* A refine walk over scripted outcomes: round r produces sets[r] (lengths lens[r], rows of stride cap). */
typedef struct Script {
  const int* sets;
  const int* lens;
  int cap;
} Script;

static int script_step(void* ctx, const int* prev, int prev_len, int round, int* next) {
  (void)prev;
  (void)prev_len;
  const Script* s = (const Script*)ctx;
  memcpy(next, s->sets + (size_t)round * s->cap, sizeof(int) * s->lens[round]);
  return s->lens[round];
}

int pnp_ref_refine_walk(const int* ransac, int ransac_len, const int* sets, const int* lens, int cap, int rounds, int min_inliers,
                        int* out, int* solves, int* exit_code) {
  Script s = {sets, lens, cap};
  return refine_loop(&s, script_step, ransac, ransac_len, rounds, min_inliers, cap, out, solves, exit_code);
}

typedef struct RealStep {
  Job* jb;
  float thr, reproj, sigma;
  float* err;
  double margin;
} RealStep;

static int real_step(void* ctx, const int* prev, int prev_len, int round, int* next) {
  (void)round;
  RealStep* r = (RealStep*)ctx;
  lm_refine(r->jb, prev, prev_len);
  int k = reproject(r->jb, r->thr, next, r->err, &r->margin);
  float var = pnp_variance(r->err, k);
  float s = r->sigma * (float)sqrt(var);
  r->thr = r->reproj < s ? r->reproj : s;
  return k;
}

/* One job. Returns the status; res, inliers (up to npairs from-indices), and optionally the compacted points (cxyz N * 3,
 * cuv N * 2, cmatch N), the RANSAC inliers (ransac, up to N; *nransac), every hypothesis (hyp: iterations records; solving
 * the ones the loop never reaches is extra work, so without hyp only the reference's own work is done) and the least distance
 * of any point's refine residual to the threshold of its round (gate_margin; +inf when no refine ran). */
int pnp_ref_estimate(const float* xyz_from, int nf, const float* kpts_to, const float* xyz_to, int nt, const int* pairs, int npairs,
                     const double* K, const float* local, const sbm_pnp_params* p, sbm_pnp_result* res, int* inliers, float* cxyz,
                     float* cuv, int* cmatch, int* ransac, int* nransac, sbm_pnp_hypothesis* hyp, double* gate_margin) {
  const int cap = npairs > 0 ? npairs : 1;
  float* X = (float*)malloc(sizeof(float) * 3 * cap);
  float* U = (float*)malloc(sizeof(float) * 2 * cap);
  int* mt = (int*)malloc(sizeof(int) * cap);
  int* tt = (int*)malloc(sizeof(int) * cap);
  int* best_set = (int*)malloc(sizeof(int) * (cap + 1));
  int* cur = (int*)malloc(sizeof(int) * (cap + 1));
  float* err = (float*)malloc(sizeof(float) * (cap + 1));
  double lam[33];
  pnp_ref_lambda_table(lam);
  memset(res, 0, sizeof(*res));
  res->best_iteration = -1;
  res->refine_exit = -1;
  res->cov_dist = res->cov_angle = 1.0;
  if (gate_margin) *gate_margin = INFINITY;
  /* gather */
  int N = 0;
  for (int i = 0; i < npairs; i++) {
    const int f = pairs[2 * i], t = pairs[2 * i + 1];
    if (f < 0 || f >= nf || t < 0 || t >= nt) continue;
    if (!pnp_finite3(xyz_from + 3 * f)) continue;
    memcpy(X + 3 * N, xyz_from + 3 * f, 12);
    memcpy(U + 2 * N, kpts_to + 2 * t, 8);
    mt[N] = f;
    tt[N] = t;
    N++;
  }
  res->num_matches = N;
  if (cxyz) memcpy(cxyz, X, sizeof(float) * 3 * N);
  if (cuv) memcpy(cuv, U, sizeof(float) * 2 * N);
  if (cmatch) memcpy(cmatch, mt, sizeof(int) * N);
  if (hyp)
    for (int i = 0; i < p->iterations; i++) {
      memset(&hyp[i], 0, sizeof(hyp[i]));
      for (int k = 0; k < 6; k++) hyp[i].subset[k] = -1;
      hyp[i].count = -1;
    }
  int nin = 0;
  if (nransac) *nransac = 0;
  if (N < p->min_inliers) {
    res->status = SBM_PNP_FEW_MATCHES;
    goto done;
  }
  /* RANSAC */
  double bR[9], bt[3];
  int good = 0;
  if (N == 6) {
    const int all[6] = {0, 1, 2, 3, 4, 5};
    pnp_epnp6(X, U, K, bR, bt);
    good = 6;
    res->best_iteration = 0;
    res->niters = 1;
    for (int i = 0; i < 6; i++) best_set[i] = i;
    if (hyp) {
      memcpy(hyp[0].subset, all, sizeof(all));
      hyp[0].count = 6;
      memcpy(hyp[0].R, bR, sizeof(bR));
      memcpy(hyp[0].t, bt, sizeof(bt));
    }
  } else {
    const float gate = (float)((double)p->reprojection_error * p->reprojection_error);
    uint64_t rng = (uint64_t)-1;
    int niters = p->iterations > 1 ? p->iterations : 1;
    for (int iter = 0; iter < niters; iter++) {
      int idx[6];
      float sx[18], su[12];
      double R[9], t[3];
      pnp_draw_subset(&rng, N, idx);
      for (int k = 0; k < 6; k++) {
        memcpy(sx + 3 * k, X + 3 * idx[k], 12);
        memcpy(su + 2 * k, U + 2 * idx[k], 8);
      }
      pnp_epnp6(sx, su, K, R, t);
      int c = 0;
      for (int i = 0; i < N; i++) {
        int f = pnp_reproj_err(R, t, X + 3 * i, U + 2 * i, K) <= gate;
        if (f) cur[c] = i;
        c += f;
      }
      if (hyp) {
        memcpy(hyp[iter].subset, idx, sizeof(idx));
        hyp[iter].count = c;
        memcpy(hyp[iter].R, R, sizeof(R));
        memcpy(hyp[iter].t, t, sizeof(t));
      }
      if (c > (good > 5 ? good : 5)) {
        memcpy(best_set, cur, sizeof(int) * c);
        memcpy(bR, R, sizeof(R));
        memcpy(bt, t, sizeof(t));
        good = c;
        res->best_iteration = iter;
        niters = pnp_update_num_iters(p->confidence, (double)(N - good) / N, 6, niters);
      }
    }
    res->niters = niters;
    if (hyp) /* every hypothesis, including those the loop did not reach */
      for (int iter = 0; iter < p->iterations; iter++) {
        if (hyp[iter].count >= 0) continue;
        /* the draws continue the same sequence: redraw from the start */
        uint64_t s2 = (uint64_t)-1;
        int idx[6];
        for (int r = 0; r <= iter; r++) pnp_draw_subset(&s2, N, idx);
        float sx[18], su[12];
        for (int k = 0; k < 6; k++) {
          memcpy(sx + 3 * k, X + 3 * idx[k], 12);
          memcpy(su + 2 * k, U + 2 * idx[k], 8);
        }
        pnp_epnp6(sx, su, K, hyp[iter].R, hyp[iter].t);
        memcpy(hyp[iter].subset, idx, sizeof(idx));
        int c = 0;
        for (int i = 0; i < N; i++) c += pnp_reproj_err(hyp[iter].R, hyp[iter].t, X + 3 * i, U + 2 * i, K) <= gate;
        hyp[iter].count = c;
      }
  }
  res->ransac_inliers = good;
  if (good <= 0) {
    res->status = SBM_PNP_NO_MODEL;
    goto done;
  }
  if (ransac) memcpy(ransac, best_set, sizeof(int) * good);
  if (nransac) *nransac = good;
  Job jb = {X, U, N, K, lam, {0, 0, 0}, {bt[0], bt[1], bt[2]}};
  pnp_rodrigues_inv(bR, jb.rv);
  memcpy(cur, best_set, sizeof(int) * good);
  nin = good;
  if (nin >= p->min_inliers && p->refine_iterations > 0) {
    RealStep rs = {&jb, p->reprojection_error, p->reprojection_error, p->refine_sigma, err, INFINITY};
    nin = refine_loop(&rs, real_step, best_set, good, p->refine_iterations, p->min_inliers, N, cur, &res->refine_solves,
                      &res->refine_exit);
    if (gate_margin) *gate_margin = rs.margin;
  }
  double R[9], dR[27];
  pnp_rodrigues(jb.rv, R, dR);
  memcpy(res->rvec, jb.rv, sizeof(jb.rv));
  memcpy(res->tvec, jb.tv, sizeof(jb.tv));
  memcpy(res->R, R, sizeof(R));
  if (nin < p->min_inliers) {
    res->status = res->refine_exit < 0 ? SBM_PNP_FEW_RANSAC_INLIERS : SBM_PNP_FEW_REFINED_INLIERS;
  } else {
    res->status = SBM_PNP_OK;
    pnp_transform(R, jb.tv, local, res->transform);
    float* d = (float*)malloc(sizeof(float) * (nin + 1));
    float* a = (float*)malloc(sizeof(float) * (nin + 1));
    int nv = 0;
    for (int i = 0; i < nin; i++) {
      const float* to = xyz_to + 3 * tt[cur[i]];
      if (!pnp_finite3(to)) continue;
      pnp_cov_terms(X + 3 * cur[i], to, res->transform, d + nv, a + nv);
      nv++;
    }
    if (nv) {   /* the median: element nv >> 1 in sorted order */
      int k = nv >> 1;
      float md = 0, ma = 0;
      for (int i = 0; i < nv; i++) {
        int lt = 0, eq = 0, lt2 = 0, eq2 = 0;
        for (int j = 0; j < nv; j++) {
          lt += d[j] < d[i];
          eq += d[j] == d[i] && j < i;
          lt2 += a[j] < a[i];
          eq2 += a[j] == a[i] && j < i;
        }
        if (lt + eq == k) md = d[i];
        if (lt2 + eq2 == k) ma = a[i];
      }
      res->cov_dist = md < 0.0001 ? 0.0001 : (double)md;
      res->cov_angle = ma < 0.0001 ? 0.0001 : (double)ma;
    }
    free(d);
    free(a);
  }
done:
  res->num_inliers = nin;
  for (int i = 0; i < nin; i++) inliers[i] = mt[cur[i]];
  free(X);
  free(U);
  free(mt);
  free(tt);
  free(best_set);
  free(cur);
  free(err);
  return res->status;
}
