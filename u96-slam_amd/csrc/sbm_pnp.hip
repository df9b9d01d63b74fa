// Motion estimation of the reference's computeTransform (src/slam/src/core/Registration.cpp:337-397): estimateMotion3DTo2D's
// gather, cv3::solvePnPRansac's RANSAC over six-point EPnP hypotheses, the solvePnP(ITERATIVE) refine loop and the result
// (transform, covariance scales). DESIGN.md section 12; the semantics and the parity contract are in include/sbm.h.
//
// The subsets a job draws depend on N alone, so the sequential RANSAC loop is restated exactly as
//   gather   one wavefront per job: the finite pairs compacted in order (ballot + prefix); lane 0 then runs the RNG and writes
//            `iterations` six-index subsets.
//   hyp      one lane per (job, iteration): EPnP in double (sbm_pnp_math.h, shared with the CPU restatement), R and t to scratch.
//   score    one wavefront per (job, iteration): the inlier count over the job's N points (double projection, float residual,
//            norm <= reprojection_error^2), lanes strided over the points, ballot counts.
//   finish   one wavefront per job: the replay of the RANSAC loop over the counts (best iteration, niters), the RANSAC inlier
//            set, the refine rounds (Levenberg-Marquardt with J^T J / J^T e reduced over the lanes through LDS in a fixed order,
//            the reprojection gate, the variance and the swap rule), the float transform and the covariance medians (rank
//            selection over the lanes).
// Contraction is off in this file (and in sbm_pnp_math.h): every a * b + c stays a multiply and an add, as on the host.
#include <algorithm>
#include <cmath>

#include "sbm_handle.h"
#include "sbm_pnp_math.h"

#pragma clang fp contract(off)

namespace sbm {
namespace {

constexpr int kArgJobs = 64;                          // jobs per launch sequence: their (from, to) travel as a kernel argument
constexpr size_t kScratchBudget = (size_t)256 << 20;  // one launch's scratch
constexpr int kWave = 64;

struct PnpJobs {
  int2 j[kArgJobs];
};

struct PnpArgs {
  double K[4];
  double lam[33];      // CvLevMarq's lambda for lambdaLg10 = -16..16, computed on the host
  float local[12];
  int has_local;
  int min_inliers, refine_iterations, iterations;
  float gate, reproj, sigma;
  double confidence;
};

// One job's slice of the launch scratch; slice_layout has the sizes.
struct Slice {
  float *X, *U;           // compacted object and image points
  int *mt, *tt;           // from- and to-indices (the reference's matches)
  int *sub, *cnt;         // per iteration: the subset and the count,
  double* hR;             // and (R, t)
  int *setA, *setB;       // refine lists
  float *err, *cd, *ca;
  int* n;
};

// The slice's layout: sized by its counting pass, placed by the same statements (host and kernels alike).
__host__ __device__ inline Slice slice_layout(Carve& c, int cap, int iters) {
  const size_t n = (size_t)cap, n1 = n + 1, it = (size_t)iters;
  Slice s;
  s.X = c.take<float>(n * 3);   // n = cap points, n1 = cap + 1
  s.U = c.take<float>(n * 2);
  s.mt = c.take<int>(n);
  s.tt = c.take<int>(n);
  s.sub = c.take<int>(it * 6);
  s.hR = c.take<double>(it * 12);   // (R, t)
  s.cnt = c.take<int>(it);
  s.setA = c.take<int>(n1);
  s.setB = c.take<int>(n1);
  s.err = c.take<float>(n1);
  s.cd = c.take<float>(n1);
  s.ca = c.take<float>(n1);
  s.n = c.take<int>(4);
  return s;
}
__host__ __device__ inline size_t slice_bytes(int cap, int iters) { return carve_bytes([&](Carve& c) { slice_layout(c, cap, iters); }); }
__host__ __device__ inline Slice slice_at(char* base, int job, int cap, int iters) {
  __builtin_assume(base != nullptr);   // the launch scratch: a kernel's thirteen pointers need no null test
  Carve place{base + (size_t)job * slice_bytes(cap, iters)};
  return slice_layout(place, cap, iters);
}

__device__ __forceinline__ int clamp_count(int c, int cap) { return min(max(c, 0), cap); }
__device__ __forceinline__ int prefix(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

__global__ void __launch_bounds__(64) pnp_gather_kernel(const float* __restrict__ xyz, const float* __restrict__ kpts,
                                                        const int* __restrict__ count, const int2* __restrict__ pairs,
                                                        const int* __restrict__ npairs, int cap, int j0, PnpJobs jobs, int iters,
                                                        int min_inliers, char* scratch) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x, job = blockIdx.x;
  Slice s = slice_at(scratch, job, cap, iters);
  const int F = jobs.j[job].x, T = jobs.j[job].y;
  const int nf = clamp_count(count[F], cap), nt = clamp_count(count[T], cap), np = clamp_count(npairs[j0 + job], cap);
  const int2* pr = pairs + (size_t)(j0 + job) * cap;
  int base = 0;
  for (int c = 0; c < np; c += kWave) {
    const int i = c + lane;
    bool keep = false;
    int f = 0, t = 0;
    const float* p = nullptr;
    if (i < np) {
      const int2 q = pr[i];
      f = q.x;
      t = q.y;
      if (f >= 0 && f < nf && t >= 0 && t < nt) {
        p = xyz + ((size_t)F * cap + f) * 3;
        keep = pnp_finite3(p);
      }
    }
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int o = base + prefix(m, lane);
      s.X[3 * o] = p[0];
      s.X[3 * o + 1] = p[1];
      s.X[3 * o + 2] = p[2];
      const float* k = kpts + ((size_t)T * cap + t) * 2;
      s.U[2 * o] = k[0];
      s.U[2 * o + 1] = k[1];
      s.mt[o] = f;
      s.tt[o] = t;
    }
    base += __popcll(m);
  }
  if (lane == 0) {
    s.n[0] = base;
    if (base >= min_inliers && base > 6) {
      uint64_t st = (uint64_t)-1;
      for (int i = 0; i < iters; i++) pnp_draw_subset(&st, base, s.sub + 6 * i);
    }
  }
}

__global__ void __launch_bounds__(64) pnp_hyp_kernel(int cap, int j0, int iters, int min_inliers, PnpArgs a, char* scratch,
                                                     sbm_pnp_hypothesis* __restrict__ hyp) {
#pragma clang fp contract(off)
  const int job = blockIdx.y, it = blockIdx.x * kWave + threadIdx.x;
  if (it >= iters) return;
  Slice s = slice_at(scratch, job, cap, iters);
  const int N = s.n[0];
  sbm_pnp_hypothesis* rec = hyp ? hyp + (size_t)(j0 + job) * iters + it : nullptr;
  if (N < min_inliers || (N == 6 && it > 0)) {
    if (rec) {
      for (int k = 0; k < 6; k++) rec->subset[k] = -1;
      rec->count = -1;
      rec->pad = 0;
      for (int k = 0; k < 9; k++) rec->R[k] = 0;
      for (int k = 0; k < 3; k++) rec->t[k] = 0;
    }
    return;
  }
  int idx[6];
  for (int k = 0; k < 6; k++) idx[k] = N == 6 ? k : s.sub[6 * it + k];
  float sx[18], su[12];
  for (int k = 0; k < 6; k++) {
    sx[3 * k] = s.X[3 * idx[k]];
    sx[3 * k + 1] = s.X[3 * idx[k] + 1];
    sx[3 * k + 2] = s.X[3 * idx[k] + 2];
    su[2 * k] = s.U[2 * idx[k]];
    su[2 * k + 1] = s.U[2 * idx[k] + 1];
  }
  double R[9], t[3];
  pnp_epnp6(sx, su, a.K, R, t);
  double* o = s.hR + 12 * it;
  for (int k = 0; k < 9; k++) o[k] = R[k];
  for (int k = 0; k < 3; k++) o[9 + k] = t[k];
  if (rec) {
    for (int k = 0; k < 6; k++) rec->subset[k] = idx[k];
    rec->pad = 0;
    for (int k = 0; k < 9; k++) rec->R[k] = R[k];
    for (int k = 0; k < 3; k++) rec->t[k] = t[k];
  }
}

__global__ void __launch_bounds__(256) pnp_score_kernel(int cap, int j0, int iters, int min_inliers, PnpArgs a, char* scratch,
                                                        sbm_pnp_hypothesis* __restrict__ hyp) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & (kWave - 1), job = blockIdx.y, it = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (it >= iters) return;   // uniform over the wavefront
  Slice s = slice_at(scratch, job, cap, iters);
  const int N = s.n[0];
  if (N < min_inliers || (N == 6 && it > 0)) return;
  int c = 6;   // N == 6: every point is an inlier, nothing is scored
  if (N > 6) {
    double R[9], t[3];
    for (int k = 0; k < 9; k++) R[k] = s.hR[12 * it + k];
    for (int k = 0; k < 3; k++) t[k] = s.hR[12 * it + 9 + k];
    c = 0;
    for (int b = 0; b < N; b += kWave) {
      const int i = b + lane;
      const bool in = i < N && pnp_reproj_err(R, t, s.X + 3 * i, s.U + 2 * i, a.K) <= a.gate;
      c += __popcll(__ballot(in));
    }
  }
  if (lane == 0) {
    s.cnt[it] = c;
    if (hyp) hyp[(size_t)(j0 + job) * iters + it].count = c;
  }
}

// The wavefront's J^T J, J^T e, e^T e at `param` over the points set[0..len): lane s sums points s, s + 64, ..., then every lane
// adds the 64 partials in lane order (the CPU restatement's order).
__device__ void lm_eval(const Slice& s, const int* set, int len, const double* param, const double* K, int with_j, double* acc,
                        double (*part)[PNP_ACC]) {
  const int lane = threadIdx.x;
  double R[9], dR[27], mine[PNP_ACC];
  pnp_rodrigues(param, R, dR);
  for (int q = 0; q < PNP_ACC; q++) mine[q] = 0;
  for (int i = lane; i < len; i += kWave) {
    const int k = set[i];
    pnp_lm_point(R, dR, param + 3, s.X + 3 * k, s.U + 2 * k, K, with_j, mine);
  }
  __syncthreads();
  for (int q = 0; q < PNP_ACC; q++) part[lane][q] = mine[q];
  __syncthreads();
  for (int q = 0; q < PNP_ACC; q++) acc[q] = 0;
  for (int l = 0; l < kWave; l++)
    for (int q = 0; q < PNP_ACC; q++) acc[q] += part[l][q];
}

__global__ void __launch_bounds__(64) pnp_finish_kernel(const float* __restrict__ xyz, int cap, int j0, PnpJobs jobs, PnpArgs a,
                                                        char* scratch, sbm_pnp_result* __restrict__ result,
                                                        int* __restrict__ inliers) {
#pragma clang fp contract(off)
  __shared__ double part[kWave][PNP_ACC];
  const int lane = threadIdx.x, job = blockIdx.x;
  const int iters = a.iterations;
  Slice s = slice_at(scratch, job, cap, iters);
  const int N = s.n[0];
  sbm_pnp_result r;
  memset(&r, 0, sizeof(r));
  r.num_matches = N;
  r.best_iteration = -1;
  r.refine_exit = -1;
  r.cov_dist = r.cov_angle = 1.0;
  int nin = 0;
  const int* list = s.setA;
  if (N < a.min_inliers) {
    r.status = SBM_PNP_FEW_MATCHES;
  } else {
    // the RANSAC loop, replayed over the counts
    int niters = max(iters, 1), good = 0, best = -1;
    if (N == 6) {
      niters = 1;
      good = 6;
      best = 0;
    } else {
      for (int it = 0; it < niters; it++) {
        const int c = s.cnt[it];
        if (c > max(good, 5)) {
          best = it;
          good = c;
          niters = pnp_update_num_iters(a.confidence, (double)(N - c) / N, 6, niters);
        }
      }
    }
    r.niters = niters;
    r.ransac_inliers = good;
    r.best_iteration = best;
    if (good <= 0) {
      r.status = SBM_PNP_NO_MODEL;
      r.best_iteration = -1;
    } else {
      double bR[9], bt[3];
      for (int k = 0; k < 9; k++) bR[k] = s.hR[12 * best + k];
      for (int k = 0; k < 3; k++) bt[k] = s.hR[12 * best + 9 + k];
      // the RANSAC inlier set, in index order
      int base = 0;
      for (int b = 0; b < N; b += kWave) {
        const int i = b + lane;
        const bool in = i < N && (N == 6 || pnp_reproj_err(bR, bt, s.X + 3 * i, s.U + 2 * i, a.K) <= a.gate);
        const unsigned long long m = __ballot(in);
        if (in) s.setA[base + prefix(m, lane)] = i;
        base += __popcll(m);
      }
      __syncthreads();   // the set was written by every lane; the refine or the covariance loop reads it across lanes
      nin = good;
      double param[6];
      pnp_rodrigues_inv(bR, param);
      for (int k = 0; k < 3; k++) param[3 + k] = bt[k];
      if (nin >= a.min_inliers && a.refine_iterations > 0) {
        int* prev = s.setA;
        int* next = s.setB;
        int prev_len = nin, next_len = 0, count = 0, solves = 0, exit_code = 0;
        float thr = a.reproj;
        __syncthreads();
        while (count < a.refine_iterations) {
          // cv::solvePnP(ITERATIVE, useExtrinsicGuess) on prev: CvLevMarq's state machine, unrolled
          double acc[PNP_ACC], JtJ[PNP_ACC], prm[6];
          int lg = -3, lm_iters = 0;
          lm_eval(s, prev, prev_len, param, a.K, 1, JtJ, part);
          double prev_norm = sqrt(JtJ[27]);
          for (;;) {
            for (int k = 0; k < 6; k++) prm[k] = param[k];
            pnp_lm_step(JtJ, a.lam[lg + 16], prm, param);
            double err_norm;
            for (;;) {
              lm_eval(s, prev, prev_len, param, a.K, 0, acc, part);
              err_norm = sqrt(acc[27]);
              if (err_norm > prev_norm && ++lg <= 16) {
                pnp_lm_step(JtJ, a.lam[lg + 16], prm, param);
                continue;
              }
              break;
            }
            lg = max(lg - 1, -16);
            if (++lm_iters >= 20 || pnp_lm_converged(param, prm)) break;
            prev_norm = err_norm;
            lm_eval(s, prev, prev_len, param, a.K, 1, JtJ, part);
          }
          // computeReprojErrors over all N points
          double R[9], dR[27];
          pnp_rodrigues(param, R, dR);
          int k = 0;
          for (int b = 0; b < N; b += kWave) {
            const int i = b + lane;
            float e = 0.f;
            bool in = false;
            if (i < N) {
              e = pnp_reproj_err(R, param + 3, s.X + 3 * i, s.U + 2 * i, a.K);
              in = e <= thr;
            }
            const unsigned long long m = __ballot(in);
            if (in) {
              const int o = k + prefix(m, lane);
              next[o] = i;
              s.err[o] = e;
            }
            k += __popcll(m);
          }
          next_len = k;
          __syncthreads();
          const float var = pnp_variance(s.err, k);
          const float sg = a.sigma * (float)sqrt(var);
          thr = a.reproj < sg ? a.reproj : sg;
          solves++;
          if (next_len < a.min_inliers) {
            exit_code = 1;
            break;
          }
          bool same = next_len == prev_len;
          if (same) {
            bool diff = false;
            for (int i = lane; i < next_len; i += kWave) diff |= next[i] != prev[i];
            same = __ballot(diff) == 0ull;
          }
          if (same) {
            exit_code = 2;
            break;
          }
          int* tp = next;   // std::swap(new_inliers, prev_inliers)
          next = prev;
          prev = tp;
          const int tl = next_len;
          next_len = prev_len;
          prev_len = tl;
          count++;
          __syncthreads();
        }
        list = next;   // std::swap(new_inliers, inliers)
        nin = next_len;
        r.refine_solves = solves;
        r.refine_exit = exit_code;
      }
      double R[9], dR[27];
      pnp_rodrigues(param, R, dR);
      for (int k = 0; k < 3; k++) {
        r.rvec[k] = param[k];
        r.tvec[k] = param[3 + k];
      }
      for (int k = 0; k < 9; k++) r.R[k] = R[k];
      if (nin < a.min_inliers) {
        r.status = r.refine_exit < 0 ? SBM_PNP_FEW_RANSAC_INLIERS : SBM_PNP_FEW_REFINED_INLIERS;
      } else {
        r.status = SBM_PNP_OK;
        pnp_transform(R, param + 3, a.has_local ? a.local : nullptr, r.transform);
        // covariance terms of the inliers whose to-point is finite, then the medians by rank
        const float* xto = xyz + (size_t)jobs.j[job].y * cap * 3;
        int nv = 0;
        for (int b = 0; b < nin; b += kWave) {
          const int i = b + lane;
          bool ok = false;
          float d = 0.f, g = 0.f;
          if (i < nin) {
            const int q = list[i];
            const float* to = xto + (size_t)s.tt[q] * 3;
            ok = pnp_finite3(to);
            if (ok) pnp_cov_terms(s.X + 3 * q, to, r.transform, &d, &g);
          }
          const unsigned long long m = __ballot(ok);
          if (ok) {
            s.cd[nv + prefix(m, lane)] = d;
            s.ca[nv + prefix(m, lane)] = g;
          }
          nv += __popcll(m);
        }
        __syncthreads();
        if (nv) {
          const int kth = nv >> 1;
          int hit_d = 0, hit_a = 0;
          float md = 0.f, ma = 0.f;
          for (int i = lane; i < nv; i += kWave) {
            const float di = s.cd[i], ai = s.ca[i];
            int rd = 0, ra = 0;
            for (int j = 0; j < nv; j++) {
              const float dj = s.cd[j], aj = s.ca[j];
              rd += (dj < di) || (dj == di && j < i);
              ra += (aj < ai) || (aj == ai && j < i);
            }
            if (rd == kth) { md = di; hit_d = 1; }
            if (ra == kth) { ma = ai; hit_a = 1; }
          }
          // exactly one lane holds each median; broadcast through LDS
          __syncthreads();
          if (hit_d) part[0][0] = md;
          if (hit_a) part[0][1] = ma;
          __syncthreads();
          const double vd = part[0][0], va = part[0][1];
          r.cov_dist = vd < 0.0001 ? 0.0001 : vd;
          r.cov_angle = va < 0.0001 ? 0.0001 : va;
        }
      }
    }
  }
  __syncthreads();   // the lists were written by every lane
  r.num_inliers = nin;
  int* out = inliers + (size_t)(j0 + job) * cap;
  for (int i = lane; i < nin; i += kWave) out[i] = s.mt[list[i]];
  if (lane == 0) result[j0 + job] = r;
}

}  // namespace

static bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

static int pnp_check(int n, int m, const int* jobs, int cap, const double* K, const void* d_xyz, const void* d_kpts,
                     const void* d_count, const void* d_pairs, const void* d_npairs, const void* d_result, const void* d_inliers,
                     const void* d_hyp) {
  if (n <= 0 || m <= 0) return SBM_ERR_BATCH;
  if (cap < 1 || cap > 65535) return SBM_ERR_SIZE;
  if (m > 65535) return SBM_ERR_UNSUPPORTED;
  for (int j = 0; j < 2 * m; j++)
    if (jobs[j] < 0 || jobs[j] >= n) return SBM_ERR_SIZE;
  for (int k = 0; k < 4; k++)
    if (!std::isfinite(K[k])) return SBM_ERR_UNSUPPORTED;
  if (K[0] == 0 || K[1] == 0) return SBM_ERR_UNSUPPORTED;
  if (misaligned(d_xyz, 4) || misaligned(d_count, 4) || misaligned(d_npairs, 4) || misaligned(d_inliers, 4) ||
      misaligned(d_kpts, 8) || misaligned(d_pairs, 8) || misaligned(d_result, 8) || misaligned(d_hyp, 8))
    return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

enum PnpStage { kPnpHyp, kPnpScore, kPnpRefine, kPnpTotal, kPnpStageCount };
static const char* const kPnpNames[] = {"pnp_hyp", "pnp_score", "pnp_refine", "pnp_total"};
StageTable pnp_stages() { return stage_table<kPnpStageCount, kPnpStageCount>(kPnpNames); }

static int pnp_run(sbm_handle* h, int m, const int* jobs, const void* d_xyz, const void* d_kpts, const void* d_count, int cap,
                   const void* d_pairs, const void* d_npairs, const double* K, const sbm_stereo_model* model,
                   const sbm_pnp_params* p, void* d_result, void* d_inliers, void* d_hyp) {
  StageClock& clk = h->pnp.clock;
  PnpArgs a;
  memset(&a, 0, sizeof(a));
  for (int k = 0; k < 4; k++) a.K[k] = K[k];
  const double LOG10 = std::log(10.);
  for (int k = -16; k <= 16; k++) a.lam[k + 16] = std::exp(k * LOG10);
  a.has_local = model && model->has_local ? 1 : 0;
  if (a.has_local) memcpy(a.local, model->local, sizeof(a.local));
  a.min_inliers = p->min_inliers;
  a.refine_iterations = p->refine_iterations;
  a.iterations = p->iterations;
  a.gate = (float)((double)p->reprojection_error * p->reprojection_error);
  a.reproj = p->reprojection_error;
  a.sigma = p->refine_sigma;
  a.confidence = p->confidence;
  const int iters = p->iterations;
  const size_t per_job = slice_bytes(cap, iters);
  const int mj = (int)std::max<size_t>(1, std::min<size_t>(kArgJobs, kScratchBudget / per_job));
  HIPCHK(h, h->pnp.scratch.grow(per_job * mj, h->stream));   // one piece of mj slices, each the counting pass of slice_layout: slice_at
  char* scratch = h->pnp.scratch.as<char>();
  for (int j0 = 0; j0 < m; j0 += mj) {
    const int k = std::min(mj, m - j0);
    PnpJobs jb;
    memset(&jb, 0, sizeof(jb));
    for (int j = 0; j < k; j++) jb.j[j] = make_int2(jobs[2 * (j0 + j)], jobs[2 * (j0 + j) + 1]);
    HIPCHK(h, clk.mark(kPnpHyp, h->stream));
    hipLaunchKernelGGL(pnp_gather_kernel, dim3(k), dim3(kWave), 0, h->stream, (const float*)d_xyz, (const float*)d_kpts,
                       (const int*)d_count, (const int2*)d_pairs, (const int*)d_npairs, cap, j0, jb, iters, p->min_inliers,
                       scratch);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(pnp_hyp_kernel, dim3((iters + kWave - 1) / kWave, k), dim3(kWave), 0, h->stream, cap, j0, iters,
                       p->min_inliers, a, scratch, (sbm_pnp_hypothesis*)d_hyp);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, clk.mark(kPnpScore, h->stream));
    hipLaunchKernelGGL(pnp_score_kernel, dim3((iters + 3) / 4, k), dim3(256), 0, h->stream, cap, j0, iters, p->min_inliers, a,
                       scratch, (sbm_pnp_hypothesis*)d_hyp);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, clk.mark(kPnpRefine, h->stream));
    hipLaunchKernelGGL(pnp_finish_kernel, dim3(k), dim3(kWave), 0, h->stream, (const float*)d_xyz, cap, j0, jb, a, scratch,
                       (sbm_pnp_result*)d_result, (int*)d_inliers);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, clk.mark(kPnpTotal, h->stream));
    for (int s = kPnpHyp; s < kPnpTotal; s++) HIPCHK(h, clk.add(s, s, s + 1));
  }
  if (clk.on) clk.ms[kPnpTotal] = clk.ms[kPnpHyp] + clk.ms[kPnpScore] + clk.ms[kPnpRefine];
  return SBM_OK;
}

}  // namespace sbm

// ---- entry points --------------------------------------------------------------------------------------------------------
using namespace sbm;

extern "C" {

void sbm_pnp_params_default(sbm_pnp_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->min_inliers = 20;
  p->refine_iterations = 1;
  p->iterations = 300;
  p->reprojection_error = 2.0f;
  p->refine_sigma = 3.0f;
  p->confidence = 0.99;
}

int sbm_pnp_params_validate(const sbm_pnp_params* p) {
  if (!p) return SBM_ERR_NULL;
  if (p->min_inliers < 6 || p->min_inliers > 65535) return SBM_ERR_UNSUPPORTED;
  if (p->refine_iterations < 0 || p->refine_iterations > 100) return SBM_ERR_UNSUPPORTED;
  if (p->iterations < 1 || p->iterations > 1000) return SBM_ERR_UNSUPPORTED;
  if (!std::isfinite(p->reprojection_error) || !(p->reprojection_error > 0.f)) return SBM_ERR_UNSUPPORTED;
  if (!std::isfinite(p->refine_sigma) || !(p->refine_sigma >= 0.f)) return SBM_ERR_UNSUPPORTED;
  if (!(p->confidence > 0.0 && p->confidence < 1.0)) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

int sbm_estimate_motion_device(sbm_handle* h, int n, int m, const int* jobs, const void* d_xyz, const void* d_kpts, const void* d_count,
                               int cap, const void* d_pairs, const void* d_npairs, const double* K, const sbm_stereo_model* model,
                               const sbm_pnp_params* p, void* d_result, void* d_inliers, void* d_hyp, int sync) {
  if (!h || !jobs || !d_xyz || !d_kpts || !d_count || !d_pairs || !d_npairs || !K || !p || !d_result || !d_inliers)
    return SBM_ERR_NULL;
  int st = sbm_pnp_params_validate(p);
  if (st == SBM_OK) st = pnp_check(n, m, jobs, cap, K, d_xyz, d_kpts, d_count, d_pairs, d_npairs, d_result, d_inliers, d_hyp);
  if (st != SBM_OK) return st;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, h->pnp.clock.start(pnp_stages(), h->profiling != 0));
  st = pnp_run(h, m, jobs, d_xyz, d_kpts, d_count, cap, d_pairs, d_npairs, K, model, p, d_result, d_inliers, d_hyp);
  if (st == SBM_OK && sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return st;
}

// The host form: the from-points as frame 0, the to-keypoints and to-points as frame 1 of a store with cap = max(nf, nt,
// npairs, 1); one job; the record and the inlier list come back.
int sbm_estimate_motion(sbm_handle* h, const float* xyz_from, int nf, const float* kpts_to, const float* xyz_to, int nt,
                        const int* pairs, int npairs, const double* K, const sbm_stereo_model* model, const sbm_pnp_params* p,
                        sbm_pnp_result* result, int* inliers) {
  if (!h || !K || !p || !result || (nf > 0 && !xyz_from) || (nt > 0 && (!kpts_to || !xyz_to)) ||
      (npairs > 0 && (!pairs || !inliers)))
    return SBM_ERR_NULL;
  if (nf < 0 || nt < 0 || npairs < 0) return SBM_ERR_SIZE;
  const int cap = std::max({nf, nt, npairs, 1});
  if (cap > 65535) return SBM_ERR_SIZE;
  int st = sbm_pnp_params_validate(p);
  if (st != SBM_OK) return st;
  const int job[2] = {0, 1};
  st = pnp_check(2, 1, job, cap, K, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (st != SBM_OK) return st;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  float *d_xyz = nullptr, *d_kp = nullptr;
  int *d_n = nullptr, *d_pairs = nullptr, *d_inl = nullptr;
  sbm_pnp_result* d_res = nullptr;
  HIPCHK(h, carve(h->pnp.io, h->stream, [&](Carve& c) {
    d_xyz = c.take<float>((size_t)2 * cap * 3);   // 2 frames
    d_kp = c.take<float>((size_t)2 * cap * 2);    // 2 frames
    d_n = c.take<int>(4);                         // counts (2) + npairs (1) + pad
    d_pairs = c.take<int>((size_t)cap * 2);
    d_res = c.take<sbm_pnp_result>(1);
    d_inl = c.take<int>(cap);
  }));
  const int cnt[3] = {nf, nt, npairs};
  if (nf > 0) HIPCHK(h, hipMemcpyAsync(d_xyz, xyz_from, (size_t)nf * 12, hipMemcpyHostToDevice, h->stream));
  if (nt > 0) {
    HIPCHK(h, hipMemcpyAsync(d_xyz + (size_t)cap * 3, xyz_to, (size_t)nt * 12, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_kp + (size_t)cap * 2, kpts_to, (size_t)nt * 8, hipMemcpyHostToDevice, h->stream));
  }
  if (npairs > 0) HIPCHK(h, hipMemcpyAsync(d_pairs, pairs, (size_t)npairs * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_n, cnt, sizeof(cnt), hipMemcpyHostToDevice, h->stream));
  st = h->pnp.clock.start(pnp_stages(), h->profiling != 0) == hipSuccess ? SBM_OK : SBM_ERR_HIP;
  if (st == SBM_OK) st = pnp_run(h, 1, job, d_xyz, d_kp, d_n, cap, d_pairs, d_n + 2, K, model, p, d_res, d_inl, nullptr);
  if (st != SBM_OK) {
    hipStreamSynchronize(h->stream);   // enqueued copies read the caller's arrays and `cnt`
    return st;
  }
  HIPCHK(h, hipMemcpyAsync(result, d_res, sizeof(sbm_pnp_result), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (result->num_inliers > 0)
    HIPCHK(h, hipMemcpy(inliers, d_inl, (size_t)result->num_inliers * 4, hipMemcpyDeviceToHost));
  return SBM_OK;
}

}  // extern "C"
