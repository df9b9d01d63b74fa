// Keypoint matching of the reference's computeTransform (src/slam/src/core/Registration.cpp): matchingNoGuess's brute-force
// knnMatch(k = 2) + NNDR, matchingGuess's projection of the "from" frame's 3-D keypoints (matchingGuess_Projection), the 40 px
// radius gate (radiusMatch, NORM_L2) and the per-query k-NN-2 + NNDR over the gated candidates (matchingGuess_search), and in both
// modes the "each to-index at most once, first come first served" rule of the std::set. DESIGN.md section 11.
//
//   knn      one wavefront per (job, 64-query tile, train slice): each lane keeps its query row in 8 VGPRs; the slice's train rows
//            (and in guided mode their keypoints) pass through LDS 64 at a time and are read as broadcasts; per row 8 XOR +
//            8 popcount, the radius gate, the k-NN-2 update. Partial (best, d0, d1, count) records per slice go to scratch.
//   claim    one lane per (job, query): merges the slices in train order (the lower index wins ties), decides acceptance, writes
//            the record, and an accepted query atomicMin's its index into the owner slot of its train row.
//   emit     one workgroup per job: keeps (q, t) with owner[t] == q, in q order (ballot + prefix, as orb_compact_kernel).
//   project  one lane per (job, point slot): transformPoint's z in float and projectPoints' pinhole model in double, unfused.
#include <algorithm>
#include <climits>
#include <cmath>

#include "sbm_handle.h"

namespace sbm {

constexpr int kReadMatchFusedL2 = 256;   // SBM_CV_READING: the radius test's squared distance is fmaf(dy, dy, dx * dx)
constexpr int kMatchNone = 257;          // d0 / d1 of a record with fewer candidates: above every Hamming distance (0..256)

namespace {

constexpr int kTile = 64;        // queries per wavefront (= workgroup)
constexpr int kStage = 64;       // train rows per LDS stage
constexpr int kMaxSlice = 32;    // train slices per query tile, at most
constexpr int kArgJobs = 64;     // jobs per launch: their (from, to) pairs travel as a kernel argument
constexpr int kProjJobs = 32;    // jobs per projection launch (their transforms travel as a kernel argument)
constexpr int kTargetWaves = 8192;                        // slices are added until a launch has about this many wavefronts

struct MatchJobs {
  int2 j[kArgJobs];   // (from frame, to frame)
};
struct ProjJobs {
  int from[kProjJobs];
  float T[kProjJobs][12];
};

__device__ __forceinline__ int clamp_count(const int* count, int f, int cap) { return min(max(count[f], 0), cap); }

template <bool kGuess>
__global__ void __launch_bounds__(64) match_knn_kernel(const uint8_t* __restrict__ desc, const int* __restrict__ count,
                                                       const float* __restrict__ kpts, const float* __restrict__ proj, int cap,
                                                       int slice_rows, int j0, MatchJobs jobs, float thr, int fused,
                                                       int4* __restrict__ part, int* __restrict__ owner) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) uint4 s_row[kStage][2];
  __shared__ float2 s_xy[kStage];
  const int lane = threadIdx.x, job = blockIdx.z, slice = blockIdx.y, nslice = gridDim.y;
  const int q = blockIdx.x * kTile + lane;
  const int f = jobs.j[job].x, t = jobs.j[job].y;
  if (slice == 0 && q < cap) owner[(size_t)job * cap + q] = INT_MAX;   // the claim kernel that follows reads it
  const int nf = clamp_count(count, f, cap), nt = clamp_count(count, t, cap);
  const int r0 = slice * slice_rows, r1 = min(r0 + slice_rows, nt);
  if (blockIdx.x * kTile >= nf || r0 >= r1) return;   // uniform over the workgroup; the claim kernel reads no such slice

  uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
  float px = 0.f, py = 0.f;
  if (q < nf) {
    const uint4* qa = (const uint4*)(desc + ((size_t)f * cap + q) * 32);
    a0 = qa[0];
    a1 = qa[1];
    if (kGuess) {
      const float2 p = ((const float2*)proj)[(size_t)(j0 + job) * cap + q];
      px = p.x;
      py = p.y;
    }
  }
  int best = -1, d0 = kMatchNone, d1 = kMatchNone, cnt = 0;
  const uint4* trow = (const uint4*)(desc + (size_t)t * cap * 32);
  const float2* txy = (const float2*)kpts + (size_t)t * cap;
  for (int c0 = r0; c0 < r1; c0 += kStage) {
    const int nr = min(kStage, r1 - c0);
    __syncthreads();   // the previous stage has been read
    if (lane < nr) {
      s_row[lane][0] = trow[2 * (c0 + lane)];
      s_row[lane][1] = trow[2 * (c0 + lane) + 1];
      if (kGuess) s_xy[lane] = txy[c0 + lane];
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < nr; k++) {
      const uint4 b0 = s_row[k][0], b1 = s_row[k][1];
      const int d = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
                    __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
      bool cand = true;
      if (kGuess) {
        const float2 p = s_xy[k];
        const float dx = px - p.x, dy = py - p.y;
        const float xx = dx * dx;
        const float d2 = fused ? __fmaf_rn(dy, dy, xx) : xx + dy * dy;
        cand = d2 < thr;   // == sqrtf(d2) < radius (thr: the least float whose rounded square root reaches the radius)
      }
      if (cand) {
        cnt++;
        if (d < d0) {
          d1 = d0;
          d0 = d;
          best = c0 + k;
        } else if (d < d1) {
          d1 = d;
        }
      }
    }
  }
  if (q < nf) part[((size_t)job * nslice + slice) * cap + q] = make_int4(best, d0, d1, cnt);
}

// Merges the slices of every (job, query) in train order, writes the record (d_knn) and the accepted train index, and claims it.
template <bool kGuess>
__global__ void __launch_bounds__(256) match_claim_kernel(const int* __restrict__ count, int cap, int slice_rows, int nslice, int j0,
                                                          MatchJobs jobs, float nndr, const int4* __restrict__ part,
                                                          int* __restrict__ owner, int* __restrict__ acc, int4* __restrict__ knn) {
  const int q = blockIdx.x * 256 + threadIdx.x, job = blockIdx.y;
  if (q >= cap) return;
  const int f = jobs.j[job].x, t = jobs.j[job].y;
  const int nf = clamp_count(count, f, cap), nt = clamp_count(count, t, cap);
  int best = -1, d0 = kMatchNone, d1 = kMatchNone, cnt = 0;
  if (q < nf) {
    const int ns = min(nslice, (nt + slice_rows - 1) / slice_rows);
    for (int s = 0; s < ns; s++) {
      const int4 r = part[((size_t)job * nslice + s) * cap + q];
      if (r.y < d0) {
        d1 = min(d0, r.z);
        d0 = r.y;
        best = r.x;
      } else {
        d1 = min(d1, r.y);
      }
      cnt += r.w;
    }
  }
  // no-guess: fewer than two rows is no match (nt == 1 is undefined in the reference); guided: one candidate is taken as it is
  const bool ok = cnt >= 2 ? (float)d0 < nndr * (float)d1 : (kGuess && cnt == 1);
  acc[(size_t)job * cap + q] = ok ? best : -1;
  if (ok) atomicMin(&owner[(size_t)job * cap + best], q);
  if (knn) knn[(size_t)(j0 + job) * cap + q] = make_int4(best, d0, d1, cnt);
}

__global__ void __launch_bounds__(256) match_emit_kernel(const int* __restrict__ count, int cap, int j0, MatchJobs jobs,
                                                         const int* __restrict__ owner, const int* __restrict__ acc,
                                                         int2* __restrict__ pairs, int* __restrict__ npairs) {
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, job = blockIdx.x;
  const int nf = clamp_count(count, jobs.j[job].x, cap);
  const int* a = acc + (size_t)job * cap;
  const int* o = owner + (size_t)job * cap;
  int2* out = pairs + (size_t)(j0 + job) * cap;
  int kept = 0;
  for (int base = 0; base < nf; base += 256) {
    const int q = base + tid;
    int t = -1;
    if (q < nf) t = a[q];
    const bool keep = t >= 0 && o[t] == q;
    const unsigned long long m = __ballot(keep);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wv] = __popcll(m);
    __syncthreads();
    int off = kept;
    for (int w = 0; w < wv; w++) off += s_wave[w];
    const int tot = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (keep) out[off + below] = make_int2(q, t);
    kept += tot;
    __syncthreads();
  }
  if (tid == 0) npairs[j0 + job] = kept;
}

__global__ void __launch_bounds__(256) match_project_kernel(const float* __restrict__ xyz, const int* __restrict__ count, int cap,
                                                            int j0, ProjJobs jobs, double fx, double fy, double cx, double cy,
                                                            int W, int H, float* __restrict__ proj) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * 256 + threadIdx.x, job = blockIdx.y;
  if (s >= cap) return;
  const int f = jobs.from[job];
  const int n = clamp_count(count, f, cap);
  float u = NAN, v = NAN;
  if (s < n) {
    const float* p = xyz + ((size_t)f * cap + s) * 3;
    const float x = p[0], y = p[1], z = p[2];
    const float* T = jobs.T[job];
    const float zc = T[8] * x + T[9] * y + T[10] * z + T[11];   // transformPoint(p, guessCameraRef).z
    const double X = (double)x, Y = (double)y, Z = (double)z;
    const double xc = (double)T[0] * X + (double)T[1] * Y + (double)T[2] * Z + (double)T[3];
    const double yc = (double)T[4] * X + (double)T[5] * Y + (double)T[6] * Z + (double)T[7];
    const double wc = (double)T[8] * X + (double)T[9] * Y + (double)T[10] * Z + (double)T[11];
    const double inv = wc != 0.0 ? 1.0 / wc : 1.0;
    const double xn = xc * inv, yn = yc * inv;
    const float pu = (float)(xn * fx + cx), pv = (float)(yn * fy + cy);
    if (0.f < pu && pu < (float)(W - 1) && 0.f < pv && pv < (float)(H - 1) && zc > 0.f) {
      u = pu;
      v = pv;
    }
  }
  ((float2*)proj)[(size_t)(j0 + job) * cap + s] = make_float2(u, v);
}

}  // namespace

// The least float x >= 0 with sqrtf(x) >= r (correctly rounded square root; +inf when there is none): sqrtf(d) < r <=> d < x,
// because the rounded square root is monotone. Host arithmetic, without contraction.
static float radius_threshold(float r) {
  float x = (float)((double)r * (double)r);
  while (x > 0.f && std::sqrt(std::nextafter(x, 0.f)) >= r) x = std::nextafter(x, 0.f);
  while (std::isfinite(x) && std::sqrt(x) < r) x = std::nextafter(x, INFINITY);
  return x;
}

}  // namespace sbm

// ---- entry points --------------------------------------------------------------------------------------------------------
using namespace sbm;

static bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// The limits on a call's job count and store capacity, shared by the checks and the plan.
static int match_limits(int m, int cap) {
  if (m <= 0) return SBM_ERR_BATCH;
  if (cap < 1 || cap > 65535) return SBM_ERR_SIZE;
  if (m > 65535) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

// The plan of one call: everything the host decides before it launches anything, as plain data, computed without a HIP call.
// match_run and project_run execute it and recompute nothing; sbm_match_plan (include/sbm.h) copies it out.
//   slices   added until a launch has about kTargetWaves wavefronts, at most kMaxSlice, each a whole number of LDS stages; the
//            count is then what those rows need, so the last slice is never empty at nt == cap.
//   scratch  per job: nslice partial records (16 bytes) + owner + accepted (4 bytes each) per slot. For every legal (cap, m)
//            jobs_per_launch == min(m, kArgJobs) and scratch_bytes <= 96 MiB, well within the 256 MiB the header promises
//            (tests/test_match_plan.py enumerates every cap through the export), so no budget clamp cuts the jobs per launch.
// One launch's scratch. Whole words on 4-byte boundaries: nothing is padded, which keeps the published scratch_bytes exact.
struct MatchScratch { int4* part; int *owner, *acc; };
constexpr size_t kMatchAlign = 4;
static MatchScratch match_scratch(Carve& c, size_t slots, int nslice) { return {c.take<int4>(slots * nslice), c.take<int>(slots), c.take<int>(slots)}; }
static int match_plan(int cap, int m, sbm_match_plan_info* pl) {
  memset(pl, 0, sizeof(*pl));
  const int st = match_limits(m, cap);
  if (st != SBM_OK) return st;
  const int qtiles = (cap + kTile - 1) / kTile;
  const int mj = std::min(m, kArgJobs);
  int nslice = std::max(1, (kTargetWaves + qtiles * mj - 1) / (qtiles * mj));
  nslice = std::min({nslice, kMaxSlice, (cap + kStage - 1) / kStage});
  const int slice_rows = ((cap + nslice - 1) / nslice + kStage - 1) / kStage * kStage;
  nslice = (cap + slice_rows - 1) / slice_rows;
  pl->qtiles = qtiles;
  pl->nslice = nslice;
  pl->slice_rows = slice_rows;
  pl->jobs_per_launch = mj;
  pl->launches = (m + mj - 1) / mj;
  pl->proj_jobs_per_launch = std::min(m, kProjJobs);
  pl->proj_launches = (m + kProjJobs - 1) / kProjJobs;
  pl->scratch_bytes = (int64_t)carve_bytes([&](Carve& c) { match_scratch(c, (size_t)mj * cap, nslice); }, kMatchAlign);
  return SBM_OK;
}

static int match_check(int n, int m, const int* jobs, int cap, const void* d_desc, const void* d_count, const void* d_pairs,
                       const void* d_npairs, const void* d_knn) {
  if (n <= 0) return SBM_ERR_BATCH;
  const int st = match_limits(m, cap);
  if (st != SBM_OK) return st;
  for (int j = 0; j < 2 * m; j++)
    if (jobs[j] < 0 || jobs[j] >= n) return SBM_ERR_SIZE;
  if (misaligned(d_desc, 16) || misaligned(d_count, 4) || misaligned(d_pairs, 8) || misaligned(d_npairs, 4) ||
      misaligned(d_knn, 16))
    return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

// Stage times of a call, and the marks it records: match_run all three per launch, project_run the first two around its kernel.
enum MatchStage { kMtKnn, kMtUnique, kMtTotal, kMtProject, kMtStageCount };
enum MatchMark { kMtBegin, kMtMid, kMtEnd, kMtMarkCount };
static const char* const kMatchNames[] = {"match_knn", "match_unique", "match_total", "match_project"};
StageTable sbm::match_stages() { return stage_table<kMtStageCount, kMtMarkCount>(kMatchNames); }

// Enqueues the three kernels per launch of up to kArgJobs jobs; with profiling, times k-NN and claim + emit.
static int match_run(sbm_handle* h, int m, const int* jobs, const void* d_desc, const void* d_count, int cap,
                     const sbm_match_params* p, const void* d_kpts, const void* d_proj, void* d_pairs, void* d_npairs, void* d_knn,
                     bool guess) {
  StageClock& clk = h->mt.clock;
  const int reading = env_switch("SBM_CV_READING", 0);
  const int fused = (reading & kReadMatchFusedL2) ? 1 : 0;
  const float thr = radius_threshold(p->radius);
  sbm_match_plan_info pl;
  const int pst = match_plan(cap, m, &pl);
  if (pst != SBM_OK) return pst;
  const int qtiles = pl.qtiles, nslice = pl.nslice, slice_rows = pl.slice_rows, mj = pl.jobs_per_launch;
  MatchScratch sc;
  HIPCHK(h, carve(h->mt.scratch, h->stream, [&](Carve& c) { sc = match_scratch(c, (size_t)mj * cap, nslice); }, kMatchAlign));
  const auto [part, owner, acc] = sc;
  for (int j0 = 0; j0 < m; j0 += mj) {
    const int k = std::min(mj, m - j0);
    MatchJobs a;
    memset(&a, 0, sizeof(a));
    for (int j = 0; j < k; j++) a.j[j] = make_int2(jobs[2 * (j0 + j)], jobs[2 * (j0 + j) + 1]);
    const dim3 gk(qtiles, nslice, k), gc((cap + 255) / 256, k);
    HIPCHK(h, clk.mark(kMtBegin, h->stream));
    if (guess)
      hipLaunchKernelGGL(match_knn_kernel<true>, gk, dim3(64), 0, h->stream, (const uint8_t*)d_desc, (const int*)d_count,
                         (const float*)d_kpts, (const float*)d_proj, cap, slice_rows, j0, a, thr, fused, part, owner);
    else
      hipLaunchKernelGGL(match_knn_kernel<false>, gk, dim3(64), 0, h->stream, (const uint8_t*)d_desc, (const int*)d_count,
                         (const float*)nullptr, (const float*)nullptr, cap, slice_rows, j0, a, thr, fused, part, owner);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, clk.mark(kMtMid, h->stream));
    if (guess)
      hipLaunchKernelGGL(match_claim_kernel<true>, gc, dim3(256), 0, h->stream, (const int*)d_count, cap, slice_rows, nslice, j0, a,
                         p->nndr, (const int4*)part, owner, acc, (int4*)d_knn);
    else
      hipLaunchKernelGGL(match_claim_kernel<false>, gc, dim3(256), 0, h->stream, (const int*)d_count, cap, slice_rows, nslice, j0, a,
                         p->nndr, (const int4*)part, owner, acc, (int4*)d_knn);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(match_emit_kernel, dim3(k), dim3(256), 0, h->stream, (const int*)d_count, cap, j0, a, (const int*)owner,
                       (const int*)acc, (int2*)d_pairs, (int*)d_npairs);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, clk.mark(kMtEnd, h->stream));
    HIPCHK(h, clk.add(kMtKnn, kMtBegin, kMtMid));
    HIPCHK(h, clk.add(kMtUnique, kMtMid, kMtEnd));
  }
  if (clk.on) clk.ms[kMtTotal] = clk.ms[kMtKnn] + clk.ms[kMtUnique] + clk.ms[kMtProject];
  return SBM_OK;
}

static int project_run(sbm_handle* h, int m, const int* from, const void* d_xyz, const void* d_count, int cap, const float* T,
                       const double* K, int W, int H, void* d_proj) {
  StageClock& clk = h->mt.clock;
  sbm_match_plan_info pl;
  const int pst = match_plan(cap, m, &pl);
  if (pst != SBM_OK) return pst;
  const int pj = pl.proj_jobs_per_launch;
  for (int j0 = 0; j0 < m; j0 += pj) {
    const int k = std::min(pj, m - j0);
    ProjJobs a;
    memset(&a, 0, sizeof(a));
    for (int j = 0; j < k; j++) {
      a.from[j] = from[j0 + j];
      memcpy(a.T[j], T + (size_t)(j0 + j) * 12, 12 * sizeof(float));
    }
    HIPCHK(h, clk.mark(kMtBegin, h->stream));
    hipLaunchKernelGGL(match_project_kernel, dim3((cap + 255) / 256, k), dim3(256), 0, h->stream, (const float*)d_xyz,
                       (const int*)d_count, cap, j0, a, K[0], K[1], K[2], K[3], W, H, (float*)d_proj);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, clk.mark(kMtMid, h->stream));
    HIPCHK(h, clk.add(kMtProject, kMtBegin, kMtMid));
  }
  return SBM_OK;
}

static int project_check(int n, int m, const int* from, int cap, int W, int H, const void* d_xyz, const void* d_count,
                         const void* d_proj) {
  if (n <= 0 || m <= 0) return SBM_ERR_BATCH;
  if (cap < 1 || cap > 65535 || W < 1 || H < 1) return SBM_ERR_SIZE;
  if (m > 65535) return SBM_ERR_UNSUPPORTED;
  for (int j = 0; j < m; j++)
    if (from[j] < 0 || from[j] >= n) return SBM_ERR_SIZE;
  if (misaligned(d_xyz, 4) || misaligned(d_count, 4) || misaligned(d_proj, 8)) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

extern "C" {

void sbm_match_params_default(sbm_match_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->nndr = 0.8f;
  p->radius = 40.0f;
}

int sbm_match_params_validate(const sbm_match_params* p) {
  if (!p) return SBM_ERR_NULL;
  if (!std::isfinite(p->nndr) || !std::isfinite(p->radius)) return SBM_ERR_UNSUPPORTED;
  if (!(p->nndr > 0.f && p->nndr <= 1.f) || !(p->radius > 0.f)) return SBM_ERR_UNSUPPORTED;
  return SBM_OK;
}

int sbm_match_plan(int cap, int m, sbm_match_plan_info* out, size_t out_bytes) {
  if (!out) return SBM_ERR_NULL;
  if (out_bytes != sizeof(sbm_match_plan_info)) return SBM_ERR_SIZE;
  return match_plan(cap, m, out);
}

int sbm_match_device(sbm_handle* h, int n, int m, const int* jobs, const void* d_desc, const void* d_count, int cap,
                     const sbm_match_params* p, void* d_pairs, void* d_npairs, void* d_knn, int sync) {
  if (!h || !jobs || !d_desc || !d_count || !p || !d_pairs || !d_npairs) return SBM_ERR_NULL;
  int st = sbm_match_params_validate(p);
  if (st == SBM_OK) st = match_check(n, m, jobs, cap, d_desc, d_count, d_pairs, d_npairs, d_knn);
  if (st != SBM_OK) return st;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, h->mt.clock.start(match_stages(), h->profiling != 0));
  st = match_run(h, m, jobs, d_desc, d_count, cap, p, nullptr, nullptr, d_pairs, d_npairs, d_knn, false);
  if (st == SBM_OK && sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return st;
}

int sbm_match_guess_device(sbm_handle* h, int n, int m, const int* jobs, const void* d_desc, const void* d_count, int cap,
                           const void* d_kpts, const void* d_proj, const sbm_match_params* p, void* d_pairs, void* d_npairs,
                           void* d_knn, int sync) {
  if (!h || !jobs || !d_desc || !d_count || !d_kpts || !d_proj || !p || !d_pairs || !d_npairs) return SBM_ERR_NULL;
  int st = sbm_match_params_validate(p);
  if (st == SBM_OK) st = match_check(n, m, jobs, cap, d_desc, d_count, d_pairs, d_npairs, d_knn);
  if (st == SBM_OK && (misaligned(d_kpts, 8) || misaligned(d_proj, 8))) st = SBM_ERR_UNSUPPORTED;
  if (st != SBM_OK) return st;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, h->mt.clock.start(match_stages(), h->profiling != 0));
  st = match_run(h, m, jobs, d_desc, d_count, cap, p, d_kpts, d_proj, d_pairs, d_npairs, d_knn, true);
  if (st == SBM_OK && sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return st;
}

int sbm_project_points_device(sbm_handle* h, int n, int m, const int* from, const void* d_xyz, const void* d_count, int cap,
                              const float* T, const double* K, int width, int height, void* d_proj, int sync) {
  if (!h || !from || !d_xyz || !d_count || !T || !K || !d_proj) return SBM_ERR_NULL;
  int st = project_check(n, m, from, cap, width, height, d_xyz, d_count, d_proj);
  if (st != SBM_OK) return st;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  HIPCHK(h, h->mt.clock.start(match_stages(), h->profiling != 0));
  st = project_run(h, m, from, d_xyz, d_count, cap, T, K, width, height, d_proj);
  if (h->mt.clock.on) h->mt.clock.ms[kMtTotal] = h->mt.clock.ms[kMtProject];
  if (st == SBM_OK && sync) HIPCHK(h, hipStreamSynchronize(h->stream));
  return st;
}

// The host forms: both descriptor sets (and for the guided form the points) go to handle staging as frames 0 (from) and 1 (to)
// of a store with cap = max(nf, nt, 1); one job; the pairs come back.
static int match_host(sbm_handle* h, bool guess, const float* xyz_from, const float* kpts_to, const uint8_t* desc_from, size_t stride_from,
                      int nf, const uint8_t* desc_to, size_t stride_to, int nt, const float* T, const double* K, int width,
                      int height, const sbm_match_params* p, int* pairs, int* npairs) {
  if (!h || !p || !npairs || (nf > 0 && (!desc_from || !pairs)) || (nt > 0 && !desc_to)) return SBM_ERR_NULL;
  if (guess && (!T || !K || (nf > 0 && !xyz_from) || (nt > 0 && !kpts_to))) return SBM_ERR_NULL;
  if (nf < 0 || nt < 0 || (nf > 0 && stride_from < 32) || (nt > 0 && stride_to < 32)) return SBM_ERR_SIZE;
  if (guess && (width < 1 || height < 1)) return SBM_ERR_SIZE;
  const int cap = std::max({nf, nt, 1});
  if (cap > 65535) return SBM_ERR_SIZE;
  int st = sbm_match_params_validate(p);
  if (st != SBM_OK) return st;
  DeviceScope dscope(h->device);
  HIPCHK(h, dscope.enter());
  uint8_t* d_desc = nullptr;
  int *d_n = nullptr, *d_pairs = nullptr;
  float *d_xyz = nullptr, *d_kp = nullptr, *d_proj = nullptr;   // the guided form's
  HIPCHK(h, carve(h->mt.io, h->stream, [&](Carve& c) {
    d_desc = c.take<uint8_t>((size_t)2 * cap * 32);   // 2 frames
    d_n = c.take<int>(4);                             // counts (2) + npairs (1) + pad
    d_pairs = c.take<int>((size_t)cap * 2);
    if (!guess) return;
    d_xyz = c.take<float>((size_t)2 * cap * 3);       // points of frame 0 (2 frames)
    d_kp = c.take<float>((size_t)2 * cap * 2);        // keypoints of frame 1 (2 frames)
    d_proj = c.take<float>((size_t)cap * 2);          // projections
  }));
  const int cnt[2] = {nf, nt};
  if (nf > 0) HIPCHK(h, hipMemcpy2DAsync(d_desc, 32, desc_from, stride_from, 32, nf, hipMemcpyHostToDevice, h->stream));
  if (nt > 0)
    HIPCHK(h, hipMemcpy2DAsync(d_desc + (size_t)cap * 32, 32, desc_to, stride_to, 32, nt, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(d_n, cnt, sizeof(cnt), hipMemcpyHostToDevice, h->stream));
  if (guess && nf > 0) HIPCHK(h, hipMemcpyAsync(d_xyz, xyz_from, (size_t)nf * 12, hipMemcpyHostToDevice, h->stream));
  if (guess && nt > 0) HIPCHK(h, hipMemcpyAsync(d_kp + (size_t)cap * 2, kpts_to, (size_t)nt * 8, hipMemcpyHostToDevice, h->stream));
  const int job[2] = {0, 1};
  st = h->mt.clock.start(match_stages(), h->profiling != 0) == hipSuccess ? SBM_OK : SBM_ERR_HIP;
  if (st == SBM_OK && guess) st = project_run(h, 1, job, d_xyz, d_n, cap, T, K, width, height, d_proj);
  if (st == SBM_OK)
    st = match_run(h, 1, job, d_desc, d_n, cap, p, d_kp, d_proj, d_pairs, d_n + 2, nullptr, guess);
  if (st != SBM_OK) {
    hipStreamSynchronize(h->stream);   // enqueued copies read the caller's arrays and `cnt`
    return st;
  }
  int k = 0;
  HIPCHK(h, hipMemcpyAsync(&k, d_n + 2, sizeof(k), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (k > 0) HIPCHK(h, hipMemcpy(pairs, d_pairs, (size_t)k * 8, hipMemcpyDeviceToHost));
  *npairs = k;
  return SBM_OK;
}

int sbm_match(sbm_handle* h, const uint8_t* desc_from, size_t stride_from, int nf, const uint8_t* desc_to, size_t stride_to, int nt,
              const sbm_match_params* p, int* pairs, int* npairs) {
  return match_host(h, false, nullptr, nullptr, desc_from, stride_from, nf, desc_to, stride_to, nt, nullptr, nullptr, 0, 0, p, pairs,
                    npairs);
}

int sbm_match_guess(sbm_handle* h, const float* xyz_from, const float* kpts_to, const uint8_t* desc_from, size_t stride_from, int nf,
                    const uint8_t* desc_to, size_t stride_to, int nt, const float* T, const double* K, int width, int height,
                    const sbm_match_params* p, int* pairs, int* npairs) {
  return match_host(h, true, xyz_from, kpts_to, desc_from, stride_from, nf, desc_to, stride_to, nt, T, K, width, height, p, pairs, npairs);
}

}  // extern "C"
